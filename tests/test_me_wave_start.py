"""Full-pel ME wave kernel, the start of a wave (csrc/sad.hip: stage_window_wave, the head of me_fullpel_wave_kernel, the ring-row read of me_search_strips).

The window is staged by straight-line code: every 16-byte chunk load of a lane is issued before the first wait, and a lane whose row lies below the window takes the
window's last row instead (its store repeats the store of the lane that owns the row).  What can go wrong: the number of passes against the number of rows (a row
never loaded, or a row loaded from below the window), the lane -> (row, chunk) map with five chunks per row (lanes 60-63 have no chunk), the partial chunk at every
width % 16 and every byte alignment, and a clamp that is off by one row or one lane.  The search reads one new ring row per step; a read of the row below the last
one a column needs (a row fetched a step ahead without its guard) would be a read below the window.  So: every width and height at which the staging takes another path, all 16 alignments of the
window, a stride that is no multiple of 16, the window's last row as the last row of the plane array, and EVERY byte of the plane outside the windows filled with 0 in
one run and 255 in another -- all 85 SADs and MVs of every item identical in both and equal to the C checker's.
"""
import numpy as np
import pytest
from conftest import rng
from test_me_wave_groups import make_pair, run_batch, want

# W - 1 + 64 = window width: 64 no partial chunk, 65 one byte, 71 pitch 18, 72 pitch 26 / four chunks, 79 the workload, 80 five chunks, 81 five + 1 byte, 87 the widest
WIDTHS = [1, 2, 8, 9, 16, 17, 18, 24]
# 64 + H - 1 rows: 64 whole passes with NF = 4 but not NF = 5, 65 one row in the last pass, 72 the workload, 76, 79 the most rows
HEIGHTS = [1, 2, 9, 13, 16]
AREAS = [(w, h) for w in WIDTHS for h in HEIGHTS]
# the last step of a column on every position of a ring block
RING_AREAS = [(4, 1), (4, 2), (4, 7), (4, 8), (4, 9), (8, 15), (8, 16), (24, 16), (4, 3), (4, 4), (4, 5), (4, 6)]
GAP = 19  # bytes between two windows of a launch (no multiple of 16, and more than a 16-byte chunk)


def aligns_of(case, n):
    return [(3 * case + 7 * i) % 16 for i in range(n)]


def test_cases_cover_every_alignment_and_path():
    assert {a for c in range(len(AREAS)) for a in aligns_of(c, 3)} == set(range(16))
    assert {64 + w - 1 for w in WIDTHS} == {64, 65, 71, 72, 79, 80, 81, 87} and {64 + h - 1 for h in HEIGHTS} == {64, 65, 72, 76, 79}
    assert {(h - 1) % 8 for _, h in RING_AREAS} == set(range(8))  # the ring position of a column's last step


def layout(be, items, aligns, kind, seed):
    """items = [(W, H)] side by side, windows starting at row 0, item i at byte alignment aligns[i]; the reference plane has exactly as many rows as the tallest window.
    -> (src, ref, descs, inside) with inside = the bytes of ref that belong to a window."""
    g = rng(seed)
    rows = max([64 + h - 1 for _, h in items if h > 0] + [64])
    xs, x = [], 0
    for (w, h), al in zip(items, aligns):
        x += (al - x) % 16
        xs.append(x)
        x += 64 + max(w, 1) - 1 + GAP
    stride = x + 16 - x % 16 + 5  # no multiple of 16
    src, _ = make_pair(kind, g, 64 + 8, 64 * len(items) + 40)
    _, ref = make_pair(kind, g, rows, stride)
    descs = np.zeros(len(items), dtype=be.pkg.MeSearchDesc)
    inside = np.zeros(ref.shape, bool)
    for i, ((w, h), x0) in enumerate(zip(items, xs)):
        descs[i] = (i * 64 + i + (i % 3) * src.shape[1], x0, src.shape[1], stride, -(w >> 1), -(h >> 1), w, h)
        if w > 0 and h > 0:
            inside[:64 + h - 1, x0:x0 + 64 + w - 1] = True
    assert stride % 16 != 0 and inside[rows - 1].any()  # a window ends on the last row of the array
    return src, ref, descs, inside


def check_both_fills(be, oracle, items, aligns, kind, seed, sub_sad, n=None):
    src, ref, descs, inside = layout(be, items, aligns, kind, seed)
    n = len(items) if n is None else n
    mw, mh = max(w for w, _ in items), max(h for _, h in items)
    wanted = [want(oracle, src, ref, descs[i], sub_sad) if items[i][0] > 0 and items[i][1] > 0 else None for i in range(n)]
    for fill in (0, 255):
        r = np.where(inside, ref, np.uint8(fill))
        bs, bm = run_batch(be, src, r, descs[:n], mw, mh, sub_sad)
        for i in range(n):
            if wanted[i] is None:
                assert (bs[i] == be.pkg.MAX_SAD_VALUE).all() and (bm[i] == 0).all(), (items, i, fill)
                continue
            assert np.array_equal(bs[i], wanted[i][0]), (items[i], kind, sub_sad, fill, i, np.nonzero(bs[i] != wanted[i][0])[0][:8])
            assert np.array_equal(bm[i], wanted[i][1]), (items[i], kind, sub_sad, fill, i, np.nonzero(bm[i] != wanted[i][1])[0][:8])


@pytest.mark.parametrize("kind", ["random", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("case", range(len(AREAS)), ids=lambda c: "%dx%d" % AREAS[c])
def test_staging_geometry(be, oracle, case, sub_sad, kind):
    check_both_fills(be, oracle, [AREAS[case]] * 3, aligns_of(case, 3), kind, 500 + 4 * case + sub_sad, sub_sad)


@pytest.mark.parametrize("kind", ["random", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("case", range(len(RING_AREAS)), ids=lambda c: "%dx%d" % RING_AREAS[c])
def test_ring_row_read_stays_in_the_window(be, oracle, case, sub_sad, kind):
    check_both_fills(be, oracle, [RING_AREAS[case]] * 3, aligns_of(case + 5, 3), kind, 900 + 4 * case + sub_sad, sub_sad)


@pytest.mark.parametrize("kind", ["random", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
def test_nine_mixed_items_with_an_empty_area(be, oracle, sub_sad, kind):
    """Two workgroups plus one wave; every item has its own W and H, one has none."""
    items = [(16, 9), (7, 3), (1, 1), (0, 0), (13, 8), (16, 2), (4, 9), (9, 5), (15, 7)]
    check_both_fills(be, oracle, items, aligns_of(2, 9), kind, 1300 + sub_sad, sub_sad)


@pytest.mark.parametrize("sub_sad", [0, 1])
def test_last_workgroup_has_waves_past_n(be, oracle, sub_sad):
    items = [(16, 9), (16, 9), (5, 9), (16, 4), (16, 9), (16, 9), (16, 9), (16, 9)]
    src, ref, descs, inside = layout(be, items, aligns_of(4, 8), "random", 1400 + sub_sad)
    sentinel = np.uint32(0xA5A5A5A5)
    ds, dr, dd = be.dev(src), be.dev(np.where(inside, ref, np.uint8(255))), be.dev(descs)
    bs, bm = be.dev(np.full(8 * 85, sentinel, np.uint32)), be.dev(np.full(8 * 85, sentinel, np.uint32))
    be.lib.svt_hip_me_fullpel_search_batch(be.ptr(ds), be.ptr(dr), be.ptr(dd), 5, 16, 9, sub_sad, be.ptr(bs), be.ptr(bm), None, be.stream)
    hs, hm = be.host(bs).reshape(8, 85), be.host(bm).reshape(8, 85)
    for i in range(5):
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(hs[i], ws) and np.array_equal(hm[i], wm), (sub_sad, i)
    assert (hs[5:] == sentinel).all() and (hm[5:] == sentinel).all()  # the waves past n wrote nothing
