"""Full-pel ME search, the tail of the wave kernel (csrc/sad.hip: me_search_strips, me_fullpel_wave_kernel).

A last group of ONE y step (H % 4 == 1) takes a path of its own through the 32x32 / 64x64 levels: its 32x32 sum is all-reduced over the four quads of a row and
kept by one quad, the x group's number within a pool of four x groups, and the two levels are evaluated once per pool (quad c then stands for x group c of the
pool instead of step c of a group).  The 21 results of the large blocks leave through one store pass: lanes 0-20 fetch the 64x64, 32x32 and 16x16 winners from
lanes that hold them.
What can go wrong: a remainder step that is dropped or counted under a wrong row or x group, a quad without an x group (pools of fewer than four) or an invalid
position of the last strip that contributes, the tie-break between a remainder step and an earlier full group, a winner fetched from the wrong lane, and waves of one workgroup that take different paths.  So: H in {1, 5, 9, 13}
with one to six x groups and with invalid positions in the last strip, planes whose winners lie in the remainder step of the last x group, a launch of nine
items of mixed H % 4 -- all 85 outputs of every item against the C checker, both sub_sad forms, both backends.
"""
import numpy as np
import pytest
from conftest import rng
from test_me_wave_groups import make_pair, run_batch, want

TAIL_HEIGHTS = [1, 5, 9, 13]
# 1-6 x groups; 13 and 22: one resp. two valid positions in the last strip; 28 and 61: the workgroup kernel (a wave walks every fourth x group: one pool per wave)
TAIL_WIDTHS = [4, 8, 12, 16, 20, 24, 13, 22, 28, 61]
N_ITEMS = 3


def check_all(be, oracle, src, ref, descs, bs, bm, sub_sad, tag):
    for i in range(len(descs)):
        if descs[i]["width"] == 0:
            assert (bs[i] == be.pkg.MAX_SAD_VALUE).all() and (bm[i] == 0).all(), (tag, i)
            continue
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(bs[i], ws), (tag, sub_sad, i, np.nonzero(bs[i] != ws)[0][:8])
        assert np.array_equal(bm[i], wm), (tag, sub_sad, i, np.nonzero(bm[i] != wm)[0][:8])


@pytest.mark.parametrize("kind", ["random", "constant", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("ah", TAIL_HEIGHTS)
@pytest.mark.parametrize("aw", TAIL_WIDTHS)
def test_me_tail_single_step_remainder(be, oracle, aw, ah, sub_sad, kind):
    g = rng(5000 + 100 * aw + 2 * ah + sub_sad)
    stride, rows = 64 * N_ITEMS + aw + 40, 64 + ah + 8
    src, ref = make_pair(kind, g, rows, stride)
    descs = np.zeros(N_ITEMS, dtype=be.pkg.MeSearchDesc)
    for i in range(N_ITEMS):  # odd offsets: every byte alignment of the window rows
        descs[i] = (i * 64 + i, (i % 3) * stride + i * 64 + ((3 * i + 2) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, aw, ah, sub_sad)
    check_all(be, oracle, src, ref, descs, bs, bm, sub_sad, (kind, aw, ah))
    if kind == "constant":  # all positions tie: (0, 0) wins for all 85 blocks
        first = ((np.uint32(np.uint16(np.int16(-(ah >> 1)))) << np.uint32(16)) | np.uint32(np.uint16(np.int16(-(aw >> 1)))))
        assert (bm == first).all(), (aw, ah, sub_sad, np.unique(bm))


def sheared_plane(g, rows, cols, dx, dy):
    """P[i][j] = h(j * dy - i * dx): invariant under the shift (dx, dy) and, gcd(dx, dy) = 1, under no shorter one inside a search area."""
    h = g.integers(0, 256, rows * dx + cols * dy + 1, dtype=np.uint8)
    i, j = np.mgrid[0:rows, 0:cols]
    return h[j * dy - i * dx + rows * dx].copy()


@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("both", [True, False], ids=["tie_with_first_group", "remainder_alone"])
@pytest.mark.parametrize("area", [(16, 9), (24, 13), (8, 5), (13, 9), (22, 5)], ids=lambda a: "%dx%d" % a)
def test_me_tail_winner_in_remainder_of_last_x_group(be, oracle, area, both, sub_sad):
    """SAD 0 at B = (W - 1, H - 1), the remainder step of the last x group, for every block size.  With `both`, also at a position A in the first full group of
    the first x group (x = 1, 2 or 3, y = 2): the tie goes to A, the earlier position in raster order, for all 85 blocks."""
    aw, ah = area
    ya, xb, yb = 2, aw - 1, ah - 1
    xa = next(x for x in (1, 2, 3) if np.gcd(xb - x, yb - ya) == 1)  # no third position on the line from A to B
    g = rng(900 + aw + ah)
    rows, cols = 64 + ah + 6, 64 + aw + 10
    if both:
        assert np.gcd(xb - xa, yb - ya) == 1
        ref = sheared_plane(g, rows, cols, xb - xa, yb - ya)
        src = ref[ya:ya + 64, xa:xa + 64].copy()
        assert np.array_equal(src, ref[yb:yb + 64, xb:xb + 64])
    else:
        ref = g.integers(0, 256, (rows, cols), dtype=np.uint8)
        src = ref[yb:yb + 64, xb:xb + 64].copy()
    descs = np.zeros(1, dtype=be.pkg.MeSearchDesc)
    descs[0] = (0, 0, 64, cols, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, aw, ah, sub_sad)
    check_all(be, oracle, src, ref, descs, bs, bm, sub_sad, (area, both))
    wx, wy = (xa, ya) if both else (xb, yb)
    mv = (np.uint32(np.uint16(np.int16(wy - (ah >> 1)))) << np.uint32(16)) | np.uint32(np.uint16(np.int16(wx - (aw >> 1))))
    assert (bs == 0).all() and (bm == mv).all(), (area, both, sub_sad, np.unique(bm))


@pytest.mark.parametrize("kind", ["random", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
def test_me_tail_nine_items_mixed_remainders(be, oracle, sub_sad, kind):
    """Nine items = two full workgroups of four waves and one wave alone; neighbours in a workgroup differ in H % 4 (and in W), one item is empty."""
    areas = [(16, 9), (16, 8), (16, 5), (13, 7), (24, 13), (20, 1), (0, 0), (22, 10), (16, 9)]
    g = rng(4242 + sub_sad)
    stride, rows = 64 * len(areas) + 64, 64 + 13 + 8
    src, ref = make_pair(kind, g, rows, stride)
    descs = np.zeros(len(areas), dtype=be.pkg.MeSearchDesc)
    for i, (w, h) in enumerate(areas):
        descs[i] = (i * 64 + (i % 5), (i % 4) * stride + i * 64 + ((5 * i + 3) % 11), stride, stride, -(w >> 1), -(h >> 1), w, h)
    bs, bm = run_batch(be, src, ref, descs, 24, 13, sub_sad)
    check_all(be, oracle, src, ref, descs, bs, bm, sub_sad, kind)
