"""Full-pel ME search, the grouped 32x32 / 64x64 levels (csrc/sad.hip: me_search_strips, dpp_scatter_sum_quads).

The wave kernel evaluates the 32x32 and 64x64 SADs once per group of four y steps: a reduce-scatter leaves step c of the group in quad c of every 16-lane row,
and a last group of fewer than four steps carries a sentinel for the steps it does not have.  What can go wrong is the rotate direction of the bank-masked
row rotates (a wrong one swaps steps 1 and 3 of a group), the position bits that are ORed in after the loops, the sentinel, and the tie-break ("first minimum in
raster order") now that the candidates of one block sit in different lanes.  So: every class of (W mod 4, H mod 4) with H on both sides of every group
boundary, both sub_sad forms, and planes whose ties fall across steps, groups and quads -- every item of every launch against the C checker.
28x9 is the first area past the wave kernel: the workgroup form shares me_search_strips and merges the lanes' winners through LDS atomics.
"""
import ctypes as C

import numpy as np
import pytest
from conftest import p, rng

# the eight areas the wave kernel is specified for, then one for every remaining class of (W % 4, H % 4); heights 1-16 cover both sides of 4, 8, 12 and 16
WAVE_AREAS = [(16, 9), (8, 3), (8, 4), (8, 1), (12, 5), (13, 7), (23, 16), (24, 13),
              (20, 10), (5, 8), (9, 5), (17, 14), (6, 12), (10, 1), (14, 6), (22, 15), (7, 9), (11, 2), (19, 11)]
WORKGROUP_AREA = (28, 9)
AREAS = WAVE_AREAS + [WORKGROUP_AREA]
N_ITEMS = 3


def test_area_list_covers_every_class():
    assert {(w % 4, h % 4) for w, h in WAVE_AREAS} == {(a, b) for a in range(4) for b in range(4)}
    heights = {h for _, h in WAVE_AREAS}
    assert {3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16} <= heights
    assert all(w <= 24 and h <= 16 for w, h in WAVE_AREAS) and WORKGROUP_AREA[0] > 24


def make_pair(kind, g, rows, stride):
    if kind == "random":
        return g.integers(0, 256, (rows, stride), dtype=np.uint8), g.integers(0, 256, (rows, stride), dtype=np.uint8)
    if kind == "constant":  # every position ties at every block size
        return np.full((rows, stride), 90, np.uint8), np.full((rows, stride), 131, np.uint8)
    assert kind == "periodic"  # period 4 in x and in y: position (x, y) ties with (x + 4 i, y + 4 j) -- across x groups, groups of four steps and quads
    ts, tr = g.integers(0, 256, (4, 4), dtype=np.uint8), g.integers(0, 256, (4, 4), dtype=np.uint8)
    reps = ((rows + 3) // 4, (stride + 3) // 4)
    return np.tile(ts, reps)[:rows, :stride].copy(), np.tile(tr, reps)[:rows, :stride].copy()


def run_batch(be, src, ref, descs, max_w, max_h, sub_sad):
    ds, dr, dd = be.dev(src), be.dev(ref), be.dev(descs)
    n = len(descs)
    bs, bm = be.empty(n * 85, np.uint32), be.empty(n * 85, np.uint32)
    ws_bytes = be.lib.svt_hip_me_fullpel_search_workspace(n, max_w, max_h)
    ws = be.empty(max(ws_bytes, 8), np.uint8)
    be.lib.svt_hip_me_fullpel_search_batch(be.ptr(ds), be.ptr(dr), be.ptr(dd), n, max_w, max_h, sub_sad, be.ptr(bs), be.ptr(bm),
                                           be.ptr(ws) if ws_bytes else None, be.stream)
    return be.host(bs).reshape(n, 85), be.host(bm).reshape(n, 85)


def want(oracle, src, ref, d, sub_sad):
    bs, bm = np.zeros(85, np.uint32), np.zeros(85, np.uint32)
    oracle.oracle_me_fullpel_search(C.c_void_p(src.ctypes.data + int(d["src_off"])), int(d["src_stride"]),
                                    C.c_void_p(ref.ctypes.data + int(d["ref_off"])), int(d["ref_stride"]), int(d["x_origin"]),
                                    int(d["y_origin"]), int(d["width"]), int(d["height"]), sub_sad, p(bs), p(bm))
    return bs, bm


@pytest.mark.parametrize("kind", ["random", "constant", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("area", AREAS, ids=lambda a: "%dx%d" % a)
def test_me_groups_every_item(be, oracle, area, sub_sad, kind):
    aw, ah = area
    g = rng(1000 * aw + 10 * ah + sub_sad)
    stride, rows = 64 * N_ITEMS + aw + 40, 64 + ah + 8
    src, ref = make_pair(kind, g, rows, stride)
    descs = np.zeros(N_ITEMS, dtype=be.pkg.MeSearchDesc)
    for i in range(N_ITEMS):  # odd offsets: every byte alignment of the window rows
        descs[i] = (i * 64 + i, (i % 3) * stride + i * 64 + ((5 * i + 1) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, aw, ah, sub_sad)
    for i in range(N_ITEMS):
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(bs[i], ws), (kind, area, sub_sad, i, np.nonzero(bs[i] != ws)[0][:8])
        assert np.array_equal(bm[i], wm), (kind, area, sub_sad, i, np.nonzero(bm[i] != wm)[0][:8])
    if kind == "constant":  # all positions tie: the first one in raster order, (0, 0), wins for all 85 blocks
        first = ((np.uint32(np.uint16(np.int16(-(ah >> 1)))) << np.uint32(16)) | np.uint32(np.uint16(np.int16(-(aw >> 1)))))
        assert (bm == first).all(), (area, sub_sad, np.unique(bm))
        size = np.repeat([64, 32, 16, 8], [1, 4, 16, 64]).astype(np.uint32)
        assert (bs == size * size * np.uint32(41)).all()


@pytest.mark.parametrize("kind", ["random", "periodic"])
@pytest.mark.parametrize("sub_sad", [0, 1])
def test_me_groups_mixed_areas_in_one_launch(be, oracle, sub_sad, kind):
    """W and H are per item: a 16x9 launch whose items are 16x9, 7x3, 16x5 and empty."""
    g = rng(77 + sub_sad)
    stride, rows = 420, 96
    src, ref = make_pair(kind, g, rows, stride)
    descs = np.zeros(5, dtype=be.pkg.MeSearchDesc)
    descs[0] = (3, 2 * stride + 1, stride, stride, -8, -4, 16, 9)
    descs[1] = (64, 70, stride, stride, -3, -1, 7, 3)
    descs[2] = (130, stride + 133, stride, stride, -8, -2, 16, 5)
    descs[3] = (192, 200, stride, stride, 0, 0, 0, 0)
    descs[4] = (256, 3 * stride + 259, stride, stride, -8, -4, 16, 9)
    bs, bm = run_batch(be, src, ref, descs, 16, 9, sub_sad)
    for i in (0, 1, 2, 4):
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(bs[i], ws) and np.array_equal(bm[i], wm), (kind, sub_sad, i)
    assert (bs[3] == be.pkg.MAX_SAD_VALUE).all() and (bm[3] == 0).all()
