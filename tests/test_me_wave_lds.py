"""Full-pel ME search, the part of a step's tail that runs on the LDS pipe (csrc/sad.hip: me_search_strips<..., QLDS>).

The wave kernel forms the 16x16 sum of a quad through LDS: a slot per quad behind the wave's window is zeroed, the four lanes add their packed u16 SADs with one
no-return 64-bit atomicAdd, lane q reads position q back and consumes it one step late.  What can go wrong: slots that overlap the window or a neighbouring
wave's slots, a sum that is read before it is complete or after the next step zeroed it, a late sum that is never consumed (one step, or the last step of a
group), the packed u16 adds carrying, and invalid positions of a last strip entering a winner.  The same cases pin any other reduction moved to that pipe (the
8x8 / 16x16 winners through lane-private atomicMin slots were measured and not kept: DESIGN.md section 4.1).  So: the smallest areas at which each of these
shows, both sub_sad forms, planes whose consecutive steps differ (random), tie everywhere (constant), tie across groups (periodic) and sit at the top of the
u16 range (extreme) -- all 85 SADs and MVs of every item against the C checker.
"""
import numpy as np
import pytest
from conftest import rng
from test_me_wave_groups import make_pair, run_batch, want

# 1x1, 4x1: one step, nothing to pipeline.  3x2: one strip with an invalid position.  13x7: not FULL, remainder of 3.  17x2: five chunks per row at pitch 26.
# 24x16: the largest window, the slices at their highest offsets.  28x9: the workgroup kernel (shares me_search_strips).
AREAS = [(1, 1), (4, 1), (3, 2), (8, 3), (16, 9), (13, 7), (17, 2), (24, 16), (28, 9)]
KINDS = ["random", "constant", "periodic", "extreme"]
N_ITEMS = 3


def planes(kind, g, rows, stride):
    if kind == "extreme":  # |a - b| = 255 everywhere: an 8x8 SAD is 16 320, the quad's packed u16 sum 65 280 = the largest value that does not carry
        return np.zeros((rows, stride), np.uint8), np.full((rows, stride), 255, np.uint8)
    return make_pair(kind, g, rows, stride)


def first_mv(aw, ah):
    return (np.uint32(np.uint16(np.int16(-(ah >> 1)))) << np.uint32(16)) | np.uint32(np.uint16(np.int16(-(aw >> 1))))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("area", AREAS, ids=lambda a: "%dx%d" % a)
def test_me_lds_every_item(be, oracle, area, sub_sad, kind):
    aw, ah = area
    g = rng(2000 * aw + 20 * ah + sub_sad)
    stride, rows = 64 * N_ITEMS + aw + 40, 64 + ah + 8
    src, ref = planes(kind, g, rows, stride)
    descs = np.zeros(N_ITEMS, dtype=be.pkg.MeSearchDesc)
    for i in range(N_ITEMS):  # odd offsets: every byte alignment of the window rows
        descs[i] = (i * 64 + i, (i % 3) * stride + i * 64 + ((5 * i + 1) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, aw, ah, sub_sad)
    for i in range(N_ITEMS):
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(bs[i], ws), (kind, area, sub_sad, i, np.nonzero(bs[i] != ws)[0][:8])
        assert np.array_equal(bm[i], wm), (kind, area, sub_sad, i, np.nonzero(bm[i] != wm)[0][:8])
    if kind in ("constant", "extreme"):  # all positions tie: the first one in raster order, (0, 0), wins for all 85 blocks
        assert (bm == first_mv(aw, ah)).all(), (area, sub_sad, np.unique(bm))
        size = np.repeat([64, 32, 16, 8], [1, 4, 16, 64]).astype(np.uint32)
        diff = 255 if kind == "extreme" else 41  # 8x8: 16 320, 16x16: 65 280, 32x32: 261 120, 64x64: 1 044 480 (sub_sad: half the rows, doubled -- the same)
        assert (bs == size * size * np.uint32(diff)).all(), (area, sub_sad, np.unique(bs))


@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("sub_sad", [0, 1])
def test_me_lds_nine_mixed_items_in_one_launch(be, oracle, sub_sad, kind):
    """A 24x16 launch of nine items: the waves of a workgroup differ in W and H, one area is empty, one is the largest, and the last workgroup has a single wave --
    slices of neighbouring waves that overlap, or slots another wave left behind, show as a wrong winner."""
    g = rng(991 + sub_sad)
    areas = [(24, 16), (1, 1), (0, 0), (13, 7), (3, 2), (24, 16), (16, 9), (4, 1), (17, 2)]
    stride, rows = 64 * len(areas) + 70, 64 + 16 + 10
    src, ref = planes(kind, g, rows, stride)
    descs = np.zeros(len(areas), dtype=be.pkg.MeSearchDesc)
    for i, (aw, ah) in enumerate(areas):
        descs[i] = (i * 64 + (i % 5), (i % 4) * stride + i * 64 + ((3 * i + 1) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, 24, 16, sub_sad)
    for i, (aw, ah) in enumerate(areas):
        if aw == 0:
            assert (bs[i] == be.pkg.MAX_SAD_VALUE).all() and (bm[i] == 0).all()
            continue
        ws, wm = want(oracle, src, ref, descs[i], sub_sad)
        assert np.array_equal(bs[i], ws), (kind, sub_sad, i, np.nonzero(bs[i] != ws)[0][:8])
        assert np.array_equal(bm[i], wm), (kind, sub_sad, i, np.nonzero(bm[i] != wm)[0][:8])
        if kind == "extreme":
            assert (bm[i] == first_mv(aw, ah)).all(), (sub_sad, i)
