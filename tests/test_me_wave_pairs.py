"""Full-pel ME search, the wave kernel pairing the two step groups of a ring block (csrc/sad.hip: me_search_strips<..., QLDS>, sum_rows_pair).

A ring block of eight y steps is the step groups A (steps 0-3) and B (steps 4-7).  Where B has two steps or more, the 32x32 keys of both go through one minimum and the
two 32x32 registers go through the row / half swaps together: even rows end with the 64x64 sum of A, odd rows with that of B, and which one a lane holds is a position bit
(four rows further) ORed in behind the loops.  An A without such a B keeps the single form and a tracker of its own.  The 16x16 sums are keyed two steps at a time, and what
a group leaves over is keyed on one of four scalar-branch sides (four, three, two steps, one step).  What can go wrong: the row assignment of the swaps (a wrong lane-constant
bit moves a 64x64 winner by four rows, or lets B win a tie), A's 32x32 register being overwritten while it waits for B, a 16x16 sum keyed at the wrong step or never, invalid
positions of the last strip entering the shared minimum, and waves of one workgroup on different sides of the branches.  The areas are those the pairing of x groups was
specified with (that form did not fit the register budget: DESIGN.md section 4.1, fourth cut); their heights put every side to work: 1, 2, 3, 4 (A alone), 5 (A + pooled
step), 9 (pair + pooled step), 13 (pair, A alone, pooled step), 16 (two pairs).  Both sub_sad forms (the pairing is compiled into the one without; the other keeps the
form before it), planes whose steps differ (random) and tie across x groups and step groups (periodic) -- these two are what catch a wrong or missing position bit of the
paired 64x64 key, through the exact MV comparison -- and planes that tie everywhere (constant, extreme: the first raster position must win for all 85 blocks, which
shows a key that loses a tie it should win, an invalid position that wins, and a carry in the packed sums, not that bit).  All 85 SADs and MVs of every item
against the C checker, exactly.
"""
import numpy as np
import pytest
from conftest import rng
from test_me_wave_groups import make_pair, run_batch, want

# 4x3: one x group, A of three steps alone.  5x1: a second x group with one valid position, one step.  8x1, 8x2: one step (pool) or two (A alone, two sums left over).
# 8x5: A whole + a pooled step.  9x4: three x groups, the last with invalid positions.  12x9: a pair of groups + a pool of three.  16x9: the workload.
# 20x5: five x groups, five chunks per row.  21x13: pair, then A alone and a pooled step, invalid positions.  24x16: two pairs, the largest window.
# 28x9: the workgroup kernel, which keeps the unpaired form.
AREAS = [(4, 3), (5, 1), (8, 1), (8, 2), (8, 5), (9, 4), (12, 9), (16, 9), (20, 5), (21, 13), (24, 16), (28, 9)]
KINDS = ["random", "constant", "periodic", "extreme"]
N_ITEMS = 3


def planes(kind, g, rows, stride):
    if kind == "extreme":  # |a - b| = 255 everywhere: an 8x8 SAD is 16 320, the quad's packed u16 sum 65 280 = the largest value that does not carry
        return np.zeros((rows, stride), np.uint8), np.full((rows, stride), 255, np.uint8)
    return make_pair(kind, g, rows, stride)


def first_mv(aw, ah):
    return (np.uint32(np.uint16(np.int16(-(ah >> 1)))) << np.uint32(16)) | np.uint32(np.uint16(np.int16(-(aw >> 1))))


def check_items(oracle, src, ref, descs, bs, bm, sub_sad, tag):
    for i, d in enumerate(descs):
        ws, wm = want(oracle, src, ref, d, sub_sad)
        assert np.array_equal(bs[i], ws), (tag, i, np.nonzero(bs[i] != ws)[0][:8])
        assert np.array_equal(bm[i], wm), (tag, i, np.nonzero(bm[i] != wm)[0][:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sub_sad", [0, 1])
@pytest.mark.parametrize("area", AREAS, ids=lambda a: "%dx%d" % a)
def test_me_pairs_every_item(be, oracle, area, sub_sad, kind):
    aw, ah = area
    g = rng(3000 * aw + 30 * ah + sub_sad)
    stride, rows = 64 * N_ITEMS + aw + 40, 64 + ah + 8
    src, ref = planes(kind, g, rows, stride)
    descs = np.zeros(N_ITEMS, dtype=be.pkg.MeSearchDesc)
    for i in range(N_ITEMS):  # odd offsets: every byte alignment of the window rows
        descs[i] = (i * 64 + i, (i % 3) * stride + i * 64 + ((5 * i + 1) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, aw, ah, sub_sad)
    check_items(oracle, src, ref, descs, bs, bm, sub_sad, (kind, area, sub_sad))
    if kind in ("constant", "extreme"):  # all positions tie: the first one in raster order, (0, 0), wins for all 85 blocks
        assert (bm == first_mv(aw, ah)).all(), (area, sub_sad, np.unique(bm))
        size = np.repeat([64, 32, 16, 8], [1, 4, 16, 64]).astype(np.uint32)
        diff = 255 if kind == "extreme" else 41  # 8x8: 16 320, 16x16: 65 280, 32x32: 261 120, 64x64: 1 044 480 (sub_sad: half the rows, doubled -- the same)
        assert (bs == size * size * np.uint32(diff)).all(), (area, sub_sad, np.unique(bs))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sub_sad", [0, 1])
def test_me_pairs_nine_mixed_items_in_one_launch(be, oracle, sub_sad, kind):
    """A 24x16 launch of nine items (two full workgroups and one wave): the waves of a workgroup take different sides of the pairing branches, one area is empty --
    a wave that follows its neighbour's side, or sums another wave left behind, show as a wrong winner."""
    g = rng(1777 + sub_sad)
    areas = [(24, 16), (4, 3), (9, 4), (0, 0), (5, 1), (12, 9), (16, 9), (21, 13), (8, 5)]
    stride, rows = 64 * len(areas) + 70, 64 + 16 + 10
    src, ref = planes(kind, g, rows, stride)
    descs = np.zeros(len(areas), dtype=be.pkg.MeSearchDesc)
    for i, (aw, ah) in enumerate(areas):
        descs[i] = (i * 64 + (i % 5), (i % 4) * stride + i * 64 + ((3 * i + 1) % 7), stride, stride, -(aw >> 1), -(ah >> 1), aw, ah)
    bs, bm = run_batch(be, src, ref, descs, 24, 16, sub_sad)
    live = [i for i, (aw, _) in enumerate(areas) if aw]
    assert (bs[3] == be.pkg.MAX_SAD_VALUE).all() and (bm[3] == 0).all()
    check_items(oracle, src, ref, descs[live], bs[live], bm[live], sub_sad, (kind, sub_sad))
    if kind in ("constant", "extreme"):
        for i in live:
            assert (bm[i] == first_mv(*areas[i])).all(), (sub_sad, i, np.unique(bm[i]))
