"""The temporal-filter stage -- sub-pel refinement, final motion compensation, the frame filter, the picture stage in both forms, the noise estimate -- at picture
and buffer geometry edges.  Every other temporal-filter test uses pictures that are a whole number of 64x64 blocks wide, blocks that lie inside the picture, and
buffers of exactly (H + 2 PAD) x (W + 2 PAD) samples from element 0, which hides a kernel that clamps a vector against the wrong edge, walks one buffer with another
buffer's stride, reads past the padded rectangle or writes outside the 64x64 blocks it owns.  Here the pictures are 200x136, 136x200, 72x40 and 40x24 (blocks of the
last column and row overhang the picture or lie outside it, so the right / bottom side of clamp_mv_to_umv_border_sb goes negative); every plane lies in a flat buffer
with an odd lead, an odd stride larger than the padded width and a tail (tests/tf_geometry_common.py); inputs carry random samples -- or 0 in one run and the sample
maximum in another -- wherever they are not a padded picture; outputs and result tables are sentinel-filled and compared WHOLE, with a report that says where the first
wrong sample lies.  Everything is bit-exact against oracle/, and the two oracle pieces whose clamp the geometry exercises are first pinned against the reference
itself at 200x136 and 40x24, overhanging blocks included.  Emulator here, MI355X with -m gpu.

Regression note: the pass found svt_hip_tf_subpel_search_host returning arena garbage in the result slots of descriptors with bsize 0 (the device kernel skips them,
the host form downloaded the whole table over the caller's); the host form now carries the caller's table to the device first.  test_tf_subpel_host_geometry."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REF_LIB, p, rng
from loopfilter_geometry_common import PIX_FILL, Plane, check_table, dev_ptr
from test_tf import make_blocks, make_params
from test_tf_picture import CASES as STAGE_CASES, make_case
from test_tf_subpel import CASES, REF_ME_LIB, make_pictures, make_yuv, oracle_subpel, params
from tf_geometry_common import (PAD, SIZE_IDS, SIZES, SMALL, Stack, StagePictures, chroma_plane, dtype_of, far_me_tables, fill, luma_plane, sb_count, umv_clamp,
                                walk_blocks, yuv_planes)

RES_FILL = 0x5A  # every byte of a result slot nobody wrote


def emulator_runs_small_sizes(be, size):
    if not be.is_gpu and size not in SMALL:
        pytest.skip("emulator: 200x136 and 136x200 run on the GPU (72x40 and 40x24 take the same paths: an overhanging column, a picture smaller than a block)")


def far_vector(g, i, W, H):
    """a starting vector far outside the picture, 1/8 pel: one to two picture sizes away, the four directions in turn (what a full-pel search at the border of a
    large search area can return, nowhere near the int16 limit)"""
    return (1, -1)[i & 1] * int(g.integers(W, 2 * W)) * 8, (1, -1)[(i >> 1) & 1] * int(g.integers(H, 2 * H)) * 8


# ======================================================================================================================================================================
# 1. the checker against the reference where the clamp's right / bottom side is negative (CPU only)
# ======================================================================================================================================================================
def reference_libs(ref):
    if not os.path.exists(REF_ME_LIB):
        pytest.skip("oracle/_ref/libsvtref_me.so not available")
    ref.svt_aom_setup_common_rtcd_internal(C.c_uint64(0))
    ref.svt_aom_setup_rtcd_internal(C.c_uint64(0))
    C.CDLL(REF_LIB, mode=C.RTLD_GLOBAL)
    return C.CDLL(REF_ME_LIB)


def padded_source(src):
    return np.pad(src, PAD, mode="edge")  # the encoder pads its pictures by replicating their edges: an overhanging block's source samples


@pytest.mark.parametrize("W,H", [(200, 136), (40, 24)], ids=["200x136", "40x24"])
@pytest.mark.parametrize("bd", [8, 10])
def test_tf_subpel_oracle_vs_reference_geometry(oracle, ref, bd, W, H):
    """oracle_tf_luma_pred / oracle_tf_subpel_search == svt_aom_simple_luma_unipred / tf_subpel_search for EVERY block of the picture's 64x64 walk -- at 200x136
    pu_x = 192 with 64 / 32 / 16 / 8 wide blocks and pu_y = 128, at 40x24 every 64x64 and 32x32 block overhangs -- from vectors near and far (+-3000 / +-2000)"""
    refme = reference_libs(ref)
    g = rng(2600 + bd + W)
    dt = dtype_of(bd)
    src, refp = make_pictures(g, W, H, PAD, bd)
    pr, ps = luma_plane(W, H, 9, 13, dt), luma_plane(W, H, 23, 7, dt)
    f_ref, f_src = fill(pr, g, refp, "noise", bd), fill(ps, g, padded_source(src), "noise", bd)
    blocks = walk_blocks(W, H)
    assert any(x + ix * b + b > W for (x, y, b, ix, iy) in blocks) and any(y + iy * b >= H for (x, y, b, ix, iy) in blocks)
    # the prediction alone: every phase pair through the first sixteen, then near / far
    P = params((1, 1, 1), 0, bd, 0, W, H, PAD, pr.stride)
    for it, (sbx, sby, b, ix, iy) in enumerate(blocks):
        pu_x, pu_y = sbx + ix * b, sby + iy * b
        mvx, mvy = (int(g.integers(-40, 41)), int(g.integers(-40, 41))) if it % 3 else (int(g.integers(-3000, 3001)), int(g.integers(-2000, 2001)))
        if it < 16:
            mvx, mvy = it % 8 + 8 * (it // 8), 8 - it % 8
        bil, ss = (it // 3) % 2, (it // 7) % 2
        a = np.zeros(64 * 64, np.uint16)
        oracle.oracle_tf_luma_pred(C.byref(P), pr.host_ptr(f_ref), pu_x, pu_y, b, mvx, mvy, bil, ss, p(a))
        w = np.zeros((64, 64), dt)
        refme.ref_tf_luma_pred(C.byref(P), pr.host_ptr(f_ref), W, H, pu_x, pu_y, b, mvx, mvy, bil, ss, p(w))
        assert np.array_equal(a[:b * (b >> ss)].reshape(b >> ss, b), w[0:b:(1 << ss), :b].astype(np.uint16)), (it, pu_x, pu_y, b, mvx, mvy, bil, ss)
    # the search: the six settings in turn over the blocks (85 blocks per 64x64: every block size meets every setting)
    n_moved = 0
    for it, (sbx, sby, b, ix, iy) in enumerate(blocks):
        mode, ss, th = CASES[it % len(CASES)]
        P = params(mode, ss, bd, th, W, H, PAD, pr.stride)
        start = ((3 + int(g.integers(-1, 2))) * 8, (2 + int(g.integers(-1, 2))) * 8) if it % 3 else (int(g.integers(-3000, 3001)), int(g.integers(-2000, 2001)))
        bil = (it // 2) % 2
        mx1, my1, d1 = C.c_int16(start[0]), C.c_int16(start[1]), C.c_uint64(0x7fffffff)
        mx2, my2, d2 = C.c_int16(start[0]), C.c_int16(start[1]), C.c_uint64(0x7fffffff)
        oracle.oracle_tf_subpel_search(C.byref(P), ps.host_ptr(f_src, PAD + sby + iy * b, PAD + sbx + ix * b), ps.stride, pr.host_ptr(f_ref), sbx + ix * b, sby + iy * b, b,
                                       bil, C.byref(mx1), C.byref(my1), C.byref(d1))
        refme.ref_tf_subpel_search(C.byref(P), ps.host_ptr(f_src, PAD + sby, PAD + sbx), ps.stride, pr.host_ptr(f_ref), W, H, sbx, sby, b, ix, iy, bil, C.byref(mx2),
                                   C.byref(my2), C.byref(d2))
        assert (mx1.value, my1.value, d1.value) == (mx2.value, my2.value, d2.value), (mode, ss, th, it, sbx, sby, b, ix, iy, start)
        n_moved += (mx1.value, my1.value) != start
    assert n_moved > len(blocks) // 4  # the refinement really moves the vectors


@pytest.mark.parametrize("W,H", [(200, 136), (40, 24)], ids=["200x136", "40x24"])
@pytest.mark.parametrize("bd", [8, 10])
def test_tf_inter_pred_oracle_vs_reference_geometry(oracle, ref, bd, W, H):
    """oracle_tf_inter_pred == svt_aom_inter_prediction as the temporal filter calls it, for every block of the 64x64 walk (overhanging ones included), luma and both
    chroma planes each on a stride of its own, vectors near and far"""
    refme = reference_libs(ref)
    g = rng(2900 + bd + W)
    dt = dtype_of(bd)
    planes = yuv_planes(W, H, 9, 14, (13, 5, 3), dt)
    planes[2] = chroma_plane(W, H, 21, 9, dt)  # (the reference takes a stride per plane)
    flats = [fill(q, g, s, "noise", bd) for q, s in zip(planes, make_yuv(g, W, H, PAD, bd))]
    P = params((1, 1, 1), 0, bd, 0, W, H, PAD, planes[0].stride)
    pl = (C.c_void_p * 3)(*[q.host_ptr(f).value for q, f in zip(planes, flats)])
    st = (C.c_uint32 * 3)(*[q.stride for q in planes])
    for it, (sbx, sby, b, ix, iy) in enumerate(walk_blocks(W, H)):
        mvx, mvy = (int(g.integers(-60, 61)), int(g.integers(-60, 61))) if it % 3 else (int(g.integers(-3000, 3001)), int(g.integers(-2000, 2001)))
        if it < 16:
            mvx, mvy = it % 8, 8 - it % 8 - (it // 8) * 8
        chroma = it % 4 != 3
        outs = [np.zeros((b, b), np.uint16), np.zeros((b // 2, b // 2), np.uint16), np.zeros((b // 2, b // 2), np.uint16)]
        op = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
        pit = (C.c_int * 3)(b, b // 2, b // 2)
        oracle.oracle_tf_inter_pred(C.byref(P), pl, st, sbx + ix * b, sby + iy * b, b, mvx, mvy, int(chroma), op, pit)
        pred = [np.zeros((64, 64), dt), np.zeros((32, 32), dt), np.zeros((32, 32), dt)]
        pp = (C.c_void_p * 3)(*[x.ctypes.data for x in pred])
        refme.ref_tf_inter_pred(C.byref(P), pl, st, W, H, sbx, sby, b, ix, iy, mvx, mvy, int(chroma), pp)
        assert np.array_equal(pred[0][iy * b:(iy + 1) * b, ix * b:(ix + 1) * b], outs[0]), (it, sbx, sby, b, ix, iy, mvx, mvy)
        if chroma:
            cb, cy, cx = b // 2, (((iy * b) >> 3) << 3) // 2, (((ix * b) >> 3) << 3) // 2
            for k in (1, 2):
                assert np.array_equal(pred[k][cy:cy + cb, cx:cx + cb], outs[k]), (it, k, sbx, sby, b, ix, iy, mvx, mvy)


# ======================================================================================================================================================================
# 2. sub-pel refinement
# ======================================================================================================================================================================
_subpel_pictures = {}


def subpel_pictures(W, H, bd):
    """(padded source, reference 0, reference 1), made once per size and bit depth"""
    if (W, H, bd) not in _subpel_pictures:
        g = rng(3100 + W + bd)
        src, ref0 = make_pictures(g, W, H, PAD, bd)
        _subpel_pictures[W, H, bd] = (padded_source(src), ref0, make_pictures(g, W, H, PAD, bd, shift=(-5, 1))[1])
    return _subpel_pictures[W, H, bd]


class SubpelCase:
    """every block of the picture's 64x64 walk at all four sizes, overhanging ones included, two references in one Stack (a lead, row gaps and a tail around each),
    the source on another stride and lead; a third of the blocks start far outside the picture; a few descriptors are unused slots (bsize 0)"""

    def __init__(self, pkg, W, H, bd, seed):
        g = rng(seed)
        dt = dtype_of(bd)
        self.W, self.H, self.bd, self.g = W, H, bd, g
        self.src_pic, ref0, ref1 = subpel_pictures(W, H, bd)
        self.ref_pics = [ref0, ref1]
        self.ps = luma_plane(W, H, 27, 9, dt)
        self.refs = Stack([luma_plane(W, H, 5, 3, dt), luma_plane(W, H, 5, 11, dt, tail=61)])  # (one stride: the batch takes one ref_stride for all its pictures)
        assert self.ps.stride != self.refs.planes[0].stride
        self.f_src = fill(self.ps, g, self.src_pic, "noise", bd)
        blocks = walk_blocks(W, H)
        n = self.n = len(blocks)
        d = self.descs = np.zeros(n, pkg.TfSubpelDesc)
        for i, (sbx, sby, b, ix, iy) in enumerate(blocks):
            x, y = sbx + ix * b, sby + iy * b
            d[i]["src_off"], d[i]["src_stride"] = self.ps.lead + (PAD + y) * self.ps.stride + PAD + x, self.ps.stride
            d[i]["ref_off"], d[i]["pu_x"], d[i]["pu_y"], d[i]["bsize"], d[i]["bilinear"] = self.refs.offset(i % 2), x, y, b, (i // 2) % 2
            near = ((3 + int(g.integers(-1, 2))) * 8, (2 + int(g.integers(-1, 2))) * 8) if i % 2 == 0 else ((-5 + int(g.integers(-1, 2))) * 8, (1 + int(g.integers(-1, 2))) * 8)
            d[i]["mv_x"], d[i]["mv_y"] = near if i % 3 else far_vector(g, i // 3, W, H)
        self.unused = [1, n // 2, n - 1]
        d["bsize"][self.unused] = 0
        self.tail = 8

    def ref_flat(self, how):
        g = rng(77)
        return self.refs.build([fill(q, g, pic, how, self.bd) for q, pic in zip(self.refs.planes, self.ref_pics)])

    def P(self, mode, ss, th):
        return params(mode, ss, self.bd, th, self.W, self.H, PAD, self.refs.planes[0].stride)

    def result_table(self, pkg):
        return np.full((self.n + self.tail) * pkg.TfSubpelResult.itemsize, RES_FILL, np.uint8).view(pkg.TfSubpelResult)

    def want(self, oracle, pkg, P, f_ref):
        w = self.result_table(pkg)
        live = np.flatnonzero(self.descs["bsize"])
        o = oracle_subpel(oracle, P, self.f_src, f_ref, self.descs[live])
        w["dist"][live], w["mv_x"][live], w["mv_y"][live], w["pad"][live] = o["dist"], o["mv_x"], o["mv_y"], 0
        return w


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_tf_subpel_batch_geometry(be, oracle, W, H, bd, case):
    """svt_hip_tf_subpel_search_batch == oracle_tf_subpel_search on the whole result table (unused slots and the tail keep their sentinel), and what lies around the
    padded rectangles of the reference buffers -- leads, row gaps, tails, the gap between the two references -- is never read: 0 there in one run, the sample maximum
    in the other, both equal to each other and to the oracle"""
    if not be.is_gpu and ((W, H) != (40, 24) or case != (0 if bd == 8 else 3)):
        pytest.skip("emulator: 40x24 (every 64x64 and 32x32 block overhangs) with one setting per bit depth, about 5 s each; all 48 combinations run on the GPU")
    pkg = be.pkg
    c = SubpelCase(pkg, W, H, bd, 3200 + 7 * case + bd + W)
    mode, ss, th = CASES[case]
    P = c.P(mode, ss, th)
    want = None
    d_src, d_descs = be.dev(c.f_src), be.dev(c.descs)
    PP = pkg.TfSubpelParams.from_buffer_copy(bytes(P))
    for how in ("zero", "max"):
        f_ref = c.ref_flat(how)
        if want is None:
            want = c.want(oracle, pkg, P, f_ref)
        d_ref, d_out = be.dev(f_ref), be.dev(c.result_table(pkg))
        be.lib.svt_hip_tf_subpel_search_batch(C.byref(PP), be.ptr(d_src), be.ptr(d_ref), be.ptr(d_descs), c.n, be.ptr(d_out), be.stream)
        check_table(be.host(d_out), want, c.n, "subpel %dx%d bd %d %s, %s outside the padded rectangles" % (W, H, bd, CASES[case], how))
    live = c.descs["bsize"] != 0
    assert np.count_nonzero((want["mv_x"][:c.n] != c.descs["mv_x"])[live] | (want["mv_y"][:c.n] != c.descs["mv_y"])[live]) > c.n // 4  # the refinement moves vectors


@pytest.mark.parametrize("bd", [8, 10])
def test_tf_subpel_host_geometry(be, oracle, bd):
    """svt_hip_tf_subpel_search_host at 72x40 (the emulator: 40x24): buffers handed over from their first sample (offsets relative to it), the result table compared
    whole.  Regression: the result slots of bsize-0 descriptors came back overwritten with whatever the device arena held."""
    pkg = be.pkg
    W, H = (72, 40) if be.is_gpu else (40, 24)
    c = SubpelCase(pkg, W, H, bd, 3300 + bd)
    P = c.P(*CASES[3])
    f_ref = c.ref_flat("noise")
    want = c.want(oracle, pkg, P, f_ref)
    got = c.result_table(pkg)
    PP = pkg.TfSubpelParams.from_buffer_copy(bytes(P))
    for _ in range(2 if be.is_gpu else 1):  # (the second call finds the pooled arena holding the first call's results)
        assert be.lib.svt_hip_tf_subpel_search_host(C.byref(PP), p(c.f_src), C.c_size_t(c.f_src.size), p(f_ref), C.c_size_t(f_ref.size), p(c.descs), c.n, p(got)) == 0
        check_table(got, want, c.n, "subpel host form %dx%d bd %d" % (W, H, bd))


# ======================================================================================================================================================================
# 3. final motion compensation
# ======================================================================================================================================================================
def clamp_edge_vectors(W, H, x, y, b, k, near):
    """vectors whose doubled value lands on min_col / max_col / min_row / max_row of the luma clamp (k // 3) or one 1/16-pel step pair either side (k % 3 - 1);
    the other component is `near`"""
    lim = umv_clamp(W // 4, H // 4, x, y, b)[k // 3]
    v = lim // 2 + (k % 3 - 1)
    assert -32768 <= v <= 32767 and lim % 2 == 0
    return (v, near[1]) if k < 6 else (near[0], v)


class McCase:
    """non-overlapping blocks over the 64x64 walk -- each cell wholly tiled by one size, the size turning with the cell, the reference and `rot`, so that two rotations
    put every size at every overhanging position -- from two reference pictures (each plane kind on a stride of its own) into sentinel-guarded prediction planes: luma
    on an odd stride, chroma on an even one, per-reference pred_off, a third plane per kind that no listed block points to"""

    def __init__(self, g, pkg, oracle, W, H, bd, rot, cells=None, sizes=(64, 32, 16, 8), n_pred=3, vectors="mixed"):
        dt = dtype_of(bd)
        self.W, self.H, self.bd = W, H, bd
        nsx, nsy = sb_count(W, H)
        pw, ph = 64 * nsx, 64 * nsy
        kinds = [(luma_plane, 9, (5, 13)), (chroma_plane, 12, (7, 3)), (chroma_plane, 18, (1, 9))]
        self.refs = [Stack([mk(W, H, ex, lead, dt, tail=48 + 5 * r) for r, lead in enumerate(leads)]) for (mk, ex, leads) in kinds]
        pics = [make_yuv(g, W, H, PAD, bd), make_yuv(g, W, H, PAD, bd)]
        self.f_ref = [self.refs[pl].build([fill(self.refs[pl].planes[r], g, pics[r][pl], "noise", bd) for r in range(2)]) for pl in range(3)]
        mkp = lambda w, h, st, lead: Plane(w, h, st, lead, dt, room=pw + 16)  # noqa: E731
        self.preds = [Stack([mkp(pw, ph, (pw + 7) | 1, 3 + 2 * r) for r in range(n_pred)]), Stack([mkp(pw // 2, ph // 2, (pw // 2 + 6) & ~1, 5 + 2 * r) for r in range(n_pred)]),
                      Stack([mkp(pw // 2, ph // 2, (pw // 2 + 10) & ~1, 1 + 4 * r) for r in range(n_pred)])]
        self.P = params((1, 1, 1), 0, bd, 0, W, H, PAD, self.refs[0].planes[0].stride)
        blocks = []
        for cy in range(nsy):
            for cx in range(nsx):
                for r in range(2):
                    b = sizes[(cx + cy + rot + 2 * r) % len(sizes)]
                    blocks += [(64 * cx + ix * b, 64 * cy + iy * b, b, r, r) for iy in range(64 // b) for ix in range(64 // b)]
        if cells is not None:
            blocks = cells(self)
        n = self.n = len(blocks)
        d = self.descs = np.zeros(n, pkg.TfMcDesc)
        for i, (x, y, b, r, slot) in enumerate(blocks):
            near = (int(g.integers(-70, 71)), int(g.integers(-70, 71)))
            if vectors == "near" or i % 16 >= 14:
                mv = near
            elif i % 16 < 12:
                mv = clamp_edge_vectors(W, H, x, y, b, i % 16, near)
            else:
                mv = far_vector(g, i // 16 + (i % 16 - 12) * 2, W, H)
            d[i]["pu_x"], d[i]["pu_y"], d[i]["bsize"], d[i]["mv_x"], d[i]["mv_y"] = x, y, b, mv[0], mv[1]
            for pl in range(3):
                d[i]["ref_off"][pl], d[i]["pred_off"][pl] = self.refs[pl].offset(r), self.preds[pl].offset(slot)
        self.blocks = blocks
        self.oracle = oracle

    def want(self, upto, chroma):
        """the guarded prediction buffers with the first `upto` descriptors' blocks in place"""
        w = [s.guarded() for s in self.preds]
        pl = (C.c_void_p * 3)(*[f.ctypes.data for f in self.f_ref])
        st = (C.c_uint32 * 3)(*[s.planes[0].stride for s in self.refs])
        for i in range(upto):
            x, y, b, r, slot = self.blocks[i]
            d = self.descs[i]
            outs = [np.zeros((b, b), np.uint16), np.zeros((b // 2, b // 2), np.uint16), np.zeros((b // 2, b // 2), np.uint16)]
            op = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
            pit = (C.c_int * 3)(b, b // 2, b // 2)
            refs = (C.c_void_p * 3)(*[pl[k] + self.refs[k].offset(r) * self.f_ref[k].itemsize for k in range(3)])
            self.oracle.oracle_tf_inter_pred(C.byref(self.P), refs, st, x, y, b, int(d["mv_x"]), int(d["mv_y"]), int(chroma), op, pit)
            for k in range(3 if chroma else 1):
                q = self.preds[k].planes[slot]
                ox, oy, cb = (x, y, b) if k == 0 else (((x >> 3) << 3) // 2, ((y >> 3) << 3) // 2, b // 2)
                self.preds[k].part(w[k], slot)[q.idx[oy:oy + cb, ox:ox + cb]] = outs[k]
        return w

    def planes(self, be, d_ref, d_pred):
        PL = be.pkg.TfMcPlanes()
        for pl in range(3):
            PL.ref[pl], PL.pred[pl], PL.ref_stride[pl], PL.pred_stride[pl] = be.ptr(d_ref[pl]), be.ptr(d_pred[pl]), self.refs[pl].planes[0].stride, self.preds[pl].planes[0].stride
        return PL

    def check(self, be, d_pred, want, tag):
        for pl in range(3):
            self.preds[pl].check(be.host(d_pred[pl]), want[pl], "%s, prediction plane kind %d" % (tag, pl))


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_tf_inter_pred_batch_geometry(be, oracle, W, H, bd, rot):
    """svt_hip_tf_inter_pred_batch == oracle_tf_inter_pred, the prediction buffers compared whole: only the listed blocks' samples change, the third plane of each kind
    stays all sentinel, and with chroma = 0 both chroma buffers do; vectors on and one step either side of the four clamp limits, far and near"""
    pkg = be.pkg
    c = McCase(rng(3400 + W + bd + rot), pkg, oracle, W, H, bd, rot)
    PP = pkg.TfSubpelParams.from_buffer_copy(bytes(c.P))
    d_ref, d_descs = [be.dev(f) for f in c.f_ref], be.dev(c.descs)
    for chroma in (1, 0):
        d_pred = [be.dev(s.guarded()) for s in c.preds]
        PL = c.planes(be, d_ref, d_pred)
        be.lib.svt_hip_tf_inter_pred_batch(C.byref(PP), C.byref(PL), be.ptr(d_descs), c.n, chroma, be.stream)
        c.check(be, d_pred, c.want(c.n, chroma), "inter pred batch %dx%d bd %d rot %d chroma %d" % (W, H, bd, rot, chroma))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_tf_inter_pred_list_geometry(be, oracle, W, H, bd):
    """svt_hip_tf_inter_pred_list: the count lives in device memory.  The descriptors past it look valid and point into the third prediction plane of each kind, which
    must stay all sentinel; a count of 0 writes nothing."""
    pkg = be.pkg
    c = McCase(rng(3500 + W + bd), pkg, oracle, W, H, bd, 1)
    PP = pkg.TfSubpelParams.from_buffer_copy(bytes(c.P))
    d_ref = [be.dev(f) for f in c.f_ref]
    for count in (c.n - max(c.n // 3, 1), 0):
        descs = c.descs.copy()
        for pl in range(3):
            descs["pred_off"][count:, pl] = c.preds[pl].offset(2)
        d_descs, d_n = be.dev(descs), be.dev(np.array([count, 0x5A5A5A5A], np.uint32))
        d_pred = [be.dev(s.guarded()) for s in c.preds]
        PL = c.planes(be, d_ref, d_pred)
        be.lib.svt_hip_tf_inter_pred_list(C.byref(PP), C.byref(PL), be.ptr(d_descs), c.n, be.ptr(d_n), 1, be.stream)
        c.check(be, d_pred, c.want(count, 1), "inter pred list %dx%d bd %d, %d of %d descriptors" % (W, H, bd, count, c.n))


def test_tf_inter_pred_list_grid_stride(be, oracle):
    """one list of 8x8 blocks long enough that its 3 n / 4 workgroups exceed the launch's 4 096: the grid-stride walk runs.  5 632 descriptors = 88 cells of the
    200x136 walk (12 per prediction plane, eight guarded planes per kind), every cell tiled by 64 8x8 blocks, in shuffled order."""
    if not be.is_gpu:
        pytest.skip("emulator: 16 896 waves of the lock-step interpreter; the stride loop is the same code the shorter lists run with one trip")
    pkg = be.pkg
    W, H, bd = 200, 136, 8
    nsx, nsy = sb_count(W, H)

    def cells(c):
        out = []
        for k in range(88):
            slot, cell = divmod(k, nsx * nsy)
            out += [(64 * (cell % nsx) + ix * 8, 64 * (cell // nsx) + iy * 8, 8, (cell + slot) % 2, slot) for iy in range(8) for ix in range(8)]
        return [out[i] for i in rng(7).permutation(len(out))]
    c = McCase(rng(3600), pkg, oracle, W, H, bd, 0, cells=cells, n_pred=8)
    assert 3 * c.n // 4 > 4096 and c.n == 88 * 64
    PP = pkg.TfSubpelParams.from_buffer_copy(bytes(c.P))
    d_ref, d_descs, d_n = [be.dev(f) for f in c.f_ref], be.dev(c.descs), be.dev(np.array([c.n], np.uint32))
    d_pred = [be.dev(s.guarded()) for s in c.preds]
    PL = c.planes(be, d_ref, d_pred)
    be.lib.svt_hip_tf_inter_pred_list(C.byref(PP), C.byref(PL), be.ptr(d_descs), c.n, be.ptr(d_n), 1, be.stream)
    c.check(be, d_pred, c.want(c.n, 1), "inter pred list of %d 8x8 blocks" % c.n)


# ======================================================================================================================================================================
# 4. the frame filter
# ======================================================================================================================================================================
#             nbx nby  ss      chroma frames   (the large frame counts at the small block counts)
FRAME_RUNS = [(1, 1, (1, 1), True, 32), (1, 1, (0, 0), True, 25), (3, 1, (1, 0), True, 24), (1, 3, (0, 1), True, 13), (3, 2, (1, 1), True, 12), (3, 2, (1, 1), False, 1),
              (1, 3, (0, 0), True, 0), (3, 1, (1, 1), False, 13), (3, 2, (1, 0), True, 1), (3, 2, (0, 1), True, 0), (1, 3, (1, 1), True, 25), (3, 1, (0, 0), False, 24)]


@pytest.mark.parametrize("run", range(len(FRAME_RUNS)))
@pytest.mark.parametrize("zz", [0, 1])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tf_filter_frame_geometry(be, oracle, bd, zz, run):
    """svt_hip_tf_filter_frame / _chunked == the oracle's per-block chain with central, out and every prediction (three planes each) on an odd lead and a stride of its
    own -- the kernel's four-sample loads and stores start at odd sample addresses -- out of place into a guarded output compared whole, and in place; frame counts at
    the chunk boundaries (12 | 13, 24 | 25, 32) with a junk-filled workspace; all four sub-samplings and luma only (the chroma outputs then stay untouched)"""
    if not be.is_gpu and run % 3 != (8, 10, 12).index(bd):
        pytest.skip("emulator: every run at one bit depth and every bit depth at four runs, with both filters; all 72 combinations run on the GPU")
    pkg = be.pkg
    nbx, nby, ss, chroma, n_refs = FRAME_RUNS[run]
    g = rng(3700 + 31 * run + 2 * bd + zz)
    dt = dtype_of(bd)
    P = make_params(pkg, g, bd, zz, int(chroma), ss)
    W, H = nbx * 32, nby * 32
    cw, chh = W >> ss[0], H >> ss[1]
    room = W + 80
    def planes(ey, ec, leads):
        return [Plane(W, H, (W + ey) | 1, leads[0], dt, room=room), Plane(cw, chh, cw + ec, leads[1], dt, room=room), Plane(cw, chh, cw + ec, leads[2], dt, room=room)]
    pc, po = planes(24, 9, (3, 7, 5)), planes(14, 16, (9, 1, 11))
    pp = [planes(3 + 2 * r, 5 + r, (1 + 2 * (r % 5), 3 + 2 * (r % 3), 7 + 2 * (r % 4))) for r in range(n_refs)]
    shape = lambda q: (q.h, q.w)  # noqa: E731
    cen = [g.integers(0, 1 << bd, shape(q)) for q in pc]
    f_c = [fill(q, g, s, "noise", bd) for q, s in zip(pc, cen)]
    f_p = []
    for r in range(n_refs):
        noise = int(g.choice([2, 8, 30])) << (bd - 8)
        f_p.append([fill(q, g, np.clip(s + g.integers(-noise, noise + 1, s.shape), 0, (1 << bd) - 1), "noise", bd) for q, s in zip(pp[r], cen)])
    blocks = make_blocks(pkg, g, max(n_refs, 1) * nby * nbx, bd)
    # the oracle writes the out-of-place expectation straight into the guarded buffers
    want = [q.guarded() for q in po]
    cs, os_ = (C.c_int * 2)(pc[0].stride, pc[1].stride), (C.c_int * 2)(po[0].stride, po[1].stride)
    oracle.oracle_tf_filter_frame(C.byref(P), (C.c_void_p * 3)(*[q.host_ptr(f).value for q, f in zip(pc, f_c)]), cs,
                                  (C.c_void_p * (3 * max(n_refs, 1)))(*[q.host_ptr(f).value for r in range(n_refs) for q, f in zip(pp[r], f_p[r])]),
                                  (C.c_int * (2 * max(n_refs, 1)))(*[v for r in range(n_refs) for v in (pp[r][0].stride, pp[r][1].stride)]),
                                  C.c_void_p(blocks.ctypes.data), n_refs, nbx, nby, (C.c_void_p * 3)(*[q.host_ptr(f).value for q, f in zip(po, want)]), os_)
    want_in = [f.copy() for f in f_c]  # in place: the same samples over the central picture, its leads, gaps and tails as they were
    for k in range(3 if chroma else 1):
        want_in[k][pc[k].idx] = po[k].samples(want[k])
    d_c, d_o, d_p, d_b = [be.dev(f) for f in f_c], [be.dev(q.guarded()) for q in po], [[be.dev(f) for f in fs] for fs in f_p], be.dev(blocks)
    PL = pkg.TfPlanes
    mk = lambda qs, ds: PL(dev_ptr(be, ds[0], qs[0]), dev_ptr(be, ds[1], qs[1]), dev_ptr(be, ds[2], qs[2]), qs[0].stride, qs[1].stride)  # noqa: E731
    t_cen, t_out = mk(pc, d_c), mk(po, d_o)
    prs = (PL * max(n_refs, 1))(*[mk(pp[r], d_p[r]) for r in range(n_refs)])
    ws_bytes = be.lib.svt_hip_tf_filter_frame_workspace(C.addressof(P), nbx, nby)
    def frame(dst):
        if n_refs > 12 or run % 2:  # (the chunked entry point with few frames is one launch)
            ws = be.dev(g.integers(0, 256, ws_bytes).astype(np.uint8))  # any content
            be.lib.svt_hip_tf_filter_frame_chunked(C.addressof(P), C.addressof(t_cen), C.addressof(prs), n_refs, be.ptr(d_b), nbx, nby, C.addressof(dst), be.ptr(ws), be.stream)
            be.sync()
        else:
            be.lib.svt_hip_tf_filter_frame(C.addressof(P), C.addressof(t_cen), C.addressof(prs), n_refs, be.ptr(d_b), nbx, nby, C.addressof(dst), be.stream)
    tag = "filter frame %dx%d blocks ss %s chroma %d, %d frames, bd %d zz %d" % (nbx, nby, ss, chroma, n_refs, bd, zz)
    frame(t_out)
    for k in range(3):
        po[k].check(be.host(d_o[k]), want[k], tag + ", out of place, plane %d" % k)
        pc[k].check(be.host(d_c[k]), f_c[k], tag + ", out of place: the central picture, plane %d" % k)
    frame(t_cen)
    for k in range(3):
        pc[k].check(be.host(d_c[k]), want_in[k], tag + ", in place, plane %d" % k)


# ======================================================================================================================================================================
# 5. the stage
# ======================================================================================================================================================================
def stage_oracle(oracle, P, S, tabs, f_cen, f_ref, f_cen8, f_ref8):
    """the oracle on the flat buffers, its output into guarded buffers: what it leaves there IS the expectation, after checking that it lies in the rectangle the
    stage owns"""
    n_refs = S.n_refs
    want = [q.guarded() for q in S.out]
    base = lambda f, off: f.ctypes.data + off * f.itemsize  # noqa: E731
    cen = (C.c_void_p * 3)(*[base(f_cen[pl], S.cen[pl].lead) for pl in range(3)])
    refs = (C.c_void_p * (3 * n_refs))(*[base(f_ref[pl], S.refs[pl].offset(r)) for r in range(n_refs) for pl in range(3)])
    o = (C.c_void_p * 3)(*[base(want[pl], S.out[pl].lead) for pl in range(3)])
    arr = (lambda k: (C.c_void_p * n_refs)(*[t[k].ctypes.data for t in tabs])) if tabs else (lambda k: None)  # noqa: E731
    r8 = (C.c_void_p * n_refs)(*[base(f_ref8, S.refs8.offset(r)) for r in range(n_refs)]) if S.sp8 else None
    stats = np.zeros(5, np.uint32)
    oracle.oracle_tf_picture.restype = C.c_int
    assert oracle.oracle_tf_picture(C.byref(P), cen, refs, arr(0), arr(1), arr(2), arr(3), n_refs, o, p(stats), C.c_void_p(base(f_cen8, S.cen8.lead)) if S.sp8 else None,
                                    r8) == 0
    for pl in range(3):
        m = S.rect_mask(S.out[pl], pl, P.pic_w_sb, P.pic_h_sb)
        assert (want[pl][~m] == PIX_FILL[want[pl].itemsize]).all()
    return want, stats


def stage_check(be, oracle, P, pics, tabs, W, H, bd, tag):
    """both forms of the stage on pictures stored in flat buffers; returns the oracle's statistics"""
    pkg = be.pkg
    g = rng(4100 + W + bd)
    S = StagePictures(g, pics, W, H, bd, bool(P.subpel_8bit))
    S.set_params(P)
    n_refs = S.n_refs
    f8c, f8r = (S.cen8_flat, S.ref8_flat) if S.sp8 else (None, None)
    want, wstats = stage_oracle(oracle, P, S, tabs, S.cen_flat, S.ref_flat, f8c, f8r)
    chroma = bool(P.tf.tf_chroma)
    # -- host form, out of place into guarded planes: exactly the rectangle of 64x64 blocks from the picture origin is written
    at = lambda f, off: f.ctypes.data + off * f.itemsize  # noqa: E731
    hcen = pkg.TfHostPicture(at(S.cen_flat[0], S.cen[0].lead), at(S.cen_flat[1], S.cen[1].lead), at(S.cen_flat[2], S.cen[2].lead), S.y_samples, S.uv_samples,
                             at(f8c, S.cen8.lead) if S.sp8 else None)
    hrefs = (pkg.TfHostPicture * n_refs)(*[pkg.TfHostPicture(at(S.ref_flat[0], S.refs[0].offset(r)), at(S.ref_flat[1], S.refs[1].offset(r)),
                                                              at(S.ref_flat[2], S.refs[2].offset(r)), S.y_samples, S.uv_samples,
                                                              at(f8r, S.refs8.offset(r)) if S.sp8 else None) for r in range(n_refs)])
    me = (pkg.TfMeTables * n_refs)(*[pkg.TfMeTables(*[x.ctypes.data for x in t]) for t in tabs]) if tabs else None
    got = [q.guarded() for q in S.out]
    keep_c, keep_r = [f.copy() for f in S.cen_flat], [f.copy() for f in S.ref_flat]
    st = pkg.TfPictureStats()
    assert be.lib.svt_hip_tf_picture_host(C.byref(P), C.byref(hcen), hrefs, me, n_refs, at(got[0], S.out[0].lead), at(got[1], S.out[1].lead), at(got[2], S.out[2].lead),
                                          C.byref(st)) == 0
    gstats = np.array([st.blocks_64x64, st.blocks_32x32, st.blocks_16x16, st.blocks_8x8, st.early_exit_blocks], np.uint32)
    assert np.array_equal(gstats, wstats), (tag, "host form statistics", gstats, wstats)
    for pl in range(3):
        S.out[pl].check(got[pl], want[pl], "%s, host form, output plane %d" % (tag, pl))
        assert np.array_equal(S.cen_flat[pl], keep_c[pl]) and np.array_equal(S.ref_flat[pl], keep_r[pl])  # the inputs are inputs
    # -- resident form, in place: the central buffers come back with that rectangle replaced and everything else as it was
    want_in = [f.copy() for f in S.cen_flat]
    for pl in range(3 if chroma else 1):
        m = S.rect_mask(S.cen[pl], pl, P.pic_w_sb, P.pic_h_sb)
        want_in[pl][m] = want[pl][S.rect_mask(S.out[pl], pl, P.pic_w_sb, P.pic_h_sb)]
    d_c, d_r = [be.dev(f) for f in S.cen_flat], [be.dev(f) for f in S.ref_flat]
    D = pkg.TfDevicePictures()
    for pl in range(3):
        D.central[pl], D.refs[pl] = dev_ptr(be, d_c[pl], S.cen[pl]), be.ptr(d_r[pl]) + S.refs[pl].offset(0) * S.ref_flat[pl].itemsize
    D.ref_pitch, D.ref_uv_pitch = S.refs[0].pitch, S.refs[1].pitch
    assert S.refs[1].pitch == S.refs[2].pitch  # (one chroma pitch in the interface)
    if S.sp8:
        d_c8, d_r8 = be.dev(f8c), be.dev(f8r)
        D.central_y8, D.refs_y8, D.ref_y8_pitch = dev_ptr(be, d_c8, S.cen8), be.ptr(d_r8) + S.refs8.offset(0), S.refs8.pitch
    keep = []
    if tabs:
        d_t = [be.dev(np.concatenate([tabs[r][k].reshape(-1).view(np.uint8) for r in range(n_refs)])) for k in range(4)]
        M = pkg.TfMeTables(*[be.ptr(x) for x in d_t])
        keep.append(d_t)
    else:
        M = pkg.TfMeTables()
    ws = be.dev(g.integers(0, 256, be.lib.svt_hip_tf_picture_workspace(C.byref(P), n_refs)).astype(np.uint8))
    d_st = be.dev(np.full(32 + 16, RES_FILL, np.uint8))
    assert be.lib.svt_hip_tf_picture(C.byref(P), C.byref(D), C.byref(M), n_refs, be.ptr(ws), be.ptr(d_st), be.stream) == 0
    be.sync()
    rst = be.host(d_st)
    assert np.array_equal(rst[:20].view(np.uint32), wstats) and (rst[32:] == RES_FILL).all(), (tag, "resident form statistics", rst[:20].view(np.uint32), wstats)
    for pl in range(3):
        S.cen[pl].check(be.host(d_c[pl]), want_in[pl], "%s, resident form, central plane %d" % (tag, pl))
        assert np.array_equal(be.host(d_r[pl]), S.ref_flat[pl]), (tag, "resident form wrote a reference plane", pl)
    return wstats, not np.array_equal(want_in[0], S.cen_flat[0])


EMU_STAGE = {(40, 24): {(0, "near"), (1, "near"), (1, "far"), (2, "near"), (4, "near")}, (72, 40): {(1, "near"), (2, "near")}}


def emulator_stage_skips(be, size, bd, n_refs, run=None):
    emulator_runs_small_sizes(be, size)
    if not be.is_gpu and (bd == 10 or n_refs > 12) and run != (4, "near"):
        pytest.skip("emulator: the 10-bit case 3, the 14-reference case 5 and 10-bit zero motion run on the GPU, as in test_tf_picture.py")
    if not be.is_gpu and run is not None and run not in EMU_STAGE[size]:
        pytest.skip("emulator: the stage runs there at 40x24 (cases 0, 1, 2, 4; case 1 with the far tables too) and 72x40 (cases 1, 2); every combination on the GPU")


@pytest.mark.parametrize("tables", ["near", "far"])
@pytest.mark.parametrize("case", range(len(STAGE_CASES)))
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_tf_picture_stage_geometry(be, oracle, W, H, case, tables):
    """svt_hip_tf_picture_host and svt_hip_tf_picture == oracle_tf_picture at picture sizes with a partial last column / row and below one block, the pictures in flat
    buffers (odd leads, an odd luma stride, a chroma stride that is not half of it, reference pitches larger than a plane with guarded gaps), every output plane
    compared whole.  `far`: a quarter of the (block, reference) ME entries and HME centres point (+-W, +-H) full pel away, so the stage itself takes the clamp."""
    bd, n_refs, th64, exit_th, th32, with8, two_tap, ss, chroma, zz = STAGE_CASES[case]
    emulator_stage_skips(be, (W, H), bd, n_refs, (case, tables))
    g = rng(500 + case)  # (test_tf_picture.py's generator and seeds: its decision counts at these sizes are known)
    P, pics, tabs = make_case(g, be.pkg, W, H, PAD, bd, n_refs, th64, exit_th, th32, with8, two_tap, ss, chroma, zz, sp8=(case == 4))
    if tables == "far":
        tabs = far_me_tables(g, tabs, W, H)
    s, changed = stage_check(be, oracle, P, pics, tabs, W, H, bd, "stage %dx%d case %d %s tables" % (W, H, case, tables))
    # every decision branch is reached where the inputs are known to reach it (the oracle's statistics: a property of the inputs, not of the code under test)
    if tables == "near":
        assert changed  # the filter changed the picture
        if case == 0 and (W, H) == (200, 136): assert s[0] > 0 and s[1] > 0 and s[2] > 0 and s[3] > 0  # noqa: E701  all four sizes
        if case == 0 and (W, H) in ((200, 136), (40, 24)): assert s[1] > 0 and s[2] > 0 and s[3] > 0  # noqa: E701  8x8 blocks = a split 16x16 carrying its 8x8 errors
        if case == 1 and (W, H) in ((200, 136), (40, 24)): assert s[4] > 0 and s[0] > 0 and s[1] > 0  # noqa: E701  early exits
        if case == 2: assert s[0] == n_refs * P.pic_w_sb * P.pic_h_sb and not s[1:4].any()  # noqa: E701  the 64x64-only path


@pytest.mark.parametrize("bd,zz,ss", [(8, False, 0), (8, True, 1), (10, False, 1)])
@pytest.mark.parametrize("W,H", SIZES, ids=SIZE_IDS)
def test_tf_picture_zero_motion_geometry(be, oracle, W, H, bd, zz, ss):
    """the low-delay form (no ME tables, every block the co-located 64x64 prediction) on the same geometry"""
    emulator_stage_skips(be, (W, H), bd, 3)
    n_refs = 3
    g = rng(560 + bd + ss)
    P, pics, _ = make_case(g, be.pkg, W, H, PAD, bd, n_refs, 20, 900, 3000, False, False, ss, True, zz)
    P.zero_motion = 1
    for r in range(1, n_refs + 1):  # a static scene: the frames are the central picture + noise
        pics[r] = [np.ascontiguousarray(np.clip(x.astype(np.int32) + g.integers(-4, 5, x.shape) * (1 << (bd - 8)), 0, (1 << bd) - 1).astype(x.dtype)) for x in pics[0]]
    s, changed = stage_check(be, oracle, P, pics, None, W, H, bd, "stage %dx%d zero motion bd %d zz %d ss %d" % (W, H, bd, zz, ss))
    assert changed and s[0] == n_refs * P.pic_w_sb * P.pic_h_sb and not s[1:].any()


# ======================================================================================================================================================================
# 6. the noise estimate at its workgroup (64 columns x 64 rows) and wave (16 rows) boundaries
# ======================================================================================================================================================================
@pytest.mark.parametrize("w,h", [(63, 17), (64, 16), (65, 65), (128, 64), (129, 18)])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_noise_estimate_geometry(be, oracle, bd, w, h):
    """the host symbols and svt_hip_estimate_noise_batch == oracle_estimate_noise_fp16 on a plane with an odd lead and an odd stride; the interior is (w - 2) x (h - 2),
    so the sizes put it one short of, on and one past a workgroup's columns and a wave's rows"""
    g = rng(4500 + bd + w)
    dt = dtype_of(bd)
    q = Plane(w, h, (w + 9) | 1, 5, dt)
    amp = 3 << (bd - 8)
    pic = np.clip((np.add.outer(np.arange(h), np.arange(w)) * 2 << (bd - 8)) % (200 << (bd - 8)) + (20 << (bd - 8)) + g.integers(-amp, amp + 1, (h, w)), 0, (1 << bd) - 1)
    f = q.noisy(g, pic, bd)
    want = oracle.oracle_estimate_noise_fp16(q.host_ptr(f), w, h, q.stride, bd)
    assert want > 0  # (not the "too few smooth pixels" answer)
    got = be.lib.svt_estimate_noise_fp16_hip(q.host_ptr(f), w, h, q.stride) if bd == 8 else be.lib.svt_estimate_noise_highbd_fp16_hip(q.host_ptr(f), w, h, q.stride, bd)
    assert got == want, (bd, w, h, got, want)
    d_f, d_out = be.dev(f), be.dev(np.full(4, 0x5A5A5A5A, np.int32))
    d_ws = be.dev(np.full(be.lib.svt_hip_estimate_noise_workspace(w, h), 0x5A, np.uint8))  # any content
    for _ in range(2):
        be.lib.svt_hip_estimate_noise_batch(dev_ptr(be, d_f, q), w, h, q.stride, bd, be.ptr(d_out), be.ptr(d_ws), be.stream)
        o = be.host(d_out)
        assert int(o[0]) == want and (o[1:] == 0x5A5A5A5A).all(), (bd, w, h, o, want)
