"""Pins tests/maskpred_common.py (the numpy restatement the kernels of csrc/maskpred.hip are checked against) on the REAL reference in oracle/_ref/libsvtref.so: every byte
of the 288 wedge masks through svt_av1_init_wedge_masks + svt_aom_get_contiguous_soft_mask, the OBMC masks through svt_av1_get_obmc_mask, the smooth inter-intra masks
through build_smooth_interintra_mask, the six a64 blend `_c` functions, the two d16 blend functions, the three diff-weighted mask builders,
svt_aom_build_masked_compound_no_round, the four wedge helpers,
svt_aom_combine_interintra[_highbd] (the dispatch pointers set up with flags 0: the `_c` functions) and the search composed from the reference's own helpers as pick_wedge,
pick_wedge_fixed_sign and pick_interinter_seg compose them.  CPU only; runs where the reference's sources and the library exist, skipped elsewhere.
`SVT_MASKPRED_WRITE_GOLDEN=1` rewrites tests/golden/maskpred.npz from the reference's outputs."""
import ctypes as C
import os

import numpy as np
import pytest

import maskpred_common as mc
from conftest import REF_LIB, p

REF = os.environ.get("SVT_REF", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Source", "Lib", "Codec", "blend_a64_mask.c")) or not os.path.exists(REF_LIB),
                                reason="the reference's sources or oracle/_ref/libsvtref.so are not on this machine")

BIT_DEPTHS = (8, 10, 12)
vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int


@pytest.fixture(scope="module")
def rf(ref):
    bl = [vp, u32, vp, u32, vp, u32, vp]
    sigs = {
        "svt_av1_init_wedge_masks": (None, []),
        "svt_aom_get_contiguous_soft_mask": (vp, [i32, i32, i32]),
        "svt_av1_get_obmc_mask": (vp, [i32]),
        "build_smooth_interintra_mask": (None, [vp, i32, i32, i32]),
        "svt_aom_blend_a64_mask_c": (None, bl + [u32, i32, i32, i32, i32]),
        "svt_aom_highbd_blend_a64_mask_c": (None, bl + [u32, i32, i32, i32, i32, i32]),
        "svt_aom_blend_a64_hmask_c": (None, bl + [i32, i32]),
        "svt_aom_blend_a64_vmask_c": (None, bl + [i32, i32]),
        "svt_aom_highbd_blend_a64_hmask_16bit_c": (None, bl + [i32, i32, i32]),
        "svt_aom_highbd_blend_a64_vmask_16bit_c": (None, bl + [i32, i32, i32]),
        "svt_av1_build_compound_diffwtd_mask_c": (None, [vp, i32, vp, i32, vp, i32, i32, i32]),
        "svt_av1_build_compound_diffwtd_mask_highbd_c": (None, [vp, i32, vp, i32, vp, i32, i32, i32, i32]),
        "svt_av1_wedge_sse_from_residuals_c": (C.c_uint64, [vp, vp, vp, i32]),
        "svt_av1_wedge_sign_from_residuals_c": (C.c_int8, [vp, vp, i32, C.c_int64]),
        "svt_av1_wedge_compute_delta_squares_c": (None, [vp, vp, vp, i32]),
        "svt_aom_sum_squares_i16_c": (C.c_uint64, [vp, u32]),
        "svt_aom_lowbd_blend_a64_d16_mask_c": (None, bl + [u32, i32, i32, i32, i32, vp]),
        "svt_aom_highbd_blend_a64_d16_mask_c": (None, bl + [u32, i32, i32, i32, i32, vp, i32]),
        "svt_av1_build_compound_diffwtd_mask_d16_c": (None, [vp, i32, vp, i32, vp, i32, i32, i32, vp, i32]),
        "svt_aom_build_masked_compound_no_round": (None, [vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, vp, C.c_uint8, C.c_bool]),
        "svt_aom_combine_interintra": (None, [i32, C.c_int8, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32]),
        "svt_aom_combine_interintra_highbd": (None, [i32, C.c_uint8, C.c_uint8, C.c_uint8, i32, i32, vp, i32, vp, i32, vp, i32, i32]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(ref, name)
        f.restype, f.argtypes = res, args
    # flags 0: every dispatch pointer is the `_c` function -- svt_memcpy (svt_av1_init_wedge_masks copies through it) and the two blend pointers
    # svt_aom_combine_interintra[_highbd] call
    ref.svt_aom_setup_common_rtcd_internal(C.c_uint64(0))
    ref.svt_aom_setup_rtcd_internal(C.c_uint64(0))
    for ptr in ("svt_aom_blend_a64_mask", "svt_aom_highbd_blend_a64_mask"):
        assert vp.in_dll(ref, ptr).value == C.cast(getattr(ref, ptr + "_c"), vp).value
    ref.svt_av1_init_wedge_masks()
    return ref


def ref_wedge_mask(rf, bsize, idx, sign):
    n = mc.BW[bsize] * mc.BH[bsize]
    addr = rf.svt_aom_get_contiguous_soft_mask(idx, sign, bsize)
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(addr)).reshape(mc.BH[bsize], mc.BW[bsize]).copy()


def ref_blend(rf, case, s0, s1, mask, in_place=None):
    """one of the six blend `_c` functions on blocks inside padded planes; returns the whole destination plane's block and whether the padding survived"""
    fn, w, h, bd, subw, subh, _ = case
    hbd = bd > 8
    dt = np.uint16 if hbd else np.uint8
    fill = 0xA5A5 if hbd else 0xA5
    a, b = np.full((h + 1, w + 3), 1, dt), np.full((h + 2, w + 5), 2, dt)
    a[:h, :w], b[:h, :w] = s0, s1
    dst = a if in_place == 0 else (b if in_place == 1 else np.full((h + 1, w + 2), fill, dt))
    m = np.ascontiguousarray(mask, np.uint8)
    head = [p(dst), dst.shape[1], p(a), a.shape[1], p(b), b.shape[1], p(m)]
    if fn == "mask":
        args = head + [m.shape[1], w, h, subw, subh]
        (rf.svt_aom_highbd_blend_a64_mask_c if hbd else rf.svt_aom_blend_a64_mask_c)(*args, *([bd] if hbd else []))
    elif hbd:
        getattr(rf, "svt_aom_highbd_blend_a64_%s_16bit_c" % fn)(*head, w, h, bd)
    else:
        getattr(rf, "svt_aom_blend_a64_%s_c" % fn)(*head, w, h)
    if in_place is None:
        assert np.all(dst[h:] == fill) and np.all(dst[:, w:] == fill)
    return dst[:h, :w].astype(np.int64)


def test_wedge_masks_every_byte(rf):
    wm = mc.wedge_masks()
    assert len(wm) == 288 and sum(m.size for m in wm.values()) == 100352
    for (bsize, idx, sign), m in wm.items():
        assert np.array_equal(ref_wedge_mask(rf, bsize, idx, sign), m), (bsize, idx, sign)
    assert mc.wedge_table_bytes().size == 100352


def test_obmc_and_smooth_masks(rf):
    for n, m in mc.OBMC_MASKS.items():
        got = np.ctypeslib.as_array((C.c_uint8 * n).from_address(rf.svt_av1_get_obmc_mask(n)))
        assert np.array_equal(got, m), n
    for bsize in range(22):
        bw, bh = mc.BW[bsize], mc.BH[bsize]
        for mode in range(4):
            buf = np.full((bh, bw + 3), 0xEE, np.uint8)
            rf.build_smooth_interintra_mask(p(buf), bw + 3, bsize, mode)
            assert np.array_equal(buf[:, :bw], mc.smooth_interintra_mask(bsize, mode)) and np.all(buf[:, bw:] == 0xEE), (bsize, mode)


def test_blend_functions(rf):
    """the six blend functions at 8 / 10 / 12 bit on random, flat, extreme and equal inputs, all four sub-sampling branches, masks random and constant 0 / 64, and
    in place on either source"""
    g = np.random.default_rng(11)
    for bd in BIT_DEPTHS:
        for kind in mc.CLASSES:
            for (w, h) in ((1, 1), (2, 2), (4, 4), (2, 16), (16, 2), (8, 8), (8, 32), (32, 8), (32, 32), (64, 64), (128, 4)):
                s0, s1 = mc.make_pair(g, kind, w, h, bd)
                for (subw, subh) in ((0, 0), (1, 1), (1, 0), (0, 1)):
                    for mk in ("random", 0, 64):
                        shape = (h << subh, w << subw)
                        mask = g.integers(0, 65, shape).astype(np.uint8) if mk == "random" else np.full(shape, mk, np.uint8)
                        case = ("mask", w, h, bd, subw, subh, kind)
                        want = mc.blend_a64_mask(s0, s1, mask, subw, subh)
                        for ip in (None, 0, 1):
                            assert np.array_equal(ref_blend(rf, case, s0, s1, mask, ip), want), (case, mk, ip)
                for fn, f in (("hmask", mc.blend_a64_hmask), ("vmask", mc.blend_a64_vmask)):
                    mask = g.integers(0, 65, w if fn == "hmask" else h).astype(np.uint8)
                    for ip in (None, 0, 1):
                        assert np.array_equal(ref_blend(rf, (fn, w, h, bd, 0, 0, kind), s0, s1, mask, ip), f(s0, s1, mask)), (fn, w, h, bd, kind, ip)


def test_diffwtd_builders_and_wedge_helpers(rf):
    g = np.random.default_rng(12)
    for bd in BIT_DEPTHS:
        for kind in mc.CLASSES:
            for (w, h) in ((8, 8), (16, 32), (32, 32), (64, 16)):
                a, b = mc.make_pair(g, kind, w, h, bd)
                for t in (0, 1):
                    m = np.full(w * h + 4, 0xEE, np.uint8)
                    if bd == 8:
                        rf.svt_av1_build_compound_diffwtd_mask_c(p(m), t, p(a), w, p(b), w, h, w)
                    else:
                        rf.svt_av1_build_compound_diffwtd_mask_highbd_c(p(m), t, p(a), w, p(b), w, h, w, bd)
                    assert np.array_equal(m[:w * h].reshape(h, w), mc.diffwtd_mask(t, a, b, bd)) and np.all(m[w * h:] == 0xEE), (bd, kind, w, h, t)
                # residual-domain helpers on the residuals these pixels give, which at 10 / 12 bit exceed the 10 signed bits the C's comment speaks of
                src = g.integers(0, 1 << bd, (h, w))
                n = w * h
                r0 = (src - a.astype(np.int64)).astype(np.int16).reshape(n)
                r1 = (src - b.astype(np.int64)).astype(np.int16).reshape(n)
                d10 = (b.astype(np.int64) - a.astype(np.int64)).astype(np.int16).reshape(n)
                assert rf.svt_aom_sum_squares_i16_c(p(r0), n) == int(mc.sum_squares_i16(r0))
                ds = np.zeros(n, np.int16)
                rf.svt_av1_wedge_compute_delta_squares_c(p(ds), p(r0), p(r1), n)
                assert np.array_equal(ds, mc.wedge_compute_delta_squares(r0, r1))
                mask = g.integers(0, 65, n).astype(np.uint8)
                assert rf.svt_av1_wedge_sse_from_residuals_c(p(r1), p(d10), p(mask), n) == int(mc.wedge_sse_from_residuals(r1, d10, mask))
                total = int((ds.astype(np.int64) * mask).sum())
                for limit in (total - 1, total, total + 1, -(1 << 40), 1 << 40):
                    assert rf.svt_av1_wedge_sign_from_residuals_c(p(ds), p(mask), n, limit) == int(mc.wedge_sign_from_residuals(ds, mask, limit)), limit


def test_combine_interintra(rf):
    """the seven luma sizes and their 4:2:0 chroma sizes, four smooth modes and the wedge path with its (subw, subh) derivation"""
    g = np.random.default_rng(13)
    for bd in BIT_DEPTHS:
        dt = np.uint16 if bd > 8 else np.uint8
        for bsize in mc.II_BSIZES:
            for chroma in (False, True):
                plane_bsize = mc.BSIZE_OF[(mc.BW[bsize] // 2, mc.BH[bsize] // 2)] if chroma else bsize
                bw, bh = mc.BW[plane_bsize], mc.BH[plane_bsize]
                inter, intra = mc.make_pair(g, "random", bw, bh, bd)
                for (mode, use_wedge, idx, sign) in ((0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (3, 0, 0, 0), (0, 1, 5, 0), (2, 1, 11, 1)):
                    comp = np.zeros((bh, bw + 1), dt)
                    args = [mode, use_wedge, idx, sign, bsize, plane_bsize, p(comp), bw + 1, p(inter), bw, p(intra), bw]
                    if bd > 8:
                        rf.svt_aom_combine_interintra_highbd(*args, bd)
                    else:
                        rf.svt_aom_combine_interintra(*args)
                    want = mc.combine_interintra(mode, use_wedge, idx, sign, bsize, plane_bsize, inter, intra)
                    assert np.array_equal(comp[:, :bw], want), (bd, bsize, chroma, mode, use_wedge)


def test_d16_functions_and_masked_compound(rf):
    """svt_aom_lowbd_ / highbd_blend_a64_d16_mask_c, svt_av1_build_compound_diffwtd_mask_d16_c and svt_aom_build_masked_compound_no_round (WEDGE with the (subw, subh) it
    derives from w, h and bsize; DIFFWTD on the seg mask the builder made) on ConvBufType blocks: values inside the range predictions give, beyond it on both sides (both
    clips), flat, equal, and 0 / 65535 (the builder's clamp at 64)"""
    import interpred_common as ic
    from conftest import load_pkg
    pkg = load_pkg()
    g = np.random.default_rng(15)
    for bd in BIT_DEPTHS:
        r0, r1 = ic.conv_rounds(bd, True)
        ro = ic.round_offset(bd, r0, r1)
        hi = ro + (((1 << bd) - 1) << (14 - r0 - r1))
        cp = pkg.ConvolveParams(0, 0, None, 0, r0, r1, 0, 1, 0, 0, 0, 0)
        dt, fill = (np.uint16, 0xA5A5) if bd > 8 else (np.uint8, 0xA5)
        blend = rf.svt_aom_highbd_blend_a64_d16_mask_c if bd > 8 else rf.svt_aom_lowbd_blend_a64_d16_mask_c
        tail = [bd] if bd > 8 else []
        for kind in ("inside", "beyond", "flat", "equal", "extreme"):
            for (w, h) in ((4, 4), (8, 16), (32, 32), (128, 64), (16, 8)):
                if kind == "extreme":
                    a, b = np.full((h, w), 65535, np.uint16), np.zeros((h, w), np.uint16)
                elif kind == "flat":
                    a, b = np.full((h, w), int(g.integers(ro, hi)), np.uint16), np.full((h, w), int(g.integers(ro, hi)), np.uint16)
                else:
                    lo_, hi_ = (max(ro - 60, 0), min(hi + 60, 65535)) if kind == "beyond" else (ro, hi)
                    a = g.integers(lo_, hi_ + 1, (h, w)).astype(np.uint16)
                    b = a.copy() if kind == "equal" else g.integers(lo_, hi_ + 1, (h, w)).astype(np.uint16)
                pa, pb = np.full((h, w + 3), 1, np.uint16), np.full((h, w + 1), 2, np.uint16)
                pa[:, :w], pb[:, :w] = a, b
                for (subw, subh) in ((0, 0), (1, 1), (1, 0), (0, 1)):
                    mask = g.integers(0, 65, (h << subh, w << subw)).astype(np.uint8)
                    dst = np.full((h + 1, w + 2), fill, dt)
                    blend(p(dst), w + 2, p(pa), w + 3, p(pb), w + 1, p(mask), mask.shape[1], w, h, subw, subh, C.addressof(cp), *tail)
                    assert np.array_equal(dst[:h, :w], mc.blend_a64_d16_mask(a, b, mask, subw, subh, bd, r0, r1)) and np.all(dst[h:] == fill) and np.all(dst[:, w:] == fill), \
                        (bd, kind, w, h, subw, subh)
                segs = []
                for t in (0, 1):
                    m = np.full(w * h + 4, 0xEE, np.uint8)
                    rf.svt_av1_build_compound_diffwtd_mask_d16_c(p(m), t, p(pa), w + 3, p(pb), w + 1, h, w, C.addressof(cp), bd)
                    want = mc.diffwtd_mask_d16(t, a, b, bd, r0, r1)
                    assert np.array_equal(m[:w * h].reshape(h, w), want) and np.all(m[w * h:] == 0xEE), (bd, kind, w, h, t)
                    if kind == "extreme":
                        assert np.all(want == (0 if t else 64))
                    if kind == "equal":
                        assert np.all(want == (26 if t else 38))
                    segs.append(np.ascontiguousarray(want))
                # svt_aom_build_masked_compound_no_round: COMPOUND_DIFFWTD (3) on the seg mask, COMPOUND_WEDGE (2) where (w, h) is a wedge size or its 4:2:0 chroma size
                for t in (0, 1):
                    comp = (C.c_uint8 * 4)(3, 0, 0, t)
                    dst = np.full((h, w + 2), fill, dt)
                    rf.svt_aom_build_masked_compound_no_round(p(dst), w + 2, p(pa), w + 3, p(pb), w + 1, C.addressof(comp), p(segs[t]), mc.BSIZE_OF[(w, h)], h, w,
                                                              C.addressof(cp), bd, bd > 8)
                    assert np.array_equal(dst[:, :w], mc.blend_a64_d16_mask(a, b, segs[t], 0, 0, bd, r0, r1)), (bd, kind, w, h, t)
                for (bsize, sub) in (((mc.BSIZE_OF.get((w, h)), 0), (mc.BSIZE_OF.get((2 * w, 2 * h)), 1))):
                    if bsize in mc.WEDGE_BSIZES:
                        for (idx, sign) in ((0, 0), (7, 1), (13, 0)):
                            comp = (C.c_uint8 * 4)(2, idx, sign, 0)
                            dst = np.full((h, w + 2), fill, dt)
                            rf.svt_aom_build_masked_compound_no_round(p(dst), w + 2, p(pa), w + 3, p(pb), w + 1, C.addressof(comp), None, bsize, h, w, C.addressof(cp), bd,
                                                                      bd > 8)
                            want = mc.blend_a64_d16_mask(a, b, mc.wedge_masks()[(bsize, idx, sign)], sub, sub, bd, r0, r1)
                            assert np.array_equal(dst[:, :w], want), (bd, kind, w, h, bsize, idx, sign)


def ref_search(rf, src, p0, p1, bsize, bd, fixed_sign):
    """pick_wedge / pick_wedge_fixed_sign / pick_interinter_seg with use_rate == 0, composed from the reference's helpers exactly as those functions compose them"""
    bw, bh = mc.BW[bsize], mc.BH[bsize]
    n = bw * bh
    s, a, c = (np.asarray(v, np.int64).reshape(n) for v in (src, p0, p1))
    r0, r1, d10 = (s - a).astype(np.int16), (s - c).astype(np.int16), (c - a).astype(np.int16)
    limit = (int(rf.svt_aom_sum_squares_i16_c(p(r0), n)) - int(rf.svt_aom_sum_squares_i16_c(p(r1), n))) * 64 // 2
    ds = np.zeros(n, np.int16)
    rf.svt_av1_wedge_compute_delta_squares_c(p(ds), p(r0), p(r1), n)
    sse, sign = np.zeros(16, np.uint64), np.zeros(16, np.uint8)
    for k in range(16):
        sg = fixed_sign - 1 if fixed_sign else rf.svt_av1_wedge_sign_from_residuals_c(p(ds), rf.svt_aom_get_contiguous_soft_mask(k, 0, bsize), n, limit)
        sse[k], sign[k] = rf.svt_av1_wedge_sse_from_residuals_c(p(r1), p(d10), rf.svt_aom_get_contiguous_soft_mask(k, sg, bsize), n), sg
    seg = np.zeros(2, np.uint64)
    pa, pc = np.ascontiguousarray(p0), np.ascontiguousarray(p1)
    for t in (0, 1):
        m = np.zeros(n, np.uint8)
        if bd == 8:
            rf.svt_av1_build_compound_diffwtd_mask_c(p(m), t, p(pa), bw, p(pc), bw, bh, bw)
        else:
            rf.svt_av1_build_compound_diffwtd_mask_highbd_c(p(m), t, p(pa), bw, p(pc), bw, bh, bw, bd)
        seg[t] = rf.svt_av1_wedge_sse_from_residuals_c(p(r1), p(d10), p(m), n)
    return sse, sign, seg


def test_search(rf):
    g = np.random.default_rng(14)
    for bsize in mc.WEDGE_BSIZES:
        for bd in BIT_DEPTHS:
            for kind in ("near", "random", "equal", "tie"):
                for fs in (0, 1, 2):
                    src, p0, p1 = mc.make_search_inputs(g, kind, bsize, bd)
                    sse, sign, seg = ref_search(rf, src, p0, p1, bsize, bd, fs)
                    r = mc.wedge_search(src, p0, p1, bsize, bd, fs)
                    assert np.array_equal(sse, r["sse"]) and np.array_equal(sign, r["sign"]) and np.array_equal(seg, r["sse_diffwtd"]), (bsize, bd, kind, fs)
                    assert r["best_wedge_index"] == int(np.argmin(sse)) and r["best_wedge_sign"] == int(sign[np.argmin(sse)])  # (argmin: the first minimum)


def _golden_from_reference(rf):
    out = {"seed": np.array([mc.GOLDEN_SEED], np.int64), "wedge_table": np.concatenate([ref_wedge_mask(rf, b, i, s).reshape(-1) for b in mc.WEDGE_BSIZES
                                                                                         for i in range(16) for s in (0, 1)])}
    out["obmc"] = np.concatenate([np.ctypeslib.as_array((C.c_uint8 * n).from_address(rf.svt_av1_get_obmc_mask(n))) for n in (1, 2, 4, 8, 16, 32)])
    sm = []
    for bsize in range(10):  # the seven inter-intra sizes and their 4:2:0 chroma sizes
        for mode in range(4):
            buf = np.zeros((mc.BH[bsize], mc.BW[bsize]), np.uint8)
            rf.build_smooth_interintra_mask(p(buf), mc.BW[bsize], bsize, mode)
            sm.append(buf.reshape(-1))
    out["smooth"] = np.concatenate(sm)
    for i, case in enumerate(mc.golden_blend_cases()):
        s0, s1, mask = mc.golden_blend_inputs(i, case)
        out["blend_%d" % i] = ref_blend(rf, case, s0, s1, mask).astype(s0.dtype)
        out["blend_insum_%d" % i] = np.array([int(s0.astype(np.int64).sum()) + int(s1.astype(np.int64).sum()) + int(mask.astype(np.int64).sum())], np.int64)
    for i, case in enumerate(mc.golden_search_cases()):
        src, p0, p1 = mc.golden_search_inputs(i, case)
        sse, sign, seg = ref_search(rf, src, p0, p1, case[0], case[1], case[3])
        out["search_%d" % i] = np.concatenate([sse, seg, sign.astype(np.uint64)])
        out["search_insum_%d" % i] = np.array([int(src.astype(np.int64).sum()) + int(p0.astype(np.int64).sum()) + int(p1.astype(np.int64).sum())], np.int64)
    return out


def test_golden_file_is_what_the_reference_computes(rf):
    """tests/golden/maskpred.npz (what tests/test_maskpred.py compares the kernels with where no reference exists) == the reference's outputs, entry for entry"""
    now = _golden_from_reference(rf)
    if os.environ.get("SVT_MASKPRED_WRITE_GOLDEN") == "1":
        np.savez_compressed(mc.GOLDEN_FILE, **now)
    assert os.path.getsize(mc.GOLDEN_FILE) < 512 * 1024
    gold = mc.load_golden()
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert gold[k].dtype == now[k].dtype and np.array_equal(gold[k], now[k]), k
    assert np.array_equal(gold["wedge_table"], mc.wedge_table_bytes())
    assert len(mc.golden_blend_cases()) >= 90 and len(mc.golden_search_cases()) >= 80
