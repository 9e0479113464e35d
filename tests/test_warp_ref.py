"""Pins tests/warp_common.py (the numpy restatement the kernels of csrc/warp.hip are checked against) on the REAL reference in oracle/_ref/libsvtref.so: every entry of
svt_aom_warped_filter (read from the library's data symbol) and the range of its taps, every entry of div_lut (a static array: read from the reference's source text),
svt_av1_warp_affine_c and svt_av1_highbd_warp_affine_c over the sizes, models, positions, formats and compound forms tests/test_warp.py runs, svt_find_projection and
svt_get_shear_params on random and constructed sample sets, svt_av1_warp_error with and without a finite bound, and the roundings of get_conv_params.  CPU only; runs where
the reference's sources and the library exist, skipped elsewhere.  `SVT_WARP_WRITE_GOLDEN=1` rewrites tests/golden/warp.npz from the reference's outputs.

The reference's high-bit-depth C takes 10-bit samples by construction ((ref8b << 2) | (ref2b >> 6)): full-range 12-bit samples are checked against the restatement only
(tests/test_warp.py); the restatement's 12-bit roundings are pinned here on the C with samples <= 1023 and bd = 12.

The model fit's `shift < 0` branch and a negative determinant cannot be reached through the C: every accepted sample adds at least 4 to both diagonal sums, so by
Cauchy-Schwarz the determinant is positive and shift >= 1 inside the range the C's own asserts on the sums allow (the reference is built with them on: a sample set
beyond that range aborts the process).  The smallest shifts the sums can make are asserted here; determinants of either sign and shift < 0 are run by
tests/test_warp.py, kernel against restatement, with the `wrapped` sets whose int32_t sums wrap."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import warp_common as wc
from conftest import REF_LIB, load_pkg, p

REF = os.environ.get("SVT_REF", "/root/reference")
WM_C = os.path.join(REF, "Source", "Lib", "Codec", "warped_motion.c")
pytestmark = pytest.mark.skipif(not os.path.isfile(WM_C) or not os.path.exists(REF_LIB), reason="the reference's sources or oracle/_ref/libsvtref.so are not on this machine")

vp, i32, i16 = C.c_void_p, C.c_int, C.c_int16


class WarpedMotionParams(C.Structure):
    """EbWarpedMotionParams (definitions.h:1997)"""
    _fields_ = [("wmtype", C.c_int), ("wmmat", C.c_int32 * 6), ("alpha", i16), ("beta", i16), ("gamma", i16), ("delta", i16), ("invalid", C.c_int8)]


@pytest.fixture(scope="module")
def rf(ref):
    sigs = {
        "svt_av1_warp_affine_c": (None, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, i16, i16, i16, i16]),
        "svt_av1_highbd_warp_affine_c": (None, [vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i16, i16, i16, i16]),
        "svt_find_projection": (C.c_bool, [i32, vp, vp, C.c_uint8, i32, i32, vp, i32, i32]),
        "svt_get_shear_params": (i32, [vp]),
        "svt_av1_warp_error": (C.c_int64, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, C.c_uint8, C.c_int64]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(ref, name)
        f.restype, f.argtypes = res, args
    ref.svt_aom_setup_common_rtcd_internal(C.c_uint64(0))  # flags 0: svt_av1_warp_affine and the SAD pointer of svt_av1_warp_error are the `_c` functions
    ref.svt_aom_setup_rtcd_internal(C.c_uint64(0))
    assert vp.in_dll(ref, "svt_av1_warp_affine").value == C.cast(ref.svt_av1_warp_affine_c, vp).value
    return ref


def conv_params(r0, r1, is_compound=0, do_average=0, jnt=0, fwd=0, bck=0, dst=None, dst_stride=0):
    cp = load_pkg().ConvolveParams()
    cp.round_0, cp.round_1, cp.is_compound, cp.do_average, cp.use_jnt_comp_avg, cp.fwd_offset, cp.bck_offset = r0, r1, is_compound, do_average, jnt, fwd, bck
    cp.dst, cp.dst_stride = (dst.ctypes.data if dst is not None else None), dst_stride
    return cp


def ref_warp(rf, pic, mat, shear, width, height, p_col, p_row, pw, ph, ssx, ssy, bd, cp, highbd):
    """the C on a picture inside a padded plane; returns the p_height x p_width block of pred"""
    m = np.array(mat, np.int32)
    stride = pic.shape[1]
    fill = 0xA5A5 if highbd else 0xA5
    pred = np.full((ph + 1, pw + 3), fill, np.uint16 if highbd else np.uint8)
    if highbd:
        r8, r2 = (pic >> 2).astype(np.uint8), ((pic & 3) << 6).astype(np.uint8)
        rf.svt_av1_highbd_warp_affine_c(p(m), p(r8), p(r2), width, height, stride, stride, p(pred), p_col, p_row, pw, ph, pred.shape[1], ssx, ssy, bd, C.byref(cp), *shear)
    else:
        rf.svt_av1_warp_affine_c(p(m), p(pic), width, height, stride, p(pred), p_col, p_row, pw, ph, pred.shape[1], ssx, ssy, C.byref(cp), *shear)
    assert np.all(pred[ph:] == fill) and np.all(pred[:, pw:] == fill)
    return pred[:ph, :pw].astype(np.int64)


def ref_pred(rf, refs, p_col, p_row, pw, ph, ssx, ssy, bd, compound, fwd, bck):
    """the call sequence plane_warped_motion_prediction makes; refs = [(plane, mat, shear, width, height)]"""
    hbd = bd > 8
    if compound == 0:
        r0, r1 = wc.conv_rounds(bd, False)
        pl, mat, sh, w, h = refs[0]
        return ref_warp(rf, pl, mat, sh, w, h, p_col, p_row, pw, ph, ssx, ssy, bd, conv_params(r0, r1), hbd)
    r0, r1 = wc.conv_rounds(bd, True)
    cb = np.zeros((ph, 128), np.uint16)
    pl, mat, sh, w, h = refs[0]
    ref_warp(rf, pl, mat, sh, w, h, p_col, p_row, pw, ph, ssx, ssy, bd, conv_params(r0, r1, 1, 0, dst=cb, dst_stride=128), hbd)
    pl, mat, sh, w, h = refs[1]
    return ref_warp(rf, pl, mat, sh, w, h, p_col, p_row, pw, ph, ssx, ssy, bd, conv_params(r0, r1, 1, 1, int(compound == 2), fwd, bck, cb, 128), hbd)


def test_filter_table_every_entry(rf):
    tab = np.ctypeslib.as_array((C.c_int16 * (193 * 8)).in_dll(rf, "svt_aom_warped_filter")).reshape(193, 8)
    assert np.array_equal(tab, wc.WARPED_FILTER)
    assert tab.min() == -22 and tab.max() == 127 and np.all(tab.sum(1) == 128)  # int8 taps; the 8-bit kernel relies on the sum


def test_divisor_table_every_entry():
    text = open(WM_C).read()
    body = re.search(r"div_lut\[DIV_LUT_NUM \+ 1\]\s*=\s*\{(.*?)\}", text, re.S).group(1)
    vals = [int(v) for v in re.findall(r"\d+", body)]
    assert len(vals) == 257 and vals == wc.DIV_LUT.tolist() and vals[0] == 16384 and vals[256] == 8192
    assert re.search(r"#define USE_LIMITED_PREC_MULT 0", text)  # the get_mult_shift_* pair the restatement follows


def test_conv_params_roundings():
    """get_conv_params(0, 0, 0, 8) (what warp_error uses) and the non-compound get_conv_params_no_round at 8 bit are the same function with the same arguments
    (convolve.h:66-68): round_0 3, round_1 11; 12 bit raises round_0 to 5"""
    text = open(os.path.join(REF, "Source", "Lib", "Codec", "convolve.h")).read()
    assert re.search(r"get_conv_params\(int32_t ref, int32_t do_average, int32_t plane, int32_t bd\)\s*\{\s*return get_conv_params_no_round\(ref, do_average, plane, NULL, 0, 0, bd\);", text)
    assert re.search(r"#define ROUND0_BITS 3", text) and re.search(r"#define COMPOUND_ROUND1_BITS 7", text)
    assert wc.conv_rounds(8, False) == (3, 11) and wc.conv_rounds(10, False) == (3, 11) and wc.conv_rounds(12, False) == (5, 9)
    assert wc.conv_rounds(8, True) == (3, 7) and wc.conv_rounds(10, True) == (3, 7) and wc.conv_rounds(12, True) == (5, 7)


SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (64, 8), (4, 4), (4, 8), (12, 20), (14, 6), (1, 1)]
POSITIONS = [(16, 16), (3, 5), (-5, 21), (66, 13), (30, -4), (29, 51), (-6, -6), (67, 50), (-30, 20), (110, 20), (20, -40), (20, 100), (-400, -400), (700, 650)]


def test_warp_affine_over_the_case_list(rf):
    """sizes x models x positions (inside, straddling each border and corner, outside by a few samples and far outside), the four sub-samplings, 8 / 10 / 12 bit,
    the three sample classes, compound 0 / 1 / 2 with two different models, pictures and bounds"""
    g = np.random.default_rng(31)
    mods = wc.models()
    names = list(mods)
    wc.ROWS_SEEN.clear()
    k = 0
    for bd in (8, 10, 12):
        for kind in wc.CLASSES:
            smax = min(bd, 10)  # (the C's high-bit-depth samples are 10 bit by construction)
            A = wc.make_picture(g, kind, 72, 56, 77, smax)
            B = wc.make_picture(g, kind, 41, 33, 45, smax)
            for (pw, ph) in SIZES:
                for pos in POSITIONS:
                    k += 1
                    if (k + bd) % 3:  # a third of the product per depth and class; every size meets every position across the nine pictures
                        continue
                    ssx, ssy = ((0, 0), (1, 1), (1, 0), (0, 1))[k % 4]
                    comp, (fwd, bck) = k % 3, ((9, 7), (11, 5), (12, 4), (13, 3))[(k // 3) % 4]
                    m0, m1 = mods[names[k % len(names)]], mods[names[(k // 2 + 5) % len(names)]]
                    refs = [(A.astype(np.uint16 if bd > 8 else np.uint8), m0[0], m0[1], 72, 56), (B.astype(np.uint16 if bd > 8 else np.uint8), m1[0], m1[1], 41, 33)]
                    want = ref_pred(rf, refs, pos[0], pos[1], pw, ph, ssx, ssy, bd, comp, fwd, bck)
                    got = wc.warp_pred(refs, pos[0], pos[1], pw, ph, ssx, ssy, bd, comp, fwd, bck)
                    assert np.array_equal(got, want), (bd, kind, pw, ph, pos, ssx, ssy, comp, names[k % len(names)])
    assert 0 in wc.ROWS_SEEN and 192 in wc.ROWS_SEEN


def test_warp_affine_edge_pictures_and_clamps(rf):
    """a 1-sample-wide and a 1-row-high picture; mat[0] / mat[1] at +-WARPEDMODEL_TRANS_CLAMP; one 128 x 128 block; every do_average / use_jnt_comp_avg combination
    with roundings other than the defaults"""
    g = np.random.default_rng(32)
    ident = (0, 0, 0, 0)
    for bd in (8, 10):
        hbd = bd > 8
        dt = np.uint16 if hbd else np.uint8
        for (w, h) in ((1, 40), (40, 1), (1, 1)):
            pic = wc.make_picture(g, "random", w, h, w + 3, bd)
            for name in ("translation", "affine", "beta_limit"):
                mat, sh = wc.models()[name]
                r0, r1 = wc.conv_rounds(bd, False)
                want = ref_warp(rf, pic, mat, sh, w, h, 2, 1, 12, 20, 0, 0, bd, conv_params(r0, r1), hbd)
                assert np.array_equal(wc.warp_affine(pic, mat, sh, w, h, 2, 1, 12, 20, 0, 0, bd, r0, r1), want), (bd, w, h, name)
        pic = wc.make_picture(g, "random", 72, 56, 77, bd)
        for t0 in (-wc.TRANS_CLAMP, wc.TRANS_CLAMP - 1):
            for t1 in (-wc.TRANS_CLAMP, wc.TRANS_CLAMP - 1):
                mat = [t0, t1, 65536 + 900, -700, 650, 65536 - 800]
                sh = wc.get_shear_params(mat)
                r0, r1 = wc.conv_rounds(bd, False)
                want = ref_warp(rf, pic, mat, sh, 72, 56, 13, 22, 16, 16, 1, 1, bd, conv_params(r0, r1), hbd)
                assert np.array_equal(wc.warp_affine(pic, mat, sh, 72, 56, 13, 22, 16, 16, 1, 1, bd, r0, r1), want), (bd, t0, t1)
        mat, sh = wc.models()["rotation"]
        r0, r1 = wc.conv_rounds(bd, False)
        want = ref_warp(rf, pic, mat, sh, 72, 56, -20, -30, 128, 128, 0, 0, bd, conv_params(r0, r1), hbd)
        assert np.array_equal(wc.warp_affine(pic, mat, sh, 72, 56, -20, -30, 128, 128, 0, 0, bd, r0, r1), want), bd
        mat, sh = wc.models()["affine"]
        for (r0, r1) in ((3, 7), (5, 7), (4, 6), (0, 7), (7, 7), (7, 0)):
            cb = g.integers(0, 1 << 16, (20, 128)).astype(np.uint16)
            for avg, jnt in ((0, 0), (1, 0), (1, 1)):
                cbc = cb.copy()
                cp = conv_params(r0, r1, 1, avg, jnt, 11, 5, cbc, 128)
                want = ref_warp(rf, pic, mat, sh, 72, 56, 5, 9, 12, 20, 0, 0, bd, cp, hbd)
                got = wc.warp_affine(pic, mat, sh, 72, 56, 5, 9, 12, 20, 0, 0, bd, r0, r1, True, bool(avg), bool(jnt), 11, 5, cb[:, :12], hbd)
                assert np.array_equal(got, want if avg else cbc[:, :12]), (bd, r0, r1, avg, jnt)
            if r0 + r1 <= 14:  # not compound: round_1 is not read
                want = ref_warp(rf, pic, mat, sh, 72, 56, 5, 9, 12, 20, 0, 0, bd, conv_params(r0, r1), hbd)
                assert np.array_equal(wc.warp_affine(pic, mat, sh, 72, 56, 5, 9, 12, 20, 0, 0, bd, r0, r1, highbd=hbd), want), (bd, r0, r1)
    # 12-bit roundings on the C, samples <= 1023
    pic = wc.make_picture(g, "random", 72, 56, 77, 10)
    for comp in (0, 1, 2):
        refs = [(pic, *wc.models()["affine"], 72, 56), (pic, *wc.models()["zoom"], 72, 56)]
        assert np.array_equal(wc.warp_pred(refs, 7, 3, 16, 16, 0, 0, 12, comp, 9, 7), ref_pred(rf, refs, 7, 3, 16, 16, 0, 0, 12, comp, 9, 7)), comp


def ref_projection(rf, s):
    wm = WarpedMotionParams()
    for k in range(6):
        wm.wmmat[k] = 0x5A5A5A
    pts, ptr = np.array(s["pts"], np.int32), np.array(s["pts_inref"], np.int32)
    bad = rf.svt_find_projection(s["np"], p(pts), p(ptr), s["bsize"], s["mv_row"], s["mv_col"], C.byref(wm), s["mi_row"], s["mi_col"])
    return None if bad else (list(wm.wmmat), (wm.alpha, wm.beta, wm.gamma, wm.delta))


def test_find_projection_and_shear_params(rf):
    g = np.random.default_rng(33)
    kinds = ["random"] * 2000 + ["rejected"] * 20 + ["single"] * 200 + ["far"] * 200
    n_valid = n_clamped = 0
    min_shift = 99
    for kind in kinds:
        s = wc.model_sample_set(g, kind)
        tr = {}
        got = wc.find_projection(s["np"], s["pts"], s["pts_inref"], s["bsize"], s["mv_row"], s["mv_col"], s["mi_row"], s["mi_col"], tr)
        assert got == ref_projection(rf, s), (kind, s, tr)
        n_valid += got is not None
        assert tr["det"] >= 0 and tr.get("shift", 1) >= 1
        n_clamped += bool(tr.get("trans_clamped"))
        min_shift = min(min_shift, tr.get("shift", 99))
        if kind == "rejected":
            assert tr["det"] == 0 and got is None
    assert n_valid > 1000 and n_clamped > 50 and min_shift <= 4, (n_valid, n_clamped, min_shift)
    for _ in range(3000):  # svt_get_shear_params on its own: models around and beyond the shear limit, mat[2] <= 0
        mat = [int(g.integers(-1 << 20, 1 << 20)), int(g.integers(-1 << 20, 1 << 20)), 65536 + int(g.integers(-30000, 30000)), int(g.integers(-20000, 20000)),
               int(g.integers(-20000, 20000)), 65536 + int(g.integers(-30000, 30000))]
        if _ % 50 == 0:
            mat[2] = -mat[2] if _ % 100 else 0
        wm = WarpedMotionParams()
        wm.wmtype = 3
        for k in range(6):
            wm.wmmat[k] = mat[k]
        ok = rf.svt_get_shear_params(C.byref(wm))
        got = wc.get_shear_params(mat)
        assert (got is not None) == bool(ok), mat
        if ok:
            assert got == (wm.alpha, wm.beta, wm.gamma, wm.delta), mat


def ref_error(rf, pic, mat, sh, w, h, src, p_col, p_row, pw, ph, ss, chess, best):
    wm = WarpedMotionParams()
    wm.wmtype = 3  # AFFINE: svt_warp_plane leaves mat[4], mat[5] alone; svt_av1_warp_error recomputes the shears from mat
    for k in range(6):
        wm.wmmat[k] = mat[k]
    r = rf.svt_av1_warp_error(C.byref(wm), p(pic), w, h, pic.shape[1], p(src), p_col, p_row, pw, ph, src.shape[1], ss, ss, chess, best)
    assert (wm.alpha, wm.beta, wm.gamma, wm.delta) == tuple(sh)
    return r


def test_warp_error(rf):
    """with best_error = INT64_MAX the full sum; with finite bounds the C leaves early iff the full, undoubled sum exceeds the bound (what the header of
    svt_hip_warp_error_batch tells a caller to compare)"""
    g = np.random.default_rng(34)
    for (name, w, h, pc, pr, pw, ph, ss, chess) in wc.golden_error_cases() + [("rotation", 100, 70, 0, 0, 100, 70, 0, 0), ("affine", 100, 70, 0, 0, 100, 70, 1, 1)]:
        mat, sh = wc.models()[name]
        pic = wc.make_picture(g, "random", w, h, w + 5, 8)
        src = wc.make_picture(g, "random", pc + pw, pr + ph, pc + pw + 3, 8)
        full = wc.warp_error(pic, mat, sh, w, h, src, pc, pr, pw, ph, ss, ss, chess)
        assert ref_error(rf, pic, mat, sh, w, h, src, pc, pr, pw, ph, ss, chess, (1 << 63) - 1) == full, name
        undoubled = full // 2 if chess else full
        for best in (undoubled - 1, undoubled, undoubled + 1, undoubled // 3, 0):
            r = ref_error(rf, pic, mat, sh, w, h, src, pc, pr, pw, ph, ss, chess, best)
            assert r == wc.warp_error(pic, mat, sh, w, h, src, pc, pr, pw, ph, ss, ss, chess, best), (name, best)
            early = undoubled > best
            if not early:
                assert r == full
            else:
                assert r > best and r <= undoubled  # a partial (or the complete undoubled) sum that already exceeds the bound


def _golden_from_reference(rf):
    out = {"seed": np.array([wc.GOLDEN_SEED], np.int64)}
    mods = wc.models()
    pics = {(bd, k): wc.golden_picture(min(bd, 10), k) for bd in (8, 10, 12) for k in (0, 1)}
    for bd in (8, 10, 12):
        for k in (0, 1):
            out["pic_%d_%d" % (bd, k)] = pics[(bd, k)]
    for i, (name, bd, pc, pr, pw, ph, ssx, ssy, comp, fwd, bck, second) in enumerate(wc.golden_warp_cases()):
        refs = [(pics[(bd, 0)], *mods[name], wc.GOLDEN_W, wc.GOLDEN_H), (pics[(bd, 1)], *mods[second], wc.GOLDEN_W, wc.GOLDEN_H)]
        out["warp_%d" % i] = ref_pred(rf, refs, pc, pr, pw, ph, ssx, ssy, bd, comp, fwd, bck).astype(np.uint16)
    res = []
    for s in wc.golden_model_sets():
        r = ref_projection(rf, s)
        res.append([1] + [0] * 10 if r is None else [0] + r[0] + list(r[1]))
    out["model"] = np.array(res, np.int64)
    err = []
    for (name, w, h, pc, pr, pw, ph, ss, chess) in wc.golden_error_cases():
        err.append(ref_error(rf, pics[(8, 0)], *mods[name], w, h, pics[(8, 1)], pc, pr, pw, ph, ss, chess, (1 << 63) - 1))
    out["error"] = np.array(err, np.int64)
    return out


def test_golden_file_is_what_the_reference_computes(rf):
    """tests/golden/warp.npz (what tests/test_warp.py compares the kernels with where no reference exists) == the reference's outputs, entry for entry"""
    now = _golden_from_reference(rf)
    if os.environ.get("SVT_WARP_WRITE_GOLDEN") == "1":
        np.savez_compressed(wc.GOLDEN_FILE, **now)
    assert os.path.getsize(wc.GOLDEN_FILE) <= os.path.getsize(os.path.join(os.path.dirname(wc.GOLDEN_FILE), "maskpred.npz"))
    gold = wc.load_golden()
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert gold[k].dtype == now[k].dtype and np.array_equal(gold[k], now[k]), k
    assert len(wc.golden_warp_cases()) >= 70 and len(wc.golden_model_sets()) >= 60
