"""Pins tests/intrapred_common.py (the numpy restatement the kernels of csrc/intrapred.hip are checked against) on the REAL reference.  CPU only; needs the
reference's sources and oracle/_ref/libsvtref.so, so it runs in the build container only and is skipped elsewhere.

tests/intrapred_ref_harness.c is compiled at test time into tmp_path: it names the reference's enc_intra_prediction.c in an #include, where it lies, and adds plain-C
entry points around the two static builders (a MacroBlockD whose neighbour mode infos produce the wanted filt_type).  The exported `_c` functions and tables are
called directly from oracle/_ref/libsvtref.so.  `SVT_INTRAPRED_WRITE_GOLDEN=1` rewrites tests/golden/intrapred.npz from the harness's outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import intrapred_common as ic
from conftest import REF_LIB, ROOT, p

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "enc_intra_prediction.c")), reason="the reference's sources are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
BIT_DEPTHS = (8, 10, 12)
I32 = C.c_int32


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("intrapred") / "libintrapred_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "intrapred_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    vp = C.c_void_p
    h.harness_build_intra_predictors.restype, h.harness_build_intra_predictors.argtypes = C.c_int, [vp, vp, vp] + [C.c_int] * 11
    h.harness_build_intra_predictors_high.restype, h.harness_build_intra_predictors_high.argtypes = C.c_int, [vp, vp, vp] + [C.c_int] * 12
    h.harness_sized_predictor.restype, h.harness_sized_predictor.argtypes = None, [C.c_int] * 4 + [vp, C.c_int, vp, vp, C.c_int]
    dr = [vp, C.c_ssize_t, I32, I32, vp, vp, I32, I32, I32]
    for z in (1, 2, 3):
        f8, f16 = getattr(ref, "svt_av1_dr_prediction_z%d_c" % z), getattr(ref, "svt_av1_highbd_dr_prediction_z%d_c" % z)
        f8.restype, f8.argtypes = None, dr + ([I32] if z == 2 else [])
        f16.restype, f16.argtypes = None, dr + ([I32] if z == 2 else []) + [I32]
    ref.svt_av1_filter_intra_predictor_c.restype, ref.svt_av1_filter_intra_predictor_c.argtypes = None, [vp, C.c_ssize_t, C.c_uint8, vp, vp, I32]
    ref.svt_aom_highbd_filter_intra_predictor.restype, ref.svt_aom_highbd_filter_intra_predictor.argtypes = None, [vp, C.c_ssize_t, C.c_uint8, vp, vp, C.c_int, C.c_int]
    for n in ("svt_av1_filter_intra_edge_c", "svt_av1_filter_intra_edge_high_c", "svt_av1_upsample_intra_edge_high_c"):
        getattr(ref, n).restype, getattr(ref, n).argtypes = None, [vp, I32, I32]
    ref.svt_av1_upsample_intra_edge_c.restype, ref.svt_av1_upsample_intra_edge_c.argtypes = None, [vp, I32]
    for n in ("lbd", "hbd"):
        f = getattr(ref, "svt_cfl_predict_%s_c" % n)
        f.restype, f.argtypes = None, [vp, vp, I32, vp, I32, I32, I32, I32, I32]
        f = getattr(ref, "svt_cfl_luma_subsampling_420_%s_c" % n)
        f.restype, f.argtypes = None, [vp, I32, vp, I32, I32]
    ref.svt_subtract_average_c.restype, ref.svt_subtract_average_c.argtypes = None, [vp, I32, I32, I32, I32]
    h.ref = ref
    return h


def ref_build(h, c, top, left, bd, fill=0xA5):
    """the reference's builder on one case of intrapred_common: top[0] is the corner; returns the w x h block and checks that nothing else of dst was written"""
    dt = np.uint16 if bd > 8 else np.uint8
    w, hh = c["w"], c["h"]
    nt, ntr, nl, nbl = ic.avail_counts(c["avail"], w, hh)
    t, l = np.ascontiguousarray(top, dtype=dt), np.ascontiguousarray(left, dtype=dt)
    fillv = fill * 0x101 if bd > 8 else fill
    dst = np.full((hh + 1, w + 3), fillv, dt)
    tx = ic.TX_SIZES.index((w, hh))
    args = [t.ctypes.data + t.itemsize, p(l), p(dst), dst.shape[1], c["mode"], c["delta"], c["fi"], tx, c["disable"], nt, ntr, nl, nbl, c["filt_type"]]
    if bd > 8:
        assert h.harness_build_intra_predictors_high(*args, bd) == 0
    else:
        assert h.harness_build_intra_predictors(*args) == 0
    assert np.all(dst[hh:] == fillv) and np.all(dst[:, w:] == fillv)
    return dst[:hh, :w].astype(np.int64)


def test_tables_are_the_reference(harness):
    ref = harness.ref
    assert np.array_equal(np.ctypeslib.as_array((C.c_uint8 * 128).in_dll(ref, "sm_weight_arrays")), ic.SM_WEIGHTS)
    assert np.array_equal(np.ctypeslib.as_array((C.c_int8 * 320).in_dll(ref, "eb_av1_filter_intra_taps")).reshape(5, 8, 8), ic.FILTER_INTRA_TAPS)
    harness.harness_mode_angle.restype = C.c_int
    assert [harness.harness_mode_angle(m) for m in range(13)] == list(ic.MODE_TO_ANGLE)
    for bs0, bs1 in ((4, 4), (4, 8), (8, 8), (4, 16), (8, 16), (16, 16), (16, 32), (32, 32), (64, 64)):
        for d in range(-90, 91):
            for t in (0, 1):
                assert ref.svt_aom_intra_edge_filter_strength(bs0, bs1, d, t) == ic.edge_filter_strength(bs0, bs1, d, t)
                assert ref.svt_aom_use_intra_edge_upsample(bs0, bs1, d, t) == ic.use_upsample(bs0, bs1, d, t)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_builders_every_size_mode_delta(harness, bd):
    """all 19 sizes x 13 modes x 7 deltas and the 5 filter-intra modes at w, h <= 32, availability classes / filt_type / disable_edge_filter / input classes cycling
    (intrapred_common.every_case: what tests/test_intrapred.py launches).  The static derivative table is pinned through these results: all 56 directional angles."""
    g = np.random.default_rng(100 + bd)
    angles = set()
    for k, c in enumerate(ic.every_case()):
        top, left = ic.case_inputs(g, c, bd)
        assert np.array_equal(ref_build(harness, c, top, left, bd), ic.predict_case(c, top, left, bd)), (bd, k, c)
        if ic.V <= c["mode"] <= ic.D67:
            angles.add(ic.MODE_TO_ANGLE[c["mode"]] + 3 * c["delta"])
    assert len(angles) == 56


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_builders_every_availability_filter_type_and_class(harness, bd):
    """every availability class x both filt_types x both disable_edge_filter values x every input class, for every (mode, delta) and filter-intra mode at the sizes
    where the edge paths switch: w + h = 8, 12, 16, 20, 24, 32, 48 and above"""
    g = np.random.default_rng(200 + bd)
    for (w, h) in ((4, 4), (4, 8), (8, 8), (4, 16), (16, 8), (16, 16), (32, 16), (32, 64)):
        for avail in ic.AVAIL:
            for ft in (0, 1):
                for dis in (0, 1):
                    kind = ic.CLASSES[(ft + 2 * dis + ic.AVAIL.index(avail)) % 5]
                    md = [(m, d) for m in range(13) for d in (range(-3, 4) if ic.V <= m <= ic.D67 else (0,))]
                    for (m, d) in md:
                        c = ic.case(w, h, m, d, ic.FILTER_INTRA_OFF, avail, ft, dis, kind)
                        top, left = ic.case_inputs(g, c, bd)
                        assert np.array_equal(ref_build(harness, c, top, left, bd), ic.predict_case(c, top, left, bd)), (bd, c)
                    if w <= 32 and h <= 32 and ft == 0:
                        for fi in range(5):
                            c = ic.case(w, h, (ic.DC, ic.D203, ic.D45, ic.V, ic.PAETH)[fi], 0, fi, avail, ft, dis, kind)
                            top, left = ic.case_inputs(g, c, bd)
                            assert np.array_equal(ref_build(harness, c, top, left, bd), ic.predict_case(c, top, left, bd)), (bd, c)


def _edge(bd, values, lo):
    """(ctypes base array, pointer to entry 0, restatement Edge) of a prepared edge whose entries lo .. are `values`"""
    dt = np.uint16 if bd > 8 else np.uint8
    e = ic.Edge(bd, values, lo)
    a = e.a.astype(dt)
    return a, a.ctypes.data + e.org * a.itemsize, e


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_exported_directional_functions(harness, bd):
    """the six dr_prediction `_c` functions directly, every derivative the table holds, with and without upsampled edges (w + h <= 16)"""
    ref, g = harness.ref, np.random.default_rng(300 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    pre = "svt_av1_highbd_dr_prediction_z%d_c" if bd > 8 else "svt_av1_dr_prediction_z%d_c"
    tail = [bd] if bd > 8 else []
    for (w, h) in ((4, 4), (8, 4), (4, 8), (8, 8), (16, 4), (16, 16), (32, 8), (64, 64), (16, 64)):
        for up in ((0, 1) if w + h <= 16 else (0,)):
            for kind in ("random", "checker", "max"):
                n = ((w + h) << up) + 2
                va, vl = ic.make_samples(g, kind, n + 2, bd), ic.make_samples(g, kind, n + 2, bd)[::-1]
                aa, pa, ea = _edge(bd, va, -2)
                al, pl, el = _edge(bd, vl, -2)
                for ang in (a for a in range(1, 90) if ic.DR_DERIVATIVE[a]):
                    d = int(ic.DR_DERIVATIVE[ang])
                    dst = np.zeros((h, w), dt)
                    getattr(ref, pre % 1)(p(dst), w, w, h, pa, pl, up, d, 1, *tail)
                    assert np.array_equal(dst, ic.dr_z1(ea, w, h, up, d, bd)), (bd, w, h, up, ang)
                    getattr(ref, pre % 3)(p(dst), w, w, h, pa, pl, up, 1, d, *tail)
                    assert np.array_equal(dst, ic.dr_z3(el, w, h, up, d, bd)), (bd, w, h, up, ang)
                    d2 = int(ic.DR_DERIVATIVE[90 - ang])
                    if d2:
                        for upl in ((0, 1) if w + h <= 16 else (0,)):
                            want = ic.dr_z2(ea, el, w, h, up, upl, d, d2, bd)  # (first: it carries the C's assertion, which would end the process there)
                            getattr(ref, pre % 2)(p(dst), w, w, h, pa, pl, up, upl, d, d2, *tail)
                            assert np.array_equal(dst, want), (bd, w, h, up, upl, ang)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_exported_edge_functions_and_filter_intra(harness, bd):
    """edge filter (every strength, sizes 2 .. 129), upsampler (sizes 1 .. 16), both filter-intra predictors, a sample of the sized predictors"""
    ref, g = harness.ref, np.random.default_rng(400 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    for kind in ic.CLASSES:
        for sz in (2, 3, 5, 9, 17, 33, 65, 100, 129):
            for strength in range(4):
                a, pa, e = _edge(bd, ic.make_samples(g, kind, sz, bd), -1)
                (ref.svt_av1_filter_intra_edge_high_c if bd > 8 else ref.svt_av1_filter_intra_edge_c)(pa - a.itemsize, sz, strength)
                ic.filter_edge(e, -1, sz, strength, bd)
                assert np.array_equal(a, e.a), (bd, kind, sz, strength)
        for sz in range(1, 17):
            a, pa, e = _edge(bd, ic.make_samples(g, kind, sz + 1, bd), -1)
            if bd > 8:
                ref.svt_av1_upsample_intra_edge_high_c(pa, sz, bd)
            else:
                ref.svt_av1_upsample_intra_edge_c(pa, sz)
            ic.upsample_edge(e, sz, bd)
            assert np.array_equal(a, e.a), (bd, kind, sz)
        for tx, (w, h) in enumerate(ic.TX_SIZES):
            aa, pa, ea = _edge(bd, ic.make_samples(g, kind, w + 1, bd), -1)
            al, pl, el = _edge(bd, ic.make_samples(g, kind, h + 1, bd)[::-1], -1)
            dst = np.zeros((h, w), dt)
            if w <= 32 and h <= 32:
                for fm in range(5):
                    if bd > 8:
                        ref.svt_aom_highbd_filter_intra_predictor(p(dst), w, tx, pa, pl, fm, bd)
                    else:
                        ref.svt_av1_filter_intra_predictor_c(p(dst), w, tx, pa, pl, fm)
                    assert np.array_equal(dst, ic.filter_intra_pred(ea, el, w, h, fm, bd)), (bd, kind, w, h, fm)
            for mode, fn in ((ic.SMOOTH, ic.smooth_pred), (ic.SMOOTH_V, ic.smooth_v_pred), (ic.SMOOTH_H, ic.smooth_h_pred), (ic.PAETH, ic.paeth_pred), (ic.V, ic.v_pred),
                             (ic.H, ic.h_pred)):
                harness.harness_sized_predictor(mode, 1, 1, tx, p(dst), w, pa, pl, bd)
                assert np.array_equal(dst, fn(ea, el, w, h)), (bd, kind, w, h, mode)
            for hl in (0, 1):
                for ht in (0, 1):
                    harness.harness_sized_predictor(ic.DC, hl, ht, tx, p(dst), w, pa, pl, bd)
                    assert np.array_equal(dst, ic.dc_pred(ea, el, w, h, ht, hl, bd)), (bd, kind, w, h, hl, ht)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_exported_cfl_functions(harness, bd):
    """the CfL four and svt_subtract_average_c: every size of the table, luma all-max (where the int16_t narrowing is closest), the extreme alphas"""
    ref, g = harness.ref, np.random.default_rng(500 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    n = "hbd" if bd > 8 else "lbd"
    for (w, h) in ic.CFL_SIZES:
        for kind in ("random", "max", "zero", "checker"):
            luma = ic.make_samples(g, kind, 4 * w * h, bd).reshape(2 * h, 2 * w).astype(dt)
            q3 = np.full((h, ic.CFL_BUF_LINE), 0x5A5A, np.int16)
            getattr(ref, "svt_cfl_luma_subsampling_420_%s_c" % n)(p(luma), 2 * w, p(q3), 2 * w, 2 * h)
            want = ic.cfl_subsample_420(luma, w, h)
            assert np.array_equal(q3[:, :w], want) and np.all(q3[:, w:] == 0x5A5A), (bd, w, h, kind)
            ref.svt_subtract_average_c(p(q3), w, h, (w * h) >> 1, (w.bit_length() - 1) + (h.bit_length() - 1))
            ac = ic.cfl_subtract_average(want, w, h)
            assert np.array_equal(q3[:, :w], ac), (bd, w, h, kind)
            pred = ic.make_samples(g, "random", w * h, bd).reshape(h, w).astype(dt)
            for alpha in (-16, -1, 0, 1, 16):
                dst = np.zeros((h, w), dt)
                getattr(ref, "svt_cfl_predict_%s_c" % n)(p(q3), p(pred), w, p(dst), w, alpha, bd, w, h)
                assert np.array_equal(dst, ic.cfl_predict(ac, pred, alpha, bd, bd == 8)), (bd, w, h, kind, alpha)
    if bd == 8:  # the 8-bit form takes bit_depth as an argument too: clipped to 10 bits, then narrowed to uint8_t
        q3 = np.zeros((4, ic.CFL_BUF_LINE), np.int16)
        q3[:, :4] = 30000
        pred, dst = np.full((4, 4), 200, np.uint8), np.zeros((4, 4), np.uint8)
        ref.svt_cfl_predict_lbd_c(p(q3), p(pred), 4, p(dst), 4, 1, 10, 4, 4)
        assert np.array_equal(dst, ic.cfl_predict(q3[:, :4], pred, 1, 10, True))


def _golden_from_reference(h):
    out = {"seed": np.array([ic.GOLDEN_SEED], np.int64)}
    for i, (bd, c) in enumerate(ic.golden_cases()):
        top, left = ic.golden_inputs(i, bd, c)
        dt = np.uint16 if bd > 8 else np.uint8
        out["top_%d" % i], out["left_%d" % i] = top.astype(dt), left.astype(dt)
        out["out_%d" % i] = ref_build(h, c, top, left, bd).astype(dt)
    return out


def test_golden_file_is_what_the_reference_computes(harness):
    """tests/golden/intrapred.npz (what tests/test_intrapred.py compares the kernels with where no reference exists) == the reference's outputs, entry for entry"""
    now = _golden_from_reference(harness)
    if os.environ.get("SVT_INTRAPRED_WRITE_GOLDEN") == "1":
        np.savez_compressed(ic.GOLDEN_FILE, **now)
    assert os.path.getsize(ic.GOLDEN_FILE) < 256 * 1024
    gold = ic.load_golden()
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert gold[k].dtype == now[k].dtype and np.array_equal(gold[k], now[k]), k
    for i, (bd, c) in enumerate(ic.golden_cases()):
        assert np.array_equal(ic.predict_case(c, gold["top_%d" % i], gold["left_%d" % i], bd), gold["out_%d" % i]), (i, bd, c)
