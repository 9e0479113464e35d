"""Pins tests/picstats_common.py (the numpy restatement the kernels of csrc/picstats.hip are checked against) and the library's host-built boost table against the
REAL reference.  CPU only; needs the reference's headers and oracle/_ref/libsvtref.so, so it runs in the build container only.

tests/picstats_ref_harness.c is compiled at test time into tmp_path: zeroed control sets with only the fields filled that the two exported callers read, so the
static functions (compute_block_mean_compute_variance, av1_get_deltaq_sb_variance_boost, the histogram driver) run as the encoder runs them.  The outputs of the
harness for the inputs of tests/test_picstats.py are what tests/golden/picstats.npz holds; `SVT_PICSTATS_WRITE_GOLDEN=1` rewrites the file from the harness."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import picstats_cases as cases
import picstats_common as pc
from conftest import EMU_LIB, PKG_DIR, REF_LIB, ROOT, load_pkg, p

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "pic_analysis_process.c")), reason="the reference's sources are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
BIT_DEPTHS = (8, 10, 12)


class Plane(C.Structure):
    _fields_ = [("buffer", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint32), ("org_y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


def _plane(a, org_x, org_y, w, h):
    return Plane(a.ctypes.data, a.shape[1], org_x, org_y, w, h)


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("picstats") / "libpicstats_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "picstats_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    h.harness_picture_statistics.restype = C.c_int
    h.harness_picture_statistics.argtypes = [C.POINTER(Plane), C.POINTER(Plane)] + [C.c_int] * 5 + [C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 5
    h.harness_variance_adjust_qp.restype = C.c_int
    h.harness_variance_adjust_qp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int] * 5
    ref.svt_av1_convert_qindex_to_q_fp8.restype, ref.svt_av1_convert_qindex_to_q_fp8.argtypes = C.c_int32, [C.c_int32, C.c_int]
    ref.svt_av1_compute_qdelta_fp.restype, ref.svt_av1_compute_qdelta_fp.argtypes = C.c_int32, [C.c_int32, C.c_int32, C.c_int]
    h.ref = ref
    return h


def q_table(ref, bd):
    return np.array([ref.svt_av1_convert_qindex_to_q_fp8(i, bd) for i in range(256)], np.int32)


def ref_variance(h, padded, org_x, org_y, w, hgt, prec, sub64, init=None):
    n_sb = ((w + 63) // 64) * ((hgt + 63) // 64)
    var = np.zeros((n_sb, 85), np.uint16) if init is None else init.copy()
    avg, luma, hist, ai = np.zeros(1, np.uint16), np.zeros(1, np.uint64), np.zeros(256, np.uint32), np.zeros(1, np.uint64)
    pl = _plane(padded, org_x, org_y, w, hgt)
    # the reference writes the sub-64 entries when enable_adaptive_quantization == 1 || variance_octile: both ways of switching them on are used
    aq, octile = ((1, 0) if prec == pc.PREC_FULL else (0, 6)) if sub64 else (0, 0)
    assert h.harness_picture_statistics(C.byref(pl), C.byref(pl), prec, aq, octile, 0, 1, 1, 1, 0, p(var), p(avg), p(hist), p(ai), p(luma)) == 0
    return var, int(avg[0])


def ref_histogram(h, padded, org_x, org_y, w, hgt, rw, rh, decim):
    hist, ai, luma = np.zeros((rw, rh, 256), np.uint32), np.zeros((rw, rh), np.uint64), np.zeros(1, np.uint64)
    var, avg = np.zeros((((w + 63) // 64) * ((hgt + 63) // 64), 85), np.uint16), np.zeros(1, np.uint16)
    pl = _plane(padded, org_x, org_y, w, hgt)
    assert h.harness_picture_statistics(C.byref(pl), C.byref(pl), pc.PREC_SUB, 0, 0, 1, 0, rw, rh, int(decim == 1), p(var), p(avg), p(hist), p(ai), p(luma)) == 0
    assert ai.max() <= 255
    return hist, ai.astype(np.uint8), int(luma[0])


def ref_boost(h, var, qin, base_q_idx, strength, octile, curve, bd):
    q = qin.copy()
    nb = h.harness_variance_adjust_qp(p(np.ascontiguousarray(var)), p(q), len(q), base_q_idx, strength, octile, curve, bd)
    return q, nb


def test_leaf_functions_and_qdelta(harness):
    """the four `_c` leaf functions behind the dispatch pointers of aom_dsp_rtcd.c:516-519, and svt_av1_compute_qdelta_fp, against the restatement"""
    ref = harness.ref
    U64 = C.c_uint64
    for n in ("svt_compute_mean_c", "svt_compute_mean_squared_values_c"):
        getattr(ref, n).restype, getattr(ref, n).argtypes = U64, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    ref.svt_compute_sub_mean_8x8_c.restype, ref.svt_compute_sub_mean_8x8_c.argtypes = U64, [C.c_void_p, C.c_uint16]
    ref.svt_compute_interm_var_four8x8_c.restype, ref.svt_compute_interm_var_four8x8_c.argtypes = None, [C.c_void_p, C.c_uint16, C.c_void_p, C.c_void_p]
    g = np.random.default_rng(3)
    for kind in cases.CLASSES:
        a = cases.luma(kind, 11, 45, g)
        blk = np.ascontiguousarray(a[2:10, 5:37])
        mf, qf = pc.block_means_8x8(blk, pc.PREC_FULL)
        ms, qs = pc.block_means_8x8(blk, pc.PREC_SUB)
        at = a.ctypes.data + 2 * 45 + 5
        m4, q4 = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        ref.svt_compute_interm_var_four8x8_c(at, 45, p(m4), p(q4))
        assert np.array_equal(m4, ms[0]) and np.array_equal(q4, qs[0]), kind
        for k in range(4):
            assert ref.svt_compute_mean_c(at + 8 * k, 45, 8, 8) == int(mf[0, k]) and ref.svt_compute_mean_squared_values_c(at + 8 * k, 45, 8, 8) == int(qf[0, k]), kind
            assert ref.svt_compute_sub_mean_8x8_c(at + 8 * k, 45) == int(ms[0, k]), kind
    for bd in BIT_DEPTHS:
        q = q_table(ref, bd)
        assert np.all(np.diff(q) >= 0)
        for a in list(range(0, int(q[-1]) + 300, 97)) + [int(q[1]), int(q[128]), int(q[254]), int(q[255])]:
            for b in (0, a // 8, a // 2, a - 1, a, a + 1, int(q[255]) + 5):
                assert ref.svt_av1_compute_qdelta_fp(a, b, bd) == pc.compute_qdelta_fp(q, a, b), (bd, a, b)


def test_variance_restatement_is_the_reference(harness):
    """compute_picture_spatial_statistics through svt_aom_gathering_picture_statistics: every picture, class, precision; the sub-64 flag on and off"""
    for pi, (w, hgt) in enumerate(cases.PICTURES):
        for ci, kind in enumerate(cases.CLASSES):
            padded, _ = cases.padded_picture(kind, w, hgt, cases.variance_seed(pi, ci))
            for prec in (pc.PREC_FULL, pc.PREC_SUB):
                for sub64 in (True, False):
                    init = np.full(((((w + 63) // 64) * ((hgt + 63) // 64)), 85), 0xabcd, np.uint16)
                    got, gavg = ref_variance(harness, padded, cases.ORG_X, cases.ORG_Y, w, hgt, prec, sub64, init)
                    want, wavg = pc.picture_variance(padded, cases.ORG_X, cases.ORG_Y, w, hgt, prec, sub64, init)
                    assert np.array_equal(got, want) and gavg == wavg, (w, hgt, kind, prec, sub64)
                    if not sub64:
                        assert np.all(got[:, 1:] == 0xabcd)
    # the classes are not degenerate: random content has large 8x8 variances, flat content none
    v = pc.picture_variance(cases.padded_picture("random", 192, 128, 1)[0], cases.ORG_X, cases.ORG_Y, 192, 128, pc.PREC_SUB)[0]
    assert v[:, pc.V8:].min() > 1000


def test_boost_restatement_is_the_reference(harness):
    """svt_variance_adjust_qp on the variance tables of tests/test_picstats.py, plus random tables and every (strength, octile, curve) at a few base_q_idx"""
    ref = harness.ref
    qt = {bd: q_table(ref, bd) for bd in BIT_DEPTHS}
    for i, (n_sb, kind, mode, bq, st, oc, cv, bd) in enumerate(cases.BOOST_CASES):
        var = cases.boost_variance(n_sb, kind, cases.boost_seed(i))
        qin = cases.boost_qindex_in(n_sb, mode, cases.boost_seed(i))
        got, gnb = ref_boost(harness, var, qin, bq, st, oc, cv, bd)
        want, wnb, _, _, _ = pc.variance_boost(var, qin, bq, st, oc, cv, qt[bd])
        assert np.array_equal(got, want) and gnb == wnb, cases.BOOST_CASES[i]
    g = np.random.default_rng(11)
    for st in (1, 2, 3, 4):
        for oc in range(1, 9):
            for cv in (0, 1, 2):
                bq, bd = int(g.integers(1, 256)), BIT_DEPTHS[int(g.integers(3))]
                var = (g.integers(0, 2, (40, 85)) * g.integers(0, 65536, (40, 85)) + g.integers(0, 40, (40, 85))).clip(0, 65535).astype(np.uint16)
                qin = g.integers(0, 256, 40).astype(np.uint8)
                got, gnb = ref_boost(harness, var, qin, bq, st, oc, cv, bd)
                want, wnb, _, _, _ = pc.variance_boost(var, qin, bq, st, oc, cv, qt[bd])
                assert np.array_equal(got, want) and gnb == wnb, (st, oc, cv, bq, bd)


def test_histogram_restatement_is_the_reference(harness):
    for i, (w, hgt, rw, rh, _) in enumerate(cases.HIST_CASES):
        padded, _, pic = cases.hist_plane(i)
        for decim in (1, 4):
            gh, ga, gl = ref_histogram(harness, padded, cases.HIST_ORG_X, cases.HIST_ORG_Y, w, hgt, rw, rh, decim)
            wh, wa, wl = pc.picture_histogram(pic, rw, rh, decim)
            assert np.array_equal(gh, wh) and np.array_equal(ga, wa) and gl == wl, (cases.HIST_CASES[i], decim)


def _golden_from_harness(harness):
    out = {"seed": np.array([cases.SEED], np.int64)}
    for bd in BIT_DEPTHS:
        out["q_fp8_%d" % bd] = q_table(harness.ref, bd)
    for pi, (w, hgt) in enumerate(cases.PICTURES):
        for ci, kind in enumerate(cases.CLASSES):
            padded, _ = cases.padded_picture(kind, w, hgt, cases.variance_seed(pi, ci))
            for prec in (pc.PREC_FULL, pc.PREC_SUB):
                var, avg = ref_variance(harness, padded, cases.ORG_X, cases.ORG_Y, w, hgt, prec, True)
                out["var_%d_%d_%d" % (pi, ci, prec)] = var
                out["avg_%d_%d_%d" % (pi, ci, prec)] = np.array([avg], np.uint16)
    for i, (n_sb, kind, mode, bq, st, oc, cv, bd) in enumerate(cases.BOOST_CASES):
        var = cases.boost_variance(n_sb, kind, cases.boost_seed(i))
        q, nb = ref_boost(harness, var, cases.boost_qindex_in(n_sb, mode, cases.boost_seed(i)), bq, st, oc, cv, bd)
        out["boost_q_%d" % i], out["boost_base_%d" % i] = q, np.array([nb], np.int32)
    for i, (w, hgt, rw, rh, _) in enumerate(cases.HIST_CASES):
        padded, _, _ = cases.hist_plane(i)
        for decim in (1, 4):
            gh, ga, gl = ref_histogram(harness, padded, cases.HIST_ORG_X, cases.HIST_ORG_Y, w, hgt, rw, rh, decim)
            out["hist_%d_%d" % (i, decim)], out["hist_avg_%d_%d" % (i, decim)], out["hist_luma_%d_%d" % (i, decim)] = gh, ga, np.array([gl], np.uint64)
    return out


def test_golden_file_is_what_the_reference_computes(harness):
    """tests/golden/picstats.npz (what tests/test_picstats.py compares the kernels with where no reference exists) == the harness's outputs, entry for entry"""
    now = _golden_from_harness(harness)
    if os.environ.get("SVT_PICSTATS_WRITE_GOLDEN") == "1":
        np.savez_compressed(cases.GOLDEN_FILE, **now)
    assert os.path.getsize(cases.GOLDEN_FILE) < 256 * 1024
    gold = cases.load_golden()
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert gold[k].dtype == now[k].dtype and np.array_equal(gold[k], now[k]), k


# ---- (c) the host-built boost table ---------------------------------------------------------------------------------------------------
def test_boost_table_is_the_reference_for_every_variance(harness):
    """For every blended variance 0 .. 65535 and base_q_idx in {1, 40, 128, 255}, every strength, every curve, bit depth 8 and 10: the table the library evaluates on the
    host -- in the emulator build (g++) and in the product (hipcc's host pass), neither touches a device for it -- == av1_get_deltaq_sb_variance_boost.  The reference's
    value is read through svt_variance_adjust_qp, one call per variance (harness_boost_of_every_variance)."""
    pkg = load_pkg()
    libs = [pkg.bind(C.CDLL(EMU_LIB)), pkg.bind(C.CDLL(os.path.join(PKG_DIR, "libsvtav1_hip.so")))]
    harness.harness_boost_of_every_variance.restype, harness.harness_boost_of_every_variance.argtypes = C.c_int, [C.c_int] * 5 + [C.c_void_p]
    distinct = 0
    for bd in (8, 10):
        q = q_table(harness.ref, bd)
        for bq in (1, 40, 128, 255):
            for st in (1, 2, 3, 4):
                for cv in (0, 1, 2):
                    want = np.full(65536, -1, np.int16)
                    assert harness.harness_boost_of_every_variance(bq, st, 6, cv, bd, p(want)) == 0
                    for lib in libs:
                        got = np.full(65536, -2, np.int16)
                        assert lib.svt_hip_variance_boost_table(bq, st, cv, bd, p(q), p(got)) == 0
                        assert np.array_equal(got, want), (bd, bq, st, cv, np.flatnonzero(got != want)[:8])
                    assert want.min() >= 0 and want[0] == want[1]
                    distinct += len(np.unique(want))
    assert distinct > 96 * 4  # the tables are not all-zero
