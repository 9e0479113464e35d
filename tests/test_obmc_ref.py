"""tests/obmc_common.py pinned on the reference (oracle/_ref/libsvtref.so after svt_aom_setup_rtcd_internal(0): every dispatch pointer is its `_c` function) through
tests/obmc_ref_harness.c, compiled at test time, which includes the reference's headers where they lie.  Three levels: the two target-weighted callbacks under the
restated driver lines; svt_av1_obmc_full_pixel_search and svt_av1_find_best_obmc_sub_pixel_tree_up called directly; single_motion_search whole (its limits, its
refine_level mapping, its sad / error per bit, its rate).  libsvtref.so is built with the reference's asserts live, so every case here is one the reference runs to
completion.  CPU only; runs where the reference's sources and the library exist, skipped elsewhere.  `SVT_OBMC_WRITE_GOLDEN=1` rewrites tests/golden/obmc.npz from the
reference's outputs."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import mdsubpel_common as mc
import obmc_common as oc
from conftest import GOLDEN, REF_LIB, ROOT, p

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "av1me.c")), reason="the reference's sources are not on this machine")
INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
GOLDEN_FILE = os.path.join(GOLDEN, "obmc.npz")
PARAMS = ("best_r", "best_c", "ref_r", "ref_c", "cmin", "cmax", "rmin", "rmax", "sad_per_bit", "error_per_bit", "approx", "fpel_range", "fpel_diag", "allow_hp",
          "forced_stop", "iters_per_step", "subpel_search_type", "do_full", "do_frac", "mi_row", "mi_col", "mi_rows", "mi_cols", "qidx", "full_lambda", "refine_level")
DIRECT_FIELDS = ("mv_row", "mv_col", "fp_row", "fp_col", "thissme", "besterr", "distortion", "sse1", "rate_mv")
vp = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("obmc") / "libobmc_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "obmc_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    assert h.harness_param_count() == len(PARAMS)
    h.harness_obmc_wsrc.restype, h.harness_obmc_wsrc.argtypes = None, [C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    h.harness_obmc_search.restype, h.harness_obmc_search.argtypes = None, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    h.harness_single_motion_search.restype, h.harness_single_motion_search.argtypes = None, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    h.ref = ref
    return h


def ref_wsrc(h, case):
    src, above, left = oc.wsrc_inputs(case)
    W, H = mc.BW[case["bsize"]], mc.BH[case["bsize"]]
    wsrc, mask = np.zeros(W * H, np.int32), np.zeros(W * H, np.int32)
    a, l = np.array(case["above"], np.int32).reshape(-1), np.array(case["left"], np.int32).reshape(-1)
    h.harness_obmc_wsrc(case["bsize"], p(src), src.shape[1], p(above), above.shape[1], p(left), left.shape[1], case["up"], case["lf"], len(case["above"]), p(a),
                        len(case["left"]), p(l), p(wsrc), p(mask))
    return wsrc, mask


def flat_params(c, **more):
    f = dict(best_r=c["best_pred_mv"][0], best_c=c["best_pred_mv"][1], ref_r=c["ref_mv"][0], ref_c=c["ref_mv"][1], cmin=c["lims"][0], cmax=c["lims"][1], rmin=c["lims"][2],
             rmax=c["lims"][3], mi_row=0, mi_col=0, mi_rows=0, mi_cols=0, qidx=0, full_lambda=0, refine_level=0)
    f.update({k: c[k] for k in PARAMS if k in c})
    f.update(more)
    return np.array([f[k] for k in PARAMS], np.int32)


def tables_for(ct):
    """(joint, comp): a case without a table gives the C tables of zeros -- mvsad_err_cost and svt_av1_mv_bit_cost read theirs unconditionally, and zeros cost 0,
    which is what the interface defines for "no table" """
    joint, comp = mc.cost_tables()[ct] if ct >= 0 else (np.zeros(4, np.int32), np.zeros((2, mc.MV_VALS), np.int32))
    return np.ascontiguousarray(joint), np.ascontiguousarray(comp)


def ref_search(h, case):
    refp, ry, rx, _, _, _ = oc.search_inputs(case)
    wsrc, mask = oc.search_target(case)
    joint, comp = tables_for(case["cost_table"])
    out = np.zeros(9, np.int32)
    h.harness_obmc_search(refp.ctypes.data + ry * refp.shape[1] + rx, refp.shape[1], case["bsize"], p(wsrc), p(mask), p(flat_params(case)), p(joint),
                          comp.ctypes.data + 4 * mc.MV_MAX, comp.ctypes.data + 4 * (mc.MV_VALS + mc.MV_MAX), p(out))
    vals = out.astype(np.int64)
    vals[[5, 7]] &= 0xFFFFFFFF
    return dict(zip(DIRECT_FIELDS, (int(v) for v in vals)))


def test_obmc_masks_every_entry(ref):
    f = ref.svt_av1_get_obmc_mask
    f.restype, f.argtypes = C.POINTER(C.c_uint8), [C.c_int]
    for n, row in oc.OBMC_MASK.items():
        assert [f(n)[k] for k in range(n)] == row, n
    text = open(os.path.join(SRC, "Lib", "Codec", "mode_decision.c")).read()  # (the weight is private to the file; the harness restates it)
    assert re.search(r"#define MV_COST_WEIGHT 108\b", text)


def test_target_weighted_pred_over_the_case_list(harness):
    for c in oc.wsrc_cases():
        got, want = ref_wsrc(harness, c), oc.run_wsrc(c)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), c


def test_search_targets_are_the_references(harness):
    """the (wsrc, mask) the search cases use, from the reference's callbacks"""
    for c in oc.search_cases():
        src, above, left = oc.search_inputs(c)[3:]
        W, H = mc.BW[c["bsize"]], mc.BH[c["bsize"]]
        wsrc, mask = np.zeros(W * H, np.int32), np.zeros(W * H, np.int32)
        a, l = np.array(c["above"], np.int32).reshape(-1), np.array(c["left"], np.int32).reshape(-1)
        harness.harness_obmc_wsrc(c["bsize"], p(src), src.shape[1], p(above), above.shape[1], p(left), left.shape[1], c["up"], c["lf"], len(c["above"]), p(a), len(c["left"]),
                                  p(l), p(wsrc), p(mask))
        want = oc.search_target(c)
        assert np.array_equal(wsrc, want[0]) and np.array_equal(mask, want[1]), c


def test_the_two_search_functions_over_the_case_list(harness):
    for c in oc.search_cases():
        want = oc.run_search(c)
        got = ref_search(harness, c)
        assert got == {f: want[f] for f in DIRECT_FIELDS}, (c, got, want)


@pytest.mark.parametrize("refine_level", [0, 1, 2, 3, 4])
def test_single_motion_search_whole(harness, refine_level):
    """the driver: mi position -> limits, refine_level -> flags, base_q_idx -> sad per bit, lambda -> error per bit, the rate; forced_stop 0, two iterations, 8 taps"""
    picks = [c for c in oc.search_cases() if c["lims"] == oc.WIDE_LIMITS and c["content"] == "shift" and c["bsize"] in (3, 6, 9, 12)][:10]
    assert len(picks) == 10
    for n, c in enumerate(picks):
        refp, ry, rx, _, _, _ = oc.search_inputs(c)
        wsrc, mask = oc.search_target(c)
        ct = c["cost_table"]
        joint, comp = tables_for(ct)
        mi_rows, mi_cols = 135 + n, 240 - n
        # positions at and near the picture's corners: the window is what keeps the start vector's clamp and the candidates' range checks busy
        mi_row, mi_col = [(0, 0), (0, mi_cols - 2), (mi_rows - 2, 0), (mi_rows - 2, mi_cols - 2), (40, 70)][n % 5]
        full_lambda = (0, 30, 7000, 52000)[n % 4]
        ip = flat_params(c, mi_row=mi_row, mi_col=mi_col, mi_rows=mi_rows, mi_cols=mi_cols, qidx=(20 * n + 5) % 256, full_lambda=full_lambda, refine_level=refine_level,
                         allow_hp=n % 3 != 0)
        out = np.zeros(9, np.int32)
        harness.harness_single_motion_search(refp.ctypes.data + ry * refp.shape[1] + rx, refp.shape[1], c["bsize"], p(wsrc), p(mask), p(ip), p(joint), p(comp), p(out))
        lims = oc.obmc_mv_limits(mi_row, mi_col, c["bsize"], mi_rows, mi_cols)
        assert tuple(out[5:9].tolist()) == lims
        assert int(out[4]) == max(full_lambda >> 6, 1)  # RD_EPB_SHIFT
        do_full, do_frac = oc.refine_flags(refine_level)
        params = {k: v for k, v in c.items() if k in oc.DEFAULTS}
        params.update(lims=lims, do_full=do_full, do_frac=do_frac, sad_per_bit=int(out[3]), error_per_bit=int(out[4]), allow_hp=int(n % 3 != 0), forced_stop=0,
                      iters_per_step=2, subpel_search_type=3)
        want = oc.obmc_search(refp, ry, rx, wsrc, mask, params, (joint, comp))
        assert (int(out[0]), int(out[1]), int(out[2])) == (want["mv_row"], want["mv_col"], want["rate_mv"]), (refine_level, c, out, want)


def test_refine_levels_outside_the_switch(harness):
    """a level the switch does not name leaves both flags off: the vector is best_pred_mv >> 3 << 3"""
    c = oc.search_cases()[0]
    refp, ry, rx, _, _, _ = oc.search_inputs(c)
    wsrc, mask = oc.search_target(c)
    joint, comp = tables_for(0)
    out = np.zeros(9, np.int32)
    ip = flat_params(c, best_r=13, best_c=-11, mi_row=8, mi_col=8, mi_rows=100, mi_cols=100, qidx=60, full_lambda=9000, refine_level=5)
    harness.harness_single_motion_search(refp.ctypes.data + ry * refp.shape[1] + rx, refp.shape[1], c["bsize"], p(wsrc), p(mask), p(ip), p(joint), p(comp), p(out))
    assert oc.refine_flags(5) == (0, 0) and (int(out[0]), int(out[1])) == (8, -16)


def digest(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def golden_now(h):
    wc, sc = oc.wsrc_cases(), oc.search_cases()
    now = dict(wsrc_seeds=np.array([c["seed"] for c in wc], np.int64), wsrc_bsize=np.array([c["bsize"] for c in wc], np.int64),
               search_seeds=np.array([c["seed"] for c in sc], np.int64), search_bsize=np.array([c["bsize"] for c in sc], np.int64),
               search_out=np.array([[ref_search(h, c)[f] for f in DIRECT_FIELDS] for c in sc], np.int64))
    crc = []
    for k, c in enumerate(wc):
        w, m = ref_wsrc(h, c)
        crc.append([digest(w), digest(m)])
        if w.size <= 1024:  # the arrays themselves up to 32x32; the larger ones as their CRC-32 only (the file stays small)
            now["wsrc_%d" % k], now["mask_%d" % k] = w, m
    now["wsrc_crc"] = np.array(crc, np.int64)
    return now


def test_golden_file_is_what_the_reference_computes(harness):
    now = golden_now(harness)
    if os.environ.get("SVT_OBMC_WRITE_GOLDEN") == "1":
        np.savez_compressed(GOLDEN_FILE, **now)
    gold = np.load(GOLDEN_FILE)
    assert sorted(gold.files) == sorted(now) and os.path.getsize(GOLDEN_FILE) < 100 * 1024
    for k in now:
        assert np.array_equal(gold[k], now[k]), k
