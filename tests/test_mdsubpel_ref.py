"""tests/mdsubpel_common.py pinned on the reference (oracle/_ref/libsvtref.so after svt_aom_setup_rtcd_internal(0): every dispatch pointer is its `_c` function).
The primitives are called directly; the two searches go through tests/mdsubpel_ref_harness.c, compiled at test time, which includes the reference's headers where
they lie; the filter rows the feature uses are compared entry by entry with the tables in the reference's source text (static arrays).  CPU only; runs where the
reference's sources and the library exist, skipped elsewhere.  `SVT_MDSUBPEL_WRITE_GOLDEN=1` rewrites tests/golden/mdsubpel.npz from the reference's outputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mdsubpel_common as mc
from conftest import GOLDEN, REF_LIB, ROOT, p

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "mcomp.c")), reason="the reference's sources are not on this machine")
INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
GOLDEN_FILE = os.path.join(GOLDEN, "mdsubpel.npz")
PARAMS = ("start_r", "start_c", "ref_r", "ref_c", "cmin", "cmax", "rmin", "rmax", "allow_hp", "forced_stop", "iters_per_step", "pred_variance_th", "abs_th_mult",
          "round_dev_th", "skip_diag_refinement", "subpel_search_type", "bias_fp", "qp", "early_exit", "mv_cost_type", "error_per_bit", "early_exit_th", "mvp_th", "hp_mv_th",
          "best_mvp_err", "mvp_r", "mvp_c")
vp = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("mdsubpel") / "libmdsubpel_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "mdsubpel_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    assert h.harness_param_count() == len(PARAMS)
    h.harness_md_subpel.restype, h.harness_md_subpel.argtypes = None, [C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    h.harness_mv_limits.restype, h.harness_mv_limits.argtypes = None, [C.c_int] * 7 + [vp]
    h.ref = ref
    return h


def ref_primitive(ref, case):
    """(var, sse, sum, sad) of a primitive case from the reference's `_c` functions; sum is not returned by the C and is taken from var, sse"""
    pre, py, px, src, wsrc, mask = mc.primitive_inputs(case)
    W, H = mc.BW[case["bsize"]], mc.BH[case["bsize"]]
    name, stride = "%dx%d_c" % (W, H), pre.shape[1]
    at = pre.ctypes.data + py * stride + px
    sse = np.zeros(1, np.uint32)
    k = case["kind"]

    def fn(n, args):
        f = getattr(ref, n)
        f.restype, f.argtypes = C.c_uint32, args
        return f
    if k == mc.VAR:
        v = fn("svt_aom_variance" + name, [vp, C.c_int, vp, C.c_int, vp])(at, stride, p(src), W, p(sse))
    elif k == mc.SUBPIX:
        v = fn("svt_aom_sub_pixel_variance" + name, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp])(at, stride, case["xo"], case["yo"], p(src), W, p(sse))
    elif k == mc.UPSAMPLED:
        comp = np.zeros((H, W), np.uint8)
        f = ref.svt_aom_upsampled_pred_c
        f.restype, f.argtypes = None, [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int]
        f(None, None, 0, 0, None, p(comp), W, H, case["xo"], case["yo"], at, stride, case["taps"])
        assert np.array_equal(comp, mc.upsampled_pred(pre, py, px, W, H, case["xo"], case["yo"], case["taps"])), case
        v = fn("svt_aom_variance" + name, [vp, C.c_int, vp, C.c_int, vp])(p(comp), W, p(src), W, p(sse))
    elif k == mc.MSE:
        v = fn("svt_aom_mse16x16_c", [vp, C.c_int32, vp, C.c_int32, vp])(at, stride, p(src), W, p(sse))
        return v, int(sse[0]), None, 0
    elif k == mc.OBMC_SAD:
        return 0, 0, None, fn("svt_aom_obmc_sad" + name, [vp, C.c_int, vp, vp])(at, stride, p(wsrc), p(mask))
    elif k == mc.OBMC_VAR:
        v = fn("svt_aom_obmc_variance" + name, [vp, C.c_int, vp, vp, vp])(at, stride, p(wsrc), p(mask), p(sse))
    else:
        v = fn("svt_aom_obmc_sub_pixel_variance" + name, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp])(at, stride, case["xo"], case["yo"], p(wsrc), p(mask), p(sse))
    return v, int(sse[0]), None, 0


def ref_search(h, case, use_ctx):
    src, refp, ry, rx = mc.search_inputs(case)
    c = dict(mc.DEFAULTS)
    c.update(case)
    lims = c["lims"] if c["lims"] is not None else mc.WIDE_LIMITS
    flat = dict(c, start_r=c["start"][0], start_c=c["start"][1], ref_r=c["ref_mv"][0], ref_c=c["ref_mv"][1], cmin=lims[0], cmax=lims[1], rmin=lims[2], rmax=lims[3],
                mvp_r=c["best_mvp"][0], mvp_c=c["best_mvp"][1])
    ip = np.array([flat[k] for k in PARAMS], np.int32)
    out = np.zeros(6, np.int32)
    src = np.ascontiguousarray(src)
    joint = m0 = m1 = None
    if c["cost_table"] >= 0 or c["mv_cost_type"] == 0:
        # (svt_mv_err_cost tests `mvcost`, an array member that is never NULL, and then reads mvcost[0]: the C cannot run MV_COST_ENTROPY without tables.  "No table"
        #  is cost 0 in the interface; here the C gets tables of zeros, which cost 0 as well)
        joint, comp = mc.cost_tables()[c["cost_table"]] if c["cost_table"] >= 0 else (np.zeros(4, np.int32), np.zeros((2, mc.MV_VALS), np.int32))
        comp = np.ascontiguousarray(comp)
        m0, m1 = comp.ctypes.data + 4 * mc.MV_MAX, comp.ctypes.data + 4 * (mc.MV_VALS + mc.MV_MAX)
        joint = p(joint)
    h.harness_md_subpel(c["method"], use_ctx, p(src), src.shape[1], refp.ctypes.data + ry * refp.shape[1] + rx, refp.shape[1], c["bsize"], p(ip), joint, m0, m1, p(out))
    vals = out.astype(np.int64)
    vals[[2, 4, 5]] &= 0xFFFFFFFF
    return dict(zip(mc.RESULT_FIELDS, (int(v) for v in vals)))


def _table(text, name):
    body = re.search(name + r"\[SUBPEL_SHIFTS\]\)\s*=\s*\{(.*?)\};", text, re.S).group(1)
    rows = [[int(v) for v in re.findall(r"-?\d+", r)] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 16 and all(len(r) == 8 for r in rows), name
    return rows


def test_filter_rows_every_entry():
    text = open(os.path.join(SRC, "Lib", "C_DEFAULT", "variance.c")).read()
    for taps, name in mc.UP_TABLE_NAMES.items():
        rows = _table(text, name)
        for q in range(8):  # svt_aom_upsampled_pred_c asks for phase q3 << 1
            assert mc.UP_ROWS[taps][q] == rows[2 * q], (name, q)
            assert sum(rows[2 * q]) == 128 and (q == 0 or all(-128 <= v <= 127 for v in rows[2 * q]))
    # USE_2_TAPS / 4 / 8 are 1 / 2 / 3 and select these three tables
    assert re.search(r"USE_2_TAPS_ORIG = 0,[^\n]*\n\s*USE_2_TAPS,\s*\n\s*USE_4_TAPS,\s*\n\s*USE_8_TAPS,", open(os.path.join(SRC, "Lib", "Codec", "definitions.h")).read())
    assert re.search(r"case USE_2_TAPS: return get_4tap_interp_filter_params\(BILINEAR\);\s*case USE_4_TAPS: return get_4tap_interp_filter_params\(EIGHTTAP_REGULAR\);\s*"
                     r"case USE_8_TAPS: return &av1_interp_filter_params_list\[EIGHTTAP_REGULAR\];", text)
    assert re.search(r"\{\(const int16_t \*\)av1_sub_pel_filters_4, SUBPEL_TAPS, SUBPEL_SHIFTS, EIGHTTAP_REGULAR\},\s*\{[^}]*4smooth[^}]*\},\s*\{[^}]*\},\s*"
                     r"\{\(const int16_t \*\)av1_bilinear_filters, SUBPEL_TAPS, SUBPEL_SHIFTS, BILINEAR\}", text)
    ftext = open(os.path.join(SRC, "Lib", "Codec", "filter.h")).read()
    body = re.search(r"bilinear_filters_2t\[BIL_SUBPEL_SHIFTS\]\[2\]\s*=\s*\{(.*?)\};", ftext, re.S).group(1)
    assert [tuple(int(v) for v in re.findall(r"\d+", r)) for r in re.findall(r"\{([^{}]*)\}", body)] == mc.BILINEAR_2T


def test_constants(ref):
    offs = (C.c_uint8 * 128).in_dll(ref, "svt_aom_eb_av1_var_offs")
    assert list(offs) == [128] * 128
    text = open(os.path.join(SRC, "Lib", "Codec", "cabac_context_model.h")).read()
    assert re.search(r"#define MV_CLASSES 11\b", text) and re.search(r"#define CLASS0_BITS 1\b", text) and re.search(r"#define MV_IN_USE_BITS 14\b", text)
    assert re.search(r"#define MAX_MVSEARCH_STEPS 11\b", open(os.path.join(SRC, "Lib", "Codec", "av1me.h")).read())


def test_primitives_over_the_case_list(harness):
    cases = mc.primitive_cases()
    for c in cases:
        got, want = ref_primitive(harness.ref, c), mc.run_primitive(c)
        assert all(g is None or g == w for g, w in zip(got, want)), (c, got, want)


@pytest.mark.parametrize("use_ctx", [0, 1])
def test_searches_over_the_case_list(harness, use_ctx):
    for c in mc.search_cases():
        want = mc.run_search(c)
        got = ref_search(harness, c, use_ctx)
        assert got == {f: want[f] for f in mc.RESULT_FIELDS}, (use_ctx, c, got, want)


def test_mv_limits(harness):
    g = np.random.default_rng(3)
    lim = np.zeros(4, np.int32)
    for _ in range(500):
        b = int(g.integers(0, 22))
        mi_rows, mi_cols = int(g.integers(8, 600)), int(g.integers(8, 1000))
        mi_row, mi_col = int(g.integers(0, mi_rows)), int(g.integers(0, mi_cols))
        r = (int(g.integers(-16384, 16384)), int(g.integers(-16384, 16384))) if g.integers(0, 4) else (int(g.integers(-40, 40)), int(g.integers(-40, 40)))
        harness.harness_mv_limits(mi_row, mi_col, b, mi_rows, mi_cols, r[0], r[1], p(lim))
        assert tuple(lim.tolist()) == mc.mv_limits(mi_row, mi_col, b, mi_rows, mi_cols, r)


def test_golden_file_is_what_the_reference_computes(harness):
    pc, sc = mc.primitive_cases(), mc.search_cases()
    prim = []
    for c in pc:
        got, want = ref_primitive(harness.ref, c), mc.run_primitive(c)
        prim.append([w if g is None else g for g, w in zip(got, want)])  # (the C does not return the sum: it is the restatement's, pinned through var)
    now = dict(prim_seeds=np.array([c["seed"] for c in pc], np.int64), prim_out=np.array(prim, np.int64), search_seeds=np.array([c["seed"] for c in sc], np.int64),
               search_out=np.array([[ref_search(harness, c, 1)[f] for f in mc.RESULT_FIELDS] for c in sc], np.int64))
    if os.environ.get("SVT_MDSUBPEL_WRITE_GOLDEN") == "1":
        np.savez_compressed(GOLDEN_FILE, **now)
    gold = np.load(GOLDEN_FILE)
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert np.array_equal(gold[k], now[k]), k
