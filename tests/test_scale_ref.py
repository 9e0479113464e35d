"""tests/scale_common.py pinned on the reference (oracle/_ref/libsvtref.so: its `_c` functions called directly).  The position arithmetic and the upscale go through
tests/scale_ref_harness.c, compiled at test time, which includes the reference's sources where they lie; every table entry is compared with the library's data symbol,
or with the source text where the table is static.  CPU only; runs where the reference's sources and the library exist, skipped elsewhere.
`SVT_SCALE_WRITE_GOLDEN=1` rewrites tests/golden/scale.npz from the reference's outputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scale_common as sc
from conftest import REF_LIB, ROOT, rng

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "super_res.c")), reason="the reference's sources are not on this machine")
INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
vp = C.c_void_p
BIT_DEPTHS = (8, 10, 12)


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("scale") / "libscale_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "scale_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    h.harness_subpel_params.restype, h.harness_subpel_params.argtypes = None, [C.c_int] * 11 + [vp]
    h.harness_scale_value.restype, h.harness_scale_value.argtypes = None, [C.c_int] * 5 + [vp]
    h.harness_upscale.restype, h.harness_upscale.argtypes = None, [vp, C.c_int, vp, C.c_int] + [C.c_int] * 9 + [vp]
    h.ref = ref
    return h


# ---- 1. position arithmetic -------------------------------------------------------------------------------------------------------------------------
PAIRS = [(64, 32, 2048), (64, 57, 1150), (64, 36, 1820), (64, 48, 1365), (32, 64, 512), (16, 256, 64), (72, 41, 1798), (1920, 1080, 1820)]  # reference, current, step


def test_scale_factors_and_scale_value(harness):
    out = np.zeros(6, np.int32)
    for (other, this, step) in PAIRS:
        for (oh, th) in ((other, this), (this, this)):  # scaled both ways; scaled in x only
            sf = sc.setup_scale_factors(other, oh, this, th)
            assert sf[2] == step
            for val in (0, 1, -1, 15, 16, 1000, -1000, 30000, -30000, 123457, -123457):
                harness.harness_scale_value(other, oh, this, th, val, out.ctypes.data)
                assert tuple(out[:4]) == sf, (other, this)
                assert out[4] == sc.scale_value(val, sf[0], sc.is_scaled(sf)) and out[5] == sc.scale_value(val, sf[1], sc.is_scaled(sf)), (other, this, val)
    for (other, this) in ((65, 32), (16, 257), (64, 31)):  # outside 2:1 .. 1:16
        assert sc.setup_scale_factors(other, other, this, this) is None
        harness.harness_scale_value(other, other, this, this, 0, out.ctypes.data)
        assert out[0] == -1 and out[1] == -1
    sf = sc.setup_scale_factors(64, 64, 64, 64)
    harness.harness_scale_value(64, 64, 64, 64, -77, out.ctypes.data)
    assert tuple(out[:4]) == sf == (16384, 16384, 1024, 1024) and out[4] == out[5] == sc.scale_value(-77, sf[0], False) == -77 * 64


def test_subpel_params_clamp(harness):
    g = rng(4)
    out = np.zeros(6, np.int32)
    for (other, this, _) in PAIRS:
        oh, th = (other * 3 + 2) // 4, (this * 3 + 2) // 4
        if sc.setup_scale_factors(other, oh, this, th) is None:
            continue
        sf = sc.setup_scale_factors(other, oh, this, th)
        for _ in range(200):
            far = int(g.integers(0, 3))
            span = (this, 4 * this, 20000)[far]
            pre_x, pre_y = int(g.integers(-span, span + 1)), int(g.integers(-span, span + 1))
            mv_r, mv_c = int(g.integers(-8000, 8001)), int(g.integers(-8000, 8001))
            for ss in (0, 1):
                for sb in (64, 128):
                    harness.harness_subpel_params(sb, pre_y, pre_x, mv_r, mv_c, other, oh, this, th, ss, ss, out.ctypes.data)
                    assert tuple(out) == sc.subpel_params(pre_y, pre_x, mv_r, mv_c, sf, other, oh, ss, ss, sb), (other, this, pre_x, pre_y, mv_r, mv_c, ss, sb)


# ---- 2. the convolve-scale functions (and the unscaled functions beside them) -------------------------------------------------------------------------
UNSCALED_NAMES = {(0, 0): "convolve_2d_copy_sr", (1, 0): "convolve_x_sr", (2, 0): "convolve_y_sr", (3, 0): "convolve_2d_sr",
                  (0, 1): "jnt_convolve_2d_copy", (1, 1): "jnt_convolve_x", (2, 1): "jnt_convolve_y", (3, 1): "jnt_convolve_2d"}


def c_convolve(ref, pic, oy, ox, w, h, fxa, fya, r, bd, r0, r1, is_comp, avg, dist, fwd, bck, cb, dst):
    """one call of the C function a reference (xs, ys, sx, sy) takes: the scale function, or for an unscaled reference the convolve function of its case"""
    xs, ys, sx, sy = r
    px, keep_x = sc.filter_params(fxa)
    py, keep_y = sc.filter_params(fya)
    cp = sc.ConvolveParams(0, avg, cb.ctypes.data, cb.shape[1], r0, r1, 0, is_comp, dist, fwd, bck, dist)
    src = pic.ctypes.data + (oy * pic.shape[1] + ox) * pic.itemsize
    hb = "highbd_" if bd > 8 else ""
    if xs != 1024 or ys != 1024:
        fn = getattr(ref, "svt_av1_%sconvolve_2d_scale_c" % hb)
        args = [vp(src), pic.shape[1], vp(dst.ctypes.data), dst.shape[1], w, h, C.byref(px), C.byref(py), sx, xs, sy, ys, C.byref(cp)]
    else:
        fn = getattr(ref, "svt_av1_%s%s_c" % (hb, UNSCALED_NAMES[((sx != 0) + 2 * (sy != 0), 1 if is_comp else 0)]))
        args = [vp(src), pic.shape[1], vp(dst.ctypes.data), dst.shape[1], w, h, C.byref(px), C.byref(py), sx >> 6, sy >> 6, C.byref(cp)]
    fn.restype = None
    fn(*(args + ([bd] if bd > 8 else [])))


def c_pred(ref, spec, refs, bd):
    """the prediction of one block as the reference's inter prediction makes it: one call per reference, the second averaging into the first one's buffer"""
    w, h, comp = spec["w"], spec["h"], spec["comp"]
    r0, r1 = sc.conv_rounds(bd, comp != 0)
    fxa, fya = sc.filter_rows(spec["fx"], w), sc.filter_rows(spec["fy"], h)
    cb = np.zeros((h, w), np.uint16)
    dst = np.zeros((h, w), np.uint16 if bd > 8 else np.uint8)
    for k, (pic, oy, ox, sx, sy, xs, ys) in enumerate(refs[:2 if comp else 1]):
        c_convolve(ref, pic, oy, ox, w, h, fxa, fya, (xs, ys, sx, sy), bd, r0, r1, int(comp != 0), k, int(comp == 2), spec["wts"][0], spec["wts"][1], cb, dst)
    return dst


@pytest.mark.parametrize("kind", ("random", "extreme"))
@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_prediction_cases_against_the_c(ref, bd, kind):
    """every block of test_scale.py's case list: scaled_pred == the reference's calls (the scale function for a scaled reference, svt_aom_convolve[..]'s for an
    unscaled one), bit for bit"""
    g = rng(11 + bd)
    pic = [sc.make_picture(g, kind, 270, 270, 270, bd) for _ in range(2)]
    for i, s in enumerate(sc.pred_case_list(bd)):
        refs = []
        for k, r in enumerate(s["refs"]):
            l, rgt, t, bot = sc.ref_extent(s["w"], s["h"], r)
            refs.append((pic[(i + k) % 2], t + int(g.integers(0, 270 - t - bot)), l + int(g.integers(0, 270 - l - rgt)), r[2], r[3], r[0], r[1]))
        want = c_pred(ref, s, refs, bd)
        got = sc.scaled_pred(refs, s["w"], s["h"], s["fx"], s["fy"], bd, s["comp"], *s["wts"])
        assert np.array_equal(got, want), (bd, i, s)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_form_cases_against_the_c(ref, bd):
    """the single-call cases of test_scale.py (the caller's roundings, every conv_params mode): scale_form == the C function"""
    g = rng(21 + bd)
    pic = sc.make_picture(g, "random", 150, 150, 150, bd)
    for (w, h, r, fx, fy, is_comp, avg, dist, wi, rounds) in sc.FORM_CASES:
        r0, r1 = sc.form_rounds(bd, is_comp, rounds)
        if bd == 12 and rounds is not None:
            r0, r1 = r0 + 2, r1 - 2
        ex, ey = sc.scaled_extent(w, h, r[2], r[3], r[0], r[1])
        oy, ox = 3 + int(g.integers(0, 150 - 3 - ey)), 3 + int(g.integers(0, 150 - 3 - ex))
        fxa, fya = sc.filter_rows(fx, w), sc.filter_rows(fy, h)
        cb = g.integers(0, 1 << (bd + 3), (h, w)).astype(np.uint16)
        fwd, bck = sc.WEIGHTS[wi]
        want_dst, want_cb = sc.scale_form(pic, oy, ox, w, h, fxa, fya, r[2], r[0], r[3], r[1], bd, r0, r1, is_comp, avg, dist, fwd, bck, cb)
        dst = np.zeros((h, w), pic.dtype)
        _scale_c(ref, pic, oy, ox, w, h, fxa, fya, r, bd, r0, r1, is_comp, avg, dist, fwd, bck, cb, dst)
        if want_dst is not None:
            assert np.array_equal(dst, want_dst), (bd, w, h, r)
        else:
            assert np.array_equal(cb, want_cb), (bd, w, h, r)


def _scale_c(ref, pic, oy, ox, w, h, fxa, fya, r, bd, r0, r1, is_comp, avg, dist, fwd, bck, cb, dst):
    """the scale function itself at steps 1024 / 1024 (the forms always take it)"""
    xs, ys, sx, sy = r
    px, keep_x = sc.filter_params(fxa)
    py, keep_y = sc.filter_params(fya)
    cp = sc.ConvolveParams(0, avg, cb.ctypes.data, cb.shape[1], r0, r1, 0, is_comp, dist, fwd, bck, dist)
    fn = getattr(ref, "svt_av1_%sconvolve_2d_scale_c" % ("highbd_" if bd > 8 else ""))
    fn.restype = None
    args = [vp(pic.ctypes.data + (oy * pic.shape[1] + ox) * pic.itemsize), pic.shape[1], vp(dst.ctypes.data), dst.shape[1], w, h, C.byref(px), C.byref(py), sx, xs, sy, ys,
            C.byref(cp)]
    fn(*(args + ([bd] if bd > 8 else [])))


# ---- 3. resize ----------------------------------------------------------------------------------------------------------------------------------------
def c_resize(ref, pic, w, h, w2, h2, bd):
    out = np.zeros((h2, w2), pic.dtype)
    fn = ref.svt_av1_highbd_resize_plane_c if bd > 8 else ref.svt_av1_resize_plane_c
    args = [vp(pic.ctypes.data), h, w, pic.shape[1], vp(out.ctypes.data), h2, w2, w2]
    assert fn(*(args + ([bd] if bd > 8 else []))) == 0
    return out


@pytest.mark.parametrize("kind", sc.CLASSES)
@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_resize_plane_against_the_c(harness, bd, kind):
    """the length pairs of test_scale.py along rows and along columns, and one factor-of-two step from every length 1 .. 70 (both half-band filters, every short-input
    branch): fully clamped indexing == the C's initial / middle / end loops"""
    g = rng(31 + bd)
    planes = [(a, 9, b, 6) for (a, b) in sc.RESIZE_PAIRS] + [(10, a, 7, b) for (a, b) in sc.RESIZE_PAIRS] + [(n, 3, (n + 1) >> 1, 3) for n in range(1, 71)]
    planes += [(n, 2, m, 2) for n in (1, 2, 3, 5, 8, 13, 21, 40) for m in range(1, 2 * n + 3)] + [(523, 12, 300, 9), (300, 20, 263, 20)]
    for (w, h, w2, h2) in planes:
        pic = sc.make_picture(g, kind, w, h, w + 2, bd)
        assert np.array_equal(sc.resize_plane(pic[:, :w], w2, h2, bd), c_resize(harness.ref, pic, w, h, w2, h2, bd)), (bd, kind, w, h, w2, h2)


@pytest.mark.parametrize("bd", (8, 10))
def test_one_dimensional_functions_against_the_c(ref, bd):
    """svt_av1_[highbd_]interpolate_core_c for every in_length 1 .. 60 and out_length 1 .. 2 * in + 2 with each of the five tables, svt_av1_[highbd_]down2_symeven_c
    for every even length up to 200"""
    g = rng(41 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    mx = (1 << bd) - 1
    for n in range(1, 61):
        a = g.integers(0, mx + 1, n).astype(dt)
        for m in range(1, 2 * n + 3):
            t = (n + m) % 5
            tab = np.ascontiguousarray(sc.RESIZE_FILTERS[t], np.int16)
            out = np.zeros(m, dt)
            if bd > 8:
                ref.svt_av1_highbd_interpolate_core_c(vp(a.ctypes.data), n, vp(out.ctypes.data), m, bd, vp(tab.ctypes.data))
            else:
                ref.svt_av1_interpolate_core_c(vp(a.ctypes.data), n, vp(out.ctypes.data), m, vp(tab.ctypes.data))
            assert np.array_equal(out, sc.interpolate_core(a.astype(np.int64), m, mx, sc.RESIZE_FILTERS[t])), (n, m, t)
    for n in range(2, 201, 2):
        a = g.integers(0, mx + 1, n).astype(dt)
        out = np.zeros(n // 2, dt)
        if bd > 8:
            ref.svt_av1_highbd_down2_symeven_c(vp(a.ctypes.data), n, vp(out.ctypes.data), bd)
        else:
            ref.svt_av1_down2_symeven_c(vp(a.ctypes.data), n, vp(out.ctypes.data))
        assert np.array_equal(out, sc.down2_symeven(a.astype(np.int64), mx)), n


# ---- 4. upscale ---------------------------------------------------------------------------------------------------------------------------------------
def c_upscale(harness, src, down_luma, up_luma, denom, sub_x, starts, mi_cols, bd, sb, up):
    """svt_av1_upscale_normative_rows on a copy of src with 8 writable columns either side (the C overwrites and restores 5)"""
    rows, last = src.shape[0], starts[-1] << (2 - sub_x)
    buf = np.zeros((rows, last + 16), src.dtype)
    buf[:, 8:8 + last] = src[:, :last]
    before = buf.copy()
    out = np.zeros((rows, up), src.dtype)
    st = np.ascontiguousarray(starts, np.int32)
    harness.harness_upscale(buf.ctypes.data + 8 * sb, buf.shape[1], out.ctypes.data, up, rows, sub_x, bd, int(sb == 2 and bd == 8), down_luma, up_luma, denom, mi_cols,
                            len(starts) - 1, st.ctypes.data)
    assert np.array_equal(buf, before)
    return out


@pytest.mark.parametrize("fmt", ((8, 1), (8, 2), (10, 2), (12, 2)))
@pytest.mark.parametrize("denom", sc.UPSCALE_DENOMS)
def test_upscale_against_the_c(harness, denom, fmt):
    bd, sb = fmt
    g = rng(51 + denom + bd + sb)
    for (up_luma, ntiles) in ((64, 1), (200, 1), (384, 3), (201, 1), (333, 2)):
        for kind in ("random", "extreme"):
            for sub_x in (0, 1):
                down, up, starts, mi_cols, down_luma = sc.upscale_geometry(up_luma, denom, sub_x, ntiles)
                last = starts[-1] << (2 - sub_x)
                src = sc.make_picture(g, kind, last, 6, last, bd).astype(np.uint16 if sb == 2 else np.uint8)
                want = c_upscale(harness, src, down_luma, up_luma, denom, sub_x, starts, mi_cols, bd, sb, up)
                assert np.array_equal(sc.upscale_rows(src, down, up, denom, sub_x, starts, bd), want), (up_luma, ntiles, denom, fmt, kind, sub_x)


def test_scaled_size_helper(ref):
    for dim in (8, 16, 17, 64, 200, 201, 333, 384, 1920, 3840):
        for denom in range(9, 17):
            v = C.c_uint16(dim)
            ref.calculate_scaled_size_helper(C.byref(v), C.c_uint8(denom))
            assert v.value == sc.scaled_size(dim, denom), (dim, denom)


# ---- 5. every table entry -----------------------------------------------------------------------------------------------------------------------------
def _symbol(ref, name, n):
    return np.ctypeslib.as_array((C.c_int16 * n).in_dll(ref, name)).astype(np.int64)


def test_every_table_entry(ref):
    for t, name in ((1, "875"), (2, "750"), (3, "625"), (4, "500")):
        assert np.array_equal(_symbol(ref, "svt_aom_av1_filteredinterp_filters" + name, 512).reshape(64, 8), sc.RESIZE_FILTERS[t]), name
    assert np.array_equal(_symbol(ref, "svt_aom_av1_down2_symeven_half_filter", 4), sc.DOWN2_EVEN)
    assert np.array_equal(_symbol(ref, "av1_down2_symodd_half_filter", 4), sc.DOWN2_ODD)
    # the normative table is static in a header: its source text, without preprocessor lines and comments
    text = open(os.path.join(SRC, "Lib", "Codec", "super_res.h")).read()
    body = re.search(r"av1_resize_filter_normative\[[^=]*=\s*\{(.*?)\};", text, re.S).group(1)
    body = "\n".join(ln.split("//")[0] for ln in body.split("\n") if not ln.lstrip().startswith("#"))
    vals = np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int64)
    assert vals.size == 512 and np.array_equal(vals.reshape(64, 8), sc.UPSCALE_FILTER)
    assert re.search(r"#define filteredinterp_filters1000 av1_resize_filter_normative", open(os.path.join(SRC, "Lib", "Codec", "resize.h")).read())
    assert all(np.all(t.sum(1) == 128) for t in sc.RESIZE_FILTERS)
    for k, name in enumerate(("sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp", "bilinear_filters", "sub_pel_filters_4", "sub_pel_filters_4smooth")):
        assert np.array_equal(_symbol(ref, name, 128).reshape(16, 8), sc.INTER_FILTERS[k]), name


# ---- 6. the golden file ---------------------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_reference_computes(harness):
    ref = harness.ref
    data = dict(seed=np.array([sc.GOLDEN_SEED]))
    for k in (0, 1):
        data["pic_8_%d" % k], data["pic_12_%d" % k] = sc.golden_picture(8, k), sc.golden_picture(12, k)
    for i, (bd, w, h, fx, fy, comp, wi, refs) in enumerate(sc.GOLDEN_PRED):
        spec = sc.pred_spec(w, h, refs, fx, fy, comp, sc.WEIGHTS[wi])
        data["pred_%d" % i] = c_pred(ref, spec, [(sc.golden_picture(bd, k), 3, 3, r[2], r[3], r[0], r[1]) for k, r in enumerate(refs)], bd)
        assert np.array_equal(data["pred_%d" % i], sc.golden_pred_expect(i)), i
    for i, (bd, w, h, w2, h2) in enumerate(sc.GOLDEN_RESIZE):
        data["resize_%d" % i] = c_resize(ref, sc.golden_picture(bd, 0), w, h, w2, h2, bd)
    for i, (bd, sb, up_luma, denom, sub_x, starts) in enumerate(sc.GOLDEN_UPSCALE):
        src, (down, up, st, mi_cols, down_luma) = sc.golden_upscale_input(i)
        data["upscale_%d" % i] = c_upscale(harness, src, down_luma, up_luma, denom, sub_x, st, mi_cols, bd, sb, up)
    if os.environ.get("SVT_SCALE_WRITE_GOLDEN") == "1":
        np.savez_compressed(sc.GOLDEN, **data)
    gold = sc.load_golden()
    assert sorted(gold.files) == sorted(data)
    for name in data:
        assert np.array_equal(gold[name], data[name]), name
    assert os.path.getsize(sc.GOLDEN) < 150 * 1024
