"""Pins tests/interpred_common.py (the numpy restatement the kernels of csrc/interpred.hip are checked against) on the REAL reference: its six tap tables and its sixteen
`svt_av1_*convolve*_c` functions in oracle/_ref/libsvtref.so, called through ctypes mirrors of InterpFilterParams and ConvolveParams.  CPU only; runs where the
reference's sources and the library exist (the build container), skipped elsewhere.  `SVT_INTERPRED_WRITE_GOLDEN=1` rewrites tests/golden/interpred.npz from the
reference's outputs."""
import ctypes as C
import os

import numpy as np
import pytest

import interpred_common as ic
from conftest import REF_LIB, load_pkg, p

REF = os.environ.get("SVT_REF", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Source", "Lib", "Codec", "inter_prediction.c")) or not os.path.exists(REF_LIB),
                                reason="the reference's sources or oracle/_ref/libsvtref.so are not on this machine")

BIT_DEPTHS = (8, 10, 12)
FOREIGN = ic.FOREIGN_TAPS


@pytest.fixture(scope="module")
def rf(ref):
    pkg = load_pkg()
    cv = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    for name in ic.FUNCTIONS:
        f8, f16 = getattr(ref, "svt_av1_%s_c" % name), getattr(ref, "svt_av1_highbd_%s_c" % name)
        f8.restype, f8.argtypes = None, cv
        f16.restype, f16.argtypes = None, cv + [C.c_int32]
    ref.pkg = pkg
    ref.tables = [np.ctypeslib.as_array((C.c_int16 * (16 * 8)).in_dll(ref, n)).reshape(16, 8) for n in ic.TABLE_NAMES]
    return ref


def ref_call(rf, name, ext, w, h, taps_table_x, taps_table_y, sx, sy, bd, r0, r1, do_average=0, cb=None, use_jnt=0, fwd=0, bck=0, dst_init=0xA5):
    """one of the sixteen on the block inside `ext` ((h + 7) x (w + 7)); taps_table_*: int16[16][8] the InterpFilterParams points to.  Returns (dst, cb)."""
    pkg = rf.pkg
    hbd = bd > 8
    dt = np.uint16 if hbd else np.uint8
    ext = np.ascontiguousarray(ext, dtype=dt)
    stride = ext.shape[1]
    dst = np.full((h, w + 3), dst_init if not hbd else 0xA5A5, dt)
    cbuf = np.full((h, w + 5), 0x5A5A, np.uint16) if cb is None else np.ascontiguousarray(np.pad(np.asarray(cb, np.uint16), ((0, 0), (0, 5))))
    tx, ty = np.ascontiguousarray(taps_table_x, dtype=np.int16), np.ascontiguousarray(taps_table_y, dtype=np.int16)
    fx, fy = pkg.InterpFilterParams(tx.ctypes.data, 8, 16, 0), pkg.InterpFilterParams(ty.ctypes.data, 8, 16, 0)
    cp = pkg.ConvolveParams(0, do_average, cbuf.ctypes.data, cbuf.shape[1], r0, r1, 0, 1 if name.startswith("jnt") else 0, use_jnt, fwd, bck, use_jnt)
    src = ext.ctypes.data + (3 * stride + 3) * ext.itemsize
    args = [src, stride, p(dst), dst.shape[1], w, h, C.addressof(fx), C.addressof(fy), sx, sy, C.addressof(cp)]
    if hbd:
        getattr(rf, "svt_av1_highbd_%s_c" % name)(*args, bd)
    else:
        getattr(rf, "svt_av1_%s_c" % name)(*args)
    return dst[:, :w].astype(np.int64), cbuf[:, :w].astype(np.int64)


def check_function(rf, name, ext, w, h, kx, ky, sx, sy, bd, tag):
    """restatement == reference for one function on one block: the `_sr` result, or the jnt_ function's three behaviours (store, average, distance-weighted)"""
    case, jnt = ic.FUNCTIONS[name]
    r0, r1 = ic.conv_rounds(bd, jnt)
    tx, ty = ic.FILTERS[kx][sx], ic.FILTERS[ky][sy]
    is8 = bd == 8
    if not jnt:
        got, _ = ref_call(rf, name, ext, w, h, ic.FILTERS[kx], ic.FILTERS[ky], sx, sy, bd, r0, r1)
        assert np.array_equal(got, ic.convolve_sr(ext, w, h, tx, ty, case, bd, r0, r1, is8)), tag
        return
    dst, cb = ref_call(rf, name, ext, w, h, ic.FILTERS[kx], ic.FILTERS[ky], sx, sy, bd, r0, r1)
    assert np.array_equal(cb, ic.jnt_convolve(ext, w, h, tx, ty, case, bd, r0, r1, is8)), tag
    assert np.all(dst == (0xA5A5 if bd > 8 else 0xA5)), tag  # do_average == 0 leaves dst untouched
    first = (cb[::-1, ::-1] + 3) & 0xffff  # any ConvBufType content will do as the first call's buffer
    for (use_jnt, fwd, bck) in ((0, 0, 0),) + tuple((1, f, b) for (f, b) in ic.DIST_WEIGHTS[::3]):
        got, _ = ref_call(rf, name, ext, w, h, ic.FILTERS[kx], ic.FILTERS[ky], sx, sy, bd, r0, r1, 1, first, use_jnt, fwd, bck)
        assert np.array_equal(got, ic.jnt_convolve(ext, w, h, tx, ty, case, bd, r0, r1, is8, True, first, bool(use_jnt), fwd, bck)), tag + (use_jnt, fwd, bck)


def test_tap_tables_are_the_reference(rf):
    for k, name in enumerate(ic.TABLE_NAMES):
        assert np.array_equal(rf.tables[k], ic.FILTERS[k]), name


def test_every_function_every_phase_pair(rf):
    """all sixteen functions at 8 / 10 / 12 bit, all 16 x 16 phase pairs at 8x8 (REGULAR x SHARP), random input"""
    g = np.random.default_rng(1)
    for bd in BIT_DEPTHS:
        ext = ic.make_ext(g, "random", 8, 8, bd)
        for name in ic.FUNCTIONS:
            for sx in range(16):
                for sy in range(16):
                    check_function(rf, name, ext, 8, 8, ic.REGULAR, ic.SHARP, sx, sy, bd, (name, bd, sx, sy))


def test_every_filter_pair_every_class_and_size(rf):
    """every (filter_x, filter_y) pair of the four filters, through the block-size selection (4-tap tables at a dimension <= 4), at sizes with one, both or no such
    dimension; every input class (the 2 x 2 checkerboard reaches both clips)"""
    g = np.random.default_rng(2)
    for bd in BIT_DEPTHS:
        for (w, h) in ((4, 4), (4, 16), (16, 4), (8, 8), (2, 8), (32, 16)):
            for kind in ic.CLASSES:
                ext = ic.make_ext(g, kind, w, h, bd)
                for fx in range(4):
                    for fy in range(4):
                        kx, ky = ic.filter_kind(fx, w), ic.filter_kind(fy, h)
                        sx, sy = (1, 8, 15)[(fx + fy) % 3], (15, 1, 8)[(fx + 2 * fy) % 3]
                        for name in ic.FUNCTIONS:
                            check_function(rf, name, ext, w, h, kx, ky, sx, sy, bd, (name, bd, w, h, kind, fx, fy))


def test_foreign_taps(rf):
    """a tap set that is none of AV1's tables, one tap outside a signed byte.  (The reference is built with its assertions, which bound the sums: the set stays inside
    them, so the int16_t narrowings are never reached through the reference -- with AV1's tables and these they are the identity, and the restatement applies them
    literally all the same.)"""
    g = np.random.default_rng(3)
    table = np.zeros((16, 8), np.int16)
    table[:] = FOREIGN
    table[5] = [0, 0, 0, 128, 0, 0, 0, 0]
    table[9] = FOREIGN[::-1]
    for bd in BIT_DEPTHS:
        for kind in ("random", "checker", "max"):
            ext = ic.make_ext(g, kind, 8, 8, bd)
            for name in ic.FUNCTIONS:
                case, jnt = ic.FUNCTIONS[name]
                r0, r1 = ic.conv_rounds(bd, jnt)
                for (sx, sy) in ((3, 9), (5, 3), (9, 5)):
                    dst, cb = ref_call(rf, name, ext, 8, 8, table, table, sx, sy, bd, r0, r1)
                    if jnt:
                        assert np.array_equal(cb, ic.jnt_convolve(ext, 8, 8, table[sx], table[sy], case, bd, r0, r1, bd == 8)), (name, bd, kind)
                    else:
                        assert np.array_equal(dst, ic.convolve_sr(ext, 8, 8, table[sx], table[sy], case, bd, r0, r1, bd == 8)), (name, bd, kind)


def _golden_from_reference(rf):
    out = {"seed": np.array([ic.GOLDEN_SEED], np.int64)}
    for i, case in enumerate(ic.golden_cases()):
        w, h, bd, fx, fy, compound, _, _, (fwd, bck), _ = case
        refs = ic.golden_inputs(i, case)
        kx, ky = ic.filter_kind(fx, w), ic.filter_kind(fy, h)
        r0, r1 = ic.conv_rounds(bd, compound != 0)
        names = {(c, j): n for n, (c, j) in ic.FUNCTIONS.items()}
        cb = None
        for k, (ext, sx, sy) in enumerate(refs[:2 if compound else 1]):
            name = names[(int(sx != 0) + 2 * int(sy != 0), compound != 0)]
            dst, cbo = ref_call(rf, name, ext, w, h, ic.FILTERS[kx], ic.FILTERS[ky], sx, sy, bd, r0, r1, int(k == 1), cb, int(compound == 2), fwd, bck)
            cb = cbo
        out["out_%d" % i] = dst.astype(np.uint16 if bd > 8 else np.uint8)
        out["insum_%d" % i] = np.array([sum(int(e.astype(np.int64).sum()) for (e, _, _) in refs)], np.int64)
    return out


def test_golden_file_is_what_the_reference_computes(rf):
    """tests/golden/interpred.npz (what tests/test_interpred.py compares the kernels with where no reference exists) == the reference's outputs, entry for entry"""
    now = _golden_from_reference(rf)
    if os.environ.get("SVT_INTERPRED_WRITE_GOLDEN") == "1":
        np.savez_compressed(ic.GOLDEN_FILE, **now)
    assert os.path.getsize(ic.GOLDEN_FILE) < 256 * 1024
    gold = ic.load_golden()
    assert sorted(gold.files) == sorted(now)
    for k in now:
        assert gold[k].dtype == now[k].dtype and np.array_equal(gold[k], now[k]), k
    # and the restatement agrees with every entry
    for i, case in enumerate(ic.golden_cases()):
        w, h, bd, fx, fy, compound, _, _, (fwd, bck), _ = case
        assert np.array_equal(ic.predict(ic.golden_inputs(i, case), w, h, fx, fy, compound, bd, fwd, bck), gold["out_%d" % i]), (i, case)
