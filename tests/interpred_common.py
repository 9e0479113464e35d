"""AV1 inter prediction restated in numpy: the sixteen functions svt_av1_[highbd_]convolve_{2d_copy,x,y,2d}_sr_c and svt_av1_[highbd_]jnt_convolve_{2d_copy,x,y,2d}_c
(inter_prediction.c:311-418, 494-668, 670-777, 852-1033), the filter selection of av1_get_interp_filter_params_with_block_size (inter_prediction.h:137-145) and the
roundings of get_conv_params_no_round (convolve.h:40-64) -- with the reference's narrowings: int16_t intermediate rows, the 8-bit 2-D function's int16_t before the last
rounding, the 16-bit unsigned ConvBufType, the 16-bit shift-and-offset of jnt_convolve_2d_copy.  Vectorised: every function takes arrays whose LAST TWO axes are one
block's rows and columns, any number of leading axes.  This is the checker of tests/test_interpred.py (where the reference's sources do not exist);
tests/test_interpred_ref.py pins it on the reference's own functions and tables."""
import os

import numpy as np

REGULAR, SMOOTH, SHARP, BILINEAR = 0, 1, 2, 3
TABLE_NAMES = ("sub_pel_filters_8", "sub_pel_filters_8smooth", "sub_pel_filters_8sharp", "bilinear_filters", "sub_pel_filters_4", "sub_pel_filters_4smooth")


def _bilinear():
    return [[0, 0, 0, 128 - 8 * p, 8 * p, 0, 0, 0] for p in range(16)]


# [kind][phase][tap]: kinds 0 .. 3 are the InterpFilter values, 4 / 5 the 4-tap tables a dimension <= 4 selects
FILTERS = np.array([
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -6, 126, 8, -2, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -12, 116, 28, -8, 2, 0], [0, 2, -14, 110, 38, -10, 2, 0],
     [0, 2, -14, 102, 48, -12, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 84, 66, -12, 2, 0], [0, 2, -14, 76, 76, -14, 2, 0], [0, 2, -12, 66, 84, -14, 2, 0],
     [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -12, 48, 102, -14, 2, 0], [0, 2, -10, 38, 110, -14, 2, 0], [0, 2, -8, 28, 116, -12, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0],
     [0, 0, -2, 8, 126, -6, 2, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, 28, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0], [0, 0, 20, 60, 42, 6, 0, 0],
     [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, -2, 16, 54, 48, 12, 0, 0], [0, -2, 14, 52, 52, 14, -2, 0], [0, 0, 12, 48, 54, 16, -2, 0],
     [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0], [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0],
     [0, 0, 2, 34, 62, 28, 2, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [-2, 2, -6, 126, 8, -2, 2, 0], [-2, 6, -12, 124, 16, -6, 4, -2], [-2, 8, -18, 120, 26, -10, 6, -2], [-4, 10, -22, 116, 38, -14, 6, -2],
     [-4, 10, -22, 108, 48, -18, 8, -2], [-4, 10, -24, 100, 60, -20, 8, -2], [-4, 10, -24, 90, 70, -22, 10, -2], [-4, 12, -24, 80, 80, -24, 12, -4],
     [-2, 10, -22, 70, 90, -24, 10, -4], [-2, 8, -20, 60, 100, -24, 10, -4], [-2, 8, -18, 48, 108, -22, 10, -4], [-2, 6, -14, 38, 116, -22, 10, -4],
     [-2, 6, -10, 26, 120, -18, 8, -2], [-2, 4, -6, 16, 124, -12, 6, -2], [0, 2, -2, 8, 126, -6, 2, -2]],
    _bilinear(),
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -4, 126, 8, -2, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0], [0, 0, -10, 116, 28, -6, 0, 0], [0, 0, -12, 110, 38, -8, 0, 0],
     [0, 0, -12, 102, 48, -10, 0, 0], [0, 0, -14, 94, 58, -10, 0, 0], [0, 0, -12, 84, 66, -10, 0, 0], [0, 0, -12, 76, 76, -12, 0, 0], [0, 0, -10, 66, 84, -12, 0, 0],
     [0, 0, -10, 58, 94, -14, 0, 0], [0, 0, -10, 48, 102, -12, 0, 0], [0, 0, -8, 38, 110, -12, 0, 0], [0, 0, -6, 28, 116, -10, 0, 0], [0, 0, -4, 18, 122, -8, 0, 0],
     [0, 0, -2, 8, 126, -4, 0, 0]],
    [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, 30, 62, 34, 2, 0, 0], [0, 0, 26, 62, 36, 4, 0, 0], [0, 0, 22, 62, 40, 4, 0, 0], [0, 0, 20, 60, 42, 6, 0, 0],
     [0, 0, 18, 58, 44, 8, 0, 0], [0, 0, 16, 56, 46, 10, 0, 0], [0, 0, 14, 54, 48, 12, 0, 0], [0, 0, 12, 52, 52, 12, 0, 0], [0, 0, 12, 48, 54, 14, 0, 0],
     [0, 0, 10, 46, 56, 16, 0, 0], [0, 0, 8, 44, 58, 18, 0, 0], [0, 0, 6, 42, 60, 20, 0, 0], [0, 0, 4, 40, 62, 22, 0, 0], [0, 0, 4, 36, 62, 26, 0, 0],
     [0, 0, 2, 34, 62, 30, 0, 0]],
], np.int16)
assert FILTERS.shape == (6, 16, 8) and np.all(FILTERS.sum(axis=2) == 128)

# quant_dist_lookup_table (inter_prediction.c:268-271): the eight (fwd_offset, bck_offset) pairs svt_av1_dist_wtd_comp_weight_assign can return
DIST_WEIGHTS = [(9, 7), (11, 5), (12, 4), (13, 3), (7, 9), (5, 11), (4, 12), (3, 13)]

# a tap set that is none of AV1's tables (sums to 128, one tap outside a signed byte) and still keeps the reference's assertions on its sums: negative taps sum to
# -60 >= -64, positive ones to 188 < 192
FOREIGN_TAPS = np.array([-4, 12, -28, 150, 18, -24, 8, -4], np.int16)

# name -> (case, jnt): case bit 0 = filters in x, bit 1 = filters in y.  With the "highbd_" forms: the sixteen.
FUNCTIONS = {"convolve_2d_copy_sr": (0, False), "convolve_x_sr": (1, False), "convolve_y_sr": (2, False), "convolve_2d_sr": (3, False),
             "jnt_convolve_2d_copy": (0, True), "jnt_convolve_x": (1, True), "jnt_convolve_y": (2, True), "jnt_convolve_2d": (3, True)}


def filter_kind(interp_filter, dim):
    """av1_get_interp_filter_params_with_block_size: index into FILTERS of the kernel `interp_filter` selects for a block dimension `dim`"""
    if dim <= 4 and interp_filter in (REGULAR, SHARP):
        return 4
    if dim <= 4 and interp_filter == SMOOTH:
        return 5
    return interp_filter


def conv_rounds(bd, compound):
    """(round_0, round_1) of get_conv_params_no_round(.., is_compound = compound, bd)"""
    r0, r1 = 3, (7 if compound else 11)
    over = bd + 7 - r0 + 2 - 16
    if over > 0:
        r0 += over
        if not compound:
            r1 -= over
    return r0, r1


def rpot(v, n):
    return (v + ((1 << n) >> 1)) >> n  # ROUND_POWER_OF_TWO on signed values: arithmetic shift, as the C compilers the reference supports do


def i16(v):
    return ((v + 32768) & 0xffff) - 32768


def _hsum(a, taps, w):
    return sum(int(taps[k]) * a[..., :, k:k + w] for k in range(8))


def _vsum(a, taps, h):
    return sum(int(taps[k]) * a[..., k:k + h, :] for k in range(8))


def round_offset(bd, r0, r1):
    ob = bd + 14 - r0
    return (1 << (ob - r1)) + (1 << (ob - r1 - 1))


def core(ext, w, h, taps_x, taps_y, case, bd, r0, r1, jnt, is8):
    """ext[..., h + 7, w + 7]: the block with 3 samples left / above and 4 right / below.  Returns the value the `_sr` function clips (jnt False) or `res` of the jnt_
    function before it is stored or averaged (jnt True), int64."""
    ext = np.asarray(ext).astype(np.int64)
    assert ext.shape[-2:] == (h + 7, w + 7)
    ro, rb = round_offset(bd, r0, r1), 14 - r0 - r1
    if case == 0:
        px = ext[..., 3:3 + h, 3:3 + w]
        return (((px << rb) & 0xffff) + ro) & 0xffff if jnt else px
    if case == 1:
        s = rpot(_hsum(ext[..., 3:3 + h, :], taps_x, w), r0)
        return (1 << (7 - r1)) * s + ro if jnt else rpot(s, 7 - r0)
    if case == 2:
        s = _vsum(ext[..., :, 3:3 + w], taps_y, h)
        return rpot(s * (1 << (7 - r0)), r1) + ro if jnt else rpot(s, 7)
    im = i16(rpot(_hsum(ext, taps_x, w) + (1 << (bd + 6)), r0))
    t = rpot((1 << (bd + 14 - r0)) + _vsum(im, taps_y, h), r1)
    if jnt:
        return t & 0xffff
    t = t - ro
    if is8:
        t = i16(t)
    return rpot(t, rb)


def clip(v, bd):
    return np.clip(v, 0, (1 << bd) - 1)


def convolve_sr(ext, w, h, taps_x, taps_y, case, bd, r0, r1, is8):
    """svt_av1_[highbd_]convolve_{2d_copy,x,y,2d}_sr_c -> dst"""
    return clip(core(ext, w, h, taps_x, taps_y, case, bd, r0, r1, False, is8), bd)


def jnt_convolve(ext, w, h, taps_x, taps_y, case, bd, r0, r1, is8, do_average=False, cb=None, use_jnt_comp_avg=False, fwd_offset=0, bck_offset=0):
    """svt_av1_[highbd_]jnt_convolve_{2d_copy,x,y,2d}_c: do_average False -> what it stores in conv_params->dst (ConvBufType); True -> what it stores in dst8 / dst16,
    with cb = the ConvBufType buffer the first call left"""
    res = core(ext, w, h, taps_x, taps_y, case, bd, r0, r1, True, is8)
    if not do_average:
        return res & 0xffff
    tmp = np.asarray(cb).astype(np.int64)
    tmp = (tmp * fwd_offset + res * bck_offset) >> 4 if use_jnt_comp_avg else (tmp + res) >> 1
    return clip(rpot(tmp - round_offset(bd, r0, r1), 14 - r0 - r1), bd)


def predict(refs, w, h, filter_x, filter_y, compound, bd, fwd_offset=0, bck_offset=0):
    """One descriptor of svt_hip_inter_pred_batch.  refs = [(ext, subpel_x, subpel_y)] (two entries when compound != 0; ext as in core()); compound 0 / 1 / 2."""
    is8 = bd == 8
    r0, r1 = conv_rounds(bd, compound != 0)
    out = None
    for k, (ext, sx, sy) in enumerate(refs[:2 if compound else 1]):
        tx, ty = FILTERS[filter_kind(filter_x, w)][sx], FILTERS[filter_kind(filter_y, h)][sy]
        case = int(sx != 0) + 2 * int(sy != 0)
        if not compound:
            return convolve_sr(ext, w, h, tx, ty, case, bd, r0, r1, is8)
        if k == 0:
            out = jnt_convolve(ext, w, h, tx, ty, case, bd, r0, r1, is8)
        else:
            out = jnt_convolve(ext, w, h, tx, ty, case, bd, r0, r1, is8, True, out, compound == 2, fwd_offset, bck_offset)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
CLASSES = ("random", "zero", "max", "checker", "checker1")


def make_ext(g, kind, w, h, bd):
    """(h + 7, w + 7) samples of one input class; the maximum / zero checkerboard with 2 x 2 cells drives the sharp kernel into clipping on both sides"""
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    if kind == "random":
        return g.integers(0, mx + 1, (h + 7, w + 7)).astype(dt)
    if kind == "zero":
        return np.zeros((h + 7, w + 7), dt)
    if kind == "max":
        return np.full((h + 7, w + 7), mx, dt)
    yy, xx = np.mgrid[0:h + 7, 0:w + 7]
    if kind == "checker1":  # cells of one sample
        return (((yy + xx) & 1) * mx).astype(dt)
    return ((((yy >> 1) + (xx >> 1)) & 1) * mx).astype(dt)  # cells of 2 x 2: max max 0 0 under the SHARP half-pel taps is 152 / 128 of the maximum, and -24 / 128 one cell on


# ---- the golden cases (tests/golden/interpred.npz: what the reference's C computes for them; written by tests/test_interpred_ref.py) ------------------------------
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interpred.npz")
GOLDEN_SEED = 20260


def golden_cases():
    """[(w, h, bd, filter_x, filter_y, compound, (sx0, sy0), (sx1, sy1), (fwd, bck), class)]: every case x compound mode x bit depth, every filter, both 4-tap swaps,
    phases 1, 8, 15, every distance-weight pair; small blocks only (the file stays small)"""
    out = []
    phases = [(0, 0), (1, 0), (0, 15), (8, 1), (15, 8)]
    sizes = [(4, 4), (8, 8), (4, 16), (16, 4), (2, 2), (16, 16), (32, 8), (8, 32)]
    k = 0
    for bd in (8, 10, 12):
        for compound in (0, 1, 2):
            for pi, ph in enumerate(phases):
                for rep in range(2):
                    w, h = sizes[k % len(sizes)]
                    fx, fy = (k // 2) % 4, (k // 3 + 1) % 4 if (k // 2) % 4 != BILINEAR else BILINEAR
                    if fx != BILINEAR and fy == BILINEAR:
                        fy = SHARP
                    ph1 = phases[(pi + 1 + rep) % len(phases)]
                    out.append((w, h, bd, fx, fy, compound, ph, ph1, DIST_WEIGHTS[k % 8], CLASSES[(k // 5) % 5] if k % 3 else "random"))
                    k += 1
    return out


def golden_inputs(i, case):
    """the two references of golden case i (deterministic)"""
    w, h, bd, _, _, _, ph0, ph1, _, kind = case
    g = np.random.default_rng(GOLDEN_SEED + i)
    return [(make_ext(g, kind, w, h, bd), ph0[0], ph0[1]), (make_ext(g, "random" if kind == "zero" else kind, w, h, bd), ph1[0], ph1[1])]


def load_golden():
    return np.load(GOLDEN_FILE)
