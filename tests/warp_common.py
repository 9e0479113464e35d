"""AV1 warped motion in numpy / Python integers: what csrc/warp.hip is checked against.  Written from the arithmetic of the AV1 block warp process and of the reference's
svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c, find_affine_int, svt_get_shear_params and warp_error; tests/test_warp_ref.py pins every function here, and every
entry of the two tables, on the reference's C.  The filter works on whole (15, 8, 8) index arrays per 8x8 tile -- no lanes, no LDS, no packed dot products: a different
route to the same integers than the kernel's."""
import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp.npz")
GOLDEN_SEED = 4230

BW = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BH = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)
TRANS_CLAMP = 128 << 16  # WARPEDMODEL_TRANS_CLAMP
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# Warped_Filters (AV1 specification, block warp process): the rows for fractional positions [-1, 0) use taps 0 .. 5, those for [0, 1) all eight, those for [1, 2) are
# the first 64 moved up by two taps except the very first; row 192 repeats row 191
_LO = """0 0 127 1 0 0|0 -1 127 2 0 0|1 -3 127 4 -1 0|1 -4 126 6 -2 1|1 -5 126 8 -3 1|1 -6 125 11 -4 1|1 -7 124 13 -4 1|2 -8 123 15 -5 1|2 -9 122 18 -6 1|2 -10 121 20 -6 1|
2 -11 120 22 -7 2|2 -12 119 25 -8 2|3 -13 117 27 -8 2|3 -13 116 29 -9 2|3 -14 114 32 -10 3|3 -15 113 35 -10 2|3 -15 111 37 -11 3|3 -16 109 40 -11 3|3 -16 108 42 -12 3|
4 -17 106 45 -13 3|4 -17 104 47 -13 3|4 -17 102 50 -14 3|4 -17 100 52 -14 3|4 -18 98 55 -15 4|4 -18 96 58 -15 3|4 -18 94 60 -16 4|4 -18 91 63 -16 4|4 -18 89 65 -16 4|
4 -18 87 68 -17 4|4 -18 85 70 -17 4|4 -18 82 73 -17 4|4 -18 80 75 -17 4|4 -18 78 78 -18 4|4 -17 75 80 -18 4|4 -17 73 82 -18 4|4 -17 70 85 -18 4|4 -17 68 87 -18 4|
4 -16 65 89 -18 4|4 -16 63 91 -18 4|4 -16 60 94 -18 4|3 -15 58 96 -18 4|4 -15 55 98 -18 4|3 -14 52 100 -17 4|3 -14 50 102 -17 4|3 -13 47 104 -17 4|3 -13 45 106 -17 4|
3 -12 42 108 -16 3|3 -11 40 109 -16 3|3 -11 37 111 -15 3|2 -10 35 113 -15 3|3 -10 32 114 -14 3|2 -9 29 116 -13 3|2 -8 27 117 -13 3|2 -8 25 119 -12 2|2 -7 22 120 -11 2|
1 -6 20 121 -10 2|1 -6 18 122 -9 2|1 -5 15 123 -8 2|1 -4 13 124 -7 1|1 -4 11 125 -6 1|1 -3 8 126 -5 1|1 -2 6 126 -4 1|0 -1 4 127 -3 1|0 0 2 127 -1 0"""
_MID = """0 0 0 127 1 0 0 0|0 0 -1 127 2 0 0 0|0 1 -3 127 4 -2 1 0|0 1 -5 127 6 -2 1 0|0 2 -6 126 8 -3 1 0|-1 2 -7 126 11 -4 2 -1|-1 3 -8 125 13 -5 2 -1|
-1 3 -10 124 16 -6 3 -1|-1 4 -11 123 18 -7 3 -1|-1 4 -12 122 20 -7 3 -1|-1 4 -13 121 23 -8 3 -1|-2 5 -14 120 25 -9 4 -1|-1 5 -15 119 27 -10 4 -1|
-1 5 -16 118 30 -11 4 -1|-2 6 -17 116 33 -12 5 -1|-2 6 -17 114 35 -12 5 -1|-2 6 -18 113 38 -13 5 -1|-2 7 -19 111 41 -14 6 -2|-2 7 -19 110 43 -15 6 -2|
-2 7 -20 108 46 -15 6 -2|-2 7 -20 106 49 -16 6 -2|-2 7 -21 104 51 -16 7 -2|-2 7 -21 102 54 -17 7 -2|-2 8 -21 100 56 -18 7 -2|-2 8 -22 98 59 -18 7 -2|
-2 8 -22 96 62 -19 7 -2|-2 8 -22 94 64 -19 7 -2|-2 8 -22 91 67 -20 8 -2|-2 8 -22 89 69 -20 8 -2|-2 8 -22 87 72 -21 8 -2|-2 8 -21 84 74 -21 8 -2|
-2 8 -22 82 77 -21 8 -2|-2 8 -21 79 79 -21 8 -2|-2 8 -21 77 82 -22 8 -2|-2 8 -21 74 84 -21 8 -2|-2 8 -21 72 87 -22 8 -2|-2 8 -20 69 89 -22 8 -2|
-2 8 -20 67 91 -22 8 -2|-2 7 -19 64 94 -22 8 -2|-2 7 -19 62 96 -22 8 -2|-2 7 -18 59 98 -22 8 -2|-2 7 -18 56 100 -21 8 -2|-2 7 -17 54 102 -21 7 -2|
-2 7 -16 51 104 -21 7 -2|-2 6 -16 49 106 -20 7 -2|-2 6 -15 46 108 -20 7 -2|-2 6 -15 43 110 -19 7 -2|-2 6 -14 41 111 -19 7 -2|-1 5 -13 38 113 -18 6 -2|
-1 5 -12 35 114 -17 6 -2|-1 5 -12 33 116 -17 6 -2|-1 4 -11 30 118 -16 5 -1|-1 4 -10 27 119 -15 5 -1|-1 4 -9 25 120 -14 5 -2|-1 3 -8 23 121 -13 4 -1|
-1 3 -7 20 122 -12 4 -1|-1 3 -7 18 123 -11 4 -1|-1 3 -6 16 124 -10 3 -1|-1 2 -5 13 125 -8 3 -1|-1 2 -4 11 126 -7 2 -1|0 1 -3 8 126 -6 2 0|0 1 -2 6 127 -5 1 0|
0 1 -2 4 127 -3 1 0|0 0 0 2 127 -1 0 0"""


def _rows(text, n):
    a = np.array([[int(v) for v in r.split()] for r in text.replace("\n", "").split("|")], np.int64)
    assert a.shape == (64, n)
    return a


def _warped_filter():
    t = np.zeros((193, 8), np.int64)
    t[:64, :6] = _rows(_LO, 6)
    t[64:128] = _rows(_MID, 8)
    t[128:192, 2:] = t[:64, :6]
    t[128] = (0, 0, 0, 1, 127, 0, 0, 0)
    t[192] = t[191]
    return t


WARPED_FILTER = _warped_filter()
# the divisor table of the model fit: entry n = round(2^22 / (256 + n)), 16384 at 0 and 8192 at 256
DIV_LUT = np.array([((1 << 22) + (256 + n) // 2) // (256 + n) for n in range(257)], np.int64)
ROWS_SEEN = set()  # filter rows the last calls of warp_affine used (tests clear it and assert coverage)


def rpot(v, n):
    """ROUND_POWER_OF_TWO: (v + half) >> n with an arithmetic shift, n >= 0; ints or int64 arrays"""
    return (v + ((1 << n) >> 1)) >> n


def rpot_signed(v, n):
    return -rpot(-v, n) if v < 0 else rpot(v, n)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def i16(v):
    return ((int(v) + 32768) & 0xffff) - 32768


def i32(v):
    return ((int(v) + (1 << 31)) & 0xffffffff) - (1 << 31)


def i64(v):
    return ((int(v) + (1 << 63)) & 0xffffffffffffffff) - (1 << 63)


def rpot_signed64(v, n):
    """ROUND_POWER_OF_TWO_SIGNED_64 on an int64_t that may have wrapped (sample sets outside the range the C asserts): negation and addition modulo 2^64"""
    half = (1 << n) >> 1
    return i64(-(i64(i64(-v) + half) >> n)) if v < 0 else i64(v + half) >> n


def shear_allowed(alpha, beta, gamma, delta):
    return 4 * abs(alpha) + 7 * abs(beta) < 65536 and 4 * abs(gamma) + 4 * abs(delta) < 65536


def conv_rounds(bd, is_compound):
    """round_0, round_1 of get_conv_params_no_round(0, 0, 0, ., ., is_compound, bd): round_0 is raised while bd + FILTER_BITS - round_0 + 2 > 16"""
    r0 = 3
    r1 = 7 if is_compound else 14 - r0
    over = bd + 7 - r0 + 2 - 16
    if over > 0:
        r0 += over
        if not is_compound:
            r1 -= over
    return r0, r1


def tile_projection(mat, ssx, ssy, j, i):
    """ix4, sx4 (before the shear terms), iy4, sy4 of the tile whose first sample is (j, i); None when src or dst leave int32_t"""
    src_x, src_y = (j + 4) << ssx, (i + 4) << ssy
    dst_x = mat[2] * src_x + mat[3] * src_y + mat[0]
    dst_y = mat[4] * src_x + mat[5] * src_y + mat[1]
    if not all(INT32_MIN <= v <= INT32_MAX for v in (src_x, src_y, dst_x, dst_y)):
        return None
    x4, y4 = dst_x >> ssx, dst_y >> ssy
    return x4 >> 16, x4 & 0xffff, y4 >> 16, y4 & 0xffff


def _tile(ref, width, height, mat, shear, ssx, ssy, j, i, bd, rbh):
    """the vertical filter's sums (offset included, before rounding) of one 8x8 tile, (8, 8) int64"""
    alpha, beta, gamma, delta = shear
    ix4, sx4, iy4, sy4 = tile_projection(mat, ssx, ssy, j, i)
    sx4 = (sx4 - 4 * alpha - 4 * beta) & ~63
    sy4 = (sy4 - 4 * gamma - 4 * delta) & ~63
    k, l, m = np.arange(-7, 8), np.arange(-4, 4), np.arange(8)
    iy = np.clip(iy4 + k, 0, height - 1)
    offs = rpot(sx4 + beta * (k[:, None] + 4) + alpha * (l[None, :] + 4), 10) + 64
    assert offs.min() >= 0 and offs.max() <= 192
    xs = np.clip((ix4 + l - 3)[None, :, None] + m[None, None, :], 0, width - 1)
    samples = ref[iy[:, None, None], xs].astype(np.int64)
    tmp = rpot((1 << (bd + 6)) + (samples * WARPED_FILTER[offs]).sum(-1), rbh)  # (15, 8)
    assert tmp.min() >= 0 and tmp.max() < 1 << (bd + 8 - rbh)
    kv = np.arange(-4, 4)
    offv = rpot(sy4 + delta * (kv[:, None] + 4) + gamma * (l[None, :] + 4), 10) + 64
    assert offv.min() >= 0 and offv.max() <= 192
    ROWS_SEEN.update(np.unique(offs).tolist())
    ROWS_SEEN.update(np.unique(offv).tolist())
    rows = np.arange(8)[:, None, None] + m[None, None, :]  # output row k reads intermediate rows k .. k + 7
    return (1 << (bd + 14 - rbh)) + (tmp[rows, np.arange(8)[None, :, None]] * WARPED_FILTER[offv]).sum(-1)


def warp_affine(ref, mat, shear, width, height, p_col, p_row, p_width, p_height, ssx, ssy, bd, r0, r1, is_compound=False, do_average=False, jnt=False, fwd=0, bck=0,
                cb=None, highbd=None):
    """svt_av1_warp_affine_c (highbd False) / svt_av1_highbd_warp_affine_c on `ref` (a 2-D array whose [y, x] is sample (x, y) of the picture; only [0, height) x
    [0, width) is indexed).  Returns the p_height x p_width block it writes: pred, or the ConvBufType block when is_compound and not do_average; cb is the ConvBufType
    block read when do_average"""
    highbd = bd > 8 if highbd is None else highbd
    mat = [int(v) for v in mat]
    shear = [int(v) for v in shear]
    rbh = r0 + max(bd + 7 - r0 - 14, 0) if highbd else r0
    rbv = r1 if is_compound else 14 - rbh
    round_bits, offset_bits = 14 - r0 - r1, bd + 14 - r0
    out = np.zeros((p_height, p_width), np.int64)
    for i in range(0, p_height, 8):
        for j in range(0, p_width, 8):
            s = rpot(_tile(ref, width, height, mat, shear, ssx, ssy, p_col + j, p_row + i, bd, rbh), rbv)
            hh, ww = min(8, p_height - i), min(8, p_width - j)
            s = s[:hh, :ww]
            if not is_compound:
                v = np.clip(s - (1 << (bd - 1)) - (1 << bd), 0, (1 << bd) - 1)
            elif not do_average:
                v = s & 0xffff  # ConvBufType is uint16_t
            else:
                a = cb[i:i + hh, j:j + ww].astype(np.int64)
                t = (a * fwd + s * bck) >> 4 if jnt else (a + s) >> 1
                t = t - (1 << (offset_bits - r1)) - (1 << (offset_bits - r1 - 1))
                v = np.clip(rpot(t, round_bits), 0, (1 << bd) - 1)
            out[i:i + hh, j:j + ww] = v
    return out


def warp_pred(refs, p_col, p_row, p_width, p_height, ssx, ssy, bd, compound=0, fwd=0, bck=0):
    """what svt_hip_warp_pred_batch leaves in a block: refs = [(plane, mat, shear, width, height)] (one or two)"""
    if compound == 0:
        r0, r1 = conv_rounds(bd, False)
        pl, mat, shear, w, h = refs[0]
        return warp_affine(pl, mat, shear, w, h, p_col, p_row, p_width, p_height, ssx, ssy, bd, r0, r1)
    r0, r1 = conv_rounds(bd, True)
    pl, mat, shear, w, h = refs[0]
    cb = warp_affine(pl, mat, shear, w, h, p_col, p_row, p_width, p_height, ssx, ssy, bd, r0, r1, True, False)
    pl, mat, shear, w, h = refs[1]
    return warp_affine(pl, mat, shear, w, h, p_col, p_row, p_width, p_height, ssx, ssy, bd, r0, r1, True, True, compound == 2, fwd, bck, cb)


def read_rect(mat, width, height, p_col, p_row, p_width, p_height, ssx, ssy):
    """x_lo, x_hi, y_lo, y_hi: the bounding rectangle of the samples a call can read after clamping"""
    xs, ys = [], []
    for i in range(0, p_height, 8):
        for j in range(0, p_width, 8):
            ix4, _, iy4, _ = tile_projection([int(v) for v in mat], ssx, ssy, p_col + j, p_row + i)
            xs += [clamp(ix4 - 7, 0, width - 1), clamp(ix4 + 7, 0, width - 1)]
            ys += [clamp(iy4 - 7, 0, height - 1), clamp(iy4 + 7, 0, height - 1)]
    return min(xs), max(xs), min(ys), max(ys)


# ---- the model fit --------------------------------------------------------------------------------------------------------------------------------------
def _msb(v):
    return int(v).bit_length() - 1


def resolve_divisor(d):
    """resolve_divisor_64 / _32: the table entry for the eight bits below d's top bit, and the shift that goes with it"""
    s = _msb(d)
    e = d - (1 << s)
    f = rpot(e, s - 8) if s > 8 else e << (8 - s)
    return int(DIV_LUT[f]), s + 14


def get_shear_params(mat):
    """svt_get_shear_params: (alpha, beta, gamma, delta) or None when the C returns 0"""
    mat = [int(v) for v in mat]
    if mat[2] <= 0:
        return None
    alpha = clamp(mat[2] - 65536, -32768, 32767)
    beta = clamp(mat[3], -32768, 32767)
    y, shift = resolve_divisor(mat[2])
    gamma = clamp(i32(rpot_signed(mat[4] * 65536 * y, shift)), -32768, 32767)
    delta = clamp(mat[5] - i32(rpot_signed(mat[3] * mat[4] * y, shift)) - 65536, -32768, 32767)
    sh = tuple(i16(rpot_signed(v, 6) * 64) for v in (alpha, beta, gamma, delta))
    return sh if shear_allowed(*sh) else None


def _ls_square(a):
    return i32(a * a * 4 + a * 4 * 8 + 8 * 8 * 2) >> 4


def _ls_product1(a, b):
    return i32(a * b * 4 + (a + b) * 2 * 8 + 8 * 8) >> 4


def _ls_product2(a, b):
    return i32(a * b * 4 + (a + b) * 2 * 8 + 8 * 8 * 2) >> 4


def find_projection(np_, pts, pts_inref, bsize, mv_row, mv_col, mi_row, mi_col, trace=None):
    """svt_find_projection: (wmmat[6], (alpha, beta, gamma, delta)) or None when it returns 1.  trace (a dict) receives det, the shift after WARPEDMODEL_PREC_BITS is
    taken off, and whether a translation clamp bound"""
    bw, bh = BW[bsize], BH[bsize]
    rsuy, rsux = max(bh, 4) // 2 - 1, max(bw, 4) // 2 - 1
    suy, sux = rsuy * 8, rsux * 8
    duy, dux = suy + mv_row, sux + mv_col
    isuy, isux = mi_row * 4 + rsuy, mi_col * 4 + rsux
    a00 = a01 = a11 = bx0 = bx1 = by0 = by1 = 0
    for k in range(np_):
        dx, dy = int(pts_inref[2 * k]) - dux, int(pts_inref[2 * k + 1]) - duy
        sx, sy = int(pts[2 * k]) - sux, int(pts[2 * k + 1]) - suy
        if abs(sx - dx) < 256 and abs(sy - dy) < 256:
            a00 = i32(a00 + _ls_square(sx))
            a01 = i32(a01 + _ls_product1(sx, sy))
            a11 = i32(a11 + _ls_square(sy))
            bx0 = i32(bx0 + _ls_product2(sx, dx))
            bx1 = i32(bx1 + _ls_product1(sy, dx))
            by0 = i32(by0 + _ls_product1(sx, dy))
            by1 = i32(by1 + _ls_product2(sy, dy))
    det = a00 * a11 - a01 * a01
    if trace is not None:
        trace["det"] = det
    if det == 0:
        return None
    lut, shift = resolve_divisor(abs(det))
    i_det = i16(lut * (-1 if det < 0 else 1))
    shift -= 16
    if trace is not None:
        trace["shift"] = shift
    if shift < 0:
        i_det = i16(i_det * (1 << -shift))  # the int16_t's own left shift: 16384 << 2 becomes 0
        shift = 0
    px0, px1 = a11 * bx0 - a01 * bx1, -a01 * bx0 + a00 * bx1
    py0, py1 = a11 * by0 - a01 * by1, -a01 * by0 + a00 * by1
    m = [0] * 6
    m[2] = clamp(rpot_signed64(i64(px0 * i_det), shift), 65536 - 8192 + 1, 65536 + 8192 - 1)
    m[3] = clamp(rpot_signed64(i64(px1 * i_det), shift), -8192 + 1, 8192 - 1)
    m[4] = clamp(rpot_signed64(i64(py0 * i_det), shift), -8192 + 1, 8192 - 1)
    m[5] = clamp(rpot_signed64(i64(py1 * i_det), shift), 65536 - 8192 + 1, 65536 + 8192 - 1)
    vx = i32(mv_col * 8192 - (isux * (m[2] - 65536) + isuy * m[3]))
    vy = i32(mv_row * 8192 - (isux * m[4] + isuy * (m[5] - 65536)))
    m[0], m[1] = clamp(vx, -TRANS_CLAMP, TRANS_CLAMP - 1), clamp(vy, -TRANS_CLAMP, TRANS_CLAMP - 1)
    if trace is not None:
        trace["trans_clamped"] = m[0] != vx or m[1] != vy
    sh = get_shear_params(m)
    return None if sh is None else (m, sh)


def model_sample_set(g, kind="random"):
    """one argument set of svt_find_projection: dict(np, pts[16], pts_inref[16], bsize, mv_row, mv_col, mi_row, mi_col).  Samples as the neighbour scan makes them: 1/8
    sample positions around the block, the reference positions displaced by a small affine motion plus noise"""
    bsize = int(g.integers(3, 16))  # 8x8 .. 128x128
    bw, bh = BW[bsize], BH[bsize]
    n = int(g.integers(1, 9))
    pts = np.zeros(16, np.int64)
    cx, cy = (max(bw, 4) // 2 - 1) * 8, (max(bh, 4) // 2 - 1) * 8  # (|pts - centre| stays below 1000: the range the C's own LS_MAT asserts allow for eight samples)
    pts[0:2 * n:2] = np.clip(g.integers(-bw * 8, 2 * bw * 8, n), cx - 1000, cx + 1000)
    pts[1:2 * n:2] = np.clip(g.integers(-bh * 8, 2 * bh * 8, n), cy - 1000, cy + 1000)
    mv_row, mv_col = int(g.integers(-200, 201)), int(g.integers(-200, 201))
    a, b, c, d = 1 + g.normal(0, 0.03), g.normal(0, 0.03), g.normal(0, 0.03), 1 + g.normal(0, 0.03)
    ref = np.zeros(16, np.int64)
    ref[0:2 * n:2] = np.round(a * pts[0:2 * n:2] + b * pts[1:2 * n:2]) + mv_col + g.integers(-6, 7, n)
    ref[1:2 * n:2] = np.round(c * pts[0:2 * n:2] + d * pts[1:2 * n:2]) + mv_row + g.integers(-6, 7, n)
    s = dict(np=n, pts=pts, pts_inref=ref, bsize=bsize, mv_row=mv_row, mv_col=mv_col, mi_row=int(g.integers(0, 270)), mi_col=int(g.integers(0, 480)))
    if kind == "rejected":  # every sample fails the LS_MV_MAX test: all sums stay 0, det == 0
        s["pts_inref"][:2 * n] = s["pts"][:2 * n] + np.tile([mv_col + 300, mv_row - 300], n)
    elif kind == "wrapped":  # coordinates so large that the int32_t LS sums wrap: determinants of either sign.  Outside what the C accepts (its asserts fire): kernel against restatement only
        s["pts"][:2 * n] = g.integers(23000, 60000, 2 * n) * g.choice([-1, 1], 2 * n)
        s["pts_inref"][:2 * n] = s["pts"][:2 * n] + np.tile([mv_col, mv_row], n) + g.integers(-6, 7, 2 * n)
    elif kind == "single":  # one sample next to the centre: the smallest determinants the sums can make
        s["np"] = 1
        off = (int(g.integers(-6, 3)), int(g.integers(-6, 3)))
        s["pts"][:2] = (cx + off[0], cy + off[1])
        s["pts_inref"][:2] = (cx + off[0] + mv_col + int(g.integers(-2, 3)), cy + off[1] + mv_row + int(g.integers(-2, 3)))
    elif kind == "far":  # a block far from the origin with a strong zoom: the translation clamp binds
        s["mi_row"], s["mi_col"] = int(g.integers(2000, 4000)), int(g.integers(2000, 4000))
        s["pts_inref"][:2 * n] = np.round(1.12 * s["pts"][:2 * n]).astype(np.int64) + np.tile([mv_col, mv_row], n)
    return s


# ---- the warp error -------------------------------------------------------------------------------------------------------------------------------------
def warp_error(ref, mat, shear, width, height, src, p_col, p_row, p_width, p_height, ssx, ssy, chess, best_error=None):
    """warp_error (enc_warped_motion.c): the SAD over the 32x32 error blocks against src (a 2-D array, [y, x] = sample (x, y)); with best_error the C's early return
    of the partial sum is taken too"""
    total = 0
    bw, bh = min(p_width, 32), min(p_height, 32)
    for it, i in enumerate(range(p_row, p_row + p_height, 32)):
        jstart, jstep = (p_col if it & 1 else p_col + 32), 2
        if not chess:
            jstart, jstep = p_col, 1
        for j in range(jstart, p_col + p_width, jstep * 32):
            ww, hh = min(bw, p_col + p_width - j), min(bh, p_row + p_height - i)
            w = warp_affine(ref, mat, shear, width, height, j, i, ww, hh, ssx, ssy, 8, 3, 11)
            total += int(np.abs(w - src[i:i + hh, j:j + ww].astype(np.int64)).sum())
            if best_error is not None and total > best_error:
                return total
    return total * 2 if chess else total


# ---- shared test material -------------------------------------------------------------------------------------------------------------------------------
CLASSES = ("random", "flat", "extreme")


def make_picture(g, kind, width, height, stride, bd):
    """a (height, stride) plane whose first `width` columns are the picture; the padding columns hold a value no picture sample has at `flat`"""
    dt = np.uint16 if bd > 8 else np.uint8
    mx = (1 << bd) - 1
    a = np.full((height, stride), 3, dt)
    if kind == "random":
        a[:, :width] = g.integers(0, mx + 1, (height, width))
    elif kind == "flat":
        a[:, :width] = int(g.integers(mx // 4, mx // 2))
    else:
        a[:, :width] = ((np.add.outer(np.arange(height), np.arange(width)) & 1) * mx).astype(dt)
    return a


def rotzoom(angle_q16, zoom_q16, tx, ty):
    """a ROTZOOM model after svt_warp_plane's fix-up: mat[5] = mat[2], mat[4] = -mat[3]"""
    return [tx, ty, zoom_q16, angle_q16, -angle_q16, zoom_q16]


def models():
    """name -> (mat, shear): shears from get_shear_params where the model is one a real caller has, chosen by hand where the test wants a limit of the filter"""
    out = {}
    for name, mat in (("translation", [5 * 65536 + 20000, -3 * 65536 + 47001, 65536, 0, 0, 65536]),
                      ("zoom", [-40000, 70000, 65536 + 5000, 0, 0, 65536 + 5000]),
                      ("shrink", [90000, 10000, 65536 - 6000, 0, 0, 65536 - 6000]),
                      ("rotation", rotzoom(3300, 65536 - 83, 3 * 65536, -2 * 65536)),
                      ("rotation_neg", rotzoom(-4100, 65536 - 128, -65536, 4 * 65536 + 999)),
                      ("affine", [123456, -234567, 65536 + 2100, -1800, 2500, 65536 - 3100]),
                      ("affine_neg", [-77777, 31000, 65536 - 4000, -3000, -2800, 65536 - 2000])):
        sh = get_shear_params(mat)
        assert sh is not None, name
        out[name] = (mat, sh)
    assert all(v < 0 for v in out["affine_neg"][1])
    # one quantisation step (64) inside each shear limit; the fraction of the translation makes sx / sy reach the first and the last table row
    out["alpha_limit_row0"] = ([100, 65400, 65536, 0, 0, 65536], (16320, 0, -16320, 0))
    out["alpha_limit_row192"] = ([65400, 100, 65536, 0, 0, 65536], (-16320, 0, 16320, 0))
    out["beta_limit"] = ([2 * 65536 + 65500, 30, 65536, 0, 0, 65536], (0, 9344, 0, 16320))
    out["beta_neg_limit"] = ([30, 65500, 65536, 0, 0, 65536], (64, -9280, 8192, -8128))
    further = {"alpha_limit_row0": [(16384, 0, -16320, 0), (16320, 0, -16384, 0)], "alpha_limit_row192": [(-16384, 0, 16320, 0), (-16320, 0, 16384, 0)],
               "beta_limit": [(0, 9408, 0, 16320), (0, 9344, 0, 16384)], "beta_neg_limit": [(64, -9344, 8192, -8128), (64, -9280, 8192, -8192)]}
    for name, worse in further.items():  # one step of 64 further in either pair is no longer allowed
        assert shear_allowed(*out[name][1]) and not any(shear_allowed(*w) for w in worse), name
    return out


def load_golden():
    return np.load(GOLDEN_FILE)


def golden_warp_cases():
    """(model, bd, p_col, p_row, p_width, p_height, ssx, ssy, compound, fwd, bck, second model): the cases of tests/golden/warp.npz, on golden_picture(bd)"""
    names = list(models())
    cases = []
    k = 0
    for bd in (8, 10, 12):
        for (pw, ph) in ((8, 8), (16, 8), (12, 20), (4, 4), (1, 1), (14, 6)):
            for pos in ((16, 16), (-6, 20), (60, 50), (-40, -40)):
                ssx, ssy = ((0, 0), (1, 1), (1, 0), (0, 1))[k % 4]
                comp = k % 3
                fwd, bck = ((9, 7), (11, 5), (12, 4), (13, 3))[k % 4]
                cases.append((names[k % len(names)], bd, pos[0] + k % 5, pos[1] + k % 3, pw, ph, ssx, ssy, comp, fwd, bck, names[(k + 3) % len(names)]))
                k += 1
    return cases


GOLDEN_W, GOLDEN_H, GOLDEN_STRIDE = 72, 56, 77


def golden_picture(bd, which=0):
    return make_picture(np.random.default_rng(GOLDEN_SEED + bd + 100 * which), "random", GOLDEN_W, GOLDEN_H, GOLDEN_STRIDE, bd)


def golden_model_sets():
    g = np.random.default_rng(GOLDEN_SEED)
    kinds = ["random"] * 40 + ["rejected"] * 4 + ["single"] * 10 + ["far"] * 10
    return [model_sample_set(g, k) for k in kinds]


def golden_error_cases():
    """(model, width, height, p_col, p_row, p_width, p_height, ss, chess)"""
    return [("translation", 72, 56, 0, 0, 72, 56, 0, 0), ("rotation", 72, 56, 0, 0, 72, 56, 0, 1), ("affine", 72, 56, 0, 0, 70, 50, 0, 1), ("zoom", 72, 56, 0, 0, 36, 28, 1, 0),
            ("affine_neg", 72, 56, 0, 0, 20, 12, 0, 0), ("shrink", 72, 56, 0, 0, 36, 28, 1, 1)]
