"""AV1 intra prediction restated in numpy: build_intra_predictors / build_intra_predictors_high (enc_intra_prediction.c:60-435) with everything they call --
svt_av1_filter_intra_edge[_high]_c, filter_intra_edge_corner[_high], svt_av1_upsample_intra_edge[_high]_c, svt_av1_[highbd_]dr_prediction_z{1,2,3}_c, the sized
dc / dc_top / dc_left / dc_128 / v / h / smooth / smooth_v / smooth_h / paeth predictors, svt_av1_filter_intra_predictor_c -- and the chroma-from-luma trio
(svt_cfl_luma_subsampling_420_*, svt_subtract_average_c, svt_cfl_predict_*).  What is restated is what the C NARROWS, not what the specification says: the working
arrays are modelled as the C declares them, pre-filled with bytes 0x80 (0x8080 per uint16_t), every access checked against their bounds, so an entry the C reads
without having written it comes out as the C's value.  This is the checker of tests/test_intrapred.py (where the reference's sources do not exist);
tests/test_intrapred_ref.py pins it on the reference's own functions and tables."""
import os

import numpy as np

DC, V, H, D45, D135, D113, D157, D203, D67, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH = range(13)
FILTER_INTRA_OFF = 5
MODE_TO_ANGLE = (0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0)
ANGLE_STEP = 3
NEED_LEFT, NEED_ABOVE, NEED_ABOVERIGHT, NEED_ABOVELEFT, NEED_BOTTOMLEFT = 2, 4, 8, 16, 32
EXTEND_MODES = (NEED_ABOVE | NEED_LEFT, NEED_ABOVE, NEED_LEFT, NEED_ABOVE | NEED_ABOVERIGHT, NEED_LEFT | NEED_ABOVE | NEED_ABOVELEFT,
                NEED_LEFT | NEED_ABOVE | NEED_ABOVELEFT, NEED_LEFT | NEED_ABOVE | NEED_ABOVELEFT, NEED_LEFT | NEED_BOTTOMLEFT, NEED_ABOVE | NEED_ABOVERIGHT,
                NEED_LEFT | NEED_ABOVE, NEED_LEFT | NEED_ABOVE, NEED_LEFT | NEED_ABOVE, NEED_LEFT | NEED_ABOVE | NEED_ABOVELEFT)

# TxSize -> (w, h): tx_size_wide / tx_size_high
TX_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4), (8, 32), (32, 8),
            (16, 64), (64, 16)]
CFL_SIZES = [(4, 4), (4, 8), (4, 16), (8, 4), (8, 8), (8, 16), (8, 32), (16, 4), (16, 8), (16, 16), (16, 32), (32, 8), (32, 16), (32, 32)]  # CFL_SUB_AVG_FN
CFL_BUF_LINE = 32

SM_WEIGHTS = np.array(
    [0, 0, 255, 128, 255, 149, 85, 64, 255, 197, 146, 105, 73, 50, 37, 32, 255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
     255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
     255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
     65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4], np.int64)
_DR = {3: 1023, 6: 547, 9: 372, 14: 273, 17: 215, 20: 178, 23: 151, 26: 132, 29: 116, 32: 102, 36: 90, 39: 80, 42: 71, 45: 64, 48: 57, 51: 51, 54: 45, 58: 40, 61: 35,
       64: 31, 67: 27, 70: 23, 73: 19, 76: 15, 81: 11, 84: 7, 87: 3}
DR_DERIVATIVE = np.array([_DR.get(a, 0) for a in range(90)], np.int64)
FILTER_INTRA_TAPS = np.array([
    [[-6, 10, 0, 0, 0, 12, 0, 0], [-5, 2, 10, 0, 0, 9, 0, 0], [-3, 1, 1, 10, 0, 7, 0, 0], [-3, 1, 1, 2, 10, 5, 0, 0], [-4, 6, 0, 0, 0, 2, 12, 0], [-3, 2, 6, 0, 0, 2, 9, 0],
     [-3, 2, 2, 6, 0, 2, 7, 0], [-3, 1, 2, 2, 6, 3, 5, 0]],
    [[-10, 16, 0, 0, 0, 10, 0, 0], [-6, 0, 16, 0, 0, 6, 0, 0], [-4, 0, 0, 16, 0, 4, 0, 0], [-2, 0, 0, 0, 16, 2, 0, 0], [-10, 16, 0, 0, 0, 0, 10, 0],
     [-6, 0, 16, 0, 0, 0, 6, 0], [-4, 0, 0, 16, 0, 0, 4, 0], [-2, 0, 0, 0, 16, 0, 2, 0]],
    [[-8, 8, 0, 0, 0, 16, 0, 0], [-8, 0, 8, 0, 0, 16, 0, 0], [-8, 0, 0, 8, 0, 16, 0, 0], [-8, 0, 0, 0, 8, 16, 0, 0], [-4, 4, 0, 0, 0, 0, 16, 0], [-4, 0, 4, 0, 0, 0, 16, 0],
     [-4, 0, 0, 4, 0, 0, 16, 0], [-4, 0, 0, 0, 4, 0, 16, 0]],
    [[-2, 8, 0, 0, 0, 10, 0, 0], [-1, 3, 8, 0, 0, 6, 0, 0], [-1, 2, 3, 8, 0, 4, 0, 0], [0, 1, 2, 3, 8, 2, 0, 0], [-1, 4, 0, 0, 0, 3, 10, 0], [-1, 3, 4, 0, 0, 4, 6, 0],
     [-1, 2, 3, 4, 0, 4, 4, 0], [-1, 2, 2, 3, 4, 3, 3, 0]],
    [[-12, 14, 0, 0, 0, 14, 0, 0], [-10, 0, 14, 0, 0, 12, 0, 0], [-9, 0, 0, 14, 0, 11, 0, 0], [-8, 0, 0, 0, 14, 10, 0, 0], [-10, 12, 0, 0, 0, 0, 14, 0],
     [-9, 1, 12, 0, 0, 0, 12, 0], [-8, 0, 0, 12, 0, 1, 11, 0], [-7, 0, 0, 1, 12, 1, 9, 0]]], np.int64)


class Edge:
    """one of the C's working arrays (above_data / left_data): `size` entries pre-filled with the byte 0x80, addressed relative to `org` as above_row / left_col are;
    a read or write outside the array is an error here, where in C it would be a stray stack access"""

    def __init__(self, bd, values=None, lo=0):
        if bd == 8:
            self.size, self.org, fill = 64 * 2 + 48, 32, 0x80
        else:
            self.size, self.org, fill = 64 * 2 + 32, 16, 0x8080
        self.a = np.full(self.size, fill, np.int64)
        if values is not None:  # a caller's prepared edge: values[k] is entry lo + k
            self[lo:lo + len(values)] = np.asarray(values, np.int64)

    def _ix(self, i):
        if isinstance(i, slice):
            assert i.step is None and 0 <= i.start + self.org and i.stop + self.org <= self.size, (i, self.size)
            return slice(i.start + self.org, i.stop + self.org)
        j = np.asarray(i) + self.org
        assert np.all(j >= 0) and np.all(j < self.size), (np.min(j), np.max(j), self.size)
        return j

    def __getitem__(self, i):
        return self.a[self._ix(i)]

    def __setitem__(self, i, v):
        self.a[self._ix(i)] = v


def edge_filter_strength(bs0, bs1, delta, ftype):
    """svt_aom_intra_edge_filter_strength (intra_prediction.c:180-243)"""
    d, wh, s = abs(delta), bs0 + bs1, 0
    if ftype == 0:
        if wh <= 8:
            s = 1 if d >= 56 else 0
        elif wh <= 16:
            s = 1 if d >= 40 else 0
        elif wh <= 24:
            s = 3 if d >= 32 else 2 if d >= 16 else 1 if d >= 8 else 0
        elif wh <= 32:
            s = 3 if d >= 32 else 2 if d >= 4 else 1 if d >= 1 else 0
        else:
            s = 3 if d >= 1 else 0
    else:
        if wh <= 8:
            s = 2 if d >= 64 else 1 if d >= 40 else 0
        elif wh <= 16:
            s = 2 if d >= 48 else 1 if d >= 20 else 0
        elif wh <= 24:
            s = 3 if d >= 4 else 0
        else:
            s = 3 if d >= 1 else 0
    return s


def use_upsample(bs0, bs1, delta, ftype):
    """svt_aom_use_intra_edge_upsample (:146-152)"""
    d = abs(delta)
    if d <= 0 or d >= 40:
        return 0
    return int(bs0 + bs1 <= 8) if ftype else int(bs0 + bs1 <= 16)


EDGE_KERNELS = ((0, 4, 8, 4, 0), (0, 5, 6, 5, 0), (2, 4, 4, 4, 2))


def filter_edge(e, p, sz, strength, bd):
    """svt_av1_filter_intra_edge[_high]_c on e[p .. p + sz): reads a snapshot copy; entry 0 is a tap input and is never written; taps clamped to [0, sz - 1]"""
    if not strength:
        return
    snap = e[p:p + sz].copy()
    i = np.arange(1, sz)
    s = np.zeros(sz - 1, np.int64)
    for j, k in enumerate(EDGE_KERNELS[strength - 1]):
        s += snap[np.clip(i - 2 + j, 0, sz - 1)] * k
    e[p + 1:p + sz] = ((s + 8) >> 4) & ((1 << (8 if bd == 8 else 16)) - 1)  # (uint8_t) / (uint16_t)


def filter_corner(above, left):
    """filter_intra_edge_corner[_high] (:2293, :2415)"""
    s = (int(left[0]) * 5 + int(above[-1]) * 6 + int(above[0]) * 5 + 8) >> 4
    above[-1] = s
    left[-1] = s


def upsample_edge(e, sz, bd):
    """svt_av1_upsample_intra_edge[_high]_c (C_DEFAULT/intra_prediction_c.c:14-55): in[0] = in[1] = p[-1]; writes p[-2 .. 2 sz - 2]; clips to 8 bits / bd"""
    assert sz <= 16
    inn = np.concatenate([[e[-1], e[-1]], e[0:sz], [e[sz - 1]]]).astype(np.int64)
    e[-2] = inn[0]
    i = np.arange(sz)
    s = np.clip((-inn[i] + 9 * inn[i + 1] + 9 * inn[i + 2] - inn[i + 3] + 8) >> 4, 0, (1 << bd) - 1)
    e[2 * i - 1] = s
    e[2 * i] = inn[i + 2]


def dr_z1(above, w, h, up, dx, bd):
    """svt_av1_[highbd_]dr_prediction_z1_c: base < max_base_x per sample, otherwise above[max_base_x]"""
    r, c = np.mgrid[0:h, 0:w]
    mb = (w + h - 1) << up
    x = (r + 1) * dx
    base = (x >> (6 - up)) + (c << up)
    shift = ((x << up) & 0x3F) >> 1
    ok = base < mb
    b = np.where(ok, base, 0)
    val = np.clip((above[b] * (32 - shift) + above[b + 1] * shift + 16) >> 5, 0, (1 << bd) - 1)
    return np.where(ok, val, above[mb])


def dr_z3(left, w, h, up, dy, bd):
    return dr_z1(left, h, w, up, dy, bd).T


def dr_z2(above, left, w, h, upa, upl, dx, dy, bd):
    """svt_av1_[highbd_]dr_prediction_z2_c: negative x, y through arithmetic >> and & 0x3F on two's complement (numpy's int64 does both the same way)"""
    r, c = np.mgrid[0:h, 0:w]
    x = (c << 6) - (r + 1) * dx
    b1 = x >> (6 - upa)
    s1 = ((x * (1 << upa)) & 0x3F) >> 1
    y = (r << 6) - (c + 1) * dy
    b2 = y >> (6 - upl)
    s2 = ((y * (1 << upl)) & 0x3F) >> 1
    use_a = b1 >= -(1 << upa)
    out = np.zeros((h, w), np.int64)
    if use_a.any():
        ba, sa = b1[use_a], s1[use_a]
        out[use_a] = above[ba] * (32 - sa) + above[ba + 1] * sa
    if (~use_a).any():
        bl, sl = b2[~use_a], s2[~use_a]
        assert np.all(bl >= -(1 << upl))  # the C's assertion
        out[~use_a] = left[bl] * (32 - sl) + left[bl + 1] * sl
    return np.clip((out + 16) >> 5, 0, (1 << bd) - 1)


def dr_predictor(above, left, w, h, upa, upl, angle, bd):
    """svt_aom_[highbd_]dr_predictor (:2273, :2372)"""
    if 0 < angle < 90:
        return dr_z1(above, w, h, upa, int(DR_DERIVATIVE[angle]), bd)
    if 90 < angle < 180:
        return dr_z2(above, left, w, h, upa, upl, int(DR_DERIVATIVE[180 - angle]), int(DR_DERIVATIVE[angle - 90]), bd)
    if 180 < angle < 270:
        return dr_z3(left, w, h, upl, int(DR_DERIVATIVE[270 - angle]), bd)
    if angle == 90:
        return v_pred(above, left, w, h)
    assert angle == 180
    return h_pred(above, left, w, h)


def v_pred(above, left, w, h):
    return np.tile(above[0:w], (h, 1))


def h_pred(above, left, w, h):
    return np.tile(left[0:h][:, None], (1, w))


def dc_pred(above, left, w, h, have_top, have_left, bd):
    """svt_aom_[highbd_]dc{,_top,_left,_128}_predictor: plain integer division with + (count >> 1)"""
    if not have_top and not have_left:
        v = 128 << (bd - 8)
    else:
        s = (int(above[0:w].sum()) if have_top else 0) + (int(left[0:h].sum()) if have_left else 0)
        n = (w if have_top else 0) + (h if have_left else 0)
        v = (s + (n >> 1)) // n
    return np.full((h, w), v, np.int64)


def smooth_pred(above, left, w, h):
    wh, ww = SM_WEIGHTS[h:2 * h][:, None], SM_WEIGHTS[w:2 * w][None, :]
    p = wh * above[0:w][None, :] + ((256 - wh) & 0xFF) * int(left[h - 1]) + ww * left[0:h][:, None] + ((256 - ww) & 0xFF) * int(above[w - 1])
    return (p + 256) >> 9  # divide_round(.., 1 + sm_weight_log2_scale)


def smooth_v_pred(above, left, w, h):
    wh = SM_WEIGHTS[h:2 * h][:, None]
    return (wh * above[0:w][None, :] + ((256 - wh) & 0xFF) * int(left[h - 1]) + 128 + np.zeros((h, w), np.int64)) >> 8


def smooth_h_pred(above, left, w, h):
    ww = SM_WEIGHTS[w:2 * w][None, :]
    return (ww * left[0:h][:, None] + ((256 - ww) & 0xFF) * int(above[w - 1]) + 128 + np.zeros((h, w), np.int64)) >> 8


def paeth_pred(above, left, w, h):
    """ties: left, then top, then top-left"""
    tl = int(above[-1])
    lf, tp = np.broadcast_arrays(left[0:h][:, None], above[0:w][None, :])
    base = tp + lf - tl
    pl, pt, ptl = np.abs(base - lf), np.abs(base - tp), np.abs(base - tl)
    return np.where((pl <= pt) & (pl <= ptl), lf, np.where(pt <= ptl, tp, tl))


def rpot_signed(v, n):
    """ROUND_POWER_OF_TWO_SIGNED: half away from zero"""
    v = np.asarray(v, np.int64)
    return np.where(v < 0, -((-v + (1 << (n - 1))) >> n), (v + (1 << (n - 1))) >> n)


def filter_intra_pred(above, left, w, h, mode, bd):
    """svt_av1_filter_intra_predictor_c / svt_aom_highbd_filter_intra_predictor: 4x2 patches in raster order, each sample clipped before it feeds the next patch"""
    assert w <= 32 and h <= 32
    buf = np.zeros((33, 33), np.int64)
    buf[1:h + 1, 0] = left[0:h]
    buf[0, 0:w + 1] = above[-1:w]
    taps = FILTER_INTRA_TAPS[mode][:, :7]
    for r in range(1, h + 1, 2):
        for c in range(1, w + 1, 4):
            p = np.array([buf[r - 1, c - 1], buf[r - 1, c], buf[r - 1, c + 1], buf[r - 1, c + 2], buf[r - 1, c + 3], buf[r, c - 1], buf[r + 1, c - 1]], np.int64)
            buf[r:r + 2, c:c + 4] = np.clip(rpot_signed(taps @ p, 4), 0, (1 << bd) - 1).reshape(2, 4)
    return buf[1:h + 1, 1:w + 1].copy()


def build_intra_predictors(top, left_ref, w, h, mode, angle_delta, filter_intra_mode, n_top_px, n_topright_px, n_left_px, n_bottomleft_px, disable_edge_filter, filt_type,
                           bd):
    """build_intra_predictors (bd 8) / build_intra_predictors_high (bd 10, 12), statement by statement.  top[k] is above_ref[k - 1] (top[0] the corner), left_ref[i]
    the i-th left neighbour (ref_stride is 1 in the C; a strided caller gathers first).  Entries of either that the C would not read may be absent."""
    top, left_ref = np.asarray(top, np.int64), np.asarray(left_ref, np.int64)
    above_ref = lambda k: int(top[k + 1])  # noqa: E731
    above_row, left_col = Edge(bd), Edge(bd)
    need_left, need_above, need_al = EXTEND_MODES[mode] & NEED_LEFT, EXTEND_MODES[mode] & NEED_ABOVE, EXTEND_MODES[mode] & NEED_ABOVELEFT
    p_angle = 0
    is_dr = V <= mode <= D67
    use_fi = filter_intra_mode != FILTER_INTRA_OFF
    base = 128 << (bd - 8)
    if is_dr:
        p_angle = MODE_TO_ANGLE[mode] + angle_delta * ANGLE_STEP
        if p_angle <= 90:
            need_above, need_left, need_al = 1, 0, 1
        elif p_angle < 180:
            need_above, need_left, need_al = 1, 1, 1
        else:
            need_above, need_left, need_al = 0, 1, 1
    if use_fi:
        need_left = need_above = need_al = 1
    if (not need_above and n_left_px == 0) or (not need_left and n_top_px == 0):
        if need_left:
            val = above_ref(0) if n_top_px > 0 else base + 1
        else:
            val = int(left_ref[0]) if n_left_px > 0 else base - 1
        return np.full((h, w), val, np.int64)
    if need_left:
        need_bottom = int(bool(EXTEND_MODES[mode] & NEED_BOTTOMLEFT))
        if use_fi:
            need_bottom = 0
        if is_dr:
            need_bottom = int(p_angle > 180)
        num = h + (w if need_bottom else 0)
        i = 0
        if n_left_px > 0:
            left_col[0:n_left_px] = left_ref[0:n_left_px]
            i = n_left_px
            if need_bottom and n_bottomleft_px > 0:
                assert i == h
                left_col[h:h + n_bottomleft_px] = left_ref[h:h + n_bottomleft_px]
                i = h + n_bottomleft_px
            if i < num:
                left_col[i:num] = left_col[i - 1]
        else:
            left_col[0:num] = above_ref(0) if n_top_px > 0 else base + 1
    if need_above:
        need_right = int(bool(EXTEND_MODES[mode] & NEED_ABOVERIGHT))
        if use_fi:
            need_right = 0
        if is_dr:
            need_right = int(p_angle < 90)
        num = w + (h if need_right else 0)
        if n_top_px > 0:
            above_row[0:n_top_px] = top[1:1 + n_top_px]
            i = n_top_px
            if need_right and n_topright_px > 0:
                assert n_top_px == w
                above_row[w:w + n_topright_px] = top[1 + w:1 + w + n_topright_px]
                i += n_topright_px
            if i < num:
                above_row[i:num] = above_row[i - 1]
        else:
            above_row[0:num] = int(left_ref[0]) if n_left_px > 0 else base - 1
    if need_al:
        if n_top_px > 0 and n_left_px > 0:
            above_row[-1] = above_ref(-1)
        elif n_top_px > 0:
            above_row[-1] = above_ref(0)
        elif n_left_px > 0:
            above_row[-1] = int(left_ref[0])
        else:
            above_row[-1] = base
        left_col[-1] = above_row[-1]
    if use_fi:
        return filter_intra_pred(above_row, left_col, w, h, filter_intra_mode, bd)
    if is_dr:
        upa = upl = 0
        if not disable_edge_filter:
            need_right, need_bottom = int(p_angle < 90), int(p_angle > 180)
            if p_angle != 90 and p_angle != 180:
                ab_le = 1 if need_al else 0
                if need_above and need_left and w + h >= 24:
                    filter_corner(above_row, left_col)
                if need_above and n_top_px > 0:
                    filter_edge(above_row, -ab_le, n_top_px + ab_le + (h if need_right else 0), edge_filter_strength(w, h, p_angle - 90, filt_type), bd)
                if need_left and n_left_px > 0:
                    filter_edge(left_col, -ab_le, n_left_px + ab_le + (w if need_bottom else 0), edge_filter_strength(h, w, p_angle - 180, filt_type), bd)
            upa = use_upsample(w, h, p_angle - 90, filt_type)
            if need_above and upa:
                upsample_edge(above_row, w + (h if need_right else 0), bd)
            upl = use_upsample(h, w, p_angle - 180, filt_type)
            if need_left and upl:
                upsample_edge(left_col, h + (w if need_bottom else 0), bd)
        return dr_predictor(above_row, left_col, w, h, upa, upl, p_angle, bd)
    if mode == DC:
        return dc_pred(above_row, left_col, w, h, n_top_px > 0, n_left_px > 0, bd)
    return {SMOOTH: smooth_pred, SMOOTH_V: smooth_v_pred, SMOOTH_H: smooth_h_pred, PAETH: paeth_pred}[mode](above_row, left_col, w, h)


# ---- chroma from luma ----------------------------------------------------------------------------------------------------------------------------------
def i16(v):
    return ((np.asarray(v, np.int64) + 32768) & 0xFFFF) - 32768


def cfl_subsample_420(luma, w, h):
    """svt_cfl_luma_subsampling_420_{lbd,hbd}_c on the 2w x 2h block `luma` -> the w x h int16_t Q3 values"""
    l = np.asarray(luma, np.int64)[:2 * h, :2 * w]
    return i16((l[0::2, 0::2] + l[0::2, 1::2] + l[1::2, 0::2] + l[1::2, 1::2]) << 1)


def cfl_subtract_average(q3, w, h):
    """svt_subtract_average_c with round_offset = (w * h) >> 1 and num_pel_log2 = log2 w + log2 h"""
    q3 = np.asarray(q3, np.int64)
    avg = (int(q3.sum()) + ((w * h) >> 1)) >> (w.bit_length() - 1 + h.bit_length() - 1)
    return i16(q3 - i16(avg))


def cfl_predict(ac, pred, alpha_q3, bit_depth, is8):
    """svt_cfl_predict_{lbd,hbd}_c: ROUND_POWER_OF_TWO_SIGNED(alpha * ac, 6) + (int16_t)pred, clipped to bit_depth (the 8-bit form narrows the clipped value to uint8_t)"""
    v = np.clip(rpot_signed(int(alpha_q3) * np.asarray(ac, np.int64), 6) + i16(pred), 0, (1 << bit_depth) - 1)
    return v & 0xFF if is8 else v


def cfl_full(luma, pred, w, h, alpha_q3, bd):
    """one target of one descriptor of svt_hip_cfl_pred_batch"""
    return cfl_predict(cfl_subtract_average(cfl_subsample_420(luma, w, h), w, h), pred, alpha_q3, bd, bd == 8)


# ---- inputs and case builders ----------------------------------------------------------------------------------------------------------------------------
CLASSES = ("random", "zero", "max", "checker", "ramp")
AVAIL = ("all", "none", "top", "left", "part_top", "part_left", "part_tr", "part_bl")


def make_samples(g, kind, n, bd):
    """n edge samples of one input class"""
    mx = (1 << bd) - 1
    if kind == "random":
        return g.integers(0, mx + 1, n).astype(np.int64)
    if kind == "zero":
        return np.zeros(n, np.int64)
    if kind == "max":
        return np.full(n, mx, np.int64)
    i = np.arange(n)
    if kind == "checker":  # cells of two samples
        return ((i >> 1) & 1) * mx
    return (i * mx) // max(n - 1, 1)  # ramp


def avail_counts(kind, w, h):
    """(n_top_px, n_topright_px, n_left_px, n_bottomleft_px) of an availability class"""
    return {"all": (w, w, h, h), "none": (0, 0, 0, 0), "top": (w, w, 0, 0), "left": (0, 0, h, h), "part_top": (w // 2 + 1, 0, h, h), "part_left": (w, w, h // 2 + 1, 0),
            "part_tr": (w, w // 2 - 1, h, h), "part_bl": (w, w, h, h // 2 - 1)}[kind]


def case(w, h, mode, delta=0, fi=FILTER_INTRA_OFF, avail="all", filt_type=0, disable=0, kind="random"):
    return dict(w=w, h=h, mode=mode, delta=delta, fi=fi, avail=avail, filt_type=filt_type, disable=disable, kind=kind)


def every_case():
    """all 19 sizes x 13 modes x 7 deltas (the C ignores the delta of a non-directional mode; so must the kernel) and the 5 filter-intra modes at w, h <= 32;
    availability classes, filt_type, disable_edge_filter and input classes cycle"""
    out, k = [], 0
    for (w, h) in TX_SIZES:
        for mode in range(13):
            for delta in range(-3, 4):
                out.append(case(w, h, mode, delta, FILTER_INTRA_OFF, AVAIL[k % 8] if k % 3 else "all", (k // 2) & 1, int(k % 5 == 4), CLASSES[k % 5] if k % 4 == 0 else "random"))
                k += 1
        if w <= 32 and h <= 32:
            for fi in range(5):
                out.append(case(w, h, (DC, V, D203, PAETH, D45)[fi] if k % 2 else DC, 0, fi, AVAIL[k % 8] if k % 3 else "all", 0, 0, CLASSES[k % 5] if k % 4 == 0 else "random"))
                k += 1
    return out


def case_inputs(g, c, bd):
    """(top, left): top[0] is the corner, then 2w samples; 2h left samples"""
    return make_samples(g, c["kind"], 1 + 2 * c["w"], bd), make_samples(g, c["kind"], 2 * c["h"], bd)[::-1].copy()


def predict_case(c, top, left, bd):
    nt, ntr, nl, nbl = avail_counts(c["avail"], c["w"], c["h"])
    return build_intra_predictors(top, left, c["w"], c["h"], c["mode"], c["delta"], c["fi"], nt, ntr, nl, nbl, c["disable"], c["filt_type"], bd)


# ---- the golden cases (tests/golden/intrapred.npz: what the reference's C computes for them; written by tests/test_intrapred_ref.py) -------------------------
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "intrapred.npz")
GOLDEN_SEED = 20261


def golden_cases():
    """[(bd, case)]: a fixed subset of every_case(), small blocks only (the file stays small), every mode, every availability class, every filter-intra mode"""
    out = []
    for bd in (8, 10, 12):
        cs = [c for c in every_case() if c["w"] * c["h"] <= 256]
        out += [(bd, c) for c in cs[(bd // 2) % 5::31]]
    return out


def golden_inputs(i, bd, c):
    return case_inputs(np.random.default_rng(GOLDEN_SEED + i), c, bd)


def load_golden():
    return np.load(GOLDEN_FILE)
