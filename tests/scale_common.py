"""numpy restatement of csrc/scale.hip: scaled-reference prediction (svt_av1_[highbd_]convolve_2d_scale_c and the unscaled cases beside it), the non-normative resize
(svt_av1_[highbd_]resize_plane_c) and the normative super-resolution upscale (svt_av1_upscale_normative_rows), plus the position arithmetic a caller of
svt_hip_inter_pred_scaled_batch does (svt_av1_setup_scale_factors_for_frame, scaled_x / scaled_y, the clamp of compute_subpel_params).  Plain integer arithmetic in
int64 with the reference's narrowings spelled out; pinned on the reference's C by tests/test_scale_ref.py.  The tables are read from the text of csrc/scale.hip, the ONE
place they are typed in, and test_scale_ref.py compares every entry with the reference's."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_HIP = os.path.join(ROOT, "svt-av1-psy_amd", "csrc", "scale.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scale.npz")
GOLDEN_SEED = 20261
CLASSES = ("random", "max", "extreme")
WEIGHTS = ((9, 7), (11, 5), (12, 4), (13, 3))  # the four pairs svt_av1_dist_wtd_comp_weight_assign returns (quant_dist_lookup_table, either order)


def _table(name):
    text = open(SCALE_HIP).read()
    m = re.search(r"constexpr int16_t %s((?:\[\d+\])+)\s*=\s*\{(.*?)\};" % name, text, re.S)
    assert m, name
    shape = [int(v) for v in re.findall(r"\[(\d+)\]", m.group(1))]
    return np.array([int(v) for v in re.findall(r"-?\d+", m.group(2))], np.int64).reshape(shape)


UPSCALE_FILTER = _table("kUpscaleFilter")
RESIZE_FILTERS = [UPSCALE_FILTER, _table("kResizeFilter875"), _table("kResizeFilter750"), _table("kResizeFilter625"), _table("kResizeFilter500")]
DOWN2_EVEN, DOWN2_ODD = _table("kDown2SymEven"), _table("kDown2SymOdd")
INTER_FILTERS = _table("kInterFilters")  # [regular, smooth, sharp, bilinear, 4-tap regular / sharp, 4-tap smooth][phase][tap]


def rpot(v, n):
    """ROUND_POWER_OF_TWO on (possibly negative) int64: an arithmetic shift, as the C's on int32_t"""
    return (v + ((1 << n) >> 1)) >> n


def make_picture(g, kind, w, h, stride, bd):
    dt = np.uint16 if bd > 8 else np.uint8
    mx = (1 << bd) - 1
    if kind == "random":
        a = g.integers(0, mx + 1, (h, stride))
    elif kind == "max":
        a = np.full((h, stride), mx)
    else:  # 0 / maximum alternating: both clips and the int16_t narrowing
        a = ((np.add.outer(np.arange(h), np.arange(stride)) & 1) * mx)
    return a.astype(dt)


# ---- position arithmetic ---------------------------------------------------------------------------------------------------------------------------
def setup_scale_factors(other_w, other_h, this_w, this_h):
    """svt_av1_setup_scale_factors_for_frame (inter_prediction.c:186): (x_scale_fp, y_scale_fp, x_step_q4, y_step_q4), or None for an invalid pair"""
    if not (2 * this_w >= other_w and 2 * this_h >= other_h and this_w <= 16 * other_w and this_h <= 16 * other_h):
        return None
    xf, yf = ((other_w << 14) + this_w // 2) // this_w, ((other_h << 14) + this_h // 2) // this_h
    return xf, yf, rpot(xf, 4), rpot(yf, 4)


def is_scaled(sf):
    return sf[0] != 1 << 14 or sf[1] != 1 << 14


def scale_value(val, scale_fp, scaled=True):
    """scaled_x / scaled_y (inter_prediction.c:154, :161), or unscaled_value when the picture pair is not scaled"""
    if not scaled:
        return val << 6
    t = val * scale_fp + (scale_fp - (1 << 14)) * 8
    return -((-t + 128) >> 8) if t < 0 else (t + 128) >> 8  # ROUND_POWER_OF_TWO_SIGNED_64(., REF_SCALE_SHIFT - SCALE_EXTRA_BITS)


def subpel_params(pre_y, pre_x, mv_row, mv_col, sf, frame_w, frame_h, ss_y, ss_x, sb_size=64):
    """the is_scaled branch of compute_subpel_params (enc_inter_prediction.c:3164-3196): (subpel_x, subpel_y, xs, ys, pos_y, pos_x), frame_* the REFERENCE's size"""
    pos_y = scale_value((pre_y << 4) + mv_row * (1 << (1 - ss_y)), sf[1]) + 32
    pos_x = scale_value((pre_x << 4) + mv_col * (1 << (1 - ss_x)), sf[0]) + 32
    border = sb_size * 2 + 32
    pos_y = min(max(pos_y, -(((border >> ss_y) - 8) << 10)), ((frame_h >> ss_y) + 4) << 10)
    pos_x = min(max(pos_x, -(((border >> ss_x) - 8) << 10)), ((frame_w >> ss_x) + 4) << 10)
    return pos_x & 1023, pos_y & 1023, sf[2], sf[3], pos_y >> 10, pos_x >> 10


# ---- A. scaled prediction --------------------------------------------------------------------------------------------------------------------------
def conv_rounds(bd, compound):
    """get_conv_params_no_round (convolve.h:40-64)"""
    r0 = 5 if bd == 12 else 3
    return r0, (7 if compound else 14 - r0)


def filter_rows(filt, dim):
    """av1_get_interp_filter_params_with_block_size (inter_prediction.h:137-145)"""
    if dim <= 4 and filt != 3:
        return INTER_FILTERS[5 if filt == 1 else 4]
    return INTER_FILTERS[filt]


def convolve_2d_scale(pic, oy, ox, w, h, fx, fy, sx, xs, sy, ys, bd, r0, r1):
    """svt_av1_[highbd_]convolve_2d_scale_c up to `CONV_BUF_TYPE res`: pic[oy, ox] is the C's src[0]; fx / fy are 16 x 8 tap tables"""
    im_h = (((h - 1) * ys + sy) >> 10) + 8
    pic, oy, ox = pic[oy - 3:oy + im_h - 3, ox - 3:ox + (((w - 1) * xs + sx) >> 10) + 5].astype(np.int64), 3, 3  # exactly the readable extent
    xq = sx + np.arange(w) * xs
    cols = ox + (xq >> 10)[:, None] - 3 + np.arange(8)[None, :]
    rows = oy - 3 + np.arange(im_h)
    taps = fx[(xq & 1023) >> 6]
    s = (pic[rows[:, None, None], cols[None, :, :]] * taps[None, :, :]).sum(2) + (1 << (bd + 6))
    im = rpot(s, r0).astype(np.int16).astype(np.int64)  # (int16_t)
    yq = sy + np.arange(h) * ys
    tapy = fy[(yq & 1023) >> 6]
    ri = (yq >> 10)[:, None] + np.arange(8)[None, :]
    s = (im[ri] * tapy[:, :, None]).sum(1) + (1 << (bd + 14 - r0))
    return rpot(s, r1) & 0xffff  # CONV_BUF_TYPE


def unscaled_value_block(pic, oy, ox, w, h, fx, fy, px, py, bd, r0, r1, compound):
    """the four cases of svt_aom_convolve[px != 0][py != 0][compound]: the `_sr` value before the clip, or `res` of the jnt_ function (inter_prediction.c:311-668)"""
    top, left = (3 if py else 0), (3 if px else 0)  # read inside the block in a direction that is not filtered
    p = pic[oy - top:oy + h + (4 if py else 0), ox - left:ox + w + (4 if px else 0)].astype(np.int64)
    oy, ox = top, left
    ob = bd + 14 - r0
    ro, rb = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), 14 - r0 - r1
    k = np.arange(8)
    blk = p[oy:oy + h, ox:ox + w]
    if not px and not py:
        return (((blk << rb) + ro) & 0xffff) if compound else blk
    if px and not py:
        s = rpot((p[oy:oy + h, (ox + np.arange(w))[:, None] - 3 + k] * fx[px]).sum(2), r0)
        return (1 << (7 - r1)) * s + ro if compound else rpot(s, 7 - r0)
    if py and not px:
        s = (p[(oy + np.arange(h))[:, None] - 3 + k, ox:ox + w] * fy[py][None, :, None]).sum(1)
        return rpot(s * (1 << (7 - r0)), r1) + ro if compound else rpot(s, 7)
    rows = oy - 3 + np.arange(h + 7)
    s = (p[rows[:, None, None], (ox + np.arange(w))[None, :, None] - 3 + k] * fx[px]).sum(2) + (1 << (bd + 6))
    im = rpot(s, r0).astype(np.int16).astype(np.int64)
    s = (im[np.arange(h)[:, None] + k] * fy[py][None, :, None]).sum(1) + (1 << ob)
    res = rpot(s, r1)
    if compound:
        return res & 0xffff
    res = res - ro
    if bd == 8:
        res = res.astype(np.int16).astype(np.int64)  # the 8-bit function narrows before the last rounding (:345)
    return rpot(res, rb)


def scaled_pred(refs, w, h, filter_x, filter_y, bd, compound=0, fwd=0, bck=0):
    """what svt_hip_inter_pred_scaled_batch leaves in dst for one block.  refs: per reference (pic, oy, ox, subpel_x, subpel_y, xs, ys)"""
    comp = compound != 0
    r0, r1 = conv_rounds(bd, comp)
    ob = bd + 14 - r0
    ro, rb = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), 14 - r0 - r1
    fx, fy = filter_rows(filter_x, w), filter_rows(filter_y, h)
    vals = []
    for (pic, oy, ox, sx, sy, xs, ys) in refs[:2 if comp else 1]:
        if xs != 1024 or ys != 1024:
            v = convolve_2d_scale(pic, oy, ox, w, h, fx, fy, sx, xs, sy, ys, bd, r0, r1)
            if not comp:
                v = rpot(v - ro, rb)
        else:
            assert (sx | sy) & 63 == 0
            v = unscaled_value_block(pic, oy, ox, w, h, fx, fy, sx >> 6, sy >> 6, bd, r0, r1, comp)
        vals.append(v)
    if comp:
        a = vals[0] & 0xffff  # the first reference goes through the ConvBufType buffer
        t = (a * fwd + vals[1] * bck) >> 4 if compound == 2 else (a + vals[1]) >> 1
        out = rpot(t - ro, rb)
    else:
        out = vals[0]
    return np.clip(out, 0, (1 << bd) - 1).astype(np.uint16 if bd > 8 else np.uint8)


def scale_form(pic, oy, ox, w, h, fx, fy, sx, xs, sy, ys, bd, r0, r1, is_compound, do_average, use_dist_wtd, fwd, bck, cb):
    """one call of svt_av1_[highbd_]convolve_2d_scale_c: returns (dst block or None, ConvBufType block or None)"""
    res = convolve_2d_scale(pic, oy, ox, w, h, fx, fy, sx, xs, sy, ys, bd, r0, r1)
    ob = bd + 14 - r0
    ro, rb = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), 14 - r0 - r1
    if is_compound and not do_average:
        return None, res.astype(np.uint16)
    if is_compound:
        t = cb.astype(np.int64)
        t = (t * fwd + res * bck) >> 4 if use_dist_wtd else (t + res) >> 1
    else:
        t = res
    return np.clip(rpot(t - ro, rb), 0, (1 << bd) - 1).astype(np.uint16 if bd > 8 else np.uint8), None


def scaled_extent(w, h, sx, sy, xs, ys):
    """last readable column and row of a scaled reference, relative to src"""
    return (((w - 1) * xs + sx) >> 10) + 4, (((h - 1) * ys + sy) >> 10) + 4


# ---- B. resize -------------------------------------------------------------------------------------------------------------------------------------
def down2_length(length):
    return (length + 1) >> 1


def down2_steps(in_length, out_length):
    steps = 0
    while down2_length(in_length) >= out_length:
        steps += 1
        in_length = down2_length(in_length)
        if in_length == 1:
            break
    return steps


def choose_table(in_length, out_length):
    o16 = out_length * 16
    return 0 if o16 >= in_length * 16 else 1 if o16 >= in_length * 13 else 2 if o16 >= in_length * 11 else 3 if o16 >= in_length * 9 else 4


def down2_symeven(a, mx):
    """svt_av1_[highbd_]down2_symeven_c along the last axis, every index clamped"""
    n = a.shape[-1]
    i = np.arange(0, n, 2)
    s = np.full(a.shape[:-1] + (len(i),), 64, np.int64)
    for j in range(4):
        s += (a[..., np.maximum(i - j, 0)] + a[..., np.minimum(i + 1 + j, n - 1)]) * DOWN2_EVEN[j]
    return np.clip(s >> 7, 0, mx)


def down2_symodd(a, mx):
    n = a.shape[-1]
    i = np.arange(0, n, 2)
    s = 64 + a[..., i] * DOWN2_ODD[0]
    for j in range(1, 4):
        s += (a[..., np.maximum(i - j, 0)] + a[..., np.minimum(i + j, n - 1)]) * DOWN2_ODD[j]
    return np.clip(s >> 7, 0, mx)


def interpolate_core(a, out_length, mx, table=None):
    """svt_av1_[highbd_]interpolate_core_c along the last axis, every index clamped"""
    n = a.shape[-1]
    filt = RESIZE_FILTERS[choose_table(n, out_length)] if table is None else table
    delta = ((n << 14) + out_length // 2) // out_length
    offset = (((n - out_length) << 13) + out_length // 2) // out_length if n > out_length else -((((out_length - n) << 13) + out_length // 2) // out_length)
    y = offset + 128 + np.arange(out_length) * delta
    idx = np.clip((y >> 14)[:, None] - 3 + np.arange(8)[None, :], 0, n - 1)
    s = (a[..., idx] * filt[(y >> 8) & 63]).sum(-1)
    return np.clip(rpot(s, 7), 0, mx)


def resize_multistep(a, olength, mx):
    """resize_multistep (resize.c:350) along the last axis"""
    a = a.astype(np.int64)
    n = a.shape[-1]
    if n == olength:
        return a
    for _ in range(down2_steps(n, olength)):
        a = down2_symodd(a, mx) if a.shape[-1] & 1 else down2_symeven(a, mx)
    return a if a.shape[-1] == olength else interpolate_core(a, olength, mx)


def resize_plane(pic, width2, height2, bd):
    """svt_av1_[highbd_]resize_plane_c: rows, then columns"""
    mx = (1 << bd) - 1
    inter = resize_multistep(pic, width2, mx)
    out = resize_multistep(inter.T, height2, mx).T
    return out.astype(pic.dtype)


# ---- C. upscale ------------------------------------------------------------------------------------------------------------------------------------
def scaled_size(dim, denom):
    """calculate_scaled_size_helper (super_res.c:22) for denom 9 .. 16"""
    return max((dim * 8 + denom // 2) // denom, min(16, dim))


def tile_col_starts(mi_cols, n_tile_cols, sb_mi=16):
    """tile columns at superblock boundaries, none empty, as svt_av1_tile_set_col yields them: n + 1 mi positions"""
    sbs = (mi_cols + sb_mi - 1) // sb_mi
    assert sbs >= n_tile_cols
    return [(j * sbs // n_tile_cols) * sb_mi for j in range(n_tile_cols)] + [mi_cols]


def upscale_rows(src, down_w, up_w, denom, sub_x, starts_mi, bd):
    """svt_av1_upscale_normative_rows: src is rows x (at least the last tile column's end) samples; returns rows x up_w"""
    p = src.astype(np.int64)
    step = ((down_w << 14) + up_w // 2) // up_w
    err = up_w * step - (down_w << 14)
    num = -((up_w - down_w) << 13) + up_w // 2
    cdiv = lambda a, b: -((-a) // b) if a < 0 else a // b  # C division truncates toward zero
    x0 = (cdiv(num, up_w) + 128 - cdiv(err, 2)) & 16383
    sh = 2 - sub_x
    n = len(starts_mi) - 1
    lo, hi = starts_mi[0] << sh, (starts_mi[n] << sh) - 1
    out = np.zeros((p.shape[0], up_w), np.int64)
    for j in range(n):
        dx0, dx1 = starts_mi[j] << sh, starts_mi[j + 1] << sh
        ux0 = dx0 * denom // 8
        ux1 = up_w if j == n - 1 else dx1 * denom // 8
        xq = x0 + np.arange(ux1 - ux0) * step
        idx = np.clip(dx0 - 1 - 3 + (xq >> 14)[:, None] + np.arange(8)[None, :], lo, hi)
        out[:, ux0:ux1] = rpot((p[:, idx] * UPSCALE_FILTER[(xq & 16383) >> 8]).sum(2), 7)
        x0 += (ux1 - ux0) * step - ((dx1 - dx0) << 14)
    return np.clip(out, 0, (1 << bd) - 1).astype(src.dtype)


# ---- the case lists shared by test_scale.py (kernels), test_scale_ref.py (the reference's C) and tools/scale_timing.py ----------------------------------
PRED_SIZES = [(2, 2), (2, 8), (4, 4), (4, 16), (16, 4), (8, 32), (64, 8), (32, 64)]
PRED_STEPS = [(2048, 2048), (1024, 2048), (2048, 1024), (1150, 1150), (1820, 1365), (512, 512), (64, 64), (768, 1798)]
PRED_PHASES = (0, 1023, 512, None)  # None: random


def pred_spec(w, h, refs, fx=0, fy=0, comp=0, wts=(9, 7)):
    """refs: per reference (xs, ys, subpel_x, subpel_y)"""
    return dict(w=w, h=h, refs=list(refs), fx=fx, fy=fy, comp=comp, wts=wts)


def pred_case_list(bd):
    """every size at every step pair, the phases, the sixteen filter pairs, the compound forms and the four weight pairs cycling; the second reference of a compound
    block is scaled by another step pair, unscaled, or scaled alike; then blocks whose references are all unscaled, and one 128 x 128 block at the im_block bound"""
    g = np.random.default_rng(700 + bd)
    specs, k = [], bd

    def phase(j):
        v = PRED_PHASES[(k + j) % 4]
        return int(g.integers(0, 1024)) if v is None else v

    def unscaled():
        return (1024, 1024, 64 * int(g.integers(0, 16)), 64 * int(g.integers(0, 16)))

    for (w, h) in PRED_SIZES:
        for si, (xs, ys) in enumerate(PRED_STEPS):
            k += 1
            first = (xs, ys, phase(0), phase(1))
            kind = (k // 3) % 4
            second = (PRED_STEPS[(si + 3) % 8] + (phase(2), phase(3))) if kind == 0 else unscaled() if kind == 1 else (xs, ys, phase(1), phase(2))
            refs = [first, second]
            if k % 3 and kind == 3:  # (a single reference is always `first`)
                refs = [unscaled(), first] if k % 2 else [second, first]
            specs.append(pred_spec(w, h, refs, k % 4, (k // 4) % 4, k % 3, WEIGHTS[(k // 3) % 4]))
    for (w, h) in PRED_SIZES:  # every reference unscaled: compound 0 / 1 / 2, phases of every case (copy, x, y, 2-D)
        for cs in range(4):
            k += 1
            a = (1024, 1024, 64 * (cs & 1) * (1 + k % 15), 64 * (cs >> 1) * (1 + (k // 2) % 15))
            specs.append(pred_spec(w, h, [a, unscaled()], k % 4, (k // 2) % 4, k % 3, WEIGHTS[k % 4]))
    specs.append(pred_spec(128, 128, [(2048, 2048, 1023, 1023), (1150, 1150, 512, 7)], 0, 2, 1))  # 262 rows: the C's im_block bound
    return specs


def ref_extent(w, h, r):
    """(columns left, columns right of src, rows above, rows below) a reference (xs, ys, sx, sy) may read"""
    xs, ys, sx, sy = r
    if xs != 1024 or ys != 1024:
        ex, ey = scaled_extent(w, h, sx, sy, xs, ys)
        return 3, ex, 3, ey
    return (3 if sx else 0), w - 1 + (4 if sx else 0), (3 if sy else 0), h - 1 + (4 if sy else 0)


RESIZE_PAIRS = [(16, 16), (64, 57), (64, 32), (63, 32), (66, 32), (200, 40), (64, 48), (32, 64), (9, 4), (8, 2), (5, 3), (1, 1)]
UPSCALE_DENOMS = (9, 11, 14, 16)


def upscale_geometry(up_luma, denom, sub_x, n_tile_cols, starts_mi=None):
    """(downscaled plane width, upscaled plane width, tile-column starts in mi) of one plane of a super-res picture"""
    down_luma = scaled_size(up_luma, denom)
    mi_cols = 2 * ((down_luma + 7) >> 3)
    starts = tile_col_starts(mi_cols, n_tile_cols) if starts_mi is None else list(starts_mi)
    return (down_luma + sub_x) >> sub_x, (up_luma + sub_x) >> sub_x, starts, mi_cols, down_luma


GOLDEN_W = GOLDEN_H = 80
# bd, w, h, filter_x, filter_y, compound, weights, references (xs, ys, subpel_x, subpel_y); sources at (3, 3) of the golden pictures 0 and 1
GOLDEN_PRED = [(8, 16, 16, 0, 0, 0, 0, [(2048, 2048, 0, 1023)]), (8, 32, 32, 2, 1, 1, 0, [(2048, 2048, 1023, 1023), (1150, 1150, 512, 77)]),
               (8, 8, 32, 1, 3, 2, 1, [(1150, 1820, 300, 900), (1024, 1024, 192, 0)]), (8, 64, 8, 0, 2, 0, 0, [(1024, 2048, 640, 1)]),
               (8, 4, 4, 2, 2, 2, 3, [(64, 64, 1000, 3), (512, 768, 17, 1023)]), (8, 2, 8, 1, 0, 1, 0, [(1024, 1024, 0, 448), (1798, 768, 5, 600)]),
               (10, 16, 16, 0, 0, 0, 0, [(1820, 1365, 999, 1)]), (10, 32, 32, 2, 1, 2, 2, [(2048, 2048, 1023, 1023), (512, 512, 512, 512)]),
               (10, 4, 16, 1, 3, 1, 0, [(768, 1798, 0, 0), (1024, 1024, 64, 960)]), (10, 64, 8, 3, 2, 0, 0, [(1024, 2048, 31, 800)]),
               (12, 16, 4, 0, 2, 0, 0, [(2048, 1024, 1, 1022)]), (12, 32, 32, 2, 0, 1, 0, [(2048, 2048, 1023, 1023), (1150, 1150, 3, 700)]),
               (12, 8, 32, 1, 1, 2, 1, [(1365, 1820, 100, 200), (1024, 1024, 0, 0)]), (12, 2, 2, 0, 0, 0, 0, [(64, 64, 1023, 1023)])]
# bd, width, height, width2, height2: the top-left corner of golden picture 0
GOLDEN_RESIZE = [(8, 64, 40, 57, 40), (8, 66, 63, 32, 32), (8, 40, 70, 64, 35), (8, 80, 80, 20, 17), (8, 9, 5, 4, 3), (10, 64, 64, 57, 48), (10, 63, 66, 32, 32),
                 (10, 32, 8, 64, 2), (12, 80, 64, 40, 57), (12, 1, 1, 1, 1), (12, 70, 33, 17, 64)]
# bd, sample_bytes, upscaled luma width, denominator, sub_x, tile-column starts in mi (None: one tile column): 6 rows of golden picture 1
GOLDEN_UPSCALE = [(8, 1, 64, 9, 0, None), (8, 1, 120, 14, 0, (0, 4, 12, 18)), (8, 2, 99, 11, 1, None), (8, 1, 128, 16, 0, (0, 8, 16)), (10, 2, 64, 16, 0, None),
                  (10, 2, 121, 14, 1, (0, 4, 12, 18)), (12, 2, 100, 11, 0, (0, 16, 20)), (12, 2, 77, 9, 1, None)]


def golden_picture(bd, k):
    """the two golden pictures of a bit depth: 8-bit random, 12-bit random with extreme runs; the 10-bit pictures are the 12-bit ones >> 2"""
    g = np.random.default_rng(GOLDEN_SEED + (0 if bd == 8 else 1) * 10 + k)
    a = g.integers(0, 256 if bd == 8 else 4096, (GOLDEN_H, GOLDEN_W))
    a[20:24, :] = (np.arange(GOLDEN_W) & 1) * (255 if bd == 8 else 4095)
    a[:, 40:43] = 255 if bd == 8 else 4095
    if bd == 10:
        a >>= 2
    return a.astype(np.uint8 if bd == 8 else np.uint16)


def golden_pred_expect(i):
    bd, w, h, fx, fy, comp, wi, refs = GOLDEN_PRED[i]
    return scaled_pred([(golden_picture(bd, k), 3, 3, r[2], r[3], r[0], r[1]) for k, r in enumerate(refs)], w, h, fx, fy, bd, comp, *WEIGHTS[wi])


def golden_upscale_input(i):
    """(source rows, geometry) of golden upscale case i; 2-byte samples at bit depth 8 hold 8-bit values"""
    bd, sb, up_luma, denom, sub_x, starts = GOLDEN_UPSCALE[i]
    down, up, st, mi_cols, down_luma = upscale_geometry(up_luma, denom, sub_x, 1 if starts is None else len(starts) - 1, starts)
    src = golden_picture(bd, 1)[10:16, :st[-1] << (2 - sub_x)]
    return (src.astype(np.uint16) if sb == 2 else src), (down, up, st, mi_cols, down_luma)


def load_golden():
    return np.load(GOLDEN)


# ---- the reference's parameter structures, for the single-call forms and the reference's own functions ---------------------------------------------------
import ctypes as C  # noqa: E402


class InterpFilterParams(C.Structure):  # definitions.h:742-747
    _fields_ = [("filter_ptr", C.c_void_p), ("taps", C.c_uint16), ("subpel_shifts", C.c_uint16), ("interp_filter", C.c_uint32)]


class ConvolveParams(C.Structure):  # definitions.h:572-585
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32), ("round_0", C.c_int32), ("round_1", C.c_int32),
                ("plane", C.c_int32), ("is_compound", C.c_int32), ("use_jnt_comp_avg", C.c_int32), ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32),
                ("use_dist_wtd_comp_avg", C.c_int32)]


def filter_params(rows):
    """(InterpFilterParams, the int16 array it points at) of a 16 x 8 table"""
    a = np.ascontiguousarray(rows, np.int16)
    return InterpFilterParams(a.ctypes.data, 8, 16, 0), a


# the calls of a form test: w, h, (xs, ys, sx, sy), filter_x, filter_y, is_compound, do_average, use_dist_wtd_comp_avg, weights, round_0 / round_1 (None: no_round)
FORM_CASES = [(16, 16, (2048, 2048, 1023, 0), 0, 0, 0, 0, 0, 0, None), (8, 32, (1150, 1820, 300, 900), 2, 1, 1, 0, 0, 0, None), (8, 32, (1150, 1820, 300, 900), 2, 1, 1, 1, 0, 0, None),
              (4, 4, (64, 512, 9, 1000), 1, 2, 1, 1, 1, 3, None), (64, 8, (1024, 1024, 512, 512), 0, 3, 0, 0, 0, 0, None), (32, 64, (768, 1798, 5, 6), 2, 2, 1, 1, 1, 1, None),
              (16, 4, (1365, 2048, 0, 1023), 0, 0, 0, 0, 0, 0, (4, 9)), (2, 2, (2048, 64, 1, 2), 1, 1, 1, 0, 0, 0, (5, 6))]


def form_rounds(bd, is_compound, rounds):
    return conv_rounds(bd, is_compound) if rounds is None else rounds
