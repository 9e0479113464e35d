"""numpy restatement of AV1's masked prediction (csrc/maskpred.hip): the wedge, inter-intra and OBMC tables, the a64 blends with their four sub-sampling branches, the
pixel-domain diff-weighted mask builders, the four wedge-search helpers, build_smooth_interintra_mask, svt_aom_combine_interintra and the wedge / seg search of
pick_wedge, pick_wedge_fixed_sign and pick_interinter_seg with use_rate == 0.  Pinned on the reference's C by tests/test_maskpred_ref.py, which also writes
tests/golden/maskpred.npz.  The table generation follows svt_av1_init_wedge_masks step by step (shifted primary rows, transposes, complements, windows): a different
derivation from the closed form the device's table kernel evaluates.  Blocks are (..., h, w) arrays; leading axes are batch axes."""
import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskpred.npz")
GOLDEN_SEED = 4220

# BlockSize
BW = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BH = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)
BSIZE_OF = {(w, h): i for i, (w, h) in enumerate(zip(BW, BH))}
WEDGE_BSIZES = (3, 4, 5, 6, 7, 8, 9, 18, 19)  # 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32, 8x32, 32x8
II_BSIZES = (3, 4, 5, 6, 7, 8, 9)  # svt_aom_is_interintra_allowed_bsize (mode_decision.h:175): BLOCK_8X8 <= bsize <= BLOCK_32X32
KIND_A64, KIND_H, KIND_V = 0, 1, 2
SRC_EXPLICIT, SRC_WEDGE, SRC_SMOOTH, SRC_OBMC = 0, 1, 2, 3

HORZ, VERT, OBL27, OBL63, OBL117, OBL153 = range(6)
_ZERO, _FULL = [0] * 27, [64] * 25
PRIMARY_EVEN = np.array(_ZERO + [0, 1, 4, 11, 27, 46, 58, 62, 63] + [64] * 28, np.uint8)[:64]
PRIMARY_ODD = np.array(_ZERO + [0, 1, 2, 6, 18, 37, 53, 60, 63] + [64] * 28, np.uint8)[:64]
PRIMARY_VERT = np.array(_ZERO + [0, 0, 2, 7, 21, 43, 57, 62] + [64] * 29, np.uint8)[:64]
_COMMON = [(OBL27, 4, 2), (OBL27, 4, 6), (OBL153, 4, 2), (OBL153, 4, 6), (OBL63, 2, 4), (OBL63, 6, 4), (OBL117, 2, 4), (OBL117, 6, 4)]
_HEAD = [(OBL27, 4, 4), (OBL63, 4, 4), (OBL117, 4, 4), (OBL153, 4, 4)]
CODEBOOK_HEQW = _HEAD + [(HORZ, 4, 2), (HORZ, 4, 6), (VERT, 2, 4), (VERT, 6, 4)] + _COMMON
CODEBOOK_HGTW = _HEAD + [(HORZ, 4, 2), (HORZ, 4, 4), (HORZ, 4, 6), (VERT, 4, 4)] + _COMMON
CODEBOOK_HLTW = _HEAD + [(VERT, 2, 4), (VERT, 4, 4), (VERT, 6, 4), (HORZ, 4, 4)] + _COMMON
SIGNFLIP = {3: "1111111111011101", 6: "1111111111011101", 9: "1111111111011101", 4: "1111011111011101", 5: "1111011111011101", 7: "1111011111011101",
            8: "1111011111011101", 18: "1111011101011101", 19: "1111011111010101"}

II_WEIGHTS1D = np.array([60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20, 19, 19, 18, 18, 17,
                         16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 4, 4, 4, 4, 4, 4,
                         4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
                        np.uint8)
II_SIZE_SCALES = (32, 16, 16, 16, 8, 8, 8, 4, 4, 4, 2, 2, 2, 1, 1, 1, 8, 8, 4, 4, 2, 2)
OBMC_MASKS = {1: [64], 2: [45, 64], 4: [39, 50, 59, 64], 8: [36, 42, 48, 53, 57, 61, 64, 64], 16: [34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64],
              32: [33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64]}
OBMC_MASKS = {k: np.array(v, np.uint8) for k, v in OBMC_MASKS.items()}


# ---- tables --------------------------------------------------------------------------------------------------------------------------------------------
def _shift_copy(src, shift):
    dst = np.empty(64, np.uint8)
    if shift >= 0:
        dst[shift:] = src[:64 - shift]
        dst[:shift] = src[0]
    else:
        s = -shift
        dst[:64 - s] = src[s:]
        dst[64 - s:] = src[63]
    return dst


def primary_masks():
    """wedge_mask_obl[2][6][64][64] after init_wedge_primary_masks"""
    m = np.zeros((2, 6, 64, 64), np.int32)
    shift = 16
    for i in range(0, 64, 2):
        m[0, OBL63, i] = _shift_copy(PRIMARY_EVEN, shift)
        shift -= 1
        m[0, OBL63, i + 1] = _shift_copy(PRIMARY_ODD, shift)
        m[0, VERT, i] = m[0, VERT, i + 1] = PRIMARY_VERT
    b = m[0, OBL63]
    m[0, OBL27] = b.T
    m[0, OBL117] = 64 - b[:, ::-1]
    m[0, OBL153] = (64 - b[:, ::-1]).T  # [(w - 1 - j)][i] = 64 - b[i][j]
    m[0, HORZ] = m[0, VERT].T
    m[1] = 64 - m[0]
    return m


def _codebook(bsize):
    w, h = BW[bsize], BH[bsize]
    return CODEBOOK_HEQW if h == w else (CODEBOOK_HGTW if h > w else CODEBOOK_HLTW)


_tables = {}


def wedge_masks():
    """{(bsize, wedge_index, wedge_sign): (bh, bw) uint8}: the 288 masks svt_aom_get_contiguous_soft_mask returns after svt_av1_init_wedge_masks"""
    if "wedge" not in _tables:
        prim, out = primary_masks(), {}
        for bsize in WEDGE_BSIZES:
            bw, bh = BW[bsize], BH[bsize]
            for idx, (direction, xo, yo) in enumerate(_codebook(bsize)):
                flip = int(SIGNFLIP[bsize][idx])
                woff, hoff = (xo * bw) >> 3, (yo * bh) >> 3
                for sign in (0, 1):
                    out[(bsize, idx, sign)] = prim[sign ^ flip, direction, 32 - hoff:32 - hoff + bh, 32 - woff:32 - woff + bw].astype(np.uint8)
        _tables["wedge"] = out
    return _tables["wedge"]


def wedge_table_bytes():
    """the device table's layout: BlockSize order, then wedge index, then sign"""
    wm = wedge_masks()
    return np.concatenate([wm[(b, i, s)].reshape(-1) for b in WEDGE_BSIZES for i in range(16) for s in (0, 1)])


def smooth_interintra_mask(plane_bsize, mode):
    """build_smooth_interintra_mask: II_DC_PRED 0, II_V_PRED 1, II_H_PRED 2, II_SMOOTH_PRED 3"""
    bw, bh, sc = BW[plane_bsize], BH[plane_bsize], II_SIZE_SCALES[plane_bsize]
    i, j = np.mgrid[0:bh, 0:bw]
    if mode == 1:
        return II_WEIGHTS1D[i * sc]
    if mode == 2:
        return II_WEIGHTS1D[j * sc]
    if mode == 3:
        return II_WEIGHTS1D[np.minimum(i, j) * sc]
    return np.full((bh, bw), 32, np.uint8)


# ---- blends --------------------------------------------------------------------------------------------------------------------------------------------
def subsample_mask(mask, w, h, subw, subh):
    """the mask value per output sample of the a64_mask functions: (..., h << subh, w << subw) -> (..., h, w)"""
    m = np.asarray(mask, np.int64)[..., :h << subh, :w << subw]
    if subw and subh:
        return (m[..., 0::2, 0::2] + m[..., 1::2, 0::2] + m[..., 0::2, 1::2] + m[..., 1::2, 1::2] + 2) >> 2  # ROUND_POWER_OF_TWO(sum of four, 2)
    if subw:
        return (m[..., :, 0::2] + m[..., :, 1::2] + 1) >> 1  # AOM_BLEND_AVG
    if subh:
        return (m[..., 0::2, :] + m[..., 1::2, :] + 1) >> 1
    return m


def blend_a64(m, s0, s1):
    """AOM_BLEND_A64"""
    m = np.asarray(m, np.int64)
    return (m * np.asarray(s0, np.int64) + (64 - m) * np.asarray(s1, np.int64) + 32) >> 6


def blend_a64_mask(s0, s1, mask, subw=0, subh=0):
    h, w = np.shape(s0)[-2:]
    return blend_a64(subsample_mask(mask, w, h, subw, subh), s0, s1)


def blend_a64_hmask(s0, s1, mask):
    return blend_a64(np.asarray(mask)[..., None, :np.shape(s0)[-1]], s0, s1)


def blend_a64_vmask(s0, s1, mask):
    return blend_a64(np.asarray(mask)[..., :np.shape(s0)[-2], None], s0, s1)


def combine_interintra(mode, use_wedge, wedge_index, wedge_sign, bsize, plane_bsize, inter, intra):
    """svt_aom_combine_interintra / _highbd: the mask weighs the INTRA prediction"""
    bw, bh = BW[plane_bsize], BH[plane_bsize]
    if use_wedge:
        subw, subh = int(2 * (BW[bsize] // 4) == bw), int(2 * (BH[bsize] // 4) == bh)  # 2 * mi_size_wide[bsize] == bw
        return blend_a64_mask(intra, inter, wedge_masks()[(bsize, wedge_index, wedge_sign)], subw, subh)
    return blend_a64_mask(intra, inter, smooth_interintra_mask(plane_bsize, mode))


# ---- the search helpers ---------------------------------------------------------------------------------------------------------------------------------
def diffwtd_mask(mask_type, p0, p1, bd=8):
    """svt_av1_build_compound_diffwtd_mask_c (bd 8) / _highbd_c: 38 + (|p0 - p1| >> (bd - 8)) / 16, clamped to 64; mask_type 1 is the inverse"""
    diff = np.abs(np.asarray(p0, np.int64) - np.asarray(p1, np.int64)) >> (bd - 8)
    m = np.clip(38 + diff // 16, 0, 64)
    return (64 - m if mask_type else m).astype(np.uint8)


def sum_squares_i16(a):
    a = np.asarray(a, np.int64)
    return (a * a).sum(axis=-1)


def wedge_compute_delta_squares(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.clip(a * a - b * b, -32768, 32767).astype(np.int16)


def wedge_sign_from_residuals(ds, m, limit):
    return ((np.asarray(ds, np.int64) * np.asarray(m, np.int64)).sum(axis=-1) > limit).astype(np.int8)


def wedge_sse_terms(r1, d, m):
    """the clamped terms of svt_av1_wedge_sse_from_residuals_c and the unclamped ones"""
    raw = 64 * np.asarray(r1, np.int64) + np.asarray(m, np.int64) * np.asarray(d, np.int64)
    return np.clip(raw, -32768, 32767), raw


def wedge_sse_from_residuals(r1, d, m):
    t, _ = wedge_sse_terms(r1, d, m)
    return ((t * t).sum(axis=-1) + 2048) >> 12


def wedge_search(src, p0, p1, bsize, bd, fixed_sign=0):
    """one block: dict with sse[16], sign[16], sse_diffwtd[2], best_wedge_index, best_wedge_sign, best_mask_type and the intermediates the tests assert on"""
    n = BW[bsize] * BH[bsize]
    s, a, c = (np.asarray(v, np.int64).reshape(n) for v in (src, p0, p1))
    r0, r1, d10 = s - a, s - c, c - a
    limit = (int(sum_squares_i16(r0)) - int(sum_squares_i16(r1))) * 32
    ds = wedge_compute_delta_squares(r0, r1)
    wm = wedge_masks()
    sse, sign, clamped = np.zeros(16, np.uint64), np.zeros(16, np.uint8), 0
    best, bi, bs = None, 0, 0
    for k in range(16):
        sg = fixed_sign - 1 if fixed_sign else int(wedge_sign_from_residuals(ds, wm[(bsize, k, 0)].reshape(n), limit))
        m = wm[(bsize, k, sg)].reshape(n)
        t, raw = wedge_sse_terms(r1, d10, m)
        clamped += int((t != raw).sum())
        sse[k], sign[k] = int(wedge_sse_from_residuals(r1, d10, m)), sg
        if best is None or int(sse[k]) < best:
            best, bi, bs = int(sse[k]), k, sg
    seg = np.zeros(2, np.uint64)
    for t2 in (0, 1):
        m = diffwtd_mask(t2, a, c, bd)
        t, raw = wedge_sse_terms(r1, d10, m)
        clamped += int((t != raw).sum())
        seg[t2] = int(wedge_sse_from_residuals(r1, d10, m))
    raw_ds = r0 * r0 - r1 * r1
    return dict(sse=sse, sign=sign, sse_diffwtd=seg, best_wedge_index=bi, best_wedge_sign=bs, best_mask_type=int(seg[1] < seg[0]), clamped_terms=clamped,
                saturated_ds=int((raw_ds != ds).sum()))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------
CLASSES = ("random", "flat", "extreme", "equal")


def make_pair(g, kind, w, h, bd, lead=()):
    """two blocks of one input class: random; flat (one value each); extreme (0 / max alternating, opposite phases); equal (the same random block twice)"""
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    shape = tuple(lead) + (h, w)
    if kind == "flat":
        a = np.broadcast_to(g.integers(0, mx + 1, tuple(lead) + (1, 1)), shape)
        b = np.broadcast_to(g.integers(0, mx + 1, tuple(lead) + (1, 1)), shape)
    elif kind == "extreme":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.broadcast_to(((yy + xx) & 1) * mx, shape)
        b = mx - a
    else:
        a = g.integers(0, mx + 1, shape)
        b = a if kind == "equal" else g.integers(0, mx + 1, shape)
    return np.ascontiguousarray(a).astype(dt), np.ascontiguousarray(b).astype(dt)


def make_search_inputs(g, kind, bsize, bd):
    """source and two predictions of one luma block: `near` = predictions within a few levels of the source (what a search sees); `random` = three unrelated blocks
    (at 10 and 12 bit the int16_t clamp of the SSE term and the saturation of the delta of squares bind); `equal` = p0 == p1; `tie` = one sample of p0 differs, so several wedge indices reach the same
    minimal SSE and others a larger one"""
    w, h, mx = BW[bsize], BH[bsize], (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    src = g.integers(0, mx + 1, (h, w))
    if kind == "random":
        p0, p1 = g.integers(0, mx + 1, (h, w)), g.integers(0, mx + 1, (h, w))
    else:
        p0 = np.clip(src + g.integers(-6, 7, (h, w)) * (1 << (bd - 8)), 0, mx)
        p1 = np.clip(src + g.integers(-6, 7, (h, w)) * (1 << (bd - 8)), 0, mx)
        if kind == "equal":
            p1 = p0.copy()
        elif kind == "tie":  # p1 == src and p0 differs from it in the centre sample alone: every mask that is 0 there (after the sign choice) reaches SSE 0
            p1, p0 = src.copy(), src.copy()
            p0[h // 2, w // 2] ^= 64  # (small enough that no term is clamped at any depth: the same ties at 8, 10 and 12 bit)
    return src.astype(dt), p0.astype(dt), p1.astype(dt)


def golden_blend_cases():
    """(function, w, h, bd, subw, subh, class): a few dozen per blend function"""
    cases, k = [], 0
    for bd in (8, 10, 12):
        for (w, h) in ((4, 4), (8, 8), (16, 8), (32, 32)):
            for (subw, subh) in ((0, 0), (1, 1), (1, 0), (0, 1)):
                cases.append(("mask", w, h, bd, subw, subh, CLASSES[k % 4]))
                k += 1
        for fn in ("hmask", "vmask"):
            for (w, h) in ((1, 1), (2, 16), (16, 2), (8, 8), (32, 8), (8, 32), (64, 64), (128, 4), (4, 128)):
                cases.append((fn, w, h, bd, 0, 0, CLASSES[k % 4]))
                k += 1
    return cases


def golden_blend_inputs(i, case):
    fn, w, h, bd, subw, subh, kind = case
    g = np.random.default_rng(GOLDEN_SEED + i)
    s0, s1 = make_pair(g, kind, w, h, bd)
    if fn == "mask":
        mask = g.integers(0, 65, (h << subh, w << subw)).astype(np.uint8)
    else:
        mask = g.integers(0, 65, w if fn == "hmask" else h).astype(np.uint8)
    return s0, s1, mask


def blend_case(case, s0, s1, mask):
    fn, w, h, bd, subw, subh, kind = case
    if fn == "mask":
        return blend_a64_mask(s0, s1, mask, subw, subh)
    return blend_a64_hmask(s0, s1, mask) if fn == "hmask" else blend_a64_vmask(s0, s1, mask)


def golden_search_cases():
    """(bsize, bd, class, fixed_sign)"""
    return [(b, bd, kind, fs) for b in WEDGE_BSIZES for bd in (8, 10, 12) for (kind, fs) in (("near", 0), ("random", 0), ("near", 1 + (b + bd) % 2))]


def golden_search_inputs(i, case):
    bsize, bd, kind, _ = case
    return make_search_inputs(np.random.default_rng(GOLDEN_SEED + 1000 + i), kind, bsize, bd)


def load_golden():
    return np.load(GOLDEN_FILE)


# ---- the masked compound ---------------------------------------------------------------------------------------------------------------------------------
COMP_WEDGE, COMP_DIFFWTD, COMP_EXPLICIT = 0, 1, 2


def blend_a64_d16_mask(a, b, mask, subw, subh, bd, r0, r1):
    """svt_aom_lowbd_blend_a64_d16_mask_c / svt_aom_highbd_blend_a64_d16_mask_c on two ConvBufType blocks (..., h, w)"""
    import interpred_common as ic
    h, w = np.shape(a)[-2:]
    m = subsample_mask(mask, w, h, subw, subh)
    res = ((m * np.asarray(a, np.int64) + (64 - m) * np.asarray(b, np.int64)) >> 6) - ic.round_offset(bd, r0, r1)
    return ic.clip(ic.rpot(res, 14 - r0 - r1), bd)


def diffwtd_mask_d16(mask_type, a, b, bd, r0, r1):
    """svt_av1_build_compound_diffwtd_mask_d16_c"""
    import interpred_common as ic
    diff = ic.rpot(np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)), 14 - r0 - r1 + bd - 8)
    m = np.clip(38 + diff // 16, 0, 64)
    return (64 - m if mask_type else m).astype(np.uint8)


def masked_compound(refs, w, h, filter_x, filter_y, bd, comp_type, mask=None, mask_type=0, subw=0, subh=0):
    """One descriptor of svt_hip_inter_pred_masked_batch: svt_aom_build_masked_compound_no_round on the two jnt_convolve outputs.  refs as interpred_common.predict's;
    mask: the wedge or explicit mask ((h << subh) x (w << subw) at least) -- ignored for DIFFWTD.  Returns (dst, seg mask or None)."""
    import interpred_common as ic
    r0, r1 = ic.conv_rounds(bd, True)
    cb = []
    for (ext, sx, sy) in refs[:2]:
        tx, ty = ic.FILTERS[ic.filter_kind(filter_x, w)][sx], ic.FILTERS[ic.filter_kind(filter_y, h)][sy]
        cb.append(ic.jnt_convolve(ext, w, h, tx, ty, int(sx != 0) + 2 * int(sy != 0), bd, r0, r1, bd == 8))
    seg = None
    if comp_type == COMP_DIFFWTD:
        mask = seg = diffwtd_mask_d16(mask_type, cb[0], cb[1], bd, r0, r1)
        subw = subh = 0
    return blend_a64_d16_mask(cb[0], cb[1], mask, subw, subh, bd, r0, r1), seg
