"""numpy restatement of the picture-analysis statistics and of the variance boost (csrc/picstats.hip): block means and variances
(compute_block_mean_compute_variance, pic_analysis_process.c:306-1380), the variance boost (av1_get_deltaq_sb_variance_boost and svt_variance_adjust_qp,
rc_process.c:1403-1617) and the region histograms (sub_sample_luma_generate_pixel_intensity_histogram_bins, pic_analysis_process.c:1461-1524).
Pinned against the reference's own functions by tests/test_picstats_ref.py."""
import math

import numpy as np

PREC_FULL, PREC_SUB = 0, 1
V64, V32, V16, V8 = 0, 1, 5, 21  # ME_TIER_ZERO_PU_* (me_context.h:54-138)
MAX_DELTAQ_RANGE = 80


# ---- (1) block means and variances ------------------------------------------------------------------------------------------------------
def block_means_8x8(plane, prec):
    """plane: uint8 [64 * sbs_y, 64 * sbs_x] -> (mean, mean of squares) of every 8x8 block as uint64, the reference's fixed point"""
    h, w = plane.shape
    b = plane.astype(np.uint64).reshape(h // 8, 8, w // 8, 8)
    if prec == PREC_SUB:
        b = b[:, 0::2]
        return b.sum(axis=(1, 3)) << np.uint64(3), (b * b).sum(axis=(1, 3)) << np.uint64(11)
    return (b.sum(axis=(1, 3)) << np.uint64(8)) // np.uint64(64), ((b * b).sum(axis=(1, 3)) << np.uint64(16)) // np.uint64(64)


def _up(m):
    """(a + b + c + d) >> 2 of every 2x2 group of the level below"""
    return (m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]) >> np.uint64(2)


def _var(mean, msq):
    return ((msq - mean * mean) >> np.uint64(16)).astype(np.uint16)  # uint64 wrapping, truncated to 16 bits


def picture_variance(padded, org_x, org_y, width, height, prec, write_sub64=True, init=None):
    """padded: the uint8 padded plane -> (variance [n_sb][85] uint16, pic_avg_variance).  Entries the reference does not write keep `init`."""
    sbs_x, sbs_y = (width + 63) // 64, (height + 63) // 64
    area = padded[org_y:org_y + 64 * sbs_y, org_x:org_x + 64 * sbs_x]
    assert area.shape == (64 * sbs_y, 64 * sbs_x), "the padded plane does not cover the edge superblocks"
    m8, q8 = block_means_8x8(area, prec)
    m16, q16 = _up(m8), _up(q8)
    m32, q32 = _up(m16), _up(q16)
    m64, q64 = _up(m32), _up(q32)
    out = np.zeros((sbs_y * sbs_x, 85), np.uint16) if init is None else init.copy()
    sb = lambda v, k: v.reshape(sbs_y, k, sbs_x, k).transpose(0, 2, 1, 3).reshape(sbs_y * sbs_x, k * k)  # noqa: E731  (raster inside every superblock)
    out[:, V64] = sb(_var(m64, q64), 1)[:, 0]
    if write_sub64:
        out[:, V32:V32 + 4] = sb(_var(m32, q32), 2)
        out[:, V16:V16 + 16] = sb(_var(m16, q16), 4)
        out[:, V8:V8 + 64] = sb(_var(m8, q8), 8)
    return out, int(out[:, V64].astype(np.uint64).sum()) // (sbs_x * sbs_y) & 0xffff


# ---- (2) variance boost ---------------------------------------------------------------------------------------------------------------
def compute_qdelta_fp(q, qstart, qtarget):
    """svt_av1_compute_qdelta_fp (rc_process.c:190-210) against a 256-entry qindex -> q_fp8 table"""
    def index(t):
        for i in range(255):
            if q[i] >= t:
                return i
        return 254
    return index(qtarget) - index(qstart)


def boost_of_variance(variance, base_q_idx, strength, curve, q):
    """the part of av1_get_deltaq_sb_variance_boost after the blend (rc_process.c:1459-1493); Python floats are IEEE doubles and math.log2 / pow are the C library's"""
    variance = variance or 1
    strengths = (0, 0.65, 1.1, 1.6, 2.5)
    if curve == 1:
        ratio = 0.25 * strength * (-math.log2(float(variance)) + 8) + 1
    elif curve == 2:
        ratio = 0.15 * strength * (-math.log2(float(variance)) + 10) + 1
    else:
        ratio = math.pow(1.018, strengths[strength] * (-10 * math.log2(float(variance)) + 80))
    ratio = min(max(ratio, 1.0), 8.0)
    base_q = int(q[base_q_idx])
    target_q = int(base_q / ratio)
    d = -compute_qdelta_fp(q, base_q, target_q)
    tdiv = lambda a, b: int(math.copysign(abs(a) // b, a))  # noqa: E731  (C division truncates)
    boost = tdiv((base_q_idx + 496) * d, 255 + 1024) if curve == 2 else tdiv((base_q_idx + 40) * d, 255 + 40)
    return min(MAX_DELTAQ_RANGE, boost)


def blended_variance(var85, octile):
    """the 1:2:1 blend of three octile samples of the sorted 8x8 variances (rc_process.c:1414-1431): [n_sb][85] -> [n_sb]"""
    o = np.sort(var85[:, V8:V8 + 64].astype(np.int64), axis=1)
    mid = octile * 8 - 1
    low, upp = max(7, mid - 8), min(63, mid + 8)
    return ((o[:, low] + o[:, mid] * 2 + o[:, upp] + 2) // 4) & 0xffff


def variance_boost(var85, qindex_in, base_q_idx, strength, octile, curve, q):
    """svt_variance_adjust_qp -> (qindex_out uint8 [n_sb], normalized_base_q_idx, min, max, boost [n_sb])"""
    bl = blended_variance(var85, octile)
    cache = {}
    boost = np.array([cache.setdefault(int(v), boost_of_variance(int(v), base_q_idx, strength, curve, q)) for v in bl], np.int64)
    qi = np.clip(qindex_in.astype(np.int64) - boost, 1, 255)
    mn, mx = int(qi.min()), int(qi.max())
    base = mn + (min(mx - mn, MAX_DELTAQ_RANGE) >> 1)
    off = np.clip(qi - base, -(MAX_DELTAQ_RANGE >> 1), MAX_DELTAQ_RANGE >> 1)
    return np.clip(base + off, 1, 255).astype(np.uint8), base, mn, mx, boost


# ---- (3) histograms --------------------------------------------------------------------------------------------------------------------
def picture_histogram(plane, regions_w, regions_h, decim_step):
    """plane: the uint8 1/16 picture (no padding) -> (histogram [rw][rh][256] uint32, average_intensity_per_region [rw][rh] uint8, avg_luma)"""
    height, width = plane.shape
    rw, rh = width // regions_w, height // regions_h
    hist = np.zeros((regions_w, regions_h, 256), np.uint32)
    avg = np.zeros((regions_w, regions_h), np.uint8)
    total = 0
    d2 = decim_step * decim_step
    for wi in range(regions_w):
        for hi in range(regions_h):
            w = rw + (width - regions_w * rw if wi == regions_w - 1 else 0)
            h = rh + (height - regions_h * rh if hi == regions_h - 1 else 0)
            s = plane[hi * rh:hi * rh + h:decim_step, wi * rw:wi * rw + w:decim_step]
            hist[wi, hi] = ((1 + np.bincount(s.reshape(-1), minlength=256)) * 16 * d2) & 0xffffffff
            ssum = int(s.astype(np.uint64).sum()) * d2
            avg[wi, hi] = ((ssum + ((w * h) >> 1)) // (w * h)) & 0xff
            total += ssum
    return hist, avg, total // (width * height)
