"""The inputs of tests/test_picstats.py, regenerated from seeds: tests/test_picstats_ref.py records the reference's outputs for exactly these inputs in
tests/golden/picstats.npz (expected outputs, seeds and the three q_fp8 tables; no picture is stored)."""
import os

import numpy as np

import picstats_common as pc

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picstats.npz")
SEED = 20261
ORG_X, ORG_Y, EXTRA = 13, 5, 19  # the picture's origin inside the padded plane; stride = org_x + 64 * sbs_x + EXTRA
PICTURES = [(64, 64), (192, 128), (200, 136)]  # the last has edge superblocks read from padding
CLASSES = ["flat", "hgrad", "noise2", "random", "checker"]
LOW_VARIANCE = ["flat", "hgrad", "noise2"]


def luma(kind, h, w, g):
    """one 8-bit plane of an input class"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.full((h, w), 131, np.uint8)
    if kind == "hgrad":
        return ((xx * 3 // 8 + 7) & 255).astype(np.uint8)
    if kind == "noise2":
        return (120 + g.integers(-2, 3, (h, w))).astype(np.uint8)
    if kind == "random":
        return g.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "checker":
        return (((xx + yy) & 1) * 255).astype(np.uint8)
    raise ValueError(kind)


def padded_picture(kind, width, height, seed):
    """-> (padded plane [rows][stride], stride): class content over the whole plane, so the padding an edge superblock reads is of the class too"""
    g = np.random.default_rng(seed)
    sbs_x, sbs_y = (width + 63) // 64, (height + 63) // 64
    stride, rows = ORG_X + 64 * sbs_x + EXTRA, ORG_Y + 64 * sbs_y + 2
    return luma(kind, rows, stride, g), stride


def variance_seed(pi, ci):
    return SEED + 100 * pi + ci


# ---- boost inputs: variance tables of pictures whose superblocks cycle through low-variance content of different strength ------------------------------
BOOST_SB_COUNTS = {1: (64, 64), 6: (192, 128), 600: (1920, 1280)}
_AMPS = [0, 1, 2, 3, 5, 8, 13, 1]


def boost_picture(n_sb, kind, seed):
    """`low`: superblock k is base + noise of amplitude _AMPS[k % 8] (k % 8 == 7: a horizontal gradient instead) -- flat, gradient and `base +- a` content only;
    `random`: uniform noise (boost 0 everywhere)."""
    w, h = BOOST_SB_COUNTS[n_sb]
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.integers(0, 256, (h, w)).astype(np.uint8)
    pl = np.zeros((h, w), np.uint8)
    sbs_x = w // 64
    xx = np.mgrid[0:64, 0:64][1]
    for k in range(n_sb):
        y, x = 64 * (k // sbs_x), 64 * (k % sbs_x)
        a = _AMPS[(k + seed) % 8]
        if (k + seed) % 8 == 7:
            blk = 40 + xx * 3 // 8
        else:
            blk = 60 + 11 * (k % 9) + g.integers(-a, a + 1, (64, 64))
        pl[y:y + 64, x:x + 64] = blk
    return pl


def boost_variance(n_sb, kind, seed):
    w, h = BOOST_SB_COUNTS[n_sb]
    return pc.picture_variance(boost_picture(n_sb, kind, seed), 0, 0, w, h, pc.PREC_SUB)[0]


def boost_qindex_in(n_sb, mode, seed):
    if mode == "const":
        return np.full(n_sb, 120, np.uint8)
    g = np.random.default_rng(seed + 5)
    q = g.integers(1, 256, n_sb).astype(np.uint8)
    q[0], q[-1] = 1, 255  # (with one superblock: 255)
    return q


# (n_sb, variance kind, qindex_in mode, base_q_idx, strength, octile, curve, bit depth): octile 1, 6, 8; every curve; constant and spread qindex_in; 1, 6, 600 SBs
BOOST_CASES = [
    (1, "low", "const", 128, 2, 6, 0, 8),
    (1, "low", "spread", 200, 3, 1, 1, 10),
    (6, "low", "const", 128, 2, 6, 0, 8),
    (6, "low", "spread", 128, 2, 6, 0, 8),
    (6, "low", "const", 60, 4, 1, 1, 10),
    (6, "low", "const", 255, 1, 8, 2, 8),
    (6, "low", "spread", 40, 3, 8, 2, 12),
    (6, "random", "const", 128, 2, 6, 0, 8),
    (600, "low", "const", 128, 2, 6, 0, 8),
    (600, "low", "spread", 90, 4, 6, 1, 10),
    (600, "random", "spread", 128, 2, 1, 2, 8),
]


def boost_seed(i):
    return SEED + 1000 + i


# ---- histogram inputs -----------------------------------------------------------------------------------------------------------------
# (width, height, regions_w, regions_h, kind): 50x34 / 4x4 has remainders both ways; one all-equal plane
HIST_CASES = [(50, 34, 4, 4, "random"), (48, 32, 1, 1, "random"), (50, 34, 4, 4, "equal"), (64, 33, 4, 1, "hgrad")]
HIST_ORG_X, HIST_ORG_Y, HIST_EXTRA = 9, 4, 6


def hist_plane(i, seed=SEED + 2000):
    """-> (padded plane, stride, the picture inside it)"""
    w, h, _, _, kind = HIST_CASES[i]
    g = np.random.default_rng(seed + i)
    stride, rows = HIST_ORG_X + w + HIST_EXTRA, HIST_ORG_Y + h + 3
    pl = g.integers(0, 256, (rows, stride)).astype(np.uint8)
    pic = np.full((h, w), 77, np.uint8) if kind == "equal" else luma("hgrad" if kind == "hgrad" else "random", h, w, g)
    pl[HIST_ORG_Y:HIST_ORG_Y + h, HIST_ORG_X:HIST_ORG_X + w] = pic
    return pl, stride, pic


def load_golden():
    return np.load(GOLDEN_FILE)
