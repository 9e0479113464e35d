"""Picture-analysis statistics and the variance boost (csrc/picstats.hip) on the emulator and, under `-m gpu`, on the device: block variances, the boosted
qindex, the region histograms and the four single-call forms -- against tests/picstats_common.py (numpy; pinned to the reference by tests/test_picstats_ref.py) AND
against tests/golden/picstats.npz, the reference's own outputs for these inputs.  Everything is bit-exact.  Inputs: tests/picstats_cases.py."""
import numpy as np
import pytest

import picstats_cases as cases
import picstats_common as pc
from conftest import p

POISON = 0xabcd


@pytest.fixture(scope="module")
def gold():
    return cases.load_golden()


# ---- variance -------------------------------------------------------------------------------------------------------------------------
def _run_variance(be, planes, pitch, stride, w, h, prec, sub64):
    """planes: one uint8 buffer holding len(planes) // pitch pictures -> (variance [n_pics][n_sb][85], pic_avg [n_pics]); outputs start poisoned"""
    n_pics = len(planes) // pitch
    n_sb = ((w + 63) // 64) * ((h + 63) // 64)
    d_in = be.dev(planes)
    d_var, d_avg = be.dev(np.full((n_pics, n_sb, 85), POISON, np.uint16)), be.dev(np.full(n_pics, POISON, np.uint16))
    be.lib.svt_hip_picture_variance_batch(be.ptr(d_in), pitch, stride, cases.ORG_X, cases.ORG_Y, w, h, n_pics, prec, int(sub64), be.ptr(d_var), be.ptr(d_avg), be.stream)
    return be.host(d_var), be.host(d_avg)


@pytest.mark.parametrize("prec", [pc.PREC_FULL, pc.PREC_SUB])
@pytest.mark.parametrize("pi", range(len(cases.PICTURES)))
def test_picture_variance(be, gold, pi, prec):
    """Every input class as a one-picture launch, then three pictures in one launch with a pitch that is not the plane size; stride > width, non-zero origin, the
    200x136 picture's edge superblocks read from padding; the sub-64 flag on (all 85 entries) and off (entry 0 only, the rest untouched)."""
    w, h = cases.PICTURES[pi]
    pads = [cases.padded_picture(kind, w, h, cases.variance_seed(pi, ci)) for ci, kind in enumerate(cases.CLASSES)]
    stride = pads[0][1]
    for ci, kind in enumerate(cases.CLASSES):
        plane = pads[ci][0]
        want, wavg = pc.picture_variance(plane, cases.ORG_X, cases.ORG_Y, w, h, prec)
        assert np.array_equal(want, gold["var_%d_%d_%d" % (pi, ci, prec)]) and wavg == int(gold["avg_%d_%d_%d" % (pi, ci, prec)][0])
        got, gavg = _run_variance(be, plane.reshape(-1), plane.size, stride, w, h, prec, True)
        assert np.array_equal(got[0], want), (kind, np.argwhere(got[0] != want)[:6])
        assert int(gavg[0]) == wavg, kind
        got, gavg = _run_variance(be, plane.reshape(-1), plane.size, stride, w, h, prec, False)
        assert np.array_equal(got[0][:, 0], want[:, 0]) and np.all(got[0][:, 1:] == POISON) and int(gavg[0]) == wavg, kind
    # n_pics = 3 with a pitch
    batch = [1, 2, 4]
    pitch = pads[0][0].size + 77
    buf = np.full(3 * pitch, 0x5a, np.uint8)
    for k, ci in enumerate(batch):
        buf[k * pitch:k * pitch + pads[ci][0].size] = pads[ci][0].reshape(-1)
    got, gavg = _run_variance(be, buf, pitch, stride, w, h, prec, True)
    for k, ci in enumerate(batch):
        assert np.array_equal(got[k], gold["var_%d_%d_%d" % (pi, ci, prec)]) and int(gavg[k]) == int(gold["avg_%d_%d_%d" % (pi, ci, prec)][0]), (k, ci)
    # what was compared is not degenerate: flat content has variance 0 everywhere, the 0 / 255 checker 127.5^2 in every 8x8 block, the two precisions differ on noise,
    # and the entries of a superblock of random content differ from one another
    assert not gold["var_%d_0_%d" % (pi, prec)].any() and np.all(gold["var_%d_4_%d" % (pi, prec)][:, pc.V8:] == 16256)
    assert not np.array_equal(gold["var_%d_2_0" % pi], gold["var_%d_2_1" % pi])
    assert len(np.unique(gold["var_%d_3_%d" % (pi, prec)][0])) > 60



# ---- boost ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(cases.BOOST_CASES)))
def test_variance_boost_qindex(be, gold, ci):
    """1, 6 and 600 superblocks (600: more than one workgroup of either launch takes in one pass); qindex_in constant and spread over 1 .. 255; octile 1, 6, 8; every
    curve.  In every case built from the low-variance classes the RESTATEMENT gives a non-zero boost to at least half of the superblocks and -- where there are
    superblocks enough to have them: one superblock has one value -- at least three values of qindex_out, so a kernel that returns qindex_in cannot pass."""
    n_sb, kind, mode, bq, st, oc, cv, bd = cases.BOOST_CASES[ci]
    seed = cases.boost_seed(ci)
    var, qin = cases.boost_variance(n_sb, kind, seed), cases.boost_qindex_in(n_sb, mode, seed)
    q = gold["q_fp8_%d" % bd]
    want, wbase, wmin, wmax, boost = pc.variance_boost(var, qin, bq, st, oc, cv, q)
    assert np.array_equal(want, gold["boost_q_%d" % ci]) and wbase == int(gold["boost_base_%d" % ci][0])
    if kind == "low":
        assert 2 * np.count_nonzero(boost) >= n_sb and not np.array_equal(want, qin)
        if n_sb >= 3:
            assert len(np.unique(want)) >= 3
        if mode == "spread" and n_sb >= 6:  # both clamps act: the frame pass's +-40 and, with 600 superblocks, CLIP3(1, 255, .) before it
            assert wmax - wmin > pc.MAX_DELTAQ_RANGE and want.min() == wbase - 40 and want.max() == wbase + 40
            assert n_sb < 600 or (qin.astype(np.int64) - boost).min() < 1
    else:
        assert not boost.any()  # uniform noise: no boost anywhere (never the only input: see cases.BOOST_CASES)
    d_var, d_qin = be.dev(var), be.dev(qin)
    d_out, d_frame = be.dev(np.full(n_sb, 0xee, np.uint8)), be.dev(np.full(4, -7, np.int32))
    assert be.lib.svt_hip_variance_boost_qindex(be.ptr(d_var), be.ptr(d_qin), n_sb, bq, st, oc, cv, bd, p(q), be.ptr(d_out), be.ptr(d_frame), be.stream) == 0
    got, frame = be.host(d_out), be.host(d_frame).view(be.pkg.VarBoostFrame)[0]
    assert np.array_equal(got, want), (cases.BOOST_CASES[ci], np.flatnonzero(got != want)[:8])
    assert (int(frame["normalized_base_q_idx"]), int(frame["min_qindex"]), int(frame["max_qindex"])) == (wbase, wmin, wmax)
    assert np.array_equal(be.host(d_qin), qin)
    # in place
    assert be.lib.svt_hip_variance_boost_qindex(be.ptr(d_var), be.ptr(d_qin), n_sb, bq, st, oc, cv, bd, p(q), be.ptr(d_qin), be.ptr(d_frame), be.stream) == 0
    assert np.array_equal(be.host(d_qin), want)


def test_variance_boost_rejects_bad_arguments(be, gold):
    q = gold["q_fp8_8"]
    z = be.dev(np.zeros(85, np.uint16))
    for st, oc, cv in ((0, 6, 0), (5, 6, 0), (2, 0, 0), (2, 9, 0), (2, 6, 3)):
        assert be.lib.svt_hip_variance_boost_qindex(be.ptr(z), be.ptr(z), 1, 128, st, oc, cv, 8, p(q), be.ptr(z), be.ptr(z), be.stream) == -1


# ---- histogram ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decim", [1, 4])
@pytest.mark.parametrize("hi", range(len(cases.HIST_CASES)))
def test_picture_histogram(be, gold, hi, decim):
    """50x34 in 4x4 regions (remainder columns and rows in the last regions), 48x32 as one region, an all-equal plane (one bin takes every sample), 4x1 regions"""
    w, h, rw, rh, kind = cases.HIST_CASES[hi]
    padded, stride, pic = cases.hist_plane(hi)
    wh, wa, wl = pc.picture_histogram(pic, rw, rh, decim)
    assert np.array_equal(wh, gold["hist_%d_%d" % (hi, decim)]) and np.array_equal(wa, gold["hist_avg_%d_%d" % (hi, decim)]) and wl == int(gold["hist_luma_%d_%d" % (hi, decim)][0])
    if kind == "equal":
        assert np.all(wh[:, :, 77] > 16 * decim * decim) and np.all(np.delete(wh, 77, axis=2) == 16 * decim * decim) and (decim != 1 or np.all(wa == 77))  # (decim 4: samples * 16 is not the area of a region with remainders -- the reference's own rounding)
    d_in = be.dev(padded)
    d_h, d_a, d_l = be.dev(np.full((rw, rh, 256), 0xdeadbeef, np.uint32)), be.dev(np.full((rw, rh), 0xee, np.uint8)), be.dev(np.full(1, 0xdead, np.uint64))
    be.lib.svt_hip_picture_histogram(be.ptr(d_in) + cases.HIST_ORG_Y * stride + cases.HIST_ORG_X, stride, w, h, rw, rh, decim, be.ptr(d_h), be.ptr(d_a), be.ptr(d_l), be.stream)
    assert np.array_equal(be.host(d_h), wh) and np.array_equal(be.host(d_a), wa) and int(be.host(d_l)[0]) == wl


# ---- per-call forms --------------------------------------------------------------------------------------------------------------------
def test_per_call_forms(be):
    """one call each, host pointers, a stride that is not the width"""
    L = be.lib
    g = np.random.default_rng(cases.SEED + 3000)
    a = g.integers(0, 256, (12, 53)).astype(np.uint8)
    blk = np.ascontiguousarray(a[3:11, 7:39])
    at = a.ctypes.data + 3 * 53 + 7
    mf, qf = pc.block_means_8x8(blk, pc.PREC_FULL)
    ms, qs = pc.block_means_8x8(blk, pc.PREC_SUB)
    assert L.svt_compute_mean_8x8_hip(at, 53, 8, 8) == int(mf[0, 0])
    assert L.svt_compute_mean_square_values_8x8_hip(at + 8, 53, 8, 8) == int(qf[0, 1])
    assert L.svt_compute_sub_mean_8x8_hip(at + 16, 53) == int(ms[0, 2])
    m4, q4 = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    L.svt_compute_interm_var_four8x8_hip(at, 53, p(m4), p(q4))
    assert np.array_equal(m4, ms[0]) and np.array_equal(q4, qs[0])
    assert L.svt_hip_debug_commit_violations() == 0
