"""AV1 intra prediction (csrc/intrapred.hip): svt_hip_intra_pred_batch, svt_hip_cfl_pred_batch and the eleven single-call forms, every output sample against
tests/intrapred_common.py (numpy; pinned on the reference's C by tests/test_intrapred_ref.py) and against tests/golden/intrapred.npz (what the reference's C
computed).  Every batched launch writes into a destination plane with an odd stride (547 samples) that was filled with 0xA5 beforehand, blocks and neighbour arrays
at every byte alignment: the WHOLE destination plane is compared, so a sample written outside a block's w x h fails the test like a wrong sample inside it."""
import ctypes as C
import mmap

import numpy as np
import pytest

import dist_common as dc
import intrapred_common as ic
from conftest import EmuBackend, _backends, p, rng

SD, SP = 547, 601            # strides in samples: destination, the picture plane of the column tests
PLANE_T, PLANE_L = 3, 17     # indices into SvtHipIntraPredPlanes.base
BIT_DEPTHS = (8, 10, 12)
DIRECTIONAL = [(m, d) for m in range(ic.V, ic.D67 + 1) for d in range(-3, 4)]
CANDIDATES = [(m, d) for m in range(13) for d in (range(-3, 4) if ic.V <= m <= ic.D67 else (0,))]  # the 61 (mode, delta) pairs of one block
assert len(DIRECTIONAL) == 56 and len(CANDIDATES) == 61


def _place(cases, g):
    """shelf layout of the blocks inside a plane of stride SD: gaps of 1 .. 7 samples, so that block origins take every alignment"""
    x = y = shelf = 0
    pos = []
    for c in cases:
        gap = 1 + int(g.integers(0, 7))
        if x + gap + c["w"] > SD - 2:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + c["w"], max(shelf, c["h"])
    return pos, y + shelf + 1


def build(be, cases, bd, g):
    """neighbour planes, descriptors and the expected destination plane of one launch.  A case may carry its own "top" / "left" samples; the neighbour arrays lie
    back to back with gaps of 1 .. 7 samples."""
    dt = np.uint16 if bd > 8 else np.uint8
    pos, rows = _place(cases, g)
    fill = 0xA5A5 if bd > 8 else 0xA5
    want = np.full((rows + 2, SD), fill, dt)
    d = np.zeros(len(cases), be.pkg.IntraPredDesc)
    tops, lefts, to, lo = [], [], 0, 0
    for i, (c, (x, y)) in enumerate(zip(cases, pos)):
        w, h = c["w"], c["h"]
        top, left = (c["top"], c["left"]) if "top" in c else ic.case_inputs(g, c, bd)
        gt, gl = 1 + int(g.integers(0, 7)), 1 + int(g.integers(0, 7))
        tops += [np.full(gt, 7, np.int64), top]
        lefts += [np.full(gl, 9, np.int64), left]
        nt, ntr, nl, nbl = c["counts"] if "counts" in c else ic.avail_counts(c["avail"], w, h)
        d[i]["top_off"], d[i]["left_off"], d[i]["left_stride"] = to + gt + 1, lo + gl, 1
        to, lo = to + gt + len(top), lo + gl + len(left)
        d[i]["dst_off"], d[i]["dst_stride"], d[i]["top_plane"], d[i]["left_plane"] = y * SD + x, SD, PLANE_T, PLANE_L
        d[i]["w"], d[i]["h"], d[i]["mode"], d[i]["angle_delta"], d[i]["filter_intra_mode"] = w, h, c["mode"], c["delta"], c["fi"]
        d[i]["n_top_px"], d[i]["n_topright_px"], d[i]["n_left_px"], d[i]["n_bottomleft_px"] = nt, ntr, nl, nbl
        d[i]["disable_edge_filter"], d[i]["filt_type"] = c["disable"], c["filt_type"]
        want[y:y + h, x:x + w] = ic.build_intra_predictors(top, left, w, h, c["mode"], c["delta"], c["fi"], nt, ntr, nl, nbl, c["disable"], c["filt_type"], bd)
    return np.concatenate(tops).astype(dt), np.concatenate(lefts).astype(dt), d, want, fill


def launch(be, T, L, d, dst, bd, status=None, keep=None):
    planes = be.pkg.IntraPredPlanes()
    dT, dL, dd = be.dev(T), be.dev(L), be.dev(d)
    planes.base[PLANE_T], planes.base[PLANE_L] = be.ptr(dT), be.ptr(dL)
    if keep is not None:
        keep.extend([dT, dL, dd])
    return be.lib.svt_hip_intra_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(d), bd, None if status is None else be.ptr(status), be.stream)


def run(be, cases, bd, seed, with_status=False):
    g = rng(seed)
    T, L, d, want, fill = build(be, cases, bd, g)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    status = be.dev(np.full(len(cases), 7, np.uint8)) if with_status else None
    assert launch(be, T, L, d, dst, bd, status) == 0
    got = be.host(dst)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        for i, c in enumerate(cases):  # name the first block that differs, or say that the damage is outside every block
            y, x = divmod(int(d[i]["dst_off"]), SD)
            a, b = got[y:y + c["h"], x:x + c["w"]], want[y:y + c["h"], x:x + c["w"]]
            assert np.array_equal(a, b), (bd, i, {k: v for k, v in c.items() if k not in ("top", "left")}, np.argwhere(a != b)[:4], a[:2, :8], b[:2, :8])
        raise AssertionError("samples outside every block's w x h were written: %s" % (np.argwhere(got != want)[:8],))


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_every_size_mode_delta(be, bd):
    """all 19 sizes x 13 modes x 7 deltas and the 5 filter-intra modes at w, h <= 32 in ONE launch: availability classes, filt_type, disable_edge_filter and input
    classes cycle (the very list tests/test_intrapred_ref.py pins on the reference)"""
    cases = ic.every_case()
    assert len(cases) == 19 * 13 * 7 + 14 * 5
    run(be, cases, bd, 100 + bd, with_status=bd == 10)


@pytest.mark.parametrize("bd", (8, 10))
def test_corner_filter_threshold(be, bd):
    """filter_intra_edge_corner runs from w + h = 24 on: every zone-2 angle at w + h = 20 (4x16, 16x4) and 24 (8x16, 16x8), both filt_types; the edge filters that
    follow read the filtered corner"""
    cases = [ic.case(w, h, m, d, filt_type=ft, kind=("random", "checker")[ft]) for (w, h) in ((4, 16), (16, 4), (8, 16), (16, 8)) for (m, d) in DIRECTIONAL
             if 90 < ic.MODE_TO_ANGLE[m] + 3 * d < 180 for ft in (0, 1)]
    run(be, cases, bd, 110 + bd)


@pytest.mark.parametrize("bd", (8, 12))
def test_each_edge_filter_strength(be, bd):
    """every strength 0 .. 3 on the above edge and on the left edge, on full, partial and extended edges"""
    cases, seen_a, seen_l = [], set(), set()
    for (w, h) in ((4, 4), (8, 8), (16, 8), (16, 16), (32, 32), (64, 64)):
        for (m, d) in DIRECTIONAL:
            ang = ic.MODE_TO_ANGLE[m] + 3 * d
            if ang in (90, 180):
                continue
            for ft in (0, 1):
                for avail in ("all", "part_top", "part_left"):
                    cases.append(ic.case(w, h, m, d, avail=avail, filt_type=ft, kind="random" if ft else "ramp"))
                if ang < 180:
                    seen_a.add(ic.edge_filter_strength(w, h, ang - 90, ft))
                if ang > 90:
                    seen_l.add(ic.edge_filter_strength(h, w, ang - 180, ft))
    assert seen_a == {0, 1, 2, 3} and seen_l == {0, 1, 2, 3}
    run(be, cases, bd, 120 + bd)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_upsampling_on_and_off(be, bd):
    """svt_aom_use_intra_edge_upsample: w + h = 8 (both filt_types upsample), 16 (filt_type 0 only), 20 (never); every directional angle; the maximum / zero checkerboard
    drives the upsampler into its clip"""
    cases, on = [], {0: set(), 1: set()}
    for (w, h) in ((4, 4), (8, 8), (4, 8), (4, 16), (16, 4)):
        for (m, d) in DIRECTIONAL:
            for ft in (0, 1):
                for kind in ("checker", "random"):
                    cases.append(ic.case(w, h, m, d, filt_type=ft, kind=kind))
                on[ft].add((w + h, bool(ic.use_upsample(w, h, ic.MODE_TO_ANGLE[m] + 3 * d - 90, ft))))
    assert {(8, True), (16, True), (20, False)} <= on[0] and {(8, True), (16, False), (12, False)} <= on[1]
    run(be, cases, bd, 130 + bd)


@pytest.mark.parametrize("bd", (8, 10))
def test_partial_top_with_need_right(be, bd):
    """zone 1 with n_top_px < w: the replicated sample starts inside the block's width and the edge filter's n_px = n_top_px + 1 + h ends before the filled length"""
    cases = []
    for (w, h) in ((4, 4), (8, 16), (16, 16), (32, 8), (64, 64)):
        for (m, d) in DIRECTIONAL:
            if ic.MODE_TO_ANGLE[m] + 3 * d < 90:
                for nt in (1, w // 2, w - 1):
                    c = ic.case(w, h, m, d, filt_type=nt & 1)
                    c["counts"] = (nt, 0, h, 0)
                    cases.append(c)
    run(be, cases, bd, 140 + bd)


def test_dc_at_every_count():
    """not a GPU matter: the twelve values w + h takes over the 19 sizes, seven of them no power of two -- the kernel divides ONCE per tile on a wave-uniform value
    with the integer division of the language, so there is no reciprocal to prove; this pins the list the next test walks"""
    counts = sorted({w + h for (w, h) in ic.TX_SIZES})
    assert counts == [8, 12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128] and sum(1 for c in counts if c & (c - 1)) == 7


def test_dc_sums_at_the_rounding_boundaries(be):
    """DC at all twelve counts (and the w-only / h-only counts of dc_top / dc_left) with all-max 12-bit edges, and with sums one below and exactly at a multiple of
    the count (where (sum + (count >> 1)) / count changes)"""
    g, bd, cases = rng(150), 12, []
    for (w, h) in ic.TX_SIZES:
        for avail in ("all", "top", "left"):
            n = (w if avail != "left" else 0) + (h if avail != "top" else 0)
            base = ic.case(w, h, ic.DC, avail=avail)
            for variant in ("max", "at", "below", "half", "half_below"):
                top, left = np.full(1 + 2 * w, 4095, np.int64), np.full(2 * h, 4095, np.int64)
                if variant != "max":
                    q = int(g.integers(200, 3900))
                    top[:], left[:] = q, q  # sum = q * n: a multiple of the count
                    off = {"at": 0, "below": -1, "half": n - (n >> 1), "half_below": n - (n >> 1) - 1}[variant]
                    (top if avail != "left" else left)[1 if avail != "left" else 0] += off - (n if off > 0 else 0)
                c = dict(base)
                c["top"], c["left"] = top, left
                cases.append(c)
    run(be, cases, bd, 151)


@pytest.mark.parametrize("bd", (8, 10))
def test_left_stride_reads_a_picture_column(be, bd):
    """left_stride = the picture stride: top row, corner and left column are read in place from ONE reconstructed plane (top_plane == left_plane), the prediction goes to
    another; next to it the same blocks through neighbour arrays (left_stride 1) must give the same samples"""
    g = rng(160 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    pic = g.integers(0, 1 << bd, (200, SP)).astype(dt)
    blocks = [(w, h, m, d, fi) for (w, h) in ((4, 4), (8, 16), (16, 16), (32, 8), (64, 64), (16, 64)) for (m, d, fi) in
              [(m, d, 5) for (m, d) in CANDIDATES[::3]] + ([(ic.DC, 0, 2)] if w <= 32 and h <= 32 else [])]
    n = len(blocks)
    d = np.zeros(n, be.pkg.IntraPredDesc)
    fill = 0xA5A5 if bd > 8 else 0xA5
    cases = [ic.case(w, h, m, dl, fi, filt_type=i & 1) for i, (w, h, m, dl, fi) in enumerate(blocks)]
    pos, rows = _place(cases, g)
    want = np.full((rows + 2, SD), fill, dt)
    for i, ((w, h, m, dl, fi), (x, y)) in enumerate(zip(blocks, pos)):
        by, bx = 1 + int(g.integers(0, 200 - 2 * h - 1)), 1 + int(g.integers(0, SP - 2 * w - 1))
        d[i]["top_off"], d[i]["left_off"], d[i]["left_stride"] = (by - 1) * SP + bx, by * SP + bx - 1, SP
        d[i]["dst_off"], d[i]["dst_stride"], d[i]["w"], d[i]["h"], d[i]["mode"], d[i]["angle_delta"], d[i]["filter_intra_mode"] = y * SD + x, SD, w, h, m, dl, fi
        d[i]["n_top_px"], d[i]["n_topright_px"], d[i]["n_left_px"], d[i]["n_bottomleft_px"], d[i]["filt_type"] = w, w, h, h, i & 1
        want[y:y + h, x:x + w] = ic.build_intra_predictors(pic[by - 1, bx - 1:bx + 2 * w], pic[by:by + 2 * h, bx - 1], w, h, m, dl, fi, w, w, h, h, 0, i & 1, bd)
    planes = be.pkg.IntraPredPlanes()
    dp, dd, dst = be.dev(pic), be.dev(d), be.dev(np.full(want.shape, fill, dt))
    planes.base[0] = be.ptr(dp)
    assert be.lib.svt_hip_intra_pred_batch(planes, be.ptr(dst), be.ptr(dd), n, bd, None, be.stream) == 0
    assert np.array_equal(be.host(dst), want)


def test_golden_cases(be):
    """the cases of tests/golden/intrapred.npz: the kernel == what the reference's C computed (and == the restatement), from the RECORDED inputs"""
    gold = ic.load_golden()
    cases = ic.golden_cases()
    assert int(gold["seed"][0]) == ic.GOLDEN_SEED and len(cases) >= 60
    for bd in BIT_DEPTHS:
        idx = [i for i, (b, _) in enumerate(cases) if b == bd]
        cs = []
        for i in idx:
            c = dict(cases[i][1])
            c["top"], c["left"] = gold["top_%d" % i].astype(np.int64), gold["left_%d" % i].astype(np.int64)
            assert np.array_equal(c["top"], ic.golden_inputs(i, bd, c)[0]), "the generator of the golden inputs changed"
            cs.append(c)
        g = rng(170 + bd)
        T, L, d, want, fill = build(be, cs, bd, g)
        for j, i in enumerate(idx):
            y, x = divmod(int(d[j]["dst_off"]), SD)
            assert np.array_equal(want[y:y + cs[j]["h"], x:x + cs[j]["w"]], gold["out_%d" % i]), (i, cases[i])
        dst = be.dev(np.full(want.shape, fill, want.dtype))
        assert launch(be, T, L, d, dst, bd) == 0
        assert np.array_equal(be.host(dst), want), bd


@pytest.mark.parametrize("n", [1, 15, 16, 17, 40])
def test_launch_sizes_around_a_workgroup(be, n):
    """1, B - 1, B, B + 1 and 2B + B / 2 descriptors (B = 16 descriptors per workgroup), 4x4 blocks mixed with 64x64 ones (four tiles each): the prefix-sum dealing at
    its boundaries"""
    B = be.pkg.INTRA_DESCS_PER_WORKGROUP
    assert B == 16 and n in (1, B - 1, B, B + 1, 2 * B + B // 2)
    cases = [ic.case(*((64, 64) if i % 3 == 0 else (4, 4)), CANDIDATES[(7 * i + n) % 61][0], CANDIDATES[(7 * i + n) % 61][1], avail=ic.AVAIL[i % 8] if i % 2 else "all")
             for i in range(n)]
    run(be, cases, 10, 180 + n, with_status=n == 17)


# ---- chroma from luma ------------------------------------------------------------------------------------------------------------------------------------
def cfl_build(be, specs, bd, g, luma_kind="random"):
    """specs: [(w, h, (alpha, ..), in_place)].  Luma plane of stride SP, DC-prediction plane and destination plane of stride SD (in place: the same plane)."""
    dt = np.uint16 if bd > 8 else np.uint8
    fill = 0xA5A5 if bd > 8 else 0xA5
    cases = [dict(w=w * len(al), h=h) for (w, h, al, _) in specs]
    pos, rows = _place([dict(w=c["w"] + 2, h=c["h"]) for c in cases], g)
    lrows = 2 * rows + 4
    luma = (np.full((lrows, 2 * SD), (1 << bd) - 1, dt) if luma_kind == "max" else g.integers(0, 1 << bd, (lrows, 2 * SD)).astype(dt))
    pred = g.integers(0, 1 << bd, (rows + 2, SD)).astype(dt)
    want, want_ip = np.full((rows + 2, SD), fill, dt), pred.copy()
    d = np.zeros(len(specs), be.pkg.CflPredDesc)
    for i, ((w, h, alphas, in_place), (x, y)) in enumerate(zip(specs, pos)):
        d[i]["luma_off"], d[i]["luma_stride"], d[i]["luma_plane"] = 2 * y * 2 * SD + 2 * x + 1, 2 * SD, 0
        d[i]["w"], d[i]["h"], d[i]["n_targets"] = w, h, len(alphas)
        lum = luma[2 * y:2 * y + 2 * h, 2 * x + 1:2 * x + 1 + 2 * w]
        for t, a in enumerate(alphas):
            xt = x + t * (w + 1)
            d[i]["pred_off"][t], d[i]["pred_stride"][t], d[i]["pred_plane"][t] = y * SD + xt, SD, 1
            d[i]["dst_off"][t], d[i]["dst_stride"][t], d[i]["alpha_q3"][t] = y * SD + xt, SD, a
            out = ic.cfl_full(lum, pred[y:y + h, xt:xt + w], w, h, a, bd)
            want[y:y + h, xt:xt + w] = out
            want_ip[y:y + h, xt:xt + w] = out
    return luma, pred, d, want, want_ip, fill


@pytest.mark.parametrize("bd", BIT_DEPTHS)
@pytest.mark.parametrize("luma_kind", ["random", "max"])
def test_cfl_every_size_and_alpha(be, bd, luma_kind):
    """every size of the CFL_SUB_AVG_FN table x alpha_q3 in {-16, -1, 0, 1, 16}, one and two targets (Cb and Cr share the AC values), into a separate destination
    and in place (dst == the DC prediction); luma all-max is where (a + b + c + d) << 1 comes closest to the int16_t narrowing"""
    g = rng(200 + bd)
    alphas = (-16, -1, 0, 1, 16)
    specs = []
    for k, (w, h) in enumerate(ic.CFL_SIZES):
        for j, a in enumerate(alphas):
            specs.append((w, h, (a,), False))
            specs.append((w, h, (a, alphas[(j + k + 1) % 5]), False))
    luma, pred, d, want, want_ip, fill = cfl_build(be, specs, bd, g, luma_kind)
    planes = be.pkg.IntraPredPlanes()
    dl, dp, dd = be.dev(luma), be.dev(pred), be.dev(d)
    planes.base[0], planes.base[1] = be.ptr(dl), be.ptr(dp)
    dst, status = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(len(specs), 7, np.uint8))
    assert be.lib.svt_hip_cfl_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(specs), bd, be.ptr(status), be.stream) == 0
    assert np.array_equal(be.host(dst), want) and not be.host(status).any()
    assert np.array_equal(be.host(dp), pred)  # the DC prediction is only read
    assert be.lib.svt_hip_cfl_pred_batch(planes, be.ptr(dp), be.ptr(dd), len(specs), bd, None, be.stream) == 0  # in place
    assert np.array_equal(be.host(dp), want_ip)


def test_cfl_invalid_descriptors(be):
    g = rng(210)
    specs = [(8, 8, (3,), False), (16, 8, (-5, 7), False), (4, 4, (1,), False)]
    luma, pred, d, want, _, fill = cfl_build(be, specs, 8, g)
    for what in ("4x32", "width 12", "no targets", "NULL plane"):
        e = d.copy()
        if what == "4x32":
            e["w"][1], e["h"][1] = 4, 32
        elif what == "width 12":
            e["w"][1] = 12
        elif what == "no targets":
            e["n_targets"][1] = 0
        else:
            e["pred_plane"][1, 1] = 9
        w2 = want.copy()
        y, x = divmod(int(d[1]["dst_off"][0]), SD)
        w2[y:y + 8, x:x + 33] = fill
        planes = be.pkg.IntraPredPlanes()
        dl, dp, dd = be.dev(luma), be.dev(pred), be.dev(e)
        planes.base[0], planes.base[1] = be.ptr(dl), be.ptr(dp)
        dst, status = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(3, 7, np.uint8))
        assert be.lib.svt_hip_cfl_pred_batch(planes, be.ptr(dst), be.ptr(dd), 3, 8, None, be.stream) == -1
        assert np.all(be.host(dst) == fill), what
        assert be.lib.svt_hip_cfl_pred_batch(planes, be.ptr(dst), be.ptr(dd), 3, 8, be.ptr(status), be.stream) == 0
        assert np.array_equal(be.host(dst), w2) and be.host(status).tolist() == [0, 1, 0], what


# ---- the single-call forms ---------------------------------------------------------------------------------------------------------------------------------
def _host_edge(bd, values, lo):
    e = ic.Edge(bd, values, lo)
    a = e.a.astype(np.uint16 if bd > 8 else np.uint8)
    return a, a.ctypes.data + e.org * a.itemsize, e


def test_per_call_forms(be):
    """The eleven forms against the restatement.  The directional six: every derivative, with and without upsampled edges, dst with its own stride and nothing written
    outside w x h; filter-intra: every mode at every size it accepts; the CfL four: every size, including svt_cfl_predict in place (dst == pred)."""
    L, g = be.lib, rng(300)
    for bd in BIT_DEPTHS:
        dt = np.uint16 if bd > 8 else np.uint8
        fill = 0xA5A5 if bd > 8 else 0xA5
        pre = "svt_av1_highbd_dr_prediction_z%d_hip" if bd > 8 else "svt_av1_dr_prediction_z%d_hip"
        tail = [bd] if bd > 8 else []
        for (w, h) in ((4, 4), (8, 4), (4, 8), (8, 8), (16, 16), (32, 8), (64, 64), (16, 64)):
            ups = (0, 1) if w + h <= 16 else (0,)
            n = ((w + h) << (1 if w + h <= 16 else 0)) + 2
            aa, pa, ea = _host_edge(bd, ic.make_samples(g, "random", n + 2, bd), -2)
            al, pl, el = _host_edge(bd, ic.make_samples(g, "checker" if w == 8 else "random", n + 2, bd)[::-1], -2)
            for k, ang in enumerate(a for a in range(1, 90) if ic.DR_DERIVATIVE[a]):
                if w * h > 256 and k % 5:
                    continue
                dv, d2 = int(ic.DR_DERIVATIVE[ang]), int(ic.DR_DERIVATIVE[90 - ang])
                for up in ups:
                    dst = np.full((h + 1, w + 3), fill, dt)
                    want = np.full_like(dst, fill)
                    getattr(L, pre % 1)(p(dst), dst.shape[1], w, h, pa, pl, up, dv, 1, *tail)
                    want[:h, :w] = ic.dr_z1(ea, w, h, up, dv, bd)
                    assert np.array_equal(dst, want), (bd, 1, w, h, up, ang)
                    getattr(L, pre % 3)(p(dst), dst.shape[1], w, h, pa, pl, up, 1, dv, *tail)
                    want[:h, :w] = ic.dr_z3(el, w, h, up, dv, bd)
                    assert np.array_equal(dst, want), (bd, 3, w, h, up, ang)
                    for upl in (ups if d2 else ()):
                        want[:h, :w] = ic.dr_z2(ea, el, w, h, up, upl, dv, d2, bd)
                        getattr(L, pre % 2)(p(dst), dst.shape[1], w, h, pa, pl, up, upl, dv, d2, *tail)
                        assert np.array_equal(dst, want), (bd, 2, w, h, up, upl, ang)
        n8 = "hbd" if bd > 8 else "lbd"
        for (w, h) in ic.CFL_SIZES:
            luma = g.integers(0, 1 << bd, (2 * h + 1, 2 * w + 5)).astype(dt)
            q3 = np.full((h, ic.CFL_BUF_LINE), 0x5A5A, np.int16)
            getattr(L, "svt_cfl_luma_subsampling_420_%s_hip" % n8)(p(luma), luma.shape[1], p(q3), 2 * w, 2 * h)
            wq = np.full_like(q3, 0x5A5A)
            wq[:, :w] = ic.cfl_subsample_420(luma, w, h)
            assert np.array_equal(q3, wq), (bd, w, h)
            ac = np.full((h, ic.CFL_BUF_LINE), 0x5A5A, np.int16)
            ac[:, :w] = ic.cfl_subtract_average(wq[:, :w], w, h)
            pred = g.integers(0, 1 << bd, (h + 1, w + 3)).astype(dt)
            for alpha in (-16, 5):
                dst = np.full((h + 2, w + 1), fill, dt)
                want = np.full_like(dst, fill)
                want[:h, :w] = ic.cfl_predict(ac[:, :w], pred[:h, :w], alpha, bd, bd == 8)
                getattr(L, "svt_cfl_predict_%s_hip" % n8)(p(ac), p(pred), pred.shape[1], p(dst), dst.shape[1], alpha, bd, w, h)
                assert np.array_equal(dst, want), (bd, w, h, alpha)
            inp = pred.copy()  # in place
            getattr(L, "svt_cfl_predict_%s_hip" % n8)(p(ac), p(inp), inp.shape[1], p(inp), inp.shape[1], 7, bd, w, h)
            want = pred.copy()
            want[:h, :w] = ic.cfl_predict(ac[:, :w], pred[:h, :w], 7, bd, bd == 8)
            assert np.array_equal(inp, want), (bd, w, h)
    for tx, (w, h) in enumerate(ic.TX_SIZES):
        aa, pa, ea = _host_edge(8, ic.make_samples(g, "random", w + 1, 8), -1)
        al, pl, el = _host_edge(8, ic.make_samples(g, "random", h, 8), 0)
        for fm in range(5):
            dst = np.full((h + 1, w + 3), 0xA5, np.uint8)
            L.svt_av1_filter_intra_predictor_hip(p(dst), dst.shape[1], tx, pa, pl, fm)
            want = np.full_like(dst, 0xA5)
            if w <= 32 and h <= 32:
                want[:h, :w] = ic.filter_intra_pred(ea, el, w, h, fm, 8)
            assert np.array_equal(dst, want), (w, h, fm)  # (a 64-wide TxSize is outside the accepted range: nothing is written)
    assert L.svt_hip_debug_commit_violations() == 0


def test_per_call_forms_reject_arguments_outside_the_accepted_range(be):
    """a size outside the 19, an upsampling flag at w + h > 16, dx = 0, bd 9, a CfL size outside the table: nothing is written"""
    L = be.lib
    a8, a16 = np.full(300, 50, np.uint8), np.full(300, 50, np.uint16)
    dst8, dst16 = np.full((64, 64), 0xA5, np.uint8), np.full((64, 64), 0xA5A5, np.uint16)
    L.svt_av1_dr_prediction_z1_hip(p(dst8), 64, 12, 8, a8.ctypes.data + 16, a8.ctypes.data + 16, 0, 64, 1)
    L.svt_av1_dr_prediction_z1_hip(p(dst8), 64, 16, 16, a8.ctypes.data + 16, a8.ctypes.data + 16, 1, 64, 1)
    L.svt_av1_dr_prediction_z2_hip(p(dst8), 64, 8, 8, a8.ctypes.data + 16, a8.ctypes.data + 16, 0, 0, 0, 64)
    L.svt_av1_dr_prediction_z3_hip(p(dst8), 64, 8, 8, a8.ctypes.data + 16, a8.ctypes.data + 16, 0, 1, 0)
    L.svt_av1_highbd_dr_prediction_z1_hip(p(dst16), 64, 8, 8, a16.ctypes.data + 32, a16.ctypes.data + 32, 0, 64, 1, 9)
    L.svt_av1_filter_intra_predictor_hip(p(dst8), 64, 0, a8.ctypes.data + 16, a8.ctypes.data + 16, 5)
    q3 = np.zeros((32, 32), np.int16)
    L.svt_cfl_predict_lbd_hip(p(q3), p(a8), 4, p(dst8), 64, 1, 8, 4, 32)
    L.svt_cfl_predict_hbd_hip(p(q3), p(a16), 8, p(dst16), 64, 1, 13, 8, 8)
    L.svt_cfl_luma_subsampling_420_lbd_hip(p(dst8), 64, p(q3), 24, 16)
    assert np.all(dst8 == 0xA5) and np.all(dst16 == 0xA5A5) and not q3.any()


# ---- invalid descriptors, the read guard, the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["size 8x64", "width 12", "mode 13", "delta 4", "delta -4", "filter-intra at 64 wide", "filter-intra mode 6", "top-right without the whole top",
                                  "bottom-left without the whole left", "n_top_px above w", "NULL top plane", "NULL left plane"])
def test_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones: with status == NULL the call returns -1 and not one destination byte changes; with a status array it returns 0,
    flags that descriptor alone, leaves its block untouched and predicts the other two"""
    g = rng(9)
    cases = [ic.case(8, 8, ic.D135, 2), ic.case(16, 16, ic.D67, -1), ic.case(4, 4, ic.PAETH, fi=3)]
    T, L, d, want, fill = build(be, cases, 8, g)
    y, x = divmod(int(d[1]["dst_off"]), SD)
    want[y:y + 16, x:x + 16] = fill
    if what == "size 8x64":
        d["w"][1], d["h"][1], d["n_top_px"][1], d["n_topright_px"][1] = 8, 64, 8, 8
    elif what == "width 12":
        d["w"][1], d["n_top_px"][1], d["n_topright_px"][1] = 12, 12, 12
    elif what == "mode 13":
        d["mode"][1] = 13
    elif what.startswith("delta"):
        d["angle_delta"][1] = int(what.split()[1])
    elif what == "filter-intra at 64 wide":
        d["w"][1], d["filter_intra_mode"][1] = 64, 0
    elif what == "filter-intra mode 6":
        d["filter_intra_mode"][1] = 6
    elif what == "top-right without the whole top":
        d["n_top_px"][1], d["n_topright_px"][1] = 15, 4
    elif what == "bottom-left without the whole left":
        d["n_left_px"][1], d["n_bottomleft_px"][1] = 8, 1
    elif what == "n_top_px above w":
        d["n_top_px"][1], d["n_topright_px"][1] = 17, 0
    elif what == "NULL top plane":
        d["top_plane"][1] = 5
    else:
        d["left_plane"][1] = 31
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    assert launch(be, T, L, d, dst, 8) == -1
    assert np.all(be.host(dst) == fill)
    status = be.dev(np.full(3, 7, np.uint8))
    assert launch(be, T, L, d, dst, 8, status) == 0
    assert np.array_equal(be.host(dst), want)
    assert be.host(status).tolist() == [0, 1, 0]
    planes = be.pkg.IntraPredPlanes()
    assert be.lib.svt_hip_intra_pred_batch(planes, be.ptr(dst), be.ptr(status), 1, 9, None, be.stream) == -1  # not a bit depth


def _guarded(n_bytes):
    """a mapping whose neighbouring pages are inaccessible: (mmap, address of its first readable byte, readable length)"""
    page = mmap.PAGESIZE
    body = (n_bytes + page - 1) // page * page
    m = mmap.mmap(-1, body + 2 * page)
    base = C.addressof(C.c_char.from_buffer(m))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes, libc.mprotect.restype = [C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0
    return m, page, body


def test_read_guard_on_the_emulator():
    """CPU only.  Both edges lie flush against inaccessible pages, once with the LAST readable sample on the mapping's last byte and once with the FIRST one on its
    first byte: top is read only inside [-1, n_top_px + n_topright_px), [-1] only when n_top_px > 0 and n_left_px > 0, nothing of it when n_top_px == 0; left only
    inside [0, n_left_px + n_bottomleft_px); CfL reads luma only inside 2w x 2h and the DC prediction inside w x h.  A read outside by one sample leaves the mapping."""
    be = _backends.setdefault("emu", EmuBackend())
    g = rng(77)
    for bd in (8, 10):
        dt = np.dtype(np.uint16 if bd > 8 else np.uint8)
        for (w, h) in ((4, 4), (8, 16), (32, 32), (64, 64), (64, 16)):
            for avail in ic.AVAIL:
                nt, ntr, nl, nbl = ic.avail_counts(avail, w, h)
                corner = 1 if nt > 0 and nl > 0 else 0
                n_top, n_left = corner + nt + ntr, nl + nbl
                for at_end in (True, False):
                    maps, planes, arrs = [], be.pkg.IntraPredPlanes(), []
                    for k, n in enumerate((n_top, n_left)):
                        m, page, body = _guarded(max(n, 1) * dt.itemsize)
                        start = page + (body - n * dt.itemsize if at_end else 0)
                        a = np.frombuffer(m, dt, n, start)
                        a[:] = g.integers(0, 1 << bd, n)
                        base = C.addressof(C.c_char.from_buffer(m)) + start
                        # a pointer is formed even where nothing may be read: one sample INSIDE the guard page's neighbour would hide a stray read, so point at the edge
                        planes.base[k] = base if n else C.addressof(C.c_char.from_buffer(m)) + page
                        maps.append(m)
                        arrs.append(a)
                    cand = CANDIDATES + ([(ic.DC, 0)] * 5 if w <= 32 and h <= 32 else [])
                    d = np.zeros(len(cand), be.pkg.IntraPredDesc)
                    top_full = np.zeros(1 + 2 * w, np.int64)
                    top_full[1 - corner:1 - corner + n_top] = arrs[0]
                    left_full = np.zeros(2 * h, np.int64)
                    left_full[:n_left] = arrs[1]
                    for i, (mm, dl) in enumerate(cand):
                        fi = i - 61 if i >= 61 else 5
                        d[i]["top_off"], d[i]["left_off"], d[i]["left_stride"], d[i]["left_plane"] = corner, 0, 1, 1
                        d[i]["dst_off"], d[i]["dst_stride"], d[i]["w"], d[i]["h"] = i * w * h, w, w, h
                        d[i]["mode"], d[i]["angle_delta"], d[i]["filter_intra_mode"], d[i]["filt_type"] = mm, dl, fi, i & 1
                        d[i]["n_top_px"], d[i]["n_topright_px"], d[i]["n_left_px"], d[i]["n_bottomleft_px"] = nt, ntr, nl, nbl
                    dst = np.zeros(len(cand) * w * h, dt)
                    assert be.lib.svt_hip_intra_pred_batch(planes, p(dst), p(d), len(cand), bd, None, None) == 0
                    for i, (mm, dl) in enumerate(cand):
                        fi = i - 61 if i >= 61 else 5
                        want = ic.build_intra_predictors(top_full, left_full, w, h, mm, dl, fi, nt, ntr, nl, nbl, 0, i & 1, bd)
                        assert np.array_equal(dst[i * w * h:(i + 1) * w * h].reshape(h, w), want), (bd, w, h, avail, at_end, mm, dl, fi)
                    del arrs, a, maps
        for (w, h) in ((4, 4), (8, 32), (32, 32)):
            for at_end in (True, False):
                n = 4 * w * h
                ml, page, body = _guarded(n * dt.itemsize)
                mp, _, bodyp = _guarded(w * h * dt.itemsize)
                sl, sp = page + (body - n * dt.itemsize if at_end else 0), page + (bodyp - w * h * dt.itemsize if at_end else 0)
                luma, pred = np.frombuffer(ml, dt, n, sl).reshape(2 * h, 2 * w), np.frombuffer(mp, dt, w * h, sp).reshape(h, w)
                luma[:], pred[:] = g.integers(0, 1 << bd, luma.shape), g.integers(0, 1 << bd, pred.shape)
                planes = be.pkg.IntraPredPlanes()
                planes.base[0], planes.base[1] = C.addressof(C.c_char.from_buffer(ml)) + sl, C.addressof(C.c_char.from_buffer(mp)) + sp
                d = np.zeros(1, be.pkg.CflPredDesc)
                d["luma_stride"], d["w"], d["h"], d["n_targets"] = 2 * w, w, h, 2
                d["pred_stride"], d["pred_plane"], d["dst_stride"], d["dst_off"], d["alpha_q3"] = w, 1, w, (0, w * h), (9, -9)
                dst = np.zeros(2 * w * h, dt)
                assert be.lib.svt_hip_cfl_pred_batch(planes, p(dst), p(d), 1, bd, None, None) == 0
                for t, a in enumerate((9, -9)):
                    assert np.array_equal(dst[t * w * h:(t + 1) * w * h].reshape(h, w), ic.cfl_full(luma, pred, w, h, a, bd)), (bd, w, h, at_end, t)
                del luma, pred, ml, mp


@pytest.mark.parametrize("bd", (8, 10))
def test_intra_candidates_feed_distortion(be, bd):
    """one 16x16 and one 8x32 source block: all 61 (mode, delta) candidates plus the 5 filter-intra modes predicted in ONE launch (the asynchronous form: a status
    array), then svt_hip_pixel_dist_batch on the same stream with no host synchronisation between the two: the SSE vector and its argmin == numpy's"""
    g = rng(600 + bd)
    cases, owner = [], []
    shared = {}
    for b, (w, h) in enumerate(((16, 16), (8, 32))):
        top, left = ic.make_samples(g, "random", 1 + 2 * w, bd), ic.make_samples(g, "ramp", 2 * h, bd)
        shared[b] = g.integers(0, 1 << bd, (h, w))
        for (m, dl) in CANDIDATES:
            cases.append(dict(ic.case(w, h, m, dl, filt_type=b), top=top, left=left))
            owner.append(b)
        for fi in range(5):
            cases.append(dict(ic.case(w, h, ic.DC, 0, fi), top=top, left=left))
            owner.append(b)
    assert len(cases) == 2 * 66
    T, L, d, want, fill = build(be, cases, bd, g)
    n = len(cases)
    src = np.zeros(want.shape, want.dtype)
    for i, c in enumerate(cases):  # the candidate's copy of its block's source samples, where the prediction will lie
        y, x = divmod(int(d[i]["dst_off"]), SD)
        src[y:y + c["h"], x:x + c["w"]] = shared[owner[i]]
    dst, status, keep = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(n, 7, np.uint8)), []
    dsrc, sse = be.dev(src), be.dev(np.full(n, 0xDEADBEEF, np.uint64))
    dd = np.zeros(n, be.pkg.DistDesc)
    dd["in_off"], dd["rec_off"], dd["in_stride"], dd["rec_stride"], dd["width"], dd["height"] = d["dst_off"], d["dst_off"], SD, SD, d["w"], d["h"]
    ddd = be.dev(dd)
    assert launch(be, T, L, d, dst, bd, status, keep) == 0
    be.lib.svt_hip_pixel_dist_batch(be.ptr(dsrc), be.ptr(dst), be.ptr(ddd), n, int(bd > 8), 1, be.ptr(sse), None, be.stream)
    got = be.host(sse).astype(np.int64)
    ref = np.array([dc.sse(shared[owner[i]], want[divmod(int(d[i]["dst_off"]), SD)[0]:, divmod(int(d[i]["dst_off"]), SD)[1]:][:c["h"], :c["w"]]) for i, c in enumerate(cases)],
                   np.int64)
    assert np.array_equal(got, ref)
    for b in (0, 1):
        m = np.flatnonzero(np.array(owner) == b)
        assert int(np.argmin(got[m])) == int(np.argmin(ref[m]))
    assert not be.host(status).any()
