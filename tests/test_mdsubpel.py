"""csrc/mdsubpel.hip on the emulator (always) and on the MI355X (-m gpu): svt_hip_block_var_batch, svt_hip_md_subpel_search_batch, the limits helper and the single-call
forms against tests/mdsubpel_common.py (numpy; pinned on the reference's C by tests/test_mdsubpel_ref.py) and against tests/golden/mdsubpel.npz (what the reference's C
computed for the same case lists).  Reference planes and source blocks sit at odd lead-ins with odd strides; result arrays lie between sentinel records and are
compared whole.  The restatement's side of a launch is computed once and shared by the backends."""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

import mdsubpel_common as mc
from conftest import GOLDEN, EmuBackend, _backends, p

PLANES = (1, 5, 31)
_cache = {}


def golden():
    if "gold" not in _cache:
        _cache["gold"] = np.load(os.path.join(GOLDEN, "mdsubpel.npz"))
    return _cache["gold"]


def prim():
    """the primitive case list with the restatement's results and clip / tie statistics"""
    if "prim" not in _cache:
        cases, stats = mc.primitive_cases(), {}
        want = np.array([mc.run_primitive(c, stats.setdefault((c["content"][:7], c["kind"] >= mc.OBMC_SAD), {})) for c in cases], np.int64)
        _cache["prim"] = (cases, want, stats)
    return _cache["prim"]


def searches():
    if "search" not in _cache:
        cases = mc.search_cases()
        _cache["search"] = (cases, [mc.run_search(c) for c in cases])
    return _cache["search"]


def pack_primitives(pkg, cases, order):
    """one launch of `cases` in `order`: (planes' buffer, src, wsrc, mask, descs)"""
    d = np.zeros(len(order), pkg.BlockVarDesc)
    bufs, srcs, ws, ms = [np.zeros(3, np.uint8)], [np.zeros(5, np.uint8)], [np.zeros(7, np.int32)], [np.zeros(3, np.int32)]
    pos = [3, 5, 7, 3]
    for i, k in enumerate(order):
        c = cases[k]
        pre, py, px, src, wsrc, mask = mc.primitive_inputs(c)
        H, W = src.shape
        stride, sstride = pre.shape[1] + 1 + 2 * (i % 3), W + 1 + 2 * (i % 4)
        plane = np.zeros((pre.shape[0], stride), np.uint8)
        plane[:, :pre.shape[1]] = pre
        d[i]["pre_off"], d[i]["pre_stride"], d[i]["pre_plane"] = pos[0] + py * stride + px, stride, PLANES[i % 3]
        d[i]["bsize"], d[i]["kind"], d[i]["xoffset"], d[i]["yoffset"], d[i]["taps"] = c["bsize"], c["kind"], c["xo"], c["yo"], c["taps"]
        bufs.append(plane.reshape(-1))
        pos[0] += plane.size
        if c["kind"] >= mc.OBMC_SAD:
            d[i]["wsrc_off"], d[i]["mask_off"] = pos[2], pos[3]
            ws += [wsrc, np.zeros(1 + i % 2, np.int32)]
            ms += [mask, np.zeros(2 - i % 2, np.int32)]
            pos[2] += wsrc.size + 1 + i % 2
            pos[3] += mask.size + 2 - i % 2
        else:
            blk = np.zeros((H, sstride), np.uint8)
            blk[:, :W] = src
            d[i]["src_off"], d[i]["src_stride"] = pos[1], sstride
            srcs.append(blk.reshape(-1))
            pos[1] += blk.size
    return np.concatenate(bufs), np.concatenate(srcs), np.concatenate(ws), np.concatenate(ms), d


def launch_primitives(be, packed, with_status=True):
    buf, src, ws, ms, d = packed
    n = len(d)
    keep = [be.dev(a) for a in (buf, src, ws, ms, d)]
    out = be.dev(np.full((n + 2) * 16, 0xA5, np.uint8))
    status = be.dev(np.full(n + 2, 7, np.uint8)) if with_status else None
    planes = be.pkg.InterPredPlanes()
    for k in PLANES:
        planes.base[k] = be.ptr(keep[0])
    r = be.lib.svt_hip_block_var_batch(planes, be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), be.ptr(keep[4]), n, be.ptr(out) + 16,
                                       None if status is None else be.ptr(status) + 1, be.stream)
    be.sync()
    assert r == 0
    got = be.host(out).view(be.pkg.BlockVarResult)
    assert np.all(got[[0, -1]].view(np.uint8) == 0xA5)
    if with_status:
        st = be.host(status)
        assert st[0] == 7 and st[-1] == 7 and not st[1:-1].any()
    g = got[1:-1]
    return np.stack([g["var"], g["sse"], g["sum"], g["sad"]], 1).astype(np.int64)


def test_restatement_reaches_what_the_cases_are_for():
    """CPU only: both 8-bit clips of both stages bind under the checkerboards, the OBMC differences land on ties of both signs, the sums reach their extremes"""
    cases, want, stats = prim()
    ck = stats[("checker", False)]
    assert all(ck.get(k, 0) > 0 for k in ("h_lo", "h_hi", "v_lo", "v_hi")), ck
    ob = {}
    for (_, obmc), s in stats.items():
        if obmc:
            for k, v in s.items():
                ob[k] = ob.get(k, 0) + v
    assert ob["tie_pos"] > 100 and ob["tie_neg"] > 100
    sat = [w for c, w in zip(cases, want) if c["content"] == "sat_hi" and c["kind"] == mc.VAR][0]
    assert sat[1] == 1065369600 and sat[2] == 255 * 128 * 128 and sat[0] == 0
    sat = [w for c, w in zip(cases, want) if c["content"] == "sat_lo" and c["kind"] == mc.VAR][0]
    assert sat[1] == 1065369600 and sat[2] == -255 * 128 * 128


def test_search_cases_depend_on_every_rule():
    """CPU only: for every early exit and for bias_fp the list holds an item whose result changes when the rule is switched off in the restatement -- a kernel that
    ignored the rule could not pass test_searches"""
    cases, want = searches()
    for rule in mc.RULES:
        hit = [i for i, c in enumerate(cases) if {k: v for k, v in mc.run_search(c, off=(rule,)).items()} != want[i]]
        assert hit, rule
    # both methods take and skip each of their early returns
    for m in (0, 1):
        ev = [w["evals"] for c, w in zip(cases, want) if c.get("method", 0) == m]
        assert min(ev) == 1 and max(ev) >= 12
    # out-of-range candidates exist and steer the diagonal: the cases on a limit evaluate fewer candidates than the ones inside it
    lim = [(c, w) for c, w in zip(cases, want) if c.get("lims")]
    assert len(lim) == 16 and len({w["evals"] for _, w in lim}) > 1
    # the 1/8 sample shifts are found
    found = [c for c, w in zip(cases, want) if c["content"] == "shift" and (w["mv_row"], w["mv_col"]) == tuple(c["true_mv"])]
    assert len(found) >= 10 and any((c["true_mv"][0] | c["true_mv"][1]) & 1 for c in found)


def test_restatement_agrees_with_the_golden_file():
    cases, want, _ = prim()
    gold = golden()
    assert np.array_equal(gold["prim_seeds"], [c["seed"] for c in cases])
    assert np.array_equal(gold["prim_out"], want)
    sc, sw = searches()
    assert np.array_equal(gold["search_seeds"], [c["seed"] for c in sc])
    assert np.array_equal(gold["search_out"], np.array([[w[f] for f in mc.RESULT_FIELDS] for w in sw], np.int64))


def test_every_kind_at_every_size_single_launches(be):
    cases, want, _ = prim()
    for k in range(22 * 6 + 1):
        got = launch_primitives(be, pack_primitives(be.pkg, cases, [k]), with_status=bool(k & 1))
        assert np.array_equal(got[0], want[k]), (cases[k], got[0], want[k])


def test_mixed_launch(be):
    """every primitive case in one launch, permuted: sizes of both launch classes next to each other, odd strides and lead-ins, three plane indices"""
    cases, want, _ = prim()
    order = np.random.default_rng(5).permutation(len(cases))
    if "prim_packed" not in _cache:
        _cache["prim_packed"] = pack_primitives(be.pkg, cases, order)
    got = launch_primitives(be, _cache["prim_packed"])
    bad = np.argwhere((got != want[order]).any(1)).reshape(-1)
    assert not len(bad), [(cases[order[i]], got[i], want[order[i]]) for i in bad[:4]]
    assert np.array_equal(got, golden()["prim_out"][order])


def pack_searches(pkg, cases, order):
    d = np.zeros(len(order), pkg.MdSubpelDesc)
    bufs, srcs = [np.zeros(3, np.uint8)], [np.zeros(5, np.uint8)]
    pos = [3, 5]
    for i, k in enumerate(order):
        c = dict(mc.DEFAULTS)
        c.update(cases[k])
        src, ref, ry, rx = mc.search_inputs(cases[k])
        H, W = src.shape
        stride, sstride = ref.shape[1] + 1 + 2 * (i % 3), W + 1 + 2 * (i % 4)
        plane = np.zeros((ref.shape[0], stride), np.uint8)
        plane[:, :ref.shape[1]] = ref
        blk = np.zeros((H, sstride), np.uint8)
        blk[:, :W] = src
        e = d[i]
        e["ref_off"], e["ref_stride"], e["ref_plane"], e["src_off"], e["src_stride"] = pos[0] + ry * stride + rx, stride, PLANES[i % 3], pos[1], sstride
        lims = c["lims"] if c["lims"] is not None else mc.WIDE_LIMITS
        e["lim_col_min"], e["lim_col_max"], e["lim_row_min"], e["lim_row_max"] = lims
        (e["start_mv_row"], e["start_mv_col"]), (e["ref_mv_row"], e["ref_mv_col"]), (e["best_mvp_row"], e["best_mvp_col"]) = c["start"], c["ref_mv"], c["best_mvp"]
        for f in ("pred_variance_th", "round_dev_th", "bias_fp", "error_per_bit", "early_exit_th", "cost_table", "qp", "hp_mv_th", "best_mvp_err", "bsize", "method",
                  "allow_hp", "forced_stop", "iters_per_step", "abs_th_mult", "skip_diag_refinement", "subpel_search_type", "mv_cost_type", "early_exit", "mvp_th"):
            e[f] = c[f]
        bufs.append(plane.reshape(-1))
        srcs.append(blk.reshape(-1))
        pos[0] += plane.size
        pos[1] += blk.size
    return np.concatenate(bufs), np.concatenate(srcs), d


def device_tables(be):
    t = np.zeros(2, be.pkg.MvCostTable)
    for k, (joint, comp) in enumerate(mc.cost_tables()):
        t[k]["joint"], t[k]["comp"] = joint, comp
    return be.dev(t)


def launch_searches(be, packed, n=None, with_status=True, tables=True):
    buf, src, d = packed
    n = len(d) if n is None else n
    keep = [be.dev(a) for a in (buf, src, d)] + [device_tables(be)]
    out = be.dev(np.full((n + 2) * 24, 0xA5, np.uint8))
    status = be.dev(np.full(n + 2, 7, np.uint8)) if with_status else None
    planes = be.pkg.InterPredPlanes()
    for k in PLANES:
        planes.base[k] = be.ptr(keep[0])
    r = be.lib.svt_hip_md_subpel_search_batch(planes, be.ptr(keep[1]), be.ptr(keep[3]) if tables else None, 2 if tables else 0, be.ptr(keep[2]), n, be.ptr(out) + 24,
                                              None if status is None else be.ptr(status) + 1, be.stream)
    be.sync()
    got = be.host(out).view(be.pkg.MdSubpelResult)
    assert np.all(got[[0, -1]].view(np.uint8) == 0xA5)
    return r, got[1:-1], None if status is None else be.host(status)


FIELDS = mc.RESULT_FIELDS + ("evals",)


def test_searches(be):
    cases, want = searches()
    order = np.random.default_rng(9).permutation(len(cases))
    if "search_packed" not in _cache:
        _cache["search_packed"] = pack_searches(be.pkg, cases, order)
    r, got, st = launch_searches(be, _cache["search_packed"])
    assert r == 0 and st[0] == 7 and st[-1] == 7 and not st[1:-1].any()
    for i, k in enumerate(order):
        g = {f: int(got[i][f]) for f in FIELDS}
        assert g == want[k], (cases[k], g, want[k])
    gold = golden()["search_out"][order]
    assert np.array_equal(np.stack([got[f] for f in mc.RESULT_FIELDS], 1).astype(np.int64), gold)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_search_launch_sizes_around_a_workgroup(be, n):
    """n items, no status array (the check kernel runs), a 128x128 item among 16x16 ones so that both launch classes meet at every workgroup boundary"""
    cases, want = searches()
    big = [i for i, c in enumerate(cases) if c.get("bsize") == 15]
    small = [i for i, c in enumerate(cases) if c.get("bsize", 6) == 6]
    order = (small[:n - 1] + big[:1]) if n > 1 else big[:1]
    order = order[::-1] if n & 1 else order
    r, got, _ = launch_searches(be, pack_searches(be.pkg, cases, order), with_status=False)
    assert r == 0
    for i, k in enumerate(order):
        assert {f: int(got[i][f]) for f in FIELDS} == want[k], (n, cases[k])


def test_no_cost_table_is_cost_zero(be):
    """tables == NULL: MV_COST_ENTROPY costs 0 whatever the index says, as mvcost == NULL does"""
    cases, _ = searches()
    idx = [i for i, c in enumerate(cases) if c.get("mv_cost_type") == 0][:3]
    r, got, _ = launch_searches(be, pack_searches(be.pkg, cases, idx), tables=False)
    assert r == 0
    for i, k in enumerate(idx):
        c = dict(cases[k], cost_table=-1)
        assert {f: int(got[i][f]) for f in FIELDS} == mc.run_search(c), cases[k]


INVALID_VAR = [("bsize", 22, {}), ("kind", 7, {}), ("xoffset", 8, {"kind": mc.SUBPIX}), ("yoffset", 8, {"kind": mc.OBMC_SUBPIX}), ("xoffset", 9, {"kind": mc.UPSAMPLED, "taps": 2}),
               ("taps", 0, {"kind": mc.UPSAMPLED}), ("taps", 4, {"kind": mc.UPSAMPLED}), ("bsize", 9, {"kind": mc.MSE}), ("pre_plane", 32, {}), ("pre_plane", 2, {})]


def test_invalid_primitive_descriptors(be):
    cases, want, _ = prim()
    order = [0, 1, 2] * 4
    packed = pack_primitives(be.pkg, cases, order)
    d = packed[4]
    bad = []
    for i, (field, value, also) in enumerate(INVALID_VAR):
        for f, v in also.items():
            d[i + 1][f] = v
        d[i + 1][field] = value
        bad.append(i + 1)
    buf, src, ws, ms, _ = packed
    keep = [be.dev(a) for a in (buf, src, ws, ms, d)]
    planes = be.pkg.InterPredPlanes()
    for k in PLANES:
        planes.base[k] = be.ptr(keep[0])
    n = len(d)
    out, status = be.dev(np.full(n * 16, 0xA5, np.uint8)), be.dev(np.full(n, 7, np.uint8))
    args = (planes, be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), be.ptr(keep[4]), n, be.ptr(out))
    assert be.lib.svt_hip_block_var_batch(*args, be.ptr(status), be.stream) == 0
    be.sync()
    st, got = be.host(status), be.host(out).view(be.pkg.BlockVarResult)
    assert st.tolist() == [1 if i in bad else 0 for i in range(n)]
    for i in range(n):
        if i in bad:
            assert np.all(got[i:i + 1].view(np.uint8) == 0xA5), i
        else:
            assert [int(got[i][f]) for f in ("var", "sse", "sum", "sad")] == want[order[i]].tolist(), i
    out2 = be.dev(np.full(n * 16, 0xA5, np.uint8))
    assert be.lib.svt_hip_block_var_batch(*args[:-1], be.ptr(out2), None, be.stream) == -1  # checked before anything is launched
    be.sync()
    assert np.all(be.host(out2) == 0xA5)
    # a kind whose base pointer is missing is invalid; the others still run
    assert be.lib.svt_hip_block_var_batch(planes, be.ptr(keep[1]), None, None, be.ptr(keep[4]), 1, be.ptr(out2), None, be.stream) == 0
    d2 = np.array(d[:1])
    d2["kind"] = mc.OBMC_VAR
    k2 = be.dev(d2)
    assert be.lib.svt_hip_block_var_batch(planes, be.ptr(keep[1]), None, be.ptr(keep[3]), be.ptr(k2), 1, be.ptr(out2), None, be.stream) == -1
    be.sync()


INVALID_SEARCH = [("bsize", 22), ("method", 2), ("forced_stop", 4), ("subpel_search_type", 0), ("subpel_search_type", 4), ("mv_cost_type", 6), ("cost_table", 2),
                  ("ref_plane", 32), ("ref_plane", 2)]


def test_invalid_search_descriptors(be):
    cases, want = searches()
    order = list(range(len(INVALID_SEARCH) + 3))
    packed = pack_searches(be.pkg, cases, order)
    bad = []
    for i, (field, value) in enumerate(INVALID_SEARCH):
        packed[2][i + 1][field] = value
        bad.append(i + 1)
    r, got, st = launch_searches(be, packed)
    assert r == 0 and st[1:-1].tolist() == [1 if i in bad else 0 for i in order]
    for i in order:
        if i in bad:
            assert np.all(got[i:i + 1].view(np.uint8) == 0xA5), i
        else:
            assert {f: int(got[i][f]) for f in FIELDS} == want[i], i
    r, got, _ = launch_searches(be, packed, with_status=False)
    assert r == -1 and np.all(got.view(np.uint8) == 0xA5)


def test_nothing_to_do_and_bad_arguments(be):
    planes = be.pkg.InterPredPlanes()
    out = be.dev(np.full(64, 0xA5, np.uint8))
    assert be.lib.svt_hip_block_var_batch(planes, None, None, None, None, 0, None, None, be.stream) == 0
    assert be.lib.svt_hip_md_subpel_search_batch(planes, None, None, 0, None, 0, None, None, be.stream) == 0
    assert be.lib.svt_hip_block_var_batch(planes, None, None, None, None, 1, be.ptr(out), None, be.stream) == -1
    assert be.lib.svt_hip_md_subpel_search_batch(planes, None, None, 0, be.ptr(out), 1, be.ptr(out), None, be.stream) == -1
    be.sync()
    assert np.all(be.host(out) == 0xA5)


def test_mv_limits_helper(be):
    g = np.random.default_rng(3)
    lim = np.zeros(4, np.int32)
    for _ in range(300):
        b = int(g.integers(0, 22))
        mi_rows, mi_cols = int(g.integers(8, 600)), int(g.integers(8, 1000))
        mi_row, mi_col = int(g.integers(0, mi_rows)), int(g.integers(0, mi_cols))
        ref = (int(g.integers(-16384, 16384)), int(g.integers(-16384, 16384))) if g.integers(0, 4) else (int(g.integers(-40, 40)), int(g.integers(-40, 40)))
        assert be.lib.svt_hip_md_subpel_mv_limits(mi_row, mi_col, b, mi_rows, mi_cols, ref[0], ref[1], p(lim)) == 0
        assert tuple(lim.tolist()) == mc.mv_limits(mi_row, mi_col, b, mi_rows, mi_cols, ref), (mi_row, mi_col, b, ref)
    lim[:] = 77
    assert be.lib.svt_hip_md_subpel_mv_limits(0, 0, 22, 10, 10, 0, 0, p(lim)) == -1 and be.lib.svt_hip_md_subpel_mv_limits(0, 0, 3, 10, 10, 0, 0, None) == -1
    assert lim.tolist() == [77] * 4


def test_single_call_forms(be):
    """host pointers, the reference's prototypes: every size of the five families, svt_aom_mse16x16_hip, svt_aom_upsampled_pred_hip"""
    g = np.random.default_rng(21)
    sse = np.zeros(1, np.uint32)
    for k, (W, H) in enumerate(be.pkg.VARIANCE_SIZES):
        b = [i for i in range(22) if (mc.BW[i], mc.BH[i]) == (W, H)][0]
        stride = W + 9 + 2 * k
        pre, src = g.integers(0, 256, (H + 8, stride), dtype=np.uint8), g.integers(0, 256, (H, W + 3), dtype=np.uint8)
        mask = g.integers(0, 4097, W * H).astype(np.int32)
        wsrc = (g.integers(0, 256, W * H) * 4096 + g.integers(-3, 4, W * H) * 2048).astype(np.int32)
        xo, yo = (k * 3) % 8, (k * 5 + 1) % 8
        at, sblk = pre.ctypes.data + 2 * stride + 3, src[:, :W]
        name = "%dx%d_hip" % (W, H)
        sse[0] = 0xA5A5A5A5
        v = getattr(be.lib, "svt_aom_variance" + name)(at, stride, p(src), W + 3, p(sse))
        assert (v, int(sse[0])) == mc.block_var(mc.VAR, b, pre, 2, 3, src=sblk)[:2], name
        v = getattr(be.lib, "svt_aom_sub_pixel_variance" + name)(at, stride, xo, yo, p(src), W + 3, p(sse))
        assert (v, int(sse[0])) == mc.block_var(mc.SUBPIX, b, pre, 2, 3, xo, yo, src=sblk)[:2], name
        v = getattr(be.lib, "svt_aom_obmc_sad" + name)(at, stride, p(wsrc), p(mask))
        assert v == mc.block_var(mc.OBMC_SAD, b, pre, 2, 3, wsrc=wsrc, mask=mask)[3], name
        v = getattr(be.lib, "svt_aom_obmc_variance" + name)(at, stride, p(wsrc), p(mask), p(sse))
        assert (v, int(sse[0])) == mc.block_var(mc.OBMC_VAR, b, pre, 2, 3, wsrc=wsrc, mask=mask)[:2], name
        v = getattr(be.lib, "svt_aom_obmc_sub_pixel_variance" + name)(at, stride, xo, yo, p(wsrc), p(mask), p(sse))
        assert (v, int(sse[0])) == mc.block_var(mc.OBMC_SUBPIX, b, pre, 2, 3, xo, yo, wsrc=wsrc, mask=mask)[:2], name
        comp = np.full(W * H + 2, 0xA5, np.uint8)
        for (xq, yq) in ((0, 0), (xo | 1, 0), (0, yo | 1), (xo | 1, yo | 1)):
            at2 = pre.ctypes.data + 3 * stride + 3
            be.lib.svt_aom_upsampled_pred_hip(None, None, 0, 0, None, comp.ctypes.data + 1, W, H, xq, yq, at2, stride, 1 + k % 3)
            assert np.array_equal(comp[1:-1].reshape(H, W), mc.upsampled_pred(pre, 3, 3, W, H, xq, yq, 1 + k % 3)) and comp[0] == 0xA5 and comp[-1] == 0xA5, (name, xq, yq)
    pre, src = g.integers(0, 256, (16, 19), dtype=np.uint8), g.integers(0, 256, (16, 23), dtype=np.uint8)
    v = be.lib.svt_aom_mse16x16_hip(p(pre), 19, p(src), 23, p(sse))
    assert v == int(sse[0]) == mc.block_var(mc.MSE, 6, pre, 0, 0, src=src[:, :16])[1]
    # outside the accepted range nothing is written
    sse[0] = 0xA5A5A5A5
    assert be.lib.svt_aom_sub_pixel_variance16x16_hip(p(pre), 19, 8, 0, p(src), 23, p(sse)) == 0 and sse[0] == 0xA5A5A5A5
    assert be.lib.svt_aom_variance16x16_hip(None, 19, p(src), 23, p(sse)) == 0 and sse[0] == 0xA5A5A5A5
    comp = np.full(64, 0xA5, np.uint8)
    for args in ((6, 8, 1, 1, 3), (8, 8, 8, 0, 3), (8, 8, 1, 1, 0), (8, 8, 1, 1, 4)):
        be.lib.svt_aom_upsampled_pred_hip(None, None, 0, 0, None, p(comp), args[0], args[1], args[2], args[3], pre.ctypes.data + 4 * 19 + 4, 19, args[4])
    assert np.all(comp == 0xA5)
    assert be.lib.svt_hip_debug_commit_violations() == 0


# ---- footprint (emulator only) -------------------------------------------------------------------------------------------------------------------------------
class Recorded:
    """a plane that remembers the rectangle read from it"""

    def __init__(self, a):
        self.a, self.y, self.x = a, [1 << 30, -1], [1 << 30, -1]

    def __getitem__(self, key):
        ys, xs = key
        self.y = [min(self.y[0], ys.start), max(self.y[1], ys.stop - 1)]
        self.x = [min(self.x[0], xs.start), max(self.x[1], xs.stop - 1)]
        return self.a[key]


def _guarded(n_bytes):
    page = mmap.PAGESIZE
    body = (n_bytes + page - 1) // page * page
    m = mmap.mmap(-1, body + 2 * page)
    base = C.addressof(C.c_char.from_buffer(m))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes, libc.mprotect.restype = [C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0
    return m, page, body


def _flush(rect, at_end):
    """the rows of `rect` (2-D, row pitch = its width) flush against the inaccessible page after (at_end) or before them: (mapping, array, address)"""
    n = rect.size
    m, page, body = _guarded(n)
    start = page + (body - n if at_end else 0)
    arr = np.frombuffer(m, np.uint8, n, start)
    arr[:] = rect.reshape(-1)
    return m, arr, C.addressof(C.c_char.from_buffer(m)) + start


def test_read_footprint_on_the_emulator():
    """CPU only.  The reference plane holds exactly the rectangle the C reads for the item -- the restatement records it -- with its first byte right after an
    inaccessible page, or its last byte right before one: a read outside it leaves the mapping.  Every kind; both searches, whose rectangle is the union over the
    candidates they visit; the single-call forms read the caller's memory on the host and are run on the same mappings."""
    be = _backends.setdefault("emu", EmuBackend())
    cases, want, _ = prim()
    pick, seen = [], set()
    for k, c in enumerate(cases):
        key = (c["kind"], bool(c["xo"]), bool(c["yo"]))
        if key not in seen and c["bsize"] in (0, 3, 6, 17, 20):
            seen.add(key)
            pick.append(k)
    assert len(pick) >= 14
    rects = {(mc.VAR, False, False): (0, 0, 0, 0), (mc.SUBPIX, True, True): (0, 1, 0, 1), (mc.UPSAMPLED, True, False): (0, 0, -3, 4), (mc.UPSAMPLED, False, True): (-3, 4, 0, 0),
             (mc.UPSAMPLED, True, True): (-3, 4, -3, 4), (mc.OBMC_SUBPIX, True, False): (0, 0, 0, 1)}
    for at_end in (True, False):
        for k in pick:
            c = cases[k]
            pre, py, px, src, wsrc, mask = mc.primitive_inputs(c)
            rec = Recorded(pre)
            assert mc.block_var(c["kind"], c["bsize"], rec, py, px, c["xo"], c["yo"], c["taps"], src, wsrc, mask) == tuple(want[k])
            H, W = src.shape
            key = (c["kind"], bool(c["xo"]), bool(c["yo"]))
            if key in rects:  # the footprint table of the interface, spelled out
                assert (rec.y[0] - py, rec.y[1] - py - H + 1, rec.x[0] - px, rec.x[1] - px - W + 1) == rects[key], key
            rect = np.ascontiguousarray(pre[rec.y[0]:rec.y[1] + 1, rec.x[0]:rec.x[1] + 1])
            mp, arr, addr = _flush(rect, at_end)
            d = np.zeros(1, be.pkg.BlockVarDesc)
            d["pre_off"], d["pre_stride"], d["pre_plane"], d["src_stride"] = (py - rec.y[0]) * rect.shape[1] + (px - rec.x[0]), rect.shape[1], 4, W
            d["bsize"], d["kind"], d["xoffset"], d["yoffset"], d["taps"] = c["bsize"], c["kind"], c["xo"], c["yo"], c["taps"]
            planes = be.pkg.InterPredPlanes()
            planes.base[4] = addr
            out = np.zeros(1, be.pkg.BlockVarResult)
            srcb = np.ascontiguousarray(src)
            assert be.lib.svt_hip_block_var_batch(planes, p(srcb), None if wsrc is None else p(wsrc), None if mask is None else p(mask), p(d), 1, p(out), None, None) == 0
            assert [int(out[0][f]) for f in ("var", "sse", "sum", "sad")] == want[k].tolist(), (at_end, c)
            at = addr + int(d["pre_off"][0])
            name, sse = "%dx%d_hip" % (W, H), np.zeros(1, np.uint32)
            if c["kind"] == mc.SUBPIX:
                assert getattr(be.lib, "svt_aom_sub_pixel_variance" + name)(at, rect.shape[1], c["xo"], c["yo"], p(srcb), W, p(sse)) == want[k][0]
            elif c["kind"] == mc.OBMC_SUBPIX:
                assert getattr(be.lib, "svt_aom_obmc_sub_pixel_variance" + name)(at, rect.shape[1], c["xo"], c["yo"], p(wsrc), p(mask), p(sse)) == want[k][0]
            elif c["kind"] == mc.UPSAMPLED:
                comp = np.zeros((H, W), np.uint8)
                be.lib.svt_aom_upsampled_pred_hip(None, None, 0, 0, None, p(comp), W, H, c["xo"], c["yo"], at, rect.shape[1], c["taps"])
                assert np.array_equal(comp, mc.upsampled_pred(pre, py, px, W, H, c["xo"], c["yo"], c["taps"]))
            del arr, mp
        sc, sw = searches()
        picked = [[i for i, c in enumerate(sc) if c["method"] == m and c["bsize"] in (0, 2, 6) and sw[i]["evals"] >= 8][::5][:8] for m in (0, 1)]
        assert len(picked[0]) == 8 and len(picked[1]) == 8
        picked = picked[0] + picked[1]
        for i in picked:
            c = dict(mc.DEFAULTS)
            c.update(sc[i])
            src, ref, ry, rx = mc.search_inputs(sc[i])
            rec = Recorded(ref)
            params = {k: v for k, v in sc[i].items() if k in mc.DEFAULTS}
            ct = c["cost_table"]
            assert mc.md_subpel_search(src, rec, ry, rx, params, mc.cost_tables()[ct] if ct >= 0 else None) == sw[i]
            rect = np.ascontiguousarray(ref[rec.y[0]:rec.y[1] + 1, rec.x[0]:rec.x[1] + 1])
            mp, arr, addr = _flush(rect, at_end)
            one = [dict(sc[i])]
            buf, srcb, d = pack_searches(be.pkg, one, [0])
            # (the block's own position can lie before the rectangle its candidates read: the 64-bit offset then wraps, the sum is the same address)
            d["ref_off"], d["ref_stride"], d["ref_plane"] = ((ry - rec.y[0]) * rect.shape[1] + (rx - rec.x[0])) & mc.M64, rect.shape[1], 4
            planes = be.pkg.InterPredPlanes()
            planes.base[4] = addr
            out = np.zeros(1, be.pkg.MdSubpelResult)
            tabs = np.zeros(2, be.pkg.MvCostTable)
            for k, (joint, comp) in enumerate(mc.cost_tables()):
                tabs[k]["joint"], tabs[k]["comp"] = joint, comp
            assert be.lib.svt_hip_md_subpel_search_batch(planes, p(srcb), p(tabs), 2, p(d), 1, p(out), None, None) == 0
            assert {f: int(out[0][f]) for f in FIELDS} == sw[i], (at_end, sc[i])
            del arr, mp
