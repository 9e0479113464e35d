"""The OBMC motion refinement of csrc/mdsubpel.hip on the emulator (always) and on the MI355X (-m gpu): svt_hip_obmc_wsrc_batch, svt_hip_obmc_search_batch, the limits
helper and the host form against tests/obmc_common.py (numpy; pinned on the reference's C by tests/test_obmc_ref.py) and against tests/golden/obmc.npz (what the
reference's C computed for the same case lists).  Planes, source blocks and neighbour predictions sit at odd lead-ins with odd strides; outputs lie between sentinel
bytes and are compared whole.  The restatement's side of a launch is computed once and shared by the backends."""
import os

import numpy as np
import pytest

import mdsubpel_common as mc
import obmc_common as oc
from conftest import GOLDEN, p

PLANES = (1, 5, 31)  # reference, above prediction, left prediction
_cache = {}


def wsrcs():
    if "wsrc" not in _cache:
        cases = oc.wsrc_cases()
        _cache["wsrc"] = (cases, [oc.run_wsrc(c) for c in cases])
    return _cache["wsrc"]


def searches():
    if "search" not in _cache:
        cases, cnt = oc.search_cases(), {}
        _cache["search"] = (cases, [oc.run_search(c, cnt) for c in cases], cnt)
    return _cache["search"]


def set_spans(e, c):
    e["up_available"], e["left_available"], e["n_above"], e["n_left"] = c["up"], c["lf"], len(c["above"]), len(c["left"])
    for k, (rel, ln) in enumerate(c["above"][:4]):
        e["above_rel"][k], e["above_len"][k] = rel, ln
    for k, (rel, ln) in enumerate(c["left"][:4]):
        e["left_rel"][k], e["left_len"][k] = rel, ln


class Packer:
    """byte planes and source blocks of one launch, each at an odd lead-in with an odd stride"""

    def __init__(self):
        self.planes, self.srcs, self.ppos, self.spos = [np.zeros(3, np.uint8)], [np.zeros(5, np.uint8)], 3, 5

    def _put(self, lst, pos, a, extra):
        stride = a.shape[1] + extra
        buf = np.zeros((a.shape[0], stride), np.uint8)
        buf[:, :a.shape[1]] = a
        lst.append(buf.reshape(-1))
        return pos, stride, pos + buf.size

    def plane(self, a, i):
        off, stride, self.ppos = self._put(self.planes, self.ppos, a, 1 + 2 * (i % 3))
        return off, stride

    def src(self, a, i):
        off, stride, self.spos = self._put(self.srcs, self.spos, a, 1 + 2 * (i % 4))
        return off, stride


def pack_wsrc(pkg, cases, order):
    d, pk, pos = np.zeros(len(order), pkg.ObmcWsrcDesc), Packer(), 7
    for i, k in enumerate(order):
        c, e = cases[k], d[i]
        src, above, left = oc.wsrc_inputs(c)
        e["src_off"], e["src_stride"] = pk.src(src, i)
        e["above_off"], e["above_stride"] = pk.plane(above, i)
        e["left_off"], e["left_stride"] = pk.plane(left, i + 1)
        e["above_plane"], e["left_plane"], e["bsize"], e["out_off"] = PLANES[1], PLANES[2], c["bsize"], pos
        set_spans(e, c)
        pos += src.size + 1 + i % 3
    return np.concatenate(pk.planes), np.concatenate(pk.srcs), d, pos + 3


def launch_wsrc(be, packed, with_status=True):
    buf, src, d, total = packed
    n = len(d)
    keep = [be.dev(a) for a in (buf, src, d)]
    ow, om = be.dev(np.full(total * 4, 0xA5, np.uint8)), be.dev(np.full(total * 4, 0xA5, np.uint8))
    status = be.dev(np.full(n + 2, 7, np.uint8)) if with_status else None
    planes = be.pkg.InterPredPlanes()
    for k in PLANES[1:]:
        planes.base[k] = be.ptr(keep[0])
    r = be.lib.svt_hip_obmc_wsrc_batch(planes, be.ptr(keep[1]), be.ptr(keep[2]), n, be.ptr(ow), be.ptr(om), None if status is None else be.ptr(status) + 1, be.stream)
    be.sync()
    return r, be.host(ow).view(np.int32), be.host(om).view(np.int32), None if status is None else be.host(status)


def expected_wsrc(d, want, order, total, skip=()):
    ew, em = np.full(total * 4, 0xA5, np.uint8).view(np.int32), np.full(total * 4, 0xA5, np.uint8).view(np.int32)
    for i, k in enumerate(order):
        if i not in skip:
            o = int(d[i]["out_off"])
            ew[o:o + want[k][0].size], em[o:o + want[k][1].size] = want[k]
    return ew, em


def test_case_lists_reach_what_they_are_for():
    """CPU only.  The counters of the restatement over the search list: every branch the kernel restates is taken by some item"""
    cases, want, cnt = searches()
    assert cnt["fp_rounds_max"] >= 3 and cnt["fp_range_end"] >= 1 and cnt["fp_rejected"] >= 1 and cnt["fp_diag_winner"] >= 1 and cnt["fp_tie"] >= 1, cnt
    assert cnt["sp_axis_winner"] >= 1 and cnt["sp_diag_winner"] >= 1 and cnt["sp_second_moved"] >= 1 and cnt["sp_out_of_range"] >= 1, cnt
    have = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in cases)
    assert have(allow_hp=0) and all(have(forced_stop=f) for f in range(4)) and have(iters_per_step=1) and have(iters_per_step=2)
    assert have(approx=1) and have(approx=0, cost_table=0) and have(approx=0, cost_table=1) and have(approx=0, cost_table=-1)
    assert have(do_full=0, do_frac=1) and have(do_full=1, do_frac=0) and have(do_full=0, do_frac=0) and have(fpel_diag=0)
    assert all(have(subpel_search_type=t, form=f) for t in range(4) for f in (0, 1))
    assert {c["bsize"] for c in cases} >= {3, 5, 6, 18, 9, 12, 21, 15}
    # a walk that ends at the range moved in every round; one item's start was clamped into the limits
    assert any(c["fpel_range"] == 2 and w["fp_rounds"] == 2 for c, w in zip(cases, want))
    assert any(c["do_full"] and (w["fp_row"], w["fp_col"]) == (1, 2) and c["best_pred_mv"] == (37, 37) for c, w in zip(cases, want))
    # the 1/8 sample shifts are found
    found = [c for c, w in zip(cases, want) if c["content"] == "shift" and (w["mv_row"], w["mv_col"]) == tuple(c["true_mv"])]
    assert len(found) >= 8 and any((c["true_mv"][0] | c["true_mv"][1]) & 1 for c in found)
    wc, ww = wsrcs()
    assert {c["bsize"] for c in wc} == set(oc.OBMC_BSIZES)
    assert any(not c["up"] and not c["lf"] for c in wc) and any(c["up"] and not c["lf"] for c in wc) and any(c["lf"] and not c["up"] for c in wc)
    assert {len(c["above"]) for c in wc} >= {0, 1, 2, 4} and {len(c["left"]) for c in wc} >= {0, 1, 2, 4}
    assert any(c["above"] and c["above"][0][0] > 0 for c in wc) and any(mc.BH[c["bsize"]] > 64 for c in wc)
    sat = [w for c, w in zip(wc, ww) if c["content"] == "sat" and c["bsize"] == 3][0]
    # source 0 under neighbours of 255 at 8x8 (masks 39 50 59 64): the corner pixel carries both stages' smallest masks
    assert sat[0].min() == sat[0][0] == -(255 * 25 * 39 + (255 << 6) * 25) and sat[1][0] == 39 * 39 and sat[1].max() == 4096


def test_closed_form_is_the_pass_structure():
    """CPU only: the per-pixel closed form of the interface text against the restated passes, on every wsrc case"""
    for c, (wsrc, mask) in zip(*wsrcs()):
        src, above, left = oc.wsrc_inputs(c)
        W, H = mc.BW[c["bsize"]], mc.BH[c["bsize"]]
        ova, ovl = min(H, 64) >> 1, min(W, 64) >> 1
        in_a, in_l = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for rel, ln in (c["above"] if c["up"] else []):
            in_a[:ova, rel * 4:(rel + ln) * 4] = True
        for rel, ln in (c["left"] if c["lf"] else []):
            in_l[rel * 4:(rel + ln) * 4, :ovl] = True
        mv = np.zeros((H, W), np.int64)
        mv[:ova] = np.array(oc.OBMC_MASK[ova])[:, None]
        mh = np.zeros((H, W), np.int64)
        mh[:, :ovl] = np.array(oc.OBMC_MASK[ovl])[None, :]
        a, lf = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
        a[:ova], lf[:, :ovl] = above, left
        w, k = np.where(in_a, (64 - mv) * a, 0) * 64, np.where(in_a, mv, 64) * 64
        w, k = np.where(in_l, (w >> 6) * mh + (lf << 6) * (64 - mh), w), np.where(in_l, (k >> 6) * mh, k)
        assert np.array_equal(src.astype(np.int64) * 4096 - w, wsrc.reshape(H, W)) and np.array_equal(k, mask.reshape(H, W)), c


def test_wsrc(be):
    cases, want = wsrcs()
    order = np.random.default_rng(11).permutation(len(cases))
    if "wsrc_packed" not in _cache:
        _cache["wsrc_packed"] = pack_wsrc(be.pkg, cases, order)
    packed = _cache["wsrc_packed"]
    r, gw, gm, st = launch_wsrc(be, packed)
    assert r == 0 and st[0] == 7 and st[-1] == 7 and not st[1:-1].any()
    ew, em = expected_wsrc(packed[2], want, order, packed[3])
    assert np.array_equal(gw, ew) and np.array_equal(gm, em)
    r, gw, gm, _ = launch_wsrc(be, packed, with_status=False)
    assert r == 0 and np.array_equal(gw, ew) and np.array_equal(gm, em)


def device_tables(be):
    t = np.zeros(2, be.pkg.MvCostTable)
    for k, (joint, comp) in enumerate(mc.cost_tables()):
        t[k]["joint"], t[k]["comp"] = joint, comp
    return be.dev(t)


def fill_search_desc(e, c):
    e["bsize"], e["target_form"] = c["bsize"], c["form"]
    e["lim_col_min"], e["lim_col_max"], e["lim_row_min"], e["lim_row_max"] = c["lims"]
    (e["best_pred_mv_row"], e["best_pred_mv_col"]), (e["ref_mv_row"], e["ref_mv_col"]) = c["best_pred_mv"], c["ref_mv"]
    e["do_full_refine"], e["do_frac_refine"], e["approx_inter_rate"] = c["do_full"], c["do_frac"], c["approx"]
    e["fpel_search_range"], e["fpel_search_diag"] = c["fpel_range"], c["fpel_diag"]
    for f in ("sad_per_bit", "error_per_bit", "cost_table", "allow_hp", "forced_stop", "iters_per_step", "subpel_search_type"):
        e[f] = c[f]
    set_spans(e, c)


def pack_searches(pkg, cases, order, forms=None, offsets=None):
    """forms: the target form per packed item (default: the case's); offsets: where a previous svt_hip_obmc_wsrc_batch left item i's arrays"""
    d, pk = np.zeros(len(order), pkg.ObmcSearchDesc), Packer()
    ws, ms, pos = [np.zeros(7, np.int32)], [np.zeros(3, np.int32)], [7, 3]
    for i, k in enumerate(order):
        c, e = dict(cases[k]), d[i]
        if forms is not None:
            c["form"] = forms[i]
        ref, ry, rx, src, above, left = oc.search_inputs(c)
        off, stride = pk.plane(ref, i)
        e["ref_off"], e["ref_stride"], e["ref_plane"] = off + ry * stride + rx, stride, PLANES[0]
        fill_search_desc(e, c)
        if c["form"] == oc.DERIVED:
            e["src_off"], e["src_stride"] = pk.src(src, i)
            e["above_off"], e["above_stride"] = pk.plane(above, i + 1)
            e["left_off"], e["left_stride"] = pk.plane(left, i + 2)
            e["above_plane"], e["left_plane"] = PLANES[1], PLANES[2]
        elif offsets is not None:
            e["wsrc_off"] = e["mask_off"] = offsets[i]
        else:
            wsrc, mask = oc.search_target(c)
            e["wsrc_off"], e["mask_off"] = pos
            ws += [wsrc, np.zeros(1 + i % 2, np.int32)]
            ms += [mask, np.zeros(2 - i % 2, np.int32)]
            pos = [pos[0] + wsrc.size + 1 + i % 2, pos[1] + mask.size + 2 - i % 2]
    return np.concatenate(pk.planes), np.concatenate(pk.srcs), np.concatenate(ws), np.concatenate(ms), d


def launch_searches(be, packed, with_status=True, tables=True, arrays=None):
    buf, src, ws, ms, d = packed
    n = len(d)
    keep = [be.dev(a) for a in (buf, src, ws, ms, d)] + [device_tables(be)]
    pw, pm = (be.ptr(keep[2]), be.ptr(keep[3])) if arrays is None else arrays
    rs = be.pkg.ObmcSearchResult.itemsize
    out = be.dev(np.full((n + 2) * rs, 0xA5, np.uint8))
    status = be.dev(np.full(n + 2, 7, np.uint8)) if with_status else None
    planes = be.pkg.InterPredPlanes()
    for k in PLANES:
        planes.base[k] = be.ptr(keep[0])
    r = be.lib.svt_hip_obmc_search_batch(planes, be.ptr(keep[1]), pw, pm, be.ptr(keep[5]) if tables else None, 2 if tables else 0, be.ptr(keep[4]), n, be.ptr(out) + rs,
                                         None if status is None else be.ptr(status) + 1, be.stream)
    be.sync()
    got = be.host(out).view(be.pkg.ObmcSearchResult)
    assert np.all(got[[0, -1]].view(np.uint8) == 0xA5)
    return r, got[1:-1], None if status is None else be.host(status)


def as_dict(rec):
    return {f: int(rec[f]) for f in oc.RESULT_FIELDS}


def test_searches(be):
    """every case in one launch, permuted: both target forms and both launch classes next to each other"""
    cases, want, _ = searches()
    order = np.random.default_rng(9).permutation(len(cases))
    if "search_packed" not in _cache:
        _cache["search_packed"] = pack_searches(be.pkg, cases, order)
    r, got, st = launch_searches(be, _cache["search_packed"])
    assert r == 0 and st[0] == 7 and st[-1] == 7 and not st[1:-1].any()
    for i, k in enumerate(order):
        assert as_dict(got[i]) == want[k], (cases[k], as_dict(got[i]), want[k])


def test_derived_equals_arrays(be):
    """the same items with the arrays svt_hip_obmc_wsrc_batch wrote on this backend, and derived: identical records (and the restatement's)"""
    cases, want, _ = searches()
    order = list(range(len(cases)))
    wcases = [dict(bsize=c["bsize"], up=c["up"], lf=c["lf"], above=c["above"], left=c["left"]) for c in cases]
    d, pk, pos = np.zeros(len(order), be.pkg.ObmcWsrcDesc), Packer(), 5
    for i, c in enumerate(cases):
        _, _, _, src, above, left = oc.search_inputs(c)
        e = d[i]
        e["src_off"], e["src_stride"] = pk.src(src, i)
        e["above_off"], e["above_stride"] = pk.plane(above, i)
        e["left_off"], e["left_stride"] = pk.plane(left, i)
        e["above_plane"], e["left_plane"], e["bsize"], e["out_off"] = PLANES[1], PLANES[2], c["bsize"], pos
        set_spans(e, wcases[i])
        pos += src.size
    keep = [be.dev(a) for a in (np.concatenate(pk.planes), np.concatenate(pk.srcs), d)]
    ow, om = be.dev(np.zeros(pos, np.int32)), be.dev(np.zeros(pos, np.int32))
    planes = be.pkg.InterPredPlanes()
    for k in PLANES[1:]:
        planes.base[k] = be.ptr(keep[0])
    assert be.lib.svt_hip_obmc_wsrc_batch(planes, be.ptr(keep[1]), be.ptr(keep[2]), len(d), be.ptr(ow), be.ptr(om), None, be.stream) == 0
    offsets = [int(x) for x in d["out_off"]]
    r0, got_a, _ = launch_searches(be, pack_searches(be.pkg, cases, order, [oc.ARRAYS] * len(order), offsets), arrays=(be.ptr(ow), be.ptr(om)))
    r1, got_d, _ = launch_searches(be, pack_searches(be.pkg, cases, order, [oc.DERIVED] * len(order)))
    assert r0 == 0 and r1 == 0
    assert got_a.tobytes() == got_d.tobytes()
    for i in order:
        assert as_dict(got_d[i]) == want[i], cases[i]


def test_a_candidates_error_is_the_primitives(be):
    """The definition: every candidate the restatement visits for a dozen items goes through svt_hip_block_var_batch (the upsampled ones through
    svt_aom_upsampled_pred_hip first) with the same (pre, wsrc, mask); the errors are the restatement's, and the winner's are what the search reports."""
    cases, want, _ = searches()
    small = [i for i, c in enumerate(cases) if c["bsize"] in (3, 5, 6, 18) and c["do_frac"] and c["do_full"] and want[i]["evals"] > 1]
    pick = sum(([i for i in small if cases[i]["subpel_search_type"] == t][:3] for t in range(4)), [])
    assert len(pick) == 12
    r, got, _ = launch_searches(be, pack_searches(be.pkg, cases, pick))
    assert r == 0
    for n, i in enumerate(pick):
        c, visit = cases[i], []
        assert oc.run_search(c, None, visit) == want[i]
        ref, ry, rx, _, _, _ = oc.search_inputs(c)
        wsrc, mask = oc.search_target(c)
        W, H = mc.BW[c["bsize"]], mc.BH[c["bsize"]]
        planes_buf, d, expect = [np.ascontiguousarray(ref).reshape(-1)], np.zeros(len(visit), be.pkg.BlockVarDesc), []
        pos = ref.size
        for j, (kind, y, x, xo, yo, taps, val) in enumerate(visit):
            e = d[j]
            e["bsize"], e["pre_plane"] = c["bsize"], 4
            if kind == "up":  # the prediction by the single-call form, then ovf on it as a packed plane
                comp = np.zeros((H, W), np.uint8)
                be.lib.svt_aom_upsampled_pred_hip(None, None, 0, 0, None, p(comp), W, H, xo, yo, ref.ctypes.data + y * ref.shape[1] + x, ref.shape[1], taps)
                planes_buf.append(comp.reshape(-1))
                e["pre_off"], e["pre_stride"], e["kind"] = pos, W, mc.OBMC_VAR
                pos += comp.size
                expect.append((val[0], val[1]))
            else:
                e["pre_off"], e["pre_stride"], e["kind"], e["xoffset"], e["yoffset"] = y * ref.shape[1] + x, ref.shape[1], kind, xo, yo
                expect.append((val[3], 0) if kind == mc.OBMC_SAD else (val[0], val[1]))
        keep = [be.dev(a) for a in (np.concatenate(planes_buf), wsrc, mask, d)]
        out = be.dev(np.zeros(len(visit), be.pkg.BlockVarResult))
        planes = be.pkg.InterPredPlanes()
        planes.base[4] = be.ptr(keep[0])
        assert be.lib.svt_hip_block_var_batch(planes, None, be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), len(visit), be.ptr(out), None, be.stream) == 0
        be.sync()
        res = be.host(out)
        have = [(int(v["sad"]), 0) if d[j]["kind"] == mc.OBMC_SAD else (int(v["var"]), int(v["sse"])) for j, v in enumerate(res)]
        assert have == expect, c
        # the record's distortion / sse1 are the primitive's at the winning vector
        g = as_dict(got[n])
        assert g == want[i]
        assert (g["distortion"] & mc.M32, g["sse1"]) in [h for h, e in zip(have, d) if e["kind"] != mc.OBMC_SAD], c


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_search_launch_sizes_around_a_workgroup(be, n):
    """n items, no status array (the check kernel runs), a 128x128 item among small ones so that both launch classes meet at every workgroup boundary"""
    cases, want, _ = searches()
    big = [i for i, c in enumerate(cases) if c["bsize"] == 15]
    small = [i for i, c in enumerate(cases) if c["bsize"] in (3, 6)]
    order = (small[:n - 1] + big[:1]) if n > 1 else big[1:2]
    order = order[::-1] if n & 1 else order
    r, got, _ = launch_searches(be, pack_searches(be.pkg, cases, order), with_status=False)
    assert r == 0
    for i, k in enumerate(order):
        assert as_dict(got[i]) == want[k], (n, cases[k])


def test_golden_file(be):
    """what the reference's C computed for the case lists (tests/test_obmc_ref.py writes the file): the restatement, and one launch of each entry"""
    gold = np.load(os.path.join(GOLDEN, "obmc.npz"))
    wc, ww = wsrcs()
    sc, sw, _ = searches()
    assert np.array_equal(gold["wsrc_seeds"], [c["seed"] for c in wc]) and np.array_equal(gold["search_seeds"], [c["seed"] for c in sc])
    assert np.array_equal(gold["search_out"], np.array([[w[f] for f in oc.RESULT_FIELDS[:9]] for w in sw], np.int64))
    import zlib
    for k, (w, m) in enumerate(ww):
        assert [zlib.crc32(w.tobytes()), zlib.crc32(m.tobytes())] == gold["wsrc_crc"][k].tolist(), k
        if w.size <= 1024:
            assert np.array_equal(gold["wsrc_%d" % k], w) and np.array_equal(gold["mask_%d" % k], m), k
    order = list(range(len(sc)))
    r, got, _ = launch_searches(be, pack_searches(be.pkg, sc, order))
    assert r == 0 and np.array_equal(np.stack([got[f] for f in oc.RESULT_FIELDS[:9]], 1).astype(np.int64) & mc.M32, gold["search_out"] & mc.M32)
    worder = list(range(len(wc)))
    packed = pack_wsrc(be.pkg, wc, worder)
    r, gw, gm, _ = launch_wsrc(be, packed)
    assert r == 0
    for k in worder:
        o, nn = int(packed[2][k]["out_off"]), ww[k][0].size
        assert [zlib.crc32(gw[o:o + nn].tobytes()), zlib.crc32(gm[o:o + nn].tobytes())] == gold["wsrc_crc"][k].tolist(), k


@pytest.mark.parametrize("bsize", [6, 12])
def test_chain_neighbour_predictions_search_prediction_blend(be, bsize):
    """The OBMC_CAUSAL candidate end to end on the device, 16x16 and 64x64: the neighbours' predictions by svt_hip_inter_pred_batch, the refinement consuming them in
    place (DERIVED), the prediction at the winning vector, the OBMC blends of svt_hip_blend_batch -- against the numpy composition of the four restatements"""
    import interpred_common as ip
    g = np.random.default_rng(400 + bsize)
    W, H = mc.BW[bsize], mc.BH[bsize]
    ova, ovl, pad = min(H, 64) >> 1, min(W, 64) >> 1, oc.PAD
    ref = mc.smooth_plane(g, H + 2 * pad, W + 2 * pad)
    stride = ref.shape[1]
    src = np.clip(mc.upsampled_pred(ref, pad + 1, pad - 2, W, H, 5, 3, 3) + g.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)  # the reference moved by (11, -11)
    mv_above, mv_left = (13, -6), (-9, 20)  # 1/8 sample: the neighbours' own vectors, applied to this block's overlap regions

    def ext_at(mv, w, h):
        y, x = pad + (mv[0] >> 3), pad + (mv[1] >> 3)
        return ref[y - 3:y + h + 4, x - 3:x + w + 4], (mv[1] & 7) * 2, (mv[0] & 7) * 2

    def pred_desc(e, mv, w, h, dst_off, dst_stride):
        e["src_off"][0], e["src_stride"][0], e["plane"][0] = (pad + (mv[0] >> 3)) * stride + pad + (mv[1] >> 3), stride, 1
        e["w"], e["h"], e["subpel_x"][0], e["subpel_y"][0], e["dst_off"], e["dst_stride"] = w, h, (mv[1] & 7) * 2, (mv[0] & 7) * 2, dst_off, dst_stride

    # the numpy side
    above = ip.predict([ext_at(mv_above, W, ova)], W, ova, 0, 0, 0, 8).astype(np.uint8)
    left = ip.predict([ext_at(mv_left, ovl, H)], ovl, H, 0, 0, 0, 8).astype(np.uint8)
    spans = dict(up=1, lf=1, above=[(0, W >> 2)], left=[(0, H >> 2)])
    wsrc, mask = oc.target_weighted_pred(bsize, src, above, left, 1, 1, spans["above"], spans["left"])
    params = dict(bsize=bsize, best_pred_mv=(0, 0), ref_mv=(4, -4), cost_table=1)
    want = oc.obmc_search(ref, pad, pad, wsrc, mask, params, mc.cost_tables()[1])
    win = (want["mv_row"], want["mv_col"])
    own = ip.predict([ext_at(win, W, H)], W, H, 0, 0, 0, 8).astype(np.int64)
    blended = own.copy()
    mv_ = np.array(oc.OBMC_MASK[ova], np.int64)[:, None]
    blended[:ova] = (mv_ * blended[:ova] + (64 - mv_) * above + 32) >> 6  # build_obmc_inter_pred_above, then _left on its result
    mh_ = np.array(oc.OBMC_MASK[ovl], np.int64)[None, :]
    blended[:, :ovl] = (mh_ * blended[:, :ovl] + (64 - mh_) * left + 32) >> 6
    # the device side
    dref, dsrc, tabs = be.dev(ref), be.dev(src), device_tables(be)
    a_stride, l_stride, a_off = W + 3, ovl + 1, 5
    l_off = a_off + ova * a_stride + 2
    nb = be.dev(np.full(l_off + H * l_stride + 7, 0xA5, np.uint8))
    planes = be.pkg.InterPredPlanes()
    planes.base[1], planes.base[5] = be.ptr(dref), be.ptr(nb)
    d1 = np.zeros(2, be.pkg.InterPredDesc)
    pred_desc(d1[0], mv_above, W, ova, a_off, a_stride)
    pred_desc(d1[1], mv_left, ovl, H, l_off, l_stride)
    k1 = be.dev(d1)
    assert be.lib.svt_hip_inter_pred_batch(planes, be.ptr(nb), be.ptr(k1), 2, 8, None, be.stream) == 0
    ds = np.zeros(1, be.pkg.ObmcSearchDesc)
    c = dict(oc.DEFAULTS, form=oc.DERIVED, **spans)
    c.update(params)
    fill_search_desc(ds[0], c)
    e = ds[0]
    e["ref_off"], e["ref_stride"], e["ref_plane"], e["src_off"], e["src_stride"] = pad * stride + pad, stride, 1, 0, W
    e["above_off"], e["above_stride"], e["above_plane"], e["left_off"], e["left_stride"], e["left_plane"] = a_off, a_stride, 5, l_off, l_stride, 5
    k2, res = be.dev(ds), be.dev(np.zeros(1, be.pkg.ObmcSearchResult))
    assert be.lib.svt_hip_obmc_search_batch(planes, be.ptr(dsrc), None, None, be.ptr(tabs), 2, be.ptr(k2), 1, be.ptr(res), None, be.stream) == 0
    got = be.host(res)[0]
    assert as_dict(got) == want
    # the winner comes back to the host: a caller builds the next descriptor from it
    o_stride = W + 1
    ownb = be.dev(np.full(H * o_stride + 9, 0xA5, np.uint8))
    d3 = np.zeros(1, be.pkg.InterPredDesc)
    pred_desc(d3[0], (int(got["mv_row"]), int(got["mv_col"])), W, H, 4, o_stride)
    k3 = be.dev(d3)
    assert be.lib.svt_hip_inter_pred_batch(planes, be.ptr(ownb), be.ptr(k3), 1, 8, None, be.stream) == 0
    bp = be.pkg.BlendPlanes()
    bp.base[0], bp.base[1] = be.ptr(ownb), be.ptr(nb)
    for kind, w, h, off, st in ((be.pkg.BLEND_VMASK, W, ova, a_off, a_stride), (be.pkg.BLEND_HMASK, ovl, H, l_off, l_stride)):
        d4 = np.zeros(1, be.pkg.BlendDesc)
        b = d4[0]
        b["src_off"][0], b["src_stride"][0], b["plane"][0], b["src_off"][1], b["src_stride"][1], b["plane"][1] = 4, o_stride, 0, off, st, 1
        b["dst_off"], b["dst_stride"], b["w"], b["h"], b["kind"], b["mask_src"] = 4, o_stride, w, h, kind, be.pkg.MASK_OBMC
        k4 = be.dev(d4)
        assert be.lib.svt_hip_blend_batch(bp, be.ptr(ownb), None, be.ptr(k4), 1, 8, None, be.stream) == 0
        be.sync()
    out = be.host(ownb)
    assert np.all(out[:4] == 0xA5) and np.all(out[4 + H * o_stride:] == 0xA5)
    assert np.array_equal(out[4:4 + H * o_stride].reshape(H, o_stride)[:, :W], blended)
    assert not np.array_equal(blended, own)  # the blend did something


def test_read_footprint_on_the_emulator():
    """CPU only.  The reference plane holds exactly the rectangle the C reads for the item -- the union over the candidates the restatement visits -- with its first
    byte right after an inaccessible page, or its last byte right before one; a derived target's neighbour predictions hold exactly their overlap regions in the same
    way, its source exactly the block.  A read outside any of them leaves the mapping."""
    from conftest import EmuBackend, _backends
    from test_mdsubpel import Recorded, _flush
    be = _backends.setdefault("emu", EmuBackend())
    cases, want, _ = searches()
    pick = [i for i, c in enumerate(cases) if c["bsize"] in (3, 5, 6, 18) and want[i]["evals"] >= 8][::4][:10]
    assert len(pick) == 10 and {cases[i]["subpel_search_type"] for i in pick} >= {0, 3}
    tabs = np.zeros(2, be.pkg.MvCostTable)
    for k, (joint, comp) in enumerate(mc.cost_tables()):
        tabs[k]["joint"], tabs[k]["comp"] = joint, comp
    for at_end in (True, False):
        for n, i in enumerate(pick):
            c = dict(cases[i], form=n & 1)
            ref, ry, rx, src, above, left = oc.search_inputs(c)
            wsrc, mask = oc.search_target(c)
            rec = Recorded(ref)
            params = {k: v for k, v in c.items() if k in oc.DEFAULTS}
            ct = c["cost_table"]
            assert oc.obmc_search(rec, ry, rx, wsrc, mask, params, mc.cost_tables()[ct] if ct >= 0 else None) == want[i]
            rect = np.ascontiguousarray(ref[rec.y[0]:rec.y[1] + 1, rec.x[0]:rec.x[1] + 1])
            keep = [_flush(rect, at_end)]
            d = np.zeros(1, be.pkg.ObmcSearchDesc)
            e = d[0]
            fill_search_desc(e, c)
            # (the block's own position can lie outside the rectangle its candidates read: the 64-bit offset then wraps, the sum is the same address)
            e["ref_off"], e["ref_stride"], e["ref_plane"] = ((ry - rec.y[0]) * rect.shape[1] + (rx - rec.x[0])) & mc.M64, rect.shape[1], 4
            planes = be.pkg.InterPredPlanes()
            planes.base[4] = keep[0][2]
            srcp = None
            if c["form"] == oc.DERIVED:
                keep += [_flush(np.ascontiguousarray(a), at_end) for a in (src, above, left)]
                srcp = keep[1][2]
                planes.base[6], planes.base[7] = keep[2][2], keep[3][2]
                e["src_stride"], e["above_stride"], e["left_stride"], e["above_plane"], e["left_plane"] = src.shape[1], above.shape[1], left.shape[1], 6, 7
            out = np.zeros(1, be.pkg.ObmcSearchResult)
            assert be.lib.svt_hip_obmc_search_batch(planes, srcp, p(wsrc), p(mask), p(tabs), 2, p(d), 1, p(out), None, None) == 0
            assert as_dict(out[0]) == want[i], (at_end, c)
            del keep


INVALID_SEARCH = [("bsize", 22), ("bsize", 2), ("bsize", 16), ("target_form", 2), ("subpel_search_type", 4), ("forced_stop", 4), ("fpel_search_range", 65), ("cost_table", 2),
                  ("ref_plane", 32), ("ref_plane", 2)]
INVALID_SPANS = [("bsize", 0), ("bsize", 1), ("bsize", 17), ("bsize", 22), ("n_above", 5), ("n_left", 5), ("above_len", 0), ("left_len", 0), ("above_rel", 200),
                 ("left_rel", 31), ("above_plane", 32), ("left_plane", 2)]


def spoil(e, field, value):
    if field.endswith("_len") or field.endswith("_rel"):
        e[field][0] = value
    else:
        e[field] = value


def test_invalid_wsrc_descriptors(be):
    cases, want = wsrcs()
    order = [1, 2, 3] * 5  # 8x16, 16x8, 16x16 with one span a side
    packed = pack_wsrc(be.pkg, cases, order)
    bad = []
    for i, (field, value) in enumerate(INVALID_SPANS):
        spoil(packed[2][i + 1], field, value)
        bad.append(i + 1)
    r, gw, gm, st = launch_wsrc(be, packed)
    assert r == 0 and st[1:-1].tolist() == [1 if i in bad else 0 for i in range(len(order))]
    ew, em = expected_wsrc(packed[2], want, order, packed[3], skip=bad)
    assert np.array_equal(gw, ew) and np.array_equal(gm, em)
    r, gw, gm, _ = launch_wsrc(be, packed, with_status=False)
    assert r == -1 and np.all(gw.view(np.uint8) == 0xA5) and np.all(gm.view(np.uint8) == 0xA5)


def test_invalid_search_descriptors(be):
    cases, want, _ = searches()
    n_bad = len(INVALID_SEARCH) + len(INVALID_SPANS) - 4
    order = list(range(n_bad + 3))
    forms = [oc.DERIVED if i > len(INVALID_SEARCH) else cases[i]["form"] for i in order]
    packed = pack_searches(be.pkg, cases, order, forms)
    bad = []
    for i, (field, value) in enumerate(INVALID_SEARCH + INVALID_SPANS[4:]):  # the span rules hold for the derived form
        spoil(packed[4][i + 1], field, value)
        bad.append(i + 1)
    r, got, st = launch_searches(be, packed)
    assert r == 0 and st[1:-1].tolist() == [1 if i in bad else 0 for i in order]
    for i in order:
        if i in bad:
            assert np.all(got[i:i + 1].view(np.uint8) == 0xA5), i
        else:
            assert as_dict(got[i]) == want[i], i
    r, got, _ = launch_searches(be, packed, with_status=False)
    assert r == -1 and np.all(got.view(np.uint8) == 0xA5)
    # a form whose base pointers are missing is invalid
    one = pack_searches(be.pkg, cases, [0], [oc.ARRAYS])
    r, got, st = launch_searches(be, one, arrays=(None, None))
    assert r == 0 and st[1] == 1 and np.all(got.view(np.uint8) == 0xA5)
    # bad spans do not matter to an item that brings its arrays
    one[4][0]["n_above"] = 9
    r, got, st = launch_searches(be, one)
    assert r == 0 and st[1] == 0 and as_dict(got[0]) == want[0]


def test_nothing_to_do_and_bad_arguments(be):
    planes = be.pkg.InterPredPlanes()
    out = be.dev(np.full(64, 0xA5, np.uint8))
    assert be.lib.svt_hip_obmc_wsrc_batch(planes, None, None, 0, None, None, None, be.stream) == 0
    assert be.lib.svt_hip_obmc_search_batch(planes, None, None, None, None, 0, None, 0, None, None, be.stream) == 0
    assert be.lib.svt_hip_obmc_wsrc_batch(planes, None, be.ptr(out), 1, be.ptr(out), be.ptr(out), None, be.stream) == -1
    assert be.lib.svt_hip_obmc_search_batch(planes, None, None, None, None, 0, None, 1, be.ptr(out), None, be.stream) == -1
    be.sync()
    assert np.all(be.host(out) == 0xA5)


def test_mv_limits_helper(be):
    lim = np.zeros(4, np.int32)
    for b in range(22):
        for mi_rows, mi_cols in ((270, 480), (17, 33)):
            for mi_row, mi_col in ((0, 0), (0, mi_cols - 1), (mi_rows - 1, 0), (mi_rows - 1, mi_cols - 1), (mi_rows // 2, mi_cols // 3)):  # the picture's corners
                assert be.lib.svt_hip_obmc_mv_limits(mi_row, mi_col, b, mi_rows, mi_cols, p(lim)) == 0
                assert tuple(lim.tolist()) == oc.obmc_mv_limits(mi_row, mi_col, b, mi_rows, mi_cols)
    assert oc.obmc_mv_limits(0, 0, 6, 270, 480) == (-20, 1924, -20, 1084)
    lim[:] = 77
    assert be.lib.svt_hip_obmc_mv_limits(0, 0, 22, 10, 10, p(lim)) == -1 and be.lib.svt_hip_obmc_mv_limits(0, 0, 3, 10, 10, None) == -1
    assert lim.tolist() == [77] * 4


def test_host_form(be):
    """one item from host memory, both target forms, both launch classes, with and without a table"""
    cases, want, _ = searches()
    pick = [i for i, c in enumerate(cases) if c["bsize"] in (3, 6, 12, 15)][:10] + [i for i, c in enumerate(cases) if c["cost_table"] == 1 or c["approx"]][:3]
    assert {cases[i]["bsize"] for i in pick} >= {3, 6, 12, 15}
    tabs = np.zeros(2, be.pkg.MvCostTable)
    for k, (joint, comp) in enumerate(mc.cost_tables()):
        tabs[k]["joint"], tabs[k]["comp"] = joint, comp
    for n, i in enumerate(pick):
        c = dict(cases[i], form=n & 1)
        ref, ry, rx, src, above, left = oc.search_inputs(c)
        wsrc, mask = oc.search_target(c)
        d = np.zeros(1, be.pkg.ObmcSearchDesc)
        fill_search_desc(d[0], c)
        res = np.full(1, 0, be.pkg.ObmcSearchResult)
        ct = c["cost_table"]
        at = ref.ctypes.data + ry * ref.shape[1] + rx
        args = (p(wsrc), p(mask), None, 0, None, 0, None, 0) if c["form"] == oc.ARRAYS else (None, None, p(src), src.shape[1], p(above), above.shape[1], p(left), left.shape[1])
        r = be.lib.svt_hip_obmc_refine_host(p(d), at, ref.shape[1], oc.PAD, *args, tabs[ct:ct + 1].ctypes.data if ct >= 0 else None, p(res))
        assert r == 0 and as_dict(res[0]) == want[i], (c, as_dict(res[0]), want[i])
    # too little border for the search, an invalid item, a missing pointer: -1 and nothing written
    res.view(np.uint8)[:] = 0xA5
    c = dict(cases[pick[0]], form=oc.ARRAYS)
    ref, ry, rx, src, above, left = oc.search_inputs(c)
    wsrc, mask = oc.search_target(c)
    d = np.zeros(1, be.pkg.ObmcSearchDesc)
    fill_search_desc(d[0], c)
    at = ref.ctypes.data + ry * ref.shape[1] + rx
    assert be.lib.svt_hip_obmc_refine_host(p(d), at, ref.shape[1], 8, p(wsrc), p(mask), None, 0, None, 0, None, 0, None, p(res)) == -1
    assert be.lib.svt_hip_obmc_refine_host(p(d), at, ref.shape[1], oc.PAD, None, p(mask), None, 0, None, 0, None, 0, None, p(res)) == -1
    d[0]["forced_stop"] = 4
    assert be.lib.svt_hip_obmc_refine_host(p(d), at, ref.shape[1], oc.PAD, p(wsrc), p(mask), None, 0, None, 0, None, 0, None, p(res)) == -1
    assert np.all(res.view(np.uint8) == 0xA5)
    assert be.lib.svt_hip_debug_commit_violations() == 0
