"""A numpy restatement of the OBMC motion refinement and the case lists the obmc test files share.

Restated from Source/Lib/Codec/enc_inter_prediction.c (:1581 / :1610 the two target-weighted callbacks, :1756 calc_target_weighted_pred), Codec/av1me.c (:205
svt_av1_set_mv_search_range, :229-261 the cost forms, :709 get_obmc_mvpred_var, :721 obmc_refining_search_sad, :760 svt_av1_obmc_full_pixel_search, :778
set_subpel_mv_search_range, :822-900 the CHECK_BETTER / SECOND_LEVEL_CHECKS_BEST macros, :963 svt_av1_find_best_obmc_sub_pixel_tree_up), Codec/rd_cost.c:67-87 (the
rate) and Codec/mode_decision.c:2290 (single_motion_search).  The candidate errors come from mdsubpel_common.block_var, which tests/test_mdsubpel_ref.py pins on the
reference.  tests/test_obmc_ref.py pins the functions here on the reference; tests/test_obmc.py compares the kernels of csrc/mdsubpel.hip with them.
"""
import numpy as np

import mdsubpel_common as mc
from mdsubpel_common import BH, BW, INT_MAX, M32, MV_MAX, MV_UPP, MV_VALS, i16, i32

ARRAYS, DERIVED = 0, 1
OBMC_BSIZES = [b for b in range(22) if BW[b] >= 8 and BH[b] >= 8]
# obmc_mask_1 .. obmc_mask_32 (inter_prediction.c:2407-2417)
OBMC_MASK = {1: [64], 2: [45, 64], 4: [39, 50, 59, 64], 8: [36, 42, 48, 53, 57, 61, 64, 64],
             16: [34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64],
             32: [33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64]}
NEIGHBORS = [(-1, 0), (0, -1), (0, 1), (1, 0), (-1, 1), (1, 1), (1, -1), (-1, -1)]


# ---- the target ------------------------------------------------------------------------------------------------------------------------------------------------
def target_weighted_pred(bsize, src, above, left, up_available, left_available, above_spans, left_spans):
    """calc_target_weighted_pred with the C's pass structure.  src W x H; above / left: 2-D arrays with (0, 0) at the block's top-left sample (at least ovA rows
    resp. ovL columns; None when unused); spans: lists of (rel_mi, len_mi).  Returns (wsrc, mask), flat int32 of W * H."""
    W, H = BW[bsize], BH[bsize]
    wsrc, mask = np.zeros((H, W), np.int64), np.full((H, W), 64, np.int64)
    if up_available:
        ov = min(H, 64) >> 1
        m0 = np.array(OBMC_MASK[ov], np.int64)[:, None]
        for rel, ln in above_spans:  # svt_av1_calc_target_weighted_pred_above_c
            c0, c1 = rel * 4, (rel + ln) * 4
            wsrc[:ov, c0:c1] = (64 - m0) * above[:ov, c0:c1].astype(np.int64)
            mask[:ov, c0:c1] = m0
    wsrc *= 64
    mask *= 64
    if left_available:
        ov = min(W, 64) >> 1
        m0 = np.array(OBMC_MASK[ov], np.int64)[None, :]
        for rel, ln in left_spans:  # svt_av1_calc_target_weighted_pred_left_c
            r0, r1 = rel * 4, (rel + ln) * 4
            wsrc[r0:r1, :ov] = (wsrc[r0:r1, :ov] >> 6) * m0 + (left[r0:r1, :ov].astype(np.int64) << 6) * (64 - m0)
            mask[r0:r1, :ov] = (mask[r0:r1, :ov] >> 6) * m0
    wsrc = src.astype(np.int64) * 4096 - wsrc
    return wsrc.reshape(-1).astype(np.int32), mask.reshape(-1).astype(np.int32)


def obmc_mv_limits(mi_row, mi_col, bsize, mi_rows, mi_cols):
    """single_motion_search :2322-2327, full-pel: (col_min, col_max, row_min, row_max)"""
    mi_w, mi_h = BW[bsize] >> 2, BH[bsize] >> 2
    return (-(((mi_col + mi_w) * 4) + 4), (mi_cols - mi_col) * 4 + 4, -(((mi_row + mi_h) * 4) + 4), (mi_rows - mi_row) * 4 + 4)


def refine_flags(refine_level):
    """the switch of single_motion_search: (do_full_refine, do_frac_refine)"""
    return {0: (1, 1), 1: (1, 1), 3: (1, 1), 2: (0, 1), 4: (0, 1)}.get(refine_level, (0, 0))


# ---- the search ------------------------------------------------------------------------------------------------------------------------------------------------
WIDE_LIMITS = (-400, 400, -400, 400)
DEFAULTS = dict(bsize=6, best_pred_mv=(0, 0), ref_mv=(0, 0), lims=WIDE_LIMITS, do_full=1, do_frac=1, sad_per_bit=30, error_per_bit=120, approx=0, cost_table=0,
                fpel_range=16, fpel_diag=1, allow_hp=1, forced_stop=0, iters_per_step=2, subpel_search_type=3)
COUNTERS = ("fp_rounds_max", "fp_range_end", "fp_rejected", "fp_diag_winner", "fp_tie", "sp_axis_winner", "sp_diag_winner", "sp_second_moved", "sp_out_of_range")


def _table_cost(table, dr, dc):
    """svt_mv_cost on an MV difference (int16): joint + comp[0][row] + comp[1][col], the clip of CLIP3(MV_LOW, MV_UPP) and the table-end rule"""
    j = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
    at = lambda v: min(max(MV_MAX + min(max(v, -MV_UPP), MV_UPP), 0), MV_VALS - 1)
    return i32(int(table[0][j]) + int(table[1][0][at(dr)]) + int(table[1][1][at(dc)]))


def set_mv_search_range(lims, ref_mv):
    """svt_av1_set_mv_search_range on (col_min, col_max, row_min, row_max)"""
    rr, rc = ref_mv
    return (max(lims[0], max((rc >> 3) - 1023 + (1 if rc & 7 else 0), (-MV_UPP >> 3) + 1)), min(lims[1], min((rc >> 3) + 1023, (MV_UPP >> 3) - 1)),
            max(lims[2], max((rr >> 3) - 1023 + (1 if rr & 7 else 0), (-MV_UPP >> 3) + 1)), min(lims[3], min((rr >> 3) + 1023, (MV_UPP >> 3) - 1)))


def obmc_search(ref, ry, rx, wsrc, mask, params, table=None, counters=None, visit=None):
    """One item of svt_hip_obmc_search_batch.  ref: the reference plane, (ry, rx) the block's position in it; wsrc / mask flat int32.  counters: a dict that collects
    COUNTERS; visit: a list that receives (kind, y, x, xoffset, yoffset, taps, value) of every candidate error in svt_hip_block_var_batch terms."""
    p = dict(DEFAULTS)
    p.update(params)
    b = p["bsize"]
    rr, rc = p["ref_mv"]
    lims = p["lims"]
    light = bool(p["approx"])
    cnt = counters if counters is not None else {}

    def bump(k, v=1):
        cnt[k] = cnt.get(k, 0) + v

    def err(kind, y, x, xo=0, yo=0, taps=0):
        r = mc.block_var(kind, b, ref, y, x, xo, yo, taps, wsrc=wsrc, mask=mask)
        if visit is not None:
            visit.append((kind, y, x, xo, yo, taps, r))
        return r

    def sad_cost(r, c):  # mvsad_err_cost
        fcr, fcc = rr >> 3, rc >> 3
        if light:
            return (1296 + 50 * (abs(c - fcc) * 8 + abs(r - fcr) * 8)) & M32
        if table is None:
            return 0
        prod = ((_table_cost(table, i16((r - fcr) * 8), i16((c - fcc) * 8)) & M32) * (p["sad_per_bit"] & M32)) & M32  # (unsigned)cost * sad_per_bit
        return ((prod + 256) & M32) >> 9

    def err_cost(r, c):  # svt_aom_mv_err_cost / _light, (r, c) an MV
        r, c = i16(r), i16(c)
        if light:
            return (1296 + 50 * (abs(c - rc) + abs(r - rr))) & M32
        if table is None:
            return 0
        return i32((_table_cost(table, i16(r - rr), i16(c - rc)) * p["error_per_bit"] + 8192) >> 14) & M32

    fr, fc = i16(p["best_pred_mv"][0] >> 3), i16(p["best_pred_mv"][1] >> 3)
    evals = fp_rounds = thissme = 0
    if p["do_full"]:
        cmin, cmax, rmin, rmax = set_mv_search_range(lims, (rr, rc))
        clamp = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)
        fc, fr = i16(clamp(fc, cmin, cmax)), i16(clamp(fr, rmin, rmax))
        best_sad = (err(mc.OBMC_SAD, ry + fr, rx + fc)[3] + sad_cost(fr, fc)) & M32
        evals += 1
        ended = True
        for _ in range(p["fpel_range"]):
            best_site = -1
            for j in range(8 if p["fpel_diag"] else 4):
                r, c = i16(fr + NEIGHBORS[j][0]), i16(fc + NEIGHBORS[j][1])
                if not (cmin <= c <= cmax and rmin <= r <= rmax):
                    bump("fp_rejected")
                    continue
                sad = err(mc.OBMC_SAD, ry + r, rx + c)[3]
                evals += 1
                if best_site != -1 and (sad + sad_cost(r, c)) & M32 == best_sad:
                    bump("fp_tie")  # equal to an earlier winner of this round: the strict < keeps the lower j
                if sad < best_sad:
                    sad = (sad + sad_cost(r, c)) & M32
                    if sad < best_sad:
                        best_sad, best_site = sad, j
            if best_site == -1:
                ended = False
                break
            if best_site >= 4:
                bump("fp_diag_winner")
            fr, fc = i16(fr + NEIGHBORS[best_site][0]), i16(fc + NEIGHBORS[best_site][1])
            fp_rounds += 1
        if ended and p["fpel_range"]:
            bump("fp_range_end")
        cnt["fp_rounds_max"] = max(cnt.get("fp_rounds_max", 0), fp_rounds)
        thissme = i32(best_sad)
        if thissme < INT_MAX:
            thissme = i32(err(mc.OBMC_VAR, ry + fr, rx + fc)[0] + err_cost(fr * 8, fc * 8))
            evals += 1
    br, bc = fr * 8, fc * 8
    besterr = distortion = sse1 = 0
    if p["do_frac"]:
        mx = 8 * 1023
        minc, maxc = max(-MV_UPP + 1, max(lims[0] * 8, rc - mx)), min(MV_UPP - 1, min(lims[1] * 8, rc + mx))
        minr, maxr = max(-MV_UPP + 1, max(lims[2] * 8, rr - mx)), min(MV_UPP - 1, min(lims[3] * 8, rr + mx))
        rnd = 3 - p["forced_stop"]
        if not p["allow_hp"] and rnd == 3:
            rnd = 2
        taps = p["subpel_search_type"]
        var, sse1, _, _ = err(mc.OBMC_VAR, ry + fr, rx + fc)
        evals += 1
        distortion = i32(var)
        besterr = (var + err_cost(fr * 8, fc * 8)) & M32
        st = dict(besterr=besterr, distortion=distortion, sse1=sse1, br=br, bc=bc, evals=evals)

        def candidate(r, c):
            """(in range, total, thismse, sse)"""
            if not (minc <= c <= maxc and minr <= r <= maxr):
                bump("sp_out_of_range")
                return False, INT_MAX, 0, 0
            y, x = ry + (r >> 3), rx + (c >> 3)
            if taps == 0:
                mse, sse, _, _ = err(mc.OBMC_SUBPIX, y, x, c & 7, r & 7)
            else:
                # svt_aom_upsampled_pred, then ovf on the packed prediction
                pred = mc.upsampled_pred(ref, y, x, BW[b], BH[b], c & 7, r & 7, taps)
                mse, sse, _, _ = mc.block_var(mc.OBMC_VAR, b, pred.astype(np.uint8), 0, 0, wsrc=wsrc, mask=mask)
                if visit is not None:
                    visit.append(("up", y, x, c & 7, r & 7, taps, (mse, sse)))
            st["evals"] += 1
            return True, (err_cost(r, c) + mse) & M32, mse, sse

        def check_better(r, c):  # CHECK_BETTER0 / 1
            ok, tot, mse, sse = candidate(r, c)
            if ok and tot < st["besterr"]:
                st.update(besterr=tot, br=r, bc=c, distortion=i32(mse), sse1=sse)

        h = 4
        for _ in range(rnd):
            r0, c0 = st["br"], st["bc"]
            steps = [(0, -h), (0, h), (-h, 0), (h, 0)]
            cost, best_idx = [0] * 5, -1
            for idx in range(4):
                ok, tot, mse, sse = candidate(r0 + steps[idx][0], c0 + steps[idx][1])
                cost[idx] = tot
                if ok and tot < st["besterr"]:
                    best_idx = idx
                    st.update(besterr=tot, distortion=i32(mse), sse1=sse)
            kc = -h if cost[0] <= cost[1] else h
            kr = -h if cost[2] <= cost[3] else h
            tc, tr = c0 + kc, r0 + kr
            ok, tot, mse, sse = candidate(tr, tc)
            if ok and tot < st["besterr"]:
                best_idx = 4
                st.update(besterr=tot, distortion=i32(mse), sse1=sse)
            if 0 <= best_idx < 4:
                st["br"], st["bc"] = r0 + steps[best_idx][0], c0 + steps[best_idx][1]
                bump("sp_axis_winner")
            elif best_idx == 4:
                st["br"], st["bc"] = tr, tc
                bump("sp_diag_winner")
            if p["iters_per_step"] > 1 and best_idx != -1:  # SECOND_LEVEL_CHECKS_BEST
                br0, bc0 = st["br"], st["bc"]
                assert tr == br0 or tc == bc0
                if tr == br0 and tc != bc0:
                    kc = bc0 - tc
                elif tr != br0 and tc == bc0:
                    kr = br0 - tr
                check_better(br0 + kr, bc0)
                check_better(br0, bc0 + kc)
                if (br0, bc0) != (st["br"], st["bc"]):
                    check_better(br0 + kr, bc0 + kc)
                if (br0, bc0) != (st["br"], st["bc"]):
                    bump("sp_second_moved")
            h >>= 1
        besterr, distortion, sse1, br, bc, evals = st["besterr"], st["distortion"], st["sse1"], st["br"], st["bc"], st["evals"]
    mr, mcol = i16(br), i16(bc)
    if light:  # svt_av1_mv_bit_cost_light
        rate = i32(1296 + 50 * (abs(mcol - rc) + abs(mr - rr)))
    elif table is None:
        rate = 0
    else:  # svt_av1_mv_bit_cost, MV_COST_WEIGHT 108
        rate = i32(_table_cost(table, i16(mr - rr), i16(mcol - rc)) * 108 + 64) >> 7
    return dict(mv_row=mr, mv_col=mcol, fp_row=fr, fp_col=fc, thissme=thissme, besterr=besterr, distortion=distortion, sse1=sse1, rate_mv=rate, fp_rounds=fp_rounds,
                evals=evals)


RESULT_FIELDS = ("mv_row", "mv_col", "fp_row", "fp_col", "thissme", "besterr", "distortion", "sse1", "rate_mv", "fp_rounds", "evals")

# ---- shared inputs -------------------------------------------------------------------------------------------------------------------------------------------
PAD = 40  # samples around the block in a search's reference plane: |start| + rounds <= 30, under two samples of sub-pel movement, four of the filter


def wsrc_cases():
    """item 1: every allowed size, the span layouts, availability"""
    cases, seed = [], 9000

    def add(bsize, up=1, lf=1, above=None, left=None, content="rand"):
        nonlocal seed
        seed += 1
        n4w, n4h = BW[bsize] >> 2, BH[bsize] >> 2
        cases.append(dict(bsize=bsize, up=up, lf=lf, above=[(0, n4w)] if above is None else above, left=[(0, n4h)] if left is None else left, content=content,
                          seed=seed))
    for b in OBMC_BSIZES:
        add(b)
    add(3, 0, 0)
    add(6, 1, 0)
    add(6, 0, 1)
    add(6, 1, 1, [], [])  # available, nothing overlappable
    add(9, above=[(0, 4), (4, 4)], left=[(0, 2), (2, 6)])
    add(12, above=[(0, 4), (4, 4), (8, 4), (12, 4)], left=[(0, 2), (2, 2), (4, 4), (8, 8)])
    add(12, above=[(0, 4), (12, 4)], left=[(4, 4)])  # gaps between spans, a gap at the start
    add(13, above=[(2, 2), (8, 8)], left=[(0, 16), (16, 8), (28, 4)])  # 64x128: H > 64, ov capped at 32
    add(14, above=[(0, 16), (24, 8)], left=[(1, 1), (3, 1), (5, 1), (7, 1)])  # 128x64
    add(15, above=[(0, 8), (8, 8), (16, 8), (24, 8)], left=[(0, 32)])
    add(18, above=[(0, 1), (1, 1)], left=[(0, 2), (4, 4)])  # 8x32
    add(19, above=[(0, 2), (4, 4)], left=[(0, 1), (1, 1)])  # 32x8
    add(20, above=[(1, 2)], left=[(0, 4), (12, 4)])  # 16x64
    add(21, above=[(0, 4), (12, 4)], left=[(1, 2)])  # 64x16
    add(3, content="sat")
    add(15, content="sat")
    add(3, above=[(1, 1)], left=[(1, 1)])
    add(6, 1, 1, content="zero")
    return cases


def wsrc_inputs(case):
    """(src, above, left): src W x H; above ovA x W; left H x ovL"""
    g = np.random.default_rng(case["seed"])
    W, H = BW[case["bsize"]], BH[case["bsize"]]
    ova, ovl = min(H, 64) >> 1, min(W, 64) >> 1
    if case["content"] == "sat":
        return np.zeros((H, W), np.uint8), np.full((ova, W), 255, np.uint8), np.full((H, ovl), 255, np.uint8)
    if case["content"] == "zero":
        return np.full((H, W), 255, np.uint8), np.zeros((ova, W), np.uint8), np.zeros((H, ovl), np.uint8)
    return g.integers(0, 256, (H, W), dtype=np.uint8), g.integers(0, 256, (ova, W), dtype=np.uint8), g.integers(0, 256, (H, ovl), dtype=np.uint8)


def run_wsrc(case):
    src, above, left = wsrc_inputs(case)
    return target_weighted_pred(case["bsize"], src, above, left, case["up"], case["lf"], case["above"], case["left"])


def search_inputs(case):
    """(ref plane, ry, rx, src, above, left, spans ...): the source is the reference moved by true_mv (1/8 sample) plus noise; the neighbours' predictions are the
    reference at two other vectors plus noise, as an OBMC block's neighbours give"""
    g = np.random.default_rng(case["seed"])
    b = case["bsize"]
    W, H = BW[b], BH[b]
    ova, ovl = min(H, 64) >> 1, min(W, 64) >> 1
    content = case["content"]
    if content == "lowamp":  # two grey levels: small integer SADs, so that candidates tie
        ref = (100 + g.integers(0, 2, (H + 2 * PAD, W + 2 * PAD))).astype(np.uint8)
        src = (100 + g.integers(0, 2, (H, W))).astype(np.uint8)
    elif content == "rand":
        ref, src = g.integers(0, 256, (H + 2 * PAD, W + 2 * PAD), dtype=np.uint8), g.integers(0, 256, (H, W), dtype=np.uint8)
    else:
        ref = mc.smooth_plane(g, H + 2 * PAD, W + 2 * PAD)
        r, c = case["true_mv"]
        src = mc.upsampled_pred(ref, PAD + (r >> 3), PAD + (c >> 3), W, H, c & 7, r & 7, 3)
        src = np.clip(src + g.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
    above = np.clip(ref[PAD + 1:PAD + 1 + ova, PAD - 2:PAD - 2 + W].astype(np.int64) + g.integers(-3, 4, (ova, W)), 0, 255).astype(np.uint8)
    left = np.clip(ref[PAD - 1:PAD - 1 + H, PAD + 2:PAD + 2 + ovl].astype(np.int64) + g.integers(-3, 4, (H, ovl)), 0, 255).astype(np.uint8)
    return ref, PAD, PAD, src, above, left


def search_target(case):
    """(wsrc, mask) of a search case, by the restatement of item 1"""
    _, _, _, src, above, left = search_inputs(case)
    return target_weighted_pred(case["bsize"], src, above, left, case["up"], case["lf"], case["above"], case["left"])


def search_cases():
    cases, seed = [], 7000

    def add(content="shift", true_mv=(13, -10), **kw):
        nonlocal seed
        seed += 1
        c = dict(DEFAULTS, content=content, true_mv=true_mv, seed=seed, up=1, lf=1, form=len(cases) & 1)
        c.update(kw)
        n4w, n4h = BW[c["bsize"]] >> 2, BH[c["bsize"]] >> 2
        c.setdefault("above", [(0, n4w)])
        c.setdefault("left", [(0, n4h)] if n4h < 4 else [(0, n4h // 2), (n4h // 2, n4h - n4h // 2)])
        if "best_pred_mv" not in kw:
            c["best_pred_mv"] = (((true_mv[0] + 4) >> 3) * 8, ((true_mv[1] + 4) >> 3) * 8)
        cases.append(c)
    # sizes: both launch classes, npix < 128, 4:1, the largest intermediate; each with every subpel_search_type once somewhere
    for k, b in enumerate((3, 5, 6, 18, 9, 12, 21, 15)):  # 8x8, 16x8, 16x16, 8x32, 32x32, 64x64, 64x16, 128x128
        add("shift", (-11, 5), bsize=b, subpel_search_type=(3, 0, 1, 2)[k % 4], form=k & 1)
        add("shift", (21, -19), bsize=b, best_pred_mv=(0, 0), subpel_search_type=3, approx=k & 1, form=1 - (k & 1))  # a walk of a few full-pel rounds
    for t in range(4):
        add("shift", (-5, 7), subpel_search_type=t)
        add("rand", subpel_search_type=t, best_pred_mv=(8, -16), fpel_range=3)
    # full-pel: a long walk, one cut by the range, limits that reject neighbours, 4 neighbours only
    add("shift", (44, -37), best_pred_mv=(0, 0), bsize=9)
    add("shift", (44, -37), best_pred_mv=(0, 0), bsize=9, fpel_range=2)
    add("shift", (44, -37), best_pred_mv=(0, 0), bsize=9, fpel_diag=0)
    add("shift", (30, 30), best_pred_mv=(0, 0), lims=(-2, 2, -1, 1))
    add("shift", (30, 30), best_pred_mv=(37, 37), lims=(-2, 2, -1, 1))  # the start is clamped
    add("shift", (-30, 22), best_pred_mv=(0, 0), lims=(0, 400, -400, 0), approx=1)
    add("shift", (16, 16), best_pred_mv=(0, 0), fpel_range=0)
    for s in (7012, 7022, 7053, 7068, 0, 0):  # two grey levels and no cost: the totals are small SADs, so neighbours tie (the four seeds: ones where a later
        add("lowamp", bsize=3, best_pred_mv=(0, 0), cost_table=-1, fpel_range=4, up=0, lf=0, **({"seed": s} if s else {}))  # neighbour equals the round's winner)
    # sub-pel: rounds, precision, iterations, limits
    for hp in (0, 1):
        for fs in range(4):
            add("shift", (5, -3), allow_hp=hp, forced_stop=fs, bsize=3)
    for it in (1, 2):
        add("shift", (6, 6), iters_per_step=it)
        add("shift", (-3, 9), iters_per_step=it, subpel_search_type=0)
        add("rand", iters_per_step=it, best_pred_mv=(0, 8), fpel_range=2)
    add("shift", (18, -9), best_pred_mv=(16, -8), lims=(-1, 400, -400, 2), do_full=0)  # the sub-pel start sits on two limits: candidates out of range
    add("shift", (18, -9), best_pred_mv=(16, -8), lims=(-400, -1, 2, 400), do_full=0)
    # costs: both forms, each table, none
    add("shift", (9, 4), ref_mv=(20, -30), cost_table=1, error_per_bit=700, sad_per_bit=90)
    add("shift", (9, 4), ref_mv=(20, -30), cost_table=-1)
    add("shift", (9, 4), ref_mv=(-35, 61), approx=1)
    add("shift", (9, 4), ref_mv=(16000, -16000), cost_table=0, best_pred_mv=(8, 8), do_full=0)  # every sub-pel candidate is out of the ref_mv +- 8184 window
    # the refine levels' flag pairs
    add("shift", (12, -20), best_pred_mv=(3, -5), do_full=0, do_frac=1)
    add("shift", (12, -20), best_pred_mv=(3, -5), do_full=1, do_frac=0)
    add("shift", (12, -20), best_pred_mv=(3, -5), do_full=0, do_frac=0)
    # the target's variety: no neighbours, one side, gaps
    add("shift", (7, 3), up=0, lf=0)
    add("shift", (7, 3), up=1, lf=0)
    add("shift", (7, 3), up=0, lf=1)
    add("shift", (7, 3), bsize=12, above=[(0, 4), (12, 4)], left=[(4, 4)])
    return cases


def run_search(case, counters=None, visit=None):
    ref, ry, rx, _, _, _ = search_inputs(case)
    wsrc, mask = search_target(case)
    params = {k: v for k, v in case.items() if k in DEFAULTS}
    ct = params["cost_table"]
    return obmc_search(ref, ry, rx, wsrc, mask, params, mc.cost_tables()[ct] if ct >= 0 else None, counters, visit)
