"""A numpy restatement of the block variance family of svt_aom_mefn_ptr and of mode decision's sub-pel search, and the case lists the three mdsubpel test files share.

Restated from Source/Lib/C_DEFAULT/variance.c (:28-68 the bilinear passes, :204-254 svt_aom_upsampled_pred_c, :257-318 the variances, :347-390 the OBMC forms),
C_DEFAULT/sad_av1.c:18 (obmc_sad), Codec/svt_psnr.c:63 (svt_aom_mse16x16_c), Codec/convolve.c:244-301 (svt_aom_convolve8_horiz_c / _vert_c) and Codec/mcomp.c
(:44 svt_mv_err_cost, :183-250 the two check functions, :260-352 / :375-604 the level checks, :606-772 the two searches).  tests/test_mdsubpel_ref.py pins every
function here, and the filter rows below entry by entry, on the reference; tests/test_mdsubpel.py compares the kernels of csrc/mdsubpel.hip with it.
"""
import numpy as np

BW = [4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64]  # block_size_wide / block_size_high by BlockSize
BH = [4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16]
VAR, SUBPIX, UPSAMPLED, MSE, OBMC_SAD, OBMC_VAR, OBMC_SUBPIX = range(7)
KIND_NAMES = ("var", "subpix", "upsampled", "mse", "obmc_sad", "obmc_var", "obmc_subpix")
MV_MAX, MV_UPP, MV_VALS = 16383, 16384, 32767
INT_MAX = 0x7FFFFFFF
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

BILINEAR_2T = [(128 - 16 * k, 16 * k) for k in range(8)]  # bilinear_filters_2t, filter.h:39
# the rows svt_aom_upsampled_pred_c can reach: phase q3 << 1 of av1_bilinear_filters (USE_2_TAPS), av1_sub_pel_filters_4 (USE_4_TAPS), av1_sub_pel_filters_8
# (USE_8_TAPS); UP_ROWS[subpel_search][q3]
UP_ROWS = {
    1: [[0, 0, 0, 128 - 16 * q, 16 * q, 0, 0, 0] for q in range(8)],
    2: [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0], [0, 0, -12, 110, 38, -8, 0, 0], [0, 0, -14, 94, 58, -10, 0, 0], [0, 0, -12, 76, 76, -12, 0, 0],
        [0, 0, -10, 58, 94, -14, 0, 0], [0, 0, -8, 38, 110, -12, 0, 0], [0, 0, -4, 18, 122, -8, 0, 0]],
    3: [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 76, 76, -14, 2, 0],
        [0, 2, -12, 58, 94, -16, 2, 0], [0, 2, -10, 38, 110, -14, 2, 0], [0, 0, -4, 18, 122, -10, 2, 0]],
}
UP_TABLE_NAMES = {1: "av1_bilinear_filters", 2: "av1_sub_pel_filters_4", 3: "av1_sub_pel_filters_8"}


def i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def i32(v):
    return ((int(v) + (1 << 31)) & M32) - (1 << 31)


def tdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- the predictions: `plane` a 2-D uint8 array, (y, x) the sample the C's pointer names ---------------------------------------------------------------------
def full_pred(plane, y, x, W, H):
    return plane[y:y + H, x:x + W].astype(np.int64)


def bilinear_pred(plane, y, x, W, H, xo, yo):
    """aom_var_filter_block2d_bil_first_pass_c + _second_pass_c.  The C reads (W + 1) x (H + 1) samples whatever the offsets are; the extra column / row is
    multiplied by 0 at offset 0 and is not touched here."""
    rows = H + (1 if yo else 0)
    a = plane[y:y + rows, x:x + W + (1 if xo else 0)].astype(np.int64)
    f0, f1 = BILINEAR_2T[xo]
    g0, g1 = BILINEAR_2T[yo]
    first = (a[:, :W] * f0 + a[:, 1:W + 1] * f1 + 64) >> 7 if xo else a
    if not yo:
        return first
    return (first[:H] * g0 + first[1:H + 1] * g1 + 64) >> 7


def upsampled_pred(plane, y, x, W, H, xq, yq, taps, stats=None):
    """svt_aom_upsampled_pred_c.  stats (a dict) counts how often each 8-bit clip binds: h_lo, h_hi, v_lo, v_hi."""
    def conv(win, row, key):  # win[..., 8] samples, row 8 taps
        s = (win * np.asarray(row, np.int64)).sum(-1)
        r = (s + 64) >> 7
        if stats is not None:
            stats[key + "_lo"] = stats.get(key + "_lo", 0) + int((r < 0).sum())
            stats[key + "_hi"] = stats.get(key + "_hi", 0) + int((r > 255).sum())
        return np.clip(r, 0, 255)
    if not xq and not yq:
        return full_pred(plane, y, x, W, H)
    rows = UP_ROWS[taps]
    if not yq:
        a = plane[y:y + H, x - 3:x + W + 4].astype(np.int64)
        return conv(np.stack([a[:, k:k + W] for k in range(8)], -1), rows[xq], "h")
    if not xq:
        a = plane[y - 3:y + H + 4, x:x + W].astype(np.int64)
        return conv(np.stack([a[k:k + H] for k in range(8)], -1), rows[yq], "v")
    ih = (((H - 1) * 8 + yq) >> 3) + 8
    a = plane[y - 3:y - 3 + ih, x - 3:x + W + 4].astype(np.int64)
    tmp = conv(np.stack([a[:, k:k + W] for k in range(8)], -1), rows[xq], "h")
    return conv(np.stack([tmp[k:k + H] for k in range(8)], -1), rows[yq], "v")


def variance(pred, src):
    """variance_c + VAR(W, H): (var, sse, sum)"""
    diff = pred.astype(np.int64) - src.astype(np.int64)
    s, sse = int(diff.sum()), int((diff * diff).sum()) & M32
    return (sse - (((s * s) // diff.size) & M32)) & M32, sse, s


def obmc_diffs(pred, wsrc, mask):
    v = wsrc.astype(np.int64).reshape(pred.shape) - pred.astype(np.int64) * mask.astype(np.int64).reshape(pred.shape)
    mag = (np.abs(v) + 2048) >> 12
    return v, mag, np.where(v < 0, -mag, mag)  # ROUND_POWER_OF_TWO_SIGNED: the magnitude is rounded


def block_var(kind, bsize, pre, py, px, xo=0, yo=0, taps=0, src=None, wsrc=None, mask=None, stats=None):
    """one descriptor of svt_hip_block_var_batch: (var, sse, sum, sad); src a W x H block"""
    W, H = BW[bsize], BH[bsize]
    if kind in (SUBPIX, OBMC_SUBPIX):
        pred = bilinear_pred(pre, py, px, W, H, xo, yo)
    elif kind == UPSAMPLED:
        pred = upsampled_pred(pre, py, px, W, H, xo, yo, taps, stats)
    else:
        pred = full_pred(pre, py, px, W, H)
    if kind >= OBMC_SAD:
        v, mag, d = obmc_diffs(pred, wsrc, mask)
        if stats is not None:
            stats["tie_pos"] = stats.get("tie_pos", 0) + int(((v > 0) & ((v & 4095) == 2048)).sum())
            stats["tie_neg"] = stats.get("tie_neg", 0) + int(((v < 0) & ((-v & 4095) == 2048)).sum())
        if kind == OBMC_SAD:
            return 0, 0, 0, int(mag.sum()) & M32
        s, sse = int(d.sum()), int((d * d).sum()) & M32
        return (sse - (((s * s) // d.size) & M32)) & M32, sse, s, 0
    var, sse, s = variance(pred, src)
    if kind == MSE:
        return sse, sse, 0, 0
    return var, sse, s, 0


# ---- the search --------------------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(method=0, bsize=6, start=(0, 0), ref_mv=(0, 0), lims=None, allow_hp=1, forced_stop=0, iters_per_step=2, pred_variance_th=0, abs_th_mult=0,
                round_dev_th=INT_MAX, skip_diag_refinement=0, subpel_search_type=3, bias_fp=0, qp=40, early_exit=0, mv_cost_type=1, error_per_bit=120, early_exit_th=0,
                cost_table=-1, mvp_th=0, hp_mv_th=0, best_mvp_err=0, best_mvp=(0, 0))
RULES = ("early_exit", "pred_variance_th", "abs_th", "round_dev_th", "opt_pre_exit", "bias_fp", "mvp_th", "hp_mv_th")


def mv_limits(mi_row, mi_col, bsize, mi_rows, mi_cols, ref_mv):
    """md_subpel_search :2656-2666: (col_min, col_max, row_min, row_max)"""
    mi_w, mi_h = BW[bsize] >> 2, BH[bsize] >> 2
    row_min, col_min = -(((mi_row + mi_h) * 4) + 4), -(((mi_col + mi_w) * 4) + 4)
    row_max, col_max = (mi_rows - mi_row) * 4 + 4, (mi_cols - mi_col) * 4 + 4
    rr, rc = ref_mv
    # svt_av1_set_mv_search_range
    col_min = max(col_min, max((rc >> 3) - 1023 + (1 if rc & 7 else 0), (-MV_UPP >> 3) + 1))
    row_min = max(row_min, max((rr >> 3) - 1023 + (1 if rr & 7 else 0), (-MV_UPP >> 3) + 1))
    col_max = min(col_max, min((rc >> 3) + 1023, (MV_UPP >> 3) - 1))
    row_max = min(row_max, min((rr >> 3) + 1023, (MV_UPP >> 3) - 1))
    # svt_av1_set_subpel_mv_search_range
    mx = 8 * 1023
    return (max(-MV_UPP + 1, max(col_min * 8, rc - mx)), min(MV_UPP - 1, min(col_max * 8, rc + mx)),
            max(-MV_UPP + 1, max(row_min * 8, rr - mx)), min(MV_UPP - 1, min(row_max * 8, rr + mx)))


WIDE_LIMITS = mv_limits(64, 64, 6, 512, 512, (0, 0))


def mv_err_cost(r, c, p, table):
    """svt_mv_err_cost; table = (joint[4], comp[2][MV_VALS]) or None"""
    dr, dc = i16(r - p["ref_mv"][0]), i16(c - p["ref_mv"][1])
    ad = i16(abs(dr)) + i16(abs(dc))
    t = p["mv_cost_type"]
    if t == 0:
        if table is None:
            return 0
        j = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
        at = lambda v: min(max(MV_MAX + min(max(v, -MV_UPP), MV_UPP), 0), MV_VALS - 1)
        rate = i32(int(table[0][j]) + int(table[1][0][at(dr)]) + int(table[1][1][at(dc)]))
        return i32((rate * p["error_per_bit"] + 8192) >> 14)
    if t == 1:
        return (2 * ad) >> 3
    if t == 3:
        return ad >> 3
    if t == 4:
        return i32(((ad << 8) * p["error_per_bit"] + 8192) >> 14)
    return 0


def md_subpel_search(src, ref, ry, rx, params, table=None, off=()):
    """One item.  src: the W x H source block; ref: the reference plane, (ry, rx) the block's position in it.  `off`: rules of RULES switched off (the test's proof
    that a case depends on a rule).  Returns dict(mv_row, mv_col, besterr, distortion, sse1, fp_me_dist, evals)."""
    p = dict(DEFAULTS)
    p.update(params)
    W, H = BW[p["bsize"]], BH[p["bsize"]]
    ln = (W * H).bit_length() - 1
    lims = p["lims"] if p["lims"] is not None else WIDE_LIMITS
    pruned = p["method"] != 0
    st = dict(br=i16(p["start"][0]), bc=i16(p["start"][1]), besterr=0, distortion=0, sse1=0, evals=1, better=0)
    at = lambda r, c: (ry + (r >> 3), rx + (c >> 3))
    cost_of = lambda r, c: mv_err_cost(r, c, p, table) & M32

    y0, x0 = at(st["br"], st["bc"])
    var, _, _ = variance(full_pred(ref, y0, x0, W, H), src)
    st["distortion"] = i32(var)
    st["besterr"] = (var + cost_of(st["br"], st["bc"])) & M32
    fp_me_dist = st["besterr"]

    def result():
        return dict(mv_row=st["br"], mv_col=st["bc"], besterr=st["besterr"], distortion=st["distortion"], sse1=st["sse1"], fp_me_dist=fp_me_dist, evals=st["evals"])

    rnd = min(3 - p["forced_stop"], 3 - (0 if p["allow_hp"] else 1))
    if not pruned and p["mvp_th"] > 0:
        mvp_err, me_err = i32(p["best_mvp_err"] + 1), i32(st["besterr"] + 1)
        dev = tdiv((me_err - mvp_err) * 100, me_err) if me_err else 0
        if dev >= p["mvp_th"] and "mvp_th" not in off:
            rnd = 1
        elif (abs(st["bc"] - p["best_mvp"][1]) > p["hp_mv_th"] or abs(st["br"] - p["best_mvp"][0]) > p["hp_mv_th"]) and "hp_mv_th" not in off:
            rnd = min(rnd, 2)
    if p["early_exit"] and "early_exit" not in off:
        return result()

    def low_variance():
        v, _, _ = variance(full_pred(ref, y0, x0, W, H), np.full((H, W), 128))
        return i32(((v + ((1 << ln) >> 1)) & M32) >> ln) < p["pred_variance_th"] and "pred_variance_th" not in off

    def below_abs_th(shift):
        th = i32(((W * H) >> shift) * p["abs_th_mult"] * (p["qp"] >> 1))
        return st["besterr"] < (th & M64) and "abs_th" not in off

    org_error = 0
    if not pruned:
        if low_variance() or below_abs_th(2) or not rnd:
            return result()
    else:
        if below_abs_th(3) or not rnd or low_variance():
            return result()
        if p["skip_diag_refinement"] < 4:
            demo = (2 if (W >= 64 or H >= 64) else 1) if p["skip_diag_refinement"] >= 2 else 1
            org_error = st["besterr"] // demo if p["skip_diag_refinement"] else INT_MAX

    def check(r, c):
        r, c = i16(r), i16(c)
        if not (lims[0] <= c <= lims[1] and lims[2] <= r <= lims[3]):
            return INT_MAX
        cost = cost_of(r, c)
        if pruned and p["mv_cost_type"] == 4 and "opt_pre_exit" not in off:
            bestcost = (st["distortion"] + cost) & M32
            if bestcost > tdiv(st["besterr"] * p["early_exit_th"], 1000):
                return bestcost
        yy, xx = at(r, c)
        pred = bilinear_pred(ref, yy, xx, W, H, c & 7, r & 7) if pruned else upsampled_pred(ref, yy, xx, W, H, c & 7, r & 7, p["subpel_search_type"])
        mse, sse, _ = variance(pred, src)
        st["evals"] += 1
        cost = (cost + mse) & M32
        weight = 100
        if p["bias_fp"] and st["bc"] % 8 == 0 and st["br"] % 8 == 0 and "bias_fp" not in off:
            weight = p["bias_fp"]
        if ((cost * (weight & M64)) & M64) // 100 < st["besterr"]:
            st.update(besterr=cost, br=r, bc=c, distortion=i32(mse), sse1=sse, better=1)
        return cost

    h = 4
    for it in range(rnd):
        tr, tc, prev = st["br"], st["bc"], st["besterr"]
        left, right, up, down = check(tr, tc - h), check(tr, tc + h), check(tr - h, tc), check(tr + h, tc)
        dsr, dsc = (-h if up <= down else h), (-h if left <= right else h)
        if not pruned:
            check(tr + dsr, tc + dsc)
            if (tr, tc) != (st["br"], st["bc"]) and p["iters_per_step"] > 1:  # svt_second_level_check_v2
                b0r, b0c = st["br"], st["bc"]
                if tr == b0r:
                    dsr = -dsr
                elif tc == b0c:
                    dsc = -dsc
                st["better"] = 0
                check(b0r + dsr, b0c)
                check(b0r, b0c + dsc)
                if st["better"]:
                    check(b0r + dsr, b0c + dsc)
        else:
            if st["besterr"] < org_error:
                check(tr + dsr, tc + dsc)
            if st["besterr"] < org_error and p["iters_per_step"] > 1:  # second_level_check_fast
                b0r, b0c = st["br"], st["bc"]
                if tr != b0r and tc != b0c:
                    check(b0r, b0c + dsc)
                    check(b0r + dsr, b0c)
                elif tr == b0r and tc != b0c:
                    check(b0r + h, b0c + dsc)
                    check(b0r - h, b0c + dsc)
                    check(b0r - dsr, b0c)
                elif tr != b0r and tc == b0c:
                    check(b0r + dsr, b0c + h)
                    check(b0r + dsr, b0c - h)
                    check(b0r, b0c - dsc)
        h >>= 1
        if pruned:
            if p["skip_diag_refinement"] and it < 1:
                org_error = min(org_error, st["besterr"])
            dev = i32(tdiv((max(st["besterr"], 1) - max(prev, 1)) * 100, max(prev, 1)))
            if dev >= p["round_dev_th"] and "round_dev_th" not in off:
                break
    return result()


# ---- shared inputs -------------------------------------------------------------------------------------------------------------------------------------------
PAD = 24  # samples around the block in a search / primitive reference plane: a start vector of up to 2 samples, 7/8 of search, 4 of filter


def smooth_plane(g, h, w):
    a = g.integers(0, 256, (h + 4, w + 4)).astype(np.int64)
    for _ in range(2):
        a = a[:-2, :-2] + a[1:-1, :-2] + a[2:, :-2] + a[:-2, 1:-1] + a[1:-1, 1:-1] + a[2:, 1:-1] + a[:-2, 2:] + a[1:-1, 2:] + a[2:, 2:]
        a = (a + 4) // 9
    b = a.astype(np.float64)
    b = (b - b.min()) * (255.0 / max(b.max() - b.min(), 1.0))
    return b.astype(np.uint8)


def primitive_inputs(case):
    """(pre plane, py, px, src block, wsrc, mask) of a primitive case: dict(kind, bsize, xo, yo, taps, content, seed)"""
    g = np.random.default_rng(case["seed"])
    W, H = BW[case["bsize"]], BH[case["bsize"]]
    shape = (H + 2 * PAD, W + 2 * PAD)
    content = case["content"]
    if content == "sat_hi":
        pre, src = np.full(shape, 255, np.uint8), np.zeros((H, W), np.uint8)
    elif content == "sat_lo":
        pre, src = np.zeros(shape, np.uint8), np.full((H, W), 255, np.uint8)
    elif content.startswith("checker"):
        cell = int(content[7:])
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        pre = ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)
        src = g.integers(0, 256, (H, W), dtype=np.uint8)
    else:
        pre, src = g.integers(0, 256, shape, dtype=np.uint8), g.integers(0, 256, (H, W), dtype=np.uint8)
    wsrc = mask = None
    if case["kind"] >= OBMC_SAD:
        mode = case.get("mask", "mixed")
        mask = (np.zeros(W * H) if mode == "zero" else np.full(W * H, 4096) if mode == "full" else g.integers(0, 4097, W * H)).astype(np.int32)
        pred = bilinear_pred(pre, PAD, PAD, W, H, case["xo"], case["yo"]) if case["kind"] == OBMC_SUBPIX else full_pred(pre, PAD, PAD, W, H)
        # differences on the +-0.5 ties of the >> 12 rounding, in both signs, among ordinary ones
        v = g.integers(-40 * 4096, 40 * 4096, W * H)
        tie = g.integers(0, 4, W * H)
        v = np.where(tie == 0, 2048 + 4096 * g.integers(0, 8, W * H), np.where(tie == 1, -2048 - 4096 * g.integers(0, 8, W * H), v))
        wsrc = (pred.reshape(-1) * mask.astype(np.int64) + v).astype(np.int32)
    return pre, PAD, PAD, src, wsrc, mask


def primitive_cases():
    cases, seed = [], 1000

    def add(kind, bsize, xo=0, yo=0, taps=0, content="rand", **kw):
        nonlocal seed
        seed += 1
        cases.append(dict(kind=kind, bsize=bsize, xo=xo, yo=yo, taps=taps, content=content, seed=seed, **kw))
    for b in range(22):  # every kind at every one of its sizes
        add(VAR, b)
        add(SUBPIX, b, 1 + b % 7, 1 + (b * 3) % 7)
        add(UPSAMPLED, b, 1 + (b * 5) % 7, 1 + b % 7, 1 + b % 3)
        add(OBMC_SAD, b)
        add(OBMC_VAR, b, mask=("zero", "full", "mixed")[b % 3])
        add(OBMC_SUBPIX, b, 1 + (b * 2) % 7, (b * 3) % 8)
    add(MSE, 6)
    for b in (0, 17, 16, 12):  # 4x4, 16x4, 4x16, 64x64: all 64 offsets
        for o in range(64):
            add(SUBPIX, b, o & 7, o >> 3)
    for b in (0, 3, 20):  # 4x4, 8x8, 16x64: all 64 x 3 tap choices
        for t in (1, 2, 3):
            for o in range(64):
                add(UPSAMPLED, b, o & 7, o >> 3, t)
    for kind in (VAR, SUBPIX, UPSAMPLED):  # the sums at their extremes
        for content in ("sat_hi", "sat_lo"):
            add(kind, 15, 3 if kind != VAR else 0, 5 if kind != VAR else 0, 3 if kind == UPSAMPLED else 0, content)
    for cell in (1, 2, 3):  # both 8-bit clips of both stages
        for o in (0o44, 0o22, 0o66, 0o40, 0o04, 0o13):
            add(UPSAMPLED, 6, o & 7, o >> 3, 3, "checker%d" % cell)
    for mode in ("zero", "full", "mixed"):
        add(OBMC_VAR, 6, mask=mode)
        add(OBMC_SAD, 9, mask=mode)
        add(OBMC_SUBPIX, 3, 4, 4, mask=mode)
    return cases


def run_primitive(case, stats=None):
    pre, py, px, src, wsrc, mask = primitive_inputs(case)
    return block_var(case["kind"], case["bsize"], pre, py, px, case["xo"], case["yo"], case["taps"], src, wsrc, mask, stats)


def cost_tables():
    """two per-frame tables, deterministic: a V-shaped rate in the component's magnitude plus noise"""
    g = np.random.default_rng(77)
    out = []
    for k in range(2):
        v = np.abs(np.arange(-MV_MAX, MV_MAX + 1))
        comp = np.stack([(300 + 40 * (k + 1) * np.log2(1 + v) * 16).astype(np.int64) + g.integers(0, 64, MV_VALS) for _ in range(2)]).astype(np.int32)
        out.append((np.array([200, 900 + 100 * k, 950, 1500], np.int32), comp))
    return out


def search_inputs(case):
    """(source block, reference plane, ry, rx): `shift` content makes the source the reference moved by a known fractional vector"""
    g = np.random.default_rng(case["seed"])
    W, H = BW[case["bsize"]], BH[case["bsize"]]
    content = case["content"]
    if content == "flat":
        ref = np.clip(np.full((H + 2 * PAD, W + 2 * PAD), 128) + g.integers(-1, 2, (H + 2 * PAD, W + 2 * PAD)), 0, 255).astype(np.uint8)
        src = g.integers(100, 156, (H, W), dtype=np.uint8)
    elif content == "rand":
        ref, src = g.integers(0, 256, (H + 2 * PAD, W + 2 * PAD), dtype=np.uint8), g.integers(0, 256, (H, W), dtype=np.uint8)
    else:
        ref = smooth_plane(g, H + 2 * PAD, W + 2 * PAD)
        r, c = case["true_mv"]
        src = upsampled_pred(ref, PAD + (r >> 3), PAD + (c >> 3), W, H, c & 7, r & 7, 3)
        src = np.clip(src + g.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
    return src, ref, PAD, PAD


def search_cases():
    cases, seed = [], 5000

    def add(content="shift", true_mv=(13, -10), **kw):
        nonlocal seed
        seed += 1
        c = dict(DEFAULTS, content=content, true_mv=true_mv, seed=seed)
        c.update(kw)
        if "start" not in kw:
            c["start"] = (((true_mv[0] + 4) >> 3) * 8, ((true_mv[1] + 4) >> 3) * 8)
        cases.append(c)
    for m in (0, 1):
        for b in (0, 2, 6, 21):  # 4x4, 8x4, 16x16, 64x16
            add("rand", method=m, bsize=b, start=(8, -16))
            add("shift", (-11, 5), method=m, bsize=b)
        add("shift", (3, 6), method=m, bsize=15)  # 128x128
        for t in range(6):  # every MV_COST_TYPE; ENTROPY with each table and without one
            add(method=m, mv_cost_type=t, ref_mv=(20, -30), cost_table=t % 2 if t == 0 else -1)
        add(method=m, mv_cost_type=0, ref_mv=(-9, 4), cost_table=1, error_per_bit=700)
        add(method=m, mv_cost_type=0, ref_mv=(-9, 4), cost_table=-1)
        for hp in (0, 1):
            for fs in range(4):
                add("shift", (5, -3), method=m, allow_hp=hp, forced_stop=fs, bsize=2)
        for it in (1, 2):
            add("shift", (6, 6), method=m, iters_per_step=it)
            add("rand", method=m, iters_per_step=it, start=(0, 8))
        for t in (1, 2, 3):
            add("shift", (-5, 7), method=m, subpel_search_type=t)
        for bias in (0, 130):
            add("shift", (1, -1), method=m, bias_fp=bias, bsize=6)
            add("shift", (2, 1), method=m, bias_fp=bias, bsize=2)
        # each early return taken and not taken
        add(method=m, early_exit=1)
        add("flat", method=m, pred_variance_th=50)
        add(method=m, pred_variance_th=50)
        add(method=m, abs_th_mult=200, qp=63)
        add(method=m, abs_th_mult=1, qp=2)
        # limits: the start vector on each limit and one step inside it
        for k in range(4):
            for inside in (0, 4):
                lims = [-800, 800, -800, 800]
                start = (16, -8)
                lims[k] = (start[1] if k < 2 else start[0]) + (-inside if k % 2 == 0 else inside)
                add("shift", (18, -9), method=m, bsize=2, start=start, lims=tuple(lims))
    for sd in range(5):  # skip_diag_refinement 0 .. 4, with and without the >= 64 divisor
        add("shift", (-3, 2), method=1, skip_diag_refinement=sd)
        add("shift", (-3, 2), method=1, skip_diag_refinement=sd, bsize=21)
        add("rand", method=1, skip_diag_refinement=sd, start=(0, 0))
    add("shift", (3, 3), method=1, round_dev_th=-20)  # fires after the first round
    add("shift", (3, 3), method=1, round_dev_th=-95)
    add("shift", (3, 3), method=1, round_dev_th=0)
    for th in (900, 1000, 1050):  # the MV_COST_OPT pre-evaluation exit
        add("shift", (3, -5), method=1, mv_cost_type=4, early_exit_th=th, ref_mv=(40, 40), error_per_bit=3000)
        add("rand", method=1, mv_cost_type=4, early_exit_th=th, ref_mv=(-24, 16), error_per_bit=900, start=(8, 8))
    add("shift", (3, -5), method=0, mvp_th=10, best_mvp_err=10, hp_mv_th=1000)  # the ME centre is far worse than the MVP: round = 1
    add("shift", (3, -5), method=0, mvp_th=100, best_mvp_err=10, hp_mv_th=4, best_mvp=(40, 0))  # far from the MVP: round capped at 2
    add("shift", (3, -5), method=0, mvp_th=100, best_mvp_err=10, hp_mv_th=1000, best_mvp=(40, 0))
    return cases


def run_search(case, off=()):
    src, ref, ry, rx = search_inputs(case)
    params = {k: v for k, v in case.items() if k in DEFAULTS}
    tabs = cost_tables()
    ct = params.get("cost_table", -1)
    return md_subpel_search(src, ref, ry, rx, params, tabs[ct] if ct >= 0 else None, off)


RESULT_FIELDS = ("mv_row", "mv_col", "besterr", "distortion", "sse1", "fp_me_dist")
