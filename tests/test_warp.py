"""AV1 warped motion (csrc/warp.hip): svt_hip_warp_pred_batch, svt_hip_warp_model_batch, svt_hip_warp_error_batch and the two single-call forms, every output against
tests/warp_common.py (numpy; pinned on the reference's C by tests/test_warp_ref.py) and against tests/golden/warp.npz (what the reference's C computed).
Every batched prediction runs on reference planes with odd strides (77 / 45 samples, the pictures behind a lead-in of 11 / 7 samples, the last row ending with its last
sample), destination stride 547, blocks at every alignment, the destination filled with 0xA5 beforehand: the WHOLE destination plane is compared, so a sample written
outside a block's p_width x p_height fails like a wrong sample inside it.  Full-range 12-bit samples are checked here against the restatement only (the reference's
high-bit-depth C takes 10-bit samples by construction)."""
import ctypes as C
import mmap

import numpy as np
import pytest

import warp_common as wc
from conftest import EmuBackend, _backends, p, rng

SD = 547
PLANE_A, PLANE_B = 5, 30
PIC_A, PIC_B = (72, 56, 77, 11), (41, 33, 45, 7)  # width, height, stride, lead-in
BIT_DEPTHS = (8, 10, 12)
SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (64, 8), (4, 4), (4, 8), (12, 20), (14, 6), (1, 1)]
SUBS = ((0, 0), (1, 1), (1, 0), (0, 1))
WEIGHTS = ((9, 7), (11, 5), (12, 4), (13, 3))  # the four pairs svt_av1_dist_wtd_comp_weight_assign returns (quant_dist_lookup_table, either order)
# inside; straddling left, right, top, bottom and the four corners; outside each side by a few samples; outside by more than width + 6 / below -7; far outside
POSITIONS = [(16, 16), (3, 5), (-5, 21), (66, 13), (30, -4), (29, 51), (-6, -6), (67, -5), (-5, 50), (67, 50), (-22, 20), (84, 20), (20, -24), (20, 66), (-120, 20), (190, 20),
             (20, -100), (20, 170), (-14000, -14000), (14000, 12000)]  # (the last two: 28 000 luma samples outside when sub-sampled, just inside the int32_t range of dst_x)
MODELS = wc.models()
NAMES = list(MODELS)


def spec(pw, ph, pos, model, ss=(0, 0), comp=0, wts=(9, 7), model2="zoom", swap=False):
    return dict(pw=pw, ph=ph, pos=pos, model=model, ss=ss, comp=comp, wts=wts, model2=model2, swap=swap)


def flat_plane(pic2d, width, lead):
    """lead-in, then the picture's rows at their stride, the last row ending with its last sample"""
    body = pic2d.reshape(-1)[:pic2d.size - (pic2d.shape[1] - width)]
    return np.concatenate([np.full(lead, 7, pic2d.dtype), body])


def fill_ref(r, i, k, off, mat, sh, w, h, stride, plane):
    r["ref_off"][i, k], r["mat"][i, k], r["width"][i, k], r["height"][i, k], r["stride"][i, k], r["plane"][i, k] = off, mat, w, h, stride, plane
    r["alpha"][i, k], r["beta"][i, k], r["gamma"][i, k], r["delta"][i, k] = sh


def build(be, specs, bd, g, kind="random", pics=None):
    """the two reference pictures, descriptors and the expected destination plane of one launch"""
    dt = np.uint16 if bd > 8 else np.uint8
    A = wc.make_picture(g, kind, *PIC_A[:3], bd) if pics is None else pics[0]
    B = wc.make_picture(g, kind, *PIC_B[:3], bd) if pics is None else pics[1]
    x = y = shelf = 0
    pos = []
    for s in specs:
        gap = 1 + int(g.integers(0, 7))
        if x + gap + s["pw"] > SD - 8:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + s["pw"], max(shelf, s["ph"])
    fill = 0xA5A5 if bd > 8 else 0xA5
    want = np.full((y + shelf + 2, SD), fill, dt)
    d = np.zeros(len(specs), be.pkg.WarpDesc)
    for i, (s, (dx, dy)) in enumerate(zip(specs, pos)):
        first, second = ((B, PIC_B, PLANE_B), (A, PIC_A, PLANE_A)) if s["swap"] else ((A, PIC_A, PLANE_A), (B, PIC_B, PLANE_B))
        refs = []
        for k, ((pic, geo, plane), name) in enumerate(zip((first, second), (s["model"], s["model2"]))):
            mat, sh = MODELS[name] if isinstance(name, str) else name
            fill_ref(d["ref"], i, k, geo[3], mat, sh, geo[0], geo[1], geo[2], plane)
            refs.append((pic, mat, sh, geo[0], geo[1]))
        d["dst_off"][i], d["dst_stride"][i], d["p_col"][i], d["p_row"][i], d["p_width"][i], d["p_height"][i] = dy * SD + dx, SD, s["pos"][0], s["pos"][1], s["pw"], s["ph"]
        d["subsampling_x"][i], d["subsampling_y"][i], d["compound"][i], d["fwd_offset"][i], d["bck_offset"][i] = s["ss"][0], s["ss"][1], s["comp"], s["wts"][0], s["wts"][1]
        want[dy:dy + s["ph"], dx:dx + s["pw"]] = wc.warp_pred(refs, s["pos"][0], s["pos"][1], s["pw"], s["ph"], s["ss"][0], s["ss"][1], bd, s["comp"], *s["wts"])
    return A, B, d, want, fill


def launch(be, A, B, d, dst, bd, status=None, n=None):
    planes = be.pkg.InterPredPlanes()
    dA, dB, dd = be.dev(flat_plane(A, PIC_A[0], PIC_A[3])), be.dev(flat_plane(B, PIC_B[0], PIC_B[3])), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    r = be.lib.svt_hip_warp_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(d) if n is None else n, bd, None if status is None else be.ptr(status), be.stream)
    be.sync()
    return r, (dA, dB, dd)


_built = {}  # the restatement's side of a launch, computed once and shared by the backends


def run(be, key, make_specs, bd, seed, kind="random", with_status=False):
    if key not in _built:
        specs = make_specs()
        _built[key] = build(be, specs, bd, rng(seed), kind) + (specs,)
    A, B, d, want, fill, specs = _built[key]
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    status = be.dev(np.full(len(specs), 7, np.uint8)) if with_status else None
    r, keep = launch(be, A, B, d, dst, bd, status)
    assert r == 0
    got = be.host(dst).reshape(want.shape)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        for i, s in enumerate(specs):
            yy, xx = divmod(int(d["dst_off"][i]), SD)
            a, b = got[yy:yy + s["ph"], xx:xx + s["pw"]], want[yy:yy + s["ph"], xx:xx + s["pw"]]
            assert np.array_equal(a, b), (bd, i, s, np.argwhere(a != b)[:4], a[:2, :8], b[:2, :8])
        raise AssertionError("samples outside every block's p_width x p_height were written: %s" % (np.argwhere(got != want)[:8],))


def case_list(bd):
    """every size at every position and every model at every position, the sub-samplings, compound forms and weights cycling; one 128 x 128 block"""
    specs, k = [], bd
    for (pw, ph) in SIZES:
        for pos in POSITIONS:
            k += 1
            specs.append(spec(pw, ph, (pos[0] + k % 3, pos[1] + k % 2), NAMES[k % len(NAMES)], SUBS[k % 4], k % 3, WEIGHTS[(k // 3) % 4], NAMES[(k // 2 + 5) % len(NAMES)], k % 5 == 0))
    for name in NAMES:
        for pos in POSITIONS[:10]:
            k += 1
            specs.append(spec(16, 16, pos, name, SUBS[k % 4], k % 3, WEIGHTS[k % 4], NAMES[(k + 1) % len(NAMES)], k % 2 == 0))
    specs.append(spec(128, 128, (-20, -30), "rotation", comp=1, model2="affine"))
    for t0 in (-wc.TRANS_CLAMP, wc.TRANS_CLAMP - 1):  # mat[0], mat[1] at +-WARPEDMODEL_TRANS_CLAMP
        for t1 in (-wc.TRANS_CLAMP, wc.TRANS_CLAMP - 1):
            mat = [t0, t1, 65536 + 900, -700, 650, 65536 - 800]
            specs.append(spec(16, 16, (13, 22), (mat, wc.get_shear_params(mat)), SUBS[1], 2, WEIGHTS[1], "translation"))
    return specs


@pytest.mark.parametrize("kind", wc.CLASSES)
@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_sizes_models_positions_formats(be, bd, kind):
    """the case list at each bit depth on random, flat and extreme (0 / max alternating) pictures"""
    wc.ROWS_SEEN.clear()
    fresh = ("cases", bd, kind) not in _built
    run(be, ("cases", bd, kind), lambda: case_list(bd), bd, 100 + bd, kind, with_status=bd == 10)
    if fresh:
        assert 0 in wc.ROWS_SEEN and 192 in wc.ROWS_SEEN  # both ends of the filter table are reached (the two alpha_limit models)


@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_launch_sizes_around_a_workgroup(be, n):
    """B - 1, B, B + 1 descriptors of mixed sizes for the B = 16 descriptors one workgroup flattens: the prefix sum across workgroup boundaries"""
    assert be.pkg.WARP_DESCS_PER_WORKGROUP == 16

    def make():
        g = rng(n)
        pool = case_list(8)
        return [pool[int(g.integers(len(pool)))] for _ in range(n)]
    run(be, ("launch", n), make, 8, 400 + n, with_status=n == 17)


@pytest.mark.parametrize("bd", (8, 10))
def test_one_sample_wide_and_one_row_high_pictures(be, bd):
    """a 1 x 40, a 40 x 1 and a 1 x 1 reference picture: every tap of every sample clamps to the one column / row"""
    g = rng(50 + bd)
    dt = np.uint16 if bd > 8 else np.uint8
    for (w, h) in ((1, 40), (40, 1), (1, 1)):
        pic = wc.make_picture(g, "random", w, h, w + 2, bd)
        items = [((12, 20), (2, 1), "translation"), ((8, 8), (-3, 30), "affine"), ((16, 16), (0, 0), "beta_limit"), ((4, 4), (35, -2), "rotation")]
        d = np.zeros(len(items), be.pkg.WarpDesc)
        want = np.full((20, 64), 0xA5, dt)
        for i, ((pw, ph), pos, name) in enumerate(items):
            mat, sh = MODELS[name]
            fill_ref(d["ref"], i, 0, 3, mat, sh, w, h, w + 2, 2)
            d["dst_off"][i], d["dst_stride"][i], d["p_col"][i], d["p_row"][i], d["p_width"][i], d["p_height"][i] = 17 * i, 64, pos[0], pos[1], pw, ph
            want[:ph, 17 * i:17 * i + pw] = wc.warp_pred([(pic, mat, sh, w, h)], pos[0], pos[1], pw, ph, 0, 0, bd)
        planes = be.pkg.InterPredPlanes()
        dp, dd, dst = be.dev(flat_plane(pic, w, 3)), be.dev(d), be.dev(np.full(want.shape, 0xA5, dt))
        planes.base[2] = be.ptr(dp)
        assert be.lib.svt_hip_warp_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(items), bd, None, be.stream) == 0
        assert np.array_equal(be.host(dst), want), (bd, w, h)


def test_golden_cases(be):
    """the prediction cases of tests/golden/warp.npz through the batched entry: the kernel == what the reference's C computed"""
    gold = wc.load_golden()
    assert int(gold["seed"][0]) == wc.GOLDEN_SEED
    cases = wc.golden_warp_cases()
    for bd in BIT_DEPTHS:
        idx = [i for i, c in enumerate(cases) if c[1] == bd]
        pics = [gold["pic_%d_%d" % (bd, k)] for k in (0, 1)]
        assert all(np.array_equal(pics[k], wc.golden_picture(min(bd, 10), k)) for k in (0, 1))
        d = np.zeros(len(idx), be.pkg.WarpDesc)
        off = 0
        for j, i in enumerate(idx):
            name, _, pc, pr, pw, ph, ssx, ssy, comp, fwd, bck, second = cases[i]
            for k, nm in enumerate((name, second)):
                fill_ref(d["ref"], j, k, 0, *MODELS[nm], wc.GOLDEN_W, wc.GOLDEN_H, wc.GOLDEN_STRIDE, k)
            d["dst_off"][j], d["dst_stride"][j], d["p_col"][j], d["p_row"][j], d["p_width"][j], d["p_height"][j] = off, pw, pc, pr, pw, ph
            d["subsampling_x"][j], d["subsampling_y"][j], d["compound"][j], d["fwd_offset"][j], d["bck_offset"][j] = ssx, ssy, comp, fwd, bck
            off += pw * ph
        planes = be.pkg.InterPredPlanes()
        d0, d1, dd, dst = be.dev(pics[0]), be.dev(pics[1]), be.dev(d), be.dev(np.zeros(off, pics[0].dtype))
        planes.base[0], planes.base[1] = be.ptr(d0), be.ptr(d1)
        assert be.lib.svt_hip_warp_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(idx), bd, None, be.stream) == 0
        got = be.host(dst)
        for j, i in enumerate(idx):
            pw, ph = cases[i][4:6]
            o = int(d["dst_off"][j])
            assert np.array_equal(got[o:o + pw * ph].reshape(ph, pw), gold["warp_%d" % i]), (i, cases[i])


INVALID = ["p_width 0", "p_width 129", "p_height 0", "p_height 200", "subsampling_x 2", "subsampling_y 2", "compound 3", "width 0", "height -1", "stride 0", "plane 32",
           "NULL plane", "second width 0", "second NULL plane", "alpha beta shear", "gamma delta shear", "second shear", "dst_x overflow", "dst_y overflow",
           "last tile overflows"]


@pytest.mark.parametrize("what", INVALID)
def test_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones: with status == NULL the call returns -1 and not one destination sample changes; with a status array it returns 0,
    flags that descriptor alone, leaves its block untouched and predicts the other two.  The descriptor is compound, so its second reference is checked too"""
    g = rng(9)
    specs = [spec(8, 8, (3, 5), "affine"), spec(16, 16, (10, 12), "rotation", comp=1, model2="zoom"), spec(12, 20, (-5, 21), "translation", SUBS[1], 2, WEIGHTS[2])]
    A, B, d, want, fill = build(be, specs, 8, g)
    yy, xx = divmod(int(d["dst_off"][1]), SD)
    want[yy:yy + 16, xx:xx + 16] = fill
    r = d["ref"]
    edits = {"p_width 0": ("p_width", 0), "p_width 129": ("p_width", 129), "p_height 0": ("p_height", 0), "p_height 200": ("p_height", 200), "subsampling_x 2": ("subsampling_x", 2),
             "subsampling_y 2": ("subsampling_y", 2), "compound 3": ("compound", 3)}
    if what in edits:
        d[edits[what][0]][1] = edits[what][1]
    elif what == "width 0":
        r["width"][1, 0] = 0
    elif what == "height -1":
        r["height"][1, 0] = -1
    elif what == "stride 0":
        r["stride"][1, 0] = 0
    elif what == "plane 32":
        r["plane"][1, 0] = 32
    elif what == "NULL plane":
        r["plane"][1, 0] = 6
    elif what == "second width 0":
        r["width"][1, 1] = 0
    elif what == "second NULL plane":
        r["plane"][1, 1] = 31
    elif what == "alpha beta shear":  # 4 * 8192 + 7 * 4736 = 65920
        r["alpha"][1, 0], r["beta"][1, 0] = 8192, -4736
    elif what == "gamma delta shear":  # 4 * (8192 + 8192) = 65536: the first value that is not allowed
        r["gamma"][1, 0], r["delta"][1, 0] = -8192, 8192
    elif what == "second shear":
        r["alpha"][1, 1] = 16384
    elif what == "dst_x overflow":  # mat[0] alone is in range; with mat[2] * src_x the sum leaves int32_t
        r["mat"][1, 0] = [(1 << 31) - 70000, 0, 65536, 0, 0, 65536]
    elif what == "dst_y overflow":
        r["mat"][1, 0] = [0, -(1 << 31) + 100, 65536, 0, 0, 65536]
        d["p_row"][1] = -40
    elif what == "last tile overflows":  # the first tile fits, the tile 8 columns further does not
        r["mat"][1, 0] = [(1 << 31) - 65536 * (10 + 4) - 65536 * 4, 0, 65536, 0, 0, 65536]
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    rr, keep = launch(be, A, B, d, dst, 8)
    assert rr == -1
    assert np.all(be.host(dst) == fill)
    status = be.dev(np.full(3, 7, np.uint8))
    rr, keep = launch(be, A, B, d, dst, 8, status)
    assert rr == 0
    assert be.host(status).tolist() == [0, 1, 0]
    assert np.array_equal(be.host(dst), want)


def test_bad_arguments(be):
    g = rng(8)
    A, B, d, want, fill = build(be, [spec(8, 8, (3, 5), "affine")], 8, g)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    for bd in (0, 9, 11, 16):
        assert launch(be, A, B, d, dst, bd)[0] == -1
    planes = be.pkg.InterPredPlanes()
    dd = be.dev(d)
    L = be.lib
    assert L.svt_hip_warp_pred_batch(planes, None, be.ptr(dd), 1, 8, None, be.stream) == -1
    assert L.svt_hip_warp_pred_batch(planes, be.ptr(dst), None, 1, 8, None, be.stream) == -1
    assert L.svt_hip_warp_pred_batch(planes, None, None, 0, 8, None, be.stream) == 0  # nothing to do
    assert L.svt_hip_warp_model_batch(None, 1, be.ptr(dst), None, be.stream) == -1 and L.svt_hip_warp_model_batch(be.ptr(dd), 1, None, None, be.stream) == -1
    assert L.svt_hip_warp_error_batch(planes, None, 1, be.ptr(dst), None, be.stream) == -1 and L.svt_hip_warp_error_batch(planes, be.ptr(dd), 1, None, None, be.stream) == -1
    assert L.svt_hip_warp_model_batch(None, 0, None, None, be.stream) == 0 and L.svt_hip_warp_error_batch(planes, None, 0, None, None, be.stream) == 0
    assert np.all(be.host(dst) == fill)


# ---- the model fit ----------------------------------------------------------------------------------------------------------------------------------------
def model_descs(be, sets):
    d = np.zeros(len(sets), be.pkg.WarpModelDesc)
    for i, s in enumerate(sets):
        d["pts"][i], d["pts_inref"][i], d["np"][i], d["mi_row"][i], d["mi_col"][i] = s["pts"], s["pts_inref"], s["np"], s["mi_row"], s["mi_col"]
        d["mv_row"][i], d["mv_col"][i], d["bsize"][i] = s["mv_row"], s["mv_col"], s["bsize"]
    return d


def model_rows(results):
    """invalid, wmmat[6], alpha .. delta per set, as the golden file stores them"""
    return np.array([[1] + [0] * 10 if r is None else [0] + list(r[0]) + list(r[1]) for r in results], np.int64)


def run_models(be, sets, with_status=False):
    d = model_descs(be, sets)
    dd, out = be.dev(d), be.dev(np.full(len(sets) * be.pkg.WarpModel.itemsize, 0xA5, np.uint8))
    status = be.dev(np.full(len(sets), 7, np.uint8)) if with_status else None
    assert be.lib.svt_hip_warp_model_batch(be.ptr(dd), len(sets), be.ptr(out), None if status is None else be.ptr(status), be.stream) == 0
    got = be.host(out).view(be.pkg.WarpModel)
    if with_status:
        assert not be.host(status).any()
    assert not got["pad"].any()
    return np.concatenate([got["invalid"][:, None].astype(np.int64), got["wmmat"].astype(np.int64),
                           np.stack([got[k] for k in ("alpha", "beta", "gamma", "delta")], 1).astype(np.int64)], 1)


_models = {}


def want_models(key, make):
    if key not in _models:
        sets = make()
        _models[key] = (sets, model_rows([wc.find_projection(s["np"], s["pts"], s["pts_inref"], s["bsize"], s["mv_row"], s["mv_col"], s["mi_row"], s["mi_col"]) for s in sets]))
    return _models[key]


def test_model_golden_sets(be):
    sets = wc.golden_model_sets()
    got = run_models(be, sets)
    assert np.array_equal(got, wc.load_golden()["model"])
    assert 0 < int(got[:, 0].sum()) < len(sets)  # both outcomes occur


@pytest.mark.parametrize("n", (1, 63, 65, 4096))
def test_model_batch_against_the_restatement(be, n):
    """wave boundaries and a large launch; random, rejected (det == 0), single-sample, far (the translation clamp binds) and wrapped sets -- the last with int32_t
    sums that wrap, where negative determinants and shift < 0 occur (asserted on the restatement's trace for the large launch)"""
    def make():
        g = rng(600 + n)
        kinds = ["random", "random", "wrapped", "single", "far", "random", "rejected", "wrapped"]
        return [wc.model_sample_set(g, kinds[i % 8]) for i in range(n)]
    sets, want = want_models(n, make)
    if n == 4096:
        neg = clamped = 0
        for s in sets[:1024]:
            tr = {}
            wc.find_projection(s["np"], s["pts"], s["pts_inref"], s["bsize"], s["mv_row"], s["mv_col"], s["mi_row"], s["mi_col"], tr)
            neg += tr["det"] < 0
            clamped += bool(tr.get("trans_clamped"))
        assert neg > 20 and clamped > 20, (neg, clamped)
        assert 100 < int(want[:, 0].sum()) < n - 100
    got = run_models(be, sets, with_status=n == 65)
    bad = np.argwhere((got != want).any(1))
    assert bad.size == 0, (n, bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]], sets[bad[0, 0]])


@pytest.mark.parametrize("what", ["np 0", "np 9", "np -1", "bsize 22", "bsize 255"])
def test_model_invalid_descriptors(be, what):
    g = rng(12)
    sets = [wc.model_sample_set(g) for _ in range(3)]
    d = model_descs(be, sets)
    field, v = what.split()
    d[field][1] = int(v)
    dd, out = be.dev(d), be.dev(np.full(3 * be.pkg.WarpModel.itemsize, 0xA5, np.uint8))
    assert be.lib.svt_hip_warp_model_batch(be.ptr(dd), 3, be.ptr(out), None, be.stream) == -1
    assert np.all(be.host(out) == 0xA5)
    status = be.dev(np.full(3, 7, np.uint8))
    assert be.lib.svt_hip_warp_model_batch(be.ptr(dd), 3, be.ptr(out), be.ptr(status), be.stream) == 0
    assert be.host(status).tolist() == [0, 1, 0]
    got = be.host(out).view(be.pkg.WarpModel)
    assert np.all(got[1:2].view(np.uint8) == 0xA5)
    for i in (0, 2):
        s = sets[i]
        r = wc.find_projection(s["np"], s["pts"], s["pts_inref"], s["bsize"], s["mv_row"], s["mv_col"], s["mi_row"], s["mi_col"])
        assert int(got["invalid"][i]) == int(r is None)
        if r is not None:
            assert got["wmmat"][i].tolist() == r[0] and (int(got["alpha"][i]), int(got["beta"][i]), int(got["gamma"][i]), int(got["delta"][i])) == tuple(r[1])


# ---- the warp error ---------------------------------------------------------------------------------------------------------------------------------------
def error_desc(d, i, name, geo_pic, geo_src, pc, pr, pw, ph, ss, chess):
    mat, sh = MODELS[name]
    r = d["ref"]
    r["ref_off"][i], r["mat"][i], r["width"][i], r["height"][i], r["stride"][i], r["plane"][i] = geo_pic[3], mat, geo_pic[0], geo_pic[1], geo_pic[2], 4
    r["alpha"][i], r["beta"][i], r["gamma"][i], r["delta"][i] = sh
    d["src_off"][i], d["src_stride"][i], d["src_plane"][i] = geo_src[3], geo_src[2], 9
    d["p_col"][i], d["p_row"][i], d["p_width"][i], d["p_height"][i], d["subsampling_x"][i], d["subsampling_y"][i], d["chess_refn"][i] = pc, pr, pw, ph, ss, ss, chess


_errors = {}


@pytest.mark.parametrize("n", (1, 3, 8))
@pytest.mark.parametrize("ss", (0, 1))
@pytest.mark.parametrize("chess", (0, 1))
def test_warp_error_batch(be, chess, ss, n):
    """a 100 x 70 picture (no multiple of 32 or of 8), 1 / 3 / 8 candidates in one launch; with three or more, the second candidate appears twice and must give equal
    sums; the last candidate of the eight covers a 20 x 12 picture, smaller than one error block"""
    key = (chess, ss, n)
    geo_pic, geo_src = (100, 70, 103, 5), (100, 70, 109, 13)
    if key not in _errors:
        g = rng(700 + 10 * chess + ss)
        pic, src = wc.make_picture(g, "random", *geo_pic[:3], 8), wc.make_picture(g, "random", *geo_src[:3], 8)
        names = [NAMES[(k + chess + 2 * ss) % 7] for k in range(n)]
        if n >= 3:
            names[2] = names[1]
        dims = [(100, 70)] * n
        if n == 8:
            dims[7] = (20, 12)
        want = [wc.warp_error(pic, *MODELS[nm], 100, 70, src, 0, 0, pw, ph, ss, ss, chess) for nm, (pw, ph) in zip(names, dims)]
        _errors[key] = (pic, src, names, dims, want)
    pic, src, names, dims, want = _errors[key]
    d = np.zeros(n, be.pkg.WarpErrorDesc)
    for i, (nm, (pw, ph)) in enumerate(zip(names, dims)):
        error_desc(d, i, nm, geo_pic, geo_src, 0, 0, pw, ph, ss, chess)
    planes = be.pkg.InterPredPlanes()
    dp, ds, dd, out = be.dev(flat_plane(pic, 100, 5)), be.dev(flat_plane(src, 100, 13)), be.dev(d), be.dev(np.full(n, 0xDEADBEEF, np.uint64))
    planes.base[4], planes.base[9] = be.ptr(dp), be.ptr(ds)
    status = be.dev(np.full(n, 7, np.uint8)) if n == 3 else None
    assert be.lib.svt_hip_warp_error_batch(planes, be.ptr(dd), n, be.ptr(out), None if status is None else be.ptr(status), be.stream) == 0
    got = be.host(out).tolist()
    assert got == want, (chess, ss, n)
    assert all(v > 0 or (chess and dm == (20, 12)) for v, dm in zip(got, dims)) and (not chess or all(v % 2 == 0 for v in got))  # (one block row, chess: jstart is past it)
    if n >= 3:
        assert got[1] == got[2]
    if status is not None:
        assert not be.host(status).any()


def test_warp_error_golden_and_invalid(be):
    gold = wc.load_golden()
    cases = wc.golden_error_cases()
    pic, src = gold["pic_8_0"], gold["pic_8_1"]
    geo = (wc.GOLDEN_W, wc.GOLDEN_H, wc.GOLDEN_STRIDE, 0)
    d = np.zeros(len(cases), be.pkg.WarpErrorDesc)
    for i, (name, w, h, pc, pr, pw, ph, ss, chess) in enumerate(cases):
        error_desc(d, i, name, geo, geo, pc, pr, pw, ph, ss, chess)
    planes = be.pkg.InterPredPlanes()
    dp, ds, dd, out = be.dev(pic), be.dev(src), be.dev(d), be.dev(np.zeros(len(cases), np.uint64))
    planes.base[4], planes.base[9] = be.ptr(dp), be.ptr(ds)
    assert be.lib.svt_hip_warp_error_batch(planes, be.ptr(dd), len(cases), be.ptr(out), None, be.stream) == 0
    assert np.array_equal(be.host(out).astype(np.int64), gold["error"])
    for field, v in (("p_width", 0), ("p_height", 70000), ("chess_refn", 2), ("subsampling_x", 2), ("src_plane", 10), ("src_stride", 0)):
        bad = d.copy()
        bad[field][1] = v
        db, o2 = be.dev(bad), be.dev(np.full(len(cases), 0xDEADBEEF, np.uint64))
        assert be.lib.svt_hip_warp_error_batch(planes, be.ptr(db), len(cases), be.ptr(o2), None, be.stream) == -1
        assert np.all(be.host(o2) == 0xDEADBEEF)
        if field not in ("p_height", "src_plane"):  # (the launch with a status array: two kinds are enough, the check is the same function)
            continue
        status = be.dev(np.full(len(cases), 7, np.uint8))
        assert be.lib.svt_hip_warp_error_batch(planes, be.ptr(db), len(cases), be.ptr(o2), be.ptr(status), be.stream) == 0
        assert be.host(status).tolist() == [0, 1] + [0] * (len(cases) - 2)
        want = gold["error"].copy()
        want[1] = 0
        assert np.array_equal(be.host(o2).astype(np.int64), want), field


# ---- the single-call forms --------------------------------------------------------------------------------------------------------------------------------
def conv_params(be, r0, r1, is_compound=0, do_average=0, jnt=0, fwd=0, bck=0, dst=None, dst_stride=0):
    cp = be.pkg.ConvolveParams()
    cp.round_0, cp.round_1, cp.is_compound, cp.do_average, cp.use_jnt_comp_avg, cp.fwd_offset, cp.bck_offset = r0, r1, is_compound, do_average, jnt, fwd, bck
    cp.dst, cp.dst_stride = (dst.ctypes.data if dst is not None else None), dst_stride
    return cp


def call_form(be, pic, width, height, mat, sh, pred, pc, pr, pw, ph, ss, bd, cp, planes=None):
    """pic: the 2-D picture (uint8, or uint16 to be split into the reference's 8-bit + 2-bit planes); planes: ready-made (address8, stride8, address2, stride2)"""
    m = np.array(mat, np.int32)
    if bd == 8:
        addr, stride = (pic.ctypes.data, pic.shape[1]) if planes is None else planes[:2]
        be.lib.svt_av1_warp_affine_hip(p(m), addr, width, height, stride, p(pred), pc, pr, pw, ph, pred.shape[1], ss[0], ss[1], C.byref(cp), *sh)
        return None
    if planes is None:
        r8, r2 = (pic >> 2).astype(np.uint8), np.ascontiguousarray((((pic & 3) << 6) | 0x2A).astype(np.uint8)[:, :width + 1])  # (low bits set: only the top two count)
        planes = (r8.ctypes.data, r8.shape[1], r2.ctypes.data, r2.shape[1])
        keep = (r8, r2)
    be.lib.svt_av1_highbd_warp_affine_hip(p(m), planes[0], planes[2], width, height, planes[1], planes[3], p(pred), pc, pr, pw, ph, pred.shape[1], ss[0], ss[1], bd, C.byref(cp), *sh)
    return None


def test_per_call_forms(be):
    """both forms, every combination of is_compound / do_average / use_jnt_comp_avg, default and other roundings, sizes with a cropped last tile, positions inside, on
    the border and outside; nothing outside p_width x p_height written; the high-bit-depth form on split planes of different strides"""
    g = rng(16)
    k = 0
    for bd in (8, 10, 12):
        dt, fill = (np.uint16, 0xA5A5) if bd > 8 else (np.uint8, 0xA5)
        pic = wc.make_picture(g, "random", 72, 56, 77, min(bd, 10))
        for (pw, ph) in ((8, 8), (16, 16), (12, 20), (1, 1), (64, 8)):
            for pos in ((16, 16), (-5, 21), (67, 50), (-120, 300)):
                k += 1
                name, ss = NAMES[k % len(NAMES)], SUBS[k % 4]
                mat, sh = MODELS[name]
                for mode in ("single", "first", "average", "jnt"):
                    comp = mode != "single"
                    r0, r1 = wc.conv_rounds(bd, comp) if k % 3 else ((4, 6) if comp else (4, 10))
                    cb = g.integers(0, 1 << 16, (ph + 1, pw + 5)).astype(np.uint16)
                    cb0 = cb.copy()
                    pred = np.full((ph + 2, pw + 3), fill, dt)
                    cp = conv_params(be, r0, r1, int(comp), int(mode in ("average", "jnt")), int(mode == "jnt"), 11, 5, cb, cb.shape[1])
                    call_form(be, pic, 72, 56, mat, sh, pred, pos[0], pos[1], pw, ph, ss, bd, cp)
                    want = wc.warp_affine(pic, mat, sh, 72, 56, pos[0], pos[1], pw, ph, ss[0], ss[1], bd, r0, r1, comp, mode in ("average", "jnt"), mode == "jnt", 11, 5,
                                          cb0[:ph, :pw], bd > 8)
                    tag = (bd, pw, ph, pos, name, ss, mode, r0, r1)
                    if mode == "first":  # the ConvBufType block is written, pred is not
                        assert np.array_equal(cb[:ph, :pw], want) and np.all(pred == fill), tag
                        cb[:ph, :pw] = cb0[:ph, :pw]
                        assert np.array_equal(cb, cb0), tag
                    else:
                        assert np.array_equal(pred[:ph, :pw], want), tag
                        pred[:ph, :pw] = fill
                        assert np.all(pred == fill) and np.array_equal(cb, cb0), tag
    # outside the accepted range: nothing is written
    pred, m, sh = np.full((8, 8), 0xA5, np.uint8), [0, 0, 65536, 0, 0, 65536], (0, 0, 0, 0)
    pic = wc.make_picture(g, "random", 72, 56, 77, 8)
    for args in (dict(pw=0), dict(pw=129), dict(ss=(2, 0)), dict(sh=(16384, 0, 0, 0)), dict(r=(8, 6)), dict(r=(3, 12)), dict(width=0), dict(m=[(1 << 31) - 1, 0, 65536, 0, 0, 65536])):
        r = args.get("r", (3, 11))
        call_form(be, pic, args.get("width", 72), 56, args.get("m", m), args.get("sh", sh), pred, 0, 0, args.get("pw", 8), 8, args.get("ss", (0, 0)), 8, conv_params(be, *r))
        assert np.all(pred == 0xA5), args
    p16 = np.full((8, 8), 0xA5A5, np.uint16)
    call_form(be, pic.astype(np.uint16), 72, 56, m, sh, p16, 0, 0, 8, 8, (0, 0), 9, conv_params(be, 3, 11))  # not a bit depth of the form
    assert np.all(p16 == 0xA5A5)
    assert be.lib.svt_hip_debug_commit_violations() == 0


def _guarded(n_bytes):
    """a mapping whose neighbouring pages are inaccessible: (mmap, page size, readable length)"""
    page = mmap.PAGESIZE
    body = (n_bytes + page - 1) // page * page
    m = mmap.mmap(-1, body + 2 * page)
    base = C.addressof(C.c_char.from_buffer(m))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes, libc.mprotect.restype = [C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0
    return m, page, body


def _flush(n_items, dt, at_end):
    """n_items of dtype dt flush against the inaccessible page after (at_end) or before them: (mapping, array, address)"""
    dt = np.dtype(dt)
    m, page, body = _guarded(n_items * dt.itemsize)
    start = page + (body - n_items * dt.itemsize if at_end else 0)
    return m, np.frombuffer(m, dt, n_items, start), C.addressof(C.c_char.from_buffer(m)) + start


def test_read_guard_on_the_emulator():
    """CPU only.  The reference picture lies flush against inaccessible pages on either end -- exactly (height - 1) * stride + width samples -- for the batched kernel
    (planes given by address) and for both single-call forms (which read the caller's memory on the host): a read outside width x height leaves the mapping.  Models
    and positions that project inside, across every border and tens of thousands of samples outside"""
    be = _backends.setdefault("emu", EmuBackend())
    g = rng(77)
    w, h, stride = 40, 24, 43
    n = (h - 1) * stride + w
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        pic = wc.make_picture(g, "random", w, h, stride, bd)
        body = pic.reshape(-1)[:n]
        for at_end in (True, False):
            mp, arr, addr = _flush(n, dt, at_end)
            arr[:] = body
            items = [((16, 16), pos, NAMES[k % len(NAMES)], SUBS[k % 4]) for k, pos in enumerate([(8, 4), (-6, -6), (30, 14), (-5, 14), (33, -4), (-300, 10), (10, 400), (-30000, 14000)])]
            items += [((128, 128), (-40, -50), "rotation", (0, 0)), ((12, 20), (36, 18), "beta_limit", (0, 0))]
            d = np.zeros(len(items), be.pkg.WarpDesc)
            off, wants = 0, []
            for i, ((pw, ph), pos, name, ss) in enumerate(items):
                mat, sh = MODELS[name]
                fill_ref(d["ref"], i, 0, 0, mat, sh, w, h, stride, 1)
                d["dst_off"][i], d["dst_stride"][i], d["p_col"][i], d["p_row"][i], d["p_width"][i], d["p_height"][i] = off, pw, pos[0], pos[1], pw, ph
                d["subsampling_x"][i], d["subsampling_y"][i] = ss
                wants.append(wc.warp_pred([(pic, mat, sh, w, h)], pos[0], pos[1], pw, ph, ss[0], ss[1], bd))
                off += pw * ph
            planes = be.pkg.InterPredPlanes()
            planes.base[1] = addr
            dst = np.zeros(off, dt)
            assert be.lib.svt_hip_warp_pred_batch(planes, p(dst), p(d), len(items), bd, None, None) == 0
            for i, ((pw, ph), pos, name, ss) in enumerate(items):
                o = int(d["dst_off"][i])
                assert np.array_equal(dst[o:o + pw * ph].reshape(ph, pw), wants[i]), (bd, at_end, i)
            if bd == 8:  # the warp error reads the same picture through the same tile routine; its source lies flush too
                ms, sarr, saddr = _flush(n, np.uint8, at_end)
                sarr[:] = g.integers(0, 256, n)
                src2d = np.zeros((h, stride), np.uint8)
                src2d.reshape(-1)[:n] = sarr
                e = np.zeros(2, be.pkg.WarpErrorDesc)
                for i, name in enumerate(("affine", "rotation")):
                    error_desc(e, i, name, (w, h, stride, 0), (w, h, stride, 0), 0, 0, w, h, 0, i)
                planes.base[4], planes.base[9] = addr, saddr
                out = np.zeros(2, np.uint64)
                assert be.lib.svt_hip_warp_error_batch(planes, p(e), 2, p(out), None, None) == 0
                assert out.tolist() == [wc.warp_error(pic, *MODELS[nm], w, h, src2d, 0, 0, w, h, 0, 0, i) for i, nm in enumerate(("affine", "rotation"))]
                del sarr, ms
            # the single-call forms: 8 bit on the mapping itself; high bit depth on an 8-bit and a 2-bit plane, each in a mapping of its own
            if bd == 8:
                pl = (addr, stride)
                keep = None
            else:
                m8, a8, addr8 = _flush(n, np.uint8, at_end)
                m2, a2, addr2 = _flush(n, np.uint8, at_end)
                a8[:], a2[:] = body >> 2, (body & 3) << 6
                pl, keep = (addr8, stride, addr2, stride), (m8, a8, m2, a2)
            for i, ((pw, ph), pos, name, ss) in enumerate(items):
                mat, sh = MODELS[name]
                r0, r1 = wc.conv_rounds(bd, False)
                pred = np.zeros((ph, pw), dt)
                call_form(be, None, w, h, mat, sh, pred, pos[0], pos[1], pw, ph, ss, bd, conv_params(be, r0, r1), pl)
                assert np.array_equal(pred, wants[i]), (bd, at_end, i, "form")
                x_lo, x_hi, y_lo, y_hi = wc.read_rect(mat, w, h, pos[0], pos[1], pw, ph, *ss)
                assert 0 <= x_lo <= x_hi < w and 0 <= y_lo <= y_hi < h
            del arr, mp, keep
