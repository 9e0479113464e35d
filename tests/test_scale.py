"""Pictures of another size (csrc/scale.hip): svt_hip_inter_pred_scaled_batch, svt_hip_resize_plane_batch, svt_hip_superres_upscale_batch and their single-call forms,
every output against tests/scale_common.py (numpy; pinned on the reference's C by tests/test_scale_ref.py) and against tests/golden/scale.npz (what the reference's C
computed).  Sources have odd strides and lead-ins, every destination is filled with 0xA5 beforehand and the WHOLE destination is compared, so a sample written outside
a block or plane fails like a wrong sample inside it.  Equality is exact everywhere."""
import ctypes as C

import numpy as np
import pytest

import scale_common as sc
from conftest import rng

SD = 547
PLANE_A, PLANE_B = 5, 30
PIC_A, PIC_B = (270, 268, 277, 11), (266, 270, 281, 7)  # width, height, stride, lead-in
BIT_DEPTHS = (8, 10, 12)


def dtype_of(bd):
    return np.uint16 if bd > 8 else np.uint8


def fill_of(bd):
    return 0xA5A5 if bd > 8 else 0xA5


def flat_plane(pic2d, lead):
    return np.concatenate([np.full(lead, 7, pic2d.dtype), pic2d.reshape(-1)])


def build(be, specs, bd, g, kind="random"):
    """the two reference pictures, descriptors and the expected destination plane of one launch"""
    dt = dtype_of(bd)
    A = sc.make_picture(g, kind, *PIC_A[:3], bd)
    B = sc.make_picture(g, kind, *PIC_B[:3], bd)
    x = y = shelf = 0
    pos = []
    for s in specs:
        gap = 1 + int(g.integers(0, 7))
        if x + gap + s["w"] > SD - 8:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + s["w"], max(shelf, s["h"])
    want = np.full((y + shelf + 2, SD), fill_of(bd), dt)
    d = np.zeros(len(specs), be.pkg.ScaledPredDesc)
    for i, (s, (dx, dy)) in enumerate(zip(specs, pos)):
        refs = []
        for k, r in enumerate(s["refs"][:2 if s["comp"] else 1]):
            pic, geo, plane = ((A, PIC_A, PLANE_A), (B, PIC_B, PLANE_B))[(i + k) % 2]
            l, rgt, t, bot = sc.ref_extent(s["w"], s["h"], r)
            ox, oy = l + int(g.integers(0, geo[0] - l - rgt)), t + int(g.integers(0, geo[1] - t - bot))
            d["src_off"][i, k], d["src_stride"][i, k], d["plane"][i, k] = geo[3] + oy * geo[2] + ox, geo[2], plane
            d["xs"][i, k], d["ys"][i, k], d["subpel_x"][i, k], d["subpel_y"][i, k] = r
            refs.append((pic, oy, ox, r[2], r[3], r[0], r[1]))
        d["dst_off"][i], d["dst_stride"][i], d["w"][i], d["h"][i], d["filter_x"][i], d["filter_y"][i] = dy * SD + dx, SD, s["w"], s["h"], s["fx"], s["fy"]
        d["compound"][i], d["fwd_offset"][i], d["bck_offset"][i] = s["comp"], s["wts"][0], s["wts"][1]
        want[dy:dy + s["h"], dx:dx + s["w"]] = sc.scaled_pred(refs, s["w"], s["h"], s["fx"], s["fy"], bd, s["comp"], *s["wts"])
    return A, B, d, want


def launch(be, A, B, d, dst, bd, status=None, entry="svt_hip_inter_pred_scaled_batch"):
    planes = be.pkg.InterPredPlanes()
    dA, dB, dd = be.dev(flat_plane(A, PIC_A[3])), be.dev(flat_plane(B, PIC_B[3])), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    r = getattr(be.lib, entry)(planes, be.ptr(dst), be.ptr(dd), len(d), bd, None if status is None else be.ptr(status), be.stream)
    be.sync()
    return r, (dA, dB, dd)


_built = {}  # the restatement's side of a launch, computed once and shared by the backends


def run(be, key, make_specs, bd, seed, kind="random", with_status=False):
    if key not in _built:
        specs = make_specs()
        _built[key] = build(be, specs, bd, rng(seed), kind) + (specs,)
    A, B, d, want, specs = _built[key]
    dst = be.dev(np.full(want.shape, fill_of(bd), want.dtype))
    status = be.dev(np.full(len(specs), 7, np.uint8)) if with_status else None
    r, keep = launch(be, A, B, d, dst, bd, status)
    assert r == 0
    got = be.host(dst).reshape(want.shape)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        for i, s in enumerate(specs):
            yy, xx = divmod(int(d["dst_off"][i]), SD)
            a, b = got[yy:yy + s["h"], xx:xx + s["w"]], want[yy:yy + s["h"], xx:xx + s["w"]]
            assert np.array_equal(a, b), (bd, i, s, np.argwhere(a != b)[:4], a[:2, :8], b[:2, :8])
        raise AssertionError("samples outside every block were written: %s" % (np.argwhere(got != want)[:8],))


# ---- A. scaled prediction ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.CLASSES)
@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_pred_sizes_steps_phases_filters_compound(be, bd, kind):
    """the case list at each bit depth on random, all-maximum and 0 / maximum alternating pictures"""
    run(be, ("cases", bd, kind), lambda: sc.pred_case_list(bd), bd, 100 + bd, kind, with_status=bd == 10)


def test_pred_case_list_covers_the_issue():
    """the list holds what it is meant to hold: every size at every step pair, the four phase kinds, every filter with both 4-tap swaps, compound 0 / 1 / 2 with the
    four weight pairs, two scaled references with different steps, scaled + unscaled either way round, all unscaled, and the block at the im_block bound"""
    specs = sc.pred_case_list(8)
    assert {(s["w"], s["h"], r[:2]) for s in specs for r in s["refs"][:2 if s["comp"] else 1]} >= {(w, h, st) for (w, h) in sc.PRED_SIZES for st in sc.PRED_STEPS}
    seen = {(s["w"], s["h"]) for s in specs}
    assert seen >= set(sc.PRED_SIZES) | {(128, 128)}
    steps = {r[:2] for s in specs for r in s["refs"]}
    assert steps >= set(sc.PRED_STEPS) | {(1024, 1024)}
    phases = {p for s in specs for r in s["refs"] for p in r[2:]}
    assert {0, 1023, 512} <= phases and len(phases) > 20
    assert {(s["fx"], s["fy"]) for s in specs} == {(a, b) for a in range(4) for b in range(4)}
    assert {(s["comp"], s["wts"]) for s in specs if s["comp"] == 2} == {(2, w) for w in sc.WEIGHTS}
    scaled = lambda r: r[:2] != (1024, 1024)
    comp = [s for s in specs if s["comp"]]
    assert any(scaled(s["refs"][0]) and scaled(s["refs"][1]) and s["refs"][0][:2] != s["refs"][1][:2] for s in comp)
    assert any(scaled(s["refs"][0]) and not scaled(s["refs"][1]) for s in comp) and any(not scaled(s["refs"][0]) and scaled(s["refs"][1]) for s in comp)
    assert any(not scaled(s["refs"][0]) and not scaled(s["refs"][1]) for s in comp) and any(not s["comp"] and not scaled(s["refs"][0]) for s in specs)
    big = [s for s in specs if s["w"] == 128][0]
    assert (((big["h"] - 1) * big["refs"][0][1] + big["refs"][0][3]) >> 10) + 8 == 262


@pytest.mark.parametrize("n", (1, 300))
def test_pred_launch_sizes(be, n):
    """one block, and a few hundred mixed blocks in permuted order"""
    def make():
        g = rng(n)
        pool = sc.pred_case_list(8)[:-1]
        return [pool[int(i)] for i in g.permutation(len(pool))[:n]] if n <= len(pool) else [pool[int(g.integers(len(pool)))] for _ in range(n)]
    run(be, ("launch", n), make, 8, 400 + n, with_status=n == 300)


@pytest.mark.parametrize("bd", (8, 10))
def test_pred_all_unscaled_equals_inter_pred_batch(be, bd):
    """descriptors whose references are all unscaled: the same destination plane as svt_hip_inter_pred_batch on the same blocks"""
    key = ("unscaled", bd)
    if key not in _built:
        specs = [s for s in sc.pred_case_list(bd) if all(r[:2] == (1024, 1024) for r in s["refs"][:2 if s["comp"] else 1])]
        assert len(specs) >= 32
        _built[key] = build(be, specs, bd, rng(31 + bd)) + (specs,)
    A, B, d, want, specs = _built[key]
    e = np.zeros(len(d), be.pkg.InterPredDesc)
    for f in ("src_off", "dst_off", "src_stride", "dst_stride", "plane", "w", "h", "filter_x", "filter_y", "compound", "fwd_offset", "bck_offset"):
        e[f] = d[f]
    e["subpel_x"], e["subpel_y"] = d["subpel_x"] >> 6, d["subpel_y"] >> 6
    outs = []
    for entry, descs in (("svt_hip_inter_pred_scaled_batch", d), ("svt_hip_inter_pred_batch", e)):
        dst = be.dev(np.full(want.shape, fill_of(bd), want.dtype))
        r, keep = launch(be, A, B, descs, dst, bd, entry=entry)
        assert r == 0
        outs.append(be.host(dst).reshape(want.shape))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_pred_readable_extent_ends_with_the_allocation(be, bd):
    """each scaled source is its own allocation of exactly the documented extent: columns -3 .. (((w - 1) * xs + subpel_x) >> 10) + 4, rows likewise, the last row
    ending on the allocation's last sample"""
    g = rng(900 + bd)
    cases = [(2, 2, (2048, 2048, 1023, 1023)), (4, 16, (1150, 1820, 1, 1022)), (16, 4, (64, 64, 0, 0)), (8, 32, (768, 1798, 512, 512)), (64, 8, (1024, 2048, 1023, 0)),
             (32, 64, (2048, 1024, 0, 1023)), (128, 128, (2048, 2048, 1023, 1023)), (32, 64, (1365, 512, 700, 300))]
    dt = dtype_of(bd)
    planes = be.pkg.InterPredPlanes()
    d = np.zeros(len(cases), be.pkg.ScaledPredDesc)
    keep, off = [], 0
    want = np.full(sum(w * h for w, h, _ in cases) + 16, fill_of(bd), dt)
    for i, (w, h, r) in enumerate(cases):
        ex, ey = sc.scaled_extent(w, h, r[2], r[3], r[0], r[1])
        pic = sc.make_picture(g, "random", ex + 4, ey + 4, ex + 4, bd)
        keep.append(be.dev(pic.reshape(-1)))
        planes.base[i] = be.ptr(keep[-1])
        d["src_off"][i, 0], d["src_stride"][i, 0], d["plane"][i, 0] = 3 * (ex + 4) + 3, ex + 4, i
        d["xs"][i, 0], d["ys"][i, 0], d["subpel_x"][i, 0], d["subpel_y"][i, 0] = r
        d["dst_off"][i], d["dst_stride"][i], d["w"][i], d["h"][i], d["filter_x"][i], d["filter_y"][i] = off, w, w, h, i % 4, (i + 1) % 4
        want[off:off + w * h] = sc.scaled_pred([(pic, 3, 3, r[2], r[3], r[0], r[1])], w, h, i % 4, (i + 1) % 4, bd).reshape(-1)
        off += w * h
    dst, dd = be.dev(np.full(want.shape, fill_of(bd), dt)), be.dev(d)
    assert be.lib.svt_hip_inter_pred_scaled_batch(planes, be.ptr(dst), be.ptr(dd), len(cases), bd, None, be.stream) == 0
    assert np.array_equal(be.host(dst), want)


INVALID = ["xs 63", "xs 2049", "ys 63", "ys 2049", "subpel_x 1024", "subpel_y 1024", "unscaled remainder x", "unscaled remainder y", "w 3", "h 0", "filter_x 4",
           "compound 3", "bound overflow", "plane 32", "NULL plane", "second xs 2049", "second remainder", "second NULL plane"]


def _invalidate(d, i, what):
    if what.startswith("second"):
        d["compound"][i] = 1
        d["src_off"][i, 1], d["src_stride"][i, 1], d["plane"][i, 1] = d["src_off"][i, 0], d["src_stride"][i, 0], d["plane"][i, 0]
        d["xs"][i, 1], d["ys"][i, 1] = 1150, 1150
    if what in ("xs 63", "xs 2049", "ys 63", "ys 2049", "subpel_x 1024", "subpel_y 1024"):
        d[what.split()[0]][i, 0] = int(what.split()[1])
    elif what in ("w 3", "h 0", "filter_x 4", "compound 3"):
        d[what.split()[0]][i] = int(what.split()[1])
    elif what.startswith("unscaled remainder"):
        d["xs"][i, 0] = d["ys"][i, 0] = 1024
        d["subpel_x"][i, 0], d["subpel_y"][i, 0] = (65, 128) if what.endswith("x") else (128, 63)
    elif what == "bound overflow":  # 128 rows at a step that needs 269 rows of im_block (such a step is outside 64 .. 2048 as well: within it the bound holds)
        d["h"][i], d["ys"][i, 0], d["subpel_y"][i, 0] = 128, 2100, 1023
    elif what == "plane 32":
        d["plane"][i, 0] = 32
    elif what == "NULL plane":
        d["plane"][i, 0] = 9
    elif what == "second xs 2049":
        d["xs"][i, 1] = 2049
    elif what == "second remainder":
        d["xs"][i, 1] = d["ys"][i, 1] = 1024
        d["subpel_x"][i, 1] = 1
    elif what == "second NULL plane":
        d["plane"][i, 1] = 9
    else:
        raise AssertionError(what)


def test_pred_invalid_descriptors(be):
    """every kind of invalid descriptor between valid ones.  status != NULL: flagged, skipped, the valid blocks written; status == NULL: -1 and nothing written.
    (The im_block bound of the header cannot be exceeded by a descriptor whose sizes and steps are valid -- 2 * 128 + 6 rows at most -- so its case also has a step
    outside the range.)"""
    key = "invalid"
    if key not in _built:
        specs = [sc.pred_spec(16, 16, [(1150, 1820, 300 + i, 900 - i)], i % 4, i % 3) for i in range(2 * len(INVALID) + 1)]
        A, B, d, want = build(be, specs, 8, rng(77))
        for j, what in enumerate(INVALID):
            i = 2 * j + 1
            _invalidate(d, i, what)
            yy, xx = divmod(int(d["dst_off"][i]), SD)
            want[yy:yy + 16, xx:xx + 16] = 0xA5
        _built[key] = (A, B, d, want)
    A, B, d, want = _built[key]
    dst, status = be.dev(np.full(want.shape, 0xA5, np.uint8)), be.dev(np.full(len(d), 7, np.uint8))
    r, keep = launch(be, A, B, d, dst, 8, status)
    assert r == 0
    assert np.array_equal(be.host(status), (np.arange(len(d)) & 1).astype(np.uint8))
    assert np.array_equal(be.host(dst).reshape(want.shape), want)
    for j in range(len(INVALID)):  # each alone between two valid ones, without a status array
        dst = be.dev(np.full(want.shape, 0xA5, np.uint8))
        r, keep = launch(be, A, B, d[2 * j:2 * j + 3], dst, 8)
        assert r == -1, INVALID[j]
        assert (be.host(dst) == 0xA5).all(), INVALID[j]
    dst = be.dev(np.full(want.shape, 0xA5, np.uint8))
    r, keep = launch(be, A, B, d[::2], dst, 8)  # the valid ones alone
    assert r == 0
    planes = be.pkg.InterPredPlanes()
    assert be.lib.svt_hip_inter_pred_scaled_batch(planes, be.ptr(dst), be.ptr(keep[2]), 1, 9, None, be.stream) == -1  # bit depth
    assert be.lib.svt_hip_inter_pred_scaled_batch(planes, None, be.ptr(keep[2]), 1, 8, None, be.stream) == -1
    assert be.lib.svt_hip_inter_pred_scaled_batch(planes, be.ptr(dst), None, 0, 8, None, be.stream) == 0


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_pred_single_call_forms(be, bd):
    """svt_av1_convolve_2d_scale_hip / svt_av1_highbd_convolve_2d_scale_hip from host memory: the caller's taps and roundings, every conv_params mode; do_average == 0
    writes the ConvBufType buffer and leaves dst untouched"""
    g = rng(600 + bd)
    dt = dtype_of(bd)
    pic = sc.make_picture(g, "random", 150, 150, 157, bd)
    fn = be.lib.svt_av1_highbd_convolve_2d_scale_hip if bd > 8 else be.lib.svt_av1_convolve_2d_scale_hip
    for (w, h, r, fx, fy, is_comp, avg, dist, wi, rounds) in sc.FORM_CASES:
        xs, ys, sx, sy = r
        r0, r1 = sc.form_rounds(bd, is_comp, rounds)
        if bd == 12 and rounds is not None:
            r0, r1 = r0 + 2, r1 - 2  # bd + FILTER_BITS - round_0 + 2 <= 16, as get_conv_params_no_round keeps it
        ex, ey = sc.scaled_extent(w, h, sx, sy, xs, ys)
        oy, ox = 3 + int(g.integers(0, 150 - 3 - ey)), 3 + int(g.integers(0, 150 - 3 - ex))
        px, fxa = sc.filter_params(sc.filter_rows(fx, w))
        py, fya = sc.filter_params(sc.filter_rows(fy, h))
        cb = g.integers(0, 1 << (bd + 3), (h, w + 5)).astype(np.uint16)
        fwd, bck = sc.WEIGHTS[wi]
        want_dst, want_cb = sc.scale_form(pic, oy, ox, w, h, fxa.astype(np.int64), fya.astype(np.int64), sx, xs, sy, ys, bd, r0, r1, is_comp, avg, dist, fwd, bck, cb[:, :w])
        cb0 = cb.copy()
        dst = np.full((h + 2, w + 9), fill_of(bd), dt)
        cp = sc.ConvolveParams(0, avg, cb.ctypes.data, w + 5, r0, r1, 0, is_comp, 0, fwd, bck, dist)
        args = [pic.ctypes.data + (oy * 157 + ox) * pic.itemsize, 157, dst.ctypes.data, w + 9, w, h, C.addressof(px), C.addressof(py), sx, xs, sy, ys, C.addressof(cp)]
        fn(*(args + ([bd] if bd > 8 else [])))
        exp = np.full(dst.shape, fill_of(bd), dt)
        if want_dst is not None:
            exp[:h, :w] = want_dst
            assert np.array_equal(cb, cb0)
        else:
            cb0[:, :w] = want_cb
            assert np.array_equal(cb, cb0), (w, h, r)
        assert np.array_equal(dst, exp), (w, h, r, is_comp, avg, dist)
    # outside the accepted range nothing is written
    dst = np.full((18, 25), fill_of(bd), dt)
    cp = sc.ConvolveParams(0, 0, None, 0, 3, 11, 0, 0, 0, 0, 0, 0)
    px, fxa = sc.filter_params(sc.filter_rows(0, 16))
    for bad in (dict(w=3), dict(xs=2049), dict(sy=1024), dict(ys=63)):
        a = dict(w=16, h=16, sx=5, xs=1150, sy=5, ys=1150)
        a.update(bad)
        args = [pic.ctypes.data + (20 * 157 + 20) * pic.itemsize, 157, dst.ctypes.data, 25, a["w"], a["h"], C.addressof(px), C.addressof(px), a["sx"], a["xs"], a["sy"], a["ys"],
                C.addressof(cp)]
        fn(*(args + ([bd] if bd > 8 else [])))
        assert (dst == fill_of(bd)).all(), bad


# ---- B. resize --------------------------------------------------------------------------------------------------------------------------------------
def resize_planes(bd):
    """(width, height, width2, height2): every length pair along rows and along columns, the width-only form, and a plane larger than one workgroup's row"""
    planes = []
    for (a, b) in sc.RESIZE_PAIRS:
        planes.append((a, 9, b, 6))
        planes.append((10, a, 7, b))
    planes += [(64, 11, 57, 11), (66, 5, 32, 5), (16, 16, 16, 16), (300, 20, 263, 20), (523, 12, 300, 9)]
    return planes


def run_resize(be, planes, bd, kind, seed, one_call=True):
    g = rng(seed)
    dt, px = dtype_of(bd), 2 if bd > 8 else 1
    d = np.zeros(len(planes), be.pkg.ResizeDesc)
    srcs, dsts, wants, pics = [], [], [], []
    for i, (w, h, w2, h2) in enumerate(planes):
        stride, lead, ostride = w + 1 + 2 * (i % 3), 3 + i % 5, w2 + 3 + 2 * (i % 2)
        key = ("resize", bd, kind, seed, i)
        if key not in _built:
            pic = sc.make_picture(g, kind, w, h, stride, bd)
            _built[key] = (pic, sc.resize_plane(pic[:, :w], w2, h2, bd))
        pic, out = _built[key]
        want = np.full((h2 + 1, ostride), fill_of(bd), dt)
        want[:h2, :w2] = out
        srcs.append(be.dev(flat_plane(pic, lead)))
        dsts.append(be.dev(np.full(want.shape, fill_of(bd), dt)))
        wants.append(want)
        pics.append(pic)
        d["src"][i], d["dst"][i] = be.ptr(srcs[-1]) + lead * px, be.ptr(dsts[-1])
        d["width"][i], d["height"][i], d["in_stride"][i], d["width2"][i], d["height2"][i], d["out_stride"][i] = w, h, stride, w2, h2, ostride
    groups = [range(len(planes))] if one_call else [[i] for i in range(len(planes))]
    for grp in groups:
        dd = np.ascontiguousarray(d[list(grp)])
        need = be.lib.svt_hip_resize_workspace_bytes(dd.ctypes.data, len(dd), bd)
        assert need > 0 and need % 256 == 0
        ws = be.dev(np.full(need + 64, 0xA5, np.uint8))
        assert be.lib.svt_hip_resize_plane_batch(dd.ctypes.data, len(dd), bd, be.ptr(ws), need, be.stream) == 0
        be.sync()
        assert (be.host(ws)[need:] == 0xA5).all()
    for i, p_ in enumerate(planes):
        assert np.array_equal(be.host(dsts[i]).reshape(wants[i].shape), wants[i]), (bd, kind, i, p_)
        assert np.array_equal(be.host(srcs[i])[3 + i % 5:].reshape(pics[i].shape), pics[i])
    return d, srcs, dsts, wants


@pytest.mark.parametrize("kind", sc.CLASSES)
@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_resize_length_pairs(be, bd, kind):
    """every length pair of the list along rows and along columns (copy, one even step, one odd step, step + interpolate, two steps + interpolate, interpolate down
    and up, the short-input branches), width-only planes, all planes of the list in ONE call"""
    run_resize(be, resize_planes(bd), bd, kind, 200 + bd)


def test_resize_three_planes_and_workspace(be):
    """the three planes of a 4:2:0 picture in one call; a workspace one byte short, a NULL workspace and invalid descriptors return -1 with nothing written"""
    planes = [(130, 66, 115, 58), (65, 33, 58, 29), (65, 33, 58, 29)]
    d, srcs, dsts, wants = run_resize(be, planes, 8, "random", 55)
    need = be.lib.svt_hip_resize_workspace_bytes(d.ctypes.data, 3, 8)
    fresh = [be.dev(np.full(w.shape, 0xA5, np.uint8)) for w in wants]
    for i in range(3):
        d["dst"][i] = be.ptr(fresh[i])
    ws = be.dev(np.full(need, 0xA5, np.uint8))
    assert be.lib.svt_hip_resize_plane_batch(d.ctypes.data, 3, 8, be.ptr(ws), need - 1, be.stream) == -1
    assert be.lib.svt_hip_resize_plane_batch(d.ctypes.data, 3, 8, None, need, be.stream) == -1
    assert be.lib.svt_hip_resize_plane_batch(d.ctypes.data, 3, 9, be.ptr(ws), need, be.stream) == -1
    for field, v in (("width2", 0), ("height", -1), ("in_stride", 64), ("out_stride", 57), ("src", 0)):
        e = d.copy()
        e[field][1] = v
        assert be.lib.svt_hip_resize_plane_batch(e.ctypes.data, 3, 8, be.ptr(ws), need, be.stream) == -1, field
        assert be.lib.svt_hip_resize_workspace_bytes(e.ctypes.data, 3, 8) == 0
    be.sync()
    assert (be.host(ws) == 0xA5).all() and all((be.host(f) == 0xA5).all() for f in fresh)
    assert be.lib.svt_hip_resize_plane_batch(d.ctypes.data, 0, 8, None, 0, be.stream) == 0


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_resize_single_call_forms(be, bd):
    """svt_av1_resize_plane_hip / svt_av1_highbd_resize_plane_hip from host memory on two sizes"""
    g = rng(300 + bd)
    dt = dtype_of(bd)
    for (w, h, w2, h2) in ((66, 40, 32, 23), (37, 50, 37, 25)):
        pic = sc.make_picture(g, "random", w, h, w + 3, bd)
        out = np.full((h2 + 1, w2 + 5), fill_of(bd), dt)
        want = out.copy()
        want[:h2, :w2] = sc.resize_plane(pic[:, :w], w2, h2, bd)
        args = [pic.ctypes.data, h, w, w + 3, out.ctypes.data, h2, w2, w2 + 5]
        r = be.lib.svt_av1_highbd_resize_plane_hip(*(args + [bd])) if bd > 8 else be.lib.svt_av1_resize_plane_hip(*args)
        assert r == 0
        assert np.array_equal(out, want), (bd, w, h, w2, h2)
    bad = [pic.ctypes.data, h, w, w - 1, out.ctypes.data, h2, w2, w2 + 5]
    r = be.lib.svt_av1_highbd_resize_plane_hip(*(bad + [bd])) if bd > 8 else be.lib.svt_av1_resize_plane_hip(*bad)
    assert r == C.c_int32(0x80001005).value and np.array_equal(out, want)  # EB_ErrorBadParameter, nothing written


# ---- C. upscale -------------------------------------------------------------------------------------------------------------------------------------
UPSCALE_FORMATS = ((8, 1), (8, 2), (10, 2), (12, 2))  # bd, sample_bytes
UPSCALE_PICTURES = ((64, 1), (200, 1), (384, 3), (201, 1), (333, 2))  # up-scaled luma width, tile columns


def upscale_descs(be, up_luma, ntiles, denom, bd, sb, kind, g, rows=6):
    """the three planes (Y and two sub-sampled chroma planes) of one picture: descriptors, device buffers, sources and expected destinations"""
    dt = np.uint16 if sb == 2 else np.uint8
    fill = 0xA5A5 if sb == 2 else 0xA5
    d = np.zeros(3, be.pkg.UpscaleDesc)
    out = []
    for i, sub_x in enumerate((0, 1, 1)):
        down, up, starts, mi_cols, _ = sc.upscale_geometry(up_luma, denom, sub_x, ntiles)
        last = starts[-1] << (2 - sub_x)
        sstride, dstride, lead = last + 2 * i, up + 1 + 2 * i, 5 + i
        src = sc.make_picture(g, kind, last, rows, sstride, bd).astype(dt)
        want = np.full((rows + 1, dstride), fill, dt)
        want[:rows, :up] = sc.upscale_rows(src[:, :last], down, up, denom, sub_x, starts, bd)
        out.append((src, lead, want))
        d["src_stride"][i], d["dst_stride"][i], d["rows"][i], d["downscaled_plane_width"][i], d["upscaled_plane_width"][i] = sstride, dstride, rows, down, up
        d["superres_denom"][i], d["sub_x"][i], d["bd"][i], d["sample_bytes"][i], d["n_tile_cols"][i] = denom, sub_x, bd, sb, len(starts) - 1
        d["tile_col_start_mi"][i, :len(starts)] = starts
    return d, out


@pytest.mark.parametrize("fmt", UPSCALE_FORMATS)
@pytest.mark.parametrize("denom", sc.UPSCALE_DENOMS)
def test_upscale_widths_tiles_denominators(be, denom, fmt):
    """luma widths 64 and 200 with one tile column, 384 with three and 333 with two (interior edges, both frame edges, the x0_qn carry), an odd luma width; the luma
    and both chroma planes of a picture in ONE call; src unchanged, dst guarded"""
    bd, sb = fmt
    fill = 0xA5A5 if sb == 2 else 0xA5
    for (up_luma, ntiles) in UPSCALE_PICTURES:
        for kind in sc.CLASSES:
            key = ("upscale", up_luma, ntiles, denom, fmt, kind)
            if key not in _built:
                _built[key] = upscale_descs(be, up_luma, ntiles, denom, bd, sb, kind, rng(denom * 1000 + up_luma + bd + sb))
            d, out = _built[key]
            d = d.copy()
            srcs = [be.dev(flat_plane(src, lead)) for (src, lead, want) in out]
            dsts = [be.dev(np.full(want.shape, fill, want.dtype)) for (src, lead, want) in out]
            for i in range(3):
                d["src"][i], d["dst"][i] = be.ptr(srcs[i]) + out[i][1] * sb, be.ptr(dsts[i])
            assert be.lib.svt_hip_superres_upscale_batch(d.ctypes.data, 3, be.stream) == 0
            be.sync()
            for i, (src, lead, want) in enumerate(out):
                assert np.array_equal(be.host(dsts[i]).reshape(want.shape), want), (up_luma, ntiles, denom, fmt, kind, i)
                assert np.array_equal(be.host(srcs[i])[lead:].reshape(src.shape), src)


def test_upscale_invalid_descriptors_and_host_form(be):
    d, out = upscale_descs(be, 200, 1, 14, 8, 1, "random", rng(5))
    srcs = [be.dev(flat_plane(src, lead)) for (src, lead, want) in out]
    dsts = [be.dev(np.full(want.shape, 0xA5, want.dtype)) for (src, lead, want) in out]
    for i in range(3):
        d["src"][i], d["dst"][i] = be.ptr(srcs[i]) + out[i][1], be.ptr(dsts[i])
    for field, v in (("superres_denom", 17), ("superres_denom", 7), ("sub_x", 2), ("bd", 9), ("sample_bytes", 3), ("n_tile_cols", 0), ("n_tile_cols", 65), ("rows", 0),
                     ("dst_stride", 10), ("src_stride", 8), ("upscaled_plane_width", 3), ("dst", 0)):
        e = d.copy()
        e[field][2] = v
        assert be.lib.svt_hip_superres_upscale_batch(e.ctypes.data, 3, be.stream) == -1, (field, v)
    e = d.copy()
    e["dst"][0] = e["src"][0]  # overlapping
    assert be.lib.svt_hip_superres_upscale_batch(e.ctypes.data, 3, be.stream) == -1
    be.sync()
    assert all((be.host(t) == 0xA5).all() for t in dsts)
    assert be.lib.svt_hip_superres_upscale_batch(d.ctypes.data, 0, be.stream) == 0
    # the host form, on the luma plane and on a 10-bit chroma plane with three tile columns
    for (up_luma, ntiles, denom, bd, sb, plane) in ((200, 1, 14, 8, 1, 0), (384, 3, 9, 10, 2, 1)):
        d, out = upscale_descs(be, up_luma, ntiles, denom, bd, sb, "random", rng(6))
        src, lead, want = out[plane]
        got = np.full(want.shape, 0xA5A5 if sb == 2 else 0xA5, want.dtype)
        starts = np.ascontiguousarray(d["tile_col_start_mi"][plane], np.int32)
        r = be.lib.svt_hip_upscale_normative_rows_host(src.ctypes.data, src.shape[1], got.ctypes.data, got.shape[1], 6, int(d["downscaled_plane_width"][plane]),
                                                        int(d["upscaled_plane_width"][plane]), denom, int(d["sub_x"][plane]), ntiles, starts.ctypes.data, bd, sb)
        assert r == 0 and np.array_equal(got, want)


# ---- the golden file --------------------------------------------------------------------------------------------------------------------------------
def test_golden_cases(be):
    """tests/golden/scale.npz through the batched entries: the kernels == what the reference's C computed"""
    gold = sc.load_golden()
    assert int(gold["seed"][0]) == sc.GOLDEN_SEED
    for bd in BIT_DEPTHS:
        for k in (0, 1):
            assert np.array_equal(gold["pic_%d_%d" % (8 if bd == 8 else 12, k)] >> (2 if bd == 10 else 0), sc.golden_picture(bd, k))
    for bd in BIT_DEPTHS:
        dt = dtype_of(bd)
        idx = [i for i, c in enumerate(sc.GOLDEN_PRED) if c[0] == bd]
        d = np.zeros(len(idx), be.pkg.ScaledPredDesc)
        off = 0
        for j, i in enumerate(idx):
            _, w, h, fx, fy, comp, wi, refs = sc.GOLDEN_PRED[i]
            for k, r in enumerate(refs):
                d["src_off"][j, k], d["src_stride"][j, k], d["plane"][j, k] = 3 * sc.GOLDEN_W + 3, sc.GOLDEN_W, k
                d["xs"][j, k], d["ys"][j, k], d["subpel_x"][j, k], d["subpel_y"][j, k] = r
            d["dst_off"][j], d["dst_stride"][j], d["w"][j], d["h"][j], d["filter_x"][j], d["filter_y"][j] = off, w, w, h, fx, fy
            d["compound"][j], d["fwd_offset"][j], d["bck_offset"][j] = comp, sc.WEIGHTS[wi][0], sc.WEIGHTS[wi][1]
            off += w * h
        planes = be.pkg.InterPredPlanes()
        d0, d1, dd, dst = be.dev(sc.golden_picture(bd, 0)), be.dev(sc.golden_picture(bd, 1)), be.dev(d), be.dev(np.zeros(off, dt))
        planes.base[0], planes.base[1] = be.ptr(d0), be.ptr(d1)
        assert be.lib.svt_hip_inter_pred_scaled_batch(planes, be.ptr(dst), be.ptr(dd), len(idx), bd, None, be.stream) == 0
        got = be.host(dst)
        for j, i in enumerate(idx):
            w, h = sc.GOLDEN_PRED[i][1:3]
            o = int(d["dst_off"][j])
            assert np.array_equal(got[o:o + w * h].reshape(h, w), gold["pred_%d" % i]), (i, sc.GOLDEN_PRED[i])
        # resize
        idx = [i for i, c in enumerate(sc.GOLDEN_RESIZE) if c[0] == bd]
        d = np.zeros(len(idx), be.pkg.ResizeDesc)
        src = be.dev(sc.golden_picture(bd, 0))
        outs = [be.dev(np.zeros((sc.GOLDEN_RESIZE[i][4], sc.GOLDEN_RESIZE[i][3]), dt)) for i in idx]
        for j, i in enumerate(idx):
            _, w, h, w2, h2 = sc.GOLDEN_RESIZE[i]
            d["src"][j], d["dst"][j] = be.ptr(src), be.ptr(outs[j])
            d["width"][j], d["height"][j], d["in_stride"][j], d["width2"][j], d["height2"][j], d["out_stride"][j] = w, h, sc.GOLDEN_W, w2, h2, w2
        need = be.lib.svt_hip_resize_workspace_bytes(d.ctypes.data, len(d), bd)
        ws = be.dev(np.zeros(need, np.uint8))
        assert be.lib.svt_hip_resize_plane_batch(d.ctypes.data, len(d), bd, be.ptr(ws), need, be.stream) == 0
        for j, i in enumerate(idx):
            assert np.array_equal(be.host(outs[j]), gold["resize_%d" % i]), (i, sc.GOLDEN_RESIZE[i])
        # upscale
        for i, c in enumerate(sc.GOLDEN_UPSCALE):
            if c[0] != bd:
                continue
            srch, (down, up, starts, mi_cols, down_luma) = sc.golden_upscale_input(i)
            d = np.zeros(1, be.pkg.UpscaleDesc)
            s_, o_ = be.dev(srch), be.dev(np.zeros((6, up), srch.dtype))
            d["src"][0], d["dst"][0], d["src_stride"][0], d["dst_stride"][0], d["rows"][0] = be.ptr(s_), be.ptr(o_), srch.shape[1], up, 6
            d["downscaled_plane_width"][0], d["upscaled_plane_width"][0], d["superres_denom"][0], d["sub_x"][0], d["bd"][0] = down, up, c[3], c[4], bd
            d["sample_bytes"][0], d["n_tile_cols"][0] = c[1], len(starts) - 1
            d["tile_col_start_mi"][0, :len(starts)] = starts
            assert be.lib.svt_hip_superres_upscale_batch(d.ctypes.data, 1, be.stream) == 0
            assert np.array_equal(be.host(o_), gold["upscale_%d" % i]), (i, c)
