"""AV1 luma palette (csrc/palette.hip): svt_hip_kmeans_batch, svt_hip_count_colors_batch, svt_hip_palette_search_luma_batch, svt_hip_palette_cost_batch,
svt_hip_palette_pred_batch, svt_hip_palette_cache_y and the six single-call forms, every output against tests/palette_common.py (numpy; pinned on the reference's C by
tests/test_palette_ref.py) and against tests/golden/palette.npz (what the reference's C computed).  Every output buffer is filled with 0xA5 beforehand and compared
WHOLE, so a byte written outside an item's outputs fails like a wrong byte inside them.  Equality is exact everywhere."""
import numpy as np
import pytest

import palette_common as pc
from conftest import rng

_built = {}  # the restatement's side of a launch, computed once and shared by the backends


def once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


# ---- A. k-means -------------------------------------------------------------------------------------------------------------------------------------
def test_kmeans_case_list_covers_the_issue():
    cases = pc.kmeans_cases()
    assert {len(x) for x, _, _, _ in cases} >= set(pc.KMEANS_NS)
    assert {(x.shape[1], len(c)) for x, c, _, _ in cases} >= {(dim, k) for dim in (1, 2) for k in range(1, 9)}
    assert {int(x.max()) for x, _, _, _ in cases if int(x.min()) == 0} >= {255, 1023, 4095}
    assert any(a for _, _, _, a in cases) and any(m == 0 and not a for _, _, m, a in cases)
    assert all(m == 2 for x, _, m, _ in cases if len(x) == 16384)
    pc.COUNTERS.clear()
    for x, c, m, a in cases:
        if not a and len(x) <= 1000:
            pc.k_means(x, c, m)
    assert pc.COUNTERS["reseed_two_or_more"] and pc.COUNTERS["repeat_exit"] and pc.COUNTERS["max_itr_exit"] and not pc.COUNTERS["restore"]


def test_kmeans_batch(be):
    """every n, k, dim, value range, tie and exit of the case list, all items of different n in ONE launch; centroids and indices compared whole, gaps included"""
    L = once("kmeans", lambda: pc.kmeans_launch(be.pkg))
    data, cent, idx, dd = be.dev(L["data"]), be.dev(L["cent"]), be.dev(np.full(L["want_idx"].shape, 0xA5, np.uint8)), be.dev(L["descs"])
    status = be.dev(np.full(len(L["descs"]), 7, np.uint8))
    assert be.lib.svt_hip_kmeans_batch(be.ptr(data), be.ptr(cent), be.ptr(idx), be.ptr(dd), len(L["descs"]), be.ptr(status), be.stream) == 0
    be.sync()
    assert not be.host(status).any()
    got_c, got_i = be.host(cent), be.host(idx)
    if not (np.array_equal(got_c, L["want_cent"]) and np.array_equal(got_i, L["want_idx"])):
        for j, i in enumerate(L["order"]):
            x, c0, max_itr, assign_only = L["cases"][i]
            o, k = L["descs"][j], len(c0) * x.shape[1]
            a, b = got_c[int(o["centroids_off"]):int(o["centroids_off"]) + k], L["want_cent"][int(o["centroids_off"]):int(o["centroids_off"]) + k]
            assert np.array_equal(a, b), (i, x.shape, len(c0), max_itr, assign_only, a, b)
            a, b = got_i[int(o["indices_off"]):int(o["indices_off"]) + len(x)], L["want_idx"][int(o["indices_off"]):int(o["indices_off"]) + len(x)]
            assert np.array_equal(a, b), (i, x.shape, len(c0), max_itr, assign_only, np.argwhere(a != b)[:4])
        raise AssertionError("values outside every item were written")
    cent2, idx2 = be.dev(L["cent"]), be.dev(np.full(L["want_idx"].shape, 0xA5, np.uint8))  # without a status array
    assert be.lib.svt_hip_kmeans_batch(be.ptr(data), be.ptr(cent2), be.ptr(idx2), be.ptr(dd), len(L["descs"]), None, be.stream) == 0
    be.sync()
    assert np.array_equal(be.host(cent2), L["want_cent"]) and np.array_equal(be.host(idx2), L["want_idx"])


def test_kmeans_single_call_forms(be):
    """the four forms with the reference's prototypes, from host memory; outside the accepted range nothing is written"""
    g = rng(8)
    for dim in (1, 2):
        km, ci = getattr(be.lib, "svt_av1_k_means_dim%d_hip" % dim), getattr(be.lib, "svt_av1_calc_indices_dim%d_hip" % dim)
        for (n, k, max_itr) in ((300, 5, 50), (64, 8, 2), (4096, 3, 50)):
            x = np.ascontiguousarray(g.choice([3, 90, 91, 200, 1023], (n, dim)).astype(np.int32))
            c0 = np.ascontiguousarray(g.integers(0, 1024, (k, dim)).astype(np.int32))
            want_c, want_i = pc.k_means(x, c0, max_itr)
            c1, idx = c0.copy(), np.full(n + 3, 0xA5, np.uint8)
            km(x.ctypes.data, c1.ctypes.data, idx.ctypes.data, n, k, max_itr)
            assert np.array_equal(c1, want_c) and np.array_equal(idx[:n], want_i) and (idx[n:] == 0xA5).all(), (dim, n, k)
            idx = np.full(n + 3, 0xA5, np.uint8)
            ci(x.ctypes.data, c0.ctypes.data, idx.ctypes.data, n, k)
            assert np.array_equal(idx[:n], pc.calc_indices(x, c0)[0]) and (idx[n:] == 0xA5).all()
        for (n, k) in ((0, 3), (16385, 3), (10, 9), (10, 0)):
            idx, c1 = np.full(16, 0xA5, np.uint8), c0.copy()
            km(x.ctypes.data, c1.ctypes.data, idx.ctypes.data, n, k, 5)
            ci(x.ctypes.data, c1.ctypes.data, idx.ctypes.data, n, k)
            assert (idx == 0xA5).all() and np.array_equal(c1, c0)


# ---- B. colour count --------------------------------------------------------------------------------------------------------------------------------
COUNT_BLOCKS = ((8, 8), (16, 16), (4, 12), (64, 64), (1, 1), (33, 7), (128, 128))  # rows, cols


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_count_colors_batch(be, bd):
    """blocks at strides larger than cols behind an odd lead-in, values at 0 and at the maximum; the histograms lie in one buffer with guards between them"""
    def make():
        g = rng(20 + bd)
        dt, maxv = (np.uint16 if bd > 8 else np.uint8), (1 << bd) - 1
        d = np.zeros(len(COUNT_BLOCKS), be.pkg.CountColorsDesc)
        pieces, pos = [np.full(5, 1, dt)], 5
        hist = np.full(len(COUNT_BLOCKS) * ((1 << bd) + 3) + 2, -3, np.int32)
        ncol = np.zeros(len(COUNT_BLOCKS), np.int32)
        for i, (rows, cols) in enumerate(COUNT_BLOCKS):
            stride = cols + 1 + 2 * (i % 3)
            plane = g.integers(0, maxv + 1, (rows, stride)).astype(dt)
            vals = pc.pick_values(g, min(rows * cols, (3, 40, 200)[i % 3]), maxv)
            vals[0], vals[-1] = 0, maxv
            plane[:, :cols] = pc.screen_block(g, rows, cols, np.unique(vals))
            pieces.append(plane.reshape(-1))
            d["src_off"][i], d["src_stride"][i], d["rows"][i], d["cols"][i], d["hist_off"][i] = pos, stride, rows, cols, 2 + i * ((1 << bd) + 3)
            h, ncol[i] = pc.count_colors(plane[:, :cols], bd)
            hist[2 + i * ((1 << bd) + 3):][:1 << bd] = h
            pos += plane.size
        return np.concatenate(pieces), d, hist, ncol
    src, d, want_hist, want_n = once(("count", bd), make)
    ds, dd, dh, dn = be.dev(src), be.dev(d), be.dev(np.full(want_hist.shape, -3, np.int32)), be.dev(np.full(len(d), -1, np.int32))
    status = be.dev(np.full(len(d), 7, np.uint8))
    assert be.lib.svt_hip_count_colors_batch(be.ptr(ds), be.ptr(dd), len(d), bd, be.ptr(dh), be.ptr(dn), be.ptr(status), be.stream) == 0
    be.sync()
    assert np.array_equal(be.host(dn), want_n) and np.array_equal(be.host(dh), want_hist) and not be.host(status).any()
    if bd > 8:  # a sample at 1 << bd: not counted, zero colours, status 2; the neighbours are as before
        bad = src.copy()
        at = int(d["src_off"][1]) + 3 * int(d["src_stride"][1]) + 2
        want2 = want_hist.copy()
        want2[int(d["hist_off"][1]) + int(bad[at])] -= 1
        bad[at] = 1 << bd
        ds, dh, dn = be.dev(bad), be.dev(np.full(want_hist.shape, -3, np.int32)), be.dev(np.full(len(d), -1, np.int32))
        assert be.lib.svt_hip_count_colors_batch(be.ptr(ds), be.ptr(dd), len(d), bd, be.ptr(dh), be.ptr(dn), be.ptr(status), be.stream) == 0
        be.sync()
        exp_n = want_n.copy()
        exp_n[1] = 0
        assert np.array_equal(be.host(dn), exp_n) and np.array_equal(be.host(dh), want2)
        assert np.array_equal(be.host(status), np.array([0, 2] + [0] * (len(d) - 2), np.uint8))


def test_count_colors_single_call_forms(be):
    g = rng(9)
    for bd in (8, 10, 12):
        dt = np.uint16 if bd > 8 else np.uint8
        plane = np.ascontiguousarray(pc.screen_block(g, 20, 37, pc.pick_values(g, 30, (1 << bd) - 1)).astype(dt))
        hist = np.full((1 << bd) + 2, -3, np.int32)
        if bd == 8:
            n = be.lib.svt_av1_count_colors_hip(plane.ctypes.data + 2, 37, 19, 33, hist.ctypes.data)
        else:
            n = be.lib.svt_av1_count_colors_highbd_hip(plane.ctypes.data + 4, 37, 19, 33, bd, hist.ctypes.data)
        h, want = pc.count_colors(plane.reshape(-1)[2:2 + 19 * 37].reshape(19, 37)[:, :33], bd)
        assert n == want and np.array_equal(hist[:1 << bd], h) and (hist[1 << bd:] == -3).all()
    assert be.lib.svt_av1_count_colors_hip(plane.ctypes.data, 37, 0, 33, hist.ctypes.data) == 0 and (hist[1 << 12:] == -3).all()


# ---- C. search --------------------------------------------------------------------------------------------------------------------------------------
def test_search_case_list_covers_the_issue():
    for bd in (8, 10):
        cases = pc.search_cases(bd)
        assert len(cases) >= 40
        assert {(c["bw"], c["bh"], c["cols"], c["rows"]) for c in cases} >= set(pc.SEARCH_GEOMETRIES)
        assert {len(np.unique(c["block"])) for c in cases} >= set(pc.SEARCH_COLORS)
        assert {len(c["cache"]) for c in cases} >= {0, 1, 16} and {c["step"] for c in cases} == {1, 2, 3}
        near = {min(abs(int(v) - k) for v in np.unique(c["block"])) for c in cases for k in c["cache"][:1]}
        assert near >= {0, 1, 2}
        assert any(int(c["block"].min()) == 0 for c in cases) and any(int(c["block"].max()) == (1 << bd) - 1 for c in cases)


@pytest.mark.parametrize("bd", (8, 10))
def test_search_luma_batch(be, bd):
    """every block of the case list (eight geometries, colour counts 1 .. 65, caches, steps) in ONE launch in permuted order, the last block's samples ending with the
    source allocation; the output buffer compared whole against the restatement: counts, sizes, colours, maps, and 0xA5 everywhere else"""
    L = once(("search", bd), lambda: pc.search_launch(be.pkg, bd))
    src, dd = be.dev(L["src"]), be.dev(L["descs"])
    for with_status in (True, False):
        out, status = be.dev(np.full(L["want"].shape, 0xA5, np.uint8)), be.dev(np.full(len(L["descs"]), 7, np.uint8))
        r = be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(dd), len(L["descs"]), bd, be.ptr(out), be.ptr(status) if with_status else None, be.stream)
        be.sync()
        assert r == 0 and (not with_status or not be.host(status).any())
        got = be.host(out)
        if not np.array_equal(got, L["want"]):
            for j, i in enumerate(L["order"]):
                c, o = L["cases"][i], L["descs"][j]
                lo, hi = int(o["out_off"]), int(o["out_off"]) + pc.OUT_HEADER + pc.MAX_CANDS * int(o["map_stride"])
                a, b = got[lo:hi], L["want"][lo:hi]
                assert np.array_equal(a, b), (bd, i, c["note"], c["bw"], c["bh"], c["rows"], c["cols"], len(np.unique(c["block"])), c["cache"], c["step"], a[:16], b[:16],
                                              np.argwhere(a != b)[:6].reshape(-1))
            raise AssertionError("bytes outside every block's output were written: %s" % (np.argwhere(got != L["want"])[:8].reshape(-1),))


def test_search_sample_out_of_range(be):
    """16-bit form: a sample at 1024 gives zero candidates and status 2; nothing but the count is written"""
    L = once(("search", 10), lambda: pc.search_launch(be.pkg, 10))
    j = next(j for j, i in enumerate(L["order"]) if L["want"][int(L["descs"]["out_off"][j])] > 0)
    d = L["descs"][j:j + 1].copy()
    src = L["src"].copy()
    src[int(d["src_off"][0]) + int(d["src_stride"][0]) + 1] = 1024
    d["out_off"][0] = 2
    out, status = be.dev(np.full(pc.OUT_HEADER + 8, 0xA5, np.uint8)), be.dev(np.full(1, 7, np.uint8))
    ds, dd = be.dev(src), be.dev(d)
    assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(ds), be.ptr(dd), 1, 10, be.ptr(out), be.ptr(status), be.stream) == 0
    be.sync()
    want = np.full(pc.OUT_HEADER + 8, 0xA5, np.uint8)
    want[2] = 0
    assert np.array_equal(be.host(out), want) and be.host(status)[0] == 2


# ---- D. cost ----------------------------------------------------------------------------------------------------------------------------------------
def test_cost_batch(be):
    """every palette size with maps that reach all five contexts, rows / cols below the map, caches of 0 and 16, bit depths 8 / 10 / 12"""
    def make():
        table, seen = pc.rate_table(), set()
        maps = pc.context_maps()
        e = np.zeros(len(maps), be.pkg.PaletteCostDesc)
        buf, want = [np.full(2, 0xA5, np.uint8)], []
        for n, (cmap, size, rows, cols, colors, cache, bit_depth) in enumerate(maps):
            e["map_off"][n], e["colors_off"][n] = 2 + n * 272 + 16, 2 + n * 272
            e["rows"][n], e["cols"][n], e["block_width"][n], e["size"][n], e["n_cache"][n], e["bit_depth"][n] = rows, cols, 16, size, len(cache), bit_depth
            e["cache"][n, :len(cache)] = cache
            col8 = np.zeros(8, "<u2")
            col8[:size] = colors
            buf += [col8.view(np.uint8), cmap.reshape(-1)]
            want.append(pc.palette_costs(cmap, rows, cols, size, colors, cache, bit_depth, table, seen))
        assert seen == {0, 1, 2, 3, 4}
        assert {int(s) for s in e["size"]} == set(range(2, 9)) and {int(c) for c in e["n_cache"]} >= {0, 16}
        return np.concatenate(buf), e, np.array(want, np.int32), table
    buf, e, want, table = once("cost", make)
    db, de, dt, out = be.dev(buf), be.dev(e), be.dev(table), be.dev(np.full(want.size + 2, -5, np.int32))
    status = be.dev(np.full(len(e), 7, np.uint8))
    assert be.lib.svt_hip_palette_cost_batch(be.ptr(db), be.ptr(de), len(e), be.ptr(dt), be.ptr(out), be.ptr(status), be.stream) == 0
    be.sync()
    got = be.host(out)
    assert np.array_equal(got[:-2].reshape(-1, 3), want), np.argwhere(got[:-2].reshape(-1, 3) != want)[:6]
    assert (got[-2:] == -5).all() and not be.host(status).any()


@pytest.mark.parametrize("bd", (8, 10))
def test_cost_reads_the_search_output_in_place(be, bd):
    """the search, then one cost item per kept candidate pointing at its colours and map where the search left them"""
    L = once(("search", bd), lambda: pc.search_launch(be.pkg, bd))
    table = pc.rate_table(6)
    e, want = once(("cost_items", bd), lambda: pc.cost_items(be.pkg, L, bd, table))
    assert len(e) > 100
    src, dd, out = be.dev(L["src"]), be.dev(L["descs"]), be.dev(np.full(L["want"].shape, 0xA5, np.uint8))
    assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(dd), len(L["descs"]), bd, be.ptr(out), None, be.stream) == 0
    de, dt, bits = be.dev(e), be.dev(table), be.dev(np.full(3 * len(e), -5, np.int32))
    assert be.lib.svt_hip_palette_cost_batch(be.ptr(out), be.ptr(de), len(e), be.ptr(dt), be.ptr(bits), None, be.stream) == 0
    be.sync()
    assert np.array_equal(be.host(bits).reshape(-1, 3), want)
    assert np.array_equal(be.host(out), L["want"])  # the cost kernel wrote nothing there


# ---- E. prediction ----------------------------------------------------------------------------------------------------------------------------------
TX_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4), (8, 32), (32, 8),
            (16, 64), (64, 16)]  # tx_size_wide / tx_size_high of TX_4X4 .. TX_64X16


@pytest.mark.parametrize("form", ((0, 8), (1, 8), (1, 10)))
def test_pred_batch(be, form):
    """every transform size inside a 64 x 64 map at non-zero (x, y) wherever it fits, and inside smaller maps; 8-bit destination, 16-bit destination at bit depths 8 (a
    colour above 0xFF is clamped) and 10; the destination plane is guarded"""
    dst16, bd = form

    def make():
        g = rng(40 + 2 * dst16 + bd)
        dt, fill = (np.uint16, 0xA5A5) if dst16 else (np.uint8, 0xA5)
        colors = np.sort(g.choice(256 if not dst16 else 1024, 8, replace=False)).astype("<u2")
        if dst16:
            colors[-1] = 0x3FF  # above 0xFF: clamped at bit depth 8
        maps = {wpx: g.integers(0, 8, (64, wpx)).astype(np.uint8) for wpx in (64, 16, 8)}
        buf = np.concatenate([np.full(2, 0xA5, np.uint8), colors.view(np.uint8)] + [maps[w].reshape(-1) for w in (64, 16, 8)])
        moff = {64: 18, 16: 18 + 4096, 8: 18 + 4096 + 1024}
        specs = [(w, h, 64) for (w, h) in TX_SIZES] + [(w, h, 16) for (w, h) in TX_SIZES if w <= 16] + [(w, h, 8) for (w, h) in TX_SIZES if w <= 8]
        d = np.zeros(len(specs), be.pkg.PalettePredDesc)
        stride = 200
        want = np.full((len(specs) // 2 + 1) * 65 * stride, fill, dt).reshape(-1, stride)
        for i, (w, h, wpx) in enumerate(specs):
            x, y = (4 * int(g.integers(1, (wpx - w) // 4 + 1)) if w < wpx else 0), (int(g.integers(1, 64 - h + 1)) if h < 64 else 0)
            dy, dx = (i // 2) * 65, 3 + (i % 2) * 90
            d["map_off"][i], d["colors_off"][i], d["dst_off"][i], d["dst_stride"][i] = moff[wpx], 2, dy * stride + dx, stride
            d["w"][i], d["h"][i], d["x"][i], d["y"][i], d["wpx"][i] = w, h, x, y, wpx
            want[dy:dy + h, dx:dx + w] = pc.palette_pred(maps[wpx], colors, x, y, w, h, dst16, bd)
        assert {(int(a), int(b)) for a, b in zip(d["w"][d["wpx"] == 64], d["h"][d["wpx"] == 64])} == set(TX_SIZES) and (d["y"][d["h"] < 64] > 0).all() and (d["x"][d["w"] < d["wpx"]] > 0).all()
        assert not dst16 or bd != 8 or ((want == 0xFF).any() and not ((want > 0xFF) & (want != fill)).any())
        return buf, d, want
    buf, d, want = once(("pred", form), make)
    db, dd, dst, status = be.dev(buf), be.dev(d), be.dev(np.full(want.shape, want.flat[0], want.dtype)), be.dev(np.full(len(d), 7, np.uint8))
    for st in (status, None):
        assert be.lib.svt_hip_palette_pred_batch(be.ptr(db), be.ptr(dst), be.ptr(dd), len(d), dst16, bd, None if st is None else be.ptr(st), be.stream) == 0
        be.sync()
        assert np.array_equal(be.host(dst).reshape(want.shape), want) and not be.host(status).any()


# ---- F. host pieces, invalid descriptors, the golden file -------------------------------------------------------------------------------------------
def test_palette_cache_y(be):
    g = rng(3)
    cache = np.zeros(18, np.uint16)
    for trial in range(200):
        a = np.sort(g.choice(40, int(g.integers(0, 9)), replace=False)).astype(np.uint16)
        l = np.sort(g.choice(40, int(g.integers(0, 9)), replace=False)).astype(np.uint16)
        cache[:] = 0xA5A5
        n = be.lib.svt_hip_palette_cache_y(a.ctypes.data if len(a) else None, len(a), l.ctypes.data if len(l) else None, len(l), cache.ctypes.data)
        want = pc.palette_cache_y(a, l)
        assert n == len(want) <= 16 and list(cache[:n]) == want and (cache[n:] == 0xA5A5).all()
        assert want == sorted(set(a) | set(l))
    assert be.lib.svt_hip_palette_cache_y(a.ctypes.data, 9, l.ctypes.data, 0, cache.ctypes.data) == 0


def test_invalid_descriptors(be):
    """status != NULL: the invalid item is flagged 1 and skipped, its neighbours done; status == NULL: -1 and nothing written"""
    g = rng(12)
    # k-means: k 9, dim 3, n 0, n above 16384
    x, c0 = g.integers(0, 256, 40).astype(np.int32), g.integers(0, 256, 16).astype(np.int32)
    c0[8:12] = c0[:4]
    for field, v in (("k", 9), ("dim", 3), ("n", 0), ("n", 16385), ("k", 0)):
        d = np.zeros(3, be.pkg.KmeansDesc)
        for i in range(3):
            d["centroids_off"][i], d["indices_off"][i], d["n"][i], d["max_itr"][i], d["dim"][i], d["k"][i] = 4 * i, 10 * i, 10, 5, 1, 4
        d[field][1] = v
        dx, dd = be.dev(x), be.dev(d)
        cent, idx, status = be.dev(c0), be.dev(np.full(40, 0xA5, np.uint8)), be.dev(np.full(3, 7, np.uint8))
        assert be.lib.svt_hip_kmeans_batch(be.ptr(dx), be.ptr(cent), be.ptr(idx), be.ptr(dd), 3, be.ptr(status), be.stream) == 0
        be.sync()
        assert list(be.host(status)) == [0, 1, 0], (field, v)
        want_c, want_i = pc.k_means(x[:10], c0[:4], 5)
        gi, gc = be.host(idx), be.host(cent)
        assert np.array_equal(gi[:10], want_i) and np.array_equal(gi[20:30], want_i) and (gi[10:20] == 0xA5).all() and (gi[30:] == 0xA5).all()
        assert np.array_equal(gc[:4], want_c.reshape(-1)) and np.array_equal(gc[4:8], c0[4:8])
        cent, idx = be.dev(c0), be.dev(np.full(40, 0xA5, np.uint8))
        assert be.lib.svt_hip_kmeans_batch(be.ptr(dx), be.ptr(cent), be.ptr(idx), be.ptr(dd), 3, None, be.stream) == -1
        be.sync()
        assert (be.host(idx) == 0xA5).all() and np.array_equal(be.host(cent), c0)
    # search: block_width 128, rows above block_height, and the rest of the documented list
    L = once(("search", 8), lambda: pc.search_launch(be.pkg, 8))
    j = next(j for j, i in enumerate(L["order"]) if L["want"][int(L["descs"]["out_off"][j])] > 0 and L["cases"][i]["bw"] == 16)
    src = be.dev(L["src"])
    size = pc.OUT_HEADER + pc.MAX_CANDS * int(L["descs"]["map_stride"][j])
    for field, v in (("block_width", 128), ("rows", 17), ("cols", 17), ("block_height", 12), ("rows", 0), ("n_cache", 17), ("dominant_color_step", 0), ("map_stride", 255),
                     ("out_off", 1)):
        d = L["descs"][[j, j, j]].copy()
        d["out_off"] = [0, size, 2 * size]
        d[field][1] = v
        dd, out, status = be.dev(d), be.dev(np.full(3 * size + 2, 0xA5, np.uint8)), be.dev(np.full(3, 7, np.uint8))
        assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(dd), 3, 8, be.ptr(out), be.ptr(status), be.stream) == 0
        be.sync()
        got, lo = be.host(out), int(L["descs"]["out_off"][j])
        assert list(be.host(status)) == [0, 1, 0], (field, v)
        assert np.array_equal(got[:size], L["want"][lo:lo + size]) and np.array_equal(got[2 * size:3 * size], L["want"][lo:lo + size]) and (got[size:2 * size] == 0xA5).all()
        out = be.dev(np.full(3 * size + 2, 0xA5, np.uint8))
        assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(dd), 3, 8, be.ptr(out), None, be.stream) == -1, (field, v)
        be.sync()
        assert (be.host(out) == 0xA5).all()
    out = be.dev(np.full(8, 0xA5, np.uint8))
    assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(dd), 3, 12, be.ptr(out), None, be.stream) == -1  # bit depth
    assert be.lib.svt_hip_palette_search_luma_batch(None, be.ptr(dd), 3, 8, be.ptr(out), None, be.stream) == -1
    assert be.lib.svt_hip_palette_search_luma_batch(None, None, 0, 8, None, None, be.stream) == 0
    # count, cost, prediction: one invalid field each, status NULL
    d = np.zeros(1, be.pkg.CountColorsDesc)
    d["src_stride"], d["rows"], d["cols"] = 8, 0, 8
    dd, hist, ncol = be.dev(d), be.dev(np.full(256, -3, np.int32)), be.dev(np.full(1, -1, np.int32))
    assert be.lib.svt_hip_count_colors_batch(be.ptr(src), be.ptr(dd), 1, 8, be.ptr(hist), be.ptr(ncol), None, be.stream) == -1
    assert be.lib.svt_hip_count_colors_batch(be.ptr(src), be.ptr(dd), 1, 9, be.ptr(hist), be.ptr(ncol), None, be.stream) == -1
    table, bits = be.dev(pc.rate_table()), be.dev(np.full(3, -5, np.int32))
    for field, v in (("size", 1), ("size", 9), ("block_width", 12), ("cols", 17), ("rows", 65), ("n_cache", 17), ("bit_depth", 9), ("colors_off", 3)):
        e = np.zeros(1, be.pkg.PaletteCostDesc)
        e["map_off"], e["rows"], e["cols"], e["block_width"], e["size"], e["bit_depth"] = 16, 8, 8, 16, 4, 8
        e[field] = v
        de = be.dev(e)
        assert be.lib.svt_hip_palette_cost_batch(be.ptr(src), be.ptr(de), 1, be.ptr(table), be.ptr(bits), None, be.stream) == -1, (field, v)
    dst = be.dev(np.full(64 * 64, 0xA5, np.uint8))
    for field, v in (("w", 12), ("h", 2), ("wpx", 128), ("x", 60), ("y", 60), ("colors_off", 1)):
        p = np.zeros(1, be.pkg.PalettePredDesc)
        p["map_off"], p["dst_stride"], p["w"], p["h"], p["wpx"] = 16, 64, 8, 8, 64
        p[field] = v
        dp = be.dev(p)
        assert be.lib.svt_hip_palette_pred_batch(be.ptr(src), be.ptr(dst), be.ptr(dp), 1, 0, 8, None, be.stream) == -1, (field, v)
    assert be.lib.svt_hip_palette_pred_batch(be.ptr(src), be.ptr(dst), be.ptr(dp), 1, 0, 10, None, be.stream) == -1  # an 8-bit destination at bit depth 10
    be.sync()
    assert (be.host(hist) == -3).all() and (be.host(bits) == -5).all() and (be.host(dst) == 0xA5).all()


def test_golden_cases(be):
    """tests/golden/palette.npz through the batched entries: the kernels == what the reference's C computed on the same case lists"""
    gold = pc.load_golden()
    L = once("kmeans", lambda: pc.kmeans_launch(be.pkg))
    assert np.array_equal(gold["kmeans_data"], L["data"]) and np.array_equal(gold["kmeans_descs"], L["descs"].view(np.uint8))
    data, cent, idx, dd = be.dev(L["data"]), be.dev(L["cent"]), be.dev(np.full(L["want_idx"].shape, 0xA5, np.uint8)), be.dev(L["descs"])
    assert be.lib.svt_hip_kmeans_batch(be.ptr(data), be.ptr(cent), be.ptr(idx), be.ptr(dd), len(L["descs"]), None, be.stream) == 0
    be.sync()
    assert np.array_equal(be.host(cent), gold["kmeans_cent"]) and np.array_equal(be.host(idx), gold["kmeans_idx"])
    for bd in (8, 10):
        S = once(("search", bd), lambda: pc.search_launch(be.pkg, bd))
        assert np.array_equal(gold["search_src_%d" % bd], S["src"]) and np.array_equal(gold["search_descs_%d" % bd], S["descs"].view(np.uint8))
        src, sd, out = be.dev(S["src"]), be.dev(S["descs"]), be.dev(np.full(S["want"].shape, 0xA5, np.uint8))
        assert be.lib.svt_hip_palette_search_luma_batch(be.ptr(src), be.ptr(sd), len(S["descs"]), bd, be.ptr(out), None, be.stream) == 0
        e, _ = once(("cost_items", bd), lambda: pc.cost_items(be.pkg, S, bd, pc.rate_table(6)))
        de, dt, bits = be.dev(e), be.dev(pc.rate_table(6)), be.dev(np.full(3 * len(e), -5, np.int32))
        assert be.lib.svt_hip_palette_cost_batch(be.ptr(out), be.ptr(de), len(e), be.ptr(dt), be.ptr(bits), None, be.stream) == 0
        be.sync()
        assert np.array_equal(be.host(out), gold["search_out_%d" % bd])
        assert np.array_equal(be.host(bits).reshape(-1, 3), gold["cost_%d" % bd])
