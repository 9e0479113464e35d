"""tests/palette_common.py pinned on the reference (oracle/_ref/libsvtref.so: its `_c` functions called directly).  search_palette_luma, svt_av1_cost_color_map and
svt_get_palette_cache_y go through tests/palette_ref_harness.c, compiled at test time, which includes the reference's headers where they lie and fills the few fields
of the encoder's structures those functions read.  Every case of the lists tests/test_palette.py runs on the kernels is pinned here, and counters in the restatement
show that the lists reach the rare branches.  CPU only; runs where the reference's sources and the library exist, skipped elsewhere.
`SVT_PALETTE_WRITE_GOLDEN=1` rewrites tests/golden/palette.npz from the reference's outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import palette_common as pc
from conftest import REF_LIB, ROOT, load_pkg, rng

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "palette.c")), reason="the reference's sources are not on this machine")
INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals")]
vp = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory, ref):
    out = str(tmp_path_factory.mktemp("palette") / "libpalette_harness.so")
    cmd = ["gcc", "-O1", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *INC, os.path.join(ROOT, "tests", "palette_ref_harness.c"), "-o", out,
           "-L" + os.path.dirname(REF_LIB), "-lsvtref", "-Wl,-rpath," + os.path.dirname(REF_LIB)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    h = C.CDLL(out)
    h.harness_init()
    h.harness_search.restype, h.harness_search.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int,
                                                                   C.c_int, vp, vp, vp]
    h.harness_cost_map.restype, h.harness_cost_map.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    h.harness_cache.restype, h.harness_cache.argtypes = C.c_int, [vp, C.c_int, vp, C.c_int, vp]
    for dim in (1, 2):
        f = getattr(ref, "svt_av1_k_means_dim%d_c" % dim)
        f.restype, f.argtypes = None, [vp, vp, vp, C.c_int, C.c_int, C.c_int]
        f = getattr(ref, "svt_av1_calc_indices_dim%d_c" % dim)
        f.restype, f.argtypes = None, [vp, vp, vp, C.c_int, C.c_int]
    ref.svt_av1_count_colors.restype, ref.svt_av1_count_colors.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]
    ref.svt_av1_count_colors_highbd.restype, ref.svt_av1_count_colors_highbd.argtypes = C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    ref.svt_aom_get_palette_color_index_context_optimized.restype = C.c_int
    ref.svt_aom_get_palette_color_index_context_optimized.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    ref.svt_av1_palette_color_cost_y.restype, ref.svt_av1_palette_color_cost_y.argtypes = C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int]
    ref.svt_aom_write_uniform_cost.restype, ref.svt_aom_write_uniform_cost.argtypes = C.c_int, [C.c_int, C.c_int]
    h.ref = ref
    return h


# ---- the reference's C behind the signatures of the restatement ------------------------------------------------------------------------------------------
def c_k_means(h, x, c0, max_itr):
    x, c = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(c0, np.int32).copy()
    idx = np.zeros(len(x), np.uint8)
    getattr(h.ref, "svt_av1_k_means_dim%d_c" % x.shape[1])(x.ctypes.data, c.ctypes.data, idx.ctypes.data, len(x), len(c), max_itr)
    return c, idx


def c_calc_indices(h, x, c0):
    x, c = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(c0, np.int32)
    idx = np.zeros(len(x), np.uint8)
    getattr(h.ref, "svt_av1_calc_indices_dim%d_c" % x.shape[1])(x.ctypes.data, c.ctypes.data, idx.ctypes.data, len(x), len(c))
    return idx


def c_search(h, block, bw, bh, cache, step, bit_depth):
    """search_palette_luma on a block at (5, 3) of a picture with a stride of its own; the cache comes from above / left palettes that merge to it"""
    rows, cols = block.shape
    dt = np.uint16 if bit_depth > 8 else np.uint8
    pic = np.full((rows + 4, cols + 9), 1, dt)
    pic[3:3 + rows, 5:5 + cols] = block
    above, left = np.array(cache[0::2], np.uint16), np.array(cache[1::2], np.uint16)
    assert pc.palette_cache_y(above, left) == list(cache) and len(above) <= 8 and len(left) <= 8
    sizes, colors, maps = np.zeros(14, np.uint8), np.zeros((14, 8), np.uint16), np.zeros((14, bh, bw), np.uint8)
    n = h.harness_search(pic.ctypes.data, pic.shape[1], int(bit_depth > 8), 5, 3, bw, bh, rows, cols, above.ctypes.data, len(above), left.ctypes.data, len(left), step,
                         bit_depth, sizes.ctypes.data, colors.ctypes.data, maps.ctypes.data)
    return [(int(sizes[s]), colors[s, :sizes[s]].copy(), maps[s].copy()) for s in range(n)]


def c_costs(h, cmap, rows, cols, size, colors, cache, bit_depth, table, seen=None):
    cmap = np.ascontiguousarray(cmap)
    table = np.ascontiguousarray(table, np.int32)
    pmi = np.zeros(24, np.uint16)
    pmi[:size] = colors[:size]
    cc = np.zeros(16, np.uint16)
    cc[:len(cache)] = cache
    bw = cmap.shape[1]
    bh = max(8, 1 << int(rows - 1).bit_length()) if cmap.shape[0] not in (8, 16, 32, 64) else cmap.shape[0]
    return (h.harness_cost_map(cmap.ctypes.data, bw, bh, rows, cols, size, table.ctypes.data),
            h.ref.svt_av1_palette_color_cost_y(pmi.ctypes.data, cc.ctypes.data, size, len(cache), bit_depth), h.ref.svt_aom_write_uniform_cost(size, int(cmap[0, 0])))


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------------
def test_kmeans_and_calc_indices(harness):
    for (x, c0, max_itr, assign_only) in pc.kmeans_cases():
        if assign_only:
            assert np.array_equal(c_calc_indices(harness, x, c0), pc.calc_indices(x, c0)[0])
        else:
            got_c, got_i = c_k_means(harness, x, c0, max_itr)
            want_c, want_i = pc.k_means(x, c0, max_itr)
            assert np.array_equal(got_c, want_c) and np.array_equal(got_i, want_i), (x.shape, len(c0), max_itr)


def test_kmeans_random_runs_never_restore(harness):
    """a few hundred random runs against the C; the `this_dist > pre_dist` restore is never taken (DESIGN 4.26 says why it cannot be)"""
    g = rng(99)
    pc.COUNTERS.clear()
    for t in range(300):
        dim, k, n = 1 + t % 2, 1 + int(g.integers(0, 8)), int(g.integers(1, 400))
        vals = g.integers(0, 1024, int(g.integers(1, 12)))
        x, c0 = g.choice(vals, (n, dim)), g.integers(0, 1024, (k, dim))
        got_c, got_i = c_k_means(harness, x, c0, 50)
        want_c, want_i = pc.k_means(x, c0, 50)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_i, want_i), (t, n, k, dim)
    assert pc.COUNTERS["restore"] == 0 and pc.COUNTERS["reseed_two_or_more"] > 0


def test_count_colors(harness):
    g = rng(2)
    for bd in (8, 10, 12):
        dt = np.uint16 if bd > 8 else np.uint8
        for (rows, cols) in ((8, 8), (33, 7), (64, 64)):
            plane = np.ascontiguousarray(g.integers(0, 1 << bd, (rows, cols + 5)).astype(dt))
            hist = np.full(1 << bd, -1, np.int32)
            if bd == 8:
                n = harness.ref.svt_av1_count_colors(plane.ctypes.data, cols + 5, rows, cols, hist.ctypes.data)
            else:
                n = harness.ref.svt_av1_count_colors_highbd(plane.ctypes.data, cols + 5, rows, cols, bd, hist.ctypes.data)
            want_h, want_n = pc.count_colors(plane[:, :cols], bd)
            assert n == want_n and np.array_equal(hist, want_h)
    # (a sample at 1 << bit_depth: the C asserts, and returns 0 where asserts are compiled out -- a caller error; the kernels report status 2 and zero colours)


def test_color_index_context(harness):
    g = rng(3)
    idx = C.c_int(0)
    seen = set()
    for size in range(2, 9):
        cmap = np.ascontiguousarray(g.integers(0, size, (12, 16)).astype(np.uint8))
        cmap[::2] = np.repeat(cmap[::2, ::4], 4, axis=1)
        for r in range(12):
            for c in range(16):
                if r or c:
                    ctx = harness.ref.svt_aom_get_palette_color_index_context_optimized(cmap.ctypes.data, 16, r, c, C.addressof(idx))
                    assert (ctx, idx.value) == pc.color_index_context(cmap, r, c), (size, r, c)
                    seen.add(ctx)
    assert seen == {0, 1, 2, 3, 4}


def test_cache_merge(harness):
    g = rng(4)
    cache = np.zeros(16, np.uint16)
    for t in range(300):
        a = np.sort(g.choice(30, int(g.integers(0, 9)), replace=False)).astype(np.uint16)
        l = np.sort(g.choice(30, int(g.integers(0, 9)), replace=False)).astype(np.uint16)
        n = harness.harness_cache(a.ctypes.data, len(a), l.ctypes.data, len(l), cache.ctypes.data)
        assert list(cache[:n]) == pc.palette_cache_y(a, l)


def test_costs(harness):
    table = pc.rate_table()
    for (cmap, size, rows, cols, colors, cache, bit_depth) in pc.context_maps():
        assert c_costs(harness, cmap, rows, cols, size, colors, cache, bit_depth, table) == pc.palette_costs(cmap, rows, cols, size, colors, cache, bit_depth, table)


_launches = {}


def launches(harness):
    """the launches of tests/test_palette.py twice: expected outputs from the restatement and from the reference's C"""
    if not _launches:
        pkg = load_pkg()
        pc.COUNTERS.clear()
        _launches["kmeans"] = (pc.kmeans_launch(pkg), pc.kmeans_launch(pkg, lambda x, c, m: c_k_means(harness, x, c, m), lambda x, c: c_calc_indices(harness, x, c)))
        for bd in (8, 10):
            ours = pc.search_launch(pkg, bd)
            theirs = pc.search_launch(pkg, bd, lambda *a: c_search(harness, *a))
            table = pc.rate_table(6)
            _launches[bd] = (ours, theirs, pc.cost_items(pkg, ours, bd, table), pc.cost_items(pkg, theirs, bd, table, lambda *a: c_costs(harness, *a)))
        _launches["counters"] = dict(pc.COUNTERS)
    return _launches


def test_search_and_cost_on_every_case_of_the_gpu_test(harness):
    L = launches(harness)
    ours, theirs = L["kmeans"]
    assert np.array_equal(ours["want_cent"], theirs["want_cent"]) and np.array_equal(ours["want_idx"], theirs["want_idx"])
    for bd in (8, 10):
        ours, theirs, (e0, cost0), (e1, cost1) = L[bd]
        assert np.array_equal(ours["src"], theirs["src"]) and np.array_equal(ours["descs"], theirs["descs"])
        if not np.array_equal(ours["want"], theirs["want"]):
            for j, i in enumerate(ours["order"]):
                c, o = ours["cases"][i], ours["descs"][j]
                lo, hi = int(o["out_off"]), int(o["out_off"]) + pc.OUT_HEADER + pc.MAX_CANDS * int(o["map_stride"])
                a, b = ours["want"][lo:hi], theirs["want"][lo:hi]
                assert np.array_equal(a, b), (bd, i, c["note"], c["bw"], c["bh"], c["rows"], c["cols"], c["cache"], c["step"], a[:16], b[:16], np.argwhere(a != b)[:6].reshape(-1))
        assert np.array_equal(e0, e1) and np.array_equal(cost0, cost1) and len(e0) > 100


def test_case_lists_reach_the_rare_branches(harness):
    n = launches(harness)["counters"]
    for what in ("reseed_two_or_more", "repeat_exit", "max_itr_exit", "duplicates_removed", "shrunk_to_two_or_fewer", "snap", "colors_two", "colors_one", "colors_above_64",
                 "all_14_tried"):
        assert n.get(what, 0) > 0, what
    assert n.get("restore", 0) == 0


def test_golden_file(harness):
    """tests/golden/palette.npz holds the inputs and what the reference's C computed for them: recorded data only"""
    L = launches(harness)
    data = dict(kmeans_data=L["kmeans"][1]["data"], kmeans_descs=L["kmeans"][1]["descs"].view(np.uint8), kmeans_cent=L["kmeans"][1]["want_cent"],
                kmeans_idx=L["kmeans"][1]["want_idx"])
    for bd in (8, 10):
        ours, theirs, _, (e1, cost1) = L[bd]
        data.update({"search_src_%d" % bd: theirs["src"], "search_descs_%d" % bd: theirs["descs"].view(np.uint8), "search_out_%d" % bd: theirs["want"], "cost_%d" % bd: cost1})
    if os.environ.get("SVT_PALETTE_WRITE_GOLDEN") == "1":
        np.savez_compressed(pc.GOLDEN, **data)
    gold = pc.load_golden()
    assert set(gold.files) == set(data)
    for k, v in data.items():
        assert np.array_equal(gold[k], v), k
    assert os.path.getsize(pc.GOLDEN) < 1 << 20
