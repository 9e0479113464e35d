"""numpy restatement of the AV1 luma palette tools (csrc/palette.hip): the k-means of k_means_template.h with its reseed stream and exits, the colour counters,
search_palette_luma with palette_rd_y, the colour-map cost with the neighbour context, the colour cost, the uniform cost, the palette prediction and the cache merge.
tests/test_palette_ref.py pins every function on the reference's C; tests/test_palette.py compares the kernels with it.  COUNTERS records which branches a run took, so
that a case list can be shown to reach them.  The case lists of both tests live here."""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "palette.npz")
COUNTERS = collections.Counter()
PALETTE_MAX_SIZE, PALETTE_MIN_SIZE, MAX_CANDS = 8, 2, 14
COST_SHIFT = 9  # AV1_PROB_COST_SHIFT


# ---- k-means ----------------------------------------------------------------------------------------------------------------------------------------
def calc_indices(data, cent):
    """svt_av1_calc_indices_dimN_c: data (n, dim), cent (k, dim); the nearest centroid of every point, the lowest index on ties; and the distances"""
    d = ((data[:, None, :].astype(np.int64) - cent[None, :, :].astype(np.int64)) ** 2).sum(2)
    idx = d.argmin(1)  # the first minimum, as the C's strict `<` keeps it
    return idx.astype(np.uint8), d[np.arange(len(data)), idx]


def lcg_rand16(state):
    state = (state * 1103515245 + 12345) & 0xffffffff
    return state, (state // 65536) % 32768


def calc_centroids(data, idx, k):
    n = len(data)
    state = int(data[0, 0]) & 0xffffffff
    cent = np.zeros((k, data.shape[1]), np.int64)
    empties = 0
    for j in range(k):
        m = idx == j
        cnt = int(m.sum())
        if cnt == 0:
            state, r = lcg_rand16(state)
            cent[j] = data[r % n]
            empties += 1
        else:
            cent[j] = (data[m].astype(np.int64).sum(0) + (cnt >> 1)) // cnt
    if empties >= 1:
        COUNTERS["reseed"] += 1
    if empties >= 2:
        COUNTERS["reseed_two_or_more"] += 1
    return cent


def k_means(data, cent, max_itr):
    """svt_av1_k_means_dimN_c: returns (centroids, indices)"""
    data = np.asarray(data, np.int64).reshape(len(data), -1)
    cent = np.asarray(cent, np.int64).reshape(-1, data.shape[1]).copy()
    k = len(cent)
    idx, dmin = calc_indices(data, cent)
    this_dist = int(dmin.sum())
    for it in range(max_itr):
        pre, pre_idx, pre_dist = cent, idx, this_dist
        cent = calc_centroids(data, idx, k)
        idx, dmin = calc_indices(data, cent)
        this_dist = int(dmin.sum())
        if this_dist > pre_dist:
            COUNTERS["restore"] += 1
            return pre, pre_idx
        if np.array_equal(cent, pre):
            COUNTERS["repeat_exit"] += 1
            return cent, idx
    if max_itr > 0:
        COUNTERS["max_itr_exit"] += 1
    return cent, idx


# ---- colour count -----------------------------------------------------------------------------------------------------------------------------------
def count_colors(block, bit_depth):
    """svt_av1_count_colors[_highbd] on in-range samples: (histogram, number of non-zero bins)"""
    hist = np.bincount(np.asarray(block).reshape(-1).astype(np.int64), minlength=1 << bit_depth).astype(np.int32)
    assert len(hist) == 1 << bit_depth
    return hist, int((hist != 0).sum())


# ---- search_palette_luma ----------------------------------------------------------------------------------------------------------------------------
def palette_rd_y(data, rows, cols, bw, bh, cent, cache, bit_depth):
    """palette_rd_y: (size, colours, map) -- size 0 when fewer than two colours remain"""
    cent = [int(v) for v in cent]
    n = len(cent)
    if len(cache) > 0:  # optimize_palette_colors
        for i in range(n):
            diffs = [abs(cent[i] - int(c)) for c in cache]
            at = int(np.argmin(diffs))  # the first minimum
            if diffs[at] <= 1:
                if diffs[at] == 1:
                    COUNTERS["snap"] += 1
                cent[i] = int(cache[at])
    uniq = sorted(set(cent))  # qsort + av1_remove_duplicates
    k = len(uniq)
    if k < n:
        COUNTERS["duplicates_removed"] += 1
        if k <= 2:
            COUNTERS["shrunk_to_two_or_fewer"] += 1
    if k < PALETTE_MIN_SIZE:
        return 0, None, None
    colors = np.clip(uniq, 0, (1 << bit_depth) - 1).astype(np.uint16)
    idx, _ = calc_indices(data.reshape(-1, 1), np.array(uniq, np.int64).reshape(-1, 1))
    cmap = np.pad(idx.reshape(rows, cols), ((0, bh - rows), (0, bw - cols)), mode="edge")  # extend_palette_color_map
    return k, colors, cmap


def search_palette_luma(block, bw, bh, cache, step, bit_depth):
    """search_palette_luma on the rows x cols samples of `block`: the list of kept candidates (size, colours, map of bh x bw)"""
    block = np.asarray(block).astype(np.int64)
    rows, cols = block.shape
    hist, colors = count_colors(block, bit_depth)
    cands = []
    if not (1 < colors <= 64):
        COUNTERS["colors_%s" % ("one" if colors == 1 else "above_64")] += 1
        return cands
    data = block.reshape(-1)
    lb, ub = int(data.min()), int(data.max())
    nmax = min(colors, PALETTE_MAX_SIZE)
    count = hist.copy()
    top = []
    for i in range(nmax):
        j = int(np.argmax(count))  # highest count, the lower value on ties
        top.append(j)
        count[j] = 0
    tried = 0

    def consider(cent):
        nonlocal tried
        tried += 1
        size, cols_, cmap = palette_rd_y(data, rows, cols, bw, bh, cent, cache, bit_depth)
        if size > 2:
            cands.append((size, cols_, cmap))

    for n in range(nmax, 1, -step):
        consider(top[:n])
    for n in range(nmax, 1, -1):
        if colors == PALETTE_MIN_SIZE:
            COUNTERS["colors_two"] += 1
            cent = [lb, ub]
        else:
            cent = [lb + (2 * i + 1) * (ub - lb) // n // 2 for i in range(n)]
            cent, _ = k_means(data.reshape(-1, 1), cent, 50)
            cent = cent.reshape(-1)
        consider(cent)
    if tried == MAX_CANDS:
        COUNTERS["all_14_tried"] += 1
    assert len(cands) <= MAX_CANDS
    return cands


# ---- rate -------------------------------------------------------------------------------------------------------------------------------------------
CONTEXT_LOOKUP = [-1, -1, 0, -1, -1, 4, 3, 2, 1]


def color_index_context(cmap, r, c):
    """svt_aom_get_palette_color_index_context_optimized: (context, reordered index of the colour at (r, c))"""
    nb = [int(cmap[r, c - 1]) if c > 0 else -1, int(cmap[r - 1, c]) if r > 0 else -1, int(cmap[r - 1, c - 1]) if r > 0 and c > 0 else -1]
    sc = [2, 2, 1]
    if nb[0] == nb[1]:
        sc[0] += sc[1]
        nb[1] = -1
        if nb[0] == nb[2]:
            sc[0] += sc[2]
            nb[2] = -1
    elif nb[0] == nb[2]:
        sc[0] += sc[2]
        nb[2] = -1
    elif nb[1] == nb[2]:
        sc[1] += sc[2]
        nb[2] = -1
    col, scr = [-1, -1, -1], [0, 0, 0]
    nv = 0
    for i in range(3):
        if nb[i] != -1:
            col[nv], scr[nv] = nb[i], sc[i]
            nv += 1
    if scr[0] < scr[1] or (scr[0] == scr[1] and col[0] > col[1]):
        scr[0], scr[1], col[0], col[1] = scr[1], scr[0], col[1], col[0]
    if scr[0] < scr[2]:
        scr[0], scr[2], col[0], col[2] = scr[2], scr[0], col[2], col[0]
    if scr[1] < scr[2]:
        scr[1], scr[2], col[1], col[2] = scr[2], scr[1], col[2], col[1]
    cur = int(cmap[r, c])
    idx, same = cur, -1
    for i in range(3):
        if col[i] > cur:
            idx += 1
        elif col[i] == cur:
            same = i
    if same != -1:
        idx = same
    return CONTEXT_LOOKUP[scr[0] + 2 * scr[1] + 2 * scr[2]], idx


def cost_color_map(cmap, rows, cols, size, table, seen=None):
    """svt_av1_cost_color_map: cmap is the 2-D map at its pitch, table = palette_ycolor_fac_bitss[7][5][8]"""
    total = 0
    for r in range(rows):
        for c in range(cols):
            if r == 0 and c == 0:
                continue
            ctx, idx = color_index_context(cmap, r, c)
            if seen is not None:
                seen.add(ctx)
            total += int(table[size - 2][ctx][idx])
    return total


def ceil_log2(n):
    return 0 if n < 2 else int(n - 1).bit_length()


def color_cost_y(colors, cache, bit_depth):
    """svt_av1_palette_color_cost_y"""
    colors = [int(c) for c in colors]
    n, n_cache = len(colors), len(cache)
    flags = [0] * n
    if n_cache > 0:
        found = 0
        for i in range(n_cache):
            if found >= n:
                break
            for j in range(n):
                if colors[j] == int(cache[i]):
                    flags[j] = 1
                    found += 1
                    break
    out = [colors[j] for j in range(n) if not flags[j]]
    bits = 0
    if len(out) > 0:
        bits = bit_depth
        if len(out) > 1:
            bits += 2
            deltas = [out[i] - out[i - 1] for i in range(1, len(out))]
            per = max(ceil_log2(max(max(deltas), 0) + 1 - 1), bit_depth - 3)
            rng_ = (1 << bit_depth) - out[0] - 1
            for d in deltas:
                bits += per
                rng_ -= d
                per = min(per, ceil_log2(rng_))
    return (n_cache + bits) << COST_SHIFT


def write_uniform_cost(n, v):
    l = n.bit_length() if n > 0 else 0
    m = (1 << l) - n
    if l == 0:
        return 0
    return (l - 1 if v < m else l) << COST_SHIFT


def palette_costs(cmap, rows, cols, size, colors, cache, bit_depth, table, seen=None):
    return (cost_color_map(cmap, rows, cols, size, table, seen), color_cost_y(colors[:size], cache, bit_depth), write_uniform_cost(size, int(cmap[0, 0])))


# ---- prediction and cache ---------------------------------------------------------------------------------------------------------------------------
def palette_pred(cmap, colors, x, y, w, h, dst16, bit_depth):
    v = np.asarray(colors, np.uint16)[cmap[y:y + h, x:x + w]]
    if not dst16:
        return v.astype(np.uint8)  # the C's cast
    return np.minimum(v, 0xFF if bit_depth == 8 else 0xFFFF).astype(np.uint16)


def palette_cache_y(above, left):
    """svt_get_palette_cache_y's merge of two ascending lists"""
    cache = []

    def add(v):
        if cache and v == cache[-1]:
            return
        cache.append(v)

    a, l = list(above), list(left)
    while a and l:
        if l[0] < a[0]:
            add(l.pop(0))
        else:
            if l[0] == a[0]:
                l.pop(0)
            add(a.pop(0))
    for v in a:
        add(v)
    for v in l:
        add(v)
    return cache


# ---- case lists -------------------------------------------------------------------------------------------------------------------------------------
def rng(seed):
    return np.random.default_rng(seed)


def screen_block(g, rows, cols, values):
    """synthetic screen content with exactly the given colours: a dominant background, runs of the others, every colour at least once"""
    values = np.asarray(values, np.int64)
    p = 1.0 / (1 + np.arange(len(values))) ** 1.5
    flat = g.choice(len(values), size=rows * cols, p=p / p.sum())
    runs = g.integers(1, 6, rows * cols)
    flat = np.repeat(flat, runs)[:rows * cols]
    at = g.permutation(rows * cols)[:len(values)]
    flat[at] = np.arange(len(values))
    assert rows * cols >= len(values)
    return values[flat].reshape(rows, cols)


def pick_values(g, ncolors, maxv, spread=None):
    if spread is None:
        return np.sort(g.choice(maxv + 1, ncolors, replace=False))
    lo = int(g.integers(0, maxv + 1 - spread))
    return np.sort(lo + g.choice(spread, ncolors, replace=False))


SEARCH_GEOMETRIES = [(8, 8, 8, 8), (8, 32, 8, 32), (32, 8, 32, 8), (16, 16, 12, 16), (16, 16, 16, 4), (64, 16, 64, 16), (64, 64, 64, 64), (64, 64, 60, 52)]  # bw, bh, cols, rows
SEARCH_COLORS = [1, 2, 3, 8, 9, 64, 65]


def search_cases(bit_depth):
    """the blocks of the search tests: every geometry with every colour count it can hold, caches of 0 / 1 / 16 colours at distance 0, 1 and 2 from colours of the
    block, steps 1 / 2 / 3, values at 0 and at the maximum, and the blocks that reach the rare branches"""
    g = rng(1000 + bit_depth)
    maxv = (1 << bit_depth) - 1
    cases = []

    def add(bw, bh, cols, rows, values, cache, step, note=""):
        cases.append(dict(bw=bw, bh=bh, rows=rows, cols=cols, block=screen_block(g, rows, cols, values), cache=[int(c) for c in cache], step=step, note=note))

    def cache_near(values, n_cache, dist):
        if n_cache == 0:
            return []
        base = [int(np.clip(int(v) + (dist if i % 2 else -dist), 0, maxv)) for i, v in enumerate(values)]
        extra = [int(v) for v in g.choice(maxv + 1, 32, replace=False)]
        return sorted(set((base + extra)[:n_cache]))[:16] if n_cache > 1 else [base[0]]

    i = 0
    for (bw, bh, cols, rows) in SEARCH_GEOMETRIES:
        for nc in SEARCH_COLORS:
            if nc > rows * cols:
                continue
            values = pick_values(g, nc, maxv, None if i % 3 else min(maxv + 1, max(nc + 3, 40)))
            if i % 5 == 0:
                values[0] = 0
            if i % 5 == 1:
                values[-1] = maxv
            values = np.unique(values)
            while len(values) < nc:
                values = np.unique(np.append(values, g.integers(0, maxv + 1)))
            add(bw, bh, cols, rows, values, cache_near(values, (0, 1, 16)[i % 3], (0, 1, 2)[(i // 3) % 3]), (1, 2, 3)[(i // 2) % 3])
            i += 1
    # three neighbouring colours and a cache colour in the middle: every centroid snaps to it, the palette shrinks to one colour and is dropped
    add(16, 16, 16, 16, [100, 101, 102], [101], 1, "snap, shrink, drop")
    add(16, 16, 16, 16, [10, 11, 12, 200], [11, 201], 1, "snap, shrink to two")
    add(32, 32, 32, 32, [5, 6, 7, 8, 9, 10, 11, 12, 13, maxv - 3, maxv - 2, maxv], [6, 9, 12], 1, "duplicates from the cache")
    add(8, 8, 8, 8, np.arange(0, 64), [], 1, "64 colours in 64 samples")
    add(16, 16, 16, 16, [0, 1, 2, maxv - 2, maxv - 1, maxv, maxv // 2, maxv // 2 + 1, maxv // 2 + 2], [], 2, "clusters far apart: empty clusters in the k-means")
    for seed in range(6):
        nc = int(g.integers(3, 41))
        add(16, 16, 16, 16, pick_values(g, nc, maxv, min(maxv + 1, 2 * nc + 5) if seed % 2 else None), cache_near(pick_values(g, 8, maxv), 16 if seed % 2 else 0, 1), 1 + seed % 3)
    return cases


KMEANS_NS = (1, 63, 64, 65, 1000, 4096, 16384)


def kmeans_cases():
    """(data (n, dim), centroids (k, dim), max_itr, assign_only): every n of the list with both dims, k 1 .. 8, values at 0 and at the 8 / 10 / 12-bit maximum, ties
    between centroids, three-colour data with k 8 (reseeds of several clusters), max_itr 2 (that exit), max_itr 0 and the assignment alone"""
    g = rng(77)
    cases = []
    i = 0
    for n in KMEANS_NS:
        for dim in (1, 2):
            for k in ((1, 8) if n in (1, 4096, 16384) else (2, 3, 4, 5, 6, 7, 8) if n == 65 else (1 + i % 8, 8)):
                maxv = (255, 1023, 4095)[i % 3]
                data = g.integers(0, maxv + 1, (n, dim))
                if n > 2:
                    data[1], data[2] = 0, maxv
                cent = g.integers(0, maxv + 1, (k, dim))
                max_itr = 2 if n == 16384 else (50, 50, 2, 0)[i % 4]
                cases.append((data, cent, max_itr, i % 7 == 6))
                i += 1
    for dim in (1, 2):  # three colours, eight clusters: five clusters are empty and reseeded from one stream
        for n in (64, 200):
            data = g.choice([17, 130, 250], (n, dim))
            cases.append((data, np.linspace(0, 255, 8 * dim).astype(np.int64).reshape(8, dim), 50, False))
            cases.append((data, np.linspace(0, 255, 8 * dim).astype(np.int64).reshape(8, dim), 2, False))
        data = g.integers(0, 256, (64, dim))  # ties: equal centroids, and centroids at equal distance of every point
        cases.append((data, np.full((4, dim), 128), 50, False))
        cases.append((data * 2, np.array([[1] * dim, [1] * dim, [255] * dim, [255] * dim]), 0, False))
        cases.append((np.full((65, dim), 10), np.array([[8] * dim, [12] * dim, [10] * dim]), 50, True))
    return cases


def rate_table(seed=5):
    """a stand-in for palette_ycolor_fac_bitss[7][5][8]: distinct values, so that a wrong context or index shows"""
    return rng(seed).integers(1, 5000, (7, 5, 8)).astype(np.int32)


def load_golden():
    return np.load(GOLDEN)


# ---- launches shared by tests/test_palette.py and tests/test_palette_ref.py -------------------------------------------------------------------------------
OUT_HEADER = 240  # sizeof(SvtHipPaletteSearchOut)


def expected_search_out(out, off, map_stride, bw, bh, cands):
    """writes what the search leaves for one block into the byte buffer `out` (already holding the sentinel)"""
    out[off] = len(cands)
    for s, (size, colors, cmap) in enumerate(cands):
        out[off + 1 + s] = size
        o = off + 16 + 16 * s
        out[o:o + 2 * size] = np.asarray(colors, "<u2").view(np.uint8)
        o = off + OUT_HEADER + s * map_stride
        out[o:o + bw * bh] = cmap.reshape(-1)


def search_launch(pkg, bit_depth, searcher=search_palette_luma):
    """one launch over search_cases(bit_depth) in permuted order: the source plane (every block with its own stride and an odd lead-in, the last block ending with the
    allocation), the descriptors and the whole expected output buffer; `searcher` is the restatement, or the reference's C behind the same signature"""
    cases = search_cases(bit_depth)
    g = rng(4000 + bit_depth)
    order = [int(i) for i in g.permutation(len(cases))]
    dt = np.uint16 if bit_depth > 8 else np.uint8
    d = np.zeros(len(cases), pkg.PaletteSearchDesc)
    pieces, pos, out_pos = [np.full(3, 7, dt)], 3, 2
    for j, i in enumerate(order):
        c = cases[i]
        last = j == len(order) - 1
        stride = c["cols"] + (0 if c["cols"] == c["bw"] and j % 2 else 1 + 2 * (j % 4))
        plane = g.integers(0, 1 << bit_depth, (c["rows"], stride)).astype(dt)
        plane[:, :c["cols"]] = c["block"]
        flat = plane.reshape(-1)
        if last:
            flat = flat[:(c["rows"] - 1) * stride + c["cols"]]  # nothing readable after the block's last sample
        pieces.append(flat)
        map_stride = c["bw"] * c["bh"] + 2 * (j % 3)
        d["src_off"][j], d["src_stride"][j], d["out_off"][j], d["map_stride"][j] = pos, stride, out_pos, map_stride
        d["rows"][j], d["cols"][j], d["block_width"][j], d["block_height"][j] = c["rows"], c["cols"], c["bw"], c["bh"]
        d["n_cache"][j], d["dominant_color_step"][j] = len(c["cache"]), c["step"]
        d["cache"][j, :len(c["cache"])] = c["cache"]
        pos += len(flat)
        out_pos += OUT_HEADER + MAX_CANDS * map_stride + 2 * (j % 2)
    src = np.concatenate(pieces)
    want = np.full(out_pos + 6, 0xA5, np.uint8)
    for j, i in enumerate(order):
        c = cases[i]
        cands = searcher(c["block"], c["bw"], c["bh"], c["cache"], c["step"], bit_depth)
        expected_search_out(want, int(d["out_off"][j]), int(d["map_stride"][j]), c["bw"], c["bh"], cands)
    return dict(cases=cases, order=order, src=src, descs=d, want=want)


def cost_items(pkg, launch, bit_depth, table, coster=palette_costs):
    """every kept candidate of a search launch as a cost item that reads the search's output in place, with rows / cols of the block; expected (n, 3)"""
    d, items, want = launch["descs"], [], []
    for j, i in enumerate(launch["order"]):
        c = launch["cases"][i]
        off, ms = int(d["out_off"][j]), int(d["map_stride"][j])
        for s in range(int(launch["want"][off])):
            size = int(launch["want"][off + 1 + s])
            colors = launch["want"][off + 16 + 16 * s:off + 32 + 16 * s].view("<u2")
            cmap = launch["want"][off + OUT_HEADER + s * ms:off + OUT_HEADER + s * ms + c["bw"] * c["bh"]].reshape(c["bh"], c["bw"])
            cache = c["cache"] if (j + s) % 2 else []
            items.append((off + OUT_HEADER + s * ms, off + 16 + 16 * s, cache, c["rows"], c["cols"], c["bw"], size, bit_depth))
            want.append(coster(cmap, c["rows"], c["cols"], size, colors, cache, bit_depth, table))
    e = np.zeros(len(items), pkg.PaletteCostDesc)
    for n, (mo, co, cache, rows, cols, bw, size, bd) in enumerate(items):
        e["map_off"][n], e["colors_off"][n], e["rows"][n], e["cols"][n], e["block_width"][n], e["size"][n], e["n_cache"][n], e["bit_depth"][n] = mo, co, rows, cols, bw, size, len(cache), bd
        e["cache"][n, :len(cache)] = cache
    return e, np.array(want, np.int32).reshape(-1, 3)


def context_maps():
    """(map of 16 x 16 at pitch 16, size, rows, cols, cache, bit_depth): every palette size with random maps (all five contexts occur), rows / cols below the map"""
    g = rng(31)
    out = []
    for size in range(2, 9):
        for (rows, cols) in ((16, 16), (5, 16), (16, 3), (1, 9), (7, 1)):
            cmap = g.integers(0, size, (16, 16)).astype(np.uint8)
            cmap[::3] = np.repeat(cmap[::3, ::4], 4, axis=1)  # runs, so that equal neighbours occur as well
            colors = np.sort(g.choice(1024, size, replace=False)).astype(np.uint16)
            cache = sorted(set(int(v) for v in np.concatenate([colors[::2], g.choice(1024, 16, replace=False)])))[:16] if (size + rows) % 2 else []
            out.append((cmap, size, rows, cols, colors, cache, (8, 10, 12)[size % 3] if colors.max() < 256 else (10, 12)[size % 2]))
    return out


def kmeans_launch(pkg, kmeans=k_means, indexer=lambda x, c: calc_indices(x, c)[0]):
    """every case of kmeans_cases() as one item of ONE launch, in permuted order: flat buffers with gaps, descriptors and the expected buffers;
    `kmeans` / `indexer` are the restatement, or the reference's C behind the same signatures"""
    cases = kmeans_cases()
    order = [int(i) for i in rng(5).permutation(len(cases))]
    d = np.zeros(len(cases), pkg.KmeansDesc)
    data, cent, want_cent, want_idx = [np.full(1, -7, np.int32)], [np.full(3, -9, np.int32)], [np.full(3, -9, np.int32)], [np.full(5, 0xA5, np.uint8)]
    pos = [1, 3, 5]
    for j, i in enumerate(order):
        x, c0, max_itr, assign_only = cases[i]
        n, dim = x.shape
        k = len(c0)
        if assign_only:
            c1, idx = c0, indexer(x, c0)
        else:
            c1, idx = kmeans(x, c0, max_itr)
        d["data_off"][j], d["centroids_off"][j], d["indices_off"][j] = pos
        d["n"][j], d["max_itr"][j], d["dim"][j], d["k"][j], d["assign_only"][j] = n, max_itr, dim, k, assign_only
        gap = 1 + j % 3
        data += [x.astype(np.int32).reshape(-1), np.full(gap, -7, np.int32)]
        cent += [np.asarray(c0, np.int32).reshape(-1), np.full(gap, -9, np.int32)]
        want_cent += [np.asarray(c1, np.int32).reshape(-1), np.full(gap, -9, np.int32)]
        want_idx += [idx, np.full(gap, 0xA5, np.uint8)]
        pos = [pos[0] + n * dim + gap, pos[1] + k * dim + gap, pos[2] + n + gap]
    return dict(cases=cases, order=order, descs=d, data=np.concatenate(data), cent=np.concatenate(cent), want_cent=np.concatenate(want_cent), want_idx=np.concatenate(want_idx))
