"""AV1 inter prediction (csrc/interpred.hip): svt_hip_inter_pred_batch and the sixteen single-call forms, every output sample against tests/interpred_common.py (numpy;
pinned on the reference's C by tests/test_interpred_ref.py) and against tests/golden/interpred.npz (what the reference's C computed).  Every batched launch runs on
planes with odd strides (531 / 601 samples, destination 547), blocks at every byte alignment, the destination filled with 0xA5 beforehand: the WHOLE destination plane is
compared, so a sample written outside a block's w x h fails the test like a wrong sample inside it."""
import ctypes as C
import mmap

import numpy as np
import pytest

import dist_common as dc
import interpred_common as ic
from conftest import EmuBackend, _backends, p, rng

SA, SB, SD = 531, 601, 547  # strides in samples: reference plane 0, reference plane 1, destination
PLANE_A, PLANE_B = 3, 17    # indices into SvtHipInterPredPlanes.base
SIZES = [(2, 2), (4, 4), (4, 16), (16, 4), (8, 8), (8, 32), (16, 16), (32, 8), (32, 32), (64, 16), (64, 64), (16, 64), (128, 64), (128, 128)]
PHASES = [(0, 0), (1, 0), (8, 0), (0, 15), (0, 8), (8, 1), (15, 8), (1, 15)]  # copy, x, y, 2-D; phases 1, 8, 15 on either axis
FILTER_PAIRS = [(fx, fy) for fx in range(3) for fy in range(3)] + [(ic.BILINEAR, ic.BILINEAR)]
BIT_DEPTHS = (8, 10, 12)


def spec(w, h, fx, fy, compound, ph0, ph1=(0, 0), wt=(0, 0), kind="random"):
    return dict(w=w, h=h, fx=fx, fy=fy, compound=compound, ph=(ph0, ph1), wt=wt, kind=kind)


def _place(specs, g):
    """shelf layout of the blocks' (h + 7) x (w + 7) extents inside a plane of stride SA: gaps of 1 .. 7 samples, so that block origins take every alignment"""
    x = y = shelf = 0
    pos = []
    for s in specs:
        gap = 1 + int(g.integers(0, 7))
        ew, eh = s["w"] + 7, s["h"] + 7
        if x + gap + ew > SA - 2:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + ew, max(shelf, eh)
    return pos, y + shelf + 1


def build(be, specs, bd, g):
    """planes, descriptors and the expected destination plane of one launch"""
    dt = np.uint16 if bd > 8 else np.uint8
    mx = (1 << bd) - 1
    pos, rows = _place(specs, g)
    A = g.integers(0, mx + 1, (rows + 4, SA)).astype(dt)
    B = g.integers(0, mx + 1, (rows + 8, SB)).astype(dt)
    fill = 0xA5A5 if bd > 8 else 0xA5
    want = np.full((rows + 4, SD), fill, dt)
    d = np.zeros(len(specs), be.pkg.InterPredDesc)
    for i, (s, (x, y)) in enumerate(zip(specs, pos)):
        w, h = s["w"], s["h"]
        e0 = ic.make_ext(g, s["kind"], w, h, bd)
        e1 = ic.make_ext(g, "random" if s["kind"] == "zero" else s["kind"], w, h, bd)
        A[y:y + h + 7, x:x + w + 7] = e0
        B[y + 3:y + 3 + h + 7, x + 5:x + 5 + w + 7] = e1
        (sx0, sy0), (sx1, sy1) = s["ph"]
        d[i]["src_off"] = ((y + 3) * SA + x + 3, (y + 6) * SB + x + 8)
        d[i]["dst_off"] = (y + 3) * SD + x + 3
        d[i]["src_stride"], d[i]["dst_stride"] = (SA, SB), SD
        d[i]["plane"] = (PLANE_A, PLANE_B)
        d[i]["w"], d[i]["h"] = w, h
        d[i]["subpel_x"], d[i]["subpel_y"] = (sx0, sx1), (sy0, sy1)
        d[i]["filter_x"], d[i]["filter_y"], d[i]["compound"] = s["fx"], s["fy"], s["compound"]
        d[i]["fwd_offset"], d[i]["bck_offset"] = s["wt"]
        want[y + 3:y + 3 + h, x + 3:x + 3 + w] = ic.predict([(e0, sx0, sy0), (e1, sx1, sy1)], w, h, s["fx"], s["fy"], s["compound"], bd, *s["wt"])
    return A, B, d, want, fill


def launch(be, A, B, d, dst, bd, status=None, keep=None):
    planes = be.pkg.InterPredPlanes()
    dA, dB, dd = be.dev(A), be.dev(B), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    if keep is not None:
        keep.extend([dA, dB, dd])
    return be.lib.svt_hip_inter_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(d), bd, None if status is None else be.ptr(status), be.stream)


def run(be, specs, bd, seed, with_status=False):
    g = rng(seed)
    A, B, d, want, fill = build(be, specs, bd, g)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    status = be.dev(np.full(len(specs), 7, np.uint8)) if with_status else None
    assert launch(be, A, B, d, dst, bd, status) == 0
    got = be.host(dst)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        for i, s in enumerate(specs):  # name the first block that differs, or say that the damage is outside every block
            o, w, h = int(d[i]["dst_off"]), s["w"], s["h"]
            y, x = divmod(o, SD)
            assert np.array_equal(got[y:y + h, x:x + w], want[y:y + h, x:x + w]), (bd, i, s, got[y:y + h, x:x + w][:2, :8], want[y:y + h, x:x + w][:2, :8])
        raise AssertionError("samples outside every block's w x h were written: %s" % (np.argwhere(got != want)[:8],))


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_every_size_every_case(be, bd):
    """the fourteen sizes x (copy, x, y, 2-D) x (single, average, distance-weighted) in one launch: a dimension <= 4 on one axis only, tiles a block does not fill,
    blocks of several tiles in both directions; filters, input classes and weights cycle.  The 128-wide blocks: three each."""
    specs, k = [], 0
    for (w, h) in SIZES:
        for ci, ph in enumerate([(0, 0), (8, 0), (0, 15), (1, 8)]):
            for compound in (0, 1, 2):
                if w == 128 and (ci, compound) not in ((3, 0), (0, 1), (3, 2)):
                    continue
                fx, fy = FILTER_PAIRS[k % 10]
                specs.append(spec(w, h, fx, fy, compound, ph, PHASES[(k + 3) % 8], ic.DIST_WEIGHTS[k % 8], ic.CLASSES[k % 5] if k % 7 else "random"))
                k += 1
    assert len(specs) >= 150
    run(be, specs, bd, 100 + bd)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_every_filter_pair_and_phase(be, bd):
    """all nine pairs of the switchable filters and BILINEAR x the eight phase pairs (1, 8, 15 on either axis) at 8x8, 4x16 and 16x4 (the 4-tap tables on one axis),
    single and compound average: 480 descriptors in one launch"""
    specs, k = [], 0
    for (fx, fy) in FILTER_PAIRS:
        for (w, h) in ((8, 8), (4, 16), (16, 4)):
            for ph in PHASES:
                for compound in (0, 1):
                    specs.append(spec(w, h, fx, fy, compound, ph, PHASES[(k + 5) % 8], kind=ic.CLASSES[k % 5] if k % 3 == 0 else "random"))
                    k += 1
    run(be, specs, bd, 200 + bd)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_distance_weights_and_input_classes(be, bd):
    """all eight pairs of quant_dist_lookup_table x the four cases of either reference, and every input class x (single, average, weighted) with the SHARP kernel at
    the half-pel phase: the maximum / zero checkerboard drives it into both clips"""
    specs = []
    for wi, wt in enumerate(ic.DIST_WEIGHTS):
        for ci, ph in enumerate([(0, 0), (15, 0), (0, 1), (8, 8)]):
            specs.append(spec(16, 16, ic.REGULAR, ic.SMOOTH, 2, ph, [(8, 8), (0, 0), (1, 0), (0, 15)][(ci + wi) % 4], wt))
    for kind in ic.CLASSES:
        for compound in (0, 1, 2):
            for (w, h) in ((16, 16), (64, 64), (4, 4)):
                specs.append(spec(w, h, ic.SHARP, ic.SHARP, compound, (8, 8), (8, 15), (13, 3), kind))
    run(be, specs, bd, 300 + bd)
    if bd == 8:  # the checkerboard case does clip on both sides
        e = ic.make_ext(rng(1), "checker", 16, 16, 8)
        raw = ic.core(e, 16, 16, ic.FILTERS[ic.SHARP][8], ic.FILTERS[ic.SHARP][0], 1, 8, 3, 11, False, True)
        assert raw.min() < 0 and raw.max() > 255
        r2 = ic.core(e, 16, 16, ic.FILTERS[ic.SHARP][8], ic.FILTERS[ic.SHARP][8], 3, 8, 3, 11, False, True)
        assert r2.min() < 0 and r2.max() > 255


WIDE_SHORT = [(64, 8), (64, 4), (64, 2), (128, 8), (128, 4), (128, 2), (32, 2), (2, 128), (8, 128), (128, 16)]


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_wide_and_short_blocks(be, bd):
    """w >= 64 with h <= 8: blocks of fewer than 512 samples that are still wider than one tile, so the number of tiles is (w / 32) * (h / rows per tile) and not
    w * h / 512 -- the right-hand tiles must be predicted too.  Next to them the tall-and-narrow and the just-large-enough shapes; the four cases, single and both
    compound modes."""
    specs, k = [], 0
    for (w, h) in WIDE_SHORT:
        for ci, ph in enumerate([(0, 0), (15, 0), (0, 1), (8, 15)]):
            compound = (ci + k) % 3
            fx, fy = FILTER_PAIRS[k % 10]
            specs.append(spec(w, h, fx, fy, compound, ph, PHASES[(k + 2) % 8], ic.DIST_WEIGHTS[k % 8], ic.CLASSES[k % 5] if k % 4 == 0 else "random"))
            k += 1
    run(be, specs, bd, 700 + bd, with_status=bd == 10)


@pytest.mark.parametrize("bd", (8, 10))
def test_mixed_launch_with_status(be, bd):
    """320 descriptors of random size, case, filter and compound mode, through the asynchronous form (a status array: no synchronisation in the call)"""
    g = rng(400 + bd)
    small = [s for s in SIZES if s[0] * s[1] <= 1024]
    specs = []
    for i in range(320):
        w, h = SIZES[int(g.integers(len(SIZES) - 2))] if i % 16 == 0 else small[int(g.integers(len(small)))]
        fx, fy = FILTER_PAIRS[int(g.integers(10))]
        specs.append(spec(w, h, fx, fy, int(g.integers(3)), PHASES[int(g.integers(8))], PHASES[int(g.integers(8))], ic.DIST_WEIGHTS[int(g.integers(8))],
                          ic.CLASSES[int(g.integers(5))]))
    run(be, specs, bd, 500 + bd, with_status=True)


def test_golden_cases(be):
    """the cases of tests/golden/interpred.npz: the kernel == what the reference's C computed (and == the restatement)"""
    gold = ic.load_golden()
    cases = ic.golden_cases()
    assert int(gold["seed"][0]) == ic.GOLDEN_SEED and len(cases) >= 80
    for bd in BIT_DEPTHS:
        idx = [i for i, c in enumerate(cases) if c[2] == bd]
        dt = np.uint16 if bd > 8 else np.uint8
        planes = be.pkg.InterPredPlanes()
        d = np.zeros(len(idx), be.pkg.InterPredDesc)
        bufs, keep, off = [], [], 0
        for j, i in enumerate(idx):
            w, h, _, fx, fy, compound, _, _, (fwd, bck), _ = cases[i]
            refs = ic.golden_inputs(i, cases[i])
            assert sum(int(e.astype(np.int64).sum()) for (e, _, _) in refs) == int(gold["insum_%d" % i][0]), "the generator of the golden inputs changed"
            for k, (e, sx, sy) in enumerate(refs):
                d["src_off"][j, k], d["src_stride"][j, k] = off + 3 * (w + 7) + 3, w + 7
                d["subpel_x"][j, k], d["subpel_y"][j, k] = sx, sy
                bufs.append(e.reshape(-1))
                off += e.size
            d[j]["dst_off"], d[j]["dst_stride"], d[j]["w"], d[j]["h"] = j * 1024, w, w, h
            d[j]["filter_x"], d[j]["filter_y"], d[j]["compound"], d[j]["fwd_offset"], d[j]["bck_offset"] = fx, fy, compound, fwd, bck
        src = be.dev(np.concatenate(bufs).astype(dt))
        planes.base[0] = be.ptr(src)
        dst, dd = be.dev(np.zeros(len(idx) * 1024, dt)), be.dev(d)
        assert be.lib.svt_hip_inter_pred_batch(planes, be.ptr(dst), be.ptr(dd), len(idx), bd, None, be.stream) == 0
        got = be.host(dst)
        for j, i in enumerate(idx):
            w, h, _, fx, fy, compound, _, _, (fwd, bck), _ = cases[i]
            out = got[j * 1024:j * 1024 + w * h].reshape(h, w)
            assert np.array_equal(out, gold["out_%d" % i]), (i, cases[i])
            assert np.array_equal(out, ic.predict(ic.golden_inputs(i, cases[i]), w, h, fx, fy, compound, bd, fwd, bck)), (i, cases[i])


@pytest.mark.parametrize("bd", (8, 10))
def test_full_plane_of_16x16(be, bd):
    """the tile loop: every 16x16 block of a 1920x1080 plane, phases drawn from 0 / 1 / 8 / 15 per axis (every case occurs), REGULAR x SHARP, every third block compound
    average with the plane itself shifted as second reference; every output sample compared"""
    g = rng(1080 + bd)
    W, H, bs, pad = 1920, 1080, 16, 8
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    stride = W + 2 * pad + 5
    yy, xx = np.mgrid[0:H + 2 * pad, 0:stride]
    plane = np.clip((3 * xx + 5 * yy) % (mx + 1) + g.integers(-40, 41, yy.shape) * (1 + (xx // 48 + yy // 24) % 7), 0, mx).astype(dt)
    nx, ny = W // bs, H // bs
    n = nx * ny
    by, bx = (v.reshape(-1) for v in np.mgrid[0:ny, 0:nx])
    ph = np.array([0, 1, 8, 15])
    sx, sy = ph[g.integers(0, 4, (2, n))], ph[g.integers(0, 4, (2, n))]
    sx[1], sy[1] = ph[::-1][g.integers(0, 4, n) // 2 * 2 + (sx[0] > 1)], sy[0][::-1].copy()  # (few distinct phase sets: the checker is vectorised over the blocks that share one)
    comp = (np.arange(n) % 3 == 2).astype(np.uint8)
    d = np.zeros(n, be.pkg.InterPredDesc)
    o0 = (by * bs + pad) * stride + bx * bs + pad
    o1 = o0 + (1 - 2 * (by & 1)) * stride * 2 + (1 - 2 * (bx & 1)) * 3  # the second reference: the same plane, displaced by (+-3, +-2)
    d["src_off"], d["src_stride"], d["dst_off"], d["dst_stride"] = np.stack([o0, o1], 1), stride, by * bs * W + bx * bs, W
    d["w"], d["h"], d["subpel_x"], d["subpel_y"], d["filter_x"], d["filter_y"], d["compound"] = bs, bs, sx.T, sy.T, ic.REGULAR, ic.SHARP, comp
    planes = be.pkg.InterPredPlanes()
    dp, dd, dst = be.dev(plane), be.dev(d), be.dev(np.full(ny * bs * W, 0xA5, dt))
    planes.base[0] = planes.base[1] = be.ptr(dp)
    assert be.lib.svt_hip_inter_pred_batch(planes, be.ptr(dst), be.ptr(dd), n, bd, None, be.stream) == 0
    got = be.host(dst).reshape(ny, bs, nx, bs).transpose(0, 2, 1, 3).reshape(n, bs, bs)
    # the restatement, vectorised over the blocks that share (phases, compound)
    win = np.lib.stride_tricks.sliding_window_view(plane, (bs + 7, bs + 7))
    e0 = win[by * bs + pad - 3, bx * bs + pad - 3]
    y1, x1 = np.divmod(o1, stride)
    e1 = win[y1 - 3, x1 - 3]
    key = (((sx[0] * 16 + sy[0]) * 16 + sx[1] * comp) * 16 + sy[1] * comp) * 2 + comp
    want = np.zeros((n, bs, bs), np.int64)
    for k in np.unique(key):
        m = np.flatnonzero(key == k)
        i = m[0]
        want[m] = ic.predict([(e0[m], int(sx[0, i]), int(sy[0, i])), (e1[m], int(sx[1, i]), int(sy[1, i]))], bs, bs, ic.REGULAR, ic.SHARP, int(comp[i]), bd)
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, (bd, bad[:8], sx[:, bad[:4]], sy[:, bad[:4]], comp[bad[:4]])


def test_read_guard_on_the_emulator():
    """CPU only.  The readable extent is 3 samples left of / above and 4 right of / below each block: the reference planes lie in a mapping whose neighbouring pages are
    inaccessible, once with the LAST readable sample on the mapping's last byte and once with the FIRST one on its first byte, so a read outside the extent by as little
    as one sample leaves the allocation.  Every case, single and compound, 8 and 16 bit samples, widths from 2 (one 8-sample load spans the whole extent) to 64."""
    be = _backends.setdefault("emu", EmuBackend())
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes, libc.mprotect.restype = [C.c_void_p, C.c_size_t, C.c_int], C.c_int
    page = mmap.PAGESIZE
    g = rng(77)
    for bd in (8, 10):
        dt = np.dtype(np.uint16 if bd > 8 else np.uint8)
        for (w, h) in ((2, 2), (4, 8), (8, 4), (32, 16), (64, 32), (16, 64)):
            ext_bytes = (h + 7) * (w + 7) * dt.itemsize
            body = (ext_bytes + page - 1) // page * page
            for at_end in (True, False):
                maps = []
                for _ in range(2):  # one mapping per reference: guard page, body, guard page
                    m = mmap.mmap(-1, body + 2 * page)
                    base = C.addressof(C.c_char.from_buffer(m))
                    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0
                    maps.append((m, base))
                exts, planes = [], be.pkg.InterPredPlanes()
                for k, (m, base) in enumerate(maps):
                    start = page + (body - ext_bytes if at_end else 0)
                    a = np.frombuffer(m, dt, (h + 7) * (w + 7), start).reshape(h + 7, w + 7)
                    a[:] = ic.make_ext(g, "random", w, h, bd)
                    exts.append(a)
                    planes.base[k] = base + start
                specs = [(c, ph) for c in (0, 1, 2) for ph in ((0, 0), (8, 0), (0, 8), (15, 1))]
                d = np.zeros(len(specs), be.pkg.InterPredDesc)
                for i, (c, ph) in enumerate(specs):
                    d[i]["src_off"], d[i]["src_stride"], d[i]["plane"] = 3 * (w + 7) + 3, w + 7, (0, 1)
                    d[i]["dst_off"], d[i]["dst_stride"], d[i]["w"], d[i]["h"] = i * w * h, w, w, h
                    d[i]["subpel_x"], d[i]["subpel_y"] = (ph[0], ph[1]), (ph[1], ph[0])
                    d[i]["filter_x"], d[i]["filter_y"], d[i]["compound"], d[i]["fwd_offset"], d[i]["bck_offset"] = ic.SHARP, ic.REGULAR, c, 9, 7
                dst = np.zeros(len(specs) * w * h, dt)
                assert be.lib.svt_hip_inter_pred_batch(planes, p(dst), p(d), len(specs), bd, None, None) == 0
                for i, (c, ph) in enumerate(specs):
                    want = ic.predict([(exts[0], ph[0], ph[1]), (exts[1], ph[1], ph[0])], w, h, ic.SHARP, ic.REGULAR, c, bd, 9, 7)
                    assert np.array_equal(dst[i * w * h:(i + 1) * w * h].reshape(h, w), want), (bd, w, h, at_end, c, ph)
                del exts, a, maps  # (the mappings go with their last reference)


def _params(pkg, table_x, table_y, cbuf, do_average, r0, r1, jnt, use_jnt=0, fwd=0, bck=0):
    fx, fy = pkg.InterpFilterParams(table_x.ctypes.data, 8, 16, 0), pkg.InterpFilterParams(table_y.ctypes.data, 8, 16, 0)
    cp = pkg.ConvolveParams(0, do_average, cbuf.ctypes.data, cbuf.shape[1], r0, r1, 0, int(jnt), use_jnt, fwd, bck, use_jnt)
    return fx, fy, cp


def test_per_call_forms(be):
    """All sixteen forms at four sizes each (4x8: the 4-tap table in x; 32x16; 64x8 and 128x4: wider than a tile and shorter than one) and with a tap set that is none of AV1's tables (one tap outside a signed byte): the `_sr`
    forms' dst; the jnt_ forms' do_average = 0 -> 1 sequence through a caller-owned ConvBufType buffer with its own stride -- the first call leaves dst untouched and
    writes the buffer, the second averages (plain, then distance-weighted) -- ; nothing outside w x h of either buffer is written."""
    L, pkg = be.lib, be.pkg
    g = rng(16)
    foreign = np.ascontiguousarray(np.tile(ic.FOREIGN_TAPS, (16, 1)))
    foreign[9] = ic.FOREIGN_TAPS[::-1]
    k = 0
    for name, (case, jnt) in ic.FUNCTIONS.items():
        for hbd in (False, True):
            for (w, h, own) in ((4, 8, False), (32, 16, False), (8, 8, True), (64, 8, False), (128, 4, False)):
                bd = (10, 12)[k % 2] if hbd else 8
                k += 1
                dt = np.uint16 if hbd else np.uint8
                fill = 0xA5A5 if hbd else 0xA5
                f = getattr(L, "svt_av1_%s%s_hip" % ("highbd_" if hbd else "", name))
                tail = [bd] if hbd else []
                r0, r1 = ic.conv_rounds(bd, jnt)
                fxi, fyi = FILTER_PAIRS[k % 10]
                tab_x = foreign if own else np.ascontiguousarray(ic.FILTERS[ic.filter_kind(fxi, w)])
                tab_y = foreign if own else np.ascontiguousarray(ic.FILTERS[ic.filter_kind(fyi, h)])
                sx, sy = (9, 3) if own else ((1, 8, 15)[k % 3], (15, 1, 8)[k % 3])
                tag = (name, bd, w, h, own)
                e0, e1 = ic.make_ext(g, "checker" if k % 4 == 0 else "random", w, h, bd), ic.make_ext(g, "random", w, h, bd)
                plane0 = np.pad(e0, ((1, 2), (2, 3)), constant_values=7)  # the extent inside a larger plane: stride w + 12
                src0 = plane0.ctypes.data + ((1 + 3) * plane0.shape[1] + 2 + 3) * plane0.itemsize
                dst = np.full((h + 2, w + 3), fill, dt)
                cbuf = np.full((h + 1, w + 5), 0x5A5A, np.uint16)
                fx, fy, cp = _params(pkg, tab_x, tab_y, cbuf, 0, r0, r1, jnt)
                f(src0, plane0.shape[1], p(dst), dst.shape[1], w, h, C.addressof(fx), C.addressof(fy), sx, sy, C.addressof(cp), *tail)
                if not jnt:
                    want = np.full_like(dst, fill)
                    want[:h, :w] = ic.convolve_sr(e0, w, h, tab_x[sx], tab_y[sy], case, bd, r0, r1, not hbd)
                    assert np.array_equal(dst, want), tag
                    assert np.all(cbuf == 0x5A5A), tag
                    continue
                assert np.all(dst == fill), tag  # do_average == 0 leaves dst untouched
                wcb = np.full_like(cbuf, 0x5A5A)
                wcb[:h, :w] = ic.jnt_convolve(e0, w, h, tab_x[sx], tab_y[sy], case, bd, r0, r1, not hbd)
                assert np.array_equal(cbuf, wcb), tag
                src1 = e1.ctypes.data + (3 * (w + 7) + 3) * e1.itemsize
                for (use_jnt, fwd, bck) in ((0, 0, 0), (1,) + ic.DIST_WEIGHTS[k % 8]):
                    dst[:] = fill
                    fx, fy, cp = _params(pkg, tab_x, tab_y, cbuf, 1, r0, r1, True, use_jnt, fwd, bck)
                    f(src1, w + 7, p(dst), dst.shape[1], w, h, C.addressof(fx), C.addressof(fy), sx, sy, C.addressof(cp), *tail)
                    want = np.full_like(dst, fill)
                    want[:h, :w] = ic.jnt_convolve(e1, w, h, tab_x[sx], tab_y[sy], case, bd, r0, r1, not hbd, True, wcb[:h, :w], bool(use_jnt), fwd, bck)
                    assert np.array_equal(dst, want), tag + (use_jnt, fwd, bck)
                    assert np.array_equal(cbuf, wcb), tag  # do_average == 1 only reads the buffer
    assert L.svt_hip_debug_commit_violations() == 0


@pytest.mark.parametrize("r0,r1,jnt", [(8, 6, False), (-1, 11, False), (3, 12, False), (3, -1, False), (3, 8, True)])
def test_per_call_forms_reject_roundings_outside_the_accepted_range(be, r0, r1, jnt):
    """round_0 / round_1 are shift counts on the device: a pair outside the range include/svtav1_hip.h states (0 <= round_0 <= 7, round_1 >= 0, their sum <= 14,
    round_1 <= 7 in the jnt_ forms) is refused on the host -- neither dst nor the ConvBufType buffer is written"""
    pkg, w, h = be.pkg, 8, 8
    tab = np.ascontiguousarray(ic.FILTERS[ic.REGULAR])
    for hbd in (False, True):
        dt = np.uint16 if hbd else np.uint8
        e = ic.make_ext(rng(5), "random", w, h, 10 if hbd else 8)
        dst, cbuf = np.full((h, w), 0xA5, dt), np.full((h, w), 0x5A5A, np.uint16)
        fx, fy, cp = _params(pkg, tab, tab, cbuf, 0, r0, r1, jnt)
        f = getattr(be.lib, "svt_av1_%s%s_hip" % ("highbd_" if hbd else "", "jnt_convolve_2d" if jnt else "convolve_2d_sr"))
        f(e.ctypes.data + (3 * (w + 7) + 3) * e.itemsize, w + 7, p(dst), w, w, h, C.addressof(fx), C.addressof(fy), 8, 8, C.addressof(cp), *([10] if hbd else []))
        assert np.all(dst == 0xA5) and np.all(cbuf == 0x5A5A)


@pytest.mark.parametrize("bd", (8, 10))
def test_prediction_feeds_distortion(be, bd):
    """svt_hip_inter_pred_batch, then svt_hip_pixel_dist_batch on the same stream with no host synchronisation between them (the asynchronous form: a status array):
    the SSE of every prediction against a source plane == the SSE of the restatement's prediction"""
    g = rng(600 + bd)
    specs = []
    for i, (w, h) in enumerate([s for s in SIZES if s[0] >= 4 and s[1] >= 4 and s[0] <= 64] * 2):
        fx, fy = FILTER_PAIRS[i % 10]
        specs.append(spec(w, h, fx, fy, i % 3, PHASES[(i + 5) % 8], PHASES[i % 8], ic.DIST_WEIGHTS[i % 8]))
    A, B, d, want, fill = build(be, specs, bd, g)
    n = len(specs)
    src = g.integers(0, 1 << bd, want.shape).astype(want.dtype)
    dst, status, keep = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(n, 7, np.uint8)), []
    dsrc, sse = be.dev(src), be.dev(np.full(n, 0xDEADBEEF, np.uint64))
    dd = np.zeros(n, be.pkg.DistDesc)
    dd["in_off"], dd["rec_off"], dd["in_stride"], dd["rec_stride"], dd["width"], dd["height"] = d["dst_off"], d["dst_off"], SD, SD, d["w"], d["h"]
    ddd = be.dev(dd)
    assert launch(be, A, B, d, dst, bd, status, keep) == 0
    be.lib.svt_hip_pixel_dist_batch(be.ptr(dsrc), be.ptr(dst), be.ptr(ddd), n, int(bd > 8), 1, be.ptr(sse), None, be.stream)
    got = be.host(sse)
    for i, s in enumerate(specs):
        y, x = divmod(int(d[i]["dst_off"]), SD)
        assert int(got[i]) == dc.sse(src[y:y + s["h"], x:x + s["w"]], want[y:y + s["h"], x:x + s["w"]]), (bd, i, s)
    assert not be.host(status).any()


@pytest.mark.parametrize("what", ["width 3", "height 96", "phase 16", "filter 4", "compound 3", "NULL plane", "second NULL plane"])
def test_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones: with status == NULL the call returns -1 and not one destination byte changes; with a status array it returns 0,
    flags that descriptor alone, leaves its block untouched and predicts the other two"""
    g = rng(9)
    specs = [spec(8, 8, 0, 2, 0, (8, 1)), spec(16, 8, 1, 1, 1 if "second" in what or "compound" in what else 0, (1, 1), (2, 2)), spec(4, 4, 2, 0, 2, (0, 0), (15, 15), (9, 7))]
    A, B, d, want, fill = build(be, specs, 8, g)
    y, x = divmod(int(d[1]["dst_off"]), SD)
    want[y:y + 8, x:x + 16] = fill
    if what == "width 3":
        d["w"][1] = 3
    elif what == "height 96":
        d["h"][1] = 96
    elif what == "phase 16":
        d["subpel_y"][1, 0] = 16
    elif what == "filter 4":
        d["filter_x"][1] = 4
    elif what == "compound 3":
        d["compound"][1] = 3
    elif what == "NULL plane":
        d["plane"][1, 0] = 5
    else:
        d["plane"][1, 1] = 31
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    assert launch(be, A, B, d, dst, 8) == -1
    assert np.all(be.host(dst) == fill)
    status = be.dev(np.full(3, 7, np.uint8))
    assert launch(be, A, B, d, dst, 8, status) == 0
    assert np.array_equal(be.host(dst), want)
    assert be.host(status).tolist() == [0, 1, 0]
    planes = be.pkg.InterPredPlanes()
    assert be.lib.svt_hip_inter_pred_batch(planes, be.ptr(dst), be.ptr(status), 1, 9, None, be.stream) == -1  # not a bit depth
