"""RD distortion kernels (csrc/dist.hip): spatial SSE, coefficient SSE and the psy-rd energy term, as batched launches, as single-call forms with the
reference's prototypes, and as the round trip that returns its own distortions.  The checker is tests/dist_common.py (numpy), itself pinned against the
reference's functions by test_restatement_is_the_reference."""
import ctypes as C

import numpy as np
import pytest

import dist_common as dc
from conftest import GpuBackend, _backends, p, rng

U64 = C.c_uint64
_PIX = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32]


def _bind_ref(ref):
    ref.svt_psy_distortion.restype = ref.svt_psy_distortion_hbd.restype = U64
    ref.svt_psy_distortion.argtypes = ref.svt_psy_distortion_hbd.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    ref.get_svt_psy_full_dist.restype = U64
    ref.get_svt_psy_full_dist.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint8, C.c_double]
    for n in ("svt_spatial_full_distortion_kernel_c", "svt_full_distortion_kernel16_bits_c"):
        getattr(ref, n).restype, getattr(ref, n).argtypes = U64, _PIX
    ref.svt_spatial_psy_distortion_kernel_c.restype, ref.svt_spatial_psy_distortion_kernel_c.argtypes = U64, _PIX + [C.c_double]
    ref.svt_full_distortion_kernel32_bits_c.restype = ref.svt_full_distortion_kernel_cbf_zero32_bits_c.restype = None
    ref.svt_full_distortion_kernel32_bits_c.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    ref.svt_full_distortion_kernel_cbf_zero32_bits_c.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    return ref


def _in_plane(g, blk, pad_x, pad_y, extra, mx):
    """the block inside a larger random plane -> (plane, offset in samples, stride)"""
    h, w = blk.shape
    pl = g.integers(0, mx + 1, (h + 2 * pad_y, w + pad_x + extra)).astype(blk.dtype)
    pl[pad_y:pad_y + h, pad_x:pad_x + w] = blk
    return pl, pad_y * pl.shape[1] + pad_x, pl.shape[1]


def _coeff_cases(g):
    """(coeff, recon, width, height, strides) : uniform in +-2^20, the int32 extremes, strides larger than the width"""
    out = []
    for k, (w, h) in enumerate([(4, 4), (8, 8), (16, 16), (32, 32), (4, 16), (16, 4), (8, 32), (32, 8), (16, 32), (32, 16), (4, 8), (8, 4)]):
        cs, rs = w + 1 + k % 3, w + 2 * (k % 4)
        c = g.integers(-(1 << 20), (1 << 20) + 1, (h, cs)).astype(np.int32)
        r = g.integers(-(1 << 20), (1 << 20) + 1, (h, rs)).astype(np.int32)
        if k % 4 == 1:
            c[:, :w] = g.choice(np.array([-2 ** 31, 2 ** 31 - 1], np.int64), (h, w)).astype(np.int32)
            r[:, :w] = g.choice(np.array([-2 ** 31, 2 ** 31 - 1], np.int64), (h, w)).astype(np.int32)
        out.append((c, r, w, h))
    return out


def test_restatement_is_the_reference(ref):
    """dist_common against the reference's own functions: 8 / 10 / 12 bit, seven input classes, every size; the high-bit-depth psy value is the one the
    reference computes with its 32-bit Hadamard temporaries (a plain Hadamard energy does not pass this test at 10 / 12 bit)."""
    ref = _bind_ref(ref)
    g = rng(4242)
    plain_differs = 0
    for bd in (8, 10, 12):
        hbd = bd > 8
        fpsy = ref.svt_psy_distortion_hbd if hbd else ref.svt_psy_distortion
        fsse = ref.svt_full_distortion_kernel16_bits_c if hbd else ref.svt_spatial_full_distortion_kernel_c
        for kind in dc.CLASSES:
            for (w, h) in dc.PSY_SIZES + dc.SSE_ONLY_SIZES:
                a, b = dc.make_pair(g, kind, w, h, bd)
                pa, oa, sa = _in_plane(g, a, 3, 1, 5, (1 << bd) - 1)
                pb, ob, sb = _in_plane(g, b, 7, 2, 2, (1 << bd) - 1)
                tag = (bd, kind, w, h)
                assert fsse(p(pa), oa, sa, p(pb), ob, sb, w, h) == dc.sse(a, b), ("sse",) + tag
                if (w, h) not in dc.PSY_SIZES:
                    continue
                px = pa.itemsize
                raw = fpsy(pa.ctypes.data + oa * px, sa, pb.ctypes.data + ob * px, sb, w, h)
                assert raw == dc.psy(a, b, hbd), ("psy",) + tag
                if hbd:
                    plain_differs += int(raw != dc.psy_scale(int(dc.psy_map(a, b, False, 8 if min(w, h) >= 8 else 4).sum()), True))
                if kind in ("zero", "same"):
                    assert raw == 0, tag
                for q in dc.PSY_RD:
                    assert ref.get_svt_psy_full_dist(p(pa), oa, sa, p(pb), ob, sb, w, h, int(hbd), q) == dc.psy_full_dist(raw, q), ("full", q) + tag
                    if not hbd:
                        want = dc.sse(a, b) + (dc.psy_full_dist(raw, q) if q > 0 else 0)
                        assert ref.svt_spatial_psy_distortion_kernel_c(p(pa), oa, sa, p(pb), ob, sb, w, h, q) == want, ("spatial psy", q) + tag
    assert plain_differs > 100, "the high-bit-depth psy value is expected to differ from the plain Hadamard energy on most inputs"
    for c, r, w, h in _coeff_cases(g):
        got = np.zeros(2, np.uint64)
        ref.svt_full_distortion_kernel32_bits_c(p(c), c.shape[1], p(r), r.shape[1], p(got), w, h)
        assert tuple(int(v) for v in got) == dc.coeff_dist(c[:, :w], r[:, :w]), (w, h)
        ref.svt_full_distortion_kernel_cbf_zero32_bits_c(p(c), c.shape[1], p(got), w, h)
        assert tuple(int(v) for v in got) == dc.coeff_dist(c[:, :w]), (w, h)


def _batch_layout(g, sizes, bd, n_min):
    """n >= n_min blocks of mixed sizes (every entry of `sizes` at least twice) at unaligned offsets inside two planes whose strides are not multiples of 16."""
    order = list(sizes) * 2
    small = [s for s in sizes if s[0] * s[1] <= 256]
    while len(order) < n_min:
        order.append(small[int(g.integers(len(small)))])
    order = [order[i] for i in g.permutation(len(order))]
    sa, sb = 531, 601  # strides (samples)
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    x = y = shelf = 0
    place = []
    for (w, h) in order:
        gap = 1 + int(g.integers(0, 7))  # odd and even, never a multiple of 8 on purpose
        if x + gap + w > sa - 2:
            x, y, shelf = 0, y + shelf + 1, 0
        place.append((x + gap, y, w, h))
        x, shelf = x + gap + w, max(shelf, h)
    rows = y + shelf + 1
    pa, pb = g.integers(0, mx + 1, (rows, sa)).astype(dt), g.integers(0, mx + 1, (rows + 3, sb)).astype(dt)
    kinds = list(dc.CLASSES)
    blocks = []
    for i, (bx, by, w, h) in enumerate(place):
        a, b = dc.make_pair(g, kinds[i % len(kinds)], w, h, bd)
        bx2, by2 = bx + 5, by + 3  # the second plane holds the block elsewhere
        pa[by:by + h, bx:bx + w] = a
        pb[by2:by2 + h, bx2:bx2 + w] = b
        blocks.append((by * sa + bx, by2 * sb + bx2, w, h, a, b))
    return pa, pb, sa, sb, blocks


def test_pixel_dist_batch(be):
    """One launch, >= 300 descriptors of mixed sizes: what = SSE, PSY and both; 8-bit planes, then 16-bit planes at 10 and 12 bit; every block compared."""
    g = rng(77)
    poison = np.uint64(0xDEADBEEFCAFEF00D)
    for bd in (8, 10, 12):
        hbd = bd > 8
        for what in (1, 2, 3):
            sizes = dc.PSY_SIZES + (dc.SSE_ONLY_SIZES if what == 1 else [])
            pa, pb, sa, sb, blocks = _batch_layout(g, sizes, bd, 320)
            n = len(blocks)
            assert n >= 300
            d = np.zeros(n, be.pkg.DistDesc)
            for i, (oa, ob, w, h, _, _) in enumerate(blocks):
                d[i] = (oa, ob, sa, sb, w, h, 0)
            dpa, dpb, dd = be.dev(pa), be.dev(pb), be.dev(d)
            so, po = be.dev(np.full(n, poison)), be.dev(np.full(n, poison))
            be.lib.svt_hip_pixel_dist_batch(be.ptr(dpa), be.ptr(dpb), be.ptr(dd), n, int(hbd), what, be.ptr(so), be.ptr(po), be.stream)
            gs, gp = be.host(so), be.host(po)
            for i, (_, _, w, h, a, b) in enumerate(blocks):
                tag = (bd, what, i, w, h)
                assert int(gs[i]) == (dc.sse(a, b) if what & 1 else int(poison)), ("sse",) + tag
                assert int(gp[i]) == (dc.psy(a, b, hbd) if what & 2 else int(poison)), ("psy",) + tag


@pytest.mark.gpu
def test_pixel_dist_full_plane():
    """Every 8x8, 32x32 and 64x64 block of a 1920x1080 8-bit pair and of a 3840x2160 10-bit pair (the part of the picture whole blocks cover), every block compared."""
    be = _backends.setdefault("gpu", GpuBackend())
    g = rng(2160)
    for (W, H, bd) in ((1920, 1080, 8), (3840, 2160, 10)):
        hbd = bd > 8
        mx = (1 << bd) - 1
        dt = np.uint16 if hbd else np.uint8
        stride = W + 24
        yy, xx = np.mgrid[0:H, 0:stride]
        a = np.clip((xx + 2 * yy) % (mx + 1) + g.integers(-8, 9, (H, stride)), 0, mx).astype(dt)
        b = np.clip(a.astype(np.int64) + g.integers(-12, 13, (H, stride)) * (1 + (xx // 64 + yy // 64) % 5), 0, mx).astype(dt)
        b[:, : W // 4] = g.integers(0, mx + 1, (H, W // 4))  # a stripe of unrelated content
        dpa, dpb = be.dev(a), be.dev(b)
        for bs in (8, 32, 64):
            nx, ny = W // bs, H // bs
            d = np.zeros(nx * ny, be.pkg.DistDesc)
            by, bx = np.mgrid[0:ny, 0:nx]
            off = (by * bs * stride + bx * bs).reshape(-1)
            d["in_off"], d["rec_off"], d["in_stride"], d["rec_stride"], d["width"], d["height"] = off, off, stride, stride, bs, bs
            dd = be.dev(d)
            so, po = be.empty(nx * ny, np.uint64), be.empty(nx * ny, np.uint64)
            be.lib.svt_hip_pixel_dist_batch(be.ptr(dpa), be.ptr(dpb), be.ptr(dd), nx * ny, int(hbd), 3, be.ptr(so), be.ptr(po), be.stream)
            ca, cb = a[:ny * bs, :nx * bs], b[:ny * bs, :nx * bs]
            ws, wp = dc.sse_blocks(ca, cb, bs, bs).reshape(-1), dc.psy_blocks(ca, cb, hbd, bs, bs).reshape(-1)
            gs, gp = be.host(so), be.host(po)
            bad = np.flatnonzero((gs != ws) | (gp != wp))
            assert bad.size == 0, (W, H, bd, bs, bad[:8], gs[bad[:8]], ws[bad[:8]], gp[bad[:8]], wp[bad[:8]])
            assert np.count_nonzero(wp) > nx * ny // 2


def test_coeff_dist_batch(be):
    """Coefficient-domain distortion: +-2^20, the int32 extremes, strides larger than the width, cbf_zero mixed within one launch -- with recon_off pointing far
    outside the buffer for the cbf_zero blocks (on the emulator, where device buffers are heap blocks, reading it would fault) and poisoned recon values."""
    g = rng(5)
    cases = _coeff_cases(g) * 3
    n = len(cases)
    d = np.zeros(n, be.pkg.CoeffDistDesc)
    cbuf, rbuf, co, ro = [], [], 0, 0
    want = []
    for i, (c, r, w, h) in enumerate(cases):
        z = i % 3 == 1
        r = r.copy()
        if z:
            r[:] = 0x7fffffff
        d[i] = (co, (1 << 40) if z else ro, c.shape[1], r.shape[1], w, h, int(z), (0, 0, 0))
        want.append(dc.coeff_dist(c[:, :w], None if z else r[:, :w]))
        cbuf.append(c.reshape(-1)); rbuf.append(r.reshape(-1))
        co += c.size; ro += r.size
    dcf, drf, dd = be.dev(np.concatenate(cbuf)), be.dev(np.concatenate(rbuf)), be.dev(d)
    out = be.empty((n, 2), np.uint64)
    be.lib.svt_hip_coeff_dist_batch(be.ptr(dcf), be.ptr(drf), be.ptr(dd), n, be.ptr(out), be.stream)
    got = be.host(out)
    for i in range(n):
        assert (int(got[i, 0]), int(got[i, 1])) == want[i], (i, cases[i][2:], int(d[i]["cbf_zero"]))


def test_per_call_forms(be):
    """Every single-call form against dist_common (and against the reference's function where oracle/_ref is built): offsets, strides, psy_rd = 0 (psy term
    absent), the constant answers (all-zero, input == recon -> 0 at every size)."""
    import os
    from conftest import REF_LIB
    ref = _bind_ref(C.CDLL(REF_LIB)) if os.path.exists(REF_LIB) else None
    L = be.lib
    g = rng(99)
    sizes = dc.PSY_SIZES if be.is_gpu else [s for s in dc.PSY_SIZES if s[0] * s[1] <= 4096]
    for bd in (8, 10, 12):
        hbd = bd > 8
        mx = (1 << bd) - 1
        for si, (w, h) in enumerate(sizes):
            for kind in ("zero", "same", dc.CLASSES[si % 5]):
                a, b = dc.make_pair(g, kind, w, h, bd)
                pa, oa, sa = _in_plane(g, a, 3, 1, 5, mx)
                pb, ob, sb = _in_plane(g, b, 9, 2, 1, mx)
                tag = (bd, kind, w, h)
                px = pa.itemsize
                wsse, wraw = dc.sse(a, b), dc.psy(a, b, hbd)
                if kind in ("zero", "same"):
                    assert wsse == 0 and wraw == 0
                fs = L.svt_full_distortion_kernel16_bits_hip if hbd else L.svt_spatial_full_distortion_kernel_hip
                assert fs(p(pa), oa, sa, p(pb), ob, sb, w, h) == wsse, ("sse",) + tag
                fp = L.svt_psy_distortion_hbd_hip if hbd else L.svt_psy_distortion_hip
                assert fp(pa.ctypes.data + oa * px, sa, pb.ctypes.data + ob * px, sb, w, h) == wraw, ("psy",) + tag
                for q in (0.0, 0.3, 1.1, 6.0) if si % 4 else dc.PSY_RD:
                    got = L.svt_get_psy_full_dist_hip(p(pa), oa, sa, p(pb), ob, sb, w, h, int(hbd), q)
                    assert got == dc.psy_full_dist(wraw, q), ("full", q) + tag
                    if ref is not None:
                        assert got == ref.get_svt_psy_full_dist(p(pa), oa, sa, p(pb), ob, sb, w, h, int(hbd), q), ("full vs ref", q) + tag
                    if not hbd:
                        got = L.svt_spatial_psy_distortion_kernel_hip(p(pa), oa, sa, p(pb), ob, sb, w, h, q)
                        assert got == wsse + (dc.psy_full_dist(wraw, q) if q > 0 else 0), ("spatial psy", q) + tag
                        if ref is not None:
                            assert got == ref.svt_spatial_psy_distortion_kernel_c(p(pa), oa, sa, p(pb), ob, sb, w, h, q), ("spatial psy vs ref", q) + tag
        for (w, h) in dc.SSE_ONLY_SIZES[:3] + [(1, 1), (7, 3), (9, 17)]:
            a, b = dc.make_pair(g, "random", w, h, bd)
            pa, oa, sa = _in_plane(g, a, 2, 1, 3, mx)
            pb, ob, sb = _in_plane(g, b, 5, 0, 0, mx)
            fs = L.svt_full_distortion_kernel16_bits_hip if hbd else L.svt_spatial_full_distortion_kernel_hip
            got = fs(p(pa), oa, sa, p(pb), ob, sb, w, h)
            assert got == dc.sse(a, b), ("sse odd", bd, w, h)
            if ref is not None:
                fr = ref.svt_full_distortion_kernel16_bits_c if hbd else ref.svt_spatial_full_distortion_kernel_c
                assert got == fr(p(pa), oa, sa, p(pb), ob, sb, w, h)
    for c, r, w, h in _coeff_cases(g):
        got = np.zeros(2, np.uint64)
        L.svt_full_distortion_kernel32_bits_hip(p(c), c.shape[1], p(r), r.shape[1], p(got), w, h)
        assert tuple(int(v) for v in got) == dc.coeff_dist(c[:, :w], r[:, :w]), (w, h)
        got[:] = 7
        L.svt_full_distortion_kernel_cbf_zero32_bits_hip(p(c), c.shape[1], p(got), w, h)
        assert tuple(int(v) for v in got) == dc.coeff_dist(c[:, :w]), (w, h)
    assert L.svt_hip_debug_commit_violations() == 0


@pytest.mark.parametrize("ts", [0, 1, 2, 3, 4, 17, 12])
def test_roundtrip_dist_is_the_composition(be, ts):
    """svt_hip_txfm_quant_roundtrip_dist_batch == svt_hip_txfm_quant_roundtrip_batch, then svt_hip_coeff_dist_batch on (forward coefficients after the
    svt_handle_transform repack, dequantised coefficients) with cbf_zero where eob == 0, then svt_hip_pixel_dist_batch(src, pred) and (src, recon): recon, qcoeff,
    eob and all six distortion fields bit for bit, at 8 and 10 bit; once more with dqcoeff = NULL.  Inputs as tests/test_txfm.py's round-trip case."""
    from quant_common import make_qparams, make_scan
    pkg, L = be.pkg, be.lib
    w, h = pkg.TX_SIZES[ts]
    iw, ih = min(w, 32), min(h, 32)
    ncoef, pels = iw * ih, w * h
    ls = int(pels > 256) + int(pels > 1024)
    g = rng(900 + ts)
    types = pkg.allowed_tx_types(ts)
    steps = [(4, 4), (20, 22), (88, 112), (336, 460), (1336, 1828)]
    n = 10 if be.is_gpu else (4 if pels >= 1024 else 8)
    for bd, fp in ((8, 0), (10, 1)):
        qmode = (1 if bd > 8 else 0) + 2 * fp
        amp = (1 << bd) - 1
        dt = np.uint16 if bd > 8 else np.uint8
        stride, sstride = w + 3, w + 7
        res = g.integers(-amp, amp + 1, (n, h * stride)).astype(np.int16)
        res[0, :] = amp
        res[2, :] = g.integers(-3, 4, h * stride)
        res[3, :] = 0  # eob == 0: the cbf_zero form
        pred = g.integers(0, amp + 1, (n, h * stride)).astype(dt)
        src = g.integers(0, amp + 1, (n, h * sstride)).astype(dt)
        plist = [make_qparams(dcq * (4 if bd > 8 else 1), ac * (4 if bd > 8 else 1), fp=bool(fp)) for (dcq, ac) in steps]
        params = np.zeros(len(plist), dtype=pkg.QuantParams)
        for i, P in enumerate(plist):
            params[i] = (P["zbin"], P["round"], P["quant"], P["quant_shift"], P["dequant"], ls)
        sc = [make_scan(ncoef, g) for _ in range(2)]
        iscans = np.stack([s[1] for s in sc])
        rd, sr = np.zeros(n, dtype=pkg.RoundtripDesc), np.zeros(n, dtype=pkg.PlaneRef)
        for i in range(n):
            tt = types[i % len(types)]
            rd[i] = (i * h * stride, i * h * stride, i * h * stride, stride, stride, stride, i % len(plist), i % 2, 0, tt, (0,) * 7)
            sr[i] = (i * h * sstride + 2, sstride, 0)
        d_res, d_pred, d_src, d_rd, d_sr, d_par, d_is = (be.dev(v) for v in (res, pred, src, rd, sr, params, iscans))
        # the composition
        q1, dq1, e1, rec1 = be.empty((n, ncoef), np.int32), be.empty((n, ncoef), np.int32), be.empty(n, np.uint16), be.empty((n, h * stride), dt)
        L.svt_hip_txfm_quant_roundtrip_batch(be.ptr(d_res), be.ptr(d_pred), be.ptr(rec1), be.ptr(d_rd), n, ts, bd, qmode, be.ptr(d_par), be.ptr(d_is), None, None,
                                             be.ptr(q1), be.ptr(dq1), be.ptr(e1), be.stream)
        fd = np.zeros(n, dtype=pkg.FwdTxfmDesc)
        for i in range(n):
            fd[i] = (i * h * stride, stride, int(rd[i]["tx_type"]), (0, 0, 0))
        co = be.empty((n, pels), np.int32)
        d_fd = be.dev(fd)
        L.svt_hip_fwd_txfm2d_batch(be.ptr(d_res), be.ptr(d_fd), n, ts, bd, 0, be.ptr(co), be.stream)
        if max(w, h) == 64:
            en = be.empty(n, np.uint64)
            L.svt_hip_handle_transform_batch(be.ptr(co), n, ts, 0, be.ptr(en), be.stream)
        eobs = be.host(e1)
        assert eobs[3] == 0 and np.count_nonzero(eobs) >= n - 2
        cd = np.zeros(n, dtype=pkg.CoeffDistDesc)
        pd1, pd2 = np.zeros(n, dtype=pkg.DistDesc), np.zeros(n, dtype=pkg.DistDesc)
        for i in range(n):
            cd[i] = (i * pels, i * ncoef, iw, iw, iw, ih, int(eobs[i] == 0), (0, 0, 0))
            pd1[i] = (int(sr[i]["off"]), i * h * stride, sstride, stride, w, h, 0)
            pd2[i] = pd1[i]
        d_cd, d_pd = be.dev(cd), be.dev(pd1)
        wcd, ws1, wp1, ws2, wp2 = be.empty((n, 2), np.uint64), be.empty(n, np.uint64), be.empty(n, np.uint64), be.empty(n, np.uint64), be.empty(n, np.uint64)
        L.svt_hip_coeff_dist_batch(be.ptr(co), be.ptr(dq1), be.ptr(d_cd), n, be.ptr(wcd), be.stream)
        L.svt_hip_pixel_dist_batch(be.ptr(d_src), be.ptr(d_pred), be.ptr(d_pd), n, int(bd > 8), 3, be.ptr(ws1), be.ptr(wp1), be.stream)
        L.svt_hip_pixel_dist_batch(be.ptr(d_src), be.ptr(rec1), be.ptr(d_pd), n, int(bd > 8), 3, be.ptr(ws2), be.ptr(wp2), be.stream)
        wcd, ws1, wp1, ws2, wp2 = (be.host(v) for v in (wcd, ws1, wp1, ws2, wp2))
        assert np.count_nonzero(wcd[:, 1]) >= n - 1 and np.count_nonzero(wcd[:, 0]) >= 1 and np.count_nonzero(wp2) >= n - 1  # (the checks below compare something)
        for with_dq in (True, False):
            q2, dq2, e2, rec2 = be.empty((n, ncoef), np.int32), be.empty((n, ncoef), np.int32), be.empty(n, np.uint16), be.empty((n, h * stride), dt)
            out = be.dev(np.full(n * 6, 0x5555555555555555, np.uint64))
            L.svt_hip_txfm_quant_roundtrip_dist_batch(be.ptr(d_res), be.ptr(d_pred), be.ptr(rec2), be.ptr(d_rd), n, ts, bd, qmode, be.ptr(d_par), be.ptr(d_is), None, None,
                                                      be.ptr(q2), be.ptr(dq2) if with_dq else None, be.ptr(e2), be.ptr(d_src), be.ptr(d_sr), be.ptr(out), be.stream)
            o = be.host(out).view(pkg.RdDist)
            tag = (pkg.TX_SIZES[ts], bd, with_dq)
            assert np.array_equal(be.host(q2), be.host(q1)) and np.array_equal(be.host(e2), eobs), tag
            assert np.array_equal(be.host(rec2).reshape(n, h, stride)[:, :, :w], be.host(rec1).reshape(n, h, stride)[:, :, :w]), tag
            if with_dq:
                assert np.array_equal(be.host(dq2), be.host(dq1)), tag
            assert np.array_equal(o["coeff_dist"], wcd), tag + (o["coeff_dist"], wcd)
            assert np.array_equal(o["sse_pred"], ws1) and np.array_equal(o["psy_pred"], wp1), tag
            assert np.array_equal(o["sse_recon"], ws2) and np.array_equal(o["psy_recon"], wp2), tag
