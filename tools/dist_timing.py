#!/usr/bin/env python3
"""Event timing of the RD distortion kernels (csrc/dist.hip) on the access shape of bench.py's `sad64x64_pairs` leg.  Standalone: imports the package and
bench.py's helpers, changes neither.  Prints one JSON object per line.

  python tools/dist_timing.py [--steps 20] [--warmup 5] [--planes 128] [--no-cpu] [--only pixel64|pixel8|roundtrip|sad]

Legs
  sad64x64_pairs    bench.py's own leg, in THIS process on THIS card: the yardstick ("memory-bound done well") the fractions below stand next to
  pixel_dist_64x64  65 280 (= 128 planes x 510) disjoint read-once 64x64 pairs, footprint above the 256 MiB Infinity Cache; 8 and 10 bit; what = 1, 2, 3
  pixel_dist_8x8    the same pixels as 8x8 blocks (64 descriptors per 64x64 pair)
  roundtrip_dist    svt_hip_txfm_quant_roundtrip_dist_batch against the composition it is defined by, 32x32, 16 384 blocks
  cpu reference     svt_spatial_full_distortion_kernel_avx2 and the reference's C svt_psy_distortion (the reference has no SIMD psy variant) on 16 threads
Algorithmic bytes per block: 2 * W * H * bytes-per-sample in + 16 B out.  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12


def event_time(torch, fn, steps, warmup):
    """median and minimum seconds per launch: `steps` launches, each between its own pair of events, after `warmup` launches"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e-3 for a, b in ev)
    return t[len(t) // 2], t[0]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def pixel_legs(torch, lib, pkg, stream, bench, a, which):
    PLANE, STRIDE, PAD = bench.PLANE, bench.STRIDE, bench.PAD
    n_src = a.planes
    o = ((PAD + np.arange(17)[:, None] * 64) * STRIDE + PAD + np.arange(30)[None, :] * 64).reshape(-1).astype(np.uint64)
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        if px == 1:
            planes = torch.randint(0, 256, (2 * n_src * PLANE,), dtype=torch.uint8, device="cuda")
        else:
            planes = torch.randint(0, 1 << bd, (2 * n_src * PLANE,), dtype=torch.int16, device="cuda")
        for bs in ((64,) if which == "pixel64" else (8,) if which == "pixel8" else (64, 8)):
            k = 64 // bs
            sub = (np.arange(k)[:, None] * bs * STRIDE + np.arange(k)[None, :] * bs).reshape(-1).astype(np.uint64)
            blk = (o[:, None] + sub[None, :]).reshape(-1)
            d = np.zeros(n_src * len(blk), dtype=pkg.DistDesc)
            for f in range(n_src):
                s = slice(f * len(blk), (f + 1) * len(blk))
                d["in_off"][s] = np.uint64(f * PLANE) + blk
                d["rec_off"][s] = np.uint64((n_src + f) * PLANE + 3 + 2 * STRIDE) + blk  # the second plane's blocks sit at arbitrary offsets, as in the SAD leg
            d["in_stride"] = d["rec_stride"] = STRIDE
            d["width"] = d["height"] = bs
            dd = torch.from_numpy(d.view(np.uint8)).cuda()
            so, po = torch.zeros(len(d), dtype=torch.int64, device="cuda"), torch.zeros(len(d), dtype=torch.int64, device="cuda")
            # parity of the first and the last plane pair against the numpy restatement, before any number is recorded
            import dist_common as dc
            lib.svt_hip_pixel_dist_batch(planes.data_ptr(), planes.data_ptr(), dd.data_ptr(), len(d), int(px == 2), 3, so.data_ptr(), po.data_ptr(), stream)
            torch.cuda.synchronize()
            gs, gp = so.cpu().numpy().view(np.uint64), po.cpu().numpy().view(np.uint64)
            for f in (0, n_src - 1):
                dt = np.uint16 if px == 2 else np.uint8
                hs = planes[f * PLANE:(f + 1) * PLANE].cpu().numpy().view(dt).reshape(bench.ROWS, STRIDE)
                hr = planes[(n_src + f) * PLANE:(n_src + f + 1) * PLANE].cpu().numpy().view(dt).reshape(bench.ROWS, STRIDE)
                ca, cb = hs[PAD:PAD + 1088, PAD:PAD + 1920], hr[PAD + 2:PAD + 1090, PAD + 3:PAD + 1923]
                ws, wp = dc.sse_blocks(ca, cb, bs, bs), dc.psy_blocks(ca, cb, px == 2, bs, bs)
                # descriptor order: 64x64 pair (raster), then its sub-blocks (raster)
                ws = ws.reshape(17, k, 30, k).transpose(0, 2, 1, 3).reshape(-1)
                wp = wp.reshape(17, k, 30, k).transpose(0, 2, 1, 3).reshape(-1)
                s = slice(f * len(blk), (f + 1) * len(blk))
                if not (np.array_equal(gs[s], ws) and np.array_equal(gp[s], wp)):
                    raise SystemExit("dist_timing: parity failure (bd %d, %dx%d, plane %d)" % (bd, bs, bs, f))
            for what in (1, 2, 3):
                fn = lambda: lib.svt_hip_pixel_dist_batch(planes.data_ptr(), planes.data_ptr(), dd.data_ptr(), len(d), int(px == 2), what, so.data_ptr(), po.data_ptr(), stream)  # noqa: E731
                med, best = event_time(torch, fn, a.steps, a.warmup)
                nbytes = len(d) * (2 * bs * bs * px + 16)
                emit(leg="pixel_dist_%dx%d" % (bs, bs), kind="gpu", bd=bd, what=what, blocks=len(d), us_per_launch=round(med * 1e6, 1), us_min=round(best * 1e6, 1),
                     algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 3), footprint_MB=round(2 * n_src * PLANE * px / 1e6),
                     parity="first and last plane pair == tests/dist_common.py")
            del dd, so, po
        if bd == 8 and not a.no_cpu:
            cpu_legs(bench, planes[:n_src * PLANE].cpu().numpy(), planes[n_src * PLANE:].cpu().numpy(), n_src)
        del planes
        torch.cuda.empty_cache()


def cpu_legs(bench, src, rec, n_src):
    """The CPU side over the same pixels, 16 threads: ONE call per plane over the 1920x1088 area its 510 pairs tile (a ctypes call per 64x64 block would time
    Python).  The value of the AVX2 function is not used: its 32-bit lane sums are sized for blocks, this is a timing of its inner loop."""
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    if not os.path.exists(ref_path) or " avx2 " not in open("/proc/cpuinfo").read():
        emit(leg="cpu_reference", kind="reference", note="not measured: oracle/_ref/libsvtref.so or AVX2 missing on this host")
        return
    ref = C.CDLL(ref_path)
    PLANE, STRIDE, PAD = bench.PLANE, bench.STRIDE, bench.PAD
    pix = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32]
    ref.svt_spatial_full_distortion_kernel_avx2.restype, ref.svt_spatial_full_distortion_kernel_avx2.argtypes = C.c_uint64, pix
    ref.svt_psy_distortion.restype = C.c_uint64
    ref.svt_psy_distortion.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    o0 = PAD * STRIDE + PAD
    nh = min(n_src, 64)

    def sse(f):
        return ref.svt_spatial_full_distortion_kernel_avx2(src.ctypes.data + f * PLANE, o0, STRIDE, rec.ctypes.data + f * PLANE, o0 + 3 + 2 * STRIDE, STRIDE, 1920, 1088)

    def psy(f):
        return ref.svt_psy_distortion(src.ctypes.data + f * PLANE + o0, STRIDE, rec.ctypes.data + f * PLANE + o0 + 3 + 2 * STRIDE, STRIDE, 1920, 1088)

    for name, fn, sym in (("sse", sse, "svt_spatial_full_distortion_kernel_avx2"), ("psy", psy, "svt_psy_distortion (C: the reference has no SIMD psy variant)")):
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(fn, range(min(nh, 16))))
            t0 = time.perf_counter()
            list(ex.map(fn, range(nh)))
            dt = time.perf_counter() - t0
        pairs = nh * 510
        emit(leg="cpu_%s_64x64_pairs" % name, kind="reference", symbol=sym, threads=16, bd=8, pairs=pairs, us_for_65280_pairs=round(dt / pairs * 65280 * 1e6, 1),
             Mpairs_per_s=round(pairs / dt / 1e6, 2), note="one call per plane over the 1920x1088 area its 510 pairs tile; host wall clock")


def roundtrip_leg(torch, lib, pkg, stream, a):
    from quant_common import make_qparams, make_scan
    g = np.random.default_rng(7)
    ts, w, h, n = 3, 32, 32, 16384
    ncoef = w * h
    for bd, fp in ((8, 0), (10, 0)):
        qmode = 1 if bd > 8 else 0
        amp, dt = (1 << bd) - 1, (np.uint16 if bd > 8 else np.uint8)
        res = g.integers(-amp // 4, amp // 4 + 1, (n, h * w)).astype(np.int16)
        pred, src = g.integers(0, amp + 1, (n, h * w)).astype(dt), g.integers(0, amp + 1, (n, h * w)).astype(dt)
        P = make_qparams(88 * (4 if bd > 8 else 1), 112 * (4 if bd > 8 else 1), fp=False)
        params = np.zeros(1, dtype=pkg.QuantParams)
        params[0] = (P["zbin"], P["round"], P["quant"], P["quant_shift"], P["dequant"], 1)
        iscan = make_scan(ncoef, g)[1][None]
        rd, sr, fd = np.zeros(n, dtype=pkg.RoundtripDesc), np.zeros(n, dtype=pkg.PlaneRef), np.zeros(n, dtype=pkg.FwdTxfmDesc)
        rd["in_off"] = rd["pred_off"] = rd["recon_off"] = sr["off"] = fd["in_off"] = np.arange(n, dtype=np.uint64) * (w * h)
        rd["in_stride"] = rd["pred_stride"] = rd["recon_stride"] = sr["stride"] = fd["in_stride"] = w
        cd, pd = np.zeros(n, dtype=pkg.CoeffDistDesc), np.zeros(n, dtype=pkg.DistDesc)
        cd["coeff_off"] = cd["recon_off"] = pd["in_off"] = pd["rec_off"] = np.arange(n, dtype=np.uint64) * (w * h)
        cd["coeff_stride"] = cd["recon_stride"] = cd["width"] = cd["height"] = pd["in_stride"] = pd["rec_stride"] = pd["width"] = pd["height"] = 32
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
        zeros = lambda nb: torch.zeros(nb, dtype=torch.uint8, device="cuda")  # noqa: E731
        d_res, d_pred, d_src, d_rd, d_sr, d_fd, d_cd, d_pd, d_par, d_is = (dev(x) for x in (res, pred, src, rd, sr, fd, cd, pd, params, iscan))
        rec, q, dq, eob, co = zeros(n * w * h * pred.itemsize), zeros(n * ncoef * 4), zeros(n * ncoef * 4), zeros(n * 2), zeros(n * ncoef * 4)
        out, wcd, s1, p1, s2, p2 = zeros(n * 48), zeros(n * 16), zeros(n * 8), zeros(n * 8), zeros(n * 8), zeros(n * 8)
        P_ = lambda t: t.data_ptr()  # noqa: E731

        def fused():
            lib.svt_hip_txfm_quant_roundtrip_dist_batch(P_(d_res), P_(d_pred), P_(rec), P_(d_rd), n, ts, bd, qmode, P_(d_par), P_(d_is), None, None, P_(q), P_(dq), P_(eob),
                                                        P_(d_src), P_(d_sr), P_(out), stream)

        def composition():  # the round trip, the forward coefficients it does not return, the coefficient sums, the two pixel launches (cbf_zero left 0: timing only)
            lib.svt_hip_txfm_quant_roundtrip_batch(P_(d_res), P_(d_pred), P_(rec), P_(d_rd), n, ts, bd, qmode, P_(d_par), P_(d_is), None, None, P_(q), P_(dq), P_(eob), stream)
            lib.svt_hip_fwd_txfm2d_batch(P_(d_res), P_(d_fd), n, ts, bd, 0, P_(co), stream)
            lib.svt_hip_coeff_dist_batch(P_(co), P_(dq), P_(d_cd), n, P_(wcd), stream)
            lib.svt_hip_pixel_dist_batch(P_(d_src), P_(d_pred), P_(d_pd), n, int(bd > 8), 3, P_(s1), P_(p1), stream)
            lib.svt_hip_pixel_dist_batch(P_(d_src), P_(rec), P_(d_pd), n, int(bd > 8), 3, P_(s2), P_(p2), stream)

        def plain():
            lib.svt_hip_txfm_quant_roundtrip_batch(P_(d_res), P_(d_pred), P_(rec), P_(d_rd), n, ts, bd, qmode, P_(d_par), P_(d_is), None, None, P_(q), P_(dq), P_(eob), stream)

        fused()
        composition()
        torch.cuda.synchronize()
        o = out.cpu().numpy().view(pkg.RdDist)
        e = eob.cpu().numpy().view(np.uint16)
        nz = e != 0  # (the composition above leaves cbf_zero unset; with eob != 0 both definitions coincide)
        same = (np.array_equal(o["coeff_dist"][nz], wcd.cpu().numpy().view(np.uint64).reshape(n, 2)[nz]) and np.array_equal(o["sse_pred"], s1.cpu().numpy().view(np.uint64))
                and np.array_equal(o["psy_pred"], p1.cpu().numpy().view(np.uint64)) and np.array_equal(o["sse_recon"], s2.cpu().numpy().view(np.uint64))
                and np.array_equal(o["psy_recon"], p2.cpu().numpy().view(np.uint64)))
        if not same:
            raise SystemExit("dist_timing: the fused round trip differs from the composition (bd %d)" % bd)
        for name, fn, launches in (("roundtrip_plain", plain, 1), ("roundtrip_dist_fused", fused, 2), ("roundtrip_dist_composition", composition, 5)):
            med, best = event_time(torch, fn, a.steps, a.warmup)
            emit(leg=name, kind="gpu", bd=bd, tx="32x32", blocks=n, launches=launches, us_per_call=round(med * 1e6, 1), us_min=round(best * 1e6, 1),
                 parity="fused == composition on all six fields" if name != "roundtrip_plain" else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--planes", type=int, default=128, help="source planes (x 510 pairs each); as many again for the second plane set")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", choices=("pixel64", "pixel8", "roundtrip", "sad"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dist_timing: no GPU -- nothing here is measurable on a CPU")
    import bench
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps")
    if a.only in (None, "sad"):
        r = bench.bench_sad_pairs(torch, lib, pkg, stream, SimpleNamespace(min_leg_s=0.5), False)
        emit(leg="sad64x64_pairs", kind="gpu", note="bench.py's leg, same process", blocks=240 * 510, Mblocks_per_s=round(r["value"], 1), us_per_launch=round(r["roofline"]["kernel_us"], 1), algorithmic_GBps=round(r["roofline"]["achieved"], 1),
             frac_of_8TBps=r["roofline"].get("frac"))
    if a.only in (None, "pixel64", "pixel8"):
        pixel_legs(torch, lib, pkg, stream, bench, a, a.only)
    if a.only in (None, "roundtrip"):
        roundtrip_leg(torch, lib, pkg, stream, a)


if __name__ == "__main__":
    main()
