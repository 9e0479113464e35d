#!/usr/bin/env python3
"""Event timing of the intra-prediction kernels (csrc/intrapred.hip).  Standalone: imports the package, changes nothing.  Prints one JSON object per line and writes
the same lines to profiles/intrapred_timing.txt (--out).

  python tools/intrapred_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--out FILE]

Legs (8 and 10 bit).  Neighbours are read IN PLACE from a padded picture plane (top row, corner and left column with left_stride = the picture stride; all four
availability counts complete), the prediction goes to a packed plane.
  intra_pred <class>   every 16x16 block of one 1080p and one 4K luma plane, one mode class per launch: dc, v, h, smooth, paeth, z1 (D45 +1), z2 (D135 -2),
                       z3 (D203 +1), z1_up / z2_up (8x8 blocks with filt_type 0: both upsampled), filter_intra (mode 0)
  intra_scan66         all 61 (mode, delta) candidates + 5 filter-intra modes of every 16x16 block of a 1080p plane in ONE launch
  cfl_pred             8x8 chroma blocks of the matching 4:2:0 planes, Cb and Cr targets sharing the AC values, luma read from the plane above
  inter_pred_copy      svt_hip_inter_pred_batch's copy case on the same 16x16 blocks, in THIS process on THIS card: the memory-bound yardstick of DESIGN 4.20
  cpu reference        the reference's C functions (oracle/_ref/libsvtref.so) on 16 host threads, one ctypes call per 16x16 block of a 1080p plane, from prepared
                       edges: svt_av1_dr_prediction_z1_c, svt_aom_paeth_predictor_16x16_c, svt_aom_dc_predictor_16x16_c, svt_av1_filter_intra_predictor_c
Every GPU leg's output is compared with tests/intrapred_common.py (every 37th block) BEFORE it is timed; a difference ends the tool with status 1.  Every GPU leg takes
the median of `steps` launches, each between its own pair of HIP events, TWICE (`us_runs`).  Algorithmic bytes per block: (w * h written + 2 (w + h) + 1 read) *
bytes-per-sample; the memory floor is the store.  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
PAD = 16
LINES = []


def event_time(torch, fn, steps, warmup):
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
    return t[len(t) // 2], t


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def timed(torch, fn, a):
    runs = [event_time(torch, fn, a.steps, a.warmup) for _ in range(2)]
    t = sorted(runs[0][1] + runs[1][1])
    return t[len(t) // 2], [round(r[0] * 1e6, 1) for r in runs], round(min(r[1][0] for r in runs) * 1e6, 1)


CLASSES = {"dc": (0, 0, 5, 16), "v": (1, 0, 5, 16), "h": (2, 0, 5, 16), "smooth": (9, 0, 5, 16), "paeth": (12, 0, 5, 16), "z1": (3, 1, 5, 16), "z2": (4, -2, 5, 16),
           "z3": (7, 1, 5, 16), "z1_up": (8, 1, 5, 8), "z2_up": (5, 1, 5, 8), "filter_intra": (0, 0, 0, 16)}  # name -> (mode, delta, filter_intra_mode, block size)


def descs(pkg, W, H, stride, bs, cands):
    """one descriptor per (block, candidate): neighbours in place from the padded plane, output packed candidate-major"""
    by, bx = (v.reshape(-1) for v in np.mgrid[0:H // bs, 0:W // bs])
    nb, nc = len(by), len(cands)
    d = np.zeros(nb * nc, pkg.IntraPredDesc)
    y, x = np.tile(PAD + by * bs, nc), np.tile(PAD + bx * bs, nc)
    d["top_off"], d["left_off"], d["left_stride"] = (y - 1) * stride + x, y * stride + x - 1, stride
    d["dst_off"], d["dst_stride"] = np.repeat(np.arange(nc, dtype=np.int64), nb) * (W * H) + np.tile(by * bs * W + bx * bs, nc), W
    d["w"] = d["h"] = d["n_top_px"] = d["n_topright_px"] = d["n_left_px"] = d["n_bottomleft_px"] = bs
    for k, (m, dl, fi) in enumerate(cands):
        d["mode"][k * nb:(k + 1) * nb], d["angle_delta"][k * nb:(k + 1) * nb], d["filter_intra_mode"][k * nb:(k + 1) * nb] = m, dl, fi
    return d, nb


def check(ic, plane, d, out, W, H, bs, bd, what):
    stride = plane.shape[1]
    for i in range(0, len(d), 37):
        ty, tx = divmod(int(d[i]["top_off"]), stride)
        c, o = divmod(int(d[i]["dst_off"]), W * H)
        oy, ox = divmod(o, W)
        want = ic.build_intra_predictors(plane[ty, tx - 1:tx + 2 * bs], plane[ty + 1:ty + 1 + 2 * bs, tx - 1], bs, bs, int(d[i]["mode"]), int(d[i]["angle_delta"]),
                                         int(d[i]["filter_intra_mode"]), bs, bs, bs, bs, 0, 0, bd)
        if not np.array_equal(out[c, oy:oy + bs, ox:ox + bs], want):
            raise SystemExit("intrapred_timing: parity failure (%s, bd %d, descriptor %d)" % (what, bd, i))


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("intrapred_timing: no GPU -- nothing here is measurable on a CPU")
    import interpred_common as pc
    import intrapred_common as ic
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    g = np.random.default_rng(41)
    scan = [(m, dl, 5) for m in range(13) for dl in (range(-3, 4) if 1 <= m <= 8 else (0,))] + [(0, 0, fi) for fi in range(5)]
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        dt = np.uint16 if px == 2 else np.uint8
        for (name, W, H) in (("1080p", 1920, 1080), ("4k", 3840, 2160)):
            stride = W + 2 * PAD + 5
            plane = g.integers(0, 1 << bd, (H + 2 * PAD, stride)).astype(dt)
            dp = torch.from_numpy(plane.view(np.uint8).reshape(-1).copy()).cuda()
            planes = pkg.IntraPredPlanes()
            planes.base[0] = dp.data_ptr()
            legs = [(k, [v[:3]], v[3]) for k, v in CLASSES.items()] + ([("scan66", scan, 16)] if name == "1080p" else [])
            for (leg, cands, bs) in legs:
                if a.only and a.only not in leg:
                    continue
                d, nb = descs(pkg, W, H, stride, bs, cands)
                n = len(d)
                dd = torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()
                out = torch.zeros(len(cands) * W * H * px, dtype=torch.uint8, device="cuda")
                st = torch.zeros(n, dtype=torch.uint8, device="cuda")
                fn = lambda: lib.svt_hip_intra_pred_batch(planes, out.data_ptr(), dd.data_ptr(), n, bd, st.data_ptr(), stream)  # noqa: E731  (the asynchronous form)
                assert fn() == 0
                torch.cuda.synchronize()
                assert not bool(st.any())
                check(ic, plane, d, out.cpu().numpy().view(dt).reshape(len(cands), H, W), W, H, bs, bd, leg)
                med, runs, mn = timed(torch, fn, a)
                nbytes = n * (bs * bs + 4 * bs + 1) * px
                emit(leg="intra_scan66_16x16" if leg == "scan66" else "intra_pred_%s_%dx%d" % (leg, bs, bs), kind="gpu", bd=bd, picture=name, blocks=nb, descriptors=n,
                     us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4),
                     Msamples_per_s=round(n * bs * bs / med / 1e6), parity="every 37th descriptor == tests/intrapred_common.py")
                del dd, out, st
            # CfL on the matching chroma planes: 8x8 chroma blocks, luma 16x16 from the plane above, Cb and Cr DC predictions in one packed plane each
            cw, ch, bs = W // 2, H // 2, 8
            by, bx = (v.reshape(-1) for v in np.mgrid[0:ch // bs, 0:cw // bs])
            n = len(by)
            dc_pred = g.integers(0, 1 << bd, (2, ch, cw)).astype(dt)
            dcp = torch.from_numpy(dc_pred.view(np.uint8).reshape(-1).copy()).cuda()
            planes.base[1] = dcp.data_ptr()
            cd = np.zeros(n, pkg.CflPredDesc)
            cd["luma_off"], cd["luma_stride"] = (PAD + 2 * by * bs) * stride + PAD + 2 * bx * bs, stride
            cd["pred_off"], cd["pred_stride"], cd["pred_plane"] = np.stack([by * bs * cw + bx * bs, ch * cw + by * bs * cw + bx * bs], 1), cw, 1
            cd["dst_off"], cd["dst_stride"], cd["alpha_q3"], cd["w"], cd["h"], cd["n_targets"] = cd["pred_off"], cw, (5, -11), bs, bs, 2
            cdd = torch.from_numpy(cd.view(np.uint8).reshape(-1)).cuda()
            out = torch.zeros(2 * ch * cw * px, dtype=torch.uint8, device="cuda")
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_cfl_pred_batch(planes, out.data_ptr(), cdd.data_ptr(), n, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            o = out.cpu().numpy().view(dt).reshape(2, ch, cw)
            for i in range(0, n, 37):
                y, x = int(by[i]) * bs, int(bx[i]) * bs
                for t, al in enumerate((5, -11)):
                    want = ic.cfl_full(plane[PAD + 2 * y:PAD + 2 * y + 16, PAD + 2 * x:PAD + 2 * x + 16], dc_pred[t, y:y + 8, x:x + 8], 8, 8, al, bd)
                    if not np.array_equal(o[t, y:y + 8, x:x + 8], want):
                        raise SystemExit("intrapred_timing: parity failure (cfl, bd %d, block %d)" % (bd, i))
            med, runs, mn = timed(torch, fn, a)
            nbytes = n * (256 + 4 * 64) * px
            emit(leg="cfl_pred_8x8_two_targets", kind="gpu", bd=bd, picture=name, blocks=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="every 37th block == tests/intrapred_common.py")
            # the copy case of DESIGN 4.20 on the same 16x16 blocks, for scale
            by, bx = (v.reshape(-1) for v in np.mgrid[0:H // 16, 0:W // 16])
            n = len(by)
            idd = np.zeros(n, pkg.InterPredDesc)
            idd["src_off"][:, 0], idd["src_stride"], idd["dst_off"], idd["dst_stride"] = (PAD + by * 16) * stride + PAD + bx * 16, stride, by * 16 * W + bx * 16, W
            idd["w"] = idd["h"] = 16
            idd["filter_x"] = idd["filter_y"] = pc.REGULAR
            ip = pkg.InterPredPlanes()
            ip.base[0] = dp.data_ptr()
            iddd = torch.from_numpy(idd.view(np.uint8).reshape(-1)).cuda()
            out = torch.zeros(W * H * px, dtype=torch.uint8, device="cuda")
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_inter_pred_batch(ip, out.data_ptr(), iddd.data_ptr(), n, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            rows = (H // 16) * 16
            assert np.array_equal(out.cpu().numpy().view(dt).reshape(H, W)[:rows], plane[PAD:PAD + rows, PAD:PAD + W])
            med, runs, mn = timed(torch, fn, a)
            emit(leg="inter_pred_copy_16x16", kind="gpu", bd=bd, picture=name, blocks=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(2 * n * 256 * px / med / 1e9, 1), frac_of_8TBps=round(2 * n * 256 * px / med / HBM, 4), note="svt_hip_inter_pred_batch, same process")
            del dp, dcp, cdd, iddd, out, st
            torch.cuda.empty_cache()


def cpu_legs(a):
    """the reference's C functions on one 1080p plane's worth of 16x16 blocks from prepared edges, 16 threads, one ctypes call per block"""
    path = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    if not os.path.exists(path):
        emit(leg="cpu_intra", kind="reference", note="not measured: oracle/_ref/libsvtref.so is not on this host")
        return
    ref = C.CDLL(path)
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    vp, i32 = C.c_void_p, C.c_int32
    fns = {"svt_av1_dr_prediction_z1_c": ([vp, C.c_ssize_t, i32, i32, vp, vp, i32, i32, i32], lambda d, ab, le: (d, 16, 16, 16, ab, le, 0, 57, 1)),
           "svt_aom_paeth_predictor_16x16_c": ([vp, C.c_ssize_t, vp, vp], lambda d, ab, le: (d, 16, ab, le)),
           "svt_aom_dc_predictor_16x16_c": ([vp, C.c_ssize_t, vp, vp], lambda d, ab, le: (d, 16, ab, le)),
           "svt_av1_filter_intra_predictor_c": ([vp, C.c_ssize_t, C.c_uint8, vp, vp, i32], lambda d, ab, le: (d, 16, 2, ab, le, 0))}
    n = (1920 // 16) * (1080 // 16)
    g = np.random.default_rng(42)
    edges = g.integers(0, 256, (n, 2, 64)).astype(np.uint8)
    dst = np.zeros((n, 256), np.uint8)
    for sym, (argtypes, mk) in fns.items():
        f = getattr(ref, sym)
        f.restype, f.argtypes = None, argtypes

        def work(lo, hi):
            for i in range(lo, hi):
                f(*mk(dst.ctypes.data + i * 256, edges.ctypes.data + i * 128 + 16, edges.ctypes.data + i * 128 + 64 + 16))

        cuts = np.linspace(0, n, 17).astype(int)
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda k: work(cuts[k], cuts[k + 1]), range(16)))
            t0 = time.perf_counter()
            list(ex.map(lambda k: work(cuts[k], cuts[k + 1]), range(16)))
            t = time.perf_counter() - t0
        t0 = time.perf_counter()
        work(0, n)
        t1 = time.perf_counter() - t0
        emit(leg="cpu_" + sym, kind="reference", symbol=sym, library=os.path.relpath(path, ROOT), bd=8, blocks=n, us_per_1080p_plane_16_threads=round(t * 1e6, 1),
             us_per_1080p_plane_1_thread=round(t1 * 1e6, 1), us_per_block_1_thread=round(t1 / n * 1e6, 2), cpus=len(os.sched_getaffinity(0)), host=host,
             note="the reference's C function from prepared edges, one ctypes call per block (about 2 us of call overhead per block; the threads share the interpreter "
                  "between calls); host wall clock")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default="", help="only the intra_pred legs whose class name contains this (the CfL and copy legs always run)")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intrapred_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
