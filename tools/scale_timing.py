#!/usr/bin/env python3
"""Event timing of the scaled-prediction, resize and upscale kernels (csrc/scale.hip).  Standalone: imports the package and bench.py's helpers, changes neither.  Prints
one JSON object per line and writes the same lines to profiles/scale_timing.txt (--out).

  python tools/scale_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--reference-only] [--out FILE]

Legs (8 and 10 bit)
  sad64x64_pairs   bench.py's own leg, in THIS process on THIS card: the yardstick ("memory-bound done well") the fractions stand next to
  scaled_pred      svt_hip_inter_pred_scaled_batch on 65 280 blocks of 64x64 in one launch, one reference, steps 2048 / 2048 and 1150 / 1150
  resize           svt_hip_resize_plane_batch on a 3840 x 2160 plane at denominators 9 and 16 (width and height through calculate_scaled_size_helper)
  upscale          svt_hip_superres_upscale_batch on the three planes of a 4:2:0 picture whose up-scaled luma is 3840 x 2160, denominators 9 and 16
  cpu legs         `kind: reference`: the `_c` functions of oracle/_ref/libsvtref.so (svt_av1_[highbd_]convolve_2d_scale_c per block, svt_av1_[highbd_]resize_plane_c
                   per plane) from 16 host threads at once and from one; host wall clock, the host named.
Outputs are compared with tests/scale_common.py before anything is timed.  Every GPU leg takes the median of `steps` calls, each between its own pair of HIP events,
TWICE: `us_runs` holds both medians.  Algorithmic bytes: every output sample written once and every source sample the outputs cover read once (prediction: the
stepped extent of each block; resize / upscale: the source planes).  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
NB, COLS, BS = 65280, 256, 64
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


def timed(torch, fn, a):
    runs = [event_time(torch, fn, a.steps, a.warmup) for _ in range(2)]
    t = sorted(runs[0][1] + runs[1][1])
    return t[len(t) // 2], [round(r[0] * 1e6, 1) for r in runs], round(min(r[1][0] for r in runs) * 1e6, 1)


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scale_timing: no GPU -- nothing here is measurable on a CPU")
    import bench
    import scale_common as sc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every call, median of steps, twice (us_runs)")
    r = bench.bench_sad_pairs(torch, lib, pkg, stream, SimpleNamespace(min_leg_s=0.5), False)
    emit(leg="sad64x64_pairs", kind="gpu", note="bench.py's leg, same process", blocks=240 * 510, us_per_launch=round(r["roofline"]["kernel_us"], 1),
         algorithmic_GBps=round(r["roofline"]["achieved"], 1), frac_of_8TBps=r["roofline"].get("frac"))
    g = np.random.default_rng(47)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        dt = np.uint16 if px == 2 else np.uint8
        # scaled prediction: block (by, bx) of the 64x64 grid predicts from where the stepped grid puts it in a reference of the scaled size
        for step in (2048, 1150):
            ext = ((BS - 1) * step + 1023 >> 10) + 8
            by, bx = (v.reshape(-1) for v in np.mgrid[0:NB // COLS, 0:COLS])
            Wr, Hr = (COLS * BS * step >> 10) + ext + 8, ((NB // COLS) * BS * step >> 10) + ext + 8
            hR = g.integers(0, 1 << bd, (Hr, Wr), dtype=dt)
            R = up(hR)
            planes = pkg.InterPredPlanes()
            planes.base[0] = R.data_ptr()
            Wd = COLS * BS
            out = torch.zeros(Wd * (NB // COLS) * BS * px, dtype=torch.uint8, device="cuda")
            d = np.zeros(NB, pkg.ScaledPredDesc)
            oy, ox = 3 + (by * BS * step >> 10), 3 + (bx * BS * step >> 10)
            d["src_off"][:, 0], d["src_stride"][:, 0], d["dst_off"], d["dst_stride"] = (oy * Wr + ox).astype(np.uint64), Wr, (by * BS * Wd + bx * BS).astype(np.uint64), Wd
            d["w"] = d["h"] = BS
            d["xs"][:, 0] = d["ys"][:, 0] = step
            d["subpel_x"][:, 0], d["subpel_y"][:, 0], d["filter_x"], d["filter_y"] = (bx * 37) % 1024, (by * 53) % 1024, 2, 0
            dd, st = up(d), torch.zeros(NB, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_inter_pred_scaled_batch(planes, out.data_ptr(), dd.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert not bool(st.any())
            got = out.cpu().numpy().view(dt).reshape(-1, Wd)
            for i in list(range(0, NB, NB // 9)) + [NB - 1]:  # outputs before timing
                want = sc.scaled_pred([(hR, int(oy[i]), int(ox[i]), int(d["subpel_x"][i, 0]), int(d["subpel_y"][i, 0]), step, step)], BS, BS, 2, 0, bd)
                y, x = int(by[i]) * BS, int(bx[i]) * BS
                if not np.array_equal(got[y:y + BS, x:x + BS], want):
                    raise SystemExit("scale_timing: parity failure (prediction, bd %d, step %d, block %d)" % (bd, step, i))
            med, runs, mn = timed(torch, fn, a)
            nbytes = NB * px * (BS * BS + ((BS * step >> 10) ** 2))
            emit(leg="scaled_pred_64x64", kind="gpu", bd=bd, step=step, blocks=NB, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 ns_per_block=round(med / NB * 1e9, 2), algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4),
                 parity="10 blocks == tests/scale_common.py")
            del R, out, dd
            torch.cuda.empty_cache()
        W, H = 3840, 2160
        hP = g.integers(0, 1 << bd, (H, W), dtype=dt)
        P = up(hP)
        for denom in (9, 16):
            W2, H2 = sc.scaled_size(W, denom), sc.scaled_size(H, denom)
            # resize: the source picture down to the coded size
            d = np.zeros(1, pkg.ResizeDesc)
            out = torch.zeros(W2 * H2 * px, dtype=torch.uint8, device="cuda")
            d["src"], d["dst"], d["width"], d["height"], d["in_stride"], d["width2"], d["height2"], d["out_stride"] = P.data_ptr(), out.data_ptr(), W, H, W, W2, H2, W2
            need = lib.svt_hip_resize_workspace_bytes(d.ctypes.data, 1, bd)
            ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_resize_plane_batch(d.ctypes.data, 1, bd, ws.data_ptr(), need, stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(dt).reshape(H2, W2)
            if not np.array_equal(got[:, :64], sc.resize_plane(hP, W2, H2, bd)[:, :64]):
                raise SystemExit("scale_timing: parity failure (resize, bd %d, denominator %d)" % (bd, denom))
            med, runs, mn = timed(torch, fn, a)
            nbytes = px * (W * H + W2 * H2)
            emit(leg="resize_4k", kind="gpu", bd=bd, denominator=denom, size="%dx%d -> %dx%d" % (W, H, W2, H2), us_per_call=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="64 columns of every row == tests/scale_common.py",
                 workspace_bytes=int(need))
            del ws
            # upscale: the three planes of the coded picture back to 3840 wide
            d = np.zeros(3, pkg.UpscaleDesc)
            keep, nbytes, checks = [], 0, []
            for i, sub in enumerate((0, 1, 1)):
                down, upw, starts, mi_cols, _ = sc.upscale_geometry(W, denom, sub, 4)
                last, rows = starts[-1] << (2 - sub), (H + sub) >> sub
                hs = g.integers(0, 1 << bd, (rows, last), dtype=dt)
                s_, o_ = up(hs), torch.zeros(rows * upw * px, dtype=torch.uint8, device="cuda")
                keep.append((s_, o_))
                d["src"][i], d["dst"][i], d["src_stride"][i], d["dst_stride"][i], d["rows"][i] = s_.data_ptr(), o_.data_ptr(), last, upw, rows
                d["downscaled_plane_width"][i], d["upscaled_plane_width"][i], d["superres_denom"][i], d["sub_x"][i], d["bd"][i] = down, upw, denom, sub, bd
                d["sample_bytes"][i], d["n_tile_cols"][i] = px, len(starts) - 1
                d["tile_col_start_mi"][i, :len(starts)] = starts
                nbytes += px * rows * (down + upw)
                checks.append((hs, down, upw, sub, starts))
            fn = lambda: lib.svt_hip_superres_upscale_batch(d.ctypes.data, 3, stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            for (hs, down, upw, sub, starts), (s_, o_) in zip(checks, keep):
                got = o_.cpu().numpy().view(dt).reshape(-1, upw)
                if not np.array_equal(got[:32], sc.upscale_rows(hs[:32], down, upw, denom, sub, starts, bd)):
                    raise SystemExit("scale_timing: parity failure (upscale, bd %d, denominator %d)" % (bd, denom))
            med, runs, mn = timed(torch, fn, a)
            emit(leg="upscale_4k", kind="gpu", bd=bd, denominator=denom, planes=3, tile_cols=4, us_per_call=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="32 rows of every plane == tests/scale_common.py")
            del keep, out
        del P
        torch.cuda.empty_cache()


def threaded(fn, threads, calls):
    """wall time of `threads` host threads each calling fn(thread index) `calls` times (ctypes releases the interpreter lock for the call)"""
    def body(k):
        for _ in range(calls):
            fn(k)
    ts = [threading.Thread(target=body, args=(k,)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return time.perf_counter() - t0


def cpu_legs(a):
    import scale_common as sc
    path = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    if not os.path.exists(path):
        emit(leg="cpu_scale", kind="reference", note="not measured: oracle/_ref/libsvtref.so is not on this host")
        return
    lib = C.CDLL(path)
    lib.svt_aom_setup_common_rtcd_internal(C.c_uint64(0))
    lib.svt_aom_setup_rtcd_internal(C.c_uint64(0))  # every dispatch pointer = its C function
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    vp = C.c_void_p
    g = np.random.default_rng(48)
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        pic = g.integers(0, 1 << bd, (160, 160)).astype(dt)
        px_, keep = sc.filter_params(sc.filter_rows(2, BS))
        py_, keep2 = sc.filter_params(sc.filter_rows(0, BS))
        f = getattr(lib, "svt_av1_%sconvolve_2d_scale_c" % ("highbd_" if bd > 8 else ""))
        f.restype = None
        for step in (2048, 1150):
            dsts = [np.zeros((BS, BS), dt) for _ in range(16)]
            cps = [sc.ConvolveParams(0, 0, None, 0, 3, 11, 0, 0, 0, 0, 0, 0) for _ in range(16)]

            def call(k):
                args = [vp(pic.ctypes.data + (3 * 160 + 3) * pic.itemsize), 160, vp(dsts[k].ctypes.data), BS, BS, BS, C.byref(px_), C.byref(py_), 37, step, 53, step, C.byref(cps[k])]
                f(*(args + ([bd] if bd > 8 else [])))
            call(0)
            if not np.array_equal(dsts[0], sc.scaled_pred([(pic, 3, 3, 37, 53, step, step)], BS, BS, 2, 0, bd)):
                raise SystemExit("scale_timing: the reference's convolve_2d_scale and tests/scale_common.py DIFFER")
            calls = 400
            t16, t1 = threaded(call, 16, calls), threaded(call, 1, calls)
            emit(leg="cpu_scaled_pred_64x64", kind="reference", symbol=f.__name__, library=os.path.relpath(path, ROOT), bd=bd, step=step, threads=16, calls_per_thread=calls,
                 ns_per_block_16_threads=round(t16 / (16 * calls) * 1e9, 1), ns_per_block_1_thread=round(t1 / calls * 1e9, 1), cpus=len(os.sched_getaffinity(0)), host=host,
                 note="one foreign call per block; host wall clock")
        W, H = 3840, 2160
        src = g.integers(0, 1 << bd, (H, W)).astype(dt)
        f = lib.svt_av1_highbd_resize_plane_c if bd > 8 else lib.svt_av1_resize_plane_c
        for denom in (9, 16):
            W2, H2 = sc.scaled_size(W, denom), sc.scaled_size(H, denom)
            outs = [np.zeros((H2, W2), dt) for _ in range(16)]

            def rcall(k):
                args = [vp(src.ctypes.data), H, W, W, vp(outs[k].ctypes.data), H2, W2, W2]
                f(*(args + ([bd] if bd > 8 else [])))
            t16, t1 = threaded(rcall, 16, 1), threaded(rcall, 1, 1)
            if not np.array_equal(outs[0][:, :64], sc.resize_plane(src, W2, H2, bd)[:, :64]):
                raise SystemExit("scale_timing: the reference's resize_plane and tests/scale_common.py DIFFER")
            emit(leg="cpu_resize_4k", kind="reference", symbol=f.__name__, library=os.path.relpath(path, ROOT), bd=bd, denominator=denom, threads=16,
                 ms_per_plane_16_threads=round(t16 / 16 * 1e3, 2), ms_per_plane_1_thread=round(t1 * 1e3, 2), cpus=len(os.sched_getaffinity(0)), host=host,
                 note="16 planes at once, one per thread; host wall clock")
    emit(leg="cpu_upscale_4k", kind="reference", note="not measured: svt_av1_upscale_normative_rows takes an Av1Common and is reached through a compiled harness only "
         "(tests/scale_ref_harness.c)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
