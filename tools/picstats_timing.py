#!/usr/bin/env python3
"""Event timing of the picture-statistics kernels (csrc/picstats.hip).  Standalone: imports the package and bench.py's helpers, changes neither.  Prints one JSON
object per line and writes the same lines to profiles/picstats_timing.txt (--out).

  python tools/picstats_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--reference-only] [--out FILE]

Legs
  sad64x64_pairs     bench.py's own leg, in THIS process on THIS card: the yardstick the variance fractions stand next to
  picture_variance   a 32-picture 1920x1080 batch (68-pixel padding, bench.py's plane; 80 MB, which the 256 MiB Infinity Cache holds), the same as 128 pictures
                     (320 MB: the figure that is about HBM) and one 3840x2160 plane; both precisions; us per call (two launches: the table,
                     then pic_avg_variance) and the fraction of 8 TB/s for the bytes read once (64 x 64 per superblock at FULL, every other row at SUB -- the bytes
                     the algorithm needs, not the sectors the rows drag in) + the 170-byte table row written
  variance_boost     510 and 2 040 superblocks (1080p, 4K); us per call (two launches; the host-built table is cached after the first call)
  picture_histogram  a 480x270 plane (the 1/16 plane of 1080p), 4x4 regions, decim_step 1 and 4; us per call (two launches)
  cpu reference      svt_aom_gathering_picture_statistics and svt_variance_adjust_qp of the reference on 16 host threads, through tests/picstats_ref_harness.c -- compiled
                     here when the reference's headers and oracle/_ref/libsvtref.so are on the machine; `kind: reference`, host wall clock, the host is named
Every GPU leg is checked against tests/picstats_common.py before a number is recorded."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
LINES = []


def event_time(torch, fn, steps, warmup):
    """median and minimum seconds per call: `steps` calls, each between its own pair of events, after `warmup` calls"""
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
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def padded(g, w, h, pad):
    """a padded 8-bit plane of low-variance content (a gradient + noise of 0 .. 6 per superblock column), edges not replicated: any readable content times the same"""
    stride, rows = w + 2 * pad, h + 2 * pad
    yy, xx = np.mgrid[0:rows, 0:stride]
    amp = (xx // 64) % 7
    return ((xx // 16 + yy // 32) % 200 + 20 + (g.integers(-6, 7, (rows, stride)) * amp) // 6).astype(np.uint8), stride


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("picstats_timing: no GPU -- the kernel legs are not measurable on a CPU (--reference-only runs the host leg alone)")
    import bench
    import picstats_common as pc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every call, median of steps")
    r = bench.bench_sad_pairs(torch, lib, pkg, stream, SimpleNamespace(min_leg_s=0.5), False)
    emit(leg="sad64x64_pairs", kind="gpu", note="bench.py's leg, same process", blocks=240 * 510, us_per_launch=round(r["roofline"]["kernel_us"], 1),
         algorithmic_GBps=round(r["roofline"]["achieved"], 1), frac_of_8TBps=r["roofline"].get("frac"))
    g = np.random.default_rng(5)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    tables = {}
    for name, w, h, pad, n_pics in (("1080p_x32", 1920, 1080, bench.PAD, 32), ("1080p_x128", 1920, 1080, bench.PAD, 128), ("2160p_x1", 3840, 2160, bench.PAD, 1)):
        plane, stride = padded(g, w, h, pad)
        # the readable extent of the last superblock row / column: 64 * ceil(h / 64) rows from the origin fit inside the padding here (1088 <= 1080 + 68)
        assert 64 * ((h + 63) // 64) <= h + pad and 64 * ((w + 63) // 64) <= w + pad
        pitch = plane.size
        d_in = dev(np.tile(plane.reshape(-1), n_pics))
        n_sb = ((w + 63) // 64) * ((h + 63) // 64)
        d_var, d_avg = torch.zeros(n_pics * n_sb * 85 * 2, dtype=torch.uint8, device="cuda"), torch.zeros(n_pics * 2, dtype=torch.uint8, device="cuda")
        for prec, pname in ((pc.PREC_SUB, "sub"), (pc.PREC_FULL, "full")):
            fn = lambda: lib.svt_hip_picture_variance_batch(d_in.data_ptr(), pitch, stride, pad, pad, w, h, n_pics, prec, 1, d_var.data_ptr(), d_avg.data_ptr(), stream)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            want, wavg = pc.picture_variance(plane, pad, pad, w, h, prec)
            got = d_var.cpu().numpy().view(np.uint16).reshape(n_pics, n_sb, 85)
            if not (np.array_equal(got[0], want) and np.array_equal(got[-1], want) and int(d_avg.cpu().numpy().view(np.uint16)[-1]) == wavg):
                raise SystemExit("picstats_timing: parity failure (variance, %s, %s)" % (name, pname))
            if prec == pc.PREC_SUB:
                tables[name] = (want, d_var[:n_sb * 85 * 2].clone())
            med, best = event_time(torch, fn, a.steps, a.warmup)
            nbytes = n_pics * n_sb * (64 * 64 // (2 if prec == pc.PREC_SUB else 1) + 170)
            emit(leg="picture_variance", kind="gpu", shape=name, prec=pname, superblocks=n_pics * n_sb, launches=2, us_per_call=round(med * 1e6, 1), us_min=round(best * 1e6, 1),
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), footprint_MB=round(n_pics * pitch / 1e6, 1),
                 parity="first and last picture == tests/picstats_common.py")
        del d_in
    gold = np.load(os.path.join(ROOT, "tests", "golden", "picstats.npz"))
    q = gold["q_fp8_8"]
    for name in ("1080p_x32", "2160p_x1"):
        var, d_var = tables[name]
        n_sb = var.shape[0]
        qin = g.integers(60, 200, n_sb).astype(np.uint8)
        d_qin, d_out, d_frame = dev(qin), torch.zeros(n_sb, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda")
        fn = lambda: lib.svt_hip_variance_boost_qindex(d_var.data_ptr(), d_qin.data_ptr(), n_sb, 128, 2, 6, 0, 8, q.ctypes.data, d_out.data_ptr(), d_frame.data_ptr(), stream)  # noqa: E731
        fn()
        torch.cuda.synchronize()
        want, base, _, _, boost = pc.variance_boost(var, qin, 128, 2, 6, 0, q)
        if not (np.array_equal(d_out.cpu().numpy(), want) and int(d_frame.cpu().numpy().view(np.int32)[0]) == base):
            raise SystemExit("picstats_timing: parity failure (boost, %d superblocks)" % n_sb)
        med, best = event_time(torch, fn, a.steps, a.warmup)
        emit(leg="variance_boost", kind="gpu", superblocks=n_sb, launches=2, us_per_call=round(med * 1e6, 1), us_min=round(best * 1e6, 1),
             superblocks_boosted=int(np.count_nonzero(boost)), parity="qindex_out and normalized base == tests/picstats_common.py")
    pic = g.integers(0, 256, (270, 480)).astype(np.uint8)
    d_pic, d_h, d_a, d_l = dev(pic), torch.zeros(16 * 256 * 4, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")
    for decim in (1, 4):
        fn = lambda: lib.svt_hip_picture_histogram(d_pic.data_ptr(), 480, 480, 270, 4, 4, decim, d_h.data_ptr(), d_a.data_ptr(), d_l.data_ptr(), stream)  # noqa: E731
        fn()
        torch.cuda.synchronize()
        wh, wa, wl = pc.picture_histogram(pic, 4, 4, decim)
        if not (np.array_equal(d_h.cpu().numpy().view(np.uint32).reshape(4, 4, 256), wh) and np.array_equal(d_a.cpu().numpy().reshape(4, 4), wa)
                and int(d_l.cpu().numpy().view(np.uint64)[0]) == wl):
            raise SystemExit("picstats_timing: parity failure (histogram, decim %d)" % decim)
        med, best = event_time(torch, fn, a.steps, a.warmup)
        emit(leg="picture_histogram", kind="gpu", plane="480x270", regions="4x4", decim_step=decim, launches=2, us_per_call=round(med * 1e6, 1), us_min=round(best * 1e6, 1),
             parity="histogram, region averages and avg_luma == tests/picstats_common.py")


def cpu_legs():
    """the reference's two exported callers on 16 threads, one picture per call"""
    ref_lib = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    src = os.path.join(os.environ.get("SVT_REF", "/root/reference"), "Source")
    if not (os.path.exists(ref_lib) and os.path.isfile(os.path.join(src, "Lib", "Codec", "pcs.h"))):
        emit(leg="cpu_reference", kind="reference", note="not measured: the reference's headers or oracle/_ref/libsvtref.so are not on this host")
        return
    import picstats_common as pc
    tmp = tempfile.mkdtemp(prefix="picstats_timing_")
    out = os.path.join(tmp, "libpicstats_harness.so")
    inc = ["-I" + os.path.join(src, d) for d in ("API", os.path.join("Lib", "Codec"), os.path.join("Lib", "C_DEFAULT"), os.path.join("Lib", "Globals"))]
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *inc, os.path.join(ROOT, "tests", "picstats_ref_harness.c"), "-o", out,
                    "-L" + os.path.dirname(ref_lib), "-lsvtref", "-Wl,-rpath," + os.path.dirname(ref_lib)], check=True)
    h = C.CDLL(out)
    h.harness_init()

    class Plane(C.Structure):
        _fields_ = [("buffer", C.c_void_p), ("stride", C.c_uint32), ("org_x", C.c_uint32), ("org_y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]
    h.harness_picture_statistics.argtypes = [C.POINTER(Plane), C.POINTER(Plane)] + [C.c_int] * 5 + [C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 5
    h.harness_variance_adjust_qp.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_int] * 5
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    g = np.random.default_rng(5)
    note = "the reference's C functions (svt_aom_setup_rtcd_internal(0)); host wall clock"
    for name, w, hgt, n_pics in (("1080p_x32", 1920, 1080, 32), ("2160p_x1", 3840, 2160, 16)):
        plane, stride = padded(g, w, hgt, 68)
        six = g.integers(0, 256, (hgt // 4, w // 4)).astype(np.uint8)
        n_sb = ((w + 63) // 64) * ((hgt + 63) // 64)
        var = [np.zeros((n_sb, 85), np.uint16) for _ in range(16)]
        qin = g.integers(60, 200, n_sb).astype(np.uint8)

        def stats(i, calc_hist, calc_var):
            pl, sx = Plane(plane.ctypes.data, stride, 68, 68, w, hgt), Plane(six.ctypes.data, six.shape[1], 0, 0, six.shape[1], six.shape[0])
            o = [np.zeros(1, np.uint16), np.zeros(16 * 256, np.uint32), np.zeros(16, np.uint64), np.zeros(1, np.uint64)]
            h.harness_picture_statistics(C.byref(pl), C.byref(sx), pc.PREC_SUB, 0, 6, calc_hist, calc_var, 4, 4, 1, var[i % 16].ctypes.data, *(x.ctypes.data for x in o))

        def boost(i):
            q = qin.copy()
            h.harness_variance_adjust_qp(var[i % 16].ctypes.data, q.ctypes.data, n_sb, 128, 2, 6, 0, 8)

        for leg, fn in (("picture_variance", lambda i: stats(i, 0, 1)), ("picture_histogram", lambda i: stats(i, 1, 0)), ("variance_boost", boost)):
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(fn, range(16)))
                t0 = time.perf_counter()
                list(ex.map(fn, range(n_pics * 4)))
                dt = time.perf_counter() - t0
            emit(leg="cpu_" + leg, kind="reference", shape="%dx%d" % ((w // 4, hgt // 4) if leg == "picture_histogram" else (w, hgt)), threads=16, pictures=n_pics * 4,
                 us_per_picture=round(dt / (n_pics * 4) * 1e6, 1), us_for_the_gpu_leg_shape=round(dt / (n_pics * 4) * 1e6 * (n_pics if name == "1080p_x32" else 1), 1),
                 host=host, note=note)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="the host leg alone (needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picstats_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
