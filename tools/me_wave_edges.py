#!/usr/bin/env python3
"""Fixed cost of a launch of me_fullpel_wave_kernel: how much of the time is the fill and the drain of the device, and how much is steady state.

  python tools/me_wave_edges.py [--area 16x9] [--min-s 0.3] [--no-pmc] [--out FILE]

Calls svt_hip_me_fullpel_search_batch on the synthetic planes of bench.py with item counts n = 5 120 x {1, 2, 4, 8} and the benchmark's 65 280 (5 120 = one resident
round: 256 CUs x 5 workgroups x 4 waves), every point event-timed over at least --min-s seconds after a warm-up of the same length (the median of five batches), fits
t(n) = a + b n by least squares and prints a (what a launch costs however many items it has: fill + drain), b and the residuals.  Then one counter pass of the
headline in a child process of its own (rocprofv3 --kernel-trace --pmc, no other tracing; the counters are split over two children if one pass does not take them).
The descriptors of a point are the first n of the benchmark's table, so every point reads the same planes as the headline does.
"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (constants and the plane generator of the benchmark; nothing of it runs on import)

ROUND = 5120
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_LDS"]
PMC_LAUNCHES = 8


def workload(a):
    import torch
    pkg = bench.entry._pkg()
    lib = pkg.load(init_device=0)
    aw, ah = (int(v) for v in a.area.split("x"))
    planes = bench.synth_planes(a.frames + a.refs, 1234)
    descs = np.concatenate([pkg.me_descs_for_frame(bench.W, bench.H, bench.STRIDE, bench.PAD, bench.PAD, aw, ah, bench.PLANE, n_refs=a.refs, src_plane=f, ref_plane0=f + 1)
                            for f in range(a.frames)])
    n = len(descs)
    d_planes = torch.from_numpy(planes.reshape(-1)).cuda()
    d_descs = torch.from_numpy(descs.view(np.uint8)).cuda()
    d_sad = torch.zeros(n * 85, dtype=torch.int32, device="cuda")
    d_mv = torch.zeros(n * 85, dtype=torch.int32, device="cuda")
    ws_bytes = lib.svt_hip_me_fullpel_search_workspace(n, aw, ah)
    d_ws = torch.zeros(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch(nn):
        lib.svt_hip_me_fullpel_search_batch(d_planes.data_ptr(), d_planes.data_ptr(), d_descs.data_ptr(), nn, aw, ah, 0, d_sad.data_ptr(), d_mv.data_ptr(),
                                            d_ws.data_ptr() if ws_bytes else None, stream)
    return torch, launch, n


def time_point(torch, fn, min_s, batches=5):
    """Seconds per launch: `batches` event-timed batches that last min_s together, after a warm-up as long, the median batch."""
    t = bench.calibrate_launches(torch, fn, batches, min_s)
    reps = max(t, 3)
    for _ in range(reps * batches):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3 / reps)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts), reps


def sweep(a, out):
    torch, launch, n_all = workload(a)
    points = [ROUND * k for k in (1, 2, 4, 8) if ROUND * k < n_all] + [n_all]
    rows = []
    for nn in points:
        med, lo, hi, reps = time_point(torch, lambda nn=nn: launch(nn), a.min_s)
        rows.append((nn, med, lo, hi, reps))
    x, y = np.array([r[0] for r in rows], float), np.array([r[1] for r in rows], float) * 1e6
    b, a0 = np.polyfit(x, y, 1)
    out("sweep at %s, %d resident waves per round, each point >= %.1f s in five batches after a warm-up as long; us per launch" % (a.area, ROUND, a.min_s))
    out("        n   rounds    median      min      max   launches/batch   fit a + b n   residual")
    for (nn, med, lo, hi, reps) in rows:
        fit = a0 + b * nn
        out("  %7d   %6.2f   %7.2f  %7.2f  %7.2f   %6d          %8.2f    %+6.2f" % (nn, nn / ROUND, med * 1e6, lo * 1e6, hi * 1e6, reps, fit, med * 1e6 - fit))
    head = rows[-1][1] * 1e6
    out("fit: a = %.2f us per launch (fill + drain), b = %.4f us per 1 000 items = %.2f us per resident round; a is %.2f %% of the %.1f us headline" %
        (a0, b * 1e3, b * ROUND, 100 * a0 / head, head))
    out("     one round alone takes %.2f us = %.2f x b x 5 120: the price of a round that nothing overlaps" % (rows[0][1] * 1e6, rows[0][1] * 1e6 / (b * ROUND)))
    if a0 < 0.01 * head:
        out("     a is under 1 %% of the headline: the start-up and the drain of a launch are not where the time is")


def pmc_child(a):
    torch, launch, n_all = workload(a)
    for _ in range(PMC_LAUNCHES):
        launch(n_all)
    torch.cuda.synchronize()


def pmc_pass(a, ctrs):
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    td = tempfile.mkdtemp(prefix="me_edges_")
    try:
        cmd = [rp, "--kernel-trace", "--pmc"] + ctrs + ["--output-format", "csv", "-d", td, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--pmc-child",
               "--area", a.area, "--frames", str(a.frames), "--refs", str(a.refs)]
        r = subprocess.run(cmd, capture_output=True, timeout=300)
        files = glob.glob(os.path.join(td, "**", "*counter_collection.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, r.stderr.decode(errors="replace")[-600:]
        tot, disp = {}, set()
        for row in csv.DictReader(open(files[0])):
            if "me_fullpel_wave_kernel" not in row["Kernel_Name"]:
                continue
            disp.add(row["Dispatch_Id"])
            tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        return {c: v / max(len(disp), 1) for c, v in tot.items()}, len(disp)
    finally:
        shutil.rmtree(td, ignore_errors=True)


def counters(a, out):
    got, note = pmc_pass(a, COUNTERS)
    passes = "one pass"
    if got is None or any(c not in got for c in COUNTERS):  # more counters than one pass takes: two children, SQ_WAVES in both
        half = len(COUNTERS) // 2
        got, passes = {}, "two passes"
        for ctrs in (COUNTERS[:half] + ["SQ_WAVES"], [c for c in COUNTERS[half:] if c != "SQ_WAVES"] + ["SQ_WAVES"]):
            g, note = pmc_pass(a, ctrs)
            if g is None:
                out("counter pass %s failed: %s" % (" ".join(ctrs), note))
                return
            got.update(g)
    w = got.get("SQ_WAVES", 0.0) or 1.0
    out("counters of me_fullpel_wave_kernel at %s, per launch, mean of the launches of a child run of its own (rocprofv3 --kernel-trace --pmc, %s):" % (a.area, passes))
    for c in COUNTERS:
        if c in got:
            out("  %-22s %16.0f   / SQ_WAVES = %10.1f" % (c, got[c], got[c] / w))
    if all(c in got for c in ("SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU")):
        wc = got["SQ_WAVE_CYCLES"]
        out("  of a wave's resident cycles: waiting for anything %.1f %%, waiting for an instruction to issue %.1f %%; SQ_ACTIVE_INST_VALU x 4 / waves = %.0f cycles" %
            (100 * got["SQ_WAIT_ANY"] / wc, 100 * got["SQ_WAIT_INST_ANY"] / wc, 4 * got["SQ_ACTIVE_INST_VALU"] / w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--area", default="16x9")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--no-pmc", action="store_true")
    ap.add_argument("--out", default=None, help="append what is printed to this file")
    ap.add_argument("--label", default="", help="a heading for the output (which build this is)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.pmc_child:
        return pmc_child(a)
    fh = open(a.out, "a") if a.out else None

    def out(s):
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()
    if a.label:
        out("== " + a.label)
    if not a.no_pmc:
        counters(a, out)  # children of their own, before this process opens the GPU
    sweep(a, out)


if __name__ == "__main__":
    sys.exit(main())
