#!/usr/bin/env python3
"""Event timing of the block variance family and the MD sub-pel search (csrc/mdsubpel.hip).  Standalone: imports the package, changes nothing.  Prints one JSON
object per line and writes the same lines to profiles/mdsubpel_timing.txt (--out).

  python tools/mdsubpel_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--reference-only] [--harness LIB] [--out FILE]

Legs
  var / subpix / upsampled 16x16   svt_hip_block_var_batch on 65 280 blocks of 16x16 in one launch (the first 65 280 of a 4096 x 4096 picture; source = the reference moved by a
                                   fractional vector, plus noise), with a status array
  pruned / tree 16x16, 64x64       svt_hip_md_subpel_search_batch on 65 280 items of 16x16 and 4 080 of 64x64, MV_COST_L1_HDRES, wide limits, every early exit off,
                                   iters_per_step 2, 1/8 sample; `evals_per_item`: predictions compared with the source per item, the centre included
  tf_subpel_16x16                  svt_hip_tf_subpel_search_batch on the same 65 280 blocks in the same process: the nearest existing kernel
  cpu legs                         `kind: reference`: the reference's own functions through tests/mdsubpel_ref_harness.c, compiled by this tool against
                                   oracle/_ref/enc_avx2/libSvtAv1Enc.so with the dispatch pointers set up for AVX2, from 16 host threads and from one (host wall
                                   clock, the host named).  They need the reference's headers, so the tool compiles the harness where its sources are;
                                   --harness names one built beforehand, for a host that has only the library; --reference-only appends the host legs to an existing --out.
Outputs are compared with tests/mdsubpel_common.py before anything is timed.  Every GPU leg takes the median of `steps` launches, each between its own pair of HIP
events, TWICE: `us_runs` holds both medians.  Algorithmic bytes per item: the source block + the rectangle of the reference the C reads for ONE candidate (the
candidates of an item overlap and stay in cache).  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
COLS, ROWS, PADP = 256, 256, 32  # the picture: 4096 x 4096; the 16x16 legs take its first 65 280 blocks, the 64x64 legs its first 4 080
LINES = []
SEARCH = dict(mv_cost_type=3, iters_per_step=2, allow_hp=1, forced_stop=0, subpel_search_type=3, start=(0, 0), ref_mv=(0, 0))


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def pictures():
    """(source, reference): padded planes of one stride; the source is the reference at (+2/8, +5/8) in bilinear arithmetic, plus noise"""
    g = np.random.default_rng(43)
    H, W = ROWS * 16 + 2 * PADP, COLS * 16 + 2 * PADP
    a = g.integers(0, 256, (H + 2, W + 2)).astype(np.int32)
    ref = ((a[:-2, :-2] + a[1:-1, :-2] + a[2:, :-2] + a[:-2, 1:-1] + 4 * a[1:-1, 1:-1] + a[2:, 1:-1] + a[:-2, 2:] + a[1:-1, 2:] + a[2:, 2:] + 6) // 12).astype(np.uint8)
    r = ref.astype(np.int32)
    top = (r[:-1, :-1] * 3 + r[:-1, 1:] * 5 + 4) >> 3
    bot = (r[1:, :-1] * 3 + r[1:, 1:] * 5 + 4) >> 3
    src = np.zeros_like(ref)
    src[:-1, :-1] = np.clip(((top * 6 + bot * 2 + 4) >> 3) + g.integers(-2, 3, top.shape), 0, 255)
    return src, ref


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


def block_offsets(bs, stride):
    cols, rows = COLS * 16 // bs, ROWS * 16 // bs
    n = 65280 if bs == 16 else 4080
    by, bx = (v.reshape(-1)[:n] for v in np.mgrid[0:rows, 0:cols])
    return ((PADP + by * bs) * stride + PADP + bx * bs).astype(np.uint64), by, bx


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mdsubpel_timing: no GPU -- nothing here is measurable on a CPU")
    import mdsubpel_common as mc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    src, ref = pictures()
    stride = ref.shape[1]
    dS, dR = up(src), up(ref)
    planes = pkg.InterPredPlanes()
    planes.base[0] = dR.data_ptr()
    g = np.random.default_rng(7)
    bsize16, bsize64 = 6, 12
    # ---- the primitives
    off, by, bx = block_offsets(16, stride)
    n = len(off)
    for kind, name, ext in ((mc.VAR, "var", (0, 0)), (mc.SUBPIX, "subpix", (1, 1)), (mc.UPSAMPLED, "upsampled", (7, 7))):
        d = np.zeros(n, pkg.BlockVarDesc)
        d["pre_off"], d["src_off"], d["pre_stride"], d["src_stride"], d["bsize"], d["kind"] = off, off, stride, stride, bsize16, kind
        if kind != mc.VAR:
            d["xoffset"], d["yoffset"], d["taps"] = 1 + bx % 7, 1 + by % 7, 3 if kind == mc.UPSAMPLED else 0
        dd, res, st = up(d), torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        fn = lambda: lib.svt_hip_block_var_batch(planes, dS.data_ptr(), None, None, dd.data_ptr(), n, res.data_ptr(), st.data_ptr(), stream)  # noqa: E731
        assert fn() == 0
        torch.cuda.synchronize()
        assert not bool(st.any())
        got = res.cpu().numpy().view(pkg.BlockVarResult)
        for i in list(range(0, n, 2111)) + [n - 1]:
            y, x = PADP + int(by[i]) * 16, PADP + int(bx[i]) * 16
            want = mc.block_var(kind, bsize16, ref, y, x, int(d["xoffset"][i]), int(d["yoffset"][i]), int(d["taps"][i]), src[y:y + 16, x:x + 16])
            if (int(got["var"][i]), int(got["sse"][i]), int(got["sum"][i])) != want[:3]:
                raise SystemExit("mdsubpel_timing: parity failure (%s, block %d)" % (name, i))
        med, runs, mn = timed(torch, fn, a)
        nbytes = n * (256 + (16 + ext[0]) * (16 + ext[1]))
        emit(leg="%s_16x16" % name, kind="gpu", blocks=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_block=round(med / n * 1e9, 2),
             algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="32 blocks == tests/mdsubpel_common.py")
        del dd
    # ---- the searches
    search_us = {}
    for bs, bsize in ((16, bsize16), (64, bsize64)):
        off, by, bx = block_offsets(bs, stride)
        n = len(off)
        for method, name in ((1, "pruned"), (0, "tree")):
            d = np.zeros(n, pkg.MdSubpelDesc)
            p = dict(mc.DEFAULTS, **SEARCH, method=method, bsize=bsize)
            d["src_off"], d["ref_off"], d["src_stride"], d["ref_stride"] = off, off, stride, stride
            d["lim_col_min"], d["lim_col_max"], d["lim_row_min"], d["lim_row_max"] = mc.WIDE_LIMITS
            for f in ("pred_variance_th", "round_dev_th", "bias_fp", "error_per_bit", "early_exit_th", "cost_table", "qp", "bsize", "method", "allow_hp", "forced_stop",
                      "iters_per_step", "abs_th_mult", "skip_diag_refinement", "subpel_search_type", "mv_cost_type", "early_exit", "mvp_th"):
                d[f] = p[f]
            dd, res, st = up(d), torch.zeros(n * 24, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_md_subpel_search_batch(planes, dS.data_ptr(), None, 0, dd.data_ptr(), n, res.data_ptr(), st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert not bool(st.any())
            got = res.cpu().numpy().view(pkg.MdSubpelResult)
            for i in list(range(0, n, max(n // 12, 1))) + [n - 1]:
                y, x = PADP + int(by[i]) * bs, PADP + int(bx[i]) * bs
                want = mc.md_subpel_search(src[y:y + bs, x:x + bs], ref, y, x, p)
                if {f: int(got[f][i]) for f in want} != want:
                    raise SystemExit("mdsubpel_timing: parity failure (%s %dx%d, item %d)" % (name, bs, bs, i))
            med, runs, mn = timed(torch, fn, a)
            ev = float(got["evals"].mean())
            search_us[(name, bs)] = med
            hit = float(((got["mv_row"] == 2) & (got["mv_col"] == 5)).mean())
            emit(leg="%s_%dx%d" % (name, bs, bs), kind="gpu", items=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_item=round(med / n * 1e9, 2),
                 evals_per_item=round(ev, 2), ns_per_eval=round(med / (n * ev) * 1e9, 3), found_the_shift=round(hit, 3), parity="13 items == tests/mdsubpel_common.py")
            del dd
    # ---- the temporal filter's search on the same blocks
    off, by, bx = block_offsets(16, stride)
    n = len(off)
    P = pkg.TfSubpelParams()
    P.half_pel_mode = P.quarter_pel_mode = P.eight_pel_mode = 1
    P.subsampling_shift, P.bit_depth, P.early_exit_th = 0, 8, 0
    P.mi_rows, P.mi_cols, P.ref_org_x, P.ref_org_y, P.ref_stride = ROWS * 4, COLS * 4, PADP, PADP, stride
    d = np.zeros(n, pkg.TfSubpelDesc)
    d["src_off"], d["src_stride"], d["pu_x"], d["pu_y"], d["bsize"] = off, stride, bx * 16, by * 16, 16
    dd, res = up(d), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    fn = lambda: lib.svt_hip_tf_subpel_search_batch(C.byref(P), dS.data_ptr(), dR.data_ptr(), dd.data_ptr(), n, res.data_ptr(), stream)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    med, runs, mn = timed(torch, fn, a)
    emit(leg="tf_subpel_16x16", kind="gpu", items=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_item=round(med / n * 1e9, 2), evals_per_item=25,
         x_tree_16x16=round(search_us[("tree", 16)] / med, 2), x_pruned_16x16=round(search_us[("pruned", 16)] / med, 2),
         note="svt_check_position: the centre and three rings of eight 8-tap candidates, no early exit; another algorithm on the same blocks")


def threaded(fn, threads):
    ts = [threading.Thread(target=fn, args=(k,)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return time.perf_counter() - t0


def cpu_legs(a):
    import mdsubpel_common as mc
    refroot = os.environ.get("SVT_REF", "/root/reference")
    srcdir = os.path.join(refroot, "Source")
    path = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so")
    has_avx2 = any(ln.startswith("flags") and " avx2" in ln for ln in open("/proc/cpuinfo"))
    if not (os.path.exists(path) and has_avx2 and (a.harness or os.path.isfile(os.path.join(srcdir, "Lib", "Codec", "mcomp.h")))):
        emit(leg="cpu_mdsubpel", kind="reference", note="not measured: the reference's headers, oracle/_ref/enc_avx2/libSvtAv1Enc.so or AVX2 are not on this host")
        return
    inc = ["-I" + os.path.join(srcdir, s) for s in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/Globals")]
    with tempfile.TemporaryDirectory() as tmp:
        out = a.harness or os.path.join(tmp, "libmdsubpel_harness.so")
        cc = a.harness and subprocess.CompletedProcess([], 0) or subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *inc, os.path.join(ROOT, "tests", "mdsubpel_ref_harness.c"), "-o", out,
                             "-L" + os.path.dirname(path), "-lSvtAv1Enc", "-Wl,-rpath," + os.path.dirname(path)], capture_output=True, text=True)
        if cc.returncode != 0:
            emit(leg="cpu_mdsubpel", kind="reference", note="not measured: the harness did not compile: " + cc.stderr[-300:])
            return
        h = C.CDLL(out)
        vp = C.c_void_p
        h.harness_init_flags.argtypes = [C.c_uint64]
        h.harness_init_flags((1 << 9) - 1)  # every flag up to AVX2
        h.harness_md_subpel_many.restype, h.harness_md_subpel_many.argtypes = None, [C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]
        h.harness_prim_many.restype, h.harness_prim_many.argtypes = None, [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
        src, ref = pictures()
        stride = ref.shape[1]
        base = PADP * stride + PADP
        ps, pr = src.ctypes.data + base, ref.ctypes.data + base
        common = dict(kind="reference", library=os.path.relpath(path, ROOT), threads=16, cpus=len(os.sched_getaffinity(0)), host=host,
                      note="dispatch pointers set up for AVX2; C harness loops over the items; host wall clock")
        for kind, name in ((0, "var"), (1, "subpix"), (2, "upsampled")):
            n = 65280
            outv = np.zeros(n, np.uint32)
            h.harness_prim_many(kind, ps, pr, stride, 6, 3, 5, 3, COLS, 0, 64, outv.ctypes.data)
            for i in (0, 17, 63):
                y, x = PADP, PADP + 16 * i
                want = mc.block_var((mc.VAR, mc.SUBPIX, mc.UPSAMPLED)[kind], 6, ref, y, x, 3 if kind else 0, 5 if kind else 0, 3 if kind == 2 else 0, src[y:y + 16, x:x + 16])[0]
                if int(outv[i]) != want:
                    raise SystemExit("mdsubpel_timing: the reference's %s and tests/mdsubpel_common.py DIFFER" % name)
            per, reps = n // 16, (5 if kind == 2 else 100)  # (a thread's share is walked `reps` times: its start-up must not be what is timed)

            def walk(first):
                for _ in range(reps):
                    h.harness_prim_many(kind, ps, pr, stride, 6, 3, 5, 3, COLS, first, per, None)
            t16, t1 = threaded(lambda k: walk(k * per), 16), threaded(lambda k: walk(0), 1)
            emit(leg="cpu_%s_16x16" % name, blocks=16 * per, passes=reps, ns_per_block_16_threads=round(t16 / (16 * per * reps) * 1e9, 2),
                 ns_per_block_1_thread=round(t1 / (per * reps) * 1e9, 2), parity="3 blocks == tests/mdsubpel_common.py", **common)
        for bs, bsize in ((16, 6), (64, 12)):
            cols, n = COLS * 16 // bs, 65280 if bs == 16 else 4080
            for method, name in ((1, "pruned"), (0, "tree")):
                p = dict(mc.DEFAULTS, **SEARCH, method=method, bsize=bsize)
                lims = mc.WIDE_LIMITS
                flat = dict(p, start_r=0, start_c=0, ref_r=0, ref_c=0, cmin=lims[0], cmax=lims[1], rmin=lims[2], rmax=lims[3], mvp_r=0, mvp_c=0)
                names = ("start_r", "start_c", "ref_r", "ref_c", "cmin", "cmax", "rmin", "rmax", "allow_hp", "forced_stop", "iters_per_step", "pred_variance_th", "abs_th_mult",
                         "round_dev_th", "skip_diag_refinement", "subpel_search_type", "bias_fp", "qp", "early_exit", "mv_cost_type", "error_per_bit", "early_exit_th", "mvp_th",
                         "hp_mv_th", "best_mvp_err", "mvp_r", "mvp_c")
                ip = np.array([flat[k] for k in names], np.int32)
                res = np.zeros(6 * 8, np.int32)
                h.harness_md_subpel_many(method, ps, pr, stride, bsize, ip.ctypes.data, cols, 0, 8, res.ctypes.data)
                for i in (0, 7):
                    y, x = PADP, PADP + bs * i
                    want = mc.md_subpel_search(src[y:y + bs, x:x + bs], ref, y, x, p)
                    if [int(v) & 0xFFFFFFFF for v in res[6 * i:6 * i + 6]] != [want[f] & 0xFFFFFFFF for f in mc.RESULT_FIELDS]:
                        raise SystemExit("mdsubpel_timing: the reference's %s search and tests/mdsubpel_common.py DIFFER" % name)
                per, reps = n // 16, (10 if method == 1 else 1)

                def walk(first):
                    for _ in range(reps):
                        h.harness_md_subpel_many(method, ps, pr, stride, bsize, ip.ctypes.data, cols, first, per, None)
                t16, t1 = threaded(lambda k: walk(k * per), 16), threaded(lambda k: walk(0), 1)
                emit(leg="cpu_%s_%dx%d" % (name, bs, bs), items=16 * per, passes=reps, ns_per_item_16_threads=round(t16 / (16 * per * reps) * 1e9, 2),
                     ns_per_item_1_thread=round(t1 / (per * reps) * 1e9, 2), parity="2 items == tests/mdsubpel_common.py", **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--harness", help="a prebuilt tests/mdsubpel_ref_harness.c (shared library linked against oracle/_ref/enc_avx2/libSvtAv1Enc.so) for a host without "
                                      "the reference's headers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mdsubpel_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
