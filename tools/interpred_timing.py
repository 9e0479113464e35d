#!/usr/bin/env python3
"""Event timing of the inter-prediction kernel (csrc/interpred.hip).  Standalone: imports the package and bench.py's helpers, changes neither.  Prints one JSON object
per line and writes the same lines to profiles/interpred_timing.txt (--out).

  python tools/interpred_timing.py [--steps 20] [--warmup 5] [--planes 32] [--no-cpu] [--out FILE]

Legs (8 and 10 bit; every leg once on ONE 1080p plane -- what a picture's worth of mode-decision candidates looks like, launch-bound -- and once on --planes planes in
one launch, where the byte rate means something)
  sad64x64_pairs     bench.py's own leg, in THIS process on THIS card: the yardstick ("memory-bound done well") the fractions stand next to
  inter_pred 2d      every 16x16 / 32x32 / 64x64 block of the plane(s), pseudo-random quarter-pel vectors with both phases nonzero, SHARP x SHARP
  inter_pred avg     the same as compound average (a second reference with its own vectors)
  inter_pred 2d 8x8  the same pixels as 8x8 blocks
  inter_pred copy    both phases 0: the memory-bound end
  tf_inter_pred      svt_hip_tf_inter_pred_batch (luma only) on the same blocks and vectors: the only kernel the library had for this job, unchanged.  Its output is
                     compared with the new kernel's, sample for sample, before either is timed.
  cpu reference      svt_av1_convolve_2d_sr_avx2 / svt_av1_highbd_convolve_2d_sr_avx2 of oracle/_ref/enc_avx2/libSvtAv1Enc.so (the reference's own AVX2 build, which
                     exports them as ordinary functions) when that library is present and the host has AVX2; otherwise the `_c` functions of oracle/_ref/libsvtref.so.
                     Every line says which (`symbol`, `library`).  16 threads, one call per block; the first blocks' output is compared with the restatement.
Outputs are compared with tests/interpred_common.py (every block of the first plane) before anything is timed; a leg whose svt_hip_tf_inter_pred_batch output differs
from the new kernel's is still timed, says so in `parity`, and makes the tool exit with status 1 after the file is written.  Every GPU leg takes the median of `steps`
launches, each between its own pair of HIP events, TWICE: `us_runs` holds both medians and their difference is the run-to-run spread; `us_per_launch`, the byte rate
and the fraction are those of the median of all 2 * steps launches.  Algorithmic bytes per block: w * h * bytes-per-sample * (references + 1).  Fractions are of
8 TB/s."""
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
W, H, PAD = 1920, 1080, 80
STRIDE, ROWS = W + 2 * PAD, H + 2 * PAD
PLANE = STRIDE * ROWS
LINES = []
DIVERGED = []  # legs whose two kernels disagreed: the tool exits with status 1


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


def median_of_runs(runs):
    """the median of every launch of both runs"""
    t = sorted(runs[0][1] + runs[1][1])
    return t[len(t) // 2]


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def vectors(g, n):
    """1/8-pel vectors: full-pel part in [-4, 4], fraction a nonzero quarter pel (2, 4 or 6 eighths)"""
    return (8 * g.integers(-4, 5, n) + 2 * g.integers(1, 4, n)).astype(np.int16)


def check_plane0(ic, plane0, plane1, d, out0, bs, bd, n0):
    """every block of the first plane against the numpy restatement, vectorised over the blocks that share their phases"""
    win0 = np.lib.stride_tricks.sliding_window_view(plane0, (bs + 7, bs + 7))
    win1 = np.lib.stride_tricks.sliding_window_view(plane1, (bs + 7, bs + 7))
    dd = d[:n0]
    y0, x0 = np.divmod(dd["src_off"][:, 0].astype(np.int64), STRIDE)
    y1, x1 = np.divmod(dd["src_off"][:, 1].astype(np.int64) % PLANE, STRIDE)
    comp = int(dd["compound"][0])
    key = ((dd["subpel_x"][:, 0].astype(np.int64) * 16 + dd["subpel_y"][:, 0]) * 16 + dd["subpel_x"][:, 1] * comp) * 16 + dd["subpel_y"][:, 1] * comp
    oy, ox = np.divmod(dd["dst_off"].astype(np.int64), W)
    for k in np.unique(key):
        m = np.flatnonzero(key == k)
        i = m[0]
        refs = [(win0[y0[m] - 3, x0[m] - 3], int(dd["subpel_x"][i, 0]), int(dd["subpel_y"][i, 0]))]
        if comp:
            refs.append((win1[y1[m] - 3, x1[m] - 3], int(dd["subpel_x"][i, 1]), int(dd["subpel_y"][i, 1])))
        want = ic.predict(refs, bs, bs, int(dd["filter_x"][i]), int(dd["filter_y"][i]), comp, bd)
        for j, b in enumerate(m):
            if not np.array_equal(out0[oy[b]:oy[b] + bs, ox[b]:ox[b] + bs], want[j]):
                raise SystemExit("interpred_timing: parity failure (bd %d, %dx%d, compound %d, block %d)" % (bd, bs, bs, comp, b))


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("interpred_timing: no GPU -- nothing here is measurable on a CPU")
    import bench
    import interpred_common as ic
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    r = bench.bench_sad_pairs(torch, lib, pkg, stream, SimpleNamespace(min_leg_s=0.5), False)
    emit(leg="sad64x64_pairs", kind="gpu", note="bench.py's leg, same process", blocks=240 * 510, us_per_launch=round(r["roofline"]["kernel_us"], 1),
         algorithmic_GBps=round(r["roofline"]["achieved"], 1), frac_of_8TBps=r["roofline"].get("frac"))
    g = np.random.default_rng(31)
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        dt = np.uint16 if px == 2 else np.uint8
        for n_pl in sorted({1, a.planes}):
            if px == 1:
                refs = torch.randint(0, 256, (2 * n_pl * PLANE,), dtype=torch.uint8, device="cuda")
            else:
                refs = torch.randint(0, 1 << bd, (2 * n_pl * PLANE,), dtype=torch.int16, device="cuda")
            out = torch.zeros(n_pl * W * H * px, dtype=torch.uint8, device="cuda")
            tfo = torch.zeros(n_pl * W * H * px, dtype=torch.uint8, device="cuda")
            h0 = refs[:PLANE].cpu().numpy().view(dt).reshape(ROWS, STRIDE)
            h1 = refs[n_pl * PLANE:(n_pl + 1) * PLANE].cpu().numpy().view(dt).reshape(ROWS, STRIDE)
            planes = pkg.InterPredPlanes()
            planes.base[0], planes.base[1] = refs.data_ptr(), refs.data_ptr() + n_pl * PLANE * px
            for (bs, mode) in ((16, "2d"), (32, "2d"), (64, "2d"), (16, "avg"), (32, "avg"), (64, "avg"), (8, "2d"), (16, "copy"), (64, "copy")):
                by, bx = (v.reshape(-1) for v in np.mgrid[0:H // bs, 0:W // bs])
                n0 = len(by)
                n = n0 * n_pl
                f = np.repeat(np.arange(n_pl, dtype=np.int64), n0)
                yy, xx = np.tile(by, n_pl) * bs, np.tile(bx, n_pl) * bs
                mv = [(vectors(g, n), vectors(g, n)) for _ in range(2)]
                if mode == "copy":
                    mv = [(m[0] & ~7, m[1] & ~7) for m in mv]
                d = np.zeros(n, pkg.InterPredDesc)
                for k in range(2):
                    d["src_off"][:, k] = f * PLANE + (PAD + yy + (mv[k][1] >> 3)) * STRIDE + PAD + xx + (mv[k][0] >> 3)
                    d["subpel_x"][:, k], d["subpel_y"][:, k] = (mv[k][0] & 7) * 2, (mv[k][1] & 7) * 2
                d["src_stride"], d["plane"], d["dst_off"], d["dst_stride"] = STRIDE, (0, 1), f * (W * H) + yy * W + xx, W
                d["w"] = d["h"] = bs
                d["filter_x"] = d["filter_y"] = ic.SHARP
                d["compound"] = int(mode == "avg")
                dd = torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()
                st = torch.zeros(n, dtype=torch.uint8, device="cuda")
                fn = lambda: lib.svt_hip_inter_pred_batch(planes, out.data_ptr(), dd.data_ptr(), n, bd, st.data_ptr(), stream)  # noqa: E731  (the asynchronous form)
                out.zero_()
                assert fn() == 0
                torch.cuda.synchronize()
                assert not bool(st.any())
                check_plane0(ic, h0, h1, d, out[:W * H * px].cpu().numpy().view(dt).reshape(H, W), bs, bd, n0)
                # the temporal filter's motion compensation on the same blocks and vectors (single reference, SHARP): same samples, then its time
                tf = None
                if mode == "2d":
                    td = np.zeros(n, pkg.TfMcDesc)
                    td["ref_off"][:, 0], td["pred_off"][:, 0] = f * PLANE, f * (W * H)
                    td["pu_x"], td["pu_y"], td["bsize"], td["mv_x"], td["mv_y"] = xx, yy, bs, mv[0][0], mv[0][1]
                    P = pkg.TfSubpelParams()
                    P.bit_depth, P.mi_rows, P.mi_cols, P.ref_org_x, P.ref_org_y, P.ref_stride = bd, H // 4, W // 4, PAD, PAD, STRIDE
                    PL = pkg.TfMcPlanes()
                    PL.ref[0], PL.pred[0], PL.ref_stride[0], PL.pred_stride[0] = refs.data_ptr(), tfo.data_ptr(), STRIDE, W
                    tdd = torch.from_numpy(td.view(np.uint8).reshape(-1)).cuda()
                    tf = lambda: lib.svt_hip_tf_inter_pred_batch(C.addressof(P), C.addressof(PL), tdd.data_ptr(), n, 0, stream)  # noqa: E731
                    tfo.zero_()
                    tf()
                    torch.cuda.synchronize()
                    rows = (H // bs) * bs
                    same = bool(torch.equal(out.view(n_pl, H, W * px)[:, :rows, :(W // bs) * bs * px], tfo.view(n_pl, H, W * px)[:, :rows, :(W // bs) * bs * px]))
                    DIVERGED.extend([] if same else ["tf_inter_pred_%dx%d bd %d planes %d" % (bs, bs, bd, n_pl)])
                    tf_parity = "every sample == svt_hip_inter_pred_batch" if same else "DIFFERS from svt_hip_inter_pred_batch (which matched tests/interpred_common.py)"
                nrefs = 2 if mode == "avg" else 1
                nbytes = n * bs * bs * px * (nrefs + 1)
                runs = [event_time(torch, fn, a.steps, a.warmup) for _ in range(2)]
                med = median_of_runs(runs)
                emit(leg="inter_pred_%s_%dx%d" % (mode, bs, bs), kind="gpu", bd=bd, planes=n_pl, blocks=n, us_per_launch=round(med * 1e6, 1),
                     us_runs=[round(r[0] * 1e6, 1) for r in runs], us_min=round(min(r[1][0] for r in runs) * 1e6, 1), algorithmic_GBps=round(nbytes / med / 1e9, 1),
                     frac_of_8TBps=round(nbytes / med / HBM, 4), footprint_MB=round((nrefs * PLANE + W * H) * n_pl * px / 1e6),
                     parity="every block of the first plane == tests/interpred_common.py")
                if tf is not None:
                    runs = [event_time(torch, tf, a.steps, a.warmup) for _ in range(2)]
                    med = median_of_runs(runs)
                    emit(leg="tf_inter_pred_%dx%d" % (bs, bs), kind="gpu", bd=bd, planes=n_pl, blocks=n, us_per_launch=round(med * 1e6, 1),
                         us_runs=[round(r[0] * 1e6, 1) for r in runs], us_min=round(min(r[1][0] for r in runs) * 1e6, 1), algorithmic_GBps=round(nbytes / med / 1e9, 1),
                         frac_of_8TBps=round(nbytes / med / HBM, 4), note="svt_hip_tf_inter_pred_batch, luma only, same blocks and vectors",
                         parity=tf_parity)
                del dd, st
            del refs, out, tfo
            torch.cuda.empty_cache()


def host_has_avx2():
    try:
        return any(ln.startswith("flags") and " avx2" in ln for ln in open("/proc/cpuinfo"))
    except OSError:
        return False


def cpu_legs(a):
    """the reference's own functions on one 1080p plane's worth of blocks, 16 threads, one call per block (ctypes releases the GIL for the call): its AVX2 functions
    from the AVX2 build of the reference under oracle/_ref/, its C functions only where that library or AVX2 itself is missing"""
    import interpred_common as ic
    avx2_path = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so")
    c_path = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    if os.path.exists(avx2_path) and host_has_avx2():
        ref_path, suffix, why = avx2_path, "_avx2", "the reference's AVX2 function"
    elif os.path.exists(c_path):
        ref_path, suffix = c_path, "_c"
        why = "the reference's C function (%s)" % ("this host has no AVX2" if os.path.exists(avx2_path) else "oracle/_ref/enc_avx2/libSvtAv1Enc.so is not on this host")
    else:
        emit(leg="cpu_convolve_2d_sr", kind="reference", note="not measured: neither oracle/_ref/enc_avx2/libSvtAv1Enc.so nor oracle/_ref/libsvtref.so is on this host")
        return
    ref = C.CDLL(ref_path)
    pkg = __import__("__graft_entry__")._pkg()
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    cv = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    g = np.random.default_rng(32)
    tab = np.ascontiguousarray(ic.FILTERS[ic.SHARP])
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        sym = ("svt_av1_highbd_convolve_2d_sr" if bd > 8 else "svt_av1_convolve_2d_sr") + suffix
        fnc = getattr(ref, sym)
        fnc.restype, fnc.argtypes = None, cv + ([C.c_int32] if bd > 8 else [])
        plane = g.integers(0, 1 << bd, (ROWS, STRIDE)).astype(dt)
        dst = np.zeros((H, W), dt)
        r0, r1 = ic.conv_rounds(bd, False)
        fx, fy = pkg.InterpFilterParams(tab.ctypes.data, 8, 16, 0), pkg.InterpFilterParams(tab.ctypes.data, 8, 16, 0)
        for bs in (16, 64):
            blocks = [(x, y) for y in range(0, H - bs + 1, bs) for x in range(0, W - bs + 1, bs)]
            mvx, mvy = vectors(g, len(blocks)), vectors(g, len(blocks))

            def work(lo, hi):
                cp = pkg.ConvolveParams(0, 0, None, 0, r0, r1, 0, 0, 0, 0, 0, 0)
                for i in range(lo, hi):
                    x, y = blocks[i]
                    s = plane.ctypes.data + ((PAD + y + (int(mvy[i]) >> 3)) * STRIDE + PAD + x + (int(mvx[i]) >> 3)) * plane.itemsize
                    args = [s, STRIDE, dst.ctypes.data + (y * W + x) * dst.itemsize, W, bs, bs, C.addressof(fx), C.addressof(fy), (int(mvx[i]) & 7) * 2, (int(mvy[i]) & 7) * 2,
                            C.addressof(cp)]
                    fnc(*args, *([bd] if bd > 8 else []))

            cuts = np.linspace(0, len(blocks), 17).astype(int)
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(lambda k: work(cuts[k], cuts[k + 1]), range(16)))
                t0 = time.perf_counter()
                list(ex.map(lambda k: work(cuts[k], cuts[k + 1]), range(16)))
                t = time.perf_counter() - t0
            t0 = time.perf_counter()
            work(0, len(blocks))
            t1 = time.perf_counter() - t0
            for i in range(0, len(blocks), max(1, len(blocks) // 16)):  # the function that was timed computes what the restatement does
                x, y = blocks[i]
                yy, xx = PAD + y + (int(mvy[i]) >> 3) - 3, PAD + x + (int(mvx[i]) >> 3) - 3
                sx, sy = (int(mvx[i]) & 7) * 2, (int(mvy[i]) & 7) * 2
                want = ic.convolve_sr(plane[yy:yy + bs + 7, xx:xx + bs + 7], bs, bs, tab[sx], tab[sy], 3, bd, r0, r1, bd == 8)
                if not np.array_equal(dst[y:y + bs, x:x + bs], want):
                    DIVERGED.append("%s bd %d %dx%d block %d" % (sym, bd, bs, bs, i))
                    break
            emit(leg="cpu_convolve_2d_sr_%dx%d" % (bs, bs), kind="reference", symbol=sym, library=os.path.relpath(ref_path, ROOT), bd=bd, blocks=len(blocks),
                 us_per_1080p_plane_16_threads=round(t * 1e6, 1), us_per_1080p_plane_1_thread=round(t1 * 1e6, 1), us_per_block_1_thread=round(t1 / len(blocks) * 1e6, 2),
                 cpus=len(os.sched_getaffinity(0)), host=host,
                 note=why + ", one ctypes call per block -- the 16x16 figure includes about 2 us of call overhead per block, and the threads share the interpreter "
                      "between calls; host wall clock")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--planes", type=int, default=32, help="planes of the large shape (the small one is always 1)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interpred_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")
    if DIVERGED:
        raise SystemExit("interpred_timing: results DIFFER: " + "; ".join(DIVERGED))


if __name__ == "__main__":
    main()
