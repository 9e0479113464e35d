#!/usr/bin/env python3
"""Event timing of the warped-motion kernels (csrc/warp.hip).  Standalone: imports the package, changes nothing.  Prints one JSON object per line and writes the same
lines to profiles/warp_timing.txt (--out).

  python tools/warp_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--out FILE]

Legs
  warp_16x16          svt_hip_warp_pred_batch on 65 280 luma blocks of 16x16 in one launch (a 4096 x 4080 picture, a mild affine model), 8 and 10 bit, compound 0 and 1
  convolve_2d_16x16   svt_hip_inter_pred_batch on the same count of 16x16 blocks, both directions filtered with the 8-tap kernels, same process, same picture: the
                      yardstick the warp's ratio (`x_convolve`) stands next to
  warp_8x8, warp_64x64  65 280 blocks of 8x8 and 4 032 blocks of 64x64
  warp_model          svt_hip_warp_model_batch for 65 280 blocks
  warp_error          svt_hip_warp_error_batch over one 1920 x 1080 luma plane for 1 and 8 candidates, chess_refn 0 and 1
  cpu legs            `kind: reference`, where oracle/_ref/enc_avx2/libSvtAv1Enc.so exports them and the host has AVX2: svt_av1_warp_affine_avx2 called on 512 x 512 blocks
                      (1024 blocks of 16x16 per call, so the cost of the foreign call does not count) and the reference's svt_av1_warp_error (its dispatch pointers set
                      up for AVX2) on the same 1080p plane, each from 16 host threads at once and from one; host wall clock, the host named.
Outputs are compared with tests/warp_common.py before anything is timed.  Every GPU leg takes the median of `steps` launches, each between its own pair of HIP events,
TWICE: `us_runs` holds both medians; `us_per_launch` is the median of all 2 * steps launches.  Algorithmic bytes per block: p_width * p_height * bytes-per-sample *
(references + 1).  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
NB = 65280  # 255 x 256 blocks
COLS = 256
LINES = []
MAT = [3 * 65536 + 20000, -2 * 65536 + 47001, 65536 + 300, 200, -150, 65536 - 250]
MAT2 = [-65536 - 9000, 65536 + 31000, 65536 - 280, -170, 190, 65536 + 220]


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


def fill_ref(r, k, mat, sh, w, h, stride, plane):
    r["mat"][:, k], r["width"][:, k], r["height"][:, k], r["stride"][:, k], r["plane"][:, k] = mat, w, h, stride, plane
    r["alpha"][:, k], r["beta"][:, k], r["gamma"][:, k], r["delta"][:, k] = sh


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("warp_timing: no GPU -- nothing here is measurable on a CPU")
    import interpred_common as ic
    import warp_common as wc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    g = np.random.default_rng(43)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    sh, sh2 = wc.get_shear_params(MAT), wc.get_shear_params(MAT2)
    W, H = COLS * 16, (NB // COLS) * 16
    conv_us = {}
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        dt = np.uint16 if px == 2 else np.uint8
        hR = [g.integers(0, 1 << bd, (H, W)).astype(dt) for _ in range(2)]
        R = [up(v) for v in hR]
        planes = pkg.InterPredPlanes()
        planes.base[0], planes.base[1] = R[0].data_ptr(), R[1].data_ptr()
        out = torch.zeros(W * H * px, dtype=torch.uint8, device="cuda")
        # the convolve yardstick: 2-D 8-tap on blocks 8 samples inside the picture's border
        by, bx = (v.reshape(-1) for v in np.mgrid[0:NB // COLS, 0:COLS])
        for comp in (0, 1):
            d = np.zeros(NB, pkg.InterPredDesc)
            so = (np.clip(by * 16, 8, H - 24) * W + np.clip(bx * 16, 8, W - 24)).astype(np.uint64)
            d["src_off"][:, 0], d["src_off"][:, 1], d["src_stride"], d["plane"], d["dst_off"], d["dst_stride"] = so, so, W, (0, 1), (by * 16 * W + bx * 16).astype(np.uint64), W
            d["w"] = d["h"] = 16
            d["subpel_x"][:, 0], d["subpel_y"][:, 0], d["subpel_x"][:, 1], d["subpel_y"][:, 1] = 4 + by % 8, 2 + bx % 8, 6, 10
            d["filter_x"], d["filter_y"], d["compound"] = ic.SHARP, ic.REGULAR, comp
            dd, st = up(d), torch.zeros(NB, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_inter_pred_batch(planes, out.data_ptr(), dd.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert not bool(st.any())
            med, runs, mn = timed(torch, fn, a)
            conv_us[(bd, comp)] = med
            nbytes = NB * 256 * px * (2 + comp)
            emit(leg="convolve_2d_16x16", kind="gpu", bd=bd, compound=comp, blocks=NB, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4))
            del dd
        for bs, nb in ((16, NB), (8, NB), (64, NB // 16)):
            cols = COLS if bs != 64 else COLS // 4
            nb = nb // cols * cols  # (whole rows of blocks: 4 032 blocks of 64x64)
            by, bx = (v.reshape(-1) for v in np.mgrid[0:nb // cols, 0:cols])
            for comp in ((0, 1) if bs == 16 else (0,)):
                d = np.zeros(nb, pkg.WarpDesc)
                fill_ref(d["ref"], 0, MAT, sh, W, H, W, 0)
                fill_ref(d["ref"], 1, MAT2, sh2, W, H, W, 1)
                d["dst_off"], d["dst_stride"], d["p_col"], d["p_row"], d["p_width"], d["p_height"], d["compound"] = (by * bs * W + bx * bs).astype(np.uint64), W, bx * bs, by * bs, bs, bs, comp
                dd, st = up(d), torch.zeros(nb, dtype=torch.uint8, device="cuda")
                fn = lambda: lib.svt_hip_warp_pred_batch(planes, out.data_ptr(), dd.data_ptr(), nb, bd, st.data_ptr(), stream)  # noqa: E731
                assert fn() == 0
                torch.cuda.synchronize()
                assert not bool(st.any())
                got = out.cpu().numpy().view(dt).reshape(H, W)
                for i in list(range(0, min(nb, 512), 37)) + [nb - 1]:  # outputs before timing
                    y, x = int(by[i]) * bs, int(bx[i]) * bs
                    want = wc.warp_pred([(hR[0], MAT, sh, W, H), (hR[1], MAT2, sh2, W, H)], x, y, bs, bs, 0, 0, bd, comp)
                    if not np.array_equal(got[y:y + bs, x:x + bs], want):
                        raise SystemExit("warp_timing: parity failure (bd %d, %dx%d, compound %d, block %d)" % (bd, bs, bs, comp, i))
                med, runs, mn = timed(torch, fn, a)
                nbytes = nb * bs * bs * px * (2 + comp)
                extra = {"x_convolve": round(med / conv_us[(bd, comp)], 2)} if bs == 16 else {}
                emit(leg="warp_%dx%d" % (bs, bs), kind="gpu", bd=bd, compound=comp, blocks=nb, tiles=nb * (bs // 8) ** 2, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                     ns_per_16x16=round(med / (nb * bs * bs / 256) * 1e9, 2), algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4),
                     parity="15 blocks == tests/warp_common.py", **extra)
                del dd
        del R, out
        torch.cuda.empty_cache()
    # the model fit
    sets = [wc.model_sample_set(g, ("random", "random", "single", "far")[i % 4]) for i in range(1024)]
    d = np.zeros(NB, pkg.WarpModelDesc)
    for i, s in enumerate(sets):
        d["pts"][i::1024], d["pts_inref"][i::1024], d["np"][i::1024], d["mi_row"][i::1024], d["mi_col"][i::1024] = s["pts"], s["pts_inref"], s["np"], s["mi_row"], s["mi_col"]
        d["mv_row"][i::1024], d["mv_col"][i::1024], d["bsize"][i::1024] = s["mv_row"], s["mv_col"], s["bsize"]
    dd, res, st = up(d), torch.zeros(NB * pkg.WarpModel.itemsize, dtype=torch.uint8, device="cuda"), torch.zeros(NB, dtype=torch.uint8, device="cuda")
    fn = lambda: lib.svt_hip_warp_model_batch(dd.data_ptr(), NB, res.data_ptr(), st.data_ptr(), stream)  # noqa: E731
    assert fn() == 0
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(pkg.WarpModel)
    for i in range(0, 1024, 5):
        s = sets[i]
        r = wc.find_projection(s["np"], s["pts"], s["pts_inref"], s["bsize"], s["mv_row"], s["mv_col"], s["mi_row"], s["mi_col"])
        k = i + 1024 * (i % 60)  # (set i recurs every 1024 blocks)
        ok =int(got["invalid"][k]) == int(r is None) and (r is None or (got["wmmat"][k].tolist() == r[0] and int(got["alpha"][k]) == r[1][0] and int(got["delta"][k]) == r[1][3]))
        if not ok:
            raise SystemExit("warp_timing: model parity failure (set %d)" % i)
    med, runs, mn = timed(torch, fn, a)
    emit(leg="warp_model", kind="gpu", blocks=NB, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_block=round(med / NB * 1e9, 2),
         parity="205 sets == tests/warp_common.py")
    # the warp error of one 1080p luma plane
    Wp, Hp = 1920, 1080
    pic, src = g.integers(0, 256, (Hp, Wp)).astype(np.uint8), g.integers(0, 256, (Hp, Wp)).astype(np.uint8)
    dp, ds = up(pic), up(src)
    planes = pkg.InterPredPlanes()
    planes.base[0], planes.base[1] = dp.data_ptr(), ds.data_ptr()
    small = wc.warp_error(pic, MAT, sh, Wp, Hp, src, 0, 0, 160, 96, 0, 0, 1), wc.warp_error(pic, MAT2, sh2, Wp, Hp, src, 0, 0, 160, 96, 0, 0, 0)
    for n in (1, 8):
        for chess in (0, 1):
            d = np.zeros(n + 2, pkg.WarpErrorDesc)
            for i in range(n + 2):
                m, s = (MAT, sh) if i % 2 == 0 else (MAT2, sh2)
                r = d["ref"]
                r["mat"][i], r["width"][i], r["height"][i], r["stride"][i], r["plane"][i] = m, Wp, Hp, Wp, 0
                r["alpha"][i], r["beta"][i], r["gamma"][i], r["delta"][i] = s
            d["src_stride"], d["src_plane"], d["p_width"], d["p_height"], d["chess_refn"] = Wp, 1, Wp, Hp, chess
            d["p_width"][n:], d["p_height"][n:], d["chess_refn"][n], d["chess_refn"][n + 1] = 160, 96, 1, 0  # two small candidates at the end, for the parity check only
            d["ref"]["mat"][n], d["ref"]["mat"][n + 1] = MAT, MAT2
            for k, s in ((n, sh), (n + 1, sh2)):
                d["ref"]["alpha"][k], d["ref"]["beta"][k], d["ref"]["gamma"][k], d["ref"]["delta"][k] = s
            dd, res = up(d), torch.zeros(n + 2, dtype=torch.int64, device="cuda")
            assert lib.svt_hip_warp_error_batch(planes, dd.data_ptr(), n + 2, res.data_ptr(), None, stream) == 0
            torch.cuda.synchronize()
            got = res.cpu().numpy()
            if (int(got[n]), int(got[n + 1])) != small or (n == 8 and (got[0] != got[2] or got[1] != got[3])) or got[0] <= 0:
                raise SystemExit("warp_timing: warp error parity failure (n %d, chess %d)" % (n, chess))
            st = torch.zeros(n, dtype=torch.uint8, device="cuda")
            fn2 = lambda: lib.svt_hip_warp_error_batch(planes, dd.data_ptr(), n, res.data_ptr(), st.data_ptr(), stream)  # noqa: E731
            med, runs, mn = timed(torch, fn2, a)
            emit(leg="warp_error_1080p", kind="gpu", candidates=n, chess_refn=chess, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 us_per_candidate=round(med / n * 1e6, 1), parity="two 160x96 candidates of the same launch == tests/warp_common.py; equal candidates give equal sums",
                 note="with a status array (no synchronisation); memset + one kernel")
            del dd


def host_has_avx2():
    try:
        return any(ln.startswith("flags") and " avx2" in ln for ln in open("/proc/cpuinfo"))
    except OSError:
        return False


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
    import warp_common as wc
    path = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so")
    if not (os.path.exists(path) and host_has_avx2()):
        emit(leg="cpu_warp", kind="reference", note="not measured: oracle/_ref/enc_avx2/libSvtAv1Enc.so is not on this host or the host has no AVX2")
        return
    lib = C.CDLL(path)
    if not (hasattr(lib, "svt_av1_warp_affine_avx2") and hasattr(lib, "svt_av1_warp_error")):
        emit(leg="cpu_warp", kind="reference", note="not measured: the library does not export svt_av1_warp_affine_avx2 / svt_av1_warp_error")
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as entry
    pkg = entry._pkg()
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    vp, i32, i16 = C.c_void_p, C.c_int, C.c_int16
    f = lib.svt_av1_warp_affine_avx2
    f.restype, f.argtypes = None, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, i16, i16, i16, i16]
    e = lib.svt_av1_warp_error
    e.restype, e.argtypes = C.c_int64, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, C.c_uint8, C.c_int64]
    lib.svt_aom_setup_common_rtcd_internal(C.c_uint64((1 << 9) - 1))  # every flag up to AVX2
    lib.svt_aom_setup_rtcd_internal(C.c_uint64((1 << 9) - 1))
    g = np.random.default_rng(44)
    Wp, Hp = 1920, 1080
    pic, src = g.integers(0, 256, (Hp, Wp)).astype(np.uint8), g.integers(0, 256, (Hp, Wp)).astype(np.uint8)
    sh = wc.get_shear_params(MAT)
    m = np.array(MAT, np.int32)
    cp = pkg.ConvolveParams()
    cp.round_0, cp.round_1 = 3, 11
    preds = [np.zeros((512, 512), np.uint8) for _ in range(16)]
    call = lambda k: f(m.ctypes.data, pic.ctypes.data, Wp, Hp, Wp, preds[k].ctypes.data, 64 * (k % 8) + 200, 32 * (k // 8) + 300, 512, 512, 512, 0, 0, C.byref(cp), *sh)  # noqa: E731
    call(0)
    if not np.array_equal(preds[0][:128, :128], wc.warp_affine(pic, MAT, sh, Wp, Hp, 200, 300, 128, 128, 0, 0, 8, 3, 11)):
        raise SystemExit("warp_timing: svt_av1_warp_affine_avx2 and tests/warp_common.py DIFFER")
    calls, per_call = 100, 1024  # a 512x512 block is 1024 blocks of 16x16
    t16, t1 = threaded(call, 16, calls), threaded(call, 1, calls)
    emit(leg="cpu_warp_affine_avx2", kind="reference", symbol="svt_av1_warp_affine_avx2", library=os.path.relpath(path, ROOT), threads=16, calls_per_thread=calls,
         ns_per_16x16_16_threads=round(t16 / (16 * calls * per_call) * 1e9, 2), ns_per_16x16_1_thread=round(t1 / (calls * per_call) * 1e9, 2), cpus=len(os.sched_getaffinity(0)), host=host,
         parity="the first 128x128 samples == tests/warp_common.py", note="8 bit, not compound, 512x512 blocks (1024 16x16 blocks' worth of 8x8 tiles per call); host wall clock")

    class Wm(C.Structure):
        _fields_ = [("wmtype", C.c_int), ("wmmat", C.c_int32 * 6), ("alpha", i16), ("beta", i16), ("gamma", i16), ("delta", i16), ("invalid", C.c_int8)]
    wms = []
    for _ in range(16):
        w = Wm()
        w.wmtype = 3
        for k in range(6):
            w.wmmat[k] = MAT[k]
        wms.append(w)
    for chess in (0, 1):
        ecall = lambda k: e(C.byref(wms[k]), pic.ctypes.data, Wp, Hp, Wp, src.ctypes.data, 0, 0, Wp, Hp, Wp, 0, 0, chess, (1 << 63) - 1)  # noqa: E731
        want = wc.warp_error(pic, MAT, sh, Wp, Hp, src, 0, 0, 256, 96, 0, 0, chess)
        if e(C.byref(wms[0]), pic.ctypes.data, Wp, Hp, Wp, src.ctypes.data, 0, 0, 256, 96, Wp, 0, 0, chess, (1 << 63) - 1) != want:
            raise SystemExit("warp_timing: the reference's svt_av1_warp_error and tests/warp_common.py DIFFER")
        calls = 6
        t16, t1 = threaded(ecall, 16, calls), threaded(ecall, 1, calls)
        emit(leg="cpu_warp_error_1080p", kind="reference", symbol="svt_av1_warp_error (dispatch pointers set up for AVX2)", library=os.path.relpath(path, ROOT), chess_refn=chess,
             threads=16, calls_per_thread=calls, us_per_candidate_16_threads=round(t16 / (16 * calls) * 1e6, 1), us_per_candidate_1_thread=round(t1 / calls * 1e6, 1),
             cpus=len(os.sched_getaffinity(0)), host=host, parity="a 256x96 corner == tests/warp_common.py", note="best_error = INT64_MAX: no early exit; host wall clock")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
