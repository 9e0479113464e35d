#!/usr/bin/env python3
"""Event timing of the OBMC motion refinement (csrc/mdsubpel.hip).  Standalone: imports the package, changes nothing.  Prints one JSON object per line and writes the
same lines to profiles/obmc_timing.txt (--out).

  python tools/obmc_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--reference-only] [--harness LIB] [--out FILE]

Legs (the picture and the timing method are those of tools/mdsubpel_timing.py: 4096 x 4096, source = the reference moved by (+2/8, +5/8) plus noise)
  wsrc 16x16, 64x64      svt_hip_obmc_wsrc_batch on 65 280 blocks of 16x16 / 2 040 of 64x64 in one launch, one span a side, both sides available; the neighbour
                         predictions are the reference picture at two other positions
  search 16x16, 64x64    svt_hip_obmc_search_batch on the same items with the target as ARRAYS (what the wsrc leg wrote) and DERIVED, at the settings of refine level 0
                         (full-pel range 16 with diagonals from a start 2 and 3 samples off, then 1/8 sample with 8 taps and two iterations per step) and of level 4
                         (sub-pel only, from the full-pel position); table costs; `evals_per_item`: predictions compared with the target per item
  cpu legs               `kind: reference`: the reference's own single_motion_search through tests/obmc_ref_harness.c, compiled by this tool against
                         oracle/_ref/enc_avx2/libSvtAv1Enc.so with the dispatch pointers set up for AVX2, from 16 host threads and from one (host wall clock, the
                         host named), on the first 4 096 / 512 items.  --harness names a harness built beforehand, for a host without the reference's headers.
Outputs are compared with tests/obmc_common.py before anything is timed.  Every GPU leg takes the median of `steps` launches, each between its own pair of HIP events,
TWICE: `us_runs` holds both medians."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from mdsubpel_timing import COLS, PADP, ROWS, pictures, threaded, timed  # noqa: E402

LINES = []
START = (16, -24)  # best_pred_mv: two rows and three columns off the position the source was cut from
LEVELS = {0: dict(do_full=1, do_frac=1), 4: dict(do_full=0, do_frac=1)}
COMMON = dict(fpel_range=16, fpel_diag=1, allow_hp=1, forced_stop=0, iters_per_step=2, subpel_search_type=3, cost_table=0, approx=0, ref_mv=(0, 0), sad_per_bit=30,
              error_per_bit=120)
ITEMS = {16: 65280, 64: 2040}
BSIZE = {16: 6, 64: 12}


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def geometry(bs, stride):
    cols = COLS * 16 // bs
    by, bx = (v.reshape(-1)[:ITEMS[bs]] for v in np.mgrid[0:ROWS * 16 // bs, 0:cols])
    return ((PADP + by * bs) * stride + PADP + bx * bs).astype(np.uint64), by, bx


def neighbour_offsets(off, stride):
    """the above and the left prediction of a block: the reference picture one row down / one column left, and one row up / two columns right"""
    return off + np.uint64(stride - 1), off - np.uint64(stride - 2)


def host_target(oc, src, ref, y, x, bs):
    ov = min(bs, 64) >> 1
    return oc.target_weighted_pred(BSIZE[bs], src[y:y + bs, x:x + bs], ref[y + 1:y + 1 + ov, x - 1:x - 1 + bs], ref[y - 1:y - 1 + bs, x + 2:x + 2 + ov], 1, 1, [(0, bs >> 2)],
                                   [(0, bs >> 2)])


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("obmc_timing: no GPU -- nothing here is measurable on a CPU")
    import mdsubpel_common as mc
    import obmc_common as oc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    src, ref = pictures()
    stride = ref.shape[1]
    dS, dR = up(src), up(ref)
    tabs = np.zeros(1, pkg.MvCostTable)
    tabs[0]["joint"], tabs[0]["comp"] = mc.cost_tables()[0]
    dT = up(tabs)
    planes = pkg.InterPredPlanes()
    planes.base[0] = planes.base[1] = planes.base[2] = dR.data_ptr()
    for bs in (16, 64):
        off, by, bx = geometry(bs, stride)
        n, bsize, npix = len(off), BSIZE[bs], bs * bs
        a_off, l_off = neighbour_offsets(off, stride)
        spans = dict(up_available=1, left_available=1, n_above=1, n_left=1)
        out_off = np.arange(n, dtype=np.uint64) * np.uint64(npix)
        # ---- the target
        d = np.zeros(n, pkg.ObmcWsrcDesc)
        d["src_off"], d["above_off"], d["left_off"], d["out_off"], d["src_stride"], d["above_stride"], d["left_stride"] = off, a_off, l_off, out_off, stride, stride, stride
        d["above_plane"], d["left_plane"], d["bsize"] = 1, 2, bsize
        for k, v in spans.items():
            d[k] = v
        d["above_len"][:, 0], d["left_len"][:, 0] = bs >> 2, bs >> 2
        dd, st = up(d), torch.zeros(n, dtype=torch.uint8, device="cuda")
        dW, dM = torch.zeros(n * npix, dtype=torch.int32, device="cuda"), torch.zeros(n * npix, dtype=torch.int32, device="cuda")
        fn = lambda: lib.svt_hip_obmc_wsrc_batch(planes, dS.data_ptr(), dd.data_ptr(), n, dW.data_ptr(), dM.data_ptr(), st.data_ptr(), stream)  # noqa: E731
        assert fn() == 0
        torch.cuda.synchronize()
        assert not bool(st.any())
        sample = list(range(0, n, max(n // 12, 1))) + [n - 1]
        hw, hm = dW.cpu().numpy(), dM.cpu().numpy()
        targets = {}
        for i in sample:
            y, x = PADP + int(by[i]) * bs, PADP + int(bx[i]) * bs
            targets[i] = host_target(oc, src, ref, y, x, bs)
            if not (np.array_equal(hw[i * npix:(i + 1) * npix], targets[i][0]) and np.array_equal(hm[i * npix:(i + 1) * npix], targets[i][1])):
                raise SystemExit("obmc_timing: parity failure (wsrc %dx%d, block %d)" % (bs, bs, i))
        del hw, hm
        med, runs, mn = timed(torch, fn, a)
        ov = min(bs, 64) >> 1
        nbytes = n * (npix + 2 * bs * ov + 8 * npix)
        emit(leg="wsrc_%dx%d" % (bs, bs), kind="gpu", blocks=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_block=round(med / n * 1e9, 2),
             algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / 8e12, 4), parity="13 blocks == tests/obmc_common.py",
             bound="the 8 bytes written per pixel: a streaming store kernel")
        del dd
        # ---- the search
        for level, flags in LEVELS.items():
            p = dict(oc.DEFAULTS, **COMMON, **flags, bsize=bsize, best_pred_mv=START, lims=oc.obmc_mv_limits(64, 64, bsize, 2048, 2048))
            want = {}
            for form, fname in ((oc.ARRAYS, "arrays"), (oc.DERIVED, "derived")):
                d = np.zeros(n, pkg.ObmcSearchDesc)
                d["ref_off"], d["ref_stride"], d["bsize"], d["target_form"] = off, stride, bsize, form
                d["wsrc_off"], d["mask_off"] = out_off, out_off
                d["src_off"], d["above_off"], d["left_off"], d["src_stride"], d["above_stride"], d["left_stride"] = off, a_off, l_off, stride, stride, stride
                d["above_plane"], d["left_plane"] = 1, 2
                for k, v in spans.items():
                    d[k] = v
                d["above_len"][:, 0], d["left_len"][:, 0] = bs >> 2, bs >> 2
                d["lim_col_min"], d["lim_col_max"], d["lim_row_min"], d["lim_row_max"] = p["lims"]
                d["best_pred_mv_row"], d["best_pred_mv_col"] = START
                d["do_full_refine"], d["do_frac_refine"], d["approx_inter_rate"], d["fpel_search_range"], d["fpel_search_diag"] = (p["do_full"], p["do_frac"], p["approx"],
                                                                                                                              p["fpel_range"], p["fpel_diag"])
                for f in ("sad_per_bit", "error_per_bit", "cost_table", "allow_hp", "forced_stop", "iters_per_step", "subpel_search_type"):
                    d[f] = p[f]
                dd, res = up(d), torch.zeros(n * pkg.ObmcSearchResult.itemsize, dtype=torch.uint8, device="cuda")
                st.zero_()
                fn = lambda: lib.svt_hip_obmc_search_batch(planes, dS.data_ptr(), dW.data_ptr(), dM.data_ptr(), dT.data_ptr(), 1, dd.data_ptr(), n, res.data_ptr(),  # noqa: E731
                                                           st.data_ptr(), stream)
                assert fn() == 0
                torch.cuda.synchronize()
                assert not bool(st.any())
                got = res.cpu().numpy().view(pkg.ObmcSearchResult)
                for i in sample:
                    if i not in want:
                        y, x = PADP + int(by[i]) * bs, PADP + int(bx[i]) * bs
                        want[i] = oc.obmc_search(ref, y, x, targets[i][0], targets[i][1], p, mc.cost_tables()[0])
                    if {f: int(got[f][i]) for f in oc.RESULT_FIELDS} != want[i]:
                        raise SystemExit("obmc_timing: parity failure (search %s level %d %dx%d, item %d)" % (fname, level, bs, bs, i))
                med, runs, mn = timed(torch, fn, a)
                ev = float(got["evals"].mean())
                hit = float(((got["mv_row"] == 2) & (got["mv_col"] == 5)).mean())
                emit(leg="search_%s_level%d_%dx%d" % (fname, level, bs, bs), kind="gpu", items=n, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                     ns_per_item=round(med / n * 1e9, 2), evals_per_item=round(ev, 2), ns_per_eval=round(med / (n * ev) * 1e9, 3),
                     fp_rounds_per_item=round(float(got["fp_rounds"].mean()), 2), found_the_shift=round(hit, 3), parity="13 items == tests/obmc_common.py")
                del dd
        del dW, dM


def cpu_legs(a):
    import mdsubpel_common as mc
    import obmc_common as oc
    refroot = os.environ.get("SVT_REF", "/root/reference")
    srcdir = os.path.join(refroot, "Source")
    path = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so")
    has_avx2 = any(ln.startswith("flags") and " avx2" in ln for ln in open("/proc/cpuinfo"))
    if not (os.path.exists(path) and has_avx2 and (a.harness or os.path.isfile(os.path.join(srcdir, "Lib", "Codec", "av1me.h")))):
        emit(leg="cpu_single_motion_search", kind="reference", note="not measured: the reference's headers, oracle/_ref/enc_avx2/libSvtAv1Enc.so or AVX2 are not on this host")
        return
    inc = ["-I" + os.path.join(srcdir, s) for s in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/Globals")]
    with tempfile.TemporaryDirectory() as tmp:
        out = a.harness or os.path.join(tmp, "libobmc_harness.so")
        cc = a.harness and subprocess.CompletedProcess([], 0) or subprocess.run(
            ["gcc", "-O2", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *inc, os.path.join(ROOT, "tests", "obmc_ref_harness.c"), "-o", out,
             "-L" + os.path.dirname(path), "-lSvtAv1Enc", "-Wl,-rpath," + os.path.dirname(path)], capture_output=True, text=True)
        if cc.returncode != 0:
            emit(leg="cpu_single_motion_search", kind="reference", note="not measured: the harness did not compile: " + cc.stderr[-300:])
            return
        h = C.CDLL(out)
        vp = C.c_void_p
        h.harness_init_flags.argtypes = [C.c_uint64]
        h.harness_init_flags((1 << 9) - 1)  # every flag up to AVX2
        h.harness_single_motion_search_many.restype = None
        h.harness_single_motion_search_many.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
        host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
        src, ref = pictures()
        stride = ref.shape[1]
        pr = ref.ctypes.data + PADP * stride + PADP
        joint, comp = (np.ascontiguousarray(t) for t in mc.cost_tables()[0])
        names = ("best_r", "best_c", "ref_r", "ref_c", "cmin", "cmax", "rmin", "rmax", "sad_per_bit", "error_per_bit", "approx", "fpel_range", "fpel_diag", "allow_hp",
                 "forced_stop", "iters_per_step", "subpel_search_type", "do_full", "do_frac", "mi_row", "mi_col", "mi_rows", "mi_cols", "qidx", "full_lambda", "refine_level")
        common = dict(kind="reference", library=os.path.relpath(path, ROOT), threads=16, cpus=len(os.sched_getaffinity(0)), host=host,
                      note="single_motion_search, dispatch pointers set up for AVX2; C harness loops over the items; host wall clock")
        for bs in (16, 64):
            cols, per = COLS * 16 // bs, (256 if bs == 16 else 32)
            n, npix = 16 * per, bs * bs
            hw, hm = np.zeros(n * npix, np.int32), np.zeros(n * npix, np.int32)
            for i in range(n):
                y, x = PADP + (i // cols) * bs, PADP + (i % cols) * bs
                hw[i * npix:(i + 1) * npix], hm[i * npix:(i + 1) * npix] = host_target(oc, src, ref, y, x, bs)
            for level, flags in LEVELS.items():
                flat = dict(best_r=START[0], best_c=START[1], ref_r=0, ref_c=0, cmin=0, cmax=0, rmin=0, rmax=0, sad_per_bit=0, error_per_bit=0, approx=0, fpel_range=16,
                            fpel_diag=1, allow_hp=1, forced_stop=0, iters_per_step=2, subpel_search_type=3, mi_row=64, mi_col=64, mi_rows=2048, mi_cols=2048, qidx=120,
                            full_lambda=120 << 6, refine_level=level, **flags)
                ip = np.array([flat[k] for k in names], np.int32)
                res = np.zeros(3 * 8, np.int32)
                h.harness_single_motion_search_many(pr, stride, BSIZE[bs], hw.ctypes.data, hm.ctypes.data, ip.ctypes.data, joint.ctypes.data, comp.ctypes.data, cols, 0, 8,
                                                    res.ctypes.data)
                one = np.zeros(9, np.int32)  # (sadperbit16 is a double formula of base_q_idx on the host: the restatement takes what the C derived, through one direct call)
                h.harness_single_motion_search.restype = None
                h.harness_single_motion_search.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
                h.harness_single_motion_search(pr, stride, BSIZE[bs], hw.ctypes.data, hm.ctypes.data, ip.ctypes.data, joint.ctypes.data, comp.ctypes.data, one.ctypes.data)
                sadpb = int(one[3])
                p = dict(oc.DEFAULTS, **COMMON, **flags, bsize=BSIZE[bs], best_pred_mv=START, lims=oc.obmc_mv_limits(64, 64, BSIZE[bs], 2048, 2048))
                p["sad_per_bit"] = sadpb
                for i in (0, 7):
                    y, x = PADP, PADP + bs * i
                    want = oc.obmc_search(ref, y, x, hw[i * npix:(i + 1) * npix], hm[i * npix:(i + 1) * npix], p, (joint, comp))
                    if [int(v) for v in res[3 * i:3 * i + 3]] != [want["mv_row"], want["mv_col"], want["rate_mv"]]:
                        raise SystemExit("obmc_timing: the reference's single_motion_search and tests/obmc_common.py DIFFER (level %d, %dx%d)" % (level, bs, bs))

                def walk(first):
                    h.harness_single_motion_search_many(pr, stride, BSIZE[bs], hw.ctypes.data + 4 * first * npix, hm.ctypes.data + 4 * first * npix, ip.ctypes.data,
                                                        joint.ctypes.data, comp.ctypes.data, cols, first, per, None)
                t16, t1 = threaded(lambda k: walk(k * per), 16), threaded(lambda k: walk(0), 1)
                emit(leg="cpu_single_motion_search_level%d_%dx%d" % (level, bs, bs), items=n, ns_per_item_16_threads=round(t16 / n * 1e9, 2),
                     ns_per_item_1_thread=round(t1 / per * 1e9, 2), parity="2 items == tests/obmc_common.py", **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--harness", help="a prebuilt tests/obmc_ref_harness.c (shared library linked against oracle/_ref/enc_avx2/libSvtAv1Enc.so) for a host without the "
                                      "reference's headers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obmc_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
