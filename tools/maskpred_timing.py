#!/usr/bin/env python3
"""Event timing of the masked-prediction kernels (csrc/maskpred.hip).  Standalone: imports the package and bench.py's helpers, changes neither.  Prints one JSON object
per line and writes the same lines to profiles/maskpred_timing.txt (--out).

  python tools/maskpred_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--out FILE]

Legs (8 and 10 bit)
  sad64x64_pairs      bench.py's own leg, in THIS process on THIS card: the yardstick ("memory-bound done well") the fractions stand next to
  inter_pred_copy     svt_hip_inter_pred_batch with both phases 0 on the same 65 280 blocks: the plain-copy yardstick (one read, one write per sample)
  blend_*             svt_hip_blend_batch on 65 280 blocks of 16x16 (16.7 M samples) and of 8x8 (4.18 M samples): A64_MASK with an explicit mask, with a wedge and with
                      a smooth inter-intra mask (two reads, one write per sample, plus the mask), and the OBMC HMASK blend in place
  masked_compound     svt_hip_inter_pred_masked_batch (WEDGE; DIFFWTD with the seg mask stored) on 65 280 16x16 blocks, both references filtered in 2-D, next to
                      svt_hip_inter_pred_batch with compound = 1 on the SAME descriptors (`compound_average`, the nearest path without a mask): the difference is
                      what the mask costs
  wedge_search        svt_hip_wedge_search_batch on 8 160 blocks of 32x32 and of 8x8
  cpu wedge search    the same search of one block composed from the reference's helpers as pick_wedge and pick_interinter_seg compose them (sum_squares_i16 twice,
                      wedge_compute_delta_squares, 16 x (wedge_sign_from_residuals + wedge_sse_from_residuals), 2 x (build_compound_diffwtd_mask + sse)), called from
                      a C harness (tools/maskpred_ref_harness.c, compiled by this tool) on 16 host threads and on one: the AVX2 / SSE functions of
                      oracle/_ref/enc_avx2/libSvtAv1Enc.so when that library exports them and the host has AVX2, otherwise the `_c` functions of
                      oracle/_ref/libsvtref.so; every line says which.  The harness's results are compared with tests/maskpred_common.py.
Outputs are compared with tests/maskpred_common.py (the first blocks of every launch) before anything is timed.  Every GPU leg takes the median of `steps` launches, each
between its own pair of HIP events, TWICE: `us_runs` holds both medians; `us_per_launch` is the median of all 2 * steps launches.  Algorithmic bytes per blend block:
w * h * bytes-per-sample * 3 plus the mask bytes read; per search block: bw * bh * bytes-per-sample * 3 + 16 masks.  Fractions are of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
HBM = 8e12
NB = 65280        # 255 x 256 blocks
COLS = 256
NS = 8160         # blocks of a search launch
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
        raise SystemExit("maskpred_timing: no GPU -- nothing here is measurable on a CPU")
    import bench
    import maskpred_common as mc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every launch, median of steps, twice (us_runs)")
    r = bench.bench_sad_pairs(torch, lib, pkg, stream, SimpleNamespace(min_leg_s=0.5), False)
    emit(leg="sad64x64_pairs", kind="gpu", note="bench.py's leg, same process", blocks=240 * 510, us_per_launch=round(r["roofline"]["kernel_us"], 1),
         algorithmic_GBps=round(r["roofline"]["achieved"], 1), frac_of_8TBps=r["roofline"].get("frac"))
    g = np.random.default_rng(41)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        dt = np.uint16 if px == 2 else np.uint8
        for bs in (16, 8):
            Wp, Hp = COLS * bs, (NB // COLS) * bs
            hA, hB = g.integers(0, 1 << bd, (Hp, Wp)).astype(dt), g.integers(0, 1 << bd, (Hp, Wp)).astype(dt)
            hM = g.integers(0, 65, (Hp, Wp)).astype(np.uint8)
            A, B, M = up(hA), up(hB), up(hM)
            out = torch.zeros(Wp * Hp * px, dtype=torch.uint8, device="cuda")
            by, bx = (v.reshape(-1) for v in np.mgrid[0:NB // COLS, 0:COLS])
            off = (by * bs * Wp + bx * bs).astype(np.uint64)
            st = torch.zeros(NB, dtype=torch.uint8, device="cuda")
            # the plain-copy yardstick
            di = np.zeros(NB, pkg.InterPredDesc)
            di["src_off"][:, 0], di["src_stride"], di["dst_off"], di["dst_stride"], di["w"], di["h"] = off, Wp, off, Wp, bs, bs
            ip = pkg.InterPredPlanes()
            ip.base[0] = A.data_ptr()
            ddi = up(di)
            fn = lambda: lib.svt_hip_inter_pred_batch(ip, out.data_ptr(), ddi.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(dt).reshape(Hp, Wp), hA) and not bool(st.any())
            med, runs, mn = timed(torch, fn, a)
            nbytes = NB * bs * bs * px * 2
            emit(leg="inter_pred_copy_%dx%d" % (bs, bs), kind="gpu", bd=bd, blocks=NB, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="the whole plane == the source")
            planes = pkg.BlendPlanes()
            planes.base[0], planes.base[1] = A.data_ptr(), B.data_ptr()
            wb = mc.BSIZE_OF[(bs, bs)]
            for leg in ("explicit", "wedge", "smooth_ii", "obmc_hmask_in_place"):
                d = np.zeros(NB, pkg.BlendDesc)
                d["src_off"][:, 0], d["src_off"][:, 1], d["src_stride"], d["plane"], d["dst_off"], d["dst_stride"] = off, off, Wp, (0, 1), off, Wp
                d["w"], d["h"], d["bsize"] = bs, bs, wb
                mask_bytes = bs * bs
                if leg == "explicit":
                    d["mask_off"], d["mask_stride"] = off, Wp
                elif leg == "wedge":
                    d["mask_src"], d["wedge_index"], d["wedge_sign"] = mc.SRC_WEDGE, np.arange(NB) % 16, (np.arange(NB) // 16) % 2
                elif leg == "smooth_ii":
                    d["mask_src"], d["ii_mode"], mask_bytes = mc.SRC_SMOOTH, np.arange(NB) % 4, 0
                else:
                    d["mask_src"], d["kind"], mask_bytes = mc.SRC_OBMC, mc.KIND_H, 0
                dd = up(d)
                target = A.clone() if leg.endswith("in_place") else out
                if leg.endswith("in_place"):
                    planes.base[0] = target.data_ptr()
                fn = lambda: lib.svt_hip_blend_batch(planes, target.data_ptr(), M.data_ptr(), dd.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
                assert fn() == 0
                torch.cuda.synchronize()
                assert not bool(st.any())
                got = target.cpu().numpy().view(dt).reshape(Hp, Wp)
                for i in range(0, 512, 7):  # outputs before timing
                    y, x = int(by[i]) * bs, int(bx[i]) * bs
                    s0, s1 = hA[y:y + bs, x:x + bs], hB[y:y + bs, x:x + bs]
                    if leg == "explicit":
                        want = mc.blend_a64_mask(s0, s1, hM[y:y + bs, x:x + bs])
                    elif leg == "wedge":
                        want = mc.blend_a64_mask(s0, s1, mc.wedge_masks()[(wb, i % 16, (i // 16) % 2)])
                    elif leg == "smooth_ii":
                        want = mc.blend_a64_mask(s0, s1, mc.smooth_interintra_mask(wb, i % 4))
                    else:
                        want = mc.blend_a64_hmask(s0, s1, mc.OBMC_MASKS[bs])
                    if not np.array_equal(got[y:y + bs, x:x + bs], want):
                        raise SystemExit("maskpred_timing: parity failure (%s, bd %d, %dx%d, block %d)" % (leg, bd, bs, bs, i))
                med, runs, mn = timed(torch, fn, a)  # (the in-place leg keeps blending its own output: the time does not depend on the values)
                nbytes = NB * (bs * bs * px * 3 + mask_bytes)
                emit(leg="blend_%s_%dx%d" % (leg, bs, bs), kind="gpu", bd=bd, blocks=NB, samples=NB * bs * bs, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                     algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="75 blocks == tests/maskpred_common.py")
                planes.base[0] = A.data_ptr()
                del dd, target
            del A, B, M, out
            torch.cuda.empty_cache()
        # the masked compound next to the compound average on the same descriptors
        import interpred_common as ic
        bs, PAD = 16, 8
        Wp, Hp = COLS * bs + 2 * PAD, (NB // COLS) * bs + 2 * PAD
        hR = [g.integers(0, 1 << bd, (Hp, Wp)).astype(dt) for _ in range(2)]
        R = [up(v) for v in hR]
        by, bx = (v.reshape(-1) for v in np.mgrid[0:NB // COLS, 0:COLS])
        so = ((by * bs + PAD) * Wp + bx * bs + PAD).astype(np.uint64)
        do = (by * bs * COLS * bs + bx * bs).astype(np.uint64)
        ph = np.array([2, 4, 8, 12, 14])
        d = np.zeros(NB, pkg.InterPredDesc)
        d["src_off"][:, 0], d["src_off"][:, 1], d["src_stride"], d["plane"], d["dst_off"], d["dst_stride"] = so, so + 3, Wp, (0, 1), do, COLS * bs
        d["w"] = d["h"] = bs
        d["subpel_x"][:, 0], d["subpel_y"][:, 0], d["subpel_x"][:, 1], d["subpel_y"][:, 1] = ph[by % 5], ph[bx % 5], ph[(bx + 1) % 5], ph[(by + 2) % 5]
        d["filter_x"], d["filter_y"], d["compound"] = ic.SHARP, ic.REGULAR, 1
        ip = pkg.InterPredPlanes()
        ip.base[0], ip.base[1] = R[0].data_ptr(), R[1].data_ptr()
        out = torch.zeros(NB * bs * bs * px, dtype=torch.uint8, device="cuda")
        seg = torch.zeros(NB * bs * bs, dtype=torch.uint8, device="cuda")
        st = torch.zeros(NB, dtype=torch.uint8, device="cuda")
        nbytes = NB * bs * bs * px * 3
        wb = mc.BSIZE_OF[(bs, bs)]
        for leg in ("compound_average", "masked_compound_wedge", "masked_compound_diffwtd"):
            if leg == "compound_average":
                dd = up(d)
                fn = lambda: lib.svt_hip_inter_pred_batch(ip, out.data_ptr(), dd.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
            else:
                m = np.zeros(NB, pkg.InterPredMaskedDesc)
                m["p"] = d
                if leg.endswith("wedge"):
                    m["comp_type"], m["bsize"], m["wedge_index"], m["wedge_sign"] = mc.COMP_WEDGE, wb, np.arange(NB) % 16, (np.arange(NB) // 16) % 2
                else:
                    m["comp_type"], m["mask_type"], m["seg_off"] = mc.COMP_DIFFWTD, np.arange(NB) % 2, np.arange(NB, dtype=np.uint64) * (bs * bs)
                dd = up(m)
                fn = lambda: lib.svt_hip_inter_pred_masked_batch(ip, out.data_ptr(), None, seg.data_ptr(), dd.data_ptr(), NB, bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert not bool(st.any())
            got = out.cpu().numpy().view(dt).reshape((NB // COLS) * bs, COLS * bs)
            gseg = seg.cpu().numpy()
            for i in range(0, 512, 7):  # outputs before timing
                y, x = int(by[i]) * bs, int(bx[i]) * bs
                refs = [(hR[k][y + PAD - 3:y + PAD + bs + 4, x + PAD - 3 + 3 * k:x + PAD + bs + 4 + 3 * k], int(d["subpel_x"][i, k]), int(d["subpel_y"][i, k])) for k in range(2)]
                if leg == "compound_average":
                    want, ws = ic.predict(refs, bs, bs, ic.SHARP, ic.REGULAR, 1, bd), None
                elif leg.endswith("wedge"):
                    want, ws = mc.masked_compound(refs, bs, bs, ic.SHARP, ic.REGULAR, bd, mc.COMP_WEDGE, mc.wedge_masks()[(wb, i % 16, (i // 16) % 2)])
                else:
                    want, ws = mc.masked_compound(refs, bs, bs, ic.SHARP, ic.REGULAR, bd, mc.COMP_DIFFWTD, mask_type=i % 2)
                if not np.array_equal(got[y:y + bs, x:x + bs], want) or (ws is not None and not np.array_equal(gseg[i * bs * bs:(i + 1) * bs * bs].reshape(bs, bs), ws)):
                    raise SystemExit("maskpred_timing: parity failure (%s, bd %d, block %d)" % (leg, bd, i))
            med, runs, mn = timed(torch, fn, a)
            emit(leg="%s_2d_16x16" % leg, kind="gpu", bd=bd, blocks=NB, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="75 blocks == the restatement")
            del dd
        del R, out, seg
        torch.cuda.empty_cache()
        for wb in (9, 3):  # 32x32, 8x8
            bw = mc.BW[wb]
            n_px = bw * bw
            trip = [mc.make_search_inputs(g, "near" if i % 2 else "random", wb, bd) for i in range(64)]
            planes_h = [np.concatenate([np.tile(np.stack([t[k].reshape(-1) for t in trip]), (NS // 64 + 1, 1))[:NS]]).astype(dt) for k in range(3)]
            bufs = [up(v) for v in planes_h]
            planes = pkg.BlendPlanes()
            for k in range(3):
                planes.base[k] = bufs[k].data_ptr()
            d = np.zeros(NS, pkg.WedgeSearchDesc)
            o = (np.arange(NS) * n_px).astype(np.uint64)
            d["src_off"], d["p0_off"], d["p1_off"], d["src_stride"], d["p0_stride"], d["p1_stride"] = o, o, o, bw, bw, bw
            d["p0_plane"], d["p1_plane"], d["bsize"] = 1, 2, wb
            dd, res = up(d), torch.zeros(NS * pkg.WedgeSearchResult.itemsize, dtype=torch.uint8, device="cuda")
            st = torch.zeros(NS, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_wedge_search_batch(planes, dd.data_ptr(), NS, bd, res.data_ptr(), st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            got = res.cpu().numpy().view(pkg.WedgeSearchResult)
            for i in range(64):
                w = mc.wedge_search(*trip[i], wb, bd)
                if not (np.array_equal(got[i]["sse"], w["sse"]) and np.array_equal(got[i]["sign"], w["sign"]) and np.array_equal(got[i]["sse_diffwtd"], w["sse_diffwtd"])
                        and int(got[i]["best_wedge_index"]) == w["best_wedge_index"]):
                    raise SystemExit("maskpred_timing: search parity failure (bd %d, bsize %d, block %d)" % (bd, wb, i))
            med, runs, mn = timed(torch, fn, a)
            nbytes = NS * (n_px * px * 3 + 16 * n_px)
            emit(leg="wedge_search_%dx%d" % (bw, bw), kind="gpu", bd=bd, blocks=NS, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 ns_per_block=round(med / NS * 1e9, 1), algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4),
                 parity="64 blocks == tests/maskpred_common.py")


def host_has_avx2():
    try:
        return any(ln.startswith("flags") and " avx2" in ln for ln in open("/proc/cpuinfo"))
    except OSError:
        return False


def cpu_legs(a):
    """pick_wedge + pick_interinter_seg with use_rate == 0 for one block, composed from the reference's own helper functions by tools/maskpred_ref_harness.c (compiled
    here, the functions looked up in the reference's library at run time) on 16 host threads and on one"""
    import subprocess
    import tempfile
    import maskpred_common as mc
    avx2_path = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so")
    c_path = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    names = ["svt_aom_sum_squares_i16", "svt_av1_wedge_compute_delta_squares", "svt_av1_wedge_sign_from_residuals", "svt_av1_wedge_sse_from_residuals",
             "svt_av1_build_compound_diffwtd_mask"]
    syms, path = None, None
    if os.path.exists(avx2_path) and host_has_avx2():
        lib = C.CDLL(avx2_path)
        sfx = [next((s for s in ("_avx2", "_sse4_1", "_sse2") if hasattr(lib, n + s)), None) for n in names]
        if all(sfx):
            syms, path = [n + s for n, s in zip(names, sfx)], avx2_path
    if syms is None and os.path.exists(c_path):
        syms, path = [n + "_c" for n in names], c_path
    if syms is None:
        emit(leg="cpu_wedge_search", kind="reference", note="not measured: neither oracle/_ref/enc_avx2/libSvtAv1Enc.so nor oracle/_ref/libsvtref.so is on this host")
        return
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    g = np.random.default_rng(42)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "maskpred_ref_harness")
        cc = subprocess.run(["gcc", "-O2", "-pthread", os.path.join(ROOT, "tools", "maskpred_ref_harness.c"), "-ldl", "-o", exe], capture_output=True, text=True)
        if cc.returncode != 0:
            emit(leg="cpu_wedge_search", kind="reference", note="not measured: the harness did not compile: " + cc.stderr[-300:])
            return
        for wb in (9, 3):
            n = mc.BW[wb] * mc.BH[wb]
            src, p0, p1 = mc.make_search_inputs(g, "near", wb, 8)
            s, q0, q1 = (v.astype(np.int64).reshape(-1) for v in (src, p0, p1))
            inp = os.path.join(tmp, "in_%d.bin" % wb)
            with open(inp, "wb") as f:
                f.write(np.concatenate([mc.wedge_masks()[(wb, k, sg)].reshape(-1) for k in range(16) for sg in (0, 1)]).tobytes())
                for v in (s - q0, s - q1, q1 - q0):
                    f.write(v.astype("<i2").tobytes())
                f.write(p0.tobytes() + p1.tobytes())
            blocks = 20000 if n > 64 else 100000
            r = subprocess.run([exe, path] + syms + [inp, str(mc.BW[wb]), str(mc.BH[wb]), "16", str(blocks)], capture_output=True, text=True)
            if r.returncode != 0:
                emit(leg="cpu_wedge_search_%dx%d" % (mc.BW[wb], mc.BH[wb]), kind="reference", note="not measured: harness exit %d %s" % (r.returncode, r.stderr[-200:]))
                continue
            v = r.stdout.split()
            want = mc.wedge_search(src, p0, p1, wb, 8)
            same = ([int(x) for x in v[2:18]] == want["sse"].tolist() and [int(x) for x in v[18:34]] == want["sign"].tolist()
                    and [int(x) for x in v[34:36]] == want["sse_diffwtd"].tolist())
            if not same:
                raise SystemExit("maskpred_timing: the reference's helpers and tests/maskpred_common.py DIFFER (bsize %d)" % wb)
            emit(leg="cpu_wedge_search_%dx%d" % (mc.BW[wb], mc.BH[wb]), kind="reference", symbols=syms, library=os.path.relpath(path, ROOT), threads=16,
                 blocks_per_thread=blocks, ns_per_block_16_threads=float(v[0]), ns_per_block_1_thread=float(v[1]), cpus=len(os.sched_getaffinity(0)), host=host,
                 parity="16 SSEs, 16 signs, 2 diff-weighted SSEs == tests/maskpred_common.py",
                 note="C harness (tools/maskpred_ref_harness.c), 37 calls per block from resident buffers: 2 sum_squares, delta_squares, 16 x (sign + sse), 2 x (diffwtd "
                      "mask + sse); ns per block = wall time / (threads x blocks per thread); without forming the residuals; host wall clock")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskpred_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
