#!/usr/bin/env python3
"""Event timing of the palette kernels (csrc/palette.hip).  Standalone: imports the package and the restatement of the tests, changes neither.  Prints one JSON object
per line and writes the same lines to profiles/palette_timing.txt (--out).

  python tools/palette_timing.py [--steps 20] [--warmup 5] [--no-cpu] [--reference-only] [--out FILE]

Legs (8-bit samples in a byte plane, 10-bit samples in a 16-bit plane)
  search_16x16     svt_hip_palette_search_luma_batch on the 65 280 blocks of 16x16 of a 4080 x 4096 picture, one launch
  search_64x64     the same on the 2 040 blocks of 64x64 of a 3840 x 2160 picture (the last block row has 48 rows inside the picture)
  cost_* / pred_*  svt_hip_palette_cost_batch on every candidate those searches kept, read in place; svt_hip_palette_pred_batch of every block that has a candidate
                   from its first one, one transform block of the block's size
  kmeans_n256/4096 svt_hip_kmeans_batch alone on the same blocks' samples, k 8, the search's initial centroids, 50 iterations at most
  cpu legs         `kind: reference`: svt_av1_k_means_dim1_avx2 and search_palette_luma of the reference from 16 host threads at once and from one; host wall clock,
                   the host named.  The library is oracle/_ref/enc_avx2/libSvtAv1Enc.so (the reference with its AVX2 kernels, dispatch as it selects it on the host) or,
                   where that is absent, oracle/_ref/libsvtref.so (C); every line says which.  search_palette_luma is reached through tests/palette_ref_harness.c -- the
                   harness of the reference test, compiled here against the reference's headers where they lie, so these legs run only where the sources are.
Content is synthetic screen content: 3 to 40 colours per block, one dominant, in runs of four samples.  Outputs are compared with tests/palette_common.py before
anything is timed.  Every GPU leg takes the median of `steps` calls, each between its own pair of HIP events, TWICE: `us_runs` holds both medians."""
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
PICTURES = (("16x16", 16, 4080, 4096), ("64x64", 64, 3840, 2160))  # leg, block size, width, height
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


def screen_picture(bs, width, height, bd, seed):
    """the picture, and per block (raster order) rows / cols inside it"""
    g = np.random.default_rng(seed)
    nbx, nby = (width + bs - 1) // bs, (height + bs - 1) // bs
    nb = nbx * nby
    ncol = g.integers(3, 41, nb)
    pal = np.cumsum(g.integers(1, max(2, (1 << bd) // 41), (nb, 40)), axis=1) - 1  # ascending, distinct, below 1 << bd
    idx = np.floor(-np.log(1.0 - g.random((nb, bs, bs // 4))) * ncol[:, None, None] / 3.0).astype(np.int64) % ncol[:, None, None]
    blocks = np.take_along_axis(pal, np.repeat(idx, 4, axis=2).reshape(nb, -1), axis=1).reshape(nby, nbx, bs, bs)
    pic = blocks.transpose(0, 2, 1, 3).reshape(nby * bs, nbx * bs)[:height, :width]
    by, bx = (v.reshape(-1) for v in np.mgrid[0:nby, 0:nbx])
    return np.ascontiguousarray(pic.astype(np.uint16 if bd > 8 else np.uint8)), by, bx, np.minimum(bs, height - by * bs), np.minimum(bs, width - bx * bs)


def initial_centroids(blocks, k):
    lb, ub = blocks.min(1), blocks.max(1)
    return np.stack([lb + (2 * i + 1) * (ub - lb) // k // 2 for i in range(k)], axis=1)


def gpu_legs(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("palette_timing: no GPU -- nothing here is measurable on a CPU")
    import palette_common as pc
    import __graft_entry__ as entry
    pkg = entry._pkg()
    lib = pkg.load(init_device=0)
    stream = torch.cuda.current_stream().cuda_stream
    emit(device=lib.svt_hip_device_name().decode(), steps=a.steps, warmup=a.warmup, timing="HIP events around every call, median of steps, twice (us_runs)")
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()  # noqa: E731
    table = pc.rate_table()
    for bd in (8, 10):
        px = 2 if bd > 8 else 1
        for (leg, bs, width, height) in PICTURES:
            pic, by, bx, rows, cols = screen_picture(bs, width, height, bd, 50 + bd + bs)
            nb, slot = len(by), pc.OUT_HEADER + pc.MAX_CANDS * bs * bs
            d = np.zeros(nb, pkg.PaletteSearchDesc)
            d["src_off"], d["src_stride"], d["out_off"], d["map_stride"] = (by * bs * width + bx * bs).astype(np.uint64), width, (np.arange(nb) * slot).astype(np.uint64), bs * bs
            d["rows"], d["cols"], d["block_width"], d["block_height"], d["dominant_color_step"] = rows, cols, bs, bs, 1
            dpic, dd, out, st = up(pic), up(d), torch.zeros(nb * slot, dtype=torch.uint8, device="cuda"), torch.zeros(nb, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_palette_search_luma_batch(dpic.data_ptr(), dd.data_ptr(), nb, bd, out.data_ptr(), st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            assert not bool(st.any())
            got = out.cpu().numpy().reshape(nb, slot)
            for i in list(range(0, nb, nb // 7)) + [nb - 1]:  # outputs before timing
                want = np.full(slot, 0, np.uint8)
                blk = pic[by[i] * bs:by[i] * bs + rows[i], bx[i] * bs:bx[i] * bs + cols[i]]
                pc.expected_search_out(want, 0, bs * bs, bs, bs, pc.search_palette_luma(blk, bs, bs, [], 1, bd))
                if not np.array_equal(got[i], want):
                    raise SystemExit("palette_timing: parity failure (search, bd %d, %s, block %d)" % (bd, leg, i))
            ncand = got[:, 0].astype(np.int64)
            med, runs, mn = timed(torch, fn, a)
            emit(leg="search_" + leg, kind="gpu", bd=bd, blocks=nb, candidates=int(ncand.sum()), us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                 ns_per_block=round(med / nb * 1e9, 1), parity="9 blocks == tests/palette_common.py")
            # the rate of every kept candidate, read where the search left it
            blk_of = np.repeat(np.arange(nb), ncand)
            s_of = np.arange(len(blk_of)) - np.repeat(np.cumsum(ncand) - ncand, ncand)
            e = np.zeros(len(blk_of), pkg.PaletteCostDesc)
            e["map_off"], e["colors_off"] = (blk_of * slot + pc.OUT_HEADER + s_of * bs * bs).astype(np.uint64), (blk_of * slot + 16 + 16 * s_of).astype(np.uint64)
            e["rows"], e["cols"], e["block_width"], e["size"], e["bit_depth"] = rows[blk_of], cols[blk_of], bs, got[blk_of, 1 + s_of], bd
            de, dt, bits = up(e), up(table), torch.zeros(3 * len(e), dtype=torch.int32, device="cuda")
            ste = torch.zeros(len(e), dtype=torch.uint8, device="cuda")  # (with a status array no entry waits for a descriptor check)
            fn = lambda: lib.svt_hip_palette_cost_batch(out.data_ptr(), de.data_ptr(), len(e), dt.data_ptr(), bits.data_ptr(), ste.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            hb = bits.cpu().numpy().reshape(-1, 3)
            for n in list(range(0, len(e), len(e) // 7)):
                i, s = int(blk_of[n]), int(s_of[n])
                size = int(got[i, 1 + s])
                cmap = got[i, pc.OUT_HEADER + s * bs * bs:pc.OUT_HEADER + (s + 1) * bs * bs].reshape(bs, bs)
                want = pc.palette_costs(cmap, int(rows[i]), int(cols[i]), size, got[i, 16 + 16 * s:32 + 16 * s].view("<u2"), [], bd, table)
                if tuple(hb[n]) != want:
                    raise SystemExit("palette_timing: parity failure (cost, bd %d, %s, item %d)" % (bd, leg, n))
            med, runs, mn = timed(torch, fn, a)
            nbytes = int((e["rows"].astype(np.int64) * e["cols"]).sum())
            emit(leg="cost_" + leg, kind="gpu", bd=bd, items=len(e), us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_item=round(med / len(e) * 1e9, 1),
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="7 items == tests/palette_common.py")
            # the prediction of every block that has a candidate, from its first one
            has = np.flatnonzero(ncand > 0)
            p = np.zeros(len(has), pkg.PalettePredDesc)
            wpad = ((width + bs - 1) // bs) * bs
            p["map_off"], p["colors_off"] = (has * slot + pc.OUT_HEADER).astype(np.uint64), (has * slot + 16).astype(np.uint64)
            p["dst_off"], p["dst_stride"], p["w"], p["h"], p["wpx"] = (by[has] * bs * wpad + bx[has] * bs).astype(np.uint64), wpad, bs, bs, bs
            dp, dst = up(p), torch.zeros(wpad * ((height + bs - 1) // bs) * bs * px, dtype=torch.uint8, device="cuda")
            fn = lambda: lib.svt_hip_palette_pred_batch(out.data_ptr(), dst.data_ptr(), dp.data_ptr(), len(p), int(bd > 8), bd, st.data_ptr(), stream)  # noqa: E731
            assert fn() == 0
            torch.cuda.synchronize()
            hd = dst.cpu().numpy().view(pic.dtype).reshape(-1, wpad)
            for i in has[::max(1, len(has) // 7)]:
                cmap = got[i, pc.OUT_HEADER:pc.OUT_HEADER + bs * bs].reshape(bs, bs)
                want = pc.palette_pred(cmap, got[i, 16:32].view("<u2"), 0, 0, bs, bs, bd > 8, bd)
                if not np.array_equal(hd[by[i] * bs:(by[i] + 1) * bs, bx[i] * bs:(bx[i] + 1) * bs], want):
                    raise SystemExit("palette_timing: parity failure (prediction, bd %d, %s, block %d)" % (bd, leg, i))
            med, runs, mn = timed(torch, fn, a)
            nbytes = len(p) * bs * bs * (1 + px)
            emit(leg="pred_" + leg, kind="gpu", bd=bd, blocks=len(p), us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn, ns_per_block=round(med / len(p) * 1e9, 2),
                 algorithmic_GBps=round(nbytes / med / 1e9, 1), frac_of_8TBps=round(nbytes / med / HBM, 4), parity="blocks == tests/palette_common.py")
            del out, dst, de, dp, bits
            # k-means alone on the full blocks' samples
            if bd == 8:
                full = np.flatnonzero((rows == bs) & (cols == bs))
                n = bs * bs
                data = np.stack([pic[by[i] * bs:(by[i] + 1) * bs, bx[i] * bs:(bx[i] + 1) * bs].reshape(-1) for i in full]).astype(np.int32)
                cent = initial_centroids(data, 8).astype(np.int32)
                k = np.zeros(len(full), pkg.KmeansDesc)
                k["data_off"], k["centroids_off"], k["indices_off"] = np.arange(len(full)) * n, np.arange(len(full)) * 8, np.arange(len(full)) * n
                k["n"], k["max_itr"], k["dim"], k["k"] = n, 50, 1, 8
                ddata, dcent0, dk = up(data), up(cent), up(k)
                dcent, didx = dcent0.clone(), torch.zeros(len(full) * n, dtype=torch.uint8, device="cuda")

                def fn():
                    dcent.copy_(dcent0)  # the centroids are in / out: every call starts from the initial ones (the copy is inside the timed span: 32 bytes per item)
                    return lib.svt_hip_kmeans_batch(ddata.data_ptr(), dcent.data_ptr(), didx.data_ptr(), dk.data_ptr(), len(full), st.data_ptr(), stream)
                assert fn() == 0
                torch.cuda.synchronize()
                hc, hi = dcent.cpu().numpy().view(np.int32).reshape(-1, 8), didx.cpu().numpy().reshape(-1, n)
                for i in range(0, len(full), len(full) // 7):
                    wc, wi = pc.k_means(data[i].reshape(-1, 1), cent[i], 50)
                    if not (np.array_equal(hc[i], wc.reshape(-1)) and np.array_equal(hi[i], wi)):
                        raise SystemExit("palette_timing: parity failure (k-means, n %d, item %d)" % (n, i))
                med, runs, mn = timed(torch, fn, a)
                emit(leg="kmeans_n%d" % n, kind="gpu", items=len(full), k=8, max_itr=50, us_per_launch=round(med * 1e6, 1), us_runs=runs, us_min=mn,
                     ns_per_item=round(med / len(full) * 1e9, 1), parity="8 items == tests/palette_common.py")
                del ddata, didx
            del dpic
            torch.cuda.empty_cache()


def threaded(fn, threads):
    """wall time of `threads` host threads each calling fn(thread index) once (ctypes releases the interpreter lock for the call)"""
    ts = [threading.Thread(target=fn, args=(k,)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return time.perf_counter() - t0


def cpu_legs(a):
    import palette_common as pc
    ref = os.environ.get("SVT_REF", "/root/reference")
    src = os.path.join(ref, "Source")
    avx2, plain = os.path.join(ROOT, "oracle", "_ref", "enc_avx2", "libSvtAv1Enc.so"), os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
    path = avx2 if os.path.exists(avx2) else plain
    if not os.path.exists(path) or not os.path.isfile(os.path.join(src, "Lib", "Codec", "palette.c")):
        emit(leg="cpu_palette", kind="reference", note="not measured: the reference's library or its sources are not on this host")
        return
    host = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown")
    common = dict(kind="reference", library=os.path.relpath(path, ROOT), cpus=len(os.sched_getaffinity(0)), host=host)
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libpalette_harness.so")
        inc = ["-I" + os.path.join(src, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/Globals")]
        flags = ["-DARCH_X86_64=1", "-DEN_AVX512_SUPPORT=0"] if path == avx2 else []
        cc = subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-w", "-std=gnu99", "-fno-strict-aliasing", *flags, *inc, os.path.join(ROOT, "tests", "palette_ref_harness.c"), "-o", so,
                             "-L" + os.path.dirname(path), "-l:" + os.path.basename(path), "-Wl,-rpath," + os.path.dirname(path)], capture_output=True, text=True)
        if cc.returncode != 0:
            emit(leg="cpu_palette", note="not measured: the harness did not compile: " + cc.stderr[-300:], **common)
            return
        lib, h = C.CDLL(path, mode=C.RTLD_GLOBAL), C.CDLL(so)
        if path == avx2:  # the dispatch the reference selects on this host
            lib.svt_aom_get_cpu_flags_to_use.restype = C.c_uint64
            flags = lib.svt_aom_get_cpu_flags_to_use()
            lib.svt_aom_setup_common_rtcd_internal(C.c_uint64(flags))
            lib.svt_aom_setup_rtcd_internal(C.c_uint64(flags))
            kname = "svt_av1_k_means_dim1_avx2"
        else:
            h.harness_init()
            kname = "svt_av1_k_means_dim1_c"
        if C.c_void_p.in_dll(lib, "svt_av1_k_means_dim1").value != C.cast(getattr(lib, kname), C.c_void_p).value:
            raise SystemExit("palette_timing: the dispatch pointer svt_av1_k_means_dim1 is not %s on this host" % kname)
        h.harness_kmeans_items.restype, h.harness_kmeans_items.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        h.harness_search_picture.restype, h.harness_search_picture.argtypes = C.c_long, [C.c_void_p] + [C.c_int] * 8
        for bd in (8, 10):
            for (leg, bs, width, height) in PICTURES:
                pic, by, bx, rows, cols = screen_picture(bs, width, height, bd, 50 + bd + bs)
                # each thread searches its own horizontal band of the picture: 1/16 of the block rows
                band = max(1, len(np.unique(by)) // 16) * bs
                got = [0] * 16

                def search(k):
                    got[k] = h.harness_search_picture(pic.ctypes.data + k * band * width * pic.itemsize, width, int(bd > 8), width, band, bs, bs, 1, bd)
                t16, t1 = threaded(search, 16), threaded(search, 1)
                blk = np.ascontiguousarray(pic[:bs, :bs])
                if h.harness_search_picture(blk.ctypes.data, bs, int(bd > 8), bs, bs, bs, bs, 1, bd) != len(pc.search_palette_luma(blk, bs, bs, [], 1, bd)):
                    raise SystemExit("palette_timing: the reference's search_palette_luma and tests/palette_common.py DIFFER")
                per = (band // bs) * ((width + bs - 1) // bs)
                emit(leg="cpu_search_" + leg, symbol="search_palette_luma", bd=bd, threads=16, blocks_per_thread=per, us_per_block_16_threads=round(t16 / (16 * per) * 1e6, 2),
                     us_per_block_1_thread=round(t1 / per * 1e6, 2), candidates=int(sum(got)), note="tests/palette_ref_harness.c: one context per thread, a band of the "
                     "picture each; us per block = wall time / (threads x blocks per thread); host wall clock", **common)
                if bd == 8:
                    n = bs * bs
                    full = np.flatnonzero((rows == bs) & (cols == bs))[:16 * (256 if bs == 16 else 32)]
                    data = np.stack([pic[by[i] * bs:(by[i] + 1) * bs, bx[i] * bs:(bx[i] + 1) * bs].reshape(-1) for i in full]).astype(np.int32)
                    cent0 = initial_centroids(data, 8).astype(np.int32)
                    cent, idx, per = cent0.copy(), np.zeros((len(full), n), np.uint8), len(full) // 16

                    def run(k):
                        h.harness_kmeans_items(data[k * per:].ctypes.data, cent[k * per:].ctypes.data, idx[k * per:].ctypes.data, n, 8, 50, per)
                    t16 = threaded(run, 16)
                    wc, wi = pc.k_means(data[0].reshape(-1, 1), cent0[0], 50)
                    if not (np.array_equal(cent[0], wc.reshape(-1)) and np.array_equal(idx[0], wi)):
                        raise SystemExit("palette_timing: the reference's k-means and tests/palette_common.py DIFFER")
                    cent[:] = cent0
                    t1 = threaded(run, 1)
                    emit(leg="cpu_kmeans_n%d" % n, symbol=kname, threads=16, items_per_thread=per, k=8, max_itr=50, us_per_item_16_threads=round(t16 / (16 * per) * 1e6, 2),
                         us_per_item_1_thread=round(t1 / per * 1e6, 2), note="through the dispatch pointer, one foreign call per thread; host wall clock", **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--reference-only", action="store_true", help="only the host legs (appended to --out when it exists)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_timing.txt"))
    a = ap.parse_args()
    if not a.reference_only:
        gpu_legs(a)
    if not a.no_cpu:
        cpu_legs(a)
    with open(a.out, "a" if a.reference_only and os.path.exists(a.out) else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
