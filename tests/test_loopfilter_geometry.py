"""The in-loop filter stage -- deblocking, CDEF (search, strength pick, apply), loop restoration -- at picture and buffer geometry edges.  Every frame-level test
elsewhere passes stride == width and buffers of exactly h * w samples, which hides a kernel that indexes one buffer with another buffer's stride or stores past a row,
a plane or a table.  Here every pointer of a call has its own stride (at least one odd) and lead (at least one odd in samples), inputs carry random samples between
their rows, outputs and tables are sentinel-filled and compared WHOLE (tests/loopfilter_geometry_common.py), at the smallest sizes at which each path exists: odd
widths, planes narrower than a processing unit, ss_x != ss_y, 12 bit, 8-bit content in 16-bit buffers, 4-sample-grid deblocking edges, launch counts at the workgroup
and slice boundaries of the strength pick.  The reference for everything is the oracle (pinned against the reference's `_c` functions by tests/test_oracle_pin_*.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import p, rng
from loopfilter_geometry_common import I8_FILL, I32_FILL, U64_FILL, LrCase, Plane, check_table, dev_ptr, lpf_edge_lists, lpf_oracle, table
from test_cdef import synth_plane
from test_cdef_pick import ptr_tables, tables
from test_deblock import LENS, lim_arrays, limits, make_patch


class tuning:
    """one of the measurement knobs set for the block (read once by the library, so it is reloaded on the way in and out)"""

    def __init__(self, be, name, value):
        self.be, self.name, self.value = be, name, value

    def __enter__(self):
        os.environ[self.name] = self.value
        self.be.lib.svt_hip_tuning_reload()

    def __exit__(self, *exc):
        del os.environ[self.name]
        self.be.lib.svt_hip_tuning_reload()


# ======================================================================================================================================================================
# 1. loop restoration frame
# ======================================================================================================================================================================
#            ss_x ss_y  w    h   unit
LR_GEOM = {"a": (0, 0, 67, 75, 64),    # odd width: the last column of every row is a single-sample store; two stripes
           "b": (0, 0, 129, 41, 64),   # a third processing unit one sample wide (129 = 1 mod 8: its staging is all pixel by pixel)
           "c": (1, 1, 35, 37, 32),    # 4:2:0 chroma, 32-column processing units, 35 = 3 mod 8
           "d": (1, 0, 36, 70, 64),    # 4:2:2 chroma: 32-column processing units on 64-row stripes
           "e": (0, 1, 70, 36, 32),    # 4:4:0 chroma: 64-column processing units on 32-row stripes; restoration units narrower than a processing unit
           "f": (0, 0, 5, 5, 64),      # narrower and lower than the 3-sample halo is deep twice over: every staged sample is clamped
           "g": (1, 1, 33, 9, 32)}     # the second processing unit is one sample wide, one short stripe
LR_CASES = [(k, int(bd > 8), bd) for k in LR_GEOM for bd in (8, 10, 12)] + [("h", 1, 8)]  # h: 8-bit content in 16-bit buffers (the encoder's 16-bit pipeline)
LR_GEOM["h"] = (1, 1, 67, 75, 32)


def lr_case(oracle, be, key, highbd, bd, dst_lead, dst_odd_stride=False):
    return LrCase(rng(1000 + 7 * ord(key) + bd + dst_lead), oracle, be.pkg.LrUnit, highbd, bd, *LR_GEOM[key], dst_lead, dst_odd_stride)


@pytest.mark.parametrize("dst_lead", [16, 17])
@pytest.mark.parametrize("key,highbd,bd", LR_CASES)
def test_lr_frame_geometry(be, oracle, key, highbd, bd, dst_lead):
    """svt_hip_lr_filter_frame, device form: data, boundary lines and dst each on their own stride; an even dst lead (pair stores where the width allows) and an odd
    one (single stores everywhere)."""
    c = lr_case(oracle, be, key, highbd, bd, dst_lead)
    P, d_out, keep = c.device(be)
    be.lib.svt_hip_lr_filter_frame(C.byref(P), be.stream)
    c.po.check(be.host(d_out), c.want, "lr frame %s hbd %d bd %d dst lead %d" % (key, highbd, bd, dst_lead))


LR_BD_OF = {"a": 10, "b": 8, "c": 12, "d": 10, "e": 8, "f": 12, "g": 10, "h": 8}


@pytest.mark.parametrize("ur", ["16", "32", "64"])
def test_lr_frame_geometry_rows_per_workgroup(be, oracle, ur):
    """the three instantiations of lr_frame_kernel (SVT_HIP_LR_UR) on the device form: every geometry once, dst on an odd stride (never pair stores)"""
    with tuning(be, "SVT_HIP_LR_UR", ur):
        for key, bd in LR_BD_OF.items():
            highbd = 1 if key == "h" else int(bd > 8)
            c = lr_case(oracle, be, key, highbd, bd, 16, dst_odd_stride=True)
            P, d_out, keep = c.device(be)
            be.lib.svt_hip_lr_filter_frame(C.byref(P), be.stream)
            c.po.check(be.host(d_out), c.want, "lr frame %s bd %d SVT_HIP_LR_UR=%s" % (key, bd, ur))


@pytest.mark.parametrize("ur", ["16", "32", "64"])
@pytest.mark.parametrize("key", ["a", "c", "d", "e", "h"])
def test_lr_stripes_geometry(be, oracle, key, ur):
    """svt_hip_lr_filter_frame_stripes one stripe per call in shuffled order (every stripe's halo rows belong to another call), the last stripe through a range that
    runs past it, and empty ranges (equal ends, reversed ends, wholly past the plane): together the whole-frame result, nothing else written."""
    bd = LR_BD_OF[key]
    c = lr_case(oracle, be, key, 1 if key == "h" else int(bd > 8), bd, 17 if key in "ce" else 16)
    n = c.nstripes
    assert n >= 2
    order = [int(s) for s in rng(n + int(ur)).permutation(n - 1)]
    with tuning(be, "SVT_HIP_LR_UR", ur):
        P, d_out, keep = c.device(be)
        for (a, b) in [(1, 1), (n, n + 3)] + [(s, s + 1) for s in order] + [(n - 1, n + 3), (n - 1, 0)]:
            be.lib.svt_hip_lr_filter_frame_stripes(C.byref(P), a, b, be.stream)
        c.po.check(be.host(d_out), c.want, "lr stripes %s SVT_HIP_LR_UR=%s order %s" % (key, ur, order))


# ======================================================================================================================================================================
# 2. CDEF frame
# ======================================================================================================================================================================
CDEF_CANDS = [(0, 0), (4, 2), (15, 4), (1, 0), (0, 1), (7, 1), (9, 0), (2, 4), (5, 2)]
CDEF_GEOM = {"luma72x40": (72, 40, 0, 0, 0), "luma136x72": (136, 72, 0, 0, 0), "luma8x8": (8, 8, 0, 0, 0),
             "c420_36x20": (36, 20, 1, 1, 1), "c420_68x36": (68, 36, 1, 1, 2),   # the last filter block is 4 samples wide
             "c422_36x72": (36, 72, 1, 0, 1), "c440_72x36": (72, 36, 0, 1, 2)}
CDEF_DEPTH = [(0, 8), (1, 10), (1, 12), (1, 8)]  # (is_16bit, bit depth); the last = coeff_shift 0 on 16-bit buffers


class CdefCase:
    """One plane of CDEF: recon on an odd stride and an odd lead, source on an even stride, out on a third (odd) stride and an odd lead; dir / var / mse with sentinel
    tails.  Luma writes dir / var (they start sentinel-filled), chroma reads them (random values that must come back unchanged)."""

    def __init__(self, g, w, h, xdec, ydec, pli, is16, bd, skip_frac=0.2):
        dt = np.uint16 if is16 else np.uint8
        self.w, self.h, self.xdec, self.ydec, self.pli, self.is16, self.bd = w, h, xdec, ydec, pli, is16, bd
        bw, bh = 64 >> xdec, 64 >> ydec
        self.nhfb, self.nvfb = (w + bw - 1) // bw, (h + bh - 1) // bh
        self.nfb = self.nhfb * self.nvfb
        room = w + 18
        self.pr, self.ps, self.po = Plane(w, h, (w + 11) | 1, 13, dt, room=room), Plane(w, h, (w + 18) & ~1, 8, dt, room=room), Plane(w, h, (w + 5) | 1, 3, dt, room=room)
        pic = synth_plane(g, w, h, bd)
        self.pic = pic
        self.recon = self.pr.noisy(g, pic, bd)
        self.source = self.ps.noisy(g, np.clip(pic + g.integers(-6, 7, pic.shape), 0, (1 << bd) - 1), bd)
        self.skip = (g.random((self.nvfb * 8, self.nhfb * 8)) < skip_frac).astype(np.uint8)
        self.dir0, self.var0 = table(self.nfb * 64, 0xA5, np.uint8, 64), table(self.nfb * 64, I32_FILL, np.int32, 64)
        if pli:
            self.dir0[:self.nfb * 64] = g.integers(0, 8, self.nfb * 64)
            self.var0[:self.nfb * 64] = g.integers(0, 1 << 14, self.nfb * 64)

    def run(self, be, oracle, mode, pri, sec, tag, dev_mode=None, dir_in=None, var_in=None, sub=1, damping=5, rows=None):
        """oracle and device for one mode; everything compared whole.  rows = the (begin, end) ranges of svt_hip_cdef_frame_rows to cover the plane with.  Returns the
        oracle's (dir, var) tables."""
        ncand = len(pri) if mode == 1 else 0
        dir0, var0 = (self.dir0 if dir_in is None else dir_in), (self.var0 if var_in is None else var_in)
        o_out, o_dir, o_var, o_mse = self.po.guarded(self.pic), dir0.copy(), var0.copy(), table(self.nfb * max(ncand, 1), U64_FILL, np.uint64)
        oracle.oracle_cdef_frame(mode, self.pr.host_ptr(self.recon), self.pr.stride, self.ps.host_ptr(self.source), self.ps.stride, self.po.host_ptr(o_out), self.po.stride,
                                 self.w, self.h, self.xdec, self.ydec, self.pli, self.is16, self.bd - 8, damping, damping, sub, p(self.skip), p(pri), p(sec), ncand,
                                 p(o_dir), p(o_var), p(o_mse))
        d_rec, d_src, d_out = be.dev(self.recon), be.dev(self.source), be.dev(self.po.guarded(self.pic))
        d_skip, d_pri, d_sec = be.dev(self.skip), be.dev(pri), be.dev(sec)
        d_dir, d_var, d_mse = be.dev(dir0), be.dev(var0), be.dev(table(self.nfb * max(ncand, 1), U64_FILL, np.uint64))
        P = be.pkg.CdefParams(dev_ptr(be, d_rec, self.pr), dev_ptr(be, d_src, self.ps), dev_ptr(be, d_out, self.po), self.pr.stride, self.ps.stride, self.po.stride,
                              self.w, self.h, self.xdec, self.ydec, self.pli, self.is16, self.bd - 8, damping, damping, sub, ncand, be.ptr(d_skip), be.ptr(d_pri),
                              be.ptr(d_sec), be.ptr(d_dir), be.ptr(d_var), be.ptr(d_mse))
        dm = mode if dev_mode is None else dev_mode
        if rows is None:
            be.lib.svt_hip_cdef_frame(dm, C.byref(P), be.stream)
        else:
            for (r0, r1) in rows:
                be.lib.svt_hip_cdef_frame_rows(dm, C.byref(P), r0, r1, be.stream)
        check_table(be.host(d_dir), o_dir, self.nfb * 64, tag + " dir")
        check_table(be.host(d_var), o_var, self.nfb * 64, tag + " var")
        check_table(be.host(d_mse), o_mse, self.nfb * ncand, tag + " mse")
        self.po.check(be.host(d_out), o_out, tag + " out")
        if self.pli:
            assert np.array_equal(o_dir, dir0) and np.array_equal(o_var, var0), tag + ": chroma must not write dir / var"
        return o_dir, o_var

    def strengths(self, g):
        """apply: per-block (level, secondary): both, one alone (the 4- / 8-tap forms), none"""
        apri = g.choice(np.array([0, 4, 9, 15], np.int32), self.nfb, p=[0.25, 0.35, 0.2, 0.2]).astype(np.int32)
        asec = np.where(apri == 0, g.integers(0, 2, self.nfb), np.where(g.random(self.nfb) < 0.4, 0, g.choice(np.array([1, 2, 4], np.int32), self.nfb))).astype(np.int32)
        return apri, asec


def cand_arrays(cands):
    return np.array([c[0] for c in cands], np.int32), np.array([c[1] for c in cands], np.int32)


@pytest.mark.parametrize("is16,bd", CDEF_DEPTH)
@pytest.mark.parametrize("geom", list(CDEF_GEOM))
def test_cdef_frame_geometry(be, oracle, geom, is16, bd):
    """svt_hip_cdef_frame modes 1 (search), 0 (apply) and 2 (apply with the search pass's directions) with three distinct strides and guarded out / mse / dir / var"""
    w, h, xdec, ydec, pli = CDEF_GEOM[geom]
    g = rng(2000 + w + 3 * h + bd + is16)
    c = CdefCase(g, w, h, xdec, ydec, pli, is16, bd)
    tag = "cdef %s is16 %d bd %d" % (geom, is16, bd)
    pri, sec = cand_arrays(CDEF_CANDS)
    d, v = c.run(be, oracle, 1, pri, sec, tag + " search", sub=2 if ydec == 0 else 1, damping=3 + (bd + w) % 4)
    apri, asec = c.strengths(g)
    if geom == "luma8x8":
        apri[:], asec[:] = 4, 2
    c.run(be, oracle, 0, apri, asec, tag + " apply")
    c.run(be, oracle, 0, apri, asec, tag + " apply with given directions", dev_mode=2, dir_in=d, var_in=v)


@pytest.mark.parametrize("is16,bd", [(0, 8), (1, 10)])
def test_cdef_frame_all_units_skipped(be, oracle, is16, bd):
    """filter blocks without one active unit: the search reports zero for every candidate, apply leaves the block, dir and var alone"""
    g = rng(2100 + bd)
    c = CdefCase(g, 72, 40, 0, 0, 0, is16, bd, skip_frac=0.2)
    c.skip[:, 8:] = 1  # the 8-sample-wide second filter block
    pri, sec = cand_arrays(CDEF_CANDS)
    c.run(be, oracle, 1, pri, sec, "cdef skipped block, search")
    c.run(be, oracle, 0, np.array([4, 9], np.int32), np.array([2, 1], np.int32), "cdef skipped block, apply")


@pytest.mark.parametrize("is16,bd", [(0, 8), (1, 10)])
@pytest.mark.parametrize("plane", ["luma", "c420"])
def test_cdef_frame_rows_geometry(be, oracle, plane, is16, bd):
    """svt_hip_cdef_frame_rows, one filter-block row per call in reverse order: every strip's top and bottom halo rows belong to another strip; plus empty ranges"""
    w, h, xdec, ydec, pli = (72, 136, 0, 0, 0) if plane == "luma" else (36, 68, 1, 1, 1)
    g = rng(2200 + w + bd)
    c = CdefCase(g, w, h, xdec, ydec, pli, is16, bd)
    assert c.nvfb == 3
    rows = [(1, 1), (c.nvfb, c.nvfb + 2)] + [(r, r + 1) for r in reversed(range(c.nvfb))] + [(2, 1)]
    pri, sec = cand_arrays(CDEF_CANDS)
    tag = "cdef rows %s is16 %d bd %d" % (plane, is16, bd)
    c.run(be, oracle, 1, pri, sec, tag + " search", rows=rows)
    c.run(be, oracle, 0, *c.strengths(g), tag + " apply", rows=rows)


@pytest.mark.parametrize("gpw", ["2", "4"])
def test_cdef_search_groups_per_workgroup_geometry(be, oracle, gpw):
    """several primary-level groups per workgroup (SVT_HIP_CDEF_GPW) on strided, guarded buffers: luma 136x72 and 4:2:0 chroma 68x36"""
    g = rng(2300 + int(gpw))
    pri, sec = cand_arrays([(pr, sc) for pr in (0, 1, 2, 3, 5, 7, 8, 11, 12, 15) for sc in (0, 2, 4)] + [(4, 1)])
    with tuning(be, "SVT_HIP_CDEF_GPW", gpw):
        for (geom, sub) in (("luma136x72", 2), ("c420_68x36", 1)):
            w, h, xdec, ydec, pli = CDEF_GEOM[geom]
            CdefCase(g, w, h, xdec, ydec, pli, 1, 10).run(be, oracle, 1, pri, sec, "cdef search %s SVT_HIP_CDEF_GPW=%s" % (geom, gpw), sub=sub)


# ======================================================================================================================================================================
# 3. deblocking
# ======================================================================================================================================================================
LPF_DEPTH = [(0, 8), (1, 10), (1, 12), (1, 8)]
LPF_MARGIN = 16  # svt_hip_lpf_plane_host reads this many samples left and right of every row


def lpf_plane(g, w, h, is16, bd):
    """(Plane, flat buffer): stride w + 32 + 5, the picture one margin into its rows, random in-range samples everywhere (the plane is filtered in place, and the host
    form reads its margins)"""
    pl = Plane(w, h, w + 2 * LPF_MARGIN + 5, LPF_MARGIN + 5, np.uint16 if is16 else np.uint8)
    pic = np.empty((h, w), np.int64)
    for y0 in range(0, h, 32):
        for x0 in range(0, w, 32):
            pic[y0:y0 + 32, x0:x0 + 32] = make_patch(g, bd, int(g.integers(0, 3)), (min(32, h - y0), min(32, w - x0)))
    return pl, pl.noisy(g, pic, bd)


def lpf_device(be, pl, flat, is16, bd, batches):
    d = be.dev(flat)
    keep = []
    for e in batches:
        keep.append(be.dev(e) if len(e) else None)
        be.lib.svt_hip_lpf_edges_batch(dev_ptr(be, d, pl), pl.stride, is16, bd, be.ptr(keep[-1]) if len(e) else None, len(e), be.stream)
    return be.host(d)


def lpf_host(be, pl, flat, is16, bd, vert, horz):
    work = flat.copy()
    assert be.lib.svt_hip_lpf_plane_host(pl.host_ptr(work), pl.stride, pl.w, pl.h, is16, bd, p(vert) if len(vert) else None, len(vert), p(horz) if len(horz) else None,
                                         len(horz)) == 0
    return work


@pytest.mark.parametrize("is16,bd", LPF_DEPTH)
@pytest.mark.parametrize("w,h", [(52, 36), (68, 44), (36, 68), (132, 20)])
def test_lpf_plane_geometry(be, oracle, w, h, is16, bd):
    """svt_hip_lpf_edges_batch (vertical pass, then horizontal pass) and svt_hip_lpf_plane_host on a strided plane with 16-, 8- and 4-sample-grid edges: both equal the
    oracle applied edge by edge in the same order, over the whole buffer -- margins, row gaps, lead and tail included"""
    g = rng(3000 + w + 3 * h + bd + is16)
    pl, flat = lpf_plane(g, w, h, is16, bd)
    vert, horz = lpf_edge_lists(g, w, h, be.pkg.LpfEdge, limits)
    assert {4, 6, 8, 14} == set(vert["length"]) | set(horz["length"]) and (vert["x"] % 8 == 4).any() and (horz["y"] % 8 == 4).any()
    want = flat.copy()
    lpf_oracle(oracle, want, pl, vert, is16, bd)
    lpf_oracle(oracle, want, pl, horz, is16, bd)
    assert not np.array_equal(want, flat)
    tag = "lpf %dx%d is16 %d bd %d" % (w, h, is16, bd)
    pl.check(lpf_device(be, pl, flat, is16, bd, (vert, horz)), want, tag + " edges_batch")
    pl.check(lpf_host(be, pl, flat, is16, bd, vert, horz), want, tag + " plane_host")


@pytest.mark.parametrize("is16,bd", [(0, 8), (1, 12)])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_lpf_batch_at_workgroup_boundary(be, oracle, n, is16, bd):
    """one launch of exactly 255 / 256 / 257 segments (one thread each, 256 threads per workgroup), cut from one list"""
    g = rng(3100 + bd)
    pl, flat = lpf_plane(g, 132, 68, is16, bd)
    vert, _ = lpf_edge_lists(g, 132, 68, be.pkg.LpfEdge, limits)
    assert len(vert) >= 257
    want = flat.copy()
    lpf_oracle(oracle, want, pl, vert[:n], is16, bd)
    pl.check(lpf_device(be, pl, flat, is16, bd, (vert[:n],)), want, "lpf batch n %d is16 %d bd %d" % (n, is16, bd))


@pytest.mark.parametrize("is16,bd", [(0, 8), (1, 10)])
def test_lpf_plane_host_empty_lists(be, oracle, is16, bd):
    """svt_hip_lpf_plane_host with no vertical segments, no horizontal segments, and neither"""
    g = rng(3200 + bd)
    pl, flat = lpf_plane(g, 52, 36, is16, bd)
    vert, horz = lpf_edge_lists(g, 52, 36, be.pkg.LpfEdge, limits)
    for (v, hz, tag) in ((vert[:0], horz, "n_vert 0"), (vert, horz[:0], "n_horz 0"), (vert[:0], horz[:0], "both 0")):
        want = flat.copy()
        lpf_oracle(oracle, want, pl, v, is16, bd)
        lpf_oracle(oracle, want, pl, hz, is16, bd)
        pl.check(lpf_host(be, pl, flat, is16, bd, v, hz), want, "lpf plane_host %s is16 %d bd %d" % (tag, is16, bd))


def test_lpf_single_call_symbols_12bit(be, oracle):
    """tests/test_deblock.py::test_lpf_single_call_symbols stops at 10 bit; the 12-bit clamp of sclamp through the svt_aom_highbd_lpf_*_hip symbols"""
    bd = 12
    g = rng(210 + bd)
    for ln in LENS:
        for vert in (0, 1):
            f = getattr(be.lib, "svt_aom_highbd_lpf_%s_%d_hip" % ("vertical" if vert else "horizontal", ln))
            for it in range(12 if be.is_gpu else 3):
                a = make_patch(g, bd, it % 3).astype(np.uint16)
                b = a.copy()
                bl, li, th = limits(g, it % 2)
                off = (16 * 32 + 16) * a.itemsize
                oracle.oracle_lpf(C.c_void_p(a.ctypes.data + off), 32, 1, vert, ln, bl, li, th, bd)
                keep = lim_arrays(bl, li, th)
                f(C.c_void_p(b.ctypes.data + off), 32, *[p(k) for k in keep], bd)
                assert np.array_equal(a, b), (ln, vert, it)


# ======================================================================================================================================================================
# 4. CDEF strength pick
# ======================================================================================================================================================================
NS = 64
PICK_COUNTS = [1, 127, 128, 129, 255, 256, 257, 4097]  # search_tot_kernel slices by 128, one thread per block in 256-thread workgroups; search_best_kernel covers
PICK_RANGES = [(0, 64), (5, 37)]                        # max(sb_count, 4096) threads


def pick_workspace(m0, m1, lev0, lev1, nb, n, s, e):
    """what the search leaves in its workspace: the 64 x 64 totals (rows [s, e) only; the rest cleared), then the best_i of every block"""
    with np.errstate(over="ignore"):
        best = np.full(n, 1 << 63, np.uint64)
        for gi in range(nb):
            best = np.minimum(best, m0[:, lev0[gi]] + m1[:, lev1[gi]])
        tot = np.zeros((NS, NS), np.uint64)
        for j in range(s, e):
            tot[j] = np.minimum(best[:, None], m0[:, j:j + 1] + m1).sum(axis=0, dtype=np.uint64)
    return np.concatenate([tot.reshape(-1), best])


def run_pick(be, oracle, m0, m1, n, s, e, rounds, tag, rtcd=True):
    """`rounds` successive svt_search_one_dual calls (each adds a pair), device form and RTCD form against the oracle"""
    oracle.oracle_search_one_dual.restype = C.c_uint64
    arr, keep = ptr_tables(m0, m1)
    la, lb, ha, hb = (np.zeros(9, np.int32) for _ in range(4))
    d0, d1 = be.dev(m0), be.dev(m1)
    got = []
    for nb in range(rounds):
        want = oracle.oracle_search_one_dual(p(la), p(lb), nb, p(m0), p(m1), n, s, e)
        if rtcd:
            r = be.lib.svt_search_one_dual_hip(p(ha), p(hb), nb, arr, n, s, e)
            assert r == want and np.array_equal(la, ha) and np.array_equal(lb, hb), (tag, "rtcd form", nb, r, want, ha, la, hb, lb)
        lev = [table(NS + 1, I32_FILL, np.int32) for _ in range(2)]
        lev[0][:nb], lev[1][:nb] = la[:nb], lb[:nb]
        dla, dlb = be.dev(lev[0]), be.dev(lev[1])
        dbest, ws = be.dev(table(1, U64_FILL, np.uint64)), be.dev(table(NS * NS + n, U64_FILL, np.uint64))
        be.lib.svt_hip_cdef_search_one_dual(be.ptr(d0), be.ptr(d1), be.ptr(dla), be.ptr(dlb), nb, n, s, e, be.ptr(dbest), be.ptr(ws), be.stream)
        lev[0][nb], lev[1][nb] = la[nb], lb[nb]
        t = "%s nb %d" % (tag, nb)
        check_table(be.host(dla), lev[0], nb + 1, t + " lev0")
        check_table(be.host(dlb), lev[1], nb + 1, t + " lev1")
        wbest = table(1, U64_FILL, np.uint64)
        wbest[0] = want
        check_table(be.host(dbest), wbest, 1, t + " best_tot_mse")
        wws = table(NS * NS + n, U64_FILL, np.uint64)
        wws[:NS * NS + n] = pick_workspace(m0, m1, la, lb, nb, n, s, e)
        check_table(be.host(ws), wws, NS * NS + n, t + " workspace")
        got.append((int(la[nb]), int(lb[nb])))
    return got


@pytest.mark.parametrize("s,e", PICK_RANGES)
@pytest.mark.parametrize("n", PICK_COUNTS)
def test_cdef_pick_counts(be, oracle, n, s, e):
    """svt_hip_cdef_search_one_dual and svt_search_one_dual_hip with filter-block counts at the slice (128), workgroup (256) and 4096-thread boundaries; the
    workspace and the level arrays carry sentinel tails.  (4097 blocks: an 8K picture has 8160.)  Three successive searches per case; at 4097 blocks two on the
    MI355X and one on the CPU interpreter, where a search over 4097 blocks takes about two seconds."""
    m0, m1 = tables(rng(4000 + n + s), n)
    run_pick(be, oracle, m0, m1, n, s, e, 3 if n < 4097 else (2 if be.is_gpu else 1), "pick n %d range [%d, %d)" % (n, s, e))


@pytest.mark.parametrize("s,e", PICK_RANGES)
@pytest.mark.parametrize("n", [1, 127, 129, 256, 257])
def test_cdef_pick_joint_search_and_assignment_counts(be, oracle, n, s, e):
    """svt_hip_cdef_joint_strength_search + svt_hip_cdef_assign_fb_strengths at the same boundaries, best_gi with a sentinel tail"""
    oracle.oracle_joint_strength_search.restype = C.c_uint64
    nb = 2
    m0, m1 = tables(rng(4100 + n + s), n)
    la, lb = np.zeros(9, np.int32), np.zeros(9, np.int32)
    want = oracle.oracle_joint_strength_search(p(la), p(lb), nb, p(m0), p(m1), n, s, e)
    wgi = table(n, I8_FILL, np.int8)
    oracle.oracle_assign_fb_strengths(p(m0), p(m1), p(la), p(lb), nb, n, p(wgi))
    d0, d1 = be.dev(m0), be.dev(m1)
    dla, dlb = be.dev(table(NS + 1, I32_FILL, np.int32)), be.dev(table(NS + 1, I32_FILL, np.int32))
    dbest, ws, dgi = be.dev(table(1, U64_FILL, np.uint64)), be.dev(table(NS * NS + n, U64_FILL, np.uint64)), be.dev(table(n, I8_FILL, np.int8))
    be.lib.svt_hip_cdef_joint_strength_search(be.ptr(d0), be.ptr(d1), be.ptr(dla), be.ptr(dlb), nb, n, s, e, be.ptr(dbest), be.ptr(ws), be.stream)
    be.lib.svt_hip_cdef_assign_fb_strengths(be.ptr(d0), be.ptr(d1), be.ptr(dla), be.ptr(dlb), nb, n, be.ptr(dgi), be.stream)
    tag = "joint n %d range [%d, %d)" % (n, s, e)
    wl = [table(NS + 1, I32_FILL, np.int32) for _ in range(2)]
    wl[0][:nb], wl[1][:nb] = la[:nb], lb[:nb]
    check_table(be.host(dla), wl[0], nb, tag + " lev0")
    check_table(be.host(dlb), wl[1], nb, tag + " lev1")
    assert int(be.host(dbest)[0]) == want and np.all(be.host(dbest)[1:] == np.uint64(U64_FILL)), tag
    assert np.all(be.host(ws)[NS * NS + n:] == np.uint64(U64_FILL)), tag + ": written past the workspace"
    check_table(be.host(dgi), wgi, n, tag + " best_gi")


@pytest.mark.parametrize("n", [2, 256])
def test_cdef_pick_ties(be, oracle, n):
    """equal totals: the first (j, k) in raster order wins (svt_search_one_dual_c takes a strictly smaller total only).  search_pick_kernel gives element e = 64 j + k
    to wave (e >> 6) & 3 = j & 3, so minima at j = 5 and j = 6 are found by different waves and meet only in the last step of its reduction."""
    # every total equal: the first pair of the range
    for (s, e) in PICK_RANGES:
        m0, m1 = np.full((n, NS), 1000, np.uint64), np.full((n, NS), 500, np.uint64)
        assert run_pick(be, oracle, m0, m1, n, s, e, 1, "pick all totals equal, n %d range [%d, %d)" % (n, s, e)) == [(s, s)]
    # two equal strict minima at (5, 60) and (6, 3).  Totals of the first round are sums a_j + b_k, whose minima always form a rectangle; with one pair (0, 0) selected
    # every block's term is capped by its best_i = 2000.  Even blocks fall below the cap only at (5, 60) (900 + 900), odd blocks only at (6, 3); the next smallest
    # entries, (0, 60) / (5, 0) / (0, 3) / (6, 0), reach 1900 in half of the blocks.
    big = 1 << 20
    m0, m1 = np.full((n, NS), big, np.uint64), np.full((n, NS), big, np.uint64)
    m0[:, 0] = m1[:, 0] = 1000
    m0[0::2, 5] = m1[0::2, 60] = 900
    m0[1::2, 6] = m1[1::2, 3] = 900
    ws = pick_workspace(m0, m1, [0], [0], 1, n, 0, NS)[:NS * NS].reshape(NS, NS)
    lo = n * 2000 - (n // 2) * 200
    assert ws[5, 60] == ws[6, 3] == lo and (ws < lo).sum() == 0 and (ws == lo).sum() == 2
    assert run_pick(be, oracle, m0, m1, n, 0, NS, 2, "pick two equal minima, n %d" % n) == [(0, 0), (5, 60)]
