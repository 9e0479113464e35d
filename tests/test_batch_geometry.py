"""The batched transform / quantiser entry points at workgroup boundaries, every block of every launch against the oracle.

The kernels place B = 256 / max(W, H) blocks in a workgroup (64 for the Walsh-Hadamard batches, 256 / min(64, n_coeffs / 4) for the quantizer, 1 for
svt_handle_transform).  Every entry point runs at n in {1, B - 1, B, B + 1, 2B + B/2} and, on the GPU, at 300 B + 1 (301 workgroups, more than the device has CUs,
with a tail of one block; 3 B + 1 on the CPU interpreter, which also runs the sizes of 2048 pixels or more at {1, B + 1} only).  Every launch
  * stores block i in slot perm[i] of its planes (a seeded permutation) and mixes two strides by slot (batch_geometry_common.Layout),
  * cycles the transform types so that a block's type is not a function of its place in the workgroup,
  * writes into arrays B blocks (slots) longer than n, filled with a sentinel, which are compared WHOLE with an expected array built from the oracle: a store past
    block n - 1, into the gap between strided rows or outside a block's W x H fails the test,
and the launches that reconstruct run once more in place (pred_base == recon_base, pred_off == recon_off: include/svtav1_hip.h allows it).
Non-vacuity is asserted on the oracle's output: every inverse launch clips at 0 and at 2^bd - 1; every quantizer / round-trip launch of a workgroup or more holds a
block with eob == 0 and one with eob > ncoef / 2."""
import ctypes as C

import numpy as np
import pytest

import batch_geometry_common as bg
from conftest import p, rng
from quant_common import DEQUANTS, make_qparams, make_scan, oracle_roundtrip
from test_oracle_pin_quant import run_oracle
from test_oracle_pin_txfm import TX_SIZES, TXH, TXW, allowed_types, c_defined_types

ALL_SIZES = list(range(19))
SIZES_32 = [t for t in ALL_SIZES if 32 in (TXW[t], TXH[t])]  # the sizes whose `_any_type` form is a kernel of its own
SIZES_64 = [4, 11, 12, 17, 18]


def bpw(ts):
    return 256 // max(TXW[ts], TXH[ts])


# ---- forward --------------------------------------------------------------------------------------------------------------------------------------------------
def fwd_launch(be, oracle, g, ts, n, bd, pf):
    w, h, B = TXW[ts], TXH[ts], bpw(ts)
    amp = (1 << bd) - 1
    L = bg.Layout(g, n, B, w, h)
    plane = g.integers(-amp, amp + 1, L.size).astype(np.int16)  # (the gaps and the unused slots hold residual-like data too)
    plane[L.idx[0]] = amp  # extreme block
    res = plane[L.idx]
    types = bg.type_cycle(g, allowed_types(ts), n + B, B)
    descs = np.zeros(n + B, dtype=be.pkg.FwdTxfmDesc)  # (the descriptors past n - 1 name the unused slots: Layout)
    descs["in_off"], descs["in_stride"], descs["tx_type"] = L.off_all, L.stride_all, types
    want = np.full((n + B, w * h), bg.I32_FILL, np.int32)
    for i in range(n):
        oracle.oracle_fwd_txfm2d(p(res[i]), p(want[i]), w, int(types[i]), ts, bd, pf)
    dpl, dd = be.dev(plane), be.dev(descs)
    out = bg.filled(be, (n + B, w * h), bg.I32_FILL, np.int32)
    be.lib.svt_hip_fwd_txfm2d_batch(be.ptr(dpl), be.ptr(dd), n, ts, bd, pf, be.ptr(out), be.stream)
    bg.check_rows(be.host(out), want, n, ("fwd", TX_SIZES[ts], "n", n, "bd", bd, "pf", pf))


@pytest.mark.parametrize("ts", ALL_SIZES)
def test_fwd_txfm2d_batch(be, oracle, ts):
    g, B = rng(4000 + ts), bpw(ts)
    for n in bg.block_counts(be, B, TXW[ts] * TXH[ts]):
        fwd_launch(be, oracle, g, ts, n, 10, 0)
    for pf in (1, 2):
        fwd_launch(be, oracle, g, ts, B + 1, 10, pf)
    if be.is_gpu:
        for bd in (8, 12):
            fwd_launch(be, oracle, g, ts, B + 1, bd, 0)


# ---- inverse + reconstruction ---------------------------------------------------------------------------------------------------------------------------------
def inv_launch(be, oracle, g, ts, n, bd, u8, any_type, inplace):
    """one launch (and, `inplace`, the same launch again with the reconstruction written over the prediction); input = the oracle's forward transform of a random
    residual (test/InvTxfm2dAsmTest.cc:92-145).  The oracle has no forward 32-point ADST, so the `_any_type` forms take DCT_DCT coefficients: conformant in range."""
    w, h, B = TXW[ts], TXH[ts], bpw(ts)
    iw, ih = min(w, 32), min(h, 32)
    ncoef, amp = iw * ih, (1 << bd) - 1
    dt, fill = (np.uint8, 0xA5) if u8 else (np.uint16, 0xA5A5)
    L = bg.Layout(g, n, B, w, h)
    cperm = g.permutation(n + B)  # coefficient blocks are permuted on their own
    types = bg.type_cycle(g, c_defined_types(ts) if any_type else allowed_types(ts), n + B, B)
    coeffs = g.integers(-(1 << 20), 1 << 20, (n + B, ncoef)).astype(np.int32)
    predb = g.integers(0, amp + 1, (n, h, w)).astype(np.uint16)
    wantb = np.zeros((n, h, w), np.uint16)
    full = np.zeros(w * h, np.int32)
    for i in range(n):
        res = g.integers(-amp, amp + 1, h * w).astype(np.int16)
        oracle.oracle_fwd_txfm2d(p(res), p(full), w, 0 if any_type else int(types[i]), ts, bd, 0)
        coeffs[cperm[i]] = full.reshape(h, w)[:ih, :iw].reshape(-1)
        oracle.oracle_inv_txfm2d_add(p(coeffs[cperm[i]]), p(predb[i]), w, p(wantb[i]), w, int(types[i]), ts, bd)
    assert (wantb == 0).any() and (wantb == amp).any(), "no clipping in this launch"
    pred_plane, want_plane = L.plane(predb, fill, dt), L.plane(wantb, fill, dt)
    descs = np.zeros(n + B, dtype=be.pkg.InvTxfmDesc)
    descs["coeff_off"], descs["pred_off"], descs["recon_off"] = cperm * ncoef, L.off_all, L.off_all
    descs["pred_stride"], descs["recon_stride"], descs["tx_type"] = L.stride_all, L.stride_all, types
    dco, dd = be.dev(coeffs), be.dev(descs)
    f = getattr(be.lib, "svt_hip_inv_txfm2d_add_batch" + ("_any_type" if any_type else "") + ("_u8" if u8 else ""))
    for alias in ((False, True) if inplace else (False,)):
        dpr = be.dev(pred_plane)
        drc = dpr if alias else bg.filled(be, L.size, fill, dt)
        f(be.ptr(dco), be.ptr(dpr), be.ptr(drc), be.ptr(dd), n, ts, *(() if u8 else (bd,)), be.stream)
        L.check(be.host(drc), want_plane, (f.__name__, TX_SIZES[ts], "n", n, "bd", bd, "in place" if alias else "two planes"))


def inv_case(be, oracle, ts, seed, u8, any_type):
    g, B = rng(seed + ts), bpw(ts)
    bd = 8 if u8 else 10
    for n in bg.block_counts(be, B, TXW[ts] * TXH[ts]):
        inv_launch(be, oracle, g, ts, n, bd, u8, any_type, inplace=n in bg.inplace_counts(be, B))
    if be.is_gpu and not u8:
        inv_launch(be, oracle, g, ts, B + 1, 12, u8, any_type, inplace=False)


@pytest.mark.parametrize("ts", ALL_SIZES)
def test_inv_txfm2d_add_batch(be, oracle, ts):
    inv_case(be, oracle, ts, 4100, u8=False, any_type=False)


@pytest.mark.parametrize("ts", ALL_SIZES)
def test_inv_txfm2d_add_batch_u8(be, oracle, ts):
    inv_case(be, oracle, ts, 4200, u8=True, any_type=False)


@pytest.mark.parametrize("ts", SIZES_32)
def test_inv_txfm2d_add_batch_any_type(be, oracle, ts):
    inv_case(be, oracle, ts, 4300, u8=False, any_type=True)


@pytest.mark.parametrize("ts", SIZES_32)
def test_inv_txfm2d_add_batch_any_type_u8(be, oracle, ts):
    inv_case(be, oracle, ts, 4400, u8=True, any_type=True)


# ---- 4x4 Walsh-Hadamard ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_wht4x4_batches(be, oracle, bd):
    """svt_hip_fwht4x4_batch, svt_hip_iwht4x4_add_batch and (at 8 bit) svt_hip_iwht4x4_add_batch_u8; the 16-coefficient / DC-only form alternates on bit 1 of
    the block's slot number, which is neither the block's parity nor a function of its lane."""
    g, B = rng(4500 + bd), 64
    amp = (1 << bd) - 1
    for n in bg.block_counts(be, B):
        L = bg.Layout(g, n, B, 4, 4)
        plane = g.integers(-amp, amp + 1, L.size).astype(np.int16)
        plane[L.idx[0]] = amp
        if n > 1:
            plane[L.idx[1]] = -amp
        res = plane[L.idx]
        fd = np.zeros(n + B, dtype=be.pkg.FwdTxfmDesc)
        fd["in_off"], fd["in_stride"] = L.off_all, L.stride_all
        want = np.full((n + B, 16), bg.I32_FILL, np.int32)
        for i in range(n):
            oracle.oracle_fwht4x4(p(res[i]), p(want[i]), 4)
        dpl, dfd = be.dev(plane), be.dev(fd)
        out = bg.filled(be, (n + B, 16), bg.I32_FILL, np.int32)
        be.lib.svt_hip_fwht4x4_batch(be.ptr(dpl), be.ptr(dfd), n, be.ptr(out), be.stream)
        bg.check_rows(be.host(out), want, n, ("fwht", "n", n, "bd", bd))
        # inverse: the forward's own output for half of the blocks, raw coefficients for the rest (as tests/test_txfm.py::test_wht4x4)
        Lp = bg.Layout(g, n, B, 4, 4)
        cperm = g.permutation(n + B)
        full = ((Lp.perm_all >> 1) & 1).astype(np.uint8)
        wantb = np.zeros((n, 4, 4), np.uint16)
        for _ in range(64):  # (a launch of one or two 4x4 blocks does not clip at both ends by itself: draw until the ORACLE's output does)
            coeffs = g.integers(-(amp << 4), (amp << 4) + 1, (n + B, 16)).astype(np.int32)
            coeffs[cperm[:n // 2]] = want[:n // 2]
            predb = g.integers(0, amp + 1, (n, 4, 4)).astype(np.uint16)
            for i in range(n):
                oracle.oracle_iwht4x4_add(p(coeffs[cperm[i]]), p(predb[i]), 4, p(wantb[i]), 4, 16 if full[i] else 1, bd)
            lo, hi = (wantb == 0).any(), (wantb == amp).any()
            if (lo and hi) or ((lo or hi) and not full[:n].any()):
                break
        # (the DC-only form adds a residual of one sign: a launch without a 16-coefficient block can clip at one end only)
        assert (lo and hi) or ((lo or hi) and not full[:n].any()), "no clipping in this launch"
        idesc = np.zeros(n + B, dtype=be.pkg.InvTxfmDesc)
        idesc["coeff_off"], idesc["pred_off"], idesc["recon_off"] = cperm * 16, Lp.off_all, Lp.off_all
        idesc["pred_stride"], idesc["recon_stride"], idesc["wht_full"] = Lp.stride_all, Lp.stride_all, full
        dco, dd = be.dev(coeffs), be.dev(idesc)
        for u8 in ((False, True) if bd == 8 else (False,)):
            dt, fill = (np.uint8, 0xA5) if u8 else (np.uint16, 0xA5A5)
            pred_plane, want_plane = Lp.plane(predb, fill, dt), Lp.plane(wantb, fill, dt)
            for alias in ((False, True) if n in bg.inplace_counts(be, B) else (False,)):
                dpr = be.dev(pred_plane)
                drc = dpr if alias else bg.filled(be, Lp.size, fill, dt)
                if u8:
                    be.lib.svt_hip_iwht4x4_add_batch_u8(be.ptr(dco), be.ptr(dpr), be.ptr(drc), be.ptr(dd), n, be.stream)
                else:
                    be.lib.svt_hip_iwht4x4_add_batch(be.ptr(dco), be.ptr(dpr), be.ptr(drc), be.ptr(dd), n, bd, be.stream)
                Lp.check(be.host(drc), want_plane, ("iwht", "u8" if u8 else "u16", "n", n, "bd", bd, "in place" if alias else "two planes"))


# ---- quantizer ------------------------------------------------------------------------------------------------------------------------------------------------
def quant_inputs(g, n, extra, n_coeffs, hbd):
    """[n + extra][n_coeffs] coefficients: per block an amplitude class and a density class (dense, sparse, small tail, all zero: test_oracle_pin_quant.gen_coeff);
    block 1 dense at full amplitude and block 2 within +-3 (with the finest / coarsest step they give eob > n_coeffs / 2 and eob == 0); the tail rows are data too"""
    amps = np.array([40, 1 << 11, 1 << 15, (1 << 18) if hbd else (1 << 15)])[g.integers(0, 4, n + extra)]
    c = g.integers(-amps[:, None], amps[:, None] + 1, (n + extra, n_coeffs))
    kind = g.integers(0, 4, n + extra)
    c[(kind == 1)[:, None] & (g.random((n + extra, n_coeffs)) < 0.8)] = 0
    tail = g.integers(-3, 4, (n + extra, n_coeffs))
    tail[:, :n_coeffs // 3] = c[:, :n_coeffs // 3]
    c = np.where((kind == 2)[:, None], tail, c)
    c[kind == 3] = 0
    if n >= 3:
        c[1] = g.integers(-(1 << 15), (1 << 15) + 1, n_coeffs)
        c[2] = g.integers(-3, 4, n_coeffs)
    return c.astype(np.int32)


@pytest.mark.parametrize("mode,qm", [(0, False), (1, False), (2, False), (3, False), (1, True), (2, True)])
def test_quantize_batch(be, oracle, mode, qm):
    g = rng(4600 + 10 * mode + int(qm))
    hbd = mode in (1, 3)
    deqs = [DEQUANTS[0], DEQUANTS[3], DEQUANTS[6] if hbd else DEQUANTS[5]]  # finest, middle, coarsest (the 8-bit quantizers see 8-bit tables only)
    plist = [make_qparams(dc, ac, fp=mode >= 2) for (dc, ac) in deqs]
    for n_coeffs, ls in ((16, 0), (32, 0), (64, 0), (128, 0), (256, 0), (512, 1), (1024, 1), (1024, 2)):  # log_scale by size class; 1024 = 32x32 and the 64-point sizes
        B = 256 // min(64, n_coeffs // 4)
        params = np.zeros(len(plist), dtype=be.pkg.QuantParams)
        for i, P in enumerate(plist):
            params[i] = (P["zbin"], P["round"], P["quant"], P["quant_shift"], P["dequant"], ls)
        sc = [make_scan(n_coeffs, g) for _ in range(2)]
        scans, iscans = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
        qmt, iqmt = g.integers(16, 255, (2, n_coeffs)).astype(np.uint8), g.integers(16, 64, (2, n_coeffs)).astype(np.uint8)
        dpa, dis, dqm, diq = be.dev(params), be.dev(iscans), be.dev(qmt), be.dev(iqmt)
        for n in bg.block_counts(be, B):
            coeff = quant_inputs(g, n, B, n_coeffs, hbd)
            descs = np.zeros(n + B, dtype=be.pkg.QuantDesc)
            descs["qparam_idx"], descs["iscan_idx"], descs["qm_idx"] = g.integers(0, 3, n + B), g.integers(0, 2, n + B), g.integers(0, 2, n + B)
            if n >= 3:
                descs["qparam_idx"][1:3] = (0, 2)
            wq, wdq = (np.full((n + B, n_coeffs), bg.I32_FILL, np.int32) for _ in range(2))
            weob = np.full(n + B, bg.U16_FILL, np.uint16)
            for b in range(n):
                d = descs[b]
                wq[b], wdq[b], weob[b] = run_oracle(oracle, mode, qm, coeff[b], n_coeffs, plist[int(d["qparam_idx"])], scans[int(d["iscan_idx"])],
                                                    qmt[int(d["qm_idx"])], iqmt[int(d["qm_idx"])], ls)
            if n >= B:
                assert (weob[:n] == 0).any() and (weob[:n] > n_coeffs // 2).any(), "vacuous launch"
            dco, dde = be.dev(coeff), be.dev(descs)
            q, dq = (bg.filled(be, (n + B, n_coeffs), bg.I32_FILL, np.int32) for _ in range(2))
            eob = bg.filled(be, n + B, bg.U16_FILL, np.uint16)
            be.lib.svt_hip_quantize_batch(mode, be.ptr(dco), n, n_coeffs, be.ptr(dpa), be.ptr(dis), be.ptr(dqm) if qm else None, be.ptr(diq) if qm else None,
                                          be.ptr(dde), be.ptr(q), be.ptr(dq), be.ptr(eob), be.stream)
            tag = ("mode", mode, "qm", qm, "n_coeffs", n_coeffs, "ls", ls, "n", n)
            bg.check_rows(be.host(q), wq, n, ("qcoeff",) + tag)
            bg.check_rows(be.host(dq), wdq, n, ("dqcoeff",) + tag)
            bg.check_rows(be.host(eob), weob, n, ("eob",) + tag)


# ---- svt_handle_transform -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2n4", [0, 1])
@pytest.mark.parametrize("ts", SIZES_64)
def test_handle_transform_batch(be, oracle, ts, n2n4):
    """one block per workgroup: n in {1, 2, 301}.  Energy and the kept corner of every block; the energy sentinel and the coefficient block past block n - 1 stay as
    they were.  (What the kernel leaves in a block's discarded area is not specified by the header and is not compared.)"""
    g = rng(4700 + 2 * ts + n2n4)
    oracle.oracle_handle_transform.restype = C.c_uint64
    w, h = TXW[ts], TXH[ts]
    kept = min(w, 32) * min(h, 32)
    for n in (1, 2, 301 if be.is_gpu else 5):
        x = g.integers(-(1 << 20), 1 << 20, (n + 1, w * h)).astype(np.int32)
        d = be.dev(x)
        e = bg.filled(be, n + 1, bg.U64_FILL, np.uint64)
        be.lib.svt_hip_handle_transform_batch(be.ptr(d), n, ts, n2n4, be.ptr(e), be.stream)
        got, ge = be.host(d), be.host(e)
        want, we = x.copy(), np.full(n + 1, bg.U64_FILL, np.uint64)
        for i in range(n):
            we[i] = oracle.oracle_handle_transform(p(want[i]), w, h, n2n4)
        tag = ("handle_transform", TX_SIZES[ts], "n2_n4", n2n4, "n", n)
        bg.check_rows(ge, we, n, ("energy",) + tag)
        got[:n, kept:] = want[:n, kept:]  # only the kept corner of a block is specified
        bg.check_rows(got, want, n, ("coefficients",) + tag)


# ---- the fused round trip, without and with the distortion terms ------------------------------------------------------------------------------------------------
def roundtrip_launch(be, oracle, g, ts, n, bd, fp, qm, dist, null_dq, inplace):
    """one launch of svt_hip_txfm_quant_roundtrip_batch (`dist`: of svt_hip_txfm_quant_roundtrip_dist_batch) against oracle_roundtrip block by block, then -- null_dq --
    again with dqcoeff == NULL and -- inplace -- again with the reconstruction written over the prediction."""
    w, h, B = TXW[ts], TXH[ts], bpw(ts)
    ncoef, pels = min(w, 32) * min(h, 32), w * h
    ls = int(pels > 256) + int(pels > 1024)
    qmode, amp = (1 if bd > 8 else 0) + 2 * fp, (1 << bd) - 1
    dt, fill = (np.uint16, 0xA5A5) if bd > 8 else (np.uint8, 0xA5)
    steps = [(4, 4), (88, 112), (1336, 1828)]  # (dc, ac) dequant steps of q_index 0, a middle one and 255 (8-bit tables; x 4 at 10 bit)
    plist = [make_qparams(dc * (4 if bd > 8 else 1), ac * (4 if bd > 8 else 1), fp=bool(fp)) for (dc, ac) in steps]
    params = np.zeros(len(plist), dtype=be.pkg.QuantParams)
    for i, P in enumerate(plist):
        params[i] = (P["zbin"], P["round"], P["quant"], P["quant_shift"], P["dequant"], ls)
    sc = [make_scan(ncoef, g) for _ in range(2)]
    scans, iscans = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
    qmt = g.integers(16, 255, (2, ncoef)).astype(np.uint8) if qm else None
    iqmt = g.integers(16, 64, (2, ncoef)).astype(np.uint8) if qm else None
    Lr, Lp = bg.Layout(g, n, B, w, h), bg.Layout(g, n, B, w, h)  # residual slots and pixel slots are permuted independently
    rplane = g.integers(-amp, amp + 1, Lr.size).astype(np.int16)
    rplane[Lr.idx[0]] = amp  # extreme block
    qi = g.integers(0, 3, n + B)
    if n >= 3:  # a full-amplitude residual at the finest step (block 1 as drawn), a nearly flat one at the coarsest
        rplane[Lr.idx[2]] = g.integers(-3, 4, (h, w))
        qi[1:3] = (0, 2)
    res = rplane[Lr.idx]
    predb = g.integers(0, amp + 1, (n, h, w)).astype(np.uint16)
    types = bg.type_cycle(g, allowed_types(ts), n + B, B)
    rd = np.zeros(n + B, dtype=be.pkg.RoundtripDesc)
    rd["in_off"], rd["pred_off"], rd["recon_off"] = Lr.off_all, Lp.off_all, Lp.off_all
    rd["in_stride"], rd["pred_stride"], rd["recon_stride"] = Lr.stride_all, Lp.stride_all, Lp.stride_all
    rd["qparam_idx"], rd["iscan_idx"], rd["qm_idx"], rd["tx_type"] = qi, g.integers(0, 2, n + B), g.integers(0, 2, n + B), types
    wq, wdq = (np.full((n + B, ncoef), bg.I32_FILL, np.int32) for _ in range(2))
    weob = np.full(n + B, bg.U16_FILL, np.uint16)
    wrec, co = np.zeros((n, h, w), np.uint16), np.zeros((n, ncoef), np.int32)
    for i in range(n):
        si, mi = int(rd[i]["iscan_idx"]), int(rd[i]["qm_idx"])
        wq[i], wdq[i], weob[i], wrec[i] = oracle_roundtrip(oracle, res[i], w, predb[i], w, w, h, int(types[i]), ts, bd, qmode, plist[int(qi[i])], scans[si],
                                                           qmt[mi] if qm else None, iqmt[mi] if qm else None, ls)
        if dist:
            co[i] = bg.forward_kept(oracle, res[i], w, h, int(types[i]), ts, bd)
    if n >= B:
        assert (weob[:n] == 0).any() and (weob[:n] > ncoef // 2).any(), "vacuous launch"
    pred_plane, want_plane = Lp.plane(predb, fill, dt), Lp.plane(wrec, fill, dt)
    dev = [be.dev(v) for v in (rplane, rd, params, iscans)]
    d_qm, d_iqm = (be.dev(qmt), be.dev(iqmt)) if qm else (None, None)
    wdist = None
    if dist:  # the source blocks live in a plane of their own, permuted again
        Ls = bg.Layout(g, n, B, w, h)
        srcb = g.integers(0, amp + 1, (n, h, w)).astype(np.uint16)
        sr = np.zeros(n + B, dtype=be.pkg.PlaneRef)
        sr["off"], sr["stride"] = Ls.off_all, Ls.stride_all
        d_src, d_sr = be.dev(Ls.plane(srcb, g.integers(0, amp + 1, Ls.size), dt)), be.dev(sr)
        wdist = np.full((n + B, 6), bg.U64_FILL, np.uint64)  # SvtHipRdDist: coeff_dist[2], sse_pred, sse_recon, psy_pred, psy_recon
        wdist[:n, 0:2] = bg.coeff_dist_rows(co, wdq[:n], weob[:n])
        wdist[:n, 2], wdist[:n, 4] = bg.pixel_dist_rows(srcb, predb, bd > 8)
        wdist[:n, 3], wdist[:n, 5] = bg.pixel_dist_rows(srcb, wrec, bd > 8)
    runs = [("two planes", True, False)] + ([("dqcoeff NULL", False, False)] if null_dq else []) + ([("in place", True, True)] if inplace else [])
    for name, with_dq, alias in runs:
        dpr = be.dev(pred_plane)
        drc = dpr if alias else bg.filled(be, Lp.size, fill, dt)
        q, dq = (bg.filled(be, (n + B, ncoef), bg.I32_FILL, np.int32) for _ in range(2))
        eob = bg.filled(be, n + B, bg.U16_FILL, np.uint16)
        args = [be.ptr(dev[0]), be.ptr(dpr), be.ptr(drc), be.ptr(dev[1]), n, ts, bd, qmode, be.ptr(dev[2]), be.ptr(dev[3]), be.ptr(d_qm) if qm else None,
                be.ptr(d_iqm) if qm else None, be.ptr(q), be.ptr(dq) if with_dq else None, be.ptr(eob)]
        tag = ("roundtrip_dist" if dist else "roundtrip", TX_SIZES[ts], "n", n, "bd", bd, "qmode", qmode, "qm", qm, name)
        if dist:
            out = bg.filled(be, (n + B, 6), bg.U64_FILL, np.uint64)
            be.lib.svt_hip_txfm_quant_roundtrip_dist_batch(*args, be.ptr(d_src), be.ptr(d_sr), be.ptr(out), be.stream)
        else:
            be.lib.svt_hip_txfm_quant_roundtrip_batch(*args, be.stream)
        bg.check_rows(be.host(q), wq, n, ("qcoeff",) + tag)
        bg.check_rows(be.host(dq), wdq if with_dq else np.full_like(wdq, bg.I32_FILL), n, ("dqcoeff",) + tag)
        bg.check_rows(be.host(eob), weob, n, ("eob",) + tag)
        Lp.check(be.host(drc), want_plane, ("recon",) + tag)
        if dist:
            got = be.host(out)
            if alias:  # the pixel terms are a second launch on the planes as the round trip left them: in place, the prediction it would measure is gone
                got[:n, [2, 4]] = wdist[:n, [2, 4]]
            bg.check_rows(got, wdist, n, ("SvtHipRdDist",) + tag)


def roundtrip_case(be, oracle, ts, seed, dist):
    g, B = rng(seed + ts), bpw(ts)
    # (bit depth, quantize_fp, matrices): the u16 and the u8 kernel through quantize_b, and quantize_fp with matrices (the family is a run-time argument of the same
    # kernels, so the in-place launches run with the first two).  dqcoeff == NULL: the boundary counts of the first pair (with the distortions: tests/test_dist.py)
    pairs = ((10, 0, False), (8, 0, False), (10, 1, True)) if be.is_gpu else ((10, 0, False),)
    for k, (bd, fp, qm) in enumerate(pairs):
        for n in bg.block_counts(be, B, TXW[ts] * TXH[ts]):
            roundtrip_launch(be, oracle, g, ts, n, bd, fp, qm, dist, null_dq=k == 0 and not dist and n != bg.many_count(be, B),
                             inplace=k < 2 and n in bg.inplace_counts(be, B))


@pytest.mark.parametrize("ts", ALL_SIZES)
def test_txfm_quant_roundtrip_batch(be, oracle, ts):
    roundtrip_case(be, oracle, ts, 4800, dist=False)


@pytest.mark.parametrize("ts", ALL_SIZES)
def test_txfm_quant_roundtrip_dist_batch(be, oracle, ts):
    roundtrip_case(be, oracle, ts, 4900, dist=True)
