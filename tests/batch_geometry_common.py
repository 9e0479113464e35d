"""Launch geometry shared by tests/test_batch_geometry.py: the block counts around a workgroup boundary, a storage layout in which block order, slot order and
stride are independent, sentinel-filled outputs that are compared whole, and a report that names the first block that differs."""
import math

import numpy as np

I32_FILL, U16_FILL, U64_FILL = 0x5A5A5A5A, 0x5A5A, 0x5A5A5A5A5A5A5A5A  # outputs that are not pixels; recon planes carry 0xA5 / 0xA5A5
U64 = np.uint64


def many_count(be, B):
    """301 workgroups with a tail of one block: more workgroups than the device has CUs.  The CPU interpreter runs four workgroups with the same tail."""
    return 300 * B + 1 if be.is_gpu else 3 * B + 1


def block_counts(be, B, pels=0):
    """n around the boundaries of a kernel that places B blocks in a workgroup: one block, one short of a workgroup, exactly one, one more (a full workgroup and a
    tail of one), two and a half, and the many-workgroup launch.  The CPU interpreter runs the sizes of 2048 pixels or more at {1, B + 1} only."""
    if not be.is_gpu and pels >= 2048:
        return [1, B + 1]
    return sorted({v for v in (1, B - 1, B, B + 1, 2 * B + B // 2, many_count(be, B)) if v >= 1})


def inplace_counts(be, B):
    return [B + 1, many_count(be, B)] if be.is_gpu else [B + 1]


def type_cycle(g, types, n, B):
    """Transform types cycling through `types` from a seeded offset with a step coprime to their number; the cycle advances once more per workgroup, so that the type
    of a block is not a function of its place in the workgroup even where the number of types divides B."""
    m = len(types)
    steps = [k for k in range(1, m + 1) if math.gcd(k, m) == 1]
    off, step = int(g.integers(m)), steps[int(g.integers(len(steps)))]
    return np.array([types[(off + step * (i + i // B)) % m] for i in range(n)], np.uint8)


class Layout:
    """n blocks of w x h samples stored in n + extra slots of one flat plane.  Block i lives in slot perm[i] (a seeded permutation: block order and storage order are
    independent; the slots no block uses lie anywhere and are named by the descriptors past n - 1).  Even slots have stride w + 3, odd slots w + 8 rounded up to an odd number; a slot is h rows of the larger."""

    def __init__(self, g, n, extra, w, h):
        self.n, self.w, self.h = n, w, h
        self.perm_all = g.permutation(n + extra).astype(np.int64)
        self.perm = self.perm_all[:n]
        strides = (w + 3, (w + 8) | 1)
        self.slot = h * strides[1]
        self.size = (n + extra) * self.slot
        # descriptor arrays are n + extra long as well: the entries past n - 1 name the unused slots, so a kernel that takes one block too many reads a valid
        # descriptor and writes where the comparison sees it -- a failed assertion, not a wild access
        self.stride_all = np.where(self.perm_all & 1, strides[1], strides[0]).astype(np.int64)
        self.off_all = self.perm_all * self.slot
        self.stride, self.off = self.stride_all[:n], self.off_all[:n]
        self.idx = self.off[:, None, None] + np.arange(h)[None, :, None] * self.stride[:, None, None] + np.arange(w)[None, None, :]  # [n][h][w] -> element
        assert int(self.idx.max()) < self.size

    def plane(self, blocks, fill, dtype):
        """the flat plane: `fill` (a scalar, or a whole array for gaps that hold data) with the blocks' samples in place"""
        a = np.array(fill, dtype=dtype).reshape(-1).copy() if np.ndim(fill) else np.full(self.size, fill, dtype)
        assert a.size == self.size
        a[self.idx] = blocks
        return a

    def check(self, got, want, tag):
        """whole-plane comparison; on a difference name the first block that differs, or say that the damage lies outside every block"""
        got, want = got.reshape(-1), want.reshape(-1)
        if np.array_equal(got, want):
            return
        for i in range(self.n):
            a, b = got[self.idx[i]], want[self.idx[i]]
            assert np.array_equal(a, b), tag + ("block %d in slot %d, stride %d" % (i, self.perm[i], self.stride[i]), a[:2, :8], b[:2, :8])
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d samples outside every block's W x H were written (gap between strided rows, unused slot, or past block n - 1), the first at "
                             "element %d = slot %d" % (tag, bad.size, bad[0], bad[0] // self.slot))


def check_rows(got, want, n, tag):
    """per-block output arrays [n + extra][...]: name the first block that differs, or say that the sentinel past block n - 1 was written"""
    if np.array_equal(got, want):
        return
    for i in range(n):
        assert np.array_equal(got[i], want[i]), tag + ("block %d" % i, got[i], want[i])
    raise AssertionError("%s: written past block n - 1 (n = %d): rows %s" % (tag, n, n + np.flatnonzero((got[n:] != want[n:]).reshape(len(got) - n, -1).any(axis=1))[:8]))


def filled(be, shape, fill, dtype):
    return be.dev(np.full(shape, fill, dtype))


def forward_kept(oracle, res, w, h, tt, ts, bd):
    """the forward coefficients the round trip's quantizer sees, from the oracle: oracle_fwd_txfm2d, then (64-point sizes) oracle_handle_transform's repack; the kept
    min(w, 32) x min(h, 32) corner, packed -- the first two steps of quant_common.oracle_roundtrip"""
    import ctypes as C
    co = np.zeros(w * h, np.int32)
    oracle.oracle_fwd_txfm2d(C.c_void_p(res.ctypes.data), C.c_void_p(co.ctypes.data), w, tt, ts, bd, 0)
    if max(w, h) == 64:
        oracle.oracle_handle_transform.restype = C.c_uint64
        oracle.oracle_handle_transform(C.c_void_p(co.ctypes.data), w, h, 0)
    return co[:min(w, 32) * min(h, 32)].copy()


# ---- the six values of SvtHipRdDist from the oracle's coefficients and reconstruction, through tests/dist_common.py ----
def coeff_dist_rows(co, dq, eob):
    """dist_common.coeff_dist of every block ([n][ncoef] each; the cbf_zero form where eob == 0), in wrapping uint64 arithmetic; the first blocks are also
    computed by dist_common.coeff_dist itself (exact Python integers) and must agree."""
    import dist_common as dc
    c, r = co.astype(np.int64), dq.astype(np.int64)
    with np.errstate(over="ignore"):
        pred = (c.view(U64) * c.view(U64)).sum(axis=1, dtype=U64)
        d = (c - r).view(U64)
        res = (d * d).sum(axis=1, dtype=U64)
    out = np.stack([np.where(eob == 0, pred, res), pred], axis=1)
    for i in range(min(3, len(co))):
        assert tuple(int(v) for v in out[i]) == dc.coeff_dist(co[i], None if eob[i] == 0 else dq[i]), i
    return out


def pixel_dist_rows(src, rec, hbd):
    """(sse, raw psy) of every block pair ([n][h][w] each): dist_common.sse / dist_common.psy, vectorised over the blocks through dist_common.psy_map"""
    import dist_common as dc
    n, h, w = src.shape
    d = src.astype(np.int64) - rec.astype(np.int64)
    sse = (d * d).sum(axis=(1, 2)).astype(U64)
    sub = 8 if (w >= 8 and h >= 8) else 4
    m = dc.psy_map(src.reshape(n * h, w), rec.reshape(n * h, w), hbd, sub)
    with np.errstate(over="ignore"):
        t = m.reshape(n, h // sub, w // sub).sum(axis=(1, 2), dtype=U64)
        psy = t << U64(2) if hbd else t >> U64(1)
    for i in range(min(2, n)):
        assert int(sse[i]) == dc.sse(src[i], rec[i]) and int(psy[i]) == dc.psy(src[i], rec[i], hbd), i
    return sse, psy
