"""numpy restatement of the RD distortion family (csrc/dist.hip): the spatial and coefficient SSE sums and the two psy-rd energy algorithms of
psy_rd.c -- the 8-bit one (plain 2-D Hadamard) and the high-bit-depth one, which is NOT the same algorithm at another depth: the reference runs its Hadamard
stages through 32-bit temporaries, so only the pair SUMS of every packed 64-bit value survive, as wrapping uint32 values that are zero-extended again before the
final two-lane absolute value.  tests/test_dist.py::test_restatement_is_the_reference pins every function here against the reference's own.

Everything is vectorised over sub-blocks: the *_map functions take whole planes and return one value per 8x8 / 4x4 sub-block."""
import numpy as np

U32, U64, I64 = np.uint32, np.uint64, np.int64
_M64 = (1 << 64) - 1


def sse(a, b):
    """svt_spatial_full_distortion_kernel_c / svt_full_distortion_kernel16_bits_c"""
    d = a.astype(I64) - b.astype(I64)
    return int((d * d).sum())


def coeff_dist(c, r=None):
    """svt_full_distortion_kernel32_bits_c -> (residual, prediction); r is None: the cbf_zero form.  The reference squares an int64 difference and adds it to a
    uint64: exact integers reduced mod 2^64 (an int32 difference can reach 2^32)."""
    cv = [int(v) for v in np.asarray(c).reshape(-1)]
    pred = sum(v * v for v in cv) & _M64
    if r is None:
        return pred, pred
    rv = [int(v) for v in np.asarray(r).reshape(-1)]
    return sum((x - y) * (x - y) for x, y in zip(cv, rv)) & _M64, pred


def _tiles(p, n):
    """(H, W) plane -> (H/n, W/n, n, n) sub-blocks"""
    h, w = p.shape
    return p.reshape(h // n, n, w // n, n).swapaxes(1, 2)


def _had(x, axis):
    """unnormalised Hadamard transform along `axis` (length 4 or 8), exact integers; the output order is irrelevant to sum | . |"""
    x = np.moveaxis(x, axis, -1)
    s = 1
    while s < x.shape[-1]:
        y = x.reshape(x.shape[:-1] + (x.shape[-1] // (2 * s), 2, s))
        x = np.concatenate([y[..., 0, :] + y[..., 1, :], y[..., 0, :] - y[..., 1, :]], axis=-1).reshape(x.shape)
        s *= 2
    return np.moveaxis(x, -1, axis)


def _energy_lbd(t):
    """8-bit energy of sub-blocks t (..., n, n): ((sum|H X H| + 2) >> 2 for n = 8, sum|H X H| >> 1 for n = 4) - (sum X >> 2)"""
    t = t.astype(I64)
    satd = np.abs(_had(_had(t, -1), -2)).sum(axis=(-1, -2))
    term = (satd + 2) >> 2 if t.shape[-1] == 8 else satd >> 1
    return (term - (t.sum(axis=(-1, -2)) >> 2)).astype(np.int32)


def _had4_u32(s0, s1, s2, s3):
    t0, t1, t2, t3 = s0 + s1, s0 - s1, s2 + s3, s2 - s3  # uint32 arrays: wrapping
    return t0 + t2, t1 + t3, t0 - t2, t1 - t3


def _lanes_abs(v):
    """A(v) = (v + s) ^ s, s = (m << 32) - m, m = (v >> 31) & 0x1_0000_0001, in uint64"""
    m = (v >> U64(31)) & U64(0x100000001)
    s = (m << U64(32)) - m
    return (v + s) ^ s


def _fold(b):
    return (b & U64(0xffffffff)) + (b >> U64(32))


def _energy_hbd(t):
    """high-bit-depth energy of sub-blocks t (..., n, n) as svt_sa8d_8x8_hbd / svt_satd_4x4_hbd compute it against the zero block"""
    x = t.astype(U32)
    pix = x.astype(U64).sum(axis=(-1, -2))
    with np.errstate(over="ignore"):
        if t.shape[-1] == 8:
            p = x[..., 0::2] + x[..., 1::2]                                               # (..., 8 rows, 4 pair sums)
            d = np.stack(_had4_u32(p[..., 0], p[..., 1], p[..., 2], p[..., 3]), axis=-1)   # (..., 8 rows, 4)
            a = _had4_u32(d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :]) + _had4_u32(d[..., 4, :], d[..., 5, :], d[..., 6, :], d[..., 7, :])
            a = [v.astype(U64) for v in a]                                                # a0..a7, each (..., 4 columns), zero-extended
            b = np.zeros(a[0].shape, U64)
            for k in range(4):
                b = b + _lanes_abs(a[k] + a[k + 4]) + _lanes_abs(a[k] - a[k + 4])
            term = (_fold(b).sum(axis=-1, dtype=U64) + U64(2)) >> U64(2)
        else:
            l, r = x[..., 0] + x[..., 1], x[..., 2] + x[..., 3]
            lo = np.stack([l + r, l - r], axis=-1)                                        # (..., 4 rows, 2)
            a = [v.astype(U64) for v in _had4_u32(lo[..., 0, :], lo[..., 1, :], lo[..., 2, :], lo[..., 3, :])]
            b = _lanes_abs(a[0]) + _lanes_abs(a[1]) + _lanes_abs(a[2]) + _lanes_abs(a[3])
            term = _fold(b).sum(axis=-1, dtype=U64) >> U64(1)
        return (term - (pix >> U64(2))).astype(U32).view(np.int32)


def psy_map(a, b, hbd, n):
    """|e_in - e_rec| of every n x n sub-block of two planes whose sides are multiples of n, as the reference's int32 arithmetic gives it, widened to uint64"""
    f = _energy_hbd if hbd else _energy_lbd
    ea, eb = f(_tiles(a, n)), f(_tiles(b, n))
    with np.errstate(over="ignore"):
        d = (ea.view(U32) - eb.view(U32)).view(np.int32)
        m = np.where(d < 0, (U32(0) - d.view(U32)).view(np.int32), d)
    return m.astype(I64).view(U64)


def psy_scale(total, hbd):
    total = int(total) & _M64
    return (total << 2) & _M64 if hbd else total >> 1


def psy(a, b, hbd):
    """raw svt_psy_distortion (hbd false) / svt_psy_distortion_hbd (hbd true) of one block: 8x8 sub-blocks iff both sides are >= 8, else 4x4"""
    h, w = a.shape
    n = 8 if (w >= 8 and h >= 8) else 4
    with np.errstate(over="ignore"):
        return psy_scale(psy_map(a, b, hbd, n).sum(dtype=U64), hbd)


def psy_blocks(a, b, hbd, bw, bh):
    """raw psy of every bw x bh block (both >= 8) of two planes -> (H/bh, W/bw) uint64"""
    m = psy_map(a, b, hbd, 8)
    with np.errstate(over="ignore"):
        t = m.reshape(m.shape[0] // (bh // 8), bh // 8, m.shape[1] // (bw // 8), bw // 8).sum(axis=(1, 3), dtype=U64)
        return t << U64(2) if hbd else t >> U64(1)


def sse_blocks(a, b, bw, bh):
    d = a.astype(I64) - b.astype(I64)
    d = d * d
    return d.reshape(d.shape[0] // bh, bh, d.shape[1] // bw, bw).sum(axis=(1, 3)).astype(U64)


def psy_full_dist(raw, psy_rd):
    """get_svt_psy_full_dist's last line: (uint64_t)(raw * psy_rd) in IEEE double"""
    return int(float(raw) * float(psy_rd))


PSY_RD = (0.0, 0.3, 0.5, 1.0, 1.1, 2.5, 4.0, 6.0)
TX = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (4, 8), (8, 4), (8, 16), (16, 8), (16, 32), (32, 16), (32, 64), (64, 32), (4, 16), (16, 4), (8, 32), (32, 8),
      (16, 64), (64, 16)]
PSY_SIZES = TX + [(64, 56), (56, 64), (32, 24), (8, 40), (128, 128), (128, 64)]  # (width, height): what the psy functions are defined for
SSE_ONLY_SIZES = [(12, 16), (20, 16), (28, 16), (96, 128)]                         # test/SpatialFullDistortionTest.cc:89-96
CLASSES = ("random", "binary", "checker", "max", "gradient", "zero", "same")


def make_pair(g, kind, w, h, bd):
    """(input, recon) of one input class, dtype by bit depth"""
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    if kind == "random":
        a, b = g.integers(0, mx + 1, (h, w)), g.integers(0, mx + 1, (h, w))
    elif kind == "binary":
        a, b = g.integers(0, 2, (h, w)) * mx, g.integers(0, 2, (h, w)) * mx
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        a = ((yy + xx) & 1) * mx
        b = mx - a
    elif kind == "max":
        a, b = np.full((h, w), mx), g.integers(0, mx + 1, (h, w))
    elif kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.clip((xx * 3 + yy * 2) * (mx // 255) + g.integers(-4, 5, (h, w)), 0, mx)
        b = np.clip(a + g.integers(-6, 7, (h, w)) * (mx // 255), 0, mx)
    elif kind == "zero":
        a, b = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    elif kind == "same":
        a = g.integers(0, mx + 1, (h, w))
        b = a.copy()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a.astype(dt)), np.ascontiguousarray(b.astype(dt))
