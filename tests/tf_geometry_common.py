"""Picture and buffer geometry shared by tests/test_tf_geometry.py.  A picture is stored the way the encoder stores it -- a padded rectangle [-PAD, W + PAD) x
[-PAD, H + PAD) (chroma: PAD / 2) whose first sample is what the library calls buffer_y -- but inside a flat buffer with a lead that is odd in samples, a stride that
is odd and larger than W + 2 * PAD, and a tail (loopfilter_geometry_common.Plane).  Several such buffers laid end to end form the multi-reference buffers of the batch
entry points (ref_off / pred_off) and of the resident stage (ref_pitch); the leads, row gaps and tails between the rectangles are the guarded regions: random samples,
0 or the sample maximum for inputs, the sentinel for outputs."""
import numpy as np

from loopfilter_geometry_common import PIX_FILL, Plane

PAD = 80
SIZES = [(200, 136), (136, 200), (72, 40), (40, 24)]  # partial last column and row; the transpose; one whole block + an 8-wide column; smaller than one 64x64 block
SMALL = [(72, 40), (40, 24)]                          # what the emulator runs where the large sizes would be slow
SIZE_IDS = ["%dx%d" % s for s in SIZES]


def dtype_of(bd):
    return np.uint16 if bd > 8 else np.uint8


def sb_count(W, H):
    return (W + 63) // 64, (H + 63) // 64


def walk_blocks(W, H, sizes=(64, 32, 16, 8)):
    """every block of the picture's 64x64 walk, in the reference's order: (sb_x, sb_y, bsize, ix, iy); blocks of the last column / row overhang the picture or lie
    outside it altogether"""
    nsx, nsy = sb_count(W, H)
    return [(sx * 64, sy * 64, b, ix, iy) for sy in range(nsy) for sx in range(nsx) for b in sizes for iy in range(64 // b) for ix in range(64 // b)]


def fill(plane, g, samples, how, bd):
    """the flat buffer of an input plane: `samples` in place, and everything else random ("noise"), 0 ("zero") or the sample maximum ("max")"""
    if how == "noise":
        return plane.noisy(g, samples, bd)
    a = np.full(plane.size, 0 if how == "zero" else (1 << bd) - 1, plane.dtype)
    a[plane.idx] = samples
    return a


class Stack:
    """planes laid end to end in ONE flat buffer (the references of a batch call, the prediction planes of the references): offset(i) = samples from the buffer's
    first element to sample (0, 0) of plane i.  With equal planes the offsets are `pitch` apart (the resident stage's ref_pitch: larger than a plane, lead and tail
    lie between two planes)."""

    def __init__(self, planes):
        self.planes = planes
        self.starts = np.concatenate([[0], np.cumsum([q.size for q in planes])]).astype(np.int64)
        self.size = int(self.starts[-1])
        self.dtype = planes[0].dtype

    def offset(self, i):
        return int(self.starts[i]) + self.planes[i].lead

    @property
    def pitch(self):
        assert len({(q.size, q.lead) for q in self.planes}) == 1
        return self.planes[0].size

    def build(self, parts):
        return np.concatenate(parts)

    def guarded(self):
        return np.full(self.size, PIX_FILL[self.dtype.itemsize], self.dtype)

    def part(self, a, i):
        return a.reshape(-1)[int(self.starts[i]):int(self.starts[i + 1])]

    def check(self, got, want, tag):
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        assert got.size == want.size == self.size, (tag, got.size, want.size, self.size)
        for i, q in enumerate(self.planes):
            q.check(self.part(got, i), self.part(want, i), "%s, plane %d of the buffer" % (tag, i))


def luma_plane(W, H, stride_extra, lead, dtype, room_extra=40, tail=48):
    w = W + 2 * PAD
    return Plane(w, H + 2 * PAD, (w + stride_extra) | 1, lead, dtype, tail=tail, room=w + room_extra)


def chroma_plane(W, H, stride_extra, lead, dtype, odd=True, room_extra=40, tail=48):
    w = W // 2 + PAD
    st = w + stride_extra
    return Plane(w, H // 2 + PAD, (st | 1) if odd else ((st + 1) & ~1), lead, dtype, tail=tail, room=w + room_extra)


def yuv_planes(W, H, y_extra, uv_extra, leads, dtype, tail=48):
    """the three planes of one picture; the chroma stride is not derived from the luma stride"""
    return [luma_plane(W, H, y_extra, leads[0], dtype, tail=tail), chroma_plane(W, H, uv_extra, leads[1], dtype, tail=tail),
            chroma_plane(W, H, uv_extra, leads[2], dtype, tail=tail)]


def umv_clamp(mi_cols, mi_rows, pu_x, pu_y, bsize):
    """(min_col, max_col, min_row, max_row) of clamp_mv_to_umv_border_sb for the luma block, in 1/16 pel (enc_inter_prediction.c:30-50)"""
    bmi, mirow, micol = bsize >> 2, pu_y >> 2, pu_x >> 2
    to_top, to_bottom, to_left, to_right = -mirow * 32, (mi_rows - bmi - mirow) * 32, -micol * 32, (mi_cols - bmi - micol) * 32
    spel_l = (4 + bsize) << 4
    spel_r = spel_l - 16
    return to_left * 2 - spel_l, to_right * 2 + spel_r, to_top * 2 - spel_l, to_bottom * 2 + spel_r


def far_me_tables(g, tabs, W, H, every=4):
    """the second ME-table generator: a quarter of the (block, reference) entries get vectors far outside the picture -- (+-W, +-H) full pel, all four directions,
    a little jitter per block size -- and the HME centre the early-exit path starts from goes with them"""
    out = []
    for r, (best_sad, best_mv, hme_sc, hme_sad) in enumerate(tabs):
        best_mv, hme_sc = best_mv.copy(), hme_sc.copy()
        n_sb = best_mv.shape[0]
        for sb in range(n_sb):
            if (sb + r) % every:
                continue
            k = (sb // every + r) % 4
            fx, fy = (W, -W)[k & 1], (H, -H)[k >> 1]
            mvx, mvy = fx + g.integers(-2, 3, 85), fy + g.integers(-2, 3, 85)
            best_mv[sb] = ((mvy.astype(np.int16).astype(np.uint16).astype(np.uint32) << 16) | mvx.astype(np.int16).astype(np.uint16)).astype(np.uint32)
            hme_sc[sb] = (fx + 1, fy - 1)
        out.append([best_sad, np.ascontiguousarray(best_mv), np.ascontiguousarray(hme_sc), hme_sad])
    return out


class StagePictures:
    """central + n_refs reference pictures of the stage on the flat geometry: every picture shares the luma stride, the chroma stride (not derived from the luma one)
    and the padding origin, as the stage's contract says, and has leads of its own; the references lie in one Stack per plane (equal planes: a pitch), the 8-bit luma
    copies of subpel_8bit on a pitch of their own."""

    def __init__(self, g, pics, W, H, bd, sp8):
        dt = dtype_of(bd)
        n_refs = len(pics) - 1
        self.W, self.H, self.bd, self.n_refs = W, H, bd, n_refs
        self.cen = yuv_planes(W, H, 11, 6, (5, 9, 3), dt)
        self.out = yuv_planes(W, H, 11, 6, (7, 1, 11), dt)     # the host form's out-of-place output: the stage's strides, other leads
        # (the interface has one chroma pitch: U's and V's lead + tail add up to the same)
        self.refs = [Stack([luma_plane(W, H, 11, 13, dt, tail=56) for _ in range(n_refs)]), Stack([chroma_plane(W, H, 6, 7, dt, tail=58) for _ in range(n_refs)]),
                     Stack([chroma_plane(W, H, 6, 15, dt, tail=50) for _ in range(n_refs)])]
        self.y_stride, self.uv_stride = self.cen[0].stride, self.cen[1].stride
        assert self.uv_stride != self.y_stride // 2 and self.uv_stride != (self.y_stride + 1) // 2
        self.cen_flat = [fill(self.cen[pl], g, pics[0][pl], "noise", bd) for pl in range(3)]
        self.ref_flat = [self.refs[pl].build([fill(self.refs[pl].planes[r], g, pics[1 + r][pl], "noise", bd) for r in range(n_refs)]) for pl in range(3)]
        self.sp8 = sp8
        if sp8:  # the 8 MSBs of a 10-bit picture = its 8-bit luma buffer; same stride, leads and pitch of its own
            self.cen8 = luma_plane(W, H, 11, 21, np.uint8)
            self.refs8 = Stack([luma_plane(W, H, 11, 17, np.uint8, tail=64) for _ in range(n_refs)])
            self.cen8_flat = fill(self.cen8, g, pics[0][0] >> 2, "noise", 8)
            self.ref8_flat = self.refs8.build([fill(self.refs8.planes[r], g, pics[1 + r][0] >> 2, "noise", 8) for r in range(n_refs)])
            assert self.refs8.pitch != self.refs[0].pitch
        # samples a picture's descriptor declares from its first sample on: every picture's planes have room for them (Plane.size counts h * room + tail after the lead)
        self.y_samples = self.cen[0].h * self.y_stride + 16
        self.uv_samples = self.cen[1].h * self.uv_stride + 16

    def set_params(self, P):
        P.sp.ref_org_x = P.sp.ref_org_y = PAD
        P.sp.ref_stride, P.uv_stride = self.y_stride, self.uv_stride

    def rect_mask(self, plane, pl, nsx, nsy):
        """the elements of a plane's flat buffer the stage may rewrite: the 64 nsx x 64 nsy rectangle from the picture origin (chroma: half)"""
        s = 1 if pl else 0
        m = np.zeros(plane.size, bool)
        o = PAD >> s
        m[plane.idx[o:o + ((64 * nsy) >> s), o:o + ((64 * nsx) >> s)]] = True
        return m

