"""Buffer geometry shared by tests/test_loopfilter_geometry.py: a plane stored with a lead-in, a stride larger than its width and a tail, sentinel-filled where it is
not a picture sample (random in-range samples for inputs, so that a read with another buffer's stride changes the result), compared WHOLE with a report that says where
the first wrong sample lies; per-block tables with a sentinel tail; and the edge lists of the deblocking cases."""
import ctypes as C

import numpy as np

PIX_FILL = {1: 0xA5, 2: 0xA5A5}  # whatever is not a plane sample
I32_FILL, I8_FILL, U64_FILL = 0x5A5A5A5A, 0x5A, 0x5A5A5A5A5A5A5A5A  # tables
TAIL = 48  # samples after the last row's stride: the staging loads of both filters fetch 8 samples from a row's start even where the plane is narrower


class Plane:
    """h rows of w samples in a flat array: `lead` samples, then rows `stride` > w apart, then a tail.  dev() / ptr() place it on a back end; ptr() is the address of
    sample (0, 0), so an odd lead gives a base that is odd in samples."""

    def __init__(self, w, h, stride, lead, dtype, tail=TAIL, room=0):
        assert stride > w and lead >= 0
        self.w, self.h, self.stride, self.lead, self.dtype = w, h, stride, lead, np.dtype(dtype)
        # room = the largest stride among the buffers of the call: a kernel that walks this buffer with another one's stride stays inside the allocation, so the
        # mistake is a failed comparison and not a wild access
        self.size = lead + h * max(stride, room) + tail
        self.idx = lead + np.arange(h)[:, None] * stride + np.arange(w)[None, :]

    def guarded(self, samples=None):
        """sentinel everywhere, `samples` (h x w) in place"""
        a = np.full(self.size, PIX_FILL[self.dtype.itemsize], self.dtype)
        if samples is not None:
            a[self.idx] = samples
        return a

    def noisy(self, g, samples, bd):
        """an input: random in-range samples in the lead, the row gaps and the tail"""
        a = g.integers(0, 1 << bd, self.size).astype(self.dtype)
        a[self.idx] = samples
        return a

    def at(self, base, y=0, x=0):
        """address of sample (y, x) given the address of the flat array"""
        return base + (self.lead + y * self.stride + x) * self.dtype.itemsize

    def host_ptr(self, a, y=0, x=0):
        return C.c_void_p(self.at(a.ctypes.data, y, x))

    def samples(self, a):
        return a.reshape(-1)[self.idx]

    def check(self, got, want, tag):
        """whole-buffer comparison; on a difference say whether the first wrong sample is inside the picture (row, column), in a row gap, or before / after the plane"""
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        assert got.size == want.size == self.size, (tag, got.size, want.size, self.size)
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        e = int(bad[0])
        what = "%s: %d wrong samples (w %d, h %d, stride %d, lead %d), the first at element %d = " % (tag, bad.size, self.w, self.h, self.stride, self.lead, e)
        end = self.lead + (self.h - 1) * self.stride + self.w
        if e < self.lead:
            where = "%d samples BEFORE the plane" % (self.lead - e)
        elif e >= end:
            where = "%d samples AFTER the last picture sample" % (e - end + 1)
        else:
            r, c = divmod(e - self.lead, self.stride)
            where = ("row %d, column %d INSIDE the picture" % (r, c)) if c < self.w else ("the GAP after row %d, %d samples past its last column" % (r, c - self.w + 1))
        raise AssertionError("%s%s: got %s, want %s" % (what, where, got[e:e + 8], want[e:e + 8]))


def check_table(got, want, n, tag):
    """a per-block table of n entries followed by a sentinel tail, compared whole"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size and got.size > n, (tag, got.size, want.size, n)
    if np.array_equal(got, want):
        return
    e = int(np.flatnonzero(got != want)[0])
    where = "entry %d of %d" % (e, n) if e < n else "the sentinel tail, %d entries past the table's last one" % (e - n + 1)
    raise AssertionError("%s: first difference at %s: got %s, want %s" % (tag, where, got[e:e + 4], want[e:e + 4]))


def table(n, fill, dtype, tail=16):
    return np.full(n + tail, fill, dtype)


def dev_ptr(be, d, plane, y=0, x=0):
    """address of sample (y, x) of `plane` inside the back end's copy `d` of its flat array"""
    return plane.at(be.ptr(d), y, x)


# ---- loop restoration -----------------------------------------------------------------------------------------------------------------------------------------------
def lr_stripes(h, ss_y):
    return (h + (8 >> ss_y) + (64 >> ss_y) - 1) // (64 >> ss_y)


class LrCase:
    """One plane of loop restoration with every buffer on its own geometry: data and the two boundary-line buffers on odd strides and (the boundary buffers) odd leads,
    dst on an even stride with the lead the caller asks for (an even lead lets lr_frame_kernel store sample pairs, an odd one does not) or on an odd stride."""

    def __init__(self, g, oracle, unit_dtype, highbd, bd, ss_x, ss_y, w, h, us, dst_lead, dst_odd_stride=False):
        from test_oracle_pin_restoration import make_units, unit_grid
        dt = np.uint16 if highbd else np.uint8
        self.highbd, self.bd, self.ss_x, self.ss_y, self.w, self.h, self.us = highbd, bd, ss_x, ss_y, w, h, us
        self.nstripes = lr_stripes(h, ss_y)
        room = (w + 13) | 1
        self.pd = Plane(w, h, (w + 9) | 1, 22, dt, room=room)
        self.pa = Plane(w, 2 * self.nstripes, (w + 13) | 1, 7, dt, room=room)
        self.pb = Plane(w, 2 * self.nstripes, (w + 13) | 1, 11, dt, room=room)
        self.po = Plane(w, h, ((w + 7) | 1) if dst_odd_stride else ((w + 11) & ~1), dst_lead, dt, room=room)
        yy, xx = np.mgrid[0:h, 0:w]
        pic = np.clip(((xx * 3 + yy * 2) % (1 << bd)) // 2 + g.integers(0, 1 << (bd - 2), (h, w)), 0, (1 << bd) - 1)
        self.data = self.pd.noisy(g, pic, bd)
        self.above = self.pa.noisy(g, g.integers(0, 1 << bd, (2 * self.nstripes, w)), bd)
        self.below = self.pb.noisy(g, g.integers(0, 1 << bd, (2 * self.nstripes, w)), bd)
        self.units = make_units(g, *unit_grid(w, h, us), unit_dtype)
        self.want = self.po.guarded()
        oracle.oracle_lr_filter_frame(self.pd.host_ptr(self.data), self.pd.stride, self.pa.host_ptr(self.above), self.pb.host_ptr(self.below), self.pa.stride,
                                      self.po.host_ptr(self.want), self.po.stride, w, h, ss_y, us, C.c_void_p(self.units.ctypes.data), bd, int(highbd))

    def device(self, be):
        """upload; returns (LrParams, the device copy of the sentinel-filled dst, everything that must stay alive)"""
        d_data, d_above, d_below, d_units, d_out = be.dev(self.data), be.dev(self.above), be.dev(self.below), be.dev(self.units), be.dev(self.po.guarded())
        P = be.pkg.LrParams(dev_ptr(be, d_data, self.pd), dev_ptr(be, d_above, self.pa), dev_ptr(be, d_below, self.pb), dev_ptr(be, d_out, self.po), self.pd.stride,
                            self.pa.stride, self.po.stride, self.w, self.h, self.us, self.ss_x, self.ss_y, int(self.highbd), self.bd, be.ptr(d_units))
        return P, d_out, (d_data, d_above, d_below, d_units)


# ---- deblocking -----------------------------------------------------------------------------------------------------------------------------------------------------
def lpf_edge_lists(g, w, h, edge_dtype, limits):
    """(vertical list, horizontal list) of 4-sample segments.  The 4-sample bands along an edge direction cycle through three layouts: edges on a 16-sample grid with
    lengths 4, 6, 8, 14 in turn (14 only where 8 samples remain past the edge), on an 8-sample grid with 4, 6, 8, and on a 4-sample grid with 4 -- the densest the
    standard allows for each length, so no segment's modified samples meet another segment's taps within a pass."""
    out = []
    for vert in (1, 0):
        edges, turn = [], {16: 0, 8: 0, 4: 0}
        along_n, across_n = (h, w) if vert else (w, h)
        for a in range(0, along_n - 3, 4):
            step, lens = ((16, (14, 4, 6, 8)), (8, (8, 4, 6)), (4, (4,)))[(a // 4) % 3]
            for c in range(step, across_n - 3, step):
                ln = lens[turn[step] % len(lens)]
                turn[step] += 1
                if ln == 14 and c + 8 > across_n:
                    ln = 8
                x, y = (c, a) if vert else (a, c)
                edges.append((x, y, vert, ln) + limits(g, int(g.integers(0, 2))) + ((0, 0, 0),))
        out.append(np.array(edges, dtype=edge_dtype))
    return out


def lpf_oracle(oracle, flat, plane, edges, is16, bd):
    """the oracle, edge by edge in list order, on the flat buffer"""
    for r in edges:
        oracle.oracle_lpf(plane.host_ptr(flat, int(r["y"]), int(r["x"])), plane.stride, int(is16), int(r["vertical"]), int(r["length"]), int(r["blimit"]),
                          int(r["limit"]), int(r["thresh"]), bd)
