"""AV1 masked prediction (csrc/maskpred.hip): svt_hip_blend_batch, svt_hip_inter_pred_masked_batch (csrc/interpred.hip), svt_hip_wedge_search_batch and the fifteen single-call forms, every output sample against
tests/maskpred_common.py (numpy; pinned on the reference's C by tests/test_maskpred_ref.py) and against tests/golden/maskpred.npz (what the reference's C computed).
Every batched blend runs on planes with odd strides (531 / 601 samples, destination 547, masks at odd strides and offsets), blocks at every byte alignment, the
destination filled with 0xA5 beforehand: the WHOLE destination plane is compared, so a sample written outside a block's w x h fails like a wrong sample inside it."""
import ctypes as C
import mmap

import numpy as np
import pytest

import dist_common as dc
import maskpred_common as mc
from conftest import EmuBackend, _backends, p, rng

SA, SB, SD = 531, 601, 547
PLANE_A, PLANE_B = 5, 30
BIT_DEPTHS = (8, 10, 12)
SIZES = [(1, 1), (2, 2), (4, 4), (2, 16), (16, 2), (8, 8), (8, 32), (32, 8), (32, 32), (64, 64), (128, 128), (128, 4)]
SUBS = ((0, 0), (1, 1), (1, 0), (0, 1))


def spec(w, h, kind=mc.KIND_A64, msrc=mc.SRC_EXPLICIT, subw=0, subh=0, bsize=0, idx=0, sign=0, mode=0, mask="random", cls="random"):
    return dict(w=w, h=h, kind=kind, msrc=msrc, subw=subw, subh=subh, bsize=bsize, idx=idx, sign=sign, mode=mode, mask=mask, cls=cls)


def mask_of(s, g):
    """the mask a descriptor stands for, in the shape the matching C function reads it"""
    w, h = s["w"], s["h"]
    if s["msrc"] == mc.SRC_WEDGE:
        return mc.wedge_masks()[(s["bsize"], s["idx"], s["sign"])]
    if s["msrc"] == mc.SRC_SMOOTH:
        return mc.smooth_interintra_mask(s["bsize"], s["mode"])
    if s["msrc"] == mc.SRC_OBMC:
        return mc.OBMC_MASKS[w if s["kind"] == mc.KIND_H else h]
    shape = (h << s["subh"], w << s["subw"]) if s["kind"] == mc.KIND_A64 else ((w,) if s["kind"] == mc.KIND_H else (h,))
    return g.integers(0, 65, shape).astype(np.uint8) if s["mask"] == "random" else np.full(shape, s["mask"], np.uint8)


def expect(s, s0, s1, mask):
    if s["kind"] == mc.KIND_A64:
        return mc.blend_a64_mask(s0, s1, mask, s["subw"], s["subh"])
    return mc.blend_a64_hmask(s0, s1, mask) if s["kind"] == mc.KIND_H else mc.blend_a64_vmask(s0, s1, mask)


def _place(specs, g):
    x = y = shelf = 0
    pos = []
    for s in specs:
        gap = 1 + int(g.integers(0, 7))
        if x + gap + s["w"] > SA - 8:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + s["w"], max(shelf, s["h"])
    return pos, y + shelf + 1


def build(be, specs, bd, g, in_place=None):
    """planes, mask bytes, descriptors and the expected destination plane of one launch; in_place 0 / 1: the destination is source plane 0 / 1 itself"""
    dt = np.uint16 if bd > 8 else np.uint8
    pos, rows = _place(specs, g)
    fill = 0xA5A5 if bd > 8 else 0xA5
    A = g.integers(0, 1 << bd, (rows + 2, SA)).astype(dt)
    B = g.integers(0, 1 << bd, (rows + 5, SB)).astype(dt)
    want = np.full((rows + 2, SD), fill, dt)
    d = np.zeros(len(specs), be.pkg.BlendDesc)
    masks, mo = [np.full(3, 0xEE, np.uint8)], 3
    for i, (s, (x, y)) in enumerate(zip(specs, pos)):
        w, h = s["w"], s["h"]
        s0, s1 = mc.make_pair(g, s["cls"], w, h, bd)
        A[y:y + h, x:x + w], B[y + 2:y + 2 + h, x + 5:x + 5 + w] = s0, s1
        mask = mask_of(s, g)
        if s["msrc"] == mc.SRC_EXPLICIT:
            m2 = np.atleast_2d(mask)
            pad = np.full((m2.shape[0], m2.shape[1] + 3), 0xEE, np.uint8)  # (rows at an odd stride; 0xEE = 238 would show in any blend that read it)
            pad[:, :m2.shape[1]] = m2
            d[i]["mask_off"], d[i]["mask_stride"] = mo, pad.shape[1]
            masks.append(pad.reshape(-1)[:pad.size - 3])  # the last row ends with its last mask byte
            mo += pad.size - 3
        d[i]["src_off"], d[i]["src_stride"], d[i]["plane"] = (y * SA + x, (y + 2) * SB + x + 5), (SA, SB), (PLANE_A, PLANE_B)
        d[i]["dst_off"], d[i]["dst_stride"] = y * SD + x, SD
        d[i]["w"], d[i]["h"], d[i]["kind"], d[i]["mask_src"], d[i]["subw"], d[i]["subh"] = w, h, s["kind"], s["msrc"], s["subw"], s["subh"]
        d[i]["bsize"], d[i]["wedge_index"], d[i]["wedge_sign"], d[i]["ii_mode"] = s["bsize"], s["idx"], s["sign"], s["mode"]
        want[y:y + h, x:x + w] = expect(s, s0, s1, mask)
    if in_place is not None:
        src = (A, B)[in_place]
        full = src.copy()
        for i, s in enumerate(specs):
            yd, xd = divmod(int(d[i]["dst_off"]), SD)
            ys, xs = divmod(int(d[i]["src_off"][in_place]), src.shape[1])
            full[ys:ys + s["h"], xs:xs + s["w"]] = want[yd:yd + s["h"], xd:xd + s["w"]]
        d["dst_off"], d["dst_stride"] = d["src_off"][:, in_place], src.shape[1]
        want = full
    return A, B, np.concatenate(masks), d, want, fill


def launch(be, A, B, M, d, dst, bd, status=None, keep=None, in_place=None):
    planes = be.pkg.BlendPlanes()
    dA, dB, dM, dd = be.dev(A), be.dev(B), be.dev(M), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    if in_place is not None:
        dst = (dA, dB)[in_place]
    if keep is not None:
        keep.extend([dA, dB, dM, dd])
    r = be.lib.svt_hip_blend_batch(planes, be.ptr(dst), be.ptr(dM), be.ptr(dd), len(d), bd, None if status is None else be.ptr(status), be.stream)
    return r, dst


def run(be, specs, bd, seed, with_status=False, in_place=None):
    g = rng(seed)
    A, B, M, d, want, fill = build(be, specs, bd, g, in_place)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    status = be.dev(np.full(len(specs), 7, np.uint8)) if with_status else None
    r, dst = launch(be, A, B, M, d, dst, bd, status, in_place=in_place)
    assert r == 0
    got = be.host(dst).reshape(want.shape)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        stride = want.shape[1]
        for i, s in enumerate(specs):
            y, x = divmod(int(d[i]["dst_off"]), stride)
            a, b = got[y:y + s["h"], x:x + s["w"]], want[y:y + s["h"], x:x + s["w"]]
            assert np.array_equal(a, b), (bd, i, s, np.argwhere(a != b)[:4], a[:2, :8], b[:2, :8])
        raise AssertionError("samples outside every block's w x h were written: %s" % (np.argwhere(got != want)[:8],))


def every_kind_specs():
    """the twelve sizes x (A64_MASK with the four sub-samplings, HMASK, VMASK) with explicit masks: random, all 0, all 64; input classes cycle"""
    specs, k = [], 0
    for (w, h) in SIZES:
        for (subw, subh) in SUBS:
            specs.append(spec(w, h, subw=subw, subh=subh, mask=("random", 0, 64)[k % 3] if k % 4 else "random", cls=mc.CLASSES[k % 4]))
            k += 1
        for kind in (mc.KIND_H, mc.KIND_V):
            specs.append(spec(w, h, kind, mask=("random", 64, 0)[k % 3], cls=mc.CLASSES[k % 4]))
            k += 1
    return specs


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_every_size_kind_and_subsampling(be, bd):
    run(be, every_kind_specs(), bd, 100 + bd, with_status=bd == 10)


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("in_place", (0, 1))
def test_in_place(be, bd, in_place):
    """dst == src0 and dst == src1 at the same position and stride: the whole source plane afterwards == the plane with the blends in it"""
    run(be, every_kind_specs(), bd, 150 + bd + in_place, in_place=in_place)


@pytest.mark.parametrize("bd", (8, 12))
def test_every_wedge_mask(be, bd):
    """all nine wedge sizes x 16 indices x 2 signs at full size, and each through the three sub-samplings (the 4:2:0 chroma block under its luma mask, e.g. 4x4 under
    the 8x8 wedge; 4:2:2 and its transpose)"""
    specs = []
    for b in mc.WEDGE_BSIZES:
        for idx in range(16):
            for sign in (0, 1):
                specs.append(spec(mc.BW[b], mc.BH[b], msrc=mc.SRC_WEDGE, bsize=b, idx=idx, sign=sign))
                subw, subh = SUBS[1 + (idx + sign) % 3]
                specs.append(spec(mc.BW[b] >> subw, mc.BH[b] >> subh, msrc=mc.SRC_WEDGE, subw=subw, subh=subh, bsize=b, idx=idx, sign=sign))
    assert any(s["w"] == 4 and s["h"] == 4 and s["bsize"] == 3 for s in specs)
    run(be, specs, bd, 200 + bd)


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_smooth_interintra_and_obmc(be, bd):
    """the four inter-intra modes at every BlockSize (the seven sizes 8x8 .. 32x32 of svt_aom_is_interintra_allowed_bsize, their 4:2:0 chroma sizes 4x4 .. 16x16 and
    the rest); the OBMC masks of length 1 .. 32 both ways, at the shapes av1_build_obmc_inter_prediction blends (overlap x width, height x overlap)"""
    specs = [spec(mc.BW[b], mc.BH[b], msrc=mc.SRC_SMOOTH, bsize=b, mode=m, cls=mc.CLASSES[(b + m) % 4]) for b in range(22) for m in range(4)]
    for n in (1, 2, 4, 8, 16, 32):
        for other in (1, 8, 64, 128):
            specs.append(spec(n, other, mc.KIND_H, mc.SRC_OBMC))
            specs.append(spec(other, n, mc.KIND_V, mc.SRC_OBMC))
    run(be, specs, bd, 300 + bd)
    if bd == 8:
        run(be, [s for s in specs if s["msrc"] == mc.SRC_OBMC], bd, 310, in_place=0)  # OBMC blends in place


@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_launch_sizes_around_a_workgroup(be, n):
    """1, B - 1, B, B + 1 and 2 B + 1 descriptors of mixed sizes for the B = 16 descriptors one workgroup flattens"""
    assert be.pkg.BLEND_DESCS_PER_WORKGROUP == 16
    g = rng(n)
    pool = every_kind_specs()
    run(be, [pool[int(g.integers(len(pool)))] for _ in range(n)], 8, 400 + n, with_status=n == 17)


def test_golden_cases(be):
    """the blend cases of tests/golden/maskpred.npz: the kernel == what the reference's C computed; and the device's wedge table == the reference's, byte for byte,
    read back through full-size blends of 64 over 0 (the blend of mask m is m itself)"""
    gold = mc.load_golden()
    assert int(gold["seed"][0]) == mc.GOLDEN_SEED
    cases = mc.golden_blend_cases()
    for bd in BIT_DEPTHS:
        idx = [i for i, c in enumerate(cases) if c[3] == bd]
        dt = np.uint16 if bd > 8 else np.uint8
        d = np.zeros(len(idx), be.pkg.BlendDesc)
        s0s, s1s, ms, so, mo, do = [], [], [], 0, 0, 0
        for j, i in enumerate(idx):
            fn, w, h, _, subw, subh, _ = cases[i]
            s0, s1, mask = mc.golden_blend_inputs(i, cases[i])
            assert int(s0.astype(np.int64).sum()) + int(s1.astype(np.int64).sum()) + int(mask.astype(np.int64).sum()) == int(gold["blend_insum_%d" % i][0])
            d[j]["src_off"], d[j]["src_stride"], d[j]["plane"], d[j]["dst_off"], d[j]["dst_stride"] = (so, so), (w, w), (0, 1), do, w
            d[j]["mask_off"], d[j]["mask_stride"] = mo, mask.shape[-1]
            d[j]["w"], d[j]["h"], d[j]["kind"], d[j]["subw"], d[j]["subh"] = w, h, {"mask": 0, "hmask": 1, "vmask": 2}[fn], subw, subh
            s0s.append(s0.reshape(-1)), s1s.append(s1.reshape(-1)), ms.append(mask.reshape(-1))
            so, mo, do = so + w * h, mo + mask.size, do + w * h
        planes = be.pkg.BlendPlanes()
        d0, d1, dm, dd, dst = be.dev(np.concatenate(s0s).astype(dt)), be.dev(np.concatenate(s1s).astype(dt)), be.dev(np.concatenate(ms)), be.dev(d), be.dev(np.zeros(do, dt))
        planes.base[0], planes.base[1] = be.ptr(d0), be.ptr(d1)
        assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), be.ptr(dm), be.ptr(dd), len(idx), bd, None, be.stream) == 0
        got = be.host(dst)
        for j, i in enumerate(idx):
            fn, w, h = cases[i][:3]
            out = got[int(d[j]["dst_off"]):int(d[j]["dst_off"]) + w * h].reshape(h, w)
            assert np.array_equal(out, gold["blend_%d" % i]), (i, cases[i])
            assert np.array_equal(out, mc.blend_case(cases[i], *mc.golden_blend_inputs(i, cases[i]))), (i, cases[i])
    # the table: 288 descriptors, src0 = 64 everywhere, src1 = 0 everywhere
    keys = [(b, i, s) for b in mc.WEDGE_BSIZES for i in range(16) for s in (0, 1)]
    d = np.zeros(len(keys), be.pkg.BlendDesc)
    off = 0
    for j, (b, i, s) in enumerate(keys):
        d[j]["src_stride"], d[j]["plane"], d[j]["dst_off"], d[j]["dst_stride"] = (32, 32), (0, 1), off, mc.BW[b]
        d[j]["w"], d[j]["h"], d[j]["mask_src"], d[j]["bsize"], d[j]["wedge_index"], d[j]["wedge_sign"] = mc.BW[b], mc.BH[b], mc.SRC_WEDGE, b, i, s
        off += mc.BW[b] * mc.BH[b]
    planes = be.pkg.BlendPlanes()
    d0, d1, dd, dst = be.dev(np.full(1024, 64, np.uint8)), be.dev(np.zeros(1024, np.uint8)), be.dev(d), be.dev(np.full(off, 0xA5, np.uint8))
    planes.base[0], planes.base[1] = be.ptr(d0), be.ptr(d1)
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), None, be.ptr(dd), len(keys), 8, None, be.stream) == 0
    assert np.array_equal(be.host(dst), gold["wedge_table"])
    assert np.array_equal(gold["wedge_table"], mc.wedge_table_bytes())
    # the kernel-side OBMC and inter-intra constants against the reference's recorded bytes, read back the same way: HMASK blends of one row per OBMC length, and
    # the four smooth modes at the ten sizes the file records
    items = [(n, 1, mc.KIND_H, mc.SRC_OBMC, 0, 0) for n in (1, 2, 4, 8, 16, 32)] + [(mc.BW[b], mc.BH[b], mc.KIND_A64, mc.SRC_SMOOTH, b, m) for b in range(10) for m in range(4)]
    d = np.zeros(len(items), be.pkg.BlendDesc)
    off = 0
    for j, (w, h, kind, msrc, b, m) in enumerate(items):
        d[j]["src_stride"], d[j]["plane"], d[j]["dst_off"], d[j]["dst_stride"] = (32, 32), (0, 1), off, w
        d[j]["w"], d[j]["h"], d[j]["kind"], d[j]["mask_src"], d[j]["bsize"], d[j]["ii_mode"] = w, h, kind, msrc, b, m
        off += w * h
    dd, dst = be.dev(d), be.dev(np.full(off, 0xA5, np.uint8))
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), None, be.ptr(dd), len(items), 8, None, be.stream) == 0
    got = be.host(dst)
    assert np.array_equal(got[:63], gold["obmc"]) and np.array_equal(got[63:], gold["smooth"])


INVALID = ["width 3", "height 0", "width 24", "subw 2", "subh 2", "kind 3", "mask source 4", "wedge bsize 4x4", "wedge bsize 64x64", "wedge index 16", "wedge sign 2",
           "wedge block larger than mask", "wedge with HMASK", "mode 4", "smooth bsize mismatch", "smooth with subw", "OBMC length 64", "OBMC with A64_MASK", "NULL plane",
           "second NULL plane", "plane 32", "explicit without mask_base"]


@pytest.mark.parametrize("what", INVALID)
def test_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones: with status == NULL the call returns -1 and not one destination byte changes; with a status array it returns 0,
    flags that descriptor alone, leaves its block untouched and blends the other two"""
    g = rng(9)
    mid = spec(16, 16)
    if what.startswith("wedge"):
        mid = spec(16, 16, msrc=mc.SRC_WEDGE, bsize=6, idx=3, sign=1)
    elif what.startswith("mode") or what.startswith("smooth"):
        mid = spec(16, 16, msrc=mc.SRC_SMOOTH, bsize=6, mode=3)
    elif what.startswith("OBMC"):
        mid = spec(16, 16, mc.KIND_V, mc.SRC_OBMC)
    specs = [spec(8, 8, subw=1), mid, spec(4, 4, mc.KIND_H, mc.SRC_OBMC)]
    A, B, M, d, want, fill = build(be, specs, 8, g)
    y, x = divmod(int(d[1]["dst_off"]), SD)
    want[y:y + 16, x:x + 16] = fill
    edits = {"width 3": ("w", 3), "height 0": ("h", 0), "width 24": ("w", 24), "subw 2": ("subw", 2), "subh 2": ("subh", 2), "kind 3": ("kind", 3),
             "mask source 4": ("mask_src", 4), "wedge bsize 4x4": ("bsize", 0), "wedge bsize 64x64": ("bsize", 12), "wedge index 16": ("wedge_index", 16),
             "wedge sign 2": ("wedge_sign", 2), "wedge block larger than mask": ("bsize", 3), "wedge with HMASK": ("kind", 1), "mode 4": ("ii_mode", 4),
             "smooth bsize mismatch": ("bsize", 7), "smooth with subw": ("subw", 1), "OBMC length 64": ("h", 64), "OBMC with A64_MASK": ("kind", 0)}
    if what in edits:
        d[edits[what][0]][1] = edits[what][1]
    elif what == "NULL plane":
        d["plane"][1, 0] = 6
    elif what == "second NULL plane":
        d["plane"][1, 1] = 31
    elif what == "plane 32":
        d["plane"][1, 0] = 32
    no_mask = what == "explicit without mask_base"
    if no_mask:  # every EXPLICIT descriptor of the launch is invalid then: the OBMC one alone is blended
        want[:] = fill
        yy, xx = divmod(int(d[2]["dst_off"]), SD)
        want[yy:yy + 4, xx:xx + 4] = mc.blend_a64_hmask(A[yy:yy + 4, xx:xx + 4], B[yy + 2:yy + 6, xx + 5:xx + 9], mc.OBMC_MASKS[4])
    planes = be.pkg.BlendPlanes()
    dA, dB, dM, dd = be.dev(A), be.dev(B), be.dev(M), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    mptr = None if no_mask else be.ptr(dM)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), mptr, be.ptr(dd), 3, 8, None, be.stream) == -1
    assert np.all(be.host(dst) == fill)
    status = be.dev(np.full(3, 7, np.uint8))
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), mptr, be.ptr(dd), 3, 8, be.ptr(status), be.stream) == 0
    assert np.array_equal(be.host(dst), want)
    assert be.host(status).tolist() == ([1, 1, 0] if no_mask else [0, 1, 0])
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), mptr, be.ptr(dd), 1, 9, None, be.stream) == -1  # not a bit depth


def _guarded(n_bytes):
    """a mapping whose neighbouring pages are inaccessible: (mmap, page size, readable length)"""
    page = mmap.PAGESIZE
    body = (n_bytes + page - 1) // page * page
    m = mmap.mmap(-1, body + 2 * page)
    base = C.addressof(C.c_char.from_buffer(m))
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes, libc.mprotect.restype = [C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + page + body, page, 0) == 0
    return m, page, body


def _flush(n_items, dt, at_end):
    """n_items of dtype dt flush against the inaccessible page after (at_end) or before them: (mapping, array, address)"""
    dt = np.dtype(dt)
    m, page, body = _guarded(n_items * dt.itemsize)
    start = page + (body - n_items * dt.itemsize if at_end else 0)
    return m, np.frombuffer(m, dt, n_items, start), C.addressof(C.c_char.from_buffer(m)) + start


def test_read_guard_on_the_emulator():
    """CPU only.  Sources, explicit masks and search inputs lie flush against inaccessible pages on either end: the kernels read w x h of each source, (w << subw) x
    (h << subh) of a 2-D mask, w or h bytes of a 1-D mask, bw x bh of each search plane -- one sample more leaves the mapping."""
    be = _backends.setdefault("emu", EmuBackend())
    g = rng(77)
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        for (w, h) in ((1, 1), (4, 4), (2, 16), (32, 8), (64, 64), (128, 4)):
            for kind, subw, subh in [(mc.KIND_A64,) + sb for sb in SUBS] + [(mc.KIND_H, 0, 0), (mc.KIND_V, 0, 0)]:
                for at_end in (True, False):
                    s = spec(w, h, kind, subw=subw, subh=subh)
                    mask = mask_of(s, g)
                    m0, a0, p0 = _flush(w * h, dt, at_end)
                    m1, a1, p1 = _flush(w * h, dt, at_end)
                    mm, am, pm = _flush(mask.size, np.uint8, at_end)
                    a0[:], a1[:], am[:] = g.integers(0, 1 << bd, w * h), g.integers(0, 1 << bd, w * h), mask.reshape(-1)
                    planes = be.pkg.BlendPlanes()
                    planes.base[0], planes.base[1] = p0, p1
                    d = np.zeros(1, be.pkg.BlendDesc)
                    d["src_stride"], d["plane"], d["dst_stride"], d["mask_stride"] = (w, w), (0, 1), w, mask.shape[-1]
                    d["w"], d["h"], d["kind"], d["subw"], d["subh"] = w, h, kind, subw, subh
                    dst = np.zeros(w * h, dt)
                    assert be.lib.svt_hip_blend_batch(planes, p(dst), pm, p(d), 1, bd, None, None) == 0
                    assert np.array_equal(dst.reshape(h, w), expect(s, a0.reshape(h, w), a1.reshape(h, w), mask)), (bd, w, h, kind, subw, subh, at_end)
                    del a0, a1, am, m0, m1, mm
        for b in (3, 7, 9, 19):
            for at_end in (True, False):
                n = mc.BW[b] * mc.BH[b]
                maps = [_flush(n, dt, at_end) for _ in range(3)]
                src, q0, q1 = mc.make_search_inputs(g, "random", b, bd)
                for (_, a, _), v in zip(maps, (src, q0, q1)):
                    a[:] = v.reshape(-1)
                planes = be.pkg.BlendPlanes()
                for k in range(3):
                    planes.base[k] = maps[k][2]
                d = np.zeros(1, be.pkg.WedgeSearchDesc)
                d["src_stride"], d["p0_stride"], d["p1_stride"], d["p0_plane"], d["p1_plane"], d["bsize"] = mc.BW[b], mc.BW[b], mc.BW[b], 1, 2, b
                out = np.zeros(1, be.pkg.WedgeSearchResult)
                assert be.lib.svt_hip_wedge_search_batch(planes, p(d), 1, bd, p(out), None, None) == 0
                check_search(out[0], mc.wedge_search(src, q0, q1, b, bd), (bd, b, at_end))
                del maps, a


def test_per_call_forms(be):
    """the six blend forms at four sizes each: blocks inside larger planes with their own strides, nothing outside w x h written, in place on src0 and on src1;
    a size that is no power of two and a sub-sampling of 2 write nothing"""
    L = be.lib
    g = rng(16)
    k = 0
    for fn in ("mask", "hmask", "vmask"):
        for hbd in (False, True):
            for (w, h) in ((1, 2), (8, 8), (32, 16), (128, 4)):
                for (subw, subh) in (SUBS if fn == "mask" else SUBS[:1]):
                    bd = (10, 12)[k % 2] if hbd else 8
                    k += 1
                    dt, fill = (np.uint16, 0xA5A5) if hbd else (np.uint8, 0xA5)
                    s0, s1 = mc.make_pair(g, mc.CLASSES[k % 4], w, h, bd)
                    s = spec(w, h, {"mask": 0, "hmask": 1, "vmask": 2}[fn], subw=subw, subh=subh)
                    mask = mask_of(s, g)
                    want_blk = expect(s, s0, s1, mask)
                    mpl = np.full((np.atleast_2d(mask).shape[0], mask.shape[-1] + 5), 0xEE, np.uint8)
                    mpl[:, :mask.shape[-1]] = np.atleast_2d(mask)
                    name = "svt_aom_%sblend_a64_%s%s_hip" % ("highbd_" if hbd else "", fn, "_16bit" if hbd and fn != "mask" else "")
                    f = getattr(L, name)
                    for ip in (None, 0, 1):
                        a, b = np.full((h + 1, w + 3), 1, dt), np.full((h + 2, w + 5), 2, dt)
                        a[:h, :w], b[:h, :w] = s0, s1
                        dst = a if ip == 0 else (b if ip == 1 else np.full((h + 2, w + 1), fill, dt))
                        want = dst.copy()
                        want[:h, :w] = want_blk
                        args = [p(dst), dst.shape[1], p(a), a.shape[1], p(b), b.shape[1], p(mpl)]
                        args += [mpl.shape[1], w, h, subw, subh] if fn == "mask" else [w, h]
                        f(*args, *([bd] if hbd else []))
                        assert np.array_equal(dst, want), (name, w, h, subw, subh, bd, ip)
    dst, a, m = np.full((8, 8), 0xA5, np.uint8), np.zeros((8, 8), np.uint8), np.zeros((16, 16), np.uint8)
    L.svt_aom_blend_a64_mask_hip(p(dst), 8, p(a), 8, p(a), 8, p(m), 16, 6, 8, 0, 0)
    L.svt_aom_blend_a64_mask_hip(p(dst), 8, p(a), 8, p(a), 8, p(m), 16, 8, 8, 2, 0)
    L.svt_aom_blend_a64_vmask_hip(p(dst), 8, p(a), 8, p(a), 8, p(m), 8, 0)
    assert np.all(dst == 0xA5)
    assert L.svt_hip_debug_commit_violations() == 0


@pytest.mark.parametrize("with_status", (True, False))
@pytest.mark.parametrize("bd", (8, 10))
def test_intra_and_inter_predictions_feed_the_blend_and_the_distortion(be, bd, with_status):
    """svt_hip_intra_pred_batch + svt_hip_inter_pred_batch -> svt_hip_blend_batch (inter-intra: intra is src0, smooth masks and wedges) -> svt_hip_pixel_dist_batch
    on one stream, nothing read back in between; with status arrays no call synchronises (the asynchronous forms), without them each prediction call checks its
    descriptors first.  The SSE of every combined prediction against a source plane == the SSE of svt_aom_combine_interintra's result on the restatements' predictions"""
    import interpred_common as ipc
    import intrapred_common as iac
    import test_interpred as tep
    import test_intrapred as tip
    g = rng(700 + bd)
    bsizes = [b for b in mc.II_BSIZES for _ in range(3)]
    n = len(bsizes)
    intra_cases = [iac.case(mc.BW[b], mc.BH[b], (iac.DC, iac.V, iac.H, iac.SMOOTH)[i % 4]) for i, b in enumerate(bsizes)]
    inter_specs = [tep.spec(mc.BW[b], mc.BH[b], i % 3, (i + 1) % 3, i % 3 if i % 2 else 0, tep.PHASES[i % 8], tep.PHASES[(i + 3) % 8], ipc.DIST_WEIGHTS[i % 8])
                   for i, b in enumerate(bsizes)]
    T, Lf, di, want_i, fill = tip.build(be, intra_cases, bd, g)
    A, B, de, want_e, _ = tep.build(be, inter_specs, bd, g)
    d = np.zeros(n, be.pkg.BlendDesc)
    want = np.full((want_e.shape[0], SD), fill, want_e.dtype)
    for i, b in enumerate(bsizes):
        w, h = mc.BW[b], mc.BH[b]
        yi, xi = divmod(int(di[i]["dst_off"]), tip.SD)
        ye, xe = divmod(int(de[i]["dst_off"]), tep.SD)
        use_wedge = i % 3 == 2
        d[i]["src_off"], d[i]["src_stride"], d[i]["plane"] = (di[i]["dst_off"], de[i]["dst_off"]), (tip.SD, tep.SD), (0, 1)
        d[i]["dst_off"], d[i]["dst_stride"], d[i]["w"], d[i]["h"], d[i]["bsize"] = ye * SD + xe, SD, w, h, b
        d[i]["mask_src"], d[i]["ii_mode"], d[i]["wedge_index"], d[i]["wedge_sign"] = (mc.SRC_WEDGE if use_wedge else mc.SRC_SMOOTH), i % 4, i % 16, i % 2
        want[ye:ye + h, xe:xe + w] = mc.combine_interintra(i % 4, use_wedge, i % 16, i % 2, b, b, want_e[ye:ye + h, xe:xe + w], want_i[yi:yi + h, xi:xi + w])
    src = g.integers(0, 1 << bd, want.shape).astype(want.dtype)
    assert be.lib.svt_hip_maskpred_prepare(be.stream) == 0  # the wedge table exists from here on: no call below synchronises for it
    keep, st = [], [be.dev(np.full(n, 7, np.uint8)) if with_status else None for _ in range(3)]
    pi, pe, dst = be.dev(np.full(want_i.shape, fill, want_i.dtype)), be.dev(np.full(want_e.shape, fill, want_e.dtype)), be.dev(np.full(want.shape, fill, want.dtype))
    dsrc, sse, dbl = be.dev(src), be.dev(np.full(n, 0xDEADBEEF, np.uint64)), be.dev(d)
    dd = np.zeros(n, be.pkg.DistDesc)
    dd["in_off"], dd["rec_off"], dd["in_stride"], dd["rec_stride"], dd["width"], dd["height"] = d["dst_off"], d["dst_off"], SD, SD, d["w"], d["h"]
    ddd = be.dev(dd)
    planes = be.pkg.BlendPlanes()
    planes.base[0], planes.base[1] = be.ptr(pi), be.ptr(pe)
    assert tip.launch(be, T, Lf, di, pi, bd, st[0], keep) == 0
    assert tep.launch(be, A, B, de, pe, bd, st[1], keep) == 0
    assert be.lib.svt_hip_blend_batch(planes, be.ptr(dst), None, be.ptr(dbl), n, bd, be.ptr(st[2]) if with_status else None, be.stream) == 0
    be.lib.svt_hip_pixel_dist_batch(be.ptr(dsrc), be.ptr(dst), be.ptr(ddd), n, int(bd > 8), 1, be.ptr(sse), None, be.stream)
    got = be.host(sse)
    assert np.array_equal(be.host(dst), want)
    for i, b in enumerate(bsizes):
        y, x = divmod(int(d[i]["dst_off"]), SD)
        assert int(got[i]) == dc.sse(src[y:y + mc.BH[b], x:x + mc.BW[b]], want[y:y + mc.BH[b], x:x + mc.BW[b]]), (bd, i, b)
    assert not any(be.host(s).any() for s in st if s is not None)


# ---- the wedge / diff-weighted search ----------------------------------------------------------------------------------------------------------------------
def check_search(got, want, tag):
    assert np.array_equal(got["sse"], want["sse"]), tag + (got["sse"], want["sse"])
    assert np.array_equal(got["sign"], want["sign"]), tag
    assert np.array_equal(got["sse_diffwtd"], want["sse_diffwtd"]), tag
    assert (int(got["best_wedge_index"]), int(got["best_wedge_sign"]), int(got["best_mask_type"])) == (want["best_wedge_index"], want["best_wedge_sign"],
                                                                                                       want["best_mask_type"]), tag


def run_search(be, items, bd, with_status=False):
    """items: (bsize, fixed_sign, src, p0, p1); the three planes hold the blocks back to back at odd strides and offsets"""
    dt = np.uint16 if bd > 8 else np.uint8
    n = len(items)
    d = np.zeros(n, be.pkg.WedgeSearchDesc)
    bufs, offs = [[np.full(1 + k, 3, dt)] for k in range(3)], [1, 2, 3]
    for i, (b, fs, src, q0, q1) in enumerate(items):
        bw, bh = mc.BW[b], mc.BH[b]
        for k, (v, name) in enumerate(((src, "src"), (q0, "p0"), (q1, "p1"))):
            stride = bw + 1 + 2 * k
            pl = np.full((bh, stride), 5, dt)
            pl[:, :bw] = v
            d[i][name + "_off"], d[i][name + "_stride"], d[i][name + "_plane"] = offs[k], stride, 7 + k
            bufs[k].append(pl.reshape(-1))
            offs[k] += pl.size
        d[i]["bsize"], d[i]["fixed_sign"] = b, fs
    planes = be.pkg.BlendPlanes()
    keep = [be.dev(np.concatenate(v)) for v in bufs]
    for k in range(3):
        planes.base[7 + k] = be.ptr(keep[k])
    dd, out = be.dev(d), be.dev(np.zeros(n, be.pkg.WedgeSearchResult))
    status = be.dev(np.full(n, 7, np.uint8)) if with_status else None
    assert be.lib.svt_hip_wedge_search_batch(planes, be.ptr(dd), n, bd, be.ptr(out), None if status is None else be.ptr(status), be.stream) == 0
    got = be.host(out)
    if with_status:
        assert not be.host(status).any()
    return got


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_search_every_size_and_class(be, bd):
    """all nine sizes: predictions near the source; unrelated blocks, where at 10 and 12 bit the int16_t clamp of the SSE term binds (asserted on the restatement's
    intermediates: at least one clamped term per such case, none at 8 bit) and the delta of squares saturates (asserted, every depth); p0 == p1, where every SSE is
    equal and index 0 / sign 0 must come out; one differing sample, where several indices tie at the minimum (asserted at every depth) and the first must win; both fixed
    signs"""
    g = rng(800 + bd)
    items, wants = [], []
    for b in mc.WEDGE_BSIZES:
        for kind, fs in (("near", 0), ("random", 0), ("equal", 0), ("tie", 0), ("near", 1), ("random", 2)):
            src, q0, q1 = mc.make_search_inputs(g, kind, b, bd)
            r = mc.wedge_search(src, q0, q1, b, bd, fs)
            if kind == "random":
                assert (r["clamped_terms"] > 0) == (bd > 8) and r["saturated_ds"] > 0, (b, bd, r["clamped_terms"], r["saturated_ds"])
            if kind == "equal":
                assert len(set(r["sse"].tolist())) == 1 and (r["best_wedge_index"], r["best_wedge_sign"]) == (0, 0)
                assert r["sse_diffwtd"][0] == r["sse_diffwtd"][1] and r["best_mask_type"] == 0
            if kind == "tie":
                assert int((r["sse"] == r["sse"].min()).sum()) >= 2 and r["sse"].max() > r["sse"].min() and r["best_wedge_index"] == int(np.argmin(r["sse"]))
            if fs:
                assert np.all(r["sign"] == fs - 1)
            items.append((b, fs, src, q0, q1))
            wants.append(r)
    got = run_search(be, items, bd, with_status=bd == 10)
    for i, r in enumerate(wants):
        check_search(got[i], r, (bd, i, items[i][0], items[i][1]))


@pytest.mark.parametrize("n", (1, 3, 4, 5, 63, 64, 65))
def test_search_launch_sizes(be, n):
    """1, 63, 64 and 65 blocks, and B - 1, B, B + 1 for the B = 4 blocks of one workgroup; sizes cycle"""
    assert be.pkg.WEDGE_SEARCH_BLOCKS_PER_WORKGROUP == 4
    g = rng(900 + n)
    small = (3, 4, 5, 6, 18, 19)
    items = [(small[i % 6] if i % 9 else 9, 0) + mc.make_search_inputs(g, "near", small[i % 6] if i % 9 else 9, 8) for i in range(n)]
    got = run_search(be, items, 8)
    for i, (b, fs, src, q0, q1) in enumerate(items):
        check_search(got[i], mc.wedge_search(src, q0, q1, b, 8, fs), (n, i, b))


def test_search_golden_cases(be):
    """the search cases of tests/golden/maskpred.npz: the kernel == the reference's helpers composed as pick_wedge / pick_wedge_fixed_sign / pick_interinter_seg do"""
    gold = mc.load_golden()
    cases = mc.golden_search_cases()
    for bd in BIT_DEPTHS:
        idx = [i for i, c in enumerate(cases) if c[1] == bd]
        items = []
        for i in idx:
            src, q0, q1 = mc.golden_search_inputs(i, cases[i])
            assert int(src.astype(np.int64).sum()) + int(q0.astype(np.int64).sum()) + int(q1.astype(np.int64).sum()) == int(gold["search_insum_%d" % i][0])
            items.append((cases[i][0], cases[i][3], src, q0, q1))
        got = run_search(be, items, bd)
        for j, i in enumerate(idx):
            ref = gold["search_%d" % i]
            assert np.array_equal(got[j]["sse"], ref[:16]) and np.array_equal(got[j]["sse_diffwtd"], ref[16:18]) and np.array_equal(got[j]["sign"], ref[18:]), (i, cases[i])
            assert int(got[j]["best_wedge_index"]) == int(np.argmin(ref[:16])) and int(got[j]["best_mask_type"]) == int(ref[17] < ref[16]), (i, cases[i])


@pytest.mark.parametrize("what", ["bsize 4x4", "bsize 64x64", "bsize 22", "fixed_sign 3", "NULL plane", "plane 32"])
def test_search_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones: status == NULL -> -1 and no result written; with a status array the call returns 0, flags it alone, leaves its
    result untouched and searches the other two"""
    g = rng(10)
    items = [(b, 0) + mc.make_search_inputs(g, "near", b, 8) for b in (3, 6, 5)]
    n = 3
    d = np.zeros(n, be.pkg.WedgeSearchDesc)
    bufs, off = [], 0
    for i, (b, fs, src, q0, q1) in enumerate(items):
        for v, name in ((src, "src"), (q0, "p0"), (q1, "p1")):
            d[i][name + "_off"], d[i][name + "_stride"] = off, mc.BW[b]
            bufs.append(v.reshape(-1))
            off += v.size
        d[i]["bsize"] = b
    edits = {"bsize 4x4": ("bsize", 0), "bsize 64x64": ("bsize", 12), "bsize 22": ("bsize", 22), "fixed_sign 3": ("fixed_sign", 3), "NULL plane": ("p1_plane", 9),
             "plane 32": ("src_plane", 32)}
    d[edits[what][0]][1] = edits[what][1]
    planes = be.pkg.BlendPlanes()
    buf, dd = be.dev(np.concatenate(bufs)), be.dev(d)
    planes.base[0] = be.ptr(buf)
    out = be.dev(np.full(n * be.pkg.WedgeSearchResult.itemsize, 0xA5, np.uint8))
    assert be.lib.svt_hip_wedge_search_batch(planes, be.ptr(dd), n, 8, be.ptr(out), None, be.stream) == -1
    assert np.all(be.host(out) == 0xA5)
    status = be.dev(np.full(n, 7, np.uint8))
    assert be.lib.svt_hip_wedge_search_batch(planes, be.ptr(dd), n, 8, be.ptr(out), be.ptr(status), be.stream) == 0
    got = be.host(out).view(be.pkg.WedgeSearchResult)
    assert be.host(status).tolist() == [0, 1, 0]
    assert np.all(got[1:2].view(np.uint8) == 0xA5)
    for i in (0, 2):
        b, fs, src, q0, q1 = items[i]
        check_search(got[i], mc.wedge_search(src, q0, q1, b, 8, fs), (what, i))
    assert be.lib.svt_hip_wedge_search_batch(planes, be.ptr(dd), n, 11, be.ptr(out), None, be.stream) == -1  # not a bit depth


def test_helper_forms(be):
    """the two pixel-domain diff-weighted builders and the four wedge-search helpers as single calls: 8 / 10 / 12 bit residuals (the int16_t clamp of the SSE term and
    the saturation of the delta of squares bind at 10 and 12 bit: asserted), N from 1 to 128 x 128, the sign at limit - 1 / limit / limit + 1, the delta of squares in
    place; arguments outside the accepted range write nothing"""
    L = be.lib
    g = rng(21)
    for bd in BIT_DEPTHS:
        dt = np.uint16 if bd > 8 else np.uint8
        for kind in mc.CLASSES:
            for (w, h) in ((8, 8), (16, 32), (128, 128), (4, 2)):
                a, b = mc.make_pair(g, kind, w, h, bd)
                pa, pb = np.full((h, w + 3), 9, dt), np.full((h, w + 1), 9, dt)
                pa[:, :w], pb[:, :w] = a, b
                for t in (0, 1):
                    m = np.full(w * h + 4, 0xEE, np.uint8)
                    if bd == 8:
                        L.svt_av1_build_compound_diffwtd_mask_hip(p(m), t, p(pa), w + 3, p(pb), w + 1, h, w)
                    else:
                        L.svt_av1_build_compound_diffwtd_mask_highbd_hip(p(m), t, p(pa), w + 3, p(pb), w + 1, h, w, bd)
                    want = mc.diffwtd_mask(t, a, b, bd)
                    assert np.array_equal(m[:w * h].reshape(h, w), want) and np.all(m[w * h:] == 0xEE), (bd, kind, w, h, t)
                    if kind == "extreme":
                        assert np.all(want == (11 if t else 53))  # |a - b| is the whole range: 38 + 255 / 16, the largest value of the pixel-domain builders
                    if kind == "equal":
                        assert np.all(want == (26 if t else 38))
        for n in (1, 63, 64, 255, 256, 257, 1024, 16384):
            src, q0, q1 = (g.integers(0, 1 << bd, n).astype(np.int64) for _ in range(3))
            r0, r1, d10 = (src - q0).astype(np.int16), (src - q1).astype(np.int16), (q1 - q0).astype(np.int16)
            mask = g.integers(0, 65, n).astype(np.uint8)
            t, raw = mc.wedge_sse_terms(r1, d10, mask)
            if n >= 255:
                assert bool((t != raw).any()) == (bd > 8)
            assert L.svt_av1_wedge_sse_from_residuals_hip(p(r1), p(d10), p(mask), n) == int(mc.wedge_sse_from_residuals(r1, d10, mask)), (bd, n)
            assert L.svt_aom_sum_squares_i16_hip(p(r0), n) == int(mc.sum_squares_i16(r0)), (bd, n)
            ds = np.full(n + 2, 0x5A5A, np.int16)
            L.svt_av1_wedge_compute_delta_squares_hip(p(ds), p(r0), p(r1), n)
            want = mc.wedge_compute_delta_squares(r0, r1)
            assert np.array_equal(ds[:n], want) and np.all(ds[n:] == 0x5A5A), (bd, n)
            if n >= 255:
                assert (want == 32767).any() or (want == -32768).any()
            inpl = r0.copy()
            L.svt_av1_wedge_compute_delta_squares_hip(p(inpl), p(inpl), p(r1), n)
            assert np.array_equal(inpl, want)
            total = int((want.astype(np.int64) * mask).sum())
            for limit in (total - 1, total, total + 1, -(1 << 40), 1 << 40):
                assert L.svt_av1_wedge_sign_from_residuals_hip(p(want), p(mask), n, limit) == int(total > limit), (bd, n, limit)
    m, a = np.full(64, 0xEE, np.uint8), np.zeros((8, 8), np.uint8)
    L.svt_av1_build_compound_diffwtd_mask_hip(p(m), 2, p(a), 8, p(a), 8, 8, 8)      # not a mask type
    L.svt_av1_build_compound_diffwtd_mask_hip(p(m), 0, p(a), 8, p(a), 8, 0, 8)      # no rows
    L.svt_av1_build_compound_diffwtd_mask_highbd_hip(p(m), 0, p(a), 8, p(a), 8, 2, 2, 9)  # not a bit depth
    ds = np.full(8, 0x5A5A, np.int16)
    L.svt_av1_wedge_compute_delta_squares_hip(p(ds), p(ds), p(ds), 0)
    assert np.all(m == 0xEE) and np.all(ds == 0x5A5A)
    assert L.svt_av1_wedge_sse_from_residuals_hip(p(ds), p(ds), p(m), 0) == 0 and L.svt_aom_sum_squares_i16_hip(p(ds), 0) == 0
    assert L.svt_hip_debug_commit_violations() == 0


# ---- the masked compound (csrc/interpred.hip, the MASKED instantiation) -------------------------------------------------------------------------------------
import interpred_common as ipc  # noqa: E402

M_SIZES = [(4, 4), (4, 16), (8, 8), (16, 8), (32, 32), (64, 64), (128, 128), (8, 32)]
M_PHASES = [((0, 0), (8, 1)), ((1, 15), (0, 0)), ((15, 0), (0, 8)), ((8, 8), (1, 1)), ((0, 1), (15, 15))]  # copy + 2-D, 2-D + copy, x + y, ...


M_HALF = ((8, 8), (8, 8))  # both references at the half-pel phase in x and y: with SHARP / SHARP the strongest overshoot of the sub-pel kernels


def mspec(w, h, comp, ph=0, fx=0, fy=2, kinds=("random", "random"), bsize=0, idx=0, sign=0, mask_type=0, subw=0, subh=0, mask=None):
    return dict(w=w, h=h, comp=comp, ph=ph if isinstance(ph, tuple) else M_PHASES[ph % 5], fx=fx, fy=fy, kinds=kinds, bsize=bsize, idx=idx, sign=sign, mask_type=mask_type, subw=subw, subh=subh, mask=mask)


def m_build(be, specs, bd, g):
    """reference planes, explicit mask bytes, descriptors, the expected destination plane and the expected seg-mask buffer of one masked-compound launch"""
    dt = np.uint16 if bd > 8 else np.uint8
    x = y = shelf = 0
    pos = []
    for s in specs:
        gap = 1 + int(g.integers(0, 7))
        if x + gap + s["w"] + 7 > SA - 10:
            x, y, shelf = 0, y + shelf + 1, 0
        pos.append((x + gap, y))
        x, shelf = x + gap + s["w"] + 7, max(shelf, s["h"] + 7)
    rows = y + shelf + 1
    A = g.integers(0, 1 << bd, (rows + 4, SA)).astype(dt)
    B = g.integers(0, 1 << bd, (rows + 8, SB)).astype(dt)
    fill = 0xA5A5 if bd > 8 else 0xA5
    want = np.full((rows + 4, SD), fill, dt)
    d = np.zeros(len(specs), be.pkg.InterPredMaskedDesc)
    masks, mo, segs, so = [np.full(5, 0xEE, np.uint8)], 5, [np.full(3, 0xEE, np.uint8)], 3
    for i, (s, (x, y)) in enumerate(zip(specs, pos)):
        w, h = s["w"], s["h"]
        e0 = ipc.make_ext(g, s["kinds"][0], w, h, bd)
        if s["kinds"][1] == "complement":  # (of the 2 x 2 checkerboard: maximum where the first reference is zero)
            e1 = (((1 << bd) - 1) - e0).astype(e0.dtype)
        else:
            e1 = e0.copy() if s["kinds"][1] == "same" else ipc.make_ext(g, s["kinds"][1], w, h, bd)
        A[y:y + h + 7, x:x + w + 7] = e0
        B[y + 3:y + 3 + h + 7, x + 5:x + 5 + w + 7] = e1
        (sx0, sy0), (sx1, sy1) = s["ph"]
        if s["kinds"][1] == "same":
            sx1, sy1 = sx0, sy0
        p_ = d["p"][i]
        p_["src_off"], p_["src_stride"], p_["plane"] = ((y + 3) * SA + x + 3, (y + 6) * SB + x + 8), (SA, SB), (PLANE_A, PLANE_B)
        p_["dst_off"], p_["dst_stride"], p_["w"], p_["h"] = (y + 3) * SD + x + 3, SD, w, h
        p_["subpel_x"], p_["subpel_y"], p_["filter_x"], p_["filter_y"] = (sx0, sx1), (sy0, sy1), s["fx"], s["fy"]
        p_["compound"], p_["fwd_offset"], p_["bck_offset"] = i % 3, 9, 7  # ignored by the masked entry
        d["p"][i] = p_
        d[i]["comp_type"], d[i]["bsize"], d[i]["wedge_index"], d[i]["wedge_sign"] = s["comp"], s["bsize"], s["idx"], s["sign"]
        d[i]["mask_type"], d[i]["subw"], d[i]["subh"] = s["mask_type"], s["subw"], s["subh"]
        mask = None
        if s["comp"] == mc.COMP_WEDGE:
            mask = mc.wedge_masks()[(s["bsize"], s["idx"], s["sign"])]
        elif s["comp"] == mc.COMP_EXPLICIT:
            mask = s["mask"] if s["mask"] is not None else g.integers(0, 65, (h << s["subh"], w << s["subw"])).astype(np.uint8)
            pad = np.full((mask.shape[0], mask.shape[1] + 3), 0xEE, np.uint8)
            pad[:, :mask.shape[1]] = mask
            d[i]["mask_off"], d[i]["mask_stride"] = mo, pad.shape[1]
            masks.append(pad.reshape(-1)[:pad.size - 3])
            mo += pad.size - 3
        out, seg = mc.masked_compound([(e0, sx0, sy0), (e1, sx1, sy1)], w, h, s["fx"], s["fy"], bd, s["comp"], mask, s["mask_type"], s["subw"], s["subh"])
        want[y + 3:y + 3 + h, x + 3:x + 3 + w] = out
        if seg is not None:
            d[i]["seg_off"] = so
            segs += [seg.reshape(-1), np.full(3, 0xEE, np.uint8)]
            so += w * h + 3
            s["seg"] = seg
    return A, B, np.concatenate(masks), d, want, fill, np.concatenate(segs)


def m_launch(be, A, B, M, d, dst, seg, bd, status=None):
    planes = be.pkg.InterPredPlanes()
    keep = [be.dev(A), be.dev(B), be.dev(M), be.dev(d)]
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(keep[0]), be.ptr(keep[1])
    return be.lib.svt_hip_inter_pred_masked_batch(planes, be.ptr(dst), be.ptr(keep[2]), None if seg is None else be.ptr(seg), be.ptr(keep[3]), len(d), bd,
                                                  None if status is None else be.ptr(status), be.stream), keep


def m_run(be, specs, bd, seed, with_status=False, with_seg=True):
    g = rng(seed)
    A, B, M, d, want, fill, want_seg = m_build(be, specs, bd, g)
    dst = be.dev(np.full(want.shape, fill, want.dtype))
    seg = be.dev(np.full(want_seg.shape, 0xEE, np.uint8)) if with_seg else None
    status = be.dev(np.full(len(specs), 7, np.uint8)) if with_status else None
    r, keep = m_launch(be, A, B, M, d, dst, seg, bd, status)
    assert r == 0
    got = be.host(dst)
    if with_status:
        assert not be.host(status).any()
    if not np.array_equal(got, want):
        for i, s in enumerate(specs):
            y, x = divmod(int(d["p"][i]["dst_off"]), SD)
            a, b = got[y:y + s["h"], x:x + s["w"]], want[y:y + s["h"], x:x + s["w"]]
            assert np.array_equal(a, b), (bd, i, {k: v for k, v in s.items() if k not in ("mask", "seg")}, np.argwhere(a != b)[:4], a[:2, :8], b[:2, :8])
        raise AssertionError("samples outside every block's w x h were written: %s" % (np.argwhere(got != want)[:8],))
    if with_seg:
        assert np.array_equal(be.host(seg), want_seg)  # every seg mask, and the 0xEE bytes between them
    return specs


@pytest.mark.parametrize("bd", BIT_DEPTHS)
def test_masked_compound_every_size_and_type(be, bd):
    """the eight sizes x (DIFFWTD_38, DIFFWTD_38_INV, EXPLICIT with the four sub-samplings) with the two references in different cases (copy + 2-D, x + y, ...) at
    phases 1 / 8 / 15; WEDGE on the nine sizes at full size and through the three sub-samplings; every seg mask compared, with the bytes between them.  Inputs where
    |a - b| drives the diff-weighted clamp to 64 -- the 2 x 2 maximum / zero checkerboard against its complement under SHARP x SHARP at the half-pel phases, whose
    overshoot takes the two ConvBufType values further apart than the sample range -- and where it stays at 38 (the same block twice); unfiltered all-maximum against
    all-zero samples give 38 + 255 / 16 = 53 (54 at 10 and 12 bit).  All asserted on the restatement's own mask, so the test cannot pass on a constant mask or on a
    kernel without the clamp."""
    specs, k = [], 0
    for (w, h) in M_SIZES:
        for t in (0, 1):
            specs.append(mspec(w, h, mc.COMP_DIFFWTD, k, k % 3, (k + 1) % 3, mask_type=t))
            k += 1
        for (subw, subh) in SUBS:
            if w == 128 and (subw or subh):
                continue
            specs.append(mspec(w, h, mc.COMP_EXPLICIT, k, k % 3, (k + 2) % 3, subw=subw, subh=subh))
            k += 1
    for b in mc.WEDGE_BSIZES:
        for j, (subw, subh) in enumerate(SUBS):
            specs.append(mspec(mc.BW[b] >> subw, mc.BH[b] >> subh, mc.COMP_WEDGE, k, k % 3, k % 2, bsize=b, idx=(3 * k + j) % 16, sign=k % 2, subw=subw, subh=subh))
            k += 1
    for t in (0, 1):  # the clamp at 64: the 2 x 2 maximum / zero checkerboard against its complement, SHARP x SHARP at the half-pel phases -- the kernels overshoot
        for (w, h) in ((16, 16), (64, 64), (4, 4)):
            specs.append(mspec(w, h, mc.COMP_DIFFWTD, M_HALF, ipc.SHARP, ipc.SHARP, kinds=("checker", "complement"), mask_type=t))
    for t in (0, 1):
        specs.append(mspec(16, 16, mc.COMP_DIFFWTD, 0, kinds=("max", "zero"), mask_type=t))
        specs.append(mspec(16, 16, mc.COMP_DIFFWTD, 3, kinds=("random", "same"), mask_type=t))
    m_run(be, specs, bd, 1100 + bd, with_status=bd == 10)
    for s in specs[-10:-4]:
        if s["w"] >= 16:  # (the restatement's own mask: the clamp binds on part of the block and not on all of it)
            at = int((s["seg"] == (0 if s["mask_type"] else 64)).sum())
            assert 0 < at < s["seg"].size and (s["seg"].max() == 64 if not s["mask_type"] else s["seg"].min() == 0), (bd, s["w"], s["mask_type"], at)
    assert any(s["w"] >= 16 for s in specs[-10:-4])
    for s in specs[-4:]:
        hi = s["kinds"] == ("max", "zero")
        top = 53 if bd == 8 else 54  # 38 + 255 / 16; at 10 and 12 bit the rounding of 1023 / 4 and 4095 / 16 gives 256: 38 + 16
        assert np.all(s["seg"] == ((64 - top if hi else 26) if s["mask_type"] else (top if hi else 38))), (s["kinds"], s["mask_type"], s["seg"][0, :4])
    assert any(0 < int(s["seg"].min()) and 38 < int(s["seg"].max()) < 64 for s in specs if "seg" in s and s["kinds"] == ("random", "random") and not s["mask_type"])


@pytest.mark.parametrize("bd", (8, 10))
def test_masked_compound_seg_mask_feeds_chroma(be, bd):
    """the luma call writes the DIFFWTD seg mask to device memory; the chroma calls read it in place as EXPLICIT with stride w: a 4:2:0 block (subw = subh = 1) and a
    4:2:2 one (subw = 1, subh = 0); and a launch with seg_mask_base == NULL predicts the same samples"""
    g = rng(1200 + bd)
    luma = [mspec(16, 16, mc.COMP_DIFFWTD, 3, mask_type=0), mspec(32, 16, mc.COMP_DIFFWTD, 0, mask_type=1), mspec(8, 8, mc.COMP_DIFFWTD, 2, 1, 1)]
    A, B, M, d, want, fill, want_seg = m_build(be, luma, bd, g)
    dst, seg = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(want_seg.shape, 0xEE, np.uint8))
    r, keep = m_launch(be, A, B, M, d, dst, seg, bd)
    assert r == 0 and np.array_equal(be.host(dst), want) and np.array_equal(be.host(seg), want_seg)
    dst2 = be.dev(np.full(want.shape, fill, want.dtype))
    r, keep2 = m_launch(be, A, B, M, d, dst2, None, bd)
    assert r == 0 and np.array_equal(be.host(dst2), want)
    chroma = []
    for s, i in ((luma[0], 0), (luma[1], 1), (luma[2], 2)):
        for (subw, subh) in ((1, 1), (1, 0)):
            chroma.append(dict(mspec(s["w"] >> subw, s["h"] >> subh, mc.COMP_EXPLICIT, i + 1, 2, 0, subw=subw, subh=subh, mask=s["seg"]), luma=i))
    A2, B2, _, d2, want2, _, _ = m_build(be, chroma, bd, g)
    for j, c in enumerate(chroma):  # the mask is the luma launch's device buffer, read where it lies
        d2[j]["mask_off"], d2[j]["mask_stride"] = d[c["luma"]]["seg_off"], luma[c["luma"]]["w"]
    planes = be.pkg.InterPredPlanes()
    dA, dB, dd, dst3 = be.dev(A2), be.dev(B2), be.dev(d2), be.dev(np.full(want2.shape, fill, want2.dtype))
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    assert be.lib.svt_hip_inter_pred_masked_batch(planes, be.ptr(dst3), be.ptr(seg), None, be.ptr(dd), len(d2), bd, None, be.stream) == 0
    assert np.array_equal(be.host(dst3), want2)


@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_masked_compound_launch_sizes(be, n):
    g = rng(n)
    pool = [mspec(w, h, (mc.COMP_DIFFWTD, mc.COMP_EXPLICIT)[i % 2], i, i % 3, (i + 1) % 3, mask_type=i % 2) for i, (w, h) in enumerate(M_SIZES[:6] + [(8, 32), (16, 64)])]
    m_run(be, [dict(pool[int(g.integers(len(pool)))]) for _ in range(n)], 8, 1300 + n, with_status=n == 17)


@pytest.mark.parametrize("what", ["width 2", "height 2", "width 3", "comp_type 3", "subw 2", "wedge bsize 4x4", "wedge index 16", "wedge block larger than mask",
                                  "DIFFWTD mask_type 2", "DIFFWTD with subw", "phase 16", "second NULL plane", "explicit without mask_base"])
def test_masked_compound_invalid_descriptors(be, what):
    """an invalid descriptor between two valid ones, both status modes; `width 2` / `height 2`: a size svt_hip_inter_pred_batch accepts and the d16 functions do not"""
    g = rng(19)
    mid = mspec(16, 16, mc.COMP_WEDGE, 1, bsize=6, idx=5, sign=1) if what.startswith("wedge") else mspec(16, 16, mc.COMP_DIFFWTD, 1)
    specs = [mspec(8, 8, mc.COMP_WEDGE, 0, bsize=3, idx=2), mid, mspec(4, 4, mc.COMP_DIFFWTD, 2, mask_type=1)]
    if what == "explicit without mask_base":
        specs[1] = mspec(16, 16, mc.COMP_EXPLICIT, 1)
    A, B, M, d, want, fill, want_seg = m_build(be, specs, 8, g)
    y, x = divmod(int(d["p"][1]["dst_off"]), SD)
    want[y:y + 16, x:x + 16] = fill
    if "seg" in specs[1]:
        o = int(d[1]["seg_off"])
        want_seg[o:o + 256] = 0xEE
    pe = {"width 2": ("w", 2), "height 2": ("h", 2), "width 3": ("w", 3)}
    me = {"comp_type 3": ("comp_type", 3), "subw 2": ("subw", 2), "wedge bsize 4x4": ("bsize", 0), "wedge index 16": ("wedge_index", 16),
          "wedge block larger than mask": ("bsize", 3), "DIFFWTD mask_type 2": ("mask_type", 2), "DIFFWTD with subw": ("subw", 1)}
    if what in pe:
        d["p"][pe[what][0]][1] = pe[what][1]
    elif what in me:
        d[me[what][0]][1] = me[what][1]
    elif what == "phase 16":
        d["p"]["subpel_x"][1, 1] = 16
    elif what == "second NULL plane":
        d["p"]["plane"][1, 1] = 31
    planes = be.pkg.InterPredPlanes()
    dA, dB, dM, dd = be.dev(A), be.dev(B), be.dev(M), be.dev(d)
    planes.base[PLANE_A], planes.base[PLANE_B] = be.ptr(dA), be.ptr(dB)
    mptr = None if what == "explicit without mask_base" else be.ptr(dM)
    dst, seg = be.dev(np.full(want.shape, fill, want.dtype)), be.dev(np.full(want_seg.shape, 0xEE, np.uint8))
    assert be.lib.svt_hip_inter_pred_masked_batch(planes, be.ptr(dst), mptr, be.ptr(seg), be.ptr(dd), 3, 8, None, be.stream) == -1
    assert np.all(be.host(dst) == fill) and np.all(be.host(seg) == 0xEE)
    status = be.dev(np.full(3, 7, np.uint8))
    assert be.lib.svt_hip_inter_pred_masked_batch(planes, be.ptr(dst), mptr, be.ptr(seg), be.ptr(dd), 3, 8, be.ptr(status), be.stream) == 0
    assert np.array_equal(be.host(dst), want) and np.array_equal(be.host(seg), want_seg)
    assert be.host(status).tolist() == [0, 1, 0]
    assert be.lib.svt_hip_inter_pred_masked_batch(planes, be.ptr(dst), mptr, be.ptr(seg), be.ptr(dd), 1, 9, None, be.stream) == -1


def test_d16_forms(be):
    """svt_aom_lowbd_ / highbd_blend_a64_d16_mask_hip and svt_av1_build_compound_diffwtd_mask_d16_hip on ConvBufType blocks with their own strides: four sizes, four
    sub-samplings, 8 / 10 / 12 bit with the roundings of get_conv_params_no_round, values that reach both clips of the blend and the clamp of the builder at 64 and at 38"""
    L, pkg = be.lib, be.pkg
    g = rng(23)
    for bd in BIT_DEPTHS:
        r0, r1 = ipc.conv_rounds(bd, True)
        ro = ipc.round_offset(bd, r0, r1)
        hi = ro + (((1 << bd) - 1) << (14 - r0 - r1))
        for (w, h) in ((4, 4), (8, 16), (32, 32), (128, 4)):
            for k, (subw, subh) in enumerate(SUBS):
                lo_, hi_ = (ro - 40, hi + 40) if k % 2 else (ro, hi)  # (odd cases reach below 0 and above the maximum)
                a = g.integers(max(lo_, 0), min(hi_, 65535) + 1, (h, w)).astype(np.uint16)
                b = g.integers(max(lo_, 0), min(hi_, 65535) + 1, (h, w)).astype(np.uint16)
                pa, pb = np.full((h, w + 3), 1, np.uint16), np.full((h, w + 1), 2, np.uint16)
                pa[:, :w], pb[:, :w] = a, b
                mask = g.integers(0, 65, (h << subh, w << subw)).astype(np.uint8)
                mpl = np.full((mask.shape[0], mask.shape[1] + 5), 0xEE, np.uint8)
                mpl[:, :mask.shape[1]] = mask
                cp = pkg.ConvolveParams(0, 0, None, 0, r0, r1, 0, 1, 0, 0, 0, 0)
                dt, fill = (np.uint16, 0xA5A5) if bd > 8 else (np.uint8, 0xA5)
                dst = np.full((h + 1, w + 2), fill, dt)
                args = [p(dst), dst.shape[1], p(pa), w + 3, p(pb), w + 1, p(mpl), mpl.shape[1], w, h, subw, subh, C.addressof(cp)]
                if bd > 8:
                    L.svt_aom_highbd_blend_a64_d16_mask_hip(*args, bd)
                else:
                    L.svt_aom_lowbd_blend_a64_d16_mask_hip(*args)
                want = np.full_like(dst, fill)
                want[:h, :w] = mc.blend_a64_d16_mask(a, b, mask, subw, subh, bd, r0, r1)
                assert np.array_equal(dst, want), (bd, w, h, subw, subh)
                for t in (0, 1):
                    m = np.full(w * h + 4, 0xEE, np.uint8)
                    L.svt_av1_build_compound_diffwtd_mask_d16_hip(p(m), t, p(pa), w + 3, p(pb), w + 1, h, w, C.addressof(cp), bd)
                    wm = mc.diffwtd_mask_d16(t, a, b, bd, r0, r1)
                    assert np.array_equal(m[:w * h].reshape(h, w), wm) and np.all(m[w * h:] == 0xEE), (bd, w, h, t)
        far, same = np.full((8, 8), 65535, np.uint16), np.zeros((8, 8), np.uint16)  # (ConvBufType values no prediction produces: the clamp at 64)
        assert np.all(mc.diffwtd_mask_d16(0, far, same, bd, r0, r1) == 64) and np.all(mc.diffwtd_mask_d16(0, far, far, bd, r0, r1) == 38)
        cp = pkg.ConvolveParams(0, 0, None, 0, r0, r1, 0, 1, 0, 0, 0, 0)
        m = np.zeros(64, np.uint8)
        L.svt_av1_build_compound_diffwtd_mask_d16_hip(p(m), 0, p(far), 8, p(same), 8, 8, 8, C.addressof(cp), bd)
        assert np.all(m == 64)
        L.svt_av1_build_compound_diffwtd_mask_d16_hip(p(m), 1, p(far), 8, p(far), 8, 8, 8, C.addressof(cp), bd)
        assert np.all(m == 26)
    assert L.svt_hip_debug_commit_violations() == 0


@pytest.mark.parametrize("r0,r1", [(8, 6), (-1, 7), (3, 8), (3, -1), (7, 8)])
def test_d16_forms_reject_roundings_and_sizes_outside_the_accepted_range(be, r0, r1):
    """round_0 / round_1 outside the range of the jnt_ forms, a size below 4, a size that is no power of two: nothing is written"""
    L, pkg = be.lib, be.pkg
    a, mask = np.full((8, 8), 30000, np.uint16), np.full((16, 16), 32, np.uint8)
    for hbd in (False, True):
        dst = np.full((8, 8), 0xA5, np.uint16 if hbd else np.uint8)
        f = L.svt_aom_highbd_blend_a64_d16_mask_hip if hbd else L.svt_aom_lowbd_blend_a64_d16_mask_hip
        tail = [10] if hbd else []
        bad = pkg.ConvolveParams(0, 0, None, 0, r0, r1, 0, 1, 0, 0, 0, 0)
        good = pkg.ConvolveParams(0, 0, None, 0, 3, 7, 0, 1, 0, 0, 0, 0)
        f(p(dst), 8, p(a), 8, p(a), 8, p(mask), 16, 8, 8, 0, 0, C.addressof(bad), *tail)
        f(p(dst), 8, p(a), 8, p(a), 8, p(mask), 16, 2, 8, 0, 0, C.addressof(good), *tail)  # the d16 functions' own lower bound
        f(p(dst), 8, p(a), 8, p(a), 8, p(mask), 16, 8, 6, 0, 0, C.addressof(good), *tail)
        f(p(dst), 8, p(a), 8, p(a), 8, p(mask), 16, 8, 8, 2, 0, C.addressof(good), *tail)
        f(p(dst), 8, p(a), 8, p(a), 8, p(mask), 16, 8, 8, 0, 0, None, *tail)
        assert np.all(dst == 0xA5)
        m = np.full(64, 0xEE, np.uint8)
        L.svt_av1_build_compound_diffwtd_mask_d16_hip(p(m), 0, p(a), 8, p(a), 8, 8, 8, C.addressof(bad), 10)
        L.svt_av1_build_compound_diffwtd_mask_d16_hip(p(m), 2, p(a), 8, p(a), 8, 8, 8, C.addressof(good), 10)
        assert np.all(m == 0xEE)


def test_masked_compound_read_guard_on_the_emulator():
    """CPU only.  The EXPLICIT mask of svt_hip_inter_pred_masked_batch lies flush against inaccessible pages on either end: (w << subw) x (h << subh) bytes are read
    and not one more, with every sub-sampling; the references as in test_interpred's guard (3 before, 4 after)."""
    be = _backends.setdefault("emu", EmuBackend())
    g = rng(78)
    for bd in (8, 10):
        dt = np.uint16 if bd > 8 else np.uint8
        for (w, h) in ((4, 4), (16, 8), (32, 32)):
            for (subw, subh) in SUBS:
                for at_end in (True, False):
                    exts = [ipc.make_ext(g, "random", w, h, bd) for _ in range(2)]
                    maps = [_flush((h + 7) * (w + 7), dt, at_end) for _ in range(2)]
                    for (_, arr, _), e in zip(maps, exts):
                        arr[:] = e.reshape(-1)
                    mask = g.integers(0, 65, (h << subh, w << subw)).astype(np.uint8)
                    mm, am, pm = _flush(mask.size, np.uint8, at_end)
                    am[:] = mask.reshape(-1)
                    planes = be.pkg.InterPredPlanes()
                    planes.base[0], planes.base[1] = maps[0][2], maps[1][2]
                    d = np.zeros(1, be.pkg.InterPredMaskedDesc)
                    p_ = d["p"][0]
                    p_["src_off"], p_["src_stride"], p_["plane"], p_["dst_stride"], p_["w"], p_["h"] = 3 * (w + 7) + 3, w + 7, (0, 1), w, w, h
                    p_["subpel_x"], p_["subpel_y"], p_["filter_x"], p_["filter_y"] = (8, 1), (15, 8), ipc.SHARP, ipc.REGULAR
                    d["p"][0] = p_
                    d["comp_type"], d["mask_stride"], d["subw"], d["subh"] = mc.COMP_EXPLICIT, mask.shape[1], subw, subh
                    dst = np.zeros(w * h, dt)
                    assert be.lib.svt_hip_inter_pred_masked_batch(planes, p(dst), pm, None, p(d), 1, bd, None, None) == 0
                    want, _ = mc.masked_compound([(exts[0], 8, 15), (exts[1], 1, 8)], w, h, ipc.SHARP, ipc.REGULAR, bd, mc.COMP_EXPLICIT, mask, 0, subw, subh)
                    assert np.array_equal(dst.reshape(h, w), want), (bd, w, h, subw, subh, at_end)
                    del arr, am, maps, mm
