// dist.hip -- the distortion end of the mode-decision loop (residual -> transform -> quantise -> inverse + reconstruction -> DISTORTION) for gfx950:
// spatial SSE (picture_operators_c.c:65-83, pic_operators.c:174-197), coefficient-domain SSE (pic_operators.c:150-221) and the psy-rd energy term of this
// fork (psy_rd.c).  DESIGN.md 4.18 has the layout, the bound and the note on the high-bit-depth psy arithmetic.
//
//  * pixel_dist_kernel: one launch, n blocks of mixed sizes.  A workgroup takes 64 consecutive descriptors, flattens their 8x8 tiles into one list (prefix sum
//    of the tile counts in LDS) and hands tile u to thread u mod 256: a lane owns ONE 8x8 tile of both planes -- eight 8- or 16-byte loads per plane --, does the
//    two Hadamard energies, the SSE and the pixel sum in its own registers (no cross-lane traffic at all) and adds its two integers to the block's cells in LDS.
//    The 64 blocks' totals leave with plain stores: no global atomics, nothing to zero beforehand, results independent of launch order, and the host forms can run
//    the kernel on zero-copy buffers (HostCall::begin_small).  64 blocks of 64x64 fill 256 lanes 16 times over; 64 blocks of 8x8 fill one wave exactly.
//  * coeff_dist_kernel: one wave per block, 64-bit wrapping sums (the reference squares an int64 difference; at the int32 extremes that wraps, and so does this).
//  * rt pixel terms (svt_hip_txfm_quant_roundtrip_dist_batch, second launch): the same tile body on (source, prediction, reconstruction) -- the source energy is
//    computed once.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"

namespace {

constexpr int DPW = 64;  // descriptors per workgroup
constexpr int TPB = 256; // threads per workgroup

template <typename PIX> struct Tile; // one 8x8 tile as loaded: packed words, row-major
template <> struct Tile<uint8_t> {
    uint32_t w[8][2];
    __device__ __forceinline__ uint32_t px(int r, int c) const { return (w[r][c >> 2] >> (8 * (c & 3))) & 0xffu; }
};
template <> struct Tile<uint16_t> {
    uint32_t w[8][4];
    __device__ __forceinline__ uint32_t px(int r, int c) const { return (w[r][c >> 1] >> (16 * (c & 1))) & 0xffffu; }
};

// rows x cols (<= 8 x 8) pixels at p; what lies outside reads as zero and is never touched in memory
template <typename PIX>
__device__ __forceinline__ void load_tile(Tile<PIX>& t, const PIX* p, const uint32_t stride, const int rows, const int cols) {
    constexpr int NW = sizeof(PIX) * 2, PPW = 4 / sizeof(PIX);
    if (rows == 8 && cols == 8) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if constexpr (sizeof(PIX) == 1) {
                const svt_u32x2_a1 v = svt_hip_global_load_x2(p + (size_t)r * stride);
                t.w[r][0] = v[0]; t.w[r][1] = v[1];
            } else {
                const svt_u32x4_a2 v = svt_hip_global_load_x4(p + (size_t)r * stride);
                t.w[r][0] = v[0]; t.w[r][1] = v[1]; t.w[r][2] = v[2]; t.w[r][3] = v[3];
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
#pragma unroll
        for (int k = 0; k < NW; k++) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < PPW; j++) {
                const int c = k * PPW + j;
                if (r < rows && c < cols) word |= (uint32_t)p[(size_t)r * stride + c] << (8 * sizeof(PIX) * j);
            }
            t.w[r][k] = word;
        }
    }
}

// ---- SSE of one tile ------------------------------------------------------------------------------------------------
// 8-bit: sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b, three v_dot4_u32_u8 per four pixels (64 * 2 * 255^2 fits 32 bits)
__device__ __forceinline__ uint64_t tile_sse(const Tile<uint8_t>& a, const Tile<uint8_t>& b) {
    uint32_t sq = 0, ab = 0;
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            sq = __builtin_amdgcn_udot4(a.w[r][k], a.w[r][k], sq, false);
            sq = __builtin_amdgcn_udot4(b.w[r][k], b.w[r][k], sq, false);
            ab = __builtin_amdgcn_udot4(a.w[r][k], b.w[r][k], ab, false);
        }
    return (uint64_t)(sq - 2 * ab);
}
// 16-bit samples of any value (svt_full_distortion_kernel16_bits_c takes what it is given): one difference squared fits 32 bits, two need not
__device__ __forceinline__ uint64_t tile_sse(const Tile<uint16_t>& a, const Tile<uint16_t>& b) {
    uint64_t s = 0;
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int32_t  d = (int32_t)a.px(r, c) - (int32_t)b.px(r, c);
            const uint32_t m = (uint32_t)(d < 0 ? -d : d);
            s += (uint64_t)m * m;
        }
    return s;
}

// ---- psy energy, 8-bit (svt_psy_distortion, psy_rd.c:64-166) -------------------------------------------------------------------
// Against the zero block the reference's packed two-lane arithmetic never leaves its 16-bit lanes, so the value is the plain integer one:
// 8x8: (sum |H8 X H8| + 2) >> 2 minus (sum X >> 2); the pixel sum is the DC coefficient.  The butterflies' output order is irrelevant under sum | . |.
__device__ __forceinline__ void had8(int32_t* v) {
#pragma unroll
    for (int s = 1; s < 8; s <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (!(i & s)) { const int32_t x = v[i], y = v[i + s]; v[i] = x + y; v[i + s] = x - y; }
}
__device__ __forceinline__ int32_t energy8(const Tile<uint8_t>& t) {
    int32_t m[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
#pragma unroll
        for (int c = 0; c < 8; c++) m[r][c] = (int32_t)t.px(r, c);
        had8(m[r]);
    }
    int32_t satd = 0, dc = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int32_t v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = m[r][c];
        had8(v);
        if (c == 0) dc = v[0];
#pragma unroll
        for (int r = 0; r < 8; r++) satd += v[r] < 0 ? -v[r] : v[r];
    }
    return ((satd + 2) >> 2) - (dc >> 2);
}
// the 4x4 sub-block at (4 qy, 4 qx) of the tile: (sum |H4 X H4| >> 1) - (sum X >> 2)
__device__ __forceinline__ int32_t energy4(const Tile<uint8_t>& t, const int qy, const int qx) {
    int32_t m[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int32_t x0 = (int32_t)t.px(4 * qy + r, 4 * qx), x1 = (int32_t)t.px(4 * qy + r, 4 * qx + 1), x2 = (int32_t)t.px(4 * qy + r, 4 * qx + 2),
                      x3 = (int32_t)t.px(4 * qy + r, 4 * qx + 3);
        const int32_t a = x0 + x1, b = x0 - x1, c = x2 + x3, d = x2 - x3;
        m[r][0] = a + c; m[r][1] = b + d; m[r][2] = a - c; m[r][3] = b - d;
    }
    int32_t satd = 0, dc = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int32_t a = m[0][c] + m[1][c], b = m[0][c] - m[1][c], e = m[2][c] + m[3][c], f = m[2][c] - m[3][c];
        const int32_t v0 = a + e, v1 = b + f, v2 = a - e, v3 = b - f;
        if (c == 0) dc = v0;
        satd += (v0 < 0 ? -v0 : v0) + (v1 < 0 ? -v1 : v1) + (v2 < 0 ? -v2 : v2) + (v3 < 0 ? -v3 : v3);
    }
    return (satd >> 1) - (dc >> 2);
}

// ---- psy energy, high bit depth (svt_psy_distortion_hbd, psy_rd.c:171-271) -----------------------------------------------------
// NOT the 8-bit algorithm at another depth: the reference runs its Hadamard stages through 32-bit temporaries, so of every packed 64-bit value only
// the lower lane -- the pair SUMS -- survives, as a wrapping uint32 that is zero-extended again; the final two-lane absolute value then works on those 64-bit values.
// Encoder identity needs exactly that number.
__device__ __forceinline__ uint64_t lanes_abs(const uint64_t v) { // two-lane |.| of a packed value: lanes of 32 bits, sign bits 31 and 63
    const uint64_t m = (v >> 31) & 0x100000001ull, s = (m << 32) - m;
    return (v + s) ^ s;
}
__device__ __forceinline__ void had4_u32(uint32_t& d0, uint32_t& d1, uint32_t& d2, uint32_t& d3, const uint32_t s0, const uint32_t s1, const uint32_t s2, const uint32_t s3) {
    const uint32_t t0 = s0 + s1, t1 = s0 - s1, t2 = s2 + s3, t3 = s2 - s3;
    d0 = t0 + t2; d1 = t1 + t3; d2 = t0 - t2; d3 = t1 - t3;
}
__device__ __forceinline__ int32_t energy8(const Tile<uint16_t>& t) {
    uint32_t d[8][4];
    uint64_t pix = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = t.px(r, 2 * k) + t.px(r, 2 * k + 1);
        pix += (uint64_t)(p[0] + p[1] + p[2] + p[3]);
        had4_u32(d[r][0], d[r][1], d[r][2], d[r][3], p[0], p[1], p[2], p[3]);
    }
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t a[8];
        had4_u32(a[0], a[1], a[2], a[3], d[0][i], d[1][i], d[2][i], d[3][i]);
        had4_u32(a[4], a[5], a[6], a[7], d[4][i], d[5][i], d[6][i], d[7][i]);
        uint64_t b = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) b += lanes_abs((uint64_t)a[k] + (uint64_t)a[k + 4]) + lanes_abs((uint64_t)a[k] - (uint64_t)a[k + 4]);
        sum += (uint64_t)(uint32_t)b + (b >> 32);
    }
    return (int32_t)(uint32_t)(((sum + 2) >> 2) - (pix >> 2));
}
__device__ __forceinline__ int32_t energy4(const Tile<uint16_t>& t, const int qy, const int qx) {
    uint32_t lo[4][2];
    uint64_t pix = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t a = t.px(4 * qy + r, 4 * qx) + t.px(4 * qy + r, 4 * qx + 1), b = t.px(4 * qy + r, 4 * qx + 2) + t.px(4 * qy + r, 4 * qx + 3);
        lo[r][0] = a + b; lo[r][1] = a - b;
        pix += (uint64_t)(a + b);
    }
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        uint32_t a0, a1, a2, a3;
        had4_u32(a0, a1, a2, a3, lo[0][i], lo[1][i], lo[2][i], lo[3][i]);
        const uint64_t b = lanes_abs((uint64_t)a0) + lanes_abs((uint64_t)a1) + lanes_abs((uint64_t)a2) + lanes_abs((uint64_t)a3);
        sum += (uint64_t)(uint32_t)b + (b >> 32);
    }
    return (int32_t)(uint32_t)((sum >> 1) - (pix >> 2));
}

// |e_in - e_rec| as the reference's int32 arithmetic gives it (wrapping), widened the way `uint64_t += int` widens
__device__ __forceinline__ uint64_t nrg_absdiff(const int32_t a, const int32_t b) {
    const int32_t d = (int32_t)((uint32_t)a - (uint32_t)b);
    const int32_t m = d < 0 ? (int32_t)(0u - (uint32_t)d) : d;
    return (uint64_t)(int64_t)m;
}
template <typename PIX> struct TileEnergy { // the energies of a tile on the path its block takes: e0 of the 8x8, or e0..e3 of its four 4x4 quadrants
    int32_t e0, e1, e2, e3;
};
template <typename PIX> __device__ __forceinline__ TileEnergy<PIX> tile_energy(const Tile<PIX>& t, const bool path8) {
    TileEnergy<PIX> E;
    if (path8) {
        E.e0 = energy8(t);
        E.e1 = E.e2 = E.e3 = 0;
    } else { // (a quadrant outside the block is all zero: energy 0 on both sides)
        E.e0 = energy4(t, 0, 0); E.e1 = energy4(t, 0, 1); E.e2 = energy4(t, 1, 0); E.e3 = energy4(t, 1, 1);
    }
    return E;
}
template <typename PIX> __device__ __forceinline__ uint64_t energy_dist(const TileEnergy<PIX>& a, const TileEnergy<PIX>& b) {
    return nrg_absdiff(a.e0, b.e0) + nrg_absdiff(a.e1, b.e1) + nrg_absdiff(a.e2, b.e2) + nrg_absdiff(a.e3, b.e3);
}
// what svt_psy_distortion / _hbd do with the sum over sub-blocks (psy_rd.c:165, :270)
template <typename PIX> __device__ __forceinline__ uint64_t psy_scale(const uint64_t total) { return sizeof(PIX) == 1 ? total >> 1 : total << 2; }

// One block as the tile loop sees it.  NREC = 1: (input, recon); NREC = 2: (source, prediction, reconstruction) of the round trip.
template <typename PIX> struct BlockRef {
    const PIX *in, *rec[2];
    uint32_t   in_stride, rec_stride[2], width, height;
};

// WHAT: SVT_HIP_DIST_SSE | SVT_HIP_DIST_PSY.  FETCH(i) -> BlockRef of descriptor i.  OUT(i, k, sse, psy) stores the totals of plane pair k.
template <typename PIX, int WHAT, int NREC, typename FETCH, typename OUT>
__device__ __forceinline__ void dist_workgroup(const uint32_t n, const FETCH& fetch, const OUT& out) {
    __shared__ uint32_t           pre[DPW + 1];       // exclusive prefix sum of the tile counts
    __shared__ unsigned long long acc[DPW][2 * NREC]; // [block][pair * 2 + (0: sse, 1: psy)]
    const int      tid   = threadIdx.x;
    const uint32_t first = blockIdx.x * DPW;
    if (tid < DPW) { // (the first wave, whole: the scan's shuffles are wave-uniform)
        uint32_t cnt = 0;
        if (first + tid < n) {
            const BlockRef<PIX> b = fetch(first + tid);
            cnt                  = ((b.width + 7) >> 3) * ((b.height + 7) >> 3);
        }
        uint32_t inc = cnt;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, s);
            if (tid >= s) inc += o;
        }
        pre[tid + 1] = inc;
        if (tid == 0) pre[0] = 0;
#pragma unroll
        for (int k = 0; k < 2 * NREC; k++) acc[tid][k] = 0;
    }
    __syncthreads();
    const uint32_t total = pre[DPW];
    for (uint32_t u = tid; u < total; u += TPB) {
        int di = 0;
#pragma unroll
        for (int s = DPW >> 1; s >= 1; s >>= 1)
            if (pre[di + s] <= u) di += s;
        const BlockRef<PIX> b   = fetch(first + di);
        const uint32_t      loc = u - pre[di], nbx = (b.width + 7) >> 3, ty = loc / nbx, tx = loc - ty * nbx;
        const int           rows = (int)(b.height - 8 * ty < 8 ? b.height - 8 * ty : 8), cols = (int)(b.width - 8 * tx < 8 ? b.width - 8 * tx : 8);
        const bool          path8 = b.width >= 8 && b.height >= 8;
        Tile<PIX>           a, r;
        TileEnergy<PIX>     ea = {0, 0, 0, 0};
        load_tile(a, b.in + (size_t)(8 * ty) * b.in_stride + 8 * tx, b.in_stride, rows, cols);
        if (WHAT & SVT_HIP_DIST_PSY) ea = tile_energy(a, path8);
#pragma unroll
        for (int k = 0; k < NREC; k++) {
            load_tile(r, b.rec[k] + (size_t)(8 * ty) * b.rec_stride[k] + 8 * tx, b.rec_stride[k], rows, cols);
            if (WHAT & SVT_HIP_DIST_SSE) atomicAdd(&acc[di][2 * k], (unsigned long long)tile_sse(a, r));
            if (WHAT & SVT_HIP_DIST_PSY) {
                const TileEnergy<PIX> er = tile_energy(r, path8);
                atomicAdd(&acc[di][2 * k + 1], (unsigned long long)energy_dist(ea, er));
            }
        }
    }
    __syncthreads();
    if (tid < DPW && first + tid < n) {
#pragma unroll
        for (int k = 0; k < NREC; k++) out(first + tid, k, (uint64_t)acc[tid][2 * k], psy_scale<PIX>((uint64_t)acc[tid][2 * k + 1]));
    }
}

template <typename PIX, int WHAT>
__global__ __launch_bounds__(TPB) void pixel_dist_kernel(const PIX* __restrict__ in_base, const PIX* __restrict__ rec_base, const SvtHipDistDesc* __restrict__ descs,
                                                         const uint32_t n, uint64_t* __restrict__ sse_out, uint64_t* __restrict__ psy_out) {
    dist_workgroup<PIX, WHAT, 1>(
        n,
        [=](const uint32_t i) {
            const SvtHipDistDesc d = descs[i];
            BlockRef<PIX>        b;
            b.in = in_base + d.in_off; b.rec[0] = rec_base + d.rec_off; b.rec[1] = nullptr;
            b.in_stride = d.in_stride; b.rec_stride[0] = d.rec_stride; b.rec_stride[1] = 0;
            b.width = d.width; b.height = d.height;
            return b;
        },
        [=](const uint32_t i, int, const uint64_t sse, const uint64_t psy) {
            if (WHAT & SVT_HIP_DIST_SSE) sse_out[i] = sse;
            if (WHAT & SVT_HIP_DIST_PSY) psy_out[i] = psy;
        });
}

// the pixel terms of the round trip: (source, prediction) and (source, reconstruction) of n blocks of one TX size
template <typename PIX>
__global__ __launch_bounds__(TPB) void rt_pixel_dist_kernel(const PIX* __restrict__ src_base, const SvtHipPlaneRef* __restrict__ src, const PIX* __restrict__ pred_base,
                                                            const PIX* __restrict__ recon_base, const SvtHipRoundtripDesc* __restrict__ descs, const uint32_t n,
                                                            const uint32_t w, const uint32_t h, SvtHipRdDist* __restrict__ out) {
    dist_workgroup<PIX, SVT_HIP_DIST_SSE | SVT_HIP_DIST_PSY, 2>(
        n,
        [=](const uint32_t i) {
            const SvtHipRoundtripDesc d = descs[i];
            const SvtHipPlaneRef      s = src[i];
            BlockRef<PIX>             b;
            b.in = src_base + s.off; b.rec[0] = pred_base + d.pred_off; b.rec[1] = recon_base + d.recon_off;
            b.in_stride = s.stride; b.rec_stride[0] = d.pred_stride; b.rec_stride[1] = d.recon_stride;
            b.width = w; b.height = h;
            return b;
        },
        [=](const uint32_t i, const int k, const uint64_t sse, const uint64_t psy) {
            if (k == 0) { out[i].sse_pred = sse; out[i].psy_pred = psy; }
            else { out[i].sse_recon = sse; out[i].psy_recon = psy; }
        });
}

// ---- coefficient-domain distortion (pic_operators.c:150-221): one wave per block ----------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__global__ __launch_bounds__(TPB) void coeff_dist_kernel(const int32_t* __restrict__ coeff_base, const int32_t* __restrict__ recon_base,
                                                         const SvtHipCoeffDistDesc* __restrict__ descs, const uint32_t n, uint64_t* __restrict__ dist_out) {
    const uint32_t blk = blockIdx.x * (TPB / 64) + threadIdx.x / 64;
    const int      lane = threadIdx.x & 63;
    if (blk >= n) return; // (whole waves)
    const SvtHipCoeffDistDesc d = descs[blk];
    const int32_t*            c = coeff_base + d.coeff_off;
    const int32_t*            r = d.cbf_zero ? nullptr : recon_base + d.recon_off; // cbf_zero: recon_coeff is not read
    const uint32_t            w = d.width, cnt = w * d.height;
    uint64_t                  res = 0, pred = 0;
    for (uint32_t i = lane; i < cnt; i += 64) {
        const uint32_t y = i / w, x = i - y * w;
        const int64_t  cv = c[(size_t)y * d.coeff_stride + x];
        pred += (uint64_t)(cv * cv);
        if (r) {
            const uint64_t df = (uint64_t)(cv - (int64_t)r[(size_t)y * d.recon_stride + x]);
            res += df * df; // (an int32 difference can reach 2^32: its square wraps at 64 bits, in the reference too)
        }
    }
    res  = wave_sum_u64(res);
    pred = wave_sum_u64(pred);
    if (lane == 0) {
        dist_out[2 * (size_t)blk]     = r ? res : pred;
        dist_out[2 * (size_t)blk + 1] = pred;
    }
}

template <typename PIX>
void launch_pixel(const void* in, const void* rec, const SvtHipDistDesc* descs, uint32_t n, int what, uint64_t* sse, uint64_t* psy, hipStream_t st) {
    const dim3 grid((n + DPW - 1) / DPW), block(TPB);
    switch (what) {
    case SVT_HIP_DIST_SSE: hipLaunchKernelGGL(HIP_KERNEL_NAME(pixel_dist_kernel<PIX, 1>), grid, block, 0, st, (const PIX*)in, (const PIX*)rec, descs, n, sse, psy); break;
    case SVT_HIP_DIST_PSY: hipLaunchKernelGGL(HIP_KERNEL_NAME(pixel_dist_kernel<PIX, 2>), grid, block, 0, st, (const PIX*)in, (const PIX*)rec, descs, n, sse, psy); break;
    default: hipLaunchKernelGGL(HIP_KERNEL_NAME(pixel_dist_kernel<PIX, 3>), grid, block, 0, st, (const PIX*)in, (const PIX*)rec, descs, n, sse, psy); break;
    }
    SVT_LAUNCH_CHECK();
}

// One block from host memory: both planes packed into the call's arena, one descriptor, the two results read back with ONE synchronisation
void pixel_host(const void* input, uint32_t in_stride, const void* recon, uint32_t rec_stride, uint32_t w, uint32_t h, int is16, int what, uint64_t* sse, uint64_t* psy) {
    uint64_t r[2] = {0, 0};
    if (w && h) {
        svthip::HostCall& c = svthip::host_call();
        c.begin_small();
        const size_t px = is16 ? 2 : 1, pitch = svthip::align_up((size_t)w * px, 16), bytes = 2 * pitch * h + 4096;
        c.reserve(bytes, bytes);
        uint8_t*        di = (uint8_t*)c.dalloc(pitch * h);
        uint8_t*        dr = (uint8_t*)c.dalloc(pitch * h);
        SvtHipDistDesc* dd = (SvtHipDistDesc*)c.dalloc(sizeof(SvtHipDistDesc));
        uint64_t*       o  = (uint64_t*)c.dalloc(16);
        c.up2d(di, pitch, input, (size_t)in_stride * px, (size_t)w * px, h);
        c.up2d(dr, pitch, recon, (size_t)rec_stride * px, (size_t)w * px, h);
        SvtHipDistDesc ds = {0, 0, (uint32_t)(pitch / px), (uint32_t)(pitch / px), (uint16_t)w, (uint16_t)h, 0};
        c.up(dd, &ds, sizeof(ds));
        svt_hip_pixel_dist_batch(di, dr, dd, 1, is16, what, o, o + 1, c.stream);
        c.down(r, o, 16);
    }
    if (sse) *sse = r[0];
    if (psy) *psy = r[1];
}
void coeff_host(const int32_t* coeff, uint32_t coeff_stride, const int32_t* recon, uint32_t recon_stride, uint64_t* result, uint32_t w, uint32_t h) {
    uint64_t r[2] = {0, 0};
    if (w && h) {
        svthip::HostCall& c = svthip::host_call();
        c.begin_small();
        const size_t plane = (size_t)w * h * 4;
        c.reserve(2 * plane + 4096, 2 * plane + 4096);
        int32_t*             dc = (int32_t*)c.dalloc(plane);
        int32_t*             dr = (int32_t*)c.dalloc(plane);
        SvtHipCoeffDistDesc* dd = (SvtHipCoeffDistDesc*)c.dalloc(sizeof(SvtHipCoeffDistDesc));
        uint64_t*            o  = (uint64_t*)c.dalloc(16);
        c.up2d(dc, (size_t)w * 4, coeff, (size_t)coeff_stride * 4, (size_t)w * 4, h);
        if (recon) c.up2d(dr, (size_t)w * 4, recon, (size_t)recon_stride * 4, (size_t)w * 4, h);
        SvtHipCoeffDistDesc ds = {0, 0, w, w, (uint16_t)w, (uint16_t)h, (uint8_t)(recon ? 0 : 1), {0, 0, 0}};
        c.up(dd, &ds, sizeof(ds));
        svt_hip_coeff_dist_batch(dc, dr, dd, 1, o, c.stream);
        c.down(r, o, 16);
    }
    result[0] = r[0];
    result[1] = r[1];
}

} // namespace

namespace svthip {
void rt_pixel_dist_launch(const void* src_base, const SvtHipPlaneRef* src, const void* pred_base, const void* recon_base, const SvtHipRoundtripDesc* descs, uint32_t n,
                          int w, int h, int is16, SvtHipRdDist* out, hipStream_t st) {
    const dim3 grid((n + DPW - 1) / DPW), block(TPB);
    if (is16)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(rt_pixel_dist_kernel<uint16_t>), grid, block, 0, st, (const uint16_t*)src_base, src, (const uint16_t*)pred_base,
                           (const uint16_t*)recon_base, descs, n, (uint32_t)w, (uint32_t)h, out);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(rt_pixel_dist_kernel<uint8_t>), grid, block, 0, st, (const uint8_t*)src_base, src, (const uint8_t*)pred_base,
                           (const uint8_t*)recon_base, descs, n, (uint32_t)w, (uint32_t)h, out);
    SVT_LAUNCH_CHECK();
}
} // namespace svthip

extern "C" {

void svt_hip_pixel_dist_batch(const void* input_base, const void* recon_base, const SvtHipDistDesc* descs, uint32_t n, int is16, int what, uint64_t* sse_out,
                              uint64_t* psy_out, void* stream) {
    svthip::ensure_device();
    what &= SVT_HIP_DIST_SSE | SVT_HIP_DIST_PSY;
    if (n == 0 || what == 0) return;
    if (is16) launch_pixel<uint16_t>(input_base, recon_base, descs, n, what, sse_out, psy_out, (hipStream_t)stream);
    else launch_pixel<uint8_t>(input_base, recon_base, descs, n, what, sse_out, psy_out, (hipStream_t)stream);
}
void svt_hip_coeff_dist_batch(const int32_t* coeff_base, const int32_t* recon_coeff_base, const SvtHipCoeffDistDesc* descs, uint32_t n, uint64_t* dist_out, void* stream) {
    svthip::ensure_device();
    if (n == 0) return;
    hipLaunchKernelGGL(coeff_dist_kernel, dim3((n + TPB / 64 - 1) / (TPB / 64)), dim3(TPB), 0, (hipStream_t)stream, coeff_base, recon_coeff_base, descs, n, dist_out);
    SVT_LAUNCH_CHECK();
}

// ---- RTCD-signature single-call forms (common_dsp_rtcd.h:160-169, psy_rd.h:23-32) ----------------------------------------------------------------
uint64_t svt_spatial_full_distortion_kernel_hip(uint8_t* input, uint32_t input_offset, uint32_t input_stride, uint8_t* recon, int32_t recon_offset, uint32_t recon_stride,
                                                uint32_t area_width, uint32_t area_height) {
    uint64_t sse;
    pixel_host(input + input_offset, input_stride, recon + recon_offset, recon_stride, area_width, area_height, 0, SVT_HIP_DIST_SSE, &sse, nullptr);
    return sse;
}
uint64_t svt_full_distortion_kernel16_bits_hip(uint8_t* input, uint32_t input_offset, uint32_t input_stride, uint8_t* recon, int32_t recon_offset, uint32_t recon_stride,
                                               uint32_t area_width, uint32_t area_height) {
    uint64_t sse; // (the pointers are uint16_t planes behind a byte type; offsets and strides count samples: pic_operators.c:180-183)
    pixel_host((const uint16_t*)input + input_offset, input_stride, (const uint16_t*)recon + recon_offset, recon_stride, area_width, area_height, 1, SVT_HIP_DIST_SSE, &sse,
               nullptr);
    return sse;
}
void svt_full_distortion_kernel32_bits_hip(int32_t* coeff, uint32_t coeff_stride, int32_t* recon_coeff, uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                           uint32_t area_width, uint32_t area_height) {
    coeff_host(coeff, coeff_stride, recon_coeff, recon_coeff_stride, distortion_result, area_width, area_height);
}
void svt_full_distortion_kernel_cbf_zero32_bits_hip(int32_t* coeff, uint32_t coeff_stride, uint64_t distortion_result[2], uint32_t area_width, uint32_t area_height) {
    coeff_host(coeff, coeff_stride, nullptr, 0, distortion_result, area_width, area_height);
}
uint64_t svt_psy_distortion_hip(const uint8_t* input, uint32_t input_stride, const uint8_t* recon, uint32_t recon_stride, uint32_t width, uint32_t height) {
    uint64_t psy;
    pixel_host(input, input_stride, recon, recon_stride, width, height, 0, SVT_HIP_DIST_PSY, nullptr, &psy);
    return psy;
}
uint64_t svt_psy_distortion_hbd_hip(const uint16_t* input, uint32_t input_stride, const uint16_t* recon, uint32_t recon_stride, uint32_t width, uint32_t height) {
    uint64_t psy;
    pixel_host(input, input_stride, recon, recon_stride, width, height, 1, SVT_HIP_DIST_PSY, nullptr, &psy);
    return psy;
}
uint64_t svt_get_psy_full_dist_hip(const void* s, uint32_t so, uint32_t sp, const void* r, uint32_t ro, uint32_t rp, uint32_t w, uint32_t h, uint8_t is_hbd,
                                   double psy_rd) {
    const uint64_t raw = is_hbd == 1 ? svt_psy_distortion_hbd_hip((const uint16_t*)s + so, sp, (const uint16_t*)r + ro, rp, w, h)
                                     : svt_psy_distortion_hip((const uint8_t*)s + so, sp, (const uint8_t*)r + ro, rp, w, h);
    return (uint64_t)((double)raw * psy_rd); // host arithmetic, IEEE double, as psy_rd.c:292
}
uint64_t svt_spatial_psy_distortion_kernel_hip(uint8_t* input, uint32_t input_offset, uint32_t input_stride, uint8_t* recon, int32_t recon_offset, uint32_t recon_stride,
                                               uint32_t area_width, uint32_t area_height, double psy_rd) {
    uint64_t sse = 0, raw = 0; // one launch: both terms from the same loaded pixels
    pixel_host(input + input_offset, input_stride, recon + recon_offset, recon_stride, area_width, area_height, 0,
               psy_rd > 0.0 ? (SVT_HIP_DIST_SSE | SVT_HIP_DIST_PSY) : SVT_HIP_DIST_SSE, &sse, &raw);
    return sse + (psy_rd > 0.0 ? (uint64_t)((double)raw * psy_rd) : 0);
}

} // extern "C"

SVT_HIP_DEFINE_WARM(dist) // (svt_hip_warmup loads this translation unit's code object at encoder initialisation: svt_hip_common.h)
