// maskpred.hip -- masked prediction for gfx950: what a device-resident caller needs, besides svt_hip_inter_pred_batch and svt_hip_intra_pred_batch, to form the
// inter-intra, OBMC and wedge predictors of AV1 and to run the wedge / diff-weighted search.  DESIGN.md 4.22 has the layout, the literal roundings and the bounds.
//
//  * the tables: the 9 x 16 x 2 wedge masks svt_av1_init_wedge_masks leaves behind (inter_prediction.c:1976-2123) are generated ON THE DEVICE, once per device, by
//    wedge_fill_kernel from the three 64-entry primary rows, the three codebooks and the sign-flip table, into a 100 352-byte device array; ii_weights1d with
//    ii_size_scales (:2128-2141) and the six OBMC masks (:2407-2417) are kernel-side constants.
//  * blend_kernel: one launch, n descriptors of mixed sizes, svt_aom_blend_a64_mask_c / _hmask_c / _vmask_c and their highbd forms (blend_a64_mask.c:201-340,
//    inter_prediction.c:2374) bit for bit.  Flattened like inter_pred_kernel: a workgroup takes 16 descriptors, a prefix sum of their tile counts, ONE WAVE per tile of at
//    most 512 samples, the descriptor through v_readfirstlane, scalar branches on kind and mask source.  A lane loads the two source samples and the mask value(s) of a
//    sample, then stores it: dst may be one of the sources at the same position and stride.
//  * wedge_search_kernel: one wave per luma block of one of the nine wedge sizes.  residual1, diff10, the saturated delta of squares and the two diff-weighted masks are
//    formed once in registers (at most 16 samples per lane); the 16 masks are swept over them, a wave's 64 consecutive mask bytes being one coalesced load.  64-bit sums,
//    reduced across the wave by butterflies; no atomics, the results are plain stores of lane 0.
//  * d16_blend_kernel / diffwtd_d16_kernel: the three d16 functions of the masked compound as single calls (the batched masked compound itself is an instantiation of
//    inter_pred_kernel in interpred.hip, which takes the wedge table's address from svthip::wedge_table below).
//  * wedge_helper_kernel / diffwtd_kernel: the four residual-domain helpers and the two pixel-domain diff-weighted mask builders behind their single-call forms.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include "maskpred_tables.h"
#include <atomic>
#include <mutex>

namespace {
using namespace svt_maskpred; // kBw, kBh, kSlotBsize, kSlotOff, wedge_slot: the wedge table's layout

constexpr int DPW     = 16;  // descriptors per workgroup group
constexpr int TPB     = 256; // threads per workgroup
constexpr int WAVES   = TPB / 64;
constexpr int SPLIT   = 4;   // workgroups (blockIdx.y) that share one descriptor group's tile list
constexpr int TILE_W  = 32;
constexpr int TILE_PX = 512;
constexpr int NPL     = TILE_PX / 64;
constexpr int WEDGE_BYTES = 100352;
constexpr int MAX_SEARCH_NPL = 16; // a 32x32 block: 1024 samples over 64 lanes

// codebook of a slot: 0 = h == w, 1 = h > w, 2 = h < w
__device__ constexpr uint8_t kSlotBook[9] = {0, 1, 2, 0, 1, 2, 0, 1, 2};
// wedge_signflip_lookup (:1456-1853), bit i = wedge index i
__device__ constexpr uint16_t kSignFlip[9] = {0xBBFF, 0xBBEF, 0xBBEF, 0xBBFF, 0xBBEF, 0xBBEF, 0xBBFF, 0xBAEF, 0xABEF};
// the primary rows (:1440-1454): a soft step from 0 to 64 around position 32
__device__ constexpr uint8_t kPrimary[3][12] = {
    {0, 1, 4, 11, 27, 46, 58, 62, 63, 64, 64, 64}, // oblique, even rows: positions 27 .. 38
    {0, 1, 2, 6, 18, 37, 53, 60, 63, 64, 64, 64},  // oblique, odd rows
    {0, 0, 2, 7, 21, 43, 57, 62, 64, 64, 64, 64}}; // vertical
enum { W_HORZ = 0, W_VERT = 1, W_OBL27 = 2, W_OBL63 = 3, W_OBL117 = 4, W_OBL153 = 5 };
// the codebooks (:1855-1910): direction, x_offset, y_offset in eighths of the block
struct WedgeCode { uint8_t dir, xo, yo; };
__device__ constexpr WedgeCode kBook[3][16] = {
    // h == w
    {{W_OBL27, 4, 4}, {W_OBL63, 4, 4}, {W_OBL117, 4, 4}, {W_OBL153, 4, 4}, {W_HORZ, 4, 2}, {W_HORZ, 4, 6}, {W_VERT, 2, 4}, {W_VERT, 6, 4},
     {W_OBL27, 4, 2}, {W_OBL27, 4, 6}, {W_OBL153, 4, 2}, {W_OBL153, 4, 6}, {W_OBL63, 2, 4}, {W_OBL63, 6, 4}, {W_OBL117, 2, 4}, {W_OBL117, 6, 4}},
    // h > w
    {{W_OBL27, 4, 4}, {W_OBL63, 4, 4}, {W_OBL117, 4, 4}, {W_OBL153, 4, 4}, {W_HORZ, 4, 2}, {W_HORZ, 4, 4}, {W_HORZ, 4, 6}, {W_VERT, 4, 4},
     {W_OBL27, 4, 2}, {W_OBL27, 4, 6}, {W_OBL153, 4, 2}, {W_OBL153, 4, 6}, {W_OBL63, 2, 4}, {W_OBL63, 6, 4}, {W_OBL117, 2, 4}, {W_OBL117, 6, 4}},
    // h < w
    {{W_OBL27, 4, 4}, {W_OBL63, 4, 4}, {W_OBL117, 4, 4}, {W_OBL153, 4, 4}, {W_VERT, 2, 4}, {W_VERT, 4, 4}, {W_VERT, 6, 4}, {W_HORZ, 4, 4},
     {W_OBL27, 4, 2}, {W_OBL27, 4, 6}, {W_OBL153, 4, 2}, {W_OBL153, 4, 6}, {W_OBL63, 2, 4}, {W_OBL63, 6, 4}, {W_OBL117, 2, 4}, {W_OBL117, 6, 4}}};
// ii_weights1d / ii_size_scales (:2128-2141)
__device__ constexpr uint8_t kIiWeights[128] = {
    60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20, 19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14,
    13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9,  9,  9,  8,  8,  8,  8,  7,  7,  7,  7,  6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  4,  3,  3,  3,  3,
    3,  3,  3,  3,  3,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};
__device__ constexpr uint8_t kIiScale[22] = {32, 16, 16, 16, 8, 8, 8, 4, 4, 4, 2, 2, 2, 1, 1, 1, 8, 8, 4, 4, 2, 2};
// obmc_mask_1 .. obmc_mask_32 (:2407-2417) back to back: the mask of length n starts at n - 1
__device__ constexpr uint8_t kObmc[63] = {64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,
                                          33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64};

__device__ uint8_t g_wedge[WEDGE_BYTES]; // slot, wedge index, sign, row, column; one instance per device, written by wedge_fill_kernel

__device__ __forceinline__ int primary_at(const int row, int pos) { // the 64-entry primary row: 0 below position 27, 64 above 38
    pos = pos < 0 ? 0 : (pos > 63 ? 63 : pos);                       // shift_copy (:1960-1969) replicates the row's ends
    return pos < 27 ? 0 : (pos > 38 ? 64 : kPrimary[row][pos - 27]);
}
// wedge_mask_obl[0][WEDGE_OBLIQUE63][i][j] after init_wedge_primary_masks (:1989-2002): row i is the even / odd primary shifted by 16 - (i + 1) / 2
__device__ __forceinline__ int obl63(const int i, const int j) { return primary_at(i & 1, j - 16 + ((i + 1) >> 1)); }
// wedge_mask_obl[neg][dir][r][c] (:2019-2034): OBLIQUE27 is the transpose, 117 / 153 the mirrored complements, HORIZONTAL the transpose of VERTICAL
__device__ __forceinline__ int primary_mask(const int neg, const int dir, const int r, const int c) {
    int v;
    switch (dir) {
    case W_VERT: v = primary_at(2, c); break;
    case W_HORZ: v = primary_at(2, r); break;
    case W_OBL63: v = obl63(r, c); break;
    case W_OBL27: v = obl63(c, r); break;
    case W_OBL117: v = 64 - obl63(r, 63 - c); break;
    default: v = 64 - obl63(c, 63 - r); break;
    }
    return neg ? 64 - v : v;
}
// get_wedge_mask_inplace + init_wedge_masks (:2074-2114): every byte of the table from its own position
__global__ __launch_bounds__(TPB) void wedge_fill_kernel(int) {
    for (uint32_t p = blockIdx.x * TPB + threadIdx.x; p < (uint32_t)WEDGE_BYTES; p += gridDim.x * TPB) {
        int slot = 0;
        while (kSlotOff[slot + 1] <= p) slot++;
        const int      bsize = kSlotBsize[slot], bw = kBw[bsize], bh = kBh[bsize], n = bw * bh;
        const uint32_t q = p - kSlotOff[slot];
        const int      idx = (int)(q / (uint32_t)(2 * n)), sign = (int)(q / (uint32_t)n) & 1, pos = (int)(q % (uint32_t)n), y = pos / bw, x = pos % bw;
        const WedgeCode a    = kBook[kSlotBook[slot]][idx];
        const int      woff = (a.xo * bw) >> 3, hoff = (a.yo * bh) >> 3, flip = (kSignFlip[slot] >> idx) & 1;
        g_wedge[p]          = (uint8_t)primary_mask(sign ^ flip, a.dir, 32 - hoff + y, 32 - woff + x);
    }
}

__device__ __forceinline__ bool blend_dim_ok(const uint32_t v) { return v >= 1 && v <= 128 && (v & (v - 1)) == 0; }
// everything blend_kernel relies on
__device__ __forceinline__ bool blend_desc_ok(const SvtHipBlendDesc& d, const SvtHipBlendPlanes& planes, const uint8_t* mask_base) {
    if (!blend_dim_ok(d.w) || !blend_dim_ok(d.h) || d.kind > SVT_HIP_BLEND_VMASK || d.mask_src > SVT_HIP_MASK_OBMC || d.subw > 1 || d.subh > 1) return false;
    for (int k = 0; k < 2; k++)
        if (d.plane[k] >= 32 || planes.base[d.plane[k]] == nullptr) return false;
    switch (d.mask_src) {
    case SVT_HIP_MASK_EXPLICIT: return mask_base != nullptr;
    case SVT_HIP_MASK_WEDGE: {
        if (d.kind != SVT_HIP_BLEND_A64_MASK || wedge_slot(d.bsize) < 0 || d.wedge_index > 15 || d.wedge_sign > 1) return false;
        return ((uint32_t)d.w << d.subw) <= kBw[d.bsize] && ((uint32_t)d.h << d.subh) <= kBh[d.bsize]; // (the mask rows read stay inside this wedge's mask)
    }
    case SVT_HIP_MASK_SMOOTH_II:
        return d.kind == SVT_HIP_BLEND_A64_MASK && d.subw == 0 && d.subh == 0 && d.bsize < 22 && kBw[d.bsize] == d.w && kBh[d.bsize] == d.h && d.ii_mode <= 3;
    default: return d.kind != SVT_HIP_BLEND_A64_MASK && (d.kind == SVT_HIP_BLEND_HMASK ? d.w : d.h) <= 32;
    }
}
// the tiling of interpred.hip: tiles of 2^lw = min(w, 32) columns by th = min(h, 512 >> lw) rows
struct Tiling { int lw, th; uint32_t ntx, nty; };
__device__ __forceinline__ Tiling tiling_of(const uint32_t w, const uint32_t h) {
    Tiling   t;
    uint32_t tw = w < (uint32_t)TILE_W ? w : (uint32_t)TILE_W;
    t.lw = 0;
    while ((1u << (t.lw + 1)) <= tw) t.lw++;
    const uint32_t cap = (uint32_t)TILE_PX >> t.lw;
    t.th  = (int)(h < cap ? h : cap);
    t.ntx = w >> t.lw;
    t.nty = h / (uint32_t)t.th;
    return t;
}
__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int load_px(const uint16_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint16_t*)p; }

// dst may be one of the planes: no __restrict__ on the samples
template <typename PIX>
__global__ __launch_bounds__(TPB) void blend_kernel(const SvtHipBlendPlanes planes, PIX* dst_base, const uint8_t* mask_base, const SvtHipBlendDesc* __restrict__ descs,
                                                    const uint32_t n, uint8_t* __restrict__ status) {
    __shared__ uint32_t pre[DPW + 1]; // exclusive prefix sum of the tile counts
    const int      tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t first = blockIdx.x * DPW;
    if (tid < 64) {
        uint32_t cnt = 0;
        if (tid < DPW && first + tid < n) {
            const SvtHipBlendDesc d  = descs[first + tid];
            const bool            ok = blend_desc_ok(d, planes, mask_base);
            if (ok) {
                const Tiling t = tiling_of(d.w, d.h);
                cnt            = t.ntx * t.nty;
            }
            if (status && blockIdx.y == 0) status[first + tid] = ok ? 0 : 1;
        }
        uint32_t inc = cnt;
#pragma unroll
        for (int s = 1; s < DPW; s <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, s);
            if (tid >= s) inc += o;
        }
        if (tid < DPW) pre[tid + 1] = inc;
        if (tid == 0) pre[0] = 0;
    }
    __syncthreads();
    const uint32_t total = pre[DPW];
    for (uint32_t u = blockIdx.y * WAVES + wv; u < total; u += gridDim.y * WAVES) {
        int di = 0;
#pragma unroll
        for (int s = DPW >> 1; s >= 1; s >>= 1)
            if (pre[di + s] <= u) di += s;
        di = __builtin_amdgcn_readfirstlane(di);
        const SvtHipBlendDesc d = descs[first + di];
        const Tiling   tl = tiling_of(d.w, d.h);
        const int      lw = tl.lw, tw = 1 << lw, th = tl.th, npx = th << lw;
        const int      nj = npx >= 64 ? npx >> 6 : 1;
        const bool     on = l < npx;
        const uint32_t loc = u - pre[di], ntx = tl.ntx, tyi = loc / ntx, txi = loc - tyi * ntx;
        const uint32_t x0 = txi << lw, y0 = tyi * (uint32_t)th;
        const PIX*     s0 = (const PIX*)planes.base[d.plane[0]] + d.src_off[0] + (size_t)y0 * d.src_stride[0] + x0;
        const PIX*     s1 = (const PIX*)planes.base[d.plane[1]] + d.src_off[1] + (size_t)y0 * d.src_stride[1] + x0;
        PIX*           out = dst_base + d.dst_off + (size_t)y0 * d.dst_stride + x0;
        // the mask as bytes in memory (EXPLICIT, WEDGE) or as a rule (SMOOTH_II, OBMC)
        const int      kind = d.kind, msrc = d.mask_src, subw = d.subw, subh = d.subh;
        const bool     bytes = msrc <= SVT_HIP_MASK_WEDGE;
        const uint8_t* mp = mask_base;
        uint32_t       ms = d.mask_stride;
        if (msrc == SVT_HIP_MASK_EXPLICIT) mp = mask_base + d.mask_off;
        else if (msrc == SVT_HIP_MASK_WEDGE) {
            ms = kBw[d.bsize];
            mp = g_wedge + kSlotOff[wedge_slot(d.bsize)] + (uint32_t)(d.wedge_index * 2 + d.wedge_sign) * ms * kBh[d.bsize];
        }
        const int scale = msrc == SVT_HIP_MASK_SMOOTH_II ? kIiScale[d.bsize] : 0, mode = d.ii_mode;
        const int obmc0 = (kind == SVT_HIP_BLEND_HMASK ? d.w : d.h) - 1;
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const uint32_t col = (uint32_t)(i & (tw - 1)), row = (uint32_t)(i >> lw), x = x0 + col, y = y0 + row;
                const int      v0 = load_px(s0 + (row * d.src_stride[0] + col)), v1 = load_px(s1 + (row * d.src_stride[1] + col));
                int            m;
                if (kind == SVT_HIP_BLEND_A64_MASK) {
                    if (bytes) {
                        const uint8_t* q = mp + ((size_t)(y << subh) * ms + (x << subw));
                        m                = load_px(q);
                        if (subw && subh) m = (m + load_px(q + ms) + load_px(q + 1) + load_px(q + ms + 1) + 2) >> 2; // ROUND_POWER_OF_TWO(sum of four, 2)
                        else if (subw) m = (m + load_px(q + 1) + 1) >> 1;                                            // AOM_BLEND_AVG
                        else if (subh) m = (m + load_px(q + ms) + 1) >> 1;
                    } else { // build_smooth_interintra_mask (:2144-2179): II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED
                        const uint32_t k = mode == 1 ? y : (mode == 2 ? x : (y < x ? y : x));
                        m                = mode == 0 ? 32 : kIiWeights[k * (uint32_t)scale];
                    }
                } else {
                    const uint32_t k = kind == SVT_HIP_BLEND_HMASK ? x : y;
                    m                = bytes ? load_px(mp + k) : kObmc[obmc0 + (int)k];
                }
                out[(size_t)row * d.dst_stride + col] = (PIX)((m * v0 + (64 - m) * v1 + 32) >> 6); // AOM_BLEND_A64
            }
        }
    }
}

__global__ __launch_bounds__(TPB) void blend_check_kernel(const SvtHipBlendPlanes planes, const uint8_t* mask_base, const SvtHipBlendDesc* __restrict__ descs,
                                                          const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !blend_desc_ok(descs[i], planes, mask_base);
    if (bad) *bad_out = 1;
}

// ---- the wedge / diff-weighted search ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ int clamp16(const int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ bool search_desc_ok(const SvtHipWedgeSearchDesc& d, const SvtHipBlendPlanes& planes) {
    if (wedge_slot(d.bsize) < 0 || d.fixed_sign > 2) return false;
    return d.src_plane < 32 && d.p0_plane < 32 && d.p1_plane < 32 && planes.base[d.src_plane] && planes.base[d.p0_plane] && planes.base[d.p1_plane];
}

template <typename PIX>
__global__ __launch_bounds__(TPB) void wedge_search_kernel(const SvtHipBlendPlanes planes, const SvtHipWedgeSearchDesc* __restrict__ descs, const uint32_t n,
                                                           const int bd, SvtHipWedgeSearchResult* __restrict__ out, uint8_t* __restrict__ status) {
    const int      l = threadIdx.x & 63;
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (b >= n) return;
    const SvtHipWedgeSearchDesc d  = descs[b];
    const bool                  ok = search_desc_ok(d, planes);
    if (status && l == 0) status[b] = ok ? 0 : 1;
    if (!ok) return;
    const int      slot = wedge_slot(d.bsize), bw = kBw[d.bsize], N = bw * kBh[d.bsize], nj = N >> 6, lbw = bw == 8 ? 3 : (bw == 16 ? 4 : 5);
    const PIX*     src = (const PIX*)planes.base[d.src_plane] + d.src_off;
    const PIX*     p0 = (const PIX*)planes.base[d.p0_plane] + d.p0_off;
    const PIX*     p1 = (const PIX*)planes.base[d.p1_plane] + d.p1_off;
    int      r1[MAX_SEARCH_NPL], d10[MAX_SEARCH_NPL], ds[MAX_SEARCH_NPL], m38[MAX_SEARCH_NPL];
    uint32_t ss0 = 0, ss1 = 0; // a lane's share of sum r0^2, sum r1^2: 16 x 4095^2 < 2^32
#pragma unroll
    for (int j = 0; j < MAX_SEARCH_NPL; j++) {
        r1[j] = d10[j] = ds[j] = m38[j] = 0;
        if (j < nj) {
            const uint32_t i = (uint32_t)(l + 64 * j), x = i & (uint32_t)(bw - 1), y = i >> lbw;
            const int      s = load_px(src + (y * d.src_stride + x)), a = load_px(p0 + (y * d.p0_stride + x)), c = load_px(p1 + (y * d.p1_stride + x));
            const int      r0 = s - a;
            r1[j]  = s - c;
            d10[j] = c - a;
            ds[j]  = clamp16(r0 * r0 - r1[j] * r1[j]); // svt_av1_wedge_compute_delta_squares_c: saturated to int16_t
            ss0 += (uint32_t)(r0 * r0);
            ss1 += (uint32_t)(r1[j] * r1[j]);
            const int m = 38 + (((a > c ? a - c : c - a) >> (bd - 8)) >> 4); // diffwtd_mask / diffwtd_mask_highbd: DIFF_FACTOR 16
            m38[j]      = m > 64 ? 64 : m;
        }
    }
    const int64_t limit = ((int64_t)wave_sum_u64(ss0) - (int64_t)wave_sum_u64(ss1)) * 32; // (1 << WEDGE_WEIGHT_BITS) / 2
    const SVT_HIP_GLOBAL_AS uint8_t* tab = (const SVT_HIP_GLOBAL_AS uint8_t*)g_wedge + kSlotOff[slot];
    SvtHipWedgeSearchResult* o = out + b;
    uint64_t best = ~(uint64_t)0;
    int      best_k = 0, best_sign = 0;
    for (int k = 0; k < 16; k++) {
        int sign = d.fixed_sign - 1;
        if (d.fixed_sign == 0) { // svt_av1_wedge_sign_from_residuals_c on the sign-0 mask
            const SVT_HIP_GLOBAL_AS uint8_t* m0 = tab + (uint32_t)(2 * k) * (uint32_t)N;
            int acc = 0; // a lane's share: 16 x 32768 x 64 < 2^31
#pragma unroll
            for (int j = 0; j < MAX_SEARCH_NPL; j++)
                if (j < nj) acc += ds[j] * (int)m0[l + 64 * j];
            sign = __builtin_amdgcn_readfirstlane((int64_t)wave_sum_u64((uint64_t)(int64_t)acc) > limit ? 1 : 0);
        }
        const SVT_HIP_GLOBAL_AS uint8_t* mk = tab + (uint32_t)(2 * k + sign) * (uint32_t)N;
        uint64_t csse = 0;
#pragma unroll
        for (int j = 0; j < MAX_SEARCH_NPL; j++)
            if (j < nj) {
                const int t = clamp16(64 * r1[j] + (int)mk[l + 64 * j] * d10[j]); // svt_av1_wedge_sse_from_residuals_c: the term is clamped to int16_t
                csse += (uint64_t)(uint32_t)(t * t);
            }
        const uint64_t sse = (wave_sum_u64(csse) + 2048) >> 12; // ROUND_POWER_OF_TWO(., 2 * WEDGE_WEIGHT_BITS)
        if (l == 0) {
            o->sse[k]  = sse;
            o->sign[k] = (uint8_t)sign;
        }
        if (sse < best) best = sse, best_k = k, best_sign = sign; // strict: the first minimum wins (pick_wedge, pick_wedge_fixed_sign)
    }
    uint64_t seg[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; t2++) { // DIFFWTD_38, DIFFWTD_38_INV
        uint64_t csse = 0;
#pragma unroll
        for (int j = 0; j < MAX_SEARCH_NPL; j++)
            if (j < nj) {
                const int t = clamp16(64 * r1[j] + (t2 ? 64 - m38[j] : m38[j]) * d10[j]);
                csse += (uint64_t)(uint32_t)(t * t);
            }
        seg[t2] = (wave_sum_u64(csse) + 2048) >> 12;
    }
    if (l == 0) {
        o->sse_diffwtd[0]   = seg[0];
        o->sse_diffwtd[1]   = seg[1];
        o->best_wedge_index = (uint8_t)best_k;
        o->best_wedge_sign  = (uint8_t)best_sign;
        o->best_mask_type   = (uint8_t)(seg[1] < seg[0] ? 1 : 0); // pick_interinter_seg: strict
        for (int k = 0; k < 5; k++) o->pad[k] = 0;
    }
}
__global__ __launch_bounds__(TPB) void search_check_kernel(const SvtHipBlendPlanes planes, const SvtHipWedgeSearchDesc* __restrict__ descs, const uint32_t n,
                                                           uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !search_desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

// The wedge table of the calling thread's device: generated by the first call that may need it, which waits for the generating launch once (a launch on another stream
// must not see a half-written table).  Later calls only read a flag.
void ensure_wedge_table(hipStream_t st) {
    static std::mutex m;
    static std::atomic<bool> done[svthip::MAX_DEVICES] = {};
    const int         dev = svthip::physical_device(svthip::current_device());
    if (dev < 0 || dev >= svthip::MAX_DEVICES) svthip::device_fail(-1, "wedge table: device number", __FILE__, __LINE__);
    if (done[dev].load(std::memory_order_acquire)) return; // (every call but the first per device: no lock)
    std::lock_guard<std::mutex> g(m);
    if (done[dev].load(std::memory_order_relaxed)) return;
    hipLaunchKernelGGL(wedge_fill_kernel, dim3((WEDGE_BYTES + TPB - 1) / TPB), dim3(TPB), 0, st, 0);
    SVT_LAUNCH_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    done[dev].store(true, std::memory_order_release);
}

} // namespace
namespace svthip {
// for interpred.hip's masked compound: the address of the calling thread's device's table (generated first if need be)
const uint8_t* wedge_table(hipStream_t st) {
    ensure_wedge_table(st);
#ifdef SVT_HIP_EMU
    return g_wedge;
#else
    static std::atomic<const uint8_t*> addr[MAX_DEVICES] = {}; // the symbol's address on each device, asked for once
    const int      dev = physical_device(current_device());    // (in range: ensure_wedge_table checked it)
    const uint8_t* p   = addr[dev].load(std::memory_order_acquire);
    if (!p) {
        void* q = nullptr;
        HIP_CHECK(hipGetSymbolAddress(&q, HIP_SYMBOL(g_wedge)));
        p = (const uint8_t*)q;
        addr[dev].store(p, std::memory_order_release);
    }
    return p;
#endif
}
} // namespace svthip
namespace {

// svt_aom_lowbd_ / highbd_blend_a64_d16_mask_c and svt_av1_build_compound_diffwtd_mask_d16_c as single calls: element-wise over one block of ConvBufType values
template <typename PIX>
__global__ __launch_bounds__(TPB) void d16_blend_kernel(PIX* __restrict__ dst, const uint16_t* __restrict__ s0, const uint16_t* __restrict__ s1,
                                                        const uint8_t* __restrict__ mask, const uint32_t ms, const uint32_t w, const uint32_t h, const int subw,
                                                        const int subh, const int ro, const int rb, const int maxv) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < w * h; i += gridDim.x * TPB) {
        const uint32_t y = i / w, x = i - y * w;
        const uint8_t* q = mask + ((y << subh) * ms + (x << subw));
        int            m = q[0];
        if (subw && subh) m = (m + q[ms] + q[1] + q[ms + 1] + 2) >> 2;
        else if (subw) m = (m + q[1] + 1) >> 1;
        else if (subh) m = (m + q[ms] + 1) >> 1;
        int res = ((m * (int)s0[i] + (64 - m) * (int)s1[i]) >> 6) - ro;
        res     = (res + ((1 << rb) >> 1)) >> rb;
        dst[i]  = (PIX)(res < 0 ? 0 : (res > maxv ? maxv : res));
    }
}
__global__ __launch_bounds__(TPB) void diffwtd_d16_kernel(uint8_t* __restrict__ mask, const int inverse, const uint16_t* __restrict__ s0, const uint16_t* __restrict__ s1,
                                                          const uint32_t n, const int round) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const int a = s0[i], c = s1[i];
        int       v = 38 + ((((a > c ? a - c : c - a) + ((1 << round) >> 1)) >> round) >> 4);
        v           = v > 64 ? 64 : v;
        mask[i]     = (uint8_t)(inverse ? 64 - v : v);
    }
}
// the roundings are shift counts on the device: the range of the jnt_ forms
bool d16_rounds_ok(const SvtHipConvolveParams* cp) {
    return cp && cp->round_0 >= 0 && cp->round_0 <= 7 && cp->round_1 >= 0 && cp->round_1 <= 7 && cp->round_0 + cp->round_1 <= 14;
}
bool d16_dim_ok(const int v) { return v >= 4 && v <= 128 && (v & (v - 1)) == 0; }
template <typename PIX>
void d16_blend_host(PIX* dst, const uint32_t dst_stride, const uint16_t* src0, const uint32_t stride0, const uint16_t* src1, const uint32_t stride1, const uint8_t* mask,
                    const uint32_t mask_stride, const int w, const int h, const int subw, const int subh, const SvtHipConvolveParams* cp, const int bd) {
    if (!dst || !src0 || !src1 || !mask || !d16_dim_ok(w) || !d16_dim_ok(h) || subw < 0 || subw > 1 || subh < 0 || subh > 1 || !d16_rounds_ok(cp)) return; // nothing is written
    if (bd != 8 && bd != 10 && bd != 12) return;
    const size_t blk = (size_t)w * h, mw = (size_t)w << subw, mh = (size_t)h << subh;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = blk * (4 + sizeof(PIX)) + mw * mh + 2048;
    c.reserve(bytes, bytes);
    uint16_t* d0 = (uint16_t*)c.dalloc(blk * 2);
    uint16_t* d1 = (uint16_t*)c.dalloc(blk * 2);
    PIX*      dd = (PIX*)c.dalloc(blk * sizeof(PIX));
    uint8_t*  dm = (uint8_t*)c.dalloc(mw * mh);
    c.up2d(d0, (size_t)w * 2, src0, (size_t)stride0 * 2, (size_t)w * 2, h);
    c.up2d(d1, (size_t)w * 2, src1, (size_t)stride1 * 2, (size_t)w * 2, h);
    c.up2d(dm, mw, mask, mask_stride, mw, mh);
    const int ob = bd + 14 - cp->round_0, ro = (1 << (ob - cp->round_1)) + (1 << (ob - cp->round_1 - 1)), rb = 14 - cp->round_0 - cp->round_1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(d16_blend_kernel<PIX>), dim3((unsigned)((blk + TPB - 1) / TPB)), dim3(TPB), 0, c.stream, dd, (const uint16_t*)d0, (const uint16_t*)d1,
                       (const uint8_t*)dm, (uint32_t)mw, (uint32_t)w, (uint32_t)h, subw, subh, ro, rb, (1 << bd) - 1);
    SVT_LAUNCH_CHECK();
    c.down2d(dst, (size_t)dst_stride * sizeof(PIX), dd, (size_t)w * sizeof(PIX), (size_t)w * sizeof(PIX), h);
}
void diffwtd_d16_host(uint8_t* mask, const int mask_type, const uint16_t* src0, const int stride0, const uint16_t* src1, const int stride1, const int h, const int w,
                      const SvtHipConvolveParams* cp, const int bd) {
    if (!mask || !src0 || !src1 || mask_type < 0 || mask_type > 1 || w < 1 || h < 1 || w > 128 || h > 128 || stride0 < w || stride1 < w || !d16_rounds_ok(cp)) return;
    if (bd != 8 && bd != 10 && bd != 12) return;
    const size_t blk = (size_t)w * h;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    c.reserve(blk * 5 + 2048, blk * 5 + 2048);
    uint16_t* d0 = (uint16_t*)c.dalloc(blk * 2);
    uint16_t* d1 = (uint16_t*)c.dalloc(blk * 2);
    uint8_t*  dm = (uint8_t*)c.dalloc(blk);
    c.up2d(d0, (size_t)w * 2, src0, (size_t)stride0 * 2, (size_t)w * 2, h);
    c.up2d(d1, (size_t)w * 2, src1, (size_t)stride1 * 2, (size_t)w * 2, h);
    hipLaunchKernelGGL(diffwtd_d16_kernel, dim3((unsigned)((blk + TPB - 1) / TPB)), dim3(TPB), 0, c.stream, dm, mask_type, (const uint16_t*)d0, (const uint16_t*)d1,
                       (uint32_t)blk, 14 - cp->round_0 - cp->round_1 + bd - 8);
    SVT_LAUNCH_CHECK();
    c.down(mask, dm, blk);
}

// descriptors the host cannot read: one word says whether any is invalid (the contract of svt_hip_inter_pred_batch)
template <typename F> bool any_invalid(const uint32_t n, hipStream_t st, F&& launch_check) {
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    c.reserve(0, 256);
    uint32_t* bad = (uint32_t*)c.palloc(64);
    *bad          = 0;
    launch_check(dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), bad);
    SVT_LAUNCH_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    return *(volatile uint32_t*)bad != 0;
}

// ---- the single-call forms --------------------------------------------------------------------------------------------------------------------------
// One block from host memory: the two w x h sources and exactly the mask bytes the C reads go into the call's arena with one descriptor; one synchronisation (the
// download); nothing of the caller's is written before it, so dst may be one of the sources.
template <typename PIX>
void blend_host(PIX* dst, const uint32_t dst_stride, const PIX* src0, const uint32_t src0_stride, const PIX* src1, const uint32_t src1_stride, const uint8_t* mask,
                const uint32_t mask_stride, const int w, const int h, const int subw, const int subh, const int kind, const int bd) {
    if (w < 1 || h < 1 || w > 128 || h > 128 || (w & (w - 1)) || (h & (h - 1)) || subw < 0 || subw > 1 || subh < 0 || subh > 1) return; // nothing is written
    if (!dst || !src0 || !src1 || !mask) return;
    if (sizeof(PIX) == 2 && bd != 8 && bd != 10 && bd != 12) return;
    const size_t mw = kind == SVT_HIP_BLEND_VMASK ? (size_t)h : (size_t)w << (kind == SVT_HIP_BLEND_A64_MASK ? subw : 0);
    const size_t mh = kind == SVT_HIP_BLEND_A64_MASK ? (size_t)h << subh : 1;
    const size_t px = sizeof(PIX), blk = (size_t)w * h * px;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = 3 * blk + mw * mh + sizeof(SvtHipBlendDesc) + 2048;
    c.reserve(bytes, bytes);
    PIX*             d0 = (PIX*)c.dalloc(blk);
    PIX*             d1 = (PIX*)c.dalloc(blk);
    PIX*             dd = (PIX*)c.dalloc(blk);
    uint8_t*         dm = (uint8_t*)c.dalloc(mw * mh);
    SvtHipBlendDesc* dv = (SvtHipBlendDesc*)c.dalloc(sizeof(SvtHipBlendDesc));
    c.up2d(d0, (size_t)w * px, src0, (size_t)src0_stride * px, (size_t)w * px, h);
    c.up2d(d1, (size_t)w * px, src1, (size_t)src1_stride * px, (size_t)w * px, h);
    c.up2d(dm, mw, mask, mask_stride, mw, mh);
    SvtHipBlendDesc d{};
    d.src_stride[0] = d.src_stride[1] = d.dst_stride = (uint32_t)w;
    d.mask_stride   = (uint32_t)mw;
    d.plane[1]      = 1;
    d.w             = (uint8_t)w;
    d.h             = (uint8_t)h;
    d.kind          = (uint8_t)kind;
    d.mask_src      = SVT_HIP_MASK_EXPLICIT;
    d.subw          = (uint8_t)(kind == SVT_HIP_BLEND_A64_MASK ? subw : 0);
    d.subh          = (uint8_t)(kind == SVT_HIP_BLEND_A64_MASK ? subh : 0);
    c.up(dv, &d, sizeof(d));
    SvtHipBlendPlanes planes{};
    planes.base[0] = d0;
    planes.base[1] = d1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_kernel<PIX>), dim3(1, 1), dim3(TPB), 0, c.stream, planes, dd, (const uint8_t*)dm, (const SvtHipBlendDesc*)dv, 1u, (uint8_t*)nullptr);
    SVT_LAUNCH_CHECK();
    c.down2d(dst, (size_t)dst_stride * px, dd, (size_t)w * px, (size_t)w * px, h);
}

// ---- the residual-domain helpers and the pixel-domain diff-weighted builders as single calls ----------------------------------------------------------
// One workgroup walks the N elements; the two sums are 64-bit per lane, a butterfly per wave, the four wave totals through LDS.  op: 0 wedge_sse_from_residuals
// (a = r1, b = d, m), 1 wedge_sign_from_residuals (a = ds, m, limit), 2 sum_squares_i16 (a), 3 wedge_compute_delta_squares (a, b -> dst).
enum { OP_SSE = 0, OP_SIGN = 1, OP_SUMSQ = 2, OP_DELTA = 3 };
__global__ __launch_bounds__(TPB) void wedge_helper_kernel(const int op, const int16_t* __restrict__ a, const int16_t* __restrict__ b, const uint8_t* __restrict__ m,
                                                           const uint32_t n, const int64_t limit, int16_t* __restrict__ dst, uint64_t* __restrict__ out) {
    __shared__ uint64_t part[WAVES];
    const int tid = threadIdx.x;
    uint64_t  acc = 0;
    for (uint32_t i = (uint32_t)tid; i < n; i += TPB) {
        if (op == OP_SSE) {
            const int t = clamp16(64 * (int)a[i] + (int)m[i] * (int)b[i]);
            acc += (uint64_t)(uint32_t)(t * t);
        } else if (op == OP_SIGN) acc += (uint64_t)(int64_t)((int)a[i] * (int)m[i]);
        else if (op == OP_SUMSQ) acc += (uint64_t)(uint32_t)((int)a[i] * (int)a[i]);
        else dst[i] = (int16_t)clamp16((int)a[i] * (int)a[i] - (int)b[i] * (int)b[i]);
    }
    if (op == OP_DELTA) return; // (uniform: no barrier is skipped by part of the workgroup)
    acc = wave_sum_u64(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0;
        for (int k = 0; k < WAVES; k++) t += part[k];
        out[0] = op == OP_SSE ? (t + 2048) >> 12 : (op == OP_SIGN ? (uint64_t)((int64_t)t > limit ? 1 : 0) : t);
    }
}
// svt_av1_build_compound_diffwtd_mask_c / _highbd_c: mask[i * w + j] from two strided blocks
template <typename PIX>
__global__ __launch_bounds__(TPB) void diffwtd_kernel(uint8_t* __restrict__ mask, const int inverse, const PIX* __restrict__ s0, const uint32_t stride0,
                                                      const PIX* __restrict__ s1, const uint32_t stride1, const uint32_t h, const uint32_t w, const int shift) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < w * h; i += gridDim.x * TPB) {
        const uint32_t y = i / w, x = i - y * w;
        const int      a = (int)s0[y * stride0 + x], c = (int)s1[y * stride1 + x];
        int            v = 38 + (((a > c ? a - c : c - a) >> shift) >> 4);
        v                = v > 64 ? 64 : v;
        mask[i]          = (uint8_t)(inverse ? 64 - v : v);
    }
}
constexpr uint32_t HELPER_MAX_N = 1u << 20; // elements one helper call accepts (MAX_SB_SQUARE is 2^14)

uint64_t wedge_helper_host(const int op, const int16_t* a, const int16_t* b, const uint8_t* m, const int64_t n64, const int64_t limit, int16_t* dst) {
    if (n64 < 1 || n64 > (int64_t)HELPER_MAX_N || !a || (op == OP_SSE && (!b || !m)) || (op == OP_SIGN && !m) || (op == OP_DELTA && (!b || !dst))) return 0;
    const uint32_t    n = (uint32_t)n64;
    svthip::HostCall& c = svthip::host_call();
    if (n <= 4096) c.begin_small();
    else c.begin();
    const size_t bytes = (size_t)n * 7 + 4096;
    c.reserve(bytes, bytes);
    int16_t*  da = (int16_t*)c.dalloc((size_t)n * 2);
    int16_t*  db = (int16_t*)c.dalloc((size_t)n * 2);
    int16_t*  dd = (int16_t*)c.dalloc((size_t)n * 2);
    uint8_t*  dm = (uint8_t*)c.dalloc(n);
    uint64_t* dout = (uint64_t*)c.dalloc(8);
    c.up(da, a, (size_t)n * 2);
    if (op == OP_SSE || op == OP_DELTA) c.up(db, b, (size_t)n * 2);
    if (op == OP_SSE || op == OP_SIGN) c.up(dm, m, n);
    hipLaunchKernelGGL(wedge_helper_kernel, dim3(1), dim3(TPB), 0, c.stream, op, (const int16_t*)da, (const int16_t*)db, (const uint8_t*)dm, n, limit, dd, dout);
    SVT_LAUNCH_CHECK();
    uint64_t r = 0;
    if (op == OP_DELTA) c.down(dst, dd, (size_t)n * 2); // (dst may be a: the upload came first)
    else c.down(&r, dout, 8);
    return r;
}
template <typename PIX>
void diffwtd_host(uint8_t* mask, const int mask_type, const PIX* src0, const int stride0, const PIX* src1, const int stride1, const int h, const int w, const int bd) {
    if (!mask || !src0 || !src1 || mask_type < 0 || mask_type > 1 || w < 1 || h < 1 || w > 128 || h > 128 || stride0 < w || stride1 < w) return; // nothing is written
    if (bd != 8 && bd != 10 && bd != 12) return;
    const size_t px = sizeof(PIX), blk = (size_t)w * h;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = blk * (2 * px + 1) + 2048;
    c.reserve(bytes, bytes);
    PIX*     d0 = (PIX*)c.dalloc(blk * px);
    PIX*     d1 = (PIX*)c.dalloc(blk * px);
    uint8_t* dm = (uint8_t*)c.dalloc(blk);
    c.up2d(d0, (size_t)w * px, src0, (size_t)stride0 * px, (size_t)w * px, h);
    c.up2d(d1, (size_t)w * px, src1, (size_t)stride1 * px, (size_t)w * px, h);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(diffwtd_kernel<PIX>), dim3((unsigned)((blk + TPB - 1) / TPB)), dim3(TPB), 0, c.stream, dm, mask_type, (const PIX*)d0, (uint32_t)w,
                       (const PIX*)d1, (uint32_t)w, (uint32_t)h, (uint32_t)w, bd - 8);
    SVT_LAUNCH_CHECK();
    c.down(mask, dm, blk);
}

} // namespace

extern "C" {

int svt_hip_maskpred_prepare(void* stream) {
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    ensure_wedge_table((hipStream_t)stream);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_blend_batch(SvtHipBlendPlanes planes, void* dst_base, const uint8_t* mask_base, const SvtHipBlendDesc* descs, uint32_t n, int bit_depth, uint8_t* status,
                        void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!dst_base || !descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    ensure_wedge_table(st);
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(blend_check_kernel, grid, dim3(TPB), 0, st, planes, mask_base, descs, n, bad); }))
        return -1;
    const dim3 grid((n + DPW - 1) / DPW, SPLIT), block(TPB);
    if (bit_depth > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_kernel<uint16_t>), grid, block, 0, st, planes, (uint16_t*)dst_base, mask_base, descs, n, status);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_kernel<uint8_t>), grid, block, 0, st, planes, (uint8_t*)dst_base, mask_base, descs, n, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_wedge_search_batch(SvtHipBlendPlanes planes, const SvtHipWedgeSearchDesc* descs, uint32_t n, int bit_depth, SvtHipWedgeSearchResult* out, uint8_t* status,
                               void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!descs || !out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    ensure_wedge_table(st);
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(search_check_kernel, grid, dim3(TPB), 0, st, planes, descs, n, bad); })) return -1;
    const dim3 grid((n + WAVES - 1) / WAVES), block(TPB);
    if (bit_depth > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(wedge_search_kernel<uint16_t>), grid, block, 0, st, planes, descs, n, bit_depth, out, status);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(wedge_search_kernel<uint8_t>), grid, block, 0, st, planes, descs, n, bit_depth, out, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

#define SVT_HIP_BLEND_FORM(call)                 \
    if (svthip::failed()) return;                \
    try {                                        \
        call;                                    \
    } catch (const svthip::DeviceError&) {}
void svt_aom_blend_a64_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0, uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride, const uint8_t* mask,
                                uint32_t mask_stride, int w, int h, int subx, int suby) {
    SVT_HIP_BLEND_FORM(blend_host<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subx, suby, SVT_HIP_BLEND_A64_MASK, 8))
}
void svt_aom_highbd_blend_a64_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0, uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride,
                                       const uint8_t* mask, uint32_t mask_stride, int w, int h, int subx, int suby, int bd) {
    SVT_HIP_BLEND_FORM(blend_host<uint16_t>((uint16_t*)dst, dst_stride, (const uint16_t*)src0, src0_stride, (const uint16_t*)src1, src1_stride, mask, mask_stride, w, h, subx,
                                            suby, SVT_HIP_BLEND_A64_MASK, bd))
}
void svt_aom_blend_a64_hmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0, uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride, const uint8_t* mask,
                                 int w, int h) {
    SVT_HIP_BLEND_FORM(blend_host<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w, h, 0, 0, SVT_HIP_BLEND_HMASK, 8))
}
void svt_aom_blend_a64_vmask_hip(uint8_t* dst, uint32_t dst_stride, const uint8_t* src0, uint32_t src0_stride, const uint8_t* src1, uint32_t src1_stride, const uint8_t* mask,
                                 int w, int h) {
    SVT_HIP_BLEND_FORM(blend_host<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w, h, 0, 0, SVT_HIP_BLEND_VMASK, 8))
}
void svt_aom_highbd_blend_a64_hmask_16bit_hip(uint16_t* dst, uint32_t dst_stride, const uint16_t* src0, uint32_t src0_stride, const uint16_t* src1, uint32_t src1_stride,
                                              const uint8_t* mask, int w, int h, int bd) {
    SVT_HIP_BLEND_FORM(blend_host<uint16_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w, h, 0, 0, SVT_HIP_BLEND_HMASK, bd))
}
void svt_aom_highbd_blend_a64_vmask_16bit_hip(uint16_t* dst, uint32_t dst_stride, const uint16_t* src0, uint32_t src0_stride, const uint16_t* src1, uint32_t src1_stride,
                                              const uint8_t* mask, int w, int h, int bd) {
    SVT_HIP_BLEND_FORM(blend_host<uint16_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, 0, w, h, 0, 0, SVT_HIP_BLEND_VMASK, bd))
}

uint64_t svt_av1_wedge_sse_from_residuals_hip(const int16_t* r1, const int16_t* d, const uint8_t* m, int N) {
    if (svthip::failed()) return 0;
    try {
        return wedge_helper_host(OP_SSE, r1, d, m, N, 0, nullptr);
    } catch (const svthip::DeviceError&) { return 0; }
}
int8_t svt_av1_wedge_sign_from_residuals_hip(const int16_t* ds, const uint8_t* m, int N, int64_t limit) {
    if (svthip::failed()) return 0;
    try {
        return (int8_t)wedge_helper_host(OP_SIGN, ds, nullptr, m, N, limit, nullptr);
    } catch (const svthip::DeviceError&) { return 0; }
}
void svt_av1_wedge_compute_delta_squares_hip(int16_t* d, const int16_t* a, const int16_t* b, int N) {
    SVT_HIP_BLEND_FORM((void)wedge_helper_host(OP_DELTA, a, b, nullptr, N, 0, d))
}
uint64_t svt_aom_sum_squares_i16_hip(const int16_t* src, uint32_t N) {
    if (svthip::failed()) return 0;
    try {
        return wedge_helper_host(OP_SUMSQ, src, nullptr, nullptr, N, 0, nullptr);
    } catch (const svthip::DeviceError&) { return 0; }
}
void svt_av1_build_compound_diffwtd_mask_hip(uint8_t* mask, uint8_t mask_type, const uint8_t* src0, int src0_stride, const uint8_t* src1, int src1_stride, int h, int w) {
    SVT_HIP_BLEND_FORM(diffwtd_host<uint8_t>(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w, 8))
}
void svt_av1_build_compound_diffwtd_mask_highbd_hip(uint8_t* mask, uint8_t mask_type, const uint8_t* src0, int src0_stride, const uint8_t* src1, int src1_stride, int h,
                                                    int w, int bd) {
    SVT_HIP_BLEND_FORM(diffwtd_host<uint16_t>(mask, mask_type, (const uint16_t*)src0, src0_stride, (const uint16_t*)src1, src1_stride, h, w, bd))
}
void svt_aom_lowbd_blend_a64_d16_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint16_t* src0, uint32_t src0_stride, const uint16_t* src1, uint32_t src1_stride,
                                          const uint8_t* mask, uint32_t mask_stride, int w, int h, int subw, int subh, SvtHipConvolveParams* conv_params) {
    SVT_HIP_BLEND_FORM(d16_blend_host<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subw, subh, conv_params, 8))
}
void svt_aom_highbd_blend_a64_d16_mask_hip(uint8_t* dst, uint32_t dst_stride, const uint16_t* src0, uint32_t src0_stride, const uint16_t* src1, uint32_t src1_stride,
                                           const uint8_t* mask, uint32_t mask_stride, int w, int h, int subx, int suby, SvtHipConvolveParams* conv_params, const int bd) {
    SVT_HIP_BLEND_FORM(d16_blend_host<uint16_t>((uint16_t*)dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subx, suby, conv_params, bd))
}
void svt_av1_build_compound_diffwtd_mask_d16_hip(uint8_t* mask, uint8_t mask_type, const uint16_t* src0, int src0_stride, const uint16_t* src1, int src1_stride, int h,
                                                 int w, SvtHipConvolveParams* conv_params, int bd) {
    SVT_HIP_BLEND_FORM(diffwtd_d16_host(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w, conv_params, bd))
}
#undef SVT_HIP_BLEND_FORM

} // extern "C"
