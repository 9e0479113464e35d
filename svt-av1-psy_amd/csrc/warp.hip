// warp.hip -- AV1 warped motion for gfx950: the block warp filter, the local-warp model fit and the global-motion warp error.  DESIGN.md 4.23 has the layout, the
// literal narrowings and the bounds.
//
//  * the tables: the 193 x 8 warp filter (AV1 specification, block warp process, Warped_Filters) is kept as its two distinct 64-row thirds -- the [1, 2) third is the
//    [-1, 0) third moved up by two taps, except its first row -- and expanded at compile time into the two packings the kernels read per lane: four dwords of int16
//    pairs (v_dot2_i32_i16) and two dwords of int8 (v_dot4_i32_i8; every tap lies in -22 .. 127 and every row sums to 128, both checked at compile time).  The 257-entry
//    divisor table of the model fit is generated: round(2^22 / (256 + n)).
//  * warp_pred_kernel: one launch, n descriptors of mixed sizes, svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c (warped_motion.c:569, :714) bit for bit.  Flattened
//    like inter_pred_kernel: a workgroup takes 16 descriptors, a prefix sum of their 8x8 tile counts, ONE WAVE per tile.  The tile's ix4 / iy4 / sx4 / sy4 are
//    wave-uniform; the horizontal stage makes the 15 x 8 intermediate values in two rounds of the wave (8 lanes idle in the second), each lane with its own table row and
//    its own eight clamped samples -- one unaligned 8-sample load when the tile's 15 columns lie inside the picture (a wave-uniform branch), eight clamped loads
//    otherwise -- and leaves them in the wave's LDS slice as 16-bit values, column-major, so that the vertical stage reads a lane's eight values as five dwords.
//    With two references the first one's ConvBufType value stays in a register while the second is filtered.
//  * warp_error_kernel: the same tile routine over the 32 x 32 error blocks of a picture, the absolute differences against the source summed per wave and added to
//    out[i] with one 64-bit atomic per wave (integer sums: the result does not depend on the order).
//  * warp_model_kernel: find_affine_int + svt_get_shear_params (warped_motion.c:365, :898), one lane per block, plain integer arithmetic.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include "maskpred_tables.h"
#include <algorithm>
#include <vector>

namespace {
using svt_maskpred::kBh; // block_size_wide / block_size_high
using svt_maskpred::kBw;

constexpr int DPW   = 16;  // descriptors per workgroup group
constexpr int TPB   = 256; // threads per workgroup
constexpr int WAVES = TPB / 64;
constexpr int SPLIT = 4;   // workgroups (blockIdx.y) that share one descriptor group's tile list
constexpr int ERR_WG = 512; // workgroups of one warp-error launch, shared among its candidates (at most 256 and at least 16 each)

// ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
// Warped_Filters rows 0 .. 63, fractional positions [-1, 0): taps 0 .. 5 (taps 6 and 7 are 0)
constexpr int8_t kWarpLo[64][6] = {
    {0, 0, 127, 1, 0, 0},      {0, -1, 127, 2, 0, 0},     {1, -3, 127, 4, -1, 0},    {1, -4, 126, 6, -2, 1},    {1, -5, 126, 8, -3, 1},    {1, -6, 125, 11, -4, 1},
    {1, -7, 124, 13, -4, 1},   {2, -8, 123, 15, -5, 1},   {2, -9, 122, 18, -6, 1},   {2, -10, 121, 20, -6, 1},  {2, -11, 120, 22, -7, 2},  {2, -12, 119, 25, -8, 2},
    {3, -13, 117, 27, -8, 2},  {3, -13, 116, 29, -9, 2},  {3, -14, 114, 32, -10, 3}, {3, -15, 113, 35, -10, 2}, {3, -15, 111, 37, -11, 3}, {3, -16, 109, 40, -11, 3},
    {3, -16, 108, 42, -12, 3}, {4, -17, 106, 45, -13, 3}, {4, -17, 104, 47, -13, 3}, {4, -17, 102, 50, -14, 3}, {4, -17, 100, 52, -14, 3}, {4, -18, 98, 55, -15, 4},
    {4, -18, 96, 58, -15, 3},  {4, -18, 94, 60, -16, 4},  {4, -18, 91, 63, -16, 4},  {4, -18, 89, 65, -16, 4},  {4, -18, 87, 68, -17, 4},  {4, -18, 85, 70, -17, 4},
    {4, -18, 82, 73, -17, 4},  {4, -18, 80, 75, -17, 4},  {4, -18, 78, 78, -18, 4},  {4, -17, 75, 80, -18, 4},  {4, -17, 73, 82, -18, 4},  {4, -17, 70, 85, -18, 4},
    {4, -17, 68, 87, -18, 4},  {4, -16, 65, 89, -18, 4},  {4, -16, 63, 91, -18, 4},  {4, -16, 60, 94, -18, 4},  {3, -15, 58, 96, -18, 4},  {4, -15, 55, 98, -18, 4},
    {3, -14, 52, 100, -17, 4}, {3, -14, 50, 102, -17, 4}, {3, -13, 47, 104, -17, 4}, {3, -13, 45, 106, -17, 4}, {3, -12, 42, 108, -16, 3}, {3, -11, 40, 109, -16, 3},
    {3, -11, 37, 111, -15, 3}, {2, -10, 35, 113, -15, 3}, {3, -10, 32, 114, -14, 3}, {2, -9, 29, 116, -13, 3},  {2, -8, 27, 117, -13, 3},  {2, -8, 25, 119, -12, 2},
    {2, -7, 22, 120, -11, 2},  {1, -6, 20, 121, -10, 2},  {1, -6, 18, 122, -9, 2},   {1, -5, 15, 123, -8, 2},   {1, -4, 13, 124, -7, 1},   {1, -4, 11, 125, -6, 1},
    {1, -3, 8, 126, -5, 1},    {1, -2, 6, 126, -4, 1},    {0, -1, 4, 127, -3, 1},    {0, 0, 2, 127, -1, 0}};
// rows 64 .. 127, fractional positions [0, 1)
constexpr int8_t kWarpMid[64][8] = {
    {0, 0, 0, 127, 1, 0, 0, 0},         {0, 0, -1, 127, 2, 0, 0, 0},        {0, 1, -3, 127, 4, -2, 1, 0},       {0, 1, -5, 127, 6, -2, 1, 0},
    {0, 2, -6, 126, 8, -3, 1, 0},       {-1, 2, -7, 126, 11, -4, 2, -1},    {-1, 3, -8, 125, 13, -5, 2, -1},    {-1, 3, -10, 124, 16, -6, 3, -1},
    {-1, 4, -11, 123, 18, -7, 3, -1},   {-1, 4, -12, 122, 20, -7, 3, -1},   {-1, 4, -13, 121, 23, -8, 3, -1},   {-2, 5, -14, 120, 25, -9, 4, -1},
    {-1, 5, -15, 119, 27, -10, 4, -1},  {-1, 5, -16, 118, 30, -11, 4, -1},  {-2, 6, -17, 116, 33, -12, 5, -1},  {-2, 6, -17, 114, 35, -12, 5, -1},
    {-2, 6, -18, 113, 38, -13, 5, -1},  {-2, 7, -19, 111, 41, -14, 6, -2},  {-2, 7, -19, 110, 43, -15, 6, -2},  {-2, 7, -20, 108, 46, -15, 6, -2},
    {-2, 7, -20, 106, 49, -16, 6, -2},  {-2, 7, -21, 104, 51, -16, 7, -2},  {-2, 7, -21, 102, 54, -17, 7, -2},  {-2, 8, -21, 100, 56, -18, 7, -2},
    {-2, 8, -22, 98, 59, -18, 7, -2},   {-2, 8, -22, 96, 62, -19, 7, -2},   {-2, 8, -22, 94, 64, -19, 7, -2},   {-2, 8, -22, 91, 67, -20, 8, -2},
    {-2, 8, -22, 89, 69, -20, 8, -2},   {-2, 8, -22, 87, 72, -21, 8, -2},   {-2, 8, -21, 84, 74, -21, 8, -2},   {-2, 8, -22, 82, 77, -21, 8, -2},
    {-2, 8, -21, 79, 79, -21, 8, -2},   {-2, 8, -21, 77, 82, -22, 8, -2},   {-2, 8, -21, 74, 84, -21, 8, -2},   {-2, 8, -21, 72, 87, -22, 8, -2},
    {-2, 8, -20, 69, 89, -22, 8, -2},   {-2, 8, -20, 67, 91, -22, 8, -2},   {-2, 7, -19, 64, 94, -22, 8, -2},   {-2, 7, -19, 62, 96, -22, 8, -2},
    {-2, 7, -18, 59, 98, -22, 8, -2},   {-2, 7, -18, 56, 100, -21, 8, -2},  {-2, 7, -17, 54, 102, -21, 7, -2},  {-2, 7, -16, 51, 104, -21, 7, -2},
    {-2, 6, -16, 49, 106, -20, 7, -2},  {-2, 6, -15, 46, 108, -20, 7, -2},  {-2, 6, -15, 43, 110, -19, 7, -2},  {-2, 6, -14, 41, 111, -19, 7, -2},
    {-1, 5, -13, 38, 113, -18, 6, -2},  {-1, 5, -12, 35, 114, -17, 6, -2},  {-1, 5, -12, 33, 116, -17, 6, -2},  {-1, 4, -11, 30, 118, -16, 5, -1},
    {-1, 4, -10, 27, 119, -15, 5, -1},  {-1, 4, -9, 25, 120, -14, 5, -2},   {-1, 3, -8, 23, 121, -13, 4, -1},   {-1, 3, -7, 20, 122, -12, 4, -1},
    {-1, 3, -7, 18, 123, -11, 4, -1},   {-1, 3, -6, 16, 124, -10, 3, -1},   {-1, 2, -5, 13, 125, -8, 3, -1},    {-1, 2, -4, 11, 126, -7, 2, -1},
    {0, 1, -3, 8, 126, -6, 2, 0},       {0, 1, -2, 6, 127, -5, 1, 0},       {0, 1, -2, 4, 127, -3, 1, 0},       {0, 0, 0, 2, 127, -1, 0, 0}};
constexpr int kWarpRow128[8] = {0, 0, 0, 1, 127, 0, 0, 0}; // the one row of [1, 2) that is not its [-1, 0) counterpart moved up by two taps

constexpr int warp_tap(const int row, const int m) {
    if (row < 64) return m < 6 ? kWarpLo[row][m] : 0;
    if (row < 128) return kWarpMid[row - 64][m];
    if (row == 128) return kWarpRow128[m];
    const int r = row == 192 ? 63 : row - 128; // row 192 repeats row 191
    return m >= 2 ? kWarpLo[r][m - 2] : 0;
}
struct alignas(16) WarpTabs {
    uint32_t h2[193][4]; // taps 2k, 2k + 1 as int16 pairs
    uint32_t b4[193][2]; // taps 4k .. 4k + 3 as int8
    uint16_t div[257];   // div_lut (warped_motion.c:298)
    bool     ok;         // every tap in -128 .. 127, every row sums to 128
};
constexpr WarpTabs make_warp_tabs() {
    WarpTabs t{};
    t.ok = true;
    for (int r = 0; r < 193; r++) {
        int sum = 0;
        for (int m = 0; m < 8; m++) {
            const int v = warp_tap(r, m);
            sum += v;
            t.ok = t.ok && v >= -128 && v <= 127;
            t.h2[r][m >> 1] |= (uint32_t)(uint16_t)(int16_t)v << (16 * (m & 1));
            t.b4[r][m >> 2] |= (uint32_t)(uint8_t)(int8_t)v << (8 * (m & 3));
        }
        t.ok = t.ok && sum == 128;
    }
    for (int n = 0; n <= 256; n++) t.div[n] = (uint16_t)(((1 << 22) + (256 + n) / 2) / (256 + n));
    return t;
}
__device__ constexpr WarpTabs kTabs = make_warp_tabs();
static_assert(make_warp_tabs().ok, "the 8-bit horizontal stage relies on int8 taps that sum to 128");

typedef uint32_t u32x4 __attribute__((vector_size(16)));
typedef uint32_t u32x2 __attribute__((vector_size(8)));
typedef uint32_t u32_alias __attribute__((may_alias));
typedef int16_t  i16_alias __attribute__((may_alias));

__device__ __forceinline__ int rpot(const int v, const int n) { return (v + ((1 << n) >> 1)) >> n; } // ROUND_POWER_OF_TWO (definitions.h:459), n >= 0
__device__ __forceinline__ int sdot2(const uint32_t a, const uint32_t b, const int c) {              // v_dot2_i32_i16
    typedef short s2 __attribute__((ext_vector_type(2)));
    s2 x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return __builtin_amdgcn_sdot2(x, y, c, false);
}
__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int load_px(const uint16_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint16_t*)p; }
// the table row of a shear position: ROUND_POWER_OF_TWO(s, WARPEDDIFF_PREC_BITS) + WARPEDPIXEL_PREC_SHIFTS; is_affine_shear_allowed keeps it inside 0 .. 192, the clamp
// only keeps a descriptor the check kernel has not seen from reading outside the table
__device__ __forceinline__ int warp_row(const int s) { return clampi(((s + 512) >> 10) + 64, 0, 192); }

// sum over the eight taps of table row `offs` of tap * sample for the samples at columns clamp(ix + m, 0, wm1), m = 0 .. 7, of `row`, plus 1 << (bd + FILTER_BITS - 1)
__device__ __forceinline__ int warp_hsum(const uint8_t* row, const int ix, const int wm1, const bool interior, const int offs, const int bd) {
    uint32_t v0, v1;
    if (interior) {
        const svt_u32x2_a1 v = svt_hip_global_load_x2(row + ix);
        v0 = v[0], v1 = v[1];
    } else {
        v0 = v1 = 0;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            v0 |= (uint32_t)load_px(row + clampi(ix + m, 0, wm1)) << (8 * m);
            v1 |= (uint32_t)load_px(row + clampi(ix + m + 4, 0, wm1)) << (8 * m);
        }
    }
    const u32x2 t = *(const SVT_HIP_GLOBAL_AS u32x2*)&kTabs.b4[offs][0];
    // sample - 128 as a signed byte: the 128 * 128 of the taps' sum comes back with the offset
    return __builtin_amdgcn_sdot4((int)(v0 ^ 0x80808080u), (int)t[0], __builtin_amdgcn_sdot4((int)(v1 ^ 0x80808080u), (int)t[1], 16384 + (1 << 14), false), false);
}
__device__ __forceinline__ int warp_hsum(const uint16_t* row, const int ix, const int wm1, const bool interior, const int offs, const int bd) {
    uint32_t v[4];
    if (interior) {
        const svt_u32x4_a2 q = svt_hip_global_load_x4(row + ix);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
    } else {
#pragma unroll
        for (int m = 0; m < 4; m++)
            v[m] = (uint32_t)load_px(row + clampi(ix + 2 * m, 0, wm1)) | ((uint32_t)load_px(row + clampi(ix + 2 * m + 1, 0, wm1)) << 16);
    }
    const u32x4 t = *(const SVT_HIP_GLOBAL_AS u32x4*)&kTabs.h2[offs][0];
    return sdot2(v[0], t[0], sdot2(v[1], t[1], sdot2(v[2], t[2], sdot2(v[3], t[3], 1 << (bd + 6)))));
}

// One reference of one 8x8 tile whose top-left output sample is (j, i) of the block's plane: the vertical filter's sum for the lane's sample (row l >> 3, column l & 7),
// the 1 << offset_bits_vert included, before its rounding.  Everything but l is wave-uniform.  `lds` is the wave's slice: 8 columns of 16 halfwords.  org_x / org_y:
// the picture coordinates of the sample `ref` points at (0 in the batched entries; the single-call forms upload a sub-rectangle).
template <typename PIX>
__device__ __forceinline__ int warp_tile(const PIX* ref, const SvtHipWarpRef& R, const int org_x, const int org_y, const int ssx, const int ssy, const int j, const int i,
                                         const int l, uint32_t* lds, const int bd, const int rbh) {
    const int64_t src_x = ((int64_t)j + 4) << ssx, src_y = ((int64_t)i + 4) << ssy;
    const int32_t dst_x = (int32_t)((int64_t)R.mat[2] * src_x + (int64_t)R.mat[3] * src_y + R.mat[0]); // (fits: the descriptor check)
    const int32_t dst_y = (int32_t)((int64_t)R.mat[4] * src_x + (int64_t)R.mat[5] * src_y + R.mat[1]);
    const int32_t x4 = dst_x >> ssx, y4 = dst_y >> ssy;
    const int     ix4 = x4 >> 16, iy4 = y4 >> 16;
    const int     sx4 = ((x4 & 0xffff) - 4 * R.alpha - 4 * R.beta) & ~63; // WARP_PARAM_REDUCE_BITS
    const int     sy4 = ((y4 & 0xffff) - 4 * R.gamma - 4 * R.delta) & ~63;
    const int     wm1 = R.width - 1, hm1 = R.height - 1;
    const bool    interior = ix4 - 7 >= 0 && ix4 + 7 <= wm1; // the 15 columns the tile can touch
    const PIX*    base = ref - ((int64_t)org_y * R.stride + org_x);
    i16_alias*    st = (i16_alias*)lds;
#pragma unroll
    for (int rnd = 0; rnd < 2; rnd++) {
        const int idx = l + 64 * rnd, k = idx >> 3, c = idx & 7; // intermediate row k - 7, output column c - 4
        if (idx < 120) {
            const int iy  = clampi(iy4 + k - 7, 0, hm1);
            const int sx  = sx4 + R.beta * (k - 3) + R.alpha * c;
            const int sum = warp_hsum(base + (int64_t)iy * R.stride, ix4 + c - 7, wm1, interior, warp_row(sx), bd);
            st[c * 16 + k] = (int16_t)(rpot(sum, rbh) - 32768); // 0 .. 65535 -> a signed halfword; the 128 * 32768 comes back with the vertical offset
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int        r = l >> 3, c = l & 7;
    const u32_alias* w = (const u32_alias*)lds + (c * 8 + (r >> 1));
    const uint32_t   q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3], q4 = w[4];
    const uint32_t   sh = (r & 1) ? 16 : 0;
    const u32x4      t = *(const SVT_HIP_GLOBAL_AS u32x4*)&kTabs.h2[warp_row(sy4 + R.delta * r + R.gamma * c)][0];
    int              s = (1 << (bd + 14 - rbh)) + (1 << 22);
    s                  = sdot2(__builtin_amdgcn_alignbit(q1, q0, sh), t[0], s);
    s                  = sdot2(__builtin_amdgcn_alignbit(q2, q1, sh), t[1], s);
    s                  = sdot2(__builtin_amdgcn_alignbit(q3, q2, sh), t[2], s);
    s                  = sdot2(__builtin_amdgcn_alignbit(q4, q3, sh), t[3], s);
    __builtin_amdgcn_wave_barrier(); // the slice is rewritten by the next reference / tile
    return s;
}

// is_affine_shear_allowed (warped_motion.c:357)
__device__ __forceinline__ bool shear_ok(const int a, const int b, const int g, const int d) {
    return 4 * abs(a) + 7 * abs(b) < 65536 && 4 * abs(g) + 4 * abs(d) < 65536;
}
// everything warp_tile relies on for the tiles (0 .. ntx - 1) x (0 .. nty - 1) of a block at (p_col, p_row): dst_x / dst_y are affine in the tile index, so their
// extremes lie at the four corner tiles
__device__ __forceinline__ bool warp_ref_ok(const SvtHipWarpRef& R, const void* const* bases, const int p_col, const int p_row, const int ntx, const int nty,
                                            const int ssx, const int ssy) {
    if (R.width < 1 || R.height < 1 || R.stride < 1 || R.plane >= 32 || bases[R.plane] == nullptr) return false;
    if (!shear_ok(R.alpha, R.beta, R.gamma, R.delta)) return false;
    for (int cy = 0; cy < 2; cy++)
        for (int cx = 0; cx < 2; cx++) {
            const int64_t sx = ((int64_t)p_col + 8 * (int64_t)(cx ? ntx - 1 : 0) + 4) << ssx, sy = ((int64_t)p_row + 8 * (int64_t)(cy ? nty - 1 : 0) + 4) << ssy;
            if (sx < INT32_MIN || sx > INT32_MAX || sy < INT32_MIN || sy > INT32_MAX) return false;
            const int64_t dx = (int64_t)R.mat[2] * sx + (int64_t)R.mat[3] * sy + R.mat[0], dy = (int64_t)R.mat[4] * sx + (int64_t)R.mat[5] * sy + R.mat[1];
            if (dx < INT32_MIN || dx > INT32_MAX || dy < INT32_MIN || dy > INT32_MAX) return false;
        }
    return true;
}
__device__ __forceinline__ bool warp_desc_ok(const SvtHipWarpDesc& d, const SvtHipInterPredPlanes& planes) {
    if (d.p_width < 1 || d.p_width > 128 || d.p_height < 1 || d.p_height > 128 || d.subsampling_x > 1 || d.subsampling_y > 1 || d.compound > 2) return false;
    const int ntx = (d.p_width + 7) >> 3, nty = (d.p_height + 7) >> 3;
    if (!warp_ref_ok(d.ref[0], planes.base, d.p_col, d.p_row, ntx, nty, d.subsampling_x, d.subsampling_y)) return false;
    return d.compound == 0 || warp_ref_ok(d.ref[1], planes.base, d.p_col, d.p_row, ntx, nty, d.subsampling_x, d.subsampling_y);
}

// mode 0: the batched entry.  The single-call forms: 1 = is_compound with do_average == 0 (the ConvBufType values go to cb, dst is not written), 2 = do_average == 1
// (the first reference's values are read from cb; jnt = use_jnt_comp_avg, with the form's own offsets; the descriptor of a form is not compound).
struct WarpAux {
    int       bd, r0, r1;      // round_0; round_1 of the compound paths
    int       mode, jnt, fwd, bck;
    int       org_x, org_y;
    uint16_t* cb;
    uint32_t  cb_stride;
};

template <typename PIX>
__global__ __launch_bounds__(TPB) void warp_pred_kernel(const SvtHipInterPredPlanes planes, PIX* __restrict__ dst_base, const SvtHipWarpDesc* __restrict__ descs,
                                                        const uint32_t n, uint8_t* __restrict__ status, const WarpAux aux) {
    __shared__ uint32_t pre[DPW + 1]; // exclusive prefix sum of the tile counts
    __shared__ uint32_t tmp[WAVES][64];
    const int      tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t first = blockIdx.x * DPW;
    if (tid < 64) {
        uint32_t cnt = 0;
        if (tid < DPW && first + tid < n) {
            const SvtHipWarpDesc d  = descs[first + tid];
            const bool           ok = warp_desc_ok(d, planes);
            if (ok) cnt = (uint32_t)((d.p_width + 7) >> 3) * (uint32_t)((d.p_height + 7) >> 3);
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
    const int      bd = aux.bd, maxv = (1 << bd) - 1;
    // svt_av1_highbd_warp_affine_c: round_0 + AOMMAX(bd + FILTER_BITS - round_0 - 14, 0), as written there (0 at every depth with get_conv_params_no_round's round_0)
    const int rbh = sizeof(PIX) == 1 ? aux.r0 : aux.r0 + (bd + 7 - aux.r0 - 14 > 0 ? bd + 7 - aux.r0 - 14 : 0);
    const int round_bits = 14 - aux.r0 - aux.r1, offset_bits = bd + 14 - aux.r0;
    for (uint32_t u = blockIdx.y * WAVES + wv; u < total; u += gridDim.y * WAVES) {
        int di = 0;
#pragma unroll
        for (int s = DPW >> 1; s >= 1; s >>= 1)
            if (pre[di + s] <= u) di += s;
        di = __builtin_amdgcn_readfirstlane(di);
        const SvtHipWarpDesc d = descs[first + di];
        const uint32_t loc = u - pre[di], ntx = (uint32_t)(d.p_width + 7) >> 3, tyi = loc / ntx, txi = loc - tyi * ntx;
        const int      x0 = (int)(txi * 8), y0 = (int)(tyi * 8), r = l >> 3, c = l & 7;
        const bool     on = x0 + c < d.p_width && y0 + r < d.p_height; // the C crops the last tile: AOMMIN(4, p_col + p_width - j - 4)
        const size_t   pos = (size_t)(y0 + r) * d.dst_stride + (size_t)(x0 + c);
        const bool     comp = aux.mode != 0 || d.compound != 0;
        int            held = 0;
        if (aux.mode == 2 && on) held = aux.cb[(size_t)(y0 + r) * aux.cb_stride + (size_t)(x0 + c)];
        // one reference; `second`: its value meets the held one (written out twice so that d.ref[] is indexed by constants and the descriptor stays in registers)
        const auto one_ref = [&](const SvtHipWarpRef& R, const bool second) {
            int sum = warp_tile((const PIX*)planes.base[R.plane] + R.ref_off, R, aux.org_x, aux.org_y, d.subsampling_x, d.subsampling_y, d.p_col + x0, d.p_row + y0, l,
                                tmp[wv], bd, rbh);
            if (!comp) {
                const int v = rpot(sum, 14 - rbh) - (1 << (bd - 1)) - (1 << bd);
                if (on) dst_base[d.dst_off + pos] = (PIX)clampi(v, 0, maxv);
                return;
            }
            sum = rpot(sum, aux.r1);
            if (aux.mode == 1) {
                if (on) aux.cb[(size_t)(y0 + r) * aux.cb_stride + (size_t)(x0 + c)] = (uint16_t)sum; // ConvBufType
            } else if (!second) held = sum & 0xffff;                                                // the same narrowing, in a register
            else {
                int v;
                if (aux.mode ? aux.jnt != 0 : d.compound == 2) v = (held * (aux.mode ? aux.fwd : (int)d.fwd_offset) + sum * (aux.mode ? aux.bck : (int)d.bck_offset)) >> 4; // DIST_PRECISION_BITS
                else v = (held + sum) >> 1;
                v -= (1 << (offset_bits - aux.r1)) + (1 << (offset_bits - aux.r1 - 1));
                if (on) dst_base[d.dst_off + pos] = (PIX)clampi(rpot(v, round_bits), 0, maxv);
            }
        };
        one_ref(d.ref[0], aux.mode == 2);
        if (aux.mode == 0 && d.compound) one_ref(d.ref[1], true);
    }
}
__global__ __launch_bounds__(TPB) void warp_pred_check_kernel(const SvtHipInterPredPlanes planes, const SvtHipWarpDesc* __restrict__ descs, const uint32_t n,
                                                              uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !warp_desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

// ---- the warp error ---------------------------------------------------------------------------------------------------------------------------------
constexpr int ERR_MAX_DIM = 65536;
__device__ __forceinline__ bool error_desc_ok(const SvtHipWarpErrorDesc& d, const SvtHipInterPredPlanes& planes) {
    if (d.p_width < 1 || d.p_width > ERR_MAX_DIM || d.p_height < 1 || d.p_height > ERR_MAX_DIM || d.subsampling_x > 1 || d.subsampling_y > 1 || d.chess_refn > 1) return false;
    if (d.src_stride < 1 || d.src_plane >= 32 || planes.base[d.src_plane] == nullptr) return false;
    return warp_ref_ok(d.ref, planes.base, d.p_col, d.p_row, (d.p_width + 7) >> 3, (d.p_height + 7) >> 3, d.subsampling_x, d.subsampling_y);
}
// grid (ERR_WG / n, n): the waves of row blockIdx.y walk the 8x8 tiles of candidate blockIdx.y's selected 32x32 error blocks (16 tiles each, the last column / row of
// blocks cropped), a lane keeps the sum of its sample's absolute differences, one butterfly and one atomic per wave at the end
__global__ __launch_bounds__(TPB) void warp_error_kernel(const SvtHipInterPredPlanes planes, const SvtHipWarpErrorDesc* __restrict__ descs, uint64_t* __restrict__ out,
                                                         uint8_t* __restrict__ status) {
    __shared__ uint32_t tmp[WAVES][64];
    const int                 l = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const SvtHipWarpErrorDesc d  = descs[blockIdx.y];
    const bool                ok = error_desc_ok(d, planes);
    if (status && blockIdx.x == 0 && threadIdx.x == 0) status[blockIdx.y] = ok ? 0 : 1;
    if (!ok) return;
    const uint32_t nbx = (uint32_t)(d.p_width + 31) >> 5, nby = (uint32_t)(d.p_height + 31) >> 5, total = nbx * nby * 16;
    const uint8_t* ref = (const uint8_t*)planes.base[d.ref.plane] + d.ref.ref_off;
    const uint8_t* src = (const uint8_t*)planes.base[d.src_plane] + d.src_off;
    const int      r = l >> 3, c = l & 7;
    uint32_t       acc = 0;
    for (uint32_t u = blockIdx.x * WAVES + wv; u < total; u += gridDim.x * WAVES) {
        const uint32_t b = u >> 4, by = b / nbx, bx = b - by * nbx;
        if (d.chess_refn && !((bx + by) & 1)) continue; // jstart: the odd blocks of an even block row, the even blocks of an odd one
        const int x0 = (int)(bx * 32 + (u & 3) * 8), y0 = (int)(by * 32 + ((u >> 2) & 3) * 8);
        if (x0 >= d.p_width || y0 >= d.p_height) continue;
        // get_conv_params(0, 0, 0, 8): round_0 3, not compound
        const int sum = warp_tile(ref, d.ref, 0, 0, d.subsampling_x, d.subsampling_y, d.p_col + x0, d.p_row + y0, l, tmp[wv], 8, 3);
        const int v   = clampi(rpot(sum, 11) - 128 - 256, 0, 255);
        if (x0 + c < d.p_width && y0 + r < d.p_height) {
            const int s = load_px(src + ((int64_t)(d.p_row + y0 + r) * d.src_stride + (int64_t)(d.p_col + x0 + c)));
            acc += (uint32_t)abs(s - v);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += (uint32_t)__shfl_xor((int)acc, m);
    if (l == 0 && acc) atomicAdd((unsigned long long*)(out + blockIdx.y), (unsigned long long)acc << d.chess_refn);
}
__global__ __launch_bounds__(TPB) void warp_error_check_kernel(const SvtHipInterPredPlanes planes, const SvtHipWarpErrorDesc* __restrict__ descs, const uint32_t n,
                                                               uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !error_desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

// ---- the model fit ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int     msb32(const uint32_t v) { return 31 - __builtin_clz(v); } // get_msb, v != 0
__device__ __forceinline__ int64_t rpot64(const int64_t v, const int n) { return (v + (((int64_t)1 << n) >> 1)) >> n; }
// ROUND_POWER_OF_TWO_SIGNED_64; the negation and the addition in uint64_t, so that a product that left int64_t (sample sets outside the range the C asserts) still
// gives one defined result on every compiler
__device__ __forceinline__ int64_t wrap_neg64(const int64_t v) { return (int64_t)(0 - (uint64_t)v); }
__device__ __forceinline__ int64_t rpot64_signed(const int64_t v, const int n) {
    const uint64_t half = ((uint64_t)1 << n) >> 1;
    return v < 0 ? wrap_neg64((int64_t)((uint64_t)wrap_neg64(v) + half) >> n) : (int64_t)((uint64_t)v + half) >> n;
}
__device__ __forceinline__ int64_t mul64(const int64_t a, const int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ __forceinline__ int32_t add32(const int32_t a, const int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int     rpot_signed(const int v, const int n) { return v < 0 ? -rpot(-v, n) : rpot(v, n); }
__device__ __forceinline__ int64_t clamp64(const int64_t v, const int64_t lo, const int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// resolve_divisor_64 / _32 (warped_motion.c:320, :336)
__device__ __forceinline__ int resolve_divisor_64(const uint64_t D, int* shift) {
    const int     s = (D >> 32) ? msb32((uint32_t)(D >> 32)) + 32 : msb32((uint32_t)D);
    const int64_t e = (int64_t)(D - ((uint64_t)1 << s));
    const int64_t f = s > 8 ? rpot64(e, s - 8) : e << (8 - s);
    *shift          = s + 14;
    return kTabs.div[f];
}
__device__ __forceinline__ int resolve_divisor_32(const uint32_t D, int* shift) {
    const int     s = msb32(D);
    const int32_t e = (int32_t)(D - ((uint32_t)1 << s));
    const int32_t f = s > 8 ? rpot(e, s - 8) : e << (8 - s);
    *shift          = s + 14;
    return kTabs.div[f];
}
// LS_SQUARE, LS_PRODUCT1, LS_PRODUCT2 (warped_motion.c:46-48), LS_STEP 8, LS_MAT_DOWN_BITS 2
// (the sums in uint32_t: inside the range the C asserts nothing wraps; outside it the wrap is the same everywhere)
__device__ __forceinline__ int ls_square(const int a) { return (int32_t)((uint32_t)a * (uint32_t)a * 4u + (uint32_t)a * 32u + 128u) >> 4; }
__device__ __forceinline__ int ls_product1(const int a, const int b) { return (int32_t)((uint32_t)a * (uint32_t)b * 4u + ((uint32_t)a + (uint32_t)b) * 16u + 64u) >> 4; }
__device__ __forceinline__ int ls_product2(const int a, const int b) { return (int32_t)((uint32_t)a * (uint32_t)b * 4u + ((uint32_t)a + (uint32_t)b) * 16u + 128u) >> 4; }
// svt_get_shear_params (warped_motion.c:898): false = the C returns 0
__device__ __forceinline__ bool shear_params(const int32_t* mat, int16_t* sh) {
    if (mat[2] <= 0) return false; // is_affine_valid
    int a = clampi(mat[2] - 65536, INT16_MIN, INT16_MAX), b = clampi(mat[3], INT16_MIN, INT16_MAX);
    int       shift;
    const int y = resolve_divisor_32((uint32_t)mat[2], &shift);
    int64_t   v = ((int64_t)mat[4] * 65536) * y;
    int       g = clampi((int)rpot64_signed(v, shift), INT16_MIN, INT16_MAX);
    v           = ((int64_t)mat[3] * mat[4]) * y;
    int dl      = clampi(mat[5] - (int)rpot64_signed(v, shift) - 65536, INT16_MIN, INT16_MAX);
    // ROUND_POWER_OF_TWO_SIGNED(., WARP_PARAM_REDUCE_BITS) * (1 << WARP_PARAM_REDUCE_BITS), stored to int16_t
    sh[0] = (int16_t)(rpot_signed(a, 6) * 64), sh[1] = (int16_t)(rpot_signed(b, 6) * 64), sh[2] = (int16_t)(rpot_signed(g, 6) * 64), sh[3] = (int16_t)(rpot_signed(dl, 6) * 64);
    return shear_ok(sh[0], sh[1], sh[2], sh[3]);
}
__device__ __forceinline__ bool model_desc_ok(const SvtHipWarpModelDesc& d) { return d.np >= 1 && d.np <= 8 && d.bsize < 22; }
__global__ __launch_bounds__(TPB) void warp_model_kernel(const SvtHipWarpModelDesc* __restrict__ descs, const uint32_t n, SvtHipWarpModel* __restrict__ out,
                                                         uint8_t* __restrict__ status) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    if (b >= n) return;
    const SvtHipWarpModelDesc* d  = descs + b;
    const bool                 ok = model_desc_ok(*d);
    if (status) status[b] = ok ? 0 : 1;
    if (!ok) return;
    // find_affine_int (warped_motion.c:365)
    const int bw = kBw[d->bsize], bh = kBh[d->bsize], mvy = d->mv_row, mvx = d->mv_col;
    const int rsuy = (bh > 4 ? bh : 4) / 2 - 1, rsux = (bw > 4 ? bw : 4) / 2 - 1, suy = rsuy * 8, sux = rsux * 8, duy = suy + mvy, dux = sux + mvx;
    const int isuy = d->mi_row * 4 + rsuy, isux = d->mi_col * 4 + rsux;
    int32_t   A00 = 0, A01 = 0, A11 = 0, bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
    for (int i = 0; i < d->np; i++) {
        const int dx = d->pts_inref[i * 2] - dux, dy = d->pts_inref[i * 2 + 1] - duy, sx = d->pts[i * 2] - sux, sy = d->pts[i * 2 + 1] - suy;
        if (abs(sx - dx) < 256 && abs(sy - dy) < 256) { // LS_MV_MAX
            A00 = add32(A00, ls_square(sx));
            A01 = add32(A01, ls_product1(sx, sy));
            A11 = add32(A11, ls_square(sy));
            bx0 = add32(bx0, ls_product2(sx, dx));
            bx1 = add32(bx1, ls_product1(sy, dx));
            by0 = add32(by0, ls_product1(sx, dy));
            by1 = add32(by1, ls_product2(sy, dy));
        }
    }
    SvtHipWarpModel m{};
    m.invalid         = 1;
    const int64_t det = (int64_t)A00 * A11 - (int64_t)A01 * A01;
    if (det != 0) {
        int     shift;
        int16_t i_det = (int16_t)(resolve_divisor_64((uint64_t)(det < 0 ? -det : det), &shift) * (det < 0 ? -1 : 1));
        shift -= 16; // WARPEDMODEL_PREC_BITS
        if (shift < 0) {
            i_det = (int16_t)(i_det * (1 << -shift)); // i_det <<= -shift on an int16_t: 16384 << 2 is 0, 16384 << 1 is -32768
            shift = 0;
        }
        const int64_t px0 = (int64_t)A11 * bx0 - (int64_t)A01 * bx1, px1 = -(int64_t)A01 * bx0 + (int64_t)A00 * bx1;
        const int64_t py0 = (int64_t)A11 * by0 - (int64_t)A01 * by1, py1 = -(int64_t)A01 * by0 + (int64_t)A00 * by1;
        // get_mult_shift_diag / _ndiag, the pair compiled in (USE_LIMITED_PREC_MULT 0): WARPEDMODEL_NONDIAGAFFINE_CLAMP 1 << 13
        m.wmmat[2] = (int32_t)clamp64(rpot64_signed(mul64(px0, i_det), shift), 65536 - 8192 + 1, 65536 + 8192 - 1);
        m.wmmat[3] = (int32_t)clamp64(rpot64_signed(mul64(px1, i_det), shift), -8192 + 1, 8192 - 1);
        m.wmmat[4] = (int32_t)clamp64(rpot64_signed(mul64(py0, i_det), shift), -8192 + 1, 8192 - 1);
        m.wmmat[5] = (int32_t)clamp64(rpot64_signed(mul64(py1, i_det), shift), 65536 - 8192 + 1, 65536 + 8192 - 1);
        const int32_t vx = (int32_t)((uint32_t)mvx * 8192u - ((uint32_t)isux * (uint32_t)(m.wmmat[2] - 65536) + (uint32_t)isuy * (uint32_t)m.wmmat[3]));
        const int32_t vy = (int32_t)((uint32_t)mvy * 8192u - ((uint32_t)isux * (uint32_t)m.wmmat[4] + (uint32_t)isuy * (uint32_t)(m.wmmat[5] - 65536)));
        m.wmmat[0] = clampi(vx, -(128 << 16), (128 << 16) - 1); // WARPEDMODEL_TRANS_CLAMP
        m.wmmat[1] = clampi(vy, -(128 << 16), (128 << 16) - 1);
        int16_t sh[4];
        if (shear_params(m.wmmat, sh)) {
            m.alpha = sh[0], m.beta = sh[1], m.gamma = sh[2], m.delta = sh[3];
            m.invalid = 0;
        }
    }
    if (m.invalid) {
        for (int k = 0; k < 6; k++) m.wmmat[k] = 0;
        m.alpha = m.beta = m.gamma = m.delta = 0;
    }
    out[b] = m;
}
__global__ __launch_bounds__(TPB) void warp_model_check_kernel(const SvtHipWarpModelDesc* __restrict__ descs, const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !model_desc_ok(descs[i]);
    if (bad) *bad_out = 1;
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
bool host_shear_ok(const int a, const int b, const int g, const int d) { return 4 * abs(a) + 7 * abs(b) < 65536 && 4 * abs(g) + 4 * abs(d) < 65536; }
// One block from host memory.  The host walks the block's tiles with the C's own arithmetic and takes the bounding rectangle of the clamped rows and columns they can
// touch: exactly that rectangle of the reference goes into the call's arena (at high bit depth packed from the 8-bit and the 2-bit plane on the way), with one
// descriptor; one synchronisation (the download); nothing of the caller's is written before it.
template <typename PIX>
void warp_host(const int32_t* mat, const uint8_t* ref8b, const uint8_t* ref2b, const int width, const int height, const int stride8b, const int stride2b, PIX* pred,
               const int p_col, const int p_row, const int p_width, const int p_height, const int p_stride, const int ssx, const int ssy, const int bd,
               const SvtHipConvolveParams* cp, const int16_t alpha, const int16_t beta, const int16_t gamma, const int16_t delta) {
    if (!mat || !ref8b || (sizeof(PIX) == 2 && !ref2b) || !pred || !cp) return; // nothing is written
    if (p_width < 1 || p_width > 128 || p_height < 1 || p_height > 128 || ssx < 0 || ssx > 1 || ssy < 0 || ssy > 1 || width < 1 || height < 1 || stride8b < 1) return;
    if (sizeof(PIX) == 1 ? bd != 8 : (bd != 10 && bd != 12)) return;
    if (!host_shear_ok(alpha, beta, gamma, delta)) return;
    const bool comp = cp->is_compound != 0, average = comp && cp->do_average;
    // the roundings become shift counts on the device: the range of the jnt_ forms (svtav1_hip.h)
    if (cp->round_0 < 0 || cp->round_0 > 7 || cp->round_1 < 0 || cp->round_0 + cp->round_1 > 14 || (comp && cp->round_1 > 7)) return;
    if (comp && !cp->dst) return;
    int x_lo = INT32_MAX, x_hi = INT32_MIN, y_lo = INT32_MAX, y_hi = INT32_MIN;
    for (int i = 0; i < p_height; i += 8)
        for (int j = 0; j < p_width; j += 8) {
            const int64_t sx = ((int64_t)p_col + j + 4) << ssx, sy = ((int64_t)p_row + i + 4) << ssy;
            if (sx < INT32_MIN || sx > INT32_MAX || sy < INT32_MIN || sy > INT32_MAX) return;
            const int64_t dx = (int64_t)mat[2] * sx + (int64_t)mat[3] * sy + mat[0], dy = (int64_t)mat[4] * sx + (int64_t)mat[5] * sy + mat[1];
            if (dx < INT32_MIN || dx > INT32_MAX || dy < INT32_MIN || dy > INT32_MAX) return;
            const int ix4 = ((int32_t)dx >> ssx) >> 16, iy4 = ((int32_t)dy >> ssy) >> 16;
            const auto cl = [](const int v, const int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
            x_lo = std::min(x_lo, cl(ix4 - 7, width - 1)), x_hi = std::max(x_hi, cl(ix4 + 7, width - 1));
            y_lo = std::min(y_lo, cl(iy4 - 7, height - 1)), y_hi = std::max(y_hi, cl(iy4 + 7, height - 1));
        }
    const size_t rw = (size_t)(x_hi - x_lo + 1), rh = (size_t)(y_hi - y_lo + 1), px = sizeof(PIX), blk = (size_t)p_width * p_height;
    svthip::HostCall& c = svthip::host_call();
    if (rw * rh * px <= 65536) c.begin_small();
    else c.begin();
    const size_t bytes = rw * rh * px + blk * (px + 2) + sizeof(SvtHipWarpDesc) + 4096;
    c.reserve(bytes, bytes);
    PIX*            dr = (PIX*)c.dalloc(rw * rh * px);
    PIX*            dd = (PIX*)c.dalloc(blk * px);
    uint16_t*       db = (uint16_t*)c.dalloc(blk * 2);
    SvtHipWarpDesc* dv = (SvtHipWarpDesc*)c.dalloc(sizeof(SvtHipWarpDesc));
    if (sizeof(PIX) == 1) c.up2d(dr, rw, ref8b + (size_t)y_lo * stride8b + x_lo, (size_t)stride8b, rw, rh);
    else {
        std::vector<uint16_t> packed(rw * rh);
        for (size_t y = 0; y < rh; y++)
            for (size_t x = 0; x < rw; x++)
                packed[y * rw + x] = (uint16_t)((ref8b[(y_lo + y) * (size_t)stride8b + x_lo + x] << 2) | ((ref2b[(y_lo + y) * (size_t)stride2b + x_lo + x] >> 6) & 3));
        c.up(dr, packed.data(), rw * rh * 2);
    }
    if (average) c.up2d(db, (size_t)p_width * 2, cp->dst, (size_t)cp->dst_stride * 2, (size_t)p_width * 2, p_height);
    SvtHipWarpDesc d{};
    for (int k = 0; k < 6; k++) d.ref[0].mat[k] = mat[k];
    d.ref[0].alpha = alpha, d.ref[0].beta = beta, d.ref[0].gamma = gamma, d.ref[0].delta = delta;
    d.ref[0].width = width, d.ref[0].height = height, d.ref[0].stride = (int32_t)rw;
    d.dst_stride = (uint32_t)p_width;
    d.p_col = p_col, d.p_row = p_row;
    d.p_width = (uint8_t)p_width, d.p_height = (uint8_t)p_height;
    d.subsampling_x = (uint8_t)ssx, d.subsampling_y = (uint8_t)ssy;
    c.up(dv, &d, sizeof(d));
    SvtHipInterPredPlanes planes{};
    planes.base[0] = dr;
    WarpAux aux{};
    aux.bd = bd, aux.r0 = cp->round_0, aux.r1 = cp->round_1;
    aux.mode = comp ? (average ? 2 : 1) : 0;
    aux.jnt = average && cp->use_jnt_comp_avg;
    aux.fwd = cp->fwd_offset, aux.bck = cp->bck_offset;
    aux.org_x = x_lo, aux.org_y = y_lo;
    aux.cb = db, aux.cb_stride = (uint32_t)p_width;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(warp_pred_kernel<PIX>), dim3(1, 1), dim3(TPB), 0, c.stream, planes, dd, (const SvtHipWarpDesc*)dv, 1u, (uint8_t*)nullptr, aux);
    SVT_LAUNCH_CHECK();
    if (comp && !average) c.down2d(cp->dst, (size_t)cp->dst_stride * 2, db, (size_t)p_width * 2, (size_t)p_width * 2, p_height);
    else c.down2d(pred, (size_t)p_stride * px, dd, (size_t)p_width * px, (size_t)p_width * px, p_height);
}

} // namespace

extern "C" {

int svt_hip_warp_pred_batch(SvtHipInterPredPlanes planes, void* dst_base, const SvtHipWarpDesc* descs, uint32_t n, int bit_depth, uint8_t* status, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!dst_base || !descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(warp_pred_check_kernel, grid, dim3(TPB), 0, st, planes, descs, n, bad); })) return -1;
    WarpAux aux{};
    aux.bd = bit_depth;
    aux.r0 = bit_depth == 12 ? 5 : 3; // get_conv_params_no_round: ROUND0_BITS, raised while bd + FILTER_BITS - round_0 + 2 > 16
    aux.r1 = 7;                       // COMPOUND_ROUND1_BITS
    const dim3 grid((n + DPW - 1) / DPW, SPLIT), block(TPB);
    if (bit_depth > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(warp_pred_kernel<uint16_t>), grid, block, 0, st, planes, (uint16_t*)dst_base, descs, n, status, aux);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(warp_pred_kernel<uint8_t>), grid, block, 0, st, planes, (uint8_t*)dst_base, descs, n, status, aux);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_warp_model_batch(const SvtHipWarpModelDesc* descs, uint32_t n, SvtHipWarpModel* out, uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!descs || !out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(warp_model_check_kernel, grid, dim3(TPB), 0, st, descs, n, bad); })) return -1;
    hipLaunchKernelGGL(warp_model_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, st, descs, n, out, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_warp_error_batch(SvtHipInterPredPlanes planes, const SvtHipWarpErrorDesc* descs, uint32_t n, uint64_t* out, uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!descs || !out || n > 65535) return -1; // (one grid row per candidate)
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(warp_error_check_kernel, grid, dim3(TPB), 0, st, planes, descs, n, bad); }))
        return -1;
    HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n * sizeof(uint64_t), st));
    const uint32_t per = std::min(256u, std::max(16u, (uint32_t)ERR_WG / n));
    hipLaunchKernelGGL(warp_error_kernel, dim3(per, n), dim3(TPB), 0, st, planes, descs, out, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

void svt_av1_warp_affine_hip(const int32_t* mat, const uint8_t* ref, int width, int height, int stride, uint8_t* pred, int p_col, int p_row, int p_width, int p_height,
                             int p_stride, int subsampling_x, int subsampling_y, SvtHipConvolveParams* conv_params, int16_t alpha, int16_t beta, int16_t gamma,
                             int16_t delta) {
    if (svthip::failed()) return;
    try {
        warp_host<uint8_t>(mat, ref, nullptr, width, height, stride, 0, pred, p_col, p_row, p_width, p_height, p_stride, subsampling_x, subsampling_y, 8, conv_params, alpha,
                           beta, gamma, delta);
    } catch (const svthip::DeviceError&) {}
}
void svt_av1_highbd_warp_affine_hip(const int32_t* mat, const uint8_t* ref8b, const uint8_t* ref2b, int width, int height, int stride8b, int stride2b, uint16_t* pred,
                                    int p_col, int p_row, int p_width, int p_height, int p_stride, int subsampling_x, int subsampling_y, int bd,
                                    SvtHipConvolveParams* conv_params, int16_t alpha, int16_t beta, int16_t gamma, int16_t delta) {
    if (svthip::failed()) return;
    try {
        if (stride2b < 1) return;
        warp_host<uint16_t>(mat, ref8b, ref2b, width, height, stride8b, stride2b, pred, p_col, p_row, p_width, p_height, p_stride, subsampling_x, subsampling_y, bd,
                            conv_params, alpha, beta, gamma, delta);
    } catch (const svthip::DeviceError&) {}
}

} // extern "C"
