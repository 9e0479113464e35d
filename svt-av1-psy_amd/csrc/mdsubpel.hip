// mdsubpel.hip -- the block variance family of svt_aom_mefn_ptr and mode decision's sub-pel motion search for gfx950, 8-bit luma.  DESIGN.md 4.24 has the layout,
// the narrowings and the footprints.
//
//  * block_var_kernel: one launch, n descriptors of mixed sizes and kinds: svt_aom_variance / sub_pixel_variance / obmc_sad / obmc_variance / obmc_sub_pixel_variance
//    {W}x{H}_c (C_DEFAULT/variance.c, sad_av1.c), svt_aom_mse16x16_c (svt_psnr.c:63) and svt_aom_upsampled_pred_c + vf (what svt_upsampled_pref_error computes).
//  * md_subpel_kernel: one launch, n (block, reference) searches: svt_av1_find_best_sub_pixel_tree / _tree_pruned (mcomp.c:688, :606) as md_subpel_search calls them.
//  * obmc_wsrc_kernel / obmc_search_kernel: the OBMC motion refinement on top of the OBMC kinds -- calc_target_weighted_pred (enc_inter_prediction.c:1756) for n blocks and
//    single_motion_search (mode_decision.c:2290) for n OBMC_CAUSAL candidates; DESIGN.md 4.27.  They sit here for pred_full / pred_bil / pred_up / wave_sum.
//  Both searches and the primitives follow tf_subpel.hip: ONE WAVE per item; the candidate loop is sequential and wave-uniform -- a step counter names the next candidate, so that there is one
//  evaluation site; the 64 lanes split the block's pixels (pixel i = lane + 64 k, row-major); sum / sse are wave reductions made uniform with v_readfirstlane, accept
//  and exit decisions are scalar.  The source block is read once per item into the wave's LDS slice; the horizontally filtered intermediate of the 2-D upsampled
//  prediction ((H + 7) rows x W, uint8_t as in the C) lives behind it, COLUMN-major with a pitch of H + 8, so that the vertical stage reads a lane's eight values
//  as three aligned dwords + v_alignbyte.  Nothing is written to memory but the result.
//  * two launch classes, because the host cannot read the descriptors: blocks of up to 4096 pixels run four waves per workgroup (8 704 B of LDS per wave: 4 096
//    source + 64 x 72 intermediate; 34 816 B per workgroup, four workgroups per CU), the three larger sizes run ONE wave per workgroup (33 792 B: 16 384 source +
//    128 x 136 intermediate; four workgroups per CU instead of the one that four such waves per workgroup would leave).  Every entry launches both classes; a wave
//    whose item belongs to the other class returns after reading its descriptor.
//  * the eight-tap rows: only even phases are reachable (the C indexes its 16-phase tables with q3 << 1), and phase 0 is never filtered (the copy branch); the 3 x 7
//    rows are defined here, restated in tests/mdsubpel_common.py and pinned there on the reference's tables.  Every used tap lies in -16 .. 126 and every row sums
//    to 128 (checked at compile time): v_dot4_i32_i8 on sample - 128.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include "maskpred_tables.h"
#include <algorithm>

namespace {
using svt_maskpred::kBh; // block_size_wide / block_size_high
using svt_maskpred::kBw;

constexpr int SMALL_PIX   = 4096;
constexpr int SMALL_WAVES = 4;
constexpr int IM_SMALL    = 64 * 72;   // W * (H + 8) of the largest small block
constexpr int IM_BIG      = 128 * 136;
constexpr int SRC_BIG     = 128 * 128;
constexpr int MV_MAX_     = 16383;     // MV_MAX, cabac_context_model.h:520
constexpr int MV_UPP_     = 16384;     // MV_UPP / -MV_LOW

// rows 2, 4 .. 14 of av1_bilinear_filters, av1_sub_pel_filters_4, av1_sub_pel_filters_8 (variance.c:73-140): [subpel_search - 1][q3 - 1]
constexpr int8_t kUpRows[3][7][8] = {
    {{0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 80, 48, 0, 0, 0}, {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 48, 80, 0, 0, 0}, {0, 0, 0, 32, 96, 0, 0, 0},
     {0, 0, 0, 16, 112, 0, 0, 0}},
    {{0, 0, -8, 122, 18, -4, 0, 0}, {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0},
     {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -4, 18, 122, -8, 0, 0}},
    {{0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0}, {0, 2, -14, 76, 76, -14, 2, 0}, {0, 2, -12, 58, 94, -16, 2, 0},
     {0, 2, -10, 38, 110, -14, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}}};
struct UpTabs {
    uint32_t t[3][8][2]; // [subpel_search - 1][q3]: taps 4k .. 4k + 3 as int8; row 0 is never read
    bool     ok;
};
constexpr UpTabs make_up_tabs() {
    UpTabs t{};
    t.ok = true;
    for (int s = 0; s < 3; s++)
        for (int q = 1; q < 8; q++) {
            int sum = 0;
            for (int m = 0; m < 8; m++) {
                const int v = kUpRows[s][q - 1][m];
                sum += v;
                t.t[s][q][m >> 2] |= (uint32_t)(uint8_t)(int8_t)v << (8 * (m & 3));
            }
            t.ok = t.ok && sum == 128;
        }
    return t;
}
__device__ constexpr UpTabs kUp = make_up_tabs();
static_assert(make_up_tabs().ok, "the dot product on sample - 128 relies on rows that sum to 128");

typedef uint32_t u32_alias __attribute__((may_alias));

struct Geo {
    int W, H, lw, ln, npix; // ln = log2(W * H) = num_pels_log2_lookup
};
__device__ __forceinline__ Geo geo_of(const int bsize) {
    Geo g;
    g.W = kBw[bsize], g.H = kBh[bsize];
    g.lw   = 31 - __clz((unsigned)g.W);
    g.ln   = g.lw + 31 - __clz((unsigned)g.H);
    g.npix = g.W * g.H;
    return g;
}
__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int wave_sum(int v) { // the total as a scalar: four DPP steps inside each row of 16 lanes, then the four rows' sums (wrapping adds)
    uint32_t u = (uint32_t)v;
    u += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
    u += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
    u += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x124, 0xf, 0xf, false); // row_ror:4
    u += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x128, 0xf, 0xf, false); // row_ror:8
    const int r = (int)u;
    return (int)((uint32_t)__builtin_amdgcn_readlane(r, 0) + (uint32_t)__builtin_amdgcn_readlane(r, 16) + (uint32_t)__builtin_amdgcn_readlane(r, 32) +
                 (uint32_t)__builtin_amdgcn_readlane(r, 48));
}
// sum over the eight taps of tap * sample: the samples as bytes of v0 (0 .. 3), v1 (4 .. 7); the 128 * 128 of the taps' sum comes back with the offset
__device__ __forceinline__ int dot8(const uint32_t v0, const uint32_t v1, const uint32_t t0, const uint32_t t1) {
    return __builtin_amdgcn_sdot4((int)(v0 ^ 0x80808080u), (int)t0, __builtin_amdgcn_sdot4((int)(v1 ^ 0x80808080u), (int)t1, 16384, false), false);
}
__device__ __forceinline__ int clip_round7(int s) { // clip_pixel(ROUND_POWER_OF_TWO(sum, FILTER_BITS))
    s = (s + 64) >> 7;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// ---- the three predictions: f(i, px) for each of the lane's pixels i = l, l + 64, ..  Everything but l is wave-uniform. ---------------------------------------------
template <typename F> __device__ __forceinline__ void pred_full(const uint8_t* p, const int64_t stride, const Geo g, const int l, F&& f) {
    for (int i = l; i < g.npix; i += 64) f(i, load_px(p + (int64_t)(i >> g.lw) * stride + (i & (g.W - 1))));
}
// aom_var_filter_block2d_bil_first_pass_c / _second_pass_c (variance.c:28-68): a zero second tap returns the first sample, so column W / row H are only read when the
// offset is not 0
template <typename F> __device__ __forceinline__ void pred_bil(const uint8_t* p, const int64_t stride, const int xo, const int yo, const Geo g, const int l, F&& f) {
    const int f0 = 128 - 16 * xo, f1 = 16 * xo, g0 = 128 - 16 * yo, g1 = 16 * yo; // bilinear_filters_2t (filter.h:39)
    for (int i = l; i < g.npix; i += 64) {
        const uint8_t* q = p + (int64_t)(i >> g.lw) * stride + (i & (g.W - 1));
        int            a = load_px(q);
        if (xo) a = (a * f0 + load_px(q + 1) * f1 + 64) >> 7;
        if (yo) {
            int b = load_px(q + stride);
            if (xo) b = (b * f0 + load_px(q + stride + 1) * f1 + 64) >> 7;
            a = (a * g0 + b * g1 + 64) >> 7;
        }
        f(i, a);
    }
}
// svt_aom_upsampled_pred_c (variance.c:204-254): svt_aom_convolve8_horiz_c, then _vert_c on its clipped 8-bit output.  `im`: the wave's H + 7 intermediate rows,
// column-major, pitch H + 8 bytes.
template <typename F>
__device__ __forceinline__ void pred_up(const uint8_t* p, const int64_t stride, const int xq, const int yq, const int taps, const Geo g, uint8_t* im, const int l, F&& f) {
    if (!xq && !yq) {
        pred_full(p, stride, g, l, f);
        return;
    }
    const uint32_t tx0 = kUp.t[taps - 1][xq][0], tx1 = kUp.t[taps - 1][xq][1], ty0 = kUp.t[taps - 1][yq][0], ty1 = kUp.t[taps - 1][yq][1];
    if (!yq) {
        for (int i = l; i < g.npix; i += 64) {
            const svt_u32x2_a1 v = svt_hip_global_load_x2(p + (int64_t)(i >> g.lw) * stride + (i & (g.W - 1)) - 3);
            f(i, clip_round7(dot8(v[0], v[1], tx0, tx1)));
        }
    } else if (!xq) {
        for (int i = l; i < g.npix; i += 64) {
            const uint8_t* q  = p + (int64_t)((i >> g.lw) - 3) * stride + (i & (g.W - 1));
            uint32_t       v0 = 0, v1 = 0;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                v0 |= (uint32_t)load_px(q + m * stride) << (8 * m);
                v1 |= (uint32_t)load_px(q + (m + 4) * stride) << (8 * m);
            }
            f(i, clip_round7(dot8(v0, v1, ty0, ty1)));
        }
    } else {
        const int P = g.H + 8, cells = (g.H + 7) * g.W; // (((h - 1) * 8 + y) >> 3) + 8 rows from 3 rows above
        for (int i = l; i < cells; i += 64) {
            const int          r = i >> g.lw, x = i & (g.W - 1);
            const svt_u32x2_a1 v = svt_hip_global_load_x2(p + (int64_t)(r - 3) * stride + x - 3);
            im[x * P + r]        = (uint8_t)clip_round7(dot8(v[0], v[1], tx0, tx1));
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = l; i < g.npix; i += 64) {
            const int        y = i >> g.lw, x = i & (g.W - 1);
            const u32_alias* w = (const u32_alias*)(im + x * P + (y & ~3));
            const uint32_t   q0 = w[0], q1 = w[1], q2 = w[2], sh = (uint32_t)(y & 3);
            f(i, clip_round7(dot8(__builtin_amdgcn_alignbyte(q1, q0, sh), __builtin_amdgcn_alignbyte(q2, q1, sh), ty0, ty1)));
        }
        __builtin_amdgcn_wave_barrier(); // the slice is rewritten by the next candidate
    }
}

__device__ __forceinline__ uint32_t variance_of(const uint32_t sse, const int sum, const int ln) { return sse - (uint32_t)(((int64_t)sum * sum) >> ln); }

// ---- the primitives -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool var_desc_ok(const SvtHipBlockVarDesc& d, const SvtHipInterPredPlanes& planes, const bool have_src, const bool have_obmc) {
    if (d.bsize >= 22 || d.kind > SVT_HIP_VAR_OBMC_SUBPIX || d.pre_plane >= 32 || planes.base[d.pre_plane] == nullptr) return false;
    const bool obmc = d.kind >= SVT_HIP_VAR_OBMC_SAD;
    if (obmc ? !have_obmc : !have_src) return false;
    if (d.kind == SVT_HIP_VAR_SUBPIX || d.kind == SVT_HIP_VAR_OBMC_SUBPIX || d.kind == SVT_HIP_VAR_UPSAMPLED)
        if (d.xoffset > 7 || d.yoffset > 7) return false;
    if (d.kind == SVT_HIP_VAR_UPSAMPLED && (d.taps < 1 || d.taps > 3)) return false;
    if (d.kind == SVT_HIP_VAR_MSE && d.bsize != 6) return false; // BLOCK_16X16
    return true;
}
template <bool BIG>
__global__ __launch_bounds__(BIG ? 64 : 64 * SMALL_WAVES) void block_var_kernel(const SvtHipInterPredPlanes planes, const uint8_t* __restrict__ src_base,
                                                                                const int32_t* __restrict__ wsrc_base, const int32_t* __restrict__ mask_base,
                                                                                const SvtHipBlockVarDesc* __restrict__ descs, const uint32_t n,
                                                                                SvtHipBlockVarResult* __restrict__ out, uint8_t* __restrict__ status) {
    HIP_DYNAMIC_SHARED(uint32_t, smem)
    constexpr int  WV = BIG ? 1 : SMALL_WAVES, SLICE = BIG ? IM_BIG : IM_SMALL;
    const int      l = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t item = blockIdx.x * WV + (uint32_t)wv;
    if (item >= n) return;
    const SvtHipBlockVarDesc d  = descs[item];
    const bool               ok = var_desc_ok(d, planes, src_base != nullptr, wsrc_base != nullptr && mask_base != nullptr);
    if (status && !BIG && l == 0) status[item] = ok ? 0 : 1;
    if (!ok) return;
    const Geo g = geo_of(d.bsize);
    if ((g.npix > SMALL_PIX) != BIG) return;
    uint8_t*       im   = (uint8_t*)smem + wv * SLICE;
    const uint8_t* pre  = (const uint8_t*)planes.base[d.pre_plane] + d.pre_off;
    const bool     obmc = d.kind >= SVT_HIP_VAR_OBMC_SAD;
    const uint8_t* src  = src_base + (obmc ? 0 : d.src_off);
    const int32_t* ws   = wsrc_base + (obmc ? d.wsrc_off : 0);
    const int32_t* mk   = mask_base + (obmc ? d.mask_off : 0);
    int            sum_l = 0;
    uint32_t       sse_l = 0, sad_l = 0;
    const auto     acc = [&](const int i, const int px) {
        if (obmc) { // obmc_variance (variance.c:347) / obmc_sad (sad_av1.c:18): the magnitude is rounded, ties away from zero
            const int      v = (int)((uint32_t)ws[i] - (uint32_t)px * (uint32_t)mk[i]);
            const uint32_t r = ((v < 0 ? 0u - (uint32_t)v : (uint32_t)v) + 2048u) >> 12;
            sad_l += r;
            sum_l += v < 0 ? -(int)r : (int)r;
            sse_l += r * r;
        } else {
            const int diff = px - load_px(src + (uint32_t)(i >> g.lw) * d.src_stride + (uint32_t)(i & (g.W - 1)));
            sum_l += diff;
            sse_l += (uint32_t)(diff * diff);
        }
    };
    if (d.kind == SVT_HIP_VAR_SUBPIX || d.kind == SVT_HIP_VAR_OBMC_SUBPIX) pred_bil(pre, (int64_t)d.pre_stride, d.xoffset, d.yoffset, g, l, acc);
    else if (d.kind == SVT_HIP_VAR_UPSAMPLED) pred_up(pre, (int64_t)d.pre_stride, d.xoffset, d.yoffset, d.taps, g, im, l, acc);
    else pred_full(pre, (int64_t)d.pre_stride, g, l, acc);
    const int      sum = wave_sum(sum_l);
    const uint32_t sse = (uint32_t)wave_sum((int)sse_l), sad = (uint32_t)wave_sum((int)sad_l);
    if (l == 0) {
        SvtHipBlockVarResult r;
        r.var = r.sse = r.sad = 0, r.sum = 0;
        if (d.kind == SVT_HIP_VAR_MSE) r.var = r.sse = sse;
        else if (d.kind == SVT_HIP_VAR_OBMC_SAD) r.sad = sad;
        else r.var = variance_of(sse, sum, g.ln), r.sse = sse, r.sum = sum;
        out[item] = r;
    }
}
__global__ __launch_bounds__(256) void block_var_check_kernel(const SvtHipInterPredPlanes planes, const bool have_src, const bool have_obmc,
                                                              const SvtHipBlockVarDesc* __restrict__ descs, const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) bad |= !var_desc_ok(descs[i], planes, have_src, have_obmc);
    if (bad) *bad_out = 1;
}
// svt_aom_upsampled_pred_hip: one block, the prediction itself
template <bool BIG>
__global__ __launch_bounds__(64) void upsampled_pred_kernel(const uint8_t* __restrict__ ref, const int stride, uint8_t* __restrict__ comp, const int W, const int H,
                                                            const int xq, const int yq, const int taps) {
    HIP_DYNAMIC_SHARED(uint32_t, smem)
    Geo g;
    g.W = W, g.H = H;
    g.lw   = 31 - __clz((unsigned)W);
    g.ln   = g.lw + 31 - __clz((unsigned)H);
    g.npix = W * H;
    pred_up(ref, (int64_t)stride, xq, yq, taps, g, (uint8_t*)smem, (int)threadIdx.x, [&](const int i, const int px) { comp[i] = (uint8_t)px; });
}

// ---- the search ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool subpel_desc_ok(const SvtHipMdSubpelDesc& d, const SvtHipInterPredPlanes& planes, const bool have_tables, const uint32_t n_tables) {
    if (d.bsize >= 22 || d.method > 1 || d.forced_stop > 3 || d.subpel_search_type < 1 || d.subpel_search_type > 3 || d.mv_cost_type > 5) return false;
    if (d.ref_plane >= 32 || planes.base[d.ref_plane] == nullptr) return false;
    return !have_tables || d.cost_table < 0 || (uint32_t)d.cost_table < n_tables;
}
template <bool BIG>
__global__ __launch_bounds__(BIG ? 64 : 64 * SMALL_WAVES) void md_subpel_kernel(const SvtHipInterPredPlanes planes, const uint8_t* __restrict__ src_base,
                                                                                const SvtHipMvCostTable* __restrict__ tables, const uint32_t n_tables,
                                                                                const SvtHipMdSubpelDesc* __restrict__ descs, const uint32_t n,
                                                                                SvtHipMdSubpelResult* __restrict__ out, uint8_t* __restrict__ status) {
    HIP_DYNAMIC_SHARED(uint32_t, smem)
    constexpr int  WV = BIG ? 1 : SMALL_WAVES, SRCB = BIG ? SRC_BIG : SMALL_PIX, SLICE = SRCB + (BIG ? IM_BIG : IM_SMALL);
    const int      l = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t item = blockIdx.x * WV + (uint32_t)wv;
    if (item >= n) return;
    const SvtHipMdSubpelDesc d  = descs[item];
    const bool               ok = subpel_desc_ok(d, planes, tables != nullptr, n_tables);
    if (status && !BIG && l == 0) status[item] = ok ? 0 : 1;
    if (!ok) return;
    const Geo g = geo_of(d.bsize);
    if ((g.npix > SMALL_PIX) != BIG) return;
    uint8_t*       srcl = (uint8_t*)smem + wv * SLICE;
    uint8_t*       im   = srcl + SRCB;
    const uint8_t* ref  = (const uint8_t*)planes.base[d.ref_plane] + d.ref_off;
    const int64_t  rs   = (int64_t)d.ref_stride;
    {
        const uint8_t* src = src_base + d.src_off;
        for (int i = l; i < g.npix; i += 64) srcl[i] = (uint8_t)load_px(src + (uint32_t)(i >> g.lw) * d.src_stride + (uint32_t)(i & (g.W - 1)));
        __builtin_amdgcn_wave_barrier();
    }
    const SvtHipMvCostTable* tab = (tables != nullptr && d.cost_table >= 0) ? tables + d.cost_table : nullptr;
    // svt_mv_err_cost (mcomp.c:44): the difference and its magnitudes are MVs, i.e. int16_t
    const auto mv_cost = [&](const int16_t r, const int16_t c) -> int {
        const int16_t dr = (int16_t)(r - d.ref_mv_row), dc = (int16_t)(c - d.ref_mv_col);
        const int     ad = (int)(int16_t)(dr < 0 ? -dr : dr) + (int)(int16_t)(dc < 0 ? -dc : dc);
        switch (d.mv_cost_type) {
        case 0: { // MV_COST_ENTROPY
            if (!tab) return 0;
            const int  j  = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3); // svt_av1_get_mv_joint
            const auto at = [](const int v) {
                const int k = MV_MAX_ + (v < -MV_UPP_ ? -MV_UPP_ : (v > MV_UPP_ ? MV_UPP_ : v));
                return k < 0 ? 0 : (k > SVT_HIP_MV_VALS - 1 ? SVT_HIP_MV_VALS - 1 : k);
            };
            const int rate = (int)((uint32_t)tab->joint[j] + (uint32_t)tab->comp[0][at(dr)] + (uint32_t)tab->comp[1][at(dc)]);
            return (int)(((int64_t)rate * d.error_per_bit + 8192) >> 14); // RDDIV_BITS + AV1_PROB_COST_SHIFT - RD_EPB_SHIFT + PIXEL_TRANSFORM_ERROR_SCALE
        }
        case 1: return (2 * ad) >> 3; // SSE_LAMBDA_LOWRES
        case 2: return 0;             // SSE_LAMBDA_MIDRES 0
        case 3: return ad >> 3;       // SSE_LAMBDA_HDRES
        case 4: return (int)(((int64_t)(ad << 8) * d.error_per_bit + 8192) >> 14); // MV_COST_OPT
        default: return 0;
        }
    };
    int         sum_l;
    uint32_t    sse_l;
    const auto  acc = [&](const int i, const int px) {
        const int diff = px - (int)srcl[i];
        sum_l += diff;
        sse_l += (uint32_t)(diff * diff);
    };
    const auto at_mv = [&](const int16_t r, const int16_t c) { return ref + (int64_t)(r >> 3) * rs + (c >> 3); }; // svt_get_buf_from_mv
    const auto finish = [&](uint32_t& sse) {
        const int sum = wave_sum(sum_l);
        sse           = (uint32_t)wave_sum((int)sse_l);
        return variance_of(sse, sum, g.ln);
    };

    int16_t  br = d.start_mv_row, bc = d.start_mv_col;
    uint32_t sse1 = 0, evals = 1, sse;
    // svt_upsampled_setup_center_error: vf at the full-pel position
    sum_l = 0, sse_l = 0;
    pred_full(at_mv(br, bc), rs, g, l, acc);
    int            distortion = (int)finish(sse);
    uint32_t       besterr    = (uint32_t)distortion + (uint32_t)mv_cost(br, bc);
    const uint32_t fp_me_dist = besterr;
    const bool     pruned     = d.method != 0;
    int            round      = std::min(3 - (int)d.forced_stop, 3 - (d.allow_hp ? 0 : 1));
    if (!pruned && d.mvp_th > 0) { // mcomp.c:712-726
        const int mvp_err = (int)(d.best_mvp_err + 1u), me_err = (int)(besterr + 1u);
        const int dev     = me_err != 0 ? (int)(((int64_t)(me_err - mvp_err) * 100) / me_err) : 0;
        if (dev >= (int)d.mvp_th) round = 1;
        else if (abs((int)bc - (int)d.best_mvp_col) > d.hp_mv_th || abs((int)br - (int)d.best_mvp_row) > d.hp_mv_th) round = std::min(round, 2);
    }
    bool go = !d.early_exit;
    // the variance of the full-pel prediction against the constant 128 of svt_aom_eb_av1_var_offs
    const auto low_variance = [&]() {
        sum_l = 0, sse_l = 0;
        pred_full(at_mv(br, bc), rs, g, l, [&](const int, const int px) {
            const int diff = px - 128;
            sum_l += diff;
            sse_l += (uint32_t)(diff * diff);
        });
        uint32_t       s;
        const uint32_t var = finish(s);
        return (int)((var + ((1u << g.ln) >> 1)) >> g.ln) < d.pred_variance_th;
    };
    const auto below_abs_th = [&](const int shift) { // the product in int, compared as uint64_t
        const int32_t th = (int32_t)((uint32_t)(g.npix >> shift) * (uint32_t)d.abs_th_mult * (uint32_t)(d.qp >> 1));
        return (uint64_t)besterr < (uint64_t)(int64_t)th;
    };
    uint32_t org_error = 0;
    if (go) {
        if (!pruned) {
            if (low_variance() || below_abs_th(2) || !round) go = false;
        } else {
            if (below_abs_th(3) || !round || low_variance()) go = false;
            else if (d.skip_diag_refinement < 4) {
                const uint32_t demo = d.skip_diag_refinement >= 2 ? ((g.W >= 64 || g.H >= 64) ? 2u : 1u) : 1u;
                org_error           = d.skip_diag_refinement ? besterr / demo : 0x7fffffffu;
            }
        }
    }
    int hstep = 4; // INIT_SUBPEL_STEP_SIZE
#pragma unroll 1
    for (int iter = 0; go && iter < round; iter++) {
        const int      tr = br, tc = bc; // the iteration's centre: *bestmv at its start in both methods
        const uint32_t prev_besterr = besterr;
        uint32_t       c_left = 0, c_right = 0, c_up = 0, c_down = 0;
        int            dsr = 0, dsc = 0, b0r = 0, b0c = 0, second = 0, better = 0;
#pragma unroll 1
        for (int step = 0; step < 8; step++) {
            int cr, cc;
            if (step < 4) cr = tr + (step == 2 ? -hstep : (step == 3 ? hstep : 0)), cc = tc + (step == 0 ? -hstep : (step == 1 ? hstep : 0));
            else if (step == 4) { // svt_get_best_diag_step
                dsr = c_up <= c_down ? -hstep : hstep, dsc = c_left <= c_right ? -hstep : hstep;
                cr = tr + dsr, cc = tc + dsc;
                if (pruned && besterr >= org_error) continue; // first_level_check_fast returns before the diagonal
            } else {
                if (step == 5) {
                    b0r = br, b0c = bc, better = 0;
                    if (d.iters_per_step <= 1) break;
                    if (!pruned) { // svt_second_level_check_v2
                        if (tr == br && tc == bc) break;
                        if (tr == br) dsr = (int16_t)-dsr;
                        else if (tc == bc) dsc = (int16_t)-dsc;
                        second = 1;
                    } else { // second_level_check_fast
                        if (!(besterr < org_error)) break;
                        if (tr != br && tc != bc) second = 2;
                        else if (tr == br && tc != bc) second = 3;
                        else if (tr != br && tc == bc) second = 4;
                        else break;
                    }
                }
                const int k = step - 5;
                if (second == 1) {
                    if (k == 2 && !better) break;
                    cr = b0r + (k != 1 ? dsr : 0), cc = b0c + (k != 0 ? dsc : 0);
                } else if (second == 2) {
                    if (k == 2) break;
                    cr = b0r + (k == 1 ? dsr : 0), cc = b0c + (k == 0 ? dsc : 0);
                } else if (second == 3) cr = b0r + (k == 0 ? hstep : (k == 1 ? -hstep : -dsr)), cc = b0c + (k == 2 ? 0 : dsc);
                else cr = b0r + (k == 2 ? 0 : dsr), cc = b0c + (k == 0 ? hstep : (k == 1 ? -hstep : -dsc));
            }
            // svt_check_better / svt_check_better_fast
            const int16_t r = (int16_t)cr, c = (int16_t)cc;
            uint32_t      cost;
            if (c >= d.lim_col_min && c <= d.lim_col_max && r >= d.lim_row_min && r <= d.lim_row_max) {
                cost      = (uint32_t)mv_cost(r, c);
                bool skip = false;
                if (pruned && d.mv_cost_type == 4) { // :194-198
                    const int64_t bestcost = (int64_t)(uint32_t)((uint32_t)distortion + cost);
                    if (bestcost > ((int64_t)besterr * (int64_t)d.early_exit_th) / 1000) cost = (uint32_t)bestcost, skip = true;
                }
                if (!skip) {
                    sum_l = 0, sse_l = 0;
                    if (pruned) pred_bil(at_mv(r, c), rs, c & 7, r & 7, g, l, acc);
                    else pred_up(at_mv(r, c), rs, c & 7, r & 7, d.subpel_search_type, g, im, l, acc);
                    const uint32_t mse = finish(sse);
                    evals++;
                    cost += mse;
                    const bool fp = d.bias_fp && (bc & 7) == 0 && (br & 7) == 0;
                    if (fp ? ((uint64_t)cost * (uint64_t)(int64_t)d.bias_fp) / 100 < (uint64_t)besterr : cost < besterr) {
                        besterr = cost, br = r, bc = c, distortion = (int)mse, sse1 = sse, better = 1;
                    }
                }
            } else cost = 0x7fffffffu; // INT_MAX
            if (step == 0) c_left = cost;
            else if (step == 1) c_right = cost;
            else if (step == 2) c_up = cost;
            else if (step == 3) c_down = cost;
        }
        hstep >>= 1;
        if (pruned) {
            if (d.skip_diag_refinement && iter < 1) org_error = std::min(org_error, besterr); // iter < QUARTER_PEL
            const int64_t pb  = (int64_t)std::max(prev_besterr, 1u);
            const int32_t dev = (int32_t)((((int64_t)std::max(besterr, 1u) - pb) * 100) / pb);
            if (dev >= d.round_dev_th) break;
        }
    }
    if (l == 0) {
        SvtHipMdSubpelResult r;
        r.mv_row = br, r.mv_col = bc, r.besterr = besterr, r.distortion = distortion, r.sse1 = sse1, r.fp_me_dist = fp_me_dist, r.evals = evals;
        out[item] = r;
    }
}
__global__ __launch_bounds__(256) void md_subpel_check_kernel(const SvtHipInterPredPlanes planes, const bool have_tables, const uint32_t n_tables,
                                                              const SvtHipMdSubpelDesc* __restrict__ descs, const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) bad |= !subpel_desc_ok(descs[i], planes, have_tables, n_tables);
    if (bad) *bad_out = 1;
}

// ---- OBMC motion refinement ------------------------------------------------------------------------------------------------------------
// obmc_mask_1 .. obmc_mask_32 (inter_prediction.c:2407-2417) back to back: the mask of length n starts at n - 1 (svt_av1_get_obmc_mask)
__device__ constexpr uint8_t kObmcMask[63] = {64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,
                                              33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr int NB_SMALL = 2048; // bytes of one neighbour prediction's overlap region in LDS: W * ovA resp. H * ovL <= npix / 2
constexpr int NB_BIG   = 4096; // 128 x 32
constexpr int OBMC_WEIGHTS   = 256;  // the two 1-D weight rows of a derived target: up to 128 bytes each
constexpr int OBMC_LDS_SMALL = SMALL_WAVES * (SMALL_PIX + 2 * NB_SMALL + OBMC_WEIGHTS + IM_SMALL); // 52 224 B per workgroup of four waves
constexpr int OBMC_LDS_BIG   = SRC_BIG + 2 * NB_BIG + OBMC_WEIGHTS + IM_BIG;                       // 42 240 B per one-wave workgroup

// the spans of SvtHipObmcWsrcDesc / SvtHipObmcSearchDesc (same member names)
template <typename D> __device__ __forceinline__ bool obmc_spans_ok(const D& d, const SvtHipInterPredPlanes& planes) {
    if (d.bsize >= 22 || kBw[d.bsize] < 8 || kBh[d.bsize] < 8) return false;
    if (d.n_above > SVT_HIP_OBMC_MAX_SPANS || d.n_left > SVT_HIP_OBMC_MAX_SPANS || d.above_plane >= 32 || d.left_plane >= 32) return false;
    const int n4w = kBw[d.bsize] >> 2, n4h = kBh[d.bsize] >> 2;
#pragma unroll
    for (int k = 0; k < SVT_HIP_OBMC_MAX_SPANS; k++) {
        if (k < d.n_above && (d.above_len[k] == 0 || (int)d.above_rel[k] + (int)d.above_len[k] > n4w)) return false;
        if (k < d.n_left && (d.left_len[k] == 0 || (int)d.left_rel[k] + (int)d.left_len[k] > n4h)) return false;
    }
    if (d.up_available && d.n_above && planes.base[d.above_plane] == nullptr) return false;
    if (d.left_available && d.n_left && planes.base[d.left_plane] == nullptr) return false;
    return true;
}
struct ObmcSides {
    uint32_t amask, lmask; // bit m: mi column / row m of the block lies in an above / left span of an available side
    int      ovA, ovL;
};
template <typename D> __device__ __forceinline__ ObmcSides obmc_sides(const D& d, const int W, const int H) {
    ObmcSides s;
    s.amask = s.lmask = 0;
    s.ovA = std::min(H, 64) >> 1, s.ovL = std::min(W, 64) >> 1;
#pragma unroll
    for (int k = 0; k < SVT_HIP_OBMC_MAX_SPANS; k++) {
        if (d.up_available && k < d.n_above) s.amask |= (uint32_t)((1ull << d.above_len[k]) - 1ull) << d.above_rel[k];
        if (d.left_available && k < d.n_left) s.lmask |= (uint32_t)((1ull << d.left_len[k]) - 1ull) << d.left_rel[k];
    }
    return s;
}
// calc_target_weighted_pred (enc_inter_prediction.c:1756) for one pixel: the above callback (:1581), both times 64, the left callback (:1610), the source
__device__ __forceinline__ void obmc_target(const int s, const int a, const int lf, const bool in_a, const bool in_l, const int mv, const int mh, int& w, int& k) {
    w = 0, k = 64;
    if (in_a) w = (64 - mv) * a, k = mv;
    w *= 64, k *= 64;
    if (in_l) w = (w >> 6) * mh + (lf << 6) * (64 - mh), k = (k >> 6) * mh;
    w = s * 4096 - w;
}
// one workgroup per item, its 256 threads split the pixels; every pixel is independent
__global__ __launch_bounds__(256) void obmc_wsrc_kernel(const SvtHipInterPredPlanes planes, const uint8_t* __restrict__ src_base, const SvtHipObmcWsrcDesc* __restrict__ descs,
                                                        const uint32_t n, int32_t* __restrict__ wsrc_out, int32_t* __restrict__ mask_out, uint8_t* __restrict__ status) {
    const uint32_t item = blockIdx.x;
    if (item >= n) return;
    const SvtHipObmcWsrcDesc d  = descs[item];
    const bool               ok = obmc_spans_ok(d, planes);
    if (status && threadIdx.x == 0) status[item] = ok ? 0 : 1;
    if (!ok) return;
    const Geo       g  = geo_of(d.bsize);
    const ObmcSides sd = obmc_sides(d, g.W, g.H);
    const uint8_t*  src   = src_base + d.src_off;
    const uint8_t*  above = (const uint8_t*)planes.base[d.above_plane] + d.above_off;
    const uint8_t*  left  = (const uint8_t*)planes.base[d.left_plane] + d.left_off;
    int32_t*        ow = wsrc_out + d.out_off;
    int32_t*        om = mask_out + d.out_off;
    for (int i = (int)threadIdx.x; i < g.npix; i += 256) {
        const int  row = i >> g.lw, col = i & (g.W - 1);
        const bool in_a = row < sd.ovA && ((sd.amask >> (col >> 2)) & 1u), in_l = col < sd.ovL && ((sd.lmask >> (row >> 2)) & 1u);
        const int  a  = in_a ? load_px(above + (uint32_t)row * d.above_stride + (uint32_t)col) : 0;
        const int  lf = in_l ? load_px(left + (uint32_t)row * d.left_stride + (uint32_t)col) : 0;
        int        w, k;
        obmc_target(load_px(src + (uint32_t)row * d.src_stride + (uint32_t)col), a, lf, in_a, in_l, in_a ? kObmcMask[sd.ovA - 1 + row] : 0,
                    in_l ? kObmcMask[sd.ovL - 1 + col] : 0, w, k);
        ow[i] = w, om[i] = k;
    }
}
__global__ __launch_bounds__(256) void obmc_wsrc_check_kernel(const SvtHipInterPredPlanes planes, const SvtHipObmcWsrcDesc* __restrict__ descs, const uint32_t n,
                                                              uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) bad |= !obmc_spans_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

__device__ __forceinline__ bool obmc_search_desc_ok(const SvtHipObmcSearchDesc& d, const SvtHipInterPredPlanes& planes, const bool have_src, const bool have_arrays,
                                                    const bool have_tables, const uint32_t n_tables) {
    if (d.bsize >= 22 || kBw[d.bsize] < 8 || kBh[d.bsize] < 8) return false;
    if (d.target_form > SVT_HIP_OBMC_TARGET_DERIVED || d.subpel_search_type > 3 || d.forced_stop > 3 || d.fpel_search_range > 64) return false;
    if (d.ref_plane >= 32 || planes.base[d.ref_plane] == nullptr) return false;
    if (have_tables && d.cost_table >= 0 && (uint32_t)d.cost_table >= n_tables) return false;
    if (d.target_form == SVT_HIP_OBMC_TARGET_ARRAYS) return have_arrays;
    return have_src && obmc_spans_ok(d, planes);
}
// One wave per item, as md_subpel_kernel: candidates in the C's order, one after the other and wave-uniform; the lanes split the pixels; every decision is scalar.
// ARRAYS: wsrc / mask are re-read from memory (L2) by every candidate, as block_var_kernel reads them -- 8 bytes per pixel do not fit the wave's LDS share at the
// sizes that matter.  DERIVED: the source block and the two overlap regions sit in the wave's LDS slice as bytes and a pixel's (wsrc, mask) is recomputed from them
// wherever it is used.  The slice: source | above overlap (pitch W) | left overlap (pitch ovL) | the two 1-D weight rows | the intermediate of pred_up.
template <bool BIG>
__global__ __launch_bounds__(BIG ? 64 : 64 * SMALL_WAVES) void obmc_search_kernel(const SvtHipInterPredPlanes planes, const uint8_t* __restrict__ src_base,
                                                                                  const int32_t* __restrict__ wsrc_base, const int32_t* __restrict__ mask_base,
                                                                                  const SvtHipMvCostTable* __restrict__ tables, const uint32_t n_tables,
                                                                                  const SvtHipObmcSearchDesc* __restrict__ descs, const uint32_t n,
                                                                                  SvtHipObmcSearchResult* __restrict__ out, uint8_t* __restrict__ status) {
    HIP_DYNAMIC_SHARED(uint32_t, smem)
    constexpr int  WV = BIG ? 1 : SMALL_WAVES, SRCB = BIG ? SRC_BIG : SMALL_PIX, NBB = BIG ? NB_BIG : NB_SMALL, SLICE = SRCB + 2 * NBB + OBMC_WEIGHTS + (BIG ? IM_BIG : IM_SMALL);
    const int      l = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t item = blockIdx.x * WV + (uint32_t)wv;
    if (item >= n) return;
    const SvtHipObmcSearchDesc d  = descs[item];
    const bool                 ok = obmc_search_desc_ok(d, planes, src_base != nullptr, wsrc_base != nullptr && mask_base != nullptr, tables != nullptr, n_tables);
    if (status && !BIG && l == 0) status[item] = ok ? 0 : 1;
    if (!ok) return;
    const Geo g = geo_of(d.bsize);
    if ((g.npix > SMALL_PIX) != BIG) return;
    uint8_t*       srcl = (uint8_t*)smem + wv * SLICE;
    uint8_t*       abv  = srcl + SRCB;
    uint8_t*       lft  = abv + NBB;
    uint8_t*       wrow = lft + NBB; // Mv[row], 64 from row ovA on
    uint8_t*       wcol = wrow + OBMC_WEIGHTS / 2; // Mh[col], 64 from column ovL on
    uint8_t*       im   = wcol + OBMC_WEIGHTS / 2;
    const uint8_t* ref  = (const uint8_t*)planes.base[d.ref_plane] + d.ref_off;
    const int64_t  rs   = (int64_t)d.ref_stride;
    const bool     derived = d.target_form == SVT_HIP_OBMC_TARGET_DERIVED;
    const int32_t* ws   = wsrc_base + (derived ? 0 : d.wsrc_off);
    const int32_t* mk   = mask_base + (derived ? 0 : d.mask_off);
    ObmcSides      sd;
    sd.amask = sd.lmask = 0, sd.ovA = sd.ovL = 0;
    if (derived) {
        sd = obmc_sides(d, g.W, g.H);
        const uint8_t* src = src_base + d.src_off;
        for (int i = l; i < g.npix; i += 64) srcl[i] = (uint8_t)load_px(src + (uint32_t)(i >> g.lw) * d.src_stride + (uint32_t)(i & (g.W - 1)));
        for (int i = l; i < g.H; i += 64) wrow[i] = i < sd.ovA ? kObmcMask[sd.ovA - 1 + i] : (uint8_t)64;
        for (int i = l; i < g.W; i += 64) wcol[i] = i < sd.ovL ? kObmcMask[sd.ovL - 1 + i] : (uint8_t)64;
        if (sd.amask) {
            const uint8_t* above = (const uint8_t*)planes.base[d.above_plane] + d.above_off;
            for (int i = l; i < g.W * sd.ovA; i += 64) {
                const int row = i >> g.lw, col = i & (g.W - 1);
                if ((sd.amask >> (col >> 2)) & 1u) abv[i] = (uint8_t)load_px(above + (uint32_t)row * d.above_stride + (uint32_t)col);
            }
        }
        if (sd.lmask) {
            const uint8_t* left = (const uint8_t*)planes.base[d.left_plane] + d.left_off;
            const int      lo   = 31 - __clz((unsigned)sd.ovL);
            for (int i = l; i < g.H * sd.ovL; i += 64) {
                const int row = i >> lo, col = i & (sd.ovL - 1);
                if ((sd.lmask >> (row >> 2)) & 1u) lft[i] = (uint8_t)load_px(left + (uint32_t)row * d.left_stride + (uint32_t)col);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    const SvtHipMvCostTable* tab = (tables != nullptr && d.cost_table >= 0) ? tables + d.cost_table : nullptr;
    const int                rr = d.ref_mv_row, rc = d.ref_mv_col;
    // svt_mv_cost on a difference that is an MV, i.e. int16_t
    const auto tab_cost = [&](const int16_t dr, const int16_t dc) -> int {
        const int  j  = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3); // svt_av1_get_mv_joint
        const auto at = [](const int v) {
            const int k = MV_MAX_ + (v < -MV_UPP_ ? -MV_UPP_ : (v > MV_UPP_ ? MV_UPP_ : v));
            return k < 0 ? 0 : (k > SVT_HIP_MV_VALS - 1 ? SVT_HIP_MV_VALS - 1 : k);
        };
        return (int)((uint32_t)tab->joint[j] + (uint32_t)tab->comp[0][at(dr)] + (uint32_t)tab->comp[1][at(dc)]);
    };
    const auto light = [](const int a, const int b) { return 1296u + 50u * ((uint32_t)a + (uint32_t)b); };
    const int  fcr = rr >> 3, fcc = rc >> 3; // fcenter_mv
    const auto sad_cost = [&](const int r, const int c) -> uint32_t { // mvsad_err_cost (av1me.c:254), full-pel vectors
        if (d.approx_inter_rate) return light(abs(c - fcc) * 8, abs(r - fcr) * 8);
        if (!tab) return 0;
        return ((uint32_t)tab_cost((int16_t)((r - fcr) * 8), (int16_t)((c - fcc) * 8)) * (uint32_t)d.sad_per_bit + 256u) >> 9;
    };
    const auto err_cost = [&](const int16_t r, const int16_t c) -> uint32_t { // svt_aom_mv_err_cost / _light (av1me.c:229, :244)
        if (d.approx_inter_rate) return light(abs((int)c - rc), abs((int)r - rr));
        if (!tab) return 0;
        return (uint32_t)(int)(((int64_t)tab_cost((int16_t)(r - rr), (int16_t)(c - rc)) * d.error_per_bit + 8192) >> 14);
    };
    int        sum_l;
    uint32_t   sse_l, sad_l;
    // pixel i's (wsrc, mask).  Derived: the closed form of obmc_target without a branch -- a stage that does not apply has the weight 64, under which its neighbour
    // sample (whatever byte of the slice the index then names) is multiplied by 0: w = (64 - ka) * above * kl + (left << 6) * (64 - kl), k = ka * kl.
    const auto target = [&](const int i, int& w, int& k) {
        if (derived) {
            const int row = i >> g.lw, col = i & (g.W - 1);
            const int ka = ((sd.amask >> (col >> 2)) & 1u) ? (int)wrow[row] : 64, kl = ((sd.lmask >> (row >> 2)) & 1u) ? (int)wcol[col] : 64;
            w = (int)srcl[i] * 4096 - ((64 - ka) * (int)abv[i] * kl + ((int)lft[row * sd.ovL + col] << 6) * (64 - kl));
            k = ka * kl;
        } else w = ws[i], k = mk[i];
    };
    const auto acc = [&](const int i, const int px) { // obmc_variance (variance.c:347) / obmc_sad (sad_av1.c:18), as block_var_kernel
        int w, k;
        target(i, w, k);
        const int      v = (int)((uint32_t)w - (uint32_t)px * (uint32_t)k);
        const uint32_t r = ((v < 0 ? 0u - (uint32_t)v : (uint32_t)v) + 2048u) >> 12;
        sad_l += r;
        sum_l += v < 0 ? -(int)r : (int)r;
        sse_l += r * r;
    };
    const auto reset = [&]() { sum_l = 0, sse_l = 0, sad_l = 0; };
    const auto finish = [&](uint32_t& sse) {
        const int sum = wave_sum(sum_l);
        sse           = (uint32_t)wave_sum((int)sse_l);
        return variance_of(sse, sum, g.ln);
    };
    const auto at_fp = [&](const int r, const int c) { return ref + (int64_t)r * rs + c; }; // get_buf_from_mv

    int16_t  fr = (int16_t)(d.best_pred_mv_row >> 3), fc = (int16_t)(d.best_pred_mv_col >> 3);
    uint32_t evals = 0, fp_rounds = 0, sse;
    int      thissme = 0;
    if (d.do_full_refine) {
        // svt_av1_set_mv_search_range (av1me.c:205) on a copy of the limits: MAX_FULL_PEL_VAL 1023
        const int cmin = std::max(d.lim_col_min, std::max((rc >> 3) - 1023 + ((rc & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1));
        const int rmin = std::max(d.lim_row_min, std::max((rr >> 3) - 1023 + ((rr & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1));
        const int cmax = std::min(d.lim_col_max, std::min((rc >> 3) + 1023, (MV_UPP_ >> 3) - 1));
        const int rmax = std::min(d.lim_row_max, std::min((rr >> 3) + 1023, (MV_UPP_ >> 3) - 1));
        fc = (int16_t)((int)fc < cmin ? cmin : ((int)fc > cmax ? cmax : (int)fc)); // clamp_mv
        fr = (int16_t)((int)fr < rmin ? rmin : ((int)fr > rmax ? rmax : (int)fr));
        // obmc_refining_search_sad (av1me.c:721).  The neighbours of a round, {-1,0} {0,-1} {0,1} {1,0} {-1,1} {1,1} {1,-1} {-1,-1}, are independent given the running
        // best: their SADs come from ONE pass over the pixels -- a pixel's (wsrc, mask) is fetched or derived once and meets up to eight samples of the
        // (W + 2) x (H + 2) window around the centre -- and the C's decisions then run over the eight sums in its order.  A neighbour is_mv_in rejects is not read.
        constexpr int NR[8] = {-1, 0, 0, 1, -1, 1, 1, -1}, NC[8] = {0, -1, 1, 0, 1, 1, -1, -1};
        reset();
        pred_full(at_fp(fr, fc), rs, g, l, acc);
        evals++;
        uint32_t  best_sad = (uint32_t)wave_sum((int)sad_l) + sad_cost(fr, fc);
        const int nn = d.fpel_search_diag ? 8 : 4;
#pragma unroll 1
        for (int i = 0; i < (int)d.fpel_search_range; i++) {
            uint32_t in = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int16_t r = (int16_t)(fr + NR[j]), c = (int16_t)(fc + NC[j]);
                if (j < nn && c >= cmin && c <= cmax && r >= rmin && r <= rmax) in |= 1u << j; // is_mv_in
            }
            uint32_t       sads[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const uint8_t* ctr     = at_fp(fr, fc);
            for (int px = l; px < g.npix; px += 64) {
                int w, k;
                target(px, w, k);
                const uint8_t* q = ctr + (int64_t)(px >> g.lw) * rs + (px & (g.W - 1));
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (in & (1u << j)) {
                        const int v = (int)((uint32_t)w - (uint32_t)load_px(q + NR[j] * rs + NC[j]) * (uint32_t)k);
                        sads[j] += ((v < 0 ? 0u - (uint32_t)v : (uint32_t)v) + 2048u) >> 12;
                    }
            }
            int best_site = -1;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (in & (1u << j)) {
                    uint32_t sad = (uint32_t)wave_sum((int)sads[j]);
                    evals++;
                    if (sad < best_sad) {
                        sad += sad_cost((int16_t)(fr + NR[j]), (int16_t)(fc + NC[j]));
                        if (sad < best_sad) best_sad = sad, best_site = j;
                    }
                }
            if (best_site == -1) break;
            fr = (int16_t)(fr + ((0x2894 >> (2 * best_site)) & 3) - 1), fc = (int16_t)(fc + ((0xA61 >> (2 * best_site)) & 3) - 1); // NR / NC as 2-bit fields, value + 1
            fp_rounds++;
        }
        thissme = (int)best_sad;
        if (thissme < 0x7fffffff) { // get_obmc_mvpred_var
            reset();
            pred_full(at_fp(fr, fc), rs, g, l, acc);
            evals++;
            thissme = (int)(finish(sse) + err_cost((int16_t)(fr * 8), (int16_t)(fc * 8)));
        }
    }
    int      br = fr * 8, bc = fc * 8;
    uint32_t besterr = 0, sse1 = 0;
    int      distortion = 0;
    if (d.do_frac_refine) { // svt_av1_find_best_obmc_sub_pixel_tree_up (av1me.c:963)
        const int max_mv = 8 * 1023; // set_subpel_mv_search_range on the un-narrowed limits
        const int minc = std::max(-MV_UPP_ + 1, std::max(d.lim_col_min * 8, rc - max_mv)), maxc = std::min(MV_UPP_ - 1, std::min(d.lim_col_max * 8, rc + max_mv));
        const int minr = std::max(-MV_UPP_ + 1, std::max(d.lim_row_min * 8, rr - max_mv)), maxr = std::min(MV_UPP_ - 1, std::min(d.lim_row_max * 8, rr + max_mv));
        int       round = 3 - (int)d.forced_stop;
        if (!d.allow_hp && round == 3) round = 2;
        reset();
        pred_full(at_fp(fr, fc), rs, g, l, acc); // either centre form: the upsampled prediction at offset 0, 0 is the copy
        evals++;
        besterr    = finish(sse1);
        distortion = (int)besterr;
        besterr += err_cost((int16_t)(fr * 8), (int16_t)(fc * 8));
        int hstep = 4;
#pragma unroll 1
        for (int iter = 0; iter < round; iter++) {
            const int r0 = br, c0 = bc;
            uint32_t  c_left = 0, c_right = 0, c_up = 0, c_down = 0;
            int       best_idx = -1, kr = 0, kc = 0, tr = 0, tc = 0, br0 = 0, bc0 = 0;
            const auto ax_r = [&](const int s) { return s == 2 ? -hstep : (s == 3 ? hstep : 0); }; // search_step_table: left, right, up, down
            const auto ax_c = [&](const int s) { return s == 0 ? -hstep : (s == 1 ? hstep : 0); };
#pragma unroll 1
            for (int step = 0; step < 8; step++) {
                int r, c;
                if (step < 4) r = r0 + ax_r(step), c = c0 + ax_c(step);
                else if (step == 4) {
                    kc = c_left <= c_right ? -hstep : hstep, kr = c_up <= c_down ? -hstep : hstep;
                    tc = c0 + kc, tr = r0 + kr;
                    r = tr, c = tc;
                } else {
                    if (step == 5) {
                        if (best_idx >= 0 && best_idx < 4) br = r0 + ax_r(best_idx), bc = c0 + ax_c(best_idx);
                        else if (best_idx == 4) br = tr, bc = tc;
                        if (!(d.iters_per_step > 1 && best_idx != -1)) break;
                        // SECOND_LEVEL_CHECKS_BEST
                        if (tr == br && tc != bc) kc = bc - tc;
                        else if (tr != br && tc == bc) kr = br - tr;
                        br0 = br, bc0 = bc;
                        r = br0 + kr, c = bc0;
                    } else if (step == 6) r = br0, c = bc0 + kc;
                    else {
                        if (br0 == br && bc0 == bc) break;
                        r = br0 + kr, c = bc0 + kc;
                    }
                }
                if (c >= minc && c <= maxc && r >= minr && r <= maxr) {
                    reset();
                    const uint8_t* p = ref + (int64_t)(r >> 3) * rs + (c >> 3);
                    if (d.subpel_search_type == 0) pred_bil(p, rs, c & 7, r & 7, g, l, acc);
                    else pred_up(p, rs, c & 7, r & 7, d.subpel_search_type, g, im, l, acc);
                    const uint32_t thismse = finish(sse);
                    evals++;
                    const uint32_t tot = err_cost((int16_t)r, (int16_t)c) + thismse;
                    if (tot < besterr) {
                        besterr = tot, distortion = (int)thismse, sse1 = sse;
                        if (step < 5) best_idx = step;
                        else br = r, bc = c;
                    }
                    if (step == 0) c_left = tot;
                    else if (step == 1) c_right = tot;
                    else if (step == 2) c_up = tot;
                    else if (step == 3) c_down = tot;
                } else if (step == 0) c_left = 0x7fffffffu; // INT_MAX
                else if (step == 1) c_right = 0x7fffffffu;
                else if (step == 2) c_up = 0x7fffffffu;
                else if (step == 3) c_down = 0x7fffffffu;
            }
            hstep >>= 1;
        }
    }
    if (l == 0) {
        const int16_t mr = (int16_t)br, mc = (int16_t)bc;
        int           rate;
        if (d.approx_inter_rate) rate = (int)light(abs((int)mc - rc), abs((int)mr - rr)); // svt_av1_mv_bit_cost_light
        else if (!tab) rate = 0;
        else { // svt_av1_mv_bit_cost, MV_COST_WEIGHT 108
            const int16_t dr = (int16_t)(mr - rr), dc = (int16_t)(mc - rc);
            rate             = (int)((uint32_t)tab_cost(dr, dc) * 108u + 64u) >> 7;
        }
        SvtHipObmcSearchResult r;
        r.mv_row = mr, r.mv_col = mc, r.fp_row = fr, r.fp_col = fc, r.thissme = thissme, r.besterr = besterr, r.distortion = distortion, r.sse1 = sse1, r.rate_mv = rate;
        r.fp_rounds = fp_rounds, r.evals = evals;
        out[item] = r;
    }
}
__global__ __launch_bounds__(256) void obmc_search_check_kernel(const SvtHipInterPredPlanes planes, const bool have_src, const bool have_arrays, const bool have_tables,
                                                                const uint32_t n_tables, const SvtHipObmcSearchDesc* __restrict__ descs, const uint32_t n,
                                                                uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) bad |= !obmc_search_desc_ok(descs[i], planes, have_src, have_arrays, have_tables, n_tables);
    if (bad) *bad_out = 1;
}

// descriptors the host cannot read: one word says whether any is invalid (the contract of svt_hip_inter_pred_batch)
template <typename F> bool any_invalid(const uint32_t n, hipStream_t st, F&& launch_check) {
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    c.reserve(0, 256);
    uint32_t* bad = (uint32_t*)c.palloc(64);
    *bad          = 0;
    launch_check(dim3(n < 1024u * 256u ? (n + 255) / 256 : 1024u), bad);
    SVT_LAUNCH_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    return *(volatile uint32_t*)bad != 0;
}

// ---- the single-call forms --------------------------------------------------------------------------------------------------------------------------
constexpr uint8_t hBw[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64}; // block_size_wide / high for host code
constexpr uint8_t hBh[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};
constexpr int     bsize_of(const int w, const int h) {
    for (int b = 0; b < 22; b++)
        if (hBw[b] == w && hBh[b] == h) return b;
    return -1;
}
// One block from host memory: exactly the rectangle of `pre` the kernel reads goes into the call's arena with the source block or the two OBMC arrays, one
// descriptor, one launch, one synchronisation (the download); nothing of the caller's is written before it.  Returns false when nothing was computed.
bool var_host(const int kind, const int bsize, const uint8_t* pre, const int pre_stride, const int xo, const int yo, const uint8_t* src, const int src_stride,
              const int32_t* wsrc, const int32_t* mask, SvtHipBlockVarResult* res) {
    const bool obmc = kind >= SVT_HIP_VAR_OBMC_SAD;
    if (!pre || (obmc ? (!wsrc || !mask) : !src) || xo < 0 || xo > 7 || yo < 0 || yo > 7) return false;
    const size_t W = hBw[bsize], H = hBh[bsize], rw = W + (xo ? 1 : 0), rh = H + (yo ? 1 : 0), blk = W * H;
    const size_t bytes = rw * rh + (obmc ? blk * 8 : blk) + sizeof(SvtHipBlockVarDesc) + sizeof(SvtHipBlockVarResult) + 4096;
    svthip::HostCall& c = svthip::host_call();
    if (bytes <= 16384) c.begin_small();
    else c.begin();
    c.reserve(bytes, bytes);
    uint8_t*              dp = (uint8_t*)c.dalloc(rw * rh);
    uint8_t*              ds = obmc ? nullptr : (uint8_t*)c.dalloc(blk);
    int32_t*              dw = obmc ? (int32_t*)c.dalloc(blk * 4) : nullptr;
    int32_t*              dm = obmc ? (int32_t*)c.dalloc(blk * 4) : nullptr;
    SvtHipBlockVarDesc*   dd = (SvtHipBlockVarDesc*)c.dalloc(sizeof(SvtHipBlockVarDesc));
    SvtHipBlockVarResult* dr = (SvtHipBlockVarResult*)c.dalloc(sizeof(SvtHipBlockVarResult));
    c.up2d(dp, rw, pre, (size_t)pre_stride, rw, rh);
    if (obmc) {
        c.up(dw, wsrc, blk * 4);
        c.up(dm, mask, blk * 4);
    } else c.up2d(ds, W, src, (size_t)src_stride, W, H);
    SvtHipBlockVarDesc d{};
    d.pre_stride = (uint32_t)rw, d.src_stride = (uint32_t)W;
    d.bsize = (uint8_t)bsize, d.kind = (uint8_t)kind, d.xoffset = (uint8_t)xo, d.yoffset = (uint8_t)yo;
    c.up(dd, &d, sizeof(d));
    SvtHipInterPredPlanes planes{};
    planes.base[0] = dp;
    if (blk > (size_t)SMALL_PIX)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(block_var_kernel<true>), dim3(1), dim3(64), IM_BIG, c.stream, planes, (const uint8_t*)ds, (const int32_t*)dw, (const int32_t*)dm,
                           (const SvtHipBlockVarDesc*)dd, 1u, dr, (uint8_t*)nullptr);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(block_var_kernel<false>), dim3(1), dim3(64 * SMALL_WAVES), SMALL_WAVES * IM_SMALL, c.stream, planes, (const uint8_t*)ds,
                           (const int32_t*)dw, (const int32_t*)dm, (const SvtHipBlockVarDesc*)dd, 1u, dr, (uint8_t*)nullptr);
    SVT_LAUNCH_CHECK();
    c.down(res, dr, sizeof(*res));
    return true;
}
// the value forms: 0 and *sse untouched when nothing was computed
uint32_t var_form(const int kind, const int bsize, const uint8_t* pre, const int pre_stride, const int xo, const int yo, const uint8_t* src, const int src_stride,
                  const int32_t* wsrc, const int32_t* mask, uint32_t* sse) {
    if (svthip::failed() || (kind != SVT_HIP_VAR_OBMC_SAD && !sse)) return 0;
    try {
        SvtHipBlockVarResult r;
        if (!var_host(kind, bsize, pre, pre_stride, xo, yo, src, src_stride, wsrc, mask, &r)) return 0;
        if (kind == SVT_HIP_VAR_OBMC_SAD) return r.sad;
        *sse = r.sse;
        return r.var;
    } catch (const svthip::DeviceError&) { return 0; }
}

template <typename K> void launch_classes(K&& launch, const uint32_t n) {
    launch(false, dim3((n + SMALL_WAVES - 1) / SMALL_WAVES), dim3(64 * SMALL_WAVES));
    launch(true, dim3(n), dim3(64));
}

} // namespace

extern "C" {

int svt_hip_block_var_batch(SvtHipInterPredPlanes planes, const uint8_t* src_base, const int32_t* wsrc_base, const int32_t* mask_base, const SvtHipBlockVarDesc* descs,
                            uint32_t n, SvtHipBlockVarResult* out, uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!descs || !out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st       = (hipStream_t)stream;
    const bool  have_src = src_base != nullptr, have_obmc = wsrc_base != nullptr && mask_base != nullptr;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) {
            hipLaunchKernelGGL(block_var_check_kernel, grid, dim3(256), 0, st, planes, have_src, have_obmc, descs, n, bad);
        }))
        return -1;
    launch_classes(
        [&](const bool big, const dim3 grid, const dim3 block) {
            if (big) hipLaunchKernelGGL(HIP_KERNEL_NAME(block_var_kernel<true>), grid, block, IM_BIG, st, planes, src_base, wsrc_base, mask_base, descs, n, out, status);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(block_var_kernel<false>), grid, block, SMALL_WAVES * IM_SMALL, st, planes, src_base, wsrc_base, mask_base, descs, n, out,
                                   status);
            SVT_LAUNCH_CHECK();
        },
        n);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_md_subpel_search_batch(SvtHipInterPredPlanes planes, const uint8_t* src_base, const SvtHipMvCostTable* tables, uint32_t n_tables,
                                   const SvtHipMdSubpelDesc* descs, uint32_t n, SvtHipMdSubpelResult* out, uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!src_base || !descs || !out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) {
            hipLaunchKernelGGL(md_subpel_check_kernel, grid, dim3(256), 0, st, planes, tables != nullptr, n_tables, descs, n, bad);
        }))
        return -1;
    launch_classes(
        [&](const bool big, const dim3 grid, const dim3 block) {
            if (big)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(md_subpel_kernel<true>), grid, block, SRC_BIG + IM_BIG, st, planes, src_base, tables, n_tables, descs, n, out, status);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(md_subpel_kernel<false>), grid, block, SMALL_WAVES * (SMALL_PIX + IM_SMALL), st, planes, src_base, tables, n_tables, descs,
                                   n, out, status);
            SVT_LAUNCH_CHECK();
        },
        n);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_md_subpel_mv_limits(int mi_row, int mi_col, int bsize, int mi_rows, int mi_cols, int16_t ref_mv_row, int16_t ref_mv_col, int32_t* limits) {
    if (bsize < 0 || bsize >= 22 || !limits) return -1;
    const int mi_w = hBw[bsize] >> 2, mi_h = hBh[bsize] >> 2; // mi_size_wide / high
    // md_subpel_search :2661-2664 (MI_SIZE 4, AOM_INTERP_EXTEND 4)
    int row_min = -(((mi_row + mi_h) * 4) + 4), col_min = -(((mi_col + mi_w) * 4) + 4), row_max = (mi_rows - mi_row) * 4 + 4, col_max = (mi_cols - mi_col) * 4 + 4;
    // svt_av1_set_mv_search_range (av1me.c:205): MAX_FULL_PEL_VAL 1023
    const int c_lo = std::max((ref_mv_col >> 3) - 1023 + ((ref_mv_col & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1), c_hi = std::min((ref_mv_col >> 3) + 1023, (MV_UPP_ >> 3) - 1);
    const int r_lo = std::max((ref_mv_row >> 3) - 1023 + ((ref_mv_row & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1), r_hi = std::min((ref_mv_row >> 3) + 1023, (MV_UPP_ >> 3) - 1);
    col_min = std::max(col_min, c_lo), col_max = std::min(col_max, c_hi), row_min = std::max(row_min, r_lo), row_max = std::min(row_max, r_hi);
    // svt_av1_set_subpel_mv_search_range (mcomp.h:112)
    const int max_mv = 8 * 1023;
    limits[0] = std::max(-MV_UPP_ + 1, std::max(col_min * 8, ref_mv_col - max_mv));
    limits[1] = std::min(MV_UPP_ - 1, std::min(col_max * 8, ref_mv_col + max_mv));
    limits[2] = std::max(-MV_UPP_ + 1, std::max(row_min * 8, ref_mv_row - max_mv));
    limits[3] = std::min(MV_UPP_ - 1, std::min(row_max * 8, ref_mv_row + max_mv));
    return 0;
}

int svt_hip_obmc_wsrc_batch(SvtHipInterPredPlanes planes, const uint8_t* src_base, const SvtHipObmcWsrcDesc* descs, uint32_t n, int32_t* wsrc_out, int32_t* mask_out,
                            uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!src_base || !descs || !wsrc_out || !mask_out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status &&
        any_invalid(n, st, [&](dim3 grid, uint32_t* bad) { hipLaunchKernelGGL(obmc_wsrc_check_kernel, grid, dim3(256), 0, st, planes, descs, n, bad); }))
        return -1;
    hipLaunchKernelGGL(obmc_wsrc_kernel, dim3(n), dim3(256), 0, st, planes, src_base, descs, n, wsrc_out, mask_out, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_obmc_search_batch(SvtHipInterPredPlanes planes, const uint8_t* src_base, const int32_t* wsrc_base, const int32_t* mask_base, const SvtHipMvCostTable* tables,
                              uint32_t n_tables, const SvtHipObmcSearchDesc* descs, uint32_t n, SvtHipObmcSearchResult* out, uint8_t* status, void* stream) {
    if (n == 0) return 0;
    if (!descs || !out) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st       = (hipStream_t)stream;
    const bool  have_src = src_base != nullptr, have_arrays = wsrc_base != nullptr && mask_base != nullptr;
    if (!status && any_invalid(n, st, [&](dim3 grid, uint32_t* bad) {
            hipLaunchKernelGGL(obmc_search_check_kernel, grid, dim3(256), 0, st, planes, have_src, have_arrays, tables != nullptr, n_tables, descs, n, bad);
        }))
        return -1;
    launch_classes(
        [&](const bool big, const dim3 grid, const dim3 block) {
            if (big)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(obmc_search_kernel<true>), grid, block, OBMC_LDS_BIG, st, planes, src_base, wsrc_base, mask_base, tables, n_tables, descs, n,
                                   out, status);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(obmc_search_kernel<false>), grid, block, OBMC_LDS_SMALL, st, planes, src_base, wsrc_base, mask_base, tables, n_tables, descs,
                                   n, out, status);
            SVT_LAUNCH_CHECK();
        },
        n);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_obmc_mv_limits(int mi_row, int mi_col, int bsize, int mi_rows, int mi_cols, int32_t* limits) {
    if (bsize < 0 || bsize >= 22 || !limits) return -1;
    const int mi_w = hBw[bsize] >> 2, mi_h = hBh[bsize] >> 2; // single_motion_search :2322-2327 (MI_SIZE 4, AOM_INTERP_EXTEND 4)
    limits[0] = -(((mi_col + mi_w) * 4) + 4);
    limits[1] = (mi_cols - mi_col) * 4 + 4;
    limits[2] = -(((mi_row + mi_h) * 4) + 4);
    limits[3] = (mi_rows - mi_row) * 4 + 4;
    return 0;
}

int svt_hip_obmc_refine_host(const SvtHipObmcSearchDesc* desc, const uint8_t* ref, int ref_stride, int ref_border, const int32_t* wsrc, const int32_t* mask,
                             const uint8_t* src, int src_stride, const uint8_t* above, int above_stride, const uint8_t* left, int left_stride,
                             const SvtHipMvCostTable* table, SvtHipObmcSearchResult* result) {
    if (!desc || !ref || !result || ref_border < 0) return -1;
    SvtHipObmcSearchDesc d = *desc;
    if (d.bsize >= 22 || hBw[d.bsize] < 8 || hBh[d.bsize] < 8 || d.target_form > SVT_HIP_OBMC_TARGET_DERIVED || d.fpel_search_range > 64) return -1;
    const bool derived = d.target_form == SVT_HIP_OBMC_TARGET_DERIVED;
    if (derived ? !src : (!wsrc || !mask)) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    const size_t W = hBw[d.bsize], H = hBh[d.bsize], blk = W * H, ovA = std::min<size_t>(H, 64) >> 1, ovL = std::min<size_t>(W, 64) >> 1;
    {   // the start vector as the kernel derives it, and how far a search can move from it
        int sr = d.best_pred_mv_row >> 3, sc = d.best_pred_mv_col >> 3;
        if (d.do_full_refine) {
            const int rr = d.ref_mv_row, rc = d.ref_mv_col;
            const int cmin = std::max(d.lim_col_min, std::max((rc >> 3) - 1023 + ((rc & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1));
            const int rmin = std::max(d.lim_row_min, std::max((rr >> 3) - 1023 + ((rr & 7) ? 1 : 0), (-MV_UPP_ >> 3) + 1));
            const int cmax = std::min(d.lim_col_max, std::min((rc >> 3) + 1023, (MV_UPP_ >> 3) - 1));
            const int rmax = std::min(d.lim_row_max, std::min((rr >> 3) + 1023, (MV_UPP_ >> 3) - 1));
            sc = (int16_t)(sc < cmin ? cmin : (sc > cmax ? cmax : sc)), sr = (int16_t)(sr < rmin ? rmin : (sr > rmax ? rmax : sr));
        }
        const int need = std::max(std::abs(sr), std::abs(sc)) + (d.do_full_refine ? (int)d.fpel_search_range : 0) + (d.do_frac_refine ? 6 : 0);
        if (need > ref_border) return -1;
    }
    SVT_HIP_ENTRY_TRY
    const size_t b = (size_t)ref_border, rw = W + 2 * b, rh = H + 2 * b;
    const size_t bytes = rw * rh + (derived ? blk + W * ovA + H * ovL : blk * 8) + (table ? sizeof(SvtHipMvCostTable) : 0) + sizeof(d) + 64 + 8 * 256;
    svthip::HostCall& c = svthip::host_call();
    c.begin();
    c.reserve(bytes, bytes);
    uint8_t* dref = (uint8_t*)c.dalloc(rw * rh);
    c.up2d(dref, rw, ref - (ptrdiff_t)b * ref_stride - (ptrdiff_t)b, (size_t)ref_stride, rw, rh);
    SvtHipInterPredPlanes planes{};
    planes.base[0] = dref;
    d.ref_plane = 0, d.ref_off = b * rw + b, d.ref_stride = (uint32_t)rw, d.above_plane = 1, d.left_plane = 2;
    uint8_t* dsrc = nullptr;
    int32_t *dws = nullptr, *dmk = nullptr;
    if (derived) {
        dsrc = (uint8_t*)c.dalloc(blk);
        c.up2d(dsrc, W, src, (size_t)src_stride, W, H);
        d.src_off = 0, d.src_stride = (uint32_t)W;
        if (above && d.up_available && d.n_above) {
            uint8_t* da = (uint8_t*)c.dalloc(W * ovA);
            c.up2d(da, W, above, (size_t)above_stride, W, ovA);
            planes.base[1] = da, d.above_off = 0, d.above_stride = (uint32_t)W;
        }
        if (left && d.left_available && d.n_left) {
            uint8_t* dl = (uint8_t*)c.dalloc(H * ovL);
            c.up2d(dl, ovL, left, (size_t)left_stride, ovL, H);
            planes.base[2] = dl, d.left_off = 0, d.left_stride = (uint32_t)ovL;
        }
    } else {
        dws = (int32_t*)c.dalloc(blk * 4), dmk = (int32_t*)c.dalloc(blk * 4);
        c.up(dws, wsrc, blk * 4);
        c.up(dmk, mask, blk * 4);
        d.wsrc_off = d.mask_off = 0;
    }
    SvtHipMvCostTable* dt = nullptr;
    if (table) {
        dt = (SvtHipMvCostTable*)c.dalloc(sizeof(SvtHipMvCostTable));
        c.up(dt, table, sizeof(SvtHipMvCostTable));
    }
    d.cost_table = table ? 0 : -1;
    SvtHipObmcSearchDesc* dd = (SvtHipObmcSearchDesc*)c.dalloc(sizeof(d));
    c.up(dd, &d, sizeof(d));
    uint8_t* dres = (uint8_t*)c.dalloc(64); // the result, and at byte 52 the check kernel's word
    uint8_t  back[64];
    memset(back, 0, sizeof(back));
    c.up(dres, back, sizeof(back));
    // one item: only the launch class of its size
    if (blk > (size_t)SMALL_PIX)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(obmc_search_kernel<true>), dim3(1), dim3(64), OBMC_LDS_BIG, c.stream, planes, (const uint8_t*)dsrc, (const int32_t*)dws,
                           (const int32_t*)dmk, (const SvtHipMvCostTable*)dt, table ? 1u : 0u, (const SvtHipObmcSearchDesc*)dd, 1u, (SvtHipObmcSearchResult*)dres,
                           (uint8_t*)nullptr);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(obmc_search_kernel<false>), dim3(1), dim3(64 * SMALL_WAVES), OBMC_LDS_SMALL, c.stream, planes, (const uint8_t*)dsrc,
                           (const int32_t*)dws, (const int32_t*)dmk, (const SvtHipMvCostTable*)dt, table ? 1u : 0u, (const SvtHipObmcSearchDesc*)dd, 1u,
                           (SvtHipObmcSearchResult*)dres, (uint8_t*)nullptr);
    SVT_LAUNCH_CHECK();
    hipLaunchKernelGGL(obmc_search_check_kernel, dim3(1), dim3(256), 0, c.stream, planes, dsrc != nullptr, dws != nullptr, dt != nullptr, table ? 1u : 0u,
                       (const SvtHipObmcSearchDesc*)dd, 1u, (uint32_t*)(dres + 52));
    SVT_LAUNCH_CHECK();
    c.down(back, dres, sizeof(back));
    uint32_t bad;
    memcpy(&bad, back + 52, 4);
    if (bad) return -1;
    memcpy(result, back, sizeof(*result));
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

#define SVT_HIP_VARIANCE_FORMS(W, H)                                                                                                                                     \
    unsigned int svt_aom_variance##W##x##H##_hip(const uint8_t* a, int a_stride, const uint8_t* b, int b_stride, unsigned int* sse) {                                    \
        return var_form(SVT_HIP_VAR_VAR, bsize_of(W, H), a, a_stride, 0, 0, b, b_stride, nullptr, nullptr, sse);                                                         \
    }                                                                                                                                                                    \
    uint32_t svt_aom_sub_pixel_variance##W##x##H##_hip(const uint8_t* a, int a_stride, int xoffset, int yoffset, const uint8_t* b, int b_stride, uint32_t* sse) {        \
        return var_form(SVT_HIP_VAR_SUBPIX, bsize_of(W, H), a, a_stride, xoffset, yoffset, b, b_stride, nullptr, nullptr, sse);                                          \
    }                                                                                                                                                                    \
    unsigned int svt_aom_obmc_sad##W##x##H##_hip(const uint8_t* pre, int pre_stride, const int32_t* wsrc, const int32_t* mask) {                                         \
        return var_form(SVT_HIP_VAR_OBMC_SAD, bsize_of(W, H), pre, pre_stride, 0, 0, nullptr, 0, wsrc, mask, nullptr);                                                   \
    }                                                                                                                                                                    \
    unsigned int svt_aom_obmc_variance##W##x##H##_hip(const uint8_t* pre, int pre_stride, const int32_t* wsrc, const int32_t* mask, unsigned int* sse) {                 \
        return var_form(SVT_HIP_VAR_OBMC_VAR, bsize_of(W, H), pre, pre_stride, 0, 0, nullptr, 0, wsrc, mask, sse);                                                       \
    }                                                                                                                                                                    \
    unsigned int svt_aom_obmc_sub_pixel_variance##W##x##H##_hip(const uint8_t* pre, int pre_stride, int xoffset, int yoffset, const int32_t* wsrc, const int32_t* mask,  \
                                                                unsigned int* sse) {                                                                                     \
        return var_form(SVT_HIP_VAR_OBMC_SUBPIX, bsize_of(W, H), pre, pre_stride, xoffset, yoffset, nullptr, 0, wsrc, mask, sse);                                        \
    }
SVT_HIP_FOR_ALL_VARIANCE_SIZES(SVT_HIP_VARIANCE_FORMS)
#undef SVT_HIP_VARIANCE_FORMS

uint32_t svt_aom_mse16x16_hip(const uint8_t* src_ptr, int32_t source_stride, const uint8_t* ref_ptr, int32_t recon_stride, uint32_t* sse) {
    return var_form(SVT_HIP_VAR_MSE, bsize_of(16, 16), src_ptr, source_stride, 0, 0, ref_ptr, recon_stride, nullptr, nullptr, sse);
}

void svt_aom_upsampled_pred_hip(void* xd, const void* cm, int mi_row, int mi_col, const SvtHipMv* mv, uint8_t* comp_pred, int width, int height, int subpel_x_q3,
                                int subpel_y_q3, const uint8_t* ref, int ref_stride, int subpel_search) {
    (void)xd, (void)cm, (void)mi_row, (void)mi_col, (void)mv;
    const auto pow2 = [](const int v) { return v >= 4 && v <= 128 && (v & (v - 1)) == 0; };
    if (svthip::failed() || !comp_pred || !ref || !pow2(width) || !pow2(height) || subpel_x_q3 < 0 || subpel_x_q3 > 7 || subpel_y_q3 < 0 || subpel_y_q3 > 7 ||
        subpel_search < 1 || subpel_search > 3)
        return;
    try {
        // the C's own footprint: 3 before and 4 after the block in a filtered direction
        const size_t x0 = subpel_x_q3 ? 3 : 0, y0 = subpel_y_q3 ? 3 : 0, rw = (size_t)width + (subpel_x_q3 ? 7 : 0), rh = (size_t)height + (subpel_y_q3 ? 7 : 0);
        const size_t blk = (size_t)width * height, bytes = rw * rh + blk + 4096;
        svthip::HostCall& c = svthip::host_call();
        if (bytes <= 16384) c.begin_small();
        else c.begin();
        c.reserve(bytes, bytes);
        uint8_t* dr = (uint8_t*)c.dalloc(rw * rh);
        uint8_t* dc = (uint8_t*)c.dalloc(blk);
        c.up2d(dr, rw, ref - (ptrdiff_t)y0 * ref_stride - (ptrdiff_t)x0, (size_t)ref_stride, rw, rh);
        const uint8_t* org = dr + y0 * rw + x0;
        if ((int)(width * (height + 8)) > IM_SMALL)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(upsampled_pred_kernel<true>), dim3(1), dim3(64), IM_BIG, c.stream, org, (int)rw, dc, width, height, subpel_x_q3, subpel_y_q3,
                               subpel_search);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(upsampled_pred_kernel<false>), dim3(1), dim3(64), IM_SMALL, c.stream, org, (int)rw, dc, width, height, subpel_x_q3,
                               subpel_y_q3, subpel_search);
        SVT_LAUNCH_CHECK();
        c.down(comp_pred, dc, blk);
    } catch (const svthip::DeviceError&) {}
}

} // extern "C"
