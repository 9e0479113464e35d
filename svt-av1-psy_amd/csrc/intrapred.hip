// intrapred.hip -- the first arrow of the mode-decision loop for INTRA blocks on gfx950: what build_intra_predictors / build_intra_predictors_high
// (enc_intra_prediction.c:60, :241) compute from the two neighbour arrays -- edge assembly, corner filter, edge filters, upsampling, then the predictor -- for n
// independent blocks of mixed sizes in one launch, and the chroma-from-luma trio (luma 4:2:0 subsampling -> average subtraction -> prediction) beside it, bit for bit
// at 8, 10 and 12 bit.  DESIGN.md 4.21 has the layout, the literal narrowings, the readable-extent contract and the resources.
//
//  * intra_pred_kernel: one launch, n descriptors.  A workgroup (4 waves) takes DPW = 16 consecutive descriptors and flattens their tiles into one list (prefix sum
//    of the tile counts in LDS, as dist.hip and interpred.hip do).  A tile is the block's full width by min(h, 1024 / w) rows: at most 1024 samples, sixteen per lane;
//    only 64x64 (four tiles), 64x32 and 32x64 (two) are cut.  ONE WAVE owns a tile and prepares the block's edges -- at most 129 samples each -- in its own LDS slice;
//    a cut block repeats that preparation per tile, which costs a few hundred LDS operations against 1024 output samples.  Nothing crosses waves: wave barriers only.
//  * the descriptor index goes through readfirstlane: the mode switch, every need_* flag, the filter strengths and the upsampling decisions are scalar.
//  * filter-intra (w, h <= 32: one tile) runs its 4x2 patches as an anti-diagonal wavefront in the wave's 33 x 33 LDS buffer: patch (i, j) in step i + j, eight
//    patches of eight samples per step, one wave barrier per step.
//  * cfl_pred_kernel: one wave per descriptor (w * h <= 1024): the Q3 AC values stay in sixteen registers per lane, the sum is a wave reduction.
//  * no global atomics, nothing to zero beforehand, every output sample is written exactly once by a plain store: results do not depend on launch order.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"

namespace {

constexpr int DPW      = 16;             // descriptors per workgroup group
constexpr int TPB      = 256;            // threads per workgroup
constexpr int WAVES    = TPB / 64;
constexpr int SPLIT    = 4;              // most workgroups (blockIdx.y) that share one descriptor group's tile list
constexpr int TILE_PX  = 1024;           // samples per tile
constexpr int NPL      = TILE_PX / 64;   // samples per lane
constexpr int EDGE_ORG = 16;             // edge arrays are addressed from -16 (the upsampler writes [-2])
constexpr int EDGE_LEN = 160;            // ... to 143: the longest prepared edge is [-1, 127]
constexpr int FI_PITCH = 33;             // the filter-intra buffer: 33 x 33, row 0 = above[-1 ..], column 0 = left
constexpr int FI_LEN   = FI_PITCH * FI_PITCH + 1;
constexpr int CFL_LINE = 32;             // CFL_BUF_LINE

// sm_weight_arrays (AV1 specification 7.11.2.6: Sm_Weights_Tx_4x4 .. 64x64 at offset = block dimension)
__device__ constexpr uint8_t kSmWeights[128] = {
    0, 0, 255, 128, 255, 149, 85, 64, 255, 197, 146, 105, 73, 50, 37, 32, 255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16,
    255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17, 14, 12, 10, 9, 8, 8,
    255, 248, 240, 233, 225, 218, 210, 203, 196, 189, 182, 176, 169, 163, 156, 150, 144, 138, 133, 127, 121, 116, 111, 106, 101, 96, 91, 86, 82, 77, 73, 69,
    65, 61, 57, 54, 50, 47, 44, 41, 38, 35, 32, 29, 27, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 7, 6, 6, 5, 5, 4, 4, 4};
// Dr_Intra_Derivative (AV1 specification 7.11.2.4), indexed by the angle; only multiples of 3 (and 23 + 3k, 45 + 3k ...) that p_angle can take are non-zero
__device__ constexpr uint16_t kDrDerivative[90] = {0,   0, 0, 1023, 0, 0, 547, 0, 0, 372, 0, 0, 0, 0, 273, 0, 0, 215, 0, 0, 178, 0, 0, 151, 0, 0, 132, 0, 0, 116,
                                                   0,   0, 102, 0, 0, 0, 90, 0, 0, 80, 0, 0, 71, 0, 0, 64, 0, 0, 57, 0, 0, 51, 0, 0, 45, 0, 0, 0, 40, 0,
                                                   0,   35, 0, 0, 31, 0, 0, 27, 0, 0, 23, 0, 0, 19, 0, 0, 15, 0, 0, 0, 0, 11, 0, 0, 7, 0, 0, 3, 0, 0};
// Filter_Intra_Taps (AV1 specification 7.11.2.3): [mode][sample of the 4x2 patch][p0 .. p6]
__device__ constexpr int8_t kFilterIntraTaps[5][8][7] = {
    {{-6, 10, 0, 0, 0, 12, 0}, {-5, 2, 10, 0, 0, 9, 0}, {-3, 1, 1, 10, 0, 7, 0}, {-3, 1, 1, 2, 10, 5, 0}, {-4, 6, 0, 0, 0, 2, 12}, {-3, 2, 6, 0, 0, 2, 9},
     {-3, 2, 2, 6, 0, 2, 7}, {-3, 1, 2, 2, 6, 3, 5}},
    {{-10, 16, 0, 0, 0, 10, 0}, {-6, 0, 16, 0, 0, 6, 0}, {-4, 0, 0, 16, 0, 4, 0}, {-2, 0, 0, 0, 16, 2, 0}, {-10, 16, 0, 0, 0, 0, 10}, {-6, 0, 16, 0, 0, 0, 6},
     {-4, 0, 0, 16, 0, 0, 4}, {-2, 0, 0, 0, 16, 0, 2}},
    {{-8, 8, 0, 0, 0, 16, 0}, {-8, 0, 8, 0, 0, 16, 0}, {-8, 0, 0, 8, 0, 16, 0}, {-8, 0, 0, 0, 8, 16, 0}, {-4, 4, 0, 0, 0, 0, 16}, {-4, 0, 4, 0, 0, 0, 16},
     {-4, 0, 0, 4, 0, 0, 16}, {-4, 0, 0, 0, 4, 0, 16}},
    {{-2, 8, 0, 0, 0, 10, 0}, {-1, 3, 8, 0, 0, 6, 0}, {-1, 2, 3, 8, 0, 4, 0}, {0, 1, 2, 3, 8, 2, 0}, {-1, 4, 0, 0, 0, 3, 10}, {-1, 3, 4, 0, 0, 4, 6},
     {-1, 2, 3, 4, 0, 4, 4}, {-1, 2, 2, 3, 4, 3, 3}},
    {{-12, 14, 0, 0, 0, 14, 0}, {-10, 0, 14, 0, 0, 12, 0}, {-9, 0, 0, 14, 0, 11, 0}, {-8, 0, 0, 0, 14, 10, 0}, {-10, 12, 0, 0, 0, 0, 14}, {-9, 1, 12, 0, 0, 0, 12},
     {-8, 0, 0, 12, 0, 1, 11}, {-7, 0, 0, 1, 12, 1, 9}}};
// mode_to_angle_map (intra_prediction.h:65): DC V H D45 D135 D113 D157 D203 D67 SMOOTH SMOOTH_V SMOOTH_H PAETH
__device__ constexpr uint8_t kModeAngle[13] = {0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0};

// what a launch carries besides the descriptors.  form 0: the batched entry.  form 1 / 2 / 3: one block of svt_av1_[highbd_]dr_prediction_z1 / z2 / z3 -- the
// caller's PREPARED edges are copied into the wave's slice as they are (above [alo, ahi], left [llo, lhi]) and the caller's dx, dy and upsampling flags are used.
struct Aux { int32_t bd, form, dx, dy, up_above, up_left, alo, ahi, llo, lhi; };

// the 19 sizes of TX_SIZES_ALL: 4 .. 64 on either side, aspect ratio up to 4
__host__ __device__ __forceinline__ bool size_ok(const uint32_t w, const uint32_t h) {
    const bool pw = w >= 4 && w <= 64 && (w & (w - 1)) == 0, ph = h >= 4 && h <= 64 && (h & (h - 1)) == 0;
    return pw && ph && w <= 4 * h && h <= 4 * w;
}
// everything the kernel relies on
__host__ __device__ __forceinline__ bool desc_ok(const SvtHipIntraPredDesc& d, const SvtHipIntraPredPlanes& planes) {
    if (!size_ok(d.w, d.h) || d.mode > 12 || d.angle_delta < -3 || d.angle_delta > 3 || d.filter_intra_mode > 5) return false;
    if (d.filter_intra_mode < 5 && (d.w > 32 || d.h > 32)) return false;
    if (d.n_top_px > d.w || d.n_left_px > d.h || d.n_topright_px > d.w || d.n_bottomleft_px > d.h) return false;
    if ((d.n_topright_px > 0 && d.n_top_px != d.w) || (d.n_bottomleft_px > 0 && d.n_left_px != d.h)) return false; // the C's assertions
    if (d.disable_edge_filter > 1 || d.filt_type > 1) return false;
    if (d.top_plane >= 32 || d.left_plane >= 32 || planes.base[d.top_plane] == nullptr || planes.base[d.left_plane] == nullptr) return false;
    return true;
}
// The tiling of a w x h block, the ONE place that knows it: full-width tiles of min(h, 1024 / w) rows
__host__ __device__ __forceinline__ uint32_t tile_rows(const uint32_t w, const uint32_t h) {
    const uint32_t cap = (uint32_t)TILE_PX / w;
    return h < cap ? h : cap;
}
__host__ __device__ __forceinline__ uint32_t tile_count(const uint32_t w, const uint32_t h) { return h / tile_rows(w, h); }

__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int load_px(const uint16_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint16_t*)p; }
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int clip_px(const int v, const int maxv) { return v < 0 ? 0 : (v > maxv ? maxv : v); }
__device__ __forceinline__ int rpot_signed(const int v, const int n) { // ROUND_POWER_OF_TWO_SIGNED (definitions.h:462): half away from zero
    return v < 0 ? -((-v + ((1 << n) >> 1)) >> n) : (v + ((1 << n) >> 1)) >> n;
}

// svt_aom_intra_edge_filter_strength (intra_prediction.c:180-243)
__device__ __forceinline__ int edge_strength(const int bs0, const int bs1, const int delta, const int type) {
    const int d = delta < 0 ? -delta : delta, wh = bs0 + bs1;
    int       s = 0;
    if (type == 0) {
        if (wh <= 8) s = d >= 56 ? 1 : 0;
        else if (wh <= 16) s = d >= 40 ? 1 : 0;
        else if (wh <= 24) s = d >= 32 ? 3 : (d >= 16 ? 2 : (d >= 8 ? 1 : 0));
        else if (wh <= 32) s = d >= 32 ? 3 : (d >= 4 ? 2 : (d >= 1 ? 1 : 0));
        else s = d >= 1 ? 3 : 0;
    } else {
        if (wh <= 8) s = d >= 64 ? 2 : (d >= 40 ? 1 : 0);
        else if (wh <= 16) s = d >= 48 ? 2 : (d >= 20 ? 1 : 0);
        else if (wh <= 24) s = d >= 4 ? 3 : 0;
        else s = d >= 1 ? 3 : 0;
    }
    return s;
}
// svt_aom_use_intra_edge_upsample (intra_prediction.c:146-152)
__device__ __forceinline__ int use_upsample(const int bs0, const int bs1, const int delta, const int type) {
    const int d = delta < 0 ? -delta : delta;
    if (d <= 0 || d >= 40) return 0;
    return type ? (bs0 + bs1 <= 8) : (bs0 + bs1 <= 16);
}
// svt_av1_filter_intra_edge[_high]_c (:156-178) on p[0 .. sz): every lane reads its taps from the unfiltered array (the C's snapshot copy), the wave meets, then the
// results are stored.  p[0] is a tap input and is never written; tap indices are clamped to [0, sz - 1]; sz <= 129 = three rounds of 64 lanes.
__device__ __forceinline__ void edge_filter(uint16_t* p, const int sz, const int strength, const int l) {
    if (!strength) return; // (wave-uniform)
    const int k0 = strength == 3 ? 2 : 0, k1 = strength == 2 ? 5 : 4, k2 = strength == 1 ? 8 : (strength == 2 ? 6 : 4);
    int       v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = l + 64 * k;
        v[k]        = 0;
        if (i >= 1 && i < sz) {
            const int a = i - 2 < 0 ? 0 : i - 2, b = i - 1, c = i + 1 > sz - 1 ? sz - 1 : i + 1, e = i + 2 > sz - 1 ? sz - 1 : i + 2;
            v[k]        = (k0 * ((int)p[a] + (int)p[e]) + k1 * ((int)p[b] + (int)p[c]) + k2 * (int)p[i] + 8) >> 4;
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = l + 64 * k;
        if (i >= 1 && i < sz) p[i] = (uint16_t)v[k];
    }
    __builtin_amdgcn_wave_barrier();
}
// svt_av1_upsample_intra_edge[_high]_c (C_DEFAULT/intra_prediction_c.c:14-55) on p[-1 .. sz), sz <= 16: in[0] = in[1] = p[-1], in[sz + 2] = p[sz - 1]; writes
// p[-2 .. 2 sz - 2]
__device__ __forceinline__ void upsample_edge(uint16_t* p, const int sz, const int maxv, const int l) {
    const bool act = l < sz;
    int        s = 0, keep = 0;
    const int  corner = (int)p[-1];
    if (act) {
        // in[m] = p[m - 2] clamped to [-1, sz - 1]
        const int i0 = l - 2 < -1 ? -1 : l - 2, i1 = l - 1, i2 = l, i3 = l + 1 > sz - 1 ? sz - 1 : l + 1;
        s            = clip_px((-(int)p[i0] + 9 * (int)p[i1] + 9 * (int)p[i2] - (int)p[i3] + 8) >> 4, maxv);
        keep         = (int)p[l];
    }
    __builtin_amdgcn_wave_barrier();
    if (act) {
        p[2 * l - 1] = (uint16_t)s;
        p[2 * l]     = (uint16_t)keep;
    }
    if (l == 0) p[-2] = (uint16_t)corner;
    __builtin_amdgcn_wave_barrier();
}

// stores f(column, row of the block) for the lane's samples i = l + 64 j of the tile (sample i is column i & (w - 1), tile row i >> lw)
template <typename PIX, typename F>
__device__ __forceinline__ void emit(PIX* out, const uint32_t ds, const int lw, const int r0, const int nj, const bool on, const int l, F f) {
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int i = l + 64 * j;
        if (j < nj && on) {
            const int c = i & ((1 << lw) - 1), rr = i >> lw;
            out[(size_t)rr * ds + c] = (PIX)f(c, r0 + rr);
        }
    }
}

// FORM = false: the batched entry and the filter-intra form; FORM = true: one block of a dr_prediction form
template <typename PIX, bool FORM>
__global__ __launch_bounds__(TPB) void intra_pred_kernel(const SvtHipIntraPredPlanes planes, PIX* dst_base, const SvtHipIntraPredDesc* __restrict__ descs,
                                                         const uint32_t n, uint8_t* __restrict__ status, const Aux aux) {
    __shared__ uint32_t pre[DPW + 1];             // exclusive prefix sum of the tile counts
    __shared__ uint16_t edges[WAVES][2][EDGE_LEN]; // the waves' above / left slices
    __shared__ uint16_t fibuf[WAVES][FI_LEN];      // the waves' filter-intra buffers
    const int      tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t first = blockIdx.x * DPW;
    if (tid < 64) { // (the first wave, whole: the scan's shuffles are wave-uniform)
        uint32_t cnt = 0;
        if (tid < DPW && first + tid < n) {
            const SvtHipIntraPredDesc d  = descs[first + tid];
            const bool                ok = FORM ? size_ok(d.w, d.h) : desc_ok(d, planes);
            if (ok) cnt = tile_count(d.w, d.h);
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
    const int      bd = aux.bd, maxv = (1 << bd) - 1, base = 128 << (bd - 8);
    uint16_t* const A = edges[wv][0] + EDGE_ORG;
    uint16_t* const L = edges[wv][1] + EDGE_ORG;
    uint16_t* const B = fibuf[wv];
    for (uint32_t u = blockIdx.y * WAVES + wv; u < total; u += gridDim.y * WAVES) { // (u depends on the wave only)
        int di = 0;
#pragma unroll
        for (int s = DPW >> 1; s >= 1; s >>= 1)
            if (pre[di + s] <= u) di += s;
        di = __builtin_amdgcn_readfirstlane(di); // the descriptor, and every branch taken on it, is the wave's: scalar loads, scalar branches
        const SvtHipIntraPredDesc d = descs[first + di];
        const int      w = d.w, h = d.h, lw = __builtin_ctz((unsigned)w);
        const int      th = (int)tile_rows((uint32_t)w, (uint32_t)h), r0 = (int)(u - pre[di]) * th, npx = th << lw;
        const int      nj = npx >= 64 ? npx >> 6 : 1;
        const bool     on = l < npx;
        const uint32_t ds = d.dst_stride;
        PIX*           out = dst_base + d.dst_off + (size_t)r0 * ds;
        const PIX*     top = (const PIX*)planes.base[d.top_plane] + d.top_off;
        const PIX*     lef = (const PIX*)planes.base[d.left_plane] + d.left_off;
        __builtin_amdgcn_wave_barrier(); // the slices are rewritten: the previous tile's readers are done
        int zone = 0, dx = 1, dy = 1, upa = 0, upl = 0; // zone 1 / 2 / 3, 4 = V, 5 = H, 0 = not directional
        if (FORM) {
            for (int i = aux.alo + l; i <= aux.ahi; i += 64) A[i] = (uint16_t)load_px(top + i);
            for (int i = aux.llo + l; i <= aux.lhi; i += 64) L[i] = (uint16_t)load_px(lef + i);
            zone = aux.form, dx = aux.dx, dy = aux.dy, upa = aux.up_above, upl = aux.up_left;
        } else {
            const int  mode = d.mode, nt = d.n_top_px, ntr = d.n_topright_px, nl = d.n_left_px, nbl = d.n_bottomleft_px;
            const bool is_dr = mode >= 1 && mode <= 8, use_fi = d.filter_intra_mode != 5;
            // extend_modes (intra_prediction.c:469-483), then the overrides of :94-103
            bool need_above = mode != 2 && mode != 7, need_left = mode != 1 && mode != 3 && mode != 8, need_al = mode == 4 || mode == 5 || mode == 6 || mode == 12;
            int  p_angle = 0;
            if (is_dr) {
                p_angle    = (int)kModeAngle[mode] + (int)d.angle_delta * 3; // ANGLE_STEP
                need_above = p_angle < 180, need_left = p_angle > 90, need_al = true;
            }
            if (use_fi) need_left = need_above = need_al = true;
            if ((!need_above && nl == 0) || (!need_left && nt == 0)) {
                const int val = need_left ? (nt > 0 ? load_px(top) : base + 1) : (nl > 0 ? load_px(lef) : base - 1);
                emit(out, ds, lw, r0, nj, on, l, [&](int, int) { return val; });
                continue;
            }
            bool need_bottom = mode == 7, need_right = mode == 3 || mode == 8;
            if (use_fi) need_bottom = need_right = false;
            if (is_dr) need_bottom = p_angle > 180, need_right = p_angle < 90;
            if (need_left) { // copy, then replicate the last available sample: the index is clamped instead
                const int need = h + (need_bottom ? w : 0), avail = nl + (need_bottom ? nbl : 0);
                const int fill = nl > 0 ? 0 : (nt > 0 ? load_px(top) : base + 1);
                for (int i = l; i < need; i += 64) L[i] = (uint16_t)(nl > 0 ? load_px(lef + (size_t)(i < avail ? i : avail - 1) * d.left_stride) : fill);
            }
            if (need_above) {
                const int need = w + (need_right ? h : 0), avail = nt + (need_right ? ntr : 0);
                const int fill = nt > 0 ? 0 : (nl > 0 ? load_px(lef) : base - 1);
                for (int i = l; i < need; i += 64) A[i] = (uint16_t)(nt > 0 ? load_px(top + (i < avail ? i : avail - 1)) : fill);
            }
            if (need_al && l == 0) {
                const int c = nt > 0 && nl > 0 ? load_px(top - 1) : (nt > 0 ? load_px(top) : (nl > 0 ? load_px(lef) : base));
                A[-1] = L[-1] = (uint16_t)c;
            }
            __builtin_amdgcn_wave_barrier();
            if (use_fi) {
                // svt_av1_filter_intra_predictor_c / svt_aom_highbd_filter_intra_predictor: the whole block is this tile (w, h <= 32)
                const int fm = d.filter_intra_mode;
                if (l <= w) B[l] = A[l - 1];
                if (l < h) B[(l + 1) * FI_PITCH] = L[l];
                __builtin_amdgcn_wave_barrier();
                const int ni = h >> 1, nk = w >> 2, pj = l >> 3, k = l & 7;
                for (int s = 0; s < ni + nk - 1; s++) {
                    const int  pi = s - pj, r = 1 + 2 * pi, c = 1 + 4 * pj;
                    const bool act = pi >= 0 && pi < ni && pj < nk;
                    int        v = 0;
                    if (act) {
                        const uint16_t* q = B + (r - 1) * FI_PITCH + c - 1;
                        const int8_t*   t = kFilterIntraTaps[fm][k];
                        v = t[0] * (int)q[0] + t[1] * (int)q[1] + t[2] * (int)q[2] + t[3] * (int)q[3] + t[4] * (int)q[4] + t[5] * (int)q[FI_PITCH] + t[6] * (int)q[2 * FI_PITCH];
                        v = clip_px(rpot_signed(v, 4), maxv); // clipped before it feeds the next patch
                        B[(r + (k >> 2)) * FI_PITCH + c + (k & 3)] = (uint16_t)v;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) { return (int)B[(r + 1) * FI_PITCH + c + 1]; });
                continue;
            }
            if (is_dr) {
                if (!d.disable_edge_filter) {
                    const int ft = d.filt_type;
                    if (p_angle != 90 && p_angle != 180) {
                        if (need_above && need_left && w + h >= 24) { // filter_intra_edge_corner: both [-1] entries, before the edge filters read them
                            const int s = (5 * (int)L[0] + 6 * (int)A[-1] + 5 * (int)A[0] + 8) >> 4;
                            __builtin_amdgcn_wave_barrier();
                            if (l == 0) A[-1] = L[-1] = (uint16_t)s;
                            __builtin_amdgcn_wave_barrier();
                        }
                        if (need_above && nt > 0) edge_filter(A - 1, nt + 1 + (need_right ? h : 0), edge_strength(w, h, p_angle - 90, ft), l);
                        if (need_left && nl > 0) edge_filter(L - 1, nl + 1 + (need_bottom ? w : 0), edge_strength(h, w, p_angle - 180, ft), l);
                    }
                    upa = use_upsample(w, h, p_angle - 90, ft);
                    if (need_above && upa) upsample_edge(A, w + (need_right ? h : 0), maxv, l);
                    upl = use_upsample(h, w, p_angle - 180, ft);
                    if (need_left && upl) upsample_edge(L, h + (need_bottom ? w : 0), maxv, l);
                }
                if (p_angle < 90) zone = 1, dx = kDrDerivative[p_angle];
                else if (p_angle == 90) zone = 4;
                else if (p_angle < 180) zone = 2, dx = kDrDerivative[180 - p_angle], dy = kDrDerivative[p_angle - 90];
                else if (p_angle == 180) zone = 5;
                else zone = 3, dy = kDrDerivative[270 - p_angle];
            } else if (mode == 0) { // svt_aom_dc_pred[n_left_px > 0][n_top_px > 0]
                int val = base;
                if (nt > 0 || nl > 0) {
                    int part = 0;
                    if (nt > 0 && l < w) part += (int)A[l];
                    if (nl > 0 && l < h) part += (int)L[l];
                    const uint32_t sum = (uint32_t)__builtin_amdgcn_readfirstlane(wave_sum(part)), count = (uint32_t)((nt > 0 ? w : 0) + (nl > 0 ? h : 0));
                    val                = (int)((sum + (count >> 1)) / count); // one division per tile, on a wave-uniform value
                }
                emit(out, ds, lw, r0, nj, on, l, [&](int, int) { return val; });
                continue;
            } else if (mode == 9) { // SMOOTH: weights (uint8_t)(256 - w), divide_round by 9 bits
                const int below = L[h - 1], right = A[w - 1];
                emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                    const uint32_t wh = kSmWeights[h + r], ww = kSmWeights[w + c];
                    const uint32_t p = wh * A[c] + ((256 - wh) & 0xff) * below + ww * L[r] + ((256 - ww) & 0xff) * right;
                    return (int)((p + 256) >> 9);
                });
                continue;
            } else if (mode == 10) { // SMOOTH_V
                const int below = L[h - 1];
                emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                    const uint32_t wh = kSmWeights[h + r];
                    return (int)((wh * A[c] + ((256 - wh) & 0xff) * below + 128) >> 8);
                });
                continue;
            } else if (mode == 11) { // SMOOTH_H
                const int right = A[w - 1];
                emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                    const uint32_t ww = kSmWeights[w + c];
                    return (int)((ww * L[r] + ((256 - ww) & 0xff) * right + 128) >> 8);
                });
                continue;
            } else { // PAETH: the nearest to top + left - top_left; ties go left, top, top-left
                const int tl = A[-1];
                emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                    const int lf = L[r], tp = A[c], b = tp + lf - tl;
                    const int pl = b > lf ? b - lf : lf - b, pt = b > tp ? b - tp : tp - b, ptl = b > tl ? b - tl : tl - b;
                    return (pl <= pt && pl <= ptl) ? lf : (pt <= ptl ? tp : tl);
                });
                continue;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (zone == 4) emit(out, ds, lw, r0, nj, on, l, [&](int c, int) { return (int)A[c]; });
        else if (zone == 5) emit(out, ds, lw, r0, nj, on, l, [&](int, int r) { return (int)L[r]; });
        else if (zone == 1) { // svt_av1_[highbd_]dr_prediction_z1_c: base < max_base_x is tested per sample
            const int mb = (w + h - 1) << upa;
            emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                const int x = (r + 1) * dx, b = (x >> (6 - upa)) + (c << upa), sh = ((x << upa) & 0x3f) >> 1;
                if (b >= mb) return (int)A[mb];
                return clip_px(((int)A[b] * (32 - sh) + (int)A[b + 1] * sh + 16) >> 5, maxv);
            });
        } else if (zone == 3) {
            const int mb = (w + h - 1) << upl;
            emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                const int y = (c + 1) * dy, b = (y >> (6 - upl)) + (r << upl), sh = ((y << upl) & 0x3f) >> 1;
                if (b >= mb) return (int)L[mb];
                return clip_px(((int)L[b] * (32 - sh) + (int)L[b + 1] * sh + 16) >> 5, maxv);
            });
        } else if (zone == 2) { // negative x, y: arithmetic >> and & 0x3f on two's complement, as the C
            const int minx = -(1 << upa), miny = -(1 << upl);
            emit(out, ds, lw, r0, nj, on, l, [&](int c, int r) {
                const int x = (c << 6) - (r + 1) * dx, b1 = x >> (6 - upa);
                int       v;
                if (b1 >= minx) {
                    const int sh = ((x * (1 << upa)) & 0x3f) >> 1;
                    v            = (int)A[b1] * (32 - sh) + (int)A[b1 + 1] * sh;
                } else {
                    const int y = (r << 6) - (c + 1) * dy, sh = ((y * (1 << upl)) & 0x3f) >> 1;
                    int       b2 = y >> (6 - upl);
                    if (b2 < miny) b2 = miny; // (the C asserts it; a form's caller may pass a dx / dy pair that is no angle -- the slice is never left)
                    v = (int)L[b2] * (32 - sh) + (int)L[b2 + 1] * sh;
                }
                return clip_px((v + 16) >> 5, maxv);
            });
        }
    }
}

// descriptors the host cannot read: every thread looks at a few; whoever finds an invalid one stores 1 into the word the host zeroed (plain stores of one value)
__global__ __launch_bounds__(TPB) void intra_pred_check_kernel(const SvtHipIntraPredPlanes planes, const SvtHipIntraPredDesc* __restrict__ descs, const uint32_t n,
                                                               uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

template <bool FORM>
void launch(const SvtHipIntraPredPlanes& planes, void* dst_base, const SvtHipIntraPredDesc* descs, const uint32_t n, uint8_t* status, const Aux& aux, hipStream_t st) {
    // workgroups that share one descriptor group's tile list: four while the groups alone cannot fill the machine, one when they can (measured: DESIGN.md 4.21)
    const uint32_t groups = (n + DPW - 1) / DPW;
    const dim3     grid(groups, FORM || groups >= 4096 ? 1 : (groups >= 1024 ? 2 : SPLIT)), block(TPB);
    if (aux.bd > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(intra_pred_kernel<uint16_t, FORM>), grid, block, 0, st, planes, (uint16_t*)dst_base, descs, n, status, aux);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(intra_pred_kernel<uint8_t, FORM>), grid, block, 0, st, planes, (uint8_t*)dst_base, descs, n, status, aux);
    SVT_LAUNCH_CHECK();
}

// ---- chroma from luma --------------------------------------------------------------------------------------------------------------------------------
// the sizes of the reference's CFL_SUB_AVG_FN table (intra_prediction.h:167-181): 4 .. 32 on either side without 4x32 and 32x4
__host__ __device__ __forceinline__ bool cfl_size_ok(const uint32_t w, const uint32_t h) {
    const bool pw = w >= 4 && w <= 32 && (w & (w - 1)) == 0, ph = h >= 4 && h <= 32 && (h & (h - 1)) == 0;
    return pw && ph && w * 8 != h && h * 8 != w;
}
__host__ __device__ __forceinline__ bool cfl_desc_ok(const SvtHipCflPredDesc& d, const SvtHipIntraPredPlanes& planes) {
    if (!cfl_size_ok(d.w, d.h) || d.n_targets < 1 || d.n_targets > 2) return false;
    if (d.luma_plane >= 32 || planes.base[d.luma_plane] == nullptr) return false;
    // (no indexing of the descriptor by a variable: a by-value copy that is indexed dynamically becomes an LDS array on the device)
    if (d.pred_plane[0] >= 32 || planes.base[d.pred_plane[0]] == nullptr) return false;
    if (d.n_targets == 2 && (d.pred_plane[1] >= 32 || planes.base[d.pred_plane[1]] == nullptr)) return false;
    return true;
}
// FORM 0: the batched entry (subsample -> subtract the average -> predict one or two targets); FORM 1: svt_cfl_luma_subsampling_420_* (the Q3 values -> q3, rows of
// CFL_BUF_LINE); FORM 2: svt_cfl_predict_* (the AC values <- q3)
template <typename PIX, int FORM>
__global__ __launch_bounds__(TPB) void cfl_pred_kernel(const SvtHipIntraPredPlanes planes, PIX* dst_base, const SvtHipCflPredDesc* __restrict__ descs, const uint32_t n,
                                                       uint8_t* __restrict__ status, const int bd, int16_t* q3) {
    const int      l = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const uint32_t idx = blockIdx.x * WAVES + wv;
    if (idx >= n) return; // (the whole wave)
    const SvtHipCflPredDesc d  = descs[idx];
    const bool              ok = cfl_desc_ok(d, planes);
    if (status && l == 0) status[idx] = ok ? 0 : 1;
    if (!ok) return;
    const int  w = d.w, h = d.h, lw = __builtin_ctz((unsigned)w), lh = __builtin_ctz((unsigned)h), npx = w * h, maxv = (1 << bd) - 1;
    const int  nj = npx >= 64 ? npx >> 6 : 1;
    const bool on = l < npx;
    int        ac[NPL];
    int        part = 0;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int i = l + 64 * j;
        ac[j]       = 0;
        if (j < nj && on) {
            const int c = i & (w - 1), r = i >> lw;
            if (FORM == 2) ac[j] = q3[r * CFL_LINE + c];
            else {
                const PIX* p = (const PIX*)planes.base[d.luma_plane] + d.luma_off + (size_t)(2 * r) * d.luma_stride + 2 * c;
                ac[j]        = (int16_t)((load_px(p) + load_px(p + 1) + load_px(p + d.luma_stride) + load_px(p + d.luma_stride + 1)) << 1); // int16_t output_q3
            }
            if (FORM == 1) q3[r * CFL_LINE + c] = (int16_t)ac[j];
            part += ac[j];
        }
    }
    if (FORM == 1) return;
    if (FORM == 0) { // svt_subtract_average_c with round_offset = (w * h) >> 1, num_pel_log2 = log2 w + log2 h
        const int avg = (__builtin_amdgcn_readfirstlane(wave_sum(part)) + (npx >> 1)) >> (lw + lh);
#pragma unroll
        for (int j = 0; j < NPL; j++) ac[j] = (int16_t)(ac[j] - (int16_t)avg);
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (t >= d.n_targets) break;
        const int      alpha = t ? d.alpha_q3[1] : d.alpha_q3[0];
        const PIX*     pred = (const PIX*)planes.base[t ? d.pred_plane[1] : d.pred_plane[0]] + (t ? d.pred_off[1] : d.pred_off[0]);
        PIX*           out = dst_base + (t ? d.dst_off[1] : d.dst_off[0]);
        const uint32_t ps = t ? d.pred_stride[1] : d.pred_stride[0], ds = t ? d.dst_stride[1] : d.dst_stride[0];
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const int c = i & (w - 1), r = i >> lw;
                const int v = rpot_signed(alpha * ac[j], 6) + (int16_t)load_px(pred + (size_t)r * ps + c);
                out[(size_t)r * ds + c] = (PIX)clip_px(v, maxv); // (dst may be the DC prediction itself: the lane has read its sample)
            }
        }
    }
}
__global__ __launch_bounds__(TPB) void cfl_check_kernel(const SvtHipIntraPredPlanes planes, const SvtHipCflPredDesc* __restrict__ descs, const uint32_t n,
                                                        uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !cfl_desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}
template <int FORM>
void cfl_launch(const SvtHipIntraPredPlanes& planes, void* dst_base, const SvtHipCflPredDesc* descs, const uint32_t n, uint8_t* status, const int bd, const bool is16,
                int16_t* q3, hipStream_t st) {
    const dim3 grid((n + WAVES - 1) / WAVES), block(TPB);
    if (is16) hipLaunchKernelGGL(HIP_KERNEL_NAME(cfl_pred_kernel<uint16_t, FORM>), grid, block, 0, st, planes, (uint16_t*)dst_base, descs, n, status, bd, q3);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(cfl_pred_kernel<uint8_t, FORM>), grid, block, 0, st, planes, (uint8_t*)dst_base, descs, n, status, bd, q3);
    SVT_LAUNCH_CHECK();
}

// ---- the single-call forms ------------------------------------------------------------------------------------------------------------------------
// One block from host memory through the pinned arena of HostCall::begin_small; one synchronisation (the download); nothing of the caller's is written before it.
// svt_av1_[highbd_]dr_prediction_z{1,2,3}: exactly the index range of above / left the C function can read:
//   z1 above [0, (bw + bh - 1) << upsample_above];  z3 left [0, (bw + bh - 1) << upsample_left];
//   z2 above [-(1 << upsample_above), (bw - 1) << upsample_above], left [-(1 << upsample_left), (bh - 1) << upsample_left].
template <typename PIX>
void dr_host(PIX* dst, const ptrdiff_t stride, const int bw, const int bh, const PIX* above, const PIX* left, const int upa, const int upl, const int dx, const int dy,
             const int bd, const int zone) {
    if (!dst || !size_ok((uint32_t)bw, (uint32_t)bh)) return;
    if (sizeof(PIX) == 1 ? bd != 8 : (bd != 10 && bd != 12)) return;
    if ((upa | upl) & ~1) return;
    if ((upa || upl) && bw + bh > 16) return; // the upsampler only ever runs for edges of at most 16 samples
    if (dx < 1 || dx > 65535 || dy < 1 || dy > 65535) return; // get_dx / get_dy return uint16_t; the C asserts > 0
    if ((zone != 3 && !above) || (zone != 1 && !left)) return;
    Aux aux{};
    aux.bd = bd, aux.form = zone, aux.dx = dx, aux.dy = dy, aux.up_above = upa, aux.up_left = upl;
    aux.alo = 0, aux.ahi = -1, aux.llo = 0, aux.lhi = -1;
    if (zone == 1) aux.ahi = (bw + bh - 1) << upa;
    else if (zone == 3) aux.lhi = (bw + bh - 1) << upl;
    else aux.alo = -(1 << upa), aux.ahi = (bw - 1) << upa, aux.llo = -(1 << upl), aux.lhi = (bh - 1) << upl;
    const size_t px = sizeof(PIX), na = (size_t)(aux.ahi - aux.alo + 1), nl = (size_t)(aux.lhi - aux.llo + 1);
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = (na + nl + (size_t)bw * bh) * px + 4096;
    c.reserve(bytes, bytes);
    PIX*                 da = (PIX*)c.dalloc((na ? na : 1) * px);
    PIX*                 dl = (PIX*)c.dalloc((nl ? nl : 1) * px);
    PIX*                 dd = (PIX*)c.dalloc((size_t)bw * bh * px);
    SvtHipIntraPredDesc* dv = (SvtHipIntraPredDesc*)c.dalloc(sizeof(SvtHipIntraPredDesc));
    if (na) c.up(da, above + aux.alo, na * px);
    if (nl) c.up(dl, left + aux.llo, nl * px);
    SvtHipIntraPredDesc d{};
    d.top_off    = (uint64_t)(-aux.alo);
    d.left_off   = (uint64_t)(-aux.llo);
    d.left_plane = 1;
    d.dst_stride = (uint32_t)bw;
    d.w = (uint8_t)bw, d.h = (uint8_t)bh;
    c.up(dv, &d, sizeof(d));
    SvtHipIntraPredPlanes planes{};
    planes.base[0] = da, planes.base[1] = dl;
    launch<true>(planes, dd, dv, 1, nullptr, aux, c.stream);
    c.down2d(dst, (size_t)stride * px, dd, (size_t)bw * px, (size_t)bw * px, bh);
}
// tx_size_wide / tx_size_high (TX_4X4 = 0 .. TX_64X16 = 18)
const uint8_t kTxW[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
const uint8_t kTxH[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
// svt_av1_filter_intra_predictor: above [-1, w - 1] and left [0, h - 1] are what the C reads; the batched kernel with both edges complete
void filter_intra_host(uint8_t* dst, const ptrdiff_t stride, const int tx_size, const uint8_t* above, const uint8_t* left, const int mode) {
    if (!dst || !above || !left || tx_size < 0 || tx_size >= 19 || mode < 0 || mode > 4) return;
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    if (w > 32 || h > 32) return;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = (size_t)(w + 1 + h + w * h) + 4096;
    c.reserve(bytes, bytes);
    uint8_t*             da = (uint8_t*)c.dalloc((size_t)w + 1);
    uint8_t*             dl = (uint8_t*)c.dalloc((size_t)h);
    uint8_t*             dd = (uint8_t*)c.dalloc((size_t)w * h);
    SvtHipIntraPredDesc* dv = (SvtHipIntraPredDesc*)c.dalloc(sizeof(SvtHipIntraPredDesc));
    c.up(da, above - 1, (size_t)w + 1);
    c.up(dl, left, (size_t)h);
    SvtHipIntraPredDesc d{};
    d.top_off = 1, d.left_plane = 1, d.left_stride = 1, d.dst_stride = (uint32_t)w;
    d.w = (uint8_t)w, d.h = (uint8_t)h, d.filter_intra_mode = (uint8_t)mode, d.n_top_px = (uint8_t)w, d.n_left_px = (uint8_t)h;
    c.up(dv, &d, sizeof(d));
    SvtHipIntraPredPlanes planes{};
    planes.base[0] = da, planes.base[1] = dl;
    Aux aux{};
    aux.bd = 8;
    launch<false>(planes, dd, dv, 1, nullptr, aux, c.stream);
    c.down2d(dst, (size_t)stride, dd, (size_t)w, (size_t)w, h);
}
// svt_cfl_predict_{lbd,hbd}: width x height of pred_buf_q3 (rows of CFL_BUF_LINE) and of pred are read; dst may be pred
template <typename PIX>
void cfl_predict_host(const int16_t* q3, const PIX* pred, const int pred_stride, PIX* dst, const int dst_stride, const int alpha_q3, const int bit_depth, const int w,
                      const int h) {
    if (!q3 || !pred || !dst || !cfl_size_ok((uint32_t)w, (uint32_t)h) || bit_depth < 8 || bit_depth > 12 || alpha_q3 < -32768 || alpha_q3 > 32767) return;
    const size_t      px = sizeof(PIX);
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = (size_t)h * CFL_LINE * 2 + 2 * (size_t)w * h * px + 4096;
    c.reserve(bytes, bytes);
    int16_t*           dq = (int16_t*)c.dalloc((size_t)h * CFL_LINE * 2);
    PIX*               dp = (PIX*)c.dalloc((size_t)w * h * px);
    PIX*               dd = (PIX*)c.dalloc((size_t)w * h * px);
    SvtHipCflPredDesc* dv = (SvtHipCflPredDesc*)c.dalloc(sizeof(SvtHipCflPredDesc));
    c.up2d(dq, (size_t)CFL_LINE * 2, q3, (size_t)CFL_LINE * 2, (size_t)w * 2, h);
    c.up2d(dp, (size_t)w * px, pred, (size_t)pred_stride * px, (size_t)w * px, h);
    SvtHipCflPredDesc d{};
    d.pred_stride[0] = d.dst_stride[0] = (uint32_t)w;
    d.alpha_q3[0]    = (int16_t)alpha_q3;
    d.w = (uint8_t)w, d.h = (uint8_t)h, d.n_targets = 1;
    c.up(dv, &d, sizeof(d));
    SvtHipIntraPredPlanes planes{};
    planes.base[0] = dp;
    cfl_launch<2>(planes, dd, dv, 1, nullptr, bit_depth, px == 2, dq, c.stream);
    c.down2d(dst, (size_t)dst_stride * px, dd, (size_t)w * px, (size_t)w * px, h);
}
// svt_cfl_luma_subsampling_420_{lbd,hbd}: width x height LUMA samples are read, (width / 2) x (height / 2) Q3 values written in rows of CFL_BUF_LINE
template <typename PIX>
void cfl_subsample_host(const PIX* input, const int input_stride, int16_t* out_q3, const int width, const int height) {
    if (!input || !out_q3 || (width & 1) || (height & 1) || !cfl_size_ok((uint32_t)width >> 1, (uint32_t)height >> 1)) return;
    const int         w = width >> 1, h = height >> 1;
    const size_t      px = sizeof(PIX);
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = (size_t)h * CFL_LINE * 2 + (size_t)width * height * px + 4096;
    c.reserve(bytes, bytes);
    int16_t*           dq = (int16_t*)c.dalloc((size_t)h * CFL_LINE * 2);
    PIX*               dl = (PIX*)c.dalloc((size_t)width * height * px);
    SvtHipCflPredDesc* dv = (SvtHipCflPredDesc*)c.dalloc(sizeof(SvtHipCflPredDesc));
    c.up2d(dl, (size_t)width * px, input, (size_t)input_stride * px, (size_t)width * px, height);
    SvtHipCflPredDesc d{};
    d.luma_stride = (uint32_t)width;
    d.w = (uint8_t)w, d.h = (uint8_t)h, d.n_targets = 1;
    c.up(dv, &d, sizeof(d));
    SvtHipIntraPredPlanes planes{};
    planes.base[0] = dl;
    cfl_launch<1>(planes, dl, dv, 1, nullptr, 8, px == 2, dq, c.stream);
    c.down2d(out_q3, (size_t)CFL_LINE * 2, dq, (size_t)CFL_LINE * 2, (size_t)w * 2, h);
}

} // namespace

extern "C" {

int svt_hip_intra_pred_batch(SvtHipIntraPredPlanes planes, void* dst_base, const SvtHipIntraPredDesc* descs, uint32_t n, int bit_depth, uint8_t* status, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!dst_base || !descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status) {
        // the descriptors live in device memory: a small kernel reads them, the host waits for its one word and launches nothing if it is set
        svthip::HostCall& c = svthip::host_call();
        c.begin_small();
        c.reserve(0, 256);
        uint32_t* bad = (uint32_t*)c.palloc(64);
        *bad          = 0;
        hipLaunchKernelGGL(intra_pred_check_kernel, dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, planes, descs, n, bad);
        SVT_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        if (*(volatile uint32_t*)bad) return -1;
    }
    Aux aux{};
    aux.bd = bit_depth;
    launch<false>(planes, dst_base, descs, n, status, aux, st);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_cfl_pred_batch(SvtHipIntraPredPlanes planes, void* dst_base, const SvtHipCflPredDesc* descs, uint32_t n, int bit_depth, uint8_t* status, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!dst_base || !descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st = (hipStream_t)stream;
    if (!status) {
        svthip::HostCall& c = svthip::host_call();
        c.begin_small();
        c.reserve(0, 256);
        uint32_t* bad = (uint32_t*)c.palloc(64);
        *bad          = 0;
        hipLaunchKernelGGL(cfl_check_kernel, dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, planes, descs, n, bad);
        SVT_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        if (*(volatile uint32_t*)bad) return -1;
    }
    cfl_launch<0>(planes, dst_base, descs, n, status, bit_depth, bit_depth > 8, nullptr, st);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

#define SVT_HIP_FORM_GUARD(call)                     \
    if (svthip::failed()) return;                    \
    try {                                            \
        svthip::ensure_device();                     \
        call;                                        \
    } catch (const svthip::DeviceError&) {}

void svt_av1_dr_prediction_z1_hip(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above, const uint8_t* left, int32_t upsample_above, int32_t dx,
                                  int32_t dy) {
    SVT_HIP_FORM_GUARD(dr_host<uint8_t>(dst, stride, bw, bh, above, left, upsample_above, 0, dx, 1, 8, 1))
    (void)dy;
}
void svt_av1_dr_prediction_z2_hip(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above, const uint8_t* left, int32_t upsample_above,
                                  int32_t upsample_left, int32_t dx, int32_t dy) {
    SVT_HIP_FORM_GUARD(dr_host<uint8_t>(dst, stride, bw, bh, above, left, upsample_above, upsample_left, dx, dy, 8, 2))
}
void svt_av1_dr_prediction_z3_hip(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above, const uint8_t* left, int32_t upsample_left, int32_t dx,
                                  int32_t dy) {
    SVT_HIP_FORM_GUARD(dr_host<uint8_t>(dst, stride, bw, bh, above, left, 0, upsample_left, 1, dy, 8, 3))
    (void)dx;
}
void svt_av1_highbd_dr_prediction_z1_hip(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t* above, const uint16_t* left, int32_t upsample_above,
                                         int32_t dx, int32_t dy, int32_t bd) {
    SVT_HIP_FORM_GUARD(dr_host<uint16_t>(dst, stride, bw, bh, above, left, upsample_above, 0, dx, 1, bd, 1))
    (void)dy;
}
void svt_av1_highbd_dr_prediction_z2_hip(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t* above, const uint16_t* left, int32_t upsample_above,
                                         int32_t upsample_left, int32_t dx, int32_t dy, int32_t bd) {
    SVT_HIP_FORM_GUARD(dr_host<uint16_t>(dst, stride, bw, bh, above, left, upsample_above, upsample_left, dx, dy, bd, 2))
}
void svt_av1_highbd_dr_prediction_z3_hip(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t* above, const uint16_t* left, int32_t upsample_left,
                                         int32_t dx, int32_t dy, int32_t bd) {
    SVT_HIP_FORM_GUARD(dr_host<uint16_t>(dst, stride, bw, bh, above, left, 0, upsample_left, 1, dy, bd, 3))
    (void)dx;
}
void svt_av1_filter_intra_predictor_hip(uint8_t* dst, ptrdiff_t stride, SvtHipTxSize tx_size, const uint8_t* above, const uint8_t* left, int32_t mode) {
    SVT_HIP_FORM_GUARD(filter_intra_host(dst, stride, (int)tx_size, above, left, mode))
}
void svt_cfl_predict_lbd_hip(const int16_t* pred_buf_q3, uint8_t* pred, int32_t pred_stride, uint8_t* dst, int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth,
                             int32_t width, int32_t height) {
    SVT_HIP_FORM_GUARD(cfl_predict_host<uint8_t>(pred_buf_q3, pred, pred_stride, dst, dst_stride, alpha_q3, bit_depth, width, height))
}
void svt_cfl_predict_hbd_hip(const int16_t* pred_buf_q3, uint16_t* pred, int32_t pred_stride, uint16_t* dst, int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth,
                             int32_t width, int32_t height) {
    SVT_HIP_FORM_GUARD(cfl_predict_host<uint16_t>(pred_buf_q3, pred, pred_stride, dst, dst_stride, alpha_q3, bit_depth, width, height))
}
void svt_cfl_luma_subsampling_420_lbd_hip(const uint8_t* input, int32_t input_stride, int16_t* output_q3, int32_t width, int32_t height) {
    SVT_HIP_FORM_GUARD(cfl_subsample_host<uint8_t>(input, input_stride, output_q3, width, height))
}
void svt_cfl_luma_subsampling_420_hbd_hip(const uint16_t* input, int32_t input_stride, int16_t* output_q3, int32_t width, int32_t height) {
    SVT_HIP_FORM_GUARD(cfl_subsample_host<uint16_t>(input, input_stride, output_q3, width, height))
}
#undef SVT_HIP_FORM_GUARD

} // extern "C"
