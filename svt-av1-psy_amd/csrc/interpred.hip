// interpred.hip -- the first arrow of the mode-decision loop (PREDICTION -> residual -> transform -> quantise -> inverse + reconstruction -> distortion) for
// gfx950: AV1 inter prediction of n independent blocks of mixed sizes from read-only reference planes, i.e. the sixteen functions behind the reference's dispatch tables
// svt_aom_convolve[subx][suby][compound] / svt_aom_convolveHbd[...] (inter_prediction.c:311-418, 494-668, 670-777, 852-1063), bit for bit, at 8, 10 and 12 bit.
// DESIGN.md 4.20 has the layout, the readable-extent contract, the reference's narrowings and the bound.
//
//  * inter_pred_kernel: one launch, n descriptors.  A workgroup (4 waves) takes DPW = 16 consecutive descriptors and flattens their tiles into one list (prefix sum of
//    the tile counts in LDS, as dist.hip does); a tile is min(w, 32) columns by min(h, 512 / columns) rows -- at most 512 samples, eight per lane; a block of fewer than 512
//    samples is one tile (or, wider than 32, several) that fills only part of that: 16x16 four of the eight sample slots, 8x8 one --
//    and ONE WAVE owns a tile: the wave's branch on (copy / x / y / 2-D, compound) is uniform, nothing crosses waves, nothing is reduced.  blockIdx.y splits the list of
//    one descriptor group four ways, so that 64x64 and 128x128 blocks (8 and 32 tiles each) still spread over the machine.
//  * the 2-D case filters the th + 7 rows a tile touches horizontally into the wave's own LDS slice (row PAIRS packed in one dword, 1.5 KB per wave) and runs the
//    vertical pass as v_dot2_i32_i16 over those pairs; the horizontal sums are v_dot4_i32_i8 on (sample - 128) at 8 bit and v_dot2_i32_i16 at 10 / 12 bit.
//  * compound: both references are filtered by the same wave, the first one's ConvBufType values stay in eight registers per lane; the intermediate buffer of the
//    reference's two calls never reaches memory.
//  * masked compound (COMPOUND_WEDGE / COMPOUND_DIFFWTD): a third template parameter; the same two passes, then the d16 blend on the two register-held values with a wedge,
//    explicit or diff-weighted mask.  The unmasked instantiations compile to what they compiled to before it existed.
//  * no global atomics, nothing to zero beforehand, every output sample is written exactly once by plain stores: results do not depend on launch order.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include "maskpred_tables.h"
#include <type_traits>

namespace svthip { const uint8_t* wedge_table(hipStream_t st); } // maskpred.hip: the device's 100 352-byte wedge table, generated at first use

namespace {
using namespace svt_maskpred; // kBw, kBh, kSlotOff, wedge_slot: the wedge table's layout

constexpr int DPW     = 16;           // descriptors per workgroup group
constexpr int TPB     = 256;          // threads per workgroup
constexpr int WAVES   = TPB / 64;
constexpr int SPLIT   = 4;            // workgroups (blockIdx.y) that share one descriptor group's tile list
constexpr int TILE_W  = 32;           // widest tile
constexpr int TILE_PX = 512;          // samples per tile
constexpr int NPL     = TILE_PX / 64; // samples per lane
constexpr int IM_DW   = TILE_PX / 2 + 4 * TILE_W; // dwords of one wave's intermediate slice: (th / 2 + 4) row pairs of tw columns, th * tw <= 512, tw <= 32

// The six kernels of inter_prediction.c:223-254, :1065-1129 (AV1 specification, 7.11.3.4), one row per sub-pel phase.
constexpr int16_t kFilters[6][16][8] = {
    // 0 EIGHTTAP_REGULAR (sub_pel_filters_8)
    {{0, 0, 0, 128, 0, 0, 0, 0},      {0, 2, -6, 126, 8, -2, 0, 0},    {0, 2, -10, 122, 18, -4, 0, 0},  {0, 2, -12, 116, 28, -8, 2, 0},
     {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -14, 102, 48, -12, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0},  {0, 2, -14, 84, 66, -12, 2, 0},
     {0, 2, -14, 76, 76, -14, 2, 0},  {0, 2, -12, 66, 84, -14, 2, 0},  {0, 2, -12, 58, 94, -16, 2, 0},  {0, 2, -12, 48, 102, -14, 2, 0},
     {0, 2, -10, 38, 110, -14, 2, 0}, {0, 2, -8, 28, 116, -12, 2, 0},  {0, 0, -4, 18, 122, -10, 2, 0},  {0, 0, -2, 8, 126, -6, 2, 0}},
    // 1 EIGHTTAP_SMOOTH (sub_pel_filters_8smooth)
    {{0, 0, 0, 128, 0, 0, 0, 0},   {0, 2, 28, 62, 34, 2, 0, 0},   {0, 0, 26, 62, 36, 4, 0, 0},    {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0},  {0, 0, 18, 58, 44, 8, 0, 0},   {0, 0, 16, 56, 46, 10, 0, 0},   {0, -2, 16, 54, 48, 12, 0, 0},
     {0, -2, 14, 52, 52, 14, -2, 0}, {0, 0, 12, 48, 54, 16, -2, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0},  {0, 0, 4, 40, 62, 22, 0, 0},   {0, 0, 4, 36, 62, 26, 0, 0},    {0, 0, 2, 34, 62, 28, 2, 0}},
    // 2 MULTITAP_SHARP (sub_pel_filters_8sharp)
    {{0, 0, 0, 128, 0, 0, 0, 0},         {-2, 2, -6, 126, 8, -2, 2, 0},      {-2, 6, -12, 124, 16, -6, 4, -2},   {-2, 8, -18, 120, 26, -10, 6, -2},
     {-4, 10, -22, 116, 38, -14, 6, -2}, {-4, 10, -22, 108, 48, -18, 8, -2}, {-4, 10, -24, 100, 60, -20, 8, -2}, {-4, 10, -24, 90, 70, -22, 10, -2},
     {-4, 12, -24, 80, 80, -24, 12, -4}, {-2, 10, -22, 70, 90, -24, 10, -4}, {-2, 8, -20, 60, 100, -24, 10, -4}, {-2, 8, -18, 48, 108, -22, 10, -4},
     {-2, 6, -14, 38, 116, -22, 10, -4}, {-2, 6, -10, 26, 120, -18, 8, -2},  {-2, 4, -6, 16, 124, -12, 6, -2},   {0, 2, -2, 8, 126, -6, 2, -2}},
    // 3 BILINEAR (bilinear_filters)
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 0, 120, 8, 0, 0, 0},  {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 104, 24, 0, 0, 0},
     {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 88, 40, 0, 0, 0},  {0, 0, 0, 80, 48, 0, 0, 0},  {0, 0, 0, 72, 56, 0, 0, 0},
     {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 56, 72, 0, 0, 0},  {0, 0, 0, 48, 80, 0, 0, 0},  {0, 0, 0, 40, 88, 0, 0, 0},
     {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 24, 104, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}, {0, 0, 0, 8, 120, 0, 0, 0}},
    // 4 sub_pel_filters_4: REGULAR and SHARP of a dimension <= 4 (inter_prediction.h:137-145)
    {{0, 0, 0, 128, 0, 0, 0, 0},     {0, 0, -4, 126, 8, -2, 0, 0},    {0, 0, -8, 122, 18, -4, 0, 0},   {0, 0, -10, 116, 28, -6, 0, 0},
     {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -12, 102, 48, -10, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0},  {0, 0, -12, 84, 66, -10, 0, 0},
     {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 66, 84, -12, 0, 0},  {0, 0, -10, 58, 94, -14, 0, 0},  {0, 0, -10, 48, 102, -12, 0, 0},
     {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0},  {0, 0, -4, 18, 122, -8, 0, 0},   {0, 0, -2, 8, 126, -4, 0, 0}},
    // 5 sub_pel_filters_4smooth: SMOOTH of a dimension <= 4
    {{0, 0, 0, 128, 0, 0, 0, 0},  {0, 0, 30, 62, 34, 2, 0, 0},  {0, 0, 26, 62, 36, 4, 0, 0},  {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0},  {0, 0, 16, 56, 46, 10, 0, 0}, {0, 0, 14, 54, 48, 12, 0, 0},
     {0, 0, 12, 52, 52, 12, 0, 0}, {0, 0, 12, 48, 54, 14, 0, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0},  {0, 0, 4, 36, 62, 26, 0, 0},  {0, 0, 2, 34, 62, 30, 0, 0}}};

// the eight taps of one (kernel, phase) as the dot instructions take them: b4 = four signed bytes per dword (valid when fits8), h2 = two signed halves per dword;
// bias = 128 * (sum of the taps), what the v_dot4_i32_i8 form on (sample - 128) has to add back
struct Taps { uint32_t b4[2], h2[4]; int32_t bias; uint32_t fits8; };
constexpr Taps pack_taps(const int16_t* f) {
    Taps t{};
    int  sum = 0, fits = 1;
    for (int k = 0; k < 8; k++) {
        t.b4[k >> 2] |= (uint32_t)(f[k] & 0xff) << (8 * (k & 3));
        t.h2[k >> 1] |= (uint32_t)(f[k] & 0xffff) << (16 * (k & 1));
        sum += f[k];
        if (f[k] < -128 || f[k] > 127) fits = 0;
    }
    t.bias  = 128 * sum;
    t.fits8 = (uint32_t)fits;
    return t;
}
struct TapTables { Taps t[6][16]; };
constexpr TapTables make_tap_tables() {
    TapTables T{};
    for (int kind = 0; kind < 6; kind++)
        for (int p = 0; p < 16; p++) T.t[kind][p] = pack_taps(kFilters[kind][p]);
    return T;
}
__device__ constexpr TapTables kTaps = make_tap_tables();
// av1_get_interp_filter_params_with_block_size (inter_prediction.h:137-145): the kernel of `filter` for a block dimension `dim`
__device__ __forceinline__ int filter_kind(const int filter, const int dim) {
    if (dim <= 4 && filter != 3) return filter == 1 ? 5 : 4;
    return filter;
}

// what a launch carries besides the descriptors.  The batched entry sets the roundings of get_conv_params_no_round (convolve.h:40-64); the single-call forms pass
// their caller's ConvolveParams, their caller's taps and the case their NAME stands for.
struct Aux {
    uint16_t* cb;        // modes 1, 2: the caller's ConvBufType block (row stride cb_stride), block-relative
    uint32_t  cb_stride;
    int32_t   mode;      // 0: whole prediction; 1: reference 0 as the compound functions' do_average = 0 call -> cb; 2: reference 0 as their do_average = 1 call on cb
    int32_t   force_case; // single-call forms: the case (bit 0: x filtered, bit 1: y filtered); the batched entry takes it from the phases
    int32_t   bd, r0, r1_single, r1_compound;
    Taps      tx, ty;    // single-call forms: the caller's taps
    // the masked instantiation only (last, so that the other instantiations' argument loads stay where they were)
    const uint8_t* wedge;     // the wedge table of maskpred.hip
    const uint8_t* mask_base; // EXPLICIT masks
    uint8_t*       seg_base;  // DIFFWTD: where the mask is stored, or NULL
};

__host__ __device__ __forceinline__ bool dim_ok(const uint32_t v) { return v >= 2 && v <= 128 && (v & (v - 1)) == 0; }
// everything the kernel relies on: sizes, phases, filters, the compound mode, plane indices with a base
__host__ __device__ __forceinline__ bool desc_ok(const SvtHipInterPredDesc& d, const SvtHipInterPredPlanes& planes) {
    if (!dim_ok(d.w) || !dim_ok(d.h) || d.filter_x > 3 || d.filter_y > 3 || d.compound > 2) return false;
    const int nref = d.compound ? 2 : 1;
    for (int k = 0; k < nref; k++)
        if (d.subpel_x[k] > 15 || d.subpel_y[k] > 15 || d.plane[k] >= 32 || planes.base[d.plane[k]] == nullptr) return false;
    return true;
}
__device__ __forceinline__ bool desc_ok(const SvtHipInterPredMaskedDesc& m, const SvtHipInterPredPlanes& planes, const uint8_t* mask_base) {
    SvtHipInterPredDesc d = m.p;
    d.compound            = 1; // always two references
    if (!desc_ok(d, planes) || d.w < 4 || d.h < 4 || m.comp_type > SVT_HIP_COMP_EXPLICIT || m.subw > 1 || m.subh > 1) return false; // (the d16 functions' lower bound)
    if (m.comp_type == SVT_HIP_COMP_WEDGE)
        return wedge_slot(m.bsize) >= 0 && m.wedge_index <= 15 && m.wedge_sign <= 1 && ((uint32_t)d.w << m.subw) <= kBw[m.bsize] && ((uint32_t)d.h << m.subh) <= kBh[m.bsize];
    if (m.comp_type == SVT_HIP_COMP_DIFFWTD) return m.mask_type <= 1 && m.subw == 0 && m.subh == 0;
    return mask_base != nullptr;
}
__device__ __forceinline__ const SvtHipInterPredDesc& desc_base(const SvtHipInterPredDesc& d) { return d; }
__device__ __forceinline__ const SvtHipInterPredDesc& desc_base(const SvtHipInterPredMaskedDesc& d) { return d.p; }
__device__ __forceinline__ int load_byte(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }

// The tiling of a w x h block, the ONE place that knows it: tiles of 2^lw = min(w, 32) columns by th = min(h, 512 >> lw) rows, ntx across and nty down.  The prefix
// sum counts ntx * nty tiles and the tile loop lays them out with the same three numbers (a 64x8 block is two 32x8 tiles, not 64 * 8 / 512 = one).
struct Tiling { int lw, th; uint32_t ntx, nty; };
__host__ __device__ __forceinline__ Tiling tiling_of(const uint32_t w, const uint32_t h) {
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
__host__ __device__ __forceinline__ uint32_t tile_count(const uint32_t w, const uint32_t h) {
    const Tiling t = tiling_of(w, h);
    return t.ntx * t.nty;
}

__device__ __forceinline__ int rpot(const int v, const int n) { return (v + ((1 << n) >> 1)) >> n; } // ROUND_POWER_OF_TWO (definitions.h:459), n >= 0
__device__ __forceinline__ int sdot2(const uint32_t a, const uint32_t b, const int c) { // c + a.lo * b.lo + a.hi * b.hi, signed 16 bit (v_dot2_i32_i16)
    typedef short s2 __attribute__((ext_vector_type(2)));
    s2 x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return __builtin_amdgcn_sdot2(x, y, c, false);
}
__device__ __forceinline__ int tap_of(const Taps& t, const int k) { return (int)(int16_t)(t.h2[k >> 1] >> (16 * (k & 1))); }
__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int load_px(const uint16_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint16_t*)p; }

// sum over the eight taps of tap * sample for the samples q[0 .. 7]: ONE unaligned load of exactly those eight samples
__device__ __forceinline__ int hsum8(const uint8_t* q, const Taps& t) {
    const svt_u32x2_a1 v = svt_hip_global_load_x2(q);
    if (t.fits8) return __builtin_amdgcn_sdot4((int)(v[0] ^ 0x80808080u), (int)t.b4[0], __builtin_amdgcn_sdot4((int)(v[1] ^ 0x80808080u), (int)t.b4[1], t.bias, false), false);
    // a tap outside a signed byte (the identity kernel's 128, a caller's own table): bytes widened to halves
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = v[k >> 1] >> (16 * (k & 1));
        s                = sdot2((w & 0xffu) | ((w & 0xff00u) << 8), t.h2[k], s);
    }
    return s;
}
__device__ __forceinline__ int hsum8(const uint16_t* q, const Taps& t) {
    const svt_u32x4_a2 v = svt_hip_global_load_x4(q);
    return sdot2(v[0], t.h2[0], sdot2(v[1], t.h2[1], sdot2(v[2], t.h2[2], sdot2(v[3], t.h2[3], 0))));
}

// One reference of one tile -> v[j] for the lane's samples i = l + 64 j (i < npx; sample i is column i & (tw - 1), row i >> lw of the tile at p0):
//   compound == false: the value the `_sr` function clips and stores; compound == true: `res` of the `jnt_` function, before it is stored or averaged.
// cs: bit 0 = filtered in x, bit 1 = filtered in y -- wave-uniform, as is everything but l.
template <typename PIX>
__device__ __forceinline__ void reference_pass(int (&v)[NPL], const PIX* __restrict__ p0, const uint32_t stride, const int cs, const Taps& tx, const Taps& ty,
                                               const bool compound, const int bd, const int r0, const int r1, const int lw, const int th, uint32_t* __restrict__ imp,
                                               const int l) {
    const int  tw = 1 << lw, npx = th << lw;
    const int  nj = npx >= 64 ? npx >> 6 : 1; // npx is a power of two: whole rounds of 64 lanes, or one partial round -- `j < nj` is a scalar branch, `on` one mask
    const bool on = l < npx;
    const int ob = bd + 14 - r0, ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), rb = 14 - r0 - r1; // offset_bits, round_offset, round_bits / bits of the 2-D functions
    if (cs == 0) {
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const int px = load_px(p0 + ((uint32_t)(i >> lw) * stride + (uint32_t)(i & (tw - 1))));
                v[j]         = compound ? (int)(uint16_t)((px << rb) + ro) : px; // jnt_convolve_2d_copy shifts and offsets in 16 bits (:650-651)
            }
        }
    } else if (cs == 1) {
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const int s = rpot(hsum8(p0 - 3 + ((uint32_t)(i >> lw) * stride + (uint32_t)(i & (tw - 1))), tx), r0);
                v[j]        = compound ? (1 << (7 - r1)) * s + ro : rpot(s, 7 - r0);
            }
        }
    } else if (cs == 2) {
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const PIX*     pb = p0 - (long)3 * (long)stride;
                const uint32_t o  = (uint32_t)(i >> lw) * stride + (uint32_t)(i & (tw - 1));
                int            s  = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) s += tap_of(ty, k) * load_px(pb + (o + (uint32_t)k * stride));
                v[j] = compound ? rpot(s * (1 << (7 - r0)), r1) + ro : rpot(s, 7);
            }
        }
    } else {
        // horizontal pass of the th + 7 rows the tile touches -> imp, rounded and narrowed like the reference's int16_t im_block; im row y <-> tile row y - 3.  A lane
        // filters rows 2m and 2m + 1 at one column and stores them as ONE dword, so that the vertical pass is v_dot2_i32_i16 on row pairs.
        const PIX* pb     = p0 - (long)3 * (long)stride - 3;
        const int  imrows = th + 7, npairs = (imrows + 1) >> 1;
        for (int i = l; i < (npairs << lw); i += 64) {
            const int  m = i >> lw;
            const PIX* q = pb + ((uint32_t)(2 * m) * stride + (uint32_t)(i & (tw - 1)));
            const int  a = rpot(hsum8(q, tx) + (1 << (bd + 6)), r0);
            const int  b = 2 * m + 1 < imrows ? rpot(hsum8(q + stride, tx) + (1 << (bd + 6)), r0) : 0; // (never read; keeps the loads inside the rows the reference reads)
            imp[i]       = (uint32_t)(a & 0xffff) | ((uint32_t)b << 16);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = l + 64 * j;
            if (j < nj && on) {
                const int       y  = i >> lw;
                const uint32_t* c  = imp + ((y >> 1) << lw) + (i & (tw - 1));
                const uint32_t  sh = (uint32_t)(y & 1) << 4; // odd rows: the pair (y, y + 1) straddles two stored pairs
                int             s  = 1 << ob;
                uint32_t        lo = c[0];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t hi = c[(k + 1) << lw];
                    s                 = sdot2(__builtin_amdgcn_alignbit(hi, lo, sh), ty.h2[k], s);
                    lo                = hi;
                }
                int res = rpot(s, r1);
                if (compound) res = (int)(uint16_t)res; // ConvBufType res (:530, :1017)
                else {
                    res -= ro;
                    if (sizeof(PIX) == 1) res = (int16_t)res; // the 8-bit function narrows before the last rounding (:345)
                    res = rpot(res, rb);
                }
                v[j] = res;
            }
        }
        __builtin_amdgcn_wave_barrier(); // the slice is rewritten by the next reference / tile
    }
}

// FORM = false: the batched entry (AV1's tables, the roundings of get_conv_params_no_round, the case follows the phases); FORM = true: one block of a single-call form
// (the caller's taps and roundings, the case its name stands for, aux.mode).
// MASKED: the masked compound of svt_aom_build_masked_compound_no_round (inter_prediction.c:2227): descriptors are SvtHipInterPredMaskedDesc, both references are
// always filtered, and the last step is svt_aom_lowbd_ / highbd_blend_a64_d16_mask_c (blend_a64_mask.c:34, :105) on the two ConvBufType values, the mask a wedge, bytes
// of aux.mask_base, or svt_av1_build_compound_diffwtd_mask_d16_c (C_DEFAULT/inter_prediction_c.c:15) on those same two values.
template <typename PIX, bool FORM, bool MASKED = false>
__global__ __launch_bounds__(TPB) void inter_pred_kernel(const SvtHipInterPredPlanes planes, PIX* __restrict__ dst_base,
                                                         const std::conditional_t<MASKED, SvtHipInterPredMaskedDesc, SvtHipInterPredDesc>* __restrict__ descs,
                                                         const uint32_t n, uint8_t* __restrict__ status, const Aux aux) {
    typedef std::conditional_t<MASKED, SvtHipInterPredMaskedDesc, SvtHipInterPredDesc> DESC;
    __shared__ uint32_t pre[DPW + 1];         // exclusive prefix sum of the tile counts
    __shared__ uint32_t im[WAVES][IM_DW];     // the waves' intermediate slices
    const int      tid = threadIdx.x, l = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t first = blockIdx.x * DPW;
    if (tid < 64) { // (the first wave, whole: the scan's shuffles are wave-uniform)
        uint32_t cnt = 0;
        if (tid < DPW && first + tid < n) {
            const DESC dd = descs[first + tid];
            bool       ok;
            if constexpr (MASKED) ok = desc_ok(dd, planes, aux.mask_base);
            else ok = desc_ok(dd, planes);
            if (ok) cnt = tile_count(desc_base(dd).w, desc_base(dd).h);
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
    const int      bd = aux.bd, r0 = aux.r0, maxv = (1 << bd) - 1;
    for (uint32_t u = blockIdx.y * WAVES + wv; u < total; u += gridDim.y * WAVES) { // (u depends on the wave only)
        int di = 0;
#pragma unroll
        for (int s = DPW >> 1; s >= 1; s >>= 1)
            if (pre[di + s] <= u) di += s;
        di = __builtin_amdgcn_readfirstlane(di); // the descriptor, and every branch taken on it, is the wave's: scalar loads, scalar branches
        const DESC                 dm = descs[first + di];
        const SvtHipInterPredDesc& d  = desc_base(dm);
        const int      w = d.w, h = d.h;
        const Tiling   tl = tiling_of((uint32_t)w, (uint32_t)h);
        const int      lw = tl.lw, tw = 1 << lw, th = tl.th, npx = th << lw;
        const int      nj = npx >= 64 ? npx >> 6 : 1;
        const bool     on = l < npx;
        const uint32_t loc = u - pre[di], ntx = tl.ntx, tyi = loc / ntx, txi = loc - tyi * ntx;
        const uint32_t x0 = txi << lw, y0 = tyi * (uint32_t)th;
        const bool     compound = MASKED ? true : (FORM ? aux.mode != 0 : d.compound != 0);
        const int      r1 = compound ? aux.r1_compound : aux.r1_single;
        const int      npass = MASKED ? 2 : (!FORM && d.compound != 0 ? 2 : 1);
        const int      ob = bd + 14 - r0, ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), rb = 14 - r0 - r1;
        PIX*           out = dst_base + d.dst_off + (size_t)y0 * d.dst_stride + x0;
        int            a[NPL] = {}; // the first reference's ConvBufType values
        const uint8_t* mp = nullptr; // MASKED, WEDGE / EXPLICIT: the mask's bytes, its stride and sub-sampling
        uint32_t       ms = 0;
        int            subw = 0, subh = 0, ctype = 0, inv = 0;
        uint64_t       seg_off = 0;
        if constexpr (MASKED) {
            ctype = dm.comp_type, subw = dm.subw, subh = dm.subh, inv = dm.mask_type, seg_off = dm.seg_off;
            if (ctype == SVT_HIP_COMP_WEDGE) {
                ms = kBw[dm.bsize];
                mp = aux.wedge + kSlotOff[wedge_slot(dm.bsize)] + (uint32_t)(dm.wedge_index * 2 + dm.wedge_sign) * ms * kBh[dm.bsize];
            } else if (ctype == SVT_HIP_COMP_EXPLICIT) {
                ms = dm.mask_stride;
                mp = aux.mask_base + dm.mask_off;
            }
        }
        for (int pass = 0; pass < npass; pass++) {
            const int      sx = pass ? d.subpel_x[1] : d.subpel_x[0], sy = pass ? d.subpel_y[1] : d.subpel_y[0];
            const uint32_t stride = pass ? d.src_stride[1] : d.src_stride[0];
            const PIX*     p0 = (const PIX*)planes.base[pass ? d.plane[1] : d.plane[0]] + (pass ? d.src_off[1] : d.src_off[0]) + (size_t)y0 * stride + x0;
            const int      cs = FORM ? aux.force_case : (sx != 0) + 2 * (sy != 0);
            const Taps     tx = FORM ? aux.tx : kTaps.t[filter_kind(d.filter_x, w)][sx];
            const Taps     ty = FORM ? aux.ty : kTaps.t[filter_kind(d.filter_y, h)][sy];
            int            v[NPL];
            reference_pass<PIX>(v, p0, stride, cs, tx, ty, compound, bd, r0, r1, lw, th, im[wv], l);
            if (!compound) {
#pragma unroll
                for (int j = 0; j < NPL; j++) {
                    const int i = l + 64 * j;
                    if (j < nj && on) out[(size_t)(i >> lw) * d.dst_stride + (i & (tw - 1))] = (PIX)(v[j] < 0 ? 0 : (v[j] > maxv ? maxv : v[j]));
                }
            } else if (FORM && aux.mode == 1) {
#pragma unroll
                for (int j = 0; j < NPL; j++) {
                    const int i = l + 64 * j;
                    if (j < nj && on) aux.cb[(size_t)(y0 + (i >> lw)) * aux.cb_stride + x0 + (i & (tw - 1))] = (uint16_t)v[j];
                }
            } else if (pass + 1 < npass) {
#pragma unroll
                for (int j = 0; j < NPL; j++) a[j] = (int)(uint16_t)v[j]; // as the reference stores it: ConvBufType
            } else {
#pragma unroll
                for (int j = 0; j < NPL; j++) {
                    const int i = l + 64 * j;
                    if (j < nj && on) {
                        int tmp = FORM ? (int)aux.cb[(size_t)(y0 + (i >> lw)) * aux.cb_stride + x0 + (i & (tw - 1))] : a[j];
                        if constexpr (MASKED) {
                            const int      bq = (int)(uint16_t)v[j]; // the second reference as the reference stores it: ConvBufType
                            const uint32_t x = x0 + (uint32_t)(i & (tw - 1)), y = y0 + (uint32_t)(i >> lw);
                            int            m;
                            if (ctype == SVT_HIP_COMP_DIFFWTD) { // diffwtd_mask_d16: round = 2 * FILTER_BITS - round_0 - round_1 + (bd - 8)
                                m = 38 + (rpot(tmp > bq ? tmp - bq : bq - tmp, rb + bd - 8) >> 4); // DIFF_FACTOR 16
                                m = m > 64 ? 64 : m;
                                if (inv) m = 64 - m;
                                if (aux.seg_base) aux.seg_base[seg_off + (size_t)y * (uint32_t)w + x] = (uint8_t)m; // stride w, as the C writes it
                            } else {
                                const uint8_t* q = mp + ((size_t)(y << subh) * ms + (x << subw));
                                m                = load_byte(q);
                                if (subw && subh) m = (m + load_byte(q + ms) + load_byte(q + 1) + load_byte(q + ms + 1) + 2) >> 2;
                                else if (subw) m = (m + load_byte(q + 1) + 1) >> 1; // AOM_BLEND_AVG
                                else if (subh) m = (m + load_byte(q + ms) + 1) >> 1;
                            }
                            tmp = (m * tmp + (64 - m) * bq) >> 6; // a plain shift: the rounding comes once, below (blend_a64_mask.c:23-29)
                        } else if (d.compound == 2) tmp = (tmp * (int)d.fwd_offset + v[j] * (int)d.bck_offset) >> 4; // DIST_PRECISION_BITS
                        else tmp = (tmp + v[j]) >> 1;
                        tmp                 = rpot(tmp - ro, rb);
                        out[(size_t)(i >> lw) * d.dst_stride + (i & (tw - 1))] = (PIX)(tmp < 0 ? 0 : (tmp > maxv ? maxv : tmp));
                    }
                }
            }
        }
    }
}

// descriptors the host cannot read: every thread looks at a few; whoever finds an invalid one stores 1 into the word the host zeroed (plain stores of one value)
__global__ __launch_bounds__(TPB) void inter_pred_check_kernel(const SvtHipInterPredPlanes planes, const SvtHipInterPredDesc* __restrict__ descs, const uint32_t n,
                                                               uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

__global__ __launch_bounds__(TPB) void inter_pred_masked_check_kernel(const SvtHipInterPredPlanes planes, const uint8_t* mask_base,
                                                                      const SvtHipInterPredMaskedDesc* __restrict__ descs, const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !desc_ok(descs[i], planes, mask_base);
    if (bad) *bad_out = 1;
}

Aux batch_aux(const int bd) {
    Aux a{};
    a.bd         = bd;
    a.r0         = bd == 12 ? 5 : 3; // get_conv_params_no_round: ROUND0_BITS, raised while bd + FILTER_BITS - round_0 + 2 > 16
    a.r1_single  = 14 - a.r0;
    a.r1_compound = 7;               // COMPOUND_ROUND1_BITS
    return a;
}
template <bool FORM>
void launch(const SvtHipInterPredPlanes& planes, void* dst_base, const SvtHipInterPredDesc* descs, const uint32_t n, uint8_t* status, const Aux& aux, hipStream_t st) {
    const dim3 grid((n + DPW - 1) / DPW, FORM ? 1 : SPLIT), block(TPB);
    if (aux.bd > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_pred_kernel<uint16_t, FORM>), grid, block, 0, st, planes, (uint16_t*)dst_base, descs, n, status, aux);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_pred_kernel<uint8_t, FORM>), grid, block, 0, st, planes, (uint8_t*)dst_base, descs, n, status, aux);
    SVT_LAUNCH_CHECK();
}

// ---- the single-call forms ------------------------------------------------------------------------------------------------------------------------
// One block from host memory.  `cs` is the case the called function stands for (bit 0: filters in x, bit 1: in y), `jnt` whether it is a jnt_ function.  The part of
// the source the function reads (3 left / above, 4 right / below of the filtered directions only) goes into the call's arena, with one descriptor; the taps are read
// HERE, from filter_ptr + 8 * (subpel & 15), and travel as kernel arguments.  One synchronisation (the download); nothing of the caller's is written before it.
template <typename PIX>
void convolve_host(const PIX* src, const int32_t src_stride, PIX* dst, const int32_t dst_stride, const int32_t w, const int32_t h, const SvtHipInterpFilterParams* fx,
                   const SvtHipInterpFilterParams* fy, const int32_t subpel_x, const int32_t subpel_y, const SvtHipConvolveParams* cp, const int bd, const int cs,
                   const bool jnt) {
    if (!dim_ok((uint32_t)w) || !dim_ok((uint32_t)h)) return;                           // not an AV1 block: nothing is written
    if (((cs & 1) && (!fx || fx->taps != 8)) || ((cs & 2) && (!fy || fy->taps != 8))) return; // every InterpFilterParams of AV1 has SUBPEL_TAPS taps
    if ((cs || jnt) && !cp) return;
    if (sizeof(PIX) == 1 ? bd != 8 : (bd != 10 && bd != 12)) return; // (the sample type of the launch follows bd)
    // the roundings become shift counts on the device: only what keeps every one of them non-negative is accepted (svtav1_hip.h states the range)
    if (cp && (cp->round_0 < 0 || cp->round_0 > 7 || cp->round_1 < 0 || cp->round_0 + cp->round_1 > 14 || (jnt && cp->round_1 > 7))) return;
    Aux aux{};
    aux.force_case = cs;
    aux.bd         = bd;
    aux.r0         = cp ? cp->round_0 : 3;
    aux.r1_single = aux.r1_compound = cp ? cp->round_1 : 11;
    static const int16_t unit[8] = {0, 0, 0, 128, 0, 0, 0, 0};
    aux.tx = pack_taps((cs & 1) ? fx->filter_ptr + 8 * (subpel_x & 15) : unit);
    aux.ty = pack_taps((cs & 2) ? fy->filter_ptr + 8 * (subpel_y & 15) : unit);
    const bool average = jnt && cp->do_average;
    aux.mode           = jnt ? (average ? 2 : 1) : 0;

    const int    L = (cs & 1) ? 3 : 0, R = (cs & 1) ? 4 : 0, T = (cs & 2) ? 3 : 0, B = (cs & 2) ? 4 : 0;
    const size_t sw = (size_t)(w + L + R), sh = (size_t)(h + T + B), px = sizeof(PIX);
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = sw * sh * px + (size_t)w * h * (px + 2) + 4096;
    c.reserve(bytes, bytes);
    PIX*                 ds = (PIX*)c.dalloc(sw * sh * px);
    PIX*                 dd = (PIX*)c.dalloc((size_t)w * h * px);
    uint16_t*            db = (uint16_t*)c.dalloc((size_t)w * h * 2);
    SvtHipInterPredDesc* dv = (SvtHipInterPredDesc*)c.dalloc(sizeof(SvtHipInterPredDesc));
    c.up2d(ds, sw * px, src - (ptrdiff_t)T * src_stride - L, (size_t)src_stride * px, sw * px, sh);
    if (average) c.up2d(db, (size_t)w * 2, cp->dst, (size_t)cp->dst_stride * 2, (size_t)w * 2, h);
    SvtHipInterPredDesc d{};
    d.src_off[0]    = (uint64_t)T * sw + L;
    d.src_stride[0] = (uint32_t)sw;
    d.dst_stride    = (uint32_t)w;
    d.w             = (uint8_t)w;
    d.h             = (uint8_t)h;
    d.compound      = (uint8_t)(average && cp->use_jnt_comp_avg ? 2 : 0); // (mode 2 averages whatever this says; mode 1 never averages)
    d.fwd_offset    = (uint8_t)(average ? cp->fwd_offset : 0);
    d.bck_offset    = (uint8_t)(average ? cp->bck_offset : 0);
    c.up(dv, &d, sizeof(d));
    SvtHipInterPredPlanes planes{};
    planes.base[0] = ds;
    aux.cb         = db;
    aux.cb_stride  = (uint32_t)w;
    launch<true>(planes, dd, dv, 1, nullptr, aux, c.stream);
    if (jnt && !average) c.down2d(cp->dst, (size_t)cp->dst_stride * 2, db, (size_t)w * 2, (size_t)w * 2, h);
    else c.down2d(dst, (size_t)dst_stride * px, dd, (size_t)w * px, (size_t)w * px, h);
}

} // namespace

extern "C" {

int svt_hip_inter_pred_batch(SvtHipInterPredPlanes planes, void* dst_base, const SvtHipInterPredDesc* descs, uint32_t n, int bit_depth, uint8_t* status, void* stream) {
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
        hipLaunchKernelGGL(inter_pred_check_kernel, dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, planes, descs, n, bad);
        SVT_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        if (*(volatile uint32_t*)bad) return -1;
    }
    launch<false>(planes, dst_base, descs, n, status, batch_aux(bit_depth), st);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_inter_pred_masked_batch(SvtHipInterPredPlanes planes, void* dst_base, const uint8_t* mask_base, uint8_t* seg_mask_base,
                                    const SvtHipInterPredMaskedDesc* descs, uint32_t n, int bit_depth, uint8_t* status, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!dst_base || !descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    hipStream_t st  = (hipStream_t)stream;
    Aux         aux = batch_aux(bit_depth);
    aux.wedge       = svthip::wedge_table(st);
    aux.mask_base   = mask_base;
    aux.seg_base    = seg_mask_base;
    if (!status) {
        svthip::HostCall& c = svthip::host_call();
        c.begin_small();
        c.reserve(0, 256);
        uint32_t* bad = (uint32_t*)c.palloc(64);
        *bad          = 0;
        hipLaunchKernelGGL(inter_pred_masked_check_kernel, dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, planes, mask_base, descs, n, bad);
        SVT_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        if (*(volatile uint32_t*)bad) return -1;
    }
    const dim3 grid((n + DPW - 1) / DPW, SPLIT), block(TPB);
    if (bit_depth > 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_pred_kernel<uint16_t, false, true>), grid, block, 0, st, planes, (uint16_t*)dst_base, descs, n, status, aux);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_pred_kernel<uint8_t, false, true>), grid, block, 0, st, planes, (uint8_t*)dst_base, descs, n, status, aux);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

#define SVT_HIP_CONVOLVE_FORMS(name, cs, jnt)                                                                                                                            \
    void svt_av1_##name##_hip(const uint8_t* src, int32_t src_stride, uint8_t* dst, int32_t dst_stride, int32_t w, int32_t h, SvtHipInterpFilterParams* filter_params_x,  \
                              SvtHipInterpFilterParams* filter_params_y, const int32_t subpel_x_q4, const int32_t subpel_y_q4, SvtHipConvolveParams* conv_params) {        \
        if (svthip::failed()) return;                                                                                                                                    \
        try {                                                                                                                                                            \
            convolve_host<uint8_t>(src, src_stride, dst, dst_stride, w, h, filter_params_x, filter_params_y, subpel_x_q4, subpel_y_q4, conv_params, 8, cs, jnt);          \
        } catch (const svthip::DeviceError&) {}                                                                                                                          \
    }                                                                                                                                                                    \
    void svt_av1_highbd_##name##_hip(const uint16_t* src, int32_t src_stride, uint16_t* dst, int32_t dst_stride, int32_t w, int32_t h,                                     \
                                     const SvtHipInterpFilterParams* filter_params_x, const SvtHipInterpFilterParams* filter_params_y, const int32_t subpel_x_q4,        \
                                     const int32_t subpel_y_q4, SvtHipConvolveParams* conv_params, int32_t bd) {                                                           \
        if (svthip::failed()) return;                                                                                                                                    \
        try {                                                                                                                                                            \
            convolve_host<uint16_t>(src, src_stride, dst, dst_stride, w, h, filter_params_x, filter_params_y, subpel_x_q4, subpel_y_q4, conv_params, bd, cs, jnt);        \
        } catch (const svthip::DeviceError&) {}                                                                                                                          \
    }
SVT_HIP_CONVOLVE_FORMS(convolve_2d_copy_sr, 0, false)
SVT_HIP_CONVOLVE_FORMS(convolve_x_sr, 1, false)
SVT_HIP_CONVOLVE_FORMS(convolve_y_sr, 2, false)
SVT_HIP_CONVOLVE_FORMS(convolve_2d_sr, 3, false)
SVT_HIP_CONVOLVE_FORMS(jnt_convolve_2d_copy, 0, true)
SVT_HIP_CONVOLVE_FORMS(jnt_convolve_x, 1, true)
SVT_HIP_CONVOLVE_FORMS(jnt_convolve_y, 2, true)
SVT_HIP_CONVOLVE_FORMS(jnt_convolve_2d, 3, true)
#undef SVT_HIP_CONVOLVE_FORMS

} // extern "C"
