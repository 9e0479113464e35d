// picstats.hip -- the statistics third of the picture-analysis stage and the psy fork's variance boost, for gfx950:
//  * svt_hip_picture_variance_batch: compute_block_mean_compute_variance + compute_picture_spatial_statistics (pic_analysis_process.c:306-1380, :1531-1552).
//    A wave owns one 64x64 superblock and a lane one 8x8 block of it (lane = 8 * block row + block column, the reference's raster order): eight -- or, at
//    BLOCK_MEAN_PREC_SUB, four -- 8-byte loads, sum and sum of squares with v_dot4_u32_u8, the reference's fixed-point mean and mean of squares.  The 16x16, 32x32 and
//    64x64 levels are `(a + b + c + d) >> 2` of the level below, taken with two xor-shuffles per level (the four members of a group differ in one column bit and one
//    row bit of the lane number); they are NOT recomputed from pixels, the truncations are part of the result.  Plain stores only; pic_avg_variance is a second
//    launch (one workgroup per picture) that sums the 64x64 entries -- no global atomics, so nothing to zero and nothing that depends on launch order.
//    READABLE EXTENT: every superblock is read as a full 64x64 from the padded plane, as the reference reads it: each picture must be readable over rows
//    org_y .. org_y + 64 * ceil(height / 64) - 1 and columns org_x .. org_x + 64 * ceil(width / 64) - 1 (the encoder's padded source picture always is).
//  * svt_hip_variance_boost_qindex: svt_variance_adjust_qp + av1_get_deltaq_sb_variance_boost (rc_process.c:1403-1617).  A wave per superblock ranks its 64 8x8
//    variances by counting against an LDS copy (only the VALUES at three sorted positions matter), blends them 1:2:1, looks the boost up and clips; a second launch
//    of one workgroup takes the frame minimum / maximum and renormalises every superblock.  The boost curve is double-precision pow / log2 followed by a truncating
//    division: one ulp can move a boost, so the DEVICE never evaluates it -- the host does, with the C library the reference uses, into a table indexed by the blended
//    variance that travels as a kernel argument (no device allocation, nothing to keep alive across launches).  Tables are cached per (base_q_idx, strength, curve,
//    bit depth, q table).
//  * svt_hip_picture_histogram: sub_sample_luma_generate_pixel_intensity_histogram_bins + calculate_histogram (:1461-1524, :166-184): a workgroup per region, LDS
//    bins, one pass over the plane; avg_luma is a second launch of one workgroup that recovers every region's sum from its bins.
//  * the four dispatch pointers of aom_dsp_rtcd.c:516-519 as single-call forms (exported, not installed).
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include <math.h>
#include <map>
#include <mutex>
#include <vector>

namespace {

constexpr int      TPB  = 256;      // threads per workgroup
constexpr int      WPB  = TPB / 64; // waves (= superblocks) per workgroup
constexpr uint32_t ONES = 0x01010101u;
constexpr int      VAR_8x8_0 = 21; // ME_TIER_ZERO_PU_8x8_0 (me_context.h:75); 64x64 = 0, 32x32_0 = 1, 16x16_0 = 5
constexpr int      BOOST_LEN = 1024; // blended variances >= this have qstep_ratio clipped to 1 on every curve (log2 >= 10): boost 0
constexpr int      MAX_DELTAQ_RANGE = 80; // VAR_BOOST_MAX_DELTAQ_RANGE (rc_process.c:1394)

__device__ __forceinline__ uint64_t xor_add_u64(const uint64_t v, const int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return v + (((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = xor_add_u64(v, m);
    return v;
}
// (a + b + c + d) >> 2 over the 2x2 group whose lanes differ in bit mx (column) and bit my (row); every member gets the value
__device__ __forceinline__ uint64_t quad_mean(uint64_t v, const int mx, const int my) {
    v = xor_add_u64(v, mx);
    v = xor_add_u64(v, my);
    return v >> 2;
}
__device__ __forceinline__ uint16_t variance16(const uint64_t mean, const uint64_t mean_sq) { return (uint16_t)((mean_sq - mean * mean) >> 16); }

// ---- block means and variances ------------------------------------------------------------------------------------------------
template <int PREC>
__global__ __launch_bounds__(TPB) void picture_variance_kernel(const uint8_t* __restrict__ base, const uint64_t pic_pitch, const uint32_t stride, const uint32_t org_x,
                                                               const uint32_t org_y, const uint32_t sbs_x, const uint32_t n_sb, const uint32_t total,
                                                               const int write_sub64, uint16_t* __restrict__ variance) {
    const uint32_t item = blockIdx.x * WPB + threadIdx.x / 64;
    if (item >= total) return; // (whole waves)
    const int      lane = threadIdx.x & 63, bx = lane & 7, by = lane >> 3;
    const uint32_t pic = item / n_sb, sb = item - pic * n_sb, sby = sb / sbs_x, sbx = sb - sby * sbs_x;
    const uint8_t* p = base + (size_t)pic * pic_pitch + (size_t)(org_y + 64 * sby + 8 * by) * stride + org_x + 64 * sbx + 8 * bx;
    uint32_t       sum = 0, sq = 0;
#pragma unroll
    for (int r = 0; r < 8; r += (PREC == SVT_HIP_BLOCK_MEAN_PREC_SUB ? 2 : 1)) {
        const svt_u32x2_a1 v = svt_hip_global_load_x2(p + (size_t)r * stride);
        sum = __builtin_amdgcn_udot4(v[0], ONES, sum, false);
        sum = __builtin_amdgcn_udot4(v[1], ONES, sum, false);
        sq  = __builtin_amdgcn_udot4(v[0], v[0], sq, false);
        sq  = __builtin_amdgcn_udot4(v[1], v[1], sq, false);
    }
    // svt_compute_sub_mean_8x8_c / svt_aom_compute_sub_mean_squared_values_c (:233-271); svt_compute_mean_c / svt_compute_mean_squared_values_c (:190-231) on 8x8
    const uint64_t m8 = PREC == SVT_HIP_BLOCK_MEAN_PREC_SUB ? (uint64_t)sum << 3 : ((uint64_t)sum << 8) / 64;
    const uint64_t q8 = PREC == SVT_HIP_BLOCK_MEAN_PREC_SUB ? (uint64_t)sq << 11 : ((uint64_t)sq << 16) / 64;
    const uint64_t m16 = quad_mean(m8, 1, 8), q16 = quad_mean(q8, 1, 8);
    const uint64_t m32 = quad_mean(m16, 2, 16), q32 = quad_mean(q16, 2, 16);
    const uint64_t m64 = quad_mean(m32, 4, 32), q64 = quad_mean(q32, 4, 32);
    uint16_t*      out = variance + (size_t)item * 85;
    if (write_sub64) {
        out[VAR_8x8_0 + lane] = variance16(m8, q8);
        if (!(lane & 0x09)) out[5 + (by >> 1) * 4 + (bx >> 1)] = variance16(m16, q16);
        if (!(lane & 0x1b)) out[1 + (by >> 2) * 2 + (bx >> 2)] = variance16(m32, q32);
    }
    if (lane == 0) out[0] = variance16(m64, q64);
}

// pcs->pic_avg_variance = (uint16_t)(sum of the 64x64 variances / b64_total_count) (:1546-1549): one workgroup per picture
__global__ __launch_bounds__(TPB) void picture_avg_variance_kernel(const uint16_t* __restrict__ variance, const uint32_t n_sb, uint16_t* __restrict__ pic_avg_variance) {
    __shared__ unsigned long long part[WPB];
    const uint16_t* v = variance + (size_t)blockIdx.x * n_sb * 85;
    uint64_t        s = 0;
    for (uint32_t i = threadIdx.x; i < n_sb; i += TPB) s += v[(size_t)i * 85];
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x / 64] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < WPB; w++) t += part[w];
        pic_avg_variance[blockIdx.x] = (uint16_t)(t / n_sb);
    }
}

// ---- variance boost -------------------------------------------------------------------------------------------------------------------
struct BoostTable { int16_t boost[BOOST_LEN]; }; // by blended variance (entry 0 unused: variance 0 is mapped to 1 first); a kernel argument

__device__ __forceinline__ int clip3(const int lo, const int hi, const int v) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(TPB) void variance_boost_kernel(const uint16_t* __restrict__ variance, const uint8_t* __restrict__ qindex_in, const uint32_t n_sb,
                                                             const int low_idx, const int mid_idx, const int upp_idx, const BoostTable T,
                                                             uint8_t* __restrict__ qindex_out) {
    __shared__ __attribute__((aligned(16))) uint16_t vals[WPB][64];
    const int      wave = threadIdx.x / 64, lane = threadIdx.x & 63;
    const uint32_t sb_raw = blockIdx.x * WPB + wave, sb = sb_raw < n_sb ? sb_raw : n_sb - 1; // (a wave past the end repeats the last superblock and stores nothing)
    const int      v = variance[(size_t)sb * 85 + VAR_8x8_0 + lane];
    vals[wave][lane] = (uint16_t)v;
    __syncthreads();
    // rank by counting: the sorted array holds v at positions lt .. le - 1 (qsort's order among equal values does not matter: only values are read)
    int lt = 0, le = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const int o = vals[wave][j];
        lt += o < v;
        le += o <= v;
    }
    int s[3];
    const int pos[3] = {low_idx, mid_idx, upp_idx};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long m = __ballot(lt <= pos[k] && pos[k] < le); // never empty
        s[k] = __shfl(v, __ffsll(m) - 1);
    }
    uint32_t blend = (uint32_t)(uint16_t)((s[0] + s[1] * 2 + s[2] + 2) / 4);
    if (blend == 0) blend = 1;
    const int boost = blend < (uint32_t)BOOST_LEN ? (int)T.boost[blend] : 0;
    if (lane == 0 && sb_raw < n_sb) qindex_out[sb] = (uint8_t)clip3(1, 255, (int)qindex_in[sb] - boost);
}

// the frame pass of svt_variance_adjust_qp (:1568-1616) on the clipped values the kernel above left in qindex: ONE workgroup
__global__ __launch_bounds__(1024) void variance_boost_frame_kernel(uint8_t* __restrict__ qindex, const uint32_t n_sb, SvtHipVarBoostFrame* __restrict__ frame) {
    __shared__ int smin[16], smax[16];
    const int tid = threadIdx.x;
    int mn = 255, mx = 0; // MAX_Q_INDEX, MIN_Q_INDEX
    for (uint32_t i = tid; i < n_sb; i += 1024) {
        const int q = qindex[i];
        mn = q < mn ? q : mn;
        mx = q > mx ? q : mx;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int a = __shfl_xor(mn, m), b = __shfl_xor(mx, m);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) { smin[tid >> 6] = mn; smax[tid >> 6] = mx; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; w++) {
        mn = smin[w] < mn ? smin[w] : mn;
        mx = smax[w] > mx ? smax[w] : mx;
    }
    int range = mx - mn;
    range     = range < MAX_DELTAQ_RANGE ? range : MAX_DELTAQ_RANGE;
    const int base = mn + (range >> 1);
    for (uint32_t i = tid; i < n_sb; i += 1024) {
        const int off = clip3(-(MAX_DELTAQ_RANGE >> 1), MAX_DELTAQ_RANGE >> 1, (int)qindex[i] - base);
        qindex[i]     = (uint8_t)clip3(1, 255, base + off);
    }
    if (tid == 0) {
        frame->normalized_base_q_idx = base;
        frame->min_qindex            = mn;
        frame->max_qindex            = mx;
        frame->reserved              = 0;
    }
}

// ---- histograms ---------------------------------------------------------------------------------------------------------------------
// One workgroup per region; regions are indexed [width index][height index] as pcs->picture_histogram is.  The last region of a direction takes the remainder.
__global__ __launch_bounds__(TPB) void picture_histogram_kernel(const uint8_t* __restrict__ origin, const uint32_t stride, const uint32_t width, const uint32_t height,
                                                                const uint32_t regions_w, const uint32_t regions_h, const uint32_t step,
                                                                uint32_t* __restrict__ histogram, uint8_t* __restrict__ avg_intensity) {
    __shared__ uint32_t           bins[256];
    __shared__ unsigned long long total;
    const int      tid = threadIdx.x;
    const uint32_t wi = blockIdx.x / regions_h, hi = blockIdx.x - wi * regions_h;
    const uint32_t rw = width / regions_w, rh = height / regions_h;
    const uint32_t w = rw + (wi == regions_w - 1 ? width - regions_w * rw : 0), h = rh + (hi == regions_h - 1 ? height - regions_h * rh : 0);
    const uint8_t* p = origin + (size_t)(hi * rh) * stride + wi * rw;
    const uint32_t nx = (w + step - 1) / step, ny = (h + step - 1) / step;
    bins[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    uint64_t s = 0;
    for (uint32_t i = tid; i < nx * ny; i += TPB) {
        const uint32_t y = i / nx, x = i - y * nx;
        const uint32_t v = p[(size_t)(y * step) * stride + x * step];
        atomicAdd(&bins[v], 1u);
        s += v;
    }
    s = wave_sum_u64(s);
    if ((tid & 63) == 0) atomicAdd(&total, (unsigned long long)s);
    __syncthreads();
    histogram[(size_t)blockIdx.x * 256 + tid] = (1u + bins[tid]) * 4u * 4u * step * step; // bins start at 1 (:1480), uint32 arithmetic (:1513-1516)
    if (tid == 0) {
        const uint64_t sum  = (uint64_t)total * step * step;
        const uint32_t area = w * h;
        avg_intensity[blockIdx.x] = (uint8_t)((sum + (area >> 1)) / area);
    }
}
// avg_luma = (sum over regions of sum * step^2) / (width * height) (:1510, :1521).  A region's sum is sum over bins of bin * count, and count is what the
// histogram launch just wrote, (1 + count) * 16 * step^2, taken apart again (exact while that product fits 32 bits -- the reference's bins wrap there as well).
__global__ __launch_bounds__(TPB) void picture_avg_luma_kernel(const uint32_t* __restrict__ histogram, const uint32_t n_regions, const uint32_t step, const uint32_t area,
                                                               uint64_t* __restrict__ avg_luma) {
    __shared__ unsigned long long part[WPB];
    const int tid = threadIdx.x;
    uint64_t  s   = 0;
    for (uint32_t r = 0; r < n_regions; r++) s += (uint64_t)(histogram[(size_t)r * 256 + tid] / (16u * step * step) - 1u) * (uint32_t)tid;
    s = wave_sum_u64(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < WPB; w++) t += part[w];
        *avg_luma = t * step * step / area;
    }
}

// ---- the per-call forms' kernel: sum and sum of squares of n blocks of w x h lying side by side, every row_step-th row; one wave per block ------------------
__global__ __launch_bounds__(TPB) void block_sums_kernel(const uint8_t* __restrict__ p, const uint32_t stride, const uint32_t w, const uint32_t h, const uint32_t row_step,
                                                         const uint32_t n, uint64_t* __restrict__ out) {
    const uint32_t b = threadIdx.x / 64;
    if (b >= n) return; // (whole waves)
    const int      lane = threadIdx.x & 63;
    const uint32_t rows = (h + row_step - 1) / row_step;
    uint64_t       sum = 0, sq = 0;
    for (uint32_t i = lane; i < w * rows; i += 64) {
        const uint32_t y = i / w, x = i - y * w;
        const uint32_t v = p[(size_t)(y * row_step) * stride + b * w + x];
        sum += v;
        sq += v * v;
    }
    sum = wave_sum_u64(sum);
    sq  = wave_sum_u64(sq);
    if (lane == 0) { out[2 * b] = sum; out[2 * b + 1] = sq; }
}

// n (<= 4) blocks from host memory: the rows the reference reads go into the call's arena, the 2 n sums come back with one synchronisation
void host_block_sums(const uint8_t* in, uint32_t stride, uint32_t w, uint32_t h, uint32_t row_step, uint32_t n, uint64_t* sums) {
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const uint32_t rows  = (h - 1) / row_step * row_step + 1; // the last row read
    const size_t   pitch = svthip::align_up((size_t)w * n, 16), bytes = pitch * rows + 4096;
    c.reserve(bytes, bytes);
    uint8_t*  di = (uint8_t*)c.dalloc(pitch * rows);
    uint64_t* o  = (uint64_t*)c.dalloc(16 * n);
    c.up2d(di, pitch, in, stride, (size_t)w * n, rows);
    hipLaunchKernelGGL(block_sums_kernel, dim3(1), dim3(TPB), 0, c.stream, (const uint8_t*)di, (uint32_t)pitch, w, h, row_step, n, o);
    SVT_LAUNCH_CHECK();
    c.down(sums, o, 16 * n);
}

// ---- the boost curve, on the host (av1_get_deltaq_sb_variance_boost, rc_process.c:1462-1493) -----------------------------------------------
// svt_av1_compute_qdelta_fp (:190-210) against the caller's qindex -> q_fp8 table
int qdelta_fp(const int32_t* q, const int32_t qstart_fp8, const int32_t qtarget_fp8) {
    int start_index = 255, target_index = 255;
    for (int i = 0; i < 255; ++i) {
        start_index = i;
        if (q[i] >= qstart_fp8) break;
    }
    for (int i = 0; i < 255; ++i) {
        target_index = i;
        if (q[i] >= qtarget_fp8) break;
    }
    return target_index - start_index;
}
int boost_of_variance(const uint16_t variance, const uint8_t base_q_idx, const uint8_t strength, const uint8_t curve, const int32_t* q) {
    double       qstep_ratio = 0;
    const double strengths[] = {0, 0.65, 1.1, 1.6, 2.5};
    switch (curve) { // the reference's expressions, operand for operand: the evaluation order is part of the result
    case 1: qstep_ratio = 0.25 * strength * (-log2((double)variance) + 8) + 1; break;
    case 2: qstep_ratio = 0.15 * strength * (-log2((double)variance) + 10) + 1; break;
    default: qstep_ratio = pow(1.018, strengths[strength] * (-10 * log2((double)variance) + 80)); break;
    }
    qstep_ratio = qstep_ratio < 1 ? 1 : (qstep_ratio > 8 ? 8 : qstep_ratio); // CLIP3(1, VAR_BOOST_MAX_QSTEP_RATIO_BOOST, .)
    const int32_t base_q = q[base_q_idx], target_q = (int32_t)(base_q / qstep_ratio);
    int32_t       boost;
    if (curve == 2) boost = (int32_t)((base_q_idx + 496) * -qdelta_fp(q, base_q, target_q) / (255 + 1024));
    else boost = (int32_t)((base_q_idx + 40) * -qdelta_fp(q, base_q, target_q) / (255 + 40));
    return boost < MAX_DELTAQ_RANGE ? boost : MAX_DELTAQ_RANGE;
}

struct BoostKey {
    uint8_t base_q_idx, strength, curve, bit_depth;
    std::vector<int32_t> q;
    bool operator<(const BoostKey& o) const {
        if (base_q_idx != o.base_q_idx) return base_q_idx < o.base_q_idx;
        if (strength != o.strength) return strength < o.strength;
        if (curve != o.curve) return curve < o.curve;
        if (bit_depth != o.bit_depth) return bit_depth < o.bit_depth;
        return q < o.q;
    }
};
std::mutex                       boost_lock;
std::map<BoostKey, BoostTable*>  boost_cache; // entries live until the process ends (at most 255 x 4 x 3 per q table, 2 KiB each)

bool boost_args_ok(uint8_t strength, uint8_t octile, uint8_t curve, const int32_t* q) { return strength >= 1 && strength <= 4 && octile >= 1 && octile <= 8 && curve <= 2 && q; }

const BoostTable* boost_table(uint8_t base_q_idx, uint8_t strength, uint8_t curve, int bit_depth, const int32_t* q) {
    BoostKey k{base_q_idx, strength, curve, (uint8_t)bit_depth, std::vector<int32_t>(q, q + 256)};
    std::lock_guard<std::mutex> g(boost_lock);
    auto it = boost_cache.find(k);
    if (it != boost_cache.end()) return it->second;
    BoostTable* t = new BoostTable;
    t->boost[0]   = 0;
    for (int v = 1; v < BOOST_LEN; v++) t->boost[v] = (int16_t)boost_of_variance((uint16_t)v, base_q_idx, strength, curve, q);
    boost_cache.emplace(std::move(k), t);
    return t;
}

} // namespace

extern "C" {

void svt_hip_picture_variance_batch(const uint8_t* luma_base, uint64_t pic_pitch, uint32_t stride, uint32_t org_x, uint32_t org_y, uint32_t width, uint32_t height,
                                    uint32_t n_pics, int prec, int write_sub64, uint16_t* variance, uint16_t* pic_avg_variance, void* stream) {
    svthip::ensure_device();
    const uint32_t sbs_x = (width + 63) / 64, sbs_y = (height + 63) / 64, n_sb = sbs_x * sbs_y;
    if (n_pics == 0 || n_sb == 0) return;
    const uint64_t total64 = (uint64_t)n_pics * n_sb;
    if (total64 > 0x7fffffffull) return; // (item numbers are 32-bit)
    const uint32_t total = (uint32_t)total64;
    const dim3     grid((total + WPB - 1) / WPB), block(TPB);
    if (prec == SVT_HIP_BLOCK_MEAN_PREC_SUB)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(picture_variance_kernel<SVT_HIP_BLOCK_MEAN_PREC_SUB>), grid, block, 0, (hipStream_t)stream, luma_base, pic_pitch, stride, org_x,
                           org_y, sbs_x, n_sb, total, write_sub64, variance);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(picture_variance_kernel<SVT_HIP_BLOCK_MEAN_PREC_FULL>), grid, block, 0, (hipStream_t)stream, luma_base, pic_pitch, stride, org_x,
                           org_y, sbs_x, n_sb, total, write_sub64, variance);
    SVT_LAUNCH_CHECK();
    if (pic_avg_variance) {
        hipLaunchKernelGGL(picture_avg_variance_kernel, dim3(n_pics), dim3(TPB), 0, (hipStream_t)stream, (const uint16_t*)variance, n_sb, pic_avg_variance);
        SVT_LAUNCH_CHECK();
    }
}

int svt_hip_variance_boost_table(uint8_t base_q_idx, uint8_t strength, uint8_t curve, int bit_depth, const int32_t* q_fp8_table, int16_t* boost_out) {
    if (!boost_args_ok(strength, 1, curve, q_fp8_table) || !boost_out) return -1;
    const BoostTable* t = boost_table(base_q_idx, strength, curve, bit_depth, q_fp8_table);
    for (int v = 0; v < 65536; v++) {
        const int b  = v ? v : 1; // "variance == 0 -> 1" (rc_process.c:1459)
        boost_out[v] = b < BOOST_LEN ? t->boost[b] : 0;
    }
    return 0;
}

int svt_hip_variance_boost_qindex(const uint16_t* variance, const uint8_t* qindex_in, uint32_t n_sb, uint8_t base_q_idx, uint8_t strength, uint8_t octile, uint8_t curve,
                                  int bit_depth, const int32_t* q_fp8_table, uint8_t* qindex_out, SvtHipVarBoostFrame* frame_out, void* stream) {
    if (!boost_args_ok(strength, octile, curve, q_fp8_table)) return -1;
    svthip::ensure_device();
    if (n_sb == 0) return 0;
    const BoostTable* t = boost_table(base_q_idx, strength, curve, bit_depth, q_fp8_table);
    // SUBBLOCKS_IN_OCTILE = 8: the last subblock of the octile, of the one before and of the one after (rc_process.c:1422-1424)
    const int mid = octile * 8 - 1, low = mid - 8 > 7 ? mid - 8 : 7, upp = mid + 8 < 63 ? mid + 8 : 63;
    hipLaunchKernelGGL(variance_boost_kernel, dim3((n_sb + WPB - 1) / WPB), dim3(TPB), 0, (hipStream_t)stream, variance, qindex_in, n_sb, low, mid, upp, *t, qindex_out);
    SVT_LAUNCH_CHECK();
    hipLaunchKernelGGL(variance_boost_frame_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, qindex_out, n_sb, frame_out);
    SVT_LAUNCH_CHECK();
    return 0;
}

void svt_hip_picture_histogram(const uint8_t* origin, uint32_t stride, uint32_t width, uint32_t height, uint32_t regions_w, uint32_t regions_h, uint32_t decim_step,
                               uint32_t* histogram, uint8_t* average_intensity_per_region, uint64_t* avg_luma, void* stream) {
    svthip::ensure_device();
    if (regions_w == 0 || regions_h == 0 || width < regions_w || height < regions_h || decim_step == 0) return; // (an empty region: the reference divides by zero)
    const uint32_t n = regions_w * regions_h;
    hipLaunchKernelGGL(picture_histogram_kernel, dim3(n), dim3(TPB), 0, (hipStream_t)stream, origin, stride, width, height, regions_w, regions_h, decim_step, histogram,
                       average_intensity_per_region);
    SVT_LAUNCH_CHECK();
    if (avg_luma) {
        hipLaunchKernelGGL(picture_avg_luma_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const uint32_t*)histogram, n, decim_step, width * height, avg_luma);
        SVT_LAUNCH_CHECK();
    }
}

// ---- RTCD-signature single-call forms (aom_dsp_rtcd.h:858-862; the fixed-point step after the sums is the reference's, on the host) ------------------------
uint64_t svt_compute_mean_8x8_hip(uint8_t* input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height) {
    uint64_t s[2] = {0, 0};
    if (input_area_width == 0 || input_area_height == 0) return 0;
    host_block_sums(input_samples, input_stride, input_area_width, input_area_height, 1, 1, s);
    return (s[0] << 8) / (input_area_width * input_area_height);
}
uint64_t svt_compute_mean_square_values_8x8_hip(uint8_t* input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height) {
    uint64_t s[2] = {0, 0};
    if (input_area_width == 0 || input_area_height == 0) return 0;
    host_block_sums(input_samples, input_stride, input_area_width, input_area_height, 1, 1, s);
    return (s[1] << 16) / (input_area_width * input_area_height);
}
uint64_t svt_compute_sub_mean_8x8_hip(uint8_t* input_samples, uint16_t input_stride) {
    uint64_t s[2] = {0, 0};
    host_block_sums(input_samples, input_stride, 8, 8, 2, 1, s);
    return s[0] << 3;
}
void svt_compute_interm_var_four8x8_hip(uint8_t* input_samples, uint16_t input_stride, uint64_t* mean_of8x8_blocks, uint64_t* mean_of_squared8x8_blocks) {
    uint64_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    host_block_sums(input_samples, input_stride, 8, 8, 2, 4, s);
    for (int i = 0; i < 4; i++) {
        mean_of8x8_blocks[i]         = s[2 * i] << 3;
        mean_of_squared8x8_blocks[i] = s[2 * i + 1] << 11;
    }
}

} // extern "C"

SVT_HIP_DEFINE_WARM(picstats) // (svt_hip_warmup loads this translation unit's code object at encoder initialisation: svt_hip_common.h)
