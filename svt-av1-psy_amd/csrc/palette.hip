// palette.hip -- the AV1 luma palette tools of mode decision as batched launches (include/svtav1_hip.h, "AV1 luma palette"):
//   A. svt_hip_kmeans_batch               svt_av1_k_means_dim{1,2}_c / svt_av1_calc_indices_dim{1,2}_c (k_means_template.h)
//   B. svt_hip_count_colors_batch         svt_av1_count_colors / svt_av1_count_colors_highbd (pic_analysis_process.c:1808-1845)
//   C. svt_hip_palette_search_luma_batch  search_palette_luma with palette_rd_y (palette.c:272-428)
//   D. svt_hip_palette_cost_batch         svt_av1_cost_color_map, svt_av1_palette_color_cost_y, svt_aom_write_uniform_cost
//   E. svt_hip_palette_pred_batch         the palette branch of the intra predictor (enc_intra_prediction.c:501-508, :647-655)
//   F. svt_hip_palette_cache_y and the six single-call forms.
// All integer, bit-exact with the C.  A, C and D give one item to one wave (a workgroup of 64 lanes): every decision of an item -- iteration exit, reseed, candidate
// kept -- is then taken on values all lanes hold alike, and the lanes exchange through LDS between two barriers of a one-wave workgroup.
//
// The k-means of one wave (kmeans_run) works on WEIGHTED points: A has one point per sample (weight 1); C has one point per DISTINCT colour of the block with its
// count as weight -- at most 64, one per lane -- because every sum of the C over samples (count, centroid sum, total distance) is the same sum over colours times
// their counts, exactly, in integers.  Only the reseed (data[lcg_rand16 % n]) needs the samples themselves, and C keeps them in LDS.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"

namespace {

constexpr int WAVE = 64, TPB = 256;
constexpr int KMAX = 8;                    // PALETTE_MAX_SIZE
constexpr int ROW  = KMAX + 2 * KMAX + 1;  // one lane's partial sums: 8 counts, 8 x dim coordinate sums; odd, so that the lanes' rows start in different LDS banks
constexpr int MAX_POINTS = 16384;          // MAX_SB_SQUARE: the C's pre_indices

struct KmShared {
    int part[WAVE * ROW];
    int cent[2 * KMAX];
};

__device__ __forceinline__ int lane_of() { return (int)threadIdx.x; }
__device__ __forceinline__ int uni(const int v) { return __builtin_amdgcn_readfirstlane(v); } // a value all lanes hold alike, as a scalar the compiler can branch on
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int m = WAVE / 2; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int sqr(const int v) { return v * v; }
__device__ __forceinline__ int floor_log2(const uint32_t v) { return 31 - __clz(v); } // v != 0
__device__ __forceinline__ int ceil_log2(const int n) { return n < 2 ? 0 : floor_log2((uint32_t)(n - 1)) + 1; } // av1_ceil_log2

// svt_av1_calc_indices of one point: the nearest of c[0 .. k - 1], the first on ties (the C compares with `<`)
template <int DIM> __device__ __forceinline__ int nearest(const int (&v)[DIM], const int (&c)[KMAX * DIM], const int k, int& dist) {
    int best = 0, bd = 0;
#pragma unroll
    for (int t = 0; t < DIM; t++) bd += sqr(v[t] - c[t]);
#pragma unroll
    for (int j = 1; j < KMAX; j++) {
        if (j < k) {
            int d = 0;
#pragma unroll
            for (int t = 0; t < DIM; t++) d += sqr(v[t] - c[j * DIM + t]);
            if (d < bd) bd = d, best = j;
        }
    }
    dist = bd;
    return best;
}

// the points of A: n samples of DIM coordinates in global memory
template <int DIM> struct SamplePoints {
    const int32_t* d;
    int            n;
    __device__ int      points() const { return n; }
    __device__ int      samples() const { return n; }
    __device__ int      weight(int) const { return 1; }
    __device__ uint32_t seed() const { return (uint32_t)d[0]; }
    __device__ void     get(const int i, int (&v)[DIM]) const {
#pragma unroll
        for (int t = 0; t < DIM; t++) v[t] = d[(size_t)i * DIM + t];
    }
    __device__ void sample(const int i, int (&v)[DIM]) const { get(i, v); }
};
// the points of C: the distinct colours of a block (ascending) with their counts, and the block's rows * cols samples, all in LDS
struct ColorPoints {
    const int*      val;
    const int*      cnt;
    const uint16_t* data;
    int             colors, n;
    __device__ int      points() const { return colors; }
    __device__ int      samples() const { return n; }
    __device__ int      weight(const int i) const { return cnt[i]; }
    __device__ uint32_t seed() const { return (uint32_t)data[0]; }
    __device__ void     get(const int i, int (&v)[1]) const { v[0] = val[i]; }
    __device__ void     sample(const int i, int (&v)[1]) const { v[0] = data[i]; }
};

// One sweep over the points with the centroids c: every point's nearest centroid, into the lane's own row the weights and weighted coordinates per centroid (what
// calc_centroids of the NEXT iteration sums), and the total distance of calc_total_dist.  Ends with a barrier: the rows are readable afterwards.
template <int DIM, class PTS> __device__ __forceinline__ long long km_sweep(const PTS& P, const int (&c)[KMAX * DIM], const int k, KmShared& S) {
    int* row = S.part + lane_of() * ROW;
    for (int q = 0; q < ROW; q++) row[q] = 0;
    long long dist = 0;
    for (int i = lane_of(); i < P.points(); i += WAVE) {
        int v[DIM], d;
        P.get(i, v);
        const int w = P.weight(i), idx = nearest<DIM>(v, c, k, d);
        row[idx] += w;
#pragma unroll
        for (int t = 0; t < DIM; t++) row[KMAX + idx * DIM + t] += w * v[t];
        dist += (long long)w * d;
    }
    dist = wave_sum_i64(dist);
    __syncthreads();
    return dist;
}

// calc_centroids: lane j < k owns cluster j.  An empty cluster takes data[lcg_rand16 % n]; the C draws for the empty clusters in ascending order from ONE stream
// seeded with data[0], so lane j steps the generator once more than there are empty clusters below it.
template <int DIM, class PTS> __device__ __forceinline__ void km_centroids(const PTS& P, const int k, KmShared& S, int (&c)[KMAX * DIM]) {
    const int j   = lane_of();
    int       cnt = 1, sum[DIM];
#pragma unroll
    for (int t = 0; t < DIM; t++) sum[t] = 0;
    if (j < k) {
        cnt = 0;
        for (int l = 0; l < WAVE; l++) {
            cnt += S.part[l * ROW + j];
#pragma unroll
            for (int t = 0; t < DIM; t++) sum[t] += S.part[l * ROW + KMAX + j * DIM + t];
        }
    }
    const unsigned long long empty = __ballot(cnt == 0);
    if (j < k) {
        if (cnt == 0) {
            uint32_t  st    = P.seed();
            const int draws = __popcll(empty & ((1ull << j) - 1)) + 1;
            for (int q = 0; q < draws; q++) st = st * 1103515245u + 12345u;          // lcg_next
            P.sample((int)(((st / 65536u) % 32768u) % (uint32_t)P.samples()), sum); // lcg_rand16 % n
        } else {
#pragma unroll
            for (int t = 0; t < DIM; t++) sum[t] = (sum[t] + (cnt >> 1)) / cnt; // DIVIDE_AND_ROUND
        }
#pragma unroll
        for (int t = 0; t < DIM; t++) S.cent[j * DIM + t] = sum[t];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KMAX * DIM; q++)
        if (q < k * DIM) c[q] = S.cent[q];
}

// svt_av1_k_means_dimN_c: c holds the initial centroids and leaves with the final ones; the indices are calc_indices of those (at every exit of the C, too).
template <int DIM, class PTS> __device__ __forceinline__ void kmeans_run(const PTS& P, const int k, const int max_itr, KmShared& S, int (&c)[KMAX * DIM]) {
    long long this_dist = km_sweep<DIM>(P, c, k, S);
    for (int it = 0; it < max_itr; it++) {
        int pre[KMAX * DIM];
#pragma unroll
        for (int q = 0; q < KMAX * DIM; q++) pre[q] = c[q];
        const long long pre_dist = this_dist;
        km_centroids<DIM>(P, k, S, c);
        this_dist = km_sweep<DIM>(P, c, k, S);
        const bool worse = this_dist > pre_dist; // never true with integer centroids; kept, it costs one compare
        bool       same  = true;
#pragma unroll
        for (int q = 0; q < KMAX * DIM; q++) {
            if (q < k * DIM) same &= c[q] == pre[q];
            if (worse) c[q] = pre[q];
        }
        if (uni(worse || same)) break;
    }
}

// ---- descriptor checks ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool block_dim_ok(const int v) { return v == 8 || v == 16 || v == 32 || v == 64; }
__device__ __forceinline__ bool desc_ok(const SvtHipKmeansDesc& d) { return (d.dim == 1 || d.dim == 2) && d.k >= 1 && d.k <= KMAX && d.n >= 1 && d.n <= MAX_POINTS; }
__device__ __forceinline__ bool desc_ok(const SvtHipCountColorsDesc& d) { return d.rows >= 1 && d.cols >= 1; }
__device__ __forceinline__ bool desc_ok(const SvtHipPaletteSearchDesc& d) {
    return block_dim_ok(d.block_width) && block_dim_ok(d.block_height) && d.rows >= 1 && d.rows <= d.block_height && d.cols >= 1 && d.cols <= d.block_width &&
        d.n_cache <= 16 && d.dominant_color_step >= 1 && d.map_stride >= (uint32_t)d.block_width * d.block_height && (d.out_off & 1) == 0;
}
__device__ __forceinline__ bool desc_ok(const SvtHipPaletteCostDesc& d) {
    return d.size >= 2 && d.size <= KMAX && block_dim_ok(d.block_width) && d.rows >= 1 && d.rows <= 64 && d.cols >= 1 && d.cols <= d.block_width && d.n_cache <= 16 &&
        (d.bit_depth == 8 || d.bit_depth == 10 || d.bit_depth == 12) && (d.colors_off & 1) == 0;
}
__device__ __forceinline__ bool desc_ok(const SvtHipPalettePredDesc& d) {
    return (d.w == 4 || block_dim_ok(d.w)) && (d.h == 4 || block_dim_ok(d.h)) && block_dim_ok(d.wpx) && d.x + d.w <= d.wpx && d.y + d.h <= 64 && (d.colors_off & 1) == 0;
}
// descriptors the host cannot read: every thread looks at a few; whoever finds an invalid one stores 1 into the word the host zeroed (plain stores of one value)
template <class D> __global__ __launch_bounds__(TPB) void palette_check_kernel(const D* __restrict__ descs, const uint32_t n, uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !desc_ok(descs[i]);
    if (bad) *bad_out = 1;
}
template <class D> bool descs_all_valid(const D* descs, const uint32_t n, hipStream_t st) {
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    c.reserve(0, 256);
    uint32_t* bad = (uint32_t*)c.palloc(64);
    *bad          = 0;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(palette_check_kernel<D>), dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, descs, n, bad);
    SVT_LAUNCH_CHECK();
    HIP_CHECK(hipStreamSynchronize(st));
    return *(volatile uint32_t*)bad == 0;
}

// =====================================================================================================================================================
// A. k-means
// =====================================================================================================================================================
template <int DIM>
__device__ __forceinline__ void kmeans_item(const SvtHipKmeansDesc& d, const int32_t* data, int32_t* cent, uint8_t* ind, KmShared& S) {
    const SamplePoints<DIM> P{data, d.n};
    const int               k = uni(d.k), max_itr = uni(d.max_itr);
    int                     c[KMAX * DIM];
#pragma unroll
    for (int q = 0; q < KMAX * DIM; q++) c[q] = q < k * DIM ? cent[q] : 0;
    if (!d.assign_only) {
        kmeans_run<DIM>(P, k, max_itr, S, c);
#pragma unroll
        for (int q = 0; q < KMAX * DIM; q++)
            if (q < k * DIM && lane_of() == 0) cent[q] = c[q];
    }
    for (int i = lane_of(); i < d.n; i += WAVE) {
        int v[DIM], dist;
        P.get(i, v);
        ind[i] = (uint8_t)nearest<DIM>(v, c, k, dist);
    }
}
__global__ __launch_bounds__(WAVE) void kmeans_kernel(const int32_t* __restrict__ data_base, int32_t* __restrict__ cent_base, uint8_t* __restrict__ ind_base,
                                                      const SvtHipKmeansDesc* __restrict__ descs, const uint32_t n, uint8_t* __restrict__ status) {
    __shared__ KmShared S;
    const uint32_t      b = blockIdx.x;
    if (b >= n) return;
    const SvtHipKmeansDesc d = descs[b];
    if (!desc_ok(d)) {
        if (status && threadIdx.x == 0) status[b] = 1;
        return;
    }
    if (d.dim == 1) kmeans_item<1>(d, data_base + d.data_off, cent_base + d.centroids_off, ind_base + d.indices_off, S);
    else kmeans_item<2>(d, data_base + d.data_off, cent_base + d.centroids_off, ind_base + d.indices_off, S);
    if (status && threadIdx.x == 0) status[b] = 0;
}

// =====================================================================================================================================================
// B. colour count
// =====================================================================================================================================================
template <typename PIX>
__global__ __launch_bounds__(TPB) void count_colors_kernel(const PIX* __restrict__ src_base, const SvtHipCountColorsDesc* __restrict__ descs, const uint32_t n,
                                                           const int bins, int32_t* __restrict__ hist_base, int32_t* __restrict__ n_colors,
                                                           uint8_t* __restrict__ status) {
    __shared__ int s_hist[4096];
    __shared__ int s_colors, s_bad;
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    const SvtHipCountColorsDesc d = descs[b];
    if (!desc_ok(d)) {
        if (status && threadIdx.x == 0) status[b] = 1;
        return;
    }
    for (int v = threadIdx.x; v < bins; v += TPB) s_hist[v] = 0;
    if (threadIdx.x == 0) s_colors = 0, s_bad = 0;
    __syncthreads();
    const PIX*     src   = src_base + d.src_off;
    const uint32_t total = (uint32_t)d.rows * d.cols;
    for (uint32_t i = threadIdx.x; i < total; i += TPB) {
        const uint32_t r = i / d.cols, c = i - r * d.cols;
        const int      v = src[(size_t)r * d.src_stride + c];
        if (v < bins) atomicAdd(&s_hist[v], 1);
        else s_bad = 1;
    }
    __syncthreads();
    int32_t* hist = hist_base + d.hist_off;
    int      mine = 0;
    for (int v = threadIdx.x; v < bins; v += TPB) {
        hist[v] = s_hist[v];
        mine += s_hist[v] != 0;
    }
    if (mine) atomicAdd(&s_colors, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        n_colors[b] = s_bad ? 0 : s_colors;
        if (status) status[b] = s_bad ? 2 : 0;
    }
}

// =====================================================================================================================================================
// C. search_palette_luma
// =====================================================================================================================================================
struct SearchShared {
    uint16_t data[4096];  // the block's rows x cols samples, pitch cols: the C's kmeans_data_buf
    int      hist[1024];  // the histogram; once the colours are listed, the colour -> palette index table of the candidate in hand
    int      val[WAVE], cnt[WAVE]; // the distinct colours, ascending, and their counts
    int      top[KMAX];   // the dominant colours
    int      c[KMAX];     // the centroids of the candidate in hand
    int      cache[16];
    int      k;
    KmShared km;
};

// palette_rd_y on S.c[0 .. n - 1]; returns the new number of candidates.  Lane 0 does the eight-element work (snap to the cache, sort, duplicates), the colour ->
// index table is one colour per lane, the map one byte per lane and step.
__device__ __forceinline__ int palette_candidate(const SvtHipPaletteSearchDesc& d, const int n, const int colors, const int maxv, SearchShared& S,
                                                 SvtHipPaletteSearchOut* out, uint8_t* maps, const int tot) {
    const int lane = lane_of();
    if (lane == 0) {
        if (d.n_cache > 0) { // optimize_palette_colors: the first nearest cache colour, taken when within 1
            for (int i = 0; i < n; i++) {
                int diff = abs(S.c[i] - S.cache[0]), at = 0;
                for (int j = 1; j < d.n_cache; j++) {
                    const int t = abs(S.c[i] - S.cache[j]);
                    if (t < diff) diff = t, at = j;
                }
                if (diff <= 1) S.c[i] = S.cache[at];
            }
        }
        for (int i = 1; i < n; i++) { // ascending order
            const int v = S.c[i];
            int       j = i;
            for (; j > 0 && S.c[j - 1] > v; j--) S.c[j] = S.c[j - 1];
            S.c[j] = v;
        }
        int k = 1; // av1_remove_duplicates
        for (int i = 1; i < n; i++)
            if (S.c[i] != S.c[i - 1]) S.c[k++] = S.c[i];
        S.k = k;
    }
    __syncthreads();
    const int k = uni(S.k);
    if (k <= 2) return tot; // below PALETTE_MIN_SIZE the C skips; a palette of two is made and then not kept (palette.c:391, :422)
    if (lane < k) out->colors[tot][lane] = (uint16_t)min(max(S.c[lane], 0), maxv);
    if (lane == 0) out->size[tot] = (uint8_t)k;
    if (lane < colors) { // av1_calc_indices with the centroids as they are (before the clip), per distinct colour
        const int v    = S.val[lane];
        int       best = 0, bd = sqr(v - S.c[0]);
        for (int j = 1; j < k; j++) {
            const int t = sqr(v - S.c[j]);
            if (t < bd) bd = t, best = j;
        }
        S.hist[v] = best;
    }
    __syncthreads();
    // the map over rows x cols, extended to block_width x block_height by the last valid column and row (extend_palette_color_map)
    uint8_t*  map  = maps + (size_t)tot * d.map_stride;
    const int bw   = d.block_width, area = bw * d.block_height, sh = floor_log2((uint32_t)bw);
    for (int p = lane; p < area; p += WAVE) {
        const int r = min(p >> sh, d.rows - 1), c = min(p & (bw - 1), d.cols - 1);
        map[p]      = (uint8_t)S.hist[S.data[r * d.cols + c]];
    }
    return tot + 1;
}

template <typename PIX>
__global__ __launch_bounds__(WAVE) void palette_search_kernel(const PIX* __restrict__ src_base, const SvtHipPaletteSearchDesc* __restrict__ descs, const uint32_t n,
                                                              uint8_t* __restrict__ out_base, uint8_t* __restrict__ status) {
    __shared__ SearchShared S;
    const uint32_t          b = blockIdx.x;
    if (b >= n) return;
    const SvtHipPaletteSearchDesc d    = descs[b];
    const int                     lane = lane_of();
    if (!desc_ok(d)) {
        if (status && lane == 0) status[b] = 1;
        return;
    }
    constexpr int           bins = sizeof(PIX) == 1 ? 256 : 1024; // bit_depth_pal 8 / 10
    SvtHipPaletteSearchOut* out  = (SvtHipPaletteSearchOut*)(out_base + d.out_off);
    uint8_t*                maps = out_base + d.out_off + sizeof(SvtHipPaletteSearchOut);
    for (int v = lane; v < bins; v += WAVE) S.hist[v] = 0;
    if (lane < 16) S.cache[lane] = descs[b].cache[lane];
    __syncthreads();
    // the samples, once: into LDS and into the histogram
    const PIX* src   = src_base + d.src_off;
    const int  total = d.rows * d.cols;
    bool       bad   = false;
    for (int i = lane; i < total; i += WAVE) {
        const int r = i / d.cols, c = i - r * d.cols;
        const int v = src[(size_t)r * d.src_stride + c];
        S.data[i]   = (uint16_t)v;
        if (v < bins) atomicAdd(&S.hist[v], 1);
        else bad = true;
    }
    __syncthreads();
    // the distinct colours in ascending order
    int colors = 0;
    for (int base = 0; base < bins; base += WAVE) {
        const int                h   = S.hist[base + lane];
        const unsigned long long m   = __ballot(h != 0);
        const int                pos = colors + __popcll(m & ((1ull << lane) - 1));
        if (h != 0 && pos < WAVE) S.val[pos] = base + lane, S.cnt[pos] = h;
        colors += __popcll(m);
    }
    const bool any_bad = __ballot(bad) != 0;
    if (any_bad) colors = 0; // svt_av1_count_colors_highbd returns 0
    colors = uni(colors);
    __syncthreads();
    if (!(colors > 1 && colors <= 64)) {
        if (lane == 0) {
            out->n_cand = 0;
            if (status) status[b] = any_bad ? 2 : 0;
        }
        return;
    }
    const int lb = uni(S.val[0]), ub = uni(S.val[colors - 1]);
    const int nmax = min(colors, KMAX), maxv = bins - 1;
    // the dominant colours: highest count first, the lower value on equal counts -- a colour's place is the number of colours ahead of it
    if (lane < colors) {
        const int key = (S.cnt[lane] << 16) | (0xffff - S.val[lane]);
        int       ahead = 0;
        for (int l = 0; l < colors; l++) ahead += ((S.cnt[l] << 16) | (0xffff - S.val[l])) > key;
        if (ahead < KMAX) S.top[ahead] = S.val[lane];
    }
    __syncthreads();
    int tot = 0;
    const int step = uni(d.dominant_color_step);
    for (int m = nmax; m >= 2; m -= step) {
        if (lane < m) S.c[lane] = S.top[lane];
        __syncthreads();
        tot = palette_candidate(d, m, colors, maxv, S, out, maps, tot);
        __syncthreads();
    }
    const ColorPoints P{S.val, S.cnt, S.data, colors, total};
    for (int m = nmax; m >= 2; m--) {
        int c[KMAX];
        if (colors == 2) { // PALETTE_MIN_SIZE: the two colours are the centroids
            c[0] = lb, c[1] = ub;
#pragma unroll
            for (int q = 2; q < KMAX; q++) c[q] = 0;
        } else {
#pragma unroll
            for (int q = 0; q < KMAX; q++) c[q] = lb + (2 * q + 1) * (ub - lb) / m / 2;
            kmeans_run<1>(P, m, 50, S.km, c);
        }
#pragma unroll
        for (int q = 0; q < KMAX; q++)
            if (q < m && lane == 0) S.c[q] = c[q];
        __syncthreads();
        tot = palette_candidate(d, m, colors, maxv, S, out, maps, tot);
        __syncthreads();
    }
    if (lane == 0) {
        out->n_cand = (uint8_t)tot;
        if (status) status[b] = 0;
    }
}

// =====================================================================================================================================================
// D. rate of a candidate
// =====================================================================================================================================================
// svt_aom_get_palette_color_index_context_optimized: the context from the left, above and above-left neighbours and the index of the position's colour after the
// neighbours have been moved to the front in order of weight
__device__ __forceinline__ int color_context(const uint8_t* map, const int stride, const int r, const int c, int& color_idx) {
    int nb[3], sc[3] = {2, 2, 1};
    nb[0] = c > 0 ? map[r * stride + c - 1] & 7 : -1;
    nb[1] = r > 0 ? map[(r - 1) * stride + c] & 7 : -1;
    nb[2] = c > 0 && r > 0 ? map[(r - 1) * stride + c - 1] & 7 : -1;
    if (nb[0] == nb[1]) {
        sc[0] += sc[1], nb[1] = -1;
        if (nb[0] == nb[2]) sc[0] += sc[2], nb[2] = -1;
    } else if (nb[0] == nb[2]) {
        sc[0] += sc[2], nb[2] = -1;
    } else if (nb[1] == nb[2]) {
        sc[1] += sc[2], nb[2] = -1;
    }
    int col[3] = {-1, -1, -1}, scr[3] = {0, 0, 0}, nv = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (nb[i] != -1) {
            if (nv == 0) col[0] = nb[i], scr[0] = sc[i];
            else if (nv == 1) col[1] = nb[i], scr[1] = sc[i];
            else col[2] = nb[i], scr[2] = sc[i];
            nv++;
        }
    }
#define SVT_PAL_SWAP(a, b) { const int ts = scr[a], tc = col[a]; scr[a] = scr[b], col[a] = col[b], scr[b] = ts, col[b] = tc; }
    if (scr[0] < scr[1] || (scr[0] == scr[1] && col[0] > col[1])) SVT_PAL_SWAP(0, 1)
    if (scr[0] < scr[2]) SVT_PAL_SWAP(0, 2)
    if (scr[1] < scr[2]) SVT_PAL_SWAP(1, 2)
#undef SVT_PAL_SWAP
    const int cur = map[r * stride + c] & 7;
    int       idx = cur, same = -1;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (col[i] > cur) idx++;
        else if (col[i] == cur) same = i;
    }
    color_idx      = same != -1 ? same : idx;
    const int hash = scr[0] + 2 * scr[1] + 2 * scr[2]; // 2, 5, 6, 7 or 8
    return hash == 2 ? 0 : 9 - hash;                   // svt_aom_palette_color_index_context_lookup
}

// svt_av1_palette_color_cost_y: svt_av1_index_color_cache (which colours the cache already has), delta_encode_cost of the others with min_val 1, av1_cost_literal
__device__ int color_cost_y(const uint16_t* colors, const int n, const uint16_t* cache, const int n_cache, const int bit_depth) {
    uint32_t in_cache = 0;
    if (n_cache > 0) {
        int found = 0;
        for (int i = 0; i < n_cache && found < n; i++)
            for (int j = 0; j < n; j++)
                if (colors[j] == cache[i]) {
                    in_cache |= 1u << j;
                    found++;
                    break;
                }
    }
    int num = 0, first = 0, prev = 0, max_delta = 0;
    for (int j = 0; j < n; j++) {
        if ((in_cache >> j) & 1) continue;
        if (num == 0) first = colors[j];
        else max_delta = max(max_delta, (int)colors[j] - prev);
        prev = colors[j];
        num++;
    }
    int bits = 0;
    if (num > 0) {
        bits = bit_depth;
        if (num > 1) {
            bits += 2;
            int per   = max(ceil_log2(max_delta + 1 - 1), bit_depth - 3);
            int range = (1 << bit_depth) - first - 1;
            int seen  = 0;
            for (int j = 0; j < n; j++) {
                if ((in_cache >> j) & 1) continue;
                if (seen++ > 0) {
                    bits += per;
                    range -= (int)colors[j] - prev;
                    per = min(per, ceil_log2(range));
                }
                prev = colors[j];
            }
        }
    }
    return (n_cache + bits) * 512; // av1_cost_literal: 1 << AV1_PROB_COST_SHIFT per bit
}

__global__ __launch_bounds__(WAVE) void palette_cost_kernel(const uint8_t* __restrict__ base, const SvtHipPaletteCostDesc* __restrict__ descs, const uint32_t n,
                                                            const int32_t* __restrict__ color_cost, int32_t* __restrict__ out, uint8_t* __restrict__ status) {
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    __shared__ __attribute__((aligned(4))) uint8_t s_map[64 * 64];
    __shared__ int                                 s_table[5 * 8];
    const SvtHipPaletteCostDesc d    = descs[b];
    const int                   lane = lane_of();
    if (!desc_ok(d)) {
        if (status && lane == 0) status[b] = 1;
        return;
    }
    // the rows of the map and the 5 x 8 costs of this palette size go through LDS: every position reads four map bytes and one cost
    const uint8_t* gmap  = base + d.map_off;
    const int      bytes = d.rows * d.block_width; // a multiple of 8
    if (uni((int)((uintptr_t)gmap & 3)) == 0) {
        for (int i = 4 * lane; i < bytes; i += 4 * WAVE) *(uint32_t*)&s_map[i] = *(const uint32_t*)(gmap + i);
    } else {
        for (int i = lane; i < bytes; i += WAVE) s_map[i] = gmap[i];
    }
    if (lane < 5 * 8) s_table[lane] = color_cost[(d.size - 2) * 5 * 8 + lane];
    __syncthreads();
    const uint8_t* map   = s_map;
    const int      total = d.rows * d.cols;
    const uint32_t inv   = ((1u << 20) + d.cols - 1) / d.cols; // p / cols == (p * inv) >> 20 for p < 4096, cols <= 64
    long long      sum   = 0;
    for (int p = 1 + lane; p < total; p += WAVE) { // every position but (0, 0); the C walks them in diagonals, the sum does not care
        const int r = (int)(((uint32_t)p * inv) >> 20), c = p - r * d.cols;
        int       idx;
        const int ctx = color_context(map, d.block_width, r, c, idx);
        sum += s_table[ctx * 8 + idx];
    }
    sum = wave_sum_i64(sum);
    if (lane == 0) {
        const uint16_t* colors = (const uint16_t*)(base + d.colors_off);
        out[3 * b + 0] = (int32_t)sum;
        out[3 * b + 1] = color_cost_y(colors, d.size, descs[b].cache, d.n_cache, d.bit_depth);
        const int l = floor_log2(d.size) + 1, m = (1 << l) - d.size; // svt_aom_write_uniform_cost(size, map[0]); size >= 2, so l >= 2
        out[3 * b + 2] = ((int)map[0] < m ? l - 1 : l) * 512;
        if (status) status[b] = 0;
    }
}

// =====================================================================================================================================================
// E. prediction
// =====================================================================================================================================================
template <typename PIX>
__global__ __launch_bounds__(TPB) void palette_pred_kernel(const uint8_t* __restrict__ base, PIX* __restrict__ dst_base, const SvtHipPalettePredDesc* __restrict__ descs,
                                                           const uint32_t n, const int maxv, uint8_t* __restrict__ status) {
    const uint32_t b = blockIdx.x;
    if (b >= n) return;
    const SvtHipPalettePredDesc d = descs[b];
    if (!desc_ok(d)) {
        if (status && threadIdx.x == 0) status[b] = 1;
        return;
    }
    const uint8_t*  map    = base + d.map_off + (size_t)d.y * d.wpx + d.x;
    const uint16_t* colors = (const uint16_t*)(base + d.colors_off);
    PIX*            dst    = dst_base + d.dst_off;
    const int       sh     = floor_log2(d.w), area = d.w * d.h;
    for (int p = threadIdx.x; p < area; p += TPB) {
        const int r = p >> sh, c = p & (d.w - 1);
        const int v = colors[map[r * d.wpx + c] & 7];
        dst[(size_t)r * d.dst_stride + c] = (PIX)min(v, maxv);
    }
    if (status && threadIdx.x == 0) status[b] = 0;
}

// =====================================================================================================================================================
// F. single-call forms: host pointers; upload, one launch, download.  Nothing of the caller's is written before the last HIP operation has succeeded.
// =====================================================================================================================================================
bool kmeans_host(const int* data, int* centroids, uint8_t* indices, const int n, const int k, const int max_itr, const int dim, const bool assign_only) {
    if (!data || !centroids || !indices || n < 1 || n > MAX_POINTS || k < 1 || k > KMAX) return false;
    const size_t      db = (size_t)n * dim * 4, cb = (size_t)k * dim * 4;
    svthip::HostCall& c  = svthip::host_call();
    c.begin();
    const size_t bytes = db + cb + (size_t)n + sizeof(SvtHipKmeansDesc) + 4096;
    c.reserve(bytes, bytes);
    int32_t*          dd = (int32_t*)c.dalloc(db);
    int32_t*          dc = (int32_t*)c.dalloc(cb);
    uint8_t*          di = (uint8_t*)c.dalloc((size_t)n);
    SvtHipKmeansDesc* dv = (SvtHipKmeansDesc*)c.dalloc(sizeof(SvtHipKmeansDesc));
    SvtHipKmeansDesc  d{};
    d.n = n, d.max_itr = max_itr, d.dim = (uint8_t)dim, d.k = (uint8_t)k, d.assign_only = assign_only ? 1 : 0;
    c.up(dd, data, db);
    c.up(dc, centroids, cb);
    c.up(dv, &d, sizeof(d));
    hipLaunchKernelGGL(kmeans_kernel, dim3(1), dim3(WAVE), 0, c.stream, (const int32_t*)dd, dc, di, (const SvtHipKmeansDesc*)dv, 1u, (uint8_t*)nullptr);
    SVT_LAUNCH_CHECK();
    if (!assign_only) c.down_later(centroids, dc, cb);
    c.down_later(indices, di, (size_t)n);
    c.finish();
    return true;
}

template <typename PIX> int count_colors_host(const PIX* src, const int stride, const int rows, const int cols, const int bit_depth, int* val_count) {
    if (!src || !val_count || rows < 1 || cols < 1 || rows > 65535 || cols > 65535 || stride < cols) return 0;
    if (sizeof(PIX) == 1 ? bit_depth != 8 : (bit_depth != 8 && bit_depth != 10 && bit_depth != 12)) return 0;
    const int         bins = 1 << bit_depth;
    const size_t      sb = (size_t)rows * cols * sizeof(PIX), hb = (size_t)bins * 4;
    svthip::HostCall& c  = svthip::host_call();
    c.begin();
    const size_t bytes = sb + hb + sizeof(SvtHipCountColorsDesc) + 4096;
    c.reserve(bytes, bytes);
    PIX*                   ds = (PIX*)c.dalloc(sb);
    int32_t*               dh = (int32_t*)c.dalloc(hb);
    int32_t*               dn = (int32_t*)c.dalloc(4);
    SvtHipCountColorsDesc* dv = (SvtHipCountColorsDesc*)c.dalloc(sizeof(SvtHipCountColorsDesc));
    SvtHipCountColorsDesc  d{};
    d.src_stride = (uint32_t)cols, d.rows = (uint16_t)rows, d.cols = (uint16_t)cols;
    c.up2d(ds, (size_t)cols * sizeof(PIX), src, (size_t)stride * sizeof(PIX), (size_t)cols * sizeof(PIX), rows);
    c.up(dv, &d, sizeof(d));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(count_colors_kernel<PIX>), dim3(1), dim3(TPB), 0, c.stream, (const PIX*)ds, (const SvtHipCountColorsDesc*)dv, 1u, bins, dh, dn,
                       (uint8_t*)nullptr);
    SVT_LAUNCH_CHECK();
    int32_t colors = 0;
    c.down_later(val_count, dh, hb);
    c.down_later(&colors, dn, 4);
    c.finish();
    return colors;
}

} // namespace

extern "C" {

#define SVT_PAL_BATCH_PROLOGUE(D)                                              \
    if (n == 0) return 0;                                                      \
    if (svthip::failed()) return SVT_HIP_E_DEVICE;                             \
    SVT_HIP_ENTRY_TRY                                                          \
    svthip::ensure_device();                                                   \
    hipStream_t st = (hipStream_t)stream;                                      \
    if (!status && !descs_all_valid<D>(descs, n, st)) return -1;

int svt_hip_kmeans_batch(const int32_t* data_base, int32_t* centroids_base, uint8_t* indices_base, const SvtHipKmeansDesc* descs, uint32_t n, uint8_t* status,
                         void* stream) {
    if (n && (!data_base || !centroids_base || !indices_base || !descs)) return -1;
    SVT_PAL_BATCH_PROLOGUE(SvtHipKmeansDesc)
    hipLaunchKernelGGL(kmeans_kernel, dim3(n), dim3(WAVE), 0, st, data_base, centroids_base, indices_base, descs, n, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_count_colors_batch(const void* src_base, const SvtHipCountColorsDesc* descs, uint32_t n, int bit_depth, int32_t* hist_base, int32_t* n_colors,
                               uint8_t* status, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n && (!src_base || !descs || !hist_base || !n_colors)) return -1;
    SVT_PAL_BATCH_PROLOGUE(SvtHipCountColorsDesc)
    if (bit_depth > 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(count_colors_kernel<uint16_t>), dim3(n), dim3(TPB), 0, st, (const uint16_t*)src_base, descs, n, 1 << bit_depth, hist_base, n_colors,
                           status);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(count_colors_kernel<uint8_t>), dim3(n), dim3(TPB), 0, st, (const uint8_t*)src_base, descs, n, 256, hist_base, n_colors, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_palette_search_luma_batch(const void* src_base, const SvtHipPaletteSearchDesc* descs, uint32_t n, int bit_depth, void* out_base, uint8_t* status,
                                      void* stream) {
    if (bit_depth != 8 && bit_depth != 10) return -1;
    if (n && (!src_base || !descs || !out_base)) return -1;
    SVT_PAL_BATCH_PROLOGUE(SvtHipPaletteSearchDesc)
    if (bit_depth > 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(palette_search_kernel<uint16_t>), dim3(n), dim3(WAVE), 0, st, (const uint16_t*)src_base, descs, n, (uint8_t*)out_base, status);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(palette_search_kernel<uint8_t>), dim3(n), dim3(WAVE), 0, st, (const uint8_t*)src_base, descs, n, (uint8_t*)out_base, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_palette_cost_batch(const void* base, const SvtHipPaletteCostDesc* descs, uint32_t n, const int32_t* color_cost, int32_t* out, uint8_t* status,
                               void* stream) {
    if (n && (!base || !descs || !color_cost || !out)) return -1;
    SVT_PAL_BATCH_PROLOGUE(SvtHipPaletteCostDesc)
    hipLaunchKernelGGL(palette_cost_kernel, dim3(n), dim3(WAVE), 0, st, (const uint8_t*)base, descs, n, color_cost, out, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

int svt_hip_palette_pred_batch(const void* base, void* dst_base, const SvtHipPalettePredDesc* descs, uint32_t n, int dst16, int bit_depth, uint8_t* status,
                               void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (!dst16 && bit_depth != 8) return -1;
    if (n && (!base || !dst_base || !descs)) return -1;
    SVT_PAL_BATCH_PROLOGUE(SvtHipPalettePredDesc)
    if (dst16)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(palette_pred_kernel<uint16_t>), dim3(n), dim3(TPB), 0, st, (const uint8_t*)base, (uint16_t*)dst_base, descs, n,
                           bit_depth == 8 ? 0xFF : 0xFFFF, status);
    else // the C's 8-bit predictor casts the colour to uint8_t
        hipLaunchKernelGGL(HIP_KERNEL_NAME(palette_pred_kernel<uint8_t>), dim3(n), dim3(TPB), 0, st, (const uint8_t*)base, (uint8_t*)dst_base, descs, n, 0xFFFF, status);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}
#undef SVT_PAL_BATCH_PROLOGUE

// svt_get_palette_cache_y: the two ascending lists merged, a value equal to the last one taken is not taken again
int svt_hip_palette_cache_y(const uint16_t* above_colors, int above_n, const uint16_t* left_colors, int left_n, uint16_t* cache) {
    if (!cache || above_n < 0 || left_n < 0 || above_n > KMAX || left_n > KMAX || (above_n && !above_colors) || (left_n && !left_colors)) return 0;
    int  n = 0, a = 0, l = 0;
    auto add = [&](const uint16_t v) {
        if (n > 0 && v == cache[n - 1]) return;
        cache[n++] = v;
    };
    while (a < above_n && l < left_n) {
        const uint16_t va = above_colors[a], vl = left_colors[l];
        if (vl < va) add(vl), l++;
        else {
            add(va), a++;
            if (vl == va) l++;
        }
    }
    while (a < above_n) add(above_colors[a++]);
    while (l < left_n) add(left_colors[l++]);
    return n;
}

void svt_av1_k_means_dim1_hip(const int* data, int* centroids, uint8_t* indices, int n, int k, int max_itr) {
    if (svthip::failed()) return;
    try { kmeans_host(data, centroids, indices, n, k, max_itr, 1, false); } catch (const svthip::DeviceError&) {}
}
void svt_av1_k_means_dim2_hip(const int* data, int* centroids, uint8_t* indices, int n, int k, int max_itr) {
    if (svthip::failed()) return;
    try { kmeans_host(data, centroids, indices, n, k, max_itr, 2, false); } catch (const svthip::DeviceError&) {}
}
void svt_av1_calc_indices_dim1_hip(const int* data, const int* centroids, uint8_t* indices, int n, int k) {
    if (svthip::failed()) return;
    try { kmeans_host(data, const_cast<int*>(centroids), indices, n, k, 0, 1, true); } catch (const svthip::DeviceError&) {}
}
void svt_av1_calc_indices_dim2_hip(const int* data, const int* centroids, uint8_t* indices, int n, int k) {
    if (svthip::failed()) return;
    try { kmeans_host(data, const_cast<int*>(centroids), indices, n, k, 0, 2, true); } catch (const svthip::DeviceError&) {}
}
int svt_av1_count_colors_hip(const uint8_t* src, int stride, int rows, int cols, int* val_count) {
    if (svthip::failed()) return 0;
    try { return count_colors_host<uint8_t>(src, stride, rows, cols, 8, val_count); } catch (const svthip::DeviceError&) { return 0; }
}
int svt_av1_count_colors_highbd_hip(uint16_t* src, int stride, int rows, int cols, int bit_depth, int* val_count) {
    if (svthip::failed()) return 0;
    try { return count_colors_host<uint16_t>(src, stride, rows, cols, bit_depth, val_count); } catch (const svthip::DeviceError&) { return 0; }
}

} // extern "C"
