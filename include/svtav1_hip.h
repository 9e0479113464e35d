/*
 * svtav1_hip.h -- C ABI of libsvtav1_hip.so: the MI355X (gfx950) variant of SVT-AV1-PSY's block-DSP hot path.
 *
 * Two families of entry points:
 *
 *  (1) `*_hip` functions whose prototypes are IDENTICAL to the reference's RTCD function pointers
 *      (Source/Lib/Codec/aom_dsp_rtcd.h, common_dsp_rtcd.h).  They take HOST pointers, are synchronous and
 *      re-entrant, exactly like the `_c/_avx2` variants, so `svt_hip_setup_rtcd()` can install them as
 *      "just another SIMD variant".  Each one stages its operands to the GPU, runs the same kernel the batched
 *      entry point uses with n = 1, and copies the results back.  They exist for drop-in parity, not speed.
 *
 *  (2) `svt_hip_*_batch` functions: DEVICE pointers, asynchronous on the caller's HIP stream, one launch per
 *      primitive over all superblocks / blocks of a frame (or several frames).  These are the throughput path.
 *
 * Error policy: the reference's DSP kernels return void and cannot fail.  This library never falls back to a
 * CPU implementation: a missing device or a HIP error prints the failing call to stderr and abort()s.
 *
 * All kernels are integer and bit-exact with the reference `*_c` functions cited per declaration.
 */
#ifndef SVTAV1_HIP_H
#define SVTAV1_HIP_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* PODs of this header that mirror a struct of the reference (SvtHipMv, SvtHipMvCostParams, SvtHipTxfmParam, SvtHipBuf2D, SvtHipCdefList, SvtHipSgrParams,
 * SvtHipConvolveParams) are self-contained definitions with the reference's layout, so the header needs none of the reference's.  A translation unit that HAS the
 * reference's headers (the in-encoder binding; tests/abi/abi_typecheck.c) defines SVT_HIP_REFERENCE_TYPES after including them: each of those names is then a
 * typedef of the reference's own struct and every `_hip` prototype is spelled in the reference's types -- which is how tests/abi/abi_typecheck.c proves, at
 * compile time, that each of the 193 variants of csrc/rtcd_hooks.def has its dispatch pointer's exact prototype.  tests/abi/abi_layout.c static-asserts that the
 * self-contained definitions and the reference's structs agree in size and in every field offset. */

#ifdef SVT_HIP_REFERENCE_TYPES
typedef BlockSize SvtHipBlockSize;
#else
typedef uint8_t SvtHipBlockSize; /* BlockSize (definitions.h:764-791) is a packed one-byte enum */
#endif

/* ---------------------------------------------------------------- runtime ------------------------------------ */
/* Bind the calling process to HIP device `device` (one process per GPU). 0 on success, -1 if no usable device. */
int         svt_hip_init(int device);
void        svt_hip_shutdown(void);
const char *svt_hip_device_name(void);
/* one-time costs of the calling thread's device (context, code-object loading, first allocations) paid now instead of inside the first real call */
void svt_hip_warmup(void);
/* the same with the pooled stage arenas sized by the caller: stage_arenas = how many stage-sized host forms (`svt_hip_*_host`, `*_stage*`) will be in flight at once
 * (0-3; 0 = dispatch pointers only: nothing is pre-reserved), first_arena_mb = device MB of the first one (the loop-restoration search of a 1080p plane takes ~100 MB, of a
 * 4K plane ~400 MB; the other arenas get 96 MB).  svt_hip_warmup() = svt_hip_warmup_sized(3, 192). */
void svt_hip_warmup_sized(int stage_arenas, uint32_t first_arena_mb);
/* Page-locks a host buffer the caller will hand to the host-pointer forms again and again (an encoder's picture buffers): copies from / to it then go by DMA without
 * the runtime's staging pass.  Portable across devices.  0 on success; a buffer that is already registered, or that the runtime refuses, is left as it is (non-zero) --
 * registration is an optimisation, never a requirement.  Unregister before the buffer is freed. */
int svt_hip_host_register(void *buffer, size_t bytes);
int svt_hip_host_unregister(void *buffer);
/* Several GPUs from one process (frame-level sharding): the device is selected PER HOST THREAD, like HIP's own current device.  svt_hip_set_thread_device(d)
 * binds the calling thread to device d for every later call of this library on that thread (host-call arenas and streams are per thread AND device); -1 returns the
 * thread to the default device of svt_hip_init.  Returns 0, or -1 when d is not a device.  Objects that live on a device (ME sessions) remember it and make it current
 * inside their own entry points, whatever the calling thread's selection is.
 * Device numbers are LOGICAL: device d runs on GPU d % svt_hip_physical_device_count(), and everything the library keeps per device (arenas, streams, sessions,
 * resident planes, partition peers) is keyed by the logical number.  SVT_HIP_VIRTUAL_DEVICES=V in the environment, or svt_hip_set_virtual_devices(V) before the
 * extra devices are used, gives every GPU V logical devices (default 1: logical = physical): the multi-device paths -- SVT_HIP_DEVICES picture sharding, frame
 * partitions with their peer streams, events and peer copies -- then run concurrently on a node with a single GPU. */
int svt_hip_device_count(void);          /* logical devices */
int svt_hip_physical_device_count(void); /* GPUs */
int svt_hip_physical_device(int device); /* the GPU behind a logical device, -1 if it is not one */
int svt_hip_set_virtual_devices(int per_gpu);
int svt_hip_set_thread_device(int device);
int svt_hip_get_thread_device(void);
/* The measurement knobs SVT_HIP_LR_UR / SVT_HIP_CDEF_GPW are read from the environment once, at first use; this re-reads them (tests that sweep a knob). */
void svt_hip_tuning_reload(void);
/* Overwrite the reference's RTCD pointers (weak symbols; present only when linked into libSvtAv1Enc) with the
 * `_hip` variants.  Call right after svt_aom_setup_rtcd_internal() (Source/Lib/Globals/enc_handle.c:1444-1445).
 * Returns the number of pointers installed. */
int         svt_hip_setup_rtcd(uint64_t flags);
/* Error policy (SURVEY 8b "errors": a `_hip` variant must never propagate an error; Source/Lib/Codec/aom_dsp_rtcd.c:188: the reference's kernels cannot fail).
 * The FIRST HIP error inside the library (a failed allocation, copy, launch, synchronisation, or an arena limit) switches the device path OFF for the rest of the
 * process: it is recorded (svt_hip_last_error), every dispatch pointer svt_hip_setup_rtcd overwrote is put back to the variant the reference had selected, the
 * `_hip` call in flight finishes through that saved pointer, and every stage / host-form entry point (`svt_hip_*_host`, `svt_hip_*_stage*`, the ME session) returns
 * SVT_HIP_E_DEVICE (or NULL) from then on -- the encoder's seams decline and run the reference's own function.  Nothing aborts; there is no CPU path in here.
 * The device-pointer batch entry points (callers that own streams and device buffers: tests, bench) throw through to their caller's guard or terminate. */
#define SVT_HIP_E_DEVICE (-100)
const char *svt_hip_last_error(void); /* NULL while the device path is on */
int         svt_hip_failed(void);
void        svt_hip_rtcd_unhook(void); /* puts the saved dispatch pointers back (what the first error does) */
int         svt_hip_debug_inject_failure(void); /* test instrument: behaves as if a HIP call had just failed */
/* test instrument: how often a host form issued a HIP operation AFTER it had already written caller memory (must stay 0: a failed call is finished through the
 * reference's own function, csrc/rtcd_hook.hip, so nothing may be half done when an operation fails) */
uint64_t    svt_hip_debug_commit_violations(void);
/* SVT_HIP_COUNT mode (csrc/rtcd_hook.hip): calls made so far through each installed pointer; returns the number of counted pointers */
int         svt_hip_rtcd_call_counts(const char **names, uint64_t *counts, int max);
/* Cross-lane / packed-byte instruction self-test used by the GPU test-suite (returns 0 when the silicon agrees
 * with the C model that the CPU-side interpreter in tests/emu uses). */
int         svt_hip_selftest(uint32_t *results /* device, 64*8 u32 */, void *stream);

/* VALU issue-rate probe (kind: 0 v_sad_u8, 1 v_qsad_pk_u16_u8, 2 v_add/xor pair, 3 v_mul_lo_u32+add, 4 v_mad_i64_i32,
 * 5 v_alignbyte): each of blocks*256 lanes issues iters*8 independent ops.  Used by bench.py --probe. */
/* Streams and HIP graphs.  Every svt_hip_*_batch / *_frame entry point only enqueues work on the stream it is given (no host synchronisation),
 * so a per-picture launch sequence can be captured once (begin ... calls ... end) and replayed with one launch per picture. */
void       *svt_hip_stream_create(void);
void        svt_hip_stream_destroy(void *stream);
void        svt_hip_stream_synchronize(void *stream);
void        svt_hip_graph_capture_begin(void *stream);
void       *svt_hip_graph_capture_end(void *stream);   /* returns an executable graph */
void        svt_hip_graph_launch(void *graph_exec, void *stream);
void        svt_hip_graph_destroy(void *graph_exec);
void        svt_hip_rate_probe(int kind, uint32_t iters, uint32_t blocks, uint32_t *sink, void *stream);
/* Memory-traffic probe (bench.py calibrates rocprofv3's FETCH_SIZE / WRITE_SIZE on it, per access shape): grid lane t moves `width` (4 / 8 / 16) bytes of segment
 * t / (seg / width) -- segments of `seg` bytes every `pitch` bytes from `base` -- reading (write = 0) or storing (write = 1) every byte exactly once: lanes * width bytes. */
void        svt_hip_mem_probe(int write, int width, void *base, uint64_t lanes, uint32_t seg, uint32_t pitch, uint32_t *sink, void *stream);
/* the block kernels' shape: 64x64-byte blocks tiling a picture of `pitch`-byte rows (blocks_per_row per block row, each starting `misalign` bytes into its 64-byte column),
 * 256 lanes per block reading 64 rows x 4 x 16 bytes: lanes * 16 bytes, every byte once */
void        svt_hip_mem_probe_blocks(const void *base, uint64_t lanes, uint32_t pitch, uint32_t blocks_per_row, uint32_t misalign, uint32_t *sink, void *stream);

/* ---------------------------------------------------------------- SAD family (a1-a6) -------------- */
/* a1. svt_nxm_sad_kernel -> svt_nxm_sad_kernel_helper_c (Source/Lib/C_DEFAULT/compute_sad_c.c:209, body :20-37) */
uint32_t svt_nxm_sad_kernel_hip(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                                uint32_t height, uint32_t width);
/*     svt_aom_sad_16b_kernel_c (compute_sad_c.c:39-56) */
uint32_t svt_aom_sad_16b_kernel_hip(uint16_t *src, uint32_t src_stride, uint16_t *ref, uint32_t ref_stride,
                                    uint32_t height, uint32_t width);
/*     svt_aom_sad{W}x{H}_c / x4d (compute_sad_c.c:117-131): generic-size forms; the 22 fixed-size symbols
 *     svt_aom_sadWxH_hip / svt_aom_sadWxHx4d_hip are generated from these in sad.hip. */
uint32_t svt_aom_sad_wxh_hip(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, int w, int h);
void     svt_aom_sad_wxh_x4d_hip(const uint8_t *src, int src_stride, const uint8_t *const ref_array[4], int ref_stride,
                                 uint32_t *sad_array, int w, int h);

/* a2. svt_sad_loop_kernel -> svt_sad_loop_kernel_c (compute_sad_c.c:58-100) */
void svt_sad_loop_kernel_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride, uint32_t block_height,
                             uint32_t block_width, uint64_t *best_sad, int16_t *x_search_center, int16_t *y_search_center,
                             uint32_t src_stride_raw, uint8_t skip_search_line, int16_t search_area_width,
                             int16_t search_area_height);

/* a3. svt_ext_all_sad_calculation_8x8_16x16 -> _c (Source/Lib/Codec/motion_estimation.c:335-362) */
void svt_ext_all_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                               uint32_t mv, uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16,
                                               uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16,
                                               uint32_t p_eight_sad16x16[16][8], uint32_t p_eight_sad8x8[64][8],
                                               bool sub_sad);
/* a4. svt_ext_eight_sad_calculation_32x32_64x64 -> _c (motion_estimation.c:369-425) */
void svt_ext_eight_sad_calculation_32x32_64x64_hip(uint32_t p_sad16x16[16][8], uint32_t *p_best_sad_32x32,
                                                   uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                                   uint32_t *p_best_mv64x64, uint32_t mv, uint32_t p_sad32x32[4][8]);
/* a5. svt_ext_sad_calculation_8x8_16x16 -> _c (motion_estimation.c:98-164), ..._32x32_64x64 -> _c (:171-205) */
void svt_ext_sad_calculation_8x8_16x16_hip(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                           uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16, uint32_t *p_best_mv8x8,
                                           uint32_t *p_best_mv16x16, uint32_t mv, uint32_t *p_sad16x16,
                                           uint32_t *p_sad8x8, bool sub_sad);
void svt_ext_sad_calculation_32x32_64x64_hip(uint32_t *p_sad16x16, uint32_t *p_best_sad_32x32, uint32_t *p_best_sad_64x64,
                                             uint32_t *p_best_mv32x32, uint32_t *p_best_mv64x64, uint32_t mv,
                                             uint32_t *p_sad32x32);
/* a6. svt_initialize_buffer_32bits -> _c (Source/Lib/Codec/me_sad_calculation.c:14-17) */
void svt_initialize_buffer_32bits_hip(uint32_t *pointer, uint32_t count128, uint32_t count32, uint32_t value);

/* a7. svt_pme_sad_loop_kernel -> svt_pme_sad_loop_kernel_c (aom_dsp_rtcd.h:868, product_coding_loop.c:1900-1951): SAD + MV-rate search
 * of MD's predictive ME.  SvtHipMvCostParams is layout-identical to the reference's MV_COST_PARAMS (`struct svt_mv_cost_param`,
 * mcomp.h:37-48; MV = {int16 row, col}, block_structures.h:26; MV_COST_TYPE is a 1-byte enum, mcomp.h:29-36). */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef MV SvtHipMv;
typedef struct svt_mv_cost_param SvtHipMvCostParams;
#else
typedef struct SvtHipMv { int16_t row, col; } SvtHipMv;
typedef struct SvtHipMvCostParams {
    const SvtHipMv *ref_mv;
    SvtHipMv        full_ref_mv;
    uint8_t         mv_cost_type; /* 0 ENTROPY, 1 L1_LOWRES, 2 L1_MIDRES, 3 L1_HDRES, 4 OPT, 5 NONE */
    const int      *mvjcost;
    const int      *mvcost[2];    /* centred tables, index range [MV_LOW, MV_UPP] */
    int             error_per_bit, early_exit_th, sad_per_bit;
} SvtHipMvCostParams;
#endif
void svt_pme_sad_loop_kernel_hip(const SvtHipMvCostParams *mv_cost_params, uint8_t *src, uint32_t src_stride, uint8_t *ref,
                                 uint32_t ref_stride, uint32_t block_height, uint32_t block_width, uint32_t *best_cost, int16_t *best_mvx,
                                 int16_t *best_mvy, int16_t search_position_start_x, int16_t search_position_start_y,
                                 int16_t search_area_width, int16_t search_area_height, int16_t search_step, int16_t mvx, int16_t mvy);

/* ---- the ME stage as a per-picture service over HOST pictures (the caller owns host buffers) ----
 * A session keeps the last `ring_planes` padded luma planes (stride * rows bytes each, picture origin at (org_x, org_y)) resident in HBM: a picture is
 * uploaded once, when it is submitted as a source, and then serves as a reference by id.  Each submission runs on its own stream (upload -> descriptor
 * build -> svt_hip_me_fullpel_search_batch over every 64x64 SB x n_refs, search centre (0, 0) -> result download), so the copies of one picture overlap
 * the search of another.  Host buffers should come from svt_hip_host_alloc (pinned) for the copies to be asynchronous.
 * submit returns a slot (>= 0) to wait on; -1: a reference (or the unsent source) is not resident, -2: n_refs > max_refs, -3: ring too small.
 * Results: best_sad_host / best_mv_host [n_refs][SBs][85], valid after svt_hip_me_session_wait(slot).
 * THREADING: a session is NOT internally synchronised -- submit / invalidate / resident / wait of one session must be serialised by the caller (the ME
 * seam holds its picture lock around them); different sessions are independent.  A re-upload after invalidate reuses the freed ring entry. */
void *svt_hip_host_alloc(size_t bytes);
void  svt_hip_host_free(void *p);
void *svt_hip_me_session_create(uint32_t width, uint32_t height, uint32_t stride, uint32_t org_x, uint32_t org_y, uint32_t rows, uint32_t ring_planes,
                                uint32_t max_refs, uint32_t max_area_width, uint32_t max_area_height, uint32_t n_slots);
/* the same on a named GPU: the session's ring, slots and launches live on `device`, and its entry points make that device current for their duration whatever
 * the calling thread has selected -- one session per GPU is how an encoder shards pictures over several devices (frame-level sharding) */
void *svt_hip_me_session_create_on(int device, uint32_t width, uint32_t height, uint32_t stride, uint32_t org_x, uint32_t org_y, uint32_t rows, uint32_t ring_planes,
                                   uint32_t max_refs, uint32_t max_area_width, uint32_t max_area_height, uint32_t n_slots);
void  svt_hip_me_session_destroy(void *session);
int   svt_hip_me_session_submit(void *session, int64_t pic_id, const uint8_t *plane_host, const int64_t *ref_ids, uint32_t n_refs, uint32_t area_w,
                                uint32_t area_h, int sub_sad, uint32_t *best_sad_host, uint32_t *best_mv_host);
int  svt_hip_me_session_wait(void *session, int slot);
/* forget a resident picture whose host content changed (the next submission naming it as the source uploads it again); is a picture resident? */
void  svt_hip_me_session_invalidate(void *session, int64_t pic_id);
int   svt_hip_me_session_resident(void *session, int64_t pic_id);

/* ---- batched forms (device pointers) ---- */
typedef struct SvtHipSadPair {
    uint64_t src_off;    /* byte offset of the block's top-left sample from src_base */
    uint64_t ref_off;    /* same, from ref_base */
    uint32_t src_stride; /* bytes */
    uint32_t ref_stride;
} SvtHipSadPair;
/* n independent WxH SADs (a1 batched; BASELINE config 1 = 64x64 over all co-located SBs). sad_out[n]. */
void svt_hip_sad_nxm_batch(const uint8_t *src_base, const uint8_t *ref_base, const SvtHipSadPair *pairs, uint32_t n,
                           uint32_t width, uint32_t height, uint32_t *sad_out, void *stream);

typedef struct SvtHipSadLoopDesc {
    uint64_t src_off, ref_off;
    uint32_t src_stride, ref_stride, src_stride_raw;
    uint16_t block_width, block_height;
    int16_t  search_area_width, search_area_height;
    uint8_t  skip_search_line, pad[3];
} SvtHipSadLoopDesc;
typedef struct SvtHipSadLoopResult {
    uint64_t best_sad;
    int16_t  x_search_center, y_search_center;
    uint32_t valid; /* 0 when the search area was empty (reference leaves x/y untouched, best_sad = 0xffffff) */
} SvtHipSadLoopResult;
/* n exhaustive searches (a2 batched: pre-HME / HME level 0-2 of every SB). `keys` = device scratch, n*8 bytes.  The maxima over the batch
 * size the position tile and the LDS window (descriptors live on the device and are not read back): widest / tallest search area, widest /
 * tallest block, and the largest ref_stride / src_stride_raw (1 = full SAD, 2 = sub-sampled HME form; ref_stride must be a multiple of
 * src_stride_raw, as it is at every reference call site). */
void svt_hip_sad_loop_batch(const uint8_t *src_base, const uint8_t *ref_base, const SvtHipSadLoopDesc *descs, uint32_t n,
                            uint32_t max_area_width, uint32_t max_area_height, uint32_t max_block_width, uint32_t max_block_height,
                            int max_ref_step, SvtHipSadLoopResult *results, uint64_t *keys, void *stream);

/* One hierarchical-ME level for a whole picture = hme_level_0 / hme_level_1 / hme_level_2 (motion_estimation.c:820-921, 923-1018, 1020-1116) for
 * every (reference, 64x64 SB, search region): search-area placement (level 0: the region's cell of the num_hme_sa_w x num_hme_sa_h grid around
 * the co-located block; levels 1-2: centred on the previous level's result), clipping to the reference picture, svt_sad_loop_kernel, result
 * scaled to the next level's resolution (x4, x2, x1).  Descriptors are built and results post-processed on the device; the search itself is
 * svt_hip_sad_loop_batch.  Items are ordered ((ref * n_sb + sb) * num_hme_sa_h + sr_h) * num_hme_sa_w + sr_w.
 * prev_sc: [items][2] int16 (x, y) = the previous level's centres (levels 1, 2; ignored at level 0).  sad_out [items]; sc_out [items][2] is in/out:
 * an empty clipped area leaves the reference's centre variable untouched, so pre-fill with what init_me_hme_data leaves there (0). */
typedef struct SvtHipHmeLevelParams {
    uint8_t  level;                  /* 0: 1/16-area planes (x, y / 4), 1: quarter planes (/ 2), 2: full resolution */
    uint8_t  sub_sampled;            /* me_ctx->hme_search_method != FULL_SAD_SEARCH: every other block row, SAD doubled */
    uint8_t  num_hme_sa_w, num_hme_sa_h;
    int16_t  sa_width, sa_height;    /* per-region area: get_hme_l0_search_area at level 0, hme_l1_sa / hme_l2_sa above */
    uint32_t sbs_x, sbs_y, n_refs;   /* n_refs <= 8 */
    uint32_t prev_shift;             /* prev_sc >> prev_shift before use: 1 when level 1 is fed with level-0 output (hme_level1_b64, :2105-2110), else 0 */
    uint32_t aligned_width, aligned_height; /* full-resolution picture size rounded up to 8 (b64_width / b64_height, :3093-3100) */
    uint64_t src_off;                /* picture sample (0, 0) of the source plane at this level's resolution, from src_base */
    uint32_t src_stride;
    uint32_t ref_stride, ref_org_x, ref_org_y, ref_width, ref_height; /* EbPictureBufferDesc of the references at this resolution */
    uint64_t ref_off[8];             /* buffer_y[0] of each reference, from ref_base */
    uint8_t  per_ref_area;           /* 1: level-0 areas differ per reference (get_hme_l0_search_area, :1800-1866): use sa_*_ref[ref] instead of sa_width / sa_height */
    uint8_t  pad1[3];
    int16_t  sa_width_ref[8], sa_height_ref[8];
    uint8_t  n_refs_list0;           /* slots [0, n_refs_list0) are list 0 (needed with do_ref / pre-HME inputs) */
    uint8_t  ref_pic_index[8];       /* index of each slot inside its list */
    uint8_t  prehme_enabled;         /* chain form: after level 0 the worst of the 2 x 2 regions is replaced by the better pre-HME result if that beats it
                                        (hme_level0_b64 :2001-2031) */
    uint8_t  pad2[2];
    uint32_t zz_skip_th;             /* me_early_exit_th >> 2 (0 = off): items whose zero-motion SAD zz_sad[ref][sb] is below it skip the level with centre (0, 0) and SAD 0 (hme_level0_b64 :1922-1935, hme_level1_b64 :2057-2070; never applied at level 2) */
    /* level-0 areas that depend on the motion list 0 / reference 0 found for the SAME superblock (get_hme_l0_search_area, :1809-1836; the low-delay settings,
     * enc_mode_config.c:702-714): for every slot but 0 the divisor of the width is (1 + ref index) when that motion is horizontal (|x| > th_max, |y| < th_min), else
     * (2 + ref index); likewise the height with "vertical".  sa_*_ref[] hold the (1 + index) areas, sa_*_ref2[] the (2 + index) ones; 0 / 0 = off.  Chain form only. */
    uint16_t l0_mv_th_min, l0_mv_th_max;
    int16_t  sa_width_ref2[8], sa_height_ref2[8];
    /* enable_me_sr_adjustment == 2 (the screen-content levels 4 / 5, enc_mode_config.c:485-505) adds: when that motion is small on both axes (|x|, |y| < 3 th_min) both
     * divisors are (4 + ref index) (:1836-1841) -- sa_*_ref4[] */
    uint8_t  l0_still_rule, pad3;
    int16_t  sa_width_ref4[8], sa_height_ref4[8];
} SvtHipHmeLevelParams;
size_t svt_hip_hme_level_workspace(const SvtHipHmeLevelParams *params);
void   svt_hip_hme_level_batch(const SvtHipHmeLevelParams *params, const uint8_t *src_base, const uint8_t *ref_base, const int16_t *prev_sc,
                               const uint32_t *zz_sad, uint64_t *sad_out, int16_t *sc_out, void *workspace, void *stream);
/* Levels 0, 1 and 2 of every item in ONE launch (one wave walks an item through the three levels: level N+1 only needs level N's result of the same
 * item).  params[3] = the three levels (same n_refs / SB grid / regions; params[1].prev_shift = 1); src_base / ref_base / sad_out / sc_out: one
 * pointer per level; results identical to three svt_hip_hme_level_batch calls.  sc_out[lv] is in/out like there. */
typedef struct SvtHipPrehmeResult { /* me_ctx->prehme_data[list][ref][sr_i] (SearchInfo) of one (reference slot, SB, search region) */
    uint64_t sad;
    int16_t  mv_x, mv_y; /* best_mv.as_mv.col / row, full-resolution units */
    uint8_t  valid, performed, pad[2];
} SvtHipPrehmeResult;
typedef struct SvtHipHmeChainInputs { /* optional device inputs of the chain, any may be NULL */
    const uint32_t           *zz_sad;  /* [ref][sb]: see zz_skip_th */
    const uint8_t            *do_ref;  /* [sb][2][4] = search_results[list][ref].do_ref: a 0 entry skips levels 0 and 1 with centre (0, 0), SAD MAX_U32 (:1963-1973, :2071-2082) */
    const SvtHipPrehmeResult *prehme;  /* [ref][sb][2]: svt_hip_prehme_batch's output, used when params[0].prehme_enabled */
    uint32_t prev_me_stage_based_exit_th; /* me_ctx->prev_me_stage_based_exit_th (0 = off): a level is skipped, keeping the previous stage's centre and SAD, when that
                                           * SAD is already small -- level 0 from the better performed pre-HME region below th >> 4 (:1937-1957), level 1 from
                                           * level 0 below th >> 5 (:2086-2096), level 2 from level 1 below th >> 2 (:2144-2154) */
    uint8_t  n_levels;     /* 3 (or 0): levels 0-2; 1: level 0 only (final centre = the best level-0 region, :2215-2262); 2: enable_hme_level2_flag = 0 (presets M7 and above, enc_mode_config.c:1636-1640): levels 0 and 1 only,
                            * params[2] / sad_out[2] / sc_out[2] are not touched and the final centre is taken from level 1 (:2267-2309) */
    uint8_t  list1_no_hme; /* temporal_layer_index == 0: list 1's references take no part in HME (:1983, :2055, :2127): their items are skipped */
    uint8_t  pad[2];
} SvtHipHmeChainInputs;
void   svt_hip_hme_chain_batch(const SvtHipHmeLevelParams *params, const uint8_t *const *src_base, const uint8_t *const *ref_base,
                               const SvtHipHmeChainInputs *inputs, uint64_t *const *sad_out, int16_t *const *sc_out, void *stream);
/* What precedes the HME levels in hme_b64 (motion_estimation.c:2441-2450), for every SB of a picture:
 * svt_hip_me_ref_gate_batch = the second half of init_zz_sad (:2402-2417): when the best zero-motion SAD of the SB is below zz_sad_th, references other than the
 * first of each list whose zz_sad is zz_sad_pct % above it are dropped (temporal layers > 0 only).  do_ref [sb][2][4] in/out.
 * svt_hip_prehme_batch = prehme_b64 (:1722-1798): two long thin search regions (vertical, horizontal) on the 1/16-area planes per reference through
 * prehme_core (:1568-1666), with check_prehme_early_exit (zero-motion SAD below me_early_exit_th; list-1 shortcut from the list-0 result of the same
 * index), then reference pruning on the pre-HME SADs (:1781-1797).  out [ref][sb][2]; do_ref in/out. */
typedef struct SvtHipPrehmeParams {
    SvtHipHmeLevelParams plane;       /* level = 0 plane geometry, SB grid, n_refs, n_refs_list0, ref_pic_index, sub_sampled (areas / regions unused) */
    uint16_t sa_min_width[2], sa_min_height[2], sa_max_width[2], sa_max_height[2]; /* prehme_ctrl.prehme_sa_cfg[sr_i] */
    uint16_t hme_sr_factor[8];        /* per slot: svt_aom_get_scaled_picture_distance(picture distance) */
    uint8_t  skip_search_line, l1_early_exit, temporal_layer_gt0, pad;
    uint32_t me_early_exit_th;        /* 0 = off */
    uint32_t phme_sad_th; uint16_t phme_sad_pct; uint16_t pad2; /* me_hme_prune_ctrls */
} SvtHipPrehmeParams;
void   svt_hip_me_ref_gate_batch(const SvtHipHmeLevelParams *plane, const uint32_t *zz_sad, uint32_t zz_sad_th, uint32_t zz_sad_pct,
                                 int temporal_layer_gt0, uint8_t *do_ref, void *stream);
/* me_safe_limit_zz_th (init_zz_sad :2416-2436): where zz_sad of both lists' nearest references is below the threshold, every reference with ref_pic_index > 0
 * is dropped.  The picture-level conditions (hierarchical_levels > 0, top temporal layer, similar_brightness_refs) are the caller's: pass 0 when they fail. */
void   svt_hip_me_ref_safe_limit_batch(const SvtHipHmeLevelParams *plane, const uint32_t *zz_sad, uint32_t safe_limit_zz_th, uint8_t *do_ref, void *stream);
void   svt_hip_prehme_batch(const SvtHipPrehmeParams *params, const uint8_t *src_base, const uint8_t *ref_base, const uint32_t *zz_sad, uint8_t *do_ref,
                            SvtHipPrehmeResult *out, void *stream);

/* Integer ME of a whole picture from its HME results = set_final_seach_centre_sb (motion_estimation.c:2182-2368: per (reference, SB) the first
 * strictly smallest SAD over the search regions) + integer_search_b64's search-area geometry (:1294-1325, :1458-1508: min(sa_min * dist, sa_max),
 * enlargement for long search-centre components, division by reduce_me_sr_divisor, width rounded up to 8, centred on the HME result, clipped to the
 * picture + 63-sample border) + svt_hip_me_fullpel_search_batch, including hme_prune_ref_and_adjust_sr, the zero-motion early exit, check_00_center
 * and the 8x8-variance probe.  With me_sr_adjustment = 2 the second rule makes the references of an SB depend on the first one's final SADs: two passes.
 * hme_sad / hme_sc: the last HME level's outputs in svt_hip_hme_level_batch's item order ((ref * n_sb + sb) * regions + region).
 * do_ref ([n_sb][2][4] = search_results[list][ref].do_ref as svt_hip_me_results_batch takes it, or NULL = all; in/out: HME-based pruning clears entries): a 0 entry gets a 1 x 1 placeholder search whose results must
 * be ignored (the reference skips the reference picture, :1292-1293).  divisor ([n_sb][n_refs] uint32, or NULL = 1) = me_ctx->reduce_me_sr_divisor
 * as an input when sr_adjustment = 0; with sr_adjustment = 1 it is derived from the HME results (and written back when non-NULL).
 * zz_sad ([ref][sb], needed when me_early_exit_th != 0): svt_hip_me_zz_sad_batch.
 * Outputs: best_sad / best_mv [ref][sb][85] (as svt_hip_me_fullpel_search_batch), sc_out [ref][sb][2] + sad_out [ref][sb] = search_results[].hme_sc_x/y,
 * hme_sad. */
typedef struct SvtHipMeIntegerSearchParams {
    uint32_t sbs_x, sbs_y, n_refs;            /* reference slots (list 0 first), <= 8 */
    uint32_t regions;                         /* num_hme_sa_w * num_hme_sa_h entries per (ref, SB) in hme_sad / hme_sc */
    uint32_t aligned_width, aligned_height;   /* pcs->aligned_width / aligned_height */
    int16_t  sa_min_width, sa_min_height, sa_max_width, sa_max_height; /* me_ctx->me_sa */
    uint8_t  sub_sad;                         /* me_search_method == SUB_SAD_SEARCH */
    uint8_t  mv_adj_enabled, mv_adj_nearest_ref_only; /* me_ctx->mv_based_sa_adj */
    uint8_t  list1_no_hme;                    /* temporal_layer_index == 0 with two lists: set_final_seach_centre_sb (:2211, :2362-2373) gives list 1's slots the centre (0, 0)
                                               * and -- the variable is not reset -- the HME SAD of the last list-0 slot; their zz_sad stays ~0 (init_zz_sad :2390) */
    uint16_t mv_adj_mv_size_th, mv_adj_sa_multiplier;
    uint16_t dist[8];                         /* per slot: picture distance, through svt_aom_get_scaled_picture_distance unless ME_MCTF (:1300-1302) */
    uint8_t  ref_pic_index[8];                /* per slot: index inside its list (nearest_ref_only) */
    uint64_t src_off;                         /* picture sample (0, 0) of the source plane, from src_base */
    uint32_t src_stride;
    uint32_t ref_stride, ref_org_x, ref_org_y;
    uint64_t ref_off[8];                      /* buffer_y[0] of each reference, from ref_base */
    /* hme_prune_ref_and_adjust_sr (:2477-2518), between the final centres and the search: */
    uint8_t  n_refs_list0;                    /* slots [0, n_refs_list0) are list 0 */
    uint8_t  hme_prune_enabled;               /* me_hme_prune_ctrls.enable_me_hme_ref_pruning with a threshold != (uint16_t)~0 */
    uint16_t prune_ref_if_hme_sad_dev_bigger_than_th;
    uint8_t  sr_adjustment;                   /* me_sr_adjustment_ctrls.enable_me_sr_adjustment: 0, 1 or 2.  2 (screen-content levels 4 / 5) adds two rules to integer_search_b64
                                               * (:1349-1364, only without me_early_exit_th): the height halves when the HME result is already good (check_00_center's SAD of an
                                               * accurate centre, or -- is_ref -- the HME SAD, below 24 * 24); else both sides halve for every slot but the first when the first
                                               * slot's final 64x64 SAD of the same SB is below 5000 -- the first slot is therefore searched before the geometry of the others */
    uint8_t  pad2;
    uint16_t reduce_me_sr_based_on_mv_length_th, stationary_hme_sad_abs_th, stationary_me_sr_divisor, reduce_me_sr_based_on_hme_sad_abs_th,
             me_sr_divisor_for_low_hme_sad;
    uint32_t me_early_exit_th;                /* 0 = off; else zz_sad < th / 6 searches a single point (:1322-1327) */
    /* content-dependent steps of integer_search_b64 (extra per-item SADs / a single-point pre-search on the device): */
    uint8_t  is_ref;                          /* me_ctx->is_ref: with me_early_exit_th = 0, a non-zero search centre is checked against (0, 0) on the
                                                 sub-sampled 64x64 SAD (check_00_center, :1139-1206), after being clipped to the picture + 63 */
    uint8_t  me_8x8_var_enabled;              /* me_8x8_var_ctrls: areas > 24 positions first search the centre alone; the variance of its 64 8x8 SADs
                                                 scales the area (:1388-1420); the centre's results take part in the final minimum */
    uint8_t  pad3[2];
    uint32_t me_sr_div4_th, me_sr_div2_th, me_sr_mult2_th;
    uint32_t ref_width, ref_height;           /* EbPictureBufferDesc width / height of the references (check_00_center clips against them) */
    uint32_t tf_me_exit_th;                   /* ME_MCTF (svt_aom_motion_estimation_b64 :3109-3113): 0 = off; an SB whose first reference's HME SAD is below it is not
                                               * searched at all (its tables keep their initial content; the temporal filter then uses the 64x64 prediction only) */
    uint32_t pad4;
} SvtHipMeIntegerSearchParams;
size_t svt_hip_me_integer_search_workspace(const SvtHipMeIntegerSearchParams *params);
void   svt_hip_me_integer_search_batch(const SvtHipMeIntegerSearchParams *params, const uint8_t *src_base, const uint8_t *ref_base,
                                       const uint64_t *hme_sad, const int16_t *hme_sc, uint8_t *do_ref, uint32_t *divisor, const uint32_t *zz_sad,
                                       uint32_t *best_sad, uint32_t *best_mv, int16_t *sc_out, uint64_t *sad_out, void *workspace, void *stream);
/* init_zz_sad's per-(reference, SB) value (motion_estimation.c:2382-2400, get_zz_sad :1667-1689): SAD of the 64x64 block against the co-located
 * reference block on every other row, doubled, normalised by 4096 / (b64 width x height).  Geometry fields of params only.  zz_out [ref][sb]. */
void   svt_hip_me_zz_sad_batch(const SvtHipMeIntegerSearchParams *params, const uint8_t *src_base, const uint8_t *ref_base, uint32_t *zz_out,
                               void *stream);

/* Frame-batched integer full-pel search = open_loop_me_fullpel_search_sblock (motion_estimation.c:781-816), i.e.
 * a3+a4+a5+a6 fused: for every (64x64 SB, reference) item, all 85 block SADs (8x8..64x64) at every position of the
 * search area, keeping the first minimum in raster order (strict `<`), bests initialised to MAX_SAD_VALUE
 * (motion_estimation.h:85).  Output layout per item = p_sb_best_sad / p_sb_best_mv[85]: 64x64 @0, 32x32 @1-4,
 * 16x16 @5-20, 8x8 @21-84 (me_context.h:52-138); mv = (y << 16) | (uint16_t)x (motion_estimation.c:448-450). */
typedef struct SvtHipMeSearchDesc {
    uint64_t src_off;              /* me_ctx->b64_src_ptr relative to src_base */
    uint64_t ref_off;              /* top-left sample of the search area relative to ref_base */
    uint32_t src_stride;           /* me_ctx->b64_src_stride */
    uint32_t ref_stride;           /* interpolated_full_stride[list][ref] */
    int16_t  x_search_area_origin; /* added to the x index to form the MV */
    int16_t  y_search_area_origin;
    uint16_t search_area_width;
    uint16_t search_area_height;
} SvtHipMeSearchDesc;
#define SVT_HIP_ME_NUM_BLOCKS 85
/* bytes of device scratch needed for n items whose largest search area is max_w x max_h (0 for areas <= 64x32) */
size_t svt_hip_me_fullpel_search_workspace(uint32_t n, uint32_t max_w, uint32_t max_h);
void   svt_hip_me_fullpel_search_batch(const uint8_t *src_base, const uint8_t *ref_base, const SvtHipMeSearchDesc *descs,
                                       uint32_t n, uint32_t max_w, uint32_t max_h, int sub_sad, uint32_t *best_sad,
                                       uint32_t *best_mv, void *workspace, void *stream);

/* ---- ME result formatting: what svt_aom_motion_estimation_b64 does with the integer-search tables after the search,
 * motion_estimation.c:3121-3152 -- me_prune_ref (:1522-1566), construct_me_candidate_array{,_mrp_off,_single_ref} (:2532-2828),
 * compute_distortion (:2964-3008), perform_gm_detection (:2833-2961) -- for every 64x64 SB of a picture in one launch.
 * Inputs (device): best_sad / best_mv [ref slot][n_sb][85] as written by svt_hip_me_fullpel_search_batch with items ordered
 * slot * n_sb + sb, slot = (list ? num_of_ref_pic_to_search[0] : 0) + ref (a slot the search never wrote must hold 0 MVs, as
 * init_me_hme_data leaves them, :3049-3052); do_ref [n_sb][2][4] = search_results[list][ref].do_ref after HME pruning, updated in place;
 * sb_size [n_sb][2] = B64Geom width, height.
 * Outputs (device), addressed exactly as MeSbResults (me_sb_results.h:28-53) with n_pus = 85 / 21 / 5 (pcs.c:107-111):
 * total_me_candidate_index [n_sb][n_pus], me_mv_array [n_sb][n_pus * max_refs] (MvCandidate.as_int), me_candidate_array
 * [n_sb][n_pus * max_cand] (MeCandidate bit-field bytes).  Entries the reference does not write are left as the caller filled them. */
typedef struct SvtHipMeResultsParams {
    uint32_t n_sb;
    uint8_t  num_of_list_to_search;         /* MeContext */
    uint8_t  num_of_ref_pic_to_search[2];
    uint8_t  max_cand, max_refs, max_l0;    /* MotionEstimationData (pcs.h:500-502; svt_aom_get_max_allocated_me_refs, pcs.c:91-96) */
    uint8_t  enable_me_16x16, enable_me_8x8; /* PictureParentControlSet */
    uint8_t  only_l_bwd;                    /* scs->mrp_ctrls.only_l_bwd */
    uint8_t  use_best_unipred_cand_only;    /* MeContext */
    uint8_t  prune_ref;                     /* prune_ref && me_hme_prune_ctrls.enable_me_hme_ref_pruning (:3122) */
    uint8_t  low_resolution;                /* scs->input_resolution <= INPUT_SIZE_480p_RANGE */
    uint8_t  gm_enabled, gm_use_distance_based_active_th; /* pcs->gm_ctrls */
    uint16_t prune_ref_if_me_sad_dev_bigger_than_th;
    int32_t  prune_me_candidates_th;
    uint64_t picture_number;
    uint64_t ref_picture_number[2][4];      /* me_ds_ref_array[list][ref].picture_number */
} SvtHipMeResultsParams;
typedef struct SvtHipMeSbStats { /* the per-SB entries of the pcs arrays written by compute_distortion / perform_gm_detection */
    uint32_t me_64x64_distortion, me_32x32_distortion, me_16x16_distortion, me_8x8_distortion, me_8x8_cost_variance, rc_me_distortion;
    uint8_t  stationary_block_present_sb, rc_me_allow_gm, pad[2];
} SvtHipMeSbStats;
void svt_hip_me_results_batch(const SvtHipMeResultsParams *params, const uint32_t *best_sad, const uint32_t *best_mv, uint8_t *do_ref,
                              const uint8_t *sb_size, uint8_t *total_me_candidate_index, uint32_t *me_mv_array, uint8_t *me_candidate_array,
                              SvtHipMeSbStats *sb_stats, void *stream);
/* The session form: search as svt_hip_me_session_submit, then format on the device and download the final product instead of (or besides) the raw
 * tables.  params->n_sb is filled in by the session; num_of_ref_pic_to_search[0] + [1] must equal n_refs (list 0 references first in ref_ids),
 * else -4.  Host buffers (pinned for asynchronous copies): sizes as the device arrays above with n_pus from enable_me_16x16 / enable_me_8x8;
 * do_ref may be NULL (every reference allowed, nothing returned); best_sad / best_mv may be NULL.  Entries the reference leaves unwritten are 0. */
typedef struct SvtHipMeResultsHost {
    uint8_t         *do_ref;                   /* [n_sb][2][4] in/out, or NULL */
    uint8_t         *total_me_candidate_index; /* [n_sb][n_pus] */
    uint32_t        *me_mv_array;              /* [n_sb][n_pus * max_refs] */
    uint8_t         *me_candidate_array;       /* [n_sb][n_pus * max_cand] */
    SvtHipMeSbStats *sb_stats;                 /* [n_sb] */
    uint32_t        *best_sad, *best_mv;       /* [n_refs][n_sb][85], or NULL */
    int16_t         *hme_sc;                   /* stage form: [n_refs][n_sb][2] = search_results[list][ref].hme_sc_x / hme_sc_y, or NULL */
    uint64_t        *hme_sad;                  /* stage form: [n_refs][n_sb] = search_results[list][ref].hme_sad, or NULL */
} SvtHipMeResultsHost;
int svt_hip_me_session_submit_results(void *session, int64_t pic_id, const uint8_t *plane_host, const int64_t *ref_ids, uint32_t n_refs,
                                      uint32_t area_w, uint32_t area_h, int sub_sad, const SvtHipMeResultsParams *params,
                                      const SvtHipMeResultsHost *out);

/* ---- temporal filter pixel kernels (the DSP part of Codec/temporal_filtering.c; fixed point) ----
 * The reference's RTCD pointers take a `struct MeContext *` (aom_dsp_rtcd.h:797-826); its layout is private to the encoder, so the `_hip`
 * functions take the handful of fields the kernels read as two plain structs instead (INTEGRATION.md shows the 12-line adapter that fills
 * them from a MeContext).  Everything else of each prototype is the reference's. */
typedef struct SvtHipTfParams { /* per picture */
    uint32_t tf_decay_factor_fp16[3]; /* me_ctx->tf_decay_factor_fp16[C_Y, C_U, C_V] (me_context.h:372) */
    uint16_t tf_mv_dist_th;           /* me_context.h:490 */
    uint8_t  tf_chroma;               /* :469 */
    uint8_t  use_zz_based_filter;     /* tf_ctrls.use_zz_based_filter (frame form only: selects the kernel) */
    uint8_t  encoder_bit_depth;       /* frame form only; the symbols below take it as an argument like the reference */
    uint8_t  ss_x, ss_y;              /* frame form only */
    uint8_t  pad;
} SvtHipTfParams;
typedef struct SvtHipTfBlock { /* per 32x32 luma block (idx_32x32 = tf_block_col + 2 * tf_block_row) and reference picture */
    uint64_t block_error[4]; /* split: tf_16x16_block_error[4 idx + i]; else [0] = tf_32x32_block_error[idx] (me_context.h:477,485) */
    int16_t  mv_x[4];        /* split: tf_16x16_mv_x[4 idx + i]; else [0] = tf_32x32_mv_x[idx] */
    int16_t  mv_y[4];
    uint8_t  split;          /* tf_32x32_block_split_flag[idx] */
    uint8_t  pad[7];
} SvtHipTfBlock;
/* svt_av1_apply_temporal_filter_planewise_medium{,_hbd} -> _c (temporal_filtering.c:1145-1196, 1332-1400), aom_dsp_rtcd.h:813-826 */
void svt_av1_apply_temporal_filter_planewise_medium_hip(const SvtHipTfParams *params, const SvtHipTfBlock *block, const uint8_t *y_src,
                                                        int y_src_stride, const uint8_t *y_pre, int y_pre_stride, const uint8_t *u_src,
                                                        const uint8_t *v_src, int uv_src_stride, const uint8_t *u_pre, const uint8_t *v_pre,
                                                        int uv_pre_stride, unsigned int block_width, unsigned int block_height, int ss_x, int ss_y,
                                                        uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum,
                                                        uint16_t *v_count);
void svt_av1_apply_temporal_filter_planewise_medium_hbd_hip(const SvtHipTfParams *params, const SvtHipTfBlock *block, const uint16_t *y_src,
                                                            int y_src_stride, const uint16_t *y_pre, int y_pre_stride, const uint16_t *u_src,
                                                            const uint16_t *v_src, int uv_src_stride, const uint16_t *u_pre, const uint16_t *v_pre,
                                                            int uv_pre_stride, unsigned int block_width, unsigned int block_height, int ss_x,
                                                            int ss_y, uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                                            uint32_t *v_accum, uint16_t *v_count, uint32_t encoder_bit_depth);
/* svt_av1_apply_zz_based_temporal_filter_planewise_medium{,_hbd} -> _c (temporal_filtering.c:867-903, 970-1013), aom_dsp_rtcd.h:798-811 */
void svt_av1_apply_zz_based_temporal_filter_planewise_medium_hip(const SvtHipTfParams *params, const SvtHipTfBlock *block, const uint8_t *y_pre,
                                                                 int y_pre_stride, const uint8_t *u_pre, const uint8_t *v_pre, int uv_pre_stride,
                                                                 unsigned int block_width, unsigned int block_height, int ss_x, int ss_y,
                                                                 uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                                                 uint32_t *v_accum, uint16_t *v_count);
void svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_hip(const SvtHipTfParams *params, const SvtHipTfBlock *block,
                                                                     const uint16_t *y_pre, int y_pre_stride, const uint16_t *u_pre,
                                                                     const uint16_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                                                     unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum,
                                                                     uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum,
                                                                     uint16_t *v_count, uint32_t encoder_bit_depth);
/* svt_estimate_noise_fp16 / svt_estimate_noise_highbd_fp16 -> _c (temporal_filtering.c:3847-3920), aom_dsp_rtcd.h:876-879; RTCD-hooked */
int32_t svt_estimate_noise_fp16_hip(const uint8_t *src, uint16_t width, uint16_t height, uint16_t stride_y);
int32_t svt_estimate_noise_highbd_fp16_hip(const uint16_t *src, int width, int height, int stride, int bd);
/* device form: plane in HBM (stride in samples), result written to noise_out[0]; workspace: svt_hip_estimate_noise_workspace() bytes, any content */
size_t svt_hip_estimate_noise_workspace(uint32_t width, uint32_t height);
void svt_hip_estimate_noise_batch(const void *plane, uint32_t width, uint32_t height, uint32_t stride, int bit_depth, int32_t *noise_out,
                                  void *workspace, void *stream);
/* Whole-picture temporal filtering given the motion-compensated predictions: for every 32x32 luma block (and its chroma blocks) the
 * accumulators start from the central picture with weight 1000 (svt_aom_apply_filtering_central{,_highbd}_c, :350-425), each reference adds
 * its plane-wise term (the functions above, chosen by use_zz_based_filter / encoder_bit_depth), and (accum + count / 2) / count is written
 * out (svt_aom_get_final_filtered_pixels_c, :2608-2672) -- produce_temporally_filtered_pic's steps 2-3 (:3360-3400) in one launch, accum and
 * count never leaving registers.  Planes are device pointers, strides in samples; out may alias central.  blocks: device,
 * [n_refs][nby][nbx]; nbx x nby 32x32 blocks are processed (the planes must cover them, as the reference's padded pictures do). */
#define SVT_HIP_TF_MAX_REFS 12   /* reference frames one launch of the frame kernel takes */
#define SVT_HIP_TF_MAX_FRAMES 32 /* = ALTREF_MAX_NFRAMES - 1 (definitions.h:304): every frame count the reference's temporal filter can use (chunked form, picture stage) */
typedef struct SvtHipTfPlanes {
    void    *y, *u, *v;
    uint32_t y_stride, uv_stride;
} SvtHipTfPlanes;
void svt_hip_tf_filter_frame(const SvtHipTfParams *params, const SvtHipTfPlanes *central, const SvtHipTfPlanes *preds, uint32_t n_refs,
                             const SvtHipTfBlock *blocks, uint32_t nbx, uint32_t nby, const SvtHipTfPlanes *out, void *stream);
/* The same for up to SVT_HIP_TF_MAX_FRAMES reference frames: chunks of SVT_HIP_TF_MAX_REFS, the accumulators of the frames so far travelling between the launches through
 * `workspace` (svt_hip_tf_filter_frame_workspace bytes, any content); only the last launch writes pixels, so out may still alias central. */
size_t svt_hip_tf_filter_frame_workspace(const SvtHipTfParams *params, uint32_t nbx, uint32_t nby);
void   svt_hip_tf_filter_frame_chunked(const SvtHipTfParams *params, const SvtHipTfPlanes *central, const SvtHipTfPlanes *preds, uint32_t n_refs,
                                       const SvtHipTfBlock *blocks, uint32_t nbx, uint32_t nby, const SvtHipTfPlanes *out, void *workspace, void *stream);

/* The temporal filter's sub-pel motion refinement, batched: replaces tf_subpel_search + svt_check_position (temporal_filtering.c:1560-1790) as
 * tf_64x64_sub_pel_search / tf_32x32_ / tf_16x16_ / tf_8x8_sub_pel_search (:1793-2250) call it for each block of a (central picture, reference
 * picture) pair.  Per block: the centre (predicted on the sub-sampled rows), then the half-, quarter- and eighth-pel rings around the running
 * best MV; each candidate = luma motion compensation (svt_aom_simple_luma_unipred: MV clamped to picture + border, EIGHTTAP_REGULAR or
 * bilinear kernels, the svt_av1_[highbd_]convolve_*_sr_c roundings) + svt_aom_mefn_ptr[bsize].vf / vf_hbd_10 against the source on every
 * (1 << subsampling_shift)-th row, << subsampling_shift; the reference's skip rules (mode >= 2: no diagonals; best == 0; early_exit_th) apply
 * in its order (x offset outer loop).  Blocks start from distortion INT_MAX like the callers (:1866, :1980, :2117).  All pointers device;
 * samples u8 (bit_depth 8) or u16 (10).  One wave per block; the result is bit-exact with the reference's (dist, mv_x, mv_y). */
typedef struct SvtHipTfSubpelParams {
    uint8_t  half_pel_mode, quarter_pel_mode, eight_pel_mode; /* pcs->tf_ctrls.*: 0 = off, 1 = all 8 neighbours, >= 2 = no diagonals */
    uint8_t  subsampling_shift;                               /* pcs->tf_ctrls.sub_sampling_shift */
    uint8_t  bit_depth;                                       /* 8 or 10 */
    uint8_t  pad[3];
    uint32_t early_exit_th;                                   /* me_ctx->tf_subpel_early_exit_th (0 = off) */
    uint32_t mi_rows, mi_cols;                                /* pcs->av1_cm->mi_rows / mi_cols (MV clamp) */
    uint32_t ref_org_x, ref_org_y, ref_stride;                /* reference pictures: padding origin and stride (samples) */
} SvtHipTfSubpelParams;
typedef struct SvtHipTfSubpelDesc {
    uint64_t src_off;    /* samples from src_base to the block's top-left source sample */
    uint64_t ref_off;    /* samples from ref_base to this block's reference picture's buffer_y (the padded plane's first sample) */
    uint32_t src_stride; /* samples */
    uint16_t pu_x, pu_y; /* block origin in the picture (luma samples) */
    uint8_t  bsize;      /* 8, 16, 32 or 64 (square) */
    uint8_t  bilinear;   /* me_ctx->tf_ctrls.use_2tap for the 64x64 / 32x32 searches (:1801-1804, :1911-1914): BILINEAR; 16x16 and 8x8 always EIGHTTAP_REGULAR */
    int16_t  mv_x, mv_y; /* starting MV, 1/8 pel (the integer ME vector << 3) */
    uint16_t pad;
} SvtHipTfSubpelDesc;
typedef struct SvtHipTfSubpelResult {
    uint64_t dist;       /* best distortion (tf_*_block_error) */
    int16_t  mv_x, mv_y; /* best MV, 1/8 pel */
    uint32_t pad;
} SvtHipTfSubpelResult;
void svt_hip_tf_subpel_search_batch(const SvtHipTfSubpelParams *params, const void *src_base, const void *ref_base, const SvtHipTfSubpelDesc *descs,
                                    uint32_t n, SvtHipTfSubpelResult *results, void *stream);
/* The same from HOST memory (a seam around tf_subpel_search, temporal_filtering.c:1670, calls it once per (central picture, reference picture) pair for every
 * block the reference may ask for): src_buf / ref_buf = the two pictures' whole padded luma buffers, the descs' offsets relative to them.  Synchronous. */
int svt_hip_tf_subpel_search_host(const SvtHipTfSubpelParams *params, const void *src_buf, size_t src_samples, const void *ref_buf, size_t ref_samples,
                                   const SvtHipTfSubpelDesc *descs, uint32_t n, SvtHipTfSubpelResult *results);

/* The temporal filter's final motion compensation, batched: replaces tf_64x64_inter_prediction / tf_32x32_ / tf_16x16_ / tf_8x8_inter_prediction
 * (temporal_filtering.c:2256-2620) for the blocks of a (central picture, reference picture) pair -- svt_aom_inter_prediction's uni-directional
 * SIMPLE_TRANSLATION path (enc_inter_prediction.c:4102) with MULTITAP_SHARP kernels (the 4-tap regular kernel for a chroma dimension <= 4), the MV
 * clamped per plane, luma + (chroma != 0: me_ctx->tf_chroma) both 4:2:0 chroma blocks at ((pu >> 3) << 3) / 2.  The prediction of a block lands at the
 * block's position in picture-sized planes -- the `preds` svt_hip_tf_filter_frame reads.  params: bit_depth, mi_rows / mi_cols, ref_org_x / ref_org_y (the
 * LUMA padding origin of the reference pictures; chroma: half); the strides come from `planes`.  All pointers device. */
typedef struct SvtHipTfMcPlanes {
    const void *ref[3];  /* base of the reference pictures' Y / U / V buffers */
    void       *pred[3]; /* base of the prediction planes */
    uint32_t    ref_stride[3], pred_stride[3]; /* samples */
} SvtHipTfMcPlanes;
typedef struct SvtHipTfMcDesc {
    uint64_t ref_off[3];  /* samples from ref[pl] to this block's reference picture's padded buffer of plane pl */
    uint64_t pred_off[3]; /* samples from pred[pl] to sample (0, 0) of this block's prediction plane pl */
    uint16_t pu_x, pu_y;  /* block origin (luma samples) */
    uint8_t  bsize, pad;  /* 8, 16, 32 or 64 */
    int16_t  mv_x, mv_y;  /* 1/8 pel (me_ctx->tf_*_mv_x / _y) */
    uint16_t pad2[3];
} SvtHipTfMcDesc;
void svt_hip_tf_inter_pred_batch(const SvtHipTfSubpelParams *params, const SvtHipTfMcPlanes *planes, const SvtHipTfMcDesc *descs, uint32_t n, int chroma, void *stream);
/* the same over a list whose length another kernel left in device memory (n_dev[0] <= max_n): the waves walk it with a grid stride, no host round trip for the count */
void svt_hip_tf_inter_pred_list(const SvtHipTfSubpelParams *params, const SvtHipTfMcPlanes *planes, const SvtHipTfMcDesc *descs, uint32_t max_n, const uint32_t *n_dev,
                                int chroma, void *stream);

/* The temporal filter of ONE central picture as a single device stage: produce_temporally_filtered_pic's per-block loop (temporal_filtering.c:3037-3400) for every
 * 64x64 block and every reference picture the caller kept (the picture-level skips of :3105-3131 -- ahd error, brightness change -- are the caller's), given the
 * ME results of each (central, reference) pair:
 *   1. the sub-pel refinements of every block size the reference may search (tf_64x64_ / tf_32x32_ / tf_16x16_ / tf_8x8_sub_pel_search, :1793-2250), batched;
 *   2. per (block, reference) the reference's decision tree on those results: 64x64 only when the ME exited early (motion_estimation.c:3110) or
 *      tf_use_64x64_pred says so (:2676, :3188-3190); else 64x64 when its error beats the four 32x32 (:3263-3270); else per 32x32 block one prediction
 *      (error below pred_error_32x32_th, :3292) or the 16x16 / 8x8 split of derive_tf_32x32_block_split_flag (:237-286);
 *   3. the final motion compensation of the chosen blocks (svt_hip_tf_inter_pred_batch) into picture-sized prediction planes;
 *   4. the 32x32 block errors of the 64x64 predictions (convert_64x64_info_to_32x32_info, :2691-2758);
 *   5. svt_hip_tf_filter_frame.
 * Host form: whole padded buffers in, the filtered 64x64 blocks written to out_* (which may be the central picture's own buffers, like the reference's in-place
 * result).  All pictures share one geometry (sp.ref_org_x / ref_org_y / ref_stride for luma, uv_stride and the halved origin for chroma; 4:2:0).
 * High bit depth (sp.bit_depth 10): the planes are the packed 16-bit pictures the reference filters (altref_buffer_highbd); with subpel_8bit the searches of step 1 read the 8-bit
 * luma of the same pictures instead, as the reference does with tf_ctrls.use_8bit_subpel.
 * Returns 0, or -1 for parameters outside what is built (n_refs > SVT_HIP_TF_MAX_FRAMES, n_refs == 0, not 4:2:0). */
typedef struct SvtHipTfPictureParams {
    SvtHipTfSubpelParams sp;  /* sub-pel controls, bit depth, mi_rows / mi_cols, the LUMA padding origin and stride of every picture */
    SvtHipTfParams       tf;  /* the filter's MeContext fields (frame form: all of them) */
    uint32_t pic_w_sb, pic_h_sb;      /* 64x64 blocks per row / column: blk_cols, blk_rows (:2823-2826); the ME tables hold pic_w_sb * pic_h_sb entries */
    uint32_t uv_stride;               /* chroma stride (samples) */
    uint32_t me_exit_th;              /* tf_ctrls.me_exit_th */
    uint64_t pred_error_32x32_th;     /* tf_ctrls.pred_error_32x32_th */
    uint8_t  use_2tap;                /* tf_ctrls.use_2tap: bilinear 64x64 / 32x32 searches */
    uint8_t  enable_8x8_pred;         /* tf_ctrls.enable_8x8_pred */
    uint8_t  use_pred_64x64_only_th;  /* tf_ctrls.use_pred_64x64_only_th */
    uint8_t  subpel_8bit;             /* high bit depth only: tf_ctrls.use_8bit_subpel -- the sub-pel searches run on the pictures' 8-bit luma (`y8`), everything else on the 16-bit planes (:3203, :3242) */
    uint8_t  zero_motion;             /* the low-delay form, produce_temporally_filtered_pic_ld (:3415-3846): no ME and no refinement, every block is predicted 64x64 at vector (0, 0)
                                       * (:3711-3726); the ME tables are not read (me may be NULL) */
    uint8_t  pad[3];
} SvtHipTfPictureParams;
typedef struct SvtHipTfHostPicture {
    const void *y, *u, *v;            /* the padded planes' first samples: buffer_y / buffer_cb / buffer_cr (8 bit), altref_buffer_highbd[C_Y / C_U / C_V] (sp.bit_depth 10: uint16) */
    size_t      y_samples, uv_samples;/* samples per plane (luma_size / chroma_size) */
    const void *y8;                   /* subpel_8bit: the picture's 8-bit luma buffer (buffer_y of the 10-bit picture: its 8 MSBs), same geometry; else NULL */
} SvtHipTfHostPicture;
typedef struct SvtHipTfMeTables { /* of one (central, reference) pair, [sb] = 64x64 block in raster order; the 85 entries in the ME order (64, 4 x 32, 16 x 16 z-order, 64 x 8 z-order) */
    const uint32_t *best_sad, *best_mv; /* [n_sb][85]: p_best_sad_* / p_best_mv* ((y << 16) | x, full pel) */
    const int16_t  *hme_sc;             /* [n_sb][2]: search_results[0][0].hme_sc_x / _y */
    const uint64_t *hme_sad;            /* [n_sb] */
} SvtHipTfMeTables;
typedef struct SvtHipTfPictureStats { /* what the decisions were (sums over blocks and references) */
    uint32_t blocks_64x64, blocks_32x32, blocks_16x16, blocks_8x8; /* predictions made per size */
    uint32_t early_exit_blocks;                                     /* (block, reference) pairs whose ME exited early */
    uint32_t pad[3];
} SvtHipTfPictureStats;
int svt_hip_tf_picture_host(const SvtHipTfPictureParams *params, const SvtHipTfHostPicture *central, const SvtHipTfHostPicture *refs, const SvtHipTfMeTables *me,
                            uint32_t n_refs, void *out_y, void *out_u, void *out_v, SvtHipTfPictureStats *stats /* or NULL */);
/* Device-resident form (for a caller whose pictures and ME tables are in HBM already, e.g. right after the ME stage): the reference frames' planes lie back to back
 * (ref_pitch / ref_uv_pitch samples apart), the ME tables are device arrays over all frames ([n_refs][n_sb][85] ...: `me` points to ONE SvtHipTfMeTables of device
 * pointers), the filtered 64x64 blocks replace the central picture in place, stats_dev (or NULL) receives the counts; asynchronous on `stream`. */
typedef struct SvtHipTfDevicePictures {
    void    *central[3];               /* the central picture's padded planes (first samples) */
    void    *refs[3];                  /* first reference frame's planes; frame r at + r * ref_pitch / ref_uv_pitch samples */
    uint64_t ref_pitch, ref_uv_pitch;  /* samples */
    void    *central_y8, *refs_y8;     /* subpel_8bit: the 8-bit luma copies (refs_y8: frames ref_y8_pitch samples apart); else NULL */
    uint64_t ref_y8_pitch;
} SvtHipTfDevicePictures;
size_t svt_hip_tf_picture_workspace(const SvtHipTfPictureParams *params, uint32_t n_refs); /* bytes; 0 for parameters outside what is built */
int    svt_hip_tf_picture(const SvtHipTfPictureParams *params, const SvtHipTfDevicePictures *pictures, const SvtHipTfMeTables *me, uint32_t n_refs, void *workspace,
                          SvtHipTfPictureStats *stats_dev, void *stream);

/* The whole open-loop ME stage from a HOST picture: upload -> quarter / sixteenth planes (made once per picture on the device, kept in the ring
 * with the full plane) -> HME levels 0-2 -> final search centre + integer_search_b64 geometry + full-pel search -> MeSbResults (+ raw tables on
 * request) -> download, on the submission's own stream like svt_hip_me_session_submit.  svt_hip_me_session_enable_stage sizes the extra
 * buffers once (decimated-plane padding as the reference's 32 / 16; max_regions = num_hme_sa_w * num_hme_sa_h; the largest ME area the stage
 * parameters can produce).  ref_ids: list-0 references first; results.num_of_ref_pic_to_search[0] + [1] must equal n_refs.  Every picture that
 * will serve as a reference must have been submitted after enable_stage (its decimated planes are made at upload time).  -5: not enabled, too
 * many regions, or areas beyond the enabled maximum. */
typedef struct SvtHipMeStageParams {
    uint8_t  num_hme_sa_w, num_hme_sa_h; /* me_ctx->num_hme_sa_w / num_hme_sa_h */
    uint8_t  hme_sub_sampled;            /* hme_search_method != FULL_SAD_SEARCH */
    uint8_t  me_sub_sad;                 /* me_search_method == SUB_SAD_SEARCH */
    int16_t  hme_sa_width[3], hme_sa_height[3]; /* per level: get_hme_l0_search_area, hme_l1_sa, hme_l2_sa */
    int16_t  me_sa_min_width, me_sa_min_height, me_sa_max_width, me_sa_max_height;
    uint8_t  mv_adj_enabled, mv_adj_nearest_ref_only;
    uint16_t mv_adj_mv_size_th, mv_adj_sa_multiplier;
    uint16_t dist[8];                    /* as SvtHipMeIntegerSearchParams */
    uint8_t  ref_pic_index[8];
    uint8_t  hme_l0_per_ref;             /* level-0 areas per reference (get_hme_l0_search_area) instead of hme_sa_width/height[0] */
    uint8_t  hme_prune_enabled, sr_adjustment; /* as SvtHipMeIntegerSearchParams */
    uint8_t  me_type_mctf;               /* me_type == ME_MCTF (the temporal filter's ME): dist[] holds the UNSCALED picture distances -- the integer search uses them as
                                          * they are (:1300-1302), pre-HME scales them itself -- and tf_me_exit_th applies */
    int16_t  hme_l0_sa_width_ref[8], hme_l0_sa_height_ref[8];
    uint16_t prune_ref_if_hme_sad_dev_bigger_than_th;
    uint16_t reduce_me_sr_based_on_mv_length_th, stationary_hme_sad_abs_th, stationary_me_sr_divisor, reduce_me_sr_based_on_hme_sad_abs_th,
             me_sr_divisor_for_low_hme_sad;
    uint32_t me_early_exit_th;           /* 0 = off */
    uint8_t  is_ref, me_8x8_var_enabled; /* as SvtHipMeIntegerSearchParams */
    uint8_t  hme_levels;                 /* 3 (or 0): enable_hme_level0/1/2_flag all set; 1: level 0 only (the temporal filter at hme_me_level 3 / 4); 2: enable_hme_level2_flag = 0 (M7 and above): the integer search starts from level 1 */
    uint8_t  pad1;
    uint32_t me_sr_div4_th, me_sr_div2_th, me_sr_mult2_th;
    uint8_t  temporal_layer_gt0;         /* me_ctx->temporal_layer_index > 0 (list 1 takes part in pre-HME / HME, reference gating is active); 0 = base layer: list 1's
                                          * references skip HME, start the integer search at (0, 0) and inherit the last list-0 slot's HME SAD for the pruning steps */
    uint8_t  prehme_enabled, prehme_skip_search_line, prehme_l1_early_exit; /* me_ctx->prehme_ctrl */
    uint16_t prehme_sa_min_width[2], prehme_sa_min_height[2], prehme_sa_max_width[2], prehme_sa_max_height[2];
    uint32_t zz_sad_th, phme_sad_th;     /* me_hme_prune_ctrls (0 = off) */
    uint16_t zz_sad_pct, phme_sad_pct;
    uint32_t prev_me_stage_based_exit_th; /* as SvtHipHmeChainInputs (0 = off; the RTC screen-content and the temporal-filter ME settings use 64 * 64 * 4) */
    uint32_t me_safe_limit_zz_th;         /* me_ctx->me_safe_limit_zz_th when the picture qualifies (see svt_hip_me_ref_safe_limit_batch), else 0 */
    uint32_t tf_me_exit_th;               /* the temporal filter's ME (me_type == ME_MCTF): as SvtHipMeIntegerSearchParams; that caller also passes dist[] unscaled
                                           * (:1300-1302), leaves hme_prune_enabled / sr_adjustment / results.prune_ref at 0 and takes the raw tables (out->best_sad /
                                           * best_mv, total_me_candidate_index = NULL: no MeSbResults are formatted) */
    SvtHipMeResultsParams results;       /* formatting parameters (n_sb is filled in by the session) */
    uint16_t reduce_hme_l0_sr_th_min, reduce_hme_l0_sr_th_max; /* me_ctx->reduce_hme_l0_sr_th_* when distance_based_hme_resizing is on (else 0): see SvtHipHmeLevelParams */
    int16_t  hme_l0_sa_width_ref2[8], hme_l0_sa_height_ref2[8]; /* the level-0 areas with the (2 + ref index) divisors */
    int16_t  hme_l0_sa_width_ref4[8], hme_l0_sa_height_ref4[8]; /* ... with the (4 + ref index) divisors: read with sr_adjustment == 2 only (SvtHipHmeLevelParams.l0_still_rule) */
} SvtHipMeStageParams;
int svt_hip_me_session_enable_stage(void *session, uint32_t quarter_pad, uint32_t sixteenth_pad, uint32_t max_regions, uint32_t max_me_area_width,
                                    uint32_t max_me_area_height);
int svt_hip_me_session_submit_stage(void *session, int64_t pic_id, const uint8_t *plane_host, const int64_t *ref_ids, uint32_t n_refs,
                                    const SvtHipMeStageParams *stage, const SvtHipMeResultsHost *out);

/* ---------------------------------------------------------------- transforms (a10, a12, a13, a14) --- */
/* TxSize / TxType numbering = Source/Lib/Codec/definitions.h (TX_4X4=0 .. TX_64X16=18; DCT_DCT=0 .. H_FLIPADST=15). */
typedef struct SvtHipFwdTxfmDesc {
    uint64_t in_off;    /* int16 elements from residual_base to the block's top-left residual */
    uint32_t in_stride; /* int16 elements */
    uint8_t  tx_type;
    uint8_t  pad[3];
} SvtHipFwdTxfmDesc;
/* n forward 2-D transforms of ONE tx_size (svt_av1_fwd_txfm2d_WxH -> av1_tranform_two_d_core_c, transforms.c:2259-2324).
 * pf_shape 0 = DEFAULT, 1 = N2, 2 = N4 (transforms.c:5202-5273: only the top-left 1/2, 1/4 corner is produced, rest 0).
 * coeff_out: n blocks of W*H int32, row-major, full W x H also for 64-point sizes (as the reference's output). */
void svt_hip_fwd_txfm2d_batch(const int16_t *residual_base, const SvtHipFwdTxfmDesc *descs, uint32_t n, int tx_size, int bit_depth,
                              int pf_shape, int32_t *coeff_out, void *stream);
typedef struct SvtHipInvTxfmDesc {
    uint64_t coeff_off;  /* int32 elements from coeff_base; block = min(W,32) x min(H,32) packed (inv_transforms.c:2567-2580) */
    uint64_t pred_off;   /* pixels from pred_base  (output_r) */
    uint64_t recon_off;  /* pixels from recon_base (output_w; may alias the prediction) */
    uint32_t pred_stride, recon_stride;
    uint8_t  tx_type;
    uint8_t  wht_full; /* svt_hip_iwht4x4_add_batch only: 1 = eob > 1 (16-coefficient form), 0 = DC-only form (inv_transforms.c:2826-2831) */
    uint8_t  pad[6];
} SvtHipInvTxfmDesc;
/* n inverse 2-D transforms + reconstruction (svt_av1_inv_txfm2d_add_WxH -> inv_txfm2d_add_c, inv_transforms.c:2459-2535) */
void svt_hip_inv_txfm2d_add_batch(const int32_t *coeff_base, const uint16_t *pred_base, uint16_t *recon_base,
                                  const SvtHipInvTxfmDesc *descs, uint32_t n, int tx_size, int bd, void *stream);
/* 8-bit pixel form (svt_av1_inv_txfm_add -> svt_av1_inv_txfm_add_c, inv_transforms.c:3177-3192) */
void svt_hip_inv_txfm2d_add_batch_u8(const int32_t *coeff_base, const uint8_t *pred_base, uint8_t *recon_base,
                                     const SvtHipInvTxfmDesc *descs, uint32_t n, int tx_size, void *stream);
/* The two entry points above compute the transform types AV1 allows for the size (test/TxfmCommon.h:160-209: DCT and identity only where a dimension is 32 or 64).
 * The reference's `_c` functions accept more: av1_iadst32_new (inv_transforms.c:1119-1552) gives every ADST type a result on the seven sizes with a 32-point
 * dimension, and the reference's own InvTxfm2dAddTest feeds them (test/InvTxfm2dAsmTest.cc:755-775).  The `_any_type` forms compute every type the `_c` function of
 * the size computes; the single-call `_hip` symbols go through them.  They are separate kernels because the 32-point ADST costs the 32x32 kernel 3 of its 7
 * waves per SIMD (71 -> 125 VGPRs); no bitstream reaches them. */
void svt_hip_inv_txfm2d_add_batch_any_type(const int32_t *coeff_base, const uint16_t *pred_base, uint16_t *recon_base,
                                           const SvtHipInvTxfmDesc *descs, uint32_t n, int tx_size, int bd, void *stream);
void svt_hip_inv_txfm2d_add_batch_any_type_u8(const int32_t *coeff_base, const uint8_t *pred_base, uint8_t *recon_base,
                                              const SvtHipInvTxfmDesc *descs, uint32_t n, int tx_size, void *stream);
/* single-call generic forms; the fixed-size RTCD symbols svt_av1_fwd_txfm2d_WxH[_N2|_N4]_hip (57) and
 * svt_av1_inv_txfm2d_add_WxH_hip (19, three signature shapes, common_dsp_rtcd.h:106-116) are generated from these. */
void svt_av1_fwd_txfm2d_hip(int16_t *input, int32_t *output, uint32_t input_stride, int tx_type, int tx_size, uint8_t bit_depth, int pf);
void svt_av1_inv_txfm2d_add_hip(const int32_t *input, uint16_t *output_r, int32_t stride_r, uint16_t *output_w, int32_t stride_w,
                                int tx_type, int tx_size, int32_t bd);
void svt_av1_inv_txfm_add_u8_hip(const int32_t *dqcoeff, uint8_t *dst_r, int32_t stride_r, uint8_t *dst_w, int32_t stride_w, int tx_type,
                                 int tx_size, int lossless, int eob);
/* svt_av1_inv_txfm_add (common_dsp_rtcd.h:144) -> svt_av1_inv_txfm_add_c (inv_transforms.c:3177-3192), exact prototype.
 * SvtHipTxfmParam is TxfmParam (definitions.h:1043-1055; TxType / TxSize are packed one-byte enums). */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef TxfmParam SvtHipTxfmParam;
#else
typedef struct SvtHipTxfmParam {
    uint8_t tx_type, tx_size;
    int32_t lossless, bd, is_hbd;
    uint8_t tx_set_type; /* TxSetType, a packed one-byte enum (definitions.h:1027-1041) */
    int32_t eob;
} SvtHipTxfmParam;
#endif
void svt_av1_inv_txfm_add_hip(const int32_t *dqcoeff, uint8_t *dst_r, int32_t stride_r, uint8_t *dst_w, int32_t stride_w,
                              const SvtHipTxfmParam *txfm_param);
/* Lossless mode: 4x4 Walsh-Hadamard.  svt_av1_fwht4x4 (aom_dsp_rtcd.h:208) -> svt_av1_fwht4x4_c (transforms.c:3099-3152);
 * inverse = svt_av1_highbd_iwht4x4_16_add_c / _1_add_c (inv_transforms.c:2735-2825; reached through svt_av1_inv_txfm_add and
 * svt_av1_highbd_inv_txfm_add_4x4 when TxfmParam.lossless is set).  Batched: one 4x4 block per descriptor; coeff_out[n][16]. */
void svt_av1_fwht4x4_hip(int16_t *input, int32_t *output, uint32_t stride);
void svt_hip_fwht4x4_batch(const int16_t *residual_base, const SvtHipFwdTxfmDesc *descs, uint32_t n, int32_t *coeff_out, void *stream);
void svt_hip_iwht4x4_add_batch(const int32_t *coeff_base, const uint16_t *pred_base, uint16_t *recon_base, const SvtHipInvTxfmDesc *descs,
                               uint32_t n, int bd, void *stream);
void svt_hip_iwht4x4_add_batch_u8(const int32_t *coeff_base, const uint8_t *pred_base, uint8_t *recon_base, const SvtHipInvTxfmDesc *descs,
                                  uint32_t n, void *stream);

/* ---------------------------------------------------------------- quantization (a11, a15, a16) ------- */
typedef struct SvtHipQuantParams { /* DC/AC pairs of MacroblockPlane's tables (md_config_process.c:111-189) */
    int16_t zbin[2], round[2], quant[2], quant_shift[2], dequant[2];
    int32_t log_scale; /* 0, 1 (32x32-class), 2 (64-point) -- full_loop.c:1690 */
} SvtHipQuantParams;
typedef struct SvtHipQuantDesc {
    uint32_t qparam_idx; /* row of qparams[]                                  */
    uint32_t iscan_idx;  /* row of iscan_tables[][n_coeffs] (ScanOrder.iscan) */
    uint32_t qm_idx;     /* row of qm_tables / iqm_tables (ignored when those are NULL) */
    uint32_t reserved;
} SvtHipQuantDesc;
/* n blocks of n_coeffs (16..1024, power of two) coefficients, blocks contiguous.  mode 0 = svt_aom_quantize_b_c_ii,
 * 1 = svt_aom_highbd_quantize_b_c, 2 = quantize_fp_helper_c, 3 = highbd_quantize_fp_helper_c (full_loop.c:29-453).
 * Outputs: qcoeff/dqcoeff [n][n_coeffs] (every element written), eob[n]. */
void svt_hip_quantize_batch(int mode, const int32_t *coeff, uint32_t n, uint32_t n_coeffs, const SvtHipQuantParams *qparams,
                            const int16_t *iscan_tables, const uint8_t *qm_tables, const uint8_t *iqm_tables,
                            const SvtHipQuantDesc *descs, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob, void *stream);
/* svt_handle_transform{64x64,32x64,64x32,16x64,64x16}[_N2_N4]_c (transforms.c:2374-2542), in place on n blocks of W*H:
 * energy[n] of the discarded high-frequency area + repack of 64-wide rows to stride 32. */
void svt_hip_handle_transform_batch(int32_t *coeff, uint32_t n, int tx_size, int n2_n4, uint64_t *energy, void *stream);
/* single-call forms; the ten RTCD quantizer symbols and the ten svt_handle_transformWxH[_N2_N4]_hip are thin aliases */
void     svt_quantize_hip(int mode, const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr,
                          const int16_t *quant_ptr, const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr,
                          const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan,
                          const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int log_scale);
uint64_t svt_handle_transform_hip(int32_t *output, int tx_size, int n2_n4);

/* BASELINE config 3 in ONE launch: forward transform -> (the 32x32 corner svt_handle_transform keeps of a 64-point block) -> quantize / dequantize -> inverse
 * transform + reconstruction; the coefficients stay in LDS between the stages (10 B/px of HBM traffic instead of 26; + 4 B/px when dqcoeff != NULL).
 * Bit-identical to svt_hip_fwd_txfm2d_batch(pf 0) -> svt_hip_handle_transform_batch -> svt_hip_quantize_batch -> svt_hip_inv_txfm2d_add_batch.
 * quant_mode as svt_hip_quantize_batch (0 / 2 with 8-bit pixels, 1 / 3 with 16-bit pixels); qcoeff / dqcoeff [n][min(W,32) * min(H,32)]; qm tables may be NULL. */
typedef struct SvtHipRoundtripDesc {
    uint64_t in_off;      /* int16 elements from residual_base */
    uint64_t pred_off;    /* pixels from pred_base */
    uint64_t recon_off;   /* pixels from recon_base (may alias the prediction) */
    uint32_t in_stride, pred_stride, recon_stride;
    uint32_t qparam_idx, iscan_idx, qm_idx; /* as SvtHipQuantDesc */
    uint8_t  tx_type;
    uint8_t  pad[7];
} SvtHipRoundtripDesc;
void svt_hip_txfm_quant_roundtrip_batch(const int16_t *residual_base, const void *pred_base, void *recon_base, const SvtHipRoundtripDesc *descs, uint32_t n,
                                        int tx_size, int bd, int quant_mode, const SvtHipQuantParams *qparams, const int16_t *iscan_tables,
                                        const uint8_t *qm_tables, const uint8_t *iqm_tables, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob, void *stream);

/* ------------------------------------------- RD distortion: SSE, coefficient SSE, psy-rd energy (last arrow) --------- */
/* One launch, n blocks of mixed sizes on resident planes.  Offsets and strides in pixels (8-bit planes: is16 = 0; uint16_t planes: is16 = 1). */
typedef struct SvtHipDistDesc {
    uint64_t in_off, rec_off;
    uint32_t in_stride, rec_stride;
    uint16_t width, height;
    uint32_t reserved;
} SvtHipDistDesc;
#define SVT_HIP_DIST_SSE 1
#define SVT_HIP_DIST_PSY 2
/* what = SVT_HIP_DIST_SSE | SVT_HIP_DIST_PSY (both come from the same loaded pixels; an array that is not asked for is not touched).
 * sse_out[i] -> svt_spatial_full_distortion_kernel_c (picture_operators_c.c:65-83) / svt_full_distortion_kernel16_bits_c (pic_operators.c:174-197), any width and
 *               height >= 1.
 * psy_out[i] -> the RAW value of svt_psy_distortion / svt_psy_distortion_hbd (psy_rd.c:135-166, :241-271), before the psy_rd factor; the reference's precondition
 *               holds: width and height multiples of 4, of 8 when both are >= 8 (8x8 sub-blocks then, 4x4 otherwise). */
void svt_hip_pixel_dist_batch(const void *input_base, const void *recon_base, const SvtHipDistDesc *descs, uint32_t n, int is16, int what,
                              uint64_t *sse_out, uint64_t *psy_out, void *stream);
typedef struct SvtHipCoeffDistDesc {
    uint64_t coeff_off, recon_off;       /* int32 elements from coeff_base / recon_coeff_base */
    uint32_t coeff_stride, recon_stride;
    uint16_t width, height;
    uint8_t  cbf_zero;                   /* 1: svt_full_distortion_kernel_cbf_zero32_bits -- recon_coeff is not read, both results are sum c^2 */
    uint8_t  pad[3];
} SvtHipCoeffDistDesc;
/* dist_out[i][0] = DIST_CALC_RESIDUAL = sum (coeff - recon_coeff)^2, dist_out[i][1] = DIST_CALC_PREDICTION = sum coeff^2, 64-bit
 * (svt_full_distortion_kernel32_bits_c / svt_full_distortion_kernel_cbf_zero32_bits_c, pic_operators.c:150-221). */
void svt_hip_coeff_dist_batch(const int32_t *coeff_base, const int32_t *recon_coeff_base, const SvtHipCoeffDistDesc *descs, uint32_t n,
                              uint64_t *dist_out /* [n][2] */, void *stream);
/* The round trip that returns what it cost: svt_hip_txfm_quant_roundtrip_batch, then svt_hip_coeff_dist_batch on (forward coefficients after the svt_handle_transform
 * repack, dequantised coefficients) over min(W,32) x min(H,32) at stride min(W,32) with cbf_zero where eob == 0, then svt_hip_pixel_dist_batch(src, pred) and
 * (src, recon) over W x H -- bit-identical to that composition.  The coefficient sums leave the round-trip kernel itself (dqcoeff may be NULL); the pixel terms are a
 * second launch on the same stream.  psy_* are raw (before the psy_rd factor). */
typedef struct SvtHipPlaneRef { uint64_t off; uint32_t stride, reserved; } SvtHipPlaneRef; /* pixels from src_base */
typedef struct SvtHipRdDist { uint64_t coeff_dist[2], sse_pred, sse_recon, psy_pred, psy_recon; } SvtHipRdDist;
void svt_hip_txfm_quant_roundtrip_dist_batch(const int16_t *residual_base, const void *pred_base, void *recon_base, const SvtHipRoundtripDesc *descs, uint32_t n,
                                             int tx_size, int bd, int quant_mode, const SvtHipQuantParams *qparams, const int16_t *iscan_tables,
                                             const uint8_t *qm_tables, const uint8_t *iqm_tables, int32_t *qcoeff, int32_t *dqcoeff, uint16_t *eob,
                                             const void *src_base, const SvtHipPlaneRef *src, SvtHipRdDist *out, void *stream);
/* single-call forms with the reference's prototypes: the four dispatch pointers of common_dsp_rtcd.h:160, :161, :167, :169 (exported, NOT installed by
 * svt_hip_setup_rtcd: INTEGRATION.md), svt_spatial_psy_distortion_kernel_c (common_dsp_rtcd.h:165; the psy term only when psy_rd > 0) and psy_rd.h:23-32
 * (svt_get_psy_full_dist_hip = get_svt_psy_full_dist: (uint64_t)(raw * psy_rd) in IEEE double on the host, psy_rd.c:292). */
uint64_t svt_spatial_full_distortion_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                                uint32_t recon_stride, uint32_t area_width, uint32_t area_height);
uint64_t svt_full_distortion_kernel16_bits_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                               uint32_t recon_stride, uint32_t area_width, uint32_t area_height);
void     svt_full_distortion_kernel32_bits_hip(int32_t *coeff, uint32_t coeff_stride, int32_t *recon_coeff, uint32_t recon_coeff_stride,
                                               uint64_t distortion_result[2], uint32_t area_width, uint32_t area_height);
void     svt_full_distortion_kernel_cbf_zero32_bits_hip(int32_t *coeff, uint32_t coeff_stride, uint64_t distortion_result[2], uint32_t area_width,
                                                        uint32_t area_height);
uint64_t svt_spatial_psy_distortion_kernel_hip(uint8_t *input, uint32_t input_offset, uint32_t input_stride, uint8_t *recon, int32_t recon_offset,
                                               uint32_t recon_stride, uint32_t area_width, uint32_t area_height, double psy_rd);
uint64_t svt_psy_distortion_hip(const uint8_t *input, uint32_t input_stride, const uint8_t *recon, uint32_t recon_stride, uint32_t width, uint32_t height);
uint64_t svt_psy_distortion_hbd_hip(const uint16_t *input, uint32_t input_stride, const uint16_t *recon, uint32_t recon_stride, uint32_t width,
                                    uint32_t height);
uint64_t svt_get_psy_full_dist_hip(const void *s, uint32_t so, uint32_t sp, const void *r, uint32_t ro, uint32_t rp, uint32_t w, uint32_t h, uint8_t is_hbd,
                                   double psy_rd);

/* ------------------------------------------- AV1 inter prediction: the convolve family and its compound forms (csrc/interpred.hip) --------- */
/* One launch, n blocks of mixed sizes: the prediction svt_aom_convolve[subpel_x != 0][subpel_y != 0][compound] / svt_aom_convolveHbd[...] (inter_prediction.c:1035-1063)
 * compute, bit for bit.  Descriptors sit at the level of those dispatch pointers: the MV clamp and the block geometry of svt_aom_inter_prediction are the caller's.
 *   filters    av1_get_interp_filter_params_with_block_size (inter_prediction.h:137-145): the x kernel follows w, the y kernel h; a dimension <= 4 swaps REGULAR and
 *              SHARP for sub_pel_filters_4 and SMOOTH for sub_pel_filters_4smooth.
 *   compound 0 the `_sr` function with get_conv_params_no_round(0, 0, 0, NULL, 0, 0, bd) (convolve.h:40-64): round_0 3, round_1 11 (5 and 9 at 12 bit).
 *   compound 1 what two calls of the `jnt_` functions leave in dst: reference 0 with do_average = 0 into a ConvBufType buffer, reference 1 with do_average = 1;
 *   compound 2 the same with use_jnt_comp_avg = 1 and the two offsets (what svt_av1_dist_wtd_comp_weight_assign returned); round_1 = COMPOUND_ROUND1_BITS.  The
 *              ConvBufType buffer never reaches memory.  The two references may have different phases (the case is chosen per reference).
 * The reference's narrowings are reproduced: int16_t intermediate rows, the 8-bit 2-D function's int16_t before the last rounding (inter_prediction.c:345), the
 * 16-bit unsigned ConvBufType of the compound paths, the 16-bit shift-and-offset of jnt_convolve_2d_copy (:650-651).
 * READABLE EXTENT: 3 samples left of and above, 4 right of and below every w x h source block, as the reference reads; the kernel never reads outside it (a reference
 * that is not filtered in a direction is not read beyond the block in that direction).
 * planes.base[] are device pointers (uint8_t samples at bit_depth 8, uint16_t at 10 and 12), passed by value; dst_base and descs are device pointers.
 * INVALID DESCRIPTORS (w or h not one of 2, 4, .. 128; a phase above 15; a filter above 3; compound above 2; a plane index >= 32 or without a base) never fault:
 *   status == NULL  the descriptors are checked BEFORE anything is launched -- they are device memory, so a small kernel reads them and the call waits for its
 *                   one word (one stream synchronisation per call) -- and the call returns -1 with dst untouched if any is invalid;
 *   status != NULL  (device, n bytes) no synchronisation: the kernel writes status[i] = 0 / 1 (valid / invalid), skips the invalid blocks and the call returns 0.
 * Returns 0, -1 (bit_depth not 8 / 10 / 12, a NULL dst_base or descs, an invalid descriptor with status == NULL) or SVT_HIP_E_DEVICE. */
typedef struct SvtHipInterPredPlanes { const void *base[32]; } SvtHipInterPredPlanes;
typedef struct SvtHipInterPredDesc {
    uint64_t src_off[2];     /* samples from planes.base[plane[k]]: where the reference's `src` argument points, i.e. the block origin with the full-pel part of
                                the (already clamped) MV applied; [1] is read only when compound != 0 */
    uint64_t dst_off;        /* samples from dst_base */
    uint32_t src_stride[2], dst_stride; /* samples */
    uint8_t  plane[2];
    uint8_t  w, h;           /* 2, 4, 8, .. 128, independently */
    uint8_t  subpel_x[2], subpel_y[2]; /* subpel_*_q4 & SUBPEL_MASK, 0 .. 15, per reference */
    uint8_t  filter_x, filter_y;       /* InterpFilter 0 .. 3: EIGHTTAP_REGULAR, EIGHTTAP_SMOOTH, MULTITAP_SHARP, BILINEAR */
    uint8_t  compound;       /* 0 single reference, 1 average, 2 distance-weighted */
    uint8_t  fwd_offset, bck_offset;   /* compound == 2 */
    uint8_t  pad[7];
} SvtHipInterPredDesc;
int svt_hip_inter_pred_batch(SvtHipInterPredPlanes planes, void *dst_base, const SvtHipInterPredDesc *descs, uint32_t n, int bit_depth, uint8_t *status,
                             void *stream);
/* single-call forms with the reference's prototypes: the sixteen dispatch pointers of common_dsp_rtcd.h:184-215 (exported, NOT installed by svt_hip_setup_rtcd:
 * INTEGRATION.md).  Host pointers; the eight taps are read from filter_ptr + 8 * (subpel & 15) of the caller's InterpFilterParams (taps must be 8, as in every
 * InterpFilterParams of AV1; any values) and conv_params->round_0 / round_1 are the caller's.  The jnt_ forms honour conv_params->dst, dst_stride, do_average,
 * use_jnt_comp_avg, fwd_offset, bck_offset as the C does: do_average == 0 writes the ConvBufType buffer and leaves dst untouched.  w, h as above (otherwise
 * nothing is written).  ACCEPTED RANGE, outside of which a form returns having written nothing: 0 <= round_0 <= 7, round_1 >= 0, round_0 + round_1 <= 14, and
 * round_1 <= 7 in the jnt_ forms (every value get_conv_params_no_round yields lies inside; the roundings are shift counts); bd 10 or 12 in the highbd forms.
 * SvtHipInterpFilterParams is InterpFilterParams (definitions.h:742-747). */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef InterpFilterParams SvtHipInterpFilterParams;
#else
typedef struct SvtHipInterpFilterParams {
    const int16_t *filter_ptr;
    uint16_t       taps, subpel_shifts;
    uint32_t       interp_filter; /* InterpFilter, an int-sized enum */
} SvtHipInterpFilterParams;
#endif
/* (the forms themselves are declared next to SvtHipConvolveParams, further down) */

/* ------------------------------------------- AV1 intra prediction: edge build, every mode, filter-intra, CfL (csrc/intrapred.hip) ---------- */
/* One launch, n blocks of mixed sizes: what build_intra_predictors (bit_depth 8, uint8_t samples) / build_intra_predictors_high (10 / 12, uint16_t)
 * (enc_intra_prediction.c:60, :241) leave in dst, bit for bit.  Descriptors sit at the level of that function's parameter list: the availability derivation
 * (svt_aom_intra_has_top_right and the like), get_filt_type and palette are the caller's.  Everything from the neighbour pointers to dst happens in the kernel: the
 * need_* flags with their overrides, the constant fill when the needed edge is absent (base +- 1 or the first neighbour), copy + replicate extension, the above-left
 * rule, filter_intra_edge_corner, both svt_av1_filter_intra_edge calls (strengths and n_px as written there), both upsamplings, then z1 / z2 / z3, V / H at 90 / 180,
 * the DC variant selected by [n_left_px > 0][n_top_px > 0], SMOOTH / SMOOTH_V / SMOOTH_H, PAETH or the recursive filter-intra.  The prepared edges never reach memory.
 * READABLE EXTENT: top is read only inside [-1, n_top_px + n_topright_px), [-1] only when n_top_px > 0 and n_left_px > 0, nothing when n_top_px == 0; left only at
 * i * left_stride for i in [0, n_left_px + n_bottomleft_px).
 * planes.base[] are device pointers, passed by value; dst_base and descs are device pointers; dst may be one of the planes (the blocks of a launch are independent).
 * INVALID DESCRIPTORS (a size outside the 19 of TX_SIZES_ALL; mode > 12; |angle_delta| > 3; filter_intra_mode > 5, or < 5 with w or h above 32; n_top_px > w,
 * n_left_px > h, n_topright_px > w or > 0 without n_top_px == w, n_bottomleft_px > h or > 0 without n_left_px == h; disable_edge_filter or filt_type above 1; a plane
 * index >= 32 or without a base) never fault: status == NULL / != NULL and the return value exactly as svt_hip_inter_pred_batch. */
typedef struct SvtHipIntraPredPlanes { const void *base[32]; } SvtHipIntraPredPlanes;
typedef struct SvtHipIntraPredDesc {
    uint64_t top_off;        /* samples from planes.base[top_plane]: where top_neigh_array points; the above-left corner is at [-1] */
    uint64_t left_off;       /* samples from planes.base[left_plane]: left neighbour i is at left_off + i * left_stride */
    uint64_t dst_off;        /* samples from dst_base */
    uint32_t left_stride;    /* 1 = the reference's neighbour array; a picture stride reads a column of a reconstructed plane in place */
    uint32_t dst_stride;
    uint8_t  top_plane, left_plane;
    uint8_t  w, h;           /* tx_size_wide / tx_size_high of one of the 19 TxSize values */
    uint8_t  mode;           /* PredictionMode 0 .. 12: DC_PRED .. PAETH_PRED */
    int8_t   angle_delta;    /* -3 .. 3; ignored for non-directional modes, as the C does */
    uint8_t  filter_intra_mode; /* FilterIntraMode 0 .. 4, or 5 = FILTER_INTRA_MODES = off */
    uint8_t  n_top_px, n_topright_px, n_left_px, n_bottomleft_px;
    uint8_t  disable_edge_filter;
    uint8_t  filt_type;      /* what get_filt_type(xd, plane) returns: 1 when the above or the left neighbour block is smooth */
    uint8_t  pad[3];
} SvtHipIntraPredDesc; /* 48 bytes */
int svt_hip_intra_pred_batch(SvtHipIntraPredPlanes planes, void *dst_base, const SvtHipIntraPredDesc *descs, uint32_t n, int bit_depth, uint8_t *status,
                             void *stream);
/* Chroma from luma, one wave per descriptor: svt_cfl_luma_subsampling_420_{lbd,hbd} of the 2w x 2h luma block at luma_off -> svt_subtract_average with
 * round_offset = (w * h) >> 1, num_pel_log2 = log2 w + log2 h -> svt_cfl_predict_{lbd,hbd} for one or two chroma targets that share the AC values (Cb and Cr).
 * The Q3 AC buffer never reaches memory.  w x h: the 14 sizes of the reference's CFL_SUB_AVG_FN table (4 .. 32 either way without 4x32 and 32x4).  The DC prediction
 * of target t is read at planes.base[pred_plane[t]] + pred_off[t]; dst_base + dst_off[t] may be that very location (the encoder predicts in place,
 * product_coding_loop.c:3906).  READABLE EXTENT: luma inside 2w x 2h, each DC prediction inside w x h.  Invalid descriptors (size, n_targets not 1 / 2, planes) are
 * handled like svt_hip_intra_pred_batch's. */
typedef struct SvtHipCflPredDesc {
    uint64_t luma_off;
    uint64_t pred_off[2], dst_off[2];
    uint32_t luma_stride, pred_stride[2], dst_stride[2];
    int16_t  alpha_q3[2];    /* signed, what cfl_idx_to_alpha returns */
    uint8_t  luma_plane, pred_plane[2];
    uint8_t  w, h;           /* the chroma block */
    uint8_t  n_targets;      /* 1 or 2 */
    uint8_t  pad[2];
} SvtHipCflPredDesc; /* 72 bytes */
int svt_hip_cfl_pred_batch(SvtHipIntraPredPlanes planes, void *dst_base, const SvtHipCflPredDesc *descs, uint32_t n, int bit_depth, uint8_t *status, void *stream);
/* single-call forms with the reference's prototypes (exported, NOT installed by svt_hip_setup_rtcd: INTEGRATION.md).  Host pointers; each copies exactly the
 * index range of above / left its C function can read: z1 above [0, (bw + bh - 1) << upsample_above]; z3 left [0, (bw + bh - 1) << upsample_left]; z2 above
 * [-(1 << upsample_above), (bw - 1) << upsample_above] and left [-(1 << upsample_left), (bh - 1) << upsample_left]; filter-intra above [-1, w - 1], left [0, h - 1].
 * ACCEPTED RANGE, outside of which a form returns having written nothing: bw x bh one of the 19 sizes; upsample flags 0 / 1, 1 only with bw + bh <= 16; dx, dy in
 * 1 .. 65535; bd 10 or 12 in the highbd forms; tx_size with w, h <= 32 and mode 0 .. 4 (filter-intra); width x height (chroma; luma / 2 for the subsampling forms)
 * in the CFL_SUB_AVG_FN table, bit_depth 8 .. 12.  SvtHipTxSize is TxSize (definitions.h:849-878), a packed one-byte enum. */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef TxSize SvtHipTxSize;
#else
typedef uint8_t SvtHipTxSize;
#endif
/* svt_av1_dr_prediction_z1 / z2 / z3 (common_dsp_rtcd.h:581-586) -> svt_av1_dr_prediction_z{1,2,3}_c (intra_prediction.c:314-413) */
void svt_av1_dr_prediction_z1_hip(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above, const uint8_t *left, int32_t upsample_above, int32_t dx,
                                  int32_t dy);
void svt_av1_dr_prediction_z2_hip(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above, const uint8_t *left, int32_t upsample_above,
                                  int32_t upsample_left, int32_t dx, int32_t dy);
void svt_av1_dr_prediction_z3_hip(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above, const uint8_t *left, int32_t upsample_left, int32_t dx,
                                  int32_t dy);
/* svt_av1_highbd_dr_prediction_z1 / z3 (common_dsp_rtcd.h:587-590), z2 (:101-102) -> the `_c` functions (intra_prediction.c:2303-2370, C_DEFAULT/intra_prediction_c.c:58) */
void svt_av1_highbd_dr_prediction_z1_hip(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t *above, const uint16_t *left, int32_t upsample_above,
                                         int32_t dx, int32_t dy, int32_t bd);
void svt_av1_highbd_dr_prediction_z2_hip(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t *above, const uint16_t *left, int32_t upsample_above,
                                         int32_t upsample_left, int32_t dx, int32_t dy, int32_t bd);
void svt_av1_highbd_dr_prediction_z3_hip(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint16_t *above, const uint16_t *left, int32_t upsample_left,
                                         int32_t dx, int32_t dy, int32_t bd);
/* svt_av1_filter_intra_predictor (common_dsp_rtcd.h:91-92) -> svt_av1_filter_intra_predictor_c (C_DEFAULT/filterintra_c.c:70) */
void svt_av1_filter_intra_predictor_hip(uint8_t *dst, ptrdiff_t stride, SvtHipTxSize tx_size, const uint8_t *above, const uint8_t *left, int32_t mode);
/* svt_cfl_predict_lbd / _hbd (common_dsp_rtcd.h:79-82) -> C_DEFAULT/cfl_c.c:25, :44; pred_buf_q3 in rows of CFL_BUF_LINE = 32; dst may be pred */
void svt_cfl_predict_lbd_hip(const int16_t *pred_buf_q3, uint8_t *pred, int32_t pred_stride, uint8_t *dst, int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth,
                             int32_t width, int32_t height);
void svt_cfl_predict_hbd_hip(const int16_t *pred_buf_q3, uint16_t *pred, int32_t pred_stride, uint16_t *dst, int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth,
                             int32_t width, int32_t height);
/* svt_cfl_luma_subsampling_420_lbd / _hbd (common_dsp_rtcd.h:83-89) -> intra_prediction.c:420, :435; width x height are LUMA samples */
void svt_cfl_luma_subsampling_420_lbd_hip(const uint8_t *input, int32_t input_stride, int16_t *output_q3, int32_t width, int32_t height);
void svt_cfl_luma_subsampling_420_hbd_hip(const uint16_t *input, int32_t input_stride, int16_t *output_q3, int32_t width, int32_t height);

/* ------------------------------------------- AV1 masked prediction: blends (inter-intra, OBMC, wedge), wedge search (csrc/maskpred.hip) ------ */
/* One launch, n blocks of mixed sizes: dst = AOM_BLEND_A64(mask, src0, src1) = ROUND_POWER_OF_TWO(m * src0 + (64 - m) * src1, 6), bit for bit what
 *   kind A64_MASK  svt_aom_blend_a64_mask_c / svt_aom_highbd_blend_a64_mask_c (blend_a64_mask.c:201, :248) compute, with subw, subh in {0, 1}: the 2 x 2 mask average is
 *                  ROUND_POWER_OF_TWO(sum of four, 2), the two 1-D averages are AOM_BLEND_AVG;
 *   kind HMASK     svt_aom_blend_a64_hmask_c (:323) / svt_aom_highbd_blend_a64_hmask_16bit_c (inter_prediction.c:2374): mask[column];
 *   kind VMASK     svt_aom_blend_a64_vmask_c (:302) / svt_aom_highbd_blend_a64_vmask_16bit_c: mask[row].
 * THE ORDER (mask, src0, src1) IS THE REFERENCE'S: the mask weighs src0.  For inter-intra pass the INTRA prediction as src0 and the INTER prediction as src1, exactly as
 * svt_aom_combine_interintra does (inter_prediction.c:2341-2372); for OBMC src0 is the block's own prediction and src1 the neighbour's (enc_inter_prediction.c:1461, :1508).
 * Mask source:
 *   EXPLICIT   mask_off, mask_stride into mask_base (device bytes; HMASK / VMASK read w / h bytes at mask_off);
 *   WEDGE      (A64_MASK only) the mask svt_aom_get_contiguous_soft_mask(wedge_index, wedge_sign, bsize) returns, stride block_size_wide[bsize]: a chroma block of a
 *              4:2:0 picture reads the luma-sized mask with subw = subh = 1.  bsize is one of the nine BlockSize values with wedge bits (8x8, 8x16, 16x8, 16x16,
 *              16x32, 32x16, 32x32, 8x32, 32x8); (w << subw, h << subh) must not exceed its dimensions.  The table is generated on the device by svt_hip_maskpred_prepare, or by the
 *              first call of this section on that device, which then waits for it once (one stream synchronisation, also with a status array: call
 *              svt_hip_maskpred_prepare first where that matters, e.g. before a stream capture);
 *   SMOOTH_II  (A64_MASK only, subw = subh = 0) the mask of build_smooth_interintra_mask(plane_bsize = bsize, mode = ii_mode 0 .. 3: II_DC_PRED, II_V_PRED, II_H_PRED,
 *              II_SMOOTH_PRED) (inter_prediction.c:2144), computed in the kernel; block_size_wide / high[bsize] must equal w, h;
 *   OBMC       (HMASK / VMASK only) svt_av1_get_obmc_mask(w) for HMASK, (h) for VMASK: lengths 1, 2, 4, 8, 16, 32.
 * dst may alias src0 or src1 at the same position and stride (the reference's IMPLIES assertion): a lane reads the samples it writes before it writes them, every sample
 * is written exactly once.  OBMC blends in place.
 * READABLE EXTENT, exactly what the C reads: w x h of each source; (w << subw) x (h << subh) of a 2-D mask; w (HMASK) or h (VMASK) bytes of a 1-D mask.
 * planes.base[] are device pointers (uint8_t samples at bit_depth 8, uint16_t at 10 and 12), passed by value; dst_base, mask_base and descs are device pointers.
 * INVALID DESCRIPTORS (w or h not one of 1, 2, 4 .. 128; kind > 2; mask_src > 3; subw or subh > 1; a plane index >= 32 or without a base; EXPLICIT without mask_base;
 * WEDGE with another kind, a bsize that is not one of the nine, wedge_index > 15, wedge_sign > 1 or a block larger than the mask; SMOOTH_II with another kind, a
 * sub-sampling, ii_mode > 3 or a bsize whose dimensions are not w x h; OBMC with kind A64_MASK or a length above 32) never fault: status == NULL / != NULL and the return
 * value exactly as svt_hip_inter_pred_batch. */
#define SVT_HIP_BLEND_A64_MASK 0
#define SVT_HIP_BLEND_HMASK    1
#define SVT_HIP_BLEND_VMASK    2
#define SVT_HIP_MASK_EXPLICIT  0
#define SVT_HIP_MASK_WEDGE     1
#define SVT_HIP_MASK_SMOOTH_II 2
#define SVT_HIP_MASK_OBMC      3
typedef struct SvtHipBlendPlanes { const void *base[32]; } SvtHipBlendPlanes;
typedef struct SvtHipBlendDesc {
    uint64_t src_off[2];     /* samples from planes.base[plane[k]] */
    uint64_t dst_off;        /* samples from dst_base */
    uint64_t mask_off;       /* EXPLICIT: bytes from mask_base */
    uint32_t src_stride[2], dst_stride; /* samples */
    uint32_t mask_stride;    /* EXPLICIT, A64_MASK: bytes */
    uint8_t  plane[2];
    uint8_t  w, h;           /* 1, 2, 4 .. 128, independently */
    uint8_t  kind;           /* SVT_HIP_BLEND_* */
    uint8_t  mask_src;       /* SVT_HIP_MASK_* */
    uint8_t  subw, subh;     /* A64_MASK: 0 / 1 */
    uint8_t  bsize;          /* WEDGE: the BlockSize of the mask; SMOOTH_II: plane_bsize */
    uint8_t  wedge_index, wedge_sign; /* WEDGE */
    uint8_t  ii_mode;        /* SMOOTH_II: InterIntraMode 0 .. 3 */
    uint8_t  pad[4];
} SvtHipBlendDesc;
int svt_hip_blend_batch(SvtHipBlendPlanes planes, void *dst_base, const uint8_t *mask_base, const SvtHipBlendDesc *descs, uint32_t n, int bit_depth, uint8_t *status,
                        void *stream);
/* Generates the calling thread's device's wedge table now (one launch on `stream` and one synchronisation of it), so that no later call of this section does: a
 * device-resident caller calls it once per device while it initialises, outside any stream capture.  Returns 0 or SVT_HIP_E_DEVICE. */
int svt_hip_maskpred_prepare(void *stream);
/* The masked compound, n blocks of mixed sizes in one launch: what svt_aom_build_masked_compound_no_round (inter_prediction.c:2227) leaves in dst after the two
 * references were filtered into ConvBufType buffers with the compound roundings of get_conv_params_no_round -- here by the kernel of svt_hip_inter_pred_batch, the first
 * reference's values staying in registers while the second is filtered.  `p` is a descriptor of svt_hip_inter_pred_batch (both references always used; compound,
 * fwd_offset, bck_offset ignored; w, h 4 .. 128, the d16 functions' own lower bound).  The combine step is svt_aom_lowbd_blend_a64_d16_mask_c /
 * svt_aom_highbd_blend_a64_d16_mask_c (blend_a64_mask.c:34, :105) literally: ((m * a + (64 - m) * b) >> 6) - round_offset, ROUND_POWER_OF_TWO(., round_bits), clipped
 * to the bit depth; the mask per sample with the four (subw, subh) branches of those functions.
 *   comp_type WEDGE     svt_aom_get_contiguous_soft_mask(wedge_index, wedge_sign, bsize), stride block_size_wide[bsize]; (w << subw, h << subh) within the mask;
 *   comp_type DIFFWTD   (subw = subh = 0) svt_av1_build_compound_diffwtd_mask_d16_c (C_DEFAULT/inter_prediction_c.c:15) on the two register-held values:
 *                       clamp(38 + ROUND_POWER_OF_TWO(|a - b|, 2 * FILTER_BITS - round_0 - round_1 + bd - 8) / 16, 0, 64), 64 minus that for mask_type 1
 *                       (DIFFWTD_38_INV); stored at seg_mask_base + seg_off with stride w, one byte per sample, when seg_mask_base != NULL;
 *   comp_type EXPLICIT  mask_off, mask_stride into mask_base: how the chroma blocks consume the luma block's seg mask (mask_stride = the luma w, subw / subh = the
 *                       plane's sub-sampling).
 * READABLE EXTENT of the references as svt_hip_inter_pred_batch; (w << subw) x (h << subh) of an EXPLICIT mask.  INVALID DESCRIPTORS (those of
 * svt_hip_inter_pred_batch; w or h below 4; comp_type > 2; subw or subh > 1; WEDGE with a bsize that is not one of the nine, wedge_index > 15, wedge_sign > 1 or a
 * block larger than the mask; DIFFWTD with mask_type > 1 or a sub-sampling; EXPLICIT without mask_base): status / return value as svt_hip_inter_pred_batch. */
#define SVT_HIP_COMP_WEDGE    0
#define SVT_HIP_COMP_DIFFWTD  1
#define SVT_HIP_COMP_EXPLICIT 2
typedef struct SvtHipInterPredMaskedDesc {
    SvtHipInterPredDesc p;
    uint64_t mask_off;       /* EXPLICIT: bytes from mask_base */
    uint64_t seg_off;        /* DIFFWTD: bytes from seg_mask_base */
    uint32_t mask_stride;    /* EXPLICIT */
    uint8_t  comp_type;      /* SVT_HIP_COMP_* */
    uint8_t  bsize, wedge_index, wedge_sign; /* WEDGE */
    uint8_t  mask_type;      /* DIFFWTD: 0 DIFFWTD_38, 1 DIFFWTD_38_INV */
    uint8_t  subw, subh;
    uint8_t  pad[5];
} SvtHipInterPredMaskedDesc;
int svt_hip_inter_pred_masked_batch(SvtHipInterPredPlanes planes, void *dst_base, const uint8_t *mask_base, uint8_t *seg_mask_base,
                                    const SvtHipInterPredMaskedDesc *descs, uint32_t n, int bit_depth, uint8_t *status, void *stream);
/* The wedge / diff-weighted search of n luma blocks: what pick_wedge (fixed_sign 0), pick_wedge_fixed_sign (fixed_sign 1 / 2 = sign 0 / 1) and pick_interinter_seg
 * (enc_inter_prediction.c:383, :449, :498) compute with use_rate == 0, from the source block and the two predictions as pixel planes.  Per block:
 *   residual0 = src - p0, residual1 = src - p1, diff10 = p1 - p0 (int16_t); sign_limit = (sum r0^2 - sum r1^2) * 32 in 64 bits;
 *   ds = clamp(r0^2 - r1^2, INT16_MIN, INT16_MAX) (svt_av1_wedge_compute_delta_squares_c: the saturation is part of the result);
 *   sign[k] = sum ds * mask(k, 0) > sign_limit (svt_av1_wedge_sign_from_residuals_c, a 64-bit sum), or the fixed sign;
 *   sse[k] = ROUND_POWER_OF_TWO(sum clamp(64 * r1 + mask(k, sign[k]) * d10, INT16_MIN, INT16_MAX)^2, 12) (svt_av1_wedge_sse_from_residuals_c: the clamp binds at 10 and
 *   12 bit), a 64-bit sum; sse_diffwtd[t] the same with the DIFFWTD_38 / DIFFWTD_38_INV mask of svt_av1_build_compound_diffwtd_mask_c (bit_depth 8) or _highbd_c with
 *   its >> (bit_depth - 8) on |p0 - p1| (pick_interinter_seg itself passes EB_TEN_BIT; here the depth is the call's);
 *   best_wedge_index / best_wedge_sign and best_mask_type by the reference's strict <: the first minimum wins.
 * With the sixteen sse and sign values a caller can apply the rate model of use_rate == 1 on the host.  bsize is one of the nine wedge sizes.
 * READABLE EXTENT: block_size_wide x block_size_high[bsize] samples of src, p0 and p1.  INVALID DESCRIPTORS (bsize not one of the nine, fixed_sign > 2, a plane index
 * >= 32 or without a base): status / return value as svt_hip_inter_pred_batch; the result of an invalid descriptor is not written. */
typedef struct SvtHipWedgeSearchDesc {
    uint64_t src_off, p0_off, p1_off;          /* samples from planes.base[*_plane] */
    uint32_t src_stride, p0_stride, p1_stride; /* samples */
    uint8_t  src_plane, p0_plane, p1_plane;
    uint8_t  bsize;
    uint8_t  fixed_sign;     /* 0: the sign is chosen per wedge index; 1: sign 0 for all; 2: sign 1 for all */
    uint8_t  pad[7];
} SvtHipWedgeSearchDesc;
typedef struct SvtHipWedgeSearchResult {
    uint64_t sse[16];
    uint64_t sse_diffwtd[2];
    uint8_t  sign[16];
    uint8_t  best_wedge_index, best_wedge_sign, best_mask_type;
    uint8_t  pad[5];
} SvtHipWedgeSearchResult;
int svt_hip_wedge_search_batch(SvtHipBlendPlanes planes, const SvtHipWedgeSearchDesc *descs, uint32_t n, int bit_depth, SvtHipWedgeSearchResult *out, uint8_t *status,
                               void *stream);
/* single-call forms with the reference's prototypes: the six pixel-domain blend pointers of common_dsp_rtcd.h:67-78 (exported, NOT installed by svt_hip_setup_rtcd: INTEGRATION.md).
 * Host pointers; w, h powers of two 1 .. 128 and subx, suby 0 / 1, otherwise nothing is written; dst may be src0 or src1.  The highbd a64_mask form takes its uint16_t
 * samples through uint8_t pointers, as the reference's does (a plain cast, no CONVERT_TO_SHORTPTR shift: blend_a64_mask.c:252-254). */
void svt_aom_blend_a64_mask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride,
                                const uint8_t *mask, uint32_t mask_stride, int w, int h, int subx, int suby);
void svt_aom_highbd_blend_a64_mask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride,
                                       const uint8_t *mask, uint32_t mask_stride, int w, int h, int subx, int suby, int bd);
void svt_aom_blend_a64_hmask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride,
                                 const uint8_t *mask, int w, int h);
void svt_aom_blend_a64_vmask_hip(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride,
                                 const uint8_t *mask, int w, int h);
void svt_aom_highbd_blend_a64_hmask_16bit_hip(uint16_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride, const uint16_t *src1,
                                              uint32_t src1_stride, const uint8_t *mask, int w, int h, int bd);
void svt_aom_highbd_blend_a64_vmask_16bit_hip(uint16_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride, const uint16_t *src1,
                                              uint32_t src1_stride, const uint8_t *mask, int w, int h, int bd);
/* the two pixel-domain diff-weighted mask builders (common_dsp_rtcd.h:224-227 -> inter_prediction.c:130, :144; mask_type is DIFFWTD_MASK_TYPE, a one-byte enum:
 * DIFFWTD_38 0, DIFFWTD_38_INV 1; the highbd form takes uint16_t samples through uint8_t pointers and shifts |src0 - src1| by bd - 8) and the four helpers of the
 * wedge search (common_dsp_rtcd.h:228-229, :1009-1010, aom_dsp_rtcd.h:57-60 -> inter_prediction.c:2330, :2396, enc_inter_prediction.c:338, :375).  Host pointers,
 * contiguous arrays as in the C.  ACCEPTED RANGE, outside of which nothing is written and the value forms return 0: w, h 1 .. 128, strides >= w, mask_type 0 / 1,
 * bd 8 / 10 / 12; 1 <= N <= 2^20.  d may be a or b in svt_av1_wedge_compute_delta_squares_hip. */
void     svt_av1_build_compound_diffwtd_mask_hip(uint8_t *mask, uint8_t mask_type, const uint8_t *src0, int src0_stride, const uint8_t *src1, int src1_stride, int h,
                                                 int w);
void     svt_av1_build_compound_diffwtd_mask_highbd_hip(uint8_t *mask, uint8_t mask_type, const uint8_t *src0, int src0_stride, const uint8_t *src1, int src1_stride,
                                                        int h, int w, int bd);
uint64_t svt_av1_wedge_sse_from_residuals_hip(const int16_t *r1, const int16_t *d, const uint8_t *m, int N);
int8_t   svt_av1_wedge_sign_from_residuals_hip(const int16_t *ds, const uint8_t *m, int N, int64_t limit);
void     svt_av1_wedge_compute_delta_squares_hip(int16_t *d, const int16_t *a, const int16_t *b, int N);
uint64_t svt_aom_sum_squares_i16_hip(const int16_t *src, uint32_t N);

/* ------------------------------------------- AV1 warped motion: block warp filter, local model fit, warp error (csrc/warp.hip) ------------- */
/* One launch, n blocks of mixed sizes: what svt_av1_warp_affine_c (bit_depth 8, uint8_t samples) / svt_av1_highbd_warp_affine_c (10 / 12, uint16_t samples)
 * (warped_motion.c:569, :714) leave in dst, bit for bit, with the ConvolveParams plane_warped_motion_prediction builds (enc_inter_prediction.c:2040):
 * get_conv_params_no_round(0, 0, 0, tmp, 128, is_compound, bd), i.e. round_0 3 (5 at 12 bit), round_1 7 when compound.  Descriptors sit at the level of the dispatch
 * pointer: the ROTZOOM fix-up of svt_warp_plane, svt_get_shear_params (or svt_hip_warp_model_batch below) and the block geometry are the caller's.
 *   compound 0 one call, not compound;
 *   compound 1 what two calls leave in dst: reference 0 with do_average = 0 into a ConvBufType buffer, reference 1 with do_average = 1;
 *   compound 2 the same with use_jnt_comp_avg = 1 and the two offsets.  The ConvBufType values never reach memory; the two references have independent models,
 *              planes and bounds.
 * The reference's arithmetic is reproduced as written: dst_x / dst_y in int32_t, x4 = dst_x >> subsampling_x, the WARP_PARAM_REDUCE_BITS masking of sx4 / sy4, the
 * high-bit-depth reduce_bits_horiz = round_0 + max(bd + FILTER_BITS - round_0 - 14, 0), the 16-bit unsigned ConvBufType, the cropping of the last 8x8 tile.
 * READABLE EXTENT: exactly width x height samples at ref_off, rows `stride` apart.  Every coordinate is clamped to [0, width) x [0, height) before the address is
 * formed, however far outside the model projects: nothing is read at a negative offset or beyond row height - 1 / column width - 1.
 * planes.base[] are device pointers (uint8_t samples at bit_depth 8, uint16_t at 10 and 12; the reference's split 8-bit + 2-bit planes are handled by the single-call
 * form only), passed by value; dst_base and descs are device pointers.
 * INVALID DESCRIPTORS never fault; status == NULL / != NULL and the return value exactly as svt_hip_inter_pred_batch.  A descriptor is invalid when p_width or
 * p_height is outside 1 .. 128, a sub-sampling is above 1, compound is above 2; width, height or stride of a used reference is below 1; its plane index is >= 32 or
 * the plane has no base; 4 |alpha| + 7 |beta| >= 65536 or 4 |gamma| + 4 |delta| >= 65536 (is_affine_shear_allowed: what keeps the filter index inside 0 .. 192);
 * src_x, src_y, dst_x or dst_y of any of its tiles does not fit int32_t when computed in 64 bits (the C computes them in int32_t). */
typedef struct SvtHipWarpRef {
    uint64_t ref_off;        /* samples from planes.base[plane]: where the C's `ref` points, i.e. sample (0, 0) of the picture proper */
    int32_t  mat[6];         /* as svt_av1_warp_affine receives them */
    int16_t  alpha, beta, gamma, delta;
    int32_t  width, height, stride; /* the clamp bounds and the row pitch, samples */
    uint8_t  plane;
    uint8_t  pad[3];
} SvtHipWarpRef;
typedef struct SvtHipWarpDesc {
    SvtHipWarpRef ref[2];    /* [1] is read only when compound != 0 */
    uint64_t dst_off;        /* samples from dst_base: the block's first sample */
    uint32_t dst_stride;
    int32_t  p_col, p_row;
    uint8_t  p_width, p_height; /* 1 .. 128, any value */
    uint8_t  subsampling_x, subsampling_y;
    uint8_t  compound;       /* 0 / 1 / 2 as SvtHipInterPredDesc.compound */
    uint8_t  fwd_offset, bck_offset; /* compound == 2 */
    uint8_t  pad[5];
} SvtHipWarpDesc;
int svt_hip_warp_pred_batch(SvtHipInterPredPlanes planes, void *dst_base, const SvtHipWarpDesc *descs, uint32_t n, int bit_depth, uint8_t *status, void *stream);
/* The local-warp model of n blocks: out[i] is what svt_find_projection(np, pts, pts_inref, bsize, mv_row, mv_col, &wm, mi_row, mi_col) (warped_motion.c:472) leaves
 * in wm.wmmat[0 .. 5], wm.alpha .. wm.delta, and its return value in `invalid` -- find_affine_int followed by svt_get_shear_params, in plain integer arithmetic: the
 * LS_* sums in int32_t, the 64-bit determinant, resolve_divisor_64 / _32 with the generated table (entry n = round(2^22 / (256 + n))), the 64-bit get_mult_shift_*
 * pair (USE_LIMITED_PREC_MULT 0), the clamps, the int16_t narrowing of i_det and of its left shift, the WARP_PARAM_REDUCE_BITS rounding.  When the C returns 1,
 * invalid = 1 and every other field is 0.  svt_aom_select_samples and the neighbour scan are the caller's.  descs, out, status are device pointers; out[i] feeds a
 * SvtHipWarpRef without a host round trip.  INVALID DESCRIPTORS (np outside 1 .. 8, bsize >= 22): status / return value as svt_hip_inter_pred_batch; the result of
 * an invalid descriptor is not written. */
typedef struct SvtHipWarpModelDesc {
    int32_t pts[16], pts_inref[16]; /* x, y pairs, 1/8 sample, relative to the block's origin as svt_find_projection takes them */
    int32_t np;              /* 1 .. 8 */
    int32_t mi_row, mi_col;
    int16_t mv_row, mv_col;  /* the C's mvy, mvx */
    uint8_t bsize;           /* BlockSize */
    uint8_t pad[3];
} SvtHipWarpModelDesc;
typedef struct SvtHipWarpModel {
    int32_t wmmat[6];
    int16_t alpha, beta, gamma, delta;
    uint8_t invalid;         /* svt_find_projection's return value */
    uint8_t pad[3];
} SvtHipWarpModel;
int svt_hip_warp_model_batch(const SvtHipWarpModelDesc *descs, uint32_t n, SvtHipWarpModel *out, uint8_t *status, void *stream);
/* The warp error of n candidate models over a picture, 8 bit (as global motion runs): out[i] is what warp_error (enc_warped_motion.c:22) returns with
 * best_error = INT64_MAX -- the SAD between the source and the warp (get_conv_params(0, 0, 0, 8), not compound) over the 32 x 32 error blocks: all of them for
 * chess_refn == 0, the checkerboard half (jstart alternating by block row as written there), times two, for chess_refn == 1.  The warped samples never reach memory.
 * The C's EARLY EXIT returns a partial sum and is not reproduced: partial sums are monotone, so the C leaves early iff the full, undoubled sum exceeds best_error --
 * comparing out[i] (halved when chess_refn == 1) against best_error gives the same decision.  svt_av1_warp_error's own call of svt_get_shear_params is the caller's:
 * `ref` carries alpha .. delta.  src_off points at sample (0, 0) of the source picture: sample (x, y) of the block is read at src_off + y * src_stride + x with
 * x from p_col, y from p_row.  The sums are exact integers added with 64-bit atomics into out, which the entry zeroes first: the result does not depend on the order.
 * INVALID DESCRIPTORS (those of the reference in svt_hip_warp_pred_batch; p_width or p_height outside 1 .. 65536; a sub-sampling or chess_refn above 1; src_stride
 * below 1; src_plane >= 32 or without a base): status / return value as svt_hip_inter_pred_batch, out[i] of an invalid descriptor is 0.  n <= 65535. */
typedef struct SvtHipWarpErrorDesc {
    SvtHipWarpRef ref;
    uint64_t src_off;        /* samples from planes.base[src_plane] */
    uint32_t src_stride;
    int32_t  p_col, p_row, p_width, p_height;
    uint8_t  src_plane;
    uint8_t  subsampling_x, subsampling_y, chess_refn;
} SvtHipWarpErrorDesc;
int svt_hip_warp_error_batch(SvtHipInterPredPlanes planes, const SvtHipWarpErrorDesc *descs, uint32_t n, uint64_t *out, uint8_t *status, void *stream);
/* (the two single-call forms are declared next to SvtHipConvolveParams, further down) */

/* ------------------------------------------- pictures of another size: scaled prediction, resize, super-res upscale (csrc/scale.hip) ------- */
/* A. One launch, n blocks of mixed sizes predicted from references of another size: what svt_av1_convolve_2d_scale / svt_av1_highbd_convolve_2d_scale
 * (common_dsp_rtcd.h: svt_av1_convolve_2d_scale, svt_av1_highbd_convolve_2d_scale -> inter_prediction.c:420, :779) compute, bit for bit.  Descriptors follow
 * SvtHipInterPredDesc; the position arithmetic (svt_av1_setup_scale_factors_for_frame, scaled_x / scaled_y, the clamp of compute_subpel_params,
 * enc_inter_prediction.c:3158-3197) is the caller's, as the MV clamp is there.  Per reference k:
 *   scaled     xs[k] != 1024 || ys[k] != 1024: svt_av1_[highbd_]convolve_2d_scale_c -- both directions are always filtered (a direction whose step is 1024 too),
 *              round_0 / round_1 of get_conv_params_no_round, the int16_t intermediate, the 16-bit ConvBufType result (compound or not), the filter following w and h
 *              through av1_get_interp_filter_params_with_block_size.
 *   unscaled   xs[k] == ys[k] == 1024: the unscaled case of svt_hip_inter_pred_batch with phase subpel >> 6 (the reference calls svt_aom_convolve[..] for it,
 *              inter_prediction.c:1312-1380); a remainder in the low 6 bits makes the descriptor invalid.  A descriptor whose references are all unscaled is valid
 *              and equals svt_hip_inter_pred_batch: the caller need not split its list.
 *   compound   0 / 1 / 2 and the two offsets as in svt_hip_inter_pred_batch; the ConvBufType buffer never reaches memory.
 * READABLE EXTENT of a scaled reference, around where src_off points: columns -3 .. (((w - 1) * xs + subpel_x) >> 10) + 4, rows -3 .. (((h - 1) * ys + subpel_y)
 * >> 10) + 4; of an unscaled one: as svt_hip_inter_pred_batch.  The kernel reads nothing outside.
 * INVALID DESCRIPTORS (w or h not one of 2, 4, .. 128; a phase above 1023; a step outside 64 .. 2048, the range valid_ref_frame_size allows; an unscaled reference
 * with a low-6-bit remainder; (((h - 1) * ys + subpel_y) >> 10) + 8 > 2 * 128 + 8, the C's im_block bound, or the same in x; a filter above 3; compound above 2; a
 * plane index >= 32 or without a base) never fault: status == NULL / != NULL and the return value exactly as svt_hip_inter_pred_batch. */
typedef struct SvtHipScaledPredDesc {
    uint64_t src_off[2];     /* samples from planes.base[plane[k]]: where the C's `src` argument points, the clamped position >> SCALE_SUBPEL_BITS */
    uint64_t dst_off;        /* samples from dst_base */
    uint32_t src_stride[2], dst_stride; /* samples */
    uint16_t subpel_x[2], subpel_y[2];  /* SubpelParams after & SCALE_SUBPEL_MASK, 0 .. 1023, per reference */
    uint16_t xs[2], ys[2];   /* x_step_q4 / y_step_q4, 64 .. 2048; 1024 = not scaled in that direction */
    uint8_t  plane[2];
    uint8_t  w, h;           /* 2, 4, 8, .. 128, independently */
    uint8_t  filter_x, filter_y; /* InterpFilter 0 .. 3 */
    uint8_t  compound;       /* 0 single reference, 1 average, 2 distance-weighted */
    uint8_t  fwd_offset, bck_offset; /* compound == 2 */
    uint8_t  pad[3];
} SvtHipScaledPredDesc; /* 64 bytes */
int svt_hip_inter_pred_scaled_batch(SvtHipInterPredPlanes planes, void *dst_base, const SvtHipScaledPredDesc *descs, uint32_t n, int bit_depth, uint8_t *status,
                                    void *stream);
/* (the two single-call forms are declared next to SvtHipConvolveParams, further down) */

/* B. The non-normative picture resize, n planes per call: what svt_av1_resize_plane / svt_av1_highbd_resize_plane (aom_dsp_rtcd.h:900-903 -> resize.c:400, :680)
 * leave in dst, bit for bit -- resize_multistep whole (get_down2_steps, the even and odd half-band filters, the final interpolate with choose_interp_filter, the copy
 * when lengths are equal), rows first into a width2 x height intermediate, then columns; height2 == height is svt_av1_[highbd_]resize_plane_horizontal.  Any number of
 * factor-of-two steps and out > in are accepted, as the C accepts them.  src / dst are device pointers (uint8_t samples at bit_depth 8, uint16_t at 10 / 12), descs
 * is HOST memory.  The intermediate and what a factor-of-two step leaves live in `workspace` (device, svt_hip_resize_workspace_bytes(descs, n, bit_depth) bytes, 256-byte
 * aligned); the launches are queued on `stream` and the call does not wait.  Reads stay inside width x height of src, writes inside width2 x height2 of dst.
 * Returns 0, -1 (bit_depth; a NULL pointer; a dimension < 1 or above 65535; a stride below its width; a workspace that is NULL or too small -- nothing is launched or
 * written then) or SVT_HIP_E_DEVICE.  svt_hip_resize_workspace_bytes returns 0 for arguments the batch would reject. */
typedef struct SvtHipResizeDesc {
    const void *src;
    void       *dst;
    int32_t     width, height, in_stride;    /* samples */
    int32_t     width2, height2, out_stride;
} SvtHipResizeDesc; /* 40 bytes */
size_t svt_hip_resize_workspace_bytes(const SvtHipResizeDesc *descs, uint32_t n, int bit_depth);
int    svt_hip_resize_plane_batch(const SvtHipResizeDesc *descs /* host */, uint32_t n, int bit_depth, void *workspace, size_t workspace_bytes, void *stream);
/* single-call forms with the reference's prototypes: the two dispatch pointers of aom_dsp_rtcd.h:900, :902 (exported, NOT installed by svt_hip_setup_rtcd:
 * INTEGRATION.md).  Host pointers; upload, the launches above, download.  ACCEPTED RANGE, outside of which EB_ErrorBadParameter is returned and nothing is written:
 * the conditions of the batched entry; bd 8, 10 or 12 in the highbd form.  EB_ErrorInsufficientResources stands for a device failure.  The four 1-D pointers
 * (svt_av1_interpolate_core, svt_av1_down2_symeven and their highbd forms) exist inside the kernels only: one row per host round trip would be all latency. */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef EbErrorType SvtHipErrorType;
#else
typedef int32_t SvtHipErrorType; /* EbErrorType (EbSvtAv1.h:121): an int-sized enum with negative members */
#endif
SvtHipErrorType svt_av1_resize_plane_hip(const uint8_t *const input, int height, int width, int in_stride, uint8_t *output, int height2, int width2, int out_stride);
SvtHipErrorType svt_av1_highbd_resize_plane_hip(const uint16_t *const input, int height, int width, int in_stride, uint16_t *output, int height2, int width2,
                                                int out_stride, int bd);

/* C. The normative super-resolution upscale, the planes of a picture per call (three per launch): what svt_av1_upscale_normative_rows (super_res.c:214) leaves in
 * dst, bit for bit -- x_step_qn and x0_qn as super_res.c:43-52, the x0_qn carry from tile column to tile column (:282), the last tile column ending at
 * upscaled_plane_width, Upscale_Filter of the AV1 specification.  Frame-edge tile columns replicate their edge sample: the C overwrites and restores five border
 * columns of the SOURCE, the kernel clamps the read to [first tile column's first sample, last tile column's last sample] instead and never writes src; interior
 * tile-column edges read the real neighbours.  READABLE EXTENT: columns 0 .. (tile_col_start_mi[n_tile_cols] << (2 - sub_x)) - 1 of each of the `rows` rows.
 * src / dst are device pointers and must not overlap; descs is HOST memory; the launches are queued on `stream` and the call does not wait.
 * Returns 0, -1 (a NULL pointer; rows or a width < 1 or above 65535; upscaled below downscaled width; a stride below its width or src_stride not above the last
 * source sample; superres_denom outside 8 .. 16; sub_x above 1; n_tile_cols outside 1 .. 64 or starts that do not rise from 0; bd not 8 / 10 / 12; sample_bytes
 * not 1 / 2, or 1 with bd above 8; overlapping src and dst -- nothing is launched then) or SVT_HIP_E_DEVICE. */
typedef struct SvtHipUpscaleDesc {
    const void *src;
    void       *dst;
    int32_t     src_stride, dst_stride, rows; /* samples */
    int32_t     downscaled_plane_width, upscaled_plane_width; /* already ROUND_POWER_OF_TWO(frame_width / superres_upscaled_width, sub_x) */
    uint8_t     superres_denom, sub_x;
    uint8_t     bd;           /* 8 / 10 / 12: the clip */
    uint8_t     sample_bytes; /* 1, or 2; bd == 8 with 2-byte samples is the 16-bit pipeline and clips to 255 */
    int32_t     n_tile_cols;
    int32_t     tile_col_start_mi[65]; /* what svt_av1_tile_set_col yields: mi_col_start of every tile column, then mi_col_end of the last (= mi_cols) */
} SvtHipUpscaleDesc; /* 304 bytes */
int svt_hip_superres_upscale_batch(const SvtHipUpscaleDesc *descs /* host */, uint32_t n, void *stream);
/* The same for one plane in HOST memory, the descriptor's members flattened.  svt_av1_upscale_normative_rows takes an Av1Common * and has no dispatch pointer, so
 * there is no reference prototype to mirror: this form's argument list is the library's own.  src_stride / dst_stride in samples. */
int svt_hip_upscale_normative_rows_host(const void *src, int src_stride, void *dst, int dst_stride, int rows, int downscaled_plane_width, int upscaled_plane_width,
                                        int superres_denom, int sub_x, int n_tile_cols, const int32_t *tile_col_start_mi, int bd, int sample_bytes);

/* ------------------------------------------- AV1 luma palette: k-means, colour search, map cost, prediction (csrc/palette.hip) -------------- */
/* Everything below is bit-exact with the reference's C (palette.c, k_means_template.h, pic_analysis_process.c:1808-1845, cabac_context_model.c:2458,
 * enc_intra_prediction.c:501-508, :647-655).  Descriptors live in DEVICE memory, one launch per call, queued on `stream`; the call does not wait.
 * STATUS, all five batched entries: status != NULL -> status[i] = 0 (done), 1 (invalid descriptor: skipped, nothing of item i written) or 2 (a sample at or above
 * 1 << bit_depth, see B and C), the call returns 0.  status == NULL -> the descriptors are checked by a small kernel first and the call returns -1 with nothing
 * launched or written when one is invalid.  Other returns: -1 for a NULL base pointer or a bit depth the entry does not take, SVT_HIP_E_DEVICE.  n == 0 returns 0. */

/* A. svt_av1_k_means_dim1_c / _dim2_c complete for n items: the first assignment, then per iteration centroid sums and counts, DIVIDE_AND_ROUND, the reseed of every
 * empty cluster in ascending cluster order from one lcg_rand16 stream seeded with (unsigned)data[0], reassignment and the 64-bit total distance; the exit when the
 * centroids repeat and the exit at max_itr (max_itr <= 0: the first assignment only).  assign_only != 0 is svt_av1_calc_indices_dim1_c / _dim2_c: centroids are
 * read, never written.  Ties go to the lowest centroid index.  The `this_dist > pre_dist` exit is kept (centroids restored, indices reassigned from them, which is
 * what pre_indices held); DESIGN 4.26 shows that no input reaches it.  Data values 0 .. 32767 (the C's int arithmetic holds up to there); not checked.
 * INVALID: dim not 1 / 2, k outside 1 .. 8, n outside 1 .. 16384 (MAX_SB_SQUARE, the C's pre_indices). */
typedef struct SvtHipKmeansDesc {
    uint64_t data_off;      /* int32 elements from data_base: n * dim values */
    uint64_t centroids_off; /* int32 elements from centroids_base: k * dim values, in and out */
    uint64_t indices_off;   /* bytes from indices_base: n values out */
    int32_t  n;
    int32_t  max_itr;
    uint8_t  dim, k, assign_only;
    uint8_t  pad[5];
} SvtHipKmeansDesc; /* 40 bytes */
int svt_hip_kmeans_batch(const int32_t *data_base, int32_t *centroids_base, uint8_t *indices_base, const SvtHipKmeansDesc *descs, uint32_t n, uint8_t *status,
                         void *stream);

/* B. svt_av1_count_colors / svt_av1_count_colors_highbd for n blocks of one plane (uint8_t samples at bit_depth 8, uint16_t at 10 / 12): the full histogram
 * (256 or 1 << bit_depth int32 per block) and n_colors[i] = the number of non-zero bins.  A sample at or above 1 << bit_depth is a caller error: it is not counted
 * (nothing outside the histogram is read or written), n_colors[i] = 0 as the C returns, status[i] = 2.  INVALID: rows or cols 0. */
typedef struct SvtHipCountColorsDesc {
    uint64_t src_off;  /* samples from src_base */
    uint64_t hist_off; /* int32 elements from hist_base */
    uint32_t src_stride;
    uint16_t rows, cols;
} SvtHipCountColorsDesc; /* 24 bytes */
int svt_hip_count_colors_batch(const void *src_base, const SvtHipCountColorsDesc *descs, uint32_t n, int bit_depth, int32_t *hist_base, int32_t *n_colors,
                               uint8_t *status, void *stream);

/* C. search_palette_luma (palette.c:303) whole for n blocks of mixed sizes: the colour count (zero candidates unless 1 < colors <= 64), lb / ub, the min(colors, 8)
 * dominant colours, the dominant-colour loop (n from min(colors, 8) down to 2 in steps of dominant_color_step), the k-means loop (n down to 2, 50 iterations, the
 * colors == 2 case) and for each pass palette_rd_y: optimize_palette_colors, the sort with av1_remove_duplicates, the clip, the index map over rows x cols and
 * extend_palette_color_map to block_width x block_height.  A candidate is kept when its size is above 2, as in the C.  bit_depth 8: uint8_t samples; 10: uint16_t.
 * OUTPUT of a block, at out_off bytes from out_base: one SvtHipPaletteSearchOut, then 14 index maps map_stride bytes apart.  n_cand is always written; size[s],
 * colors[s][0 .. size - 1] and the first block_width * block_height bytes of map s only for s < n_cand -- nothing else.  A sample at or above 1 << bit_depth
 * (16-bit form): n_cand = 0, status 2.  READS rows x cols samples of the source, nothing outside.
 * INVALID: block_width / block_height not 8, 16, 32 or 64; rows outside 1 .. block_height; cols outside 1 .. block_width; n_cache above 16;
 * dominant_color_step 0; map_stride below block_width * block_height; an odd out_off. */
#define SVT_HIP_PALETTE_MAX_CANDS 14
typedef struct SvtHipPaletteSearchDesc {
    uint64_t src_off;    /* samples from src_base */
    uint64_t out_off;    /* bytes from out_base, even */
    uint32_t src_stride; /* samples */
    uint32_t map_stride; /* bytes from one candidate's map to the next */
    uint16_t cache[16];  /* what svt_get_palette_cache_y (svt_hip_palette_cache_y) makes */
    uint8_t  rows, cols; /* inside the picture */
    uint8_t  block_width, block_height;
    uint8_t  n_cache;
    uint8_t  dominant_color_step;
    uint8_t  pad[2];
} SvtHipPaletteSearchDesc; /* 64 bytes */
typedef struct SvtHipPaletteSearchOut {
    uint8_t  n_cand; /* 0 .. 14 */
    uint8_t  size[SVT_HIP_PALETTE_MAX_CANDS];
    uint8_t  pad;
    uint16_t colors[SVT_HIP_PALETTE_MAX_CANDS][8];
} SvtHipPaletteSearchOut; /* 240 bytes; the maps follow */
int svt_hip_palette_search_luma_batch(const void *src_base, const SvtHipPaletteSearchDesc *descs, uint32_t n, int bit_depth, void *out_base, uint8_t *status,
                                      void *stream);

/* D. The palette part of the luma mode rate for n (block, candidate) items, three int32 per item in out: map_bits = svt_av1_cost_color_map (every position but
 * (0, 0) of rows x cols read at pitch block_width, context and reordered index of svt_aom_get_palette_color_index_context_optimized, summed from color_cost =
 * palette_ycolor_fac_bitss[7][5][8], 280 int32 in device memory), color_bits = svt_av1_palette_color_cost_y (bit_depth is the encoder's), first_bits =
 * svt_aom_write_uniform_cost(size, map[0]).  map_off / colors_off may point into the output of C in place; rows x block_width bytes of the map are read.  Map entries must be below size (only their low three
 * bits are used).  INVALID: size outside 2 .. 8; block_width not 8 .. 64 a power of two; rows outside 1 .. 64; cols outside 1 .. block_width; n_cache above 16;
 * bit_depth not 8 / 10 / 12; an odd colors_off. */
typedef struct SvtHipPaletteCostDesc {
    uint64_t map_off;    /* bytes from base */
    uint64_t colors_off; /* bytes from base, even: `size` uint16_t */
    uint16_t cache[16];
    uint8_t  rows, cols, block_width, size, n_cache, bit_depth;
    uint8_t  pad[2];
} SvtHipPaletteCostDesc; /* 56 bytes */
int svt_hip_palette_cost_batch(const void *base, const SvtHipPaletteCostDesc *descs, uint32_t n, const int32_t *color_cost, int32_t *out, uint8_t *status,
                               void *stream);

/* E. Palette prediction of n transform blocks of mixed sizes: dst[r][c] = colors[map[(r + y) * wpx + c + x]], r < h, c < w.  dst16 == 0: uint8_t destination (the
 * colour truncated as the C's cast does); dst16 != 0: uint16_t destination, clamped to 0xFF when bit_depth is 8.  INVALID: w / h not 4, 8, 16, 32 or 64; wpx not 8,
 * 16, 32 or 64; x + w above wpx; y + h above 64; an odd colors_off. */
typedef struct SvtHipPalettePredDesc {
    uint64_t map_off;    /* bytes from base */
    uint64_t colors_off; /* bytes from base, even: 8 uint16_t are readable */
    uint64_t dst_off;    /* samples from dst_base */
    uint32_t dst_stride; /* samples */
    uint8_t  w, h, x, y, wpx;
    uint8_t  pad[7];
} SvtHipPalettePredDesc; /* 40 bytes */
int svt_hip_palette_pred_batch(const void *base, void *dst_base, const SvtHipPalettePredDesc *descs, uint32_t n, int dst16, int bit_depth, uint8_t *status,
                               void *stream);

/* F. Host pieces.  svt_hip_palette_cache_y is the merge of svt_get_palette_cache_y (palette.c:153): the above and left colour lists (either may be empty; the caller
 * passes above_n = 0 on a superblock row boundary) into cache[16], returns n_cache; no device work.  The six single-call forms have the reference's prototypes
 * (aom_dsp_rtcd.h:786-793, palette.c:298-299), take host pointers and are exported, NOT installed by svt_hip_setup_rtcd.  Outside the accepted range of A / B the
 * k-means forms write nothing and the two counters return 0. */
int  svt_hip_palette_cache_y(const uint16_t *above_colors, int above_n, const uint16_t *left_colors, int left_n, uint16_t *cache);
void svt_av1_k_means_dim1_hip(const int *data, int *centroids, uint8_t *indices, int n, int k, int max_itr);
void svt_av1_k_means_dim2_hip(const int *data, int *centroids, uint8_t *indices, int n, int k, int max_itr);
void svt_av1_calc_indices_dim1_hip(const int *data, const int *centroids, uint8_t *indices, int n, int k);
void svt_av1_calc_indices_dim2_hip(const int *data, const int *centroids, uint8_t *indices, int n, int k);
int  svt_av1_count_colors_hip(const uint8_t *src, int stride, int rows, int cols, int *val_count);
int  svt_av1_count_colors_highbd_hip(uint16_t *src, int stride, int rows, int cols, int bit_depth, int *val_count);

/* ------------------------------------------- block variance family and the MD sub-pel motion search (csrc/mdsubpel.hip) -------------------- */
/* The AomVarianceFnPtr primitives of svt_aom_mefn_ptr (av1me.c:29-197) for n blocks of mixed sizes in one launch, 8-bit luma.  bsize is a BlockSize 0 .. 21 (the 22
 * sizes of VARIANCES(W, H), variance.c:324-345).  Per block, by kind:
 *   VAR          svt_aom_variance{W}x{H}_c(pre, pre_stride, src, src_stride, &sse): var, sse, sum (sum of pre - src);
 *   SUBPIX       svt_aom_sub_pixel_variance{W}x{H}_c(pre, pre_stride, xoffset, yoffset, src, src_stride, &sse): bilinear_filters_2t, two roundings (+64 >> 7 each,
 *                horizontal to uint16_t, vertical to uint8_t), offsets 0 .. 7;
 *   UPSAMPLED    svt_aom_upsampled_pred_c(.., W, H, xoffset, yoffset, pre, pre_stride, taps) followed by vf against src -- what svt_upsampled_pref_error computes.
 *                taps 1 / 2 / 3 = USE_2_TAPS / USE_4_TAPS / USE_8_TAPS.  svt_aom_convolve8_horiz_c then _vert_c: always 8 taps wide, each stage rounds by 7 and clips
 *                to 8 bits, phase q3 << 1 of av1_interp_4tap[BILINEAR], av1_sub_pel_filters_4, av1_sub_pel_filters_8;
 *   MSE          svt_aom_mse16x16_c: sse (var repeats it, sum is 0); bsize must be BLOCK_16X16;
 *   OBMC_SAD     svt_aom_obmc_sad{W}x{H}_c(pre, pre_stride, wsrc, mask): sad (the other fields 0);
 *   OBMC_VAR     svt_aom_obmc_variance{W}x{H}_c: var, sse, sum of ROUND_POWER_OF_TWO_SIGNED(wsrc - pre * mask, 12);
 *   OBMC_SUBPIX  svt_aom_obmc_sub_pixel_variance{W}x{H}_c: the same on the bilinear prediction.
 * var = sse - (uint32_t)(((int64_t)sum * sum) / (W * H)); sse is the C's wrapping uint32_t sum.  Fields a kind does not produce are written as 0.
 * READABLE EXTENT, never more than the C reads: W x H of pre for VAR, MSE, OBMC_SAD, OBMC_VAR; (W + 1) x (H + 1) for SUBPIX, OBMC_SUBPIX (column W only with
 * xoffset != 0, row H only with yoffset != 0); UPSAMPLED: the block itself when both offsets are 0, columns -3 .. W + 3 of the block's rows when only x is
 * fractional, rows -3 .. H + 3 of the block's columns when only y is, columns -3 .. W + 3 of rows -3 .. H + 3 when both are.  W x H of src; W * H contiguous int32_t
 * of wsrc and of mask.  No vector is clamped to a picture: padding is the caller's.
 * planes.base[] (passed by value), src_base, wsrc_base, mask_base, descs, out, status are device pointers.
 * INVALID DESCRIPTORS (bsize >= 22; kind > 6; an offset above 7 where the kind reads it; UPSAMPLED with taps outside 1 .. 3; MSE at another size; a plane index
 * >= 32 or without a base; a kind whose src_base / wsrc_base / mask_base is NULL) never fault: status == NULL / != NULL and the return value exactly as
 * svt_hip_inter_pred_batch; the result of an invalid descriptor is not written. */
#define SVT_HIP_VAR_VAR         0
#define SVT_HIP_VAR_SUBPIX      1
#define SVT_HIP_VAR_UPSAMPLED   2
#define SVT_HIP_VAR_MSE         3
#define SVT_HIP_VAR_OBMC_SAD    4
#define SVT_HIP_VAR_OBMC_VAR    5
#define SVT_HIP_VAR_OBMC_SUBPIX 6
typedef struct SvtHipBlockVarDesc {
    uint64_t pre_off;        /* samples from planes.base[pre_plane]: the C's first argument */
    uint64_t src_off;        /* bytes from src_base */
    uint64_t wsrc_off;       /* OBMC kinds: int32_t elements from wsrc_base */
    uint64_t mask_off;       /* OBMC kinds: int32_t elements from mask_base */
    uint32_t pre_stride, src_stride;
    uint8_t  pre_plane;
    uint8_t  bsize;          /* BlockSize 0 .. 21 */
    uint8_t  kind;           /* SVT_HIP_VAR_* */
    uint8_t  xoffset, yoffset; /* 0 .. 7 */
    uint8_t  taps;           /* UPSAMPLED: 1 .. 3 */
    uint8_t  pad[2];
} SvtHipBlockVarDesc;
typedef struct SvtHipBlockVarResult {
    uint32_t var, sse;
    int32_t  sum;
    uint32_t sad;
} SvtHipBlockVarResult;
int svt_hip_block_var_batch(SvtHipInterPredPlanes planes, const uint8_t *src_base, const int32_t *wsrc_base, const int32_t *mask_base, const SvtHipBlockVarDesc *descs,
                            uint32_t n, SvtHipBlockVarResult *out, uint8_t *status, void *stream);
/* n (block, reference) sub-pel searches in one launch: one item is one call of md_subpel_search (product_coding_loop.c:2631), i.e. of
 * svt_av1_find_best_sub_pixel_tree (method 0) or svt_av1_find_best_sub_pixel_tree_pruned (method 1) (mcomp.c:688, :606) with is_scaled == 0, 8-bit luma, complete:
 *   tree    centre error (svt_upsampled_setup_center_error); the PD_PASS_1 round reduction from mvp_th / hp_mv_th (mvp_th == 0 switches it off: what ictx == NULL or
 *           another pass gives); early returns in the order early_exit, pred_variance_th (variance against the constant 128 of svt_aom_eb_av1_var_offs,
 *           ROUND_POWER_OF_TWO by num_pels_log2), abs_th_mult with (w * h) >> 2, round == 0; svt_first_level_check, svt_second_level_check_v2 when
 *           iters_per_step > 1; candidates by svt_upsampled_pref_error (UPSAMPLED above with subpel_search_type as taps);
 *   pruned  early returns in the order early_exit, abs_th_mult with (w * h) >> 3, round == 0, pred_variance_th; org_error from skip_diag_refinement 0 / 1 / 2,3 / >= 4
 *           with the w >= 64 || h >= 64 divisor; two_level_checks_fast; the round_dev_th deviation exit; candidates by svf (SUBPIX above); the MV_COST_OPT
 *           pre-evaluation exit of svt_check_better_fast.
 * Common: svt_mv_err_cost for the six MV_COST_TYPE values (ENTROPY reads tables[cost_table]: joint[4] and comp[2][MV_VALS] centred at MV_MAX, the difference
 * clipped at MV_LOW .. MV_UPP as svt_mv_cost does -- the one index that clip leaves outside either end of a table reads the end entry; cost_table < 0 or
 * tables == NULL is the C's mvcost == NULL: cost 0); bias_fp while the running best is full-pel; the (uint64_t)cost * weight / 100 < besterr comparison; INT_MAX for
 * candidates outside the limits; vectors narrowed to int16_t as MV does.
 * The reference position: ref_off is where the block sits in the reference picture (vector 0, 0); a candidate reads planes.base[ref_plane] + ref_off +
 * (row >> 3) * ref_stride + (col >> 3) with the extent of its kind above -- no vector is clamped, the limits and the picture's padding are the caller's.
 * Inside the encoder an item's ref_mv and early_exit come from neighbours that are already decided, so a batch spans the (list, reference, block size) candidates a
 * caller has in hand, not a frame.
 * INVALID DESCRIPTORS (bsize >= 22; method > 1; forced_stop > 3; subpel_search_type outside 1 .. 3; mv_cost_type > 5; cost_table >= n_tables; a plane index >= 32
 * or without a base) never fault: status / return value exactly as svt_hip_inter_pred_batch; the result of an invalid descriptor is not written. */
#define SVT_HIP_MV_VALS 32767 /* MV_VALS (cabac_context_model.h:521) */
typedef struct SvtHipMvCostTable {
    int32_t joint[4];                  /* mvjcost, by MvJointType */
    int32_t comp[2][SVT_HIP_MV_VALS];  /* mvcost[0] (row), mvcost[1] (col): entry [MV_MAX + v] is the C's mvcost[k][v] */
} SvtHipMvCostTable;
typedef struct SvtHipMdSubpelDesc {
    uint64_t src_off;        /* bytes from src_base: the block's first source sample */
    uint64_t ref_off;        /* samples from planes.base[ref_plane]: the block's position in the reference */
    uint32_t src_stride, ref_stride;
    int32_t  lim_col_min, lim_col_max, lim_row_min, lim_row_max; /* SubpelMvLimits (svt_hip_md_subpel_mv_limits) */
    int32_t  pred_variance_th, round_dev_th, bias_fp;
    int32_t  error_per_bit, early_exit_th; /* MV_COST_PARAMS */
    int32_t  cost_table;     /* MV_COST_ENTROPY: index into tables, < 0: none */
    int32_t  qp;
    int32_t  hp_mv_th;       /* md_subpel_me_ctrls.hp_mv_th */
    uint32_t best_mvp_err;   /* ctx->best_fp_mvp_dist[list][ref] */
    int16_t  best_mvp_row, best_mvp_col; /* ctx->mvp_array[list][ref][best_fp_mvp_idx] */
    int16_t  start_mv_row, start_mv_col; /* 1/8 sample: subpel_start_mv */
    int16_t  ref_mv_row, ref_mv_col;
    uint8_t  ref_plane;
    uint8_t  bsize;
    uint8_t  method;         /* 0 SUBPEL_TREE, 1 SUBPEL_TREE_PRUNED */
    uint8_t  allow_hp;
    uint8_t  forced_stop;    /* SUBPEL_FORCE_STOP: 0 EIGHTH_PEL .. 3 FULL_PEL */
    uint8_t  iters_per_step;
    uint8_t  abs_th_mult;
    uint8_t  skip_diag_refinement;
    uint8_t  subpel_search_type; /* 1 .. 3: USE_2_TAPS, USE_4_TAPS, USE_8_TAPS (tree) */
    uint8_t  mv_cost_type;   /* MV_COST_TYPE 0 .. 5 */
    uint8_t  early_exit;     /* early_neigh_check_exit */
    uint8_t  mvp_th;         /* md_subpel_me_ctrls.mvp_th; 0: the rule is off */
    uint8_t  pad[4];
} SvtHipMdSubpelDesc; /* 104 bytes */
typedef struct SvtHipMdSubpelResult {
    int16_t  mv_row, mv_col; /* *bestmv */
    uint32_t besterr;        /* the return value */
    int32_t  distortion;     /* *distortion */
    uint32_t sse1;           /* *sse1 of a caller that set it to 0 before the call */
    uint32_t fp_me_dist;     /* the centre error, what goes to ctx->fp_me_dist */
    uint32_t evals;          /* predictions compared with the source, the centre included (a measurement aid) */
} SvtHipMdSubpelResult;
int svt_hip_md_subpel_search_batch(SvtHipInterPredPlanes planes, const uint8_t *src_base, const SvtHipMvCostTable *tables, uint32_t n_tables,
                                   const SvtHipMdSubpelDesc *descs, uint32_t n, SvtHipMdSubpelResult *out, uint8_t *status, void *stream);
/* Host helper: the four SubpelMvLimits as md_subpel_search derives them (:2656-2666) -- the UMV window of the block, svt_av1_set_mv_search_range and
 * svt_av1_set_subpel_mv_search_range restated.  limits = col_min, col_max, row_min, row_max.  Returns 0, or -1 (nothing written) for bsize >= 22 or a NULL limits. */
int svt_hip_md_subpel_mv_limits(int mi_row, int mi_col, int bsize, int mi_rows, int mi_cols, int16_t ref_mv_row, int16_t ref_mv_col, int32_t *limits);
/* single-call forms with the reference's prototypes (aom_dsp_rtcd.h; exported, NOT installed by svt_hip_setup_rtcd: INTEGRATION.md).  Host pointers, the readable
 * extents above.  On a device error, a NULL pointer or an offset above 7 nothing is written and the value forms return 0. */
#define SVT_HIP_VARIANCE_DECL(W, H)                                                                                                                                      \
    unsigned int svt_aom_variance##W##x##H##_hip(const uint8_t *src_ptr, int source_stride, const uint8_t *ref_ptr, int ref_stride, unsigned int *sse);                  \
    uint32_t     svt_aom_sub_pixel_variance##W##x##H##_hip(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride,   \
                                                       uint32_t *sse);                                                                                                  \
    unsigned int svt_aom_obmc_sad##W##x##H##_hip(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);                                          \
    unsigned int svt_aom_obmc_variance##W##x##H##_hip(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);                  \
    unsigned int svt_aom_obmc_sub_pixel_variance##W##x##H##_hip(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask,  \
                                                            unsigned int *sse);
#define SVT_HIP_FOR_ALL_VARIANCE_SIZES(X)                                                                                                             \
    X(128, 128) X(128, 64) X(64, 128) X(64, 64) X(64, 32) X(32, 64) X(32, 32) X(32, 16) X(16, 32) X(16, 16) X(16, 8) X(8, 16) X(8, 8) X(8, 4) X(4, 8) \
    X(4, 4) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)
SVT_HIP_FOR_ALL_VARIANCE_SIZES(SVT_HIP_VARIANCE_DECL)
#undef SVT_HIP_VARIANCE_DECL
uint32_t svt_aom_mse16x16_hip(const uint8_t *src_ptr, int32_t source_stride, const uint8_t *ref_ptr, int32_t recon_stride, uint32_t *sse);
/* svt_aom_upsampled_pred: writes the width x height prediction (packed, row pitch `width`) to comp_pred; xd, cm, mi_row, mi_col, mv are not read, as in the C.
 * width, height powers of two 4 .. 128, subpel_search 1 .. 3, otherwise nothing is written. */
#ifdef SVT_HIP_REFERENCE_TYPES
void svt_aom_upsampled_pred_hip(MacroBlockD *xd, const struct AV1Common *const cm, int mi_row, int mi_col, const MV *const mv, uint8_t *comp_pred, int width, int height,
                                int subpel_x_q3, int subpel_y_q3, const uint8_t *ref, int ref_stride, int subpel_search);
#else
void svt_aom_upsampled_pred_hip(void *xd, const void *cm, int mi_row, int mi_col, const SvtHipMv *mv, uint8_t *comp_pred, int width, int height, int subpel_x_q3,
                                int subpel_y_q3, const uint8_t *ref, int ref_stride, int subpel_search);
#endif

/* ------------------------------------------- OBMC motion refinement: weighted target and MV search (csrc/mdsubpel.hip) -------------------- */
/* A. calc_target_weighted_pred (enc_inter_prediction.c:1756) for n blocks in one launch, 8-bit luma: wsrc and mask of the OBMC error
 *   error(x, y) = wsrc(x, y) - mask(x, y) * P(x, y), what ctx->wsrc_buf / ctx->mask_buf hold after the call.  Per pixel (row, col), ovA = min(H, 64) >> 1,
 *   ovL = min(W, 64) >> 1, Mv / Mh = svt_av1_get_obmc_mask(ovA) / (ovL):
 *     above stage  up_available, col inside an above span, row < ovA:  w = (64 - Mv[row]) * above(row, col), k = Mv[row];  otherwise w = 0, k = 64;
 *     both times 64;
 *     left stage   left_available, row inside a left span, col < ovL:  w = (w >> 6) * Mh[col] + (left(row, col) << 6) * (64 - Mh[col]), k = (k >> 6) * Mh[col];
 *     wsrc = src(row, col) * 4096 - w, mask = k.
 * A span is what foreach_overlappable_nb_above / _left hand to svt_av1_calc_target_weighted_pred_above_c / _left_c (:1581, :1610): (rel_mi, len_mi) in units of
 * 4 samples from the block's left / top edge.  The walk over the mi grid (is_neighbor_overlappable, the 4-wide pairing, max_neighbor_obmc, the picture-edge clip)
 * is the caller's; the spans of one side must not overlap (the walk never produces that).  above / left are the neighbours' predictions with (0, 0) at the block's
 * top-left sample, the layout svt_hip_inter_pred_batch writes and build_obmc_inter_pred reads: planes.base[above_plane] + above_off + row * above_stride + col.
 * READABLE EXTENT: W x H of src; of above the spans' columns of rows 0 .. ovA - 1, and only when up_available; of left columns 0 .. ovL - 1 of the spans' rows, and
 * only when left_available.
 * Output: W * H contiguous int32_t (pitch W) at wsrc_out + out_off and at mask_out + out_off.
 * bsize: OBMC needs 8 samples in both directions (is_motion_variation_allowed_bsize), so BlockSize 0, 1, 2, 16, 17 are invalid.
 * INVALID DESCRIPTORS (such a bsize or one >= 22; more than four spans on a side; a span with len_mi == 0 or rel_mi + len_mi > the block's mi count; a plane index
 * >= 32, or a plane without a base on a side that is available and has spans; src_base == NULL) never fault: status / return value exactly as
 * svt_hip_inter_pred_batch; the output of an invalid descriptor is not written. */
#define SVT_HIP_OBMC_MAX_SPANS 4
typedef struct SvtHipObmcWsrcDesc {
    uint64_t src_off;        /* bytes from src_base */
    uint64_t above_off;      /* samples from planes.base[above_plane] */
    uint64_t left_off;       /* samples from planes.base[left_plane] */
    uint64_t out_off;        /* int32_t elements from wsrc_out and from mask_out */
    uint32_t src_stride, above_stride, left_stride;
    uint8_t  above_plane, left_plane;
    uint8_t  bsize;
    uint8_t  up_available, left_available;
    uint8_t  n_above, n_left; /* spans per side, 0 .. 4 */
    uint8_t  pad0;
    uint8_t  above_rel[SVT_HIP_OBMC_MAX_SPANS], above_len[SVT_HIP_OBMC_MAX_SPANS]; /* rel_mi_col, nb_mi_width */
    uint8_t  left_rel[SVT_HIP_OBMC_MAX_SPANS], left_len[SVT_HIP_OBMC_MAX_SPANS];   /* rel_mi_row, nb_mi_height */
    uint8_t  pad[4];
} SvtHipObmcWsrcDesc; /* 72 bytes */
int svt_hip_obmc_wsrc_batch(SvtHipInterPredPlanes planes, const uint8_t *src_base, const SvtHipObmcWsrcDesc *descs, uint32_t n, int32_t *wsrc_out, int32_t *mask_out,
                            uint8_t *status, void *stream);
/* B. n OBMC motion refinements in one launch: one item is one call of single_motion_search (mode_decision.c:2290) with motion_mode == OBMC_CAUSAL, complete, 8-bit luma:
 *   full-pel (do_full_refine)  svt_av1_set_mv_search_range(ref_mv) on a copy of the limits; mvp_full = best_pred_mv >> 3 clamped to it;
 *           obmc_refining_search_sad (av1me.c:721): osdf + mvsad_err_cost at the centre, then up to fpel_search_range rounds of the 4 (fpel_search_diag: 8) neighbours
 *           {-1,0} {0,-1} {0,1} {1,0} {-1,1} {1,1} {1,-1} {-1,-1} in that order, is_mv_in, strict < against the running best before and after the cost is added, stop
 *           on a round without a winner; then get_obmc_mvpred_var: thissme = ovf + svt_aom_mv_err_cost(mv * 8).  Without it the start is best_pred_mv >> 3;
 *   sub-pel (do_frac_refine)   svt_av1_find_best_obmc_sub_pixel_tree_up (av1me.c:963) with set_subpel_mv_search_range on the un-narrowed limits: the centre error,
 *           round = 3 - forced_stop (2 when !allow_hp && round == 3), per round the four axis candidates, the diagonal from cost_array, the move, and
 *           SECOND_LEVEL_CHECKS_BEST when iters_per_step > 1 and the round had a winner; INT_MAX for a candidate outside the range; every comparison unsigned.
 *           subpel_search_type 0: osvf (OBMC_SUBPIX above); 1 .. 3: svt_aom_upsampled_pred with USE_2_TAPS / _4_TAPS / _8_TAPS, then ovf.  Without it the vector is << 3;
 *   rate    svt_av1_mv_bit_cost with MV_COST_WEIGHT 108, or svt_av1_mv_bit_cost_light.
 * refine_level of svt_aom_obmc_motion_refinement maps to the two flags as single_motion_search does: 0, 1, 3 -> do_full_refine = do_frac_refine = 1; 2, 4 ->
 * do_full_refine = 0, do_frac_refine = 1; any other level -> both 0.  The encoder passes forced_stop 0, iters_per_step 2, subpel_search_type 3, fpel_search_range /
 * fpel_search_diag of obmc_ctrls, sad_per_bit = svt_aom_get_sad_per_bit(base_q_idx, 0), error_per_bit = max(full_lambda_md[8 bit] >> RD_EPB_SHIFT, 1).
 * Costs: approx_inter_rate selects mvsad_err_cost_light / svt_aom_mv_err_cost_light / svt_av1_mv_bit_cost_light (1296 + 50 * the differences' magnitudes, the full-pel
 * ones times 8); otherwise tables[cost_table] as in the sub-pel search above (svt_mv_cost's clip and the table-end rule; the differences narrowed to int16_t as MV
 * does; (unsigned)cost * sad_per_bit rounded by 9 bits at full-pel, (int64_t)cost * error_per_bit rounded by 14 bits at sub-pel).  cost_table < 0 or tables == NULL is
 * mvcost == NULL: every table cost is 0 (the C tests the pointer in svt_aom_mv_err_cost only; here the full-pel cost and the rate follow it).
 * THE TARGET, per item: SVT_HIP_OBMC_TARGET_ARRAYS -- W * H int32_t at wsrc_base + wsrc_off and mask_base + mask_off, any values svt_hip_block_var_batch accepts;
 * SVT_HIP_OBMC_TARGET_DERIVED -- the inputs of A (source, the two neighbour predictions, availability, spans): the wave computes wsrc / mask from those bytes with the
 * closed form of A each time it needs them and the int32_t arrays never exist in memory.  Both forms give identical results for the arrays A produces.
 * A candidate's error is by definition what svt_hip_block_var_batch returns for the same (pre, wsrc, mask) with kind OBMC_SAD, OBMC_VAR, OBMC_SUBPIX, or UPSAMPLED
 * prediction followed by OBMC_VAR; readable extents of the reference are those of these kinds at every candidate visited.  No vector is clamped to a picture: the
 * limits (full-pel units: the UMV window of svt_hip_obmc_mv_limits) and the padding are the caller's.
 * Result: mv (1/8 sample), the full-pel winner, thissme (0 without full-pel), besterr / distortion / sse1 of the sub-pel search (0 without it; sse1 of a caller that
 * set it to 0), rate_mv, fp_rounds = full-pel rounds that moved the centre, evals = predictions compared with the target (a measurement aid).
 * INVALID DESCRIPTORS (a bsize A rejects; target_form > 1; subpel_search_type > 3; forced_stop > 3; fpel_search_range > 64; cost_table >= n_tables; a plane index >= 32
 * or a reference plane without a base; ARRAYS without wsrc_base / mask_base; DERIVED with what A rejects) never fault: status / return value exactly as
 * svt_hip_inter_pred_batch; the result of an invalid descriptor is not written. */
#define SVT_HIP_OBMC_TARGET_ARRAYS  0
#define SVT_HIP_OBMC_TARGET_DERIVED 1
typedef struct SvtHipObmcSearchDesc {
    uint64_t ref_off;        /* samples from planes.base[ref_plane]: the block's position in the reference (vector 0, 0) */
    uint64_t wsrc_off, mask_off;          /* ARRAYS: int32_t elements from wsrc_base / mask_base */
    uint64_t src_off, above_off, left_off; /* DERIVED: as in SvtHipObmcWsrcDesc */
    uint32_t ref_stride, src_stride, above_stride, left_stride;
    int32_t  lim_col_min, lim_col_max, lim_row_min, lim_row_max; /* x->mv_limits of mode_decision.c:2324-2327, full-pel (svt_hip_obmc_mv_limits) */
    int32_t  sad_per_bit, error_per_bit;
    int32_t  cost_table;     /* index into tables, < 0: none */
    int16_t  best_pred_mv_row, best_pred_mv_col; /* 1/8 sample */
    int16_t  ref_mv_row, ref_mv_col;
    uint8_t  ref_plane, above_plane, left_plane;
    uint8_t  bsize;
    uint8_t  target_form;    /* SVT_HIP_OBMC_TARGET_* */
    uint8_t  do_full_refine, do_frac_refine;
    uint8_t  approx_inter_rate;
    uint8_t  fpel_search_range; /* 0 .. 64 */
    uint8_t  fpel_search_diag;
    uint8_t  allow_hp;
    uint8_t  forced_stop;    /* 0 .. 3 */
    uint8_t  iters_per_step;
    uint8_t  subpel_search_type; /* 0 bilinear osvf, 1 .. 3 USE_2_TAPS / USE_4_TAPS / USE_8_TAPS */
    uint8_t  up_available, left_available;
    uint8_t  n_above, n_left;
    uint8_t  pad0[2];
    uint8_t  above_rel[SVT_HIP_OBMC_MAX_SPANS], above_len[SVT_HIP_OBMC_MAX_SPANS];
    uint8_t  left_rel[SVT_HIP_OBMC_MAX_SPANS], left_len[SVT_HIP_OBMC_MAX_SPANS];
} SvtHipObmcSearchDesc; /* 136 bytes */
typedef struct SvtHipObmcSearchResult {
    int16_t  mv_row, mv_col; /* x->best_mv, 1/8 sample */
    int16_t  fp_row, fp_col; /* the full-pel vector the sub-pel search started from */
    int32_t  thissme;        /* what svt_av1_obmc_full_pixel_search returns */
    uint32_t besterr;        /* what svt_av1_find_best_obmc_sub_pixel_tree_up returns */
    int32_t  distortion;
    uint32_t sse1;
    int32_t  rate_mv;
    uint32_t fp_rounds;
    uint32_t evals;
} SvtHipObmcSearchResult; /* 36 bytes */
int svt_hip_obmc_search_batch(SvtHipInterPredPlanes planes, const uint8_t *src_base, const int32_t *wsrc_base, const int32_t *mask_base, const SvtHipMvCostTable *tables,
                              uint32_t n_tables, const SvtHipObmcSearchDesc *descs, uint32_t n, SvtHipObmcSearchResult *out, uint8_t *status, void *stream);
/* Host helper: the UMV window single_motion_search sets (:2324-2327), full-pel: limits = col_min, col_max, row_min, row_max.  Returns 0, or -1 (nothing written) for
 * bsize outside 0 .. 21 or a NULL limits. */
int svt_hip_obmc_mv_limits(int mi_row, int mi_col, int bsize, int mi_rows, int mi_cols, int32_t *limits);
/* One item from host memory: upload, one launch, download.  desc gives everything but the addresses: its offsets, strides and plane indices are ignored.
 * ref points at the block's position in the reference; ref_border samples around the W x H block are readable on every side, and the call returns -1 without
 * launching when |start vector| + fpel_search_range (with full-pel) + 6 (with sub-pel: under two samples of movement and the four of the filter) exceeds it.  ARRAYS: wsrc / mask (W * H each); DERIVED: src, above, left with
 * their strides (above / left may be NULL on a side that is not available or has no span).  table: one SvtHipMvCostTable or NULL (desc->cost_table is ignored).
 * Returns 0 and writes *result; -1 for an invalid item or a NULL pointer, SVT_HIP_E_DEVICE on a device error: nothing is written then. */
int svt_hip_obmc_refine_host(const SvtHipObmcSearchDesc *desc, const uint8_t *ref, int ref_stride, int ref_border, const int32_t *wsrc, const int32_t *mask,
                             const uint8_t *src, int src_stride, const uint8_t *above, int above_stride, const uint8_t *left, int left_stride,
                             const SvtHipMvCostTable *table, SvtHipObmcSearchResult *result);

/* ------------------------------------------- picture-analysis statistics and the variance boost (csrc/picstats.hip) ------------------------- */
#define SVT_HIP_BLOCK_MEAN_PREC_FULL 0 /* BLOCK_MEAN_PREC_FULL / _SUB, definitions.h:2391-2392 */
#define SVT_HIP_BLOCK_MEAN_PREC_SUB  1
/* compute_block_mean_compute_variance (pic_analysis_process.c:306-1380) for every 64x64 superblock of n_pics equally shaped 8-bit luma planes, and
 * compute_picture_spatial_statistics (:1531-1552).  Picture i starts at luma_base + i * pic_pitch; its first picture pixel is at (org_x, org_y), stride in bytes.
 * prec = SVT_HIP_BLOCK_MEAN_PREC_SUB (what the encoder sets, enc_handle.c:4254: every other row, sum << 3, sum of squares << 11) or _FULL ((sum << 8) / 64,
 * (sum of squares << 16) / 64).  variance = [n_pics][ceil(width / 64) * ceil(height / 64)][85] uint16_t in ME_TIER_ZERO_PU_* order (me_context.h:54-138): 64x64, 4 32x32,
 * 16 16x16, 64 8x8, superblocks in raster order; with write_sub64 == 0 only entry 0 of each superblock is written (the reference writes the rest only when
 * enable_adaptive_quantization == 1 || variance_octile, :1110).  pic_avg_variance = [n_pics] (may be NULL).  All pointers device; bit-exact.
 * READABLE EXTENT: an edge superblock is read as a full 64x64 from the padded plane, as the reference reads it -- every picture must be readable over rows
 * org_y .. org_y + 64 * ceil(height / 64) - 1 and columns org_x .. org_x + 64 * ceil(width / 64) - 1. */
void svt_hip_picture_variance_batch(const uint8_t *luma_base, uint64_t pic_pitch, uint32_t stride, uint32_t org_x, uint32_t org_y, uint32_t width, uint32_t height,
                                    uint32_t n_pics, int prec, int write_sub64, uint16_t *variance, uint16_t *pic_avg_variance, void *stream);
/* svt_variance_adjust_qp + av1_get_deltaq_sb_variance_boost (rc_process.c:1403-1617) on the device table written above.  variance = [n_sb][85], qindex_in = [n_sb] what
 * TPL left in sb_ptr->qindex, qindex_out = [n_sb] (may alias qindex_in), frame_out = one SvtHipVarBoostFrame: all four device.  strength 1-4, octile 1-8, curve 0-2,
 * bit_depth 8 / 10 / 12.  q_fp8_table is a HOST array: q_fp8_table[i] = svt_av1_convert_qindex_to_q_fp8(i, bit_depth) for i = 0 .. 255 (rc_process.c:180-188) -- the
 * library embeds no quantiser table, and svt_av1_compute_qdelta_fp's two searches (:190-210) run against this one.  The boost curve (double-precision pow / log2 and a
 * truncating division, :1462-1493) is evaluated on the HOST with the C library, once per (base_q_idx, strength, curve, bit_depth, table), never on the device.
 * Two launches on `stream`; returns 0, or -1 for an argument outside the ranges above (nothing is launched). */
typedef struct SvtHipVarBoostFrame { int32_t normalized_base_q_idx, min_qindex, max_qindex, reserved; } SvtHipVarBoostFrame;
int svt_hip_variance_boost_qindex(const uint16_t *variance, const uint8_t *qindex_in, uint32_t n_sb, uint8_t base_q_idx, uint8_t strength, uint8_t octile, uint8_t curve,
                                  int bit_depth, const int32_t *q_fp8_table, uint8_t *qindex_out, SvtHipVarBoostFrame *frame_out, void *stream);
/* The host-evaluated table itself: boost_out[v] (HOST, 65 536 entries) = what av1_get_deltaq_sb_variance_boost returns for a blended 8x8 variance v
 * (v == 0 counts as 1, :1459).  No device call. */
int svt_hip_variance_boost_table(uint8_t base_q_idx, uint8_t strength, uint8_t curve, int bit_depth, const int32_t *q_fp8_table, int16_t *boost_out);
/* sub_sample_luma_generate_pixel_intensity_histogram_bins + calculate_histogram (pic_analysis_process.c:1461-1524, :166-184) on the 1/16 plane: origin = its first
 * picture pixel.  regions_w x regions_h regions (4 x 4, or 1 along a side below 64: enc_handle.c:4248), the last of a direction takes the remainder; decim_step 1 or 4.
 * histogram = [regions_w][regions_h][256] uint32_t ((1 + count) * 16 * decim_step^2), average_intensity_per_region = [regions_w][regions_h] uint8_t (the reference
 * stores that byte in a uint64_t), avg_luma = one uint64_t (may be NULL).  All pointers device; bit-exact while a bin stays below 2^32. */
void svt_hip_picture_histogram(const uint8_t *origin, uint32_t stride, uint32_t width, uint32_t height, uint32_t regions_w, uint32_t regions_h, uint32_t decim_step,
                               uint32_t *histogram, uint8_t *average_intensity_per_region, uint64_t *avg_luma, void *stream);
/* single-call forms with the reference's prototypes: the four dispatch pointers of aom_dsp_rtcd.c:516-519 (aom_dsp_rtcd.h:858-862; svt_compute_mean_c,
 * svt_compute_mean_squared_values_c, svt_compute_sub_mean_8x8_c, svt_compute_interm_var_four8x8_c, pic_analysis_process.c:190-300).  Host pointers; exported, NOT
 * installed by svt_hip_setup_rtcd. */
uint64_t svt_compute_mean_8x8_hip(uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height);
uint64_t svt_compute_mean_square_values_8x8_hip(uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height);
uint64_t svt_compute_sub_mean_8x8_hip(uint8_t *input_samples, uint16_t input_stride);
void     svt_compute_interm_var_four8x8_hip(uint8_t *input_samples, uint16_t input_stride, uint64_t *mean_of8x8_blocks, uint64_t *mean_of_squared8x8_blocks);

/* ------------------------------------------- picture preparation for ME ------------------------- */
/* downsample_2d -> svt_aom_downsample_2d_c (aom_dsp_rtcd.h:841, pic_analysis_process.c:130-160): out(x, y) = (2x2 box at the centre of cell
 * (x, y) of decim_step x decim_step input pixels + 2) >> 2; host pointers (RTCD form). */
void svt_aom_downsample_2d_hip(uint8_t *input_samples, uint32_t input_stride, uint32_t input_area_width, uint32_t input_area_height,
                               uint8_t *decim_samples, uint32_t decim_stride, uint32_t decim_step);
/* Device-resident form of one level of svt_aom_downsample_filtering_input_picture (pic_analysis_process.c:2138-2200): decimate the picture
 * whose first pixel is `in_origin` into the interior of the padded plane `out_base` (interior origin at (pad_x, pad_y)) AND replicate the
 * pad_x / pad_y wide borders (svt_aom_generate_padding, pic_operators.c:397-441) in the same launch. */
void svt_hip_downsample_2d_padded(const uint8_t *in_origin, uint32_t in_stride, uint32_t in_width, uint32_t in_height, uint8_t *out_base,
                                  uint32_t out_stride, uint32_t pad_x, uint32_t pad_y, uint32_t step, void *stream);
/* svt_aom_generate_padding on a device plane, in place: `base` = top-left of the padded plane */
void svt_hip_generate_padding(uint8_t *base, uint32_t stride, uint32_t width, uint32_t height, uint32_t pad_x, uint32_t pad_y, void *stream);

/* --------------------------------------------------- deblocking edge filters ---------------------- */
/* svt_aom_lpf_{horizontal,vertical}_{4,6,8,14} / svt_aom_highbd_lpf_* -> `_c` (common_dsp_rtcd.h:1037-1067, Codec/deblocking_common.c:141-865).
 * Batched form: n edge segments of 4 samples over a device plane; (x, y) = the q0 sample of the segment's first position; vertical = 1 for a
 * column boundary (filtering along x); length in {4, 6, 8, 14}; blimit / limit / thresh as the reference's per-edge LoopFilterThresh bytes.
 * Segments of one launch must not overlap (the reference filters all vertical edges of a picture before the horizontal ones).  One thread per
 * segment: list the segments in raster order (x fastest) and grouped by length, so that neighbouring threads touch neighbouring addresses and
 * take the same filter path; a vertical edge reads up to 8 samples either side of x (4 for lengths < 14), which must lie inside the allocation. */
typedef struct SvtHipLpfEdge {
    uint32_t x, y;
    uint8_t  vertical, length, blimit, limit, thresh, pad[3];
} SvtHipLpfEdge; /* 16 bytes */
void svt_hip_lpf_edges_batch(void *plane, uint32_t stride, int is_16bit, int bd, const SvtHipLpfEdge *edges, uint32_t n, void *stream);
/* One plane of svt_av1_loop_filter_frame (deblocking_filter.c:625) from HOST memory: all vertical-edge segments, then all horizontal-edge segments (the order
 * the standard defines; the reference's SB-by-SB schedule with its one-SB lag for horizontal edges gives the same picture), in place.  The plane must be
 * readable 16 samples left / right of its rows (the reference's picture padding).  A seam records the segments by running the reference's own driver with
 * recording leaf functions.  Synchronous.  The WHOLE width x height plane is downloaded in place: nothing else may write the plane while the call runs (the
 * frame-level seams call it from the one thread that owns the picture at that stage). */
int svt_hip_lpf_plane_host(void *plane, uint32_t stride, uint32_t width, uint32_t height, int is_16bit, int bd, const SvtHipLpfEdge *vert, uint32_t n_vert,
                            const SvtHipLpfEdge *horz, uint32_t n_horz);
#define SVT_HIP_LPF_DECL(LEN)                                                                                                              \
    void svt_aom_lpf_horizontal_##LEN##_hip(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh); \
    void svt_aom_lpf_vertical_##LEN##_hip(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit, const uint8_t *thresh);   \
    void svt_aom_highbd_lpf_horizontal_##LEN##_hip(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,                 \
                                                   const uint8_t *thresh, int32_t bd);                                                     \
    void svt_aom_highbd_lpf_vertical_##LEN##_hip(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,                   \
                                                 const uint8_t *thresh, int32_t bd);
SVT_HIP_LPF_DECL(4)
SVT_HIP_LPF_DECL(6)
SVT_HIP_LPF_DECL(8)
SVT_HIP_LPF_DECL(14)
#undef SVT_HIP_LPF_DECL

/* ---------------------------------------------------------------- CDEF (a17-a20) --------------------- */
/* One plane of one frame.  Filter-block grid = ceil(width / (64 >> xdec)) x ceil(height / (64 >> ydec)); tile
 * construction as cdef_seg_search (cdef_process.c:208-228).  Call once per plane, luma first (it produces dir/var). */
typedef struct SvtHipCdefParams {
    const void *recon;   /* deblocked reconstruction (input), PIX = uint8_t or uint16_t            */
    const void *source;  /* original picture (search mode only)                                    */
    void       *out;     /* apply mode: filtered plane, OUT OF PLACE; caller pre-copies recon->out
                            (skipped units / zero-strength blocks are not touched)                  */
    uint32_t recon_stride, source_stride, out_stride; /* pixels */
    uint32_t width, height;                           /* plane size in pixels */
    uint8_t  xdec, ydec, pli, is_16bit;
    uint8_t  coeff_shift, pri_damping, sec_damping, subsampling; /* dampings before the per-plane adjustment of cdef.c:349-350 */
    uint32_t ncand;       /* search: number of (pri, sec) candidates */
    const uint8_t *skip;  /* [(fb rows * 8)][(fb cols * 8)] 1 = 8x8 luma unit is skipped (svt_sb_compute_cdef_list) */
    const int32_t *pri;   /* search: [ncand] primary levels; apply: [nfb]                           */
    const int32_t *sec;   /* search: [ncand] secondary strengths in {0,1,2,4}; apply: [nfb]         */
    uint8_t       *dir;   /* [nfb][64] written when pli == 0, read otherwise                        */
    int32_t       *var;   /* [nfb][64]                                                              */
    uint64_t      *mse;   /* search: [nfb][ncand] = svt_compute_cdef_dist of every candidate        */
} SvtHipCdefParams;
/* mode 0 = apply (svt_cdef_filter_fb over the frame, enc_cdef.c:284), 1 = strength search (cdef_process.c:106), 2 = apply with the luma directions /
 * variances taken from dir / var (what the search pass over the same reconstruction wrote; the reference recomputes identical values, cdef.c:367-386).
 * All pointers inside `params` are DEVICE pointers; the struct itself is read on the host. */
void svt_hip_cdef_frame(int mode, const SvtHipCdefParams *params, void *stream);
/* the same over the filter-block rows [fb_row_begin, fb_row_end) of the plane only (fb_row_end < 0: to the last row) -- one GPU's strip when a picture is split
 * over several devices; halos above / below the strip are read from the full input plane, outputs outside the strip are not touched */
void svt_hip_cdef_frame_rows(int mode, const SvtHipCdefParams *params, int fb_row_begin, int fb_row_end, void *stream);
/* svt_av1_cdef_frame (enc_cdef.c:284-560) for a 4:2:0 picture from HOST memory -- what a seam at cdef_process.c:458 calls: planes filtered IN PLACE (the
 * reference keeps the neighbours' unfiltered samples in line / column buffers, which is what filtering out of place on the device gives), skip = the 8x8
 * units svt_sb_compute_cdef_list leaves out (and every unit of a filter block the reference skips: all four strengths zero), pri / sec per filter block from
 * frm_hdr->cdef_params.cdef_y_strength / cdef_uv_strength[mbmi.cdef_strength] (sec 3 -> 4).  width / height = mi_cols * 4, mi_rows * 4.  Synchronous. */
typedef struct SvtHipCdefApplyHost {
    void          *plane[3];
    uint32_t       stride[3]; /* samples */
    uint32_t       width, height;
    uint8_t        num_planes, is_16bit, coeff_shift, damping; /* scs encoder_bit_depth - 8; frm_hdr->cdef_params.cdef_damping */
    const uint8_t *skip;      /* [(fb rows * 8)][(fb cols * 8)] */
    const int32_t *pri_y, *sec_y, *pri_uv, *sec_uv; /* [fb rows * fb cols] */
} SvtHipCdefApplyHost;
int svt_hip_cdef_apply_host(const SvtHipCdefApplyHost *params);
/* cdef_seg_search (cdef_process.c:106-345) for ALL filter blocks of a 4:2:0 picture from HOST memory: for each plane the distortion
 * (svt_compute_cdef_dist of the filtered block, NOT yet multiplied by the sub-sampling factor) of every candidate (pri, sec) and every filter block, plus the
 * luma directions / variances (pcs->cdef_dir_data).  Candidates: cdef_ctrls->default_first_pass_fs[] then default_second_pass_fs[] as (fs / 4, fs % 4 with 3 -> 4);
 * the chroma list leaves out the entries whose *_fs_uv is -1.  subsampling[] = cdef_ctrls->subsampling_factor capped as :215-219 (luma 4, chroma 1).  Synchronous. */
typedef struct SvtHipCdefSearchHost {
    const void    *recon[3], *source[3]; /* pcs->cdef_input_recon / cdef_input_source */
    uint32_t       recon_stride[3], source_stride[3];
    uint32_t       width, height; /* mi_cols * 4, mi_rows * 4 */
    uint8_t        is_16bit, coeff_shift, damping, subsampling[2], pad[3];
    const uint8_t *skip;          /* [(fb rows * 8)][(fb cols * 8)] from svt_sb_compute_cdef_list */
    uint32_t       ncand_y, ncand_uv;
    const int32_t *pri_y, *sec_y, *pri_uv, *sec_uv;
    uint64_t      *mse_y, *mse_u, *mse_v; /* [nfb][ncand] */
    uint8_t       *dir;                   /* [nfb][64] */
    int32_t       *var;                   /* [nfb][64] */
} SvtHipCdefSearchHost;
int svt_hip_cdef_search_host(const SvtHipCdefSearchHost *params);
/* Strength selection over the search output: svt_search_one_dual -> svt_search_one_dual_c (aom_dsp_rtcd.h:242,
 * enc_cdef.c:627-683).  mse0 / mse1 = [sb_count][64] luma / chroma distortion tables (device; svt_hip_cdef_frame(mode 1) writes exactly this
 * layout), lev0 / lev1 = device arrays holding the nb_strengths pairs selected so far, entry [nb_strengths] receives the new pair,
 * best_tot_mse[1] the frame total.  workspace: (4096 + sb_count) * 8 bytes of device scratch. */
void svt_hip_cdef_search_one_dual(const uint64_t *mse0, const uint64_t *mse1, int *lev0, int *lev1, int nb_strengths, int sb_count, int start_gi,
                                  int end_gi, uint64_t *best_tot_mse, void *workspace, void *stream);
uint64_t svt_search_one_dual_hip(int *lev0, int *lev1, int nb_strengths, uint64_t **mse[2], int sb_count, int start_gi, int end_gi);
/* joint_strength_search_dual (enc_cdef.c:697-726): nb_strengths greedy additions followed by 4 * nb_strengths refinement rounds, every step a
 * svt_search_one_dual on the device; lev0 / lev1 (device, >= nb_strengths entries) receive the selected pairs, best_tot_mse[1] the frame total. */
void svt_hip_cdef_joint_strength_search(const uint64_t *mse0, const uint64_t *mse1, int *lev0, int *lev1, int nb_strengths, int sb_count,
                                        int start_gi, int end_gi, uint64_t *best_tot_mse, void *workspace, void *stream);
/* per filter block: index of the selected pair with the smallest luma + chroma distortion (finish_cdef_search, enc_cdef.c:916-931) */
void svt_hip_cdef_assign_fb_strengths(const uint64_t *mse0, const uint64_t *mse1, const int *lev0, const int *lev1, int nb_strengths, int sb_count,
                                      int8_t *best_gi, void *stream);
/* RTCD-signature single-call forms (common_dsp_rtcd.h:1010-1029, aom_dsp_rtcd.h:208-209) */
uint8_t  svt_aom_cdef_find_dir_hip(const uint16_t *img, int32_t stride, int32_t *var, int32_t coeff_shift);
void     svt_aom_cdef_find_dir_dual_hip(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1, int32_t *var2,
                                        int32_t coeff_shift, uint8_t *out1, uint8_t *out2);
void     svt_cdef_filter_block_hip(uint8_t *dst8, uint16_t *dst16, int32_t dstride, const uint16_t *in, int32_t pri_strength,
                                   int32_t sec_strength, int32_t dir, int32_t pri_damping, int32_t sec_damping, int32_t bsize,
                                   int32_t coeff_shift, uint8_t subsampling_factor);
/* SvtHipCdefList is CdefList (definitions.h:256-259): the (by, bx) 8x8 position of one non-skip block inside its 64x64 filter block */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef CdefList SvtHipCdefList;
#else
typedef struct SvtHipCdefList { uint8_t by, bx; } SvtHipCdefList;
#endif
uint64_t svt_compute_cdef_dist_16bit_hip(const uint16_t *dst, int32_t dstride, const uint16_t *src, const SvtHipCdefList *dlist, int32_t cdef_count,
                                         SvtHipBlockSize bsize, int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);
uint64_t svt_compute_cdef_dist_8bit_hip(const uint8_t *dst8, int32_t dstride, const uint8_t *src8, const SvtHipCdefList *dlist, int32_t cdef_count,
                                        SvtHipBlockSize bsize, int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);
void     svt_aom_copy_rect8_8bit_to_16bit_hip(uint16_t *dst, int32_t dstride, const uint8_t *src, int32_t sstride, int32_t v, int32_t h);

/* ---------------------------------------------------------------- loop restoration (a21-a23) ---------- */
typedef struct SvtHipLrUnit {          /* RestorationUnitInfo (restoration.h:184-188) without its alignment padding */
    int32_t rtype;                     /* RestorationType: 0 RESTORE_NONE, 1 RESTORE_WIENER, 2 RESTORE_SGRPROJ */
    int16_t vfilter[8], hfilter[8];    /* WienerInfo: 7 symmetric taps + a trailing 0 */
    int32_t ep, xqd[2];                /* SgrprojInfo */
} SvtHipLrUnit;
/* One plane of svt_av1_loop_restoration_filter_frame (restoration.c:1179): restoration units of unit_size pixels
 * (shifted up by 8 >> ss_y, the last one absorbing a remainder < 3/2 unit), 64 >> ss_y row stripes, 64 >> ss_x column
 * processing units, stripe boundaries taken from the saved deblocked lines (2 rows per stripe, restoration.c:288-332),
 * frame edges replicated (svt_extend_frame).  Out of place.  All pointers are device pointers.  unit_size >= 64 >> ss_y, as in AV1 (RESTORATION_UNITSIZE
 * 64 / 128 / 256 on luma, halved on 4:2:0 chroma): a processing unit takes the coefficients of the unit its first row lies in.  Columns: where unit_size is below
 * 64 >> ss_x (4:4:0 chroma with halved units) the processing units are unit_size wide, as the reference walks them inside each restoration unit. */
typedef struct SvtHipLrParams {
    const void *data;            /* CDEF output plane */
    const void *boundary_above;  /* rsb->stripe_boundary_above: rows 2*stripe, 2*stripe+1 */
    const void *boundary_below;
    void       *dst;
    uint32_t stride, boundary_stride, dst_stride; /* pixels */
    uint32_t width, height, unit_size;
    uint8_t  ss_x, ss_y, highbd, bit_depth;
    const SvtHipLrUnit *units;   /* [vert units][horz units] */
} SvtHipLrParams;
void svt_hip_lr_filter_frame(const SvtHipLrParams *params, void *stream);
/* the same over the 64-row stripes [stripe_begin, stripe_end) only (stripe_end < 0: to the last one): one GPU's strip of a picture split over several devices */
void svt_hip_lr_filter_frame_stripes(const SvtHipLrParams *params, int stripe_begin, int stripe_end, void *stream);
/* The same from HOST memory (a seam around svt_av1_loop_restoration_filter_frame, rest_process.c:632, calls it per restored plane): every pointer of params is
 * a host pointer, boundary_above / below point at frame column 0 (past the reference's RESTORATION_EXTRA_HORZ margin), dst may equal data; synchronous. */
int svt_hip_lr_filter_frame_host(const SvtHipLrParams *params);
/* The per-unit half of the loop-restoration SEARCH of one plane (restoration_seg_search, restoration_pick.c:1448-1527) as one resident device stage:
 * for every restoration unit the SSE of the unrestored unit (search_norestore_seg :1409), the Wiener solve + refinement (search_wiener_seg :1281:
 * svt_av1_compute_stats -> wiener_decompose_sep_sym -> finalize_sym_filter -> compute_score -> finer_tile_search_wiener_seg) and the self-guided
 * parameter search (search_sgrproj_seg :1205: search_selfguided_restoration + the SSE with the winner) -- everything the picture-level decisions
 * (search_*_finish / rest_finish_search, serial rate decisions against the previous unit's coefficients) read from RestUnitSearchInfo.
 * scs->use_boundaries_in_rest_search is 0 (enc_handle.c:4129): trials filter the plain plane.  dgd = the plane being restored, origin at sample (0, 0),
 * edges extended by >= 3 samples (+ 1 more on the right) as restoration_seg_search leaves it (:1480-1496); units in svt_aom_foreach_rest_unit_in_frame
 * order ([vert][horz]).  All pointers device.  Results are bit-exact with the reference's functions. */
typedef struct SvtHipLrSearchParams {
    const void *dgd, *src;
    uint32_t    dgd_stride, src_stride, width, height, unit_size; /* samples */
    uint8_t     ss_y, highbd, bit_depth;
    uint8_t     wn_enabled, wiener_win, wn_use_refinement, wn_max_one_refinement_step; /* cm->wn_filter_ctrls; wiener_win resolved (7, 5 or 3: :1286-1290) */
    uint8_t     sg_enabled, sg_start_ep, sg_end_ep, sg_ep_inc, sg_refine; /* the parameter-set loop of search_selfguided_restoration, resolved (:560-579) */
    uint8_t     pad[3];
} SvtHipLrSearchParams;
typedef struct SvtHipLrSearchUnit {
    int64_t sse[3];                 /* rusi->sse[RESTORE_NONE], [RESTORE_WIENER] (INT64_MAX: filter rejected by compute_score), [RESTORE_SGRPROJ] */
    int16_t vfilter[8], hfilter[8]; /* rusi->wiener */
    int32_t ep, xqd[2];             /* rusi->sgrproj */
    int32_t pad;
} SvtHipLrSearchUnit;
typedef struct SvtHipLrPrevUnit { /* wn_filter_ctrls.use_prev_frame_coeffs (:1297-1302): the co-located unit of the previous frame was RESTORE_WIENER */
    int32_t use;
    int16_t vfilter[8], hfilter[8];
} SvtHipLrPrevUnit;
size_t svt_hip_lr_search_workspace(const SvtHipLrSearchParams *params); /* bytes (includes 8 B per sample and self-guided parameter set searched) */
/* prev: device, [units] or NULL.  Waits on the device internally (the lock-step Wiener refinement reads the number of units still searching back every
 * few rounds, through an event on its own side stream).  Returns 0, -1 for parameters outside the reference's ranges, or -2 when the lock-step Wiener refinement hit its 4096-step cap with units
 * still searching (results of the plane must then not be used; the reference's own loops are bounded far below that).  sse[1] / sse[2] of a tool that is
 * disabled (wn_enabled / sg_enabled == 0) are 0 and carry no meaning: callers read them only for enabled tools (as integration/rest_process_seam.c does). */
int svt_hip_lr_search_plane(const SvtHipLrSearchParams *params, const SvtHipLrPrevUnit *prev, SvtHipLrSearchUnit *units, void *workspace, void *stream);
/* The same from HOST planes (what a seam around restoration_seg_search, rest_process.c:612, calls once per plane): dgd / src / prev / units are host pointers,
 * dgd readable 3 rows above / below and 3 (left) / 4 (right) samples beside the plane; uploads, runs on the calling thread's stream, downloads. */
int svt_hip_lr_search_plane_host(const SvtHipLrSearchParams *params, const SvtHipLrPrevUnit *prev, SvtHipLrSearchUnit *units);

/* RTCD-signature single-call forms (common_dsp_rtcd.h:144-181); highbd pointers use the CONVERT_TO_BYTEPTR convention.
 * SvtHipConvolveParams is ConvolveParams (definitions.h:572-585); the Wiener path reads round_0 / round_1 only (convolve.c:100-147). */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef ConvolveParams SvtHipConvolveParams;
#else
typedef struct SvtHipConvolveParams {
    int32_t   ref, do_average;
    uint16_t *dst; /* ConvBufType */
    int32_t   dst_stride, round_0, round_1, plane, is_compound, use_jnt_comp_avg, fwd_offset, bck_offset, use_dist_wtd_comp_avg;
} SvtHipConvolveParams;
#endif
/* the three d16 forms of the masked compound (csrc/maskpred.hip; common_dsp_rtcd.h:103-104, :234-237 -> blend_a64_mask.c:34, :105, C_DEFAULT/inter_prediction_c.c:30).
 * Host pointers; src0 / src1 are ConvBufType (uint16_t) blocks; round_0 / round_1 are read from conv_params.  ACCEPTED RANGE, outside of which nothing is written: the
 * roundings as for the jnt_ forms (0 <= round_0 <= 7, 0 <= round_1 <= 7, sum <= 14); w, h powers of two 4 .. 128 and subw, subh 0 / 1 in the blend forms, w, h 1 .. 128
 * and strides >= w in the builder; mask_type 0 / 1; bd 8 / 10 / 12.  The highbd blend form writes uint16_t samples through its uint8_t pointer, as the reference's. */
void svt_aom_lowbd_blend_a64_d16_mask_hip(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride, const uint16_t *src1, uint32_t src1_stride,
                                          const uint8_t *mask, uint32_t mask_stride, int w, int h, int subw, int subh, SvtHipConvolveParams *conv_params);
void svt_aom_highbd_blend_a64_d16_mask_hip(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride, const uint16_t *src1, uint32_t src1_stride,
                                           const uint8_t *mask, uint32_t mask_stride, int w, int h, int subx, int suby, SvtHipConvolveParams *conv_params,
                                           const int bd);
void svt_av1_build_compound_diffwtd_mask_d16_hip(uint8_t *mask, uint8_t mask_type, const uint16_t *src0, int src0_stride, const uint16_t *src1, int src1_stride, int h,
                                                 int w, SvtHipConvolveParams *conv_params, int bd);
/* the two warp forms (csrc/warp.hip; common_dsp_rtcd.h:1032, :1035; exported, NOT installed by svt_hip_setup_rtcd: INTEGRATION.md).  Host pointers.  The forms honour
 * conv_params->round_0 / round_1 / is_compound / do_average / use_jnt_comp_avg / fwd_offset / bck_offset / dst / dst_stride as the C does: is_compound with
 * do_average == 0 writes the ConvBufType buffer and leaves pred untouched.  The high-bit-depth form packs (ref8b << 2) | ((ref2b >> 6) & 3).  Only the sample
 * rectangle the call can read after clamping is copied to the device, never a sample outside width x height.  ACCEPTED RANGE, outside of which nothing is written:
 * the roundings as for the jnt_ forms (0 <= round_0 <= 7, round_1 >= 0, round_0 + round_1 <= 14, round_1 <= 7 when is_compound); p_width, p_height 1 .. 128; the
 * conditions of svt_hip_warp_pred_batch on sub-sampling, bounds, shear and the int32_t range; bd 10 or 12 in the highbd form. */
void svt_av1_warp_affine_hip(const int32_t *mat, const uint8_t *ref, int width, int height, int stride, uint8_t *pred, int p_col, int p_row, int p_width,
                             int p_height, int p_stride, int subsampling_x, int subsampling_y, SvtHipConvolveParams *conv_params, int16_t alpha, int16_t beta,
                             int16_t gamma, int16_t delta);
void svt_av1_highbd_warp_affine_hip(const int32_t *mat, const uint8_t *ref8b, const uint8_t *ref2b, int width, int height, int stride8b, int stride2b,
                                    uint16_t *pred, int p_col, int p_row, int p_width, int p_height, int p_stride, int subsampling_x, int subsampling_y, int bd,
                                    SvtHipConvolveParams *conv_params, int16_t alpha, int16_t beta, int16_t gamma, int16_t delta);
/* the two scaled-convolve forms (csrc/scale.hip; common_dsp_rtcd.h: svt_av1_convolve_2d_scale, svt_av1_highbd_convolve_2d_scale; exported, NOT installed by
 * svt_hip_setup_rtcd: INTEGRATION.md).  Host pointers; the 16 x 8 taps are read from filter_ptr of the caller's InterpFilterParams (taps must be 8; any values) and
 * conv_params->round_0 / round_1 / is_compound / do_average / use_dist_wtd_comp_avg / fwd_offset / bck_offset / dst / dst_stride are honoured as the C does:
 * is_compound with do_average == 0 writes the ConvBufType buffer and leaves dst untouched.  Only the rectangle the C reads is copied to the device: columns
 * -3 .. (((w - 1) * x_step_qn + subpel_x_qn) >> 10) + 4, rows likewise.  ACCEPTED RANGE, outside of which nothing is written: w, h powers of two 2 .. 128; phases
 * 0 .. 1023; steps 64 .. 2048; the roundings as for the jnt_ forms (0 <= round_0 <= 7, round_1 >= 0, round_0 + round_1 <= 14, round_1 <= 7 when is_compound); bd 10
 * or 12 in the highbd form. */
void svt_av1_convolve_2d_scale_hip(const uint8_t *src, int src_stride, uint8_t *dst, int dst_stride, int w, int h, const SvtHipInterpFilterParams *filter_params_x,
                                   const SvtHipInterpFilterParams *filter_params_y, const int subpel_x_qn, const int x_step_qn, const int subpel_y_qn,
                                   const int y_step_qn, SvtHipConvolveParams *conv_params);
void svt_av1_highbd_convolve_2d_scale_hip(const uint16_t *src, int src_stride, uint16_t *dst, int dst_stride, int w, int h,
                                          const SvtHipInterpFilterParams *filter_params_x, const SvtHipInterpFilterParams *filter_params_y, const int subpel_x_qn,
                                          const int x_step_qn, const int subpel_y_qn, const int y_step_qn, SvtHipConvolveParams *conv_params, int bd);
/* the sixteen inter-prediction forms (csrc/interpred.hip; described with svt_hip_inter_pred_batch above) */
#define SVT_HIP_DECLARE_CONVOLVE(name)                                                                                                                               \
    void svt_av1_##name##_hip(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w, int32_t h,                                        \
                              SvtHipInterpFilterParams *filter_params_x, SvtHipInterpFilterParams *filter_params_y, const int32_t subpel_x_q4,                       \
                              const int32_t subpel_y_q4, SvtHipConvolveParams *conv_params);                                                                         \
    void svt_av1_highbd_##name##_hip(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride, int32_t w, int32_t h,                               \
                                     const SvtHipInterpFilterParams *filter_params_x, const SvtHipInterpFilterParams *filter_params_y,                              \
                                     const int32_t subpel_x_q4, const int32_t subpel_y_q4, SvtHipConvolveParams *conv_params, int32_t bd);
SVT_HIP_DECLARE_CONVOLVE(convolve_2d_copy_sr)
SVT_HIP_DECLARE_CONVOLVE(convolve_x_sr)
SVT_HIP_DECLARE_CONVOLVE(convolve_y_sr)
SVT_HIP_DECLARE_CONVOLVE(convolve_2d_sr)
SVT_HIP_DECLARE_CONVOLVE(jnt_convolve_2d_copy)
SVT_HIP_DECLARE_CONVOLVE(jnt_convolve_x)
SVT_HIP_DECLARE_CONVOLVE(jnt_convolve_y)
SVT_HIP_DECLARE_CONVOLVE(jnt_convolve_2d)
#undef SVT_HIP_DECLARE_CONVOLVE
void svt_av1_wiener_convolve_add_src_hip(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst, ptrdiff_t dst_stride, const int16_t *filter_x,
                                         const int16_t *filter_y, int32_t w, int32_t h, const SvtHipConvolveParams *conv_params);
void svt_av1_highbd_wiener_convolve_add_src_hip(const uint8_t *src8, ptrdiff_t src_stride, uint8_t *dst8, ptrdiff_t dst_stride,
                                                const int16_t *filter_x, const int16_t *filter_y, int32_t w, int32_t h,
                                                const SvtHipConvolveParams *conv_params, int32_t bd);
void svt_av1_selfguided_restoration_hip(const uint8_t *dgd8, int32_t width, int32_t height, int32_t dgd_stride, int32_t *flt0, int32_t *flt1,
                                        int32_t flt_stride, int32_t sgr_params_idx, int32_t bit_depth, int32_t highbd);
void svt_apply_selfguided_restoration_hip(const uint8_t *dat8, int32_t width, int32_t height, int32_t stride, int32_t eps, const int32_t *xqd,
                                          uint8_t *dst8, int32_t dst_stride, int32_t *tmpbuf, int32_t bit_depth, int32_t highbd);

/* ---------------------------------------------------------------- SATD / Hadamard (a8, a9), LR search statistics (a24) ------ */
typedef struct SvtHipSatdDesc {
    uint64_t in_off, pred_off;       /* elements from input_base / pred_base */
    uint32_t in_stride, pred_stride;
} SvtHipSatdDesc;
/* n transform blocks of tx_n x tx_n (4, 8, 16, 32) 8-bit pixels: residual -> svt_aom_hadamard_NxN -> svt_aom_satd, i.e. the body
 * of hadamard_path_c (enc_mode_config.c:2147-2215).  satd_out[n]; coeff_out (optional) [n][tx_n^2] in the reference's order. */
void svt_hip_hadamard_satd_batch(const uint8_t *input_base, const uint8_t *pred_base, const SvtHipSatdDesc *descs, uint32_t n, int tx_n,
                                 uint32_t *satd_out, int32_t *coeff_out, void *stream);
typedef struct SvtHipRect { int32_t h_start, h_end, v_start, v_end; } SvtHipRect;
/* n restoration units: Wiener auto/cross-correlation M[n][49], H[n][49*49] (only win^2 / win^4 entries used),
 * svt_av1_compute_stats_c / _highbd_c (restoration_pick.c:659-745).  dgd needs a (win/2)-pixel readable border.  max_rect_width / height =
 * the largest unit of the batch (sizes the launch; the rects themselves stay on the device).  Runs on the matrix cores (int8 digit split,
 * int32 / int64 accumulation: exact). */
void svt_hip_lr_compute_stats_batch(const void *dgd, const void *src, const SvtHipRect *rects, uint32_t n, int max_rect_width, int max_rect_height,
                                    int dgd_stride, int src_stride, int wiener_win, int bit_depth, int64_t *M, int64_t *H, void *stream);
/* the same with the sample size stated (1 or 2 bytes) instead of derived from the bit depth: the reference's highbd function takes 16-bit pictures at every bit depth,
 * 8 included (an 8-bit encode in the 16-bit pipeline; av1_compute_stats_test_hbd runs it at EB_EIGHT_BIT, test/RestorationPickTest.cc:576-583).  The form above is
 * this one with sample_bytes = bit_depth > 8 ? 2 : 1. */
void svt_hip_lr_compute_stats_batch_samples(const void *dgd, const void *src, const SvtHipRect *rects, uint32_t n, int max_rect_width, int max_rect_height,
                                            int dgd_stride, int src_stride, int wiener_win, int bit_depth, int sample_bytes, int64_t *M, int64_t *H, void *stream);
/* single-call forms (aom_dsp_rtcd.h:62-81,210-215,276; common_dsp_rtcd.h:1075-1087) */
int      svt_aom_satd_hip(const int32_t *coeff, int length);
void     svt_aom_hadamard_nxn_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff, int n);
void     svt_aom_hadamard_4x4_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff);
void     svt_aom_hadamard_8x8_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff);
void     svt_aom_hadamard_16x16_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff);
void     svt_aom_hadamard_32x32_hip(const int16_t *src_diff, ptrdiff_t src_stride, int32_t *coeff);
uint32_t svt_hadamard_path_hip(const uint8_t *input, uint32_t in_stride, const uint8_t *pred, uint32_t pred_stride, int block_size);
/* hadamard_path (aom_dsp_rtcd.h:582) -> hadamard_path_c (enc_mode_config.c:2147-2215), exact prototype: four Buf2D BY VALUE (definitions.h:243-249; residual and
 * coeff are scratch there) and the one-byte packed enum BlockSize (definitions.h:764-791).  Unpacks and calls svt_hadamard_path_hip. */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef Buf2D SvtHipBuf2D;
#else
typedef struct SvtHipBuf2D { uint8_t *buf, *buf0; int width, height, stride; } SvtHipBuf2D;
#endif
uint32_t hadamard_path_hip(SvtHipBuf2D residual, SvtHipBuf2D coeff, SvtHipBuf2D input, SvtHipBuf2D pred, SvtHipBlockSize bsize);
void     svt_residual_kernel8bit_hip(uint8_t *input, uint32_t input_stride, uint8_t *pred, uint32_t pred_stride, int16_t *residual,
                                     uint32_t residual_stride, uint32_t area_width, uint32_t area_height);
void     svt_residual_kernel16bit_hip(uint16_t *input, uint32_t input_stride, uint16_t *pred, uint32_t pred_stride, int16_t *residual,
                                      uint32_t residual_stride, uint32_t area_width, uint32_t area_height);
/* SvtHipSgrParams is SgrParamsType (definitions.h:1750-1753).  `bit_depth` of svt_av1_compute_stats_highbd is the enum EbBitDepth (EbSvtAv1Formats.h:101-108), which
 * gcc and clang give the type unsigned int. */
#ifdef SVT_HIP_REFERENCE_TYPES
typedef SgrParamsType SvtHipSgrParams;
#else
typedef struct SvtHipSgrParams { int32_t r[2], s[2]; } SvtHipSgrParams;
#endif
void     svt_av1_compute_stats_hip(int32_t wiener_win, const uint8_t *dgd, const uint8_t *src, int32_t h_start, int32_t h_end, int32_t v_start,
                                   int32_t v_end, int32_t dgd_stride, int32_t src_stride, int64_t *M, int64_t *H);
void     svt_av1_compute_stats_highbd_hip(int32_t wiener_win, const uint8_t *dgd8, const uint8_t *src8, int32_t h_start, int32_t h_end,
                                          int32_t v_start, int32_t v_end, int32_t dgd_stride, int32_t src_stride, int64_t *M, int64_t *H,
                                          unsigned int bit_depth);
int64_t  svt_av1_lowbd_pixel_proj_error_hip(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8,
                                            int32_t dat_stride, int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride,
                                            int32_t xq[2], const SvtHipSgrParams *params);
int64_t  svt_av1_highbd_pixel_proj_error_hip(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8,
                                             int32_t dat_stride, int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride,
                                             int32_t xq[2], const SvtHipSgrParams *params);
void     svt_get_proj_subspace_hip(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride,
                                   int32_t use_highbitdepth, int32_t *flt0, int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t *xq,
                                   const SvtHipSgrParams *params);

/* ------------------------------------------------ TPL dispenser, source-based half ---------------------------------------------
 * tpl_mc_flow_dispenser_sb_generic (Codec/src_ops_process.c:519-969), the part that runs when pcs->tpl_src_data_ready == 0: per 16x16 (dispenser level 0) or
 * 32x32 (level 1; complete 64x64 SBs only, :2048-2051) block of a picture the DC intra cost from SOURCE neighbours (:620-657), the SAD of every
 * uni-directional ME candidate against its reference's source picture at the clamped full-pel vector (:761-890), the winner (:892) and, for NEWMV, the forward
 * transform (N2 / N4 shape, rows subsampled by 1 << subsample_tx) + svt_av1_quantize_fp reconstruction error of its residual (get_quantize_error, :224-247).
 * Output = exactly the TplSrcStats the reference stores per 16x16 cell (:958-967), which its own "else" branch (:969-977) consumes: a seam around
 * tpl_mc_flow_dispenser (:1848) fills pa_me_data->tpl_src_stats_buffer from one call per picture and lets the reference run the reconstruction half.
 * Covered option sets: tpl levels 4 and 5 of set_tpl_params (initial_rc_process.c:343-378: every preset from M3 up) -- use_sad_in_src_search = 1, intra_mode_end = DC_PRED,
 * subpel_depth = FULL_PEL, compute_rate = 0 -- with intra_mode_end = search_flags = 0, and tpl levels 0-3 (:301-342; level 1 = presets M0-M2: every intra mode, transform +
 * SATD costs, quarter-pel vectors, rate; 16x16 blocks only) through those two fields (csrc/tpl_full.hip).  scs->in_loop_ois = 1; the caller must run the reference's C for
 * anything else (the host forms return -1).  8-bit pictures (the reference's TPL is 8-bit only: "10BIT not supported", :464). */
typedef struct SvtHipTplRef {           /* one per rf_idx = list * 4 + ref_idx (= svt_get_ref_frame_type(list, ref_idx) - 1, :783) */
    uint64_t plane_off;                 /* bytes from ref_base to the reference picture's buffer_y (tpl_ref_ds_ptr_array[list][ref].picture_ptr: input_padded_pic, :141) */
    uint64_t picture_number;            /* tpl_ref_ds_ptr_array[list][ref].picture_number */
    uint32_t stride, org_x, org_y;      /* stride_y, org_x, org_y of that picture */
    uint16_t max_width, max_height;     /* its max_width / max_height (the vector clamp, :791-801) */
    uint8_t  valid;                     /* 0: no such reference, or excluded: ref_tpl_group_idx > 0 && !base_pcs->tpl_valid_pic[idx] (:779-781) */
    uint8_t  pad[3];
} SvtHipTplRef;
typedef struct SvtHipTplSrcParams {
    uint32_t width, height;             /* pcs->enhanced_pic->width / height */
    uint32_t aligned_width;             /* pcs->aligned_width: the statistics grid is ((aligned_width + 15) >> 4) cells wide (:552) */
    uint32_t sbs_x, n_sb;               /* 64x64 SB grid of scs->b64_geom (raster); SBs cut by the aligned picture run at dispenser level 0 */
    uint32_t src_stride;                /* enhanced_pic->stride_y */
    uint64_t src_off;                   /* bytes from src_base to picture sample (0, 0) of enhanced_pic */
    uint8_t  dispenser_search_level;    /* tpl_ctrls: 0 = 16x16 blocks, 1 = 32x32 */
    uint8_t  subsample_tx;              /* 0, 1, 2: the transform sees every (1 << subsample_tx)-th row */
    uint8_t  pf_shape;                  /* EB_TRANS_COEFF_SHAPE: 0 DEFAULT, 1 N2, 2 N4 */
    uint8_t  disable_intra_pred;        /* tpl_ctrls.disable_intra_pred_nref && temporal_layer_index == hierarchical_levels (:557) */
    uint8_t  i_slice;                   /* pcs->slice_type == I_SLICE: no ME candidates (:767) */
    uint8_t  enable_me_16x16, enable_me_8x8; /* PU count of the ME tables: 85 / 21 / 5 */
    uint8_t  max_cand, max_refs, max_l0; /* pa_me_data */
    uint8_t  intra_mode_end;            /* tpl_ctrls.intra_mode_end: DC_PRED (0) .. PAETH_PRED (12) */
    uint8_t  search_flags;              /* bit 0: !use_sad_in_src_search (transform + SATD costs), bit 1: compute_rate, bits 2-3: sub-pel rounds of tpl_subpel_search
                                           (0 FULL_PEL, 1 HALF_PEL, 2 QUARTER_PEL), bit 4: subpel_diag_refinement == 4.  Both 0 = tpl levels 4 / 5 (the fast kernels);
                                           anything else = the option set of tpl levels 0-3 (csrc/tpl_full.hip; 16x16 blocks, subsample_tx 0) */
    int16_t  quant_fp[2], round_fp[2], dequant[2]; /* quants_8bit.y_quant_fp / y_round_fp[qIndex], deq_8bit.y_dequant_qtx[qIndex] (DC, AC; :541-547) */
    SvtHipTplRef refs[8];
} SvtHipTplSrcParams;
typedef struct SvtHipTplSrcStats {      /* TplSrcStats (coding_unit.h:323-331) with explicit layout */
    int64_t  srcrf_dist, srcrf_rate;
    uint64_t ref_frame_poc;
    int16_t  mv_row, mv_col;            /* MV in 1/8 sample units */
    int32_t  best_rf_idx;               /* -1: no inter candidate */
    uint8_t  best_mode;                 /* PredictionMode: the best intra mode (DC_PRED 0 .. PAETH_PRED 12) or NEWMV (16) */
    uint8_t  best_intra_mode;           /* DC_PRED .. intra_mode_end */
    uint8_t  written;                   /* 1 for cells the reference writes (at least half of the block inside the picture, :580), else the cell is left untouched */
    uint8_t  pad[5];
} SvtHipTplSrcStats;
/* Device form: total_me_candidate_index / me_mv_array / me_candidate_array as svt_hip_me_results_batch writes them ([n_sb][n_pus], [n_sb][n_pus * max_refs],
 * [n_sb][n_pus * max_cand]); stats [rows16][cols16] with cols16 = (aligned_width + 15) >> 4 -- only the cells of processed blocks are written. */
void svt_hip_tpl_src_stage(const SvtHipTplSrcParams *params, const uint8_t *src_base, const uint8_t *ref_base, const uint8_t *total_me_candidate_index,
                           const uint32_t *me_mv_array, const uint8_t *me_candidate_array, SvtHipTplSrcStats *stats, void *stream);
/* Host form (what the seam calls once per picture): every pointer is a host pointer.  src_buf / ref_buf[rf_idx] = start of each picture's luma buffer, *_rows the
 * rows it holds (stride x rows bytes are uploaded; references that share a buffer are uploaded once); params->src_off and refs[].plane_off are offsets INSIDE
 * those buffers.  stats: host, [rows16 * cols16], zero-filled for cells no block writes.  Returns 0, or -1 for an option set outside the covered one. */
typedef struct SvtHipTplHostPlanes {
    const uint8_t *src_buf;
    uint32_t       src_rows;
    uint32_t       ref_rows[8];
    const uint8_t *ref_buf[8];
} SvtHipTplHostPlanes;
int svt_hip_tpl_src_stage_host(const SvtHipTplSrcParams *params, const SvtHipTplHostPlanes *planes, const uint8_t *total_me_candidate_index,
                               const uint32_t *me_mv_array, const uint8_t *me_candidate_array, SvtHipTplSrcStats *stats);

/* ---- TPL dispenser, RECONSTRUCTION half (tpl_mc_flow_dispenser_sb_generic, src_ops_process.c:979-1198; same option sets) ----
 * Per block, from the statistics of the source-based half: the prediction into the picture's TPL reconstruction plane (mc_flow_rec_picture_buffer[frame_idx]) --
 * NEWMV = the block at the full-pel vector of rec_refs[best_rf_idx] (:1016-1019: the TPL reconstruction of a frame inside the sliding window, else the
 * reference's source picture), else DC from the RECONSTRUCTED neighbours (:1038-1070) --, residual against the source on the rows the transform sees -> forward
 * DCT_DCT -> svt_av1_quantize_fp -> recon_error (:1112-1131), the inverse transform onto the prediction when (is_ref or intra prediction on) and a coefficient
 * survived, skipped rows copied from the row above (:1135-1167), and the block's four statistics (:1170-1180) BEFORE result_model_store (:266), which stays the
 * caller's (it depends on synth_blk_size only).  An intra block reads its left and upper neighbours' reconstruction: the stage walks the picture's blocks by
 * anti-diagonals, one launch per diagonal (a valid order for the mixed 32x32 / 16x16 grid too: DESIGN 4.16). */
typedef struct SvtHipTplReconParams {
    SvtHipTplSrcParams src;        /* geometry, option set, quantizer row as for the source-based half (src.refs is not read) */
    SvtHipTplRef       rec_refs[8]; /* per list * 4 + ref: the plane NEWMV blocks copy from, relative to rec_ref_base (valid / picture_number / max_* are not read) */
    uint64_t           recon_off;  /* bytes from recon_base to picture sample (0, 0) of the reconstruction plane */
    uint32_t           recon_stride;
    uint8_t            is_ref;     /* pcs->tpl_data.is_ref */
    uint8_t            pad[3];
} SvtHipTplReconParams;
typedef struct SvtHipTplReconStats { /* at the block's top-left 16x16 cell */
    int64_t srcrf_dist, recrf_dist, srcrf_rate, recrf_rate;
    uint8_t written;               /* as SvtHipTplSrcStats.written */
    uint8_t coded;                 /* a coefficient survived the quantizer (eob != 0) */
    uint8_t pad[2];                /* pad[0] of a row's first cell: 0xEE = the row-wavefront form (SVT_HIP_TPL_RECON_FORM=1) gave up waiting for the row above */
    uint32_t reserved;             /* the stage's own (row progress of the row-wavefront form); meaningless afterwards */
} SvtHipTplReconStats;
/* Device form: src_stats / out [rows16][cols16] as the source-based stage writes them; recon_base is read (neighbours) and written (every processed block). */
void svt_hip_tpl_recon_stage(const SvtHipTplReconParams *params, const uint8_t *src_base, const uint8_t *rec_ref_base, const SvtHipTplSrcStats *src_stats,
                             uint8_t *recon_base, SvtHipTplReconStats *out, void *stream);
/* Host form: planes->src_buf / ref_buf[] as above with ref_buf[rf] = the buffer rec_refs[rf] lives in (only the references the statistics name are uploaded);
 * recon_buf = start of the reconstruction picture's luma buffer (recon_rows rows of recon_stride bytes: uploaded, updated, downloaded). */
int svt_hip_tpl_recon_stage_host(const SvtHipTplReconParams *params, const SvtHipTplHostPlanes *planes, const SvtHipTplSrcStats *src_stats, uint8_t *recon_buf,
                                 uint32_t recon_rows, SvtHipTplReconStats *out);
/* Both halves of tpl_mc_flow_dispenser_sb_generic (src_ops_process.c:519-1198) for one picture in ONE host call: src_planes as svt_hip_tpl_src_stage_host takes them,
 * rec_planes->ref_buf[rf] = the buffer params->rec_refs[rf] lives in (every valid reference; src_buf unused).  Every distinct buffer is uploaded once, the source-based
 * statistics stay on the device between the halves and come back in src_stats (for the caller's TplSrcStats buffer), the written rectangle of the reconstruction and
 * `out` as svt_hip_tpl_recon_stage_host returns them; one synchronisation.  Returns 0, -1 (option set not covered), -3 (a reference buffer is missing), -4 (a block
 * gave up waiting for its neighbours). */
int svt_hip_tpl_stage_host(const SvtHipTplReconParams *params, const SvtHipTplHostPlanes *src_planes, const SvtHipTplHostPlanes *rec_planes,
                           const uint8_t *total_me_candidate_index, const uint32_t *me_mv_array, const uint8_t *me_candidate_array, SvtHipTplSrcStats *src_stats,
                           uint8_t *recon_buf, uint32_t recon_rows, SvtHipTplReconStats *out);
/* The same with the planes kept RESIDENT on the device across calls.  ids names the CONTENT of every buffer (0 = do not keep): a buffer found under its (pointer, id)
 * is not uploaded again, an uploaded one stays for later calls, and the reconstruction this call produces stays under (recon_buf, ids->recon) with its borders
 * replicated as svt_aom_generate_padding replicates the host copy's after the dispenser (recon_width / height / org: the reconstruction picture's geometry).  A picture
 * of a TPL group is the source of one call and a reference of several others: with ids a call uploads one new plane instead of up to nine.
 * total_me_candidate_index == NULL: the source-based statistics are the CALLER's (src_stats is an input: an earlier TPL group's, src_ops_process.c:969-977) and only
 * the reconstruction half runs.  svt_hip_tpl_plane_drop(buffer): the host rewrote that buffer by other means -- forget what the device holds of it. */
typedef struct SvtHipTplPlaneIds {
    uint64_t src, src_ref[8], rec_ref[8], recon;
    uint32_t recon_width, recon_height, recon_org_x, recon_org_y;
} SvtHipTplPlaneIds;
int  svt_hip_tpl_stage_host_resident(const SvtHipTplReconParams *params, const SvtHipTplHostPlanes *src_planes, const SvtHipTplHostPlanes *rec_planes,
                                     const SvtHipTplPlaneIds *ids, const uint8_t *total_me_candidate_index, const uint32_t *me_mv_array, const uint8_t *me_candidate_array,
                                     SvtHipTplSrcStats *src_stats, uint8_t *recon_buf, uint32_t recon_rows, SvtHipTplReconStats *out);
void svt_hip_tpl_plane_drop(const void *host_buffer);
void svt_hip_tpl_plane_counts(uint64_t *hits, uint64_t *misses); /* resident-plane look-ups of the calling thread's device so far */

/* ---- ONE picture over several GPUs from a C host (the frame-partition case; csrc/partition.hip) ----
 * devices[0] = the HOME device: every pointer of the calls below lives there and `stream` belongs to it.  Each call is the batched primitive of the same name cut
 * into contiguous strips (ME: descriptor ranges = bands of SB rows; CDEF: filter-block rows; LR: 64-row stripes), strip k on devices[k]: the inputs are copied home ->
 * k (hipMemcpyPeerAsync, xGMI inside a node), the strip runs on k, its output rows are copied back into the caller's arrays exactly where the single-device call
 * writes them; the call returns with everything enqueued (the home stream waits for the peers).  Results are bit-identical to the single-device call.  A partition
 * is used by one host thread at a time.  create returns NULL for an empty / repeated / unavailable device list. */
void *svt_hip_frame_partition_create(const int *devices, int n);
void  svt_hip_frame_partition_destroy(void *partition);
int   svt_hip_frame_partition_size(const void *partition);
/* Test instruments.  svt_hip_debug_spin: a delay kernel of about `microseconds` (at most 100 ms) on `stream`.  svt_hip_frame_partition_set_jitter: from now on every
 * call of this partition puts delays of pseudo-random length (0 .. max_us, seeded) between the steps of its protocol on the home and the peer streams; 0 = off. */
void  svt_hip_debug_spin(void *stream, uint32_t microseconds);
void  svt_hip_frame_partition_set_jitter(void *partition, uint32_t seed, uint32_t max_us);
void  svt_hip_frame_partition_stats(const void *partition, uint64_t *calls, uint64_t *peer_bytes_in, uint64_t *peer_bytes_out);
/* svt_hip_me_fullpel_search_batch over items [0, n): src_bytes / ref_bytes = the extent of the plane sets behind src_base / ref_base (mirrored whole) */
int   svt_hip_frame_partition_me(void *partition, const uint8_t *src_base, size_t src_bytes, const uint8_t *ref_base, size_t ref_bytes, const SvtHipMeSearchDesc *descs,
                                 uint32_t n, uint32_t max_w, uint32_t max_h, int sub_sad, uint32_t *best_sad, uint32_t *best_mv, void *workspace, void *stream);
/* svt_hip_cdef_frame (modes 0 / 1 / 2) */
int   svt_hip_frame_partition_cdef(void *partition, int mode, const SvtHipCdefParams *params, void *stream);
/* svt_hip_lr_filter_frame */
int   svt_hip_frame_partition_lr(void *partition, const SvtHipLrParams *params, void *stream);
/* The host forms' switch: with n > 1 devices set, svt_hip_cdef_apply_host / svt_hip_cdef_search_host / svt_hip_lr_filter_frame_host run their frame launches through a
 * partition of the calling thread (home = devices[0], which must be the thread's device; other threads keep the single-device path); n <= 1 switches it off.
 * The binding of the reference encoder sets it from SVT_HIP_STRIPS=<d0,d1,...>.  Returns 0, or -1 for an invalid list. */
int   svt_hip_set_frame_partition(const int *devices, int n);
unsigned long long svt_hip_frame_partition_host_calls(void); /* frame launches of host forms that went through a partition so far */

/* ---- the fixed-size symbols of the RTCD tables (what svt_hip_setup_rtcd installs): thin aliases of the generic forms above, declared here so that a caller can
 * also bind them by name.  Prototypes as the reference's pointers (aom_dsp_rtcd.h / common_dsp_rtcd.h). ---- */
#define SVT_HIP_FOR_ALL_SAD_SIZES(X)                                                                                                              \
    X(128, 128) X(128, 64) X(64, 128) X(64, 64) X(64, 32) X(32, 64) X(32, 32) X(32, 16) X(16, 32) X(16, 16) X(16, 8) X(8, 16) X(8, 8) X(8, 4) X(4, 8) \
    X(4, 4) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)
#define SVT_HIP_SAD_DECL(W, H)                                                                                              \
    uint32_t svt_aom_sad##W##x##H##_hip(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);            \
    void     svt_aom_sad##W##x##H##x4d_hip(const uint8_t *src, int src_stride, const uint8_t *const ref_array[], int ref_stride, uint32_t *sad_array);
SVT_HIP_FOR_ALL_SAD_SIZES(SVT_HIP_SAD_DECL)
#undef SVT_HIP_SAD_DECL
#define SVT_HIP_FOR_ALL_TX_SIZES(X)                                                                                                                \
    X(4, 4) X(8, 8) X(16, 16) X(32, 32) X(64, 64) X(4, 8) X(8, 4) X(8, 16) X(16, 8) X(16, 32) X(32, 16) X(32, 64) X(64, 32) X(4, 16) X(16, 4) X(8, 32) \
    X(32, 8) X(16, 64) X(64, 16)
#define SVT_HIP_FWD_DECL(W, H)                                                                                                        \
    void svt_av1_fwd_txfm2d_##W##x##H##_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd);           \
    void svt_av1_fwd_txfm2d_##W##x##H##_N2_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd);        \
    void svt_av1_fwd_txfm2d_##W##x##H##_N4_hip(int16_t *input, int32_t *output, uint32_t stride, uint8_t tx_type, uint8_t bd);
SVT_HIP_FOR_ALL_TX_SIZES(SVT_HIP_FWD_DECL)
#undef SVT_HIP_FWD_DECL
/* inverse: squares (input, r, stride_r, w, stride_w, tx_type, bd); 4x8 / 8x4 / 4x16 / 16x4 add tx_size; the rest add tx_size, eob (common_dsp_rtcd.h:106-116) */
#define SVT_HIP_INV_SQ_DECL(N) \
    void svt_av1_inv_txfm2d_add_##N##x##N##_hip(const int32_t *in, uint16_t *r, int32_t sr, uint16_t *w, int32_t sw, uint8_t tx_type, int32_t bd);
#define SVT_HIP_INV_R1_DECL(W, H) \
    void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *in, uint16_t *r, int32_t sr, uint16_t *w, int32_t sw, uint8_t tx_type, uint8_t tx_size, int32_t bd);
#define SVT_HIP_INV_R2_DECL(W, H) \
    void svt_av1_inv_txfm2d_add_##W##x##H##_hip(const int32_t *in, uint16_t *r, int32_t sr, uint16_t *w, int32_t sw, uint8_t tx_type, uint8_t tx_size, int32_t eob, int32_t bd);
SVT_HIP_INV_SQ_DECL(4) SVT_HIP_INV_SQ_DECL(8) SVT_HIP_INV_SQ_DECL(16) SVT_HIP_INV_SQ_DECL(32) SVT_HIP_INV_SQ_DECL(64)
SVT_HIP_INV_R1_DECL(4, 8) SVT_HIP_INV_R1_DECL(8, 4) SVT_HIP_INV_R1_DECL(4, 16) SVT_HIP_INV_R1_DECL(16, 4)
SVT_HIP_INV_R2_DECL(8, 16) SVT_HIP_INV_R2_DECL(16, 8) SVT_HIP_INV_R2_DECL(16, 32) SVT_HIP_INV_R2_DECL(32, 16) SVT_HIP_INV_R2_DECL(32, 64) SVT_HIP_INV_R2_DECL(64, 32)
SVT_HIP_INV_R2_DECL(8, 32) SVT_HIP_INV_R2_DECL(32, 8) SVT_HIP_INV_R2_DECL(16, 64) SVT_HIP_INV_R2_DECL(64, 16)
#undef SVT_HIP_INV_SQ_DECL
#undef SVT_HIP_INV_R1_DECL
#undef SVT_HIP_INV_R2_DECL
/* the ten quantizer pointers (aom_dsp_rtcd.h: svt_aom_quantize_b ... svt_av1_highbd_quantize_fp_qm) and the ten svt_handle_transformWxH[_N2_N4] */
#define SVT_HIP_QARGS                                                                                                                       \
    const int32_t *coeff_ptr, intptr_t n_coeffs, const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr,                \
        const int16_t *quant_shift_ptr, int32_t *qcoeff_ptr, int32_t *dqcoeff_ptr, const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, \
        const int16_t *iscan
void svt_aom_quantize_b_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, const int32_t log_scale);
void svt_aom_highbd_quantize_b_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, const int32_t log_scale);
void svt_av1_quantize_fp_hip(SVT_HIP_QARGS);
void svt_av1_quantize_fp_32x32_hip(SVT_HIP_QARGS);
void svt_av1_quantize_fp_64x64_hip(SVT_HIP_QARGS);
void svt_av1_quantize_fp_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale);
void svt_av1_highbd_quantize_fp_hip(SVT_HIP_QARGS, int16_t log_scale);
void svt_av1_highbd_quantize_fp_qm_hip(SVT_HIP_QARGS, const uint8_t *qm_ptr, const uint8_t *iqm_ptr, int16_t log_scale);
#undef SVT_HIP_QARGS
#define SVT_HIP_HT_DECL(W, H)                                   \
    uint64_t svt_handle_transform##W##x##H##_hip(int32_t *output); \
    uint64_t svt_handle_transform##W##x##H##_N2_N4_hip(int32_t *output);
SVT_HIP_HT_DECL(64, 64) SVT_HIP_HT_DECL(32, 64) SVT_HIP_HT_DECL(64, 32) SVT_HIP_HT_DECL(16, 64) SVT_HIP_HT_DECL(64, 16)
#undef SVT_HIP_HT_DECL

#ifdef __cplusplus
}
#endif
#endif /* SVTAV1_HIP_H */
