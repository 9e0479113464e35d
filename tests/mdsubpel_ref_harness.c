/* mdsubpel_ref_harness.c -- TEST INFRASTRUCTURE: reaches the reference's two sub-pel searches with flat arguments.
 *
 * Compiled by tests/test_mdsubpel_ref.py (CPU, needs the reference's sources) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so; the reference's headers are included WHERE THEY LIE (nothing is copied).  harness_md_subpel fills SUBPEL_MOTION_SEARCH_PARAMS as
 * md_subpel_search does (product_coding_loop.c:2631-2743) and calls svt_av1_find_best_sub_pixel_tree / _tree_pruned:
 *   use_ctx 0  ictx = NULL.  The ctx-dependent part of the tree search (mcomp.c:710-727) is restated here from the same flat inputs: the centre error, the round
 *              reduction, expressed as the forced_stop that gives that round; fp_me_dist is the centre error computed here.
 *   use_ctx 1  a zeroed ModeDecisionContext with pd_pass = PD_PASS_1, the mvp controls and tables set, search_stage = SPEL_ME: the reference's own lines run, and
 *              fp_me_dist is what they store. */
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "mcomp.h"
#include "md_process.h"
#include "aom_dsp_rtcd.h"

void init_fn_ptr(void);

void harness_init(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0); /* every dispatch pointer = its C function */
    init_fn_ptr();                  /* svt_aom_mefn_ptr from those pointers */
}

/* the same with the dispatch pointers of a CPU feature mask (tools/mdsubpel_timing.py: the reference's SIMD functions) */
void harness_init_flags(uint64_t flags) {
    svt_aom_setup_common_rtcd_internal(flags);
    svt_aom_setup_rtcd_internal(flags);
    init_fn_ptr();
}

enum { P_START_R, P_START_C, P_REF_R, P_REF_C, P_CMIN, P_CMAX, P_RMIN, P_RMAX, P_ALLOW_HP, P_FORCED_STOP, P_ITERS, P_PRED_VAR_TH, P_ABS_TH_MULT, P_ROUND_DEV_TH,
       P_SKIP_DIAG, P_SEARCH_TYPE, P_BIAS_FP, P_QP, P_EARLY_EXIT, P_COST_TYPE, P_EPB, P_EARLY_EXIT_TH, P_MVP_TH, P_HP_MV_TH, P_MVP_ERR, P_MVP_R, P_MVP_C, P_COUNT };

int harness_param_count(void) { return P_COUNT; }

/* ref points at the block's position in the reference (vector 0, 0); mvcost0 / mvcost1 at the CENTRE of their tables, or all three NULL.
 * out: mv_row, mv_col, besterr, distortion, sse1, fp_me_dist */
void harness_md_subpel(int method, int use_ctx, uint8_t *src, int src_stride, uint8_t *ref, int ref_stride, int bsize, const int *ip, const int *mvjcost,
                       const int *mvcost0, const int *mvcost1, int *out) {
    SUBPEL_MOTION_SEARCH_PARAMS ms;
    MacroBlockD                 xd;
    struct svt_buf_2d           ref_struct, src_struct;
    MV                          ref_mv, start_mv, best_mv;
    memset(&ms, 0, sizeof(ms));
    memset(&xd, 0, sizeof(xd));
    ref_mv.row = (int16_t)ip[P_REF_R], ref_mv.col = (int16_t)ip[P_REF_C];
    start_mv.row = (int16_t)ip[P_START_R], start_mv.col = (int16_t)ip[P_START_C];
    ms.search_stage           = SPEL_ME;
    ms.allow_hp               = ip[P_ALLOW_HP];
    ms.forced_stop            = (SUBPEL_FORCE_STOP)ip[P_FORCED_STOP];
    ms.iters_per_step         = ip[P_ITERS];
    ms.mv_limits.col_min      = ip[P_CMIN], ms.mv_limits.col_max = ip[P_CMAX], ms.mv_limits.row_min = ip[P_RMIN], ms.mv_limits.row_max = ip[P_RMAX];
    ms.mv_cost_params.ref_mv  = &ref_mv;
    ms.mv_cost_params.mv_cost_type  = (MV_COST_TYPE)ip[P_COST_TYPE];
    ms.mv_cost_params.mvjcost       = mvjcost;
    ms.mv_cost_params.mvcost[0]     = mvcost0;
    ms.mv_cost_params.mvcost[1]     = mvcost1;
    ms.mv_cost_params.error_per_bit = ip[P_EPB];
    ms.mv_cost_params.early_exit_th = ip[P_EARLY_EXIT_TH];
    ms.var_params.vfp                = &svt_aom_mefn_ptr[bsize];
    ms.var_params.subpel_search_type = (SUBPEL_SEARCH_TYPE)ip[P_SEARCH_TYPE];
    ms.var_params.w                  = block_size_wide[bsize];
    ms.var_params.h                  = block_size_high[bsize];
    ms.var_params.bias_fp            = ip[P_BIAS_FP];
    memset(&ref_struct, 0, sizeof(ref_struct));
    memset(&src_struct, 0, sizeof(src_struct));
    ref_struct.buf = ref, ref_struct.stride = ref_stride;
    src_struct.buf = src, src_struct.stride = src_stride;
    ms.var_params.ms_buffers.ref = &ref_struct;
    ms.var_params.ms_buffers.src = &src_struct;
    ms.pred_variance_th     = ip[P_PRED_VAR_TH];
    ms.abs_th_mult          = (uint8_t)ip[P_ABS_TH_MULT];
    ms.round_dev_th         = ip[P_ROUND_DEV_TH];
    ms.skip_diag_refinement = (uint8_t)ip[P_SKIP_DIAG];

    /* the centre error, as svt_upsampled_setup_center_error computes it */
    unsigned int       sse;
    const uint8_t     *at      = ref + (start_mv.row >> 3) * ref_stride + (start_mv.col >> 3);
    const unsigned int var     = svt_aom_mefn_ptr[bsize].vf(at, ref_stride, src, src_stride, &sse);
    const unsigned int besterr = var + svt_aom_fp_mv_err_cost(&start_mv, &ms.mv_cost_params);

    ModeDecisionContext *ctx = NULL;
    if (use_ctx) {
        ctx = (ModeDecisionContext *)calloc(1, sizeof(*ctx));
        ctx->pd_pass                     = PD_PASS_1;
        ctx->md_subpel_me_ctrls.mvp_th   = (uint8_t)ip[P_MVP_TH];
        ctx->md_subpel_me_ctrls.hp_mv_th = ip[P_HP_MV_TH];
        ctx->best_fp_mvp_dist[0][0]      = (uint32_t)ip[P_MVP_ERR];
        ctx->best_fp_mvp_idx[0][0]       = 1;
        ctx->mvp_array[0][0][1].row = (int16_t)ip[P_MVP_R], ctx->mvp_array[0][0][1].col = (int16_t)ip[P_MVP_C];
    } else if (method == 0 && ip[P_MVP_TH] > 0) { /* mcomp.c:712-726 from the flat inputs */
        int           round     = AOMMIN(FULL_PEL - ip[P_FORCED_STOP], 3 - !ip[P_ALLOW_HP]);
        const int     mvp_err   = ip[P_MVP_ERR] + 1;
        const int     me_err    = besterr + 1;
        const int32_t deviation = ((me_err - mvp_err) * 100) / me_err;
        if (deviation >= ip[P_MVP_TH]) round = 1;
        else if (ABS(start_mv.col - ip[P_MVP_C]) > ip[P_HP_MV_TH] || ABS(start_mv.row - ip[P_MVP_R]) > ip[P_HP_MV_TH]) round = MIN(round, 2);
        ms.forced_stop = (SUBPEL_FORCE_STOP)(FULL_PEL - round);
    }
    int          distortion = 0;
    unsigned int sse1       = 0;
    const int    err = (method == 0 ? svt_av1_find_best_sub_pixel_tree : svt_av1_find_best_sub_pixel_tree_pruned)(
        ctx, &xd, NULL, &ms, start_mv, &best_mv, &distortion, &sse1, ip[P_QP], (BlockSize)bsize, (uint8_t)ip[P_EARLY_EXIT]);
    out[0] = best_mv.row, out[1] = best_mv.col, out[2] = err, out[3] = distortion, out[4] = (int)sse1;
    out[5] = ctx ? (int)ctx->fp_me_dist[0][0] : (int)besterr;
    free(ctx);
}

/* tools/mdsubpel_timing.py: items first .. first + count - 1 of a picture cut into `cols` blocks per row, source and reference with one stride, without the cost of a
 * foreign call per item.  out: 6 values per item (may be NULL) */
void harness_md_subpel_many(int method, uint8_t *src, uint8_t *ref, int stride, int bsize, const int *ip, int cols, int first, int count, int *out) {
    int       tmp[6];
    const int bw = block_size_wide[bsize], bh = block_size_high[bsize];
    for (int k = first; k < first + count; k++) {
        const size_t off = (size_t)(k / cols) * bh * stride + (size_t)(k % cols) * bw;
        harness_md_subpel(method, 0, src + off, stride, ref + off, stride, bsize, ip, NULL, NULL, NULL, out ? out + 6 * (size_t)k : tmp);
    }
}
/* kind 0 vf, 1 svf, 2 svt_aom_upsampled_pred + vf through the dispatch pointers; out: the variance per item (may be NULL) */
void harness_prim_many(int kind, uint8_t *src, uint8_t *ref, int stride, int bsize, int xo, int yo, int taps, int cols, int first, int count, unsigned *out) {
    const int bw = block_size_wide[bsize], bh = block_size_high[bsize];
    DECLARE_ALIGNED(16, uint8_t, pred[MAX_SB_SQUARE]);
    MacroBlockD xd;
    MV          mv = {0, 0};
    memset(&xd, 0, sizeof(xd));
    for (int k = first; k < first + count; k++) {
        const size_t off = (size_t)(k / cols) * bh * stride + (size_t)(k % cols) * bw;
        unsigned int sse, v;
        if (kind == 0) v = svt_aom_mefn_ptr[bsize].vf(ref + off, stride, src + off, stride, &sse);
        else if (kind == 1) v = svt_aom_mefn_ptr[bsize].svf(ref + off, stride, xo, yo, src + off, stride, &sse);
        else {
            svt_aom_upsampled_pred(&xd, NULL, 0, 0, &mv, pred, bw, bh, xo, yo, ref + off, stride, taps);
            v = svt_aom_mefn_ptr[bsize].vf(pred, bw, src + off, stride, &sse);
        }
        if (out) out[k] = v;
    }
}

/* md_subpel_search :2656-2666: limits = col_min, col_max, row_min, row_max */
void harness_mv_limits(int mi_row, int mi_col, int bsize, int mi_rows, int mi_cols, int ref_mv_row, int ref_mv_col, int *limits) {
    MvLimits       mv_limits;
    SubpelMvLimits sub;
    MV             ref_mv;
    ref_mv.row = (int16_t)ref_mv_row, ref_mv.col = (int16_t)ref_mv_col;
    const int mi_width = mi_size_wide[bsize], mi_height = mi_size_high[bsize];
    mv_limits.row_min = -(((mi_row + mi_height) * MI_SIZE) + AOM_INTERP_EXTEND);
    mv_limits.col_min = -(((mi_col + mi_width) * MI_SIZE) + AOM_INTERP_EXTEND);
    mv_limits.row_max = (mi_rows - mi_row) * MI_SIZE + AOM_INTERP_EXTEND;
    mv_limits.col_max = (mi_cols - mi_col) * MI_SIZE + AOM_INTERP_EXTEND;
    svt_av1_set_mv_search_range(&mv_limits, &ref_mv);
    svt_av1_set_subpel_mv_search_range(&sub, (FullMvLimits *)&mv_limits, &ref_mv);
    limits[0] = sub.col_min, limits[1] = sub.col_max, limits[2] = sub.row_min, limits[3] = sub.row_max;
}
