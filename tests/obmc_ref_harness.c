/* obmc_ref_harness.c -- TEST INFRASTRUCTURE: reaches the reference's OBMC motion refinement with flat arguments.
 *
 * Compiled by tests/test_obmc_ref.py (CPU, needs the reference's sources) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so; the reference's headers are included WHERE THEY LIE (nothing is copied).  Three levels:
 *   harness_obmc_wsrc             the two exported callbacks svt_av1_calc_target_weighted_pred_above_c / _left_c, once per span, between the lines of the static
 *                                 driver calc_target_weighted_pred, which are written out here (clear, above, both times 64, left, source);
 *   harness_obmc_search           svt_av1_obmc_full_pixel_search and svt_av1_find_best_obmc_sub_pixel_tree_up called directly on a zeroed ModeDecisionContext /
 *                                 IntraBcContext with the members they read filled in, in the order single_motion_search calls them: every result is visible;
 *   harness_single_motion_search  single_motion_search itself on zeroed picture / context structures: its limits, its refine_level mapping, its sad / error per bit
 *                                 and its rate. */
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "mcomp.h"
#include "md_process.h"
#include "mode_decision.h"
#include "pcs.h"
#include "enc_inter_prediction.h"
#include "rd_cost.h"
#include "av1me.h"
#include "aom_dsp_rtcd.h"

#define MV_COST_WEIGHT 108 /* mode_decision.c:251, private to that file; tests/test_obmc_ref.py checks the text */

void init_fn_ptr(void);
void svt_av1_init_me_luts(void);
int  svt_av1_obmc_full_pixel_search(ModeDecisionContext *ctx, IntraBcContext *x, MV *mvp_full, int sadpb, const AomVarianceFnPtr *fn_ptr, const MV *ref_mv, MV *dst_mv,
                                    int is_second);
int  svt_av1_find_best_obmc_sub_pixel_tree_up(ModeDecisionContext *ctx, IntraBcContext *x, const AV1_COMMON *const cm, int mi_row, int mi_col, MV *bestmv, const MV *ref_mv,
                                              int allow_hp, int error_per_bit, const AomVarianceFnPtr *vfp, int forced_stop, int iters_per_step, int *mvjcost,
                                              int *mvcost[2], int *distortion, unsigned int *sse1, int is_second, int use_accurate_subpel_search);
void single_motion_search(PictureControlSet *pcs, ModeDecisionContext *ctx, ModeDecisionCandidate *cand, IntMv best_pred_mv, IntraBcContext *x, BlockSize bsize, MV *ref_mv,
                          int *rate_mv, int refine_level);

void harness_init_flags(uint64_t flags) { /* 0: every dispatch pointer = its C function */
    svt_aom_setup_common_rtcd_internal(flags);
    svt_aom_setup_rtcd_internal(flags);
    init_fn_ptr();
    svt_av1_init_me_luts();
}
void harness_init(void) { harness_init_flags(0); }

/* spans: (rel_mi, len_mi) pairs.  above / left have (0, 0) at the block's top-left sample. */
void harness_obmc_wsrc(int bsize, const uint8_t *src, int src_stride, const uint8_t *above, int above_stride, const uint8_t *left, int left_stride, int up_available,
                       int left_available, int n_above, const int *above_spans, int n_left, const int *left_spans, int32_t *wsrc_buf, int32_t *mask_buf) {
    MacroBlockD xd;
    memset(&xd, 0, sizeof(xd));
    const int bw = block_size_wide[bsize], bh = block_size_high[bsize];
    xd.n4_w = (uint8_t)(bw >> MI_SIZE_LOG2), xd.n4_h = (uint8_t)(bh >> MI_SIZE_LOG2);
    memset(wsrc_buf, 0, sizeof(int32_t) * bw * bh);
    for (int i = 0; i < bw * bh; ++i) mask_buf[i] = AOM_BLEND_A64_MAX_ALPHA;
    if (up_available) {
        struct calc_target_weighted_pred_ctxt ctxt = {mask_buf, wsrc_buf, above, above_stride, AOMMIN(bh, block_size_high[BLOCK_64X64]) >> 1};
        for (int k = 0; k < n_above; k++) svt_av1_calc_target_weighted_pred_above_c(0, &xd, above_spans[2 * k], (uint8_t)above_spans[2 * k + 1], NULL, &ctxt, 1);
    }
    for (int i = 0; i < bw * bh; ++i) wsrc_buf[i] *= AOM_BLEND_A64_MAX_ALPHA, mask_buf[i] *= AOM_BLEND_A64_MAX_ALPHA;
    if (left_available) {
        struct calc_target_weighted_pred_ctxt ctxt = {mask_buf, wsrc_buf, left, left_stride, AOMMIN(bw, block_size_wide[BLOCK_64X64]) >> 1};
        for (int k = 0; k < n_left; k++) svt_av1_calc_target_weighted_pred_left_c(0, &xd, left_spans[2 * k], (uint8_t)left_spans[2 * k + 1], NULL, &ctxt, 1);
    }
    for (int row = 0; row < bh; ++row)
        for (int col = 0; col < bw; ++col)
            wsrc_buf[row * bw + col] = src[row * src_stride + col] * AOM_BLEND_A64_MAX_ALPHA * AOM_BLEND_A64_MAX_ALPHA - wsrc_buf[row * bw + col];
}

enum { P_BEST_R, P_BEST_C, P_REF_R, P_REF_C, P_CMIN, P_CMAX, P_RMIN, P_RMAX, P_SADPB, P_EPB, P_APPROX, P_RANGE, P_DIAG, P_ALLOW_HP, P_FORCED_STOP, P_ITERS, P_SEARCH_TYPE,
       P_DO_FULL, P_DO_FRAC, P_MI_ROW, P_MI_COL, P_MI_ROWS, P_MI_COLS, P_QIDX, P_LAMBDA, P_REFINE_LEVEL, P_COUNT };
int harness_param_count(void) { return P_COUNT; }

typedef struct {
    ModeDecisionContext *ctx;
    IntraBcContext       x;
    MacroBlockD          xd;
    BlockGeom            geom;
    int                 *stack[2];
} Setup;
/* ctx: a zeroed ModeDecisionContext to (re)use, or NULL to allocate one */
static void setup(Setup *s, ModeDecisionContext *ctx, uint8_t *ref, int ref_stride, int bsize, int32_t *wsrc, int32_t *mask, const int *ip, int *mvjcost, int *mvcost0,
                  int *mvcost1) {
    memset(s, 0, sizeof(*s));
    s->ctx                               = ctx ? ctx : (ModeDecisionContext *)calloc(1, sizeof(ModeDecisionContext));
    s->geom.bsize                        = (BlockSize)bsize;
    s->ctx->blk_geom                     = &s->geom;
    s->ctx->wsrc_buf                     = wsrc;
    s->ctx->mask_buf                     = mask;
    s->ctx->obmc_ctrls.fpel_search_range = (uint8_t)ip[P_RANGE];
    s->ctx->obmc_ctrls.fpel_search_diag  = (uint8_t)ip[P_DIAG];
    s->ctx->approx_inter_rate            = (uint8_t)ip[P_APPROX];
    s->x.xd                              = &s->xd;
    s->x.xdplane[0].pre[0].buf           = ref;
    s->x.xdplane[0].pre[0].stride        = ref_stride;
    s->stack[0] = mvcost0, s->stack[1] = mvcost1;
    s->x.nmv_vec_cost  = mvjcost;
    s->x.mv_cost_stack = s->stack;
}

/* ref points at the block's position in the reference (vector 0, 0); mvcost0 / mvcost1 at the CENTRE of their tables.
 * out: mv_row, mv_col, fp_row, fp_col, thissme, besterr, distortion, sse1, rate_mv */
void harness_obmc_search(uint8_t *ref, int ref_stride, int bsize, int32_t *wsrc, int32_t *mask, const int *ip, int *mvjcost, int *mvcost0, int *mvcost1, int *out) {
    Setup s;
    setup(&s, NULL, ref, ref_stride, bsize, wsrc, mask, ip, mvjcost, mvcost0, mvcost1);
    IntraBcContext *x = &s.x;
    MV              ref_mv, best_pred;
    ref_mv.row = (int16_t)ip[P_REF_R], ref_mv.col = (int16_t)ip[P_REF_C];
    best_pred.row = (int16_t)ip[P_BEST_R], best_pred.col = (int16_t)ip[P_BEST_C];
    x->mv_limits.col_min = ip[P_CMIN], x->mv_limits.col_max = ip[P_CMAX], x->mv_limits.row_min = ip[P_RMIN], x->mv_limits.row_max = ip[P_RMAX];
    x->errorperbit = ip[P_EPB];
    int          thissme = 0, besterr = 0, dis = 0;
    unsigned int sse1 = 0;
    if (ip[P_DO_FULL]) {
        MvLimits tmp = x->mv_limits;
        svt_av1_set_mv_search_range(&x->mv_limits, &ref_mv);
        MV mvp_full = best_pred;
        mvp_full.col >>= 3;
        mvp_full.row >>= 3;
        thissme      = svt_av1_obmc_full_pixel_search(s.ctx, x, &mvp_full, ip[P_SADPB], &svt_aom_mefn_ptr[bsize], &ref_mv, &x->best_mv.as_mv, 0);
        x->mv_limits = tmp;
    } else {
        x->best_mv.as_mv.col = best_pred.col >> 3;
        x->best_mv.as_mv.row = best_pred.row >> 3;
    }
    out[2] = x->best_mv.as_mv.row, out[3] = x->best_mv.as_mv.col;
    if (ip[P_DO_FRAC])
        besterr = svt_av1_find_best_obmc_sub_pixel_tree_up(s.ctx, x, NULL, 0, 0, &x->best_mv.as_mv, &ref_mv, ip[P_ALLOW_HP], x->errorperbit, &svt_aom_mefn_ptr[bsize],
                                                           ip[P_FORCED_STOP], ip[P_ITERS], x->nmv_vec_cost, x->mv_cost_stack, &dis, &sse1, 0, ip[P_SEARCH_TYPE]);
    else {
        x->best_mv.as_mv.col <<= 3;
        x->best_mv.as_mv.row <<= 3;
    }
    out[0] = x->best_mv.as_mv.row, out[1] = x->best_mv.as_mv.col, out[4] = thissme, out[5] = besterr, out[6] = dis, out[7] = (int)sse1;
    out[8] = s.ctx->approx_inter_rate ? svt_av1_mv_bit_cost_light(&x->best_mv.as_mv, &ref_mv)
                                      : svt_av1_mv_bit_cost(&x->best_mv.as_mv, &ref_mv, x->nmv_vec_cost, x->mv_cost_stack, MV_COST_WEIGHT);
    free(s.ctx);
}

/* the picture-level structures single_motion_search reads, zeroed, allocated once and reused from item to item */
typedef struct {
    PictureControlSet       *pcs;
    PictureParentControlSet *ppcs;
    Av1Common               *cm;
    MdRateEstimationContext *rate;
    BlkStruct               *blk;
    ModeDecisionContext     *ctx;
} Env;
static Env env_new(const int *joint, const int *comp) {
    Env e;
    e.pcs  = (PictureControlSet *)calloc(1, sizeof(PictureControlSet));
    e.ppcs = (PictureParentControlSet *)calloc(1, sizeof(PictureParentControlSet));
    e.cm   = (Av1Common *)calloc(1, sizeof(Av1Common));
    e.rate = (MdRateEstimationContext *)calloc(1, sizeof(MdRateEstimationContext));
    e.blk  = (BlkStruct *)calloc(1, sizeof(BlkStruct));
    e.ctx  = (ModeDecisionContext *)calloc(1, sizeof(ModeDecisionContext));
    e.pcs->ppcs = e.ppcs, e.ppcs->av1_cm = e.cm;
    memcpy(e.rate->nmv_vec_cost, joint, sizeof(e.rate->nmv_vec_cost));
    memcpy(e.rate->nmv_costs, comp, sizeof(e.rate->nmv_costs));
    e.rate->nmvcoststack[0] = &e.rate->nmv_costs[0][MV_MAX], e.rate->nmvcoststack[1] = &e.rate->nmv_costs[1][MV_MAX];
    return e;
}
static void env_free(Env *e) { free(e->blk), free(e->rate), free(e->cm), free(e->ppcs), free(e->pcs), free(e->ctx); }
static void env_run(Env *e, uint8_t *ref, int ref_stride, int bsize, int32_t *wsrc, int32_t *mask, const int *ip, int *out) {
    Setup s;
    setup(&s, e->ctx, ref, ref_stride, bsize, wsrc, mask, ip, NULL, NULL, NULL);
    ModeDecisionCandidate cand;
    memset(&cand, 0, sizeof(cand));
    cand.motion_mode = OBMC_CAUSAL;
    e->cm->mi_rows = ip[P_MI_ROWS], e->cm->mi_cols = ip[P_MI_COLS];
    e->ppcs->frm_hdr.allow_high_precision_mv        = (uint8_t)ip[P_ALLOW_HP];
    e->ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)ip[P_QIDX];
    s.ctx->full_lambda_md[EB_8_BIT_MD]              = (uint32_t)ip[P_LAMBDA];
    s.ctx->blk_ptr                                  = e->blk;
    s.ctx->md_rate_est_ctx                          = e->rate;
    e->blk->av1xd                                   = &s.xd;
    s.xd.mb_to_top_edge = -(ip[P_MI_ROW] * MI_SIZE * 8), s.xd.mb_to_left_edge = -(ip[P_MI_COL] * MI_SIZE * 8);
    IntMv best_pred;
    best_pred.as_int    = 0;
    best_pred.as_mv.row = (int16_t)ip[P_BEST_R], best_pred.as_mv.col = (int16_t)ip[P_BEST_C];
    MV ref_mv;
    ref_mv.row = (int16_t)ip[P_REF_R], ref_mv.col = (int16_t)ip[P_REF_C];
    int rate_mv = 0;
    single_motion_search(e->pcs, s.ctx, &cand, best_pred, &s.x, (BlockSize)bsize, &ref_mv, &rate_mv, ip[P_REFINE_LEVEL]);
    out[0] = s.x.best_mv.as_mv.row, out[1] = s.x.best_mv.as_mv.col, out[2] = rate_mv, out[3] = s.x.sadperbit16, out[4] = s.x.errorperbit;
    out[5] = s.x.mv_limits.col_min, out[6] = s.x.mv_limits.col_max, out[7] = s.x.mv_limits.row_min, out[8] = s.x.mv_limits.row_max;
}

/* joint[4], comp[2][MV_VALS]: copied into an MdRateEstimationContext, whose own nmvcoststack single_motion_search takes.
 * out: mv_row, mv_col, rate_mv, sadperbit16, errorperbit, col_min, col_max, row_min, row_max (x->mv_limits after the call) */
void harness_single_motion_search(uint8_t *ref, int ref_stride, int bsize, int32_t *wsrc, int32_t *mask, const int *ip, const int *joint, const int *comp, int *out) {
    Env e = env_new(joint, comp);
    env_run(&e, ref, ref_stride, bsize, wsrc, mask, ip, out);
    env_free(&e);
}

/* tools/obmc_timing.py: single_motion_search for items first .. first + count - 1 of a picture cut into `cols` blocks per row (block k's reference position is its own
 * position in `ref`; wsrc / mask are W * H per item, back to back, item `first` at index 0), without the cost of a foreign call per item and with the structures
 * allocated once.  out: 3 values per item (may be NULL) */
void harness_single_motion_search_many(uint8_t *ref, int stride, int bsize, int32_t *wsrc, int32_t *mask, const int *ip, const int *joint, const int *comp, int cols,
                                       int first, int count, int *out) {
    int       tmp[9];
    const int bw = block_size_wide[bsize], bh = block_size_high[bsize];
    Env       e = env_new(joint, comp);
    for (int k = first; k < first + count; k++) {
        const size_t off = (size_t)(k / cols) * bh * stride + (size_t)(k % cols) * bw, t = (size_t)(k - first) * bw * bh;
        env_run(&e, ref + off, stride, bsize, wsrc + t, mask + t, ip, tmp);
        if (out) memcpy(out + 3 * (size_t)(k - first), tmp, 3 * sizeof(int));
    }
    env_free(&e);
}
