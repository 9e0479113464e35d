/* intrapred_ref_harness.c -- TEST INFRASTRUCTURE: reaches the reference's two static intra-prediction builders.
 *
 * Compiled by tests/test_intrapred_ref.py (CPU, needs the reference's sources) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so.  build_intra_predictors and build_intra_predictors_high (enc_intra_prediction.c:60, :241) are `static`: this translation unit compiles
 * that reference source file WHERE IT LIES (the #include below resolves through -I<reference>/Source/Lib/Codec; nothing is copied) and adds plain-C entry points that
 * call them.  The MacroBlockD they receive is zeroed except for the two neighbour mode infos get_filt_type reads: a SMOOTH_PRED above neighbour makes it return 1. */
#include "enc_intra_prediction.c"
#include "aom_dsp_rtcd.h"

void svt_aom_init_intra_dc_predictors_c_internal(void);
void svt_aom_init_intra_predictors_internal(void);

/* every dispatch pointer = its C function; the sized-predictor tables filled */
void harness_init(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
    svt_aom_init_intra_dc_predictors_c_internal();
    svt_aom_init_intra_predictors_internal();
}

static void neighbours(MacroBlockD *xd, MbModeInfo *above, MbModeInfo *left, int filt_type) {
    memset(xd, 0, sizeof(*xd));
    memset(above, 0, sizeof(*above));
    memset(left, 0, sizeof(*left));
    above->block_mi.mode = filt_type ? SMOOTH_PRED : DC_PRED;
    left->block_mi.mode  = DC_PRED;
    xd->above_mbmi       = above;
    xd->left_mbmi        = left;
}

/* top points at above_ref[0] (the corner is at [-1]); luma plane */
int harness_build_intra_predictors(uint8_t *top, uint8_t *left, uint8_t *dst, int dst_stride, int mode, int angle_delta, int filter_intra_mode, int tx_size,
                                   int disable_edge_filter, int n_top_px, int n_topright_px, int n_left_px, int n_bottomleft_px, int filt_type) {
    MacroBlockD xd;
    MbModeInfo  ab, le;
    neighbours(&xd, &ab, &le, filt_type);
    if (get_filt_type(&xd, 0) != filt_type) return -1;
    build_intra_predictors(&xd, top, left, dst, dst_stride, (PredictionMode)mode, angle_delta, (FilterIntraMode)filter_intra_mode, (TxSize)tx_size, disable_edge_filter,
                           n_top_px, n_topright_px, n_left_px, n_bottomleft_px, 0);
    return 0;
}
int harness_build_intra_predictors_high(uint16_t *top, uint16_t *left, uint16_t *dst, int dst_stride, int mode, int angle_delta, int filter_intra_mode, int tx_size,
                                        int disable_edge_filter, int n_top_px, int n_topright_px, int n_left_px, int n_bottomleft_px, int filt_type, int bd) {
    MacroBlockD xd;
    MbModeInfo  ab, le;
    neighbours(&xd, &ab, &le, filt_type);
    if (get_filt_type(&xd, 0) != filt_type) return -1;
    build_intra_predictors_high(&xd, top, left, dst, dst_stride, (PredictionMode)mode, angle_delta, (FilterIntraMode)filter_intra_mode, (TxSize)tx_size,
                                disable_edge_filter, n_top_px, n_topright_px, n_left_px, n_bottomleft_px, 0, bd);
    return 0;
}
/* one entry of the sized-predictor tables: svt_aom_eb_pred[mode][tx_size] / svt_aom_dc_pred[have_left][have_top][tx_size] and their highbd twins */
void harness_sized_predictor(int mode, int have_left, int have_top, int tx_size, void *dst, int stride, const void *above, const void *left, int bd) {
    if (bd == 8) {
        if (mode == DC_PRED) svt_aom_dc_pred[have_left][have_top][tx_size](dst, stride, above, left);
        else svt_aom_eb_pred[mode][tx_size](dst, stride, above, left);
    } else {
        if (mode == DC_PRED) svt_aom_dc_pred_high[have_left][have_top][tx_size](dst, stride, above, left, bd);
        else svt_aom_pred_high[mode][tx_size](dst, stride, above, left, bd);
    }
}
int harness_mode_angle(int mode) { return mode_to_angle_map[mode]; } /* the static table of intra_prediction.h:65 */
