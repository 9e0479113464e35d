/* scale_ref_harness.c -- TEST INFRASTRUCTURE: reaches two pieces of the reference that ctypes cannot reach with flat arguments.
 *
 * Compiled by tests/test_scale_ref.py (CPU, needs the reference's sources) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so; the reference's sources are included WHERE THEY LIE (nothing is copied).
 *   harness_subpel_params  compute_subpel_params (enc_inter_prediction.c:3158) is static: its translation unit is included whole, and the function is called with the
 *                          ScaleFactors svt_av1_setup_scale_factors_for_frame filled for the picture pair.
 *   harness_scale_value    the struct's scale_value_x / scale_value_y function pointers, as compute_subpel_params calls them.
 *   harness_upscale        svt_av1_upscale_normative_rows with a hand-filled Av1Common: only frm_size, tiles_info and mi_cols are read. */
#include "enc_inter_prediction.c"

/* every dispatch pointer = its C function: svt_av1_[highbd_]resize_plane_c reaches the 1-D functions through svt_av1_interpolate_core / svt_av1_down2_symeven */
void harness_init(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
}

/* out: subpel_x, subpel_y, xs, ys, pos_y, pos_x; frame_w / frame_h: the reference picture's size, as the call sites pass it */
void harness_subpel_params(int sb_size, int pre_y, int pre_x, int mv_row, int mv_col, int other_w, int other_h, int this_w, int this_h, int ss_y, int ss_x, int *out) {
    SequenceControlSet *scs = (SequenceControlSet *)calloc(1, sizeof(*scs));
    ScaleFactors        sf;
    SubpelParams        sp;
    MV                  mv;
    int32_t             pos_y = 0, pos_x = 0;
    memset(&sf, 0, sizeof(sf));
    memset(&sp, 0, sizeof(sp));
    scs->super_block_size = (uint32_t)sb_size;
    mv.row = (int16_t)mv_row, mv.col = (int16_t)mv_col;
    svt_av1_setup_scale_factors_for_frame(&sf, other_w, other_h, this_w, this_h);
    compute_subpel_params(scs, (int16_t)pre_y, (int16_t)pre_x, mv, &sf, (uint16_t)other_w, (uint16_t)other_h, 0, 0, NULL, (uint32_t)ss_y, (uint32_t)ss_x, &sp, &pos_y, &pos_x);
    out[0] = sp.subpel_x, out[1] = sp.subpel_y, out[2] = sp.xs, out[3] = sp.ys, out[4] = pos_y, out[5] = pos_x;
    free(scs);
}

/* out: x_scale_fp, y_scale_fp, x_step_q4, y_step_q4, scale_value_x(val), scale_value_y(val); x_scale_fp == -1 for an invalid pair (then nothing else is set) */
void harness_scale_value(int other_w, int other_h, int this_w, int this_h, int val, int *out) {
    ScaleFactors sf;
    memset(&sf, 0, sizeof(sf));
    svt_av1_setup_scale_factors_for_frame(&sf, other_w, other_h, this_w, this_h);
    out[0] = sf.x_scale_fp, out[1] = sf.y_scale_fp, out[2] = sf.x_step_q4, out[3] = sf.y_step_q4;
    if (sf.x_scale_fp == REF_INVALID_SCALE) return;
    out[4] = sf.scale_value_x(val, &sf), out[5] = sf.scale_value_y(val, &sf);
}

void svt_av1_upscale_normative_rows(const Av1Common *cm, const uint8_t *src, int src_stride, uint8_t *dst, int dst_stride, int rows, int sub_x, int bd,
                                    bool is_16bit_pipeline);

/* strides in samples, as the C takes them; starts_mi: n_tile_cols + 1 entries */
void harness_upscale(const uint8_t *src, int src_stride, uint8_t *dst, int dst_stride, int rows, int sub_x, int bd, int is_16bit, int frame_width, int upscaled_width,
                     int denom, int mi_cols, int n_tile_cols, const int *starts_mi) {
    Av1Common *cm = (Av1Common *)calloc(1, sizeof(*cm));
    cm->frm_size.frame_width             = (uint16_t)frame_width;
    cm->frm_size.superres_upscaled_width = (uint16_t)upscaled_width;
    cm->frm_size.superres_denominator    = (uint8_t)denom;
    cm->mi_cols                          = mi_cols;
    cm->tiles_info.tile_cols             = (uint8_t)n_tile_cols;
    for (int j = 0; j <= n_tile_cols; j++) cm->tiles_info.tile_col_start_mi[j] = (uint16_t)starts_mi[j];
    svt_av1_upscale_normative_rows(cm, src, src_stride, dst, dst_stride, rows, sub_x, bd, is_16bit != 0);
    free(cm);
}
