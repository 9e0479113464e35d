/* picstats_ref_harness.c -- TEST INFRASTRUCTURE: reaches the reference's picture statistics and variance boost through their exported callers.
 *
 * Compiled by tests/test_picstats_ref.py (CPU, needs the reference's headers) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so.  Zeroed SequenceControlSet / PictureParentControlSet / PictureControlSet with only the fields filled that
 * svt_aom_gathering_picture_statistics (pic_analysis_process.c:1559) and svt_variance_adjust_qp (rc_process.c:1508) read; the static functions behind them
 * (compute_block_mean_compute_variance, av1_get_deltaq_sb_variance_boost, ...) are reached through those two. */
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "sequence_control_set.h"
#include "pcs.h"
#include "pd_process.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"

void svt_variance_adjust_qp(PictureControlSet *pcs, bool readjust_base_q_idx); /* rc_process.c:1508 (no header declares it) */

void harness_init(void) { svt_aom_setup_rtcd_internal(0); } /* every dispatch pointer = its C function */

typedef struct HarnessPlane { uint8_t *buffer; uint32_t stride, org_x, org_y, width, height; } HarnessPlane;

static void fill_desc(EbPictureBufferDesc *d, const HarnessPlane *p) {
    memset(d, 0, sizeof(*d));
    d->buffer_y = p->buffer;
    d->stride_y = (uint16_t)p->stride;
    d->org_x    = (uint16_t)p->org_x;
    d->org_y    = (uint16_t)p->org_y;
    d->width    = (uint16_t)p->width;
    d->height   = (uint16_t)p->height;
}

/* variance: [n_sb][85] in / out (entries the reference does not write keep what the caller put there); histogram: [rw][rh][256]; avg_intensity: [rw][rh] */
int harness_picture_statistics(const HarnessPlane *padded, const HarnessPlane *sixteenth, int prec, int adaptive_quantization, int variance_octile, int calc_hist,
                               int calculate_variance, uint32_t regions_w, uint32_t regions_h, int scene_change_detection, uint16_t *variance, uint16_t *pic_avg_variance,
                               uint32_t *histogram, uint64_t *avg_intensity, uint64_t *avg_luma) {
    SequenceControlSet      *scs = calloc(1, sizeof(*scs));
    PictureParentControlSet *pcs = calloc(1, sizeof(*pcs));
    EbPictureBufferDesc      pad, six;
    if (!scs || !pcs) return -1;
    fill_desc(&pad, padded);
    fill_desc(&six, sixteenth);
    const uint32_t sbs_x = (padded->width + 63) / 64, sbs_y = (padded->height + 63) / 64, n_sb = sbs_x * sbs_y;
    scs->calc_hist                                      = (uint8_t)calc_hist;
    scs->calculate_variance                             = (uint8_t)calculate_variance;
    scs->block_mean_calc_prec                           = prec;
    scs->picture_analysis_number_of_regions_per_width   = regions_w;
    scs->picture_analysis_number_of_regions_per_height  = regions_h;
    scs->static_config.scene_change_detection           = scene_change_detection;
    scs->static_config.enable_adaptive_quantization     = adaptive_quantization;
    scs->static_config.variance_octile                  = variance_octile;
    pcs->b64_total_count = (uint16_t)n_sb;
    pcs->b64_geom        = calloc(n_sb, sizeof(*pcs->b64_geom));
    pcs->variance        = calloc(n_sb, sizeof(*pcs->variance));
    for (uint32_t i = 0; i < n_sb; i++) {
        pcs->b64_geom[i].org_x = (uint16_t)(64 * (i % sbs_x));
        pcs->b64_geom[i].org_y = (uint16_t)(64 * (i / sbs_x));
        pcs->variance[i]       = variance + 85 * i;
    }
    pcs->picture_histogram = calloc(regions_w, sizeof(*pcs->picture_histogram));
    for (uint32_t w = 0; w < regions_w; w++) {
        pcs->picture_histogram[w] = calloc(regions_h, sizeof(**pcs->picture_histogram));
        for (uint32_t h = 0; h < regions_h; h++) pcs->picture_histogram[w][h] = histogram + 256 * (w * regions_h + h);
    }
    svt_aom_gathering_picture_statistics(scs, pcs, &pad, &six);
    for (uint32_t w = 0; w < regions_w; w++)
        for (uint32_t h = 0; h < regions_h; h++) avg_intensity[w * regions_h + h] = pcs->average_intensity_per_region[w][h];
    *avg_luma         = pcs->avg_luma;
    *pic_avg_variance = pcs->pic_avg_variance;
    for (uint32_t w = 0; w < regions_w; w++) free(pcs->picture_histogram[w]);
    free(pcs->picture_histogram);
    free(pcs->variance);
    free(pcs->b64_geom);
    free(pcs);
    free(scs);
    return 0;
}

/* qindex: [n_sb] in / out; returns the normalised base_q_idx the reference writes back with readjust_base_q_idx */
int harness_variance_adjust_qp(uint16_t *variance, uint8_t *qindex, uint32_t n_sb, int base_q_idx, int strength, int octile, int curve, int bit_depth) {
    SequenceControlSet      *scs  = calloc(1, sizeof(*scs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    PictureControlSet       *pcs  = calloc(1, sizeof(*pcs));
    SuperBlock              *sbs  = calloc(n_sb, sizeof(*sbs));
    if (!scs || !ppcs || !pcs || !sbs) return -1;
    pcs->ppcs                                        = ppcs;
    ppcs->scs                                        = scs;
    scs->sb_total_count                              = (uint16_t)n_sb;
    ppcs->b64_total_count                            = (uint16_t)n_sb;
    scs->static_config.variance_boost_strength       = (uint8_t)strength;
    scs->static_config.variance_octile               = (uint8_t)octile;
    scs->static_config.variance_boost_curve          = (uint8_t)curve;
    scs->static_config.encoder_bit_depth             = (uint32_t)bit_depth;
    scs->static_config.min_qp_allowed                = 0;
    scs->static_config.max_qp_allowed                = 63;
    ppcs->frm_hdr.quantization_params.base_q_idx     = (uint8_t)base_q_idx;
    ppcs->variance                                   = calloc(n_sb, sizeof(*ppcs->variance));
    pcs->sb_ptr_array                                = calloc(n_sb, sizeof(*pcs->sb_ptr_array));
    for (uint32_t i = 0; i < n_sb; i++) {
        ppcs->variance[i]    = variance + 85 * i;
        pcs->sb_ptr_array[i] = &sbs[i];
        sbs[i].qindex        = qindex[i];
    }
    svt_variance_adjust_qp(pcs, true);
    for (uint32_t i = 0; i < n_sb; i++) qindex[i] = sbs[i].qindex;
    const int normalized = ppcs->frm_hdr.quantization_params.base_q_idx;
    free(pcs->sb_ptr_array);
    free(ppcs->variance);
    free(sbs);
    free(pcs);
    free(ppcs);
    free(scs);
    return normalized;
}

/* av1_get_deltaq_sb_variance_boost for EVERY blended variance: one superblock whose 64 8x8 variances all equal v blends to v; with qindex 255 going in, the
 * boost is 255 - qindex coming out, and with a single superblock the frame pass is the identity (range 0).  boost_out: [65536] */
int harness_boost_of_every_variance(int base_q_idx, int strength, int octile, int curve, int bit_depth, int16_t *boost_out) {
    SequenceControlSet      *scs  = calloc(1, sizeof(*scs));
    PictureParentControlSet *ppcs = calloc(1, sizeof(*ppcs));
    PictureControlSet       *pcs  = calloc(1, sizeof(*pcs));
    SuperBlock              *sb   = calloc(1, sizeof(*sb));
    uint16_t                 var[85], *varp = var;
    if (!scs || !ppcs || !pcs || !sb) return -1;
    pcs->ppcs                                  = ppcs;
    ppcs->scs                                  = scs;
    scs->sb_total_count                        = 1;
    ppcs->b64_total_count                      = 1;
    scs->static_config.variance_boost_strength = (uint8_t)strength;
    scs->static_config.variance_octile         = (uint8_t)octile;
    scs->static_config.variance_boost_curve    = (uint8_t)curve;
    scs->static_config.encoder_bit_depth       = (uint32_t)bit_depth;
    ppcs->variance                             = &varp;
    pcs->sb_ptr_array                          = &sb;
    int bad = 0;
    for (int v = 0; v < 65536; v++) {
        for (int k = 0; k < 85; k++) var[k] = (uint16_t)v;
        sb->qindex                                   = 255;
        ppcs->frm_hdr.quantization_params.base_q_idx = (uint8_t)base_q_idx;
        svt_variance_adjust_qp(pcs, false);
        boost_out[v] = (int16_t)(255 - sb->qindex);
        bad += ppcs->frm_hdr.quantization_params.base_q_idx != base_q_idx;
    }
    free(sb);
    free(pcs);
    free(ppcs);
    free(scs);
    return bad;
}
