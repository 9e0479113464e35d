/* palette_ref_harness.c -- TEST INFRASTRUCTURE: reaches the pieces of the reference's palette code that ctypes cannot reach with flat arguments.
 *
 * Compiled by tests/test_palette_ref.py (CPU, needs the reference's sources) into a shared library next to the test's temporary files and linked against
 * oracle/_ref/libsvtref.so; the reference's headers are included WHERE THEY LIE (nothing is copied).  Each entry fills the few fields the function reads of the
 * encoder's structures -- everything else stays zero -- and calls it:
 *   harness_search      search_palette_luma: the picture descriptor (8-bit enhanced_pic or input_frame16bit), hbd_md, the block origin, bsize, mb_to_right_edge /
 *                       mb_to_bottom_edge, the above / left MbModeInfo palettes (svt_get_palette_cache_y makes the cache from them), kmeans_data_buf,
 *                       dominant_color_step, encoder_bit_depth.
 *   harness_search_picture  the same over every block of a picture with one context, for the timing tool.
 *   harness_kmeans_items    svt_av1_k_means_dim1 (the dispatch pointer) over many items, for the timing tool.
 *   harness_cost_map    svt_av1_cost_color_map with the rate table's palette_ycolor_fac_bitss.
 *   harness_cache       svt_get_palette_cache_y alone.
 * The k-means functions, the colour counters, the context function, svt_av1_palette_color_cost_y and svt_aom_write_uniform_cost take flat arguments and are called
 * from python directly. */
#include <stdlib.h>
#include <string.h>
#include "definitions.h"
#include "utility.h"
#include "coding_unit.h"
#include "pcs.h"
#include "sequence_control_set.h"
#include "md_process.h"
#include "mode_decision.h"
#include "md_rate_estimation.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"

void search_palette_luma(PictureControlSet *pcs, ModeDecisionContext *ctx, PaletteInfo *palette_cand, uint8_t *palette_size_array, uint32_t *tot_palette_cands);
int  svt_av1_cost_color_map(ModeDecisionCandidate *cand, MdRateEstimationContext *rate_table, BlkStruct *blk_ptr, int plane, BlockSize bsize, COLOR_MAP_TYPE type);
int  svt_get_palette_cache_y(const MacroBlockD *const xd, uint16_t *cache);

/* every dispatch pointer = its C function */
void harness_init(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
}

static BlockSize bsize_of(int bw, int bh) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == bw && block_size_high[b] == bh) return (BlockSize)b;
    return BLOCK_INVALID;
}

typedef struct {
    MacroBlockD xd;
    MbModeInfo  above, left;
} Neighbours;
/* a block one mode-info row below a superblock boundary (the above neighbour counts), rows x cols of it inside the picture */
static void neighbours(Neighbours *nb, int bw, int bh, int rows, int cols, const uint16_t *above, int above_n, const uint16_t *left, int left_n) {
    memset(nb, 0, sizeof(*nb));
    nb->xd.mb_to_top_edge    = -8 * 4;
    nb->xd.mb_to_right_edge  = (cols - bw) * 8;
    nb->xd.mb_to_bottom_edge = (rows - bh) * 8;
    nb->above.palette_mode_info.palette_size = (uint8_t)above_n;
    nb->left.palette_mode_info.palette_size  = (uint8_t)left_n;
    for (int i = 0; i < above_n; i++) nb->above.palette_mode_info.palette_colors[i] = above[i];
    for (int i = 0; i < left_n; i++) nb->left.palette_mode_info.palette_colors[i] = left[i];
    nb->xd.above_mbmi = &nb->above;
    nb->xd.left_mbmi  = &nb->left;
}

int harness_cache(const uint16_t *above, int above_n, const uint16_t *left, int left_n, uint16_t *cache) {
    Neighbours nb;
    neighbours(&nb, 8, 8, 8, 8, above, above_n, left, left_n);
    return svt_get_palette_cache_y(&nb.xd, cache);
}

/* what search_palette_luma reads of a picture control set and a mode-decision context, for one picture */
typedef struct {
    PictureControlSet       *pcs;
    PictureParentControlSet *ppcs;
    SequenceControlSet      *scs;
    ModeDecisionContext     *ctx;
    BlkStruct               *blk;
    BlockGeom               *geom;
    EbPictureBufferDesc     *pic;
    Neighbours               nb;
    PaletteInfo              cand[MAX_PAL_CAND];
    uint8_t                  size_array[MAX_PAL_CAND];
} Search;
static Search *search_new(void *plane, int stride, int is16, int step, int encoder_bit_depth) {
    Search *s = (Search *)calloc(1, sizeof(*s));
    s->pcs    = (PictureControlSet *)calloc(1, sizeof(*s->pcs));
    s->ppcs   = (PictureParentControlSet *)calloc(1, sizeof(*s->ppcs));
    s->scs    = (SequenceControlSet *)calloc(1, sizeof(*s->scs));
    s->ctx    = (ModeDecisionContext *)calloc(1, sizeof(*s->ctx));
    s->blk    = (BlkStruct *)calloc(1, sizeof(*s->blk));
    s->geom   = (BlockGeom *)calloc(1, sizeof(*s->geom));
    s->pic    = (EbPictureBufferDesc *)calloc(1, sizeof(*s->pic));
    s->pic->buffer_y = (uint8_t *)plane, s->pic->stride_y = (uint16_t)stride;
    if (is16) s->pcs->input_frame16bit = s->pic;
    else s->ppcs->enhanced_pic = s->pic;
    s->scs->encoder_bit_depth                  = (uint32_t)encoder_bit_depth;
    s->ppcs->scs                               = s->scs;
    s->ppcs->palette_ctrls.dominant_color_step = (uint8_t)step;
    s->pcs->ppcs                               = s->ppcs;
    s->blk->av1xd                              = &s->nb.xd;
    s->ctx->hbd_md = (uint8_t)is16;
    s->ctx->blk_ptr = s->blk, s->ctx->blk_geom = s->geom;
    s->ctx->palette_buffer = (PALETTE_BUFFER *)calloc(1, sizeof(PALETTE_BUFFER));
    for (int i = 0; i < MAX_PAL_CAND; i++) s->cand[i].color_idx_map = (uint8_t *)calloc(MAX_PALETTE_SQUARE, 1);
    return s;
}
static void search_free(Search *s) {
    for (int i = 0; i < MAX_PAL_CAND; i++) free(s->cand[i].color_idx_map);
    free(s->ctx->palette_buffer), free(s->pic), free(s->geom), free(s->blk), free(s->ctx), free(s->scs), free(s->ppcs), free(s->pcs), free(s);
}
static uint32_t search_block(Search *s, int org_x, int org_y, int bw, int bh, int rows, int cols, const uint16_t *above, int above_n, const uint16_t *left, int left_n) {
    uint32_t tot = 0;
    neighbours(&s->nb, bw, bh, rows, cols, above, above_n, left, left_n);
    s->geom->bsize = bsize_of(bw, bh);
    s->ctx->blk_org_x = (uint16_t)org_x, s->ctx->blk_org_y = (uint16_t)org_y;
    search_palette_luma(s->pcs, s->ctx, s->cand, s->size_array, &tot);
    return tot;
}

/* plane: the picture (the block at org_x, org_y of it); sizes[14], colors[14][8], maps[14][bw * bh]; returns the number of candidates */
int harness_search(void *plane, int stride, int is16, int org_x, int org_y, int bw, int bh, int rows, int cols, const uint16_t *above, int above_n, const uint16_t *left,
                   int left_n, int step, int encoder_bit_depth, uint8_t *sizes, uint16_t *colors, uint8_t *maps) {
    Search        *s   = search_new(plane, stride, is16, step, encoder_bit_depth);
    const uint32_t tot = search_block(s, org_x, org_y, bw, bh, rows, cols, above, above_n, left, left_n);
    for (uint32_t i = 0; i < tot; i++) {
        sizes[i] = s->size_array[i];
        memcpy(colors + 8 * i, s->cand[i].pmi.palette_colors, 8 * sizeof(uint16_t));
        memcpy(maps + (size_t)i * bw * bh, s->cand[i].color_idx_map, (size_t)bw * bh);
    }
    search_free(s);
    return (int)tot;
}

/* for timing (tools/palette_timing.py): every bw x bh block of a width x height picture, those at the right and bottom edge partly outside it, no cache; one context
 * for the whole picture; returns the number of candidates found */
long harness_search_picture(void *plane, int stride, int is16, int width, int height, int bw, int bh, int step, int encoder_bit_depth) {
    Search *s   = search_new(plane, stride, is16, step, encoder_bit_depth);
    long    tot = 0;
    for (int y = 0; y < height; y += bh)
        for (int x = 0; x < width; x += bw)
            tot += search_block(s, x, y, bw, bh, height - y < bh ? height - y : bh, width - x < bw ? width - x : bw, NULL, 0, NULL, 0);
    search_free(s);
    return tot;
}

/* for timing: `items` k-means runs of n points each through the dispatch pointer, as av1_k_means calls it */
void harness_kmeans_items(const int *data, int *centroids, uint8_t *indices, int n, int k, int max_itr, int items) {
    for (int i = 0; i < items; i++) svt_av1_k_means_dim1(data + (size_t)i * n, centroids + (size_t)i * k, indices + (size_t)i * n, n, k, max_itr);
}

/* map at pitch bw; table = palette_ycolor_fac_bitss[7][5][8] */
int harness_cost_map(uint8_t *map, int bw, int bh, int rows, int cols, int size, const int32_t *table) {
    MdRateEstimationContext *rate = (MdRateEstimationContext *)calloc(1, sizeof(*rate));
    ModeDecisionCandidate   *cand = (ModeDecisionCandidate *)calloc(1, sizeof(*cand));
    BlkStruct               *blk  = (BlkStruct *)calloc(1, sizeof(*blk));
    PaletteInfo              info;
    Neighbours               nb;
    neighbours(&nb, bw, bh, rows, cols, NULL, 0, NULL, 0);
    memset(&info, 0, sizeof(info));
    memcpy(rate->palette_ycolor_fac_bitss, table, sizeof(rate->palette_ycolor_fac_bitss));
    info.color_idx_map = map;
    cand->palette_info = &info, cand->palette_size[0] = (uint8_t)size;
    blk->av1xd = &nb.xd;
    const int bits = svt_av1_cost_color_map(cand, rate, blk, 0, bsize_of(bw, bh), PALETTE_MAP);
    free(blk), free(cand), free(rate);
    return bits;
}
