// scale.hip -- pictures of another size for gfx950: scaled-reference inter prediction, the non-normative picture resize and the normative super-resolution upscale.
// DESIGN.md 4.25 has the layout, the readable extents and the bounds.  The three share their arithmetic: a stepped fixed-point position per output sample (10 bits
// per sample in prediction, 14 bits in resize / upscale), its integer part the first of eight source samples, its top fraction bits the row of an 8-tap table --
// positions are closed-form (start + index * step), so every output sample is independent of its neighbours and each lane fetches its own table row.
//
//  * scaled_pred_kernel: one launch, n descriptors of mixed sizes, one workgroup per descriptor walking the block's tiles of min(w, 32) x min(h, 32) samples.  A
//    SCALED reference (a step other than 1024 in either direction) is svt_av1_[highbd_]convolve_2d_scale_c (inter_prediction.c:420, :779): the horizontal pass of the
//    at most 2 * 32 + 6 rows a tile touches goes into LDS as the reference's int16_t im_block, the vertical pass reads it; an UNSCALED reference of the same
//    descriptor takes the four cases of svt_aom_convolve[..] with phase subpel >> 6, as svt_hip_inter_pred_batch does.  With two references the first one's
//    ConvBufType values stay in registers.  Neither im_block nor the ConvBufType buffer reaches memory.
//  * resize_pass_kernel: ONE 1-D step of resize_multistep (resize.c:350) over a whole plane, along rows or along columns: copy, down2_symeven, down2_symodd or
//    interpolate with the table choose_interp_filter names; every index clamped to [0, length), which is what the C's initial / middle / end loops amount to.  The
//    host chains the steps of svt_av1_[highbd_]resize_plane_c (rows into the width2 x height intermediate, then columns) through the caller's workspace; no step
//    needs more than the plane it reads and the plane it writes, so there is no size cap.
//  * upscale_kernel: svt_av1_upscale_normative_rows (super_res.c:214) for up to three planes per launch; the host walks the tile columns once (x0_qn and its carry,
//    :282) and the kernel clamps reads to the frame's first / last source column instead of overwriting and restoring five border columns of the source.
//  * no atomics, nothing to zero beforehand, every output sample is written exactly once by a plain store: results do not depend on launch order.
#include "svt_hip_common.h"
#include "../../include/svtav1_hip.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int TPB = 256;

// ---- the tables -------------------------------------------------------------------------------------------------------------------------------------
// Upscale_Filter of the AV1 specification (7.16, super-resolution upscaling process) = av1_resize_filter_normative (super_res.h:22), which resize.h:75 also names
// filteredinterp_filters1000: the full-band table of the non-normative resize.
alignas(16) __device__ constexpr int16_t kUpscaleFilter[64][8] = {
    {0, 0, 0, 128, 0, 0, 0, 0},        {0, 0, -1, 128, 2, -1, 0, 0},      {0, 1, -3, 127, 4, -2, 1, 0},      {0, 1, -4, 127, 6, -3, 1, 0},
    {0, 2, -6, 126, 8, -3, 1, 0},      {0, 2, -7, 125, 11, -4, 1, 0},     {-1, 2, -8, 125, 13, -5, 2, 0},    {-1, 3, -9, 124, 15, -6, 2, 0},
    {-1, 3, -10, 123, 18, -6, 2, -1},  {-1, 3, -11, 122, 20, -7, 3, -1},  {-1, 4, -12, 121, 22, -8, 3, -1},  {-1, 4, -13, 120, 25, -9, 3, -1},
    {-1, 4, -14, 118, 28, -9, 3, -1},  {-1, 4, -15, 117, 30, -10, 4, -1}, {-1, 5, -16, 116, 32, -11, 4, -1}, {-1, 5, -16, 114, 35, -12, 4, -1},
    {-1, 5, -17, 112, 38, -12, 4, -1}, {-1, 5, -18, 111, 40, -13, 5, -1}, {-1, 5, -18, 109, 43, -14, 5, -1}, {-1, 6, -19, 107, 45, -14, 5, -1},
    {-1, 6, -19, 105, 48, -15, 5, -1}, {-1, 6, -19, 103, 51, -16, 5, -1}, {-1, 6, -20, 101, 53, -16, 6, -1}, {-1, 6, -20, 99, 56, -17, 6, -1},
    {-1, 6, -20, 97, 58, -17, 6, -1},  {-1, 6, -20, 95, 61, -18, 6, -1},  {-2, 7, -20, 93, 64, -18, 6, -2},  {-2, 7, -20, 91, 66, -19, 6, -1},
    {-2, 7, -20, 88, 69, -19, 6, -1},  {-2, 7, -20, 86, 71, -19, 6, -1},  {-2, 7, -20, 84, 74, -20, 7, -2},  {-2, 7, -20, 81, 76, -20, 7, -1},
    {-2, 7, -20, 79, 79, -20, 7, -2},  {-1, 7, -20, 76, 81, -20, 7, -2},  {-2, 7, -20, 74, 84, -20, 7, -2},  {-1, 6, -19, 71, 86, -20, 7, -2},
    {-1, 6, -19, 69, 88, -20, 7, -2},  {-1, 6, -19, 66, 91, -20, 7, -2},  {-2, 6, -18, 64, 93, -20, 7, -2},  {-1, 6, -18, 61, 95, -20, 6, -1},
    {-1, 6, -17, 58, 97, -20, 6, -1},  {-1, 6, -17, 56, 99, -20, 6, -1},  {-1, 6, -16, 53, 101, -20, 6, -1}, {-1, 5, -16, 51, 103, -19, 6, -1},
    {-1, 5, -15, 48, 105, -19, 6, -1}, {-1, 5, -14, 45, 107, -19, 6, -1}, {-1, 5, -14, 43, 109, -18, 5, -1}, {-1, 5, -13, 40, 111, -18, 5, -1},
    {-1, 4, -12, 38, 112, -17, 5, -1}, {-1, 4, -12, 35, 114, -16, 5, -1}, {-1, 4, -11, 32, 116, -16, 5, -1}, {-1, 4, -10, 30, 117, -15, 4, -1},
    {-1, 3, -9, 28, 118, -14, 4, -1},  {-1, 3, -9, 25, 120, -13, 4, -1},  {-1, 3, -8, 22, 121, -12, 4, -1},  {-1, 3, -7, 20, 122, -11, 3, -1},
    {-1, 2, -6, 18, 123, -10, 3, -1},  {0, 2, -6, 15, 124, -9, 3, -1},    {0, 2, -5, 13, 125, -8, 2, -1},    {0, 1, -4, 11, 125, -7, 2, 0},
    {0, 1, -3, 8, 126, -6, 2, 0},      {0, 1, -3, 6, 127, -4, 1, 0},      {0, 1, -2, 4, 127, -3, 1, 0},      {0, 0, -1, 2, 128, -1, 0, 0}};
// svt_aom_av1_filteredinterp_filters875 (resize.c:112), libaom's av1/common/resize.c: 0.875-band
alignas(16) __device__ constexpr int16_t kResizeFilter875[64][8] = {
    {3, -8, 13, 112, 13, -8, 3, 0},   {2, -7, 12, 112, 15, -8, 3, -1},  {3, -7, 10, 112, 17, -9, 3, -1},  {2, -6, 8, 112, 19, -9, 3, -1},
    {2, -6, 7, 112, 21, -10, 3, -1},  {2, -5, 6, 111, 22, -10, 3, -1},  {2, -5, 4, 111, 24, -10, 3, -1},  {2, -4, 3, 110, 26, -11, 3, -1},
    {2, -4, 1, 110, 28, -11, 3, -1},  {2, -4, 0, 109, 30, -12, 4, -1},  {1, -3, -1, 108, 32, -12, 4, -1}, {1, -3, -2, 108, 34, -13, 4, -1},
    {1, -2, -4, 107, 36, -13, 4, -1}, {1, -2, -5, 106, 38, -13, 4, -1}, {1, -1, -6, 105, 40, -14, 4, -1}, {1, -1, -7, 104, 42, -14, 4, -1},
    {1, -1, -7, 103, 44, -15, 4, -1}, {1, 0, -8, 101, 46, -15, 4, -1},  {1, 0, -9, 100, 48, -15, 4, -1},  {1, 0, -10, 99, 50, -15, 4, -1},
    {1, 1, -11, 97, 53, -16, 4, -1},  {0, 1, -11, 96, 55, -16, 4, -1},  {0, 1, -12, 95, 57, -16, 4, -1},  {0, 2, -13, 93, 59, -16, 4, -1},
    {0, 2, -13, 91, 61, -16, 4, -1},  {0, 2, -14, 90, 63, -16, 4, -1},  {0, 2, -14, 88, 65, -16, 4, -1},  {0, 2, -15, 86, 67, -16, 4, 0},
    {0, 3, -15, 84, 69, -17, 4, 0},   {0, 3, -16, 83, 71, -17, 4, 0},   {0, 3, -16, 81, 73, -16, 3, 0},   {0, 3, -16, 79, 75, -16, 3, 0},
    {0, 3, -16, 77, 77, -16, 3, 0},   {0, 3, -16, 75, 79, -16, 3, 0},   {0, 3, -16, 73, 81, -16, 3, 0},   {0, 4, -17, 71, 83, -16, 3, 0},
    {0, 4, -17, 69, 84, -15, 3, 0},   {0, 4, -16, 67, 86, -15, 2, 0},   {-1, 4, -16, 65, 88, -14, 2, 0},  {-1, 4, -16, 63, 90, -14, 2, 0},
    {-1, 4, -16, 61, 91, -13, 2, 0},  {-1, 4, -16, 59, 93, -13, 2, 0},  {-1, 4, -16, 57, 95, -12, 1, 0},  {-1, 4, -16, 55, 96, -11, 1, 0},
    {-1, 4, -16, 53, 97, -11, 1, 1},  {-1, 4, -15, 50, 99, -10, 0, 1},  {-1, 4, -15, 48, 100, -9, 0, 1},  {-1, 4, -15, 46, 101, -8, 0, 1},
    {-1, 4, -15, 44, 103, -7, -1, 1}, {-1, 4, -14, 42, 104, -7, -1, 1}, {-1, 4, -14, 40, 105, -6, -1, 1}, {-1, 4, -13, 38, 106, -5, -2, 1},
    {-1, 4, -13, 36, 107, -4, -2, 1}, {-1, 4, -13, 34, 108, -2, -3, 1}, {-1, 4, -12, 32, 108, -1, -3, 1}, {-1, 4, -12, 30, 109, 0, -4, 2},
    {-1, 3, -11, 28, 110, 1, -4, 2},  {-1, 3, -11, 26, 110, 3, -4, 2},  {-1, 3, -10, 24, 111, 4, -5, 2},  {-1, 3, -10, 22, 111, 6, -5, 2},
    {-1, 3, -10, 21, 112, 7, -6, 2},  {-1, 3, -9, 19, 112, 8, -6, 2},   {-1, 3, -9, 17, 112, 10, -7, 3},  {-1, 3, -8, 15, 112, 12, -7, 2}};
// svt_aom_av1_filteredinterp_filters750 (resize.c:86): 0.75-band
alignas(16) __device__ constexpr int16_t kResizeFilter750[64][8] = {
    {2, -11, 25, 96, 25, -11, 2, 0}, {2, -11, 24, 96, 26, -11, 2, 0}, {2, -11, 22, 96, 28, -11, 2, 0}, {2, -10, 21, 96, 29, -12, 2, 0},
    {2, -10, 19, 96, 31, -12, 2, 0}, {2, -10, 18, 95, 32, -11, 2, 0}, {2, -10, 17, 95, 34, -12, 2, 0}, {2, -9, 15, 95, 35, -12, 2, 0},
    {2, -9, 14, 94, 37, -12, 2, 0},  {2, -9, 13, 94, 38, -12, 2, 0},  {2, -8, 12, 93, 40, -12, 1, 0},  {2, -8, 11, 93, 41, -12, 1, 0},
    {2, -8, 9, 92, 43, -12, 1, 1},   {2, -8, 8, 92, 44, -12, 1, 1},   {2, -7, 7, 91, 46, -12, 1, 0},   {2, -7, 6, 90, 47, -12, 1, 1},
    {2, -7, 5, 90, 49, -12, 1, 0},   {2, -6, 4, 89, 50, -12, 1, 0},   {2, -6, 3, 88, 52, -12, 0, 1},   {2, -6, 2, 87, 54, -12, 0, 1},
    {2, -5, 1, 86, 55, -12, 0, 1},   {2, -5, 0, 85, 57, -12, 0, 1},   {2, -5, -1, 84, 58, -11, 0, 1},  {2, -5, -2, 83, 60, -11, 0, 1},
    {2, -4, -2, 82, 61, -11, -1, 1}, {1, -4, -3, 81, 63, -10, -1, 1}, {2, -4, -4, 80, 64, -10, -1, 1}, {1, -4, -4, 79, 66, -10, -1, 1},
    {1, -3, -5, 77, 67, -9, -1, 1},  {1, -3, -6, 76, 69, -9, -1, 1},  {1, -3, -6, 75, 70, -8, -2, 1},  {1, -2, -7, 74, 71, -8, -2, 1},
    {1, -2, -7, 72, 72, -7, -2, 1},  {1, -2, -8, 71, 74, -7, -2, 1},  {1, -2, -8, 70, 75, -6, -3, 1},  {1, -1, -9, 69, 76, -6, -3, 1},
    {1, -1, -9, 67, 77, -5, -3, 1},  {1, -1, -10, 66, 79, -4, -4, 1}, {1, -1, -10, 64, 80, -4, -4, 2}, {1, -1, -10, 63, 81, -3, -4, 1},
    {1, -1, -11, 61, 82, -2, -4, 2}, {1, 0, -11, 60, 83, -2, -5, 2},  {1, 0, -11, 58, 84, -1, -5, 2},  {1, 0, -12, 57, 85, 0, -5, 2},
    {1, 0, -12, 55, 86, 1, -5, 2},   {1, 0, -12, 54, 87, 2, -6, 2},   {1, 0, -12, 52, 88, 3, -6, 2},   {0, 1, -12, 50, 89, 4, -6, 2},
    {0, 1, -12, 49, 90, 5, -7, 2},   {1, 1, -12, 47, 90, 6, -7, 2},   {0, 1, -12, 46, 91, 7, -7, 2},   {1, 1, -12, 44, 92, 8, -8, 2},
    {1, 1, -12, 43, 92, 9, -8, 2},   {0, 1, -12, 41, 93, 11, -8, 2},  {0, 1, -12, 40, 93, 12, -8, 2},  {0, 2, -12, 38, 94, 13, -9, 2},
    {0, 2, -12, 37, 94, 14, -9, 2},  {0, 2, -12, 35, 95, 15, -9, 2},  {0, 2, -12, 34, 95, 17, -10, 2}, {0, 2, -11, 32, 95, 18, -10, 2},
    {0, 2, -12, 31, 96, 19, -10, 2}, {0, 2, -12, 29, 96, 21, -10, 2}, {0, 2, -11, 28, 96, 22, -11, 2}, {0, 2, -11, 26, 96, 24, -11, 2}};
// svt_aom_av1_filteredinterp_filters625 (resize.c:60): 0.625-band
alignas(16) __device__ constexpr int16_t kResizeFilter625[64][8] = {
    {-1, -8, 33, 80, 33, -8, -1, 0}, {-1, -8, 31, 80, 34, -8, -1, 1}, {-1, -8, 30, 80, 35, -8, -1, 1}, {-1, -8, 29, 80, 36, -7, -2, 1},
    {-1, -8, 28, 80, 37, -7, -2, 1}, {-1, -8, 27, 80, 38, -7, -2, 1}, {0, -8, 26, 79, 39, -7, -2, 1},  {0, -8, 25, 79, 40, -7, -2, 1},
    {0, -8, 24, 79, 41, -7, -2, 1},  {0, -8, 23, 78, 42, -6, -2, 1},  {0, -8, 22, 78, 43, -6, -2, 1},  {0, -8, 21, 78, 44, -6, -2, 1},
    {0, -8, 20, 78, 45, -5, -3, 1},  {0, -8, 19, 77, 47, -5, -3, 1},  {0, -8, 18, 77, 48, -5, -3, 1},  {0, -8, 17, 77, 49, -5, -3, 1},
    {0, -8, 16, 76, 50, -4, -3, 1},  {0, -8, 15, 76, 51, -4, -3, 1},  {0, -8, 15, 75, 52, -3, -4, 1},  {0, -7, 14, 74, 53, -3, -4, 1},
    {0, -7, 13, 74, 54, -3, -4, 1},  {0, -7, 12, 73, 55, -2, -4, 1},  {0, -7, 11, 73, 56, -2, -4, 1},  {0, -7, 10, 72, 57, -1, -4, 1},
    {1, -7, 10, 71, 58, -1, -5, 1},  {0, -7, 9, 71, 59, 0, -5, 1},    {1, -7, 8, 70, 60, 0, -5, 1},    {1, -7, 7, 69, 61, 1, -5, 1},
    {1, -6, 6, 68, 62, 1, -5, 1},    {0, -6, 6, 68, 62, 2, -5, 1},    {1, -6, 5, 67, 63, 2, -5, 1},    {1, -6, 5, 66, 64, 3, -6, 1},
    {1, -6, 4, 65, 65, 4, -6, 1},    {1, -6, 3, 64, 66, 5, -6, 1},    {1, -5, 2, 63, 67, 5, -6, 1},    {1, -5, 2, 62, 68, 6, -6, 0},
    {1, -5, 1, 62, 68, 6, -6, 1},    {1, -5, 1, 61, 69, 7, -7, 1},    {1, -5, 0, 60, 70, 8, -7, 1},    {1, -5, 0, 59, 71, 9, -7, 0},
    {1, -5, -1, 58, 71, 10, -7, 1},  {1, -4, -1, 57, 72, 10, -7, 0},  {1, -4, -2, 56, 73, 11, -7, 0},  {1, -4, -2, 55, 73, 12, -7, 0},
    {1, -4, -3, 54, 74, 13, -7, 0},  {1, -4, -3, 53, 74, 14, -7, 0},  {1, -4, -3, 52, 75, 15, -8, 0},  {1, -3, -4, 51, 76, 15, -8, 0},
    {1, -3, -4, 50, 76, 16, -8, 0},  {1, -3, -5, 49, 77, 17, -8, 0},  {1, -3, -5, 48, 77, 18, -8, 0},  {1, -3, -5, 47, 77, 19, -8, 0},
    {1, -3, -5, 45, 78, 20, -8, 0},  {1, -2, -6, 44, 78, 21, -8, 0},  {1, -2, -6, 43, 78, 22, -8, 0},  {1, -2, -6, 42, 78, 23, -8, 0},
    {1, -2, -7, 41, 79, 24, -8, 0},  {1, -2, -7, 40, 79, 25, -8, 0},  {1, -2, -7, 39, 79, 26, -8, 0},  {1, -2, -7, 38, 80, 27, -8, -1},
    {1, -2, -7, 37, 80, 28, -8, -1}, {1, -2, -7, 36, 80, 29, -8, -1}, {1, -1, -8, 35, 80, 30, -8, -1}, {1, -1, -8, 34, 80, 31, -8, -1}};
// svt_aom_av1_filteredinterp_filters500 (resize.c:34): 0.5-band
alignas(16) __device__ constexpr int16_t kResizeFilter500[64][8] = {
    {-3, 0, 35, 64, 35, 0, -3, 0},    {-3, 0, 34, 64, 36, 0, -3, 0},    {-3, -1, 34, 64, 36, 1, -3, 0},   {-3, -1, 33, 64, 37, 1, -3, 0},
    {-3, -1, 32, 64, 38, 1, -3, 0},   {-3, -1, 31, 64, 39, 1, -3, 0},   {-3, -1, 31, 63, 39, 2, -3, 0},   {-2, -2, 30, 63, 40, 2, -3, 0},
    {-2, -2, 29, 63, 41, 2, -3, 0},   {-2, -2, 29, 63, 41, 3, -4, 0},   {-2, -2, 28, 63, 42, 3, -4, 0},   {-2, -2, 27, 63, 43, 3, -4, 0},
    {-2, -3, 27, 63, 43, 4, -4, 0},   {-2, -3, 26, 62, 44, 5, -4, 0},   {-2, -3, 25, 62, 45, 5, -4, 0},   {-2, -3, 25, 62, 45, 5, -4, 0},
    {-2, -3, 24, 62, 46, 5, -4, 0},   {-2, -3, 23, 61, 47, 6, -4, 0},   {-2, -3, 23, 61, 47, 6, -4, 0},   {-2, -3, 22, 61, 48, 7, -4, -1},
    {-2, -3, 21, 60, 49, 7, -4, 0},   {-1, -4, 20, 60, 49, 8, -4, 0},   {-1, -4, 20, 60, 50, 8, -4, -1},  {-1, -4, 19, 59, 51, 9, -4, -1},
    {-1, -4, 19, 59, 51, 9, -4, -1},  {-1, -4, 18, 58, 52, 10, -4, -1}, {-1, -4, 17, 58, 52, 11, -4, -1}, {-1, -4, 16, 58, 53, 11, -4, -1},
    {-1, -4, 16, 57, 53, 12, -4, -1}, {-1, -4, 15, 57, 54, 12, -4, -1}, {-1, -4, 15, 56, 54, 13, -4, -1}, {-1, -4, 14, 56, 55, 13, -4, -1},
    {-1, -4, 14, 55, 55, 14, -4, -1}, {-1, -4, 13, 55, 56, 14, -4, -1}, {-1, -4, 13, 54, 56, 15, -4, -1}, {-1, -4, 12, 54, 57, 15, -4, -1},
    {-1, -4, 12, 53, 57, 16, -4, -1}, {-1, -4, 11, 53, 58, 16, -4, -1}, {-1, -4, 11, 52, 58, 17, -4, -1}, {-1, -4, 10, 52, 58, 18, -4, -1},
    {-1, -4, 9, 51, 59, 19, -4, -1},  {-1, -4, 9, 51, 59, 19, -4, -1},  {-1, -4, 8, 50, 60, 20, -4, -1},  {0, -4, 8, 49, 60, 20, -4, -1},
    {0, -4, 7, 49, 60, 21, -3, -2},   {-1, -4, 7, 48, 61, 22, -3, -2},  {0, -4, 6, 47, 61, 23, -3, -2},   {0, -4, 6, 47, 61, 23, -3, -2},
    {0, -4, 5, 46, 62, 24, -3, -2},   {0, -4, 5, 45, 62, 25, -3, -2},   {0, -4, 5, 45, 62, 25, -3, -2},   {0, -4, 5, 44, 62, 26, -3, -2},
    {0, -4, 4, 43, 63, 27, -3, -2},   {0, -4, 3, 43, 63, 27, -2, -2},   {0, -4, 3, 42, 63, 28, -2, -2},   {0, -4, 3, 41, 63, 29, -2, -2},
    {0, -3, 2, 41, 63, 29, -2, -2},   {0, -3, 2, 40, 63, 30, -2, -2},   {0, -3, 2, 39, 63, 31, -1, -3},   {0, -3, 1, 39, 64, 31, -1, -3},
    {0, -3, 1, 38, 64, 32, -1, -3},   {0, -3, 1, 37, 64, 33, -1, -3},   {0, -3, 1, 36, 64, 34, -1, -3},   {0, -3, 0, 36, 64, 34, 0, -3}};
// the half filters of the factor-of-two steps: svt_aom_av1_down2_symeven_half_filter, av1_down2_symodd_half_filter (resize.c:30-31)
__device__ constexpr int16_t kDown2SymEven[4] = {56, 12, -3, -1};
__device__ constexpr int16_t kDown2SymOdd[4]  = {64, 35, 0, -3};
// The six kernels of inter_prediction.c:223-254, :1065-1129 (AV1 specification, 7.11.3.4), one row per sub-pel phase: 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH,
// 2 MULTITAP_SHARP, 3 BILINEAR, 4 sub_pel_filters_4 (REGULAR and SHARP of a dimension <= 4), 5 sub_pel_filters_4smooth
alignas(16) __device__ constexpr int16_t kInterFilters[6][16][8] = {
    {{0, 0, 0, 128, 0, 0, 0, 0},      {0, 2, -6, 126, 8, -2, 0, 0},    {0, 2, -10, 122, 18, -4, 0, 0},  {0, 2, -12, 116, 28, -8, 2, 0},
     {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -14, 102, 48, -12, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0},  {0, 2, -14, 84, 66, -12, 2, 0},
     {0, 2, -14, 76, 76, -14, 2, 0},  {0, 2, -12, 66, 84, -14, 2, 0},  {0, 2, -12, 58, 94, -16, 2, 0},  {0, 2, -12, 48, 102, -14, 2, 0},
     {0, 2, -10, 38, 110, -14, 2, 0}, {0, 2, -8, 28, 116, -12, 2, 0},  {0, 0, -4, 18, 122, -10, 2, 0},  {0, 0, -2, 8, 126, -6, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0},   {0, 2, 28, 62, 34, 2, 0, 0},   {0, 0, 26, 62, 36, 4, 0, 0},    {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0},  {0, 0, 18, 58, 44, 8, 0, 0},   {0, 0, 16, 56, 46, 10, 0, 0},   {0, -2, 16, 54, 48, 12, 0, 0},
     {0, -2, 14, 52, 52, 14, -2, 0}, {0, 0, 12, 48, 54, 16, -2, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0},  {0, 0, 4, 40, 62, 22, 0, 0},   {0, 0, 4, 36, 62, 26, 0, 0},    {0, 0, 2, 34, 62, 28, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0},         {-2, 2, -6, 126, 8, -2, 2, 0},      {-2, 6, -12, 124, 16, -6, 4, -2},   {-2, 8, -18, 120, 26, -10, 6, -2},
     {-4, 10, -22, 116, 38, -14, 6, -2}, {-4, 10, -22, 108, 48, -18, 8, -2}, {-4, 10, -24, 100, 60, -20, 8, -2}, {-4, 10, -24, 90, 70, -22, 10, -2},
     {-4, 12, -24, 80, 80, -24, 12, -4}, {-2, 10, -22, 70, 90, -24, 10, -4}, {-2, 8, -20, 60, 100, -24, 10, -4}, {-2, 8, -18, 48, 108, -22, 10, -4},
     {-2, 6, -14, 38, 116, -22, 10, -4}, {-2, 6, -10, 26, 120, -18, 8, -2},  {-2, 4, -6, 16, 124, -12, 6, -2},   {0, 2, -2, 8, 126, -6, 2, -2}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 0, 120, 8, 0, 0, 0},  {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 104, 24, 0, 0, 0},
     {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 88, 40, 0, 0, 0},  {0, 0, 0, 80, 48, 0, 0, 0},  {0, 0, 0, 72, 56, 0, 0, 0},
     {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 56, 72, 0, 0, 0},  {0, 0, 0, 48, 80, 0, 0, 0},  {0, 0, 0, 40, 88, 0, 0, 0},
     {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 24, 104, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}, {0, 0, 0, 8, 120, 0, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0},     {0, 0, -4, 126, 8, -2, 0, 0},    {0, 0, -8, 122, 18, -4, 0, 0},   {0, 0, -10, 116, 28, -6, 0, 0},
     {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -12, 102, 48, -10, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0},  {0, 0, -12, 84, 66, -10, 0, 0},
     {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 66, 84, -12, 0, 0},  {0, 0, -10, 58, 94, -14, 0, 0},  {0, 0, -10, 48, 102, -12, 0, 0},
     {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0},  {0, 0, -4, 18, 122, -8, 0, 0},   {0, 0, -2, 8, 126, -4, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0},  {0, 0, 30, 62, 34, 2, 0, 0},  {0, 0, 26, 62, 36, 4, 0, 0},  {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0},  {0, 0, 16, 56, 46, 10, 0, 0}, {0, 0, 14, 54, 48, 12, 0, 0},
     {0, 0, 12, 52, 52, 12, 0, 0}, {0, 0, 12, 48, 54, 14, 0, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0},  {0, 0, 4, 36, 62, 26, 0, 0},  {0, 0, 2, 34, 62, 30, 0, 0}}};

// ---- shared arithmetic ------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int rpot(const int v, const int n) { return (v + ((1 << n) >> 1)) >> n; } // ROUND_POWER_OF_TWO (definitions.h:459), n >= 0
__host__ __device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int load_px(const uint8_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint8_t*)p; }
__device__ __forceinline__ int load_px(const uint16_t* p) { return (int)*(const SVT_HIP_GLOBAL_AS uint16_t*)p; }
__device__ __forceinline__ int sdot2(const uint32_t a, const uint32_t b, const int c) { // c + a.lo * b.lo + a.hi * b.hi, signed 16 bit (v_dot2_i32_i16)
    typedef short s2 __attribute__((ext_vector_type(2)));
    s2 x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return __builtin_amdgcn_sdot2(x, y, c, false);
}
// the eight taps of one table row as four dwords of int16 pairs: ONE 16-byte load (every table here is 16-byte aligned and a row is 16 bytes; the forms' tables
// sit at 256-byte aligned arena offsets)
struct Taps4 { uint32_t h2[4]; };
typedef uint32_t svt_u32x4_a16 __attribute__((vector_size(16), aligned(16)));
__device__ __forceinline__ Taps4 load_taps(const int16_t* f) {
    const svt_u32x4_a16 v = *(const svt_u32x4_a16*)f;
    Taps4               t;
    t.h2[0] = v[0], t.h2[1] = v[1], t.h2[2] = v[2], t.h2[3] = v[3];
    return t;
}
__device__ __forceinline__ uint32_t pack2(const int16_t lo, const int16_t hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); }
// sum of tap * sample over the eight CONTIGUOUS samples q[0 .. 7]: one unaligned load of exactly those samples, v_dot2_i32_i16 on pairs (the bytes widened first)
__device__ __forceinline__ int hsum8(const uint8_t* q, const Taps4& t, int s) {
    const svt_u32x2_a1 v = svt_hip_global_load_x2(q);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = v[k >> 1] >> (16 * (k & 1));
        s                = sdot2((w & 0xffu) | ((w & 0xff00u) << 8), t.h2[k], s);
    }
    return s;
}
__device__ __forceinline__ int hsum8(const uint16_t* q, const Taps4& t, const int s) {
    const svt_u32x4_a2 v = svt_hip_global_load_x4(q);
    return sdot2(v[0], t.h2[0], sdot2(v[1], t.h2[1], sdot2(v[2], t.h2[2], sdot2(v[3], t.h2[3], s))));
}
// the same for samples base[clamp(p0 + k, lo, hi) * step]: eight clamped loads (picture edges, and every column access)
template <typename PIX>
__device__ __forceinline__ int csum8(const PIX* base, const size_t step, const int p0, const int lo, const int hi, const int16_t* f, int s) {
#pragma unroll
    for (int k = 0; k < 8; k++) s += (int)f[k] * load_px(base + (size_t)clampi(p0 + k, lo, hi) * step);
    return s;
}

// =====================================================================================================================================================
// A. scaled inter prediction
// =====================================================================================================================================================
constexpr int SP_TW      = 32;                // widest tile
constexpr int SP_TH      = 32;                // tallest tile
constexpr int SP_IM_ROWS = 2 * SP_TH + 8;     // (((th - 1) * 2048 + 1023) >> 10) + 8 = 2 * th + 6 rows at the largest step
constexpr int SP_NPL     = SP_TW * SP_TH / TPB; // samples per thread
constexpr int SP_IM_BOUND = 2 * 128 + 8;      // rows of the C's im_block: (2 * MAX_SB_SIZE + MAX_FILTER_TAP)

struct ScaleAux {
    uint16_t*      cb;        // modes 1, 2: the caller's ConvBufType block (row stride cb_stride)
    uint32_t       cb_stride;
    int32_t        mode;      // 0: whole prediction; 1: the C's is_compound, do_average = 0 call -> cb; 2: its do_average = 1 call on cb
    int32_t        bd, r0, r1_single, r1_compound;
    const int16_t *fx, *fy;   // single-call forms: the caller's 16 x 8 taps
};

__host__ __device__ __forceinline__ bool sp_dim_ok(const uint32_t v) { return v >= 2 && v <= 128 && (v & (v - 1)) == 0; }
__host__ __device__ __forceinline__ bool sp_ref_scaled(const SvtHipScaledPredDesc& d, const int k) { return d.xs[k] != 1024 || d.ys[k] != 1024; }
// everything the kernel relies on
__host__ __device__ __forceinline__ bool sp_desc_ok(const SvtHipScaledPredDesc& d, const SvtHipInterPredPlanes& planes) {
    if (!sp_dim_ok(d.w) || !sp_dim_ok(d.h) || d.filter_x > 3 || d.filter_y > 3 || d.compound > 2) return false;
    const int nref = d.compound ? 2 : 1;
    for (int k = 0; k < nref; k++) {
        if (d.subpel_x[k] > 1023 || d.subpel_y[k] > 1023 || d.xs[k] < 64 || d.xs[k] > 2048 || d.ys[k] < 64 || d.ys[k] > 2048) return false;
        if (!sp_ref_scaled(d, k) && ((d.subpel_x[k] | d.subpel_y[k]) & 63)) return false; // the unscaled functions take a q4 phase
        if (((((int)d.h - 1) * d.ys[k] + d.subpel_y[k]) >> 10) + 8 > SP_IM_BOUND || ((((int)d.w - 1) * d.xs[k] + d.subpel_x[k]) >> 10) + 8 > SP_IM_BOUND) return false;
        if (d.plane[k] >= 32 || planes.base[d.plane[k]] == nullptr) return false;
    }
    return true;
}
// av1_get_interp_filter_params_with_block_size (inter_prediction.h:137-145): the kernel of `filter` for a block dimension `dim`
__device__ __forceinline__ int filter_kind(const int filter, const int dim) {
    if (dim <= 4 && filter != 3) return filter == 1 ? 5 : 4;
    return filter;
}

// FORM = false: the batched entry (AV1's tables, the roundings of get_conv_params_no_round); FORM = true: one block of a single-call form (the caller's taps and
// roundings, always the scale function, aux.mode).
template <typename PIX, bool FORM>
__global__ __launch_bounds__(TPB) void scaled_pred_kernel(const SvtHipInterPredPlanes planes, PIX* __restrict__ dst_base, const SvtHipScaledPredDesc* __restrict__ descs,
                                                          const uint32_t n, uint8_t* __restrict__ status, const ScaleAux aux) {
    __shared__ int16_t im[SP_IM_ROWS * SP_TW];
    const int      tid = threadIdx.x;
    const uint32_t b   = blockIdx.x;
    if (b >= n) return;
    const SvtHipScaledPredDesc d  = descs[b];
    const bool                 ok = FORM || sp_desc_ok(d, planes); // (the workgroup's: every branch below is uniform)
    if (status && tid == 0) status[b] = ok ? 0 : 1;
    if (!ok) return;
    const int  w = d.w, h = d.h, tw = w < SP_TW ? w : SP_TW, th = h < SP_TH ? h : SP_TH, lw = 31 - __clz(tw), npx = th << lw;
    const int  ntx = w >> lw, ntiles = ntx * (h / th);
    const int  bd = aux.bd, r0 = aux.r0, maxv = (1 << bd) - 1;
    const bool compound = FORM ? aux.mode != 0 : d.compound != 0;
    const int  r1 = compound ? aux.r1_compound : aux.r1_single, npass = !FORM && d.compound != 0 ? 2 : 1;
    const int  ob = bd + 14 - r0, ro = (1 << (ob - r1)) + (1 << (ob - r1 - 1)), rb = 14 - r0 - r1; // offset_bits, round_offset, bits
    for (int t = 0; t < ntiles; t++) {
        const int ty = t / ntx, x0 = (t - ty * ntx) << lw, y0 = ty * th;
        PIX*      out = dst_base + d.dst_off + (size_t)y0 * d.dst_stride + x0;
        int       a[SP_NPL] = {}; // the first reference's ConvBufType values
        for (int pass = 0; pass < npass; pass++) {
            // (selects, not indexing by `pass`: the descriptor stays in scalar registers)
            const int      sx = pass ? d.subpel_x[1] : d.subpel_x[0], sy = pass ? d.subpel_y[1] : d.subpel_y[0], xs = pass ? d.xs[1] : d.xs[0], ys = pass ? d.ys[1] : d.ys[0];
            const uint32_t stride = pass ? d.src_stride[1] : d.src_stride[0];
            const PIX*     src    = (const PIX*)planes.base[pass ? d.plane[1] : d.plane[0]] + (pass ? d.src_off[1] : d.src_off[0]);
            const bool     scaled = FORM || xs != 1024 || ys != 1024;
            const int      cs     = scaled ? 3 : ((sx >> 6) != 0) + 2 * ((sy >> 6) != 0); // the unscaled case: bit 0 filtered in x, bit 1 in y
            const int16_t* fxp    = FORM ? aux.fx : &kInterFilters[filter_kind(d.filter_x, w)][0][0];
            const int16_t* fyp    = FORM ? aux.fy : &kInterFilters[filter_kind(d.filter_y, h)][0][0];
            int            v[SP_NPL];
            if (cs == 3) {
                // horizontal pass of the rows the tile touches -> im, rounded and narrowed like the C's int16_t im_block; im row r <-> source row brow - 3 + r
                const int yq0 = sy + y0 * ys, brow = yq0 >> 10, frac = yq0 & 1023, imrows = (((th - 1) * ys + frac) >> 10) + 8;
                const PIX* pb = src + ((long)(brow - 3) * (long)stride - 3);
                for (int i = tid; i < (imrows << lw); i += TPB) {
                    const int xq = sx + (x0 + (i & (tw - 1))) * xs;
                    const int s  = hsum8(pb + ((size_t)(i >> lw) * stride + (size_t)(xq >> 10)), load_taps(fxp + ((xq & 1023) >> 6) * 8), 1 << (bd + 6));
                    im[i]        = (int16_t)rpot(s, r0);
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < SP_NPL; j++) {
                    const int i = tid + TPB * j;
                    if (i < npx) {
                        const int      yq = frac + (i >> lw) * ys;
                        const Taps4    f  = load_taps(fyp + ((yq & 1023) >> 6) * 8);
                        const int16_t* c  = im + ((yq >> 10) << lw) + (i & (tw - 1));
                        int            s  = 1 << ob;
#pragma unroll
                        for (int k = 0; k < 4; k++) s = sdot2(pack2(c[(2 * k) << lw], c[(2 * k + 1) << lw]), f.h2[k], s);
                        int res = rpot(s, r1);
                        if (compound || scaled) res = (int)(uint16_t)res; // ConvBufType res (:465, :823; :530, :1017)
                        if (!compound) {
                            res -= ro;
                            if (!scaled && sizeof(PIX) == 1) res = (int16_t)res; // the unscaled 8-bit function narrows before the last rounding (:345)
                            res = rpot(res, rb);
                        }
                        v[j] = res;
                    }
                }
                __syncthreads(); // im is rewritten by the next reference / tile
            } else {
                // an unscaled reference that is not filtered in both directions: svt_av1_[highbd_][jnt_]convolve_{2d_copy, x, y}[_sr]_c, read inside the block in
                // the unfiltered direction
                const int16_t* fx = fxp + (sx >> 6) * 8;
                const int16_t* fy = fyp + (sy >> 6) * 8;
#pragma unroll
                for (int j = 0; j < SP_NPL; j++) {
                    const int i = tid + TPB * j;
                    if (i < npx) {
                        const PIX* q = src + ((size_t)(y0 + (i >> lw)) * stride + (size_t)(x0 + (i & (tw - 1))));
                        if (cs == 0) {
                            const int px = load_px(q);
                            v[j]         = compound ? (int)(uint16_t)((px << rb) + ro) : px; // jnt_convolve_2d_copy shifts and offsets in 16 bits (:650-651)
                        } else if (cs == 1) {
                            const int s = rpot(hsum8(q - 3, load_taps(fx), 0), r0);
                            v[j]        = compound ? (1 << (7 - r1)) * s + ro : rpot(s, 7 - r0);
                        } else {
                            int s = 0;
#pragma unroll
                            for (int k = 0; k < 8; k++) s += (int)fy[k] * load_px(q + (long)(k - 3) * (long)stride);
                            v[j] = compound ? rpot(s * (1 << (7 - r0)), r1) + ro : rpot(s, 7);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < SP_NPL; j++) {
                const int i = tid + TPB * j;
                if (i >= npx) continue;
                const int yy = i >> lw, xx = i & (tw - 1);
                if (!compound) out[(size_t)yy * d.dst_stride + xx] = (PIX)clampi(v[j], 0, maxv);
                else if (FORM && aux.mode == 1) aux.cb[(size_t)(y0 + yy) * aux.cb_stride + x0 + xx] = (uint16_t)v[j];
                else if (pass + 1 < npass) a[j] = (int)(uint16_t)v[j]; // as the reference stores it: ConvBufType
                else {
                    int tmp = FORM ? (int)aux.cb[(size_t)(y0 + yy) * aux.cb_stride + x0 + xx] : a[j];
                    if (d.compound == 2) tmp = (tmp * (int)d.fwd_offset + v[j] * (int)d.bck_offset) >> 4; // DIST_PRECISION_BITS
                    else tmp = (tmp + v[j]) >> 1;
                    out[(size_t)yy * d.dst_stride + xx] = (PIX)clampi(rpot(tmp - ro, rb), 0, maxv);
                }
            }
        }
    }
}

// descriptors the host cannot read: every thread looks at a few; whoever finds an invalid one stores 1 into the word the host zeroed (plain stores of one value)
__global__ __launch_bounds__(TPB) void scaled_pred_check_kernel(const SvtHipInterPredPlanes planes, const SvtHipScaledPredDesc* __restrict__ descs, const uint32_t n,
                                                                uint32_t* __restrict__ bad_out) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) bad |= !sp_desc_ok(descs[i], planes);
    if (bad) *bad_out = 1;
}

// One block from host memory: the rectangle the C reads (3 left / above of src, 4 right of / below the last stepped position) goes into the call's arena with the
// two 16 x 8 tap tables and one descriptor.  One synchronisation (the download); nothing of the caller's is written before it.
template <typename PIX>
void scale_host(const PIX* src, const int src_stride, PIX* dst, const int dst_stride, const int w, const int h, const SvtHipInterpFilterParams* fx,
                const SvtHipInterpFilterParams* fy, const int sx, const int xs, const int sy, const int ys, const SvtHipConvolveParams* cp, const int bd) {
    if (!src || !dst || !fx || !fy || !cp || !fx->filter_ptr || !fy->filter_ptr) return; // nothing is written
    if (!sp_dim_ok((uint32_t)w) || !sp_dim_ok((uint32_t)h) || fx->taps != 8 || fy->taps != 8) return;
    if (sx < 0 || sx > 1023 || sy < 0 || sy > 1023 || xs < 64 || xs > 2048 || ys < 64 || ys > 2048) return;
    if (sizeof(PIX) == 1 ? bd != 8 : (bd != 10 && bd != 12)) return;
    const bool comp = cp->is_compound != 0, average = comp && cp->do_average;
    if (cp->round_0 < 0 || cp->round_0 > 7 || cp->round_1 < 0 || cp->round_0 + cp->round_1 > 14 || (comp && cp->round_1 > 7)) return;
    if (comp && !cp->dst) return;
    const size_t sw = (size_t)((((w - 1) * xs + sx) >> 10) + 8), sh = (size_t)((((h - 1) * ys + sy) >> 10) + 8), px = sizeof(PIX), blk = (size_t)w * h;
    svthip::HostCall& c = svthip::host_call();
    c.begin_small();
    const size_t bytes = sw * sh * px + blk * (px + 2) + 2 * 256 + sizeof(SvtHipScaledPredDesc) + 4096;
    c.reserve(bytes, bytes);
    PIX*                  ds  = (PIX*)c.dalloc(sw * sh * px);
    PIX*                  dd  = (PIX*)c.dalloc(blk * px);
    uint16_t*             db  = (uint16_t*)c.dalloc(blk * 2);
    int16_t*              dfx = (int16_t*)c.dalloc(256);
    int16_t*              dfy = (int16_t*)c.dalloc(256);
    SvtHipScaledPredDesc* dv  = (SvtHipScaledPredDesc*)c.dalloc(sizeof(SvtHipScaledPredDesc));
    c.up2d(ds, sw * px, src - (ptrdiff_t)3 * src_stride - 3, (size_t)src_stride * px, sw * px, sh);
    c.up(dfx, fx->filter_ptr, 256);
    c.up(dfy, fy->filter_ptr, 256);
    if (average) c.up2d(db, (size_t)w * 2, cp->dst, (size_t)cp->dst_stride * 2, (size_t)w * 2, h);
    SvtHipScaledPredDesc d{};
    d.src_off[0]    = 3 * sw + 3;
    d.src_stride[0] = (uint32_t)sw;
    d.dst_stride    = (uint32_t)w;
    d.w = (uint8_t)w, d.h = (uint8_t)h;
    d.subpel_x[0] = (uint16_t)sx, d.subpel_y[0] = (uint16_t)sy, d.xs[0] = (uint16_t)xs, d.ys[0] = (uint16_t)ys;
    d.compound   = (uint8_t)(average && cp->use_dist_wtd_comp_avg ? 2 : 0); // (mode 2 averages whatever this says; mode 1 never averages)
    d.fwd_offset = (uint8_t)(average ? cp->fwd_offset : 0);
    d.bck_offset = (uint8_t)(average ? cp->bck_offset : 0);
    c.up(dv, &d, sizeof(d));
    SvtHipInterPredPlanes planes{};
    planes.base[0] = ds;
    ScaleAux aux{};
    aux.cb = db, aux.cb_stride = (uint32_t)w;
    aux.mode = comp ? (average ? 2 : 1) : 0;
    aux.bd = bd, aux.r0 = cp->round_0, aux.r1_single = aux.r1_compound = cp->round_1;
    aux.fx = dfx, aux.fy = dfy;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(scaled_pred_kernel<PIX, true>), dim3(1), dim3(TPB), 0, c.stream, planes, dd, (const SvtHipScaledPredDesc*)dv, 1u, (uint8_t*)nullptr, aux);
    SVT_LAUNCH_CHECK();
    if (comp && !average) c.down2d(cp->dst, (size_t)cp->dst_stride * 2, db, (size_t)w * 2, (size_t)w * 2, h);
    else c.down2d(dst, (size_t)dst_stride * px, dd, (size_t)w * px, (size_t)w * px, h);
}

// =====================================================================================================================================================
// B. picture resize
// =====================================================================================================================================================
enum { RS_COPY = 0, RS_DOWN2_EVEN = 1, RS_DOWN2_ODD = 2, RS_INTERP = 3 };
__device__ __forceinline__ const int16_t* resize_table(const int t) {
    return t == 0 ? &kUpscaleFilter[0][0] : t == 1 ? &kResizeFilter875[0][0] : t == 2 ? &kResizeFilter750[0][0] : t == 3 ? &kResizeFilter625[0][0] : &kResizeFilter500[0][0];
}
// One step of resize_multistep over a plane: out_w x out_h samples, each from the line (row or, vertical != 0, column) of in_len samples it lies on.
//   RS_DOWN2_EVEN svt_av1_[highbd_]down2_symeven_c (resize.c:166), RS_DOWN2_ODD down2_symodd (:213), RS_INTERP svt_av1_[highbd_]interpolate_core_c (:276) with
//   delta / offset as computed there (position offset + RS_SCALE_EXTRA_OFF + i * delta, 14 fraction bits, the top 6 the table row).
template <typename PIX>
__global__ __launch_bounds__(TPB) void resize_pass_kernel(const PIX* __restrict__ src, const uint32_t s_stride, PIX* __restrict__ dst, const uint32_t d_stride,
                                                          const int in_len, const int out_w, const int out_h, const int vertical, const int kind, const int table,
                                                          const int delta, const int offset, const int maxv) {
    const int x = blockIdx.x * TPB + threadIdx.x, y = blockIdx.y;
    if (x >= out_w) return;
    const int    i    = vertical ? y : x;                                                    // index along the filtered line
    const PIX*   line = vertical ? src + x : src + (size_t)y * s_stride;                     // its first sample
    const size_t step = vertical ? s_stride : 1;
    int          r;
    if (kind == RS_COPY) r = load_px(line + (size_t)i * step);
    else if (kind == RS_INTERP) {
        const int      pos = offset + 128 + i * delta, p0 = (pos >> 14) - 3; // RS_SCALE_EXTRA_OFF; SUBPEL_TAPS / 2 - 1
        const int16_t* f   = resize_table(table) + ((pos >> 8) & 63) * 8;
        int            s;
        if (!vertical && p0 >= 0 && p0 + 7 < in_len) s = hsum8(line + p0, load_taps(f), 0);
        else s = csum8(line, step, p0, 0, in_len - 1, f, 0);
        r = clampi(rpot(s, 7), 0, maxv);
    } else {
        const int c = 2 * i, hi = in_len - 1;
        int       s = 64; // 1 << (FILTER_BITS - 1)
        if (kind == RS_DOWN2_EVEN) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                s += (load_px(line + (size_t)clampi(c - j, 0, hi) * step) + load_px(line + (size_t)clampi(c + 1 + j, 0, hi) * step)) * (int)kDown2SymEven[j];
        } else {
            s += load_px(line + (size_t)c * step) * (int)kDown2SymOdd[0];
#pragma unroll
            for (int j = 1; j < 4; j++)
                s += (load_px(line + (size_t)clampi(c - j, 0, hi) * step) + load_px(line + (size_t)clampi(c + j, 0, hi) * step)) * (int)kDown2SymOdd[j];
        }
        r = clampi(s >> 7, 0, maxv);
    }
    dst[(size_t)y * d_stride + x] = (PIX)r;
}

int down2_length(const int length) { return (length + 1) >> 1; }
int down2_steps(int in_length, const int out_length) { // get_down2_steps (resize.c:150)
    int steps = 0, proj;
    while ((proj = down2_length(in_length)) >= out_length) {
        ++steps;
        in_length = proj;
        if (in_length == 1) break;
    }
    return steps;
}
int interp_table(const int in_length, const int out_length) { // choose_interp_filter (resize.c:262)
    const int o16 = out_length * 16;
    return o16 >= in_length * 16 ? 0 : o16 >= in_length * 13 ? 1 : o16 >= in_length * 11 ? 2 : o16 >= in_length * 9 ? 3 : 4;
}
bool resize_desc_ok(const SvtHipResizeDesc& d) {
    return d.src && d.dst && d.width > 0 && d.height > 0 && d.width2 > 0 && d.height2 > 0 && d.width <= 65536 && d.height <= 65535 && d.width2 <= 65536 &&
        d.height2 <= 65535 && d.in_stride >= d.width && d.out_stride >= d.width2;
}
// the workspace of one plane, in samples: the width2 x height intermediate, then two buffers for what a factor-of-two step leaves (rows: at most
// ceil(width / 2) x height; columns: width2 x ceil(height / 2))
struct ResizePlan { size_t inter, tmp; };
ResizePlan resize_plan(const SvtHipResizeDesc& d) {
    ResizePlan p;
    p.inter = (size_t)d.width2 * d.height;
    p.tmp   = std::max((size_t)down2_length(d.width) * d.height, (size_t)d.width2 * down2_length(d.height));
    return p;
}
size_t resize_plane_bytes(const SvtHipResizeDesc& d, const size_t px) {
    const ResizePlan p = resize_plan(d);
    return svthip::align_up(p.inter * px, 256) + 2 * svthip::align_up(p.tmp * px, 256);
}
// resize_multistep (resize.c:350) for every line of a plane: `length` -> `olength` along rows (vertical = 0: `lines` rows) or columns (vertical = 1: `lines` columns)
template <typename PIX>
void resize_direction(const PIX* src, const uint32_t s_stride, PIX* dst, const uint32_t d_stride, const int length, const int olength, const int lines, const int vertical,
                      PIX* tmp0, PIX* tmp1, const int maxv, hipStream_t st) {
    const auto pass = [&](const PIX* in, const uint32_t in_stride, PIX* out, const uint32_t out_stride, const int in_len, const int out_len, const int kind) {
        const int out_w = vertical ? lines : out_len, out_h = vertical ? out_len : lines;
        int       delta = 0, offset = 0, table = 0;
        if (kind == RS_INTERP) { // svt_av1_interpolate_core_c (resize.c:278-281)
            delta  = (int)((((uint32_t)in_len << 14) + (uint32_t)(out_len / 2)) / (uint32_t)out_len);
            offset = in_len > out_len ? (int)((((int64_t)(in_len - out_len) << 13) + out_len / 2) / out_len) : -(int)((((int64_t)(out_len - in_len) << 13) + out_len / 2) / out_len);
            table  = interp_table(in_len, out_len);
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(resize_pass_kernel<PIX>), dim3((out_w + TPB - 1) / TPB, out_h), dim3(TPB), 0, st, in, in_stride, out, out_stride, in_len, out_w,
                           out_h, vertical, kind, table, delta, offset, maxv);
        SVT_LAUNCH_CHECK();
    };
    if (length == olength) return pass(src, s_stride, dst, d_stride, length, olength, RS_COPY);
    const int steps = down2_steps(length, olength);
    if (steps == 0) return pass(src, s_stride, dst, d_stride, length, olength, RS_INTERP);
    const PIX* in        = src;
    uint32_t   in_stride = s_stride;
    int        filtered  = length;
    for (int s = 0; s < steps; s++) {
        const int proj  = down2_length(filtered);
        const bool last = s == steps - 1 && proj == olength;
        PIX*      out   = last ? dst : ((s & 1) ? tmp1 : tmp0);
        const uint32_t out_stride = last ? d_stride : (vertical ? (uint32_t)lines : (uint32_t)proj); // a packed temporary
        pass(in, in_stride, out, out_stride, filtered, proj, (filtered & 1) ? RS_DOWN2_ODD : RS_DOWN2_EVEN);
        in = out, in_stride = out_stride, filtered = proj;
    }
    if (filtered != olength) pass(in, in_stride, dst, d_stride, filtered, olength, RS_INTERP);
}
template <typename PIX> void resize_plane_launch(const SvtHipResizeDesc& d, uint8_t* ws, const int bd, hipStream_t st) {
    const ResizePlan p     = resize_plan(d);
    PIX*             inter = (PIX*)ws;
    PIX*             tmp0  = (PIX*)(ws + svthip::align_up(p.inter * sizeof(PIX), 256));
    PIX*             tmp1  = (PIX*)((uint8_t*)tmp0 + svthip::align_up(p.tmp * sizeof(PIX), 256));
    const int        maxv  = (1 << bd) - 1;
    if (d.height2 == d.height) // svt_av1_[highbd_]resize_plane_horizontal (resize.c:440, :716): the rows go straight to the output
        return resize_direction<PIX>((const PIX*)d.src, (uint32_t)d.in_stride, (PIX*)d.dst, (uint32_t)d.out_stride, d.width, d.width2, d.height, 0, tmp0, tmp1, maxv, st);
    resize_direction<PIX>((const PIX*)d.src, (uint32_t)d.in_stride, inter, (uint32_t)d.width2, d.width, d.width2, d.height, 0, tmp0, tmp1, maxv, st);
    resize_direction<PIX>(inter, (uint32_t)d.width2, (PIX*)d.dst, (uint32_t)d.out_stride, d.height, d.height2, d.width2, 1, tmp0, tmp1, maxv, st);
}
int resize_batch(const SvtHipResizeDesc* descs, const uint32_t n, const int bd, void* workspace, const size_t workspace_bytes, hipStream_t st) {
    const size_t px = bd > 8 ? 2 : 1;
    size_t       need = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!resize_desc_ok(descs[i])) return -1;
        need += resize_plane_bytes(descs[i], px);
    }
    if (!workspace || workspace_bytes < need) return -1;
    uint8_t* ws = (uint8_t*)workspace;
    for (uint32_t i = 0; i < n; i++) {
        if (bd > 8) resize_plane_launch<uint16_t>(descs[i], ws, bd, st);
        else resize_plane_launch<uint8_t>(descs[i], ws, bd, st);
        ws += resize_plane_bytes(descs[i], px);
    }
    return 0;
}
// one plane from host memory: upload, the batched entry's launches on the calling thread's stream, download
template <typename PIX>
uint32_t resize_host(const PIX* input, const int height, const int width, const int in_stride, PIX* output, const int height2, const int width2, const int out_stride,
                     const int bd) {
    constexpr uint32_t kNone = 0, kInsufficient = 0x80001000u, kBadParameter = 0x80001005u; // EB_ErrorNone, EB_ErrorInsufficientResources, EB_ErrorBadParameter
    SvtHipResizeDesc   d{};
    d.src = input, d.dst = output, d.width = width, d.height = height, d.in_stride = in_stride, d.width2 = width2, d.height2 = height2, d.out_stride = out_stride;
    if (!resize_desc_ok(d) || (sizeof(PIX) == 1 ? bd != 8 : (bd != 8 && bd != 10 && bd != 12))) return kBadParameter;
    if (svthip::failed()) return kInsufficient;
    try {
        const size_t      px = sizeof(PIX), in_bytes = (size_t)width * height * px, out_bytes = (size_t)width2 * height2 * px, ws_bytes = resize_plane_bytes(d, px);
        svthip::HostCall& c  = svthip::host_call();
        c.begin();
        c.reserve(in_bytes + out_bytes + ws_bytes + 4096, in_bytes + out_bytes + 4096);
        PIX*     di = (PIX*)c.dalloc(in_bytes);
        PIX*     dout = (PIX*)c.dalloc(out_bytes);
        uint8_t* ws = (uint8_t*)c.dalloc(ws_bytes);
        c.up2d(di, (size_t)width * px, input, (size_t)in_stride * px, (size_t)width * px, height);
        d.src = di, d.dst = dout, d.in_stride = width, d.out_stride = width2;
        resize_plane_launch<PIX>(d, ws, bd, c.stream);
        c.down2d(output, (size_t)out_stride * px, dout, (size_t)width2 * px, (size_t)width2 * px, height2);
    } catch (const svthip::DeviceError&) { return kInsufficient; }
    return kNone;
}

// =====================================================================================================================================================
// C. super-resolution normative upscale
// =====================================================================================================================================================
constexpr int UP_PLANES = 3; // planes per launch (their tile-column lists travel as kernel arguments)
struct UpPlane {
    const void* src;
    void*       dst;
    int32_t     src_stride, dst_stride, rows, width2, step, lo, hi, maxv, ncols, two_byte;
    int32_t     x0[64];        // x0_qn of each tile column (super_res.c:223, :282)
    uint16_t    dst_start[64]; // upscaled_x0
    uint16_t    src_start[64]; // downscaled_x0
};
struct UpArgs { UpPlane p[UP_PLANES]; };

template <typename PIX> __device__ __forceinline__ void upscale_sample(const UpPlane& P, const int x, const int y) {
    // the tile column of x: the last one that starts at or before it (a uniform walk; pictures have a handful)
    int ds = P.dst_start[0], ss = P.src_start[0], x0 = P.x0[0];
    for (int j = 1; j < P.ncols; j++)
        if ((int)P.dst_start[j] <= x) ds = P.dst_start[j], ss = P.src_start[j], x0 = P.x0[j];
    const int      xq = x0 + (x - ds) * P.step;
    const int      p0 = ss - 1 - 3 + (xq >> 14); // the C filters from input - 1 (:130), minus UPSCALE_NORMATIVE_TAPS / 2 - 1 (:56)
    const int16_t* f  = &kUpscaleFilter[(xq & 16383) >> 8][0];
    const PIX*     row = (const PIX*)P.src + (size_t)y * P.src_stride;
    int            s;
    if (p0 >= P.lo && p0 + 7 <= P.hi) s = hsum8(row + p0, load_taps(f), 0);
    else s = csum8(row, 1, p0, P.lo, P.hi, f, 0); // a frame edge: the edge sample, replicated
    ((PIX*)P.dst)[(size_t)y * P.dst_stride + x] = (PIX)clampi(rpot(s, 7), 0, P.maxv);
}
__global__ __launch_bounds__(TPB) void upscale_kernel(const UpArgs args) {
    const UpPlane& P = args.p[blockIdx.z];
    const int      x = blockIdx.x * TPB + threadIdx.x, y = blockIdx.y;
    if (x >= P.width2 || y >= P.rows) return;
    if (P.two_byte) upscale_sample<uint16_t>(P, x, y);
    else upscale_sample<uint8_t>(P, x, y);
}
// svt_av1_upscale_normative_rows' walk over the tile columns (super_res.c:222-283)
bool upscale_plan(const SvtHipUpscaleDesc& d, UpPlane& P) {
    if (!d.src || !d.dst || d.rows < 1 || d.rows > 65535 || d.downscaled_plane_width < 1 || d.upscaled_plane_width < d.downscaled_plane_width ||
        d.upscaled_plane_width > 65535 || d.superres_denom < 8 || d.superres_denom > 16 || d.sub_x > 1 || d.n_tile_cols < 1 || d.n_tile_cols > 64)
        return false;
    if ((d.bd != 8 && d.bd != 10 && d.bd != 12) || (d.sample_bytes != 1 && d.sample_bytes != 2) || (d.sample_bytes == 1 && d.bd != 8)) return false;
    const int down = d.downscaled_plane_width, up = d.upscaled_plane_width;
    if (d.src_stride < down || d.dst_stride < up) return false;
    P.src = d.src, P.dst = d.dst, P.src_stride = d.src_stride, P.dst_stride = d.dst_stride, P.rows = d.rows, P.width2 = up;
    P.maxv = (1 << d.bd) - 1, P.ncols = d.n_tile_cols, P.two_byte = d.sample_bytes == 2;
    P.step = ((down << 14) + up / 2) / up; // av1_get_upscale_convolve_step (:43)
    const int err = up * P.step - (down << 14);
    int       x0  = (-((up - down) << 13) + up / 2) / up + 128 - err / 2; // get_upscale_convolve_x0 (:47)
    x0            = (int)((uint32_t)x0 & 16383u);
    const int sh  = 2 - d.sub_x; // MI_SIZE_LOG2 - sub_x
    for (int j = 0; j < d.n_tile_cols; j++) {
        const int mi0 = d.tile_col_start_mi[j], mi1 = d.tile_col_start_mi[j + 1];
        if (mi0 < 0 || mi1 <= mi0 || mi1 > (65535 >> sh)) return false;
        const int dx0 = mi0 << sh, dx1 = mi1 << sh, ux0 = dx0 * d.superres_denom / 8, ux1 = j == d.n_tile_cols - 1 ? up : dx1 * d.superres_denom / 8;
        if (ux1 < ux0 || ux1 > up || (j == 0 && ux0 != 0)) return false;
        P.x0[j] = x0, P.dst_start[j] = (uint16_t)ux0, P.src_start[j] = (uint16_t)dx0;
        x0 += (ux1 - ux0) * P.step - ((dx1 - dx0) << 14);
    }
    P.lo = d.tile_col_start_mi[0] << sh;                  // pad_left: the first tile column's first sample
    P.hi = (d.tile_col_start_mi[d.n_tile_cols] << sh) - 1; // pad_right: the last tile column's last sample
    if (d.src_stride <= P.hi) return false;               // (that sample lies inside the row)
    return true;
}
int upscale_batch(const SvtHipUpscaleDesc* descs, const uint32_t n, hipStream_t st) {
    std::vector<UpPlane> planes(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!upscale_plan(descs[i], planes[i])) return -1;
        // src and dst must not overlap
        const uint8_t *s0 = (const uint8_t*)descs[i].src, *d0 = (const uint8_t*)descs[i].dst;
        const size_t   sb = (size_t)descs[i].src_stride * descs[i].rows * descs[i].sample_bytes, db = (size_t)descs[i].dst_stride * descs[i].rows * descs[i].sample_bytes;
        if (s0 < d0 + db && d0 < s0 + sb) return -1;
    }
    for (uint32_t i = 0; i < n; i += UP_PLANES) {
        UpArgs   a{};
        const uint32_t m = std::min<uint32_t>(UP_PLANES, n - i);
        int      mw = 0, mr = 0;
        for (uint32_t k = 0; k < m; k++) a.p[k] = planes[i + k], mw = std::max(mw, planes[i + k].width2), mr = std::max(mr, planes[i + k].rows);
        hipLaunchKernelGGL(upscale_kernel, dim3((mw + TPB - 1) / TPB, mr, m), dim3(TPB), 0, st, a);
        SVT_LAUNCH_CHECK();
    }
    return 0;
}

} // namespace

extern "C" {

int svt_hip_inter_pred_scaled_batch(SvtHipInterPredPlanes planes, void* dst_base, const SvtHipScaledPredDesc* descs, uint32_t n, int bit_depth, uint8_t* status,
                                    void* stream) {
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
        hipLaunchKernelGGL(scaled_pred_check_kernel, dim3(n < 1024u * TPB ? (n + TPB - 1) / TPB : 1024u), dim3(TPB), 0, st, planes, descs, n, bad);
        SVT_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(st));
        if (*(volatile uint32_t*)bad) return -1;
    }
    ScaleAux aux{};
    aux.bd          = bit_depth;
    aux.r0          = bit_depth == 12 ? 5 : 3; // get_conv_params_no_round: ROUND0_BITS, raised while bd + FILTER_BITS - round_0 + 2 > 16
    aux.r1_single   = 14 - aux.r0;
    aux.r1_compound = 7;                       // COMPOUND_ROUND1_BITS
    if (bit_depth > 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(scaled_pred_kernel<uint16_t, false>), dim3(n), dim3(TPB), 0, st, planes, (uint16_t*)dst_base, descs, n, status, aux);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(scaled_pred_kernel<uint8_t, false>), dim3(n), dim3(TPB), 0, st, planes, (uint8_t*)dst_base, descs, n, status, aux);
    SVT_LAUNCH_CHECK();
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

void svt_av1_convolve_2d_scale_hip(const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride, int w, int h, const SvtHipInterpFilterParams* filter_params_x,
                                   const SvtHipInterpFilterParams* filter_params_y, const int subpel_x_qn, const int x_step_qn, const int subpel_y_qn,
                                   const int y_step_qn, SvtHipConvolveParams* conv_params) {
    if (svthip::failed()) return;
    try {
        scale_host<uint8_t>(src, src_stride, dst, dst_stride, w, h, filter_params_x, filter_params_y, subpel_x_qn, x_step_qn, subpel_y_qn, y_step_qn, conv_params, 8);
    } catch (const svthip::DeviceError&) {}
}
void svt_av1_highbd_convolve_2d_scale_hip(const uint16_t* src, int src_stride, uint16_t* dst, int dst_stride, int w, int h,
                                          const SvtHipInterpFilterParams* filter_params_x, const SvtHipInterpFilterParams* filter_params_y, const int subpel_x_qn,
                                          const int x_step_qn, const int subpel_y_qn, const int y_step_qn, SvtHipConvolveParams* conv_params, int bd) {
    if (svthip::failed()) return;
    try {
        scale_host<uint16_t>(src, src_stride, dst, dst_stride, w, h, filter_params_x, filter_params_y, subpel_x_qn, x_step_qn, subpel_y_qn, y_step_qn, conv_params, bd);
    } catch (const svthip::DeviceError&) {}
}

size_t svt_hip_resize_workspace_bytes(const SvtHipResizeDesc* descs, uint32_t n, int bit_depth) {
    if (!descs || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12)) return 0;
    size_t need = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!resize_desc_ok(descs[i])) return 0;
        need += resize_plane_bytes(descs[i], bit_depth > 8 ? 2 : 1);
    }
    return need;
}
int svt_hip_resize_plane_batch(const SvtHipResizeDesc* descs, uint32_t n, int bit_depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) return -1;
    if (n == 0) return 0;
    if (!descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    int r = 0;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    r = resize_batch(descs, n, bit_depth, workspace, workspace_bytes, (hipStream_t)stream);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return r;
}
SvtHipErrorType svt_av1_resize_plane_hip(const uint8_t* const input, int height, int width, int in_stride, uint8_t* output, int height2, int width2, int out_stride) {
    return (SvtHipErrorType)resize_host<uint8_t>(input, height, width, in_stride, output, height2, width2, out_stride, 8);
}
SvtHipErrorType svt_av1_highbd_resize_plane_hip(const uint16_t* const input, int height, int width, int in_stride, uint16_t* output, int height2, int width2,
                                                int out_stride, int bd) {
    return (SvtHipErrorType)resize_host<uint16_t>(input, height, width, in_stride, output, height2, width2, out_stride, bd);
}

int svt_hip_superres_upscale_batch(const SvtHipUpscaleDesc* descs, uint32_t n, void* stream) {
    if (n == 0) return 0;
    if (!descs) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    int r = 0;
    SVT_HIP_ENTRY_TRY
    svthip::ensure_device();
    r = upscale_batch(descs, n, (hipStream_t)stream);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return r;
}
int svt_hip_upscale_normative_rows_host(const void* src, int src_stride, void* dst, int dst_stride, int rows, int downscaled_plane_width, int upscaled_plane_width,
                                        int superres_denom, int sub_x, int n_tile_cols, const int32_t* tile_col_start_mi, int bd, int sample_bytes) {
    if (!src || !dst || !tile_col_start_mi || n_tile_cols < 1 || n_tile_cols > 64 || rows < 1 || (sample_bytes != 1 && sample_bytes != 2)) return -1;
    if (svthip::failed()) return SVT_HIP_E_DEVICE;
    SVT_HIP_ENTRY_TRY
    SvtHipUpscaleDesc d{};
    d.rows = rows, d.downscaled_plane_width = downscaled_plane_width, d.upscaled_plane_width = upscaled_plane_width;
    d.superres_denom = (uint8_t)superres_denom, d.sub_x = (uint8_t)sub_x, d.bd = (uint8_t)bd, d.sample_bytes = (uint8_t)sample_bytes, d.n_tile_cols = n_tile_cols;
    for (int j = 0; j <= n_tile_cols; j++) d.tile_col_start_mi[j] = tile_col_start_mi[j];
    if (superres_denom < 8 || superres_denom > 16 || sub_x < 0 || sub_x > 1 || tile_col_start_mi[0] != 0) return -1;
    // the source rectangle: everything from the row's first sample to the last tile column's last sample
    const int sw = tile_col_start_mi[n_tile_cols] << (2 - sub_x);
    if (sw < 1 || sw > src_stride || upscaled_plane_width < 1 || upscaled_plane_width > dst_stride) return -1;
    d.src_stride = sw, d.dst_stride = upscaled_plane_width;
    const size_t px = (size_t)sample_bytes, in_bytes = (size_t)sw * rows * px, out_bytes = (size_t)upscaled_plane_width * rows * px;
    svthip::ensure_device();
    svthip::HostCall& c = svthip::host_call();
    c.begin();
    c.reserve(in_bytes + out_bytes + 4096, in_bytes + out_bytes + 4096);
    void* di = c.dalloc(in_bytes);
    void* dout = c.dalloc(out_bytes);
    d.src = di, d.dst = dout;
    UpPlane P;
    if (!upscale_plan(d, P)) return -1;
    c.up2d(di, (size_t)sw * px, src, (size_t)src_stride * px, (size_t)sw * px, rows);
    if (upscale_batch(&d, 1, c.stream) != 0) return -1;
    c.down2d(dst, (size_t)dst_stride * px, dout, (size_t)upscaled_plane_width * px, (size_t)upscaled_plane_width * px, rows);
    SVT_HIP_ENTRY_CATCH(SVT_HIP_E_DEVICE)
    return 0;
}

} // extern "C"
