/* abi_typecheck_mdsubpel.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the single-call forms of csrc/mdsubpel.hip.
 *
 * Compiled by tests/test_mdsubpel_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  Each `_hip` form is assigned to the run-time
 * dispatch pointer of aom_dsp_rtcd.h it stands for -- the forms are exported, not installed, so they are not lines of rtcd_hooks.def and this file
 * is where their prototypes are proven.  Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

#define SVT_HIP_ASSIGN(W, H)                                                                   \
    svt_aom_variance##W##x##H = svt_aom_variance##W##x##H##_hip; n++;                           \
    svt_aom_sub_pixel_variance##W##x##H = svt_aom_sub_pixel_variance##W##x##H##_hip; n++;       \
    svt_aom_obmc_sad##W##x##H = svt_aom_obmc_sad##W##x##H##_hip; n++;                           \
    svt_aom_obmc_variance##W##x##H = svt_aom_obmc_variance##W##x##H##_hip; n++;                 \
    svt_aom_obmc_sub_pixel_variance##W##x##H = svt_aom_obmc_sub_pixel_variance##W##x##H##_hip; n++;

int svt_hip_abi_typecheck_mdsubpel(void) {
    int n = 0;
    SVT_HIP_FOR_ALL_VARIANCE_SIZES(SVT_HIP_ASSIGN)
    svt_aom_mse16x16 = svt_aom_mse16x16_hip; n++;
    svt_aom_upsampled_pred = svt_aom_upsampled_pred_hip; n++;
    return n;
}
