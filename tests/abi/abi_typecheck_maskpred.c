/* abi_typecheck_maskpred.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the fifteen masked-prediction forms of csrc/maskpred.hip.
 *
 * Compiled by tests/test_maskpred_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  Each `_hip` form is assigned to the run-time
 * dispatch pointer of common_dsp_rtcd.h / aom_dsp_rtcd.h it stands for -- the forms are exported, not installed, so they are not lines of
 * rtcd_hooks.def and this file is where their prototypes are proven.  Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

int svt_hip_abi_typecheck_maskpred(void) {
    int n = 0;
    svt_aom_blend_a64_mask = svt_aom_blend_a64_mask_hip; n++;
    svt_aom_highbd_blend_a64_mask = svt_aom_highbd_blend_a64_mask_hip; n++;
    svt_aom_blend_a64_hmask = svt_aom_blend_a64_hmask_hip; n++;
    svt_aom_blend_a64_vmask = svt_aom_blend_a64_vmask_hip; n++;
    svt_aom_highbd_blend_a64_hmask_16bit = svt_aom_highbd_blend_a64_hmask_16bit_hip; n++;
    svt_aom_highbd_blend_a64_vmask_16bit = svt_aom_highbd_blend_a64_vmask_16bit_hip; n++;
    svt_av1_build_compound_diffwtd_mask = svt_av1_build_compound_diffwtd_mask_hip; n++;
    svt_av1_build_compound_diffwtd_mask_highbd = svt_av1_build_compound_diffwtd_mask_highbd_hip; n++;
    svt_av1_wedge_sse_from_residuals = svt_av1_wedge_sse_from_residuals_hip; n++;
    svt_av1_wedge_sign_from_residuals = svt_av1_wedge_sign_from_residuals_hip; n++;
    svt_av1_wedge_compute_delta_squares = svt_av1_wedge_compute_delta_squares_hip; n++;
    svt_aom_sum_squares_i16 = svt_aom_sum_squares_i16_hip; n++;
    svt_aom_lowbd_blend_a64_d16_mask = svt_aom_lowbd_blend_a64_d16_mask_hip; n++;
    svt_aom_highbd_blend_a64_d16_mask = svt_aom_highbd_blend_a64_d16_mask_hip; n++;
    svt_av1_build_compound_diffwtd_mask_d16 = svt_av1_build_compound_diffwtd_mask_d16_hip; n++;
    return n;
}
