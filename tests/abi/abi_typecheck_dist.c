/* abi_typecheck_dist.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the RD distortion forms of csrc/dist.hip.
 *
 * Compiled by tests/test_dist_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  The four `_hip` forms that stand for a run-time
 * dispatch pointer of common_dsp_rtcd.h are assigned to that pointer -- they are exported, not installed, so they are not lines of rtcd_hooks.def and
 * this file is where their prototypes are proven --; the psy forms are assigned to pointers typed from the reference's own function declarations (psy_rd.h,
 * common_dsp_rtcd.h:165).  Nothing here is ever run. */
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "psy_rd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

int svt_hip_abi_typecheck_dist(void) {
    int n = 0;
    svt_spatial_full_distortion_kernel = svt_spatial_full_distortion_kernel_hip; n++;
    svt_full_distortion_kernel16_bits = svt_full_distortion_kernel16_bits_hip; n++;
    svt_full_distortion_kernel32_bits = svt_full_distortion_kernel32_bits_hip; n++;
    svt_full_distortion_kernel_cbf_zero32_bits = svt_full_distortion_kernel_cbf_zero32_bits_hip; n++;
    __typeof__(&svt_psy_distortion) psy8 = svt_psy_distortion_hip; n++;
    __typeof__(&svt_psy_distortion_hbd) psy16 = svt_psy_distortion_hbd_hip; n++;
    __typeof__(&get_svt_psy_full_dist) full = svt_get_psy_full_dist_hip; n++;
    __typeof__(&svt_spatial_psy_distortion_kernel_c) spatial = svt_spatial_psy_distortion_kernel_hip; n++;
    (void)psy8; (void)psy16; (void)full; (void)spatial;
    return n;
}
