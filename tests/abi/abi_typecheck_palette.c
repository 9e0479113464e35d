/* abi_typecheck_palette.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the single-call forms of csrc/palette.hip.
 *
 * Compiled by tests/test_palette_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  The four k-means forms are assigned to the
 * run-time dispatch pointers of aom_dsp_rtcd.h they stand for.  The two colour counters are plain functions of the reference without a header: the test takes their
 * declarations from the reference's palette.c at run time, passes them in as SVT_PALETTE_COUNT_DECLS, and each form is assigned to a pointer of the function's own
 * type.  The forms are exported, not installed, so they are not lines of rtcd_hooks.def and this file is where their prototypes are proven.
 * Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

SVT_PALETTE_COUNT_DECLS

int svt_hip_abi_typecheck_palette(void) {
    int n = 0;
    svt_av1_k_means_dim1 = svt_av1_k_means_dim1_hip; n++;
    svt_av1_k_means_dim2 = svt_av1_k_means_dim2_hip; n++;
    svt_av1_calc_indices_dim1 = svt_av1_calc_indices_dim1_hip; n++;
    svt_av1_calc_indices_dim2 = svt_av1_calc_indices_dim2_hip; n++;
    __typeof__(&svt_av1_count_colors) count_colors = svt_av1_count_colors_hip; n++;
    __typeof__(&svt_av1_count_colors_highbd) count_colors_highbd = svt_av1_count_colors_highbd_hip; n++;
    (void)count_colors;
    (void)count_colors_highbd;
    return n;
}
