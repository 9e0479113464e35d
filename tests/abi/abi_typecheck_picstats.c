/* abi_typecheck_picstats.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the single-call forms of csrc/picstats.hip.
 *
 * Compiled by tests/test_picstats_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  The four `_hip` forms stand for the run-time
 * dispatch pointers of aom_dsp_rtcd.c:516-519 and are assigned to them -- they are exported, not installed, so they are not lines of rtcd_hooks.def
 * and this file is where their prototypes are proven.  Nothing here is ever run. */
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

int svt_hip_abi_typecheck_picstats(void) {
    int n = 0;
    svt_compute_mean_8x8 = svt_compute_mean_8x8_hip; n++;
    svt_compute_mean_square_values_8x8 = svt_compute_mean_square_values_8x8_hip; n++;
    svt_compute_sub_mean_8x8 = svt_compute_sub_mean_8x8_hip; n++;
    svt_compute_interm_var_four8x8 = svt_compute_interm_var_four8x8_hip; n++;
    return n;
}
