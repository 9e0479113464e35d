/* abi_typecheck_scale.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the four forms of csrc/scale.hip that have a reference prototype.
 *
 * Compiled by tests/test_scale_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  Each `_hip` form is assigned to the run-time
 * dispatch pointer of common_dsp_rtcd.h / aom_dsp_rtcd.h it stands for -- the forms are exported, not installed, so they are not lines of
 * rtcd_hooks.def and this file is where their prototypes are proven.  Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

int svt_hip_abi_typecheck_scale(void) {
    int n = 0;
    svt_av1_convolve_2d_scale = svt_av1_convolve_2d_scale_hip; n++;
    svt_av1_highbd_convolve_2d_scale = svt_av1_highbd_convolve_2d_scale_hip; n++;
    svt_av1_resize_plane = svt_av1_resize_plane_hip; n++;
    svt_av1_highbd_resize_plane = svt_av1_highbd_resize_plane_hip; n++;
    return n;
}
