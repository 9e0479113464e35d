/* abi_typecheck_interpred.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the sixteen inter-prediction forms of csrc/interpred.hip.
 *
 * Compiled by tests/test_interpred_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  Each `_hip` form is assigned to the run-time
 * dispatch pointer of common_dsp_rtcd.h it stands for -- the forms are exported, not installed, so they are not lines of rtcd_hooks.def and this file
 * is where their prototypes are proven.  SvtHipInterpFilterParams is InterpFilterParams here (SVT_HIP_REFERENCE_TYPES); the self-contained mirror of the header is
 * restated below under another name and static-asserted against the reference's struct, field by field.  Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

/* the definition include/svtav1_hip.h gives without SVT_HIP_REFERENCE_TYPES (tests/test_interpred_abi.py checks that this text is the header's) */
typedef struct SvtHipInterpFilterParamsMirror {
    const int16_t *filter_ptr;
    uint16_t       taps, subpel_shifts;
    uint32_t       interp_filter; /* InterpFilter, an int-sized enum */
} SvtHipInterpFilterParamsMirror;
#define SAME_FIELD(f)                                                                                                         \
    _Static_assert(offsetof(SvtHipInterpFilterParamsMirror, f) == offsetof(InterpFilterParams, f) &&                          \
                       sizeof(((SvtHipInterpFilterParamsMirror *)0)->f) == sizeof(((InterpFilterParams *)0)->f),             \
                   "SvtHipInterpFilterParams." #f " differs from InterpFilterParams")
_Static_assert(sizeof(SvtHipInterpFilterParamsMirror) == sizeof(InterpFilterParams), "SvtHipInterpFilterParams differs in size from InterpFilterParams");
SAME_FIELD(filter_ptr);
SAME_FIELD(taps);
SAME_FIELD(subpel_shifts);
SAME_FIELD(interp_filter);

int svt_hip_abi_typecheck_interpred(void) {
    int n = 0;
    svt_av1_convolve_2d_copy_sr = svt_av1_convolve_2d_copy_sr_hip; n++;
    svt_av1_convolve_x_sr = svt_av1_convolve_x_sr_hip; n++;
    svt_av1_convolve_y_sr = svt_av1_convolve_y_sr_hip; n++;
    svt_av1_convolve_2d_sr = svt_av1_convolve_2d_sr_hip; n++;
    svt_av1_jnt_convolve_2d_copy = svt_av1_jnt_convolve_2d_copy_hip; n++;
    svt_av1_jnt_convolve_x = svt_av1_jnt_convolve_x_hip; n++;
    svt_av1_jnt_convolve_y = svt_av1_jnt_convolve_y_hip; n++;
    svt_av1_jnt_convolve_2d = svt_av1_jnt_convolve_2d_hip; n++;
    svt_av1_highbd_convolve_2d_copy_sr = svt_av1_highbd_convolve_2d_copy_sr_hip; n++;
    svt_av1_highbd_convolve_x_sr = svt_av1_highbd_convolve_x_sr_hip; n++;
    svt_av1_highbd_convolve_y_sr = svt_av1_highbd_convolve_y_sr_hip; n++;
    svt_av1_highbd_convolve_2d_sr = svt_av1_highbd_convolve_2d_sr_hip; n++;
    svt_av1_highbd_jnt_convolve_2d_copy = svt_av1_highbd_jnt_convolve_2d_copy_hip; n++;
    svt_av1_highbd_jnt_convolve_x = svt_av1_highbd_jnt_convolve_x_hip; n++;
    svt_av1_highbd_jnt_convolve_y = svt_av1_highbd_jnt_convolve_y_hip; n++;
    svt_av1_highbd_jnt_convolve_2d = svt_av1_highbd_jnt_convolve_2d_hip; n++;
    return n;
}
