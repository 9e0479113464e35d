/* abi_typecheck_intrapred.c -- TEST INFRASTRUCTURE: the compile-time proof of abi_typecheck.c for the eleven intra-prediction forms of csrc/intrapred.hip.
 *
 * Compiled by tests/test_intrapred_abi.py (CPU, needs the reference's headers) with -Werror=incompatible-pointer-types.  Each `_hip` form is assigned to the run-time
 * dispatch pointer of common_dsp_rtcd.h it stands for -- the forms are exported, not installed, so they are not lines of rtcd_hooks.def and this file
 * is where their prototypes are proven.  SvtHipTxSize is TxSize here (SVT_HIP_REFERENCE_TYPES); without the reference's types the header spells it uint8_t, and the
 * static assertion below says that this is the packed enum's size.  Nothing here is ever run. */
#include <stddef.h>
#include "definitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#define SVT_HIP_REFERENCE_TYPES 1
#include "svtav1_hip.h"

_Static_assert(sizeof(TxSize) == sizeof(uint8_t), "SvtHipTxSize differs in size from TxSize");

int svt_hip_abi_typecheck_intrapred(void) {
    int n = 0;
    svt_av1_dr_prediction_z1 = svt_av1_dr_prediction_z1_hip; n++;
    svt_av1_dr_prediction_z2 = svt_av1_dr_prediction_z2_hip; n++;
    svt_av1_dr_prediction_z3 = svt_av1_dr_prediction_z3_hip; n++;
    svt_av1_highbd_dr_prediction_z1 = svt_av1_highbd_dr_prediction_z1_hip; n++;
    svt_av1_highbd_dr_prediction_z2 = svt_av1_highbd_dr_prediction_z2_hip; n++;
    svt_av1_highbd_dr_prediction_z3 = svt_av1_highbd_dr_prediction_z3_hip; n++;
    svt_av1_filter_intra_predictor = svt_av1_filter_intra_predictor_hip; n++;
    svt_cfl_predict_lbd = svt_cfl_predict_lbd_hip; n++;
    svt_cfl_predict_hbd = svt_cfl_predict_hbd_hip; n++;
    svt_cfl_luma_subsampling_420_lbd = svt_cfl_luma_subsampling_420_lbd_hip; n++;
    svt_cfl_luma_subsampling_420_hbd = svt_cfl_luma_subsampling_420_hbd_hip; n++;
    return n;
}
