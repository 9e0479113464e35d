"""Compile-time proof that the eleven intra-prediction forms of csrc/intrapred.hip have the reference's prototypes: each is assigned to its dispatch pointer of
common_dsp_rtcd.h -- tests/abi/abi_typecheck_intrapred.c under the flags of test_abi_typecheck.py.  Needs the reference's headers, so it runs in the build container
only, as its siblings do."""
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "common_dsp_rtcd.h")), reason="the reference's headers are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals"),
       "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
STRICT = ["-std=gnu11", "-fsyntax-only", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers", "-Werror=int-conversion",
          "-Werror=implicit-function-declaration"]
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_intrapred.c")


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def test_intra_prediction_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    assert base.count("_hip; n++;") == 11
    # teeth: a form assigned to a pointer of another prototype is rejected
    for ptr, wrong in (("svt_av1_highbd_dr_prediction_z1", "svt_av1_dr_prediction_z1_hip"),      # an 8-bit form in a highbd pointer (uint16_t samples, a trailing bd)
                       ("svt_av1_dr_prediction_z2", "svt_av1_highbd_dr_prediction_z2_hip"),       # and the other way round
                       ("svt_av1_dr_prediction_z1", "svt_av1_dr_prediction_z2_hip"),              # zone 2 takes one flag more
                       ("svt_cfl_predict_hbd", "svt_cfl_predict_lbd_hip"),
                       ("svt_cfl_luma_subsampling_420_lbd", "svt_cfl_luma_subsampling_420_hbd_hip"),
                       ("svt_av1_filter_intra_edge", "svt_av1_filter_intra_predictor_hip")):      # another function's pointer
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)
    # and the size assertion has teeth
    r = _cc(base.replace("sizeof(uint8_t), \"SvtHipTxSize", "sizeof(uint32_t), \"SvtHipTxSize"))
    assert r.returncode != 0 and "differs" in r.stderr
