"""Compile-time proof that the fifteen masked-prediction forms of csrc/maskpred.hip have the reference's prototypes: each is assigned to its dispatch pointer of
common_dsp_rtcd.h / aom_dsp_rtcd.h -- tests/abi/abi_typecheck_maskpred.c under the flags of test_abi_typecheck.py.  Needs the reference's headers, so it runs in the
build container only, as its siblings do."""
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
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_maskpred.c")


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def test_masked_prediction_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    assert base.count("_hip; n++;") == 15
    # teeth: a form assigned to a pointer of another prototype is rejected
    for ptr, wrong in (("svt_aom_highbd_blend_a64_mask", "svt_aom_blend_a64_mask_hip"),                  # the 8-bit form lacks the trailing bd
                       ("svt_aom_blend_a64_hmask", "svt_aom_highbd_blend_a64_hmask_16bit_hip"),           # uint16_t planes in a uint8_t pointer
                       ("svt_aom_blend_a64_mask", "svt_aom_blend_a64_vmask_hip"),                         # a 1-D mask form in the 2-D pointer
                       ("svt_av1_wedge_sse_from_residuals", "svt_av1_wedge_sign_from_residuals_hip"),     # another helper
                       ("svt_aom_lowbd_blend_a64_d16_mask", "svt_aom_highbd_blend_a64_d16_mask_hip"),      # a trailing bd
                       ("svt_av1_build_compound_diffwtd_mask_d16", "svt_av1_build_compound_diffwtd_mask_highbd_hip"),  # pixel planes where ConvBufType is expected
                       ("svt_av1_build_compound_diffwtd_mask", "svt_av1_build_compound_diffwtd_mask_highbd_hip")):
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)
