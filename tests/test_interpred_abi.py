"""Compile-time proof that the sixteen inter-prediction forms of csrc/interpred.hip have the reference's prototypes: each is assigned to its dispatch pointer of
common_dsp_rtcd.h, and SvtHipInterpFilterParams is laid out like InterpFilterParams -- tests/abi/abi_typecheck_interpred.c under the flags of test_abi_typecheck.py.
Needs the reference's headers, so it runs in the build container only, as its siblings do."""
import os
import re
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
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_interpred.c")


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def _struct_body(text, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
    assert m, name
    return " ".join(m.group(1).split())


def test_inter_prediction_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    assert base.count("_hip; n++;") == 16
    # the struct that is static-asserted there is, word for word, the one the header defines for builds without the reference's types
    header = open(os.path.join(ROOT, "include", "svtav1_hip.h")).read()
    assert _struct_body(base, "SvtHipInterpFilterParamsMirror") == _struct_body(header, "SvtHipInterpFilterParams")
    # teeth: a form assigned to a pointer of another prototype is rejected
    for ptr, wrong in (("svt_av1_highbd_convolve_2d_sr", "svt_av1_convolve_2d_sr_hip"),      # an 8-bit form in a highbd pointer (uint16_t planes, const params, a trailing bd)
                       ("svt_av1_jnt_convolve_x", "svt_av1_highbd_jnt_convolve_x_hip"),       # and the other way round
                       ("svt_av1_wiener_convolve_add_src", "svt_av1_convolve_x_sr_hip")):     # another family's pointer
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)
    # and the layout assertion has teeth: a mirror with a narrower enum field fails
    bad = base.replace("uint32_t       interp_filter;", "uint8_t        interp_filter;")
    r = _cc(bad)
    assert r.returncode != 0 and "differs" in r.stderr
