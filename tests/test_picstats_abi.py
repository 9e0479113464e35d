"""Compile-time proof that the four single-call forms of csrc/picstats.hip have the reference's prototypes: each is assigned to the dispatch pointer of
aom_dsp_rtcd.h it stands for -- tests/abi/abi_typecheck_picstats.c under the flags of test_abi_typecheck.py.  Needs the reference's headers, so it runs in the build
container only, as its siblings do."""
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "aom_dsp_rtcd.h")), reason="the reference's headers are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals"),
       "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
STRICT = ["-std=gnu11", "-fsyntax-only", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers", "-Werror=int-conversion",
          "-Werror=implicit-function-declaration"]
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_picstats.c")


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def test_picstats_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    assert base.count(" = svt_") == 4
    # teeth: a form installed into a pointer of another prototype is rejected
    for ptr, wrong in (("svt_compute_mean_8x8", "svt_compute_sub_mean_8x8_hip"),                 # two parameters fewer, uint16_t stride
                       ("svt_compute_sub_mean_8x8", "svt_compute_interm_var_four8x8_hip")):      # two parameters more, no return value
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)
