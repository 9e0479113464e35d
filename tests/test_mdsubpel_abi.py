"""The boundary of csrc/mdsubpel.hip.  (1) Compile-time proof that the 112 single-call forms have the reference's prototypes: each is assigned to its dispatch pointer
of aom_dsp_rtcd.h -- tests/abi/abi_typecheck_mdsubpel.c under the flags of test_abi_typecheck.py; needs the reference's headers, so it runs in the build container
only, as its siblings do.  (2) The entry points are exported by the product library (loaded without touching a device).  (3) Size and every member offset of the
five structures of include/svtav1_hip.h, as gcc lays them out, against the numpy definitions of the package: no implicit padding on either side."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT, load_pkg

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
needs_reference = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "aom_dsp_rtcd.h")), reason="the reference's headers are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals"),
       "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
STRICT = ["-std=gnu11", "-fsyntax-only", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers", "-Werror=int-conversion",
          "-Werror=implicit-function-declaration"]
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_mdsubpel.c")
FAMILIES = ("svt_aom_variance", "svt_aom_sub_pixel_variance", "svt_aom_obmc_sad", "svt_aom_obmc_variance", "svt_aom_obmc_sub_pixel_variance")
STRUCTS = (("SvtHipBlockVarDesc", "BlockVarDesc"), ("SvtHipBlockVarResult", "BlockVarResult"), ("SvtHipMvCostTable", "MvCostTable"), ("SvtHipMdSubpelDesc", "MdSubpelDesc"),
           ("SvtHipMdSubpelResult", "MdSubpelResult"))


def entries(pkg):
    names = ["svt_hip_block_var_batch", "svt_hip_md_subpel_search_batch", "svt_hip_md_subpel_mv_limits", "svt_aom_mse16x16_hip", "svt_aom_upsampled_pred_hip"]
    return names + ["%s%dx%d_hip" % (f, w, h) for f in FAMILIES for (w, h) in pkg.VARIANCE_SIZES]


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def test_the_library_exports_the_entries():
    lib = C.CDLL(os.path.join(PKG_DIR, "libsvtav1_hip.so"))  # resolves its ROCm dependencies; no HIP call is made
    pkg = load_pkg()
    names = entries(pkg)
    assert len(names) == 5 + 5 * 22 and len(set(pkg.VARIANCE_SIZES)) == 22
    for name in names:
        assert hasattr(lib, name), name
        assert name in pkg.PROTOTYPES, name


@needs_reference
def test_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    expanded = subprocess.run(["gcc", "-E", "-P", *INC, FILE], capture_output=True, text=True, check=True).stdout
    assert expanded.count("_hip; n++;") == 5 * 22 + 2
    # teeth: a form assigned to the pointer of another prototype is rejected
    for ptr, wrong in (("svt_aom_variance16x16", "svt_aom_sub_pixel_variance16x16_hip"), ("svt_aom_sub_pixel_variance8x8", "svt_aom_obmc_sub_pixel_variance8x8_hip"),
                       ("svt_aom_obmc_sad4x4", "svt_aom_obmc_variance4x4_hip"), ("svt_aom_obmc_variance64x64", "svt_aom_variance64x64_hip"),
                       ("svt_aom_upsampled_pred", "svt_aom_mse16x16_hip"), ("svt_aom_mse16x16", "svt_aom_obmc_sad16x16_hip")):
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)


def test_structure_layouts_match_the_header(tmp_path):
    pkg = load_pkg()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "svtav1_hip.h"', "int main(void) {"]
    for cname, pname in STRUCTS:
        dt = getattr(pkg, pname)
        lines.append('    printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out if ln}
    for cname, pname in STRUCTS:
        dt = getattr(pkg, pname)
        assert got[(cname, "size")] == dt.itemsize, cname
        covered = 0
        for f in dt.names:
            assert got[(cname, f)] == dt.fields[f][1], (cname, f)
            covered += dt.fields[f][0].itemsize
        assert covered == dt.itemsize, cname  # the members fill the structure: no implicit padding
    assert pkg.MV_VALS == 32767 and pkg.MvCostTable.fields["comp"][0].shape == (2, pkg.MV_VALS)
