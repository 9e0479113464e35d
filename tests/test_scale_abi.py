"""The boundary of csrc/scale.hip.  (1) Compile-time proof that the four forms with a reference prototype have it: each is assigned to its dispatch pointer of
common_dsp_rtcd.h / aom_dsp_rtcd.h -- tests/abi/abi_typecheck_scale.c under the flags of test_abi_typecheck.py; needs the reference's headers, so it runs in the build
container only, as its siblings do.  (2) Every new entry point is exported by the product library (loaded without touching a device) and present in PROTOTYPES.
(3) Size and every member offset of the three descriptor structures of include/svtav1_hip.h, as gcc lays them out, against the numpy definitions of the package: no
implicit padding on either side."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT, load_pkg

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
needs_reference = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "common_dsp_rtcd.h")), reason="the reference's headers are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals"),
       "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
STRICT = ["-std=gnu11", "-fsyntax-only", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers", "-Werror=int-conversion",
          "-Werror=implicit-function-declaration"]
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_scale.c")
FORMS = ("svt_av1_convolve_2d_scale_hip", "svt_av1_highbd_convolve_2d_scale_hip", "svt_av1_resize_plane_hip", "svt_av1_highbd_resize_plane_hip")
ENTRIES = FORMS + ("svt_hip_inter_pred_scaled_batch", "svt_hip_resize_workspace_bytes", "svt_hip_resize_plane_batch", "svt_hip_superres_upscale_batch",
                   "svt_hip_upscale_normative_rows_host")
STRUCTS = (("SvtHipScaledPredDesc", "ScaledPredDesc"), ("SvtHipResizeDesc", "ResizeDesc"), ("SvtHipUpscaleDesc", "UpscaleDesc"))


def _cc(src_text=None):
    cmd = ["gcc", *STRICT, *INC]
    if src_text is not None:
        return subprocess.run(cmd + ["-x", "c", "-"], input=src_text, capture_output=True, text=True)
    return subprocess.run(cmd + [FILE], capture_output=True, text=True)


def test_the_library_exports_the_scale_entries():
    lib = C.CDLL(os.path.join(PKG_DIR, "libsvtav1_hip.so"))  # resolves its ROCm dependencies; no HIP call is made
    pkg = load_pkg()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in pkg.PROTOTYPES, name


@needs_reference
def test_scale_forms_have_the_reference_prototypes():
    r = _cc()
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    base = open(FILE).read()
    assert base.count("_hip; n++;") == len(FORMS)
    # teeth: a form assigned to the pointer of another prototype is rejected
    for ptr, wrong in (("svt_av1_highbd_convolve_2d_scale", "svt_av1_convolve_2d_scale_hip"), ("svt_av1_convolve_2d_scale", "svt_av1_highbd_convolve_2d_scale_hip"),
                       ("svt_av1_highbd_resize_plane", "svt_av1_resize_plane_hip"), ("svt_av1_resize_plane", "svt_av1_highbd_resize_plane_hip"),
                       ("svt_av1_resize_plane", "svt_av1_convolve_2d_scale_hip")):
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)


def test_descriptor_layouts_match_the_header(tmp_path):
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
    assert pkg.ScaledPredDesc.itemsize == 64 and pkg.ResizeDesc.itemsize == 40 and pkg.UpscaleDesc.itemsize == 304
