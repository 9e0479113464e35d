"""The boundary of csrc/palette.hip.  (1) Compile-time proof that the six single-call forms have the reference's prototypes: the four k-means forms are assigned to their
dispatch pointers of aom_dsp_rtcd.h, the two colour counters to pointers of the type the reference's palette.c declares them with -- tests/abi/abi_typecheck_palette.c
under the flags of test_abi_typecheck.py; needs the reference's headers, so it runs in the build container only, as its siblings do.  (2) Every new entry point is
exported by the product library (loaded without touching a device) and present in PROTOTYPES.  (3) Size and every member offset of the six structures of
include/svtav1_hip.h, as gcc lays them out, against the numpy definitions of the package: no implicit padding on either side."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import PKG_DIR, ROOT, load_pkg

REF = os.environ.get("SVT_REF", "/root/reference")
SRC = os.path.join(REF, "Source")
needs_reference = pytest.mark.skipif(not os.path.isfile(os.path.join(SRC, "Lib", "Codec", "palette.c")), reason="the reference's headers are not on this machine")

INC = ["-I" + os.path.join(SRC, "API"), "-I" + os.path.join(SRC, "Lib", "Codec"), "-I" + os.path.join(SRC, "Lib", "C_DEFAULT"), "-I" + os.path.join(SRC, "Lib", "Globals"),
       "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
STRICT = ["-std=gnu11", "-fsyntax-only", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=discarded-qualifiers", "-Werror=int-conversion",
          "-Werror=implicit-function-declaration"]
FILE = os.path.join(ROOT, "tests", "abi", "abi_typecheck_palette.c")
FORMS = ("svt_av1_k_means_dim1_hip", "svt_av1_k_means_dim2_hip", "svt_av1_calc_indices_dim1_hip", "svt_av1_calc_indices_dim2_hip", "svt_av1_count_colors_hip",
         "svt_av1_count_colors_highbd_hip")
ENTRIES = FORMS + ("svt_hip_kmeans_batch", "svt_hip_count_colors_batch", "svt_hip_palette_search_luma_batch", "svt_hip_palette_cost_batch", "svt_hip_palette_pred_batch",
                   "svt_hip_palette_cache_y")
STRUCTS = (("SvtHipKmeansDesc", "KmeansDesc"), ("SvtHipCountColorsDesc", "CountColorsDesc"), ("SvtHipPaletteSearchDesc", "PaletteSearchDesc"),
           ("SvtHipPaletteSearchOut", "PaletteSearchOut"), ("SvtHipPaletteCostDesc", "PaletteCostDesc"), ("SvtHipPalettePredDesc", "PalettePredDesc"))


def count_decls():
    """the declarations of the two colour counters as the reference's palette.c has them"""
    text = open(os.path.join(SRC, "Lib", "Codec", "palette.c")).read()
    decls = re.findall(r"^int svt_av1_count_colors(?:_highbd)?\([^)]*\);", text, flags=re.M)
    assert len(decls) == 2, decls
    return " ".join(decls)


def _cc(src_text):
    return subprocess.run(["gcc", *STRICT, *INC, "-x", "c", "-"], input=src_text, capture_output=True, text=True)


def test_the_library_exports_the_palette_entries():
    lib = C.CDLL(os.path.join(PKG_DIR, "libsvtav1_hip.so"))  # resolves its ROCm dependencies; no HIP call is made
    pkg = load_pkg()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in pkg.PROTOTYPES, name


@needs_reference
def test_palette_forms_have_the_reference_prototypes():
    base = open(FILE).read().replace("SVT_PALETTE_COUNT_DECLS", count_decls())
    r = _cc(base)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-6000:]
    assert base.count("_hip; n++;") == len(FORMS)
    # teeth: a form assigned to the pointer of another prototype is rejected
    for ptr, wrong in (("svt_av1_k_means_dim1", "svt_av1_calc_indices_dim1_hip"), ("svt_av1_calc_indices_dim2", "svt_av1_k_means_dim2_hip"),
                       ("svt_av1_k_means_dim2", "svt_av1_count_colors_hip"), ("count_colors", "svt_av1_count_colors_highbd_hip"),
                       ("count_colors_highbd", "svt_av1_count_colors_hip")):
        bad = base.replace("    return n;", "    %s = %s;\n    return n;" % (ptr, wrong))
        r = _cc(bad)
        assert r.returncode != 0 and "incompatible-pointer-types" in r.stderr, (ptr, wrong)


def test_descriptor_layouts_match_the_header(tmp_path):
    pkg = load_pkg()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "svtav1_hip.h"', "int main(void) {"]
    for cname, pname in STRUCTS:
        dt = getattr(pkg, pname)
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
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
        assert got[(cname, "sizeof")] == dt.itemsize, cname
        covered = 0
        for f in dt.names:
            assert got[(cname, f)] == dt.fields[f][1], (cname, f)
            covered += dt.fields[f][0].itemsize
        assert covered == dt.itemsize, cname  # the members fill the structure: no implicit padding
    assert [getattr(pkg, p).itemsize for _, p in STRUCTS] == [40, 24, 64, 240, 56, 40]
