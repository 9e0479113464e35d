"""The boundary of the OBMC motion refinement (csrc/mdsubpel.hip).  (1) The entry points are exported by the product library (loaded without touching a device) and
have a ctypes prototype in the package.  (2) Size and every member offset of the three structures of include/svtav1_hip.h, as gcc lays them out in a compiled probe,
against the numpy definitions of the package: no implicit padding on either side.  (3) The constants."""
import ctypes as C
import os
import subprocess

from conftest import PKG_DIR, ROOT, load_pkg

ENTRIES = ("svt_hip_obmc_wsrc_batch", "svt_hip_obmc_search_batch", "svt_hip_obmc_mv_limits", "svt_hip_obmc_refine_host")
STRUCTS = (("SvtHipObmcWsrcDesc", "ObmcWsrcDesc"), ("SvtHipObmcSearchDesc", "ObmcSearchDesc"), ("SvtHipObmcSearchResult", "ObmcSearchResult"))
CONSTANTS = (("SVT_HIP_OBMC_MAX_SPANS", "OBMC_MAX_SPANS"), ("SVT_HIP_OBMC_TARGET_ARRAYS", "OBMC_TARGET_ARRAYS"), ("SVT_HIP_OBMC_TARGET_DERIVED", "OBMC_TARGET_DERIVED"))


def test_the_library_exports_the_entries():
    lib = C.CDLL(os.path.join(PKG_DIR, "libsvtav1_hip.so"))  # resolves its ROCm dependencies; no HIP call is made
    pkg = load_pkg()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in pkg.PROTOTYPES, name
    assert len(pkg.PROTOTYPES["svt_hip_obmc_wsrc_batch"][1]) == 8 and len(pkg.PROTOTYPES["svt_hip_obmc_search_batch"][1]) == 11
    assert len(pkg.PROTOTYPES["svt_hip_obmc_mv_limits"][1]) == 6 and len(pkg.PROTOTYPES["svt_hip_obmc_refine_host"][1]) == 14


def test_structure_layouts_match_the_header(tmp_path):
    pkg = load_pkg()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "svtav1_hip.h"', "int main(void) {"]
    for cname, pname in STRUCTS:
        dt = getattr(pkg, pname)
        lines.append('    printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in dt.names:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    for cname, _ in CONSTANTS:
        lines.append('    printf("const %s %%d\\n", (int)%s);' % (cname, cname))
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
    for cname, pname in CONSTANTS:
        assert got[("const", cname)] == getattr(pkg, pname), cname
    assert (pkg.ObmcWsrcDesc.itemsize, pkg.ObmcSearchDesc.itemsize, pkg.ObmcSearchResult.itemsize) == (72, 136, 36)
    # the two descriptors name the target's inputs alike, so that one helper fills both
    shared = ("src_off", "above_off", "left_off", "src_stride", "above_stride", "left_stride", "above_plane", "left_plane", "bsize", "up_available", "left_available",
              "n_above", "n_left", "above_rel", "above_len", "left_rel", "left_len")
    assert all(f in pkg.ObmcWsrcDesc.names and f in pkg.ObmcSearchDesc.names for f in shared)
