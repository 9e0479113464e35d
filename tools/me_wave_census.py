#!/usr/bin/env python3
"""VALU census of me_fullpel_wave_kernel (csrc/sad.hip) from the cross-compiler's assembly: no GPU needed.

  python tools/me_wave_census.py [--area 16x9] [--kernel me_fullpel_wave_kernelILb0ELi26E] [--keep x.s]

Compiles sad.hip for gfx950 with the flags of csrc/Makefile plus `-S --cuda-device-only`, cuts the kernel into basic blocks and sorts them, in layout order, into

  set-up + staging : everything before the first ring prologue (the block that issues the 14 ds_read2 of rows 0-6): descriptor, the lane's source block,
                     stage_window_wave.  Its loop (a branch back to an earlier label) is the four-chunks-in-flight loop, ceil(rows / (4 * (64 / NF))) trips;
                     the figure is the heaviest forward path through the region, an upper bound (the staging is instantiated per NF, one instance runs).
  search instance  : one per instantiation of me_search_strips (FULL = W % 4 == 0, and the general one); an instance starts at a ring prologue.
                       prologue : per x group, the blocks without a v_qsad_pk_u16_u8 or a v_permlane32_swap
                       step     : a block with 16 (sub_sad: 8) qsad = one y step; its tail = VALU - qsad
                       group    : a block with v_permlane32_swap = the 32x32 / 64x64 levels of a group of four steps
  final            : after the last search block: DPP minima over the lanes and the stores.

Static counts are exact.  "Executed" weights them with the trip counts of the area: G = ceil(W / 4) x groups, H steps and ceil(H / 4) groups each.  The unrolled
ring has eight step variants that differ by a few scalar-fed instructions, and which of them a given H runs is not derived here: the step and group terms use the
mean over the variants, and the [min, max] over the variants is printed as the bound.  Predicated blocks (skipped when no lane needs them) count as executed.
SQ_INSTS_VALU / SQ_WAVES of a counter pass on the GPU is the exact figure; this script is the desk check before that pass.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svt-av1-psy_amd", "csrc")


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    return os.environ.get("HIPCC", hipcc), flags


def compile_asm(out):
    hipcc, flags = makefile_flags()
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", "-Wno-unused-command-line-argument", "sad.hip", "-o", out], cwd=CSRC, check=True)


def blocks_of(lines, name):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(name), l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    out, cur = [], {"label": "entry", "ops": [], "to": []}
    for l in lines[start + 1:end + 1]:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            out.append(cur)
            cur = {"label": m.group(1), "ops": [], "to": []}
            continue
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        cur["ops"].append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            cur["to"].append(t.split()[1])
            out.append(cur)
            cur = {"label": cur["label"] + "+", "ops": [], "to": []}
    out.append(cur)
    out = [b for b in out if b["ops"]]
    for b in out:
        b["valu"] = sum(o.startswith("v_") for o in b["ops"])
        b["qsad"] = sum(o.startswith("v_qsad_pk_u16_u8") for o in b["ops"])
        b["dsr"] = sum(o.startswith("ds_read") for o in b["ops"])
        b["grp"] = any(o.startswith("v_permlane32_swap") for o in b["ops"])
    return out


def metadata(lines, name):
    text = "\n".join(lines)
    sym = re.search(r"\.name:\s+(_Z\w*%s\w*)" % re.escape(name), text).group(1)
    i = text.index("- .agpr_count", 0)
    doc = [d for d in text[i:].split("  - .agpr_count") if ".name:           " + sym + "\n" in d][0]
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, doc).group(1))  # noqa: E731
    return {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size"), "spill_vgpr": g("vgpr_spill_count")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--area", default="16x9")
    ap.add_argument("--kernel", default="me_fullpel_wave_kernelILb0ELi26E")
    ap.add_argument("--keep", default=None, help="write the assembly here")
    ap.add_argument("--asm", default=None, help="census of an existing assembly file instead of compiling")
    a = ap.parse_args()
    W, H = (int(v) for v in a.area.split("x"))
    path = a.asm or a.keep or os.path.join(tempfile.mkdtemp(), "sad.s")
    if not a.asm:
        compile_asm(path)
    lines = open(path).read().split("\n")
    bl = blocks_of(lines, a.kernel)
    md = metadata(lines, a.kernel)
    idx = {b["label"]: i for i, b in enumerate(bl)}
    starts = [i for i, b in enumerate(bl) if b["dsr"] >= 14 and not b["qsad"]]  # ring prologues
    last_search = max(i for i, b in enumerate(bl) if b["qsad"] or b["grp"])
    print("kernel %s: VGPR %d, SGPR %d, scratch %d bytes, spilled VGPRs %d" % (a.kernel, md["vgpr"], md["sgpr"], md["scratch"], md["spill_vgpr"]))
    print("static: VALU %d, of them qsad %d, in %d basic blocks" % (sum(b["valu"] for b in bl), sum(b["qsad"] for b in bl), len(bl)))

    # set-up + staging
    pre = bl[:starts[0]]
    NF = (64 + W - 1) >> 4
    trips = -(-(64 + H - 1) // (4 * (64 // NF)))
    weight = [1] * len(pre)
    for i, b in enumerate(pre):
        for t in b["to"]:
            if t in idx and idx[t] <= i:  # back edge: the chunk loop
                for j in range(idx[t], i + 1):
                    weight[j] = trips
    # the heaviest forward path through the region (the dispatch on NF instantiates the staging twice, only one runs): an upper bound on what a wave executes
    best = [0] * (len(pre) + 1)
    for i in range(len(pre) - 1, -1, -1):
        b = pre[i]
        nxt = [idx[t] for t in b["to"] if t in idx and idx[t] > i]
        if b["ops"][-1] != "s_branch":
            nxt.append(i + 1)
        best[i] = b["valu"] * weight[i] + max([best[j] for j in nxt if j < len(pre)] + [0])
    st_static, st_exec = sum(b["valu"] for b in pre), best[0]
    chunks = (64 + H - 1) * ((64 + W - 1 + 15) >> 4)
    print("set-up + staging : static %4d, executed at %dx%d <= %4d (chunk loop x %d; %d chunks of 16 bytes, source block and descriptor included)" %
          (st_static, W, H, st_exec, trips, chunks))

    G, groups = (W + 3) // 4, (H + 3) // 4
    total = {}
    for k, s0 in enumerate(starts):
        s1 = starts[k + 1] if k + 1 < len(starts) else last_search + 1
        inst = bl[s0:s1]
        steps = [b for b in inst if b["qsad"]]
        grp = [b for b in inst if b["grp"] and not b["qsad"]]
        other = [b for b in inst if not b["qsad"] and not b["grp"]]
        tails = [b["valu"] - b["qsad"] for b in steps]
        gt = [b["valu"] for b in grp] or [0]  # (no group blocks: the levels are part of every step)
        q = steps[0]["qsad"]
        mean = lambda v: sum(v) / len(v)  # noqa: E731
        pro = sum(b["valu"] for b in other)
        ex = [G * (pro + H * (q + f(tails)) + groups * f(gt)) for f in (min, mean, max)]
        total[k] = (sum(tails), ex)
        print("search instance %d : %d step blocks, tail VALU per step %s (mean %.1f) + %d qsad; %d group blocks, VALU per group of four steps %s (mean %.1f); "
              "prologue and loop control %d per x group" % (k, len(steps), sorted(tails), mean(tails), q, len(grp), sorted(gt), mean(gt), pro))
        print("                    executed at %dx%d: %d x groups x (%d + %d steps x (%d + tail) + %d groups x group) = %.0f  [%d, %d]" %
              (W, H, G, pro, H, q, groups, ex[1], ex[0], ex[2]))
    fin = sum(b["valu"] for b in bl[last_search + 1:])
    print("final minima + emit : %d" % fin)
    full = min(total, key=lambda k: total[k][0])  # the instantiation without the invalid-position ORs
    which = full if W % 4 == 0 else max(total, key=lambda k: total[k][0])
    ex = total[which][1]
    print("executed VALU per wave at %dx%d (instance %d): %.0f  [%.0f, %.0f]; qsad %d" %
          (W, H, which, st_exec + ex[1] + fin, st_exec + ex[0] + fin, st_exec + ex[2] + fin, G * H * [b for b in bl if b["qsad"]][0]["qsad"]))


if __name__ == "__main__":
    sys.exit(main())
