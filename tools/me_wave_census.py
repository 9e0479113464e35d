#!/usr/bin/env python3
"""VALU and LDS census of me_fullpel_wave_kernel (csrc/sad.hip) from the cross-compiler's assembly: no GPU needed.

  python tools/me_wave_census.py [--area 16x9] [--kernel me_fullpel_wave_kernelILb0ELi26E] [--keep x.s]

Compiles sad.hip for gfx950 with the flags of csrc/Makefile plus `-S --cuda-device-only`, cuts the kernel into basic blocks and sorts them, in layout order, into

  set-up + staging : everything before the first ring prologue (the block that issues the 14 ds_read2 of rows 0-6): descriptor, the lane's source block,
                     stage_window_wave.  Its loop (a branch back to an earlier label) is the four-chunks-in-flight loop, ceil(rows / (4 * (64 / NF))) trips;
                     the figure is the heaviest forward path through the region, an upper bound (the staging is instantiated per NF, one instance runs).
  start of a wave  : three figures of the latency a wave meets before and inside its search (start_figures below): the window loads a path of the set-up issues
                     before its first `s_waitcnt vmcnt`, the scalar waits (kernel arguments, descriptor) in front of the first vector load, and per step block the
                     qsads between the read of the new ring row and the first qsad that takes it.
  search instance  : one per instantiation of me_search_strips (FULL = W % 4 == 0, and the general one); an instance starts at a ring prologue.
                       prologue : per x group, the blocks without a v_qsad_pk_u16_u8 or a v_permlane32_swap
                       step     : a block with 16 (sub_sad: 8) qsad = one y step; its tail = VALU - qsad
                       group    : a block with v_permlane32_swap and the bank-masked adds of the reduce-scatter = the 32x32 / 64x64 levels of a group
                                  of two to four steps
                       pool add : a block with full-row v_add_u32_dpp row_ror and neither qsad nor swap = a last group of ONE step (H % 4 == 1): its 32x32
                                  sum goes into the pool of up to four x groups
                       pool     : a block with v_permlane32_swap, no reduce-scatter and the refill of the pool register (0x7ffff) = the 32x32 / 64x64 levels of
                                  a pool, once per four x groups
                     A build that pairs the two step groups of a ring block (steps 0-3 = A, 4-7 = B; it has a reduce-scatter block WITHOUT a swap) is modelled
                     per ring block of eight steps instead of per group:
                       scatter  : the reduce-scatter of group A alone, whose levels wait for group B (A of two steps or more)
                       group    : reduce-scatter of B + both 32x32 keys + the row / half swaps on both registers (B of two steps or more)
                       alone    : a block with the swaps and neither reduce-scatter nor pool refill = the levels of an A without such a B
                       leftover : the blocks behind the steps of a group that key the 16x16 sums not yet taken, one of four scalar-branch sides: two sums
                                  (a group of four or two steps; the dearer sides) or one (three steps, one step; the cheaper sides)
  final            : from the first v_min_u32_dpp on: minima over the lanes, the cross-lane read (ds_bpermute, counted apart: LDS pipe) and the two store
                     passes.  The stores of an empty search area (the loop at the very end) are laid out here too; no wave with an area runs them.

Static counts are exact.  "Executed" weights them with the trip counts of the area: G = ceil(W / 4) x groups, H steps and ceil(H / 4) groups each.  The unrolled
ring has eight step variants that differ by a few scalar-fed instructions, and which of them a given H runs is not derived here: the step and group terms use the
mean over the variants, and the [min, max] over the variants is printed as the bound.  Predicated blocks (skipped when no lane needs them) count as executed.
Groups per x group: H // 4 full ones, one more (with the sentinel) for H % 4 in {2, 3}; H % 4 == 1 is a pool add per x group and ceil(G / 4) pools per wave.
LDS instructions (every ds_* but ds_bpermute; atomics = ds_min / ds_add, counted apart) are reported per step and, with the same weights, per wave:
the quad sums of me_search_strips run on that pipe instead of the VALU, and four SIMDs share it.  The metadata line gives the static LDS bytes; the
launcher's dynamic bytes per workgroup and the workgroups per CU they allow (160 KB per CU) are printed for the area.
SQ_INSTS_VALU / SQ_WAVES and SQ_INSTS_LDS / SQ_WAVES of a counter pass on the GPU are the exact figures; this script is the desk check before that pass.
The model of a build that pairs step groups is approximate: its blocks are told apart by text patterns (the pool's refill constant 0x7ffff, a key's shift by 11), and
the sides of its scalar branches are smaller blocks whose copies and sentinel moves land in "prologue and loop control" or in a step's tail as the compiler pleases.
Against the counters it missed the change of the commit that introduced the pairing by about 20 instructions per wave (-42 predicted, -64 measured at 16x9:
profiles/me_wave_pairs_timing.txt).
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
    out, cur = [], {"label": "entry", "ops": [], "txt": [], "to": []}
    for l in lines[start + 1:end + 1]:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            out.append(cur)
            cur = {"label": m.group(1), "ops": [], "txt": [], "to": []}
            continue
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        cur["ops"].append(op)
        cur["txt"].append(t)
        if op.startswith("s_cbranch") or op == "s_branch":
            cur["to"].append(t.split()[1])
            out.append(cur)
            cur = {"label": cur["label"] + "+", "ops": [], "txt": [], "to": []}
    out.append(cur)
    out = [b for b in out if b["ops"]]
    for b in out:
        b["valu"] = sum(o.startswith("v_") for o in b["ops"])
        b["qsad"] = sum(o.startswith("v_qsad_pk_u16_u8") for o in b["ops"])
        b["dsr"] = sum(o.startswith("ds_read") for o in b["ops"])
        b["lds"] = sum(o.startswith("ds_") and not o.startswith("ds_bpermute") for o in b["ops"])
        b["atom"] = sum(o.startswith(("ds_min", "ds_max", "ds_add", "ds_sub", "ds_or", "ds_and")) for o in b["ops"])
        swap = any(o.startswith("v_permlane32_swap") for o in b["ops"])
        scatter = any(t.startswith("v_add_u32_dpp") and "bank_mask:0x3" in t for t in b["txt"])
        b["grp"] = swap and scatter
        refill = any(t.startswith("v_mov_b32") and t.endswith("0x7ffff") for t in b["txt"])
        b["pool"] = swap and not scatter and refill
        b["alone"] = swap and not scatter and not refill  # (only a build that pairs step groups has such a block)
        b["scat"] = scatter and not swap
        dpp = any("_dpp" in o for o in b["ops"])
        b["left"] = (not b["qsad"] and not swap and not dpp and any(o.startswith(("v_min_u32", "v_min3_u32")) for o in b["ops"])
                     and any(re.match(r"v_lshl_or_b32 \S+ \S+ 11,", t) for t in b["txt"]))
        b["padd"] = not swap and not b["qsad"] and any(t.startswith("v_add_u32_dpp") and "row_ror" in t and "bank_mask:0xf" in t for t in b["txt"])
        b["fin"] = any(o.startswith("v_min_u32_dpp") for o in b["ops"])
        b["bperm"] = sum(o.startswith("ds_bpermute") for o in b["ops"])
    return out


def start_figures(bl, idx, n_pre):
    """The start of a wave, from the set-up blocks bl[:n_pre] (forward paths only) and the step blocks:
      window loads before the first vmcnt wait : 16-byte (or 12 + 4) vector loads a path issues before its first `s_waitcnt vmcnt`, [min, max] over the paths
      scalar waits before the first vector load: `s_waitcnt lgkmcnt` with a scalar load outstanding, on the path from the entry to the first global load (max over paths)
      qsads between ring-row read and first use: per step block, the qsads issued between the last ds_read2_b32 pair of the ring row and the first qsad that takes its
                                                 register; where the step that reads the row does not use it (sub_sad), the qsads left in the block, marked '+'."""
    def succ(i):
        b = bl[i]
        nxt = [idx[t] for t in b["to"] if t in idx and idx[t] > i]
        if b["ops"][-1] != "s_branch":
            nxt.append(i + 1)
        return [j for j in nxt if j < n_pre]

    loads, waits = [], []

    def walk(i, nload, pend, nwait, seen_vec, done_l):
        for t in bl[i]["txt"]:
            op = t.split()[0]
            if op.startswith("s_load"):
                pend = True
            elif op == "s_waitcnt":
                if "lgkmcnt" in t and pend and not seen_vec:
                    nwait, pend = nwait + 1, False
                if "vmcnt" in t and not done_l:
                    loads.append(nload)
                    done_l = True
            elif op.startswith(("global_load", "flat_load")):
                if not seen_vec:
                    waits.append(nwait)
                    seen_vec = True
                if op.endswith(("dwordx4", "dwordx3")) and not done_l:
                    nload += 1
        if done_l and seen_vec:
            return
        nx = succ(i)
        if not nx and not done_l and nload:
            loads.append(nload)
        for j in nx:
            walk(j, nload, pend, nwait, seen_vec, done_l)
    walk(0, 0, False, 0, False, False)
    loads = [n for n in loads if n]  # (a path that waits without a window load behind it is the exit of an empty area or of a wave past n)
    dist = []
    for b in bl:
        if not b["qsad"] or b["qsad"] < 8:
            continue
        reads = [(k, re.match(r"ds_read2_b32 (v\[\d+:\d+\])", t).group(1)) for k, t in enumerate(b["txt"]) if t.startswith("ds_read2_b32")]
        if not reads:
            dist.append("none in the block")
            continue
        k0, reg = reads[0]
        after = [t for t in b["txt"][k0:] if t.startswith("v_qsad_pk_u16_u8")]
        use = next((n for n, t in enumerate(after) if re.match(r"v_qsad_pk_u16_u8 \S+ %s," % re.escape(reg), t)), None)
        dist.append(str(use) if use is not None else "%d+" % len(after))
    return loads, waits, dist


def metadata(lines, name):
    text = "\n".join(lines)
    sym = re.search(r"\.name:\s+(_Z\w*%s\w*)" % re.escape(name), text).group(1)
    i = text.index("- .agpr_count", 0)
    doc = [d for d in text[i:].split("  - .agpr_count") if ".name:           " + sym + "\n" in d][0]
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, doc).group(1))  # noqa: E731
    return {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size"), "spill_vgpr": g("vgpr_spill_count"),
            "lds_static": g("group_segment_fixed_size"), "slice_dw": slice_dw()}


def slice_dw():
    """Dwords a wave owns in LDS behind its window (the launcher sizes the dynamic LDS as 4 x (window + this)): the constant the source states."""
    m = re.search(r"constexpr int ME_WAVE_QSUM_DW = (\d+);", open(os.path.join(CSRC, "sad.hip")).read())
    return int(m.group(1)) if m else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--area", default="16x9")
    ap.add_argument("--kernel", default="me_fullpel_wave_kernelILb0ELi26E")
    ap.add_argument("--keep", default=None, help="write the assembly here")
    ap.add_argument("--asm", default=None, help="census of an existing assembly file instead of compiling")
    ap.add_argument("--slice-dw", type=int, default=None, help="dwords a wave owns behind its window (default: ME_WAVE_QSUM_DW of the source; 0 for a commit without it)")
    a = ap.parse_args()
    W, H = (int(v) for v in a.area.split("x"))
    path = a.asm or a.keep or os.path.join(tempfile.mkdtemp(), "sad.s")
    if not a.asm:
        compile_asm(path)
    lines = open(path).read().split("\n")
    bl = blocks_of(lines, a.kernel)
    md = metadata(lines, a.kernel)
    if a.slice_dw is not None:
        md["slice_dw"] = a.slice_dw
    idx = {b["label"]: i for i, b in enumerate(bl)}
    starts = [i for i, b in enumerate(bl) if b["dsr"] >= 14 and not b["qsad"]]  # ring prologues
    fins = [i for i, b in enumerate(bl) if b["fin"]]
    last_search = (fins[0] - 1) if fins else max(i for i, b in enumerate(bl) if b["qsad"] or b["grp"])
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

    wl, sw, dist = start_figures(bl, idx, len(pre))
    print("start of a wave  : window loads issued before the first vmcnt wait %s over the paths of the set-up; scalar waits before the first vector load %s; "
          "qsads between a step's ring-row read and its first use %s" %
          ("[%d, %d]" % (min(wl), max(wl)) if wl else "none", max(sw) if sw else "none", sorted(set(dist))))

    G, groups = (W + 3) // 4, (H + 3) // 4
    pooled = any(b["padd"] for b in bl)
    if pooled and H % 4 == 1:
        groups -= 1
    n_padd, n_pool = (1, -(-G // 4)) if pooled and H % 4 == 1 else (0, 0)
    total, lds_total = {}, {}
    pairing = any(b["scat"] for b in bl)  # the two step groups of a ring block share their 32x32 / 64x64 levels
    for k, s0 in enumerate(starts):
        s1 = starts[k + 1] if k + 1 < len(starts) else last_search + 1
        inst = bl[s0:s1]
        steps = [b for b in inst if b["qsad"]]
        grp = [b for b in inst if b["grp"] and not b["qsad"]]
        padd = [b["valu"] for b in inst if b["padd"]] or [0]
        pool = [b["valu"] for b in inst if b["pool"]] or [0]
        other = [b for b in inst if not b["qsad"] and not b["grp"] and not b["padd"] and not b["pool"] and not (pairing and (b["scat"] or b["alone"] or b["left"]))]
        tails = [b["valu"] - b["qsad"] for b in steps]
        gt = [b["valu"] for b in grp] or [0]  # (no group blocks: the levels are part of every step)
        q = steps[0]["qsad"]
        mean = lambda v: sum(v) / len(v)  # noqa: E731
        pro = sum(b["valu"] for b in other)
        # the same weights for the LDS pipe (means over the step / group variants)
        lds_step, atom_step = mean([b["lds"] for b in steps]), mean([b["atom"] for b in steps])
        lds_ex = G * (sum(b["lds"] for b in other) + H * lds_step + groups * mean([b["lds"] for b in grp] or [0])
                      + n_padd * mean([b["lds"] for b in inst if b["padd"]] or [0])) + n_pool * mean([b["lds"] for b in inst if b["pool"]] or [0])
        lds_total[k] = (lds_step, atom_step, lds_ex, G * H * atom_step)
        ex = [G * (pro + H * (q + f(tails)) + groups * f(gt) + n_padd * f(padd)) + n_pool * f(pool) for f in (min, mean, max)]
        if pairing:  # per ring block: what its groups A and B of nA and nB steps run (a group of one step goes to the pool)
            scat, alone = [b["valu"] for b in inst if b["scat"]] or [0], [b["valu"] for b in inst if b["alone"]] or [0]
            left = [b["valu"] for b in inst if b["left"] and b["valu"]] or [0]
            lv = [0, 0, 0]
            for yb in range(0, H, 8):
                nA, nB = min(4, H - yb), max(0, min(4, H - yb - 4))
                for m, f in enumerate((min, mean, max)):
                    lv[m] += sum((max(left) if n in (2, 4) else min(left)) for n in (nA, nB) if n)
                    if nA >= 2:
                        lv[m] += f(scat) + (f(gt) if nB >= 2 else f(alone))
            ex = [G * (pro + H * (q + f(tails)) + lv[m] + n_padd * f(padd)) + n_pool * f(pool) for m, f in enumerate((min, mean, max))]
            print("search instance %d : paired step groups: scatter of A %s, levels of A + B %s, of A alone %s, leftover 16x16 keys of a group %s (dearer: two sums)" %
                  (k, sorted(scat), sorted(gt), sorted(alone), sorted(left)))
            nleft = len([b for b in inst if b["left"] and b["valu"]])
            if nleft < 4:  # (the source keeps the four sides apart with empty asm statements; as selects they would all run in every group)
                print("                    WARNING: %d leftover blocks, 4 or more expected: the compiler has turned scalar-branch sides into selects" % nleft)
        total[k] = (sum(tails), ex)
        print("search instance %d : %d step blocks, tail VALU per step %s (mean %.1f) + %d qsad; %d group blocks, VALU per group of four steps %s (mean %.1f); "
              "prologue and loop control %d per x group" % (k, len(steps), sorted(tails), mean(tails), q, len(grp), sorted(gt), mean(gt), pro))
        if pooled:
            print("                    pool add (a last group of one step) %s per x group, pool %s per four x groups" % (sorted(padd), sorted(pool)))
        if pairing:
            print("                    executed at %dx%d: %d x groups x (%d + %d steps x (%d + tail) + %.0f for the levels and leftovers of %d ring blocks + %d x pool add) "
                  "+ %d x pool = %.0f  [%d, %d]" % (W, H, G, pro, H, q, lv[1], -(-H // 8), n_padd, n_pool, ex[1], ex[0], ex[2]))
        else:
            print("                    executed at %dx%d: %d x groups x (%d + %d steps x (%d + tail) + %d groups x group + %d x pool add) + %d x pool = %.0f  [%d, %d]" %
                  (W, H, G, pro, H, q, groups, n_padd, n_pool, ex[1], ex[0], ex[2]))
    final = bl[last_search + 1:]
    back = [idx[t] - (last_search + 1) for i, b in enumerate(final) for t in b["to"] if t in idx and last_search + 1 <= idx[t] <= last_search + 1 + i]
    empty = final[max(min(back) - 1, 0):] if back else []  # the store loop of an empty area and its preheader
    fin = sum(b["valu"] for b in final) - sum(b["valu"] for b in empty)
    print("final minima + emit : %d, ds_bpermute %d (and %d in the stores of an empty area, which no wave with an area runs)" %
          (fin, sum(b["bperm"] for b in final), sum(b["valu"] for b in empty)))
    full = min(total, key=lambda k: total[k][0])  # the instantiation without the invalid-position ORs
    which = full if W % 4 == 0 else max(total, key=lambda k: total[k][0])
    ex = total[which][1]
    print("executed VALU per wave at %dx%d (instance %d): %.0f  [%.0f, %.0f]; qsad %d" %
          (W, H, which, st_exec + ex[1] + fin, st_exec + ex[0] + fin, st_exec + ex[2] + fin, G * H * [b for b in bl if b["qsad"]][0]["qsad"]))
    ls, at, lex, aex = lds_total[which]
    print("LDS instructions (instance %d): %.1f per step, of them %.1f atomics; search per wave at %dx%d: %.0f, of them %.0f atomics "
          "(+ staging: %d static in set-up, 2 stores per 16-byte chunk)" % (which, ls, at, W, H, lex, aex, sum(b["lds"] for b in pre)))
    pitch = 18 if 16 + G <= 18 else 26
    shm = 4 * 4 * pitch * (64 + H - 1) + 4 * 4 * md["slice_dw"]
    print("LDS bytes per workgroup at %dx%d: 4 x (%d window + %d slice) = %d -> %d workgroups per CU (160 KB; static %d bytes)" %
          (W, H, 4 * pitch * (64 + H - 1), 4 * md["slice_dw"], shm, min(163840 // shm, 8), md["lds_static"]))


if __name__ == "__main__":
    sys.exit(main())
