"""Static instruction counts of k_pipeline's partition search, per source
region (no GPU needed).

  python tools/isa_regions.py [--asm file.s] [--kernel substring] [--fam3] [--root other-checkout]

Builds the gfx950 assembly of hl_encoder.hip (--fam3: hl_encoder_fam3.hip)
with the product's flags plus -gline-tables-only, or reads one built before,
and attributes every instruction of the kernel to the region of hl_mbcore.h
its .loc line lies in.  A region runs from its anchor (a regular expression
matched against the source lines, in file order) to the next anchor.  Lines
of other headers (the DPP and quad primitives are inlined) count for the
region of the last hl_mbcore.h line before them, so the scheduler's
interleaving blurs region borders by a few instructions; copies of a region
(the search is instantiated once per call site and unrolled loops repeat
their body) are summed: the figures are static sizes, not executed counts.
Development tool.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "-Wno-unused-function", "-Wno-unused-variable",
         "-mllvm", "-amdgpu-sched-strategy=iterative-ilp", "-gline-tables-only", "--cuda-device-only", "-S"]

# (anchor, region) in the order of hl_mbcore.h; None = not part of the search
ANCHORS = [
    (r"^// A candidate's result of an evaluation pass", "record"),  # CandRec's pack and unpack, inlined into every user
    (r"^// partitions whose passes chain speculative steps", None),
    (r"^// log2 of a power of two", "search prologue"),          # lg2, part_x .. sub_y
    (r"^HD void sub_part_idx\(", None),
    (r"^struct MvN \{", "mvp"),                                   # mv_at, nb_motion, median3, mvp
    (r"^// 8\.4\.1\.1 P_Skip motion vector", None),
    (r"^// Per-search constants", "search prologue"),             # the table of (j, pi, spi)
    (r"^// marks the 4x4 blocks of the luma rectangle", None),
    (r"^struct PartGeo \{", "search prologue"),                   # part_geo
    (r"^HD void put_cand\(", "put_cand"),
    (r"^HD double mv_cost\(", "cost phase"),
    (r"^HD void eval_candidates\(", "probe/emit"),
    (r"^\s+HL_PROF_T\(ta0\);", "miss path"),
    (r"^\s+\}  // \(a wave with a miss\)", "probe/emit"),         # the pass barrier, the pending marks
    (r"^\s+// phase 2: one row per candidate", "cost phase"),
    (r"^HD void commit_candidates\(", "commit"),
    (r"^HD int pick_first_min\(", None),
    (r"^// The selection's view of a pass", "minima"),            # sel_load, sel_minima
    (r"^// The winner in lane bi becomes the search's best", "resolution"),  # sel_take
    (r"^// Pipelined runs \(hl_pipeline\.h\): the task of a picture", "search prologue"),  # reach_task, reach_wait
    (r"^HD bool search_partition\(", "search prologue"),
    (r"^    auto take = \[&\]\(int bi, double m\)", "resolution"),  # the winner's broadcast (trees that have it here)
    (r"^    // first step of stage st from best MV", "search prologue"),
    (r"^    while \(stage >= 0\) \{", "generation"),
    (r"^        const int total = lo\[nseg - 1\]", "probe/emit"),  # the call of eval_candidates
    (r"^        HL_PROF_T\(tsel\);", "minima"),
    (r"^        auto seg_pick = ", "resolution"),
    (r"^        if \(used\) commit_candidates", "commit"),
    (r"^    // \(no barrier before these stores", "search end"),
    (r"^// Intra prediction \(8\.3", None),
]
REGIONS = ["search prologue", "mvp", "generation", "put_cand", "probe/emit", "miss path", "cost phase", "minima", "resolution", "commit",
           "record", "search end"]
CLASSES = ["VALU", "SALU", "LDS", "VMEM", "readlane", "branch", "waitcnt", "other"]


def line_regions(src):
    """Region of every line of the source file (1-based), by the anchors."""
    lines = open(src).read().splitlines()
    out, cur, k = [None] * (len(lines) + 2), None, 0
    for i, ln in enumerate(lines, 1):
        # anchors may be absent (a region that this tree does not have); look a few ahead
        for kk in range(k, len(ANCHORS)):
            if re.search(ANCHORS[kk][0], ln):
                cur, k = ANCHORS[kk][1], kk + 1
                break
        out[i] = cur
    return out


def classify(m):
    if m.startswith(("v_readlane", "v_readfirstlane")):
        return "readlane"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_waitcnt"):
        return "waitcnt"
    if m.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if m.startswith(("s_barrier", "s_nop", "s_sleep", "s_endpgm", "s_setprio")):
        return "other"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "VMEM"
    if m.startswith("s_"):
        return "SALU"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "VMEM"
    return "other"


def count(asm, kernel, regs):
    files, counts = {}, collections.defaultdict(collections.Counter)
    inside, cur, total = False, None, 0
    for ln in asm:
        s = ln.strip()
        m = re.match(r"\.file\s+(\d+)\s+(?:\"[^\"]*\"\s+)?\"([^\"]*)\"", s)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
            continue
        if not inside:
            if re.match(r"[A-Za-z_][\w$.]*:", s) and kernel in s and s.startswith("_Z"):
                inside = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if files.get(int(m.group(1))) == "hl_mbcore.h":
                n = int(m.group(2))
                cur = regs[n] if n < len(regs) else None
            continue
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        total += 1
        counts[cur][classify(s.split()[0])] += 1
    return counts, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--kernel", default="k_pipeline")
    ap.add_argument("--fam3", action="store_true")
    ap.add_argument("--root", default=ROOT, help="another checkout of the project (same anchors: a like-for-like comparison)")
    a = ap.parse_args()
    regs = line_regions(os.path.join(a.root, "hartallo_amd", "csrc", "hl_mbcore.h"))
    if a.asm:
        asm = open(a.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            src = os.path.join(a.root, "hartallo_amd", "csrc", "hl_encoder_fam3.hip" if a.fam3 else "hl_encoder.hip")
            subprocess.run([HIPCC] + FLAGS + ["-o", out, src], check=True)
            asm = open(out).read().splitlines()
    counts, total = count(asm, a.kernel, regs)
    print(f"{a.kernel}{' (fam3 build)' if a.fam3 else ''}: {total} instructions")
    print(f"{'region':16s} {'all':>6s} " + " ".join(f"{c:>8s}" for c in CLASSES))
    for r in REGIONS + [None]:
        c = counts.get(r, {})
        print(f"{(r or '(elsewhere)'):16s} {sum(c.values()):6d} " + " ".join(f"{c.get(k, 0):8d}" for k in CLASSES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
