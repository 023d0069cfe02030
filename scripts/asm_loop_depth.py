#!/usr/bin/env python3
"""Static instruction count of one kernel by loop depth, from hipcc's assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -x hip --cuda-device-only -S \
          viamd_amd/csrc/vmd_kernels.hip -o kernels.s
    python scripts/asm_loop_depth.py kernels.s _Z12k_rdf_pencilILi0ELb1ELi0ELb1ELi2EEv17vmd_pair_params_t

LLVM annotates every basic block that lies in a loop with the depth of its innermost loop ("This Loop Header: Depth=N",
"in Loop: Header=... Depth=N").  The script sums, per depth, the vector-ALU instructions (and, of those, the cross-lane moves between
VGPR lanes and SGPRs), the scalar-ALU instructions and the scalar / vector / LDS memory instructions of the blocks at that depth.  Static
counts: they say what a trip through a loop level costs at most, not how often it is taken.  Needs no GPU."""
import collections
import re
import sys

LANE_MOVES = ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32")


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_setprio", "s_sleep")):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


def count(path, symbol):
    depth = 0
    inside = False
    pending_label = False
    out = collections.defaultdict(collections.Counter)
    for line in open(path):
        if not inside:
            inside = line.startswith(symbol + ":")
            continue
        if line.startswith(".Lfunc_end"):
            break
        s = line.strip()
        if re.match(r"\.LBB\d+_\d+:", s) or s.startswith("; %bb."):
            # the annotation of a block starts on the line of its label and may go on in comment lines below it
            depth, pending_label = 0, True
        if s.startswith((";", ".LBB")) or not s:
            if pending_label:
                m = re.search(r"(?:This (?:Inner )?Loop Header: Depth=|in Loop: Header=\S+ Depth=)(\d+)", s)
                if m:
                    depth = int(m.group(1))
            continue
        if s.startswith("."):
            continue
        pending_label = False
        text = s.split(";", 1)[0]
        # an inline-asm block is one listing line per instruction as well; "\n\t" was expanded by the assembler printer
        op = text.split()[0]
        kind = classify(op)
        out[depth][kind] += 1
        if op in LANE_MOVES:
            out[depth]["lane_moves"] += 1
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    out = count(sys.argv[1], sys.argv[2])
    if not out:
        sys.exit(f"{sys.argv[2]}: no such function in {sys.argv[1]}")
    print(f"{'depth':>5} {'VALU':>6} {'lane moves':>10} {'SALU':>6} {'SMEM':>6} {'VMEM':>6} {'LDS':>6}")
    for d in sorted(out):
        c = out[d]
        print(f"{d:>5} {c['valu']:>6} {c['lane_moves']:>10} {c['salu']:>6} {c['smem']:>6} {c['vmem']:>6} {c['lds']:>6}")


if __name__ == "__main__":
    main()
