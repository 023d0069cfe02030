"""Writes ir_pin.json: for every case of tests/ir_cases.py what the vmd_ir_add_* entry points (viamd_amd/csrc/vmd_eval_ir.cpp) make of
it on the CPU library - per call `ok` or the text of vmd_last_error, then the fingerprint, the names, their flags, the work estimate, the
atoms vmd_ir_geometry_atoms lists (contexts -1, 0, P - 1 and P with an ample buffer, -1 and 0 again with half the room) and what
vmd_eval_create sets up per property over 3 frames under both settings of spec_angle_radians.  tests/test_ir_pin.py holds the library
against the file, so that reshaping the descriptor cannot change a fingerprint, a message, the order of two checks or a view unseen.
Also writes ir_cases.txt, the same cases with their lists written out, which tests/native/ir_replay.cpp replays under sanitizers.

Refuses to write unless every entry point is reached by an accepted call and every refusal of vmd_eval_ir.cpp is produced.
Run: python tests/golden/make_ir_pin.py [commit the outcomes are recorded from]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import conftest  # noqa: E402
import ir_cases as IC  # noqa: E402
from viamd_amd import VmdLib  # noqa: E402

OUT = os.path.join(HERE, "ir_pin.json")
DUMP = os.path.join(HERE, "ir_cases.txt")

# every vmd_fail text of vmd_eval_ir.cpp, with what its % arguments become in some case
MESSAGES = (
    "ir is NULL", "property name is empty", "property 'r0' already defined", "rdf reference set is empty",
    "rdf target set contains a negative atom index", "rdf range must satisfy 0 <= rmin < rmax", "sdf cutoff must be positive",
    "unknown distance kind 4", "distance population is empty", "context offsets must start at 0", "distance context 1 has an empty set",
    "distance_pair needs contexts of equal size", "angle population is empty", "dihedral population is empty",
    "angle set b has no context offsets", "dihedral set d has no context offsets",
    "angle context 1 has an empty set c (offsets must increase)", "dihedral context 0 has an empty set d (offsets must increase)",
    "angle set too large", "dihedral set too large", "shape_weights needs three property names", "shape_weights population is empty",
    "shape_weights set has no context offsets", "shape_weights context 1 has an empty set (offsets must increase)",
    "shape_weights set too large", "rmsd population is empty", "rmsd set has no context offsets",
    "rmsd context 1 has an empty set (offsets must increase)", "rmsd set too large",
    "within range must be finite and satisfy 0 <= rmin < rmax", "shell expression is NULL", "shell expression needs 1 to 4 terms, got 5",
    "shell expression truth table has bits above 2^2", "ramachandran needs two property names and a backbone",
    "ramachandran backbone has no segment", "ramachandran backbone too large", "ramachandran backbone has a NULL atom list",
    "ramachandran backbone has no range offsets", "backbone range offsets must start at 0", "backbone range 0 is empty (offsets must increase)",
    "backbone range offsets end at 1, not at the 2 segments", "backbone segment 1 has class 7 (0..3 or 255)")
# ... except this one.  Each of its five sites stands behind idx_ok over the list in question, which reads every entry: a call that
# reaches it needs a list of 2^31 valid indices (8 GiB), which no quick test and no sanitizer run can afford
NOT_PRODUCED = ("within set too large",)


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=HERE, text=True).strip()
    lib = VmdLib(conftest.build_emu())
    cases, reached, produced = [], set(), set()
    for cid, P, lines in IC.cases():
        out, r = IC.outcome(lib, P, lines)
        cases.append([cid, out])
        reached |= r
        produced |= set(out["calls"])
    source = open(os.path.join(os.path.dirname(TESTS), "viamd_amd", "csrc", "vmd_eval_ir.cpp")).read()
    fails = source.count("vmd_fail(")
    problems = [f"no accepted call reaches vmd_ir_add_{e}" for e in IC.SPEC if e not in reached]
    problems += [f"no call produces {m!r}" for m in MESSAGES if m not in produced]
    problems += [f"{m!r} is not a text of vmd_eval_ir.cpp" for m in NOT_PRODUCED if m not in source]
    for msg in produced - {"ok"}:
        print(f"  {msg}")
    print(f"{len(cases)} cases, {sum(len(c[1]['calls']) for c in cases)} calls, {len(produced) - 1} distinct refusals; vmd_eval_ir.cpp holds "
          f"{fails} vmd_fail sites")
    if problems:
        raise SystemExit("the cases do not meet their conditions:\n  " + "\n  ".join(problems))
    header = dict(recorded_from=commit, cases=len(cases), entry_points=sorted(reached), not_produced=list(NOT_PRODUCED))
    with open(OUT, "w") as f:
        f.write('{"header": ' + json.dumps(header) + ',\n "cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    with open(DUMP, "w") as f:
        f.write(IC.dump())
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; {DUMP}: {os.path.getsize(DUMP)} bytes")


if __name__ == "__main__":
    main()
