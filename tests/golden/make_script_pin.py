"""Writes script_pin.json: for every case of tests/script_cases.py the digest of what each front-end (viamd_amd/script.py,
viamd_amd/csrc/vmd_script.cpp) makes of it in strict and in partial mode, on the CPU library.  tests/test_script_pin.py holds both
front-ends against these digests, so that reshaping a front-end cannot change a descriptor, a name, a message, a skipped record or
the fallback text unseen.  Each front-end has its own digest: the two word `unexpected character` differently.

Also checks that the corpus is worth pinning - a third of it compiles in strict mode, every descriptor call is reached by ten
accepted statements, every refusal of the statement forms is produced - and refuses to write the file otherwise.
Run: python tests/golden/make_script_pin.py [commit the digests are recorded from]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import conftest  # noqa: E402
import script_cases as SC  # noqa: E402
from viamd_amd import VmdLib  # noqa: E402

OUT = os.path.join(HERE, "script_pin.json")

# the refusals of the statement forms (the selection parser's own are not counted)
MESSAGES = (
    "rmsd defines one property, not a tuple", "unsupported function 'plane'", "unsupported expression '5'", "not 2", "not 1", ": missing ')'",
    "shape_weights takes one selection", "rmsd takes one selection", ": empty selection", ": empty selection inside a context",
    "`in` needs an array of structures", "an rdf argument takes exactly one within() factor, found 2",
    "an sdf argument takes exactly one within() factor, found 2", "count takes exactly one within() factor, found 2",
    "within() must be a factor of the top-level AND", "within range needs 0 <= a < b", "within needs a radius > 0",
    "a dynamic factor under a top-level or with a static selection", "within() nested in a within() argument",
    "more than four distinct within() terms", "a static selection inside a parenthesised dynamic factor",
    "within() in the structures argument of sdf() is not supported", "sdf reference structures must be non-empty and of equal size",
    "count of a static selection is a constant", "count(...) in <contexts> is outside the subset", "expected ;, found")


def descriptor_call(rec, mask):
    """the vmd_ir_add_* call that the C++ front-end makes for a property the Python front-end describes as `rec`"""
    kind = rec["kind"]
    if kind == "rdf":
        shell = rec.get("ref_shell") is not None or rec.get("target_shell") is not None
        return "rdf_shell+shell" if shell else "rdf" if not mask & SC.SHELL_RDF else "rdf_shell"
    if kind == "sdf":
        return "sdf_shell_expr" if "terms" in rec else "sdf_shell+shell" if "target_shell" in rec else "sdf_shell"
    if kind in ("within_count", "within_count_expr"):
        return "within_count_expr" if "terms" in rec else "within_count"
    if kind in ("angle", "dihedral"):
        return kind + ("_population" if isinstance(rec["sets"][0], list) else "")
    if kind in ("shape_weights", "rmsd"):
        return kind + "_population"
    return "distance_population" if "a_sets" in rec else "distance"


CALLS = ("rdf", "rdf_shell+shell", "sdf_shell", "sdf_shell+shell", "sdf_shell_expr", "distance", "distance_population", "angle", "dihedral",
         "angle_population", "dihedral_population", "shape_weights_population", "rmsd_population", "within_count", "within_count_expr")


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=HERE, text=True).strip()
    lib = VmdLib(conftest.build_emu())
    topo = SC.topology()
    cases, accepted, agree = [], 0, 0
    calls = dict.fromkeys(CALLS + ("rdf_shell",), 0)       # (rdf_shell without a shell: not one of the fifteen)
    seen = dict.fromkeys(MESSAGES, 0)
    for text, mask in SC.corpus():
        py, info = SC.outcome(False, text, mask, topo, lib)
        cc, _ = SC.outcome(True, text, mask, topo, lib)
        cases.append([text, mask, SC.digest(py), SC.digest(cc)])
        accepted += py["strict"][0] == "ok" and cc["strict"][0] == "ok"
        agree += py == cc
        for name, rec in (info[1] or {}).items():
            if rec["kind"] != "shape_weights" or rec["component"] == 0:           # a shape_weights statement is one call
                calls[descriptor_call(rec, mask)] += 1
        reasons = [o["strict"][1] for o in (py, cc) if o["strict"][0] == "error"]
        reasons += [k[3] for o in (py, cc) if o["partial"][0] == "ok" for k in o["partial"][3]]
        for m in MESSAGES:
            seen[m] += any(r.endswith(m) or m in r for r in reasons)
    print(f"{len(cases)} cases, {accepted} compile in strict mode, the two front-ends agree in full on {agree}")
    for k, v in calls.items():
        print(f"  {v:4d} accepted statements reach {k}")
    for k, v in seen.items():
        print(f"  {v:4d} cases produce {k!r}")
    problems = [f"only {accepted} of {len(cases)} cases compile in strict mode"] * (3 * accepted < len(cases))
    problems += [f"{k} is reached by {v} accepted statements only" for k, v in calls.items() if v < 10 and k in CALLS]
    problems += [f"no case produces {k!r}" for k, v in seen.items() if v == 0]
    if problems:
        raise SystemExit("the corpus does not meet its conditions:\n  " + "\n  ".join(problems))
    header = dict(recorded_from=commit, cases=len(cases), strict_accepted=accepted, front_ends_agree=agree, descriptor_calls=calls,
                  columns=["text", "feature mask", "digest of viamd_amd/script.py", "digest of vmd_script.cpp"])
    with open(OUT, "w") as f:
        f.write('{"header": ' + json.dumps(header) + ',\n "cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
