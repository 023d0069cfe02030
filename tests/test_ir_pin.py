"""The vmd_ir_add_* entry points against tests/golden/ir_pin.json: for every case of tests/ir_cases.py the outcome of each call (`ok` or
the refusal's text), the fingerprint, names, flags, work estimate, the atoms of vmd_ir_geometry_atoms and what vmd_eval_create sets up
per property are what tests/golden/make_ir_pin.py recorded.  Pure host code: no GPU - where the library finds no device (the product
library on a machine without one) vmd_eval_create has nothing to run on and the descriptor part alone is held."""
import json
import os

import ir_cases as IC

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = os.path.join(HERE, "golden", "ir_pin.json")


def pinned():
    with open(PIN) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones():
    pin = pinned()
    assert pin["header"]["cases"] == len(pin["cases"])
    assert [cid for cid, _ in pin["cases"]] == [cid for cid, _, _ in IC.cases()]
    assert sorted(IC.SPEC) == pin["header"]["entry_points"]
    for cid, out in pin["cases"]:
        assert bool(out["names"]) == ("eval" in out), cid
    with open(os.path.join(HERE, "golden", "ir_cases.txt")) as f:
        assert f.read() == IC.dump()


def test_the_entry_points_give_the_recorded_outcomes(host_lib):
    with_eval = host_lib.vmd_device_count() > 0
    want = dict(pinned()["cases"])
    wrong = []
    for cid, P, lines in IC.cases():
        got, _ = IC.outcome(host_lib, P, lines, with_eval=with_eval)
        ref = dict(want[cid])
        if not with_eval:
            ref.pop("eval", None)
        got = json.loads(json.dumps(got))
        if got != ref:
            wrong.append(cid)
            for key in ref:
                if got.get(key) != ref[key]:
                    print(f"{cid}: {key}\n  got  {json.dumps(got.get(key))}\n  want {json.dumps(ref[key])}")
    assert not wrong, f"{len(wrong)} cases differ from the recorded outcomes: {wrong}"


def test_the_replay_under_sanitizers_reports_nothing(tmp_path):
    """tests/native/ir_replay.cpp and vmd_eval_ir.cpp alone, g++ -fsanitize=address,undefined, on the CPU: every call of the cases, then the
    fingerprint, the work estimate and vmd_ir_geometry_atoms with room for half the atoms.  Nothing on stderr, and what it prints is the pin's."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "ir_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(HERE, "emu"), "-I" + os.path.join(root, "include"), os.path.join(HERE, "native", "ir_replay.cpp"),
                           "-x", "c++", os.path.join(root, "viamd_amd", "csrc", "vmd_eval_ir.cpp"), "-o", exe])
    out = subprocess.run([exe, os.path.join(HERE, "golden", "ir_cases.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    want = []
    for cid, rec in pinned()["cases"]:
        want += ["case " + cid] + rec["calls"] + ["= " + rec["fingerprint"]]
    got = [line.rsplit(" ", 1)[0] if line.startswith("= ") else line for line in out.stdout.splitlines()]
    assert got == want
