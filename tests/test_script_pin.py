"""Both script front-ends against tests/golden/script_pin.json: for every case of the corpus (tests/script_cases.py) the digest of the
whole outcome - strict mode: fingerprint and names, or the error text; partial mode: fingerprint, names, skipped records with their
reasons, fallback text - is what tests/golden/make_script_pin.py recorded.  Pure host code: no GPU."""
import json
import os

import script_cases as SC

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "script_pin.json")


def pinned():
    with open(PIN) as f:
        return json.load(f)


def test_the_corpus_is_the_recorded_one():
    pin = pinned()
    assert pin["header"]["cases"] == len(pin["cases"])
    assert [(text, mask) for text, mask, *_ in pin["cases"]] == SC.corpus()


def test_both_front_ends_give_the_recorded_outcomes(host_lib):
    topo = SC.topology()
    wrong = []
    for text, mask, want_py, want_cc in pinned()["cases"]:
        for native, want in ((False, want_py), (True, want_cc)):
            got, _ = SC.outcome(native, text, mask, topo, host_lib)
            if SC.digest(got) != want:
                wrong.append((text, mask, native))
                print(f"{'vmd_script.cpp' if native else 'script.py'}, mask {mask}: {text!r}\n  -> {json.dumps(got)}")
    assert not wrong, f"{len(wrong)} outcomes differ from the recorded ones, the first: {wrong[0]}"
