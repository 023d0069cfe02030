"""Random scripts through both front-ends (viamd_amd/script.py and the C++ vmd_ir_compile_from_source): both must accept and
produce the same IR fingerprint, or both must reject.  Every script also goes through the PARTIAL mode of both (round 5), salted with statements
outside the subset (arithmetic, within() on its own, stray characters): same compiled properties, same skipped names and source ranges, same
fallback text; whatever the strict mode accepts the partial mode compiles identically with nothing skipped.
The statements come from tests/script_cases.py, the generator of the pinned corpus, under a random feature mask each.
usage: python scripts/fuzz_script.py [cases] [seed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest
import script_cases as SC
import viamd_amd as V
from viamd_amd import script

lib = V.VmdLib(conftest.build_emu())
topo = SC.topology()
ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
gen = SC.Generator(int(sys.argv[2]) if len(sys.argv) > 2 else 0, bad=0.1)      # the statements of the pinned corpus, opt-in forms included
rng, rint, statement, foreign = gen.rng, gen.rint, gen.statement, gen.foreign


agree_ok = agree_err = partial_ok = 0
for it in range(ncases):
    mask = rng.choice(SC.MASKS)
    kw = SC.keywords(mask)
    text = "s0 = residue(2:6); " + "; ".join(statement(i, mask) for i in range(rint(1, 4))) + rng.choice([";", "", " ;  # tail comment"])
    res = []
    for fn in (lambda: script.compile_script(text, topo, lib=lib, **kw)[0], lambda: script.compile_script_native(text, topo, lib=lib, **kw)):
        try:
            ir = fn()
            res.append(("ok", ir.fingerprint(), tuple(ir.property_names())))
        except (script.ScriptError, V.VmdError, ValueError) as e:
            res.append(("err", str(e)[:80]))
    if res[0][0] != res[1][0] or (res[0][0] == "ok" and res[0] != res[1]):
        print("DISAGREE:", mask, text, res)
    elif res[0][0] == "ok":
        agree_ok += 1
    else:
        agree_err += 1
    # partial mode: the same statements with a few foreign ones mixed in
    parts = ["s0 = residue(2:6)"] + [statement(i, mask) if rng.random() < 0.7 else foreign(i) for i in range(rint(1, 5))]
    ptext = "; ".join(parts) + rng.choice([";", ""])
    try:
        ir_py, _, rep_py = script.compile_script(ptext, topo, lib=lib, partial=True, **kw)
        ir_c, rep_c = script.compile_script_native(ptext, topo, lib=lib, partial=True, **kw)
        same = (ir_py.fingerprint() == ir_c.fingerprint() and ir_py.property_names() == ir_c.property_names() and
                [(k["names"], k["beg"], k["end"]) for k in rep_py["skipped"]] == [(k["names"], k["beg"], k["end"]) for k in rep_c["skipped"]] and
                rep_py["fallback_source"] == rep_c["fallback_source"] and len(rep_c["fallback_source"]) == len(ptext))
        if res[0][0] == "ok":      # the strict text above: partial mode must agree with strict mode, nothing skipped
            ir_s, rep_s = script.compile_script_native(text, topo, lib=lib, partial=True, **kw)
            same = same and rep_s["skipped"] == [] and ir_s.fingerprint() == res[1][1]
        if not same:
            print("PARTIAL DISAGREE:", mask, ptext, rep_py["skipped"], rep_c["skipped"])
        else:
            partial_ok += 1
    except Exception as e:          # noqa: BLE001
        print("PARTIAL ERROR:", mask, ptext, repr(e)[:200])
print(f"{ncases} scripts: {agree_ok} accepted identically, {agree_err} rejected by both; partial mode: {partial_ok} of {ncases} agree (properties, skipped names and ranges, fallback text)")
