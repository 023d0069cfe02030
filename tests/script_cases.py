"""The script corpus of the two front-ends (viamd_amd/script.py and viamd_amd/csrc/vmd_script.cpp): a deterministic generator of
(text, feature mask) cases over every statement form either front-end takes, and the digest of what a front-end makes of a case.
tests/golden/make_script_pin.py records the digests (tests/golden/script_pin.json), tests/test_script_pin.py holds both front-ends
against them, scripts/fuzz_script.py draws its random statements from the same generator.

A new statement form gets one generator method here, an entry in Generator.FORMS, and the refusals it adds a line in EDGE_CASES.
No numpy RNG: random.Random(seed) is the same sequence on every platform and version."""
import hashlib
import json
import random

from viamd_amd import script, synth
from viamd_amd.eval import VmdError

ANGLES, SHAPE, RMSD, WITHIN, SHELL_RDF, SHELL_SDF, SHELL_EXPR = (script.FEATURE_ANGLES, script.FEATURE_SHAPE, script.FEATURE_RMSD,
                                                                 script.FEATURE_WITHIN, script.FEATURE_SHELL_RDF, script.FEATURE_SHELL_SDF,
                                                                 script.FEATURE_SHELL_EXPR)
ALL = 127
KEYWORDS = ((ANGLES, "angles"), (SHAPE, "shape"), (RMSD, "rmsd"), (WITHIN, "within"), (SHELL_RDF, "shell_rdf"), (SHELL_SDF, "shell_sdf"),
            (SHELL_EXPR, "shell_expr"))
# 0, all seven bits, each bit alone, and the combinations under which the shell forms take their other routes
MASKS = (0, ALL, ALL, ALL, ANGLES, SHAPE, RMSD, WITHIN, SHELL_RDF, SHELL_SDF, SHELL_EXPR, ANGLES | SHAPE, SHAPE | RMSD, WITHIN | SHELL_EXPR,
         SHELL_SDF | SHELL_EXPR, SHELL_RDF | SHELL_SDF, WITHIN | SHELL_RDF | SHELL_SDF, ALL & ~SHELL_EXPR, ALL & ~SHELL_EXPR,
         ALL & ~WITHIN, ALL & ~SHELL_SDF, WITHIN, WITHIN | ANGLES | RMSD)
CORPUS_SEED = 20240
CORPUS_RANDOM_CASES = 460
PREFIX = "s0 = residue(2:6); "


def keywords(mask):
    """the feature mask as the keyword arguments of script.compile_script / compile_script_native"""
    return {kw: bool(mask & bit) for bit, kw in KEYWORDS}


def topology():
    """30 ALA residues of 10 atoms, then 100 waters: what the fuzzer uses"""
    return synth.water_box_topology(300 + 300, n_blob=300)


class Generator:
    """Random statements.  bad: the chance that a leaf is one that cannot compile (an index out of range, an empty selection, ...)."""

    def __init__(self, seed, bad=0.04):
        self.rng = random.Random(seed)
        self.bad = bad

    # ---- leaves ----------------------------------------------------------------------------------------------------------------------------
    def rint(self, lo, hi):
        return self.rng.randint(lo, hi)

    def pick(self, seq):
        return seq[self.rng.randrange(len(seq))]

    def range_(self, hi, wide=None):
        """a | a:b within 1..hi; with the chance `bad` one that starts at 0 or ends past hi"""
        if self.rng.random() < self.bad:
            a = self.rint(0, hi + 2)
            return str(a) if self.rng.random() < 0.4 else f"{a}:{self.rint(max(0, a - 1), hi + 3)}"
        a = self.rint(1, hi)
        if self.rng.random() < 0.4:
            return str(a)
        return f"{a}:{self.rint(a, min(hi, a + (wide or hi)))}"

    def atom_sel(self, depth=0):
        r = self.rng.random()
        if depth > 2 or r < 0.6:
            if self.rng.random() < self.bad:
                return self.pick(["type('Q')", "resid(3)", "nobody", "residue(0)", "atom(601)", "water[101]", "all[1]", "plane(all)"])
            return self.pick(["all", "water", "protein", "element('O')", "element('H', 'C')", "name('N')", 'resname("ALA")', "resname('HOH')",
                              f"residue({self.range_(130)})", f"atom({self.range_(600)})", self.range_(600),
                              f'resname("ALA")[{self.range_(30)}]', f"water[{self.range_(100)}]", "label('O')", "s0"])
        if r < 0.72:
            return f"not {self.atom_sel(depth + 1)}"
        if r < 0.86:
            return f"({self.atom_sel(depth + 1)} {self.pick(['and', 'or'])} {self.atom_sel(depth + 1)})"
        return f"{self.atom_sel(depth + 1)} {self.pick(['and', 'or', 'or'])} {self.atom_sel(depth + 1)}"

    def struct_sel(self):
        """the structures argument of sdf(): mostly arrays of equally sized structures"""
        if self.rng.random() < 0.12:
            return self.atom_sel()
        return self.pick([f'resname("ALA")[{self.range_(30, 6)}]', f"water[{self.range_(100, 8)}]", f"residue({self.range_(30, 5)})",
                          f"residue({31 + self.rint(0, 90)}:{125 + self.rint(0, 5)})", "s0", "s0[2:3]", f"residue({self.range_(130, 3)})",
                          "water and element('O')", f"atom({self.range_(600, 12)})"])

    def context(self):
        """-> (`in` clause, atoms per structure)"""
        if self.rng.random() < 0.08:
            return self.pick([" in all", " in element('O')", " in type('Q')", " in protein and not protein"]), 3
        if self.rng.random() < 0.5:
            return " in " + self.pick([f"water[{self.range_(100, 10)}]", f"residue({31 + self.rint(0, 60)}:{95 + self.rint(0, 35)})", "water"]), 3
        return " in " + self.pick([f'resname("ALA")[{self.range_(30, 8)}]', f"residue({self.range_(30, 4)})", "s0", "protein"]), 10

    def local_sel(self, size):
        """an argument under `in`: indices are local to the context"""
        r = self.rng.random()
        if r < 0.6:
            return self.range_(size)
        if r < 0.75:
            return f"atom({self.range_(size)})"
        return self.pick(["element('H')", "element('O')", "all", "not element('H')"] + ["element('C', 'N')", "name('N')"] * (size == 10))

    def radius(self):
        if self.rng.random() < self.bad:
            return self.pick(["0", "0.0", "5:3", "2.5:2.5"])
        return self.pick(["3.5", "5.0", "2.8", "6", "0.5:2.8", "1:4.5", "3.0:6.0", ".5"])

    def within(self):
        return f"within({self.radius()}, {self.atom_sel(1)})"

    # ---- statement forms ---------------------------------------------------------------------------------------------------------------------
    def selection(self, i):
        return f"s{i} = {self.atom_sel()}"

    def rdf_cut(self):
        return self.pick(["7.5", "{1.0, 6.25}", "0.5:9", "12", ".5"])

    def rdf(self, i):
        return f"g{i} = rdf({self.atom_sel()}, {self.atom_sel()}, {self.rdf_cut()})"

    def sdf(self, i):
        return f"v{i} = sdf({self.struct_sel()}, {self.atom_sel()}, {self.pick(['4.0', '10', '3.25e0'])})"

    def geometry(self, i, fn, nargs):
        if self.rng.random() < 0.5:
            return f"{fn[0]}{i} = {fn}({', '.join(self.atom_sel() for _ in range(nargs))})"
        ctx, size = self.context()
        return f"{fn[0]}{i} = {fn}({', '.join(self.local_sel(size) for _ in range(nargs))}){ctx}"

    def distance(self, i):
        return self.geometry(i, self.pick(["distance", "distance_min", "distance_max", "distance_pair"]), 2)

    def angle(self, i):
        return self.geometry(i, "angle", 3)

    def dihedral(self, i):
        return self.geometry(i, "dihedral", 4)

    def one_selection(self, fn):
        """shape_weights / rmsd behind the `=`: one selection, plain or per context, now and then two"""
        if self.rng.random() < 0.5:
            args = [self.atom_sel()]
            ctx = ""
        else:
            ctx, size = self.context()
            args = [self.local_sel(size) if self.rng.random() < 0.5 else self.pick(["all", "not element('H')", "element('C', 'N', 'O')"])]
        if self.rng.random() < 0.06:
            args.append("water")
        return f"{fn}({', '.join(args)}){ctx}"

    def shape(self, i):
        r = self.rng.random()
        lhs = f"{{l{i}, p{i}, i{i}}}" if r < 0.86 else f"{{l{i}, p{i}}}" if r < 0.93 else f"w{i}"
        return f"{lhs} = {self.one_selection('shape_weights')}"

    def rmsd(self, i):
        lhs = f"m{i}" if self.rng.random() < 0.9 else f"{{m{i}, n{i}}}"
        return f"{lhs} = {self.one_selection('rmsd')}"

    def shell(self):
        """an AND with exactly one within() factor at its top level"""
        parts = [self.atom_sel(1) for _ in range(self.rint(0, 2))]
        parts.insert(self.rint(0, len(parts)), self.within())
        return " and ".join(parts)

    def shell_expr(self):
        """an AND of static factors and of within(), not within() and parenthesised and / or / not over within() terms"""
        pool = [self.within() for _ in range(self.rint(1, 3))]

        def term(depth=0):
            r = self.rng.random()
            if depth > 1 or r < 0.5:
                return self.pick(pool)
            if r < 0.7:
                return f"not {term(depth + 1)}"
            return f"({term(depth + 1)} {self.pick(['and', 'or'])} {term(depth + 1)})"

        parts = [self.atom_sel(1) for _ in range(self.rint(0, 2))] + [term() for _ in range(self.rint(1, 3))]
        self.rng.shuffle(parts)
        return " and ".join(parts)

    def count(self, i):
        r = self.rng.random()
        w = self.within
        if r < 0.45:
            arg = self.shell()
        elif r < 0.8:
            arg = self.shell_expr()
        else:
            arg = self.pick([f"{self.atom_sel(1)} and {w()} and {w()}",                           # several
                             f"{self.atom_sel(1)} and not {w()}",                                 # not
                             f"{self.atom_sel(1)} and ({w()} or {w()})",                          # a parenthesised or
                             f"within({self.radius()}, {w()})",                                    # nested
                             f"{self.atom_sel(1)} or {w()}",                                      # under a top-level or
                             f"{self.atom_sel(1)} and ({w()} or water)",                          # a static selection among the dynamic terms
                             f"({self.atom_sel(1)} and {w()})",                                   # one within(), but in parentheses
                             self.atom_sel(), f"{self.atom_sel(1)}, {w()}"])                      # static; two arguments
        tail = self.pick([" in residue(1:3)", " in water"]) if self.rng.random() < 0.06 else ""
        return f"n{i} = count({arg}){tail}"

    def shell_rdf(self, i):
        side = self.rint(1, 3)
        a = self.shell() if side & 1 else self.atom_sel()
        b = self.shell() if side & 2 else self.atom_sel()
        if self.rng.random() < 0.1:
            a = self.pick([f"{self.within()} and {self.within()}", f"not {self.within()}", f"water or {self.within()}"])
        return f"g{i} = rdf({a}, {b}, {self.rdf_cut()})"

    def shell_sdf(self, i):
        ref = self.struct_sel()
        r = self.rng.random()
        if r < 0.08:
            ref = f"{ref} and {self.within()}"                                                     # within() in the structures
        tgt = self.shell() if r < 0.6 else self.shell_expr() if r < 0.92 else f"({self.within()})"
        return f"v{i} = sdf({ref}, {tgt}, {self.pick(['4.0', '10', '3.25e0'])})"

    def foreign(self, i):
        """statements outside the subset under every mask"""
        return self.pick([f"x{i} = 3 * 4 + 2", f"w{i} = within(5.0, protein)", f"q{i} = rdf(w{max(i - 1, 0)}, all, 5.0)", f"z{i} = rmsd(protein) @ 2",
                          f"y{i} = distance(1, 2) + 1", "{a,b} = plane(resname('ALA'))", f"u{i} = 'unterminated", f"{{a{i}}} = 5", f"k{i} = $"])

    # (method, the feature bits it needs, weight)
    FORMS = ((selection, 0, 3), (rdf, 0, 4), (sdf, 0, 4), (distance, 0, 5), (angle, ANGLES, 5), (dihedral, ANGLES, 6), (shape, SHAPE, 4),
             (rmsd, RMSD, 4), (count, WITHIN, 9), (shell_rdf, SHELL_RDF, 4), (shell_sdf, SHELL_SDF, 10))

    def statement(self, i, mask=0):
        """a statement of a form that `mask` takes; one time in ten of any form (the forms the mask leaves out are then refused)"""
        forms = self.FORMS if self.rng.random() < 0.1 else [f for f in self.FORMS if mask & f[1] == f[1]]
        r = self.rng.random() * sum(f[2] for f in forms)
        for method, _, weight in forms:
            r -= weight
            if r < 0:
                return method(self, i)
        return forms[-1][0](self, i)

    def malform(self, text):
        """the malformed tails: a missing `)`, a missing comma, an unterminated string"""
        kind = self.rint(0, 2)
        if kind == 0 and ")" in text:
            k = text.rindex(")")
            return text[:k] + text[k + 1:]
        if kind == 1 and ", " in text:
            k = text.rindex(", ")
            return text[:k] + text[k + 1:]
        return text + " t = name('N"

    def script(self, mask):
        parts = [self.statement(i, mask) if self.rng.random() < 0.94 else self.foreign(i) for i in range(1, self.rint(1, 3) + 1)]
        text = PREFIX + "; ".join(parts)
        if self.rng.random() < 0.06:
            return self.malform(text)
        return text + self.pick([";", ";", "", " ;  # tail comment"])


# every refusal of the statement forms, once at least, whatever the random part draws: (text, mask)
EDGE_CASES = (
    ("{a, b} = rmsd(protein);", RMSD),
    ("{a, b} = rmsd(protein);", 0),
    ("{a, b, c} = plane(protein);", ALL),
    ("{a, b, c} = 5;", SHAPE),
    ("{a, b} = shape_weights(protein);", SHAPE),
    ("{a, b, c} = shape_weights(protein;", SHAPE),
    ("{a, b, c} = shape_weights(protein, water);", SHAPE),
    ("{a, b, c} = shape_weights(type('Q'));", SHAPE),
    ("{a, b, c} = shape_weights(element('O')) in resname('ALA')[1:2];", SHAPE),
    ("{a, b, c} = shape_weights(all) in all;", SHAPE),
    ("{a, b, c} = shape_weights(all) in type('Q');", SHAPE),
    ("{a, b, c} = shape_weights(all) in water[1:3]; d = distance(a, 1) + 1;", ALL),
    ("a = shape_weights(protein);", SHAPE),
    ("a = shape_weights(protein);", 0),
    ("g = rdf(water and within(3, protein) and within(4, protein), all, 5.0);", SHELL_RDF),
    ("g = rdf(all, not within(3, protein), 5.0);", SHELL_RDF),
    ("g = rdf(all, water or within(3, protein), 5.0);", SHELL_RDF),
    ("g = rdf(all, (within(3, protein)), 5.0);", SHELL_RDF),
    ("g = rdf(within(5:3, protein), all, 5.0);", SHELL_RDF),
    ("g = rdf(within(0, protein), all, 5.0);", SHELL_RDF),
    ("g = rdf(within(3, type('Q')), all, 5.0);", SHELL_RDF),
    ("g = rdf(type('Q') and within(3, protein), all, 5.0);", SHELL_RDF),
    ("g = rdf(type('Q'), all, 5.0);", 0),
    ("g = rdf(water and within(3, protein), within(1:4, water) and element('O'), {0.5, 6});", ALL),
    ("g = rdf(water and within(3, protein), all, 5.0);", 0),
    ("v = sdf(s0 and within(3, water), water, 4.0);", SHELL_SDF),
    ("v = sdf(residue(29:32), water, 4.0);", 0),
    ("v = sdf(residue(29:32), water and within(3, protein), 4.0);", SHELL_SDF),
    ("v = sdf(type('Q'), water, 4.0);", SHELL_SDF | SHELL_EXPR),
    ("v = sdf(resname('ALA')[1:0], water, 4.0);", 0),
    ("v = sdf(s0, type('Q') and within(3, protein), 4.0);", SHELL_SDF),
    ("v = sdf(s0, type('Q') and not within(3, protein), 4.0);", SHELL_SDF | SHELL_EXPR),
    ("v = sdf(s0, water and within(3, protein) and within(4, protein), 4.0);", SHELL_SDF),
    ("v = sdf(s0, water and within(3, protein) and not within(4, s0), 4.0);", SHELL_SDF | SHELL_EXPR),
    ("v = sdf(s0, water or within(3, protein), 4.0);", SHELL_SDF | SHELL_EXPR),
    ("n = count(water);", WITHIN),
    ("n = count(water);", WITHIN | SHELL_EXPR),
    ("n = count(water);", 0),
    ("n = count(water and within(3, protein)) in residue(1:3);", WITHIN),
    ("n = count(water and within(3, protein)) in residue(1:3);", WITHIN | SHELL_EXPR),
    ("n = count(water and within(3, protein) and within(4, protein));", WITHIN),
    ("n = count(water and (within(3, protein)));", WITHIN),
    ("n = count(water or within(3, protein));", WITHIN),
    ("n = count(water or within(3, protein));", WITHIN | SHELL_EXPR),
    ("n = count(water and within(3, protein);", WITHIN),
    ("n = count(water, within(3, protein));", WITHIN),
    ("n = count(water, within(3, protein));", WITHIN | SHELL_EXPR),
    ("n = count(within(3, protein), water);", WITHIN),
    ("n = count(within(4:2, protein));", WITHIN),
    ("n = count(within(0.0, protein));", WITHIN),
    ("n = count(within(4:2, protein));", WITHIN | SHELL_EXPR),
    ("n = count(within(0.0, protein));", WITHIN | SHELL_EXPR),
    ("n = count(within(3, type('Q')));", WITHIN),
    ("n = count(within(3, type('Q')));", WITHIN | SHELL_EXPR),
    ("n = count(type('Q') and within(3, protein));", WITHIN),
    ("n = count(type('Q') and within(3, protein));", WITHIN | SHELL_EXPR),
    ("n = count(within(3, within(2, protein)));", WITHIN | SHELL_EXPR),
    ("n = count(within(3, within(2, protein)));", WITHIN),
    ("n = count(within(1, s0) and within(2, s0) and within(3, s0) and within(4, s0) and not within(5, s0));", WITHIN | SHELL_EXPR),
    ("n = count(within(1, s0) and within(2, s0) and within(3, s0) and within(4, s0) and not within(1, s0));", WITHIN | SHELL_EXPR),
    ("n = count(water and (within(3, protein) or water));", WITHIN | SHELL_EXPR),
    ("n = count(water and not (within(3, protein) and not within(2:5, s0)));", ALL),
    ("m = rmsd(protein, water);", RMSD),
    ("m = rmsd(type('Q'));", RMSD),
    ("m = rmsd(element('O')) in resname('ALA')[1:2];", RMSD),
    ("m = rmsd(all) in all;", RMSD),
    ("m = rmsd(protein;", RMSD),
    ("m = rmsd(all) in water[1:4]; x = m * 2;", RMSD),
    ("m = rmsd(protein);", 0),
    ("d = distance(1, 2) in all;", 0),
    ("d = distance(1, 2;", 0),
    ("d = distance(1 2);", 0),
    ("d = distance(4, 1) in water[1:3];", 0),
    ("d = distance(element('N'), 1) in water[1:3];", 0),
    ("a = angle(element('N'), 1, 2) in water[1:3];", ANGLES),
    ("a = angle(2, 1, 3) in resname(\"ALA\");", ANGLES),
    ("a = angle(2, 1, 3) in resname(\"ALA\");", 0),
    ("a = angle(1, 2);", ANGLES),
    ("a = dihedral(1, 2, 3, 4) in residue(1:30); b = dihedral(1, 2, 3, 4, 5);", ANGLES),
    ("d = distance(1, 2) extra;", 0),
    ("d = distance(1, 2) d2 = distance(2, 3);", 0),
    ("d = distance(1, 2); x = d * 2; e = distance(2, 3);", 0),
    ("d = distance(1, 2);;; ; e = 'open", 0),
    ("d = distance(1, 2) # no semicolon", 0),
    ("= 5; d = distance(1, 2);", 0),
    ("d = distance(1.5, 2);", 0),
    ("", 0),
    ("# nothing but a comment", ALL),
)


def corpus():
    """[(text, mask)]: the edge cases, each behind the prefix that binds s0, then the random scripts"""
    gen = Generator(CORPUS_SEED)
    out = [(PREFIX + text if text else text, mask) for text, mask in EDGE_CASES]
    for k in range(CORPUS_RANDOM_CASES):
        mask = MASKS[k % len(MASKS)]
        out.append((gen.script(mask), mask))
    return out


# ---- what a front-end makes of a case --------------------------------------------------------------------------------------------------------

def outcome(native, text, mask, topo, lib):
    """the whole outcome of one front-end on one case, as JSON-able data.  strict: fingerprint and names, or the error text; partial:
    fingerprint, names, the skipped records and the fallback text.  (+ the Python front-end's info, for make_script_pin's counts)"""
    kw = keywords(mask)
    fn = script.compile_script_native if native else script.compile_script
    info = [None, None]
    try:
        res = fn(text, topo, lib=lib, **kw)
        ir = res if native else res[0]
        info[0] = None if native else res[1]
        strict = ["ok", str(ir.fingerprint()), ir.property_names()]
    except (script.ScriptError, VmdError, ValueError) as e:
        strict = ["error", str(e)]
    try:
        res = fn(text, topo, lib=lib, partial=True, **kw)
        ir, rep = res[0], res[-1]
        info[1] = None if native else res[1]
        partial = ["ok", str(ir.fingerprint()), ir.property_names(), [[k["names"], k["beg"], k["end"], k["reason"]] for k in rep["skipped"]],
                   rep["fallback_source"]]
    except (script.ScriptError, VmdError, ValueError) as e:
        partial = ["error", str(e)]
    return dict(strict=strict, partial=partial), info


def digest(out):
    return hashlib.sha256(json.dumps(out, sort_keys=True, ensure_ascii=True).encode()).hexdigest()[:16]
