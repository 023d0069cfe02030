"""Mini front-end for the subset of the VIAMD script language the hot path needs.

Stands in for md_script_ir_compile_from_source (/root/reference/src/main.cpp:878) for scripts of the forms VIAMD itself
generates or ships as defaults (src/main.cpp:528, :2817-2858):

    s1 = resname("ALA")[2:8];
    r  = rdf(element('C'), element('H'), 10.0);
    v  = sdf(s1, element('H'), 10.0);
    d1 = distance(10, 30);          # 1-based atom indices (src/main.cpp:2817)
    d2 = distance_min(residue(3), water);

Selections: element('X') | type/name('X') | resname("X") | residue(a:b) | resid(a:b) | atom(a:b) | integer | all | water |
protein, combined with `and`, `or`, `not`, parentheses; `sel[a:b]` slices an array of structures (1-based, inclusive).
The output is a ScriptIR of property descriptors (vmd_ir_add_rdf/_sdf/_distance); nothing is evaluated here.

The twin of viamd_amd/csrc/vmd_script.cpp, cut into the same functions under the same names (with a leading underscore): _statement()
reads the left-hand side and calls one _*_statement function per statement form.  A new form is one such function here, its twin
there, and a generator method plus the form's refusals in tests/script_cases.py.
"""
import re

import numpy as np

from . import _lib as L
from .eval import ScriptIR, VmdError

WATER_RESNAMES = {"HOH", "WAT", "SOL", "TIP3", "TIP4", "SPC", "H2O"}
PROTEIN_RESNAMES = {"ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO",
                    "SER", "THR", "TRP", "TYR", "VAL"}


class ScriptError(ValueError):
    pass


class Topology:
    """What selections are resolved against: per-atom element / name / residue name / residue index (0-based, contiguous)."""

    def __init__(self, elements, resnames=None, residue_index=None, names=None, mass=None, residue_seq_id=None):
        self.elements = np.asarray(elements)
        n = self.elements.size
        # per atom: the residue sequence number the file carries (PDB resSeq, GRO residue number) - what resid() selects by;
        # None = unknown (resid() is then an error, never an alias of residue(); src/main.cpp:2843-2848 emits both forms)
        self.residue_seq_id = None if residue_seq_id is None else np.asarray(residue_seq_id, dtype=np.int64)
        self.resnames = np.asarray(resnames) if resnames is not None else np.array(["UNK"] * n)
        self.residue_index = np.asarray(residue_index, dtype=np.int64) if residue_index is not None else np.zeros(n, np.int64)
        self.names = np.asarray(names) if names is not None else self.elements
        self.mass = mass
        self.num_atoms = n
        self.num_residues = int(self.residue_index.max()) + 1 if n else 0
        # atom range of every residue (residues are contiguous runs of atoms)
        order = np.argsort(self.residue_index, kind="stable")
        self._res_atoms = np.split(order, np.cumsum(np.bincount(self.residue_index, minlength=self.num_residues))[:-1])

    def residue_atoms(self, r):
        return np.sort(self._res_atoms[r])

    def residue_name(self, r):
        return str(self.resnames[self._res_atoms[r][0]])


class Sel:
    """A selection value: a boolean atom mask plus, when it came from a per-residue construct, the list of structures."""

    def __init__(self, mask, structures=None):
        self.mask = mask
        self.structures = structures      # list of index arrays, or None

    def indices(self):
        return np.nonzero(self.mask)[0].astype(np.int32)


_TOKEN = re.compile(r"""\s*(?:(?P<num>\d+\.\d*(?:[eE][-+]?\d+)?|\.\d+|\d+)|(?P<str>'[^']*'|"[^"]*")|(?P<id>[A-Za-z_]\w*)|(?P<op>[=(),;:\[\]{}]))""")


def _tokenize(text, tolerant=False, spans=None):
    """tokens as (kind, text); `spans` (a list) receives the [beg, end) byte range of each.  tolerant: a character outside the subset
    becomes a one-character op token instead of an error (partial compilation)."""
    text = re.sub(r"#[^\n]*", lambda m: " " * len(m.group()), text)       # comments -> blanks: offsets stay those of the source
    pos, out = 0, []
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            if text[pos:].strip() == "":
                break
            bad = pos + len(text[pos:]) - len(text[pos:].lstrip())
            if not tolerant:
                raise ScriptError(f"unexpected character {text[bad]!r} at offset {pos}")
            out.append(("op", text[bad]))
            if spans is not None:
                spans.append((bad, bad + 1))
            pos = bad + 1
            continue
        pos = m.end()
        kind = m.lastgroup
        out.append((kind, m.group(kind)))
        if spans is not None:
            spans.append((m.start(kind), m.end(kind)))
    return out


class _Parser:
    def __init__(self, tokens, topo, env, ctx=None):
        # ctx: atom indices of the evaluation context (`... in residue(3)`): integer / atom() indices are then relative to it
        # (src/main.cpp:2836-2840: `distance(i, j) in residue(k)` uses indices local to the residue) and every mask is clipped to it
        self.t, self.i, self.topo, self.env, self.ctx = tokens, 0, topo, env, ctx
        self.ctx_mask = None
        if ctx is not None:
            self.ctx_mask = np.zeros(topo.num_atoms, bool)
            self.ctx_mask[ctx] = True

    def peek(self):
        return self.t[self.i] if self.i < len(self.t) else (None, None)

    def take(self, value=None, kind=None):
        k, v = self.peek()
        if k is None or (value is not None and v != value) or (kind is not None and k != kind):
            raise ScriptError(f"expected {value or kind}, found {v!r}")
        self.i += 1
        return v

    def accept(self, value):
        if self.peek()[1] == value:
            self.i += 1
            return True
        return False

    # range a[:b], 1-based inclusive -> python slice bounds (0-based, exclusive)
    def range_(self):
        a = int(self.take(kind="num"))
        b = a
        if self.accept(":"):
            b = int(self.take(kind="num"))
        if a < 1 or b < a:
            raise ScriptError(f"bad range {a}:{b} (script indices are 1-based)")
        return a - 1, b

    def sel_or(self):
        s = self.sel_and()
        while self.accept("or"):
            s = Sel(s.mask | self.sel_and().mask)
        return s

    def sel_and(self):
        s = self.sel_not()
        while self.accept("and"):
            r = self.sel_not()
            structs = None
            if s.structures is not None:      # per-structure intersection keeps the array shape
                structs = [st[r.mask[st]] for st in s.structures]
            s = Sel(s.mask & r.mask, structs)
        return s

    def sel_not(self):
        if self.accept("not"):
            return Sel(~self.sel_not().mask)
        return self.sel_postfix()

    def sel_postfix(self):
        s = self.sel_atom()
        while self.accept("["):
            a, b = self.range_()
            self.take("]")
            if s.structures is None:
                raise ScriptError("[a:b] applies to an array of structures (resname(...), residue(...))")
            if b > len(s.structures):
                raise ScriptError(f"slice [{a + 1}:{b}] exceeds the {len(s.structures)} structures of the selection")
            st = s.structures[a:b]
            mask = np.zeros(self.topo.num_atoms, bool)
            for x in st:
                mask[x] = True
            s = Sel(mask, st)
        return s

    def _residues(self, pred):
        topo = self.topo
        st = [topo.residue_atoms(r) for r in range(topo.num_residues) if pred(r)]
        mask = np.zeros(topo.num_atoms, bool)
        for x in st:
            mask[x] = True
        return Sel(mask, st)

    def _atom_range(self, a, b):
        topo = self.topo
        mask = np.zeros(topo.num_atoms, bool)
        if self.ctx is not None:
            if b > len(self.ctx):
                raise ScriptError(f"atom index {b} out of range (the context has {len(self.ctx)} atoms)")
            mask[self.ctx[a:b]] = True
        else:
            if b > topo.num_atoms:
                raise ScriptError(f"atom index {b} out of range (system has {topo.num_atoms} atoms)")
            mask[a:b] = True
        return mask

    def sel_atom(self):
        s = self._sel_atom()
        if self.ctx_mask is not None and self.peek()[1] != "[":
            structs = None if s.structures is None else [st[self.ctx_mask[st]] for st in s.structures]
            s = Sel(s.mask & self.ctx_mask, structs)
        return s

    def _sel_atom(self):
        k, v = self.peek()
        topo = self.topo
        if v == "(":
            self.take("(")
            s = self.sel_or()
            self.take(")")
            return s
        if k == "num":
            a, b = self.range_()
            return Sel(self._atom_range(a, b))
        if k != "id":
            raise ScriptError(f"unexpected token {v!r} in selection")
        self.i += 1
        if v in self.env and isinstance(self.env[v], Sel):
            return self.env[v]
        if v == "all":
            return Sel(np.ones(topo.num_atoms, bool))
        if v == "water":
            return self._residues(lambda r: topo.residue_name(r).upper() in WATER_RESNAMES)
        if v == "protein":
            return self._residues(lambda r: topo.residue_name(r).upper() in PROTEIN_RESNAMES)
        if v in ("element", "type", "name", "label", "resname"):
            self.take("(")
            names = [self.take(kind="str")[1:-1]]
            while self.accept(","):
                names.append(self.take(kind="str")[1:-1])
            self.take(")")
            if v == "resname":
                return self._residues(lambda r: topo.residue_name(r) in names)
            arr = topo.elements if v == "element" else topo.names
            return Sel(np.isin(arr, names))
        if v == "resid":
            self.take("(")
            a = int(self.take(kind="num"))
            b = a
            if self.accept(":"):
                b = int(self.take(kind="num"))
            self.take(")")
            if b < a:
                raise ScriptError(f"bad range {a}:{b}")
            if topo.residue_seq_id is None:
                raise ScriptError("resid(): the topology carries no residue sequence numbers (vmd_topology_t.residue_seq_id); "
                                  "use residue() for the 1-based residue index")
            seq = [int(topo.residue_seq_id[topo._res_atoms[r][0]]) for r in range(topo.num_residues)]
            s = self._residues(lambda r: a <= seq[r] <= b)
            if not s.structures:
                raise ScriptError(f"resid({a}:{b}) matches no residue")
            return s
        if v in ("residue", "atom"):
            self.take("(")
            a, b = self.range_()
            self.take(")")
            if v == "atom":
                return Sel(self._atom_range(a, b))
            if b > topo.num_residues:
                raise ScriptError(f"{v}({b}) out of range (system has {topo.num_residues} residues)")
            return self._residues(lambda r: a <= r < b)
        if self.peek()[1] == "(":
            raise ScriptError(f"unsupported function {v!r} (outside the rdf / sdf / distance path)")
        raise ScriptError(f"unknown identifier {v!r}")

    def number(self):
        return float(self.take(kind="num"))


_FUNCS = {"rdf", "sdf", "distance", "distance_min", "distance_max", "distance_pair"}
_DIST_KIND = {"distance": L.DIST_COM, "distance_min": L.DIST_MIN, "distance_max": L.DIST_MAX, "distance_pair": L.DIST_PAIR}
_GEOM_NARGS = {"angle": 3, "dihedral": 4}       # opt-in (angles=True)
FEATURE_ANGLES = 1                              # VMD_SCRIPT_FEATURE_ANGLES
FEATURE_SHAPE = 2                               # VMD_SCRIPT_FEATURE_SHAPE
FEATURE_RMSD = 4                                # VMD_SCRIPT_FEATURE_RMSD
FEATURE_WITHIN = 8                              # VMD_SCRIPT_FEATURE_WITHIN
FEATURE_SHELL_RDF = 16                          # VMD_SCRIPT_FEATURE_SHELL_RDF
FEATURE_SHELL_SDF = 32                          # VMD_SCRIPT_FEATURE_SHELL_SDF
FEATURE_SHELL_EXPR = 64                         # VMD_SCRIPT_FEATURE_SHELL_EXPR


def _feature_mask(angles, shape, rmsd, within, shell_rdf, shell_sdf, shell_expr):
    """the keyword switches of compile_script / compile_script_native as the `features` of vmd_ir_compile_from_source_ex"""
    switches = (angles, shape, rmsd, within, shell_rdf, shell_sdf, shell_expr)
    return sum(1 << k for k, on in enumerate(switches) if on)


def compile_script(text, topo, lib=None, partial=False, angles=False, shape=False, rmsd=False, within=False, shell_rdf=False,
                   shell_sdf=False, shell_expr=False):
    """Returns (ScriptIR, info) where info[name] = dict(kind=..., plus the resolved index arrays).

    partial=True (vmd_ir_compile_from_source_partial): statements outside the subset are reported instead of failing the script;
    returns (ScriptIR, info, report) with report = dict(skipped=[dict(names, beg, end, reason)], fallback_source=text with the compiled
    property statements blanked out).  VIAMD's default script (src/main.cpp:528) then yields d1, r, v and reports a1 and lin,plan,iso.

    angles=True (VMD_SCRIPT_FEATURE_ANGLES, opt-in): angle(sel, sel, sel) and dihedral(sel, sel, sel, sel), plain or `in <contexts>`,
    are compiled too (DESIGN S6b); the default script then yields d1, a1, r, v and reports lin,plan,iso only.

    shape=True (VMD_SCRIPT_FEATURE_SHAPE, opt-in): `{n0, n1, n2} = shape_weights(sel)`, plain or `in <contexts>`, defines three temporal
    properties, info[n] = dict(kind="shape_weights", component=0 | 1 | 2, sets=[one index array per context]); with both
    opt-ins the default script compiles whole: d1, a1, r, v, lin, plan, iso, nothing skipped.

    rmsd=True (VMD_SCRIPT_FEATURE_RMSD, opt-in): `name = rmsd(sel)`, plain or `in <contexts>`,
    info[name] = dict(kind="rmsd", sets=[one index array per context]).

    within=True (VMD_SCRIPT_FEATURE_WITHIN, opt-in): `name = count(<sel> and within(<r> | <a>:<b>, <sel>) [and <sel> ...])`:
    exactly one within() factor at the top level of the AND, everything else static;
    info[name] = dict(kind="within_count", target=idx, ref=idx, rmin=, rmax=).

    shell_rdf=True (VMD_SCRIPT_FEATURE_SHELL_RDF, opt-in): either selection argument of rdf() may be such an AND;
    info[name] = dict(kind="rdf", ref=idx, target=idx, rmin=, rmax=, ref_shell=, target_shell=), a shell being None (that side is its
    static list) or dict(ref=idx, rmin=, rmax=).

    shell_sdf=True (VMD_SCRIPT_FEATURE_SHELL_SDF, opt-in): the target argument of sdf() may be such an AND; within() in the
    structures argument is refused; info[name] = dict(kind="sdf", structures=, target=idx, cutoff=, target_shell=) with the shell as above.

    shell_expr=True (VMD_SCRIPT_FEATURE_SHELL_EXPR, opt-in): with within=True the argument of count(), with shell_sdf=True the target of
    sdf(), may hold several dynamic factors at the top level of its AND - within(...), not within(...), or a parenthesised and / or / not
    over within() terms only.  info[name] gains terms=[dict(ref=idx, rmin=, rmax=)] in order of first appearance and
    truth= (bit sum(h_i << i) set: a member); a count that does not reduce to one positive term has kind="within_count_expr"."""
    features = _feature_mask(angles, shape, rmsd, within, shell_rdf, shell_sdf, shell_expr)
    ir = ScriptIR(lib)
    env, info = {}, {}
    spans = []
    toks = _tokenize(text, tolerant=partial, spans=spans)
    p = _Parser(toks, topo, env)
    skipped = []
    fallback = list(text)
    blanked, skipped_toks = [], []      # compiled property statements [name, tok_first, tok_end, beg, end, kept]; token ranges of the skipped ones
    while p.peek()[0] is not None:
        if p.accept(";"):
            continue
        first = p.i
        last, depth = first, 0          # the statement's extent: up to the next ';' outside brackets (or the end of the text)
        while last < len(toks):
            v = toks[last][1] if toks[last][0] == "op" else None
            if v in ("(", "[", "{"):
                depth += 1
            elif v in (")", "]", "}"):
                depth -= 1
            elif v == ";" and depth <= 0:
                break
            last += 1
        s = _Statement(p, topo, env, ir, info, features)
        try:
            commit = _statement(s)
            if p.peek()[0] is not None and p.peek()[1] != ";":
                raise ScriptError(f"expected ;, found {p.peek()[1]!r}")
            commit()
            if p.peek()[0] is not None:
                p.take(";")
            if s.is_property and partial:
                e = spans[last][1] if last < len(toks) else spans[last - 1][1]
                for c in range(spans[first][0], min(e, len(fallback))):
                    if fallback[c] != "\n":
                        fallback[c] = " "
                blanked.append([s.name, first, last, spans[first][0], min(e, len(fallback)), False])
        except (ValueError, VmdError) as e:   # ScriptError, int() / float() on a malformed number, a descriptor the library refuses
            if not partial:
                raise
            send = spans[last - 1][1] if last > first else spans[first][1]
            skipped.append(dict(names=s.name or toks[first][1], beg=spans[first][0], end=send, reason=str(e)))
            skipped_toks.append((first, last))
            p.i = last + 1 if last < len(toks) else last
    if partial:
        _restore_mentioned(fallback, text, toks, blanked, skipped_toks)
        return ir, info, dict(skipped=skipped, fallback_source="".join(fallback))
    return ir, info


def _restore_mentioned(fallback, text, toks, blanked, skipped_toks):
    """a compiled property that a skipped statement uses stays in the fallback's text (the twin of restore_mentioned in vmd_script.cpp;
    ADVICE r05 #2)"""
    used = set()

    def collect(a, b):
        k = a
        for q in range(a, min(b, len(toks))):
            if toks[q][0] == "op" and toks[q][1] == "=":
                k = q + 1
                break
        used.update(toks[q][1] for q in range(k, min(b, len(toks))) if toks[q][0] == "id")

    for a, b in skipped_toks:
        collect(a, b)
    changed = True
    while changed:
        changed = False
        for item in blanked:
            if item[5] or not any(n in used for n in item[0].split(",")):      # (shape_weights: three names joined by ',')
                continue
            item[5] = changed = True
            fallback[item[3]:item[4]] = text[item[3]:item[4]]
            collect(item[1], item[2])


class _Statement:
    """What a statement function works on (the twin of struct Statement in vmd_script.cpp).  p stands behind the `(` of the call when a
    _*_statement function is entered; name: the left-hand side, one name or the names of a tuple joined by ','."""

    def __init__(self, p, topo, env, ir, info, features):
        self.p, self.topo, self.env, self.ir, self.info, self.features = p, topo, env, ir, info, features
        self.t, self.name, self.is_property = p.t, "", False

    def has(self, bit):
        return bool(self.features & bit)

    def is_within_at(self, q):
        return q + 1 < len(self.t) and self.t[q] == ("id", "within") and self.t[q + 1] == ("op", "(")


# ---- helpers the statement forms share (each the twin of the function of the same name in vmd_script.cpp) -------------------------------------

def _closing_paren(s):
    """the token behind the `)` that closes the call p stands in"""
    j, depth = s.p.i, 1
    while depth:
        if j >= len(s.t):
            raise ScriptError(f"{s.name}: missing ')'")
        depth += {"(": 1, ")": -1}.get(s.t[j][1], 0) if s.t[j][0] == "op" else 0
        j += 1
    return j


def _per_context(s, after, body):
    """`f(<arguments>) [in <contexts>]`, after = _closing_paren(): body(parser, where) reads the arguments and the `)` - once with the
    statement's parser (where = ""), or, under `in`, once per structure of the contexts with a parser bound to it (where = " inside a
    context").  Returns the number of contexts, 0 without `in`."""
    if not (after < len(s.t) and s.t[after] == ("id", "in")):
        body(s.p, "")
        return 0
    start = s.p.i
    q = _Parser(s.t, s.topo, s.env)
    q.i = after + 1
    ctx = q.sel_or()
    if ctx.structures is None or not ctx.structures:
        raise ScriptError(f"{s.name}: `in` needs an array of structures (residue(...), resname(...))")
    for st in ctx.structures:
        r = _Parser(s.t, s.topo, s.env, ctx=np.asarray(st))
        r.i = start
        body(r, " inside a context")
    s.p.i = q.i
    return len(ctx.structures)


def _one_selection_population(s, fn):
    """`fn(sel) [in <contexts>]` (shape_weights, rmsd): one selection, one index set per context"""
    sets = []

    def one_set(r, where):
        ix = r.sel_or().indices()
        if r.peek() == ("op", ","):
            raise ScriptError(f"{s.name}: {fn} takes one selection")
        r.take(")")
        if ix.size == 0:
            raise ScriptError(f"{s.name}: empty selection{where}")
        sets.append(ix)

    _per_context(s, _closing_paren(s), one_set)
    return sets


def _within_head(s):
    """`within(` r | a:b `,` - p stands on `within`; the reference selection follows.  -> (rmin, rmax)"""
    p = s.p
    p.i += 1
    p.take("(")
    rmin, rmax = 0.0, p.number()
    if p.accept(":"):
        rmin, rmax = rmax, p.number()
        if not rmin < rmax:
            raise ScriptError(f"{s.name}: within range needs 0 <= a < b")
    elif not rmax > 0.0:
        raise ScriptError(f"{s.name}: within needs a radius > 0")
    p.take(",")
    return float(np.float32(rmin)), float(np.float32(rmax))


def _within_ref(s):
    """... and the reference selection with the `)`"""
    ref = s.p.sel_or().indices()
    s.p.take(")")
    if ref.size == 0:
        raise ScriptError(f"{s.name}: empty selection")
    return ref


def _scan_arg(s, start, stop_and=False, end=None):
    """One pass over an argument from token `start` -> (where it ends, how many within( it holds, how many of those are factors of its
    top-level AND, whether it has an `or` at depth 0).  end=None: the argument ends at the `,` `;` or unmatched `)` (with stop_and also
    at an `and`) at depth 0; otherwise the scan runs to `end` whatever is on the way (count(): the whole call)."""
    n_within = n_top = depth = 0
    top_or = False
    q = start
    while q < (len(s.t) if end is None else end):
        k, v = s.t[q]
        if end is None and depth == 0 and k == "op" and v in (",", ";"):
            break
        if (k, v) == ("op", "("):
            depth += 1
        if (k, v) == ("op", ")"):
            if depth == 0:
                break
            depth -= 1
        if stop_and and depth == 0 and (k, v) == ("id", "and"):
            break
        if s.is_within_at(q):
            n_within += 1
            if depth == 0 and (q == start or s.t[q - 1] == ("id", "and")):
                n_top += 1
        if (k, v) == ("id", "or") and depth == 0:
            top_or = True
        q += 1
    return q, n_within, n_top, top_or


def _single_within_and(s, scan, what):
    """`<factor> and ... and within(<r> | <a>:<b>, <static selection>) and ...`: exactly one within() factor, at the
    top level of the AND; the other factors are static and their AND is the list.  what: who takes it, for the message.
    -> (index list, dict(ref=, rmin=, rmax=))"""
    p = s.p
    _, n_within, n_top, top_or = scan
    if n_within > 1:
        raise ScriptError(f"{s.name}: {what} takes exactly one within() factor, found {n_within}")
    if n_top != 1 or top_or:
        raise ScriptError(f"{s.name}: within() must be a factor of the top-level AND (not under not / or / parentheses)")
    tmask = np.ones(s.topo.num_atoms, bool)
    shell = None
    while True:
        if p.peek() == ("id", "within"):
            rmin, rmax = _within_head(s)
            shell = dict(ref=_within_ref(s), rmin=rmin, rmax=rmax)
        else:
            tmask = tmask & p.sel_not().mask
        if not p.accept("and"):
            break
    return np.nonzero(tmask)[0].astype(np.int32), shell


def _selection_arg(s, dynamic, what):
    """a selection argument of rdf() / the target of sdf(): static, or with `dynamic` (the function's feature bit) possibly a single-within
    AND -> (index list, shell or None)"""
    scan = _scan_arg(s, s.p.i) if dynamic else None
    if scan is not None and scan[1]:
        return _single_within_and(s, scan, what)
    return s.p.sel_or().indices(), None


_EXPR_VAR = (0xAAAA, 0xCCCC, 0xF0F0, 0xFF00)


class _ExprParser:
    """the argument of count() / the target of sdf() under shell_expr=True (the twin of ExprParser in vmd_script.cpp): an AND of static
    factors and dynamic ones - within(...), not within(...), or a parenthesised and / or / not over within() terms only"""

    def __init__(self, s):
        self.s, self.p, self.terms = s, s.p, []

    def parse(self):
        """-> (index list, terms, truth), terms None for a static argument"""
        s, p = self.s, self.p
        _, has_within, _, top_or = _scan_arg(s, p.i)
        if not has_within:
            return p.sel_or().indices(), None, 0
        if top_or:
            raise ScriptError(f"{s.name}: a dynamic factor under a top-level or with a static selection")
        tmask = np.ones(s.topo.num_atoms, bool)
        table = 0xffff
        while True:
            if _scan_arg(s, p.i, stop_and=True)[1]:
                table &= self.dyn_not()
            else:
                tmask = tmask & p.sel_not().mask
            if not p.accept("and"):
                break
        return np.nonzero(tmask)[0].astype(np.int32), self.terms, table & ((1 << (1 << len(self.terms))) - 1)

    def within_term(self):
        s, terms = self.s, self.terms
        rmin, rmax = _within_head(s)
        if _scan_arg(s, self.p.i)[1]:
            raise ScriptError(f"{s.name}: within() nested in a within() argument")
        t = dict(ref=_within_ref(s), rmin=rmin, rmax=rmax)
        for k, u in enumerate(terms):
            if np.array_equal(u["ref"], t["ref"]) and u["rmin"] == t["rmin"] and u["rmax"] == t["rmax"]:
                return _EXPR_VAR[k]
        if len(terms) == L.SHELL_EXPR_MAX_TERMS:
            raise ScriptError(f"{s.name}: more than four distinct within() terms")
        terms.append(t)
        return _EXPR_VAR[len(terms) - 1]

    def dyn_not(self):
        p = self.p
        if p.accept("not"):
            return ~self.dyn_not() & 0xffff
        if self.s.is_within_at(p.i):
            return self.within_term()
        if p.peek() == ("op", "("):
            p.take("(")
            t = self.dyn_or()
            p.take(")")
            return t
        raise ScriptError(f"{self.s.name}: a static selection inside a parenthesised dynamic factor")

    def dyn_and(self):
        t = self.dyn_not()
        while self.p.accept("and"):
            t &= self.dyn_not()
        return t

    def dyn_or(self):
        t = self.dyn_and()
        while self.p.accept("or"):
            t |= self.dyn_and()
        return t


def _shell_tuple(sh):
    return sh and (sh["ref"], sh["rmin"], sh["rmax"])


def _rdf_range(p):
    """rdf's third argument: `{a, b}` | `r` | `a:b` -> (rmin, rmax)"""
    if p.accept("{"):
        rmin = p.number(); p.take(","); rmax = p.number(); p.take("}")
        return rmin, rmax
    rmin, rmax = 0.0, p.number()
    if p.accept(":"):
        rmin, rmax = rmax, p.number()
    return rmin, rmax


# ---- one function per statement form: each parses up to (not including) the ';' and returns the statement's commit.  Nothing is added
# to the IR, to info or to the identifiers before commit() runs, so a statement that fails half way leaves nothing behind ------------------

def _shape_statement(s):
    """`{n0, n1, n2} = shape_weights(sel) [in <contexts>]` from the function name on"""
    nm = s.name.split(",")
    if len(nm) != 3:
        raise ScriptError(f"{s.name}: shape_weights defines three properties, {{linear, planar, isotropic}}, not {len(nm)}")
    s.p.i += 1
    s.p.take("(")
    sets = _one_selection_population(s, "shape_weights")

    def commit():
        s.ir.add_shape_weights_population(nm, sets)
        for k, n in enumerate(nm):
            s.info[n] = dict(kind="shape_weights", component=k, sets=sets)
    return commit


def _rmsd_statement(s):
    """`name = rmsd(sel) [in <contexts>]`"""
    sets = _one_selection_population(s, "rmsd")

    def commit():
        s.ir.add_rmsd_population(s.name, sets)
        s.info[s.name] = dict(kind="rmsd", sets=sets)
    return commit


def _no_count_contexts(s):
    s.p.take(")")
    if s.p.peek() == ("id", "in"):
        raise ScriptError(f"{s.name}: count(...) in <contexts> is outside the subset")


def _count_statement(s):
    """`name = count(<factor> and ...)` with exactly one within() factor.  The scan covers the whole call, commas included:
    a second argument is met by the parse, not by the scan."""
    scan = _scan_arg(s, s.p.i, end=_closing_paren(s) - 1)
    if scan[1] == 0:
        raise ScriptError(f"{s.name}: count of a static selection is a constant (left to the fallback)")
    tgt, sh = _single_within_and(s, scan, "count")
    _no_count_contexts(s)
    if tgt.size == 0:
        raise ScriptError(f"{s.name}: empty selection")

    def commit():
        s.ir.add_within_count(s.name, tgt, sh["ref"], sh["rmin"], sh["rmax"])
        s.info[s.name] = dict(kind="within_count", target=tgt, **sh)
    return commit


def _count_expr_statement(s):
    """the same with any number of dynamic factors"""
    tgt, terms, truth = _ExprParser(s).parse()
    if terms is None:
        raise ScriptError(f"{s.name}: count of a static selection is a constant (left to the fallback)")
    _no_count_contexts(s)
    if tgt.size == 0:
        raise ScriptError(f"{s.name}: empty selection")

    def commit():
        s.ir.add_within_count_expr(s.name, tgt, [_shell_tuple(t) for t in terms], truth)
        if len(terms) == 1 and truth == 2:
            s.info[s.name] = dict(kind="within_count", target=tgt, **terms[0], terms=terms, truth=truth)
        else:
            s.info[s.name] = dict(kind="within_count_expr", target=tgt, terms=terms, truth=truth)
    return commit


def _rdf_statement(s):
    """`name = rdf(sel, sel, <range>)` - with shell_rdf=True either selection may be a single-within AND"""
    p, shells = s.p, s.has(FEATURE_SHELL_RDF)
    a, sha = _selection_arg(s, shells, "an rdf argument"); p.take(",")
    b, shb = _selection_arg(s, shells, "an rdf argument"); p.take(",")
    rmin, rmax = _rdf_range(p)
    p.take(")")
    if a.size == 0 or b.size == 0:
        raise ScriptError(f"{s.name}: empty selection")

    def commit():
        shells = {}
        if sha is None and shb is None:
            s.ir.add_rdf(s.name, a, b, (rmin, rmax))
        else:
            s.ir.add_rdf_shell(s.name, a, b, (rmin, rmax), ref_shell=_shell_tuple(sha), target_shell=_shell_tuple(shb))
            shells = dict(ref_shell=sha, target_shell=shb)
        s.info[s.name] = dict(kind="rdf", ref=a, target=b, rmin=rmin, rmax=rmax, **shells)
    return commit


def _sdf_statement(s):
    """`name = sdf(structures, sel, cutoff)` - with shell_sdf=True the target may be a single-within AND, with shell_expr=True
    on top of it an expression over within() terms.  The structures stay static: the alignment needs fixed atoms."""
    p, shells = s.p, s.has(FEATURE_SHELL_SDF)
    if shells and _scan_arg(s, p.i)[1]:
        raise ScriptError(f"{s.name}: within() in the structures argument of sdf() is not supported (the alignment needs fixed atoms)")
    ref = p.sel_or(); p.take(",")
    terms, truth = None, 0
    if shells and s.has(FEATURE_SHELL_EXPR):
        tg, terms, truth = _ExprParser(s).parse()
        sh = terms[0] if terms is not None and len(terms) == 1 and truth == 2 else None
    else:
        tg, sh = _selection_arg(s, shells, "an sdf argument")
    p.take(",")
    cutoff = p.number()
    p.take(")")
    structs = ref.structures if ref.structures is not None else [ref.indices()]
    sizes = {len(x) for x in structs}
    if len(sizes) != 1 or 0 in sizes:
        raise ScriptError(f"{s.name}: sdf reference structures must be non-empty and of equal size, got sizes {sorted(sizes)}")
    st = np.stack([np.asarray(x, np.int32) for x in structs])
    if (sh is not None or terms is not None) and tg.size == 0:
        raise ScriptError(f"{s.name}: empty selection")

    def commit():
        dynamic = {}
        if terms is not None:
            s.ir.add_sdf_shell_expr(s.name, st, tg, cutoff, [_shell_tuple(t) for t in terms], truth)
            dynamic = dict(terms=terms, truth=truth)
        elif sh is None:
            s.ir.add_sdf(s.name, st, tg, cutoff)
        else:
            s.ir.add_sdf_shell(s.name, st, tg, cutoff, target_shell=_shell_tuple(sh))
        if sh is not None:
            dynamic["target_shell"] = sh
        s.info[s.name] = dict(kind="sdf", structures=st, target=tg, cutoff=cutoff, **dynamic)
    return commit


def _geometry_statement(s, fn):
    """`name = distance*(a, b) | angle(a, b, c) | dihedral(a, b, c, d) [in <contexts>]` (DESIGN S6b): fn is the function's name"""
    nargs = _GEOM_NARGS.get(fn, 2)
    sets = [[] for _ in range(nargs)]

    def one_context(r, where):
        idx = []
        for n in range(nargs):
            if n:
                r.take(",")
            idx.append(r.sel_or().indices())
        r.take(")")
        if where and any(x.size == 0 for x in idx):
            raise ScriptError(f"{s.name}: empty selection{where}")
        for n in range(nargs):
            sets[n].append(idx[n])

    populations = _per_context(s, _closing_paren(s), one_context)
    ir, name = s.ir, s.name

    def commit():
        if populations and nargs > 2:
            (ir.add_angle_population if nargs == 3 else ir.add_dihedral_population)(name, *sets)
            s.info[name] = dict(kind=fn, sets=sets)
        elif populations:
            ir.add_distance_population(name, sets[0], sets[1], _DIST_KIND[fn])
            s.info[name] = dict(kind=fn, a_sets=sets[0], b_sets=sets[1])
        elif nargs > 2:
            idx = [x[0] for x in sets]
            (ir.add_angle if nargs == 3 else ir.add_dihedral)(name, *idx)
            s.info[name] = dict(kind=fn, sets=idx)
        else:
            ir.add_distance(name, sets[0][0], sets[1][0], _DIST_KIND[fn])
            s.info[name] = dict(kind=fn, a=sets[0][0], b=sets[1][0])
    return commit


def _statement(s):
    """One statement from its first token up to (not including) its ';' (the twin of statement() in vmd_script.cpp): the left-hand side
    into s.name, then the form's function.  Returns the statement's commit."""
    p = s.p
    if p.peek() == ("op", "{"):
        p.take("{")
        s.name = p.take(kind="id")
        while p.accept(","):
            s.name += "," + p.take(kind="id")
        p.take("}")
        p.take("=")
        k, v = p.peek()
        if s.has(FEATURE_RMSD) and k == "id" and v == "rmsd":
            raise ScriptError(f"{s.name}: rmsd defines one property, not a tuple")
        if not (s.has(FEATURE_SHAPE) and k == "id" and v == "shape_weights"):
            raise ScriptError(f"unsupported {'function' if k == 'id' else 'expression'} {v!r} (outside the rdf / sdf / distance path)")
        s.is_property = True
        return _shape_statement(s)
    name = s.name = p.take(kind="id")
    p.take("=")
    k, v = p.peek()
    if s.has(FEATURE_SHAPE) and (k, v) == ("id", "shape_weights"):
        raise ScriptError(f"{name}: shape_weights defines three properties, {{linear, planar, isotropic}}, not 1")
    if not (k == "id" and (v in _FUNCS or (s.has(FEATURE_ANGLES) and v in _GEOM_NARGS) or (s.has(FEATURE_RMSD) and v == "rmsd") or
                           (s.has(FEATURE_WITHIN) and v == "count"))):
        sel = p.sel_or()
        return lambda: s.env.__setitem__(name, sel)
    s.is_property = True
    p.i += 1
    p.take("(")
    if v == "rdf":
        return _rdf_statement(s)
    if v == "sdf":
        return _sdf_statement(s)
    if v == "rmsd":
        return _rmsd_statement(s)
    if v == "count":
        return _count_expr_statement(s) if s.has(FEATURE_SHELL_EXPR) else _count_statement(s)
    return _geometry_statement(s, v)


def compile_script_native(text, topo, lib=None, partial=False, angles=False, shape=False, rmsd=False, within=False, shell_rdf=False,
                          shell_sdf=False, shell_expr=False):
    """The same front-end in C++ (vmd_ir_compile_from_source, viamd_amd/csrc/vmd_script.cpp): what a C / C++ host calls.
    Returns a ScriptIR; raises ScriptError with the library's message.  angles=True: vmd_ir_compile_from_source_ex with
    VMD_SCRIPT_FEATURE_ANGLES; shape=True: with VMD_SCRIPT_FEATURE_SHAPE; rmsd=True: with VMD_SCRIPT_FEATURE_RMSD; within=True: with
    VMD_SCRIPT_FEATURE_WITHIN; shell_rdf=True: with VMD_SCRIPT_FEATURE_SHELL_RDF; shell_sdf=True: with VMD_SCRIPT_FEATURE_SHELL_SDF;
    shell_expr=True: with VMD_SCRIPT_FEATURE_SHELL_EXPR."""
    import ctypes as C
    ir = ScriptIR(lib)
    n = topo.num_atoms
    features = _feature_mask(angles, shape, rmsd, within, shell_rdf, shell_sdf, shell_expr)

    def strings(arr):
        return (C.c_char_p * n)(*[str(v).encode() for v in arr])

    el, nm, rn = strings(topo.elements), strings(topo.names), strings(topo.resnames)
    ri = np.ascontiguousarray(topo.residue_index, np.int32)
    sq = None if topo.residue_seq_id is None else np.ascontiguousarray(topo.residue_seq_id, np.int32)
    tc = L.TopologyC(n, el, nm, rn, ri.ctypes.data_as(L.c_int32_p), sq.ctypes.data_as(L.c_int32_p) if sq is not None else None)
    if not partial:
        ok = (ir.lib.vmd_ir_compile_from_source_ex(ir.h, text.encode(), C.byref(tc), features, None) if features
              else ir.lib.vmd_ir_compile_from_source(ir.h, text.encode(), C.byref(tc)))
        if not ok:
            raise ScriptError(ir.lib.last_error())
        return ir
    rep = C.c_void_p()
    ok = (ir.lib.vmd_ir_compile_from_source_ex(ir.h, text.encode(), C.byref(tc), features, C.byref(rep)) if features
          else ir.lib.vmd_ir_compile_from_source_partial(ir.h, text.encode(), C.byref(tc), C.byref(rep)))
    if not ok:
        raise ScriptError(ir.lib.last_error())
    try:
        n = ir.lib.vmd_script_report_skipped_count(rep)
        items = ir.lib.vmd_script_report_skipped(rep)
        skipped = [dict(names=items[k].names.decode(), beg=items[k].beg, end=items[k].end, reason=items[k].reason.decode()) for k in range(n)]
        report = dict(skipped=skipped, fallback_source=ir.lib.vmd_script_report_fallback_source(rep).decode())
    finally:
        ir.lib.vmd_script_report_free(rep)
    return ir, report


def backbone_from_topology(topo):
    """A backbone from a topology, for hosts without mdlib's protein_backbone (DECISION D-BB-TOPOLOGY; the twin of
    vmd_topology_backbone).  Names only - no coordinates, no bond test: a segment is a residue that owns atoms named "N", "CA" and "C"
    (the first of each), a range a maximal run of such residues with consecutive residue_index; class: resname GLY -> 1, PRO -> 2, else
    successor in the same range is PRO -> 3, else 0.  Returns dict(n, ca, c: int32 [nseg]; range_offsets: uint32 [num_ranges + 1];
    rama_class: uint8 [nseg]) - the arguments of ScriptIR.add_ramachandran."""
    seg_res, n, ca, c, offsets = [], [], [], [], []
    for r in range(topo.num_residues):
        at = {}
        for i in topo.residue_atoms(r):
            nm = str(topo.names[i])
            if nm in ("N", "CA", "C") and nm not in at:
                at[nm] = int(i)
        if len(at) != 3:
            continue
        if not seg_res or seg_res[-1] + 1 != r:
            offsets.append(len(seg_res))
        seg_res.append(r)
        n.append(at["N"]); ca.append(at["CA"]); c.append(at["C"])
    offsets.append(len(seg_res))
    cls = np.zeros(len(seg_res), np.uint8)
    for s, r in enumerate(seg_res):
        rn = topo.residue_name(r).upper()
        next_pro = s + 1 < len(seg_res) and seg_res[s + 1] == r + 1 and topo.residue_name(seg_res[s + 1]).upper() == "PRO"
        cls[s] = 1 if rn == "GLY" else 2 if rn == "PRO" else 3 if next_pro else 0
    return dict(n=np.array(n, np.int32), ca=np.array(ca, np.int32), c=np.array(c, np.int32),
                range_offsets=np.array(offsets, np.uint32), rama_class=cls)


def backbone_oxygens_from_topology(topo, bb):
    """The carbonyl oxygen of every segment of the backbone `bb` (the dict of backbone_from_topology), for
    ScriptIR.add_secondary_structure (DECISION D-SS-TOPOLOGY-O; the twin of vmd_topology_backbone_oxygens): the first atom of
    the CA's residue named "O", failing that "OT1", then "O1", then "OC1", else -1.  Returns int32 [nseg]."""
    o = np.full(len(bb["ca"]), -1, np.int32)
    for s, ca in enumerate(bb["ca"]):
        atoms = topo.residue_atoms(int(topo.residue_index[int(ca)]))
        for want in ("O", "OT1", "O1", "OC1"):
            hit = [int(i) for i in atoms if str(topo.names[i]) == want]
            if hit:
                o[s] = hit[0]
                break
    return o


def hbond_sites_from_topology(topo, bonds):
    """Hydrogen-bond sites for ScriptIR.add_hbonds (DECISION D-HB-TOPOLOGY; the twin of vmd_topology_hbond_sites): a donor
    pair for every bond between an atom of element H and an atom of element N or O, the acceptors every atom of element N, O or F.  Both
    lists in ascending atom order; elements only, no coordinates.  bonds: [nbonds, 2] atom indices.
    Returns dict(donor, hydrogen, acceptor) of int32 arrays."""
    el = [str(e).upper() for e in topo.elements]
    pairs = set()
    for i, j in np.asarray(bonds, np.int64).reshape(-1, 2):
        for h, d in ((int(i), int(j)), (int(j), int(i))):
            if el[h] == "H" and el[d] in ("N", "O"):
                pairs.add((d, h))
    pairs = sorted(pairs)
    return dict(donor=np.array([p[0] for p in pairs], np.int32), hydrogen=np.array([p[1] for p in pairs], np.int32),
                acceptor=np.array([i for i, e in enumerate(el) if e in ("N", "O", "F")], np.int32))


VDW_RADII = {"H": 1.20, "C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80, "CL": 1.75, "BR": 1.85, "I": 1.98}


def vdw_radii_from_topology(topo):
    """Van der Waals radii for ScriptIR.add_sasa (DECISION D-SASA-RADII; the twin of vmd_topology_vdw_radii): Bondi's values by
    element without regard to case, 2.00 for anything else.  -> float32 [num_atoms]"""
    return np.array([VDW_RADII.get(str(e).upper(), 2.00) for e in topo.elements], np.float32)


def vdw_radii_from_topology_native(topo, lib=None):
    """The same through the C ABI (vmd_topology_vdw_radii).  Raises ScriptError with the library's message."""
    import ctypes as C
    lib = lib or L.default_lib()
    n = topo.num_atoms
    el = (C.c_char_p * max(n, 1))(*[str(v).encode() for v in topo.elements])
    tc = L.TopologyC(n, el, None, None, None, None)
    out = np.zeros(max(n, 1), np.float32)
    if lib.vmd_topology_vdw_radii(C.byref(tc), out.ctypes.data_as(L.c_float_p), n) != n:
        raise ScriptError(lib.last_error())
    return out[:n].copy()


def contact_sites_from_topology(topo, heavy_only=True):
    """Contact sites for ScriptIR.add_contacts (DECISION D-CT-TOPOLOGY; the twin of vmd_topology_contact_sites): an entry
    for every atom - heavy_only: for every atom whose element is not H, whatever its case - in ascending atom order; its group is the
    atom's residue_index renumbered densely in order of first appearance.  A topology without residue_index is one group.
    The same sites serve ScriptIR.add_clusters: every group has an entry, and a water residue is a molecule.
    Returns dict(atoms, groups int32 arrays, ngroups)."""
    el = [str(e).upper() for e in topo.elements]
    ri = getattr(topo, "residue_index", None)
    atoms, groups, dense = [], [], {}
    for i in range(topo.num_atoms):
        if heavy_only and el[i] == "H":
            continue
        atoms.append(i)
        groups.append(dense.setdefault(int(ri[i]) if ri is not None else 0, len(dense)))
    return dict(atoms=np.array(atoms, np.int32), groups=np.array(groups, np.int32), ngroups=len(dense))


def contact_sites_from_topology_native(topo, heavy_only=True, lib=None):
    """The same through the C ABI (vmd_topology_contact_sites).  Raises ScriptError with the library's message."""
    import ctypes as C
    lib = lib or L.default_lib()
    n = topo.num_atoms
    el = (C.c_char_p * max(n, 1))(*[str(v).encode() for v in topo.elements])
    ri = getattr(topo, "residue_index", None)
    ri = None if ri is None else np.ascontiguousarray(ri, np.int32)
    tc = L.TopologyC(n, el, None, None, ri.ctypes.data_as(L.c_int32_p) if ri is not None else None, None)
    h = lib.vmd_topology_contact_sites(C.byref(tc), bool(heavy_only))
    if not h:
        raise ScriptError(lib.last_error())
    try:
        v = lib.vmd_contact_sites_view(h).contents

        def arr(ptr, count):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(np.int32).copy() if count else np.zeros(0, np.int32)

        return dict(atoms=arr(v.atom, int(v.nentries)), groups=arr(v.group, int(v.nentries)), ngroups=int(v.ngroups))
    finally:
        lib.vmd_contact_sites_free(h)


def sasa_points(npoints, lib=None):
    """The unit vectors the sasa kernels read (vmd_sasa_points, D-SASA-POINTS) -> float32 [npoints, 3]"""
    lib = lib or L.default_lib()
    out = np.zeros((max(int(npoints), 1), 3), np.float32)
    n = lib.vmd_sasa_points(int(npoints), out.ctypes.data_as(L.c_float_p), out.shape[0])
    if n == 0:
        raise ScriptError(lib.last_error())
    return out[:n].copy()


def hbond_sites_from_topology_native(topo, bonds, lib=None):
    """The same through the C ABI (vmd_topology_hbond_sites).  Raises ScriptError with the library's message."""
    import ctypes as C
    lib = lib or L.default_lib()
    n = topo.num_atoms
    el = (C.c_char_p * max(n, 1))(*[str(v).encode() for v in topo.elements])
    tc = L.TopologyC(n, el, None, None, None, None)
    b = np.ascontiguousarray(bonds, np.int32).reshape(-1, 2)
    h = lib.vmd_topology_hbond_sites(C.byref(tc), b.ctypes.data_as(L.c_int32_p) if b.size else None, b.shape[0])
    if not h:
        raise ScriptError(lib.last_error())
    try:
        v = lib.vmd_hbond_sites_view(h).contents

        def arr(ptr, count):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(np.int32).copy() if count else np.zeros(0, np.int32)

        return dict(donor=arr(v.donor, int(v.npairs)), hydrogen=arr(v.hydrogen, int(v.npairs)), acceptor=arr(v.acceptor, int(v.nacc)))
    finally:
        lib.vmd_hbond_sites_free(h)


def backbone_oxygens_from_topology_native(topo, bb, lib=None):
    """The same through the C ABI (vmd_topology_backbone_oxygens).  Raises ScriptError with the library's message."""
    import ctypes as C
    lib = lib or L.default_lib()
    n = topo.num_atoms

    def strings(arr):
        return (C.c_char_p * max(n, 1))(*[str(v).encode() for v in arr])

    el, nm, rn = strings(topo.elements), strings(topo.names), strings(topo.resnames)
    ri = np.ascontiguousarray(topo.residue_index, np.int32)
    tc = L.TopologyC(n, el, nm, rn, ri.ctypes.data_as(L.c_int32_p), None)
    n_, a_, c_ = (np.ascontiguousarray(bb[k], np.int32) for k in ("n", "ca", "c"))
    off = np.ascontiguousarray(bb["range_offsets"], np.uint32)
    bc = L.BackboneC(a_.size, n_.ctypes.data_as(L.c_int32_p), a_.ctypes.data_as(L.c_int32_p), c_.ctypes.data_as(L.c_int32_p),
                     max(off.size, 1) - 1, off.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    o = np.full(a_.size, -1, np.int32)
    got = lib.vmd_topology_backbone_oxygens(C.byref(tc), C.byref(bc), o.ctypes.data_as(L.c_int32_p), o.size)
    if got != a_.size:
        raise ScriptError(lib.last_error())
    return o


def backbone_from_topology_native(topo, lib=None):
    """The same through the C ABI (vmd_topology_backbone): what a C / C++ host calls.  Raises ScriptError with the library's message."""
    import ctypes as C
    lib = lib or L.default_lib()
    n = topo.num_atoms

    def strings(arr):
        return (C.c_char_p * max(n, 1))(*[str(v).encode() for v in arr])

    el, nm, rn = strings(topo.elements), strings(topo.names), strings(topo.resnames)
    ri = np.ascontiguousarray(topo.residue_index, np.int32)
    tc = L.TopologyC(n, el, nm, rn, ri.ctypes.data_as(L.c_int32_p), None)
    h = lib.vmd_topology_backbone(C.byref(tc))
    if not h:
        raise ScriptError(lib.last_error())
    try:
        v = lib.vmd_backbone_view(h).contents
        ns, nr = int(v.num_segments), int(v.num_ranges)

        def arr(ptr, count, dtype):
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype).copy() if count else np.zeros(0, dtype)

        return dict(n=arr(v.n, ns, np.int32), ca=arr(v.ca, ns, np.int32), c=arr(v.c, ns, np.int32),
                    range_offsets=arr(v.range_offsets, nr + 1, np.uint32), rama_class=arr(v.rama_class, ns, np.uint8))
    finally:
        lib.vmd_backbone_free(h)
