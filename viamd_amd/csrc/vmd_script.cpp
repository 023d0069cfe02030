// Mini script front-end in C++: md_script_ir_compile_from_source stand-in (/root/reference/src/main.cpp:878) for
// the subset of the VIAMD script language the hot path needs - the forms VIAMD ships as defaults or generates itself
// (src/main.cpp:528, :2817-2858):
//
//     s1 = resname("ALA")[2:8];
//     r  = rdf(element('C'), element('H'), 10.0);            # also rdf(a, b, {rmin, rmax}) and rdf(a, b, rmin:rmax)
//     v  = sdf(s1, element('H'), 10.0);
//     d1 = distance(10, 30);                                  # 1-based atom indices (src/main.cpp:2817)
//     d2 = distance_min(1:3, element('O')) in residue(2:9);   # one value per context, indices local to the context
//
// Selections: element('X') | type/name/label('X') | resname("X") | residue(a:b) | resid(a:b) | atom(a:b) | integer [: integer] |
// all | water | protein | identifiers bound earlier, combined with `and`, `or`, `not`, parentheses; `sel[a:b]` slices an array of
// structures (1-based, inclusive).  Output: property descriptors appended to a vmd_script_ir_t (vmd_ir_add_*); nothing is
// evaluated here.  viamd_amd/script.py is the same front-end in Python, cut into the same functions under the same names;
// tests/test_script.py checks that both produce identical IR fingerprints, tests/test_script_pin.py holds each to its recorded outcomes.
//
// A new statement form is one *_statement function here, called from statement(), its twin in script.py, and a generator method plus
// the form's refusals in tests/script_cases.py.  What the forms share - closing_paren, per_context, one_selection_population,
// within_head, scan_arg, single_within_and, rdf_range - is written once, above them.
#include <algorithm>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "vmd_eval.h"

extern "C" void vmd_set_last_error(const char* msg);

namespace {

struct ScriptError : std::runtime_error { using std::runtime_error::runtime_error; };

[[noreturn]] void fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw ScriptError(buf);
}

enum TokKind { T_END, T_NUM, T_STR, T_ID, T_OP };
struct Token { TokKind kind; std::string text; size_t beg = 0, end = 0; };     // [beg, end): byte range in the source

// tolerant: a character outside the subset becomes a one-character T_OP token instead of an error (partial compilation: the statement
// it belongs to is then reported as skipped, the others still compile)
std::vector<Token> tokenize(const char* src, bool tolerant = false) {
    std::string text(src);
    // strip comments
    for (size_t i = 0; i < text.size(); ++i)
        if (text[i] == '#') { size_t j = i; while (j < text.size() && text[j] != '\n') text[j++] = ' '; }
    std::vector<Token> out;
    size_t p = 0;
    const size_t n = text.size();
    while (p < n) {
        if (isspace((unsigned char)text[p])) { ++p; continue; }
        const char c = text[p];
        if (isdigit((unsigned char)c) || (c == '.' && p + 1 < n && isdigit((unsigned char)text[p + 1]))) {
            size_t q = p;
            while (q < n && isdigit((unsigned char)text[q])) ++q;
            if (q < n && text[q] == '.') {
                ++q;
                while (q < n && isdigit((unsigned char)text[q])) ++q;
                if (q < n && (text[q] == 'e' || text[q] == 'E')) {
                    size_t r = q + 1;
                    if (r < n && (text[r] == '+' || text[r] == '-')) ++r;
                    if (r < n && isdigit((unsigned char)text[r])) { while (r < n && isdigit((unsigned char)text[r])) ++r; q = r; }
                }
            }
            out.push_back({T_NUM, text.substr(p, q - p), p, q});
            p = q;
        } else if (c == '\'' || c == '"') {
            const size_t q = text.find(c, p + 1);
            if (q == std::string::npos) {
                if (!tolerant) fail("unexpected character '%c' at offset %zu", c, p);
                out.push_back({T_OP, std::string(1, c), p, p + 1});
                ++p;
                continue;
            }
            out.push_back({T_STR, text.substr(p + 1, q - p - 1), p, q + 1});
            p = q + 1;
        } else if (isalpha((unsigned char)c) || c == '_') {
            size_t q = p;
            while (q < n && (isalnum((unsigned char)text[q]) || text[q] == '_')) ++q;
            out.push_back({T_ID, text.substr(p, q - p), p, q});
            p = q;
        } else if (strchr("=(),;:[]{}", c) || tolerant) {
            out.push_back({T_OP, std::string(1, c), p, p + 1});
            ++p;
        } else {
            fail("unexpected character '%c' at offset %zu", c, p);
        }
    }
    return out;
}

struct Topo {
    size_t n = 0, nres = 0;
    std::vector<std::string> elements, names, resnames;
    std::vector<std::vector<int32_t>> res_atoms;     // ascending atom indices per residue
    std::vector<int32_t> res_seq;                    // residue sequence number of the file per residue (resid()); empty = unknown

    explicit Topo(const vmd_topology_t* t) {
        n = t->num_atoms;
        elements.resize(n); names.resize(n); resnames.resize(n);
        std::vector<int32_t> ri(n, 0);
        for (size_t i = 0; i < n; ++i) {
            elements[i] = t->elements && t->elements[i] ? t->elements[i] : "";
            names[i] = t->names && t->names[i] ? t->names[i] : elements[i];
            resnames[i] = t->resnames && t->resnames[i] ? t->resnames[i] : "UNK";
            ri[i] = t->residue_index ? t->residue_index[i] : 0;
            if (ri[i] < 0) fail("topology: negative residue index at atom %zu", i);
            nres = std::max(nres, (size_t)ri[i] + 1);
        }
        if (n == 0) nres = 0;
        res_atoms.resize(nres);
        for (size_t i = 0; i < n; ++i) res_atoms[ri[i]].push_back((int32_t)i);
        if (t->residue_seq_id) {
            res_seq.assign(nres, 0);
            for (size_t r = 0; r < nres; ++r) if (!res_atoms[r].empty()) res_seq[r] = t->residue_seq_id[res_atoms[r][0]];
        }
    }
    const std::string& residue_name(size_t r) const { static const std::string unk = "UNK"; return res_atoms[r].empty() ? unk : resnames[res_atoms[r][0]]; }
};

std::string upper(std::string s) { for (auto& c : s) c = (char)toupper((unsigned char)c); return s; }
const std::set<std::string> WATER = {"HOH", "WAT", "SOL", "TIP3", "TIP4", "SPC", "H2O"};
const std::set<std::string> PROTEIN = {"ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE",
                                       "PRO", "SER", "THR", "TRP", "TYR", "VAL"};

struct Sel {
    std::vector<uint8_t> mask;
    bool has_structs = false;
    std::vector<std::vector<int32_t>> structs;
    std::vector<int32_t> indices() const {
        std::vector<int32_t> out;
        for (size_t i = 0; i < mask.size(); ++i) if (mask[i]) out.push_back((int32_t)i);
        return out;
    }
};

struct Parser {
    const std::vector<Token>& t;
    size_t i = 0;
    const Topo& topo;
    const std::map<std::string, Sel>& env;
    const std::vector<int32_t>* ctx;          // atoms of the evaluation context (`... in residue(3)`), or null
    std::vector<uint8_t> ctx_mask;

    Parser(const std::vector<Token>& toks, const Topo& tp, const std::map<std::string, Sel>& e, const std::vector<int32_t>* c = nullptr)
        : t(toks), topo(tp), env(e), ctx(c) {
        if (ctx) { ctx_mask.assign(topo.n, 0); for (int32_t a : *ctx) ctx_mask[a] = 1; }
    }
    const Token& peek() const { static const Token end{T_END, ""}; return i < t.size() ? t[i] : end; }
    bool is_word(const char* w) const { const Token& k = peek(); return (k.kind == T_ID || k.kind == T_OP) && k.text == w; }
    std::string take(const char* value, TokKind kind = T_END) {
        const Token& k = peek();
        if (k.kind == T_END || (value && k.text != value) || (kind != T_END && k.kind != kind))
            fail("expected %s, found '%s'", value ? value : (kind == T_NUM ? "num" : kind == T_STR ? "str" : "id"), k.text.c_str());
        ++i;
        return k.text;
    }
    bool accept(const char* value) { if (is_word(value)) { ++i; return true; } return false; }

    long integer() {
        const std::string s = take(nullptr, T_NUM);
        for (char c : s) if (!isdigit((unsigned char)c)) fail("expected an integer, found '%s'", s.c_str());
        return strtol(s.c_str(), nullptr, 10);
    }
    // range a[:b], 1-based inclusive -> 0-based [a, b)
    void range(long& a, long& b) {
        a = integer(); b = a;
        if (accept(":")) b = integer();
        if (a < 1 || b < a) fail("bad range %ld:%ld (script indices are 1-based)", a, b);
        a -= 1;
    }
    double number() { return strtod(take(nullptr, T_NUM).c_str(), nullptr); }

    Sel sel_or() {
        Sel s = sel_and();
        while (accept("or")) {
            const Sel r = sel_and();
            Sel o; o.mask.resize(topo.n);
            for (size_t k = 0; k < topo.n; ++k) o.mask[k] = s.mask[k] | r.mask[k];
            s = o;
        }
        return s;
    }
    Sel sel_and() {
        Sel s = sel_not();
        while (accept("and")) {
            const Sel r = sel_not();
            Sel o; o.mask.resize(topo.n);
            for (size_t k = 0; k < topo.n; ++k) o.mask[k] = s.mask[k] & r.mask[k];
            if (s.has_structs) {      // per-structure intersection keeps the array shape
                o.has_structs = true;
                for (auto& st : s.structs) { std::vector<int32_t> f; for (int32_t a : st) if (r.mask[a]) f.push_back(a); o.structs.push_back(f); }
            }
            s = o;
        }
        return s;
    }
    Sel sel_not() {
        if (accept("not")) {
            const Sel r = sel_not();
            Sel o; o.mask.resize(topo.n);
            for (size_t k = 0; k < topo.n; ++k) o.mask[k] = !r.mask[k];
            return o;
        }
        return sel_postfix();
    }
    Sel from_structs(const std::vector<std::vector<int32_t>>& st) {
        Sel s; s.mask.assign(topo.n, 0); s.has_structs = true; s.structs = st;
        for (auto& x : st) for (int32_t a : x) s.mask[a] = 1;
        return s;
    }
    Sel sel_postfix() {
        Sel s = sel_atom();
        while (accept("[")) {
            long a, b;
            range(a, b);
            take("]");
            if (!s.has_structs) fail("[a:b] applies to an array of structures (resname(...), residue(...))");
            if ((size_t)b > s.structs.size()) fail("slice [%ld:%ld] exceeds the %zu structures of the selection", a + 1, b, s.structs.size());
            s = from_structs(std::vector<std::vector<int32_t>>(s.structs.begin() + a, s.structs.begin() + b));
        }
        return s;
    }
    template <class Pred> Sel residues(Pred pred) {
        std::vector<std::vector<int32_t>> st;
        for (size_t r = 0; r < topo.nres; ++r) if (pred(r)) st.push_back(topo.res_atoms[r]);
        return from_structs(st);
    }
    Sel atom_range(long a, long b) {
        Sel s; s.mask.assign(topo.n, 0);
        if (ctx) {
            if ((size_t)b > ctx->size()) fail("atom index %ld out of range (the context has %zu atoms)", b, ctx->size());
            for (long k = a; k < b; ++k) s.mask[(*ctx)[k]] = 1;
        } else {
            if ((size_t)b > topo.n) fail("atom index %ld out of range (system has %zu atoms)", b, topo.n);
            for (long k = a; k < b; ++k) s.mask[k] = 1;
        }
        return s;
    }
    Sel sel_atom() {
        Sel s = sel_atom_raw();
        if (ctx && !is_word("[")) {
            for (size_t k = 0; k < topo.n; ++k) s.mask[k] &= ctx_mask[k];
            if (s.has_structs) for (auto& st : s.structs) { std::vector<int32_t> f; for (int32_t a : st) if (ctx_mask[a]) f.push_back(a); st = f; }
        }
        return s;
    }
    Sel sel_atom_raw() {
        const Token k = peek();
        if (k.kind == T_OP && k.text == "(") {
            take("(");
            Sel s = sel_or();
            take(")");
            return s;
        }
        if (k.kind == T_NUM) {
            long a, b;
            range(a, b);
            return atom_range(a, b);
        }
        if (k.kind != T_ID) fail("unexpected token '%s' in selection", k.text.c_str());
        ++i;
        const std::string& v = k.text;
        auto it = env.find(v);
        if (it != env.end()) return it->second;
        if (v == "all") { Sel s; s.mask.assign(topo.n, 1); return s; }
        if (v == "water") return residues([&](size_t r) { return WATER.count(upper(topo.residue_name(r))) != 0; });
        if (v == "protein") return residues([&](size_t r) { return PROTEIN.count(upper(topo.residue_name(r))) != 0; });
        if (v == "element" || v == "type" || v == "name" || v == "label" || v == "resname") {
            take("(");
            std::vector<std::string> names{take(nullptr, T_STR)};
            while (accept(",")) names.push_back(take(nullptr, T_STR));
            take(")");
            auto in_names = [&](const std::string& x) { return std::find(names.begin(), names.end(), x) != names.end(); };
            if (v == "resname") return residues([&](size_t r) { return in_names(topo.residue_name(r)); });
            const std::vector<std::string>& arr = v == "element" ? topo.elements : topo.names;
            Sel s; s.mask.resize(topo.n);
            for (size_t a = 0; a < topo.n; ++a) s.mask[a] = in_names(arr[a]);
            return s;
        }
        if (v == "resid") {
            // the residue sequence number of the file (PDB resSeq: may start anywhere and restart per chain), NOT the residue index:
            // VIAMD emits both forms side by side (src/main.cpp:2843-2848)
            take("(");
            const long a = integer();
            long b = a;
            if (accept(":")) b = integer();
            take(")");
            if (b < a) fail("bad range %ld:%ld", a, b);
            if (topo.res_seq.empty()) fail("resid(): the topology carries no residue sequence numbers (vmd_topology_t.residue_seq_id); use residue() for the 1-based residue index");
            Sel s = residues([&](size_t r) { return (long)topo.res_seq[r] >= a && (long)topo.res_seq[r] <= b; });
            if (s.structs.empty()) fail("resid(%ld:%ld) matches no residue", a, b);
            return s;
        }
        if (v == "residue" || v == "atom") {
            take("(");
            long a, b;
            range(a, b);
            take(")");
            if (v == "atom") return atom_range(a, b);
            if ((size_t)b > topo.nres) fail("%s(%ld) out of range (system has %zu residues)", v.c_str(), b, topo.nres);
            return residues([&](size_t r) { return (size_t)a <= r && r < (size_t)b; });
        }
        if (is_word("(")) fail("unsupported function '%s' (outside the rdf / sdf / distance path)", v.c_str());
        fail("unknown identifier '%s'", v.c_str());
    }
};

vmd_distance_kind_t dist_kind(const std::string& f) {
    if (f == "distance") return VMD_DISTANCE_COM;
    if (f == "distance_min") return VMD_DISTANCE_MIN;
    if (f == "distance_max") return VMD_DISTANCE_MAX;
    return VMD_DISTANCE_PAIR;
}

struct Skipped { std::string names; size_t beg, end; std::string reason; };
struct Report {
    std::vector<Skipped> skipped;
    std::vector<vmd_script_skipped_t> view;
    std::string fallback_source;
};

using Commit = std::function<void()>;       // appends the statement's descriptor / binds its identifier; runs once the whole statement has parsed
using Indices = std::vector<int32_t>;

// What a statement function works on.  p stands behind the `(` of the call when a *_statement function is entered.
struct Statement {
    const std::vector<Token>& toks;
    const Topo& topo;
    std::map<std::string, Sel>& env;
    vmd_script_ir_t* ir;
    uint32_t features;
    Parser& p;
    std::string name;               // the left-hand side: one name, or the names of a tuple joined by ','
    bool is_property = false;

    bool has(uint32_t bit) const { return (features & bit) != 0; }
    const char* nm() const { return name.c_str(); }
    bool is(size_t q, TokKind kind, const char* text) const { return q < toks.size() && toks[q].kind == kind && toks[q].text == text; }
    bool is_within_at(size_t q) const { return is(q, T_ID, "within") && is(q + 1, T_OP, "("); }
};

void added(bool ok) { if (!ok) throw ScriptError(vmd_last_error()); }       // a descriptor the library refuses

// ---- helpers the statement forms share -------------------------------------------------------------------------------------------------

// the token behind the `)` that closes the call p stands in
size_t closing_paren(const Statement& s) {
    size_t j = s.p.i;
    for (int depth = 1; depth; ++j) {
        if (j >= s.toks.size()) fail("%s: missing ')'", s.nm());
        if (s.is(j, T_OP, "(")) depth += 1;
        if (s.is(j, T_OP, ")")) depth -= 1;
    }
    return j;
}

// `f(<arguments>) [in <contexts>]`, after = closing_paren(): body(parser, where) reads the arguments and the `)` - once with the
// statement's parser (where = ""), or, under `in`, once per structure of the contexts with a parser bound to it (where = " inside a
// context").  Returns the number of contexts, 0 without `in`.
template <class Body> size_t per_context(Statement& s, size_t after, Body body) {
    if (!s.is(after, T_ID, "in")) { body(s.p, ""); return 0; }
    const size_t start = s.p.i;
    Parser q(s.toks, s.topo, s.env);
    q.i = after + 1;
    const Sel ctx = q.sel_or();
    if (!ctx.has_structs || ctx.structs.empty()) fail("%s: `in` needs an array of structures (residue(...), resname(...))", s.nm());
    for (auto& st : ctx.structs) {
        Parser r(s.toks, s.topo, s.env, &st);
        r.i = start;
        body(r, " inside a context");
    }
    s.p.i = q.i;
    return ctx.structs.size();
}

// index sets back to back: set k is all[off[k] .. off[k + 1])
struct Population {
    Indices all, off{0};
    void push(const Indices& ix) { all.insert(all.end(), ix.begin(), ix.end()); off.push_back((int32_t)all.size()); }
};

// `fn(sel) [in <contexts>]` (shape_weights, rmsd): one selection, one set per context
Population one_selection_population(Statement& s, const char* fn) {
    Population out;
    per_context(s, closing_paren(s), [&](Parser& r, const char* where) {
        const Indices ix = r.sel_or().indices();
        if (r.is_word(",")) fail("%s: %s takes one selection", s.nm(), fn);
        r.take(")");
        if (ix.empty()) fail("%s: empty selection%s", s.nm(), where);
        out.push(ix);
    });
    return out;
}

// A selection argument that may hold within(): the static list and, when shell is set, the one shell that narrows it per frame.
struct DynArg { Indices list, ref; bool shell = false; double rmin = 0.0, rmax = 0.0; };

// `within(` r | a:b `,` - p stands on `within`; the reference selection follows
void within_head(Statement& s, double* rmin, double* rmax) {
    Parser& p = s.p;
    ++p.i;
    p.take("(");
    *rmin = 0.0;
    *rmax = p.number();
    if (p.accept(":")) {
        *rmin = *rmax; *rmax = p.number();
        if (!(*rmin < *rmax)) fail("%s: within range needs 0 <= a < b", s.nm());
    } else if (!(*rmax > 0.0)) fail("%s: within needs a radius > 0", s.nm());
    p.take(",");
}

// ... and the reference selection with the `)`
Indices within_ref(Statement& s) {
    Indices ref = s.p.sel_or().indices();
    s.p.take(")");
    if (ref.empty()) fail("%s: empty selection", s.nm());
    return ref;
}

// One pass over an argument from token `from`: where it ends, how many within( it holds, how many of those are factors of its top-level
// AND, whether it has an `or` at depth 0.  end == npos: the argument ends at the `,` `;` or unmatched `)` (with stop_and also at an
// `and`) at depth 0; otherwise the scan runs to `end` whatever is on the way (count(): the whole call).
struct ArgScan { size_t end = 0, n_within = 0, n_top = 0; bool top_or = false; };
const size_t npos = (size_t)-1;

ArgScan scan_arg(const Statement& s, size_t from, bool stop_and = false, size_t end = npos) {
    ArgScan out;
    int depth = 0;
    size_t q = from;
    for (; q < std::min(end, s.toks.size()); ++q) {
        if (end == npos && depth == 0 && (s.is(q, T_OP, ",") || s.is(q, T_OP, ";"))) break;
        if (s.is(q, T_OP, "(")) depth += 1;
        if (s.is(q, T_OP, ")")) { if (depth == 0) break; depth -= 1; }
        if (stop_and && depth == 0 && s.is(q, T_ID, "and")) break;
        if (s.is_within_at(q)) {
            out.n_within += 1;
            if (depth == 0 && (q == from || s.is(q - 1, T_ID, "and"))) out.n_top += 1;
        }
        if (depth == 0 && s.is(q, T_ID, "or")) out.top_or = true;
    }
    out.end = q;
    return out;
}

// `<factor> and ... and within(<r> | <a>:<b>, <static selection>) and ...`: exactly one within() factor, at the top
// level of the AND; the other factors are static and their AND is the list (all atoms when there is none).  what: who takes it, for
// the message.
DynArg single_within_and(Statement& s, const ArgScan& scan, const char* what) {
    Parser& p = s.p;
    if (scan.n_within > 1) fail("%s: %s takes exactly one within() factor, found %zu", s.nm(), what, scan.n_within);
    if (scan.n_top != 1 || scan.top_or) fail("%s: within() must be a factor of the top-level AND (not under not / or / parentheses)", s.nm());
    DynArg out;
    out.shell = true;
    std::vector<uint8_t> tmask(s.topo.n, 1);
    do {
        if (p.is_word("within") && p.peek().kind == T_ID) {
            within_head(s, &out.rmin, &out.rmax);
            out.ref = within_ref(s);
        } else {
            const Sel f = p.sel_not();
            for (size_t a = 0; a < s.topo.n; ++a) tmask[a] &= f.mask[a];
        }
    } while (p.accept("and"));
    for (size_t a = 0; a < s.topo.n; ++a) if (tmask[a]) out.list.push_back((int32_t)a);
    return out;
}

// a selection argument of rdf() / the target of sdf(): static, or with `dynamic` (the function's feature bit) possibly a single-within AND
DynArg selection_arg(Statement& s, bool dynamic, const char* what) {
    const ArgScan scan = dynamic ? scan_arg(s, s.p.i) : ArgScan();
    if (scan.n_within) return single_within_and(s, scan, what);
    DynArg out;
    out.list = s.p.sel_or().indices();
    return out;
}

// DESIGN 1.9 (VMD_SCRIPT_FEATURE_SHELL_EXPR): the argument of count() and the target of sdf() may hold several dynamic factors at the
// top level of their AND - within(...), not within(...), or a parenthesised and / or / not over within() terms only.  Terms that repeat
// are one term, numbered in order of first appearance; a table over four variables is carried through the parse and cut to the terms
// there are.
struct ExprTerm { Indices ref; float rmin, rmax; };
struct ExprArg { Indices list; std::vector<ExprTerm> terms; uint32_t truth = 0; bool dynamic = false; };

struct ExprParser {
    Statement& s;
    Parser& p;
    ExprArg out;
    explicit ExprParser(Statement& st) : s(st), p(st.p) {}

    ExprArg parse() {
        const ArgScan whole = scan_arg(s, p.i);
        if (!whole.n_within) { out.list = p.sel_or().indices(); return out; }
        if (whole.top_or) fail("%s: a dynamic factor under a top-level or with a static selection", s.nm());
        out.dynamic = true;
        std::vector<uint8_t> tmask(s.topo.n, 1);
        uint32_t table = 0xffffu;
        do {
            if (scan_arg(s, p.i, true).n_within) table &= dyn_not();
            else { const Sel f = p.sel_not(); for (size_t a = 0; a < s.topo.n; ++a) tmask[a] &= f.mask[a]; }
        } while (p.accept("and"));
        for (size_t a = 0; a < s.topo.n; ++a) if (tmask[a]) out.list.push_back((int32_t)a);
        out.truth = table & ((1u << (1u << out.terms.size())) - 1u);
        return out;
    }
    uint32_t within_term() {
        static const uint32_t VAR[4] = {0xAAAAu, 0xCCCCu, 0xF0F0u, 0xFF00u};
        double rmin, rmax;
        within_head(s, &rmin, &rmax);
        if (scan_arg(s, p.i).n_within) fail("%s: within() nested in a within() argument", s.nm());
        ExprTerm t{within_ref(s), (float)rmin, (float)rmax};
        for (size_t k = 0; k < out.terms.size(); ++k)
            if (out.terms[k].ref == t.ref && out.terms[k].rmin == t.rmin && out.terms[k].rmax == t.rmax) return VAR[k];
        if (out.terms.size() == VMD_SHELL_EXPR_MAX_TERMS) fail("%s: more than four distinct within() terms", s.nm());
        out.terms.push_back(std::move(t));
        return VAR[out.terms.size() - 1];
    }
    uint32_t dyn_not() {
        if (p.accept("not")) return ~dyn_not() & 0xffffu;
        if (s.is_within_at(p.i)) return within_term();
        if (p.is_word("(")) { p.take("("); const uint32_t t = dyn_or(); p.take(")"); return t; }
        fail("%s: a static selection inside a parenthesised dynamic factor", s.nm());
    }
    uint32_t dyn_and() { uint32_t t = dyn_not(); while (p.accept("and")) t &= dyn_not(); return t; }
    uint32_t dyn_or() { uint32_t t = dyn_and(); while (p.accept("or")) t |= dyn_and(); return t; }
};

vmd_shell_expr_t expr_view(const ExprArg& x, std::vector<vmd_shell_t>* terms) {
    terms->clear();
    for (auto& t : x.terms) terms->push_back(vmd_shell_t{t.ref.data(), t.ref.size(), t.rmin, t.rmax});
    return vmd_shell_expr_t{terms->data(), terms->size(), x.truth};
}

vmd_shell_t shell_view(const DynArg& a) { return vmd_shell_t{a.ref.data(), a.ref.size(), (float)a.rmin, (float)a.rmax}; }

// rdf's third argument: `{a, b}` | `r` | `a:b`
void rdf_range(Parser& p, double* rmin, double* rmax) {
    *rmin = 0.0;
    if (p.accept("{")) { *rmin = p.number(); p.take(","); *rmax = p.number(); p.take("}"); return; }
    *rmax = p.number();
    if (p.accept(":")) { *rmin = *rmax; *rmax = p.number(); }
}

// ---- one function per statement form: each parses up to (not including) the ';' and returns the statement's commit ------------------------

// `{lin, plan, iso} = shape_weights(sel) [in <contexts>];`, from the function's name on: the one function of the subset
// that defines a tuple
Commit shape_statement(Statement& s) {
    std::vector<std::string> nm(1);
    for (char ch : s.name) { if (ch == ',') nm.emplace_back(); else nm.back() += ch; }
    if (nm.size() != 3) fail("%s: shape_weights defines three properties, {linear, planar, isotropic}, not %zu", s.nm(), nm.size());
    ++s.p.i;
    s.p.take("(");
    const Population sets = one_selection_population(s, "shape_weights");
    return [ir = s.ir, nm, sets]() {
        const char* const cn[3] = {nm[0].c_str(), nm[1].c_str(), nm[2].c_str()};
        added(vmd_ir_add_shape_weights_population(ir, cn, sets.off.size() - 1, sets.all.data(), sets.off.data()));
    };
}

// `name = rmsd(sel) [in <contexts>];`: one selection, the selection and context rules of distance()
Commit rmsd_statement(Statement& s) {
    const Population sets = one_selection_population(s, "rmsd");
    return [ir = s.ir, name = s.name, sets]() { added(vmd_ir_add_rmsd_population(ir, name.c_str(), sets.off.size() - 1, sets.all.data(), sets.off.data())); };
}

void no_count_contexts(Statement& s) {
    s.p.take(")");
    if (s.p.is_word("in")) fail("%s: count(...) in <contexts> is outside the subset", s.nm());
}

// `name = count(<factor> and <factor> ...);`: exactly one factor is within(<r> | <a>:<b>, <static selection>), the others
// are static selections whose AND is the target set.  The scan covers the whole call, commas included: a second argument is met by
// the parse, not by the scan.
Commit count_statement(Statement& s) {
    const ArgScan scan = scan_arg(s, s.p.i, false, closing_paren(s) - 1);
    if (scan.n_within == 0) fail("%s: count of a static selection is a constant (left to the fallback)", s.nm());
    const DynArg A = single_within_and(s, scan, "count");
    no_count_contexts(s);
    if (A.list.empty()) fail("%s: empty selection", s.nm());
    return [ir = s.ir, name = s.name, A]() {
        added(vmd_ir_add_within_count(ir, name.c_str(), A.list.data(), A.list.size(), A.ref.data(), A.ref.size(), (float)A.rmin, (float)A.rmax));
    };
}

// the same with any number of dynamic factors
Commit count_expr_statement(Statement& s) {
    const ExprArg X = ExprParser(s).parse();
    if (!X.dynamic) fail("%s: count of a static selection is a constant (left to the fallback)", s.nm());
    no_count_contexts(s);
    if (X.list.empty()) fail("%s: empty selection", s.nm());
    return [ir = s.ir, name = s.name, X]() {
        std::vector<vmd_shell_t> tv;
        const vmd_shell_expr_t xv = expr_view(X, &tv);
        added(vmd_ir_add_within_count_expr(ir, name.c_str(), X.list.data(), X.list.size(), &xv));
    };
}

// `name = rdf(sel, sel, <range>);` - with VMD_SCRIPT_FEATURE_SHELL_RDF either selection may be a single-within AND
Commit rdf_statement(Statement& s) {
    Parser& p = s.p;
    const bool shells = s.has(VMD_SCRIPT_FEATURE_SHELL_RDF);
    const DynArg A = selection_arg(s, shells, "an rdf argument"); p.take(",");
    const DynArg B = selection_arg(s, shells, "an rdf argument"); p.take(",");
    double rmin, rmax;
    rdf_range(p, &rmin, &rmax);
    p.take(")");
    if (A.list.empty() || B.list.empty()) fail("%s: empty selection", s.nm());
    if (!shells) return [ir = s.ir, name = s.name, A, B, rmin, rmax]() {
        added(vmd_ir_add_rdf(ir, name.c_str(), A.list.data(), A.list.size(), B.list.data(), B.list.size(), (float)rmin, (float)rmax));
    };
    return [ir = s.ir, name = s.name, A, B, rmin, rmax]() {
        const vmd_shell_t sa = shell_view(A), sb = shell_view(B);
        added(vmd_ir_add_rdf_shell(ir, name.c_str(), A.list.data(), A.list.size(), A.shell ? &sa : nullptr, B.list.data(), B.list.size(),
                                   B.shell ? &sb : nullptr, (float)rmin, (float)rmax));
    };
}

// `name = sdf(structures, sel, cutoff);` - with VMD_SCRIPT_FEATURE_SHELL_SDF the target may be a single-within AND, with
// VMD_SCRIPT_FEATURE_SHELL_EXPR on top of it an expression over within() terms.  The structures stay static: the alignment
// needs fixed atoms.
Commit sdf_statement(Statement& s) {
    Parser& p = s.p;
    const bool shells = s.has(VMD_SCRIPT_FEATURE_SHELL_SDF);
    if (shells && scan_arg(s, p.i).n_within)
        fail("%s: within() in the structures argument of sdf() is not supported (the alignment needs fixed atoms)", s.nm());
    const Sel ref = p.sel_or(); p.take(",");
    DynArg T;
    ExprArg X;
    if (shells && s.has(VMD_SCRIPT_FEATURE_SHELL_EXPR)) { X = ExprParser(s).parse(); T.list = X.list; }
    else T = selection_arg(s, shells, "an sdf argument");
    p.take(",");
    const double cutoff = p.number();
    p.take(")");
    const std::vector<Indices> structs = ref.has_structs ? ref.structs : std::vector<Indices>{ref.indices()};
    const size_t K = structs.size(), m = K ? structs[0].size() : 0;
    Indices flat;
    for (auto& st : structs) {
        if (st.size() != m) break;
        flat.insert(flat.end(), st.begin(), st.end());
    }
    if (m == 0 || flat.size() != K * m) fail("%s: sdf reference structures must be non-empty and of equal size", s.nm());
    if ((T.shell || X.dynamic) && T.list.empty()) fail("%s: empty selection", s.nm());
    if (X.dynamic) return [ir = s.ir, name = s.name, flat, K, m, X, cutoff]() {
        std::vector<vmd_shell_t> tv;
        const vmd_shell_expr_t xv = expr_view(X, &tv);
        added(vmd_ir_add_sdf_shell_expr(ir, name.c_str(), flat.data(), K, m, X.list.data(), X.list.size(), &xv, (float)cutoff));
    };
    return [ir = s.ir, name = s.name, flat, K, m, T, cutoff]() {
        const vmd_shell_t sh = shell_view(T);
        added(vmd_ir_add_sdf_shell(ir, name.c_str(), flat.data(), K, m, T.list.data(), T.list.size(), T.shell ? &sh : nullptr, (float)cutoff));
    };
}

// `name = distance*(a, b) | angle(a, b, c) | dihedral(a, b, c, d) [in <contexts>];` (DESIGN S6b): fn is the function's name
Commit geometry_statement(Statement& s, const std::string& fn) {
    const size_t nargs = fn == "angle" ? 3 : (fn == "dihedral" ? 4 : 2);
    std::vector<Population> sets(nargs);
    const size_t P = per_context(s, closing_paren(s), [&](Parser& r, const char* where) {
        std::vector<Indices> idx;
        for (size_t k = 0; k < nargs; ++k) { if (k) r.take(","); idx.push_back(r.sel_or().indices()); }
        r.take(")");
        if (*where) for (auto& ix : idx) if (ix.empty()) fail("%s: empty selection%s", s.nm(), where);
        for (size_t k = 0; k < nargs; ++k) sets[k].push(idx[k]);
    });
    const vmd_distance_kind_t kind = dist_kind(fn);
    if (P) return [ir = s.ir, name = s.name, sets, nargs, kind, P]() {          // one value per context
        const int32_t *a = sets[0].all.data(), *ao = sets[0].off.data(), *b = sets[1].all.data(), *bo = sets[1].off.data();
        if (nargs == 2) { added(vmd_ir_add_distance_population(ir, name.c_str(), kind, P, a, ao, b, bo)); return; }
        const int32_t *c = sets[2].all.data(), *co = sets[2].off.data();
        added(nargs == 3 ? vmd_ir_add_angle_population(ir, name.c_str(), P, a, ao, b, bo, c, co)
                         : vmd_ir_add_dihedral_population(ir, name.c_str(), P, a, ao, b, bo, c, co, sets[3].all.data(), sets[3].off.data()));
    };
    return [ir = s.ir, name = s.name, sets, nargs, kind]() {
        const Indices &a = sets[0].all, &b = sets[1].all;
        if (nargs == 2) { added(vmd_ir_add_distance(ir, name.c_str(), kind, a.data(), a.size(), b.data(), b.size())); return; }
        const Indices& c = sets[2].all;
        added(nargs == 3 ? vmd_ir_add_angle(ir, name.c_str(), a.data(), a.size(), b.data(), b.size(), c.data(), c.size())
                         : vmd_ir_add_dihedral(ir, name.c_str(), a.data(), a.size(), b.data(), b.size(), c.data(), c.size(), sets[3].all.data(),
                                               sets[3].all.size()));
    };
}

// One statement from its first token up to (not including) its ';': the left-hand side into s.name, then the form's function.
// features: VMD_SCRIPT_FEATURE_ANGLES also takes angle() / dihedral(), VMD_SCRIPT_FEATURE_SHAPE the tuple statement
// `{lin, plan, iso} = shape_weights(sel)`, VMD_SCRIPT_FEATURE_RMSD `name = rmsd(sel)`, VMD_SCRIPT_FEATURE_WITHIN
// `name = count(sel and within(r, sel))`, VMD_SCRIPT_FEATURE_SHELL_RDF the same AND as an argument of rdf(), VMD_SCRIPT_FEATURE_SHELL_SDF
// as the target argument of sdf(), VMD_SCRIPT_FEATURE_SHELL_EXPR expressions over within() in count() and sdf() (opt-in; 0 = the subset
// of the header, byte for byte)
Commit statement(Statement& s) {
    Parser& p = s.p;
    if (p.is_word("{")) {
        // tuple assignment `{a, b, c} = f(...)`: shape_weights, under its bit, or nothing
        p.take("{");
        s.name = p.take(nullptr, T_ID);
        while (p.accept(",")) s.name += "," + p.take(nullptr, T_ID);
        p.take("}");
        p.take("=");
        const Token& f = p.peek();
        if (s.has(VMD_SCRIPT_FEATURE_RMSD) && f.kind == T_ID && f.text == "rmsd") fail("%s: rmsd defines one property, not a tuple", s.nm());
        if (!(s.has(VMD_SCRIPT_FEATURE_SHAPE) && f.kind == T_ID && f.text == "shape_weights"))
            fail("unsupported %s '%s' (outside the rdf / sdf / distance path)", f.kind == T_ID ? "function" : "expression", f.text.c_str());
        s.is_property = true;
        return shape_statement(s);
    }
    s.name = p.take(nullptr, T_ID);
    p.take("=");
    const Token k = p.peek();
    const std::string& v = k.text;
    if (s.has(VMD_SCRIPT_FEATURE_SHAPE) && k.kind == T_ID && v == "shape_weights")
        fail("%s: shape_weights defines three properties, {linear, planar, isotropic}, not 1", s.nm());
    const bool is_func = k.kind == T_ID && (v == "rdf" || v == "sdf" || v == "distance" || v == "distance_min" || v == "distance_max" ||
                                            v == "distance_pair" || (s.has(VMD_SCRIPT_FEATURE_ANGLES) && (v == "angle" || v == "dihedral")) ||
                                            (s.has(VMD_SCRIPT_FEATURE_RMSD) && v == "rmsd") || (s.has(VMD_SCRIPT_FEATURE_WITHIN) && v == "count"));
    if (!is_func) {
        const Sel sel = p.sel_or();
        return [&env = s.env, name = s.name, sel]() { env[name] = sel; };
    }
    s.is_property = true;
    ++p.i;
    p.take("(");
    if (v == "rdf") return rdf_statement(s);
    if (v == "sdf") return sdf_statement(s);
    if (v == "rmsd") return rmsd_statement(s);
    if (v == "count") return s.has(VMD_SCRIPT_FEATURE_SHELL_EXPR) ? count_expr_statement(s) : count_statement(s);
    return geometry_statement(s, v);
}

// a compiled property that a SKIPPED statement uses (`d = distance(1,2); x = d * 2;`) must stay in the fallback's text, or
// mdlib cannot compile the reduced script.  Blanked statements {left-hand name, token range, byte range} and the token ranges of the
// skipped ones are recorded; after the pass every blanked statement whose name a kept statement mentions is restored, transitively
struct Blanked { std::string name; size_t tok_first, tok_end, beg, end; bool kept; };
using TokRange = std::pair<size_t, size_t>;

void restore_mentioned(std::string& fallback, const char* source, const std::vector<Token>& toks, std::vector<Blanked>& blanked,
                       const std::vector<TokRange>& skipped_toks) {
    std::set<std::string> used;
    // identifiers on the right-hand side of a statement (everything after its first `=`; the whole statement when it has none)
    auto collect = [&](size_t a, size_t b) {
        size_t k = a;
        for (size_t q = a; q < b && q < toks.size(); ++q) if (toks[q].kind == T_OP && toks[q].text == "=") { k = q + 1; break; }
        for (; k < b && k < toks.size(); ++k) if (toks[k].kind == T_ID) used.insert(toks[k].text);
    };
    for (const auto& r : skipped_toks) collect(r.first, r.second);
    for (bool changed = true; changed;) {
        changed = false;
        for (Blanked& b : blanked) {
            // (a shape_weights statement carries its three names joined by ',')
            bool mentioned = false;
            for (size_t n0 = 0; n0 <= b.name.size() && !mentioned;) {
                const size_t n1 = std::min(b.name.find(',', n0), b.name.size());
                mentioned = used.count(b.name.substr(n0, n1 - n0)) != 0;
                n0 = n1 + 1;
            }
            if (b.kept || !mentioned) continue;
            b.kept = changed = true;
            for (size_t c = b.beg; c < b.end; ++c) fallback[c] = source[c];        // the GPU still evaluates it; mdlib evaluates it too, for its users
            collect(b.tok_first, b.tok_end);
        }
    }
}

// One statement at a time.  A statement is parsed completely - up to its ';' - before its descriptor is appended, so a statement that
// fails leaves neither a property nor an identifier behind.  report == nullptr: the first error ends the compilation (the strict
// mode).  Otherwise the failing statement is recorded {left-hand names, source range, reason} and the next one is compiled: what a host
// hands to the evaluator it falls back on (include/vmd_md_script_shim.h), e.g. `a1 = angle(2,1,3) in resname("ALA");` and
// `{lin,plan,iso} = shape_weights(all);` of VIAMD's default script (src/main.cpp:528).  A later statement that uses an identifier of a
// skipped one is skipped with it ("unknown identifier").
void compile(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* t, Report* report, uint32_t features = 0) {
    const Topo topo(t);
    const std::vector<Token> toks = tokenize(source, report != nullptr);
    std::map<std::string, Sel> env;
    Parser p(toks, topo, env);
    std::string fallback(source);
    std::vector<Blanked> blanked;
    std::vector<TokRange> skipped_toks;
    while (p.peek().kind != T_END) {
        if (p.accept(";")) continue;
        const size_t first = p.i;
        // the statement's extent: up to the next ';' outside brackets (or the end of the text)
        size_t last = first;
        for (int depth = 0; last < toks.size(); ++last) {
            const Token& k = toks[last];
            if (k.kind != T_OP) continue;
            if (k.text == "(" || k.text == "[" || k.text == "{") depth += 1;
            else if (k.text == ")" || k.text == "]" || k.text == "}") depth -= 1;
            else if (k.text == ";" && depth <= 0) break;
        }
        Statement s{toks, topo, env, ir, features, p, ""};
        try {
            const Commit commit = statement(s);
            // the end of every statement: its ';', the descriptor, and in partial mode the statement's text taken out of the fallback's
            if (p.peek().kind != T_END && !p.is_word(";")) fail("expected ;, found '%s'", p.peek().text.c_str());
            commit();
            if (p.peek().kind != T_END) p.take(";");
            if (s.is_property && report) {
                // the fallback evaluates the text WITHOUT this statement: blanked in place, so that every other offset stays what the editor shows
                const size_t e = last < toks.size() ? toks[last].end : toks[last - 1].end;
                for (size_t c = toks[first].beg; c < e && c < fallback.size(); ++c) if (fallback[c] != '\n') fallback[c] = ' ';
                blanked.push_back(Blanked{s.name, first, last, toks[first].beg, std::min(e, fallback.size()), false});
            }
        } catch (const ScriptError& e) {
            if (!report) throw;
            const size_t send = last > first ? toks[last - 1].end : toks[first].end;
            report->skipped.push_back({s.name.empty() ? toks[first].text : s.name, toks[first].beg, send, e.what()});
            skipped_toks.emplace_back(first, last);
            p.i = last < toks.size() ? last + 1 : last;
        }
    }
    if (report) {
        restore_mentioned(fallback, source, toks, blanked, skipped_toks);
        report->fallback_source = fallback;
    }
}

}  // namespace

static bool compile_strict(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* topology, uint32_t features) {
    if (!ir || !source || !topology) { vmd_set_last_error("vmd_ir_compile_from_source: NULL argument"); return false; }
    try {
        compile(ir, source, topology, nullptr, features);
    } catch (const std::exception& e) {
        vmd_set_last_error(e.what());
        return false;
    }
    return true;
}

extern "C" bool vmd_ir_compile_from_source(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* topology) {
    return compile_strict(ir, source, topology, 0);
}

struct vmd_script_report_t { Report r; };

static bool compile_partial(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* topology, vmd_script_report_t** report,
                            uint32_t features) {
    if (report) *report = nullptr;
    if (!ir || !source || !topology || !report) { vmd_set_last_error("vmd_ir_compile_from_source_partial: NULL argument"); return false; }
    std::unique_ptr<vmd_script_report_t> rep(new vmd_script_report_t());
    try {
        compile(ir, source, topology, &rep->r, features);
    } catch (const std::exception& e) {          // the topology itself is malformed: nothing a fallback could take over
        vmd_set_last_error(e.what());
        return false;
    }
    for (const Skipped& k : rep->r.skipped) rep->r.view.push_back(vmd_script_skipped_t{k.names.c_str(), k.beg, k.end, k.reason.c_str()});
    *report = rep.release();
    return true;
}

extern "C" bool vmd_ir_compile_from_source_partial(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* topology, vmd_script_report_t** report) {
    return compile_partial(ir, source, topology, report, 0);
}

extern "C" bool vmd_ir_compile_from_source_ex(vmd_script_ir_t* ir, const char* source, const vmd_topology_t* topology, uint32_t features,
                                              vmd_script_report_t** report) {
    return report ? compile_partial(ir, source, topology, report, features) : compile_strict(ir, source, topology, features);
}
extern "C" size_t vmd_script_report_skipped_count(const vmd_script_report_t* r) { return r ? r->r.view.size() : 0; }
extern "C" const vmd_script_skipped_t* vmd_script_report_skipped(const vmd_script_report_t* r) { return r && !r->r.view.empty() ? r->r.view.data() : nullptr; }
extern "C" const char* vmd_script_report_fallback_source(const vmd_script_report_t* r) { return r ? r->r.fallback_source.c_str() : ""; }
extern "C" void vmd_script_report_free(vmd_script_report_t* r) { delete r; }

// ---- a backbone from a topology (DECISION D-BB-TOPOLOGY): for hosts without mdlib's protein_backbone.  Names only - no
// coordinates, no bond test: a segment is a residue that owns atoms named "N", "CA" and "C" (the first of each), a range a maximal run of
// such residues with consecutive residue_index.
struct vmd_backbone_owned_t {
    std::vector<int32_t> n, ca, c;
    std::vector<uint32_t> offsets;
    std::vector<uint8_t> cls;
    vmd_backbone_t view;
};

extern "C" vmd_backbone_owned_t* vmd_topology_backbone(const vmd_topology_t* topology) {
    if (!topology) { vmd_set_last_error("vmd_topology_backbone: topology is NULL"); return nullptr; }
    try {
        Topo topo(topology);
        auto bb = std::make_unique<vmd_backbone_owned_t>();
        std::vector<size_t> seg_res;
        for (size_t r = 0; r < topo.nres; ++r) {
            int32_t at[3] = {-1, -1, -1};
            static const char* const want[3] = {"N", "CA", "C"};
            for (int32_t i : topo.res_atoms[r])
                for (int k = 0; k < 3; ++k) if (at[k] < 0 && topo.names[i] == want[k]) at[k] = i;
            if (at[0] < 0 || at[1] < 0 || at[2] < 0) continue;
            if (seg_res.empty() || seg_res.back() + 1 != r) bb->offsets.push_back((uint32_t)seg_res.size());
            seg_res.push_back(r);
            bb->n.push_back(at[0]); bb->ca.push_back(at[1]); bb->c.push_back(at[2]);
        }
        const size_t nseg = seg_res.size();
        bb->offsets.push_back((uint32_t)nseg);
        bb->cls.assign(nseg, 0);
        for (size_t s = 0; s < nseg; ++s) {
            const std::string rn = upper(topo.residue_name(seg_res[s]));
            const bool next_pro = s + 1 < nseg && seg_res[s + 1] == seg_res[s] + 1 && upper(topo.residue_name(seg_res[s + 1])) == "PRO";
            bb->cls[s] = rn == "GLY" ? 1 : rn == "PRO" ? 2 : next_pro ? 3 : 0;
        }
        bb->view.num_segments = nseg;
        bb->view.n = bb->n.data(); bb->view.ca = bb->ca.data(); bb->view.c = bb->c.data();
        bb->view.num_ranges = bb->offsets.size() - 1;
        bb->view.range_offsets = bb->offsets.data();
        bb->view.rama_class = bb->cls.data();
        return bb.release();
    } catch (const std::exception& e) {
        vmd_set_last_error(e.what());
        return nullptr;
    }
}

// the carbonyl oxygen of every segment (DECISION D-SS-TOPOLOGY-O): by name, in the residue of the segment's CA
extern "C" size_t vmd_topology_backbone_oxygens(const vmd_topology_t* topology, const vmd_backbone_t* backbone, int32_t* out, size_t cap) {
    if (!topology || !backbone) { vmd_set_last_error("vmd_topology_backbone_oxygens: NULL argument"); return 0; }
    try {
        Topo topo(topology);
        static const char* const want[4] = {"O", "OT1", "O1", "OC1"};
        for (size_t s = 0; s < backbone->num_segments; ++s) {
            const int32_t ca = backbone->ca ? backbone->ca[s] : -1;
            if (ca < 0 || (size_t)ca >= topo.n) fail("backbone CA of segment %zu is atom %d (the topology has %zu atoms)", s, ca, topo.n);
            int32_t o = -1;
            const size_t r = topology->residue_index ? (size_t)topology->residue_index[ca] : 0;
            for (int k = 0; k < 4 && o < 0; ++k)
                for (int32_t i : topo.res_atoms[r]) if (topo.names[i] == want[k]) { o = i; break; }
            if (out && s < cap) out[s] = o;
        }
        return backbone->num_segments;
    } catch (const std::exception& e) {
        vmd_set_last_error(e.what());
        return 0;
    }
}

extern "C" const vmd_backbone_t* vmd_backbone_view(const vmd_backbone_owned_t* backbone) { return backbone ? &backbone->view : nullptr; }

extern "C" void vmd_backbone_free(vmd_backbone_owned_t* backbone) { delete backbone; }

// ---- hydrogen-bond sites from a topology and its bonds (DECISION D-HB-TOPOLOGY): elements only, no coordinates.  A donor pair
// for every bond between an H and an N or O, the acceptors every N, O or F; both in ascending atom order.
struct vmd_hbond_sites_owned_t {
    std::vector<int32_t> donor, hydrogen, acceptor;
    vmd_hbond_sites_t view;
};

extern "C" vmd_hbond_sites_owned_t* vmd_topology_hbond_sites(const vmd_topology_t* topology, const int32_t (*bonds)[2], size_t nbonds) {
    if (!topology) { vmd_set_last_error("vmd_topology_hbond_sites: topology is NULL"); return nullptr; }
    if (!bonds && nbonds) { vmd_set_last_error("vmd_topology_hbond_sites: bonds is NULL"); return nullptr; }
    try {
        const size_t n = topology->num_atoms;
        std::vector<std::string> el(n);
        for (size_t i = 0; i < n; ++i) el[i] = upper(topology->elements && topology->elements[i] ? topology->elements[i] : "");
        auto hs = std::make_unique<vmd_hbond_sites_owned_t>();
        std::vector<std::pair<int32_t, int32_t>> pairs;
        for (size_t b = 0; b < nbonds; ++b) {
            const int32_t i = bonds[b][0], j = bonds[b][1];
            if (i < 0 || j < 0 || (size_t)i >= n || (size_t)j >= n) fail("bond %zu names atoms %d and %d (the topology has %zu atoms)", b, i, j, n);
            for (int k = 0; k < 2; ++k) {
                const int32_t h = k ? j : i, d = k ? i : j;
                if (el[h] == "H" && (el[d] == "N" || el[d] == "O")) pairs.push_back({d, h});
            }
        }
        std::sort(pairs.begin(), pairs.end());
        pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());       // a bond listed twice is one pair
        for (auto& q : pairs) { hs->donor.push_back(q.first); hs->hydrogen.push_back(q.second); }
        for (size_t i = 0; i < n; ++i) if (el[i] == "N" || el[i] == "O" || el[i] == "F") hs->acceptor.push_back((int32_t)i);
        hs->view.npairs = hs->donor.size(); hs->view.donor = hs->donor.data(); hs->view.hydrogen = hs->hydrogen.data();
        hs->view.nacc = hs->acceptor.size(); hs->view.acceptor = hs->acceptor.data();
        return hs.release();
    } catch (const std::exception& e) {
        vmd_set_last_error(e.what());
        return nullptr;
    }
}

extern "C" const vmd_hbond_sites_t* vmd_hbond_sites_view(const vmd_hbond_sites_owned_t* sites) { return sites ? &sites->view : nullptr; }

extern "C" void vmd_hbond_sites_free(vmd_hbond_sites_owned_t* sites) { delete sites; }

// ---- contact sites from a topology (DECISION D-CT-TOPOLOGY): every atom, or every atom that is not a hydrogen, in ascending
// atom order; the group is the residue_index renumbered densely in order of first appearance.  No native list.
struct vmd_contact_sites_owned_t {
    std::vector<int32_t> atom, group;
    vmd_contact_sites_t view;
};

extern "C" vmd_contact_sites_owned_t* vmd_topology_contact_sites(const vmd_topology_t* topology, bool heavy_only) {
    if (!topology) { vmd_set_last_error("vmd_topology_contact_sites: topology is NULL"); return nullptr; }
    try {
        auto cs = std::make_unique<vmd_contact_sites_owned_t>();
        std::map<int32_t, int32_t> dense;
        for (size_t i = 0; i < topology->num_atoms; ++i) {
            if (heavy_only && upper(topology->elements && topology->elements[i] ? topology->elements[i] : "") == "H") continue;
            const int32_t r = topology->residue_index ? topology->residue_index[i] : 0;
            const auto it = dense.emplace(r, (int32_t)dense.size()).first;
            cs->atom.push_back((int32_t)i); cs->group.push_back(it->second);
        }
        cs->view.nentries = cs->atom.size(); cs->view.atom = cs->atom.data(); cs->view.group = cs->group.data();
        cs->view.ngroups = dense.size(); cs->view.nnative = 0; cs->view.native = nullptr;
        return cs.release();
    } catch (const std::exception& e) {
        vmd_set_last_error(e.what());
        return nullptr;
    }
}

extern "C" const vmd_contact_sites_t* vmd_contact_sites_view(const vmd_contact_sites_owned_t* sites) { return sites ? &sites->view : nullptr; }

extern "C" void vmd_contact_sites_free(vmd_contact_sites_owned_t* sites) { delete sites; }

// ---- van der Waals radii from a topology's elements (DECISION D-SASA-RADII): Bondi's values, 2.00 for anything else
extern "C" size_t vmd_topology_vdw_radii(const vmd_topology_t* topology, float* out, size_t cap) {
    if (!topology) { vmd_set_last_error("vmd_topology_vdw_radii: topology is NULL"); return 0; }
    static const struct { const char* el; float r; } kBondi[] = {{"H", 1.20f}, {"C", 1.70f}, {"N", 1.55f}, {"O", 1.52f}, {"F", 1.47f},
            {"P", 1.80f}, {"S", 1.80f}, {"CL", 1.75f}, {"BR", 1.85f}, {"I", 1.98f}};
    const size_t n = topology->num_atoms;
    for (size_t i = 0; out && i < n && i < cap; ++i) {
        const std::string el = upper(topology->elements && topology->elements[i] ? topology->elements[i] : "");
        float r = 2.00f;
        for (auto& b : kBondi) if (el == b.el) r = b.r;
        out[i] = r;
    }
    return n;
}
