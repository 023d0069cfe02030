// viamd_amd/csrc/vmd_eval_ir.cpp - the property descriptors behind vmd_ir_*: what md_script_ir_t carries for the hot-path properties
// (rdf / sdf / distance family, angle / dihedral, shape_weights; /root/reference/src/main.cpp:528, 2817-2858), their fingerprint and the work estimate a host compares
// with its threshold (include/vmd_md_script_shim.h).
#include "vmd_eval_internal.h"

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

extern "C" vmd_script_ir_t* vmd_ir_create(void) { return new vmd_script_ir_t(); }

static uint64_t sum_sizes(std::initializer_list<const std::vector<int32_t>*> sets) { uint64_t n = 0; for (auto* v : sets) n += v->size(); return n; }
static uint64_t expr_refs(const Property& p) { uint64_t n = 0; for (auto& t : p.expr_terms) n += t.ref.size(); return n; }

// atom pairs one frame of this script asks for (rdf: |ref| x |target|; sdf: K x |target| + K m for the alignment; distance: |a| x |b| of
// every context; angle / dihedral / shape_weights: the atoms of every context's sets): what a host compares with its threshold before it sends a SMALL script to the GPU at all (include/vmd_md_script_shim.h,
// vmd_shim_set_min_work; VIAMD's default dataset is ~1e2 atoms, src/main.cpp:522-528)
extern "C" uint64_t vmd_ir_work_per_frame(const vmd_script_ir_t* ir) {
    if (!ir) return 0;
    uint64_t w = 0;
    for (const Property& p : ir->props) {
        switch (p.form) {
        case Form::RDF:
            w += (uint64_t)p.a.size() * (uint64_t)p.b.size();
            // the parent sizes (a bound that needs no frame) plus one neighbour query per shell, |T| + |R|
            for (int k = 0; k < 2; ++k) if (p.shell[k].on) w += (uint64_t)(k ? p.b : p.a).size() + (uint64_t)p.shell[k].ref.size();
            break;
        case Form::SDF:
            w += (uint64_t)p.K * ((uint64_t)p.b.size() + (uint64_t)p.m);
            if (p.shell[1].on) w += (uint64_t)p.b.size() + (uint64_t)p.shell[1].ref.size();     // the parent list plus the shell's query
            if (p.is_expr_sdf()) w += (uint64_t)p.b.size() + expr_refs(p);                      // |T| + sum |R_i|
            break;
        case Form::DISTANCE:
            for (size_t c = 0; c + 1 < p.aoff.size(); ++c) w += (uint64_t)(p.aoff[c + 1] - p.aoff[c]) * (uint64_t)(p.boff[c + 1] - p.boff[c]);
            break;
        case Form::ANGLE: case Form::DIHEDRAL: w += sum_sizes({&p.a, &p.b, &p.c, &p.d}); break;     // each context: the sum of its set sizes
        case Form::SHAPE: if (p.shape_comp == 0) w += p.a.size(); break;     // one pass over every context's set per statement
        case Form::RMSD: w += p.a.size(); break;                             // the atoms of every context's set
        case Form::RMSF: w += 2 * (uint64_t)p.a.size(); break;               // twice, the sums and the second pass
        case Form::WITHIN: w += sum_sizes({&p.a, &p.b}); break;              // |T| + |R|: a neighbour query, not all pairs
        case Form::WITHIN_EXPR: w += p.a.size() + expr_refs(p); break;       // |T| + sum |R_i|
        case Form::RAMA_TABLE: w += 3 * (uint64_t)p.a.size(); break;         // N, CA, C of every segment
        case Form::RAMA_MAP: break;                                          // binned by its table's launch
        // the CA gate of every ordered pair of segments - 64 to a wave, an eighth of them reach an energy on a folded chain -
        // plus N, CA, C, O of every segment
        case Form::SS_CLASS: w += (uint64_t)p.a.size() * (uint64_t)p.a.size() / 8 + 4 * (uint64_t)p.a.size(); break;
        case Form::SS_POP: break;                                            // counted by its table's launch
        case Form::HBOND_COUNT: w += 2 * (uint64_t)p.a.size() + 2 * (uint64_t)p.b.size(); break;     // a neighbour query per pair (D, H), the acceptors sorted and identified
        case Form::HBOND_OCC: break;                                         // added to by its count's launch
        // a neighbour query per measured entry, npoints bits to keep per entry (in units of 32), the environment sorted and identified
        case Form::SASA_AREA: w += (uint64_t)p.a.size() * (1 + (p.sasa_npoints + 31) / 32) + 2 * (uint64_t)p.b.size(); break;
        case Form::SASA_OCC: break;                                          // added to by its area's launch
        case Form::CONTACT_COUNT: w += 4 * (uint64_t)p.a.size(); break;      // 1.14's rule for a list against itself - a query per entry, the list sorted and identified
        case Form::CONTACT_OCC: case Form::CONTACT_NATIVE: break;            // written by their count's launch
        case Form::CLUSTER_COUNT: w += 4 * (uint64_t)p.a.size(); break;      // 1.16's rule
        case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST: break;         // written by their count's launch
        case Form::MSD_TABLE: w += p.a.size(); break;                        // one gather per atom
        }
    }
    return w;
}

extern "C" void vmd_ir_free(vmd_script_ir_t* ir) { delete ir; }

bool ir_name_ok(vmd_script_ir_t* ir, const char* name) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!name || !*name) return vmd_fail("property name is empty");
    for (auto& p : ir->props) if (p.name == name) return vmd_fail("property '%s' already defined", name);
    return true;
}

bool idx_ok(const int32_t* idx, size_t n, const char* what) {
    if (n == 0 || !idx) return vmd_fail("%s is empty", what);
    for (size_t i = 0; i < n; ++i) if (idx[i] < 0) return vmd_fail("%s contains a negative atom index", what);
    return true;
}

static const size_t kMaxSet = 0x7fffffff;     // ---- from here: what the entry points share, each check and each piece of construction once

// the names of a statement that defines several properties: each free, no two alike
static bool names_ok(vmd_script_ir_t* ir, const char* const* names, int n) {
    for (int k = 0; k < n; ++k) {
        if (!ir_name_ok(ir, names[k])) return false;
        for (int j = 0; j < k; ++j) if (!strcmp(names[j], names[k])) return vmd_fail("property '%s' already defined", names[k]);
    }
    return true;
}

// one argument set of a population: P + 1 offsets that start at 0 and increase, valid indices.  `what` is the form's word; `arg` names the set
// among several (" a"), or is "" where the form has one
static bool population_ok(const char* what, const char* arg, size_t P, const int32_t* idx, const int32_t* offs) {
    if (!offs) return vmd_fail("%s set%s has no context offsets", what, arg);
    if (offs[0] != 0) return vmd_fail("context offsets must start at 0");
    for (size_t c = 0; c < P; ++c)
        if (offs[c + 1] <= offs[c]) return vmd_fail("%s context %zu has an empty set%s (offsets must increase)", what, c, arg);
    char label[48];
    snprintf(label, sizeof(label), "%s set%s", what, arg);
    return idx_ok(idx, (size_t)offs[P], label);
}

static bool range_ok(Form f, float rmin, float rmax) {
    if (f == Form::RDF) return (rmin >= 0.0f && rmax > rmin) || vmd_fail("rdf range must satisfy 0 <= rmin < rmax");
    return (std::isfinite(rmin) && std::isfinite(rmax) && rmin >= 0.0f && rmax > rmin)
        || vmd_fail("within range must be finite and satisfy 0 <= rmin < rmax");
}

static bool set_size_ok(std::initializer_list<size_t> sizes) {
    for (size_t n : sizes) if (n > kMaxSet) return vmd_fail("within set too large");
    return true;
}

// a within() shell (an rdf / sdf argument, a term of an expression): its reference list, its size, its range
static bool shell_ok(const vmd_shell_t& h) {
    return idx_ok(h.ref, h.nref, "within reference set") && set_size_ok({h.nref}) && range_ok(Form::WITHIN, h.rmin, h.rmax);
}

static Property make_property(Form form, const char* name) { Property p; p.name = name; p.form = form; return p; }

// the part of a descriptor every rdf entry point shares, checked and filled; the same for sdf
static bool rdf_head(Property& p, vmd_script_ir_t* ir, const char* name, const int32_t* ref, size_t nref, const int32_t* target, size_t ntarget,
                     float rmin, float rmax) {
    if (!ir_name_ok(ir, name) || !idx_ok(ref, nref, "rdf reference set") || !idx_ok(target, ntarget, "rdf target set")
        || !range_ok(Form::RDF, rmin, rmax)) return false;
    p = make_property(Form::RDF, name);
    p.a.assign(ref, ref + nref); p.b.assign(target, target + ntarget);
    p.rmin = rmin; p.rmax = rmax;
    return true;
}

static bool sdf_head(Property& p, vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m, const int32_t* target,
                     size_t ntarget, float cutoff) {
    if (!ir_name_ok(ir, name) || !idx_ok(structures, K * m, "sdf reference structures") || !idx_ok(target, ntarget, "sdf target set"))
        return false;
    if (!(cutoff > 0.0f)) return vmd_fail("sdf cutoff must be positive");
    p = make_property(Form::SDF, name);
    p.a.assign(structures, structures + K * m); p.b.assign(target, target + ntarget);
    p.K = K; p.m = m; p.rmax = cutoff;
    return true;
}

static void shell_copy(Property::ShellArg& dst, const vmd_shell_t& h) {
    dst.on = true; dst.ref.assign(h.ref, h.ref + h.nref); dst.rmin = h.rmin; dst.rmax = h.rmax;
}

static bool commit(vmd_script_ir_t* ir, Property* p, int n = 1) {
    for (int k = 0; k < n; ++k) ir->props.push_back(std::move(p[k]));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_rdf(vmd_script_ir_t* ir, const char* name, const int32_t* ref, size_t nref,
                               const int32_t* target, size_t ntarget, float rmin, float rmax) {
    Property p;
    return rdf_head(p, ir, name, ref, nref, target, ntarget, rmin, rmax) && commit(ir, &p);
}

extern "C" bool vmd_ir_add_sdf(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                               const int32_t* target, size_t ntarget, float cutoff) {
    Property p;
    return sdf_head(p, ir, name, structures, K, m, target, ntarget, cutoff) && commit(ir, &p);
}

static bool distance_kind_ok(vmd_distance_kind_t kind) { return ((int)kind >= 0 && (int)kind <= 3) || vmd_fail("unknown distance kind %d", (int)kind); }

extern "C" bool vmd_ir_add_distance(vmd_script_ir_t* ir, const char* name, vmd_distance_kind_t kind,
                                    const int32_t* a, size_t na, const int32_t* b, size_t nb) {
    if (!ir_name_ok(ir, name) || !idx_ok(a, na, "distance set a") || !idx_ok(b, nb, "distance set b") || !distance_kind_ok(kind)) return false;
    Property p = make_property(Form::DISTANCE, name);
    p.a.assign(a, a + na); p.b.assign(b, b + nb);
    p.aoff = {0, (int32_t)na}; p.boff = {0, (int32_t)nb};
    p.distance_kind = (int)kind;
    return commit(ir, &p);
}

// (the one population whose two sets are checked context by context, side by side: its messages name no set)
extern "C" bool vmd_ir_add_distance_population(vmd_script_ir_t* ir, const char* name, vmd_distance_kind_t kind, size_t P,
                                               const int32_t* a, const int32_t* a_offsets, const int32_t* b, const int32_t* b_offsets) {
    if (!ir_name_ok(ir, name)) return false;
    if (P == 0 || !a_offsets || !b_offsets) return vmd_fail("distance population is empty");
    if (!distance_kind_ok(kind)) return false;
    if (a_offsets[0] != 0 || b_offsets[0] != 0) return vmd_fail("context offsets must start at 0");
    for (size_t c = 0; c < P; ++c) {
        if (a_offsets[c + 1] <= a_offsets[c] || b_offsets[c + 1] <= b_offsets[c]) return vmd_fail("distance context %zu has an empty set",
                c);
        if (kind == VMD_DISTANCE_PAIR && ((a_offsets[c + 1] - a_offsets[c]) != a_offsets[1] || (b_offsets[c + 1]
                - b_offsets[c]) != b_offsets[1]))
            return vmd_fail("distance_pair needs contexts of equal size");
    }
    if (!idx_ok(a, (size_t)a_offsets[P], "distance set a") || !idx_ok(b, (size_t)b_offsets[P], "distance set b")) return false;
    Property p = make_property(Form::DISTANCE, name);
    p.a.assign(a, a + a_offsets[P]); p.b.assign(b, b + b_offsets[P]);
    p.aoff.assign(a_offsets, a_offsets + P + 1); p.boff.assign(b_offsets, b_offsets + P + 1);
    p.distance_kind = (int)kind;
    return commit(ir, &p);
}

// angle / dihedral (DESIGN S6b), `{n0, n1, n2} = shape_weights(sel)` and `name = rmsd(sel)` `[in <contexts>]`: the
// form's argument sets per context; shape_weights defines three properties over its one set, a component each
static bool ir_add_sets(vmd_script_ir_t* ir, Form form, const char* const* names, size_t P, const int32_t* const* sets, const int32_t* const* offs) {
    static const char* const arg[4] = {" a", " b", " c", " d"};
    const FormFacts& f = kFormFacts[(int)form];
    const int nprops = form == Form::SHAPE ? 3 : 1;
    if (!names_ok(ir, names, nprops)) return false;
    if (P == 0) return vmd_fail("%s population is empty", f.word);
    for (int k = 0; k < f.nargs; ++k) if (!population_ok(f.word, f.nargs > 1 ? arg[k] : "", P, sets[k], offs[k])) return false;
    Property p[3];
    for (int j = 0; j < nprops; ++j) {
        p[j] = make_property(form, names[j]);
        p[j].shape_comp = j;
        std::vector<int32_t>* dst[4] = {&p[j].a, &p[j].b, &p[j].c, &p[j].d};
        std::vector<int32_t>* dof[4] = {&p[j].aoff, &p[j].boff, &p[j].coff, &p[j].doff};
        for (int k = 0; k < f.nargs; ++k) { dst[k]->assign(sets[k], sets[k] + offs[k][P]); dof[k]->assign(offs[k], offs[k] + P + 1); }
    }
    return commit(ir, p, nprops);
}

// the single forms: one context whose offsets are {0, n}
static bool ir_add_sets_single(vmd_script_ir_t* ir, Form form, const char* const* names, const int32_t* const* sets, const size_t* n) {
    const FormFacts& f = kFormFacts[(int)form];
    int32_t o[4][2];
    const int32_t* offs[4];
    for (int k = 0; k < f.nargs; ++k) {
        if (n[k] > kMaxSet) return vmd_fail("%s set too large", f.word);
        o[k][0] = 0; o[k][1] = (int32_t)n[k]; offs[k] = o[k];
    }
    return ir_add_sets(ir, form, names, 1, sets, offs);
}

extern "C" bool vmd_ir_add_angle(vmd_script_ir_t* ir, const char* name, const int32_t* a, size_t na, const int32_t* b, size_t nb,
                                 const int32_t* c, size_t nc) {
    const int32_t* sets[3] = {a, b, c};
    const size_t n[3] = {na, nb, nc};
    return ir_add_sets_single(ir, Form::ANGLE, &name, sets, n);
}

extern "C" bool vmd_ir_add_dihedral(vmd_script_ir_t* ir, const char* name, const int32_t* a, size_t na, const int32_t* b, size_t nb,
                                    const int32_t* c, size_t nc, const int32_t* d, size_t nd) {
    const int32_t* sets[4] = {a, b, c, d};
    const size_t n[4] = {na, nb, nc, nd};
    return ir_add_sets_single(ir, Form::DIHEDRAL, &name, sets, n);
}

extern "C" bool vmd_ir_add_angle_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* a, const int32_t* a_offsets,
                                            const int32_t* b, const int32_t* b_offsets, const int32_t* c, const int32_t* c_offsets) {
    const int32_t* sets[3] = {a, b, c};
    const int32_t* offs[3] = {a_offsets, b_offsets, c_offsets};
    return ir_add_sets(ir, Form::ANGLE, &name, P, sets, offs);
}

extern "C" bool vmd_ir_add_dihedral_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* a, const int32_t* a_offsets,
                                               const int32_t* b, const int32_t* b_offsets, const int32_t* c, const int32_t* c_offsets,
                                               const int32_t* d, const int32_t* d_offsets) {
    const int32_t* sets[4] = {a, b, c, d};
    const int32_t* offs[4] = {a_offsets, b_offsets, c_offsets, d_offsets};
    return ir_add_sets(ir, Form::DIHEDRAL, &name, P, sets, offs);
}

// (a statement of three names: the descriptor list and the names are looked at before anything else)
static bool shape_names_ok(vmd_script_ir_t* ir, const char* const names[3]) {
    if (!ir) return vmd_fail("ir is NULL");
    return names || vmd_fail("shape_weights needs three property names");
}

extern "C" bool vmd_ir_add_shape_weights(vmd_script_ir_t* ir, const char* const names[3], const int32_t* idx, size_t n) {
    if (n > kMaxSet) return vmd_fail("shape_weights set too large");
    return shape_names_ok(ir, names) && ir_add_sets_single(ir, Form::SHAPE, names, &idx, &n);
}

extern "C" bool vmd_ir_add_shape_weights_population(vmd_script_ir_t* ir, const char* const names[3], size_t P, const int32_t* idx,
                                                    const int32_t* offsets) {
    return shape_names_ok(ir, names) && ir_add_sets(ir, Form::SHAPE, names, P, &idx, &offsets);
}

extern "C" bool vmd_ir_add_rmsd(vmd_script_ir_t* ir, const char* name, const int32_t* idx, size_t n) {
    return ir_add_sets_single(ir, Form::RMSD, &name, &idx, &n);
}

extern "C" bool vmd_ir_add_rmsd_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* idx, const int32_t* offsets) {
    return ir_add_sets(ir, Form::RMSD, &name, P, &idx, &offsets);
}

// rmsf: rmsd's sets and rmsd's checks; one MAP-class record of per-atom accumulators
extern "C" bool vmd_ir_add_rmsf(vmd_script_ir_t* ir, const char* name, const int32_t* idx, size_t n) {
    return ir_add_sets_single(ir, Form::RMSF, &name, &idx, &n);
}

extern "C" bool vmd_ir_add_rmsf_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* idx, const int32_t* offsets) {
    return ir_add_sets(ir, Form::RMSF, &name, P, &idx, &offsets);
}

// `name = rdf(T and within(a:b, R), target, {rmin, rmax});`: vmd_ir_add_rdf with either side a shell
extern "C" bool vmd_ir_add_rdf_shell(vmd_script_ir_t* ir, const char* name, const int32_t* ref, size_t nref, const vmd_shell_t* ref_shell,
                                     const int32_t* target, size_t ntarget, const vmd_shell_t* target_shell, float rmin, float rmax) {
    if (!ref_shell && !target_shell) return vmd_ir_add_rdf(ir, name, ref, nref, target, ntarget, rmin, rmax);
    Property p;
    if (!rdf_head(p, ir, name, ref, nref, target, ntarget, rmin, rmax) || !set_size_ok({nref, ntarget})) return false;
    const vmd_shell_t* sh[2] = {ref_shell, target_shell};
    for (const vmd_shell_t* h : sh) if (h && !shell_ok(*h)) return false;
    for (int k = 0; k < 2; ++k) if (sh[k]) shell_copy(p.shell[k], *sh[k]);
    return commit(ir, &p);
}

// `name = sdf(structures, T and within(a:b, R), cutoff);`: vmd_ir_add_sdf with the target a shell
extern "C" bool vmd_ir_add_sdf_shell(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                                     const int32_t* target, size_t ntarget, const vmd_shell_t* target_shell, float cutoff) {
    if (!target_shell) return vmd_ir_add_sdf(ir, name, structures, K, m, target, ntarget, cutoff);
    Property p;
    const vmd_shell_t& h = *target_shell;
    // (the target's size is checked between the shell's list and the shell's size)
    if (!sdf_head(p, ir, name, structures, K, m, target, ntarget, cutoff) || !idx_ok(h.ref, h.nref, "within reference set")
        || !set_size_ok({ntarget, h.nref}) || !range_ok(Form::WITHIN, h.rmin, h.rmax)) return false;
    shell_copy(p.shell[1], h);
    return commit(ir, &p);
}

// `name = count(T and within(rmin:rmax, R));`: one temporal property, one value per frame
extern "C" bool vmd_ir_add_within_count(vmd_script_ir_t* ir, const char* name, const int32_t* target, size_t ntarget,
                                        const int32_t* ref, size_t nref, float rmin, float rmax) {
    if (!ir_name_ok(ir, name) || !idx_ok(target, ntarget, "within target set") || !idx_ok(ref, nref, "within reference set")) return false;
    if (!set_size_ok({ntarget, nref}) || !range_ok(Form::WITHIN, rmin, rmax)) return false;
    Property p = make_property(Form::WITHIN, name);
    p.a.assign(target, target + ntarget); p.b.assign(ref, ref + nref);
    p.aoff = {0, (int32_t)ntarget}; p.boff = {0, (int32_t)nref};
    p.rmin = rmin; p.rmax = rmax;
    return commit(ir, &p);
}

// and / or / not over within() shells: the checks both entry points share
static bool expr_ok(const vmd_shell_expr_t* x) {
    if (!x) return vmd_fail("shell expression is NULL");
    if (x->nterms < 1 || x->nterms > VMD_SHELL_EXPR_MAX_TERMS || !x->terms)
        return vmd_fail("shell expression needs 1 to %d terms, got %zu", VMD_SHELL_EXPR_MAX_TERMS, x->nterms);
    if (x->truth >> (1u << x->nterms)) return vmd_fail("shell expression truth table has bits above 2^%zu", x->nterms);
    for (size_t i = 0; i < x->nterms; ++i) if (!shell_ok(x->terms[i])) return false;
    return true;
}

static void expr_copy(Property& p, const vmd_shell_expr_t* x) {
    p.expr_terms.resize(x->nterms);
    for (size_t i = 0; i < x->nterms; ++i) shell_copy(p.expr_terms[i], x->terms[i]);
    p.expr_truth = x->truth;
}

// `name = count(T and <expression over within() terms>);`.  One term with truth 0b10 IS the one-term count
extern "C" bool vmd_ir_add_within_count_expr(vmd_script_ir_t* ir, const char* name, const int32_t* target, size_t ntarget,
                                             const vmd_shell_expr_t* expr) {
    if (!ir_name_ok(ir, name) || !idx_ok(target, ntarget, "within target set") || !expr_ok(expr) || !set_size_ok({ntarget})) return false;
    if (expr->nterms == 1 && expr->truth == 2u)
        return vmd_ir_add_within_count(ir, name, target, ntarget, expr->terms[0].ref, expr->terms[0].nref, expr->terms[0].rmin, expr->terms[0].rmax);
    Property p = make_property(Form::WITHIN_EXPR, name);
    p.a.assign(target, target + ntarget);
    p.aoff = {0, (int32_t)ntarget}; p.boff = {0, 0};
    expr_copy(p, expr);
    return commit(ir, &p);
}

// `name = sdf(structures, T and <expression over within() terms>, cutoff);`.  One term with truth 0b10 IS vmd_ir_add_sdf_shell
extern "C" bool vmd_ir_add_sdf_shell_expr(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                                          const int32_t* target, size_t ntarget, const vmd_shell_expr_t* expr, float cutoff) {
    Property p;
    if (!sdf_head(p, ir, name, structures, K, m, target, ntarget, cutoff) || !expr_ok(expr) || !set_size_ok({ntarget})) return false;
    if (expr->nterms == 1 && expr->truth == 2u) return vmd_ir_add_sdf_shell(ir, name, structures, K, m, target, ntarget, &expr->terms[0], cutoff);
    expr_copy(p, expr);
    return commit(ir, &p);
}

// a backbone statement: the names and the backbone, checked in this order; `word` is the form's
static bool backbone_ok(vmd_script_ir_t* ir, const char* word, const char* const names[2], const vmd_backbone_t* bb) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !bb) return vmd_fail("%s needs two property names and a backbone", word);
    if (!names_ok(ir, names, 2)) return false;
    const size_t nseg = bb->num_segments;
    if (nseg == 0) return vmd_fail("%s backbone has no segment", word);
    if (nseg > 0x3fffffff) return vmd_fail("%s backbone too large", word);
    if (!bb->n || !bb->ca || !bb->c) return vmd_fail("%s backbone has a NULL atom list", word);
    if (!idx_ok(bb->n, nseg, "backbone N list") || !idx_ok(bb->ca, nseg, "backbone CA list") || !idx_ok(bb->c, nseg, "backbone C list"))
        return false;
    if (!bb->range_offsets || bb->num_ranges == 0) return vmd_fail("%s backbone has no range offsets", word);
    if (bb->range_offsets[0] != 0) return vmd_fail("backbone range offsets must start at 0");
    for (size_t r = 0; r < bb->num_ranges; ++r)
        if (bb->range_offsets[r + 1] <= bb->range_offsets[r]) return vmd_fail("backbone range %zu is empty (offsets must increase)", r);
    if (bb->range_offsets[bb->num_ranges] != nseg)
        return vmd_fail("backbone range offsets end at %u, not at the %zu segments", bb->range_offsets[bb->num_ranges], nseg);
    if (bb->rama_class)
        for (size_t s = 0; s < nseg; ++s)
            if (bb->rama_class[s] > 3 && bb->rama_class[s] != 255)
                return vmd_fail("backbone segment %zu has class %u (0..3 or 255)", s, (unsigned)bb->rama_class[s]);
    return true;
}

// ... and copied into the statement's first descriptor: a = N, b = CA, c = C, aoff = the range offsets, the class bytes
static Property backbone_property(Form form, const char* name, const vmd_backbone_t* bb) {
    const size_t nseg = bb->num_segments;
    Property t = make_property(form, name);
    t.a.assign(bb->n, bb->n + nseg); t.b.assign(bb->ca, bb->ca + nseg); t.c.assign(bb->c, bb->c + nseg);
    t.aoff.assign(bb->range_offsets, bb->range_offsets + bb->num_ranges + 1);
    if (bb->rama_class) t.rama_class.assign(bb->rama_class, bb->rama_class + nseg); else t.rama_class.assign(nseg, 0);
    return t;
}

// `{table, map} = ramachandran(backbone)`: the angle table and the density map, two descriptors in a row
extern "C" bool vmd_ir_add_ramachandran(vmd_script_ir_t* ir, const char* const names[2], const vmd_backbone_t* bb) {
    if (!backbone_ok(ir, "ramachandran", names, bb)) return false;
    const size_t nseg = bb->num_segments;
    Property t = backbone_property(Form::RAMA_TABLE, names[0], bb);
    t.rama_link.assign(nseg, 3);
    for (size_t r = 0; r < bb->num_ranges; ++r) {
        t.rama_link[bb->range_offsets[r]] &= (uint8_t)~1u;
        t.rama_link[bb->range_offsets[r + 1] - 1] &= (uint8_t)~2u;
    }
    Property tm[2] = {std::move(t), make_property(Form::RAMA_MAP, names[1])};
    tm[1].K = nseg;
    return commit(ir, tm, 2);
}

// `{classes, populations} = secondary_structure(backbone, o)`: the class table and the populations, two descriptors in a row
extern "C" bool vmd_ir_add_secondary_structure(vmd_script_ir_t* ir, const char* const names[2], const vmd_backbone_t* bb, const int32_t* o) {
    if (!backbone_ok(ir, "secondary_structure", names, bb)) return false;
    const size_t nseg = bb->num_segments;
    if (!o) return vmd_fail("secondary_structure has no carbonyl oxygen list");
    for (size_t s = 0; s < nseg; ++s)
        if (o[s] < -1) return vmd_fail("backbone O list holds %d for segment %zu (an atom index, or -1 for none)", o[s], s);
    if (nseg > VMD_SS_MAX_SEGMENTS) return vmd_fail("secondary_structure backbone has %zu segments (at most %d)", nseg, VMD_SS_MAX_SEGMENTS);
    Property t = backbone_property(Form::SS_CLASS, names[0], bb);
    t.ss_o.assign(o, o + nseg);
    Property tp[2] = {std::move(t), make_property(Form::SS_POP, names[1])};
    tp[1].K = nseg;
    return commit(ir, tp, 2);
}

// `{count, occupancy} = hbonds(sites, r_da, angle_min)`: the per-frame count and the occupancy record, two descriptors in a row
extern "C" bool vmd_ir_add_hbonds(vmd_script_ir_t* ir, const char* const names[2], const vmd_hbond_sites_t* sites, float r_da, float angle_min_deg) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !sites) return vmd_fail("hbonds needs two property names and the sites");
    if (!names_ok(ir, names, 2)) return false;
    if (sites->npairs == 0 || !sites->donor || !sites->hydrogen) return vmd_fail("hbonds donor pair list is empty");
    if (!idx_ok(sites->donor, sites->npairs, "hbonds donor list") || !idx_ok(sites->hydrogen, sites->npairs, "hbonds hydrogen list") ||
        !idx_ok(sites->acceptor, sites->nacc, "hbonds acceptor list")) return false;
    if (sites->npairs > kMaxSet || sites->nacc > kMaxSet || sites->npairs + sites->nacc + 1 > kMaxSet) return vmd_fail("hbonds set too large");
    for (size_t j = 0; j < sites->npairs; ++j)
        if (sites->hydrogen[j] == sites->donor[j]) return vmd_fail("hbonds pair %zu names atom %d as donor and as its hydrogen", j, sites->donor[j]);
    if (!std::isfinite(r_da) || !(r_da > 0.0f)) return vmd_fail("hbonds donor-acceptor distance must be finite and positive");
    if (!(angle_min_deg >= 90.0f && angle_min_deg <= 180.0f)) return vmd_fail("hbonds minimum angle must lie in [90, 180] degrees");
    Property t = make_property(Form::HBOND_COUNT, names[0]);
    t.a.assign(sites->donor, sites->donor + sites->npairs); t.c.assign(sites->hydrogen, sites->hydrogen + sites->npairs);
    t.b.assign(sites->acceptor, sites->acceptor + sites->nacc);
    t.aoff = {0, (int32_t)sites->npairs}; t.boff = {0, (int32_t)sites->nacc}; t.coff = {0, (int32_t)sites->npairs};
    t.rmin = 0.0f; t.rmax = r_da;
    t.hb_angle = angle_min_deg;
    // c2 = cos^2(angle_min): formed in double, rounded once to fp32 (180 degrees: 1 exactly; 90 degrees: 0 exactly)
    const double cs = angle_min_deg == 90.0f ? 0.0 : angle_min_deg == 180.0f ? -1.0 : std::cos((double)angle_min_deg * (M_PI / 180.0));
    t.hb_c2 = (float)(cs * cs);
    Property tp[2] = {std::move(t), make_property(Form::HBOND_OCC, names[1])};
    tp[1].K = sites->npairs; tp[1].m = sites->nacc;
    return commit(ir, tp, 2);
}

// D-SASA-POINTS: the golden-section spiral, formed in double, rounded once to fp32.  The evaluator uploads what this function
// hands out; a restatement takes its points from here, because libm's last bit is nobody's contract.
extern "C" size_t vmd_sasa_points(uint32_t npoints, float (*out)[3], size_t cap) {
    if (npoints < 1 || npoints > VMD_SASA_MAX_POINTS) { vmd_fail("sasa points per sphere must lie in [1, %d]", VMD_SASA_MAX_POINTS); return 0; }
    if (!out && cap) { vmd_fail("vmd_sasa_points: out is NULL"); return 0; }
    const double golden = M_PI * (3.0 - std::sqrt(5.0));
    for (uint32_t k = 0; k < npoints && k < cap; ++k) {
        const double z = 1.0 - (2.0 * (double)k + 1.0) / (double)npoints;
        const double rho = std::sqrt(1.0 - z * z), phi = (double)k * golden;
        out[k][0] = (float)(rho * std::cos(phi)); out[k][1] = (float)(rho * std::sin(phi)); out[k][2] = (float)z;
    }
    return npoints;
}

// `{area, points} = sasa(sites, probe, npoints)`: the per-frame area and the record of accessible points, two descriptors in a row
extern "C" bool vmd_ir_add_sasa(vmd_script_ir_t* ir, const char* const names[2], const vmd_sasa_sites_t* sites, float probe, uint32_t npoints) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !sites) return vmd_fail("sasa needs two property names and the sites");
    if (!names_ok(ir, names, 2)) return false;
    if (sites->nmeas == 0 || !sites->measured || !sites->measured_radius) return vmd_fail("sasa measured list is empty");
    if (sites->nenv == 0 || !sites->env || !sites->env_radius) return vmd_fail("sasa environment list is empty");
    if (!idx_ok(sites->measured, sites->nmeas, "sasa measured list") || !idx_ok(sites->env, sites->nenv, "sasa environment list")) return false;
    if (sites->nmeas >= kMaxSet || sites->nenv > kMaxSet) return vmd_fail("sasa set too large");
    if (!std::isfinite(probe) || !(probe >= 0.0f)) return vmd_fail("sasa probe radius must be finite and not negative");
    if (npoints < 1 || npoints > VMD_SASA_MAX_POINTS) return vmd_fail("sasa points per sphere must lie in [1, %d]", VMD_SASA_MAX_POINTS);
    float rmax = 0.0f;
    for (int side = 0; side < 2; ++side) {
        const float* r = side ? sites->env_radius : sites->measured_radius;
        const size_t n = side ? sites->nenv : sites->nmeas;
        for (size_t i = 0; i < n; ++i) {
            if (!std::isfinite(r[i]) || !(r[i] > 0.0f))
                return vmd_fail("sasa %s radius %zu must be finite and positive", side ? "environment" : "measured", i);
            const float R = r[i] + probe;
            // (keeps the point weight in 32 bits and the cutoff at most 16 A)
            if (!(R <= 8.0f)) return vmd_fail("sasa %s radius %zu plus the probe exceeds 8", side ? "environment" : "measured", i);
            rmax = std::max(rmax, R);
        }
    }
    Property t = make_property(Form::SASA_AREA, names[0]);
    t.a.assign(sites->measured, sites->measured + sites->nmeas); t.b.assign(sites->env, sites->env + sites->nenv);
    t.aoff = {0, (int32_t)sites->nmeas}; t.boff = {0, (int32_t)sites->nenv};
    t.sasa_ra.assign(sites->measured_radius, sites->measured_radius + sites->nmeas);
    t.sasa_rb.assign(sites->env_radius, sites->env_radius + sites->nenv);
    t.sasa_probe = probe; t.sasa_npoints = npoints;
    t.rmin = 0.0f; t.rmax = rmax + rmax;            // r_cut = 2 max(R): exact in fp32
    Property tp[2] = {std::move(t), make_property(Form::SASA_OCC, names[1])};
    tp[1].K = sites->nmeas; tp[1].m = npoints;
    return commit(ir, tp, 2);
}

// `{count, map[, q]} = contacts(sites, r_cut, min_sep)`: the per-frame count, the record of the map and, with a native list,
// the native fraction - two or three descriptors in a row
extern "C" bool vmd_ir_add_contacts(vmd_script_ir_t* ir, const char* const names[3], const vmd_contact_sites_t* sites, float r_cut,
                                    uint32_t min_sep) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !sites) return vmd_fail("contacts needs its property names and the sites");
    if (sites->nnative > 0 && !names[2]) return vmd_fail("contacts with a native list needs a third property name");
    if (sites->nnative == 0 && names[2]) return vmd_fail("contacts without a native list takes two property names (the third must be NULL)");
    const int nnames = sites->nnative > 0 ? 3 : 2;
    if (!names_ok(ir, names, nnames)) return false;
    if (sites->nentries == 0 || !sites->atom || !sites->group) return vmd_fail("contacts entry list is empty");
    if (!idx_ok(sites->atom, sites->nentries, "contacts entry list")) return false;
    if (sites->nentries > kMaxSet) return vmd_fail("contacts set too large");
    if (sites->ngroups < 2 || sites->ngroups > VMD_CONTACT_MAX_GROUPS) return vmd_fail("contacts group count must lie in [2, %d]", VMD_CONTACT_MAX_GROUPS);
    const int64_t G = (int64_t)sites->ngroups;
    for (size_t i = 0; i < sites->nentries; ++i)
        if (sites->group[i] < 0 || sites->group[i] >= G) return vmd_fail("contacts entry %zu names group %d outside [0, %zu)", i, sites->group[i], sites->ngroups);
    if (!std::isfinite(r_cut) || !(r_cut > 0.0f)) return vmd_fail("contacts cutoff must be finite and positive");
    if (min_sep < 1 || (int64_t)min_sep > G - 1) return vmd_fail("contacts minimum separation must lie in [1, %zu]", sites->ngroups - 1);
    if (sites->nnative > 0 && !sites->native) return vmd_fail("contacts native list is NULL");
    if (sites->nnative > (size_t)(G * (G - 1) / 2)) return vmd_fail("contacts native list names a pair twice");
    Property t = make_property(Form::CONTACT_COUNT, names[0]);
    std::vector<uint8_t> seen(sites->nnative ? (size_t)(G * (G - 1) / 2) : 0, 0);
    for (size_t k = 0; k < sites->nnative; ++k) {
        int64_t g = sites->native[k][0], h = sites->native[k][1];
        if (g < 0 || h < 0 || g >= G || h >= G) return vmd_fail("contacts native pair %zu names a group outside [0, %zu)", k, sites->ngroups);
        if (g == h) return vmd_fail("contacts native pair %zu names group %d twice", k, (int)g);
        if (g > h) std::swap(g, h);
        if (h - g < (int64_t)min_sep) return vmd_fail("contacts native pair %zu is closer than the minimum separation", k);
        const size_t pidx = (size_t)(g * (2 * G - g - 1) / 2 + (h - g - 1));
        if (seen[pidx]) return vmd_fail("contacts native pair %zu is listed twice", k);
        seen[pidx] = 1;
        t.ct_native.push_back((int32_t)g); t.ct_native.push_back((int32_t)h);
    }
    t.a.assign(sites->atom, sites->atom + sites->nentries);
    t.ct_group.assign(sites->group, sites->group + sites->nentries);
    t.aoff = {0, (int32_t)sites->nentries};
    t.rmin = 0.0f; t.rmax = r_cut;
    t.K = sites->ngroups; t.ct_min_sep = min_sep;
    Property tp[3] = {std::move(t), make_property(Form::CONTACT_OCC, names[1]), make_property(Form::CONTACT_NATIVE, names[2] ? names[2] : "")};
    tp[1].K = (size_t)(G * (G - 1) / 2);
    tp[2].K = sites->nnative;
    return commit(ir, tp, nnames);
}

// `{count, sizes, largest} = clusters(sites, r_cut)`: the clusters per frame, the record of their sizes and the largest
// cluster per frame - three descriptors in a row
extern "C" bool vmd_ir_add_clusters(vmd_script_ir_t* ir, const char* const names[3], const vmd_contact_sites_t* sites, float r_cut) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !sites) return vmd_fail("clusters needs its property names and the sites");
    if (!names[0] || !names[1] || !names[2]) return vmd_fail("clusters needs three property names");
    if (!names_ok(ir, names, 3)) return false;
    if (sites->nentries == 0 || !sites->atom || !sites->group) return vmd_fail("clusters entry list is empty");
    if (!idx_ok(sites->atom, sites->nentries, "clusters entry list")) return false;
    if (sites->nentries > kMaxSet) return vmd_fail("clusters set too large");
    if (sites->ngroups < 1 || sites->ngroups > VMD_CLUSTER_MAX_GROUPS) return vmd_fail("clusters group count must lie in [1, %u]", VMD_CLUSTER_MAX_GROUPS);
    if (sites->nnative != 0) return vmd_fail("clusters takes no native list (nnative must be 0)");
    const int64_t G = (int64_t)sites->ngroups;
    std::vector<uint8_t> named((size_t)G, 0);
    for (size_t i = 0; i < sites->nentries; ++i) {
        if (sites->group[i] < 0 || sites->group[i] >= G) return vmd_fail("clusters entry %zu names group %d outside [0, %zu)", i, sites->group[i], sites->ngroups);
        named[(size_t)sites->group[i]] = 1;
    }
    for (size_t g = 0; g < (size_t)G; ++g)
        if (!named[g]) return vmd_fail("clusters group %zu has no entry (a cluster of nothing has no size)", g);
    if (!std::isfinite(r_cut) || !(r_cut > 0.0f)) return vmd_fail("clusters cutoff must be finite and positive");
    Property t = make_property(Form::CLUSTER_COUNT, names[0]);
    t.a.assign(sites->atom, sites->atom + sites->nentries);
    t.ct_group.assign(sites->group, sites->group + sites->nentries);
    t.aoff = {0, (int32_t)sites->nentries};
    t.rmin = 0.0f; t.rmax = r_cut;
    t.K = sites->ngroups;
    Property tp[3] = {std::move(t), make_property(Form::CLUSTER_SIZES, names[1]), make_property(Form::CLUSTER_LARGEST, names[2])};
    tp[1].K = sites->ngroups;
    return commit(ir, tp, 3);
}

// `name = the position table of atoms`: one descriptor; vmd_eval_msd correlates its rows over lag times
extern "C" bool vmd_ir_add_msd(vmd_script_ir_t* ir, const char* name, const int32_t* idx, size_t n) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!name) return vmd_fail("msd needs a property name");
    if (!idx || n == 0) return vmd_fail("msd atom list is empty");
    if (!ir_name_ok(ir, name) || !idx_ok(idx, n, "msd atom list")) return false;
    if (n > VMD_MSD_MAX_ATOMS) return vmd_fail("msd set too large");
    Property t = make_property(Form::MSD_TABLE, name);
    t.a.assign(idx, idx + n);
    t.aoff = {0, (int32_t)n};
    return commit(ir, &t);
}

// what vmd_ir_geometry_atoms has counted and written so far
struct AtomSink {
    int32_t* out; size_t cap, n = 0;
    void put(int32_t i) { if (out && n < cap) out[n] = i; n += 1; }
    void put(const std::vector<int32_t>& v) { for (int32_t i : v) put(i); }
    void put(const std::vector<int32_t>& v, int32_t beg, int32_t end) { for (int32_t i = beg; i < end; ++i) put(v[(size_t)i]); }
};

// the atoms of an angle / dihedral property: every set of context `context` (all contexts when < 0), in argument order.  Returns the
// count and writes up to `cap` of them; 0 for other properties (the shim's MD_SCRIPT_VISUALIZE_ATOMS payload)
extern "C" size_t vmd_ir_geometry_atoms(const vmd_script_ir_t* ir, const char* name, int64_t context, int32_t* out, size_t cap) {
    if (!ir || !name) return 0;
    for (const Property& p : ir->props) {
        if (p.name != name) continue;
        AtomSink s{out, cap};
        // the contexts asked for, of `count`: [c0, c1), empty when there is no such context
        auto contexts = [&](size_t count, size_t& c0, size_t& c1) {
            c0 = context < 0 ? 0 : (size_t)context; c1 = context < 0 ? count : (size_t)context + 1;
            return context < (int64_t)count;
        };
        size_t c0 = 0, c1 = 0;
        switch (p.form) {
        case Form::RDF: case Form::SDF: case Form::DISTANCE: case Form::RAMA_MAP: case Form::SS_POP: case Form::HBOND_OCC: case Form::SASA_OCC:
        case Form::CONTACT_OCC: case Form::CONTACT_NATIVE: case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST:
            return 0;
        case Form::CONTACT_COUNT: case Form::CLUSTER_COUNT: case Form::MSD_TABLE:   // the entries' atoms; 1.18: the atoms (one context)
            if (context > 0) return 0;
            s.put(p.a);
            return s.n;
        case Form::SASA_AREA:       // the measured atoms, then the environment (one context)
            if (context > 0) return 0;
            s.put(p.a); s.put(p.b);
            return s.n;
        case Form::HBOND_COUNT:     // the donors, then their hydrogens, then the acceptors (one context)
            if (context > 0) return 0;
            s.put(p.a); s.put(p.c); s.put(p.b);
            return s.n;
        case Form::WITHIN:          // the static candidates: the reference set, then the target set (one context)
            if (context > 0) return 0;
            s.put(p.b); s.put(p.a);
            return s.n;
        case Form::WITHIN_EXPR:     // every term's reference set in term order, then the target set (one context)
            if (context > 0) return 0;
            for (auto& t : p.expr_terms) s.put(t.ref);
            s.put(p.a);
            return s.n;
        case Form::RAMA_TABLE:      // N, CA, C of the segment(s)
            if (!contexts(p.a.size(), c0, c1)) return 0;
            for (size_t sg = c0; sg < c1; ++sg) for (const auto* v : {&p.a, &p.b, &p.c}) s.put((*v)[sg]);
            return s.n;
        case Form::SS_CLASS:        // N, CA, C, O of the segment(s), a missing O left out
            if (!contexts(p.a.size(), c0, c1)) return 0;
            for (size_t sg = c0; sg < c1; ++sg) {
                for (const auto* v : {&p.a, &p.b, &p.c}) s.put((*v)[sg]);
                if (p.ss_o[sg] >= 0) s.put(p.ss_o[sg]);
            }
            return s.n;
        case Form::SHAPE: case Form::RMSD: case Form::RMSF:      // the set of the context(s)
            if (!contexts(p.aoff.size() - 1, c0, c1)) return 0;
            s.put(p.a, p.aoff[c0], p.aoff[c1]);
            return s.n;
        case Form::ANGLE: case Form::DIHEDRAL: {
            if (!contexts(p.aoff.size() - 1, c0, c1)) return 0;
            const std::vector<int32_t>* sets[4] = {&p.a, &p.b, &p.c, &p.d};
            const std::vector<int32_t>* offs[4] = {&p.aoff, &p.boff, &p.coff, &p.doff};
            for (size_t c = c0; c < c1; ++c) for (int k = 0; k < p.nargs(); ++k) s.put(*sets[k], (*offs[k])[c], (*offs[k])[c + 1]);
            return s.n;
        }
        }
    }
    return 0;
}

extern "C" bool vmd_ir_valid(const vmd_script_ir_t* ir) { return ir != nullptr; }

extern "C" uint64_t vmd_ir_fingerprint(const vmd_script_ir_t* ir) {
    if (!ir) return 0;
    const uint64_t cached = ir->fingerprint.load();
    if (cached) return cached;
    uint64_t h = 0xCBF29CE484222325ull;
    for (auto& p : ir->props) {
        const uint32_t kind = (uint32_t)p.cls();      // what used to be the descriptor's kind (4 bytes, 0..3) and dist_kind (an int, 0..10)
        const int geom = p.geom_code();
        h = fnv1a(h, p.name.data(), p.name.size());
        h = fnv1a(h, &kind, sizeof(kind));
        h = fnv1a(h, p.a.data(), p.a.size() * sizeof(int32_t));
        h = fnv1a(h, p.b.data(), p.b.size() * sizeof(int32_t));
        h = fnv1a(h, &p.rmin, sizeof(float)); h = fnv1a(h, &p.rmax, sizeof(float));
        h = fnv1a(h, &p.K, sizeof(p.K)); h = fnv1a(h, &p.m, sizeof(p.m)); h = fnv1a(h, &geom, sizeof(int));
        h = fnv1a(h, p.aoff.data(), p.aoff.size() * sizeof(int32_t)); h = fnv1a(h, p.boff.data(), p.boff.size() * sizeof(int32_t));
        // angle / dihedral only (empty otherwise: hashing no bytes leaves every earlier fingerprint as it was)
        h = fnv1a(h, p.c.data(), p.c.size() * sizeof(int32_t)); h = fnv1a(h, p.d.data(), p.d.size() * sizeof(int32_t));
        h = fnv1a(h, p.coff.data(), p.coff.size() * sizeof(int32_t)); h = fnv1a(h, p.doff.data(), p.doff.size() * sizeof(int32_t));
        switch (p.form) {     // what a form hashes of its own
        case Form::SHAPE: h = fnv1a(h, &p.shape_comp, sizeof(int)); break;
        case Form::RAMA_TABLE: h = fnv1a(h, p.rama_class.data(), p.rama_class.size()); break;     // 
        case Form::RDF: case Form::SDF: case Form::DISTANCE: case Form::ANGLE: case Form::DIHEDRAL: case Form::RMSD: case Form::WITHIN:
        case Form::WITHIN_EXPR: case Form::RAMA_MAP: case Form::SS_POP: case Form::RMSF: case Form::HBOND_OCC: break;
        case Form::HBOND_COUNT: h = fnv1a(h, &p.hb_angle, sizeof(float)); break;      // (the hydrogens are c, hashed above)
        case Form::SASA_OCC: case Form::CONTACT_OCC: case Form::CONTACT_NATIVE: case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST: break;
        case Form::MSD_TABLE: break;                                    // (the atoms are a, hashed above, the code 24)
        case Form::CLUSTER_COUNT:                                       // (the atoms are a, r_cut is rmax, the groups' number K; one group per entry of a)
            h = fnv1a(h, p.ct_group.data(), p.ct_group.size() * sizeof(int32_t));
            break;
        case Form::CONTACT_COUNT:                                       // (the atoms are a, r_cut is rmax, the groups' number K; one group per entry of a, the rest is the native list)
            h = fnv1a(h, &p.ct_min_sep, sizeof(uint32_t)); h = fnv1a(h, p.ct_group.data(), p.ct_group.size() * sizeof(int32_t));
            h = fnv1a(h, p.ct_native.data(), p.ct_native.size() * sizeof(int32_t));
            break;
        case Form::SASA_AREA:                                          // (the lists are a and b, boff says where a's radii end)
            h = fnv1a(h, &p.sasa_probe, sizeof(float)); h = fnv1a(h, &p.sasa_npoints, sizeof(uint32_t));
            h = fnv1a(h, p.sasa_ra.data(), p.sasa_ra.size() * sizeof(float)); h = fnv1a(h, p.sasa_rb.data(), p.sasa_rb.size() * sizeof(float));
            break;
        case Form::SS_CLASS:                                            // 
            h = fnv1a(h, p.rama_class.data(), p.rama_class.size()); h = fnv1a(h, p.ss_o.data(), p.ss_o.size() * sizeof(int32_t));
            break;
        }
        for (int k = 0; k < 2; ++k) {                                   // rdf / sdf over shells only, as above
            if (!p.shell[k].on) continue;
            const int32_t side = 0x5348454c + k;                        // "SHEL": which side carries the shell
            h = fnv1a(h, &side, sizeof(side));
            h = fnv1a(h, p.shell[k].ref.data(), p.shell[k].ref.size() * sizeof(int32_t));
            h = fnv1a(h, &p.shell[k].rmin, sizeof(float)); h = fnv1a(h, &p.shell[k].rmax, sizeof(float));
        }
        if (!p.expr_terms.empty()) {                                    // shell expressions only, as above
            const int32_t tag = 0x45585052;                             // "EXPR"
            const uint32_t nt = (uint32_t)p.expr_terms.size();
            h = fnv1a(h, &tag, sizeof(tag)); h = fnv1a(h, &nt, sizeof(nt)); h = fnv1a(h, &p.expr_truth, sizeof(uint32_t));
            for (auto& t : p.expr_terms) {
                const uint32_t nr = (uint32_t)t.ref.size();             // the lists of consecutive terms must not run into each other
                h = fnv1a(h, &nr, sizeof(nr)); h = fnv1a(h, t.ref.data(), t.ref.size() * sizeof(int32_t));
                h = fnv1a(h, &t.rmin, sizeof(float)); h = fnv1a(h, &t.rmax, sizeof(float));
            }
        }
    }
    h = h ? h : 1;
    ir->fingerprint = h;
    return h;
}

extern "C" size_t vmd_ir_property_count(const vmd_script_ir_t* ir) { return ir ? ir->props.size() : 0; }

extern "C" const char* const* vmd_ir_property_names(const vmd_script_ir_t* ir) { return ir ? ir->names.data() : nullptr; }

extern "C" vmd_property_flags_t vmd_ir_property_flags(const vmd_script_ir_t* ir, const char* name) {
    if (!ir || !name) return VMD_PROPERTY_FLAG_NONE;
    for (auto& p : ir->props) if (p.name == name) return p.flags();
    return VMD_PROPERTY_FLAG_NONE;
}
