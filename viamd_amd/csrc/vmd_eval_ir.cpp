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

// atom pairs one frame of this script asks for (rdf: |ref| x |target|; sdf: K x |target| + K m for the alignment; distance: |a| x |b| of
// every context; angle / dihedral / shape_weights: the atoms of every context's sets): what a host compares with its threshold before it sends a SMALL script to the GPU at all (include/vmd_md_script_shim.h,
// vmd_shim_set_min_work; VIAMD's default dataset is ~1e2 atoms, src/main.cpp:522-528)
extern "C" uint64_t vmd_ir_work_per_frame(const vmd_script_ir_t* ir) {
    if (!ir) return 0;
    uint64_t w = 0;
    for (const Property& p : ir->props) {
        if (p.kind == PROP_RDF) {
            w += (uint64_t)p.a.size() * (uint64_t)p.b.size();
            // the parent sizes (a bound that needs no frame) plus one neighbour query per shell, |T| + |R|
            for (int k = 0; k < 2; ++k) if (p.shell[k].on) w += (uint64_t)(k ? p.b : p.a).size() + (uint64_t)p.shell[k].ref.size();
        }
        else if (p.kind == PROP_SDF) {
            w += (uint64_t)p.K * ((uint64_t)p.b.size() + (uint64_t)p.m);
            if (p.shell[1].on) w += (uint64_t)p.b.size() + (uint64_t)p.shell[1].ref.size();     // the parent list plus the shell's query
            if (p.is_expr_sdf()) { w += (uint64_t)p.b.size(); for (auto& t : p.expr_terms) w += (uint64_t)t.ref.size(); }     // |T| + sum |R_i|
        }
        else if (p.is_shape()) { if (p.shape_comp == 0) w += (uint64_t)p.a.size(); }     // one pass over every context's set per statement
        else if (p.is_rmsd()) w += (uint64_t)p.a.size();                                 // the atoms of every context's set
        else if (p.is_rama()) w += 3 * (uint64_t)p.a.size();                             // N, CA, C of every segment
        else if (p.is_within()) w += (uint64_t)p.a.size() + (uint64_t)p.b.size();        // |T| + |R|: a neighbour query, not all pairs
        else if (p.is_within_expr()) { w += (uint64_t)p.a.size(); for (auto& t : p.expr_terms) w += (uint64_t)t.ref.size(); }     // |T| + sum |R_i|
        else if (p.nargs() > 2) { for (const auto* v : {&p.a, &p.b, &p.c, &p.d}) w += (uint64_t)v->size(); }     // each context: the sum of its set sizes
        else if (p.aoff.size() > 1) { for (size_t c = 0; c + 1 < p.aoff.size(); ++c) w += (uint64_t)(p.aoff[c + 1] - p.aoff[c])
                * (uint64_t)(p.boff[c + 1] - p.boff[c]); }
        else w += (uint64_t)p.a.size() * (uint64_t)p.b.size();
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

extern "C" bool vmd_ir_add_rdf(vmd_script_ir_t* ir, const char* name, const int32_t* ref, size_t nref,
                               const int32_t* target, size_t ntarget, float rmin, float rmax) {
    if (!ir_name_ok(ir, name) || !idx_ok(ref, nref, "rdf reference set") || !idx_ok(target, ntarget, "rdf target set")) return false;
    if (!(rmin >= 0.0f) || !(rmax > rmin)) return vmd_fail("rdf range must satisfy 0 <= rmin < rmax");
    Property p;
    p.name = name; p.kind = PROP_RDF; p.flags = VMD_PROPERTY_FLAG_DISTRIBUTION;
    p.a.assign(ref, ref + nref); p.b.assign(target, target + ntarget);
    p.rmin = rmin; p.rmax = rmax;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_sdf(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                               const int32_t* target, size_t ntarget, float cutoff) {
    if (!ir_name_ok(ir, name) || !idx_ok(structures, K * m, "sdf reference structures") || !idx_ok(target, ntarget,
            "sdf target set")) return false;
    if (!(cutoff > 0.0f)) return vmd_fail("sdf cutoff must be positive");
    Property p;
    p.name = name; p.kind = PROP_SDF; p.flags = VMD_PROPERTY_FLAG_VOLUME;
    p.a.assign(structures, structures + K * m); p.b.assign(target, target + ntarget);
    p.K = K; p.m = m; p.rmax = cutoff;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_distance(vmd_script_ir_t* ir, const char* name, vmd_distance_kind_t kind,
                                    const int32_t* a, size_t na, const int32_t* b, size_t nb) {
    if (!ir_name_ok(ir, name) || !idx_ok(a, na, "distance set a") || !idx_ok(b, nb, "distance set b")) return false;
    if ((int)kind < 0 || (int)kind > 3) return vmd_fail("unknown distance kind %d", (int)kind);
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.a.assign(a, a + na); p.b.assign(b, b + nb);
    p.aoff = {0, (int32_t)na}; p.boff = {0, (int32_t)nb};
    p.dist_kind = (int)kind;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_distance_population(vmd_script_ir_t* ir, const char* name, vmd_distance_kind_t kind, size_t P,
                                               const int32_t* a, const int32_t* a_offsets, const int32_t* b, const int32_t* b_offsets) {
    if (!ir_name_ok(ir, name)) return false;
    if (P == 0 || !a_offsets || !b_offsets) return vmd_fail("distance population is empty");
    if ((int)kind < 0 || (int)kind > 3) return vmd_fail("unknown distance kind %d", (int)kind);
    if (a_offsets[0] != 0 || b_offsets[0] != 0) return vmd_fail("context offsets must start at 0");
    for (size_t c = 0; c < P; ++c) {
        if (a_offsets[c + 1] <= a_offsets[c] || b_offsets[c + 1] <= b_offsets[c]) return vmd_fail("distance context %zu has an empty set",
                c);
        if (kind == VMD_DISTANCE_PAIR && ((a_offsets[c + 1] - a_offsets[c]) != a_offsets[1] || (b_offsets[c + 1]
                - b_offsets[c]) != b_offsets[1]))
            return vmd_fail("distance_pair needs contexts of equal size");
    }
    if (!idx_ok(a, (size_t)a_offsets[P], "distance set a") || !idx_ok(b, (size_t)b_offsets[P], "distance set b")) return false;
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.a.assign(a, a + a_offsets[P]); p.b.assign(b, b + b_offsets[P]);
    p.aoff.assign(a_offsets, a_offsets + P + 1); p.boff.assign(b_offsets, b_offsets + P + 1);
    p.dist_kind = (int)kind;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// angle / dihedral (DESIGN S6b): n argument sets per context, validated like the distance population
static bool ir_add_geometry(vmd_script_ir_t* ir, const char* name, int kind, size_t P, const int32_t* const* sets, const int32_t* const* offs) {
    static const char* const arg[4] = {"a", "b", "c", "d"};
    const char* what = kind == GEOM_ANGLE ? "angle" : "dihedral";
    const int n = kind == GEOM_ANGLE ? 3 : 4;
    if (!ir_name_ok(ir, name)) return false;
    if (P == 0) return vmd_fail("%s population is empty", what);
    char label[48];
    for (int k = 0; k < n; ++k) {
        if (!offs[k]) return vmd_fail("%s set %s has no context offsets", what, arg[k]);
        if (offs[k][0] != 0) return vmd_fail("context offsets must start at 0");
        for (size_t c = 0; c < P; ++c)
            if (offs[k][c + 1] <= offs[k][c]) return vmd_fail("%s context %zu has an empty set %s (offsets must increase)", what, c, arg[k]);
        snprintf(label, sizeof(label), "%s set %s", what, arg[k]);
        if (!idx_ok(sets[k], (size_t)offs[k][P], label)) return false;
    }
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.dist_kind = kind;
    std::vector<int32_t>* dst[4] = {&p.a, &p.b, &p.c, &p.d};
    std::vector<int32_t>* dof[4] = {&p.aoff, &p.boff, &p.coff, &p.doff};
    for (int k = 0; k < n; ++k) { dst[k]->assign(sets[k], sets[k] + offs[k][P]); dof[k]->assign(offs[k], offs[k] + P + 1); }
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_angle(vmd_script_ir_t* ir, const char* name, const int32_t* a, size_t na, const int32_t* b, size_t nb,
                                 const int32_t* c, size_t nc) {
    if (na > 0x7fffffff || nb > 0x7fffffff || nc > 0x7fffffff) return vmd_fail("angle set too large");
    const int32_t ao[2] = {0, (int32_t)na}, bo[2] = {0, (int32_t)nb}, co[2] = {0, (int32_t)nc};
    const int32_t* sets[3] = {a, b, c};
    const int32_t* offs[3] = {ao, bo, co};
    return ir_add_geometry(ir, name, GEOM_ANGLE, 1, sets, offs);
}

extern "C" bool vmd_ir_add_dihedral(vmd_script_ir_t* ir, const char* name, const int32_t* a, size_t na, const int32_t* b, size_t nb,
                                    const int32_t* c, size_t nc, const int32_t* d, size_t nd) {
    if (na > 0x7fffffff || nb > 0x7fffffff || nc > 0x7fffffff || nd > 0x7fffffff) return vmd_fail("dihedral set too large");
    const int32_t ao[2] = {0, (int32_t)na}, bo[2] = {0, (int32_t)nb}, co[2] = {0, (int32_t)nc}, dof[2] = {0, (int32_t)nd};
    const int32_t* sets[4] = {a, b, c, d};
    const int32_t* offs[4] = {ao, bo, co, dof};
    return ir_add_geometry(ir, name, GEOM_DIHEDRAL, 1, sets, offs);
}

extern "C" bool vmd_ir_add_angle_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* a, const int32_t* a_offsets,
                                            const int32_t* b, const int32_t* b_offsets, const int32_t* c, const int32_t* c_offsets) {
    const int32_t* sets[3] = {a, b, c};
    const int32_t* offs[3] = {a_offsets, b_offsets, c_offsets};
    return ir_add_geometry(ir, name, GEOM_ANGLE, P, sets, offs);
}

extern "C" bool vmd_ir_add_dihedral_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* a, const int32_t* a_offsets,
                                               const int32_t* b, const int32_t* b_offsets, const int32_t* c, const int32_t* c_offsets,
                                               const int32_t* d, const int32_t* d_offsets) {
    const int32_t* sets[4] = {a, b, c, d};
    const int32_t* offs[4] = {a_offsets, b_offsets, c_offsets, d_offsets};
    return ir_add_geometry(ir, name, GEOM_DIHEDRAL, P, sets, offs);
}

// `{n0, n1, n2} = shape_weights(sel) [in <contexts>];`: three temporal properties over one population of sets
static bool ir_add_shape(vmd_script_ir_t* ir, const char* const names[3], size_t P, const int32_t* idx, const int32_t* offs) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names) return vmd_fail("shape_weights needs three property names");
    for (int k = 0; k < 3; ++k) {
        if (!ir_name_ok(ir, names[k])) return false;
        for (int j = 0; j < k; ++j)
            if (!strcmp(names[j], names[k])) return vmd_fail("property '%s' already defined", names[k]);
    }
    if (P == 0) return vmd_fail("shape_weights population is empty");
    if (!offs) return vmd_fail("shape_weights set has no context offsets");
    if (offs[0] != 0) return vmd_fail("context offsets must start at 0");
    for (size_t c = 0; c < P; ++c)
        if (offs[c + 1] <= offs[c]) return vmd_fail("shape_weights context %zu has an empty set (offsets must increase)", c);
    if (!idx_ok(idx, (size_t)offs[P], "shape_weights set")) return false;
    for (int k = 0; k < 3; ++k) {
        Property p;
        p.name = names[k]; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
        p.dist_kind = GEOM_SHAPE; p.shape_comp = k;
        p.a.assign(idx, idx + offs[P]); p.aoff.assign(offs, offs + P + 1);
        ir->props.push_back(std::move(p));
    }
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_shape_weights(vmd_script_ir_t* ir, const char* const names[3], const int32_t* idx, size_t n) {
    if (n > 0x7fffffff) return vmd_fail("shape_weights set too large");
    const int32_t off[2] = {0, (int32_t)n};
    return ir_add_shape(ir, names, 1, idx, off);
}

extern "C" bool vmd_ir_add_shape_weights_population(vmd_script_ir_t* ir, const char* const names[3], size_t P, const int32_t* idx,
                                                    const int32_t* offsets) {
    return ir_add_shape(ir, names, P, idx, offsets);
}

// `name = rmsd(sel) [in <contexts>];`: one temporal property over a population of sets, validated like ir_add_geometry
static bool ir_add_rmsd(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* idx, const int32_t* offs) {
    if (!ir_name_ok(ir, name)) return false;
    if (P == 0) return vmd_fail("rmsd population is empty");
    if (!offs) return vmd_fail("rmsd set has no context offsets");
    if (offs[0] != 0) return vmd_fail("context offsets must start at 0");
    for (size_t c = 0; c < P; ++c)
        if (offs[c + 1] <= offs[c]) return vmd_fail("rmsd context %zu has an empty set (offsets must increase)", c);
    if (!idx_ok(idx, (size_t)offs[P], "rmsd set")) return false;
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.dist_kind = GEOM_RMSD;
    p.a.assign(idx, idx + offs[P]); p.aoff.assign(offs, offs + P + 1);
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

extern "C" bool vmd_ir_add_rmsd(vmd_script_ir_t* ir, const char* name, const int32_t* idx, size_t n) {
    if (n > 0x7fffffff) return vmd_fail("rmsd set too large");
    const int32_t off[2] = {0, (int32_t)n};
    return ir_add_rmsd(ir, name, 1, idx, off);
}

extern "C" bool vmd_ir_add_rmsd_population(vmd_script_ir_t* ir, const char* name, size_t P, const int32_t* idx, const int32_t* offsets) {
    return ir_add_rmsd(ir, name, P, idx, offsets);
}

// `name = rdf(T and within(a:b, R), target, {rmin, rmax});`: vmd_ir_add_rdf with either side a shell; the shells validated like
// vmd_ir_add_within_count
extern "C" bool vmd_ir_add_rdf_shell(vmd_script_ir_t* ir, const char* name, const int32_t* ref, size_t nref, const vmd_shell_t* ref_shell,
                                     const int32_t* target, size_t ntarget, const vmd_shell_t* target_shell, float rmin, float rmax) {
    if (!ref_shell && !target_shell) return vmd_ir_add_rdf(ir, name, ref, nref, target, ntarget, rmin, rmax);
    if (!ir_name_ok(ir, name) || !idx_ok(ref, nref, "rdf reference set") || !idx_ok(target, ntarget, "rdf target set")) return false;
    if (!(rmin >= 0.0f) || !(rmax > rmin)) return vmd_fail("rdf range must satisfy 0 <= rmin < rmax");
    if (nref > 0x7fffffff || ntarget > 0x7fffffff) return vmd_fail("within set too large");
    const vmd_shell_t* sh[2] = {ref_shell, target_shell};
    for (const vmd_shell_t* h : sh) {
        if (!h) continue;
        if (!idx_ok(h->ref, h->nref, "within reference set")) return false;
        if (h->nref > 0x7fffffff) return vmd_fail("within set too large");
        if (!std::isfinite(h->rmin) || !std::isfinite(h->rmax) || !(h->rmin >= 0.0f) || !(h->rmax > h->rmin))
            return vmd_fail("within range must be finite and satisfy 0 <= rmin < rmax");
    }
    Property p;
    p.name = name; p.kind = PROP_RDF; p.flags = VMD_PROPERTY_FLAG_DISTRIBUTION;
    p.a.assign(ref, ref + nref); p.b.assign(target, target + ntarget);
    p.rmin = rmin; p.rmax = rmax;
    for (int k = 0; k < 2; ++k) {
        if (!sh[k]) continue;
        p.shell[k].on = true;
        p.shell[k].ref.assign(sh[k]->ref, sh[k]->ref + sh[k]->nref);
        p.shell[k].rmin = sh[k]->rmin; p.shell[k].rmax = sh[k]->rmax;
    }
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// `name = sdf(structures, T and within(a:b, R), cutoff);`: vmd_ir_add_sdf with the target a shell, validated like
// vmd_ir_add_within_count
extern "C" bool vmd_ir_add_sdf_shell(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                                     const int32_t* target, size_t ntarget, const vmd_shell_t* target_shell, float cutoff) {
    if (!target_shell) return vmd_ir_add_sdf(ir, name, structures, K, m, target, ntarget, cutoff);
    if (!ir_name_ok(ir, name) || !idx_ok(structures, K * m, "sdf reference structures") || !idx_ok(target, ntarget,
            "sdf target set")) return false;
    if (!(cutoff > 0.0f)) return vmd_fail("sdf cutoff must be positive");
    const vmd_shell_t* h = target_shell;
    if (!idx_ok(h->ref, h->nref, "within reference set")) return false;
    if (ntarget > 0x7fffffff || h->nref > 0x7fffffff) return vmd_fail("within set too large");
    if (!std::isfinite(h->rmin) || !std::isfinite(h->rmax) || !(h->rmin >= 0.0f) || !(h->rmax > h->rmin))
        return vmd_fail("within range must be finite and satisfy 0 <= rmin < rmax");
    Property p;
    p.name = name; p.kind = PROP_SDF; p.flags = VMD_PROPERTY_FLAG_VOLUME;
    p.a.assign(structures, structures + K * m); p.b.assign(target, target + ntarget);
    p.K = K; p.m = m; p.rmax = cutoff;
    p.shell[1].on = true;
    p.shell[1].ref.assign(h->ref, h->ref + h->nref);
    p.shell[1].rmin = h->rmin; p.shell[1].rmax = h->rmax;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// `name = count(T and within(rmin:rmax, R));`: one temporal property, one value per frame; validated like ir_add_geometry
extern "C" bool vmd_ir_add_within_count(vmd_script_ir_t* ir, const char* name, const int32_t* target, size_t ntarget,
                                        const int32_t* ref, size_t nref, float rmin, float rmax) {
    if (!ir_name_ok(ir, name) || !idx_ok(target, ntarget, "within target set") || !idx_ok(ref, nref, "within reference set")) return false;
    if (ntarget > 0x7fffffff || nref > 0x7fffffff) return vmd_fail("within set too large");
    if (!std::isfinite(rmin) || !std::isfinite(rmax) || !(rmin >= 0.0f) || !(rmax > rmin))
        return vmd_fail("within range must be finite and satisfy 0 <= rmin < rmax");
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.dist_kind = GEOM_WITHIN;
    p.a.assign(target, target + ntarget); p.b.assign(ref, ref + nref);
    p.aoff = {0, (int32_t)ntarget}; p.boff = {0, (int32_t)nref};
    p.rmin = rmin; p.rmax = rmax;
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// and / or / not over within() shells: the checks both entry points share; every term validated like vmd_ir_add_within_count
static bool expr_ok(const vmd_shell_expr_t* x) {
    if (!x) return vmd_fail("shell expression is NULL");
    if (x->nterms < 1 || x->nterms > VMD_SHELL_EXPR_MAX_TERMS || !x->terms)
        return vmd_fail("shell expression needs 1 to %d terms, got %zu", VMD_SHELL_EXPR_MAX_TERMS, x->nterms);
    if (x->truth >> (1u << x->nterms)) return vmd_fail("shell expression truth table has bits above 2^%zu", x->nterms);
    for (size_t i = 0; i < x->nterms; ++i) {
        const vmd_shell_t& h = x->terms[i];
        if (!idx_ok(h.ref, h.nref, "within reference set")) return false;
        if (h.nref > 0x7fffffff) return vmd_fail("within set too large");
        if (!std::isfinite(h.rmin) || !std::isfinite(h.rmax) || !(h.rmin >= 0.0f) || !(h.rmax > h.rmin))
            return vmd_fail("within range must be finite and satisfy 0 <= rmin < rmax");
    }
    return true;
}

static void expr_copy(Property& p, const vmd_shell_expr_t* x) {
    p.expr_terms.resize(x->nterms);
    for (size_t i = 0; i < x->nterms; ++i) {
        p.expr_terms[i].ref.assign(x->terms[i].ref, x->terms[i].ref + x->terms[i].nref);
        p.expr_terms[i].rmin = x->terms[i].rmin; p.expr_terms[i].rmax = x->terms[i].rmax;
    }
    p.expr_truth = x->truth;
}

// `name = count(T and <expression over within() terms>);`.  One term with truth 0b10 IS the one-term count
extern "C" bool vmd_ir_add_within_count_expr(vmd_script_ir_t* ir, const char* name, const int32_t* target, size_t ntarget,
                                             const vmd_shell_expr_t* expr) {
    if (!ir_name_ok(ir, name) || !idx_ok(target, ntarget, "within target set") || !expr_ok(expr)) return false;
    if (ntarget > 0x7fffffff) return vmd_fail("within set too large");
    if (expr->nterms == 1 && expr->truth == 2u)
        return vmd_ir_add_within_count(ir, name, target, ntarget, expr->terms[0].ref, expr->terms[0].nref, expr->terms[0].rmin, expr->terms[0].rmax);
    Property p;
    p.name = name; p.kind = PROP_DIST; p.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    p.dist_kind = GEOM_WITHIN_EXPR;
    p.a.assign(target, target + ntarget);
    p.aoff = {0, (int32_t)ntarget}; p.boff = {0, 0};
    expr_copy(p, expr);
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// `name = sdf(structures, T and <expression over within() terms>, cutoff);`.  One term with truth 0b10 IS vmd_ir_add_sdf_shell
extern "C" bool vmd_ir_add_sdf_shell_expr(vmd_script_ir_t* ir, const char* name, const int32_t* structures, size_t K, size_t m,
                                          const int32_t* target, size_t ntarget, const vmd_shell_expr_t* expr, float cutoff) {
    if (!ir_name_ok(ir, name) || !idx_ok(structures, K * m, "sdf reference structures") || !idx_ok(target, ntarget,
            "sdf target set")) return false;
    if (!(cutoff > 0.0f)) return vmd_fail("sdf cutoff must be positive");
    if (!expr_ok(expr)) return false;
    if (ntarget > 0x7fffffff) return vmd_fail("within set too large");
    if (expr->nterms == 1 && expr->truth == 2u) return vmd_ir_add_sdf_shell(ir, name, structures, K, m, target, ntarget, &expr->terms[0], cutoff);
    Property p;
    p.name = name; p.kind = PROP_SDF; p.flags = VMD_PROPERTY_FLAG_VOLUME;
    p.a.assign(structures, structures + K * m); p.b.assign(target, target + ntarget);
    p.K = K; p.m = m; p.rmax = cutoff;
    expr_copy(p, expr);
    ir->props.push_back(std::move(p));
    ir->rebuild_names();
    return true;
}

// `{table, map} = ramachandran(backbone)`: the angle table and the density map, two descriptors in a row
extern "C" bool vmd_ir_add_ramachandran(vmd_script_ir_t* ir, const char* const names[2], const vmd_backbone_t* bb) {
    if (!ir) return vmd_fail("ir is NULL");
    if (!names || !bb) return vmd_fail("ramachandran needs two property names and a backbone");
    for (int k = 0; k < 2; ++k) if (!ir_name_ok(ir, names[k])) return false;
    if (!strcmp(names[0], names[1])) return vmd_fail("property '%s' already defined", names[1]);
    const size_t nseg = bb->num_segments;
    if (nseg == 0) return vmd_fail("ramachandran backbone has no segment");
    if (nseg > 0x3fffffff) return vmd_fail("ramachandran backbone too large");
    if (!bb->n || !bb->ca || !bb->c) return vmd_fail("ramachandran backbone has a NULL atom list");
    if (!idx_ok(bb->n, nseg, "backbone N list") || !idx_ok(bb->ca, nseg, "backbone CA list") || !idx_ok(bb->c, nseg, "backbone C list"))
        return false;
    if (!bb->range_offsets || bb->num_ranges == 0) return vmd_fail("ramachandran backbone has no range offsets");
    if (bb->range_offsets[0] != 0) return vmd_fail("backbone range offsets must start at 0");
    for (size_t r = 0; r < bb->num_ranges; ++r)
        if (bb->range_offsets[r + 1] <= bb->range_offsets[r]) return vmd_fail("backbone range %zu is empty (offsets must increase)", r);
    if (bb->range_offsets[bb->num_ranges] != nseg)
        return vmd_fail("backbone range offsets end at %u, not at the %zu segments", bb->range_offsets[bb->num_ranges], nseg);
    if (bb->rama_class)
        for (size_t s = 0; s < nseg; ++s)
            if (bb->rama_class[s] > 3 && bb->rama_class[s] != 255)
                return vmd_fail("backbone segment %zu has class %u (0..3 or 255)", s, (unsigned)bb->rama_class[s]);
    Property t;
    t.name = names[0]; t.kind = PROP_DIST; t.flags = VMD_PROPERTY_FLAG_TEMPORAL;
    t.dist_kind = GEOM_RAMA;
    t.a.assign(bb->n, bb->n + nseg); t.b.assign(bb->ca, bb->ca + nseg); t.c.assign(bb->c, bb->c + nseg);
    t.aoff.assign(bb->range_offsets, bb->range_offsets + bb->num_ranges + 1);
    if (bb->rama_class) t.rama_class.assign(bb->rama_class, bb->rama_class + nseg); else t.rama_class.assign(nseg, 0);
    t.rama_link.assign(nseg, 3);
    for (size_t r = 0; r < bb->num_ranges; ++r) {
        t.rama_link[bb->range_offsets[r]] &= (uint8_t)~1u;
        t.rama_link[bb->range_offsets[r + 1] - 1] &= (uint8_t)~2u;
    }
    Property m;
    m.name = names[1]; m.kind = PROP_RAMA; m.flags = VMD_PROPERTY_FLAG_MAP;
    m.K = nseg;
    ir->props.push_back(std::move(t));
    ir->props.push_back(std::move(m));
    ir->rebuild_names();
    return true;
}

// the atoms of an angle / dihedral property: every set of context `context` (all contexts when < 0), in argument order.  Returns the
// count and writes up to `cap` of them; 0 for other properties (the shim's MD_SCRIPT_VISUALIZE_ATOMS payload)
extern "C" size_t vmd_ir_geometry_atoms(const vmd_script_ir_t* ir, const char* name, int64_t context, int32_t* out, size_t cap) {
    if (!ir || !name) return 0;
    for (const Property& p : ir->props) {
        if (p.name != name) continue;
        if (p.is_within()) {     // the static candidates: the reference set, then the target set (one context)
            if (context > 0) return 0;
            size_t n = 0;
            for (const auto* v : {&p.b, &p.a}) for (int32_t i : *v) { if (out && n < cap) out[n] = i; n += 1; }
            return n;
        }
        if (p.is_within_expr()) {     // every term's reference set in term order, then the target set (one context)
            if (context > 0) return 0;
            size_t n = 0;
            for (auto& t : p.expr_terms) for (int32_t i : t.ref) { if (out && n < cap) out[n] = i; n += 1; }
            for (int32_t i : p.a) { if (out && n < cap) out[n] = i; n += 1; }
            return n;
        }
        if (p.is_rama()) {     // N, CA, C of the segment(s)
            if (context >= (int64_t)p.a.size()) return 0;
            const size_t s0 = context < 0 ? 0 : (size_t)context, s1 = context < 0 ? p.a.size() : (size_t)context + 1;
            size_t n = 0;
            for (size_t sg = s0; sg < s1; ++sg)
                for (const auto* v : {&p.a, &p.b, &p.c}) { if (out && n < cap) out[n] = (*v)[sg]; n += 1; }
            return n;
        }
        if (p.kind != PROP_DIST || (p.nargs() < 3 && !p.is_shape() && !p.is_rmsd())) return 0;
        const size_t P = p.aoff.size() - 1;
        if (context >= (int64_t)P) return 0;
        const size_t c0 = context < 0 ? 0 : (size_t)context, c1 = context < 0 ? P : (size_t)context + 1;
        if (p.is_shape() || p.is_rmsd()) {     // shape_weights, rmsd: the set of the context(s)
            size_t n = 0;
            for (int32_t i = p.aoff[c0]; i < p.aoff[c1]; ++i) { if (out && n < cap) out[n] = p.a[(size_t)i]; n += 1; }
            return n;
        }
        const std::vector<int32_t>* sets[4] = {&p.a, &p.b, &p.c, &p.d};
        const std::vector<int32_t>* offs[4] = {&p.aoff, &p.boff, &p.coff, &p.doff};
        size_t n = 0;
        for (size_t c = c0; c < c1; ++c)
            for (int k = 0; k < p.nargs(); ++k)
                for (int32_t i = (*offs[k])[c]; i < (*offs[k])[c + 1]; ++i) { if (out && n < cap) out[n] = (*sets[k])[(size_t)i]; n += 1; }
        return n;
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
        h = fnv1a(h, p.name.data(), p.name.size());
        h = fnv1a(h, &p.kind, sizeof(p.kind));
        h = fnv1a(h, p.a.data(), p.a.size() * sizeof(int32_t));
        h = fnv1a(h, p.b.data(), p.b.size() * sizeof(int32_t));
        h = fnv1a(h, &p.rmin, sizeof(float)); h = fnv1a(h, &p.rmax, sizeof(float));
        h = fnv1a(h, &p.K, sizeof(p.K)); h = fnv1a(h, &p.m, sizeof(p.m)); h = fnv1a(h, &p.dist_kind, sizeof(int));
        h = fnv1a(h, p.aoff.data(), p.aoff.size() * sizeof(int32_t)); h = fnv1a(h, p.boff.data(), p.boff.size() * sizeof(int32_t));
        // angle / dihedral only (empty otherwise: hashing no bytes leaves every earlier fingerprint as it was)
        h = fnv1a(h, p.c.data(), p.c.size() * sizeof(int32_t)); h = fnv1a(h, p.d.data(), p.d.size() * sizeof(int32_t));
        h = fnv1a(h, p.coff.data(), p.coff.size() * sizeof(int32_t)); h = fnv1a(h, p.doff.data(), p.doff.size() * sizeof(int32_t));
        if (p.is_shape()) h = fnv1a(h, &p.shape_comp, sizeof(int));     // shape_weights only, as above
        if (p.is_rama()) h = fnv1a(h, p.rama_class.data(), p.rama_class.size());     // ramachandran only, as above
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
    for (auto& p : ir->props) if (p.name == name) return p.flags;
    return VMD_PROPERTY_FLAG_NONE;
}
