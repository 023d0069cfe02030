// viamd_amd/csrc/vmd_eval_core.cpp - the evaluator object: vmd_eval_create / _free / _clear_data / _interrupt (md_script_eval_create
// ..., /root/reference/src/main.cpp:960-990), the plan of pair passes for co-evaluated RDFs, the host views VIAMD polls
// (md_script_property_data_t: values / weights / aggregate / ranges / fingerprint, :1286-1524), accessors, block / source settings of
// the filtered evaluation, and the sdf() vis payload (reference pose + per-frame matrices, density_volume.cpp:183-204).
#include "vmd_eval_internal.h"

// what `values` of a volume points at between clear_data and the evaluation's first view: zero pages shared by every volume of the process,
// mapped read-only (a write through the pointer is a bug and faults loudly) and never backed by memory of their own (anonymous pages that
// are only ever read all alias the kernel's zero page)
float* zero_volume_view(size_t nfloats) {
    static std::mutex mtx;
    static float* view = nullptr;
    static size_t cap = 0;
    std::lock_guard<std::mutex> l(mtx);
    if (nfloats > cap) {
        void* m = mmap(nullptr, nfloats * sizeof(float), PROT_READ, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return nullptr;
        view = (float*)m; cap = nfloats;        // (an earlier, smaller mapping stays: readers may still hold it)
    }
    return view;
}

TrajId traj_id(const vmd_trajectory_i* t) {
    TrajId id;
    if (t) { id.inst = t->inst; id.fn = t->load_frame ? reinterpret_cast<const void*>(t->load_frame)
            : reinterpret_cast<const void*>(t->device_view); }
    return id;
}

PropState* find_prop(const vmd_script_eval_t* e, const char* name) {
    if (!e || !name) return nullptr;
    for (auto& p : e->props) if (p->prop.name == name) return p.get();
    return nullptr;
}

int intern_selection(vmd_script_eval_t* e, const std::vector<int32_t>& idx) {
    for (size_t i = 0; i < e->sels.size(); ++i) if (e->sels[i]->idx == idx) return (int)i;
    auto s = std::make_unique<Selection>();
    s->idx = idx;
    // periodic? the smallest m <= 4 with idx[t + m] - idx[t] the same for every t ("every third atom", "the two H of every water")
    if (g_opt.cells_sel_pattern.load() && idx.size() >= 8) {
        for (int m = 1; m <= 4 && !s->pat_m; ++m) {
            const int64_t period = (int64_t)idx[(size_t)m] - (int64_t)idx[0];
            if (period <= 0 || period > (1 << 20)) continue;
            bool ok = true;
            for (size_t t = 0; t + (size_t)m < idx.size() && ok; ++t) ok = (int64_t)idx[t + (size_t)m] - (int64_t)idx[t] == period;
            if (!ok) continue;
            s->pat_m = m; s->pat_first = idx[0]; s->pat_period = (int)period;
            for (int k = 0; k < m; ++k) s->pat_off[k] = idx[(size_t)k] - idx[0];
        }
    }
    s->overflow_bit = 1u << (e->sels.size() % 32);
    e->sels.push_back(std::move(s));
    return (int)e->sels.size() - 1;
}

// A shell argument (T, R, r_min, r_max) of an rdf or an sdf (1.8) as selections plus an interned Shell: its list T (T minus R
// under D-WITHIN-SELF flipped, as build_within_plan) and R are selections like any other, and properties that name the same shell share
// one object - its walk, its compaction, its mask.  -> the index in e->shells; *sel_t is T' (-1: nothing left, empty in every frame)
static int intern_shell(vmd_script_eval_t* e, std::vector<int32_t> t, const Property::ShellArg& h, int* sel_t) {
    if (e->spec.within_exclude_ref) {
        std::vector<int32_t> ref = h.ref;
        std::sort(ref.begin(), ref.end());
        t.erase(std::remove_if(t.begin(), t.end(), [&](int32_t a) { return std::binary_search(ref.begin(), ref.end(), a); }), t.end());
    }
    const int st = t.empty() ? -1 : intern_selection(e, t);
    const int sr = intern_selection(e, h.ref);
    *sel_t = st;
    for (size_t q = 0; q < e->shells.size(); ++q) {
        const Shell& x = *e->shells[q];
        if (x.sel_t == st && x.sel_r == sr && memcmp(&x.rmin, &h.rmin, sizeof(float)) == 0 && memcmp(&x.rmax, &h.rmax, sizeof(float)) == 0)
            return (int)q;
    }
    auto x = std::make_unique<Shell>();
    x->sel_t = st; x->sel_r = sr; x->rmin = h.rmin; x->rmax = h.rmax;
    e->shells.push_back(std::move(x));
    return (int)e->shells.size() - 1;
}

// Groups the RDF properties by range and decides, per group, between one pair pass per property and the class decomposition
// (see PairPass).  Classes are used when every set is duplicate-free, there are at most 8 of them, and the pair work
// (sum over passes of n_a * n_b, halved for same-set passes) drops by at least 10 %.
void build_rdf_plan(vmd_script_eval_t* e) {
    e->rdf_groups.clear();
    e->shells.clear();
    for (size_t i = 0; i < e->props.size(); ++i) {
        const Property& d = e->props[i]->prop;
        if (d.cls() != ResultClass::DISTRIBUTION) continue;
        RdfGroup* g = nullptr;
        for (auto& q : e->rdf_groups) if (memcmp(&q.rmin, &d.rmin, sizeof(float)) == 0 && memcmp(&q.rmax, &d.rmax, sizeof(float)) == 0) g =
                &q;
        if (!g) { e->rdf_groups.emplace_back(); g = &e->rdf_groups.back(); g->rmin = d.rmin; g->rmax = d.rmax; g->grid_r = d.rmax; }
        // an rdf over shells joins the group of its pair range - one grid, shared sorted copies - but not its passes or classes
        if (d.is_shell_rdf()) {
            g->shell_props.push_back((int)i);
            for (int k = 0; k < 2; ++k) if (d.shell[k].on) g->grid_r = std::max(g->grid_r, d.shell[k].rmax);
        } else g->props.push_back((int)i);
    }
    // every property keeps its own sets as selections (index lists only; sorted copies exist for the selections passes use):
    // the all-pairs kernel, which takes over when a batch cannot use the grid, works per property
    for (auto& p : e->props) {
        if (p->prop.cls() != ResultClass::DISTRIBUTION) continue;
        if (p->prop.is_shell_rdf()) {
            for (int k = 0; k < 2; ++k) {
                const Property::ShellArg& h = p->prop.shell[k];
                const std::vector<int32_t>& t = k ? p->prop.b : p->prop.a;
                int& sel = k ? p->sel_b : p->sel_a;
                if (!h.on) { sel = t.empty() ? -1 : intern_selection(e, t); continue; }
                p->shell_of[k] = intern_shell(e, t, h, &sel);
                e->shells[p->shell_of[k]]->rdf_use = true;
            }
            continue;
        }
        p->sel_a = intern_selection(e, p->prop.a);
        p->sel_b = p->same_set ? p->sel_a : intern_selection(e, p->prop.b);
    }
    // sdfs over a shell target: (T or T minus R, R, r_min, r_max) interned with the rdfs' shells - a shell an rdf and an sdf
    // both name is one Shell, and R one selection whose cell-sorted copy every user on the same grid shares.  sel_b of the property is the
    // shell's T'; the scatter itself keeps the property's own target list (owner, progression), the mask says who takes part
    e->shell_sdf_props.clear();
    for (size_t i = 0; i < e->props.size(); ++i) {
        PropState* p = e->props[i].get();
        if (!p->prop.is_shell_sdf()) continue;
        p->shell_of[1] = intern_shell(e, p->prop.b, p->prop.shell[1], &p->sel_b);
        e->shells[p->shell_of[1]]->sdf_use = true;
        e->shell_sdf_props.push_back((int)i);
    }
    for (auto& g : e->rdf_groups) {
        auto direct = [&]() {
            g.passes.clear(); g.classes = false;
            for (int pi : g.props) {
                PropState* p = e->props[pi].get();
                PairPass ps;
                ps.sel_a = p->sel_a; ps.sel_b = p->sel_b;
                ps.same = p->same_set;
                ps.targets.push_back({pi, 1});
                g.passes.push_back(std::move(ps));
            }
        };
        const size_t np = g.props.size();
        if (np < 2 || np > 30 || !g_opt.rdf_classes) { direct(); continue; }
        // signature of every atom: bit 2k = in the reference set of the group's k-th property, bit 2k + 1 = in its target set
        int32_t amax = 0;
        for (int pi : g.props) { for (int32_t a : e->props[pi]->prop.a) amax = std::max(amax, a); for (int32_t b
                : e->props[pi]->prop.b) amax = std::max(amax, b); }
        std::vector<uint64_t> sig((size_t)amax + 1, 0);
        bool dup = false;
        for (size_t k = 0; k < np && !dup; ++k) {
            const Property& d = e->props[g.props[k]]->prop;
            for (int side = 0; side < 2 && !dup; ++side) {
                const uint64_t bit = 1ull << (2 * k + side);
                for (int32_t a : (side ? d.b : d.a)) { if (sig[a] & bit) { dup = true; break; } sig[a] |= bit; }
            }
        }
        if (dup) { direct(); continue; }      // a set that lists an atom twice counts it twice: only the direct passes reproduce that
        std::vector<uint64_t> csig;
        std::vector<std::vector<int32_t>> cidx;
        bool too_many = false;
        for (int32_t a = 0; a <= amax && !too_many; ++a) {
            if (!sig[a]) continue;
            size_t c = 0;
            while (c < csig.size() && csig[c] != sig[a]) ++c;
            if (c == csig.size()) { if (csig.size() == 8) { too_many = true; break; } csig.push_back(sig[a]); cidx.emplace_back(); }
            cidx[c].push_back(a);
        }
        if (too_many) { direct(); continue; }
        std::vector<PairPass> passes;
        double cost_classes = 0.0, cost_direct = 0.0;
        for (size_t c = 0; c < csig.size(); ++c)
            for (size_t d = c; d < csig.size(); ++d) {
                PairPass ps;
                for (size_t k = 0; k < np; ++k) {
                    const uint64_t X = 1ull << (2 * k), Y = 1ull << (2 * k + 1);
                    uint64_t mult;
                    if (c == d) mult = ((csig[c] & X) && (csig[c] & Y)) ? 1 : 0;
                    else mult = (((csig[c] & X) && (csig[d] & Y)) ? 1 : 0) + (((csig[d] & X) && (csig[c] & Y)) ? 1 : 0);
                    if (mult) ps.targets.push_back({g.props[k], mult});
                }
                if (ps.targets.empty()) continue;
                ps.same = c == d;
                ps.sel_a = (int)c; ps.sel_b = (int)d;          // class indices for now
                cost_classes += (double)cidx[c].size() * (double)cidx[d].size() * (c == d ? 0.5 : 1.0);
                passes.push_back(std::move(ps));
            }
        for (int pi : g.props) {
            const PropState* p = e->props[pi].get();
            cost_direct += (double)p->prop.a.size() * (double)p->prop.b.size() * (p->same_set ? 0.5 : 1.0);
        }
        if (!(cost_classes < 0.9 * cost_direct)) { direct(); continue; }
        std::vector<int> csel(csig.size());
        for (size_t c = 0; c < csig.size(); ++c) csel[c] = intern_selection(e, cidx[c]);
        for (auto& ps : passes) { ps.sel_a = csel[ps.sel_a]; ps.sel_b = csel[ps.sel_b]; }
        g.passes = std::move(passes);
        g.classes = true;
    }
}

// T minus R, in T's order (D-WITHIN-SELF / D-EXPR-SELF flipped)
static std::vector<int32_t> minus(std::vector<int32_t> t, std::vector<int32_t> ref) {
    std::sort(ref.begin(), ref.end());
    t.erase(std::remove_if(t.begin(), t.end(), [&](int32_t a) { return std::binary_search(ref.begin(), ref.end(), a); }), t.end());
    return t;
}

// within counts: the target and reference sets become interned selections - shared with the RDF properties of the script -
// so that a cell-sorted copy one of them built on the same grid in a batch is not built again.  D-WITHIN-SELF flipped: T minus R, formed here
void build_within_plan(vmd_script_eval_t* e) {
    e->within_props.clear();
    for (size_t i = 0; i < e->props.size(); ++i) {
        PropState* p = e->props[i].get();
        if (p->prop.form != Form::WITHIN) continue;
        const std::vector<int32_t> tgt = e->spec.within_exclude_ref ? minus(p->prop.a, p->prop.b) : p->prop.a;
        p->within_empty = tgt.empty();
        p->sel_a = p->within_empty ? -1 : intern_selection(e, tgt);
        p->sel_b = intern_selection(e, p->prop.b);
        e->within_props.push_back((int)i);
    }
}

// The neighbour analyses - hydrogen bonds, accessible area (1.15), contact maps (1.16), clusters (1.17): the side that is cell-sorted (the
// acceptors, the environment, the entry list) becomes an interned selection - shared with everything else of the script, so that a
// cell-sorted copy another pass built on the same grid in a batch is not built again.  The side in the lanes (the donors, the measured
// entries) is walked in list order and is never sorted: its selection only says how many lanes the grid is chosen for.  Contacts and clusters have ONE
// list, on both sides: its cell-sorted copy is what its own entries walk.
void build_neighbour_plan(vmd_script_eval_t* e) {
    const struct { Form count; std::vector<int> vmd_script_eval_t::* props; bool one_list; } kinds[] = {
        {Form::HBOND_COUNT, &vmd_script_eval_t::hbond_props, false}, {Form::SASA_AREA, &vmd_script_eval_t::sasa_props, false},
        {Form::CONTACT_COUNT, &vmd_script_eval_t::contact_props, true}, {Form::CLUSTER_COUNT, &vmd_script_eval_t::cluster_props, true}};
    for (auto& k : kinds) {
        (e->*k.props).clear();
        for (size_t i = 0; i < e->props.size(); ++i) {
            PropState* p = e->props[i].get();
            if (p->prop.form != k.count) continue;
            p->sel_a = intern_selection(e, p->prop.a);
            p->sel_b = k.one_list ? p->sel_a : intern_selection(e, p->prop.b);
            (e->*k.props).push_back((int)i);
        }
    }
}

uint32_t shell_expr_live(uint32_t truth, const std::vector<int>& order, size_t pos) {
    uint32_t done = 0, later = 0;
    for (size_t k = 0; k < order.size(); ++k) { if (k < pos) done |= 1u << order[k]; else if (k > pos) later |= 1u << order[k]; }
    const uint32_t bit = 1u << order[pos];
    uint32_t live = 0;
    for (uint32_t v = 0; v < (1u << order.size()); ++v) {
        if (v & ~done) continue;
        for (uint32_t x = later;; x = (x - 1) & later) {          // every subset of the terms still to come
            if (((truth >> (v | x)) & 1u) != ((truth >> (v | x | bit)) & 1u)) { live |= 1u << v; break; }
            if (!x) break;
        }
    }
    return live;
}

// shell expressions: T, every R_i and, under D-EXPR-SELF flipped, every T minus R_i become interned selections - shared with
// everything else of the script, so that a cell-sorted copy of an R_i another pass built on the same grid in a batch is not built again
void build_expr_plan(vmd_script_eval_t* e) {
    e->exprs.clear();
    e->expr_count_props.clear();
    e->expr_sdf_props.clear();
    for (size_t i = 0; i < e->props.size(); ++i) {
        PropState* p = e->props[i].get();
        const Property& d = p->prop;
        if (d.form != Form::WITHIN_EXPR && !d.is_expr_sdf()) continue;
        const std::vector<int32_t>& T = d.is_expr_sdf() ? d.b : d.a;
        auto x = std::make_unique<ShellExpr>();
        x->sel_t = intern_selection(e, T);
        x->truth = d.expr_truth;
        for (const Property::ExprTerm& t : d.expr_terms) {
            ShellExpr::Term tm;
            tm.sel_r = intern_selection(e, t.ref);
            tm.rmin = t.rmin; tm.rmax = t.rmax;
            tm.sel_tt = x->sel_t;
            if (e->spec.within_exclude_ref) {
                const std::vector<int32_t> tt = minus(T, t.ref);
                tm.sel_tt = tt.empty() ? -1 : intern_selection(e, tt);
            }
            x->terms.push_back(tm);
        }
        for (size_t k = 0; k < x->terms.size(); ++k) x->order.push_back((int)k);
        std::stable_sort(x->order.begin(), x->order.end(), [&](int a, int b) {
            return e->sels[x->terms[a].sel_r]->idx.size() < e->sels[x->terms[b].sel_r]->idx.size(); });
        int found = -1;
        for (size_t q = 0; q < e->exprs.size() && found < 0; ++q) {
            const ShellExpr& y = *e->exprs[q];
            bool same = y.sel_t == x->sel_t && y.truth == x->truth && y.terms.size() == x->terms.size();
            for (size_t k = 0; same && k < y.terms.size(); ++k)
                same = y.terms[k].sel_r == x->terms[k].sel_r && memcmp(&y.terms[k].rmin, &x->terms[k].rmin, sizeof(float)) == 0 &&
                       memcmp(&y.terms[k].rmax, &x->terms[k].rmax, sizeof(float)) == 0;
            if (same) found = (int)q;
        }
        if (found < 0) { e->exprs.push_back(std::move(x)); found = (int)e->exprs.size() - 1; }
        p->expr_of = found;
        (d.is_expr_sdf() ? e->expr_sdf_props : e->expr_count_props).push_back((int)i);
    }
}

extern "C" vmd_script_eval_t* vmd_eval_create(size_t num_frames, const vmd_script_ir_t* ir) {
    if (!ir) { vmd_fail("vmd_eval_create: ir is NULL"); return nullptr; }
    if (vmd_device_count() <= 0) { vmd_fail("vmd_eval_create: no usable HIP device (the evaluator has no CPU path)"); return nullptr; }
    auto e = std::make_unique<vmd_script_eval_t>();
    if (hipGetDevice(&e->device) != hipSuccess) { vmd_fail("hipGetDevice failed"); return nullptr; }
    // streams and events come out of the process-wide cache (an eval has nine streams and ~20 events; VIAMD makes one per script edit)
    if (!(e->stream = pool_stream(false)) || !(e->copy_stream = pool_stream(false)) || !(e->aux_stream = pool_stream(false)) ||
        !(e->pair_stream = pool_stream(false))) { vmd_fail("hipStreamCreate failed"); return nullptr; }
    if (!(e->pair_fork = pool_event(false)) || !(e->pair_join = pool_event(false))) { vmd_fail("hipEventCreate failed"); return nullptr; }
    // the decoder's waves should get the wave slots the pair kernel leaves free as soon as a batch has arrived: highest priority
    for (auto& ds : e->decode_streams) if (!(ds = pool_stream(true))) { vmd_fail("hipStreamCreate failed"); return nullptr; }
    e->decode_stream = e->decode_streams[0];
    for (auto& rs : e->raw_slots) if (!(rs.uploaded = pool_event(false))) { vmd_fail("hipEventCreate failed"); return nullptr; }
    for (auto& st : e->stages) if (!(st.ready = pool_event(true))) { vmd_fail("hipEventCreate failed"); return nullptr; }
    e->ir_fingerprint = vmd_ir_fingerprint(ir);
    e->num_frames = num_frames;
    e->spec.rdf_closed = g_opt.spec_rdf_closed.load() != 0;
    e->spec.sdf_include_self = g_opt.spec_sdf_include_self.load() != 0;
    e->spec.sdf_density = g_opt.spec_sdf_density.load() != 0;
    e->spec.rdf_raw = g_opt.spec_rdf_raw.load() != 0;
    e->spec.rdf_norm = g_opt.spec_rdf_norm.load();
    e->spec.dist_geometric_com = g_opt.spec_dist_geometric_com.load() != 0;
    e->spec.angle_radians = g_opt.spec_angle_radians.load() != 0;
    e->spec.within_closed = g_opt.spec_within_closed.load() != 0;
    e->spec.within_exclude_ref = g_opt.spec_within_exclude_ref.load() != 0;
    e->spec.shell_norm = g_opt.spec_shell_norm.load() != 0;
    e->spec.rama_skip_ends = g_opt.spec_rama_skip_ends.load() != 0;
    e->ss_scratch_bytes = (size_t)std::max(0, g_opt.ss_scratch_bytes.load());
    e->frame_mask.assign(num_frames, 0);
    for (auto& p : ir->props) {
        auto st = std::make_unique<PropState>();
        st->prop = p;
        memset(&st->data, 0, sizeof(st->data));
        memset(&st->aggregate, 0, sizeof(st->aggregate));
        const FormFacts& f = p.facts();
        st->data.unit_str[0] = f.unit[0];
        st->data.unit_str[1] = e->spec.angle_radians && f.unit_y_radians ? f.unit_y_radians : f.unit[1];     // DESIGN S6b, D-ANGLE-UNIT
        bool aggregate = true;      // a temporal population has one
        if (p.temporal()) st->dist_P = p.aoff.size() - 1;     // the contexts (a table: its segments, below)
        // the 8 + 17 MB host views of a volume (a map: 4 + 8 MB) are pinned: their D2H refresh runs at PCIe speed
        auto pinned_views = [&](size_t n) { st->ncounts = n; st->values.assign(n, 0.0f, true); st->counts.assign(n, 0, true);
                                            st->pinned = st->values.pinned && st->counts.pinned; };
        auto largest_set = [&]() { int n = 0; for (size_t c = 0; c + 1 < p.aoff.size(); ++c) n = std::max(n, (int)(p.aoff[c + 1] - p.aoff[c])); return n; };
        switch (p.form) {
        case Form::RDF:
            st->ncounts = VMD_RDF_NUM_BINS;
            st->values.assign(st->ncounts, 0.0f); st->weights.assign(st->ncounts, 0.0f);
            st->counts.assign(st->ncounts, 0); st->weights64.assign(st->ncounts, 0.0);
            st->data.dim[0] = 1; st->data.dim[1] = 1; st->data.dim[2] = (int32_t)st->ncounts; st->data.dim[3] = 0;
            st->data.weights = st->weights.data();
            st->data.weights64 = st->weights64.data();
            st->data.min_range[0] = p.rmin; st->data.max_range[0] = p.rmax;
            st->same_set = (p.a == p.b);         // selections are interned by build_rdf_plan (own sets, or the classes they split into)
            break;
        case Form::SDF:
            pinned_views((size_t)VMD_VOLUME_DIM * VMD_VOLUME_DIM * VMD_VOLUME_DIM);
            st->data.dim[0] = 1; st->data.dim[1] = st->data.dim[2] = st->data.dim[3] = VMD_VOLUME_DIM;
            st->data.min_range[0] = -p.rmax; st->data.max_range[0] = p.rmax;
            break;
        case Form::RAMA_MAP:
            // the class map behind the angle table; pinned views like a volume's (4 + 8 MB)
            pinned_views((size_t)VMD_RAMA_DIM * VMD_RAMA_DIM * VMD_RAMA_CLASSES);
            st->data.dim[0] = 1; st->data.dim[1] = VMD_RAMA_CLASSES; st->data.dim[2] = st->data.dim[3] = VMD_RAMA_DIM;
            st->data.min_range[0] = -(float)M_PI; st->data.max_range[0] = (float)M_PI;
            break;
        case Form::RAMA_TABLE:
            // {phi, psi} per segment; no aggregate (VIAMD's table has none); the whole table lives on the device
            st->dist_P = p.a.size(); st->dist_per = 2;
            aggregate = false;
            if (!st->d_table.ensure(num_frames * 2 * p.a.size())) return nullptr;
            if (hipMemsetAsync(st->d_table.p, 0, num_frames * 2 * p.a.size() * sizeof(float), e->stream) != hipSuccess) {
                vmd_fail("hipMemset failed"); return nullptr; }
            break;
        case Form::MSD_TABLE:
            // x, y, z of every atom and the cell, 12 n + 36 bytes per frame; no aggregate (a mean of coordinates over atoms is
            // not what the table is for); the whole table lives on the device, as the angle table does
            st->dist_P = 3 * p.a.size() + VMD_MSD_CELL_FLOATS; st->dist_per = 1;
            aggregate = false;
            if (!st->d_table.ensure(num_frames * st->dist_P)) return nullptr;
            if (hipMemsetAsync(st->d_table.p, 0, num_frames * st->dist_P * sizeof(float), e->stream) != hipSuccess) {
                vmd_fail("hipMemset failed"); return nullptr; }
            break;
        // one code per segment, nine counts per frame; no aggregate (a mean of class codes says nothing)
        case Form::SS_CLASS: st->dist_P = p.a.size(); aggregate = false; break;
        case Form::SS_POP: st->dist_P = VMD_SS_NUM_CODES; aggregate = false; break;
        case Form::DISTANCE: st->dist_per = p.distance_kind == VMD_DISTANCE_PAIR ? (size_t)p.aoff[1] * (size_t)p.boff[1] : 1; break;
        case Form::ANGLE: case Form::DIHEDRAL: case Form::WITHIN: case Form::WITHIN_EXPR: case Form::HBOND_COUNT: case Form::SASA_AREA:
        case Form::CONTACT_COUNT: case Form::CLUSTER_COUNT: break;
        case Form::CONTACT_NATIVE: st->dist_P = 1; break;       // one fraction per frame (the descriptor carries no set)
        case Form::CLUSTER_LARGEST: st->dist_P = 1; break;      // one size per frame (likewise)
        case Form::CLUSTER_SIZES:
            // one u64 word per cluster size 1 .. G and the frame count; the float view is the words as numbers
            pinned_views(p.K + 1);
            st->data.dim[0] = (int32_t)(p.K + 1); st->data.dim[1] = 1; st->data.dim[2] = st->data.dim[3] = 0;
            break;
        case Form::CONTACT_OCC:
            // one u64 word per group pair and the frame count (16 MB at 2048 groups); the float view is the words as numbers
            pinned_views(p.K + 1);
            st->data.dim[0] = (int32_t)(p.K + 1); st->data.dim[1] = 1; st->data.dim[2] = st->data.dim[3] = 0;
            break;
        case Form::SASA_OCC:
            // one u64 word per measured entry and the frame count; the float view is the words as numbers, as a map's
            pinned_views(p.K + 1);
            st->data.dim[0] = (int32_t)(p.K + 1); st->data.dim[1] = 1; st->data.dim[2] = st->data.dim[3] = 0;
            break;
        case Form::HBOND_OCC:
            // one u64 word per donor pair, per acceptor, and the frame count; the float view is the words as numbers, as a map's
            pinned_views(p.K + p.m + 1);
            st->data.dim[0] = (int32_t)(p.K + p.m + 1); st->data.dim[1] = 1; st->data.dim[2] = st->data.dim[3] = 0;
            break;
        case Form::SHAPE: st->shape_max_set = largest_set(); break;
        case Form::RMSD: st->rmsd_max_set = largest_set(); break;
        case Form::RMSF: {
            // four u64 words per entry of the set and the row of the frame count; the float view is the words as numbers, as a
            // map's.  An rmsd property in front of it over the same sets lends it pose, sums and chunk shifts
            st->rmsd_max_set = largest_set();
            st->dist_P = p.aoff.size() - 1;
            st->rmsf_groups = std::max(0, g_opt.rmsf_frame_groups.load());
            pinned_views((p.a.size() + 1) * 4);
            st->data.dim[0] = (int32_t)(p.a.size() + 1); st->data.dim[1] = 4; st->data.dim[2] = st->data.dim[3] = 0;
            for (size_t j = 0; j < e->props.size(); ++j) {
                const Property& o = e->props[j]->prop;
                if (o.form == Form::RMSD && o.a == p.a && o.aoff == p.aoff) { st->rmsf_of = (int)j; break; }
            }
            break;
        }
        }
        if (p.temporal()) {     // [num_frames][contexts x values per context]
            st->dim1 = st->dist_P * st->dist_per;
            st->values.assign(num_frames * st->dim1, 0.0f);
            st->data.dim[0] = (int32_t)num_frames; st->data.dim[1] = (int32_t)st->dim1;
            if (aggregate && st->dim1 > 1) {
                st->agg_mean.assign(num_frames, 0.0f); st->agg_var.assign(num_frames, 0.0f); st->agg_ext.assign(num_frames * 2, 0.0f);
                st->aggregate.num_values = num_frames;
                st->aggregate.population_mean = st->agg_mean.data();
                st->aggregate.population_var = st->agg_var.data();
                st->aggregate.population_ext = (float(*)[2])st->agg_ext.data();
                st->data.aggregate = &st->aggregate;
            }
        }
        st->data.values = st->values.data();
        st->data.num_values = st->values.size();
        st->data.counts = st->counts.empty() ? nullptr : st->counts.data();
        st->data.fingerprint = 1;
        if (st->ncounts) {
            if (!st->d_counts.ensure(st->ncounts)) return nullptr;
            if (hipMemsetAsync(st->d_counts.p, 0, st->ncounts * sizeof(uint64_t), e->stream) != hipSuccess) { vmd_fail("hipMemset failed");
                    return nullptr; }
        }
        e->props.push_back(std::move(st));
    }
    build_rdf_plan(e.get());
    build_within_plan(e.get());
    build_neighbour_plan(e.get());
    build_expr_plan(e.get());
    if (!e->d_overflow.ensure(1) || hipMemsetAsync(e->d_overflow.p, 0, sizeof(uint32_t), e->stream) != hipSuccess ||
        pool_take(kPinned, (void**)&e->h_overflow, 2 * sizeof(uint32_t)) != hipSuccess) { vmd_fail("allocating the overflow flag failed");
                return nullptr; }
    e->h_overflow[0] = e->h_overflow[1] = 0;
    for (auto& ev : e->batch_done) if (!(ev = pool_event(false))) { vmd_fail("hipEventCreate failed"); return nullptr; }
    if (hipStreamSynchronize(e->stream) != hipSuccess) { vmd_fail("hipStreamSynchronize failed"); return nullptr; }
    return e.release();
}

extern "C" void vmd_eval_free(vmd_script_eval_t* eval) {
    if (!eval) return;
    VMD_STAGE("vmd_eval_free");
    lone_stop(eval);                     // the helper thread of a deferred-settle eval finishes what it is doing and ends
    int prev_dev = 0;
    (void)hipGetDevice(&prev_dev);
    (void)hipSetDevice(eval->device);
    {
        std::lock_guard<std::mutex> l(eval->mtx);
        // everything this eval ever queued ran on its own streams: once they are idle its blocks, streams and events can go back to
        // the process-wide cache without another synchronisation (PoolIdle)
        if (eval->stream) { (void)hipStreamSynchronize(eval->stream); }
        if (eval->copy_stream) { (void)hipStreamSynchronize(eval->copy_stream); }
        if (eval->aux_stream) { (void)hipStreamSynchronize(eval->aux_stream); }
        if (eval->pair_stream) { (void)hipStreamSynchronize(eval->pair_stream); }
        for (auto& ds : eval->decode_streams) { if (ds) { (void)hipStreamSynchronize(ds); pool_stream_give(ds, true); } ds = nullptr; }
        eval->decode_stream = nullptr;
        PoolIdle idle;
        for (auto& rs : eval->raw_slots) {
            if (rs.h) pool_give(rs.h);
            rs.h = nullptr;
            rs.d.release();
            pool_event_give(rs.uploaded, false);
            rs.uploaded = nullptr;
        }
        for (auto& st : eval->stages) {
            if (st.h) pool_give(st.h);
            st.h = nullptr;
            if (st.hraw) pool_give(st.hraw);
            st.hraw = nullptr;
            if (st.h_raw_status) pool_give(st.h_raw_status);
            st.h_raw_status = nullptr;
            st.d.release(); st.d_boxes.release(); st.d_bbox.release(); st.d_gboxes.release();
            st.d_raw.release(); st.d_raw_info.release(); st.d_raw_status.release(); st.d_raw_scratch.release();
            pool_event_give(st.ready, true);
            st.ready = nullptr;
        }
        pool_stream_give(eval->copy_stream, false); eval->copy_stream = nullptr;
        pool_stream_give(eval->aux_stream, false); eval->aux_stream = nullptr;
        pool_stream_give(eval->pair_stream, false); eval->pair_stream = nullptr;
        pool_event_give(eval->pair_fork, false); pool_event_give(eval->pair_join, false);
        eval->pair_fork = eval->pair_join = nullptr;
        eval->props.clear();
        eval->sels.clear();
        if (eval->h_overflow) pool_give(eval->h_overflow);
        eval->h_overflow = nullptr;
        if (eval->h_snap) pool_give(eval->h_snap);
        eval->h_snap = nullptr;
        for (auto& ev : eval->batch_done) { pool_event_give(ev, false); ev = nullptr; }
        eval->d_partial.release(); eval->d_partial2.release(); eval->d_pass.release(); eval->d_overflow.release();
                eval->d_pen_sample.release();
        pool_stream_give(eval->stream, false);
        eval->stream = nullptr;
    }
    {
        PoolIdle idle;              // whatever the destructors still hold (the profilers' events, the remaining buffers)
        delete eval;
    }
    (void)hipSetDevice(prev_dev);
}

extern "C" void vmd_eval_clear_data(vmd_script_eval_t* eval) {
    VMD_STAGE("vmd_eval_clear_data");
    if (!eval) return;
    lone_cancel(eval);                   // a deferred settle of the evaluation that ends here must neither start nor be running
    std::lock_guard<std::mutex> l(eval->mtx);
    eval->interrupt = false;
    for (size_t f = 0; f < eval->frame_mask.size(); ++f) mask_set(eval->frame_mask, f, 0);
    eval->frames_done = 0;
    eval->frames_computed = 0; eval->frames_reused = 0; eval->frames_device_decoded = 0; eval->frames_section_decoded = 0;
            eval->frames_mapped = 0;
    for (size_t b = 0; b < eval->num_blocks; ++b) eval->block_ready[b] = 0;
    eval->blocks_inst = TrajId();
    ra_reset(eval);
    for (auto& p : eval->props) {
        // The float view of a volume (8.4 MB, pinned) is NOT zeroed: `data.values` is pointed at a shared, read-only page range of zeros
        // until the next view of this evaluation has been written - k_counts_to_float rewrites every voxel of the real view, then the
        // pointer flips back (refresh_volume).  Round 6: the zeroing was a second 8.4 MB pass over PCIe per
        // evaluation - 0.15 ms that the kernel trace showed IN FRONT of the evaluation's kernels, not under them
        // (profiles/r06a_c4_1250_timeline.txt) - a fifth of a rank's 1 250-frame share of configs[3].  A reader polling `fingerprint`
        // (src/main.cpp:1508; density_volume.cpp:159-163, 279-283) sees zeros under the new fingerprint at once, never the previous run's
        // voxels; VIAMD dereferences prop_data->values when it uploads.
        if (p->prop.cls() == ResultClass::VOLUME) {
            float* zeros = zero_volume_view(p->ncounts);
            if (zeros) pub(p->data.values, zeros);
            else {      // no address space for the shared zeros: zero the view itself, as before round 6 (never a NULL `values`)
                std::fill(p->values.begin(), p->values.end(), 0.0f);
                pub(p->data.values, p->values.data());
            }
        }
        else std::fill(p->values.begin(), p->values.end(), 0.0f);
        std::fill(p->weights.begin(), p->weights.end(), 0.0f);
        // the 17 MB u64 mirror of a volume is only ever read after vmd_eval_refresh_counts: mark it stale instead of zeroing it
        if (p->prop.cls() == ResultClass::VOLUME) p->counts_stale = true;
        else std::fill(p->counts.begin(), p->counts.end(), (uint64_t)0);
        std::fill(p->weights64.begin(), p->weights64.end(), 0.0);
        std::fill(p->agg_mean.begin(), p->agg_mean.end(), 0.0f);
        std::fill(p->agg_var.begin(), p->agg_var.end(), 0.0f);
        std::fill(p->agg_ext.begin(), p->agg_ext.end(), 0.0f);
        if (p->ncounts) (void)hipMemsetAsync(p->d_counts.p, 0, p->ncounts * sizeof(uint64_t), eval->stream);
        if (p->prop.device_table()) {
            (void)hipMemsetAsync(p->d_table.p, 0, p->values.size() * sizeof(float), eval->stream);
            p->table_stale = false;
        }
        pub(p->data.max_value, 0.0f); pub(p->data.min_value, 0.0f);
        pub(p->data.max_range[1], 0.0f);
        p->dirty = false;
        if (p->prop.cls() != ResultClass::VOLUME) p->counts_stale = false;
        pub_touch(p->data.fingerprint);
    }
    (void)hipStreamSynchronize(eval->stream);
}

extern "C" void vmd_eval_interrupt(vmd_script_eval_t* eval) {
    if (!eval) return;
    eval->interrupt = true;
    // deferred-settle mode: a settle that is owed is dropped, one that is running ends at its next batch boundary - and has ended when this
    // returns: VIAMD resets the arena that holds molecule and trajectory right after interrupt_async_tasks (src/viamd.cpp:234-241, 624-630)
    if (eval->ra.lone.load()) lone_cancel(eval);
}

extern "C" uint64_t vmd_eval_ir_fingerprint(const vmd_script_eval_t* eval) { return eval ? eval->ir_fingerprint : 0; }

extern "C" const vmd_script_property_data_t* vmd_eval_property_data(const vmd_script_eval_t* eval, const char* name) {
    PropState* p = find_prop(eval, name);
    return p ? &p->data : nullptr;
}

extern "C" const uint8_t* vmd_eval_frame_mask(const vmd_script_eval_t* eval) { return eval ? eval->frame_mask.data() : nullptr; }

extern "C" size_t vmd_eval_frame_mask_bits(const vmd_script_eval_t* eval, uint64_t* words, size_t cap) {
    if (!eval) return 0;
    const size_t nw = (eval->num_frames + 63) / 64;
    for (size_t w = 0; w < nw && w < cap && words; ++w) {
        uint64_t v = 0;
        const size_t f1 = std::min(eval->num_frames, (w + 1) * 64);
        for (size_t f = w * 64; f < f1; ++f) if (mask_get(eval->frame_mask, f)) v |= 1ull << (f & 63);
        words[w] = v;
    }
    return nw;
}

extern "C" size_t vmd_eval_num_frames(const vmd_script_eval_t* eval) { return eval ? eval->num_frames : 0; }

extern "C" size_t vmd_eval_frames_done(const vmd_script_eval_t* eval) { return eval ? eval->frames_done.load() : 0; }

// ---- host views -------------------------------------------------------------------------------------------------
// the float views of a distribution from integer counts and fp64 weights (the device accumulators, or a snapshot of them)
void refresh_distribution_from(PropState* p, const uint64_t* counts, const double* weights64) {
    float ymax = 0.0f, vmax = 0.0f;
    for (size_t b = 0; b < p->ncounts; ++b) {
        p->counts[b] = counts[b];
        const float v = (float)counts[b];
        const float w = (float)weights64[b];
        p->values[b] = v; p->weights[b] = w;
        vmax = std::max(vmax, v);
        if (w > 0.0f) ymax = std::max(ymax, v / w);
    }
    pub(p->data.min_value, 0.0f); pub(p->data.max_value, vmax);
    pub(p->data.min_range[1], 0.0f); pub(p->data.max_range[1], ymax);
    pub_touch(p->data.fingerprint);
}

bool refresh_distribution(vmd_script_eval_t* e, PropState* p) {
    HIP_OK(hipMemcpyAsync(p->counts.data(), p->d_counts.p, p->ncounts * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    float ymax = 0.0f, vmax = 0.0f;
    for (size_t b = 0; b < p->ncounts; ++b) {
        const float v = (float)p->counts[b];
        const float w = (float)p->weights64[b];
        p->values[b] = v; p->weights[b] = w;
        vmax = std::max(vmax, v);
        if (w > 0.0f) ymax = std::max(ymax, v / w);
    }
    pub(p->data.min_value, 0.0f); pub(p->data.max_value, vmax);
    pub(p->data.min_range[1], 0.0f); pub(p->data.max_range[1], ymax);
    pub_touch(p->data.fingerprint);
    p->dirty = false;
    return true;
}

bool refresh_volume(vmd_script_eval_t* e, PropState* p) {
    VMD_STAGE("refresh_volume: counts -> float view, D2H");
    if (!p->d_max.ensure(1)) return false;
    float scale = 1.0f;
    if (p->prop.form == Form::SDF && e->spec.sdf_density) {
        // DECISION(D-SDF-NORM) flipped: number density per cubic Angstrom, averaged over the frames evaluated so far
        const double edge = 2.0 * (double)p->prop.rmax / (double)VMD_VOLUME_DIM;
        const size_t nf = e->frames_done.load();
        scale = nf ? (float)(1.0 / ((double)nf * edge * edge * edge)) : 0.0f;
    }
    float vmax = 0.0f;
    float* host_view_dev = nullptr;
    if (g_opt.sdf_direct_view.load() && p->values.pinned && hipHostGetDevicePointer((void**)&host_view_dev, p->values.data(),
            0) != hipSuccess) {
        (void)hipGetLastError();
        host_view_dev = nullptr;
    }
    if (host_view_dev) {
        // the conversion kernel writes the float view VIAMD reads straight into its pinned host pages (8.4 MB over PCIe at the
        // DMA's rate): no device-side copy of the view, no separate DMA behind the kernel
        KRN_OK(vmd_hip_counts_to_float(e->stream, p->d_counts.p, p->ncounts, host_view_dev, p->d_max.p, scale));
    } else {
        if (!p->d_values.ensure(p->ncounts)) return false;
        KRN_OK(vmd_hip_counts_to_float(e->stream, p->d_counts.p, p->ncounts, p->d_values.p, p->d_max.p, scale));
        HIP_OK(hipMemcpyAsync(p->values.data(), p->d_values.p, p->ncounts * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    }
    // the 17 MB u64 mirror behind `counts` is an extension VIAMD never reads: it is synchronised on demand
    // (vmd_eval_refresh_counts), only the float view travels after every range
    p->counts_stale = true;
    HIP_OK(hipMemcpyAsync(&vmax, p->d_max.p, sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    // every voxel of the real view has just been rewritten: readers leave the shared zeros (clear_data)
    pub(p->data.values, p->values.data());
    pub(p->data.min_value, 0.0f); pub(p->data.max_value, vmax);
    pub_touch(p->data.fingerprint);
    p->dirty = false;
    return true;
}

void refresh_temporal_stats(vmd_script_eval_t* e, PropState* p) {
    float lo = 3.4e38f, hi = -3.4e38f;
    bool any = false;
    for (size_t f = 0; f < e->num_frames; ++f) {
        if (!e->frame_mask[f]) continue;
        const float* row = &p->values[f * p->dim1];
        float rlo = row[0], rhi = row[0];
        double s = 0.0;
        for (size_t i = 0; i < p->dim1; ++i) { rlo = std::min(rlo, row[i]); rhi = std::max(rhi, row[i]); s += row[i]; }
        if (p->dim1 > 1 && !p->agg_mean.empty()) {      // (a ramachandran table keeps no aggregate)
            const double mean = s / (double)p->dim1;
            double v = 0.0;
            for (size_t i = 0; i < p->dim1; ++i) { const double d = row[i] - mean; v += d * d; }
            p->agg_mean[f] = (float)mean;
            p->agg_var[f] = (float)std::sqrt(v / (double)p->dim1);   // VIAMD plots mean +- var as a band (src/main.cpp:1409-1424)
            p->agg_ext[2 * f] = rlo; p->agg_ext[2 * f + 1] = rhi;
        }
        lo = std::min(lo, rlo); hi = std::max(hi, rhi);
        any = true;
    }
    if (!any) { lo = hi = 0.0f; }
    pub(p->data.min_value, lo); pub(p->data.max_value, hi);
    pub(p->data.min_range[0], lo); pub(p->data.max_range[0], hi);
    pub_touch(p->data.fingerprint);
    p->dirty = false;
}

// brings the host view of one property up to date, by what a host reads of it
bool refresh_view(vmd_script_eval_t* e, PropState* p) {
    switch (p->prop.cls()) {
    case ResultClass::DISTRIBUTION: return refresh_distribution(e, p);
    case ResultClass::VOLUME: case ResultClass::MAP: return refresh_volume(e, p);
    case ResultClass::TEMPORAL: refresh_temporal_stats(e, p); return true;
    }
    return true;
}

extern "C" bool vmd_eval_defer_volume_views(vmd_script_eval_t* eval, bool defer) {
    if (!eval) return vmd_fail("eval is NULL");
    eval->defer_volume_views.store(defer, std::memory_order_relaxed);
    return true;
}

extern "C" bool vmd_eval_finalize(vmd_script_eval_t* eval) {
    if (!eval) return vmd_fail("eval is NULL");
    if (!vmd_eval_wait_settled(eval)) return false;       // deferred-settle evals: the totals first
    std::lock_guard<std::mutex> l(eval->mtx);
    HIP_OK(hipSetDevice(eval->device));
    for (auto& p : eval->props) {
        const bool ok = refresh_view(eval, p.get());
        // rows of other ranks may have joined the host table (vmd_eval_reduce): the device copy follows before the next filtered map
        if (p->prop.device_table()) p->table_stale = true;
        if (!ok) return false;
    }
    return true;
}

extern "C" bool vmd_eval_refresh_counts(vmd_script_eval_t* eval, const char* name) {
    PropState* p = find_prop(eval, name);
    if (!p) return vmd_fail("vmd_eval_refresh_counts: no property '%s'", name ? name : "(null)");
    std::lock_guard<std::mutex> l(eval->mtx);
    if (!p->counts_stale || !p->ncounts) return true;
    HIP_OK(hipSetDevice(eval->device));
    HIP_OK(hipMemcpyAsync(p->counts.data(), p->d_counts.p, p->ncounts * sizeof(uint64_t), hipMemcpyDeviceToHost, eval->stream));
    HIP_OK(hipStreamSynchronize(eval->stream));
    p->counts_stale = false;
    return true;
}

extern "C" bool vmd_eval_set_block_frames(vmd_script_eval_t* eval, size_t block_frames) {
    if (!eval) return vmd_fail("eval is NULL");
    std::lock_guard<std::mutex> l(eval->mtx);
    HIP_OK(hipSetDevice(eval->device));
    if (eval->frames_done.load() != 0)
        return vmd_fail("vmd_eval_set_block_frames: call before the first frame_range or right after clear_data");
    // read-ahead re-engages on the new blocks
    eval->ra.on = false; eval->ra.own_blocks = false; eval->ra.blk_state.reset(); eval->ra.frame_req.reset();
    eval->block_frames = 0; eval->num_blocks = 0; eval->block_ready.reset();
    for (auto& p : eval->props) { p->d_blocks.release(); p->block_weights64.clear(); }
    if (block_frames == 0) return true;
    const size_t nblocks = (eval->num_frames + block_frames - 1) / block_frames;
    size_t bytes = 0;
    for (auto& p : eval->props) bytes += nblocks * p->ncounts * sizeof(uint64_t);
    if (bytes > ((size_t)96 << 30))
        return vmd_fail("vmd_eval_set_block_frames: %zu blocks need %.1f GB of block partials; use larger blocks", nblocks,
                (double)bytes / 1073741824.0);
    for (auto& p : eval->props) {
        if (!p->ncounts) continue;
        if (!p->d_blocks.ensure(nblocks * p->ncounts)) return false;
        if (p->prop.cls() == ResultClass::DISTRIBUTION) p->block_weights64.assign(nblocks * p->ncounts, 0.0);
    }
    eval->block_ready.reset(new std::atomic<uint8_t>[nblocks]);
    for (size_t b = 0; b < nblocks; ++b) eval->block_ready[b] = 0;
    eval->num_blocks = nblocks;
    eval->block_frames = block_frames;
    return true;
}

extern "C" bool vmd_eval_set_source(vmd_script_eval_t* eval, vmd_script_eval_t* source) {
    if (!eval) return vmd_fail("eval is NULL");
    std::lock_guard<std::mutex> l(eval->mtx);
    if (!source) { eval->source = nullptr; return true; }
    if (source == eval) return vmd_fail("vmd_eval_set_source: an eval cannot be its own source");
    if (source->ir_fingerprint != eval->ir_fingerprint || source->num_frames != eval->num_frames
            || source->props.size() != eval->props.size())
        return vmd_fail("vmd_eval_set_source: source was created from a different script or frame count");
    if (source->device != eval->device) return vmd_fail("vmd_eval_set_source: source lives on another device");
    // (a source without block partials is accepted since round 4: read-ahead gives an eval driven by pool threads block partials of its own
    // accord, and whether the source has any is looked up, under its mutex, whenever a range is served)
    eval->source = source;
    return true;
}

extern "C" size_t vmd_eval_frames_device_decoded(const vmd_script_eval_t* eval) { return eval ? eval->frames_device_decoded.load() : 0; }

extern "C" size_t vmd_eval_frames_section_decoded(const vmd_script_eval_t* eval) { return eval ? eval->frames_section_decoded.load() : 0; }

extern "C" size_t vmd_eval_frames_mapped(const vmd_script_eval_t* eval) { return eval ? eval->frames_mapped.load() : 0; }

extern "C" void vmd_eval_cell_build_stats(const vmd_script_eval_t* eval, size_t* bucket_overflows, size_t* selections_off_buckets) {
    size_t ov = 0, off = 0;
    if (eval) for (auto& s : eval->sels) { ov += (size_t)std::min(s->overflows, 98); off += s->overflows >= 3 ? 1 : 0; }
    if (bucket_overflows) *bucket_overflows = ov;
    if (selections_off_buckets) *selections_off_buckets = off;
}

extern "C" void vmd_eval_frame_stats(const vmd_script_eval_t* eval, size_t* frames_computed, size_t* frames_reused) {
    if (frames_computed) *frames_computed = eval ? eval->frames_computed.load() : 0;
    if (frames_reused) *frames_reused = eval ? eval->frames_reused.load() : 0;
}

extern "C" void vmd_eval_set_frame_mask(vmd_script_eval_t* eval, const uint8_t* mask, size_t n) {
    if (!eval || !mask) return;
    std::lock_guard<std::mutex> l(eval->mtx);
    size_t done = 0;
    for (size_t f = 0; f < eval->num_frames; ++f) {
        if (f < n) mask_set(eval->frame_mask, f, mask[f] ? 1 : 0);
        done += eval->frame_mask[f] ? 1 : 0;
    }
    eval->frames_done = done;
    for (auto& p : eval->props) if (p->prop.device_table()) p->table_stale = true;     // frames evaluated elsewhere: their rows are on the host
}

extern "C" size_t vmd_eval_accum_views(vmd_script_eval_t* eval, vmd_accum_view_t* out, size_t cap) {
    if (!eval) return 0;
    size_t n = 0;
    for (auto& p : eval->props) {
        if (n < cap && out) {
            vmd_accum_view_t v;
            memset(&v, 0, sizeof(v));
            v.name = p->prop.name.c_str();
            v.flags = p->prop.flags();
            if (p->ncounts) { v.counts_dev = p->d_counts.p; v.num_counts = p->ncounts; }
            // a voxel receives at most one count per (frame, structure, target atom), a bin of a map one per (frame, segment)
            if (p->prop.counts_view()) {
                // (a donor row at most one count per acceptor and frame, an acceptor row one per pair)
                // (a row at most npoints per frame)
                // (a pair is in contact in a frame or it is not)
                // (a frame has at most G clusters, of whatever size)
                const long double per_frame = p->prop.form == Form::CONTACT_OCC ? 1.0L
                        : p->prop.form == Form::CLUSTER_SIZES ? (long double)p->prop.K
                        : p->prop.form == Form::SASA_OCC ? (long double)p->prop.m
                        : p->prop.form == Form::HBOND_OCC ? (long double)std::max(p->prop.K, p->prop.m)
                        : (long double)p->prop.K * (p->prop.form == Form::SDF ? (long double)p->prop.b.size() : 1.0L);
                const long double b = (long double)eval->num_frames * per_frame;
                v.count_bound = b < 1.8e19L ? (uint64_t)b : 0;
            }
            if (!p->weights64.empty()) { v.weights64 = p->weights64.data(); v.num_weights = p->weights64.size(); }
            if (p->prop.temporal()) { v.temporal = p->values.data(); v.num_temporal = p->values.size(); }
            out[n] = v;
        }
        n += 1;
    }
    return n;
}

// hooks for vmd_reduce.cpp (same library, not part of the public headers)
extern "C" int vmd_eval_internal_device(const vmd_script_eval_t* eval) { return eval ? eval->device : 0; }

extern "C" void vmd_eval_internal_lock(vmd_script_eval_t* eval, int lock) { if (eval) { if (lock) eval->mtx.lock();
        else eval->mtx.unlock(); } }

extern "C" vmd_reduce_stats_t* vmd_eval_internal_reduce_stats(vmd_script_eval_t* eval) { return eval ? &eval->reduce_stats : nullptr; }

extern "C" void vmd_eval_reduce_stats(const vmd_script_eval_t* eval, vmd_reduce_stats_t* out) {
    if (!out) return;
    if (eval) *out = eval->reduce_stats; else memset(out, 0, sizeof(*out));
}

// ---- the filtered Ramachandran map: one zeroing, one k_rama_bin over the device table with the frame mask as the row mask,
// one copy-out.  Under the eval's mutex like vmd_eval_shell_mask, so it takes its turn between the batches of running calls; it writes only
// the table property's own scratch.
extern "C" bool vmd_eval_rama_density(vmd_script_eval_t* eval, const char* name, uint32_t frame_beg, uint32_t frame_end, float* values,
                                      uint64_t sums[4]) {
    if (!eval || !name) return vmd_fail("vmd_eval_rama_density: NULL argument");
    vmd_script_eval_t* e = eval;
    size_t mi = e->props.size();
    for (size_t i = 0; i < e->props.size(); ++i) if (e->props[i]->prop.name == name) mi = i;
    if (mi == e->props.size()) return vmd_fail("unknown property '%s'", name);
    if (e->props[mi]->prop.form != Form::RAMA_MAP || mi == 0 || e->props[mi - 1]->prop.form != Form::RAMA_TABLE)
        return vmd_fail("'%s' is not a ramachandran map", name);
    if (frame_beg < frame_end && frame_end > e->num_frames)
        return vmd_fail("frames [%u, %u) are outside the %zu frames of the evaluation", frame_beg, frame_end, e->num_frames);
    const size_t nmap = (size_t)VMD_RAMA_DIM * VMD_RAMA_DIM * VMD_RAMA_CLASSES;
    uint64_t s4[4] = {0, 0, 0, 0};
    if (frame_beg >= frame_end) {
        if (values) std::fill(values, values + nmap, 0.0f);
        if (sums) memcpy(sums, s4, sizeof(s4));
        return true;
    }
    PropState* t = e->props[mi - 1].get();
    std::lock_guard<std::mutex> lock(e->mtx);
    HIP_OK(hipSetDevice(e->device));
    // (a rank that has evaluated nothing itself still answers after a merge: the binning needs only the per-segment bytes)
    if (!t->uploaded && (!t->d_rama_class.upload(t->prop.rama_class.data(), t->prop.rama_class.size(), e->stream) ||
                         !t->d_rama_link.upload(t->prop.rama_link.data(), t->prop.rama_link.size(), e->stream))) return false;
    const size_t nseg = t->prop.a.size(), F = frame_end - frame_beg;
    if (!t->d_rama_scratch.ensure(nmap + 4) || !t->d_rama_mask.ensure(e->num_frames) || !t->d_values.ensure(nmap) || !t->d_max.ensure(1))
        return false;
    if (t->table_stale) {
        HIP_OK(hipMemcpyAsync(t->d_table.p, t->values.data(), t->values.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
        t->table_stale = false;
    }
    std::vector<uint8_t> mask(F);
    for (size_t f = 0; f < F; ++f) mask[f] = mask_get(e->frame_mask, frame_beg + f);
    HIP_OK(hipMemcpyAsync(t->d_rama_mask.p, mask.data(), F, hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipMemsetAsync(t->d_rama_scratch.p, 0, (nmap + 4) * sizeof(uint64_t), e->stream));
    // (rows beyond 2^31 - 1 entries per launch: in pieces)
    const size_t step = std::max<size_t>(1, (size_t)0x7fffffff / nseg);
    for (size_t f = 0; f < F; f += step) {
        const size_t nf = std::min(step, F - f);
        KRN_OK(vmd_hip_rama_bin(e->stream, t->d_table.p + (frame_beg + f) * 2 * nseg, (int)nf, t->d_rama_mask.p + f, (int)nseg,
                t->d_rama_class.p, t->d_rama_link.p, e->spec.rama_skip_ends ? 1 : 0, t->d_rama_scratch.p, t->d_rama_scratch.p + nmap));
    }
    if (values) {
        KRN_OK(vmd_hip_counts_to_float(e->stream, t->d_rama_scratch.p, nmap, t->d_values.p, t->d_max.p, 1.0f));
        HIP_OK(hipMemcpyAsync(values, t->d_values.p, nmap * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_OK(hipMemcpyAsync(s4, t->d_rama_scratch.p + nmap, sizeof(s4), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (sums) memcpy(sums, s4, sizeof(s4));
    return true;
}

// ---- mean-squared displacement over lag times: the time unwrap of the window (k_msd_unwrap), then the sums over origins and
// atoms per lag (k_msd_lags), from the position table the device holds.  Under the eval's mutex like the filtered map above; it writes only
// the table property's own scratch.  The profile (vmd_profile_ms) splits it into "msd_unwrap" and "msd_lags".
extern "C" bool vmd_eval_msd(vmd_script_eval_t* eval, const char* name, uint32_t frame_beg, uint32_t frame_end, uint32_t max_lag,
                             uint32_t origin_stride, uint64_t (*sums)[4], uint32_t* frames_used) {
    if (!eval || !name || !sums) return vmd_fail("vmd_eval_msd: NULL argument");
    vmd_script_eval_t* e = eval;
    PropState* t = nullptr;
    for (auto& p : e->props) if (p->prop.name == name) t = p.get();
    if (!t) return vmd_fail("unknown property '%s'", name);
    if (t->prop.form != Form::MSD_TABLE) return vmd_fail("'%s' is not an msd position table", name);
    if (frame_beg >= frame_end) return vmd_fail("vmd_eval_msd: the window [%u, %u) is empty or reversed", frame_beg, frame_end);
    if (frame_end > e->num_frames)
        return vmd_fail("frames [%u, %u) are outside the %zu frames of the evaluation", frame_beg, frame_end, e->num_frames);
    if (origin_stride == 0) return vmd_fail("vmd_eval_msd: the origin stride must be at least 1");
    const size_t F = frame_end - frame_beg, n = t->prop.a.size(), w = t->dim1;
    if (max_lag >= F) return vmd_fail("vmd_eval_msd: max_lag %u needs more than the %zu frames of the window", max_lag, F);
    if (F > (size_t)65535 * 32) return vmd_fail("vmd_eval_msd: a window of %zu frames exceeds the launch limit (%d)", F, 65535 * 32);
    std::lock_guard<std::mutex> lock(e->mtx);
    HIP_OK(hipSetDevice(e->device));
    // the unwrap needs consecutive frames: a gap is a refusal, not a guess
    for (size_t f = frame_beg; f < frame_end; ++f)
        if (!mask_get(e->frame_mask, f)) return vmd_fail("vmd_eval_msd: frame %zu of the window has not been evaluated", f);
    for (size_t f = frame_beg; f < frame_end; ++f) {
        const float* cell = t->values.data() + f * w + 3 * n;
        if (cell[6] != 0.0f || cell[7] != 0.0f || cell[8] != 0.0f)
            return vmd_fail("vmd_eval_msd: frame %zu has a triclinic cell (the time unwrap is defined for orthorhombic cells)", f);
    }
    if (!t->d_msd_counts.ensure(F * 3 * n) || !t->d_msd_sums.ensure(((size_t)max_lag + 1) * 4)) return false;
    if (t->table_stale) {
        HIP_OK(hipMemcpyAsync(t->d_table.p, t->values.data(), t->values.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
        t->table_stale = false;
    }
    const float* rows = t->d_table.p + (size_t)frame_beg * w;
    const size_t nsums = ((size_t)max_lag + 1) * 4;
    HIP_OK(hipMemsetAsync(t->d_msd_sums.p, 0, nsums * sizeof(uint64_t), e->stream));
    e->prof.begin("msd_unwrap", e->stream);
    KRN_OK(vmd_hip_msd_unwrap(e->stream, rows, (int)F, (int)n, t->d_msd_counts.p));
    e->prof.end(e->stream);
    e->prof.begin("msd_lags", e->stream);
    KRN_OK(vmd_hip_msd_lags(e->stream, rows, t->d_msd_counts.p, (int)F, (int)n, (int)max_lag, (int)std::min<uint32_t>(origin_stride, 0x7fffffffu),
            t->d_msd_sums.p));
    e->prof.end(e->stream);
    HIP_OK(hipMemcpyAsync(sums, t->d_msd_sums.p, nsums * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->prof.resolve();
    if (frames_used) *frames_used = (uint32_t)F;
    return true;
}

extern "C" size_t vmd_eval_msd_atoms(const vmd_script_eval_t* eval, const char* name) {
    PropState* p = find_prop(eval, name);
    return p && p->prop.form == Form::MSD_TABLE ? p->prop.a.size() : 0;
}

// ---- what the readers of the records and the one-frame calls share
// A record as it stands - a partial evaluation, a merged one - copied to the host: under the eval's mutex, touching nothing it keeps.
static bool read_record(vmd_script_eval_t* e, const PropState* p, std::vector<uint64_t>* acc) {
    acc->resize(p->ncounts);
    std::lock_guard<std::mutex> lock(e->mtx);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipMemcpyAsync(acc->data(), p->d_counts.p, p->ncounts * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return true;
}
// rows / frames, 0 where no frame has been counted
static void rows_over_frames(const uint64_t* rows, size_t n, uint64_t F, double* out) {
    if (out) for (size_t j = 0; j < n; ++j) out[j] = F ? (double)rows[j] / (double)F : 0.0;
}
// Any name of a statement names it: the count (form `count`) or a companion behind it, companions[k] standing k + 1 places behind ->
// the index of the count, or props.size() + vmd_last_error ("'name' is not <what> property")
static size_t count_statement(vmd_script_eval_t* e, const char* name, Form count, std::initializer_list<Form> companions, const char* what) {
    size_t pi = e->props.size();
    for (size_t i = 0; i < e->props.size(); ++i) if (e->props[i]->prop.name == name) pi = i;
    if (pi == e->props.size()) { vmd_fail("unknown property '%s'", name); return pi; }
    size_t k = 0;
    for (Form f : companions) { k += 1; if (e->props[pi]->prop.form == f && pi >= k) { pi -= k; break; } }
    if (e->props[pi]->prop.form != count) { vmd_fail("'%s' is not %s property", name, what); return e->props.size(); }
    return pi;
}
// One frame on demand: fn(src) with frame `frame` of traj fetched as a batch of one (boxes and pbc: e->stages[0]'s), under the eval's
// mutex, so that it takes its turn between the batches of running calls.  fn launches on e->stream and waits for what it reads back.
template <class Fn>
static bool on_one_frame(vmd_script_eval_t* e, const char* who, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame, Fn fn) {
    if (frame >= e->num_frames) return vmd_fail("%s: frame %u outside the trajectory (%zu frames)", who, frame, e->num_frames);
    std::lock_guard<std::mutex> lock(e->mtx);
    if (hipSetDevice(e->device) != hipSuccess) return vmd_fail("hipSetDevice failed");
    const size_t num_atoms = traj->num_atoms(traj->inst);
    if (!check_atoms(e, num_atoms) || !upload_static(e, sys, num_atoms)) return false;
    vmd_device_view_t view;
    memset(&view, 0, sizeof(view));
    const bool have_view = traj->device_view && traj->device_view(traj->inst, &view) && view.device == e->device;
    BatchSrc src;
    if (!fetch_batch(e, traj, view_holds(have_view, view, frame) ? &view : nullptr, num_atoms, frame, 1, &src)) return false;
    return fn(src);
}

// ---- rmsf read from its record: m = sum_q / (2^24 F) per axis, msf = sum_q2 / (2^24 F) - |m|^2 clamped at 0, rmsf = sqrt(msf).
// Whatever the record holds - a partial evaluation, a merged one - is what is read; under the eval's mutex, touching nothing it keeps.
extern "C" bool vmd_eval_rmsf(vmd_script_eval_t* eval, const char* name, double* rmsf, double* mean_dev, uint64_t* frames) {
    if (!eval || !name) return vmd_fail("vmd_eval_rmsf: NULL argument");
    PropState* p = find_prop(eval, name);
    if (!p) return vmd_fail("unknown property '%s'", name);
    if (p->prop.form != Form::RMSF) return vmd_fail("'%s' is not an rmsf property", name);
    const size_t ntot = p->prop.a.size();
    std::vector<uint64_t> acc;
    if (!read_record(eval, p, &acc)) return false;
    const uint64_t F = acc[4 * ntot];
    if (frames) *frames = F;
    const double scale = 16777216.0 * (double)F;
    for (size_t j = 0; j < ntot; ++j) {
        double m[3] = {0.0, 0.0, 0.0}, r = 0.0;
        if (F) {
            for (int k = 0; k < 3; ++k) m[k] = (double)(int64_t)acc[4 * j + k] / scale;
            const double msf = (double)acc[4 * j + 3] / scale - ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            r = std::sqrt(msf < 0.0 ? 0.0 : msf);
        }
        if (rmsf) rmsf[j] = r;
        if (mean_dev) for (int k = 0; k < 3; ++k) mean_dev[3 * j + k] = m[k];
    }
    return true;
}

// ---- hydrogen-bond occupancies read from their record: count / frames per donor pair and per acceptor.  Whatever the
// record holds - a partial evaluation, a merged one - is what is read; under the eval's mutex, touching nothing it keeps.
extern "C" bool vmd_eval_hbonds(vmd_script_eval_t* eval, const char* name, double* donor_occ, double* acc_occ, uint64_t* frames) {
    if (!eval || !name) return vmd_fail("vmd_eval_hbonds: NULL argument");
    PropState* p = find_prop(eval, name);
    if (!p) return vmd_fail("unknown property '%s'", name);
    if (p->prop.form != Form::HBOND_OCC) return vmd_fail("'%s' is not a hydrogen-bond occupancy", name);
    const size_t npairs = p->prop.K, nacc = p->prop.m;
    std::vector<uint64_t> acc;
    if (!read_record(eval, p, &acc)) return false;
    const uint64_t F = acc[npairs + nacc];
    if (frames) *frames = F;
    rows_over_frames(acc.data(), npairs, F, donor_occ);
    rows_over_frames(acc.data() + npairs, nacc, F, acc_occ);
    return true;
}

// The bonds of one frame.  One frame on demand, as vmd_eval_shell_mask: all pairs from the raw frame (for ONE frame the cell
// build and the identity pass a walk needs cost more than they save) into a capped list behind a counter, sorted on the host.  Nothing the
// evaluation keeps is touched: canon, counter and list live in one buffer of the eval that only this call uses (kept between calls).
extern "C" size_t vmd_eval_hbond_pairs(vmd_script_eval_t* eval, const char* name, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame,
                                       int32_t (*out)[3], size_t cap) {
    const size_t failed = VMD_HBOND_PAIRS_FAILED;
    if (!eval || !traj || !name || (!out && cap)) { vmd_fail("vmd_eval_hbond_pairs: NULL argument"); return failed; }
    vmd_script_eval_t* e = eval;
    const size_t pi = count_statement(e, name, Form::HBOND_COUNT, {Form::HBOND_OCC}, "a hydrogen-bond");
    if (pi == e->props.size()) return failed;
    PropState* p = e->props[pi].get();
    const Property& d = p->prop;
    const size_t npairs = d.a.size(), nacc = d.b.size();
    std::vector<uint32_t> list, canon_h(nacc);
    uint32_t found = 0;
    {
        auto run = [&](const BatchSrc& src) -> bool {
            // two passes at the most: the list is sized for what a caller asks for (and a fair share more), the second pass for what was found
            size_t room = std::min<size_t>(std::max<size_t>(cap, 4 * npairs), (size_t)0x3fffffff);
            for (int pass = 0; pass < 2; ++pass) {
                if (!e->d_one_hbonds.ensure(nacc + 1 + 2 * room)) return false;
                uint32_t* canon = e->d_one_hbonds.p;
                uint32_t* counter = canon + nacc;
                uint32_t* dl = counter + 1;
                KRN_OK(vmd_hip_hbond_list(e->stream, src.base, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), p->d_a.p,
                        p->d_c.p, (int)npairs, p->d_b.p, (int)nacc, canon, d.rmax, d.hb_c2, e->spec.within_closed ? 1 : 0, dl, (uint32_t)room,
                        counter));
                HIP_OK(hipMemcpyAsync(&found, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
                HIP_OK(hipStreamSynchronize(e->stream));
                if (found <= room) {
                    list.resize(2 * (size_t)found);
                    if (found) HIP_OK(hipMemcpyAsync(list.data(), dl, list.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
                    HIP_OK(hipMemcpyAsync(canon_h.data(), canon, nacc * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
                    HIP_OK(hipStreamSynchronize(e->stream));
                    return true;
                }
                if (found > 0x3fffffffu) return vmd_fail("vmd_eval_hbond_pairs: %u bonds in one frame", found);
                room = found;
            }
            return vmd_fail("vmd_eval_hbond_pairs: the frame's bonds changed between two passes");
        };
        if (!on_one_frame(e, "vmd_eval_hbond_pairs", sys, traj, frame, run)) return failed;
    }
    // ascending (pair index, acceptor list position); the appends arrive in no order.  The acceptor named is the entry that answers for
    // the position (D-HB-COINCIDENT)
    std::vector<uint64_t> keys(found);
    for (size_t i = 0; i < found; ++i) keys[i] = ((uint64_t)list[2 * i] << 32) | list[2 * i + 1];
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < found && i < cap; ++i) {
        const size_t j = (size_t)(keys[i] >> 32), k = (size_t)(keys[i] & 0xffffffffu);
        out[i][0] = d.a[j]; out[i][1] = d.c[j]; out[i][2] = d.b[canon_h[k]];
    }
    return found;
}

// ---- the mean accessible area per measured entry read from its record: count / frames * 4 pi R^2 / npoints in double.
// Whatever the record holds - a partial evaluation, a merged one - is what is read; under the eval's mutex, touching nothing it keeps.
extern "C" bool vmd_eval_sasa(vmd_script_eval_t* eval, const char* name, double* mean_area, uint64_t* frames) {
    if (!eval || !name) return vmd_fail("vmd_eval_sasa: NULL argument");
    size_t pi = eval->props.size();
    for (size_t i = 0; i < eval->props.size(); ++i) if (eval->props[i]->prop.name == name) pi = i;
    if (pi == eval->props.size()) return vmd_fail("unknown property '%s'", name);
    PropState* p = eval->props[pi].get();
    if (p->prop.form != Form::SASA_OCC || pi == 0 || eval->props[pi - 1]->prop.form != Form::SASA_AREA)
        return vmd_fail("'%s' is not a record of accessible surface points", name);
    if (!mean_area && !frames) return true;        // (asked for the form alone)
    const Property& d = eval->props[pi - 1]->prop;
    const size_t nmeas = p->prop.K;
    std::vector<uint64_t> acc;
    if (!read_record(eval, p, &acc)) return false;
    const uint64_t F = acc[nmeas];
    if (frames) *frames = F;
    if (mean_area)
        for (size_t i = 0; i < nmeas; ++i) {
            const double R = (double)(d.sasa_ra[i] + d.sasa_probe);
            mean_area[i] = F ? (double)acc[i] / (double)F * (4.0 * M_PI * R * R) / (double)d.sasa_npoints : 0.0;
        }
    return true;
}

// The accessible points of one frame.  One frame on demand, as vmd_eval_hbond_pairs: all pairs from the raw frame.  Nothing the
// evaluation keeps is touched: canon and counts live in one buffer of the eval that only this call uses (kept between calls).
extern "C" size_t vmd_eval_sasa_atoms(vmd_script_eval_t* eval, const char* name, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame,
                                      uint32_t* counts, size_t cap) {
    const size_t failed = VMD_SASA_ATOMS_FAILED;
    if (!eval || !traj || !name || (!counts && cap)) { vmd_fail("vmd_eval_sasa_atoms: NULL argument"); return failed; }
    vmd_script_eval_t* e = eval;
    const size_t pi = count_statement(e, name, Form::SASA_AREA, {Form::SASA_OCC}, "a sasa");
    if (pi == e->props.size()) return failed;
    PropState* p = e->props[pi].get();
    const Property& d = p->prop;
    const size_t nmeas = d.a.size(), nenv = d.b.size();
    std::vector<uint32_t> got(nmeas);
    {
        auto run = [&](const BatchSrc& src) -> bool {
            if (!e->d_one_sasa.ensure(nenv + nmeas)) return false;
            uint32_t* canon = e->d_one_sasa.p;
            uint32_t* dn = canon + nenv;
            KRN_OK(vmd_hip_sasa_list(e->stream, src.base, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), p->d_a.p, (int)nmeas,
                    p->d_b.p, (int)nenv, canon, p->d_sasa_ra.p, p->d_sasa_rb.p, p->sasa_rmax_env, p->d_sasa_pts.p, (int)d.sasa_npoints, d.rmax,
                    e->spec.within_closed ? 1 : 0, dn));
            HIP_OK(hipMemcpyAsync(got.data(), dn, nmeas * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            HIP_OK(hipStreamSynchronize(e->stream));
            return true;
        };
        if (!on_one_frame(e, "vmd_eval_sasa_atoms", sys, traj, frame, run)) return failed;
    }
    for (size_t i = 0; i < nmeas && i < cap; ++i) counts[i] = got[i];
    return nmeas;
}

// ---- contact maps.  Any name of the statement names it: -> the index of its count, or props.size() + vmd_last_error
static size_t contact_statement(vmd_script_eval_t* e, const char* name) {
    const size_t pi = count_statement(e, name, Form::CONTACT_COUNT, {Form::CONTACT_OCC, Form::CONTACT_NATIVE}, "a contacts");
    if (pi == e->props.size() || (pi + 1 < e->props.size() && e->props[pi + 1]->prop.form == Form::CONTACT_OCC)) return pi;
    vmd_fail("'%s' is not a contacts property", name);
    return e->props.size();
}

// count / frames per group pair, read from the record as it stands - a partial evaluation, a merged one; under the eval's mutex, touching
// nothing it keeps
extern "C" bool vmd_eval_contacts(vmd_script_eval_t* eval, const char* name, double* occupancy, uint64_t* frames) {
    if (!eval || !name) return vmd_fail("vmd_eval_contacts: NULL argument");
    const size_t pi = contact_statement(eval, name);
    if (pi == eval->props.size()) return false;
    if (!occupancy && !frames) return true;        // (asked for the form alone)
    PropState* p = eval->props[pi + 1].get();
    const size_t P = p->prop.K;
    std::vector<uint64_t> acc;
    if (!read_record(eval, p, &acc)) return false;
    if (frames) *frames = acc[P];
    rows_over_frames(acc.data(), P, acc[P], occupancy);
    return true;
}

// The group pairs in contact in one frame.  One frame on demand, as vmd_eval_hbond_pairs: all pairs from the raw frame into one row of
// bits, read back and listed on the host in ascending pair index.  Nothing the evaluation keeps is touched: canon and the row live in one
// buffer of the eval that only this call uses (kept between calls).
extern "C" size_t vmd_eval_contact_pairs(vmd_script_eval_t* eval, const char* name, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame,
                                         int32_t (*out)[2], size_t cap) {
    const size_t failed = VMD_CONTACT_PAIRS_FAILED;
    if (!eval || !traj || !name || (!out && cap)) { vmd_fail("vmd_eval_contact_pairs: NULL argument"); return failed; }
    vmd_script_eval_t* e = eval;
    const size_t pi = contact_statement(e, name);
    if (pi == e->props.size()) return failed;
    PropState* p = e->props[pi].get();
    const Property& d = p->prop;
    const size_t nent = d.a.size(), G = d.K, P = G * (G - 1) / 2, W = (P + 31) / 32;
    std::vector<uint32_t> row(W);
    {
        auto run = [&](const BatchSrc& src) -> bool {
            if (!e->d_one_contacts.ensure(nent + W)) return false;
            uint32_t* canon = e->d_one_contacts.p;
            uint32_t* bits = canon + nent;
            KRN_OK(vmd_hip_contact_brute(e->stream, src.base, 0, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), 1, p->d_a.p,
                    p->d_c.p, (int)nent, (int)G, d.ct_min_sep, canon, d.rmax, e->spec.within_closed ? 1 : 0, bits, nullptr));
            HIP_OK(hipMemcpyAsync(row.data(), bits, W * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            HIP_OK(hipStreamSynchronize(e->stream));
            return true;
        };
        if (!on_one_frame(e, "vmd_eval_contact_pairs", sys, traj, frame, run)) return failed;
    }
    size_t found = 0, pidx = 0;
    for (size_t g = 0; g + 1 < G; ++g)
        for (size_t h = g + 1; h < G; ++h, ++pidx)
            if ((row[pidx >> 5] >> (pidx & 31)) & 1u) {
                if (found < cap) { out[found][0] = (int32_t)g; out[found][1] = (int32_t)h; }
                found += 1;
            }
    return found;
}

// ---- clusters.  Any name of the statement names it: -> the index of its count, or props.size() + vmd_last_error
static size_t cluster_statement(vmd_script_eval_t* e, const char* name) {
    const size_t pi = count_statement(e, name, Form::CLUSTER_COUNT, {Form::CLUSTER_SIZES, Form::CLUSTER_LARGEST}, "a clusters");
    if (pi == e->props.size() || (pi + 1 < e->props.size() && e->props[pi + 1]->prop.form == Form::CLUSTER_SIZES)) return pi;
    vmd_fail("'%s' is not a clusters property", name);
    return e->props.size();
}

// the clusters of s groups per frame, row / frames, read from the record as it stands - a partial evaluation, a merged one; under the
// eval's mutex, touching nothing it keeps
extern "C" bool vmd_eval_cluster_sizes(vmd_script_eval_t* eval, const char* name, double* mean_count, uint64_t* frames) {
    if (!eval || !name) return vmd_fail("vmd_eval_cluster_sizes: NULL argument");
    const size_t pi = cluster_statement(eval, name);
    if (pi == eval->props.size()) return false;
    if (!mean_count && !frames) return true;       // (asked for the form alone)
    PropState* p = eval->props[pi + 1].get();
    const size_t G = p->prop.K;
    std::vector<uint64_t> acc;
    if (!read_record(eval, p, &acc)) return false;
    if (frames) *frames = acc[G];
    rows_over_frames(acc.data(), G, acc[G], mean_count);
    return true;
}

// The labels of one frame.  One frame on demand, as vmd_eval_hbond_pairs: all pairs from the raw frame into a union-find of its own, the
// roots read back.  Nothing the evaluation keeps is touched: parent, root, size and the two counts live in one buffer of the eval that
// only this call uses (kept between calls).
extern "C" size_t vmd_eval_cluster_labels(vmd_script_eval_t* eval, const char* name, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame,
                                          uint32_t* labels) {
    const size_t failed = VMD_CLUSTER_LABELS_FAILED;
    if (!eval || !traj || !name || !labels) { vmd_fail("vmd_eval_cluster_labels: NULL argument"); return failed; }
    vmd_script_eval_t* e = eval;
    const size_t pi = cluster_statement(e, name);
    if (pi == e->props.size()) return failed;
    PropState* p = e->props[pi].get();
    const Property& d = p->prop;
    const size_t nent = d.a.size(), G = d.K;
    uint32_t counts[2] = {0, 0};
    auto run = [&](const BatchSrc& src) -> bool {
        if (!e->d_one_clusters.ensure(3 * G + 2)) return false;
        uint32_t* parent = e->d_one_clusters.p;
        uint32_t* root = parent + G;
        uint32_t* size = root + G;
        uint32_t* dc = size + G;
        KRN_OK(vmd_hip_cluster_brute(e->stream, src.base, 0, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), 1, p->d_a.p,
                p->d_c.p, (int)nent, (int)G, d.rmax, e->spec.within_closed ? 1 : 0, parent, nullptr));
        KRN_OK(vmd_hip_cluster_finish(e->stream, parent, root, size, 1, (int)G, dc, nullptr, nullptr, nullptr, 0, nullptr));
        HIP_OK(hipMemcpyAsync(labels, root, G * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipMemcpyAsync(counts, dc, sizeof(counts), hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        return true;
    };
    if (!on_one_frame(e, "vmd_eval_cluster_labels", sys, traj, frame, run)) return failed;
    return counts[0];
}

// ---- the hot call -----------------------------------------------------------------------------------------------
bool upload_static(vmd_script_eval_t* e, const vmd_system_t* sys, size_t traj_atoms) {
    for (auto& s : e->sels) {
        if (!s->d_idx.p) { if (!s->d_idx.upload(s->idx.data(), s->idx.size(), e->stream)) return false; }
    }
    for (auto& p : e->props) {
        if (p->uploaded) continue;
        const Property& d = p->prop;
        auto masses = [&](const std::vector<int32_t>& idx, std::vector<float>& out) {
            out.resize(idx.size());
            for (size_t i = 0; i < idx.size(); ++i)
                out[i] = (sys && sys->mass && (size_t)idx[i] < sys->atom_count) ? sys->mass[idx[i]] : 1.0f;
            if ((d.temporal() || d.form == Form::RMSF) && e->spec.dist_geometric_com) std::fill(out.begin(), out.end(), 1.0f);   // D-DIST-COM flipped
        };
        std::vector<float> tmp;
        switch (d.form) {
        case Form::RDF: case Form::RAMA_MAP: case Form::SS_POP: case Form::HBOND_OCC: case Form::SASA_OCC: case Form::CONTACT_OCC:
        case Form::CONTACT_NATIVE: case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST:
            break;      // the sets of an rdf are interned selections; a map, the populations, an occupancy, a native fraction and the companions of a cluster count have none
        case Form::CLUSTER_COUNT:
            // the entries' atoms and groups in list order (the atoms are an interned selection as well)
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream) || !p->d_c.upload(d.ct_group.data(), d.ct_group.size(), e->stream)) return false;
            break;
        case Form::CONTACT_COUNT: {
            // the entries' atoms and groups in list order (the atoms are an interned selection as well), the native pairs as
            // condensed indices
            const uint32_t G = (uint32_t)d.K;
            std::vector<uint32_t> nat(d.ct_native.size() / 2);
            for (size_t k = 0; k < nat.size(); ++k) {
                const uint32_t g = (uint32_t)d.ct_native[2 * k], h = (uint32_t)d.ct_native[2 * k + 1];
                nat[k] = g * (2u * G - g - 1u) / 2u + (h - g - 1u);
            }
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream) || !p->d_c.upload(d.ct_group.data(), d.ct_group.size(), e->stream) ||
                (!nat.empty() && !p->d_ct_native.upload(nat.data(), nat.size(), e->stream))) return false;
            break;
        }
        case Form::SASA_AREA: {
            // both lists in list order, R = radius + probe (one fp32 add per entry), the weights
            // w_i = llround(4 pi R_i^2 / P * 2^20) formed in double, and the point table vmd_sasa_points hands out
            std::vector<float> ra(d.a.size()), rb(d.b.size()), pts(3 * (size_t)d.sasa_npoints);
            std::vector<uint32_t> w(d.a.size());
            float rmax_env = 0.0f;
            for (size_t i = 0; i < ra.size(); ++i) {
                ra[i] = d.sasa_ra[i] + d.sasa_probe;
                w[i] = (uint32_t)std::llround(4.0 * M_PI * (double)ra[i] * (double)ra[i] / (double)d.sasa_npoints * 1048576.0);
            }
            for (size_t j = 0; j < rb.size(); ++j) { rb[j] = d.sasa_rb[j] + d.sasa_probe; rmax_env = std::max(rmax_env, rb[j]); }
            p->sasa_rmax_env = rmax_env;
            if (vmd_sasa_points(d.sasa_npoints, (float(*)[3])pts.data(), d.sasa_npoints) != d.sasa_npoints) return false;
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream) || !p->d_b.upload(d.b.data(), d.b.size(), e->stream) ||
                !p->d_sasa_ra.upload(ra.data(), ra.size(), e->stream) || !p->d_sasa_rb.upload(rb.data(), rb.size(), e->stream) ||
                !p->d_sasa_w.upload(w.data(), w.size(), e->stream) || !p->d_sasa_pts.upload(pts.data(), pts.size(), e->stream)) return false;
            break;
        }
        case Form::HBOND_COUNT:
            // the donors, their hydrogens, the acceptors in list order (the acceptors are an interned selection as well)
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream) || !p->d_c.upload(d.c.data(), d.c.size(), e->stream) ||
                !p->d_b.upload(d.b.data(), d.b.size(), e->stream)) return false;
            break;
        case Form::SS_CLASS: {
            // N, CA, C, O per segment and what the kernels read of the ranges - the range of every segment, the proline bytes,
            // the bit row "has both neighbours in its range"
            const size_t nseg = d.a.size();
            std::vector<int32_t> rng(nseg);
            std::vector<uint8_t> pro(nseg);
            std::vector<uint64_t> nb((nseg + 63) / 64, 0);
            for (size_t r = 0; r + 1 < d.aoff.size(); ++r)
                for (int32_t s = d.aoff[r]; s < d.aoff[r + 1]; ++s) {
                    rng[(size_t)s] = (int32_t)r;
                    if (s > d.aoff[r] && s + 1 < d.aoff[r + 1]) nb[(size_t)s >> 6] |= 1ull << (s & 63);
                }
            for (size_t s = 0; s < nseg; ++s) pro[s] = d.rama_class[s] == 2;
            if (!p->d_a.upload(d.a.data(), nseg, e->stream) || !p->d_b.upload(d.b.data(), nseg, e->stream) ||
                !p->d_c.upload(d.c.data(), nseg, e->stream) || !p->d_ss_o.upload(d.ss_o.data(), nseg, e->stream) ||
                !p->d_ss_rng.upload(rng.data(), nseg, e->stream) || !p->d_ss_pro.upload(pro.data(), nseg, e->stream) ||
                !p->d_ss_nb.upload(nb.data(), nb.size(), e->stream)) return false;
            HIP_OK(hipStreamSynchronize(e->stream));       // the vectors go out of scope
            break;
        }
        case Form::WITHIN_EXPR: break;                   // the lists live in the interned selections
        case Form::MSD_TABLE:                            // the atoms in list order
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream)) return false;
            break;
        case Form::SDF: {
            if (!p->d_structs.upload(d.a.data(), d.a.size(), e->stream)) return false;
            if (!p->d_tgt.upload(d.b.data(), d.b.size(), e->stream)) return false;
            masses(d.a, tmp);
            if (!p->d_mass.upload(tmp.data(), tmp.size(), e->stream)) return false;
            if (!p->d_ref_pose.ensure(d.m * 3)) return false;
            p->have_tree = false;
            if (sys && sys->bonds && sys->bond_count) {
                // D-SDF-UNWRAP with bonds: breadth-first from local atom 0 over the bonds among the structure's atoms, neighbours in
                // increasing local index; atoms the walk does not reach hang on their index predecessor (oracle: vo_bond_tree)
                std::vector<int32_t> order(d.K * d.m), parent(d.K * d.m);
                std::map<int32_t, std::vector<int32_t>> adj;            // only atoms of reference structures matter
                std::map<int32_t, char> member;
                for (int32_t a : d.a) member[a] = 1;
                for (size_t b = 0; b < sys->bond_count; ++b) {
                    const int32_t i = sys->bonds[b][0], j = sys->bonds[b][1];
                    if (member.count(i) && member.count(j)) { adj[i].push_back(j); adj[j].push_back(i); }
                }
                for (size_t k = 0; k < d.K; ++k) {
                    const int32_t* idx = &d.a[k * d.m];
                    int32_t* ord = &order[k * d.m];
                    int32_t* par = &parent[k * d.m];
                    std::map<int32_t, int32_t> local;
                    for (size_t a = 0; a < d.m; ++a) local.emplace(idx[a], (int32_t)a);
                    std::vector<char> seen(d.m, 0);
                    size_t head = 0, tail = 0;
                    ord[tail++] = 0; seen[0] = 1; par[0] = -1;
                    while (head < tail) {
                        const int32_t a = ord[head++];
                        std::vector<int32_t> nb;
                        auto it = adj.find(idx[a]);
                        if (it != adj.end()) for (int32_t g : it->second) { auto l = local.find(g);
                                if (l != local.end()) nb.push_back(l->second); }
                        std::sort(nb.begin(), nb.end());
                        for (int32_t c : nb) if (!seen[c]) { seen[c] = 1; par[c] = a; ord[tail++] = c; }
                    }
                    for (size_t a = 1; a < d.m; ++a) if (!seen[a]) { par[a] = (int32_t)a - 1; ord[tail++] = (int32_t)a; }
                }
                if (!p->d_tree_order.upload(order.data(), order.size(), e->stream) || !p->d_tree_parent.upload(parent.data(),
                        parent.size(), e->stream)) return false;
                HIP_OK(hipStreamSynchronize(e->stream));                 // the vectors go out of scope
                p->have_tree = true;
            }
            // owner[t]: the structure target t is a member of (exclusion rule); only valid when memberships are unique
            std::vector<int8_t> owner(d.b.size(), (int8_t)-1);
            bool unique = d.K <= 127;
            if (unique) {
                std::map<int32_t, int> where;
                for (size_t k = 0; k < d.K && unique; ++k)
                    for (size_t a = 0; a < d.m; ++a) {
                        auto it = where.find(d.a[k * d.m + a]);
                        if (it != where.end() && it->second != (int)k) { unique = false; break; }
                        where[d.a[k * d.m + a]] = (int)k;
                    }
                if (unique) for (size_t t = 0; t < d.b.size(); ++t) { auto it = where.find(d.b[t]);
                        if (it != where.end()) owner[t] = (int8_t)it->second; }
            }
            p->have_owner = unique;
            if (unique && !p->d_owner.upload(owner.data(), owner.size(), e->stream)) return false;
            p->unowned = unique && std::all_of(owner.begin(), owner.end(), [](int8_t o) { return o < 0; });
            // an arithmetic progression (every water oxygen of a regular solvent box: first + 3 t) needs no index list on the device
            p->tgt_first = d.b[0]; p->tgt_stride = 0;
            if (d.b.size() >= 2 && d.b[1] > d.b[0] && g_opt.sdf_arith != 0) {
                const int64_t st = (int64_t)d.b[1] - d.b[0];
                bool ok = true;
                for (size_t t = 2; t < d.b.size() && ok; ++t) ok = (int64_t)d.b[t] - d.b[t - 1] == st;
                if (ok && st < (1 << 20)) p->tgt_stride = (int)st;
            }
            // dense targets: stream whole frames and select by a per-atom tag instead of gathering through the index list
            // sized from the TRAJECTORY's atom count (the target indices were validated against it, check_atoms), never from
            // sys->atom_count, which a host may leave unset or out of step
            const size_t natoms = traj_atoms;
            p->have_tag = unique && d.K <= 253 && natoms > 0 && d.b.size() * 8 >= natoms && g_opt.sdf_dense != 0;
            if (p->have_tag) {
                p->tag_len = (natoms + 63) & ~(size_t)63;
                std::vector<uint8_t> tag(p->tag_len, (uint8_t)255);
                for (size_t t = 0; t < d.b.size(); ++t) tag[d.b[t]] = owner[t] < 0 ? (uint8_t)254 : (uint8_t)owner[t];
                if (!p->d_tag.upload(tag.data(), tag.size(), e->stream)) return false;
                HIP_OK(hipStreamSynchronize(e->stream));
            }
            HIP_OK(hipStreamSynchronize(e->stream));
            break;
        }
        case Form::RAMA_TABLE:
            // N, CA, C per segment and the per-segment bytes (the descriptor's vectors live as long as the eval)
            if (!p->d_a.upload(d.a.data(), d.a.size(), e->stream) || !p->d_b.upload(d.b.data(), d.b.size(), e->stream) ||
                !p->d_c.upload(d.c.data(), d.c.size(), e->stream) || !p->d_rama_class.upload(d.rama_class.data(), d.rama_class.size(), e->stream)
                || !p->d_rama_link.upload(d.rama_link.data(), d.rama_link.size(), e->stream)) return false;
            break;
        case Form::DISTANCE: case Form::ANGLE: case Form::DIHEDRAL: case Form::SHAPE: case Form::RMSD: case Form::RMSF: case Form::WITHIN: {
            // the form's argument sets (two for distance, three and four for angle / dihedral, DESIGN S6b), their offsets and masses
            const std::vector<int32_t>* sets[4] = {&d.a, &d.b, &d.c, &d.d};
            const std::vector<int32_t>* offs[4] = {&d.aoff, &d.boff, &d.coff, &d.doff};
            DevBuf<int32_t>* d_set[4] = {&p->d_a, &p->d_b, &p->d_c, &p->d_d};
            DevBuf<int32_t>* d_off[4] = {&p->d_aoff, &p->d_boff, &p->d_coff, &p->d_doff};
            DevBuf<float>* d_m[4] = {&p->d_ma, &p->d_mb, &p->d_mc, &p->d_md};
            for (int k = 0; k < d.nargs(); ++k) {
                if (k) HIP_OK(hipStreamSynchronize(e->stream));       // tmp is refilled below
                if (!d_set[k]->upload(sets[k]->data(), sets[k]->size(), e->stream) || !d_off[k]->upload(offs[k]->data(), offs[k]->size(), e->stream))
                    return false;
                masses(*sets[k], tmp);
                if (!d_m[k]->upload(tmp.data(), tmp.size(), e->stream)) return false;
            }
            break;
        }
        }
        HIP_OK(hipStreamSynchronize(e->stream));   // tmp goes out of scope
        p->uploaded = true;
    }
    return true;
}

extern "C" const int32_t* vmd_eval_sdf_structures(const vmd_script_eval_t* eval, const char* name, size_t* num_structures,
        size_t* atoms_per_structure) {
    PropState* p = find_prop(eval, name);
    if (!p || p->prop.form != Form::SDF) { vmd_fail("'%s' is not an sdf property", name ? name : "(null)"); return nullptr; }
    if (num_structures) *num_structures = p->prop.K;
    if (atoms_per_structure) *atoms_per_structure = p->prop.m;
    return p->prop.a.data();
}

extern "C" bool vmd_eval_sdf_matrices(vmd_script_eval_t* eval, const char* name, const vmd_system_t* sys,
                                      vmd_trajectory_i* traj, uint32_t frame, float* matrices, size_t* K_out, float* extent_out) {
    if (!eval || !traj) return vmd_fail("vmd_eval_sdf_matrices: NULL argument");
    PropState* p = find_prop(eval, name);
    if (!p || p->prop.form != Form::SDF) return vmd_fail("'%s' is not an sdf property", name ? name : "(null)");
    std::lock_guard<std::mutex> lock(eval->mtx);
    HIP_OK(hipSetDevice(eval->device));
    vmd_script_eval_t* e = eval;
    const size_t num_atoms = traj->num_atoms(traj->inst);
    if (!check_atoms(e, num_atoms) || !upload_static(e, sys, num_atoms)) return false;
    vmd_device_view_t view;
    memset(&view, 0, sizeof(view));
    const bool have_view = traj->device_view && traj->device_view(traj->inst, &view) && view.device == e->device;
    BatchSrc src;
    if (!p->ref_pose_ready) {
        if (!fetch_batch(e, traj, view_holds(have_view, view, 0) ? &view : nullptr, num_atoms, 0, 1, &src)) return false;
        KRN_OK(vmd_hip_sdf_ref_pose(e->stream, src.base, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), p->d_structs.p,
                p->d_mass.p, (int)p->prop.m, p->d_ref_pose.p, p->have_tree ? p->d_tree_order.p : nullptr, p->have_tree
                ? p->d_tree_parent.p : nullptr));
        HIP_OK(hipStreamSynchronize(e->stream));
        p->ref_pose_ready = true;
    }
    if (!fetch_batch(e, traj, view_holds(have_view, view, frame) ? &view : nullptr, num_atoms, frame, 1, &src)) return false;
    const size_t K = p->prop.K;
    DevBuf<double> dM;
    if (!dM.ensure(K * 12) || !p->d_R32.ensure(K * 9) || !p->d_c32.ensure(K * 3)) return false;
    if (p->have_tree && !p->d_tree_pos.ensure(K * p->prop.m * 3)) return false;
    KRN_OK(vmd_hip_sdf_align(e->stream, src.base, src.frame_stride, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), 1,
            p->d_structs.p, p->d_mass.p, (int)K, (int)p->prop.m, p->d_ref_pose.p, p->d_R32.p, p->d_c32.p, dM.p, nullptr, p->have_tree
            ? p->d_tree_order.p : nullptr, p->have_tree ? p->d_tree_parent.p : nullptr, p->have_tree ? p->d_tree_pos.p : nullptr));
    std::vector<double> M(K * 12);
    HIP_OK(hipMemcpyAsync(M.data(), dM.p, K * 12 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (matrices) {
        for (size_t k = 0; k < K; ++k) {
            float* o = matrices + 16 * k;   // column-major mat4
            const double* r = &M[12 * k];
            for (int c = 0; c < 4; ++c) for (int rr = 0; rr < 3; ++rr) o[4 * c + rr] = (float)r[4 * rr + c];
            o[3] = 0.0f; o[7] = 0.0f; o[11] = 0.0f; o[15] = 1.0f;
        }
    }
    if (K_out) *K_out = K;
    if (extent_out) *extent_out = p->prop.rmax;
    return true;
}

// The members of one shell at one frame, by atom.  One frame on demand, as vmd_eval_sdf_matrices: all pairs from the raw frame
// with the bytes in atom order (for ONE frame the cell build a walk needs costs more than it saves), packed to bits on the host.  Nothing
// the evaluation keeps is touched: the mask and count live in two buffers of the eval that only this call uses (kept between calls: a
// host asks for every displayed frame, and giving device memory back may wait for the device).
extern "C" size_t vmd_eval_shell_mask(vmd_script_eval_t* eval, const char* name, int which, const vmd_system_t* sys, vmd_trajectory_i* traj,
                                      uint32_t frame, uint64_t* words, size_t cap) {
    const size_t failed = VMD_SHELL_MASK_FAILED;
    if (!eval || !traj || !name) { vmd_fail("vmd_eval_shell_mask: NULL argument"); return failed; }
    PropState* p = find_prop(eval, name);
    if (!p) { vmd_fail("unknown property '%s'", name); return failed; }
    if (which != 0 && which != 1) { vmd_fail("vmd_eval_shell_mask: which must be 0 (reference) or 1 (target)"); return failed; }
    vmd_script_eval_t* e = eval;
    // (properties, selections and shells are read in front of the mutex: build_rdf_plan / build_within_plan run once, when the eval is
    // created, and nothing changes them afterwards - pool threads inside frame_range only read them too)
    int sel_t = -1, sel_r = -1;
    float rmin = 0.0f, rmax = 0.0f;
    if (p->prop.form == Form::WITHIN && which == 1) {
        sel_t = p->sel_a; sel_r = p->sel_b; rmin = p->prop.rmin; rmax = p->prop.rmax;
    } else if ((p->prop.is_shell_rdf() || p->prop.is_shell_sdf()) && p->prop.shell[which].on) {
        const Shell& h = *e->shells[p->shell_of[which]];
        sel_t = h.sel_t; sel_r = h.sel_r; rmin = h.rmin; rmax = h.rmax;
    } else if ((p->prop.form == Form::WITHIN_EXPR || p->prop.is_expr_sdf()) && which == 1) {
        // every term by all pairs into the eval's one-frame bits, then the finish - handled below
    } else {
        vmd_fail("the %s side of '%s' is not a within() shell", which ? "target" : "reference", name);
        return failed;
    }
    if (frame >= e->num_frames) { vmd_fail("vmd_eval_shell_mask: frame %u outside the trajectory (%zu frames)", frame, e->num_frames); return failed; }
    std::lock_guard<std::mutex> lock(eval->mtx);
    if (hipSetDevice(eval->device) != hipSuccess) { vmd_fail("hipSetDevice failed"); return failed; }
    const size_t num_atoms = traj->num_atoms(traj->inst);
    const size_t nwords = (num_atoms + 63) / 64;
    if (cap < nwords || (!words && nwords)) { vmd_fail("vmd_eval_shell_mask: %zu words needed, room for %zu", nwords, words ? cap : (size_t)0); return failed; }
    if (!check_atoms(e, num_atoms) || !upload_static(e, sys, num_atoms)) return failed;
    std::fill(words, words + nwords, (uint64_t)0);
    const ShellExpr* x = p->expr_of >= 0 ? e->exprs[p->expr_of].get() : nullptr;
    if (!x && sel_t < 0) return 0;             // T minus R is empty (spec_within_exclude_ref)
    auto run = [&](size_t* members) -> bool {
        vmd_device_view_t view;
        memset(&view, 0, sizeof(view));
        const bool have_view = traj->device_view && traj->device_view(traj->inst, &view) && view.device == e->device;
        BatchSrc src;
        if (!fetch_batch(e, traj, view_holds(have_view, view, frame) ? &view : nullptr, num_atoms, frame, 1, &src)) return false;
        const size_t stride = std::max(src.row_stride, num_atoms);
        DevBuf<uint8_t>& d_mask = e->d_one_mask;
        DevBuf<uint32_t>& d_count = e->d_one_count;
        if (!d_mask.ensure(stride) || !d_count.ensure(1)) return false;
        HIP_OK(hipMemsetAsync(d_mask.p, 0, stride, e->stream));
        if (x) {
            if (!e->d_one_bits.ensure(stride)) return false;
            HIP_OK(hipMemsetAsync(e->d_one_bits.p, 0, stride, e->stream));
            const bool skip = g_opt.shell_expr_skip.load() != 0;
            for (size_t pos = 0; pos < x->order.size(); ++pos) {
                const ShellExpr::Term& tm = x->terms[x->order[pos]];
                const uint32_t live = skip ? shell_expr_live(x->truth, x->order, pos) : 0xffffu;
                if (!live || tm.sel_tt < 0) continue;
                const Selection* tt = e->sels[tm.sel_tt].get();
                const Selection* tr = e->sels[tm.sel_r].get();
                KRN_OK(vmd_hip_within_brute_expr(e->stream, src.base, src.frame_stride, src.row_stride, e->stages[0].d_boxes.p,
                        batch_pbc(e->stages[0]), 1, tt->d_idx.p, (int)tt->idx.size(), tr->d_idx.p, (int)tr->idx.size(), tm.rmin, tm.rmax,
                        e->spec.within_closed ? 1 : 0, x->order[pos], live, e->d_one_bits.p, stride, nullptr));
            }
            const Selection* xt = e->sels[x->sel_t].get();
            KRN_OK(vmd_hip_shell_expr_finish(e->stream, 1, xt->d_idx.p, (int)xt->idx.size(), e->d_one_bits.p, x->truth, d_mask.p, stride,
                    d_count.p, nullptr));
        } else {
            const Selection* st = e->sels[sel_t].get();
            const Selection* sr = e->sels[sel_r].get();
            KRN_OK(vmd_hip_within_brute_atoms(e->stream, src.base, src.frame_stride, src.row_stride, e->stages[0].d_boxes.p,
                    batch_pbc(e->stages[0]), 1, st->d_idx.p, (int)st->idx.size(), sr->d_idx.p, (int)sr->idx.size(), rmin, rmax,
                    e->spec.within_closed ? 1 : 0, d_count.p, d_mask.p, stride));
        }
        std::vector<uint8_t> bytes(num_atoms);
        HIP_OK(hipMemcpyAsync(bytes.data(), d_mask.p, num_atoms, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        // counted from the bytes, not taken from d_count: a list that names an atom twice marks it once, and the answer is in ATOMS
        size_t set = 0;
        for (size_t a = 0; a < num_atoms; ++a) if (bytes[a]) { words[a >> 6] |= (uint64_t)1 << (a & 63); set += 1; }
        *members = set;
        return true;
    };
    size_t members = 0;
    if (!run(&members)) { std::fill(words, words + nwords, (uint64_t)0); return failed; }
    return members;
}
