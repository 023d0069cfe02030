// viamd_amd/csrc/vmd_eval_launch.cpp - what one batch of a range run puts on the device: launch_rdf (the cell builds and everything
// behind them that a bucket overflow voids and repeats - pair passes, shells, within counts, shell masks and the sdfs under them, the
// commits) and one launch function per kind of the remaining properties (launch_property).  Who calls them, and when: vmd_eval_range.cpp.
#include "vmd_eval_internal.h"

// The grid of this batch for radius r, and the boxes it is cut from: fully periodic cells use the frame boxes; open axes (non-periodic
// systems, slabs) span the batch's bounding box.  `lanes` is the size of the sparsest list a walk over this grid puts in its lanes
// (the denser of the two sides of every pass); its density against the first frame's cell decides the pencil split, so that equal
// radii over equal selections meet on equal grids whoever asks.  -> 1 a grid, 0 none (all pairs), -1 an error
int RangeRun::grid_for(BatchCtx& c, size_t lanes, float r, vmd_grid_t* grid, const float** d_gb) {
    const bool open_axes = (c.pbc & 8u) == 0 && (c.pbc & VMD_UNITCELL_PBC_ALL) != VMD_UNITCELL_PBC_ALL;
    if (open_axes && !g_opt.force_brute && !prepare_open_boxes(e, *c.src, c.nb, c.pbc, num_atoms)) return -1;
    const bool gboxes = open_axes && c.src->gboxes_ready;
    const std::vector<float>& gb = gboxes ? c.src->h_gboxes : c.src->h_boxes;
    *d_gb = gboxes ? c.src->d_gboxes.p : c.src->d_boxes.p;
    bool dense_lanes = !open_axes;
    if (dense_lanes) {
        const float* q = gb.data();
        const double vol = (double)q[0] * q[1] * q[2];
        dense_lanes = vol > 0.0 && (double)lanes / vol >= 0.08;
    }
    return choose_grid(gb, c.pbc, c.nb, r, grid, dense_lanes) ? 1 : 0;
}

// both selections of a pass sorted on `grid`, once when they are the same one (build_selection keeps what this batch already sorted on
// the same grid and re-sorts when the grid differs)
bool RangeRun::build_pair(BatchCtx& c, Selection* a, Selection* b, const float* d_gb, const vmd_grid_t& grid) {
    return build_selection(e, a, *c.src, d_gb, c.pbc, c.nb, grid) && (b == a || build_selection(e, b, *c.src, d_gb, c.pbc, c.nb, grid));
}

// Walk or all pairs for the shell within(.. r, R) of the targets T?  -> 1 the walk on *grid, the cell-sorted copy of R built (and T's where
// the pass walks T sorted: a count); 0 all pairs from the raw frame; -1 an error.  atom_order couples two things: the pass keeps T in list
// order, so R alone is sorted (masks, expression terms), AND the RULE measured for such passes applies - all pairs not only where no grid
// exists for r but also when R has fewer than shell_brute_below atoms (480: DESIGN 1.8 measures where the two costs cross).
int RangeRun::within_route(BatchCtx& c, Selection* st, Selection* sr, float r, bool atom_order, vmd_grid_t* grid, const float** d_gb) {
    if (atom_order && (int)sr->idx.size() < g_opt.shell_brute_below.load()) return 0;
    const int have_grid = grid_for(c, std::max(st->idx.size(), sr->idx.size()), r, grid, d_gb);
    if (have_grid > 0 && !build_pair(c, atom_order ? sr : st, sr, *d_gb, *grid)) return -1;
    return have_grid;
}

// pair_stream takes up behind what the eval's stream holds so far ...
bool RangeRun::pair_fork() {
    HIP_OK(hipEventRecord(e->pair_fork, e->stream));
    HIP_OK(hipStreamWaitEvent(e->pair_stream, e->pair_fork, 0));
    forked = true;
    return true;
}

// ... and the eval's stream waits for it before anything overwrites what its launches read, or reads what they wrote
bool RangeRun::pair_join() {
    if (!forked) return true;
    HIP_OK(hipEventRecord(e->pair_join, e->pair_stream));
    HIP_OK(hipStreamWaitEvent(e->stream, e->pair_join, 0));
    forked = false;
    return true;
}

// One pair pass over the batch: one launch of the pair kernel per sub, each into its own scratch row.  The blocks' launches alternate
// between the eval's stream and pair_stream (own partial rows) when the batch asks for it; on_row(sub, scratch row, stream) follows
// every launch on its stream - what else the row needs, and who it is committed to.
template <class OnRow>
bool RangeRun::launch_pair_pass(BatchCtx& c, const PairSide (&side)[2], bool same, const RdfGroup& g, const float* d_gb,
        const vmd_grid_t& grid, OnRow on_row) {
    if (c.two_streams && !pair_fork()) return false;
    const PairSide &a = side[0], &b = side[1];
    size_t si = 0;
    for (auto& su : c.subs) {
        uint64_t* dst = e->d_pass.p + (row++) * VMD_RDF_NUM_BINS;
        const bool second = c.two_streams && (si++ & 1);
        hipStream_t ks = second ? e->pair_stream : e->stream;
        if (!second) e->prof.begin("rdf_pencil", ks);
        KRN_OK(vmd_hip_rdf_pencil(ks, a.sorted + su.off * 3 * (size_t)a.npad, a.cell_start + su.off * (size_t)(grid.ncell + 1), a.n,
                a.npad, b.sorted + su.off * 3 * (size_t)b.npad, b.cell_start + su.off * (size_t)(grid.ncell + 1), b.n, b.npad,
                d_gb + 9 * su.off, (int)su.nb, grid, g.rmin, g.rmax, VMD_RDF_NUM_BINS, same ? 1 : 0, g_opt.rdf_variant, c.pbc,
                second ? e->d_partial2.p : e->d_partial.p, dst, e->d_overflow.p));
        if (!second) e->prof.end(ks);
        if (!on_row(su, dst, ks)) return false;
    }
    return true;
}

// ---- shells as rdf arguments.  One walk + one compaction per shell, batch and grid, whichever properties use it; the
// per-frame populations travel to the host from here, behind the overflow flag like everything else of launch_rdf.
bool RangeRun::shell_pops(BatchCtx& c, size_t hi) {
    Shell* h = e->shells[hi].get();
    c.shell_pop[hi].assign(c.nb, 0);
    if (h->sel_t >= 0)
        HIP_OK(hipMemcpyAsync(c.shell_pop[hi].data(), h->count.p, c.nb * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    return true;
}

// the hit copy of shell hi on `grid`: (sorted, cell_start) of the members, a selection the pair kernel takes as it is
bool RangeRun::shell_pencil(BatchCtx& c, size_t hi, const float* d_gb, const vmd_grid_t& grid) {
    Shell* h = e->shells[hi].get();
    if (h->sel_t < 0) { h->built = 1; return shell_pops(c, hi); }
    if (h->built == 1 && h->built_grid.nxf == grid.nxf && h->built_grid.ny == grid.ny && h->built_grid.nz == grid.nz) return true;
    Selection* st = e->sels[h->sel_t].get();
    Selection* sr = e->sels[h->sel_r].get();
    if (!build_pair(c, st, sr, d_gb, grid)) return false;
    const size_t npen = (size_t)grid.ny * grid.nz;
    const size_t rows = c.nb * 3 * (size_t)st->nsel_pad + 64;           // the parent's rows, slack included
    if (rows > h->sorted.cap) {
        if (!h->sorted.ensure(rows)) return false;
        HIP_OK(hipMemsetAsync(h->sorted.p, 0, rows * sizeof(float), e->stream));     // what lies beyond a population stays finite
    }
    if (!h->flags.ensure(c.nb * (size_t)st->nsel_pad) || !h->count.ensure(c.nb) || !h->pen_hits.ensure(c.nb * (npen + 1)) ||
        !h->pen_base.ensure(c.nb * (npen + 1)) || !h->cell_start.ensure(c.nb * (size_t)(grid.ncell + 1))) return false;
    e->prof.begin("shell_flags", e->stream);
    KRN_OK(vmd_hip_within_pencil_flags(e->stream, sr->sorted.p, sr->cell_start.p, (int)sr->idx.size(), sr->nsel_pad, st->sorted.p,
            st->cell_start.p, (int)st->idx.size(), st->nsel_pad, d_gb, (int)c.nb, grid, h->rmin, h->rmax,
            e->spec.within_closed ? 1 : 0, c.pbc, h->count.p, e->d_overflow.p, h->flags.p, h->pen_hits.p));
    e->prof.end(e->stream);
    e->prof.begin("shell_compact", e->stream);
    KRN_OK(vmd_hip_shell_compact(e->stream, h->flags.p, h->pen_hits.p, h->pen_base.p, st->sorted.p, st->cell_start.p, st->nsel_pad,
            (int)c.nb, grid, h->sorted.p, h->cell_start.p, e->d_overflow.p));
    e->prof.end(e->stream);
    h->built = 1; h->built_grid = grid;
    return shell_pops(c, hi);
}

// no grid: the members as one byte per list entry, from all pairs of the raw frame (always wrapped positions)
bool RangeRun::shell_brute(BatchCtx& c, size_t hi) {
    Shell* h = e->shells[hi].get();
    if (h->built == 2) return true;
    if (h->sel_t >= 0) {
        Selection* st = e->sels[h->sel_t].get();
        Selection* sr = e->sels[h->sel_r].get();
        if (!h->flags.ensure(c.nb * st->idx.size()) || !h->count.ensure(c.nb)) return false;
        e->prof.begin("shell_brute", e->stream);
        KRN_OK(vmd_hip_within_brute_flags(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc,
                (int)c.nb, st->d_idx.p, (int)st->idx.size(), sr->d_idx.p, (int)sr->idx.size(), h->rmin, h->rmax,
                e->spec.within_closed ? 1 : 0, h->count.p, h->flags.p));
        e->prof.end(e->stream);
    }
    h->built = 2;
    return shell_pops(c, hi);
}

// a shell property by all pairs: list-order masks on the shell sides.  choose_grid failed for the group, or this is spec_rdf_raw
bool RangeRun::shell_rdf_brute(BatchCtx& c, const RdfGroup& g, PropState* p) {
    for (int k = 0; k < 2; ++k) if (p->shell_of[k] >= 0 && !shell_brute(c, (size_t)p->shell_of[k])) return false;
    for (auto& su : c.subs) {
        uint64_t* dst = e->d_pass.p + (row++) * VMD_RDF_NUM_BINS;
        if (p->sel_a < 0 || p->sel_b < 0) continue;                      // T minus R is empty: no member in any frame
        Selection* sa = e->sels[p->sel_a].get();
        Selection* sb = e->sels[p->sel_b].get();
        const uint8_t* ma = p->shell_of[0] >= 0 ? e->shells[p->shell_of[0]]->flags.p + su.off * sa->idx.size() : nullptr;
        const uint8_t* mb = p->shell_of[1] >= 0 ? e->shells[p->shell_of[1]]->flags.p + su.off * sb->idx.size() : nullptr;
        e->prof.begin("rdf_brute", e->stream);
        KRN_OK(vmd_hip_rdf_brute_masked(e->stream, c.src->base + su.off * c.src->frame_stride, c.src->frame_stride,
                c.src->row_stride, c.src->d_boxes.p + 9 * su.off, c.pbc, (int)su.nb, sa->d_idx.p, (int)sa->idx.size(), ma,
                sb->d_idx.p, (int)sb->idx.size(), mb, g.rmin, g.rmax, VMD_RDF_NUM_BINS, dst));
        e->prof.end(e->stream);
        commits.push_back({acc_of(p, su), dst, 1});
    }
    return true;
}

// ---- RDF: one pair pass per (group, pass), then the group's rdfs over shells
bool RangeRun::launch_rdf_groups(BatchCtx& c) {
    for (auto& h : e->shells) h->built = 0;
    c.shell_pop.resize(e->shells.size());
    for (auto& g : e->rdf_groups) {
        vmd_grid_t grid;
        const float* d_gb = nullptr;
        // the sparsest selection any pass of this group puts in the lanes (the denser of its two); shell properties by the parent
        // lists: what the cell builds sort
        size_t lanes = (g.passes.empty() && g.shell_props.empty()) ? 0 : SIZE_MAX;
        for (auto& ps : g.passes) lanes = std::min(lanes, std::max(e->sels[ps.sel_a]->idx.size(), e->sels[ps.sel_b]->idx.size()));
        for (int pi : g.shell_props) {
            const PropState* p = e->props[pi].get();
            lanes = std::min(lanes, std::max(p->sel_a >= 0 ? e->sels[p->sel_a]->idx.size() : 0,
                                             p->sel_b >= 0 ? e->sels[p->sel_b]->idx.size() : 0));
        }
        // (grid_r: the larger of the pair cutoff and the shell radii of the group's members - walk and pair kernel accept a wider edge)
        const int have_grid = grid_for(c, lanes, g.grid_r, &grid, &d_gb);
        if (have_grid < 0) return false;
        if (e->spec.rdf_raw || !have_grid) {
            // no grid for this batch (cutoff >= half the cell width, ...): all pairs, per property
            for (int pi : g.props) {
                PropState* p = e->props[pi].get();
                Selection* sa = e->sels[p->sel_a].get();
                Selection* sb = e->sels[p->sel_b].get();
                for (auto& su : c.subs) {
                    uint64_t* dst = e->d_pass.p + (row++) * VMD_RDF_NUM_BINS;
                    e->prof.begin("rdf_brute", e->stream);
                    KRN_OK(vmd_hip_rdf_brute(e->stream, c.src->base + su.off * c.src->frame_stride, c.src->frame_stride,
                            c.src->row_stride, c.src->d_boxes.p + 9 * su.off, c.pbc, (int)su.nb, sa->d_idx.p, (int)sa->idx.size(),
                            sb->d_idx.p, (int)sb->idx.size(), g.rmin, g.rmax, VMD_RDF_NUM_BINS, dst));
                    e->prof.end(e->stream);
                    commits.push_back({acc_of(p, su), dst, 1});
                }
            }
            for (int pi : g.shell_props) if (!shell_rdf_brute(c, g, e->props[pi].get())) return false;
            continue;
        }
        if (!e->d_partial.ensure(vmd_hip_rdf_partial_words())) return false;
        if (c.two_streams && !e->d_partial2.ensure(vmd_hip_rdf_partial_words())) return false;
        for (auto& ps : g.passes) {
            Selection* sa = e->sels[ps.sel_a].get();
            Selection* sb = e->sels[ps.sel_b].get();
            // passes with the same cutoff share the sorted copies; the second stream still reads the sorted copies of the previous pass
            if (!pair_join() || !build_pair(c, sa, sb, d_gb, grid)) return false;
            // the pair set is symmetric in (ref, target): put the denser selection in the lanes - 64 of its atoms span a
            // shorter stretch of the pencil, so the x window of every segment carries less padding
            if (sb->idx.size() > sa->idx.size()) std::swap(sa, sb);
            const PairSide side[2] = {{sa->sorted.p, sa->cell_start.p, (int)sa->idx.size(), sa->nsel_pad},
                                      {sb->sorted.p, sb->cell_start.p, (int)sb->idx.size(), sb->nsel_pad}};
            const bool bump = e->spec.rdf_closed && ps.same && g.rmin <= 0.0f && 0.0f <= g.rmax;
            if (!launch_pair_pass(c, side, ps.same, g, d_gb, grid, [&](const Sub& su, uint64_t* dst, hipStream_t ks) -> bool {
                if (bump) {
                    // closed interval: d = 0 is a hit, but a same-set pass walks the half shell (j > i, every hit twice) and never
                    // meets the pairs (i, i) - one per list entry and frame, all in the bin of d = 0 (SPEC S4 binning of 0)
                    int bin0 = (int)(((0.0f - g.rmin) * (1.0f / (g.rmax - g.rmin))) * (float)VMD_RDF_NUM_BINS);
                    bin0 = std::min(std::max(bin0, 0), VMD_RDF_NUM_BINS - 1);
                    KRN_OK(vmd_hip_bump_u64(ks, dst + bin0, (uint64_t)su.nb * (uint64_t)sa->idx.size()));
                }
                for (auto& tg : ps.targets) commits.push_back({acc_of(e->props[tg.first].get(), su), dst, tg.second});
                return true;
            })) return false;
        }
        // ---- the group's rdfs over shells: the same pair kernel over the hit copies.  Never the half-shell pass: a shell pass counts
        // ordered pairs, (i, i) included at d = 0 where the sides overlap (dropped by the open interval, a hit under spec_rdf_closed)
        for (int pi : g.shell_props) {
            PropState* p = e->props[pi].get();
            // the second stream may still read a hit copy or sorted rows the builds below overwrite
            if (!pair_join()) return false;
            for (int k = 0; k < 2; ++k) if (p->shell_of[k] >= 0 && !shell_pencil(c, (size_t)p->shell_of[k], d_gb, grid)) return false;
            if (p->sel_a < 0 || p->sel_b < 0) { row += c.subs.size(); continue; }     // T minus R is empty
            PairSide side[2];
            for (int k = 0; k < 2; ++k) {
                Selection* sl = e->sels[k ? p->sel_b : p->sel_a].get();
                if (p->shell_of[k] < 0 && !build_pair(c, sl, sl, d_gb, grid)) return false;
                const Shell* h = p->shell_of[k] >= 0 ? e->shells[p->shell_of[k]].get() : nullptr;
                // sizes feed launch heuristics only: the parents'
                side[k] = {h ? h->sorted.p : sl->sorted.p, h ? h->cell_start.p : sl->cell_start.p, (int)sl->idx.size(), sl->nsel_pad};
            }
            if (!launch_pair_pass(c, side, false, g, d_gb, grid, [&](const Sub& su, uint64_t* dst, hipStream_t) -> bool {
                commits.push_back({acc_of(p, su), dst, 1});
                return true;
            })) return false;
        }
    }
    return pair_join();
}

// ---- within counts: the same grids and cell-sorted copies (a selection an RDF pass of this batch sorted on the same
// grid is not sorted again), an any-reduction per target atom instead of a histogram.  Part of launch_rdf because a bucket overflow
// of ITS cell builds repeats the batch like any other; the rows travel to the host from here for the same reason.  Always wrapped
// positions (spec_rdf_raw does not apply); no grid -> all pairs from the raw frame.
bool RangeRun::launch_within_counts(BatchCtx& c) {
    for (int pi : e->within_props) {
        PropState* p = e->props[pi].get();
        const Property& d = p->prop;
        if (!p->d_out.ensure(c.nb) || !p->d_within_count.ensure(c.nb)) return false;
        if (p->within_empty) {
            HIP_OK(hipMemsetAsync(p->d_out.p, 0, c.nb * sizeof(float), e->stream));       // T minus R is empty: +0 in every frame
        } else {
            Selection* st = e->sels[p->sel_a].get();
            Selection* sr = e->sels[p->sel_b].get();
            vmd_grid_t grid;
            const float* d_gb = nullptr;
            const int have_grid = within_route(c, st, sr, d.rmax, false, &grid, &d_gb);
            if (have_grid < 0) return false;
            if (have_grid) {
                e->prof.begin("within_pencil", e->stream);
                KRN_OK(vmd_hip_within_pencil(e->stream, sr->sorted.p, sr->cell_start.p, (int)sr->idx.size(), sr->nsel_pad, st->sorted.p,
                        st->cell_start.p, (int)st->idx.size(), st->nsel_pad, d_gb, (int)c.nb, grid, d.rmin, d.rmax,
                        e->spec.within_closed ? 1 : 0, c.pbc, p->d_within_count.p, e->d_overflow.p));
                e->prof.end(e->stream);
            } else {
                e->prof.begin("within_brute", e->stream);
                KRN_OK(vmd_hip_within_brute(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc,
                        (int)c.nb, st->d_idx.p, (int)st->idx.size(), sr->d_idx.p, (int)sr->idx.size(), d.rmin, d.rmax,
                        e->spec.within_closed ? 1 : 0, p->d_within_count.p));
                e->prof.end(e->stream);
            }
            KRN_OK(vmd_hip_within_to_float(e->stream, p->d_within_count.p, (int)c.nb, p->d_out.p, have_grid ? e->d_overflow.p : nullptr));
        }
        if (!queue_temporal_rows(c, pi, p->d_out.p)) return false;
    }
    return true;
}

// ---- sdfs over a shell target.  First every shell's mask in atom order, then, behind the LAST cell build of the batch,
// alignment and masked scatter.  Walk or all pairs by within_route's RULE, on the grid a within count of the same radius and lists gets.
bool RangeRun::launch_shell_masks(BatchCtx& c) {
    for (auto& h : e->shells) h->abuilt = 0;
    for (int pi : e->shell_sdf_props) {
        PropState* p = e->props[pi].get();
        Shell* h = e->shells[p->shell_of[1]].get();
        if (h->abuilt || h->sel_t < 0) continue;
        Selection* st = e->sels[h->sel_t].get();
        Selection* sr = e->sels[h->sel_r].get();
        const size_t stride = c.src->row_stride;
        if (h->amask_stride != stride || c.nb * stride > h->amask.cap) {
            if (!h->amask.ensure(c.nb * stride)) return false;
            HIP_OK(hipMemsetAsync(h->amask.p, 0, h->amask.cap, e->stream));        // atoms outside T' read 0 for ever
            h->amask_stride = stride;
        }
        if (!h->acount.ensure(c.nb)) return false;
        vmd_grid_t grid;
        const float* d_gb = nullptr;
        const int have_grid = within_route(c, st, sr, h->rmax, true, &grid, &d_gb);
        if (have_grid < 0) return false;
        if (have_grid) {
            e->prof.begin("shell_mask", e->stream);
            KRN_OK(vmd_hip_within_atoms(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, d_gb, c.pbc, (int)c.nb, st->d_idx.p,
                    (int)st->idx.size(), sr->sorted.p, sr->cell_start.p, (int)sr->idx.size(), sr->nsel_pad, grid, h->rmin, h->rmax,
                    e->spec.within_closed ? 1 : 0, h->acount.p, h->amask.p, stride, e->d_overflow.p));
            e->prof.end(e->stream);
            h->abuilt = 1;
        } else {
            e->prof.begin("shell_mask_brute", e->stream);
            KRN_OK(vmd_hip_within_brute_atoms(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc,
                    (int)c.nb, st->d_idx.p, (int)st->idx.size(), sr->d_idx.p, (int)sr->idx.size(), h->rmin, h->rmax,
                    e->spec.within_closed ? 1 : 0, h->acount.p, h->amask.p, stride));
            e->prof.end(e->stream);
            h->abuilt = 2;
        }
    }
    return true;
}

// The scatter under a shell mask adds to the volume with atomics, so unlike a static sdf it has to be all or nothing: it sits here,
// where the overflow flag is final, and tests it like the commits of launch_rdf; a repeated batch runs launch_rdf again and its
// voxels are added exactly once.
bool RangeRun::launch_shell_sdfs(BatchCtx& c) {
    for (int pi : e->shell_sdf_props) {
        PropState* p = e->props[pi].get();
        const Shell* h = e->shells[p->shell_of[1]].get();
        if (h->sel_t < 0) continue;                   // T minus R is empty: no member in any frame, no voxel
        if (!launch_sdf(c, p, h->amask.p, h->amask_stride)) return false;
    }
    return true;
}

// ---- the neighbour analyses: hydrogen bonds, accessible area (1.15), contact maps (1.16), clusters (1.17).  Each statement adds to a record
// with atomics (or sets bits of one), so like a masked scatter it has to be all or nothing: its launches stand behind the LAST cell build
// of the batch, where the overflow flag is final, and test it.  First every statement's cell build (build_neighbour_cells), then, kind by
// kind and statement by statement, the identity of the sorted copy and the walk - per sub, so that a frame block's part lands in its own
// partial (launch_neighbours).  What a kind contributes is a NeighbourKind.
//
// ident_table: the statement's route at launch time and its table in d_hb_ident.  A sorted copy that another statement's build has
// re-sorted on another grid since build_neighbour_cells is not built a second time (that would be a cell build behind an accumulation): the
// statement takes all pairs for this batch, which answers the same bit for bit.  *have_grid 1: the grid, its boxes, and k_sorted_atoms'
// table of sel_b's copy, u32[nb][nsel_pad]; 0: room for the all-pairs route's canonical entries, u32[nb][|sel_b|].
bool RangeRun::ident_table(BatchCtx& c, PropState* p, int route, int* have_grid, vmd_grid_t* grid, const float** d_gb) {
    Selection* sl = e->sels[p->sel_a].get();
    Selection* sr = e->sels[p->sel_b].get();
    *have_grid = route;
    if (*have_grid) {        // (the grid again: it also sets this thread's pencil reach for the walk)
        *have_grid = grid_for(c, std::max(sl->idx.size(), sr->idx.size()), p->prop.rmax, grid, d_gb);
        if (*have_grid < 0) return false;
        if (*have_grid && !(sr->built && sr->built_grid.nxf == grid->nxf && sr->built_grid.ny == grid->ny && sr->built_grid.nz == grid->nz))
            *have_grid = 0;
    }
    if (!p->d_hb_ident.ensure(c.nb * (*have_grid ? (size_t)sr->nsel_pad : sr->idx.size()))) return false;
    if (*have_grid) {
        const Stage& st = *c.src;
        e->prof.begin("sorted_atoms", e->stream);
        KRN_OK(vmd_hip_sorted_atoms(e->stream, st.base, st.frame_stride, st.row_stride, *d_gb, c.pbc, (int)c.nb, sr->d_idx.p,
                (int)sr->idx.size(), sr->sorted.p, sr->cell_start.p, sr->nsel_pad, *grid, p->d_hb_ident.p, e->d_overflow.p));
        e->prof.end(e->stream);
    }
    return true;
}

// One sub of one statement as a kind's calls see it, every pointer at the sub's first frame: the frames and their boxes, the statement p
// with its descriptor d and its record's partial acc; the walk's grid, boxes and copy of sel_b; ident: k_sorted_atoms' table (walk) or the
// room for the canonical entries (all pairs).
struct NeighbourSub {
    hipStream_t s; const uint32_t* overflow;
    PropState* p; const Property& d; uint64_t* acc;
    const Stage& st; const Sub& su; uint32_t pbc; int closed;
    const float *xyz, *fboxes;
    vmd_grid_t grid; const float *gboxes, *sorted; const uint32_t* cell_start; int npad;
    uint32_t* ident;
};

// What differs between the kinds.  record: the companion properties behind the count are still there -> the record (nullptr: vmd_fail said
// why).  walk / brute / finish: the vmd_hip_* call of one sub.  finish_label: the finishes run in a loop of their own behind the
// statement's launches, under this profile label (nullptr: behind each sub's launch).  more_rows: temporal rows besides d_out.
struct NeighbourKind {
    int slot;                                            // RangeRun::neighbour_route[slot]
    std::vector<int> vmd_script_eval_t::* props;
    const char *walk_label, *brute_label, *finish_label;
    PropState* (*record)(vmd_script_eval_t* e, int pi);
    bool (*ensure)(PropState* p, size_t nb);
    int (*walk)(const NeighbourSub& x);
    int (*brute)(const NeighbourSub& x);
    int (*finish)(const NeighbourSub& x);
    bool (*more_rows)(RangeRun& r, BatchCtx& c, int pi, PropState* p);
};

static PropState* record_behind(vmd_script_eval_t* e, int pi, Form form, const char* lost) {
    if ((size_t)pi + 1 < e->props.size() && e->props[pi + 1]->prop.form == form) return e->props[pi + 1].get();
    vmd_fail(lost, e->props[pi]->prop.name.c_str());
    return nullptr;
}

static const NeighbourKind kHbonds = {
    0, &vmd_script_eval_t::hbond_props, "hbond_atoms", "hbond_brute", nullptr,
    [](vmd_script_eval_t* e, int pi) { return record_behind(e, pi, Form::HBOND_OCC, "hydrogen-bond count '%s' has lost its occupancy"); },
    [](PropState* p, size_t nb) { return p->d_out.ensure(nb) && p->d_hb_count.ensure(nb); },
    [](const NeighbourSub& x) {
        return vmd_hip_hbond_atoms(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.gboxes, x.fboxes, x.pbc, (int)x.su.nb, x.p->d_a.p,
                x.p->d_c.p, (int)x.d.a.size(), x.p->d_b.p, (int)x.d.b.size(), x.sorted, x.cell_start, x.npad, x.ident, x.grid, x.d.rmax,
                x.d.hb_c2, x.closed, x.p->d_hb_count.p + x.su.off, x.acc, x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_hbond_brute(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.fboxes, x.pbc, (int)x.su.nb, x.p->d_a.p, x.p->d_c.p,
                (int)x.d.a.size(), x.p->d_b.p, (int)x.d.b.size(), x.ident, x.d.rmax, x.d.hb_c2, x.closed, x.p->d_hb_count.p + x.su.off,
                x.acc, x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_hbond_finish(x.s, x.p->d_hb_count.p + x.su.off, (int)x.su.nb, x.p->d_out.p + x.su.off,
                x.acc + x.d.a.size() + x.d.b.size(), x.overflow);
    },
    nullptr};

static const NeighbourKind kSasa = {
    1, &vmd_script_eval_t::sasa_props, "sasa_atoms", "sasa_brute", nullptr,
    [](vmd_script_eval_t* e, int pi) { return record_behind(e, pi, Form::SASA_OCC, "sasa area '%s' has lost its record"); },
    [](PropState* p, size_t nb) { return p->d_out.ensure(nb) && p->d_sasa_total.ensure(nb); },
    [](const NeighbourSub& x) {
        return vmd_hip_sasa_atoms(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.gboxes, x.pbc, (int)x.su.nb, x.p->d_a.p,
                (int)x.d.a.size(), x.p->d_b.p, (int)x.d.b.size(), x.sorted, x.cell_start, x.npad, x.ident, x.grid, x.p->d_sasa_ra.p,
                x.p->d_sasa_rb.p, x.p->sasa_rmax_env, x.p->d_sasa_w.p, x.p->d_sasa_pts.p, (int)x.d.sasa_npoints, x.d.rmax, x.closed,
                x.p->d_sasa_total.p + x.su.off, x.acc, x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_sasa_brute(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.fboxes, x.pbc, (int)x.su.nb, x.p->d_a.p,
                (int)x.d.a.size(), x.p->d_b.p, (int)x.d.b.size(), x.ident, x.p->d_sasa_ra.p, x.p->d_sasa_rb.p, x.p->sasa_rmax_env,
                x.p->d_sasa_w.p, x.p->d_sasa_pts.p, (int)x.d.sasa_npoints, x.d.rmax, x.closed, x.p->d_sasa_total.p + x.su.off, x.acc,
                x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_sasa_finish(x.s, x.p->d_sasa_total.p + x.su.off, (int)x.su.nb, x.p->d_out.p + x.su.off, x.acc + x.d.a.size(),
                x.overflow);
    },
    nullptr};

// (contacts: every sub has its own rows of the batch's bit matrix - cleared by the launch, so also in a repeated batch - and of the counts;
// the native pairs, where the statement has any, stand as a third property behind the record)
static size_t contact_words(const Property& d) { return ((size_t)d.K * (size_t)(d.K - 1) / 2 + 31) / 32; }
static int contact_nnative(const Property& d) { return (int)(d.ct_native.size() / 2); }
static const NeighbourKind kContacts = {
    2, &vmd_script_eval_t::contact_props, "contact_atoms", "contact_brute", "contact_finish",
    [](vmd_script_eval_t* e, int pi) {
        PropState* m = record_behind(e, pi, Form::CONTACT_OCC, "contact count '%s' has lost its record");
        if (m && contact_nnative(e->props[pi]->prop) &&
            !((size_t)pi + 2 < e->props.size() && e->props[pi + 2]->prop.form == Form::CONTACT_NATIVE)) {
            vmd_fail("contact count '%s' has lost its record", e->props[pi]->prop.name.c_str());
            return (PropState*)nullptr;
        }
        return m;
    },
    [](PropState* p, size_t nb) {
        return p->d_out.ensure(nb) && (!contact_nnative(p->prop) || p->d_ct_q.ensure(nb)) && p->d_ct_count.ensure(2 * nb) &&
               p->d_ct_bits.ensure(nb * contact_words(p->prop));
    },
    [](const NeighbourSub& x) {
        return vmd_hip_contact_atoms(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.gboxes, x.pbc, (int)x.su.nb, x.p->d_a.p, x.p->d_c.p,
                (int)x.d.a.size(), (int)x.d.K, x.d.ct_min_sep, x.sorted, x.cell_start, x.npad, x.ident, x.grid, x.d.rmax, x.closed,
                g_opt.contact_lds_rows.load(), x.p->d_ct_bits.p + x.su.off * contact_words(x.d), x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_contact_brute(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.fboxes, x.pbc, (int)x.su.nb, x.p->d_a.p, x.p->d_c.p,
                (int)x.d.a.size(), (int)x.d.K, x.d.ct_min_sep, x.ident, x.d.rmax, x.closed,
                x.p->d_ct_bits.p + x.su.off * contact_words(x.d), x.overflow);
    },
    [](const NeighbourSub& x) {
        const int nnative = contact_nnative(x.d);
        return vmd_hip_contact_finish(x.s, x.p->d_ct_bits.p + x.su.off * contact_words(x.d), (int)x.su.nb, (int)x.d.K, x.p->d_ct_native.p,
                nnative, x.p->d_ct_count.p + 2 * x.su.off, x.p->d_out.p + x.su.off, nnative ? x.p->d_ct_q.p + x.su.off : nullptr, x.acc,
                x.overflow);
    },
    [](RangeRun& r, BatchCtx& c, int pi, PropState* p) { return !contact_nnative(p->prop) || r.queue_temporal_rows(c, pi + 2, p->d_ct_q.p); }};

// (clusters, DESIGN 1.17: every sub has its own rows of the batch's union-find - parent preset by the walk's and all pairs' launch, size
// and the counts zeroed by the finish's, so also in a repeated batch; the largest cluster stands as a third property behind the record)
static const NeighbourKind kClusters = {
    3, &vmd_script_eval_t::cluster_props, "cluster_atoms", "cluster_brute", "cluster_finish",
    [](vmd_script_eval_t* e, int pi) {
        PropState* m = record_behind(e, pi, Form::CLUSTER_SIZES, "cluster count '%s' has lost its record");
        if (m && !((size_t)pi + 2 < e->props.size() && e->props[pi + 2]->prop.form == Form::CLUSTER_LARGEST)) {
            vmd_fail("cluster count '%s' has lost its largest cluster", e->props[pi]->prop.name.c_str());
            return (PropState*)nullptr;
        }
        return m;
    },
    [](PropState* p, size_t nb) {
        const size_t G = p->prop.K;
        return p->d_out.ensure(nb) && p->d_cl_largest.ensure(nb) && p->d_cl_count.ensure(2 * nb) && p->d_cl_parent.ensure(nb * G) &&
               p->d_cl_root.ensure(nb * G) && p->d_cl_size.ensure(nb * G);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_cluster_atoms(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.gboxes, x.pbc, (int)x.su.nb, x.p->d_a.p, x.p->d_c.p,
                (int)x.d.a.size(), (int)x.d.K, x.sorted, x.cell_start, x.npad, x.ident, x.grid, x.d.rmax, x.closed,
                g_opt.cluster_skip_same.load(), x.p->d_cl_parent.p + x.su.off * x.d.K, x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_cluster_brute(x.s, x.xyz, x.st.frame_stride, x.st.row_stride, x.fboxes, x.pbc, (int)x.su.nb, x.p->d_a.p, x.p->d_c.p,
                (int)x.d.a.size(), (int)x.d.K, x.d.rmax, x.closed, x.p->d_cl_parent.p + x.su.off * x.d.K, x.overflow);
    },
    [](const NeighbourSub& x) {
        return vmd_hip_cluster_finish(x.s, x.p->d_cl_parent.p + x.su.off * x.d.K, x.p->d_cl_root.p + x.su.off * x.d.K,
                x.p->d_cl_size.p + x.su.off * x.d.K, (int)x.su.nb, (int)x.d.K, x.p->d_cl_count.p + 2 * x.su.off, x.p->d_out.p + x.su.off,
                x.p->d_cl_largest.p + x.su.off, x.acc, g_opt.cluster_wave_singles.load(), x.overflow);
    },
    [](RangeRun& r, BatchCtx& c, int pi, PropState* p) { return r.queue_temporal_rows(c, pi + 2, p->d_cl_largest.p); }};

// Every statement's cell build, of all four kinds, as ONE step in front of the first accumulation: no cell build of the batch may stand
// behind any kind's atomics.  By within_route's RULE: sel_a in the lanes, sel_b alone sorted (contacts: the one list on both sides), on the
// grid a within count of the radius rmax gets; all pairs below shell_brute_below entries of sel_b or where no grid exists -> per statement
// 1 the walk, 0 all pairs.  The ORDER of the builds - accessible area, contacts, clusters, hydrogen bonds - is part of the behaviour: where two
// statements sort one selection on different grids the later build wins, and the earlier statement falls back to all pairs (ident_table).
bool RangeRun::build_neighbour_cells(BatchCtx& c) {
    for (const NeighbourKind* k : {&kSasa, &kContacts, &kClusters, &kHbonds}) {
        std::vector<int>& route = neighbour_route[k->slot];
        route.clear();
        for (int pi : e->*(k->props)) {
            PropState* p = e->props[pi].get();
            vmd_grid_t grid;
            const float* d_gb = nullptr;
            route.push_back(within_route(c, e->sels[p->sel_a].get(), e->sels[p->sel_b].get(), p->prop.rmax, true, &grid, &d_gb));
            if (route.back() < 0) return false;
        }
    }
    return true;
}

bool RangeRun::launch_neighbours(BatchCtx& c, const NeighbourKind& k) {
    const std::vector<int>& props = e->*(k.props);
    const Stage& st = *c.src;
    for (size_t i = 0; i < props.size(); ++i) {
        const int pi = props[i];
        PropState* p = e->props[pi].get();
        PropState* m = k.record(e, pi);
        if (!m) return false;
        Selection* sr = e->sels[p->sel_b].get();
        vmd_grid_t grid{};
        const float* d_gb = nullptr;
        int have_grid = 0;
        if (!k.ensure(p, c.nb) || !ident_table(c, p, neighbour_route[k.slot][i], &have_grid, &grid, &d_gb)) return false;
        const size_t ident_row = have_grid ? (size_t)sr->nsel_pad : sr->idx.size();
        auto sub = [&](const Sub& su) {
            return NeighbourSub{e->stream, e->d_overflow.p, p, p->prop, acc_of(m, su), st, su, c.pbc, e->spec.within_closed ? 1 : 0,
                    st.base + su.off * st.frame_stride, st.d_boxes.p + 9 * su.off, grid, have_grid ? d_gb + 9 * su.off : nullptr,
                    have_grid ? sr->sorted.p + su.off * 3 * (size_t)sr->nsel_pad : nullptr,
                    have_grid ? sr->cell_start.p + su.off * (size_t)(grid.ncell + 1) : nullptr, sr->nsel_pad,
                    p->d_hb_ident.p + su.off * ident_row};
        };
        e->prof.begin(have_grid ? k.walk_label : k.brute_label, e->stream);
        for (auto& su : c.subs) {
            const NeighbourSub x = sub(su);
            KRN_OK(have_grid ? k.walk(x) : k.brute(x));
            if (!k.finish_label) KRN_OK(k.finish(x));
        }
        e->prof.end(e->stream);
        if (k.finish_label) {
            e->prof.begin(k.finish_label, e->stream);
            for (auto& su : c.subs) KRN_OK(k.finish(sub(su)));
            e->prof.end(e->stream);
        }
        if (!queue_temporal_rows(c, pi, p->d_out.p) || (k.more_rows && !k.more_rows(*this, c, pi, p))) return false;
    }
    return true;
}

// ---- shell expressions: one pass per term over T in atom order, ascending |R_i|, then the finish.  Walk or all pairs per term
// by within_route's RULE; the cell-sorted copies come from build_pair, so one that another pass of the batch built on the same grid is
// reused.  The bits start clean in every batch and in every repeat of one; the counts travel to the host from here, like
// launch_within_counts' rows and for the same reason.
bool RangeRun::launch_shell_exprs(BatchCtx& c) {
    const bool skip = g_opt.shell_expr_skip.load() != 0;
    const int closed = e->spec.within_closed ? 1 : 0;
    for (auto& xp : e->exprs) {
        ShellExpr* x = xp.get();
        Selection* st = e->sels[x->sel_t].get();
        const size_t stride = c.src->row_stride;
        if (x->stride != stride || c.nb * stride > x->mask.cap) {
            if (!x->mask.ensure(c.nb * stride) || !x->bits.ensure(c.nb * stride)) return false;
            HIP_OK(hipMemsetAsync(x->mask.p, 0, x->mask.cap, e->stream));          // atoms outside T read 0 for ever
            x->stride = stride;
        }
        if (!x->count.ensure(c.nb)) return false;
        HIP_OK(hipMemsetAsync(x->bits.p, 0, c.nb * stride, e->stream));
        for (size_t pos = 0; pos < x->order.size(); ++pos) {
            const int i = x->order[pos];
            const ShellExpr::Term& tm = x->terms[i];
            const uint32_t live = skip ? shell_expr_live(x->truth, x->order, pos) : 0xffffu;
            if (!live || tm.sel_tt < 0) continue;              // the table ignores the term here, or T minus R_i is empty: h_i reads 0
            Selection* tt = e->sels[tm.sel_tt].get();
            Selection* sr = e->sels[tm.sel_r].get();
            vmd_grid_t grid;
            const float* d_gb = nullptr;
            const int have_grid = within_route(c, st, sr, tm.rmax, true, &grid, &d_gb);
            if (have_grid < 0) return false;
            if (have_grid) {
                e->prof.begin("shell_expr", e->stream);
                KRN_OK(vmd_hip_within_atoms_expr(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, d_gb, c.pbc, (int)c.nb,
                        tt->d_idx.p, (int)tt->idx.size(), sr->sorted.p, sr->cell_start.p, (int)sr->idx.size(), sr->nsel_pad, grid, tm.rmin,
                        tm.rmax, closed, i, live, x->bits.p, stride, e->d_overflow.p));
                e->prof.end(e->stream);
            } else {
                e->prof.begin("shell_expr_brute", e->stream);
                KRN_OK(vmd_hip_within_brute_expr(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc,
                        (int)c.nb, tt->d_idx.p, (int)tt->idx.size(), sr->d_idx.p, (int)sr->idx.size(), tm.rmin, tm.rmax, closed, i, live,
                        x->bits.p, stride, e->d_overflow.p));
                e->prof.end(e->stream);
            }
        }
        e->prof.begin("shell_expr_finish", e->stream);
        KRN_OK(vmd_hip_shell_expr_finish(e->stream, (int)c.nb, st->d_idx.p, (int)st->idx.size(), x->bits.p, x->truth, x->mask.p, stride,
                x->count.p, e->d_overflow.p));
        e->prof.end(e->stream);
    }
    for (int pi : e->expr_count_props) {
        PropState* p = e->props[pi].get();
        if (!p->d_out.ensure(c.nb)) return false;
        KRN_OK(vmd_hip_within_to_float(e->stream, e->exprs[p->expr_of]->count.p, (int)c.nb, p->d_out.p, e->d_overflow.p));
        if (!queue_temporal_rows(c, pi, p->d_out.p)) return false;
    }
    return true;
}

// the scatter of an sdf over a shell expression: all or nothing behind the overflow flag, as launch_shell_sdfs
bool RangeRun::launch_expr_sdfs(BatchCtx& c) {
    for (int pi : e->expr_sdf_props) {
        PropState* p = e->props[pi].get();
        const ShellExpr* x = e->exprs[p->expr_of].get();
        if (!launch_sdf(c, p, x->mask.p, x->stride)) return false;
    }
    return true;
}

// ---- everything of a batch that a cell build takes part in; runs again for the batch when a bucket of one overflowed (complete_batch).
// Every pass accumulates into its own scratch row and the rows are committed to the properties' accumulators by ONE
// group of k_axpy_u64 launches at the very end, behind the overflow flag: by then every cell build of the batch has run,
// so the flag is final and the batch's RDF part is all-or-nothing (a bucket of a LATER build may overflow after earlier
// passes have long finished; nothing of them may stay behind when the batch is repeated).
bool RangeRun::launch_rdf(BatchCtx& c) {
    VMD_STAGE("batch: cell build + pair kernels");
    vmd_hip_set_rdf_closed(e->spec.rdf_closed ? 1 : 0);
    vmd_hip_set_rdf_raw(e->spec.rdf_raw ? 1 : 0);
    size_t scratch_rows = 0;
    for (auto& g : e->rdf_groups) scratch_rows += std::max(g.passes.size(), g.props.size()) + g.shell_props.size();
    scratch_rows *= c.subs.size();
    if (!e->d_pass.ensure(std::max<size_t>(scratch_rows, 1) * VMD_RDF_NUM_BINS)) return false;
    if (scratch_rows) HIP_OK(hipMemsetAsync(e->d_pass.p, 0, scratch_rows * VMD_RDF_NUM_BINS * sizeof(uint64_t), e->stream));
    commits.clear();
    row = 0;
    forked = false;
    if (!launch_rdf_groups(c) || !launch_within_counts(c) || !launch_shell_masks(c) || !launch_shell_exprs(c) || !build_neighbour_cells(c) ||
        !launch_neighbours(c, kHbonds) || !launch_neighbours(c, kSasa) || !launch_neighbours(c, kContacts) || !launch_neighbours(c, kClusters) ||
        !launch_shell_sdfs(c) ||
        !launch_expr_sdfs(c)) return false;
    for (auto& cm : commits) KRN_OK(vmd_hip_axpy_u64(e->stream, cm.dst, cm.src, VMD_RDF_NUM_BINS, cm.mult, e->d_overflow.p));
    HIP_OK(hipMemcpyAsync(&e->h_overflow[c.slot], e->d_overflow.p, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    return true;
}

// ---- an sdf's alignment and scatter over the batch.  mask: the shell the targets are taken from (launch_shell_sdfs) -
// or the shell expression (launch_expr_sdfs): the atom-order mask gates the scatter, which then tests the overflow flag;
// nullptr: a static sdf, gated by its own tag list
bool RangeRun::launch_sdf(BatchCtx& c, PropState* p, const uint8_t* mask, size_t mask_stride) {
    const Property& d = p->prop;
    if (!p->d_R32.ensure(c.nb * d.K * 9) || !p->d_c32.ensure(c.nb * d.K * 3) || !p->d_group.ensure(c.nb * 4)) return false;
    e->prof.begin("sdf_align", e->stream);
    if (p->have_tree && !p->d_tree_pos.ensure(c.nb * d.K * d.m * 3)) return false;
    KRN_OK(vmd_hip_sdf_align(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc,
            (int)c.nb, p->d_structs.p, p->d_mass.p, (int)d.K, (int)d.m, p->d_ref_pose.p, p->d_R32.p, p->d_c32.p, nullptr,
            p->d_group.p, p->have_tree ? p->d_tree_order.p : nullptr, p->have_tree ? p->d_tree_parent.p : nullptr, p->have_tree
            ? p->d_tree_pos.p : nullptr));
    e->prof.end(e->stream);
    e->prof.begin("sdf_scatter", e->stream);
    for (auto& su : c.subs) {
        if (mask) KRN_OK(vmd_hip_sdf_scatter_masked(e->stream, c.src->base + su.off * c.src->frame_stride,
                c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p + 9 * su.off, c.pbc, (int)su.nb, p->d_structs.p, (int)d.K,
                (int)d.m, p->d_R32.p + su.off * d.K * 9, p->d_c32.p + su.off * d.K * 3, p->d_tgt.p, (p->have_owner
                && !e->spec.sdf_include_self) ? p->d_owner.p : nullptr, (int)d.b.size(), d.rmax, VMD_VOLUME_DIM, acc_of(p, su),
                p->d_group.p + 4 * su.off, p->tgt_first, p->tgt_stride, (p->unowned || e->spec.sdf_include_self) ? 1 : 0,
                mask + su.off * mask_stride, mask_stride, e->d_overflow.p));
        else KRN_OK(vmd_hip_sdf_scatter(e->stream, c.src->base + su.off * c.src->frame_stride,
                c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p + 9 * su.off, c.pbc, (int)su.nb, p->d_structs.p, (int)d.K,
                (int)d.m, p->d_R32.p + su.off * d.K * 9, p->d_c32.p + su.off * d.K * 3, p->d_tgt.p, (p->have_owner
                && !e->spec.sdf_include_self) ? p->d_owner.p : nullptr, (int)d.b.size(), d.rmax, VMD_VOLUME_DIM, acc_of(p, su),
                p->d_group.p + 4 * su.off, (p->have_tag && p->tag_len == c.src->row_stride && !e->spec.sdf_include_self)
                ? p->d_tag.p : nullptr, p->tgt_first, p->tgt_stride, (p->unowned || e->spec.sdf_include_self) ? 1 : 0));
    }
    e->prof.end(e->stream);
    return true;
}

// shape_weights: the statement's three descriptors stand in a row; the first one computes all three [nb][P] blocks,
// each of them copies its own (queue_batch)
bool RangeRun::launch_shape(BatchCtx& c, size_t pi) {
    PropState* p = e->props[pi].get();
    if (p->prop.shape_comp != 0) return true;
    if (pi + 2 >= e->props.size() || e->props[pi + 1]->prop.form != Form::SHAPE || e->props[pi + 2]->prop.form != Form::SHAPE)
        return vmd_fail("shape_weights property '%s' has lost its companions", p->prop.name.c_str());
    PropState* p1 = e->props[pi + 1].get();
    PropState* p2 = e->props[pi + 2].get();
    if (!p1->d_out.ensure(c.nb * p->dim1) || !p2->d_out.ensure(c.nb * p->dim1)) return false;
    if (!p->d_shape_partial.ensure(vmd_hip_shape_partial_doubles((int)c.nb, (int)p->dist_P, p->shape_max_set))) return false;
    e->prof.begin("shape", e->stream);
    KRN_OK(vmd_hip_shape(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc, (int)c.nb,
            (int)p->dist_P, p->d_a.p, p->d_ma.p, p->d_aoff.p, p->shape_max_set, p->d_shape_partial.p, p->d_out.p,
            p1->d_out.p, p2->d_out.p));
    e->prof.end(e->stream);
    return true;
}

// rmsd: the same [nb][P] block, the same copy; the batch knows which of its rows is frame 0
bool RangeRun::launch_rmsd(BatchCtx& c, PropState* p) {
    const size_t ws = vmd_hip_rmsd_workspace_bytes((int)c.nb, (int)p->dist_P, p->rmsd_max_set);
    if (!p->d_rmsd_ws.ensure((ws + 7) / 8)) return false;
    e->prof.begin("rmsd", e->stream);
    KRN_OK(vmd_hip_rmsd(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc, (int)c.nb,
            (int)p->dist_P, p->d_a.p, p->d_ma.p, p->d_aoff.p, p->rmsd_max_set, p->d_rmsd_pose.p, p->d_rmsd_const.p,
            c.f0 == 0 ? 0 : -1, p->d_rmsd_ws.p, p->d_out.p));
    e->prof.end(e->stream);
    return true;
}

// rmsf: the sums of the batch - left in its workspace by the rmsd property in front over the same sets, if there is one -,
// the rotations, then the second pass per sub, so that a frame block's frames land in its own partial.  No cell grid, no overflow flag:
// a batch repeated for an overflow does not come here again.  A frame evaluated twice is counted twice, as a map counts it.
bool RangeRun::launch_rmsf(BatchCtx& c, size_t pi) {
    PropState* p = e->props[pi].get();
    PropState* s = p->rmsf_of >= 0 && (size_t)p->rmsf_of < pi ? e->props[(size_t)p->rmsf_of].get() : p;     // whose pose, sums and shifts
    if (s != p && (!s->rmsd_pose_ready || s->prop.form != Form::RMSD))
        return vmd_fail("rmsf property '%s' has lost the rmsd property it reads", p->prop.name.c_str());
    const int B = (int)c.nb, P = (int)p->dist_P;
    if (s == p && !p->d_rmsd_ws.ensure((vmd_hip_rmsd_workspace_bytes(B, P, p->rmsd_max_set) + 7) / 8)) return false;
    if (!p->d_rmsf_rot.ensure(vmd_hip_rmsf_rot_doubles(B, P))) return false;
    const Stage& st = *c.src;
    e->prof.begin("rmsf_rotation", e->stream);
    KRN_OK(vmd_hip_rmsf_fit(e->stream, st.base, st.frame_stride, st.row_stride, st.d_boxes.p, c.pbc, B, P, p->d_a.p, p->d_ma.p, p->d_aoff.p,
            p->rmsd_max_set, s->d_rmsd_pose.p, s->d_rmsd_const.p, s->d_rmsd_ws.p, s != p ? 1 : 0, p->d_rmsf_rot.p));
    e->prof.end(e->stream);
    e->prof.begin("rmsf", e->stream);
    for (auto& su : c.subs)
        KRN_OK(vmd_hip_rmsf_accumulate(e->stream, st.base, st.frame_stride, st.row_stride, st.d_boxes.p, c.pbc, B, P, p->d_a.p, p->d_ma.p,
                p->d_aoff.p, p->rmsd_max_set, s->d_rmsd_pose.p, s->d_rmsd_const.p, c.f0 == 0 ? 0 : -1, s->d_rmsd_ws.p, p->d_rmsf_rot.p,
                (int)su.off, (int)su.nb, p->rmsf_groups, acc_of(p, su)));
    e->prof.end(e->stream);
    return true;
}

// angle / dihedral (DESIGN S6b): the same [nb][P] block, the same copy
bool RangeRun::launch_geometry(BatchCtx& c, PropState* p) {
    const int32_t* sets[4] = {p->d_a.p, p->d_b.p, p->d_c.p, p->d_d.p};
    const float* ms[4] = {p->d_ma.p, p->d_mb.p, p->d_mc.p, p->d_md.p};
    const int32_t* offs[4] = {p->d_aoff.p, p->d_boff.p, p->d_coff.p, p->d_doff.p};
    e->prof.begin("geometry", e->stream);
    KRN_OK(vmd_hip_geometry(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc, (int)c.nb,
            p->prop.nargs(), (int)p->dist_P, sets, ms, offs, e->spec.angle_radians ? 1 : 0, p->d_out.p));
    e->prof.end(e->stream);
    return true;
}

// ramachandran: phi / psi of the batch into its rows of the device table, then those rows binned into the map behind the
// table - per sub, so that a frame block's samples land in its own partial.  The rows travel to the host from the table (queue_batch).
// No cell grid, no overflow flag; a frame evaluated twice is counted twice, as an sdf volume counts it.
bool RangeRun::launch_rama(BatchCtx& c, size_t pi) {
    PropState* p = e->props[pi].get();
    if (pi + 1 >= e->props.size() || e->props[pi + 1]->prop.form != Form::RAMA_MAP)
        return vmd_fail("ramachandran table '%s' has lost its map", p->prop.name.c_str());
    PropState* m = e->props[pi + 1].get();
    const size_t nseg = p->prop.a.size();
    float* rows = p->d_table.p + c.f0 * p->dim1;
    e->prof.begin("backbone_angles", e->stream);
    KRN_OK(vmd_hip_backbone_angles(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc, (int)c.nb,
            (int)nseg, p->d_a.p, p->d_b.p, p->d_c.p, p->d_rama_link.p, rows));
    e->prof.end(e->stream);
    e->prof.begin("rama_bin", e->stream);
    for (auto& su : c.subs)
        KRN_OK(vmd_hip_rama_bin(e->stream, rows + su.off * p->dim1, (int)su.nb, nullptr, (int)nseg, p->d_rama_class.p, p->d_rama_link.p,
                e->spec.rama_skip_ends ? 1 : 0, acc_of(m, su), nullptr));
    e->prof.end(e->stream);
    return true;
}

// position table: the batch's rows of the device table, written in place; they travel to the host from the table
// (queue_batch).  No cell grid, no overflow flag, nothing accumulated: a frame evaluated twice gets the same row twice.
bool RangeRun::launch_msd(BatchCtx& c, PropState* p) {
    e->prof.begin("msd_gather", e->stream);
    // (the cells' own flags, which no frame of a trajectory may change - not c.pbc, which drops an axis for the whole batch when the edge of
    // its FIRST frame is not positive: the gather looks at every frame's own edge, so a row is the same whatever batch writes it)
    KRN_OK(vmd_hip_msd_gather(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p,
            c.src->cells[0].flags & VMD_UNITCELL_PBC_ALL, (int)c.nb, p->d_a.p,
            (int)p->prop.a.size(), p->d_table.p + c.f0 * p->dim1));
    e->prof.end(e->stream);
    return true;
}

// secondary structure: the class rows [nb][nseg] and, in the descriptor behind, the populations [nb][9]; each copies its own
// (queue_batch).  The bit matrices take nseg^2 / 2 bytes per frame: the batch runs in as many sub-batches of frames as the eval's bound
// (ss_scratch_bytes) and the launch limit of 2^31 - 1 words ask for, one after another over the same scratch, never below one frame.
bool RangeRun::launch_ss(BatchCtx& c, size_t pi) {
    PropState* p = e->props[pi].get();
    if (pi + 1 >= e->props.size() || e->props[pi + 1]->prop.form != Form::SS_POP)
        return vmd_fail("secondary_structure table '%s' has lost its populations", p->prop.name.c_str());
    PropState* q = e->props[pi + 1].get();
    if (!q->d_out.ensure(c.nb * q->dim1)) return false;
    const size_t nseg = p->prop.a.size();
    const size_t frame_words = vmd_hip_ss_scratch_words(1, (int)nseg);
    if (frame_words / 4 > 0x7fffffffull) return vmd_fail("secondary_structure: %zu segments exceed the launch limit", nseg);
    size_t step = std::max<size_t>(1, e->ss_scratch_bytes / (frame_words * sizeof(uint64_t)));
    step = std::min(std::min(step, c.nb), (size_t)0x7fffffffull / (frame_words / 4));
    if (!e->d_ss_scratch.ensure(step * frame_words)) return false;
    const Stage& s = *c.src;
    for (size_t f = 0; f < c.nb; f += step) {
        const int nf = (int)std::min(step, c.nb - f);
        const float* xyz = s.base + f * s.frame_stride;
        const float* boxes = s.d_boxes.p + 9 * f;
        e->prof.begin("ss_hbond", e->stream);
        KRN_OK(vmd_hip_ss_hbond(e->stream, xyz, s.frame_stride, s.row_stride, boxes, c.pbc, nf, (int)nseg, p->d_a.p, p->d_b.p, p->d_c.p,
                p->d_ss_o.p, p->d_ss_rng.p, p->d_ss_pro.p, p->d_ss_nb.p, e->d_ss_scratch.p));
        e->prof.end(e->stream);
        e->prof.begin("ss_bridges", e->stream);
        KRN_OK(vmd_hip_ss_bridges(e->stream, xyz, s.frame_stride, s.row_stride, boxes, c.pbc, nf, (int)nseg, p->d_a.p, p->d_b.p, p->d_c.p,
                p->d_ss_o.p, p->d_ss_rng.p, p->d_ss_pro.p, p->d_ss_nb.p, e->d_ss_scratch.p));
        e->prof.end(e->stream);
        e->prof.begin("ss_assign", e->stream);
        KRN_OK(vmd_hip_ss_assign(e->stream, xyz, s.frame_stride, s.row_stride, boxes, c.pbc, nf, (int)nseg, p->d_a.p, p->d_b.p, p->d_c.p,
                p->d_ss_o.p, p->d_ss_rng.p, p->d_ss_pro.p, p->d_ss_nb.p, e->d_ss_scratch.p, p->d_out.p + f * nseg, q->d_out.p + f * q->dim1));
        e->prof.end(e->stream);
    }
    return true;
}

bool RangeRun::launch_distance(BatchCtx& c, PropState* p) {
    e->prof.begin("distance", e->stream);
    KRN_OK(vmd_hip_distance(e->stream, c.src->base, c.src->frame_stride, c.src->row_stride, c.src->d_boxes.p, c.pbc, (int)c.nb,
            p->prop.distance_kind, (int)p->dist_P, (int)p->dist_per, p->d_a.p, p->d_ma.p, p->d_aoff.p, p->d_b.p, p->d_mb.p, p->d_boff.p,
            p->d_out.p));
    e->prof.end(e->stream);
    return true;
}

// what property pi adds to the batch's queue outside launch_rdf, by form.  The rows of a temporal form are left in d_out.
bool RangeRun::launch_property(BatchCtx& c, size_t pi) {
    PropState* p = e->props[pi].get();
    const Property& d = p->prop;
    if (d.behind_cells()) {     // launched by launch_rdf: rdfs, within counts, everything over a shell or an expression (1.8, 1.9)
        // SPEC S4 normalisation, fp64 on the host (needs only the box).  An rdf over shells needs the populations too: its weights
        // are formed in complete_batch, when they have arrived
        if (d.form == Form::RDF && !d.is_shell_rdf()) rdf_weights(c, p);
        return true;
    }
    if (d.temporal() && !d.device_table() && !p->d_out.ensure(c.nb * p->dim1)) return false;     // (the table's rows have their place)
    switch (d.form) {
    case Form::RDF: case Form::WITHIN: case Form::WITHIN_EXPR: case Form::HBOND_COUNT: case Form::HBOND_OCC: case Form::SASA_AREA:
    case Form::SASA_OCC: case Form::CONTACT_COUNT: case Form::CONTACT_OCC: case Form::CONTACT_NATIVE: case Form::CLUSTER_COUNT: case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST: return true;     // (behind the cell builds, above)
    case Form::SDF: VMD_STAGE("batch: sdf align + scatter"); return launch_sdf(c, p, nullptr, 0);
    case Form::RAMA_MAP: return true;                                           // filled by the launch of the table in front of it
    case Form::RAMA_TABLE: return launch_rama(c, pi);
    case Form::MSD_TABLE: return launch_msd(c, p);
    case Form::SS_POP: return true;                                             // filled by the launch of the class table in front of it
    case Form::SS_CLASS: return launch_ss(c, pi);
    case Form::SHAPE: return launch_shape(c, pi);
    case Form::RMSD: return launch_rmsd(c, p);
    case Form::RMSF: return launch_rmsf(c, pi);
    case Form::ANGLE: case Form::DIHEDRAL: return launch_geometry(c, p);
    case Form::DISTANCE: return launch_distance(c, p);
    }
    return vmd_fail("property '%s' has no form", d.name.c_str());
}
