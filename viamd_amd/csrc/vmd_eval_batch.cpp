// viamd_amd/csrc/vmd_eval_batch.cpp - what a range run is built from: the two-level cell build per selection on the pencil grid of a
// batch (md_spatial_hash's role), batch sizes and batch planning, reuse of another eval's block partials (filtered evaluation,
// src/main.cpp:1014-1039 of VIAMD), which frames a device view holds - and, around a run, the refresh of the host views and the
// combining queue.  The run itself (process_range) is in vmd_eval_range.cpp, what its batches launch in vmd_eval_launch.cpp.
#include "vmd_eval_internal.h"

// Bucket capacities of the two-level build for selection `s` on the pencils of grid `g`: per-pencil maximum over the first and
// last (up to) 4 frames of the batch x margin + a few standard deviations.  One small readback, then kept for the eval's
// lifetime (frames of one trajectory look alike; a bucket that overflows later is caught by the device flag and re-measured).
bool ensure_pencil_caps(vmd_script_eval_t* e, Selection* s, const Stage& src, const float* d_boxes, uint32_t pbc, size_t nb,
        const vmd_grid_t& g) {
    if (!s->pen_off.empty() && s->pen_ny == g.ny && s->pen_nz == g.nz) return true;
    if (!s->pen_off.empty()) {                 // keep what was measured for the layout we are leaving
        bool known = false;
        for (auto& c : s->caps_cache) known = known || (c.ny == s->pen_ny && c.nz == s->pen_nz);
        if (!known) {
            if (s->caps_cache.size() >= 4) s->caps_cache.erase(s->caps_cache.begin());
            s->caps_cache.push_back({s->pen_ny, s->pen_nz, s->cap_max, s->total_cap, s->pen_off});
        }
    }
    for (auto& c : s->caps_cache) {
        if (c.ny != g.ny || c.nz != g.nz) continue;
        s->pen_off = c.pen_off; s->cap_max = c.cap_max; s->total_cap = c.total_cap; s->pen_ny = c.ny; s->pen_nz = c.nz;
        // pageable source: the copy is staged before the call returns
        return s->d_pen_off.upload(s->pen_off.data(), s->pen_off.size(), e->stream);
    }
    const int npen = g.ny * g.nz, nsel = (int)s->idx.size();
    // after an overflow: every frame of the batch (exact populations), otherwise 4 frames each from its beginning, middle and end (round 6:
    // the middle was not looked at, and a solute that wanders through the batch - config 5 - overflowed the solvent's buckets there)
    // (cells_cap_sample = 2: beginning and end only, as before - the overflow tests ask for it)
    const bool exhaustive = s->overflows > 0 || nb <= 8;
    const size_t nsamp = exhaustive ? 1 : (g_opt.cells_cap_sample.load() >= 3 ? 3 : 2);
    const size_t S = exhaustive ? nb : 4, rows = exhaustive ? nb : 4 * nsamp;
    if (!e->d_pen_sample.ensure(rows * (size_t)npen)) return false;
    std::vector<uint32_t> h(rows * (size_t)npen);
    const size_t starts[3] = {0, nsamp == 3 ? (nb - S) / 2 : nb - S, nb - S};
    for (size_t k = 0; k < nsamp; ++k)
        KRN_OK(vmd_hip_cells_pencil_count(e->stream, src.base + starts[k] * src.frame_stride, src.frame_stride, src.row_stride,
                d_boxes + 9 * starts[k], pbc, (int)S, s->d_idx.p, nsel, g, e->d_pen_sample.p + k * S * (size_t)npen));
    HIP_OK(hipMemcpyAsync(h.data(), e->d_pen_sample.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    s->pen_off.assign((size_t)npen + 1, 0);
    s->cap_max = 0;
    uint64_t total = 0;
    const double mean_pop = g_opt.cells_cap_floor.load() ? (double)nsel / (double)npen : 0.0;
    for (int p = 0; p < npen; ++p) {
        uint32_t m = 0;
        for (size_t k = 0; k < rows; ++k) m = std::max(m, h[k * npen + p]);
        uint32_t cap = (uint32_t)std::ceil((double)m * s->cap_margin + 6.0 * std::sqrt((double)m)) + 16;
        // ... but never below what a pencil holds at the selection's MEAN density (round 6).  A solute that sits in a pencil for the whole
        // of the batch the capacities were measured on (config 5's wandering blob) leaves that pencil's bucket too small for the batches in
        // which it has moved on: two overflows, i.e. two repeated batches, per evaluation of c5.  Costs at most 1.15 x nsel records.
        cap = std::max(cap, (uint32_t)std::ceil(mean_pop * 1.15 + 6.0 * std::sqrt(mean_pop)) + 16);
        cap = (cap + 3u) & ~3u;
        s->pen_off[p] = (uint32_t)total;
        total += cap;
        s->cap_max = std::max<int>(s->cap_max, (int)cap);
    }
    if (total > 0x7fffffffull) { s->pen_off.clear(); s->overflows = 99; return true; }     // not a job for the buckets
    s->pen_off[npen] = (uint32_t)total;
    s->total_cap = (int)total;
    s->pen_ny = g.ny; s->pen_nz = g.nz;
    return s->d_pen_off.upload(s->pen_off.data(), s->pen_off.size(), e->stream);
}

// the kernels of this selection's builds compute a periodic index list instead of reading it: set for the calls below, cleared on every way
// out
struct SelPatternScope {
    explicit SelPatternScope(const Selection* s) {
        if (s->pat_m) vmd_hip_set_cells_sel_pattern(s->pat_m, s->pat_first, s->pat_period, s->pat_off);
    }
    ~SelPatternScope() { vmd_hip_set_cells_sel_pattern(0, 0, 0, nullptr); }
};

bool build_selection(vmd_script_eval_t* e, Selection* s, const Stage& src, const float* d_boxes, uint32_t pbc, size_t nb,
        const vmd_grid_t& g) {
    if (s->built && s->built_grid.nxf == g.nxf && s->built_grid.ny == g.ny && s->built_grid.nz == g.nz) return true;
    const SelPatternScope pattern(s);
    const int nsel = (int)s->idx.size();
    s->nsel_pad = (nsel + 63) & ~63;
    // +64: the pair kernel prefetches past a segment
    if (!s->cell_start.ensure(nb * (size_t)(g.ncell + 1)) || !s->sorted.ensure(nb * 3 * (size_t)s->nsel_pad + 64)) return false;
    s->used_pencil = false;
    // two-level build through per-pencil buckets (one read of the frame, coalesced sorted rows); single-level builds otherwise A small
    // selection (a solute: the 2 000-atom blob of config 5) is not spread evenly over the pencils and wanders through them as the
    // trajectory goes on: capacities measured on one batch overflow in the next, and every overflow repeats the batch's pair passes.  It is
    // sorted by ONE block per frame in LDS instead (k_cells_fused: no buckets, nothing to overflow), which costs such a selection nothing.
    // (round 6: whether or not the grid's cell table fits the fused kernel's LDS - c5's 30 000 cells do not, and its 1 200-atom solute
    // class went through the buckets after all: one overflow, i.e. one repeated batch, in each of an evaluation's first two passes.  The
    // single-level builds behind vmd_hip_cells_build pick the fused, the split or the atomic three-kernel variant themselves.)
    const bool small = nsel <= g_opt.cells_small.load();
    if (vmd_hip_cells_pencil_ok(g) && s->overflows < 3 && !small) {
        if (!ensure_pencil_caps(e, s, src, d_boxes, pbc, nb, g)) return false;
        if (!s->pen_off.empty() && s->cap_max <= vmd_hip_cells_pencil_cap_max()) {
            const size_t npen = (size_t)g.ny * g.nz;
            if (!s->pen_count.ensure(nb * npen) || !s->pen_start.ensure(nb * (npen + 1)) || !s->bucket.ensure(nb * (size_t)s->total_cap
                    * 4)) return false;
            e->prof.begin("cells_build", e->stream);
            vmd_hip_set_cells_overflow_bit(s->overflow_bit);
            KRN_OK(vmd_hip_cells_build_pencil(e->stream, src.base, src.frame_stride, src.row_stride, d_boxes, pbc, (int)nb, s->d_idx.p,
                    nsel, s->nsel_pad, g, s->d_pen_off.p, s->total_cap, s->cap_max, s->pen_count.p, s->pen_start.p, s->bucket.p,
                    e->d_overflow.p, s->cell_start.p, s->sorted.p));
            e->prof.end(e->stream);
            s->built = true; s->built_grid = g; s->used_pencil = true;
            return true;
        }
    }
    if (!s->cell_count.ensure(nb * (size_t)(g.ncell + 1)) || !s->rank.ensure(nb * vmd_hip_cells_scratch_words(g, nsel))) return false;
    const bool use_aos = g_opt.cells_aos != 0;
    if (use_aos && !s->aos.ensure(nb * 4 * (size_t)s->nsel_pad)) return false;
    e->prof.begin("cells_build", e->stream);
    KRN_OK(vmd_hip_cells_build(e->stream, src.base, src.frame_stride, src.row_stride, d_boxes, pbc, (int)nb, s->d_idx.p, nsel,
                               s->nsel_pad, g, s->cell_count.p, s->rank.p, s->cell_start.p, s->sorted.p, use_aos ? s->aos.p : nullptr));
    e->prof.end(e->stream);
    s->built = true;
    s->built_grid = g;
    return true;
}

size_t auto_batch(const vmd_script_eval_t* e, size_t num_atoms, bool staged) {
    const int forced = g_opt.batch_frames;
    if (forced > 0) return (size_t)forced;
    // scratch per frame: a selection that takes part in a pair pass holds ~40 B per atom (sorted rows, bucket records, tables);
    // host trajectories add the staged frame itself; SDF / distance properties need a few hundred bytes
    size_t per_frame = staged ? 12 * num_atoms : 0;
    std::vector<char> used(e->sels.size(), 0);
    for (auto& g : e->rdf_groups) for (auto& ps : g.passes) { used[ps.sel_a] = 1; used[ps.sel_b] = 1; }
    for (int pi : e->within_props) { if (e->props[pi]->sel_a >= 0) used[e->props[pi]->sel_a] = 1; used[e->props[pi]->sel_b] = 1; }
    // hydrogen bonds: the acceptors sorted, and four bytes per sorted slot for their identity
    for (int pi : e->hbond_props) { used[e->props[pi]->sel_b] = 1; per_frame += 4 * (e->sels[e->props[pi]->sel_b]->idx.size() + 64); }
    // accessible area: the environment sorted, four bytes per sorted slot for its identity
    for (int pi : e->sasa_props) { used[e->props[pi]->sel_b] = 1; per_frame += 4 * (e->sels[e->props[pi]->sel_b]->idx.size() + 64); }
    // contact maps: the entry list sorted and identified, and the frame's row of the bit matrix (256 KB at 2048 groups)
    for (int pi : e->contact_props) {
        const size_t G = e->props[pi]->prop.K;
        used[e->props[pi]->sel_b] = 1;
        per_frame += 4 * (e->sels[e->props[pi]->sel_b]->idx.size() + 64) + (G * (G - 1) / 2 + 31) / 32 * 4 + 8;
    }
    // clusters: the entry list sorted and identified, and the frame's rows of the union-find - parent, root, size - and counts
    for (int pi : e->cluster_props) {
        used[e->props[pi]->sel_b] = 1;
        per_frame += 4 * (e->sels[e->props[pi]->sel_b]->idx.size() + 64) + 12 * e->props[pi]->prop.K + 8;
    }
    for (auto& g : e->rdf_groups)
        for (int pi : g.shell_props) for (int sl : {e->props[pi]->sel_a, e->props[pi]->sel_b}) if (sl >= 0) used[sl] = 1;
    // a shell keeps a hit copy the size of its parent's sorted rows, one byte per entry and its tables
    // ... and an sdf over it one byte per atom of the frame, the mask in atom order; R is sorted for either
    for (auto& h : e->shells) {
        used[h->sel_r] = 1;
        if (h->sel_t < 0) continue;
        if (h->rdf_use) per_frame += 24 * e->sels[h->sel_t]->idx.size();
        if (h->sdf_use) per_frame += num_atoms + 64;
    }
    // a shell expression: two bytes per atom of the frame - the term outcomes and the mask -, every R_i sorted
    for (auto& x : e->exprs) {
        for (auto& tm : x->terms) used[tm.sel_r] = 1;
        per_frame += 2 * (num_atoms + 64);
    }
    for (size_t i = 0; i < e->sels.size(); ++i) if (used[i]) per_frame += 40 * e->sels[i]->idx.size();
    for (auto& p : e->props) per_frame += p->prop.form == Form::SDF ? 64 * p->prop.K : (p->prop.temporal() ? 4 * p->dim1 : 0);
    // 288 GB of HBM: a 16 GB scratch budget holds the 1 000 frames of the 1M-atom RDF (333k selected atoms) in ONE batch
    // (every batch boundary costs ~1 ms of host round trips against ~37 ms of kernels per 500 frames)
    size_t B = (size_t)(16ull << 30) / std::max<size_t>(per_frame, 1);
    // pair passes are long (a 1 024-frame batch of the 1M-atom RDF runs ~90 ms: interrupts are polled between batches); scripts
    // without them stream whole frames at HBM speed and take much larger batches, so that launches, the alignment kernel's
    // latency and the per-batch synchronisation stay small against the stream (grid.y = frames of the batch <= 65535)
    const size_t cap = (e->rdf_groups.empty() && e->within_props.empty() && e->shell_sdf_props.empty() && e->exprs.empty() &&
                        e->hbond_props.empty() && e->sasa_props.empty() && e->contact_props.empty() && e->cluster_props.empty()) ? 16384 : 1024;
    B = std::max<size_t>(1, std::min<size_t>(B, cap));
    return B;
}

void plan_batches(const vmd_script_eval_t* e, size_t beg, size_t end, size_t Bmax, std::vector<Batch>* out) {
    auto even = [&](size_t a, size_t b) {
        const size_t total = b - a;
        if (!total) return;
        const size_t nbatch = (total + Bmax - 1) / Bmax;
        const size_t B = (total + nbatch - 1) / nbatch;
        for (size_t f = a; f < b; f += B) out->push_back({f, std::min(B, b - f), -1, 0});
    };
    const size_t S = e->block_frames;
    if (S == 0) { even(beg, end); return; }
    const bool super = g_opt.block_superbatch.load() != 0;
    // whole blocks that fit one batch become a batch of blocks (their partials are kept), everything else is a plain piece
    size_t run = beg;                          // start of the pending plain piece
    for (size_t f = beg; f < end;) {
        const size_t blk = f / S;
        const size_t bend = std::min((blk + 1) * S, e->num_frames);
        if (f == blk * S && bend <= end && bend - f <= Bmax) {
            even(run, f);
            Batch* last = out->empty() ? nullptr : &out->back();
            if (super && last && last->blk >= 0 && last->f0 + last->nb == f && last->nb + (bend - f) <= Bmax) { last->nb += bend - f;
                    last->nblk += 1; }
            else out->push_back({f, bend - f, (long)blk, 1});
            f = bend; run = f;
        } else {
            f = std::min(bend, end);
        }
    }
    even(run, end);
}

const float* block_rows(const vmd_script_eval_t* src, const PropState* q, size_t blk) {
    return src->block_ready[blk].load() == BLOCK_ROWS_AHEAD && q->ahead_values.size() == q->values.size()
            ? q->ahead_values.data() : q->values.data();
}

bool reuse_blocks(vmd_script_eval_t* e, const TrajId& traj_inst, size_t beg, size_t end, std::vector<std::pair<size_t, size_t>>* todo) {
    vmd_script_eval_t* src = e->source;
    if (!src) { todo->push_back({beg, end}); return true; }
    std::lock_guard<std::mutex> lock(src->mtx);   // order: own mutex, then the source's (a source never locks its users)
    // (looked up under its mutex: read-ahead may be giving it blocks right now)
    if (src->block_frames == 0 || src->blocks_inst != traj_inst) { todo->push_back({beg, end}); return true; }
    const size_t S = src->block_frames;
    size_t run = beg, reused = 0;
    for (size_t f = beg; f < end;) {
        const size_t blk = f / S;
        const size_t bend = std::min((blk + 1) * S, e->num_frames);
        if (f == blk * S && bend <= end && blk < src->num_blocks && src->block_ready[blk]) {
            if (run < f) todo->push_back({run, f});
            for (size_t i = 0; i < e->props.size(); ++i) {
                PropState* p = e->props[i].get();
                const PropState* q = src->props[i].get();
                if (p->ncounts) {
                    KRN_OK(vmd_hip_add_u64(e->stream, p->d_counts.p, q->d_blocks.p + blk * p->ncounts, p->ncounts));
                    if (p->prop.cls() == ResultClass::DISTRIBUTION)
                        for (size_t k = 0; k < p->ncounts; ++k) p->weights64[k] += q->block_weights64[blk * p->ncounts + k];
                } else {
                    memcpy(&p->values[f * p->dim1], block_rows(src, q, blk) + f * p->dim1, (bend - f) * p->dim1 * sizeof(float));
                    if (p->prop.device_table()) p->table_stale = true;     // the device table follows before the next filtered map
                }
                p->dirty = true;
            }
            for (size_t g = f; g < bend; ++g) mask_set(e->frame_mask, g);
            reused += bend - f;
            f = bend; run = f;
        } else {
            f = std::min(bend, end);
        }
    }
    if (run < end) todo->push_back({run, end});
    if (reused) {
        HIP_OK(hipStreamSynchronize(e->stream));   // the source's partials are read before its mutex is released
        e->frames_done += reused;
        e->frames_reused += reused;
        { HostTimer host_timer("host_refresh");
          for (auto& p : e->props) if (p->prop.cls() == ResultClass::DISTRIBUTION) { if (!refresh_distribution(e, p.get())) return false; } }
    }
    return true;
}

// a sharded device trajectory keeps only its block of frames behind the view; other frames (frame 0 for the SDF reference
// pose) come through load_frame
// (resident_beg, resident_end) = (0, 0) means "every frame"; any other pair is a shard, and beg == end != 0 is an EMPTY shard (a rank
// that owns no frame: 4 ranks on 5 frames) - nothing is resident then, not everything
bool view_sharded(const vmd_device_view_t& view) { return view.resident_beg != 0 || view.resident_end != 0; }

bool view_holds(bool have_view, const vmd_device_view_t& view, size_t frame) {
    return have_view && (!view_sharded(view) || (frame >= view.resident_beg && frame < view.resident_end));
}

// the host views of every property whose accumulators changed since its last refresh (the combining queue calls this when no call
// is waiting, process_range(views = true) does the same at its end)
bool refresh_views_locked(vmd_script_eval_t* e) {
    HIP_OK(hipSetDevice(e->device));
    for (auto& p : e->props) {
        if (!p->dirty) continue;
        // vmd_eval_defer_volume_views: a rank of a multi-GPU evaluation does not materialise ITS partial volume's float view (8.4 MB
        // over PCIe after every range) - the merge re-derives the view of the merged counts (vmd_eval_reduce -> vmd_eval_finalize); the
        // volume stays dirty until then
        if (p->prop.counts_view() && e->defer_volume_views.load(std::memory_order_relaxed)) continue;
        if (!refresh_view(e, p.get())) return false;
    }
    e->views_at = std::chrono::steady_clock::now();
    return true;
}

bool refresh_views(vmd_script_eval_t* e) {
    std::lock_guard<std::mutex> lock(e->mtx);
    return refresh_views_locked(e);
}

// The hot call.  VIAMD invokes it from N pool threads with small disjoint ranges (grain 1, src/main.cpp:993-997,
// src/task_system.cpp:73-81).  Launching kernels per call would drown the GPU in tiny batches, so calls COMBINE: the first
// caller becomes the leader, later callers queue their range and sleep; the leader repeatedly takes everything queued so far,
// merges adjacent ranges into long runs and evaluates those in large frame batches, then wakes the owners.
bool combine_call(vmd_script_eval_t* eval, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame_beg, uint32_t frame_end) {
    RangeRequest me;
    me.beg = frame_beg; me.end = frame_end; me.sys = sys; me.traj = traj;
    std::unique_lock<std::mutex> ql(eval->queue_mtx);
    eval->queue.push_back(&me);
    if (eval->leader_active) {
        eval->queue_cv.wait(ql, [&] { return me.done; });
        if (!me.ok) g_last_error = me.error;
        return me.ok;
    }
    eval->leader_active = true;
    while (!eval->queue.empty()) {
        // VIAMD's pool threads pull ranges of a few frames each (enkiTS: num_frames / (threads x (threads - 1)), at least 1) and every
        // one of them blocks in here, so a round can never hold more than threads x grain frames - and far fewer if the leader runs
        // off with whatever is queued the instant it looks: the threads it has just released are back with their next ranges within
        // microseconds.  It waits for them (gather_us at most, only while requests keep arriving) - a batch of 16 x 4 frames costs the
        // same ~0.15 ms of launches and round trips as a batch of 4.
        // Waiting is only worth a fraction of what a round costs: the slowest of the released threads needs 50 - 100 us to come back,
        // which a round of the 10 000-frame SDF (0.08 ms for 16 frames) cannot afford and a round of the 100k-atom RDF (0.3 ms) can:
        // at most half the previous round's time.  A large pool brings enough frames per round by itself, and on an oversubscribed
        // host waiting for 128 threads costs more than it gathers: pools of up to 32 callers only.
        const int gather = (int)std::min<long>(g_opt.gather_us.load(), eval->last_round_us / 2);
        // Scripts without pair passes (SDF / distance only: 0.7 us of kernels per frame) never gain from it - measured r03an: 129 ms
        // without, 195 ms with, for the 10 000 frames of config 4 from 16 threads - so only evals with RDF groups wait.
        if (gather >= 20 && !eval->rdf_groups.empty() && eval->queue.size() < eval->last_round && eval->last_round <= 32) {
            const auto t0 = std::chrono::steady_clock::now();
            const auto deadline = t0 + std::chrono::microseconds(gather);
            auto last_arrival = t0;
            size_t seen = eval->queue.size();
            while (eval->queue.size() < eval->last_round && !eval->interrupt) {
                ql.unlock();
                std::this_thread::yield();
                ql.lock();
                const auto now = std::chrono::steady_clock::now();
                if (eval->queue.size() != seen) { seen = eval->queue.size(); last_arrival = now; }
                // nobody new for a third of the window: the task is running out of ranges (its tail), or the pool is busy elsewhere
                if (now >= deadline || now - last_arrival > std::chrono::microseconds(gather / 3 + 1)) break;
            }
        }
        std::vector<RangeRequest*> taken;
        taken.swap(eval->queue);
        eval->last_round = taken.size();
        ql.unlock();
        // the views are for readers, and a reader only needs them final when the LAST call returns: while other calls are waiting they
        // are brought up to date at most every lazy_views_ms (a polling GUI still sees progress), and always before a round whose end
        // finds the queue empty hands its callers back
        const bool lazy = g_opt.lazy_views.load() != 0;
        bool all_ok = true;
        const auto round_t0 = std::chrono::steady_clock::now();
        // requests for the same trajectory, sorted by first frame; touching ranges fuse into one run
        // "the same trajectory" = the same instance behind the same callbacks, not the same interface STRUCT: a host that wraps its own
        // trajectory type per call (include/vmd_md_script_shim.h did, from every pool thread) presents a different address each time
        // (such ranges never fused)
        auto same_traj = [](const vmd_trajectory_i* a, const vmd_trajectory_i* b) {
            return a == b || (a->inst == b->inst && a->load_frame == b->load_frame && a->device_view == b->device_view
                    && a->load_raw == b->load_raw);
        };
        std::sort(taken.begin(), taken.end(), [](const RangeRequest* a, const RangeRequest* b) {
            return a->traj->inst != b->traj->inst ? a->traj->inst < b->traj->inst : a->beg < b->beg; });
        size_t i = 0;
        while (i < taken.size()) {
            size_t j = i + 1;
            uint32_t run_end = taken[i]->end;
            while (j < taken.size() && same_traj(taken[j]->traj, taken[i]->traj) && taken[j]->beg == run_end) { run_end = taken[j]->end;
                    ++j; }
            const bool ok = process_range(eval, taken[i]->sys, taken[i]->traj, taken[i]->beg, run_end, !lazy);
            const std::string err = ok ? std::string() : g_last_error;
            for (size_t k = i; k < j; ++k) { taken[k]->ok = ok; taken[k]->error = err; }
            all_ok = all_ok && ok;
            i = j;
        }
        const long round_us = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now()
                - round_t0).count();
        ql.lock();
        eval->last_round_us = round_us;
        if (lazy) {
            const bool overdue = std::chrono::steady_clock::now() - eval->views_at > std::chrono::milliseconds(std::max(1,
                    g_opt.lazy_views_ms.load()));
            if (eval->queue.empty() || overdue) {
                ql.unlock();
                const bool vok = refresh_views(eval);
                if (!vok && all_ok) { const std::string err = g_last_error; for (RangeRequest* r : taken) { r->ok = false; r->error = err;
                        } }
                ql.lock();
            }
        }
        for (RangeRequest* r : taken) r->done = true;
        eval->queue_cv.notify_all();
    }
    eval->leader_active = false;
    ql.unlock();
    if (!me.ok) g_last_error = me.error;
    return me.ok;
}
