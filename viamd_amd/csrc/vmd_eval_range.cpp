// viamd_amd/csrc/vmd_eval_range.cpp - process_range: one range of frames through the batch pipeline.  The reference poses, the plan
// (batch size, raw-ring policy, how far staging runs ahead), the loop that queues the kernels of batch k + 1 before it waits for
// batch k, and the completion of a batch: a batch whose buckets overflowed is repeated, its frames, temporal rows and frame-mask bits
// are booked.  What a batch launches is in vmd_eval_launch.cpp; both work on one RangeRun (vmd_eval_internal.h).
#include "vmd_eval_internal.h"

bool RangeRun::prepare_reference_poses() {
    // SDF reference pose: structure 0 at trajectory frame 0 (SPEC S5)
    for (auto& p : e->props) {
        if (p->prop.form != Form::SDF || p->ref_pose_ready) continue;
        BatchSrc src;
        if (!fetch_batch(e, traj, view_holds(have_view, view, 0) ? &view : nullptr, num_atoms, 0, 1, &src)) return false;
        KRN_OK(vmd_hip_sdf_ref_pose(e->stream, src.base, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), p->d_structs.p,
                p->d_mass.p, (int)p->prop.m, p->d_ref_pose.p, p->have_tree ? p->d_tree_order.p : nullptr, p->have_tree
                ? p->d_tree_parent.p : nullptr));
        HIP_OK(hipStreamSynchronize(e->stream));
        p->ref_pose_ready = true;
    }

    // rmsd reference pose: every context's set at trajectory frame 0.  It belongs to (evaluator, trajectory): rebuilt when
    // this call's trajectory is not the one it was built for
    for (auto& p : e->props) {
        if (p->prop.form != Form::RMSD && !(p->prop.form == Form::RMSF && p->rmsf_of < 0)) continue;     // (rmsf, DESIGN 1.13: the same pose)
        const TrajId now = traj_id(traj);
        if (p->rmsd_pose_ready && p->rmsd_pose_inst == now.inst && p->rmsd_pose_fn == now.fn) continue;
        BatchSrc src;
        if (!fetch_batch(e, traj, view_holds(have_view, view, 0) ? &view : nullptr, num_atoms, 0, 1, &src)) return false;
        const size_t ws = vmd_hip_rmsd_workspace_bytes(1, (int)p->dist_P, p->rmsd_max_set);
        if (!p->d_rmsd_pose.ensure(p->prop.a.size() * 3) || !p->d_rmsd_const.ensure(p->dist_P * 8) || !p->d_rmsd_ws.ensure((ws + 7) / 8))
            return false;
        e->prof.begin("rmsd", e->stream);
        KRN_OK(vmd_hip_rmsd_pose(e->stream, src.base, src.row_stride, e->stages[0].d_boxes.p, batch_pbc(e->stages[0]), (int)p->dist_P,
                p->d_a.p, p->d_ma.p, p->d_aoff.p, p->rmsd_max_set, p->d_rmsd_ws.p, p->d_rmsd_pose.p, p->d_rmsd_const.p));
        e->prof.end(e->stream);
        HIP_OK(hipStreamSynchronize(e->stream));
        p->rmsd_pose_inst = now.inst; p->rmsd_pose_fn = now.fn;
        p->rmsd_pose_ready = true;
    }
    return true;
}

// The plan of the run: which way the frames reach the device, the batches of `segments`, how far staging runs ahead of the kernels and
// whether a batch is completed behind the next one.  Asks the trajectory and the options; changes nothing but the run.
void RangeRun::plan_range(const std::vector<std::pair<size_t, size_t>>& segments) {
    // compressed frames for the device decoder travel two batches ahead through a ring of three slots (RawSlot)
    vmd_host_view_t hv_probe;
    vmd_raw_device_view_t rv_probe;
    raw_ring = !have_view && traj->load_raw && g_opt.xtc_device_decode.load() != 0 &&
               !(traj->host_view && traj->host_view(traj->inst, &hv_probe)) &&
               !(traj->raw_device_view && traj->raw_device_view(traj->inst, &rv_probe));
    vmd_raw_mapped_view_t mv_probe;
    memset(&mv_probe, 0, sizeof(mv_probe));
    have_map = raw_ring && g_opt.xtc_mapped.load() && traj->raw_mapped_view && traj->raw_mapped_view(traj->inst, &mv_probe);
    // plain-float files (TRR, DCD) take the ring only out of a mapping: without one their frames go through load_frame as before
    f32_ring = false;
    if (raw_ring && frame_beg < frame_end) {
        vmd_raw_frame_t probe;
        memset(&probe, 0, sizeof(probe));
        if (!traj->load_raw(traj->inst, (int64_t)frame_beg, nullptr, &probe, nullptr, 0)) raw_ring = false;
        else if (probe.codec == VMD_RAW_CODEC_F32) { f32_ring = have_map && mv_probe.codec == VMD_RAW_CODEC_F32
                && g_opt.raw_f32_device.load(); raw_ring = f32_ring; }
    }
    // how many batches the bit streams run ahead of the kernels (one more than the decoder, which runs two ahead).  Copied through pinned
    // blocks (host threads read them, this thread waits): 3.  Taken out of the mapped file by the copy engine alone: as many as the ring
    // holds minus the one being decoded - the DMAs then queue back to back and PCIe never waits for this thread (r03n: 12.4 ms per c2 step
    // against 9.4 ms of transfers). always > stage_ahead
    raw_ahead = (raw_ring && have_map && (f32_ring || g_opt.xtc_device_decode.load() == 3)) ? vmd_script_eval_t::kRawSlots - 1 : 3;
    // batches decompressed on the device while the previous batch is in the pair kernel: the persistent pair grid leaves room for them
    device_decode = raw_ring || (!have_view && traj->raw_device_view && traj->raw_device_view(traj->inst, &rv_probe));

    cold_walk = false;
    // frames per launch: as many as the scratch budget allows, split evenly so that no small tail batch is left
    size_t Bmax = auto_batch(e, num_atoms, !have_view);
    // host trajectories are staged in smaller batches so that load_frame of batch k+1 overlaps the kernels of batch k
    // ... except when the batches are decompressed on the device (profiles/r03_xtc_device_decode.txt).  The FIRST decode of a frame
    // walks its whole bit stream - a latency-bound chain, 7 ms per batch whether it holds 64 or 1 000 synthetic frames - so first passes
    // use large batches (4 x stage_frames).  It leaves checkpoints; every later pass decodes in sections at 2 - 3 us per frame, and
    // then small batches win from a file (the PCIe trip of batch k + 1 hides under decode + pair kernel of batch k: 64.6k frames/s
    // with batches of 128 against 51.3k with 512) and one large batch from HBM (103.8k against 98.8k).
    if (!have_view && g_opt.batch_frames <= 0) {
        // stage_frames is quoted for a 100 000-atom system (a 154 MB float stage); larger systems get proportionally fewer frames per
        // batch - r03u: 1M atoms in batches of 128 frames (0.64 GB of bit streams each) spent 15 of 34 ms waiting for the first batch
        const size_t npad_s = (num_atoms + 63) & ~(size_t)63;
        const size_t S0 = (size_t)std::max(1, g_opt.stage_frames.load());
        const size_t S = std::max<size_t>(1, std::min<size_t>(S0, S0 * 100032 / std::max<size_t>(npad_s, 1)));
        // does the first frame of the range have checkpoints already?  (plain floats need none)
        bool warm = f32_ring;
        if (!f32_ring && device_decode && g_opt.xtc_checkpoints.load() && frame_beg < frame_end) {
            if (raw_ring) {
                std::lock_guard<std::mutex> l(g_ck_mtx);
                auto it = g_ck_store.find(CkKey(traj->inst, e->device));
                warm = it != g_ck_store.end() && it->second && it->second->frames == traj->num_frames(traj->inst)
                        && it->second->atoms == num_atoms &&
                       it->second->device == e->device && it->second->have.size() > frame_beg && flag_get(&it->second->have[frame_beg]);
            }
            else warm = rv_probe.ck_have && flag_get(&rv_probe.ck_have[frame_beg]);
        }
        // a first pass out of a mapped file keeps four walks in flight (stage_ahead below): half-size batches, twice as many
        cold_walk = raw_ring && !f32_ring && !warm && have_map && g_opt.xtc_device_decode.load() == 3 && g_opt.xtc_cold_streams.load() != 0;
        // (a walk takes as long for one frame as for a thousand - 7 ms for a c2 frame, 70 ms for 1M atoms -: never more launches than
        // decode streams for a short range)
        const size_t cold_b = std::max<size_t>(2 * S, (frame_end - frame_beg + vmd_script_eval_t::kDecodeStreams
                - 1) / vmd_script_eval_t::kDecodeStreams);
        Bmax = std::min<size_t>(Bmax, !device_decode ? S : (raw_ring ? (warm ? S : (cold_walk ? cold_b : 4 * S)) : (warm ? 8 * S : 4 * S)));
    }
    for (auto& sg : segments) plan_batches(e, sg.first, sg.second, Bmax, &batches);
    // From a file the first batch has to cross PCIe and be decompressed before any kernel can start, and nothing overlaps the last
    // batch's kernels (r03p timeline: 1.7 ms of a 12.3 ms c2 step before the first pair kernel, one DMA = 1.13 ms per 128 frames).
    // Option xtc_ramp: the run starts with an eighth and a quarter of a batch and ends with a quarter.  Measured (r03o): the shorter
    // fill is paid back by the pair kernel's lower efficiency on small launches - 81.5k frames/s either way, so it is off.
    // (Only plain pieces are carved: a batch of whole frame blocks stays one, and a plain piece stays plain.)
    if (raw_ring && g_opt.xtc_ramp.load() && batches.size() >= 3) {
        std::vector<Batch> ramped;
        auto carve_front = [&](Batch& b, size_t n) { ramped.push_back({b.f0, n, -1, 0}); b.f0 += n; b.nb -= n; };
        Batch first = batches.front(), last = batches.back();
        if (first.blk < 0 && first.nb >= 64) { carve_front(first, first.nb / 8); carve_front(first, first.nb / 3); }
        ramped.push_back(first);
        for (size_t i = 1; i + 1 < batches.size(); ++i) ramped.push_back(batches[i]);
        if (last.blk < 0 && last.nb >= 64) { const size_t tail = last.nb / 4; ramped.push_back({last.f0, last.nb - tail, -1, 0});
                ramped.push_back({last.f0 + last.nb - tail, tail, -1, 0}); }
        else ramped.push_back(last);
        batches.swap(ramped);
    }
    // Batches staged ahead of the one being evaluated: one; optionally two when they are decompressed on the device (the decoder runs
    // UNDER the pair kernel, in the wave slots that kernel leaves).  r03n/r03p: the wait in settle_stage is the pipeline filling at the
    // start of a range, not a late decoder - two ahead measures the same, so one is the default.
    // A FIRST pass (no checkpoints yet) out of a mapped file: the walks of up to four batches run side by side (decode_streams).
    stage_ahead = (raw_ring && g_opt.xtc_device_decode.load() == 3 && g_opt.xtc_decode_ahead.load() >= 2) ? 2 : 1;
    if (cold_walk) stage_ahead = std::min<size_t>(vmd_script_eval_t::kDecodeStreams, raw_ahead - 1);
    decode_blocks = device_decode && batches.size() > 1 && g_opt.rdf_blocks_decode.load() >= 8;
    // Evals that keep block partials complete every batch before the next is queued.
    defer = g_opt.defer_sync.load() != 0 && e->block_frames == 0 && batches.size() > 1;
    rdf_counts = 0;
    for (auto& p : e->props) if (p->prop.cls() == ResultClass::DISTRIBUTION) rdf_counts += p->ncounts;
}

// SPEC S4 normalisation of one RDF property over the frames of a batch, fp64 on the host
void RangeRun::rdf_weights(BatchCtx& c, PropState* p) {
    const Property& d = p->prop;
    const bool shells = d.is_shell_rdf();
    for (auto& su : c.subs) {
        double* bw = su.blk >= 0 ? &p->block_weights64[(size_t)su.blk * p->ncounts] : nullptr;
        if (bw) std::fill(bw, bw + p->ncounts, 0.0);
        for (size_t b = su.off; b < su.off + su.nb; ++b) {
            const float* L = &c.src->h_boxes[9 * b];
            double V;
            // also the triclinic volume
            if ((c.pbc & VMD_UNITCELL_PBC_ALL) == VMD_UNITCELL_PBC_ALL && e->spec.rdf_norm != 1) V = (double)L[0]
                    * (double)L[1] * (double)L[2];
            else V = (4.0 / 3.0) * M_PI * (double)d.rmax * (double)d.rmax * (double)d.rmax;
            double Na = (double)d.a.size(), Nb = (double)d.b.size();
            if (shells) {
                // DECISION(D-SHELL-NORM): the populations of this frame; a frame with an empty shell adds no weight (whatever
                // spec_rdf_norm and spec_shell_norm say: nothing was counted in it)
                bool empty = false;
                for (int k = 0; k < 2; ++k) {
                    if (p->shell_of[k] < 0) continue;
                    const uint32_t pop = c.shell_pop[p->shell_of[k]][b];
                    empty = empty || pop == 0;
                    if (!e->spec.shell_norm) (k ? Nb : Na) = (double)pop;
                }
                if (empty) continue;
            }
            const double rho = (e->spec.rdf_norm == 2 ? 1.0 : Na) * Nb / V;
            const double w = ((double)d.rmax - (double)d.rmin) / (double)p->ncounts;
            for (size_t k = 0; k < p->ncounts; ++k) {
                const double r0 = (double)d.rmin + w * (double)k;
                const double r1 = (double)d.rmin + w * (double)(k + 1);
                const double wk = rho * (4.0 / 3.0) * M_PI * (r1 * r1 * r1 - r0 * r0 * r0);
                if (!spec) p->weights64[k] += wk;
                if (bw) bw[k] += wk;
            }
        }
    }
}

// waits for a queued batch (`later`: the batch already queued behind it, if any), repeats its RDF part when a bucket overflowed, books
// its frames
bool RangeRun::complete_batch(BatchCtx& c, BatchCtx* later) {
    if (!c.active) return true;
    c.active = false;
    const bool behind = later && later->active;
    VMD_STAGE("batch: waiting for its kernels");
    { HostTimer host_timer("host_sync_wait");
      if (behind) HIP_OK(hipEventSynchronize(e->batch_done[c.slot]));
      else HIP_OK(hipStreamSynchronize(e->stream)); }
    VMD_STAGE("batch: host bookkeeping");
    // a bucket of the two-level cell build was too small: nothing reached the histograms (every consumer saw the flag).
    // Re-measure the selections that used buckets with more head room and evaluate the RDF part of this batch again.
    bool repeated = false;
    for (int attempt = 0; e->h_overflow[c.slot] != 0; ++attempt) {
        if (attempt >= 4) return vmd_fail("cell build: pencil buckets keep overflowing");
        // the batch behind this one saw the flag too: let it drain, it repeats its RDF part at its own completion
        if (behind) {
            HIP_OK(hipStreamSynchronize(e->stream));
            later->poisoned = true;
        }
        const bool own = !(c.poisoned && attempt == 0);      // a poisoned batch did not overflow itself (as far as anyone knows)
        // one bit per selection (Selection::overflow_bit; selections beyond 32 share)
        const uint32_t who = e->h_overflow[c.slot];
        for (size_t si = 0; si < e->sels.size(); ++si) {
            Selection* sl = e->sels[si].get();
            sl->built = false;
            // only the selection whose buckets were too small gets wider ones.  (Its bit, not used_pencil, says so: a selection can
            // be sorted through buckets on one group's grid and by the single-block build on another's within ONE batch - co-evaluated
            // RDFs with different cutoffs - and used_pencil only remembers the last of them; fuzz seed 8941, round 4.)
            if (!own) continue;
            if (!(who & sl->overflow_bit)) {
                // round 6: the others are re-measured with more head room too, without a strike against them - what crowded one
                // selection's pencils crowds the next one's a batch later, and every overflow repeats a batch
                if (sl->used_pencil && sl->cap_margin < 2.0f) { sl->pen_off.clear(); sl->caps_cache.clear(); sl->cap_margin = 2.0f; }
                continue;
            }
            // a rare event worth a line in the host's log: it costs the batch a second cell build, and after three of them the
            // selection leaves the two-level build for good
            char msg[256];
            snprintf(msg, sizeof(msg),
                    "cell build: a pencil bucket of selection %zu (%zu atoms, %d x %d pencils, capacity margin %.2f, "
                     "largest bucket %d) overflowed in frames [%zu, %zu): re-measured on every frame of the batch, margin x 1.6",
                     si, sl->idx.size(), sl->pen_ny, sl->pen_nz, (double)sl->cap_margin, sl->cap_max, c.f0, c.f0 + c.nb);
            vmd_log(VMD_LOG_INFO, msg);
            sl->pen_off.clear();
            sl->caps_cache.clear();
            sl->cap_margin *= 1.6f;
            sl->overflows += 1;
        }
        e->h_overflow[c.slot] = 0;
        HIP_OK(hipMemsetAsync(e->d_overflow.p, 0, sizeof(uint32_t), e->stream));
        if (!launch_rdf(c)) return false;
        HIP_OK(hipStreamSynchronize(e->stream));
        repeated = true;
    }
    // rdfs over shells: the populations of this batch are final now (a repeated batch sent them again)
    for (auto& g : e->rdf_groups) for (int pi : g.shell_props) rdf_weights(c, e->props[pi].get());
    if (c.bt.blk >= 0 && !spec)
        for (auto& su : c.subs)
            for (auto& p : e->props) if (p->ncounts) KRN_OK(vmd_hip_add_u64(e->stream, p->d_counts.p, acc_of(p.get(), su), p->ncounts));
    e->prof.resolve();
    if (g_prof_on) { std::lock_guard<std::mutex> l(g_prof_mtx); g_prof["batches"].launches += 1; }
    for (size_t pi = 0; pi < e->props.size(); ++pi) {
        PropState* p = e->props[pi].get();
        if (!p->prop.temporal()) continue;
        // evaluated ahead: the rows wait beside the view until their block is committed (a reader of the values array never sees a
        // frame nobody asked for)
        if (spec && p->ahead_values.size() != p->values.size()) p->ahead_values.assign(p->values.size(), 0.0f);
        memcpy(spec ? &p->ahead_values[c.f0 * p->dim1] : &p->values[c.f0 * p->dim1], e->h_temporal_slot[c.slot].data() + c.toff[pi], c.nb
                * p->dim1 * sizeof(float));
    }
    e->frames_computed += c.nb;
    if (c.bt.blk >= 0) for (auto& su : c.subs) e->block_ready[su.blk] = spec ? BLOCK_ROWS_AHEAD : BLOCK_ROWS_IN_PLACE;
    if (spec) return true;
    for (size_t b = 0; b < c.nb; ++b) mask_set(e->frame_mask, c.f0 + b);
    e->frames_done += c.nb;
    // cheap views are refreshed every batch so a polling GUI sees progress (src/main.cpp:1508-1524): from the device when nothing
    // is queued behind this batch, from the snapshot taken behind its commits otherwise
    size_t soff = (size_t)c.slot * rdf_counts;
    for (auto& p : e->props) {
        if (p->prop.cls() != ResultClass::DISTRIBUTION) continue;
        // (an rdf over shells has its weights up to THIS batch in weights64: the batch behind adds its own at its completion)
        if (behind && c.snapshot && !repeated && !(later && later->poisoned)) refresh_distribution_from(p.get(), e->h_snap + soff,
                p->prop.is_shell_rdf() ? p->weights64.data() : e->w_snap.data() + soff);
        else if (!behind && views) { if (!refresh_distribution(e, p.get())) return false; }
        soff += p->ncounts;
    }
    return true;
}

// where launch_property has left the batch's rows of a property on the device (NULL: it has none to send from here)
static const float* batch_rows(const PropState* p, size_t f0) {
    switch (p->prop.form) {
    // accumulators, no rows; a within count's rows are sent by launch_rdf, behind the overflow flag
    case Form::RDF: case Form::SDF: case Form::RAMA_MAP: case Form::RMSF: case Form::WITHIN: case Form::WITHIN_EXPR: case Form::HBOND_COUNT:
    case Form::HBOND_OCC: case Form::SASA_AREA: case Form::SASA_OCC: case Form::CONTACT_COUNT: case Form::CONTACT_OCC:
    case Form::CONTACT_NATIVE: case Form::CLUSTER_COUNT: case Form::CLUSTER_SIZES: case Form::CLUSTER_LARGEST: return nullptr;
    case Form::RAMA_TABLE: case Form::MSD_TABLE: return p->d_table.p + f0 * p->dim1;                            // the batch's rows of the whole table
    case Form::DISTANCE: case Form::ANGLE: case Form::DIHEDRAL: case Form::SHAPE: case Form::RMSD: case Form::SS_CLASS: case Form::SS_POP:
        return p->d_out.p;
    }
    return nullptr;
}

// queues batch bi behind whatever is in flight, completes the batch in front of it (deferred) or itself, and stages later batches
bool RangeRun::queue_batch(size_t bi) {
    BatchCtx& c = ctx[bi & 1];
    BatchCtx& prev = ctx[(bi & 1) ^ 1];
    c = BatchCtx{};
    c.bt = batches[bi]; c.f0 = c.bt.f0; c.nb = c.bt.nb; c.slot = (int)(bi & 1);
    c.src = &stage_of(bi);
    { HostTimer host_timer("host_settle"); if (!settle_stage(e, *c.src, traj, num_atoms)) return false; }
    VMD_STAGE("batch: kernels queued");
    HostTimer queue_timer("host_queue_to_sync");
    HIP_OK(hipStreamWaitEvent(e->stream, c.src->ready, 0));
    c.pbc = batch_pbc(*c.src);
    for (auto& s : e->sels) s->built = false;

    // where each temporal property's rows stand in the batch's host slot: in the order of props, [nb][dim1] each.  The within counts
    // (launch_rdf), the other temporal kinds (below) and complete_batch all go by this one table.
    size_t temporal_floats = 0;
    c.toff.assign(e->props.size(), 0);
    for (size_t pi = 0; pi < e->props.size(); ++pi) {
        if (!e->props[pi]->prop.temporal()) continue;
        c.toff[pi] = temporal_floats;
        temporal_floats += c.nb * e->props[pi]->dim1;
    }
    e->h_temporal_slot[c.slot].resize(temporal_floats);

    // a whole frame block accumulates into its own partial first and is merged into the totals afterwards.  A batch of blocks
    // (filtered evaluation) is evaluated block by block - `subs` - behind one cell build and in front of one synchronisation.
    if (c.bt.blk >= 0 && c.bt.nblk > 1) {
        const size_t S = e->block_frames;
        for (size_t j = 0; j < c.bt.nblk; ++j) c.subs.push_back({j * S, std::min(S, c.nb - j * S), c.bt.blk + (long)j});
    } else c.subs.push_back({0, c.nb, c.bt.blk});
    if (c.bt.blk >= 0)
        for (auto& sb : c.subs)
            for (auto& p : e->props) if (p->ncounts) HIP_OK(hipMemsetAsync(acc_of(p.get(), sb), 0, p->ncounts * sizeof(uint64_t),
                    e->stream));
    // the blocks' pair launches alternate between the eval's stream and a second one (own partial rows): a 50-frame launch of a
    // 100k-atom system is ~3 work items per resident wave, and the tail of one launch then runs under the head of the next
    c.two_streams = c.subs.size() > 1 && g_opt.block_two_streams.load() != 0;

    e->h_overflow[c.slot] = 0;
    if ((!e->rdf_groups.empty() || !e->within_props.empty() || !e->shell_sdf_props.empty() || !e->exprs.empty() || !e->hbond_props.empty() ||
         !e->sasa_props.empty() || !e->contact_props.empty() || !e->cluster_props.empty()) &&
        !launch_rdf(c)) return false;

    for (size_t pi = 0; pi < e->props.size(); ++pi) {
        PropState* p = e->props[pi].get();
        if (!launch_property(c, pi)) return false;
        if (const float* rows = batch_rows(p, c.f0))
            HIP_OK(hipMemcpyAsync(e->h_temporal_slot[c.slot].data() + c.toff[pi], rows, c.nb * p->dim1 * sizeof(float), hipMemcpyDeviceToHost,
                    e->stream));
        p->dirty = p->dirty || !spec;
    }
    if (defer) {
        // what the host will want from this batch once a later one is queued behind it: the RDF counts as they stand behind its
        // commits (the weights as they stand now), and an event to wait on
        size_t soff = (size_t)c.slot * rdf_counts;
        for (auto& p : e->props) {
            if (p->prop.cls() != ResultClass::DISTRIBUTION) continue;
            HIP_OK(hipMemcpyAsync(e->h_snap + soff, p->d_counts.p, p->ncounts * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
            memcpy(e->w_snap.data() + soff, p->weights64.data(), p->ncounts * sizeof(double));
            soff += p->ncounts;
        }
        c.snapshot = true;
        HIP_OK(hipEventRecord(e->batch_done[c.slot], e->stream));
    }
    c.active = true;
    // deferred: the batch in front of this one is completed now that the device has this one to go on with (its stage is free
    // for the staging below only then)
    if (defer && !complete_batch(prev, &c)) return false;
    VMD_STAGE("batch: staging the next batch (fetch_stage)");
    // the kernels of this batch are queued: load the next batch on the host while they run
    if (bi + 1 < batches.size() && !e->interrupt) {
        if (bi + stage_ahead < batches.size()) {
            HostTimer host_timer("host_fetch_stage");
            const size_t nx = bi + stage_ahead;
            if (!fetch_stage(e, stage_of(nx), traj, vw, num_atoms, batches[nx].f0, batches[nx].nb, false, slot_of(nx))) return false;
        }
        // ... and send the bit streams of the batch after that on their way (its slot held batch bi - 1: decoded long ago)
        if (raw_ring && bi + raw_ahead < batches.size() &&
            raw_upload(e, *slot_of(bi + raw_ahead), traj, num_atoms, batches[bi + raw_ahead].f0, batches[bi
                    + raw_ahead].nb) < 0) return false;
    }
    return defer || complete_batch(c, nullptr);
}

// evaluates frames [frame_beg, frame_end) in large batches; returns false on interrupt (empty error) or failure
// views: bring the host views (values / weights / volume / aggregates) up to date before returning; false = the caller does it later
// (refresh_views), the device accumulators and the frame mask are complete either way
// spec (read-ahead): [frame_beg, frame_end) is a run of whole frame blocks; every block is evaluated into its own partial and
// NOTHING else changes - no add into the totals, no frame mask, no frames_done, no normalisation weights outside the block's own, no view
// (temporal rows are written: a frame's row is the same whenever it is computed, and nobody reads it before its mask bit is set)
bool process_range_locked(vmd_script_eval_t* eval, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame_beg, uint32_t frame_end,
        bool views, bool spec) {
    HIP_OK(hipSetDevice(eval->device));
    vmd_script_eval_t* e = eval;
    RangeRun run;
    run.e = e; run.traj = traj; run.frame_beg = frame_beg; run.frame_end = frame_end; run.views = views; run.spec = spec;
    run.num_atoms = traj->num_atoms(traj->inst);
    if (traj->num_frames(traj->inst) < frame_end) return vmd_fail("trajectory has fewer frames than the requested range");
    if (!check_atoms(e, run.num_atoms)) return false;
    if (!upload_static(e, sys, run.num_atoms)) return false;

    vmd_device_view_t& view = run.view;
    memset(&view, 0, sizeof(view));
    run.have_view = traj->device_view && traj->device_view(traj->inst, &view) && view.device == e->device;
    if (run.have_view && view_sharded(view) && frame_beg < frame_end && (frame_beg < view.resident_beg || frame_end > view.resident_end))
        return vmd_fail("frames [%u, %u) are not resident on this rank (its shard holds [%zu, %zu))", frame_beg, frame_end,
                view.resident_beg, view.resident_end);
    run.vw = run.have_view ? &view : nullptr;

    if (!run.prepare_reference_poses()) return false;

    // frames served from the block partials of the source eval (filtered evaluation), the rest is computed
    std::vector<std::pair<size_t, size_t>> segments;
    // a region's blocks are adopted from the source by the region leader, or evaluated here
    if (spec) segments.push_back({frame_beg, frame_end});
    else if (!reuse_blocks(e, traj_id(traj), frame_beg, frame_end, &segments)) return false;
    if (e->block_frames) {
        // a source evaluated over trajectory A and then, WITHOUT clear_data, over another trajectory of the same length must
        // not hand A's block partials to users that evaluate B - the blocks kept from now on belong to B, the ones kept so far are
        // forgotten
        const TrajId now = traj_id(traj);
        if (e->blocks_inst.inst && e->blocks_inst != now)
            for (size_t b = 0; b < e->num_blocks; ++b) e->block_ready[b] = 0;
        e->blocks_inst = now;
    }

    run.plan_range(segments);
    const std::vector<Batch>& batches = run.batches;
    e->raw_skip = traj->load_raw && !run.raw_ring;          // fetch_stage: do not ask this trajectory for raw frames batch by batch
    if (spec) for (auto& b : batches) if (b.blk < 0) return vmd_fail("read-ahead: region [%u, %u) is not made of whole frame blocks",
            frame_beg, frame_end);
    struct BlocksGuard {
        int old = -1;
        ~BlocksGuard() { if (old > 0) vmd_hip_set_rdf_blocks(old); }
    } blocks_guard;
    if (run.decode_blocks) {
        blocks_guard.old = vmd_hip_set_rdf_blocks(g_opt.rdf_blocks_decode.load());
        // never raise a smaller setting
        if (blocks_guard.old < g_opt.rdf_blocks_decode.load()) vmd_hip_set_rdf_blocks(blocks_guard.old);
    }
    if (run.raw_ring) {
        for (auto& rs : e->raw_slots) rs.state = 0;
        for (size_t bi = 0; bi < std::min<size_t>(run.raw_ahead, batches.size()); ++bi)
            if (raw_upload(e, *run.slot_of(bi), traj, run.num_atoms, batches[bi].f0, batches[bi].nb) < 0) return false;
    }
    for (size_t bi = 0; bi < std::min(run.stage_ahead, batches.size()); ++bi)
        if (!fetch_stage(e, run.stage_of(bi), traj, run.vw, run.num_atoms, batches[bi].f0, batches[bi].nb, false, run.slot_of(bi)))
            return false;
    // ---- one batch in flight, one being queued.  The kernels of batch k + 1 are queued BEFORE the host waits for batch k (on an event,
    // not on the stream): the device never idles across the host's per-batch work - the wait itself, the bookkeeping, the ~15 launches
    // of the next batch (~0.15 ms per boundary, a tenth of a step when batches are the 128 frames a file-backed pass stages).  Everything
    // a batch hands to the host has two slots (overflow flag, temporal rows, a snapshot of the RDF counts behind its commits); a batch
    // whose cell build overflowed still voids itself AND whatever was queued behind it (the flag is sticky): the later batch is marked
    // and repeats its RDF part when its turn comes.
    if (run.defer && run.rdf_counts) {
        if (e->h_snap_cap < 2 * run.rdf_counts) {
            if (e->h_snap) pool_give(e->h_snap);
            e->h_snap = nullptr; e->h_snap_cap = 0;
            HIP_OK(pool_take(kPinned, (void**)&e->h_snap, 2 * run.rdf_counts * sizeof(uint64_t)));
            e->h_snap_cap = 2 * run.rdf_counts;
        }
        e->w_snap.resize(2 * run.rdf_counts);
    }
    bool completed = true;
    for (size_t bi = 0; bi < batches.size(); ++bi) {
        if (e->interrupt) { completed = false; break; }
        if (!run.queue_batch(bi)) return false;
    }
    // whatever is still in flight (deferred: the last batch queued; after an interrupt: the one before the break)
    { BatchCtx* ctx = run.ctx;
      BatchCtx& a = ctx[0].active && ctx[1].active ? (ctx[0].f0 < ctx[1].f0 ? ctx[0] : ctx[1]) : ctx[0];
      BatchCtx& b = &a == &ctx[0] ? ctx[1] : ctx[0];
      if (!run.complete_batch(a, b.active ? &b : nullptr)) return false;
      if (!run.complete_batch(b, nullptr)) return false; }
    if (views) {
        for (auto& p : e->props) {
            if (!p->dirty) continue;
            if (p->prop.cls() != ResultClass::DISTRIBUTION && !refresh_view(e, p.get())) return false;     // (a distribution: per batch)
        }
        e->views_at = std::chrono::steady_clock::now();
    }
    return completed;
}

bool process_range(vmd_script_eval_t* eval, const vmd_system_t* sys, vmd_trajectory_i* traj, uint32_t frame_beg, uint32_t frame_end,
        bool views) {
    g_last_error.clear();
    if (eval->interrupt) return false;
    std::lock_guard<std::mutex> lock(eval->mtx);
    return process_range_locked(eval, sys, traj, frame_beg, frame_end, views, false);
}
