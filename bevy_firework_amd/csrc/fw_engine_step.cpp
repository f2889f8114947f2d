// fw_engine_step.cpp -- fw_step: one frame = spawn_particles + update_particles for every spawner (core.rs:367-670).  This unit is
// the frame's plan -- mode exits, lifetime windows, emission clocks, ring-op routing, the tile table -- which a failure undoes
// through `rollback`; fw_engine_launch.cpp enqueues what it planned (FwFrame).
// (host engine of libfirework_hip.so: fw_engine.h lists its translation units; there is no CPU simulation path in this library)
#include "fw_engine.h"

namespace {

// ---- before anything of the frame is entered anywhere (a failure returns as it is)

// poisoned spawners, snapshot rows, derived planes, per-frame scratch, the modes a dt ends
fw_status begin_frame(fw_ctx *ctx, float dt) {
    // a spawner whose particle state an internal error invalidated (SpawnerHost::poisoned): no further frame is enqueued on
    // top of it -- for anybody: the frame is all-or-nothing -- until it has been rebuilt or destroyed
    poll_device_error(ctx);
    if (ctx->n_poisoned)  // (counted, not looked for: with thousands of spawners a scan of their records would be a cost of every frame)
        for (const SpawnerHost &sp : ctx->spawners)
            if (sp.alive && sp.poisoned) return poisoned_status(ctx);
    poll_snapshots(ctx);
    if (ctx->derive_ready_any) {  // types whose caller-written particles have all been through an update (see the end of a frame)
        ctx->derive_ready_any = false;
        for (uint32_t i = 0; i < ctx->segs.size(); i++) {
            SegHost &S = ctx->segs[i];
            if (!S.in_use || !S.derive_ready) continue;
            S.derive_ready = false;
            if (S.colors_dirty || !wants_derived(ctx, S)) continue;  // (detached / rewritten since)
            const fw_status dst = set_derived(ctx, i, true);
            if (dst) return dst;
        }
    }

    // per-frame scratch lives in the context: with thousands of emitters the allocations were a visible part of the
    // host's ~60 ns per emitter
    for (auto &L : ctx->levels) L.g.clear(), L.n.clear();
    ctx->fifo_ops.clear(), ctx->fifo_mat_ops.clear(), ctx->range_mat_ops.clear();
    ctx->seg_kind_changed = false;
    if (!std::isfinite(dt))  // 0 * inf = NaN: an angular velocity of zero does not stay zero (core.rs:648-650)
        for (uint32_t si = 0; si < ctx->segs.size(); si++)
            if (ctx->segs[si].in_use && ctx->segs[si].nospin) {
                fw_status nst = leave_nospin(ctx, si);
                if (nst) return nst;
            }
    if (ctx->census.n_fifo) {
        // the FIFO order rests on ages that never decrease: a negative or non-finite dt ends the mode (as does a dt so
        // small that the cohort list grows without bound)
        const bool dt_ok = dt >= 0.0f && std::isfinite(dt);
        for (uint32_t si = 0; si < ctx->segs.size(); si++) {
            SegHost &S = ctx->segs[si];
            // (a type that receives Nested children: a step as long as its lifetime would destroy children whose number only
            // this frame's Nested pass will know)
            if (!S.in_use || !S.fifo || (dt_ok && S.coh.size() < kMaxCohorts && !(S.fifo_dev && dt >= S.fifo_life))) continue;
            fw_status cst = fifo_to_general(ctx, si);
            if (cst) return cst;
        }
    }
    ctx->range_ops.clear();
    if (ctx->census.n_range) {
        // The in-place young part of a range ring rests on ages that never decrease and on nobody -- a particle spawned this
        // frame included -- dying before its age reaches lifetime.min: a negative or non-finite dt, a step as long as the
        // shortest lifetime, or a cohort list that grows without bound (a dt thousands of times smaller than the
        // lifetimes) end the mode; the type continues on the compacting path.
        const bool flood = ctx->birth_age.size() > (1u << 22);
        for (uint32_t si = 0; si < ctx->segs.size(); si++) {
            SegHost &S = ctx->segs[si];
            if (!S.in_use || !S.range) continue;
            if (!flood && dt >= 0.0f && dt < S.range_life_lo && S.ycoh.size() < kMaxCohorts && S.dcoh.size() < kMaxCohorts) continue;
            fw_status cst = fifo_to_general(ctx, si);
            if (cst) return cst;
        }
    }
    if (!ctx->census.n_range) ctx->birth_age.clear();
    return FW_OK;
}

// Round 6: rings that receive Nested children need the size of a cohort -- which only the device knows -- in
// the frame that cohort may start to die; the update of the cohort's own frame left it in a pinned report ring, a lifetime.min
// ago.  A report that is STILL missing after the stream has been waited for is looked for HERE, before anything of the frame is
// committed: such a ring continues on the compacting path -- exact counts from the device, particles and order kept
// (fifo_to_general) -- and the frame goes ahead.  A failed check of the host's bookkeeping costs a conversion, not the spawner's
// particles.  (FW_DEBUG 512 in the `ab` build pretends the report of the first due cohort of frame 60 is missing:
// tests/test_gpu_range.py.)
bool report_missing(fw_ctx *ctx, const SegHost &S, uint64_t frame) {
    if (FW_DBG(ctx->dbg, 512u) && ctx->frame == 60u) return true;
    if (wait_report(S, frame)) return false;
    if (sync(ctx) != FW_OK) return true;
    return !report_landed(S, frame);
}

fw_status recover_missing_reports(fw_ctx *ctx, float dt) {
    if (!ctx->census.n_fifo && !ctx->census.n_range) return FW_OK;
    for (uint32_t si = 0; si < ctx->segs.size(); si++) {
        SegHost &S = ctx->segs[si];
        if (!S.in_use || !S.h_report) continue;
        bool missing = false;
        if (S.fifo && S.fifo_dev) {
            for (const SegHost::Cohort &c : S.coh) {
                if (!(c.age + dt >= S.fifo_life)) break;  // (the oldest die first: launch_fifo's own test)
                if (!c.known && c.frame != ctx->frame && report_missing(ctx, S, c.frame)) missing = true;
            }
        } else if (S.range && S.range_dev) {
            for (const SegHost::DCohort &c : S.dcoh) {
                if (birth_age_before(ctx, c.frame) + dt < S.range_life_lo) break;  // (launch_range's own test)
                if (!c.known && report_missing(ctx, S, c.frame)) missing = true;
            }
        }
        if (!missing) continue;
        ctx->recovered_rings++;
        fw_status cst = fifo_to_general(ctx, si);
        if (cst) return cst;
    }
    return FW_OK;
}

// the lifetime window of a segment: drop the spawns that must have expired, tighten the bound with what is left
// (an age is an fp32 running sum of the dt values: up to half an ulp of the age per step taken, i.e. a relative
// error below steps * 6e-8; the horizon carries that (with a factor 4) on top of a fixed 1e-3)
inline void expire_window(fw_ctx *ctx, SegHost &S) {
    while (!S.win.empty() &&
           ctx->sim_time - S.win.front().t >=
               S.life_bound * (1.0 + 1e-3 + 2.4e-7 * (double)(ctx->frame - S.win.front().frame)) + 1e-6) {
        S.win_sum -= S.win.front().n;
        S.win.pop_front();
    }
    if (S.win_sum < S.ub) S.ub = (uint32_t)S.win_sum;
}

// lifetime windows: drop the spawns that must have expired by now and tighten the bounds with what is left.
// (ages are fp32 sums of the same dt values on the device; the margin covers the rounding difference)
// The same pass notes what the rest of the frame asks of every segment: which Nested-fed ones must grow, whether a particle type
// collides, whether a compacting segment has an instance buffer attached.
fw_status segment_pass(fw_ctx *ctx, FwFrame &fr) {
    const float dt = fr.dt;
    // (frame_spawn is reset here: one pass over the segments instead of two)
    fr.new_static = std::isfinite(dt);
    if (!(dt >= 0.0f) || !std::isfinite(dt))
        for (auto &S : ctx->segs) S.win_ok = false;  // ages would not grow monotonically
    ctx->grow_scratch.clear();
    // (solo segments -- small types with one feeder, thousands of them -- are not visited: the spawner loop does this for
    // them where it makes their op; fw_ctx::big_list holds everybody else)
    const bool by_list = ctx->census.n_solo != 0;
    if (by_list && ctx->big_dirty) {
        ctx->big_list.clear();
        for (uint32_t si = 0; si < ctx->segs.size(); si++)
            if (ctx->segs[si].in_use && !ctx->segs[si].solo) ctx->big_list.push_back(si);
        ctx->big_dirty = false;
    }
    const bool solo_ok = ctx->host_fast && ctx->use_small;
    auto &rs = fr.ring_stats;
    for (size_t k = 0, ns = by_list ? ctx->big_list.size() : ctx->segs.size(); k < ns; k++) {
        const size_t si = by_list ? ctx->big_list[k] : k;
        SegHost &S = ctx->segs[si];
        if (k + 8 < ns) {  // the oldest window entry of a later segment: a heap line of its own, fetched ahead of time
            const SegHost &N = ctx->segs[by_list ? ctx->big_list[k + 8] : k + 8];
            if (N.win.n) __builtin_prefetch(&N.win.v[N.win.head]);
        }
        S.frame_spawn = 0;
        if (!S.in_use) continue;
        S.dead_at_end = false;  // (set again by launch_range for the segments this frame updates as range rings)
        fr.any_coll |= S.collides && !S.ring() && !S.small;  // (a colliding type in a ring / on the small kernel is updated by that kernel)
        // (what decides the tile size of the ring launches -- fifo_small / range_small -- gathered while the record is hot)
        if (S.fifo) rs.fifo_parts += S.ub, rs.fifo_dev |= S.fifo_dev, rs.fifo_coll |= S.collides, rs.fifo_inst |= S.inst != nullptr;
        if (S.range) rs.range_parts += S.ub, rs.range_dev |= S.range_dev, rs.range_coll |= S.collides, rs.range_inst |= S.inst != nullptr;
        fr.any_inst_general |= !S.ring() && S.inst != nullptr;
        if (S.nested_fed && nested_fed_wants_growth(S)) ctx->grow_scratch.push_back((uint32_t)si);
        if (S.win_ok) expire_window(ctx, S);
        // a small type with one feeder: solo from here on (this was its last visit by this pass)
        if (S.small && S.one_feeder && solo_ok) seg_becomes_solo(ctx, S), ctx->big_dirty = true;
    }

    // Nested-fed segments whose count (or its growth) nears their derived capacity: nested_fed_wants_growth.  By half again,
    // not by doubling.  Caller-given capacities are left alone.
    for (uint32_t si : ctx->grow_scratch) {
        SegHost &S = ctx->segs[si];
        // (growing one type's children may already have grown a later entry of the list)
        if (!S.in_use || !nested_fed_wants_growth(S)) continue;
        const uint32_t want = (uint32_t)std::min<uint64_t>((uint64_t)S.capacity * 3 / 2 + (uint64_t)(64.0f * S.dev_rate), 0x70000000ull);
        S.dev_count = 0, S.dev_rate = 0.f, S.dev_epoch = 0;
        fw_status gst = grow_segment(ctx, si, want, false);
        if (!gst) gst = grow_nested_children(ctx, ctx->spawners[S.spawner], (uint32_t)S.type);
        if (gst) return gst;
    }
    return FW_OK;
}

// Frames of a context with small types hand their Global ops to the kernels as a TABLE in a parameter slot ({first op, one past
// the last, particles} per segment, then the ops): the spawner loop writes both IN PLACE (OpList::borrow) -- with thousands of
// emitters the ops are 200-400 KB a frame, and writing them to a list, reading the list and writing the table was a tenth of the
// host's frame.  The headers are kept while the ops arrive (segments ascending, each one's ops next to each other: what a
// context whose spawners were built in order delivers); anything else -- an op routed later, a list that outgrows the slot, a
// frame that turns out to need the separate spawn passes -- falls back to the sort + header pass of the enqueue, over the same
// memory or the list's own.
fw_status take_op_slot(fw_ctx *ctx, FwFrame &fr) {
    auto &levels = ctx->levels;
    // (not a table small enough for host-written device memory -- fw_ctx::b_param: that one is copied there in one sequential pass)
    if (!(ctx->host_fast && ctx->census.n_small != 0 && ctx->update_mode == FW_MODE_FUSED && !levels.empty() &&
          !(ctx->param_bar && ctx->segs.size() * sizeof(OpHdr) + ((size_t)ctx->census.n_in_use + 16) * sizeof(FwOp) <= kBarParamBytes)))
        return FW_OK;
    const size_t n_seg0 = ctx->segs.size(), off_ops0 = n_seg0 * sizeof(OpHdr);
    const size_t want_ops = (size_t)ctx->census.n_in_use + 16;
    fw_status pst = FW_OK;
    if (ctx->param_bytes < off_ops0 + want_ops * sizeof(FwOp)) pst = ensure_param_ring(ctx, off_ops0 + (want_ops * 2 + 64) * sizeof(FwOp));
    if (!pst) pst = acquire_slot(ctx, &fr.pre_slot);
    if (pst) return pst;
    fr.pre_hdr = (OpHdr *)ctx->h_param[fr.pre_slot].get();
    memset(fr.pre_hdr, 0, off_ops0);
    levels[0].g.borrow((FwOp *)(ctx->h_param[fr.pre_slot] + off_ops0), (ctx->param_bytes - off_ops0) / sizeof(FwOp));
    fr.pre_hdr_ok = true;
    return FW_OK;
}

// ---- from here on, everything the host half changes goes through the undo log (fw_ctx::undo_em / undo_sp) or into a list
// `rollback` walks

// Restores what the plan has changed when the frame cannot be enqueued (the per-segment live-count bounds only ever get looser,
// which is harmless).
fw_status rollback(fw_ctx *ctx, fw_status why) {
    for (const auto &u : ctx->undo_em) {
        EmissionHost &E = ctx->spawners[u.spawner].em[u.entry];
        E.last_emission = u.last_emission, E.time_passed_in_cycle = u.time_passed_in_cycle;
        E.enabled = u.enabled, E.serial = u.serial;
    }
    for (const auto &u : ctx->undo_sp) ctx->spawners[u.spawner].manual_queued_count = u.manual_queued_count;
    // the spawn totals and lifetime windows the ops of this frame were entered into (note_spawned)
    auto forget = [&](const FwOp &op) {
        SegHost &S = ctx->segs[op.seg];
        S.cum_spawn -= op.n;
        if (S.solo) S.ub -= std::min(S.ub, op.n);  // (its frame_spawn stays 0: the loop over the segments below does nothing for it)
        if (S.fifo || !S.win_ok || S.win.empty() || S.win.back().t != ctx->sim_time) return;
        S.win_sum -= op.n;
        if ((S.win.back().n -= op.n) == 0) S.win.pop_back();
    };
    for (auto &L : ctx->levels)
        for (const FwOp &op : L.g) forget(op);
    for (const FwOp &op : ctx->fifo_ops) forget(op);
    for (const FwOp &op : ctx->range_ops) forget(op);
    for (const auto &io : ctx->fifo_mat_ops) forget(io.second);
    for (const auto &io : ctx->range_mat_ops) forget(io.second);
    for (auto &S : ctx->segs) S.ub -= std::min(S.ub, S.frame_spawn), S.frame_spawn = 0;
    return why;
}

// a Global op enters its segment's spawn total and lifetime window as it is made (the segment record is in the cache
// then; `rollback` takes it out again)
inline void note_spawned(fw_ctx *ctx, SegHost &S, uint64_t n) {
    S.cum_spawn += n;
    if (S.fifo || !S.win_ok) return;
    if (!S.win.empty() && S.win.back().t == ctx->sim_time) {
        S.win.back().n += n;
    } else {
        if (S.win.size() >= 8192) {  // very long lifetimes: fold the two oldest entries into the newer
            const uint64_t m = S.win.front().n;
            S.win.pop_front();
            S.win.front().n += m;
        }
        S.win.push_back(SegHost::Spawned{ctx->sim_time, n, ctx->frame});
    }
    S.win_sum += n;
}

// a refresh of the exact counts drops this frame's appends from every bound: back in they go
void readd_frame_spawns(fw_ctx *ctx) {
    for (auto &X : ctx->segs) X.ub += X.frame_spawn;
    if (ctx->census.n_solo)  // (a solo segment's appends of the frame are in its op)
        for (auto &L : ctx->levels)
            for (const FwOp &op : L.g)
                if (ctx->segs[op.seg].solo) ctx->segs[op.seg].ub += op.n;
}

// spawn_particles, host half (core.rs:377-428): emission clocks and Global counts.  A failure is the caller's to roll back.
fw_status spawner_loop(fw_ctx *ctx, FwFrame &fr) {
    const float dt = fr.dt;
    auto &levels = ctx->levels;
    // (the loop's own copies of the frame's flags, stored back at its end)
    bool new_static = fr.new_static, pre_hdr_ok = fr.pre_hdr_ok;
    size_t pre_tracked = fr.pre_tracked;
    OpHdr *const pre_hdr = fr.pre_hdr;
    for (size_t h = 0; h < ctx->spawners.size(); h++) {
        SpawnerHost &sp = ctx->spawners[h];
        if (h + 8 < ctx->spawners.size()) {  // the entries of a later spawner live on the heap: fetch them ahead of time
            const SpawnerHost &nx = ctx->spawners[h + 8];
            if (nx.em.size() > 1) {  // (a single entry is part of the spawner's record: the array is streamed as it is)
                __builtin_prefetch(nx.em.data());
                __builtin_prefetch((const char *)nx.em.data() + 128);
            }
        }
        // (solo segments -- visited here and nowhere else in the frame -- fetched a few spawners ahead of time, record first, then the
        // two ends of the lifetime window: built and measured, 38.5 -> 42 us per frame at 2048 x 200, the loop is bound by its
        // instructions and stores by now, not by the latency of its loads: profiles/r05/host_fast_prefetch.txt)
        if (!sp.alive) continue;
        // `if data.active()` (core.rs:378): an entry that emits on other particles contributes only when
        // some particle exists; with no particle at all the Nested arm below is a no-op anyway, so the
        // host-side gate "any entry enabled" gives the same state transitions without a device round trip.
        bool any_enabled = false;
        for (const EmissionHost &e : sp.em) any_enabled |= e.enabled;
        if (!any_enabled) continue;
        for (size_t i = 0; i < sp.em.size(); i++) {
            EmissionHost &E = sp.em[i];
            if (!E.enabled) continue;
            const fw_emission_settings &es = E.es;
            const uint32_t dst = E.dst_seg;
            if (es.mode == FW_MODE_GLOBAL) {
                uint64_t n = 0;
                ctx->undo_em.push_back(fw_ctx::EmUndo{(uint32_t)h, (uint32_t)i, E.last_emission, E.time_passed_in_cycle,
                                                      E.enabled, E.serial});
                if (es.pacing_kind == FW_PACING_ONESHOT) {
                    E.enabled = false;  // core.rs:397-400
                    n = es.oneshot_count;
                } else if (es.pacing_kind == FW_PACING_ONDEMAND) {
                    n = sp.manual_queued_count;  // core.rs:401-405
                    if (n) ctx->undo_sp.push_back(fw_ctx::SpUndo{(uint32_t)h, n});
                    sp.manual_queued_count = 0;
                } else {
                    E.time_passed_in_cycle = fw_rem_euclid(E.time_passed_in_cycle + dt, es.duration);  // core.rs:412-414
                    float next = 0.f;
                    n = es.duration == 1.0f
                            ? fw_emission_count_unit(E.time_passed_in_cycle, E.last_emission, es.offset_start, es.offset_end, E.between, &next)
                            : fw_emission_count(E.time_passed_in_cycle, E.last_emission, es.duration, es.offset_start, es.offset_end,
                                                es.count, &next);
                    E.last_emission = next;
                }
                if (!n) continue;
                if (n > kMaxSpawnPerOp) return fail(ctx, FW_ECAPACITY, "emission count exceeds 2^30 particles in one frame");
                SegHost &S = ctx->segs[dst];
                if (S.solo && S.win_ok) expire_window(ctx, S);  // its frame begins here (FwPathCensus::n_solo)
                if (S.nested_fed && S.auto_capacity && S.capacity < 0x70000000u) {
                    // A type that receives Nested children too: its children are counted on the device, but its Global
                    // particles are counted right here.  Count of the latest snapshot row + every Global particle since
                    // (at most those the lifetime window still holds) + this op: past half the capacity, the segment grows
                    // NOW, however fast the burst -- the snapshot rule above only follows what the device has seen.
                    uint64_t since = S.cum_spawn - S.snap_cum;  // (includes this frame's earlier ops: note_spawned)
                    if (S.win_ok) since = std::min<uint64_t>(since, S.win_sum);
                    const uint64_t est = (uint64_t)S.snap_count + since + n;
                    if (est > S.capacity / 2) {
                        fw_status st = grow_segment(ctx, dst, (uint32_t)std::min<uint64_t>(est * 2, 0x70000000ull));
                        if (!st) st = grow_nested_children(ctx, sp, (uint32_t)es.particle_index);
                        // (the growth refreshed every bound from the device's exact counts, without this frame's appends)
                        readd_frame_spawns(ctx);
                        if (st) return st;
                        S.snap_count = S.ub - std::min(S.ub, S.frame_spawn), S.snap_cum = S.cum_spawn - S.frame_spawn;
                        S.dev_count = 0;
                    }
                }
                if (!S.nested_fed && (uint64_t)S.ub + n > S.capacity) {
                    fw_status st = refresh_counts_exact(ctx);
                    if (st) return st;
                    // the refresh dropped this frame's earlier appends from ub: add them back
                    readd_frame_spawns(ctx);
                    if ((uint64_t)S.ub + n > S.capacity) {
                        if ((uint64_t)S.ub + n > 0xF0000000ull) return fail(ctx, FW_ECAPACITY, "particle type too large");
                        // grow_segment copies `ub - frame_spawn` settled particles; appended ones are not on the
                        // device yet (spawn kernels of this frame have not been enqueued)
                        const uint32_t fs = S.frame_spawn;
                        S.ub -= fs;
                        const uint32_t settled = S.ub;
                        st = grow_segment(ctx, dst, (uint32_t)(settled + fs + n));
                        if (!st) st = grow_nested_children(ctx, sp, (uint32_t)es.particle_index);
                        readd_frame_spawns(ctx);
                        if (st) return st;
                    }
                }
                // does every particle of this op outlive the step?  (TypeHost::life_lo_safe; false for NaN)
                if (!S.ring() && !(dt < E.life_lo_safe)) new_static = false;
                auto fill = [&](FwOp &op) {
                    memset(&op, 0, sizeof op);
                    op.seg = dst, op.emit = E.emit_idx, op.n = (uint32_t)n;
                    op.rel_base = S.frame_spawn;
                    op.serial_base = E.serial;
                    memcpy(op.origin_pos, sp.origin_pos, sizeof sp.origin_pos);
                    memcpy(op.origin_rot, sp.origin_rot, sizeof sp.origin_rot);
                    memcpy(op.parent_vel, sp.parent_vel, sizeof sp.parent_vel);
                    op.speed = sp.mod_speed, op.scale = sp.mod_scale;
                };
                if (!S.ring()) {
                    // a compacting or small segment: the op goes to its emission level, written where it will stay
                    OpList &G = levels[i].g;
                    if (i == 0 && pre_hdr_ok) {  // ... and, in a list that lives in a parameter slot, into the segment's header
                        const uint32_t idx = (uint32_t)G.size();
                        OpHdr &H = pre_hdr[dst];
                        // (the kernels read a segment's ops through its header only: the ops of a segment must sit next to each other,
                        // in emission order -- segments need not ascend, which they do not once slots have been re-used)
                        if (H.o1 == 0) H.o0 = idx, H.o1 = idx + 1u, H.n = (uint32_t)n;
                        else if (H.o1 == idx) H.o1 = idx + 1u, H.n = (uint32_t)std::min<uint64_t>((uint64_t)H.n + n, 0xFFFFFFFFull);
                        else pre_hdr_ok = false;  // (ops of one segment apart: the sort + header pass of the enqueue)
                        pre_tracked = idx + 1u;
                    }
                    fill(G.push_slot());
                } else {
                    FwOp op;
                    fill(op);
                    if (S.fifo && S.fifo_mat && !S.virt_parent)
                        ctx->fifo_mat_ops.push_back({(uint32_t)i, op});  // routed by route_ring_ops, once the frame's Nested ops are known
                    else if (S.fifo)
                        ctx->fifo_ops.push_back(op);  // spawned inside fw_k_update_fifo, whatever else the frame holds
                    else if (S.range_mat && !S.virt_parent)
                        ctx->range_mat_ops.push_back({(uint32_t)i, op});  // routed by route_ring_ops, once the frame's Nested ops are known
                    else
                        ctx->range_ops.push_back(op);  // spawned inside fw_k_update_range
                }
                E.serial += n;
                if (!S.solo) S.frame_spawn += (uint32_t)n;  // (a solo segment's one op of the frame carries the count)
                S.ub = (uint32_t)std::min<uint64_t>((uint64_t)S.ub + n, 0xFFFFFFFFull);
                if (S.small && S.ub > ctx->small_max && !S.wide) {
                    // no longer a few hundred particles: a WIDE type (a workgroup of the same kernel) from this frame on -- or, in a
                    // context that does not run wide types (fw_ctx::wide_mid_on), a compacting segment that stays eligible
                    S.wide = true, S.wide_big = false, ctx->small_dirty = true;
                    if (!ctx->wide_mid_on) {
                        const bool was_solo = S.solo;
                        small_deactivate(ctx, S);
                        if (was_solo) S.frame_spawn = (uint32_t)n;
                    }
                }
                if (S.small && S.wide && S.ub > std::max(ctx->small_max, 2u * ctx->wide_max)) {
                    // ... no longer a few thousand: a compacting segment
                    const bool was_solo = S.solo;
                    leave_small(ctx, S);
                    if (was_solo) S.frame_spawn = (uint32_t)n;
                }
                note_spawned(ctx, S, n);
            } else {
                if (es.pacing_kind != FW_PACING_COUNT_OVER_DURATION) continue;  // warn_once + continue core.rs:474-485
                const SegHost &P = ctx->segs[sp.seg[es.target_particle_type]];
                // children are born with age 0 like any new particle: do they all outlive this step?
                if (!(dt < E.life_lo_safe)) new_static = false;
                FwNestOp op{};
                op.parent_seg = sp.seg[es.target_particle_type], op.child_seg = dst;
                op.emit = E.emit_idx, op.emit_slot = E.emit_slot;
                {  // parent tiles of the launch: from the host's bound of the parent count (exact counts live on the device)
                    const uint32_t par_ub = P.nested_fed ? P.capacity : std::min(P.ub, P.capacity);
                    op.n_tiles = (par_ub + FW_NEST_TILE - 1) / FW_NEST_TILE + 1;
                }
                op.speed = sp.mod_speed, op.scale = sp.mod_scale;
                // (parent_buf / parent_cap are filled in when the launch is built: a later entry of this frame may
                // still grow the parent segment)
                for (uint32_t k = 0; k < P.n_lplanes; k++)
                    if (P.lplane_emission[k] == (int32_t)i) op.parent_lplane = k;
                op.n_count = es.count, op.n_start = es.offset_start, op.n_end = es.offset_end;
                levels[i].n.push_back(op);
            }
        }
    }
    fr.new_static = new_static, fr.pre_hdr_ok = pre_hdr_ok, fr.pre_tracked = pre_tracked;
    return FW_OK;
}

// Rings of spawners with Nested entries: a frame that runs a Nested pass (anywhere in the context: the launches are
// per emission level) materialises their new particles with fw_k_spawn, at their level, so that the per-parent pass
// finds them in memory (core.rs:488); any other frame spawns them inside fw_k_update_fifo like every other ring's.
void route_ring_ops(fw_ctx *ctx, FwFrame &fr) {
    auto &levels = ctx->levels;
    for (auto &L : levels) fr.nested_frame |= !L.n.empty();
    for (auto &io : ctx->fifo_mat_ops) {
        if (fr.nested_frame) {
            io.second.head = ctx->segs[io.second.seg].enqueue_head();
            levels[io.first].g.push_back(io.second);
        } else {
            ctx->fifo_ops.push_back(io.second);
        }
    }
    // (range rings other particles' entries emit from: the same choice; materialised at the tail of the ring -- the slot of
    // the list's first particle follows from the old part's size, which the device keeps: FwOp::range_ring)
    for (auto &io : ctx->range_mat_ops) {
        if (fr.nested_frame) {
            io.second.head = ctx->segs[io.second.seg].enqueue_head(), io.second.range_ring = 1u;
            levels[io.first].g.push_back(io.second);
        } else {
            ctx->range_ops.push_back(io.second);
        }
    }
    // every routed op now sits in exactly one list `rollback` walks (levels[].g, fifo_ops or range_ops): forgetting this one
    // too would take its particles out of cum_spawn twice
    ctx->fifo_mat_ops.clear(), ctx->range_mat_ops.clear();

    // A ring that had to grow past its mode's slot limit inside the spawner loop (realloc_segment) continues as a compacting
    // segment from this very frame: the ops already queued for it as a ring's go where a compacting segment's ops go -- its
    // emission level -- or they would never be spawned while cum_spawn, ub and the lifetime window count them.
    if (!ctx->seg_kind_changed) return;
    auto reroute = [&](std::vector<FwOp> &list, bool was_fifo) {
        size_t w = 0;
        for (size_t r = 0; r < list.size(); r++) {
            const FwOp &op = list[r];
            const SegHost &S = ctx->segs[op.seg];
            if (was_fifo ? S.fifo : S.range) {
                list[w++] = op;
                continue;
            }
            size_t lvl = 0;
            const SpawnerHost &osp = ctx->spawners[S.spawner];
            for (size_t i = 0; i < osp.em.size(); i++)
                if (osp.em[i].emit_idx == op.emit) lvl = i;
            levels[lvl].g.push_back(op);
            if (!(fr.dt < osp.em[lvl].life_lo_safe)) fr.new_static = false;  // (the test a compacting segment's op gets in spawner_loop)
        }
        list.resize(w);
    };
    reroute(ctx->fifo_ops, true);
    reroute(ctx->range_ops, false);
    for (auto &L : levels)
        for (FwOp &op : L.g)
            if (op.range_ring && !ctx->segs[op.seg].range) op.range_ring = 0u, op.head = 0u;
}

// ---- Nested entries run INSIDE the FIFO launch (fw_kernels.h: FwFifoNest; core.rs:471-546).  Every Nested entry of the frame
// must qualify -- parents in a FIFO ring the host knows the count of (Global-fed), spawned inside the update kernel
// (virt_parent), no other entry emitting from them; children received by a FIFO ring nothing else feeds and nothing emits from;
// both in the one FIFO launch of the context, parents first; no instance buffers, no colliders -- and no ring may wait for
// fw_k_spawn (the ops left at the levels then belong to compacting segments, which no Nested entry of the frame touches: the
// general launch spawns them itself).  Otherwise the frame runs the separate passes (fw_k_spawn / fw_k_nest), as before.
void plan_fuse(fw_ctx *ctx, FwFrame &fr) {
    const float dt = fr.dt;
    if (fr.nested_frame && ctx->nest_fuse && !fr.any_coll && !ctx->seg_kind_changed && ctx->update_mode == FW_MODE_FUSED && ctx->census.n_fifo != 0 &&
        ctx->census.n_fifo <= FW_FIFO_PER_LAUNCH && ctx->fifo_ops.size() <= FW_INLINE_OPS && !fr.ring_stats.fifo_coll && !fr.ring_stats.fifo_inst &&
        dt >= 0.0f && std::isfinite(dt)) {
        bool fuse = true;
        for (auto &L : ctx->levels) {
            for (const FwOp &op : L.g) fuse &= !ctx->segs[op.seg].ring();
            for (const FwNestOp &op : L.n) {
                if (!fuse || fr.n_fuse == FW_FIFO_NEST_MAX) {
                    fuse = false;
                    break;
                }
                const SegHost &P = ctx->segs[op.parent_seg], &Cs = ctx->segs[op.child_seg];
                const uint32_t p_in = P.ub - std::min(P.ub, P.frame_spawn);  // (a Global-fed FIFO ring: `ub` is exact)
                fuse = P.fifo && !P.fifo_dev && P.virt_parent && P.n_lplanes == 1 && Cs.fifo && Cs.fifo_dev && Cs.n_lplanes == 0 &&
                       op.parent_seg < op.child_seg && Cs.capacity <= FW_RANGE_MAX_CAPACITY &&
                       // the ring must not wrap into its head tile: the tiles' ranks are then the list order
                       (uint64_t)(P.head % FW_TILE) + p_in <= P.capacity;
                for (uint32_t k = 0; k < fr.n_fuse; k++)
                    fuse &= fr.fuse_plan[k].parent_seg != op.parent_seg && fr.fuse_plan[k].parent_seg != op.child_seg &&
                            fr.fuse_plan[k].child_seg != op.parent_seg && fr.fuse_plan[k].child_seg != op.child_seg;
                if (fuse) fr.fuse_plan[fr.n_fuse++] = op;
            }
            if (!fuse) break;
        }
        fr.fuse = fuse && fr.n_fuse != 0;
    }
    if (fr.nested_frame) (fr.fuse ? ctx->fused_nest_frames : ctx->nest_pass_frames)++;
}

// ---- segment -> tile table (device resident, re-uploaded only when a bound moves out of its band), and room for the op tables
// of either form: the last things that can fail before the frame is enqueued
fw_status finish_plan(fw_ctx *ctx, FwFrame &fr) {
    fr.prof(ctx, 1);
    fr.n_seg = (uint32_t)ctx->segs.size();
    fw_status st = update_tile_table(ctx);
    fr.prof(ctx, 2);
    if (st) return st;
    fr.total_tiles = ctx->total_tiles_dev;
    // (every per-tile array of the context -- status words, forecast entries, tile boxes -- holds tiles_cap entries: a table that
    // asks for more is a bookkeeping error, and nothing of the frame has been enqueued yet)
    if (fr.total_tiles > ctx->tiles_cap) return fail(ctx, FW_EHIP, "internal error: the tile table exceeds the tile scratch (frame not enqueued)");
    for (auto &L : ctx->levels) fr.n_g += L.g.size(), fr.n_n += L.n.size();
    return ensure_ring(ctx, fr, (size_t)fr.n_seg * 16 + fr.n_g * sizeof(FwOp) + fr.n_n * sizeof(FwNestOp) + 16);
}

}  // namespace

extern "C" {

// ---- the frame ---------------------------------------------------------------------------
fw_status fw_step(fw_ctx *ctx, float dt) {
    if (!ctx) return FW_EINVAL;
    hipSetDevice(ctx->device);
    FwFrame fr;
    fr.prof_t = std::chrono::steady_clock::now();
    fr.dt = dt;
    fw_status st = begin_frame(ctx, dt);
    if (!st) st = recover_missing_reports(ctx, dt);
    if (!st) st = segment_pass(ctx, fr);
    if (st) return st;
    ctx->undo_em.clear(), ctx->undo_sp.clear();
    if ((st = take_op_slot(ctx, fr))) return st;  // (nothing of the frame has been entered anywhere yet)
    fr.prof(ctx, 0);
    st = spawner_loop(ctx, fr);
    if (!st) {
        route_ring_ops(ctx, fr);
        plan_fuse(ctx, fr);
        st = finish_plan(ctx, fr);
    }
    if (st) return rollback(ctx, st);
    // ---- the frame will run
    fr.prof(ctx, 3);
    return enqueue_frame(ctx, fr);
}

}  // extern "C"
