// fw_engine_mem.cpp -- device / pinned memory of a context, exact counts, the error words of the update kernels
// (host engine of libfirework_hip.so: fw_engine.h lists its translation units; there is no CPU simulation path in this library)
#include "fw_engine.h"

namespace fwh {

fw_status sync(fw_ctx *ctx) {
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (what the caller waits for includes a withheld frame: fw_ctx::withheld)
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->side_dirty) {
        FW_HIP(ctx, hipStreamSynchronize(ctx->fifo_stream));
        ctx->side_dirty = false;
    }
    ctx->main_reads_ring = false;
    return FW_OK;
}

// before work that reads ring data is enqueued on the main stream without a synchronisation: the main stream waits for
// the ring launches on the side stream (and the next ring launch will wait for that work)
fw_status join_side(fw_ctx *ctx) {
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (work that reads ring data comes behind a withheld frame: fw_ctx::withheld)
    if (ctx->side_dirty) {
        FW_HIP(ctx, hipEventRecord(ctx->ev_side, ctx->fifo_stream));
        FW_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
        ctx->side_dirty = false;
    }
    ctx->main_reads_ring = true;
    return FW_OK;
}

// the age rule's per-frame condition on dt: the host's cohort sums and the device's `age + dt` are the same fp32 additions only where
// neither side may treat dt differently -- +0, or a positive normal finite value (a denormal may be flushed on one side only)
bool ageless_dt_ok(float dt) { return !std::signbit(dt) && (dt == 0.0f || std::isnormal(dt)); }

// What ensure_ages and ensure_spin share: one entry (E) per cohort that holds particles -- the ring's live particles are its cohorts laid
// end to end, oldest first -- and `tail` bytes behind them, through the one staging buffer of `T` into its device table, in the stream
// of the kernel that reads it.  stream null: the main stream, which first waits for the ring launches on the side stream.  `work`
// false: only that.  build(entries, &live) writes the entries (and what follows them) and returns their number; launch(stream, live,
// table, n) enqueues the kernel, and the fence goes behind it: it covers the pinned words (the copy) and the device table (the kernel).
template <typename E, typename Build, typename Launch>
static fw_status replay_cohorts(fw_ctx *ctx, uint32_t si, hipStream_t stream, bool work, fw_ctx::CohortTable &T, size_t tail, size_t floor,
                                Build build, Launch launch) {
    const SegHost &S = ctx->segs[si];
    fw_status st;
    if (!stream) {
        if ((st = join_side(ctx))) return st;
        stream = ctx->stream;
    }
    if (!work) return FW_OK;
    const size_t need = S.coh.size() * sizeof(E) + tail;
    char *h;
    if ((st = T.h.take(ctx, need, std::max(need * 2, floor), &h, &T.d))) return st;
    uint64_t live = 0;
    const uint32_t n = build(reinterpret_cast<E *>(h), &live);
    if (live > S.capacity) return poison_segment(ctx, si, "a FIFO ring's cohorts hold more particles than the ring");
    if (n) {
        FW_HIP(ctx, hipMemcpyAsync(T.d, h, n * sizeof(E) + tail, hipMemcpyHostToDevice, stream));
        FW_HIP(ctx, launch(stream, (uint32_t)live, reinterpret_cast<const E *>(T.d.get()), n));
        if ((st = T.h.commit(ctx, stream))) return st;
        T.launches++;
    }
    return FW_OK;
}

fw_status ensure_ages(fw_ctx *ctx, uint32_t si, hipStream_t stream) {
    SegHost &S = ctx->segs[si];
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (whoever asks is about to read, copy or launch over the ring: fw_ctx::withheld)
    if (!S.ages_stale) return FW_OK;
    fw_status st = replay_cohorts<FwAgeEntry>(
        ctx, si, stream, S.fifo && !S.coh.empty(), ctx->age_tab, 0, 1024 * sizeof(FwAgeEntry),
        [&](FwAgeEntry *tab, uint64_t *live) {  // (fw_ages.h)
            uint32_t n = 0;
            for (const SegHost::Cohort &c : S.coh) {
                if (!c.n) continue;
                tab[n++] = FwAgeEntry{(uint32_t)*live, c.age};
                *live += c.n;
            }
            return n;
        },
        [&](hipStream_t s, uint32_t live, const FwAgeEntry *tab, uint32_t n) { return fw_launch_fifo_ages(s, S.buf[0], S.capacity, S.head, live, tab, n); });
    if (st) return st;
    S.ages_stale = false;
    return FW_OK;
}

// the deferred spin's per-frame condition on dt: a positive normal fp32 (after a frame of +0 the newest cohort would take the next
// frame's spawn in, and one cohort would hold particles with different numbers of pending steps)
bool spin_dt_ok(float dt) { return !std::signbit(dt) && std::isnormal(dt); }

fw_status ensure_spin(fw_ctx *ctx, uint32_t si, hipStream_t stream, bool keep_streak) {
    SegHost &S = ctx->segs[si];
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (as in ensure_ages)
    if (!keep_streak) S.spin_streak = 0;
    if (!S.spin.stale) return FW_OK;
    // behind the entries: the log (fw_spin.h); a ring that was emptied since has nothing to replay
    const size_t log_n = S.spin.log.size();
    const bool pending = S.fifo && !S.coh.empty() && log_n;
    fw_status st = replay_cohorts<FwSpinEntry>(
        ctx, si, stream, pending && S.axis != 0u, ctx->spin_tab, log_n * sizeof(float), 16384,
        [&](FwSpinEntry *tab, uint64_t *live) {
            const uint32_t n = S.spin.table(S.coh, tab, live);
            std::copy(S.spin.log.begin(), S.spin.log.end(), reinterpret_cast<float *>(tab + n));
            return n;
        },
        [&](hipStream_t s, uint32_t live, const FwSpinEntry *tab, uint32_t n) {
            return fw_launch_fifo_spin(s, S.buf[0], S.capacity, S.head, live, ctx->d_types + S.type_idx, S.axis, tab, n, (uint32_t)log_n);
        });
    if (st) return st;
    if (pending && S.axis == 0u) return poison_segment(ctx, si, "a FIFO ring with a deferred spin lost its axis");
    S.spin.current(S.coh);
    S.spin_last = false;
    return FW_OK;
}

// grows the [2][max_seg] bookkeeping arrays and the snapshot ring: every new array is made (and filled) before any is installed --
// the rows of the [2][max_seg] ones sit max_seg apart
fw_status ensure_max_seg(fw_ctx *ctx, uint32_t need) {
    if (need <= ctx->max_seg) return FW_OK;
    fw_status st = sync(ctx);
    if (st) return st;
    const uint32_t omax = ctx->max_seg, nmax = std::max<uint32_t>(need, omax ? omax * 2 : 1024);
    HipBuf<uint32_t> *const cur[6] = {&ctx->gm.count, &ctx->gm.spawned, &ctx->gm.appended, &ctx->gm.rold, &ctx->gm.ndestroyed, &ctx->gm.range_ticket};
    HipBuf<uint32_t> nb[6], segids;
    HipBuf<unsigned long long> snap;
    for (int i = 0; i < 6; i++) {
        const int rows = i < 4 ? 2 : 1;
        if ((st = alloc_buf(ctx, nb[i], (size_t)rows * nmax, Mem::device, true))) return st;
        for (int r = 0; r < rows && omax; r++)
            FW_HIP(ctx, hipMemcpy(nb[i] + (size_t)r * nmax, *cur[i] + (size_t)r * omax, omax * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    }
    if ((st = alloc_buf(ctx, snap, (size_t)kSnapRing * nmax, Mem::pinned, true))) return st;
    if ((st = alloc_buf(ctx, segids, nmax))) return st;
    for (int i = 0; i < 6; i++) *cur[i] = std::move(nb[i]);
    ctx->g.count = ctx->gm.count, ctx->g.spawned = ctx->gm.spawned, ctx->g.appended = ctx->gm.appended, ctx->g.rold = ctx->gm.rold;
    ctx->g.ndestroyed = ctx->gm.ndestroyed, ctx->g.range_ticket = ctx->gm.range_ticket;
    ctx->h_snap = std::move(snap);
    for (int i = 0; i < kSnapRing; i++) ctx->snap_pending[i] = false;
    ctx->d_segids = std::move(segids);
    ctx->max_seg = nmax;
    ctx->g.max_seg = nmax;
    return FW_OK;
}

// tiles the update grid must cover for a segment: the live region in tiles of FW_TILE, plus this frame's new
// particles in tiles of FW_VTILE (fw_k_update's tiling of the index space)
uint32_t seg_live_tiles(const SegHost &s) {
    const uint32_t live_ub = s.nested_fed ? s.capacity : std::min(s.ub - std::min(s.ub, s.frame_spawn), s.capacity);
    return (live_ub + FW_TILE - 1) / FW_TILE;
}
uint32_t seg_tiles(const SegHost &s, uint32_t vt_rounds) {
    if (!s.in_use || s.ring() || s.small) return 0;  // (rings and small types have their own launches: fw_k_update_fifo / _range / _small)
    const uint32_t vtile = vt_rounds * FW_VTILE;
    if (!s.nested_fed && s.frame_spawn <= FW_VTILE) {
        // At most one round of new particles: they ride in the last live tile whenever it has room for them (both
        // update kernels apply the same rule), otherwise they take one tile of their own right behind it -- either
        // way ceil((live + new) / FW_TILE) tiles, for any live count up to the bound.  Thousands of small emitters
        // then cost ONE workgroup each instead of three (every workgroup pays ~5 us of launch-time latencies).
        const uint64_t live_ub = std::min(s.ub - std::min(s.ub, s.frame_spawn), s.capacity);
        return std::max<uint32_t>(1, (uint32_t)((live_ub + s.frame_spawn + FW_TILE - 1) / FW_TILE));
    }
    // (new particles beyond the capacity are dropped by the kernels -- spawn_room -- and need no tiles: a burst of 30 000 queued
    // particles into a type with 4096 caller-given slots used to ask for 118 new-particle tiles, more than the tile scratch of the
    // context -- ensure_tile_arrays, sized from the capacities -- holds: the entries of tiles beyond it were written out of bounds
    // (round 6: found as `check 2` under GPU contention, tools/r06_burst_repro.py))
    const uint32_t spawn_eff = std::min(s.frame_spawn, s.capacity);
    return std::max<uint32_t>(1, seg_live_tiles(s) + (spawn_eff + vtile - 1) / vtile + 1);
}

// (size of the new-particle tiles of a frame, update_tile_table: the smallest -- most parallel -- of 1 or 2 rounds for
// which all ACTIVE tiles of the frame are resident at once (kResidentSlots workgroups: 4 per CU); a second, nearly
// empty round of workgroups would cost a full tile lifetime)

// tile scratch sized for every segment at full capacity
fw_status ensure_tile_arrays(fw_ctx *ctx) {
    size_t tiles = 0, nest_tiles = 0, nest_ops = 0;
    for (auto &s : ctx->segs)
        // (worst case: every slot a new particle -- in one-round tiles -- behind a full buffer of live ones that all die: the bound of
        // update_tile_table's cap_tiles, whatever the frame asks for)
        if (s.in_use && !s.ring()) tiles += (s.capacity + FW_TILE - 1) / FW_TILE + (s.capacity + FW_VTILE - 1) / FW_VTILE + 3;
    for (auto &sp : ctx->spawners) {
        if (!sp.alive) continue;
        for (auto &e : sp.em)
            if (e.es.mode == FW_MODE_NESTED) {
                nest_tiles += (ctx->segs[sp.seg[e.es.target_particle_type]].capacity + FW_NEST_TILE - 1) / FW_NEST_TILE + 1;
                nest_ops++;
            }
    }
    fw_status st;
    if (tiles > ctx->tiles_cap) {
        if ((st = sync(ctx))) return st;
        size_t ncap = tiles * 2;
        auto &m = ctx->gm;
        ctx->tiles_cap = 0, drop_forecast_and_boxes(ctx);
        ctx->fc_len = ncap + (ncap / 64 + 2) * FW_FC_S2_STRIDE + 8;  // P | P2 | tag (64-bit words)
        if ((st = alloc_buf(ctx, m.tile_cnt, ncap, Mem::device, false, &ctx->g.tile_cnt)) ||
            (st = alloc_buf(ctx, m.tile_off, ncap, Mem::device, false, &ctx->g.tile_off)) ||
            (st = alloc_buf(ctx, m.tile_status, ncap, Mem::device, true, &ctx->g.tile_status)) ||
            (st = alloc_buf(ctx, m.tile_box, ncap * 8, Mem::device, true, &ctx->g.tile_box)) ||
            (st = alloc_buf(ctx, m.dbg_ts, 32768 + 8 * ncap, Mem::device, true, &ctx->g.dbg_ts)) ||
            (st = alloc_buf(ctx, ctx->d_fce, 2 * ncap, Mem::device, true)) || (st = alloc_buf(ctx, ctx->d_fc, 3 * ctx->fc_len, Mem::device, true)))
            return st;
        ctx->fc_dirty = false;
        ctx->tiles_cap = ncap;
    }
    if (nest_tiles > ctx->gm.nest_status.cap()) {
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->gm.nest_status, nest_tiles * 2, Mem::device, true, &ctx->g.nest_status))) return st;
    }
    if (nest_ops > ctx->gm.nest_ticket.cap()) {
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->gm.nest_ticket, nest_ops * 2 + 16, Mem::device, true, &ctx->g.nest_ticket))) return st;
    }
    return FW_OK;
}

// device table, look-back words and per-frame pinned records of the range launch, sized for the worst case of every range
// segment (old + young workgroups cover at most the ring, new ones at most a ring of new particles) when a segment is built
// or reallocated: fw_step itself never allocates for them
fw_status ensure_range_arrays(fw_ctx *ctx) {
    size_t tiles = 0;
    for (auto &s : ctx->segs)
        if (s.in_use && s.range)  // OLD tiles of FW_TILE, YOUNG tiles of the build's size, NEW workgroups of FW_BLOCK
            // (... or, a launch on one-round tiles -- fw_ctx::range_small -- OLD and YOUNG tiles of FW_BLOCK)
            tiles += 2 * ((size_t)s.capacity / FW_BLOCK + 4) + (size_t)s.capacity / FW_BLOCK + 2;
    fw_status st;
    if (tiles > ctx->rdesc_cap) {
        if ((st = sync(ctx))) return st;
        const size_t ncap = tiles + tiles / 2 + 64;
        ctx->rdesc_cap = 0;
        if ((st = alloc_buf(ctx, ctx->d_rdesc, ncap)) || (st = alloc_buf(ctx, ctx->h_rdesc, ncap, Mem::pinned)) ||
            (st = alloc_buf(ctx, ctx->d_rstatus, ncap, Mem::device, true)))
            return st;
        // per-workgroup timestamps of the last range launch (tools/range_timeline.py)
        if ((ctx->dbg & 8u) && (st = alloc_buf(ctx, ctx->d_rts, ncap * 8, Mem::device, true))) return st;
        ctx->rdesc_cap = ncap;
        ctx->r_force = true, ctx->rtab_fence.forget();
    }
    // one record per segment slot + one op per emission entry of the context
    const size_t need = round_up((uint32_t)(ctx->max_seg * sizeof(FwRangeRec)), 64) + (size_t)(ctx->n_emits + 8) * sizeof(FwOp) + 64;
    if (ctx->census.n_range && need > ctx->rparam_bytes) {
        if ((st = sync(ctx))) return st;
        const size_t nb = need * 2;
        ctx->rparam_bytes = 0;
        for (int i = 0; i < kParamRing; i++) {
            if ((st = alloc_buf(ctx, ctx->h_rparam[i], nb, ctx->param_bar ? Mem::fine : Mem::pinned, true))) return st;
            ctx->rslot_frame[i] = 0;
        }
        ctx->rparam_bytes = nb;
    }
    return FW_OK;
}

// slot of particle 0 of a segment whose live count is `count` (exact): 0 unless the segment is a ring
// (a range ring: the old part sits right before the young part; its size is the device's -- rold_seen, refreshed together
// with the exact counts -- for a type that receives Nested children, and count - young_n, the same number, otherwise)
uint32_t ring_head_exact(const SegHost &S, uint32_t count) {
    if (S.fifo) return S.head;
    if (!S.range) return 0u;
    const uint32_t n_old = S.range_dev ? std::min(S.rold_seen, count) : (count > S.young_n ? count - S.young_n : 0u);
    return (uint32_t)(((uint64_t)S.young_lo + S.capacity - (n_old % S.capacity)) % S.capacity);
}

// How the readers outside the update kernels find the particles of segment si in buffer `parity` (FwSegView, fw_kernels.h): the one
// place a view is made, every field from SegHost.  There are two heads.  A launch that is enqueued behind updates still in
// flight cannot know a range ring's old part: it gets the first young slot and the device's word of FwGlobals::rold ...
FwSegView seg_view(const fw_ctx *ctx, uint32_t si, uint32_t parity) {
    const SegHost &S = ctx->segs[si];
    FwSegView v{};
    v.buf = S.buf[parity], v.capacity = S.capacity;
    v.head = S.enqueue_head();
    v.d_rold = S.range ? ctx->g.rold + (size_t)parity * ctx->max_seg + si : nullptr;
    v.cpl = S.cpl_bits();
    v.nospin = S.nospin ? 1u : 0u;
    v.rot = S.nospin ? make_float4(S.const_rot[0], S.const_rot[1], S.const_rot[2], S.const_rot[3]) : make_float4(0.f, 0.f, 0.f, 1.f);
    v.life_plane = S.life_plane(), v.life_const = S.fifo_life;
    v.derived = S.derived ? ctx->d_types + S.type_idx : nullptr, v.keys = ctx->d_keys;
    return v;
}
// ... a caller that has waited for the stream and holds the segment's exact `count` (read_counts) places particle 0 itself
// (ring_head_exact): the form of the synchronous readers
FwSegView seg_view_exact(const fw_ctx *ctx, uint32_t si, uint32_t parity, uint32_t count) {
    FwSegView v = seg_view(ctx, si, parity);
    v.head = ring_head_exact(ctx->segs[si], count), v.d_rold = nullptr;
    return v;
}

fw_status ensure_param_ring(fw_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->param_bytes) return FW_OK;
    fw_status st = sync(ctx);
    if (st) return st;
    FW_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    size_t nb = std::max<size_t>(bytes * 2, 1 << 16);
    ctx->param_bytes = 0;
    for (int i = 0; i < kParamRing; i++) {
        if ((st = alloc_buf(ctx, ctx->h_param[i], nb, Mem::pinned)) || (st = alloc_buf(ctx, ctx->d_param[i], nb))) return st;
        ctx->consumed[i].forget();
    }
    ctx->param_bytes = nb;
    return FW_OK;
}

// A parameter slot the kernels read in place is tagged with the frame that used it last (+1; 0 = free): free once a launch AFTER
// that frame has started, which the pinned "frame started" word (h_done) tells
fw_status wait_slot_free(fw_ctx *ctx, uint64_t &tag) {
    if (!tag) return FW_OK;
    const volatile unsigned long long *done = ctx->h_done;
    for (int spin = 0; *done < tag && spin < 200000; spin++) __builtin_ia32_pause();
    if (*done < tag) FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tag = 0;
    return FW_OK;
}

// A parameter slot of the ring (pinned host memory the kernels read in place, or stage from): free once the frame that used
// it last has been consumed.
fw_status acquire_slot(fw_ctx *ctx, int *out) {
    const int slot = (int)(ctx->ring_seq++ % kParamRing);
    fw_status st;
    if ((st = ctx->consumed[slot].wait(ctx)) || (st = wait_slot_free(ctx, ctx->slot_frame[slot]))) return st;  // (... zero-copy use)
    *out = slot;
    return FW_OK;
}

fw_status upload_seg(fw_ctx *ctx, uint32_t si) {
    const SegHost &s = ctx->segs[si];
    FwSeg d{};
    d.buf[0] = s.buf[0], d.buf[1] = s.buf[1];
    d.destroyed = s.destroyed;
    d.capacity = s.capacity;
    d.type_idx = s.type_idx;
    d.n_lplanes = s.n_lplanes;
    d.inst = s.inst, d.inst_cap = s.inst_cap;
    d.cpl = s.cpl_bits();  // (a ring's Q1 / Q3 regions, a FIFO ring's Q2 too: component planes, fw_device.h)
    d.lplane_emit[0] = d.lplane_emit[1] = 0xFFFFFFFFu;
    if (s.virt_parent && s.spawner >= 0)
        for (uint32_t k = 0; k < s.n_lplanes && k < 2u; k++) {
            const auto &em = ctx->spawners[s.spawner].em;
            const int32_t ei = s.lplane_emission[k];
            if (ei >= 0 && (size_t)ei < em.size() && em[ei].assigned) d.lplane_emit[k] = em[ei].emit_idx;
        }
    FW_HIP(ctx, hipMemcpy(ctx->d_segs + si, &d, sizeof d, hipMemcpyHostToDevice));
    return FW_OK;
}

fw_status alloc_seg_buffers(fw_ctx *ctx, const SegHost &s, uint32_t capacity, bool ring, bool want_destroyed, SegBufs &out) {
    const size_t bytes = FW_BUF_BYTES((size_t)capacity, s.n_lplanes + s.n_xplanes);
    if (alloc_buf(ctx, out.mem, bytes * (ring ? 1 : 2)))  // a ring is updated in place: one buffer
        return fail(ctx, FW_ENOMEM, "particle buffers: " + ctx->err);
    if (want_destroyed && alloc_buf(ctx, out.destroyed, (size_t)capacity * sizeof(fw_particle)))
        return fail(ctx, FW_ENOMEM, "destroyed buffer: " + ctx->err);
    out.buf[0] = out.mem;
    out.buf[1] = ring ? out.mem.get() : out.mem + bytes;
    out.capacity = capacity;
    FW_HIP(ctx, fw_launch_fill_colors(ctx->stream, out.buf[0], ring ? nullptr : out.buf[1], capacity, s.fill_bc, s.fill_em));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));  // callers go on with blocking copies on the null stream
    return FW_OK;
}

// the size of the old part of every range ring that receives Nested children, as the device has it (the stream has been
// waited for): what ring_head_exact derives such a ring's first slot from
fw_status refresh_rold(fw_ctx *ctx) {
    bool any = false;
    for (const SegHost &S : ctx->segs) any |= S.in_use && S.range && S.range_dev;
    if (!any) return FW_OK;
    const uint32_t n = (uint32_t)ctx->segs.size();
    std::vector<uint32_t> r(n);
    FW_HIP(ctx, hipMemcpy(r.data(), ctx->g.rold + (size_t)ctx->parity * ctx->max_seg, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++)
        if (ctx->segs[i].in_use && ctx->segs[i].range) ctx->segs[i].rold_seen = r[i];
    return FW_OK;
}

// exact device counts -> host upper bounds (synchronises)
fw_status refresh_counts_exact(fw_ctx *ctx) {
    fw_status st = sync(ctx);
    if (st) return st;
    const uint32_t n = (uint32_t)ctx->segs.size();
    if (!n) return FW_OK;
    std::vector<uint32_t> c(n);
    FW_HIP(ctx, hipMemcpy(c.data(), count_slot(ctx), n * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++)
        if (ctx->segs[i].in_use) ctx->segs[i].ub = c[i];
    for (int i = 0; i < kSnapRing; i++) ctx->snap_pending[i] = false;
    return refresh_rold(ctx);
}

fw_status check_device_errors(fw_ctx *ctx) {
    // (the stream has been waited for: whatever a kernel reported is in the pinned word by now)
    const bool fresh = poll_device_error(ctx);
    // (every kernel that sets a flag says so in the pinned word next to err_host -- fw_flag: nothing there, nothing to fetch)
    if (!*(const volatile unsigned long long *)(ctx->h_err + 1) && !ctx->trace) return FW_OK;
    ctx->h_err[1] = 0ull;
    uint32_t ev[8] = {};
    FW_HIP(ctx, hipMemcpy(ev, ctx->g.err, sizeof ev, hipMemcpyDeviceToHost));
    const uint32_t e = ev[0];
    if (ctx->trace && ctx->d_tile_first) {
        uint32_t t[2] = {77, 77};
        hipMemcpy(t, ctx->d_tile_first, sizeof t, hipMemcpyDeviceToHost);
        fprintf(stderr, "[fw] check: flags=%u table=[%u,%u] ptr=%p fc=%p tiles_cap=%zu\n", e, t[0], t[1],
                (void *)ctx->d_tile_first, (void *)ctx->d_fc, ctx->tiles_cap);
    }
    if (!e) return FW_OK;
    uint32_t zero = 0;
    FW_HIP(ctx, hipMemcpy(ctx->g.err, &zero, sizeof zero, hipMemcpyHostToDevice));
    // (the two bits are looked at independently -- a word with both set used to lose the capacity report when the internal
    // error was not news: ADVICE r04 -- and the more severe status wins)
    fw_status cap = FW_OK;
    if (e & FW_ERR_CAPACITY)
        cap = fail(ctx, FW_ECAPACITY,
                   "a particle type overflowed its device capacity; particles were dropped "
                   "(raise fw_particle_settings.capacity) [device flags " + std::to_string(e) + ", segment " +
                       std::to_string(ev[1]) + ": " + std::to_string(ev[2]) + " particles (" + std::to_string(ev[4]) +
                       " resident), " + std::to_string(ev[3]) + " tiles launched]");
    if ((e & FW_ERR_FORECAST) && fresh) {
        // An internal check of an update kernel failed.  The spawner it names is marked (poll_device_error): its own calls
        // refuse from now on.  Whoever synchronises first is told once; later synchronisations -- of healthy spawners -- are
        // not failed again for an error that has been reported and contained.
        ctx->poison_msg += " [device flags " + std::to_string(e) + ", check " + std::to_string(ev[5]) + ": " + std::to_string(ev[6]) +
                           " " + std::to_string(ev[7]) + "]";
        return poisoned_status(ctx);
    }
    return cap;  // FW_ERR_LOOKBACK_TIMEOUT is informational: the fallback path produced the same result
}

// The pinned error word (FwGlobals::err_host): a kernel's internal check failed.  No synchronisation, no HIP call: fw_step and
// every reader look here first.  The spawner the segment belongs to (every spawner, when the error names none) is marked.
bool poll_device_error(fw_ctx *ctx) {
    const volatile unsigned long long *w = ctx->h_err;
    const unsigned long long v = w ? *w : 0ull;
    if (!v) return false;
    *ctx->h_err = 0ull;
    const uint32_t check = (uint32_t)(v >> 32) & 0x7FFFFFFFu, seg = (uint32_t)v;
    // (frames enqueued before the host looked here repeat the report: only a spawner that was healthy so far is news)
    bool one = false, news = false;
    if (seg < ctx->segs.size() && ctx->segs[seg].in_use && ctx->segs[seg].spawner >= 0 &&
        (size_t)ctx->segs[seg].spawner < ctx->spawners.size()) {
        SpawnerHost &sp = ctx->spawners[ctx->segs[seg].spawner];
        news = !sp.poisoned;
        sp.poisoned = true;
        one = true;
        ctx->n_poisoned++;
    }
    if (!one)
        for (auto &sp : ctx->spawners) news |= sp.alive && !sp.poisoned, sp.poisoned |= sp.alive, ctx->n_poisoned++;
    if (!news) return false;
    ctx->poison_msg = "internal error: check " + std::to_string(check) + " of an update kernel failed" +
                      (one ? " for segment " + std::to_string(seg) : std::string()) +
                      "; the particle state of the spawner is invalid -- rebuild it with fw_spawner_update_settings (drops its "
                      "particles) or destroy it";
    return true;
}
fw_status poisoned_status(fw_ctx *ctx) { return fail(ctx, FW_EHIP, ctx->poison_msg.empty() ? "spawner poisoned by an earlier internal error" : ctx->poison_msg); }
// A check of the HOST half of fw_step failed after the frame's bookkeeping was committed (clocks, RNG serials, cohorts, ring heads
// have advanced; a launch may be out): nothing can be rolled back, so the spawner the segment belongs to (every spawner, when no
// segment is named) is treated like one a kernel's check failed for -- sticky until rebuilt or destroyed
fw_status poison_segment(fw_ctx *ctx, uint32_t si, const std::string &what) {
    bool one = false;
    if (si < ctx->segs.size() && ctx->segs[si].in_use && ctx->segs[si].spawner >= 0 && (size_t)ctx->segs[si].spawner < ctx->spawners.size()) {
        SpawnerHost &sp = ctx->spawners[ctx->segs[si].spawner];
        if (!sp.poisoned) sp.poisoned = true, ctx->n_poisoned++;
        one = true;
    }
    if (!one)
        for (auto &sp : ctx->spawners)
            if (sp.alive && !sp.poisoned) sp.poisoned = true, ctx->n_poisoned++;
    ctx->poison_msg = "internal error: " + what + (one ? " (segment " + std::to_string(si) + ")" : std::string()) +
                      "; the particle state of the spawner is invalid -- rebuild it with fw_spawner_update_settings (drops its "
                      "particles) or destroy it";
    return poisoned_status(ctx);
}

SpawnerHost *get_spawner(fw_ctx *ctx, fw_spawner h) {
    if (!ctx || h < 0 || (size_t)h >= ctx->spawners.size() || !ctx->spawners[h].alive) {
        if (ctx) ctx->err = "invalid spawner handle";
        return nullptr;
    }
    return &ctx->spawners[h];
}

fw_status read_counts(fw_ctx *ctx, std::vector<uint32_t> &out) {
    fw_status st = sync(ctx);
    if (st) return st;
    out.assign(ctx->segs.size(), 0);
    if (!out.empty())
        FW_HIP(ctx, hipMemcpy(out.data(), count_slot(ctx),
                              out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if ((st = refresh_rold(ctx))) return st;
    return check_device_errors(ctx);
}

// ParticleSpawnerData::active (core.rs:288-302) with exact device counts
bool spawner_active(const fw_ctx *ctx, const SpawnerHost &sp, const std::vector<uint32_t> &counts) {
    bool any = false;
    for (uint32_t si : sp.seg) any |= counts[si] != 0;
    bool enabled = false;
    for (const EmissionHost &e : sp.em) enabled |= e.emits_on_other_particles ? (e.enabled && any) : e.enabled;
    (void)ctx;
    return enabled;
}

}  // namespace fwh
