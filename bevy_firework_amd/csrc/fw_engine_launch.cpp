// fw_engine_launch.cpp -- the enqueue of a frame fw_step has planned (fw_engine_step.cpp, FwFrame): update arguments and forecast,
// the spawn / nest passes or the op table, the FIFO, range, small and general launches, the frame's bookkeeping.  Nothing here
// rolls back: a failure from here on leaves the frame half enqueued, and the paths that cannot continue poison what they touched.
// (host engine of libfirework_hip.so: fw_engine.h lists its translation units; there is no CPU simulation path in this library)
#include "fw_engine.h"

namespace fwh {

// (the ring may be re-allocated when a frame needs more than it holds: a list that lives in it moves out first)
fw_status ensure_ring(fw_ctx *ctx, FwFrame &fr, size_t bytes) {
    if (bytes > ctx->param_bytes && fr.pre_slot >= 0) {
        ctx->levels[0].g.reserve_own(ctx->levels[0].g.size());
        fr.pre_slot = -1, fr.pre_hdr = nullptr, fr.pre_hdr_ok = false;
    }
    return ensure_param_ring(ctx, bytes);
}

}  // namespace fwh

namespace {

uint32_t next_nest_seq(fw_ctx *ctx) {  // the tag of a Nested launch's look-back words: 30 bits, never 0
    ctx->nest_seq = (ctx->nest_seq + 1u) & 0x3FFFFFFFu;
    if (!ctx->nest_seq) ctx->nest_seq = 1u;
    return ctx->nest_seq;
}

// sorted by segment, emission order kept inside a segment; a list in spawner (= segment creation) order is already sorted most
// of the time: no sort then
void sort_by_segment(FwOp *b, FwOp *e) {
    if (!std::is_sorted(b, e, [](const FwOp &x, const FwOp &y) { return x.seg < y.seg; }))
        std::stable_sort(b, e, [](const FwOp &x, const FwOp &y) { return x.seg < y.seg; });
}

// the headers of an op table: {first op, one past the last, particles} per segment (ops sorted by segment)
void write_op_headers(OpHdr *hdr, uint32_t n_seg, const FwOp *ops, size_t n_ops) {
    size_t oi = 0;
    for (uint32_t sgi = 0; sgi < n_seg; sgi++) {
        const size_t b = oi;
        uint64_t n = 0;
        while (oi < n_ops && ops[oi].seg == sgi) n += ops[oi].n, oi++;
        hdr[sgi] = OpHdr{(uint32_t)b, (uint32_t)oi, (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull), 0u};
    }
}

// (write-combining stores into host-written device memory, fw_ctx::b_param / h_rparam: drained, and known to have arrived -- a
// read may not pass posted writes -- before a launch that reads them is announced)
void drain_bar_writes(const void *p) {
    _mm_sfence();
    (void)*(volatile const uint32_t *)p;
}

// the main stream waits for the ring launches on the side stream
fw_status main_waits_side(fw_ctx *ctx) {
    FW_HIP(ctx, hipEventRecord(ctx->ev_side, ctx->fifo_stream));
    FW_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
    ctx->side_dirty = false;
    return FW_OK;
}

// Orders a launch that goes to the side stream (side) or the main one against the previous launch of its kind (on the side stream
// when last_side) and against readers of its data on the main stream (fw_ctx::main_reads_ring)
fw_status order_side(fw_ctx *ctx, bool side, bool &last_side) {
    if (side && (!last_side || ctx->main_reads_ring)) {
        // the previous launch, or a reader of its data, sits on the main stream: this launch comes after it
        FW_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
        FW_HIP(ctx, hipStreamWaitEvent(ctx->fifo_stream, ctx->ev_main, 0));
        ctx->main_reads_ring = false;
    } else if (!side && last_side && ctx->side_dirty) {
        fw_status st = main_waits_side(ctx);
        if (st) return st;
    }
    last_side = side;
    return FW_OK;
}

// timing: the events ride on the dispatch packet (its begin / end timestamps), no marker packets in the stream
void next_timing_pair(fw_ctx *ctx, FwFrame &fr, hipEvent_t *e0, hipEvent_t *e1) {
    *e0 = *e1 = nullptr;
    if (!ctx->timing || ctx->tev_used + 2 > ctx->tev.size()) return;
    *e0 = ctx->tev[ctx->tev_used], *e1 = ctx->tev[ctx->tev_used + 1];
    ctx->tev_used += 2;
    fr.timed = true;
}

// the arguments of the general launch, which the ring and small launches take their common part from
void update_args(fw_ctx *ctx, FwFrame &fr) {
    const uint32_t n_seg = fr.n_seg, p = fr.p;
    // Particle types with collision settings (core.rs:607-624) run the count / scan / update-with-collisions launches
    // (everything materialised first, like FW_UPDATE_MODE=split); the streaming kernels never see a collider.
    if (ctx->seg_kind_changed)  // (a colliding ring that left its mode inside the spawner loop is a compacting segment from this frame on)
        for (const SegHost &S : ctx->segs) fr.any_coll |= S.in_use && S.collides && !S.ring() && !S.small;
    fr.frame_mode = fr.any_coll ? FW_MODE_SPLIT_COLL : ctx->update_mode;
    fr.legacy = (fr.n_n != 0 && !fr.fuse) || fr.frame_mode != FW_MODE_FUSED;  // (fuse: the Nested entries run inside the FIFO launch)

    FwUpdateArgs &a = fr.a;
    a.seg_tile_first = ctx->d_tile_first;
    a.tile_desc = ctx->d_tile_desc;
    a.n_seg = n_seg;
    a.total_tiles = fr.total_tiles;
    a.parity = p;
    a.epoch = frame_epoch(ctx->frame);
    a.dt = fr.dt;
    a.spin_limit = ctx->spin_limit;
    a.dbg = ctx->dbg;
    a.vt_rounds = ctx->vt_rounds;
    a.resident_slots = (uint32_t)kResidentSlots;
    a.seg0_type = n_seg ? ctx->segs[0].type_idx | (ctx->segs[0].nospin ? FW_TYPE_IDX_NOSPIN : 0u) : 0;
    a.seg0_keys_off = n_seg ? ctx->segs[0].keys_off : 0;
    a.seg0_keys_len = n_seg ? ctx->segs[0].keys_len : 0;
    a.tile_keys = ctx->d_tile_keys;
    if (n_seg == 1 && ctx->segs[0].in_use && !ctx->segs[0].ring()) {
        const SegHost &S0 = ctx->segs[0];
        a.seg0_ib = S0.buf[p], a.seg0_ob = S0.buf[p ^ 1u];
        a.seg0_destroyed = S0.destroyed, a.seg0_inst = S0.inst;
        a.seg0_capacity = S0.capacity, a.seg0_n_lplanes = S0.n_lplanes, a.seg0_inst_cap = S0.inst_cap;
    }
    if (ctx->live_ring) {
        a.live_out = ctx->live_ring + (ctx->live_ring_frames % ctx->live_ring_n);
        a.live_next = ctx->live_ring + ((ctx->live_ring_frames + 1) % ctx->live_ring_n);
        ctx->live_ring_frames++;
    }
    a.new_static = (fr.new_static && ctx->use_static_new) ? 1u : 0u;
    a.boxes = (ctx->track_aabb && fr.frame_mode == FW_MODE_FUSED) ? 1u : 0u;
    a.force_colors = ctx->colors_dirty ? 1u : 0u;
    // (a ring that had to grow past the ring limit during this frame's spawner loop continues as a compacting segment:
    // look again -- never in a steady-state frame)
    if (ctx->seg_kind_changed)
        for (const SegHost &S : ctx->segs) fr.any_inst_general |= S.in_use && !S.ring() && S.inst != nullptr;
    a.any_inst = fr.any_inst_general ? 1u : 0u;
    a.use_stream = ctx->use_stream ? 1u : 0u;
    memcpy(&fr.dt_bits, &fr.dt, 4);
}

// survivor forecast of the compacting launch, and the threshold forecast of a dt that varies
fw_status set_forecast(fw_ctx *ctx, FwFrame &fr) {
    FwUpdateArgs &a = fr.a;
    const float dt = fr.dt;
    const uint32_t n_seg = fr.n_seg, total_tiles = fr.total_tiles, dt_bits = fr.dt_bits;
    const bool legacy = fr.legacy;
    // Frames with Nested entries materialise their new particles before the update; the streaming kernel takes them as
    // loaded new-particle tiles with static slots, which needs every one of them to survive the step (new_static).
    const bool split = fr.frame_mode != FW_MODE_FUSED;
    const bool fc_frame = !split && ctx->use_forecast && ctx->d_fc != nullptr;
    if (fc_frame) {
        for (uint32_t i = 0; i < n_seg; i++) a.fc_sums |= ctx->tiles_dev[i] > FW_FC_DIRECT ? 1u : 0u;
        const bool usable = ctx->fc_ok && ctx->fc_dt_bits == dt_bits && ctx->fc_tab_seq == ctx->tab_seq && a.epoch != 1u &&
                            ctx->fc_sums_prev == a.fc_sums &&  // the previous frame left the other format otherwise
                            (!legacy || (a.use_stream && a.new_static));
        if (ctx->fc_dirty) {
            // the tile indexing changed: sums left at indices of the old table must not leak into the new one
            FW_HIP(ctx, hipMemsetAsync(ctx->d_fc, 0, 3 * ctx->fc_len * sizeof(unsigned long long), ctx->stream));
            ctx->fc_dirty = false;
        }
        a.fc_s2 = (uint32_t)ctx->tiles_cap;
        a.fc_tag = (uint32_t)(ctx->fc_len - 1);
        a.fc_out = ctx->d_fc + (size_t)(ctx->fc_seq % 3u) * ctx->fc_len;
        a.fc_zero = ctx->d_fc + (size_t)((ctx->fc_seq + 1u) % 3u) * ctx->fc_len;
        a.fce_out = ctx->d_fce + (size_t)(ctx->fc_seq & 1u) * ctx->tiles_cap;
        a.fce_in = ctx->d_fce + (size_t)((ctx->fc_seq + 1u) & 1u) * ctx->tiles_cap;
        if (usable) a.fc_in = ctx->d_fc + (size_t)((ctx->fc_seq + 2u) % 3u) * ctx->fc_len;
        // ---- threshold forecast (fw_ctx::use_tf): a dt that differs from the previous frame's, below the theta its lists were made for
        const bool dt_same = ctx->fc_dt_bits == dt_bits;
        const bool tf_size = ctx->use_tf && !a.fc_sums && total_tiles >= ctx->tf_min_tiles && a.use_stream && dt > 0.0f && std::isfinite(dt);
        if (!usable && tf_size && ctx->tf_prev_theta > 0.0f && dt < ctx->tf_prev_theta && !dt_same && ctx->fc_ok &&
            ctx->fc_tab_seq == ctx->tab_seq && a.epoch != 1u && ctx->fc_sums_prev == a.fc_sums && (!legacy || a.new_static) &&
            ctx->tf_cap == ctx->tiles_cap) {
            FwResolveArgs ra{};
            ra.fce = ctx->d_fce + (size_t)((ctx->fc_seq + 1u) & 1u) * ctx->tiles_cap;
            ra.fct = ctx->d_fct + (size_t)((ctx->fc_seq + 1u) & 1u) * ctx->tiles_cap;
            ra.fcl = ctx->d_fcl + (size_t)((ctx->fc_seq + 1u) & 1u) * ctx->tiles_cap * FW_TF_K;
            ra.tile_desc = n_seg == 1 ? nullptr : ctx->d_tile_desc.get();
            ra.total_tiles = total_tiles, ra.parity = fr.p, ra.epoch = a.epoch, ra.dt = dt;
            FW_HIP(ctx, fw_launch_fc_resolve(ctx->stream, ctx->g, ra));
            a.fc_in = ctx->d_fc + (size_t)((ctx->fc_seq + 2u) % 3u) * ctx->fc_len;  // (per-tile entries: only its non-nullness matters)
            ctx->tf_frames++;
        }
        // producers: lists for the NEXT frame while dt has been seen to vary (64 frames after the last change)
        if (!dt_same && ctx->fc_ok) ctx->tf_armed = 64u;
        ctx->tf_prev_theta = 0.0f;
        if (tf_size && ctx->tf_armed) {
            ctx->tf_armed--;
            if (ctx->tf_cap != ctx->tiles_cap) {  // (first use, or the tile scratch grew: ensure_tile_arrays)
                ctx->tf_cap = 0;
                if (alloc_buf(ctx, ctx->d_fct, 2 * ctx->tiles_cap) == FW_OK && alloc_buf(ctx, ctx->d_fcl, 2 * ctx->tiles_cap * FW_TF_K) == FW_OK)
                    ctx->tf_cap = ctx->tiles_cap;
                else
                    (void)hipGetLastError();  // (no memory for the lists: the look-back schedule stays)
            }
            if (ctx->tf_cap == ctx->tiles_cap) {
                a.fc_theta = dt * 1.25f;
                a.fct_out = ctx->d_fct + (size_t)(ctx->fc_seq & 1u) * ctx->tiles_cap;
                a.fcl_out = ctx->d_fcl + (size_t)(ctx->fc_seq & 1u) * ctx->tiles_cap * FW_TF_K;
                ctx->tf_prev_theta = a.fc_theta;
            }
        }
        ctx->fc_seq++;
        ctx->fc_sums_prev = a.fc_sums;
        if (ctx->trace)
            fprintf(stderr, "[fw] frame %llu epoch %u fc: usable=%d ok=%d dt_same=%d tab %llu/%llu sums %u legacy=%d new_static=%u seq %llu tiles %u\n",
                    (unsigned long long)ctx->frame, a.epoch, (int)usable, (int)ctx->fc_ok, (int)(ctx->fc_dt_bits == dt_bits),
                    (unsigned long long)ctx->fc_tab_seq, (unsigned long long)ctx->tab_seq, a.fc_sums, (int)legacy, a.new_static,
                    (unsigned long long)ctx->fc_seq, total_tiles);
    }
    fr.fc_frame = fc_frame;
    return FW_OK;
}

// a snapshot row stays armed until its stores have been seen (a free-running host can be hundreds of frames
// ahead of the device; re-arming by frame number would never catch one)
void pick_snapshot(fw_ctx *ctx, FwFrame &fr) {
    int snap = -1;
    if ((ctx->frame % kSnapEvery) == 0)
        for (int k = 0; k < kSnapRing && snap < 0; k++)
            if (!ctx->snap_pending[k]) snap = k;
    // (small types are bounded by their lifetime windows and have no grid to size: a context of nothing else takes no snapshots --
    // a row is a pass over every segment record on the host and a store over the bus per segment on the device)
    if (ctx->census.n_in_use == ctx->census.n_small) snap = -1;
    fr.snap = snap;
    fr.a.host_counts = snap >= 0 ? ctx->h_snap + (size_t)snap * ctx->max_seg : nullptr;
}

// Frames with Nested entries: parents spawned earlier in the frame must exist in memory before the per-parent pass reads them
// (core.rs:488), so Global ops are materialised by fw_k_spawn, level by level.
// Not those of SMALL types (round 5): no Nested entry reads them, their kernel spawns them itself (virtual particles) from a
// table as in any other frame -- one spawner with a Nested entry among hundreds of small emitters used to send every op of
// the context through fw_k_spawn and its staged table: 512 small emitters 16.7 us per frame, with examples/textures.rs next
// to them 56.3 (profiles/r05/nested_among_small.txt).
fw_status spawn_passes(fw_ctx *ctx, FwFrame &fr) {
    auto &levels = ctx->levels;
    const uint32_t n_seg = fr.n_seg, p = fr.p;
    fw_status st = FW_OK;
    const bool small_virtual = ctx->census.n_small != 0 && ctx->host_fast;
    auto stays_virtual = [&](const FwOp &op) { return small_virtual && ctx->segs[op.seg].small; };
    size_t n_virtual = 0;
    if (small_virtual)
        for (auto &L : levels)
            for (const FwOp &op : L.g) n_virtual += stays_virtual(op) ? 1u : 0u;
    fr.n_g -= n_virtual;
    const size_t off_nops = fr.n_g * sizeof(FwOp);
    const size_t bytes = off_nops + fr.n_n * sizeof(FwNestOp) + 16;
    if ((st = ensure_ring(ctx, fr, bytes))) return st;
    if ((st = acquire_slot(ctx, &fr.slot))) return st;
    char *hp = ctx->h_param[fr.slot];
    char *dp = ctx->d_param[fr.slot];  // staged copy here: the few workgroups of the small spawn / nest kernels would
                                       // wait for the bus on their critical path (measured: no gain from reading in place)
    struct Launch {
        bool nested;
        size_t first, count;
        uint32_t blocks;
    };
    std::vector<Launch> launches;
    FwOp *h_ops = (FwOp *)hp;
    FwNestOp *h_nops = (FwNestOp *)(hp + off_nops);
    size_t gi = 0, ni = 0, pend_first = 0;
    uint32_t pend_blocks = 0;
    auto flush_global = [&]() {
        if (gi > pend_first) launches.push_back(Launch{false, pend_first, gi - pend_first, pend_blocks});
        pend_first = gi;
        pend_blocks = 0;
    };
    for (auto &L : levels) {
        for (FwOp op : L.g) {
            if (stays_virtual(op)) continue;
            op.first_block = pend_blocks;
            pend_blocks += (op.n + FW_BLOCK - 1) / FW_BLOCK;
            h_ops[gi++] = op;
        }
        if (!L.n.empty()) {
            flush_global();
            const size_t first = ni;
            uint32_t tiles = 0;
            for (FwNestOp op : L.n) {
                op.first_tile = tiles;
                tiles += op.n_tiles;
                // (a range ring: the slot of its first YOUNG particle as of the last update -- this frame's cohorts join the
                // old part in launch_range, after these launches have been enqueued -- and the device subtracts the old part)
                const SegHost &PS = ctx->segs[op.parent_seg], &CS = ctx->segs[op.child_seg];
                op.parent_buf = PS.buf[p], op.parent_cap = PS.capacity;
                op.parent_head = PS.enqueue_head(), op.child_head = CS.enqueue_head();
                op.parent_range = PS.range ? 1u : 0u, op.child_range = CS.range ? 1u : 0u;
                op.parent_nospin = (PS.nospin ? 1u : 0u) | (PS.cpl_bits() << 1);  // (bit 1: Q1 / Q3 in component planes, bit 2: Q2 too, bit 3: Q0 too)
                memcpy(op.parent_rot, PS.const_rot, sizeof op.parent_rot);
                op.parent_life_plane = PS.life_plane(), op.parent_life_const = PS.fifo_life;  // (read under bit 0 of parent_nospin only)
                // (START tickets, fw_kernels.h: every workgroup of the op takes one)
                op.ticket_base = ctx->nest_ticket_base[op.emit_slot], ctx->nest_ticket_base[op.emit_slot] += op.n_tiles;
                h_nops[ni++] = op;
            }
            launches.push_back(Launch{true, first, ni - first, tiles});
        }
    }
    flush_global();
    // launches with at most FW_INLINE_OPS ops carry them in their kernel arguments; only longer lists (many
    // spawners with Nested entries) are staged through the copy stream
    bool staged = false;
    for (const Launch &L : launches) staged |= L.count > FW_INLINE_OPS;
    if (staged) {
        FW_HIP(ctx, hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
        FW_HIP(ctx, hipEventRecord(ctx->ev_copied[fr.slot], ctx->copy_stream));
        FW_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_copied[fr.slot], 0));
    }
    for (const Launch &L : launches) {
        const bool inl_ops = L.count <= FW_INLINE_OPS;
        if (!L.nested) {
            FW_HIP(ctx, fw_launch_spawn(ctx->stream, ctx->g, inl_ops ? nullptr : (const FwOp *)dp + L.first,
                                        h_ops + L.first, (uint32_t)L.count, L.blocks, p));
        } else {
            const uint32_t tag = next_nest_seq(ctx);
            FW_HIP(ctx, fw_launch_nested(ctx->stream, ctx->g,
                                         inl_ops ? nullptr : (const FwNestOp *)(dp + off_nops) + L.first,
                                         h_nops + L.first, (uint32_t)L.count, L.blocks, p, tag,
                                         ctx->spin_limit, ctx->dbg));
        }
    }
    if (!staged) fr.slot = -1;  // nothing in the ring slot is read by the device: no consumed-event needed
    if (!n_virtual) return FW_OK;
    // ---- the table of the small launch: {first op, one past the last, particles} per segment, then the ops
    const size_t off_ops = (size_t)n_seg * sizeof(OpHdr);
    bool others = false;  // small types' ops at an emission level other than the first
    for (size_t li = 1; li < levels.size(); li++)
        for (const FwOp &op : levels[li].g) others |= stays_virtual(op);
    OpList &g0 = levels[0].g;
    int tslot = -1;
    char *tp = nullptr;
    if (fr.pre_slot >= 0 && g0.lent && !others && fr.pre_hdr_ok && fr.pre_tracked == g0.size()) {
        // the list of the first level lives in the slot taken before the spawner loop, headers and all: the ops of the other
        // types next to the small ones' are simply not looked at (fw_k_update_small reads its segments' headers only)
        tslot = fr.pre_slot, tp = ctx->h_param[tslot];
    } else {
        OpList &ops = ctx->ops_scratch;
        ops.clear();
        ops.reserve_own(n_virtual);
        for (auto &L : levels)
            for (const FwOp &op : L.g)
                if (stays_virtual(op)) ops.push_back(op);
        sort_by_segment(ops.begin(), ops.end());
        const size_t tbytes = off_ops + ops.size() * sizeof(FwOp);
        if ((st = ensure_ring(ctx, fr, tbytes))) return st;
        if ((st = acquire_slot(ctx, &tslot))) return st;
        const bool bar = ctx->param_bar && tbytes <= kBarParamBytes;
        tp = bar ? ctx->b_param[tslot] : ctx->h_param[tslot];
        write_op_headers((OpHdr *)tp, n_seg, ops.data(), ops.size());
        memcpy(tp + off_ops, ops.data(), ops.size() * sizeof(FwOp));
        if (bar) drain_bar_writes(tp);
    }
    fr.small_hdr = (const uint4 *)tp, fr.small_ops = (const FwOp *)(tp + off_ops);
    fr.small_tslot = tslot;  // (read in place: recycled where the small launch is enqueued)
    return FW_OK;
}

// Global-only frame: spawn is fused into the update kernel (virtual particles).  Ops sorted by segment;
// the order inside a segment stays the emission order (rel_base was assigned in that order).
fw_status op_table(fw_ctx *ctx, FwFrame &fr) {
    auto &levels = ctx->levels;
    FwUpdateArgs &a = fr.a;
    const uint32_t n_seg = fr.n_seg;
    fw_status st = FW_OK;
    // (one emission level holds all of them most of the time: its list is used as it is)
    OpList *one = nullptr;
    size_t n_lists = 0;
    for (auto &L : levels)
        if (!L.g.empty()) one = &L.g, n_lists++;
    if (n_lists != 1) {
        one = &ctx->ops_scratch;
        one->clear();
        one->reserve_own(fr.n_g);
        for (auto &L : levels) one->append(L.g.begin(), L.g.end());
    }
    OpList &ops = *one;
    // the list lives in the parameter slot taken before the spawner loop (`pre_slot`), and so may its headers
    const bool in_place = fr.pre_slot >= 0 && one == &levels[0].g && ops.lent;
    const bool hdr_done = in_place && fr.pre_hdr_ok && fr.pre_tracked == ops.size();
    if (!hdr_done) sort_by_segment(ops.begin(), ops.end());
    a.n_ops = (uint32_t)ops.size();
    if (ops.size() <= FW_INLINE_OPS && (ops.empty() || !ctx->census.n_small)) {  // (small types read their ops from the table: fw_k_update_small)
        fr.spawn_form = ops.empty() ? FW_SPAWN_NONE : FW_SPAWN_INLINE;
        for (size_t i = 0; i < ops.size(); i++) fr.inl.ops[i] = ops[i];
        return FW_OK;
    }
    fr.spawn_form = FW_SPAWN_TABLE;
    const size_t off_ops = (size_t)n_seg * sizeof(OpHdr);
    const size_t bytes = off_ops + ops.size() * sizeof(FwOp);
    int slot = fr.pre_slot;  // (taken, waited for and large enough since before the spawner loop; the ops are where they belong)
    if (!in_place) {
        if ((st = ensure_ring(ctx, fr, bytes))) return st;
        if ((st = acquire_slot(ctx, &slot))) return st;
    }
    // (a small table goes to device memory the host writes through the large BAR: fw_ctx::b_param)
    const bool bar = !in_place && ctx->param_bar && bytes <= kBarParamBytes;
    char *hp = bar ? ctx->b_param[slot] : ctx->h_param[slot];
    if (!hdr_done) write_op_headers((OpHdr *)hp, n_seg, ops.data(), ops.size());
    if (!in_place) memcpy(hp + off_ops, ops.data(), ops.size() * sizeof(FwOp));
    if (bar) drain_bar_writes(hp);
    // pinned host memory is device-visible: the tiles read their few ops over the bus (tens of bytes each)
    a.seg_op_first = (const uint4 *)hp;
    a.ops = (const FwOp *)(hp + off_ops);
    ctx->slot_frame[slot] = ctx->frame + 1;  // free once done_tag >= frame + 1 (no consumed-event for this slot)
    fr.small_hdr = a.seg_op_first, fr.small_ops = a.ops;
    return FW_OK;
}

// the size of a cohort of Nested children, needed now (its age reaches the lifetime): the update of the cohort's frame left it in
// the ring's pinned report ring long ago; a report still missing after the stream has been waited for poisons the segment
template <class Cohort>
fw_status take_report(fw_ctx *ctx, uint32_t si, Cohort &c, const char *what) {
    const SegHost &S = ctx->segs[si];
    if (!wait_report(S, c.frame)) FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!report_landed(S, c.frame)) return poison_segment(ctx, si, what);
    c.n = (uint32_t)*(const volatile unsigned long long *)(S.h_report + (c.frame % kReportRing)), c.known = true;
    return FW_OK;
}

// the rings' latest launch ran L.depth frames.  The cohorts the withheld frames of a group spawned -- every frame of the launch but the last
// -- keep the pointer of their birth frame: the launch spun none of them, every frame of the group from their own on is in the log
// (fw_spin_newborn_deferred, fw_spin.h; every ring of a group defers and spawns for itself).  Under the eager rule alone (FW_NEWBORN_SPIN=1)
// the launch gave them every later frame's spin as well: their pointer is the last frame's cohort's (L.spin_from, per ring of the launch)
void group_launched(fw_ctx *ctx, const FwFifoLaunch &L) {
    const uint32_t n_withheld = L.depth - 1u;
    for (uint32_t j = 0; j < L.fa.n_segs; j++) {
        if (L.fa.s[j].seg >= ctx->segs.size()) continue;
        SegHost &S = ctx->segs[L.fa.s[j].seg];
        for (auto c = S.coh.rbegin(); ctx->newborn_spin && n_withheld && c != S.coh.rend() && c->frame >= L.frame[0]; ++c)
            for (uint32_t f = 0; f < n_withheld; f++)
                if (c->frame == L.frame[f]) c->spin_from = L.spin_from[j];
        S.fuse_last = L.depth >= 2u ? L.depth : 0u;
    }
}

// fw_debug_whole_tiles: the ring tiles of a launch that is about to go to the stream which the predicate calls whole -- the kernel's own
// predicate (fw_fifo_tile_whole over the tiles FwFifoSeg lays out, in the closed form fw_fifo_whole_span: no walk over the tiles, round 30)
// and its own conditions (fw_update_fifo_body).  The workgroups of a FUSED launch take the arm for exactly these tiles; an unfused launch's
// are counted too, and keep the streaming loop (the arm lost there)
void count_whole_tiles(fw_ctx *ctx, const FwFifoArgs &fa) {
    if (!fa.fuse_pad[FW_FIFO_WHOLE] || fa.dbg != 0u) return;
    uint64_t n = 0;
    for (uint32_t j = 0; j < fa.n_segs; j++) {
        const FwFifoSeg &F = fa.s[j];
        if (F.mat) continue;
        // (the arm of the fused forms asks for the age rule too -- every ring of a fused launch is under it: ring_rules)
        if (fa.fused >= 2u && !(F.type_idx & FW_TYPE_IDX_AGELESS)) continue;
        const uint32_t live_tiles = F.n_tiles - std::min(F.n_tiles, F.n_vt_a + F.n_vt_b);
        n += fw_fifo_whole_span(F.capacity, FW_TILE, F.head, F.n_in, F.dead, F.tile0, live_tiles).count;
    }
    ctx->whole_tiles += n, ctx->whole_launches += n ? 1u : 0u;
}
// fw_debug_newborn_spin: a launch that is about to go to the stream in which some ring's spawning workgroups defer the spin of what they
// spawn -- the kernel's own condition (fw_update_fifo_body: nb_defer), from the kernel's own arguments
void count_newborn(fw_ctx *ctx, const FwFifoArgs &fa) {
    bool any = false;
    for (uint32_t j = 0; j < fa.n_segs; j++) {
        const FwFifoSeg &F = fa.s[j];
        any |= fa.q0pl != 0u && fa.fuse_pad[FW_FIFO_NEWBORN] != 0u && (F.type_idx & FW_TYPE_IDX_NOSPIN) != 0u && (F.type_idx & FW_TYPE_IDX_AXIS) != 0u && F.mat == 0u;
    }
    ctx->newborn_launches += any ? 1u : 0u;
}

// A FIFO launch goes to the stream -- a frame's own, a group closed by its last frame, the group somebody who reads asked for: everything
// that happens then.  fw_debug_fuse2: launches that ran two or more frames / withheld frames that went alone
fw_status enqueue_fifo(fw_ctx *ctx, const FwFifoLaunch &L, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    const bool fused = L.depth >= 2u;
    group_launched(ctx, L);
    if (fused) ctx->fused_launches++, ctx->fuse_frames += L.depth;
    else if (L.held) ctx->fuse2_flushed++;
    count_whole_tiles(ctx, L.fa), count_newborn(ctx, L.fa);
    FW_HIP(ctx, fw_launch_update_fifo(stream, ctx->g, L.fa, L.fio, L.tiles, L.nt, e0, e1, fused ? &L.rec : nullptr));  // (every depth: routed there)
    return FW_OK;
}

}  // namespace

namespace fwh {

// (a group only ever waits behind quiet frames, whose launches go to the main stream: launch_fifo)
fw_status flush_withheld(fw_ctx *ctx) {
    const FwFifoLaunch *L = ctx->withheld.take();
    return L ? enqueue_fifo(ctx, *L, ctx->stream, nullptr, nullptr) : FW_OK;
}

void drop_withheld(fw_ctx *ctx) { ctx->withheld.drop(); }

}  // namespace fwh

namespace {

// ---- FIFO segments: in place, everything they need in the kernel arguments (fw_kernels.h: FwFifoSeg)

// what the ring launches of one frame share: their stream and their tile grid
struct FifoFrame {
    hipStream_t stream;
    // (with a colliding ring in the context every FIFO launch of it runs the COLL instantiation, whose workgroups cover one
    // round -- FW_FIFO_COLL_TILE slots -- each: the tile grid of all of them follows)
    // ... and so do the launches of a context whose rings hold too few particles to fill the chip with four-round workgroups
    // (the reference's own stress_test: 157k particles = 154 of them on 256 CUs, each lane working through four particles one
    // after the other): below FW_FIFO_SMALL four-round tiles in all, one round per workgroup.  Not with a ring whose count
    // only the device knows (its grid covers its capacity: four times the idle workgroups).
    // (counted in the first pass over the segments of this frame; a ring that changed its kind since then: next frame)
    bool small, coll_real;
    bool coll;  // (the same tile grid; which instantiation runs: FwFifoArgs::any_coll / small_tiles)
};

// the launch being accumulated, ring by ring: its arguments built in place, and what every ring of it so far has in common
struct FifoAccum {
    FwFifoLaunch L;        // fa, fio, tiles, n_ops; spin_from: what a cohort this frame spawns carries as its spin pointer, per ring
    uint64_t bytes = 0;    // what the launch streams, roughly: its tiles x the bytes a particle of the type moves
    bool nospin = true;    // every ring of the launch so far carries FW_TYPE_IDX_NOSPIN in it (FwFifoArgs::spinless)
    bool derived = true;   // ... and is of a FW_TYPE_DERIVED type (FwFifoArgs::fuse_pad[FW_FIFO_WHOLE])
    uint32_t rung = FW_RUNG_FAR;  // several frames in one launch: the lowest rung of the depth ladder any ring so far stands on (fw_fuse_rung,
                           // fw_fuse2.h; FW_RUNG_NONE: a ring that did not defer its spin in the launch, or holds fewer than fuse2_min particles)
    uint32_t n_launches = 0;  // the launches of this frame so far
    bool sent = false;     // the launch has been offered: a ring that follows starts the frame's next one (most frames have one: cleared for nobody)

    void restart() {
        const uint32_t n = n_launches;
        *this = FifoAccum{};
        n_launches = n;
    }
    // the launch-wide words, once every ring is in: FwFifoArgs::spinless and fuse_pad, L.nt; may the launch wait or take the waiting ones
    // in, and how deep a group it may close or continue
    struct Words {
        bool candidate;
        uint32_t depth_max;
    };
    Words derive(const fw_ctx *ctx, bool quiet) {
        FwFifoArgs &fa = L.fa;
        // (no ring tile of the launch touches rotation or angular velocity: the kernel form compiled for that -- rings with Q0 in planes,
        // four-round tiles, no instance records)
        fa.spinless = (ctx->use_spinless && nospin && fa.q0pl && !fa.any_inst && !fa.small_tiles) ? 1u : 0u;
        // (... and its whole ring tiles owe nothing but position, age and velocity: the arm without a divergent lane, fw_fifo_tile_whole)
        fa.fuse_pad[FW_FIFO_WHOLE] = (ctx->use_whole_tiles && fa.spinless && derived && fa.write_mask == 0) ? 1u : 0u;
        // (... and whose spawning workgroups leave the spin of what they spawn into a deferring ring to its log: fw_spin_newborn_deferred)
        // (one rule for the whole context: a fused launch, every ring of which defers under it, takes the set of kernels the word names)
        fa.fuse_pad[FW_FIFO_NEWBORN] = ctx->newborn_spin ? 0u : 1u;        L.nt = bytes > ctx->nt_bytes ? 2 : bytes > ctx->nt_wo_bytes ? 1 : 0;
        // the frame's one launch, spin-less, every ring unread and large: it may wait for the next frame, or take the waiting one in
        const bool candidate = fw_fuse2_candidate(ctx->use_fuse2, quiet, n_launches == 0 && fa.n_segs == ctx->census.n_fifo, fa.spinless != 0u, rung >= FW_RUNG_TWO);
        // (how deep: the launch's rung of the ladder, the knobs, and for the far tier the forms that defer their newborns' spin.  A depth_max
        // above FW_FUSE_MAX is also what lets the group merge its ops: FwWithheld::offer)
        return Words{candidate, fw_fuse_depth_max(rung, ctx->fuse_depth, ctx->fuse_far_depth, fa.fuse_pad[FW_FIFO_NEWBORN] != 0u)};
    }
};

// what a ring brings into this frame's launch
struct RingInput {
    bool mat_frame;    // frames that materialise (Nested pass): the segment's Global particles of this frame already sit in the ring
    bool mat;
    uint32_t n_spawn;  // spawned by fw_k_update_fifo itself
    uint32_t n_in;     // live particles before fw_k_update_fifo's own spawns (a type that receives children: only the device knows)
};
RingInput ring_input(const SegHost &S, const FwFrame &fr) {
    RingInput in;
    in.mat_frame = S.fifo_mat && fr.nested_frame && !S.virt_parent;
    in.mat = S.fifo_dev || in.mat_frame;
    in.n_spawn = in.mat_frame ? 0u : S.frame_spawn;
    in.n_in = S.fifo_dev ? 0xFFFFFFFFu : S.ub - in.n_spawn;
    return in;
}

// the Nested entries of this frame that run inside the FIFO launch (FwFrame::fuse_plan) and emit from the ring / into it, or -1
struct NestRole {
    int parent = -1, child = -1;
    bool any() const { return parent >= 0 || child >= 0; }
};
NestRole nest_role(const FwFrame &fr, uint32_t si) {
    NestRole r;
    for (uint32_t k = 0; fr.fuse && k < fr.n_fuse; k++) {
        if (fr.fuse_plan[k].parent_seg == si) r.parent = (int)k;
        if (fr.fuse_plan[k].child_seg == si) r.child = (int)k;
    }
    return r;
}

// the rules that hold for a ring in this launch; the planes of a ring that leaves a rule are made true first (ensure_ages, ensure_spin)
struct RingRules {
    bool ageless, spin_defer, newborn_defer;
    uint64_t spin_from_new;  // what a cohort this frame spawns carries as its spin pointer
};
fw_status ring_rules(fw_ctx *ctx, uint32_t si, float dt, const FifoFrame &ff, const RingInput &in, bool nest_touches, RingRules &R) {
    SegHost &S = ctx->segs[si];
    fw_status st = FW_OK;
    // the age rule (fw_device.h: FW_TYPE_IDX_AGELESS), per launch: a streaming launch -- four-round tiles, no collider, no instance
    // records of this ring --, a ring fed by Global entries alone that no Nested entry touches, a FW_TYPE_DERIVED type that reports
    // no destroyed particles, a dt both sides add alike.  Any other launch finds the true ages in the plane: written back first,
    // from the cohorts as they stand BEFORE this frame's spawns and dt (what the ring holds).
    // ("streaming" is judged by the context's own threshold, fw_ctx::fifo_small_tiles: with FW_FIFO_SMALL=0 -- no threshold, four-round
    // tiles at any size -- nothing says the launch is bound by bandwidth, and the rule stays off)
    R.ageless = ctx->use_ageless && S.q0pl && ctx->fifo_small_tiles != 0u && !ff.small && !ff.coll_real && S.inst == nullptr && !S.collides && !S.fifo_dev && !S.fifo_mat &&
                !S.nested_fed && S.n_lplanes == 0 && !nest_touches && S.derived && S.destroyed == nullptr && ageless_dt_ok(dt);
    if (!R.ageless && (st = ensure_ages(ctx, si, ff.stream))) return st;
    if (R.ageless) S.ages_stale = true;
    S.ageless_last = R.ageless;
    // the deferred spin (fw_device.h: FW_TYPE_IDX_NOSPIN with FW_TYPE_IDX_AXIS; fw_spin.h), per launch: everything the age rule asks,
    // the axis rule in force for this dt (its proof makes the replay independent of who shares a wave), a positive normal dt (no
    // cohort then takes a later frame's spawn in: its age is above +0), a ring large enough to be bound by bandwidth -- and one
    // that has met all of this for spin_defer_after launches in a row without anybody asking for its planes.  Any other launch
    // finds the true spin in the planes: replayed first, under the axis the log was written for (before S.axis is cleared).
    const bool spin_ok = R.ageless && ctx->use_spin_defer && S.axis != 0u && axis_dt_ok(S, dt) && spin_dt_ok(dt) && in.n_in >= ctx->spin_defer_min &&
                         !(S.frame_spawn && !S.coh.empty() && S.coh.back().age == 0.0f);
    R.spin_defer = spin_ok && S.spin_streak >= ctx->spin_defer_after;
    if (!spin_ok) {
        if ((st = ensure_spin(ctx, si, ff.stream))) return st;
    } else if (!R.spin_defer) {
        S.spin_streak++;
    } else if (fw_spin_full(S.spin.log.size(), std::max(1u, ctx->spin_log_cap)) && (st = ensure_spin(ctx, si, ff.stream, true))) {
        return st;  // (the log at its cap: replayed, and the ring goes on deferring)
    }
    // (what this frame spawns into a deferring ring defers its spin too, its cohort points at the frame's own log entry: unless
    // somebody else writes the ring's new particles, or the eager rule is asked for -- fw_spin_newborn_deferred, which the kernel's
    // flag follows as well: FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN] with the ring's type_idx and FwFifoSeg::mat, ring_record)
    R.newborn_defer = fw_spin_newborn_deferred(R.spin_defer, !in.mat, ctx->newborn_spin);
    R.spin_from_new = R.spin_defer ? S.spin.defer_spawn(S.coh, dt, R.newborn_defer) : S.spin.end();
    S.spin_last = R.spin_defer;
    return FW_OK;
}

// the cohorts age by this dt exactly as their particles do (fp32 additions, fw_survives); the oldest die first.  *dead: how many
fw_status age_cohorts(fw_ctx *ctx, uint32_t si, float dt, uint64_t spin_from_new, uint32_t *dead) {
    SegHost &S = ctx->segs[si];
    fw_status st = FW_OK;
    if (S.fifo_dev) {
        S.coh.push_back(SegHost::Cohort{0u, 0.0f, ctx->frame, false});  // size: whatever the device appends
    } else if (S.frame_spawn) {
        if (!S.coh.empty() && S.coh.back().age == 0.0f && !std::signbit(S.coh.back().age))
            S.coh.back().n += S.frame_spawn;
        else
            S.coh.push_back(SegHost::Cohort{S.frame_spawn, 0.0f, ctx->frame, true, spin_from_new});
    }
    for (auto &c : S.coh) c.age = c.age + dt;
    *dead = 0;
    while (!S.coh.empty() && S.coh.front().age >= S.fifo_life) {
        SegHost::Cohort &c = S.coh.front();
        // (children added `lifetime` ago)
        if (!c.known && c.frame != ctx->frame && (st = take_report(ctx, si, c, "cohort report missing"))) return st;
        *dead += c.n;
        S.coh.pop_front();
    }
    if (S.spin.stale) S.spin.trim(S.coh);  // (log entries only dead particles lacked: a particle that dies unread never has the work done)
    return FW_OK;
}

// the ring's record in the launch -- FwFifoSeg, its ops and its workgroups --, what the ring adds to the launch-wide facts, and the ring's
// head and bound behind the frame
void ring_record(fw_ctx *ctx, const FifoFrame &ff, FifoAccum &acc, uint32_t si, float dt, const RingInput &in, const RingRules &R, uint32_t dead,
                 bool nest_parent) {
    SegHost &S = ctx->segs[si];
    FwFifoArgs &fa = acc.L.fa;
    const int32_t wm = S.derived ? 0 : S.fifo_wm;  // (FW_TYPE_DERIVED: none of the optional planes is stored)
    if (!fa.n_segs) fa.write_mask = wm;
    else if (fa.write_mask != wm) fa.write_mask = -1;
    // (a fused launch's kernels hold the rule as a fact of their code: a ring that defers its spin and not its newborns' -- none exists
    // today, `mat` is false wherever spin_ok holds -- would not be fused)
    const bool defers = R.spin_defer && (R.newborn_defer || ctx->newborn_spin);
    acc.rung = std::min(acc.rung, defers ? fw_fuse_rung(in.n_in, ctx->fuse2_min, ctx->fuse_deep_min, ctx->fuse_wide_min, ctx->fuse_far_min) : (uint32_t)FW_RUNG_NONE);
    acc.L.spin_from[fa.n_segs] = R.spin_from_new;
    // (acceleration and drag of the ring's type, for the whole tiles of a fused launch this frame may close: FwFuseArgs::move)
    memcpy(acc.L.rec.fz.move[fa.n_segs], S.fifo_move, sizeof S.fifo_move);
    FwFifoSeg &F = fa.s[fa.n_segs++];
    F.buf = S.buf[0], F.destroyed = S.destroyed, F.inst = S.inst;
    F.inst_cap = S.inst_cap, F.capacity = S.capacity, F.seg = si;
    // (the axis-spin rule travels per launch: a frame whose dt voids its proof runs without it, and so does every frame after it)
    if (S.axis != 0u && !axis_dt_ok(S, dt)) S.axis = 0u;
    F.type_idx = S.type_idx | ((S.nospin || R.spin_defer) ? FW_TYPE_IDX_NOSPIN : 0u) | (S.axis << FW_TYPE_IDX_AXIS_SHIFT) | (R.ageless ? FW_TYPE_IDX_AGELESS : 0u), F.life = S.fifo_life;
    F.keys_off = S.keys_off, F.keys_len = S.keys_len;
    F.head = S.head, F.n_in = in.n_in, F.n_spawn = in.n_spawn, F.dead = dead;
    F.mat = in.mat ? 1u : 0u;
    fa.q0pl = S.q0pl ? 1u : 0u;  // (the same for every ring of a launch: the two passes)
    acc.nospin &= (F.type_idx & FW_TYPE_IDX_NOSPIN) != 0u;
    acc.derived &= S.derived;
    F.n_lplanes = S.n_lplanes;
    F.report = S.fifo_dev ? S.h_report + (ctx->frame % kReportRing) : nullptr;
    F.op0 = acc.L.n_ops;
    if (!in.mat_frame)
        for (const FwOp &op : ctx->fifo_ops)
            if (op.seg == si) acc.L.fio.ops[acc.L.n_ops++] = op;
    F.op1 = acc.L.n_ops;
    // workgroups: the new particles first, FW_BLOCK each, in two groups of consecutive slots (up to the end of the
    // buffer / from slot 0); then the ring tiles from the first slot the update touches (the first destroyed particle
    // when their records are wanted, the first survivor otherwise) to the last old particle (a type whose count
    // only the device knows: the whole ring, empty tiles leave at once); at least one in all (it publishes the counts)
    const uint32_t n_old = S.fifo_dev ? S.capacity : in.n_in;
    // (... or a ring whose particles a Nested entry of this launch emits from: the ones about to die still emit, and the
    // tiles' ranks count from the ring's head)
    const uint32_t lo = std::min((S.destroyed || nest_parent) ? 0u : dead, n_old);
    const uint32_t ftile = ff.coll ? FW_FIFO_COLL_TILE : FW_TILE;
    const FwFifoLayout L = fw_fifo_layout(S.capacity, ftile, FW_BLOCK, S.head, lo, n_old, S.fifo_dev ? 0u : in.n_in, in.n_spawn);  // (fw_fuse2.h)
    F.spawn_a = L.spawn_a, F.n_vt_a = L.n_vt_a, F.n_vt_b = L.n_vt_b, F.tile0 = L.tile0, F.n_tiles = L.n_tiles;
    F.tile_first = acc.L.tiles;
    acc.L.tiles += F.n_tiles;
    F.nest = 0u;
    // (the estimate fw_ctx::nt_bytes / nt_wo_bytes were calibrated against in round 3 -- 104 / 164 B whatever the launch moves, two to
    // seven times the truth by now: the thresholds and it go together, and a fused launch takes the form its last frame would have)
    acc.bytes += (uint64_t)L.live_tiles * ftile * (S.nospin ? 104u : 164u);
    fa.any_inst |= S.inst != nullptr ? 1u : 0u;
    // (a launch of q0pl rings -- none of them collides -- in a context with a colliding ring: the plain one-round form on the same tile grid)
    fa.any_coll |= (ff.coll_real && !S.q0pl) ? 1u : 0u;
    fa.small_tiles = (ff.coll && !(ff.coll_real && !S.q0pl)) ? 1u : 0u;
    S.head = (uint32_t)(((uint64_t)S.head + dead) % S.capacity);
    if (!S.fifo_dev) S.ub = in.n_in + in.n_spawn - std::min(dead, in.n_in + in.n_spawn);  // exact
}

// the latest ring of the launch is the parents' or the children's ring of a Nested entry that runs inside it (FwFifoNest).
// *status_next: look-back words handed to the Nested entries of this frame so far (FwFifoNest::status_first)
void wire_nest(fw_ctx *ctx, const FwFrame &fr, FwFifoArgs &fa, const NestRole &nest, uint32_t nest_tag, uint32_t *status_next) {
    FwFifoSeg &F = fa.s[fa.n_segs - 1u];
    if (nest.parent >= 0) {
        const FwNestOp &op = fr.fuse_plan[nest.parent];
        FwFifoNest &N = fa.nest[nest.parent];
        F.nest = (uint32_t)nest.parent + 1u;
        N.parent = fa.n_segs - 1u;
        N.emit = op.emit, N.emit_slot = op.emit_slot, N.parent_lplane = op.parent_lplane;
        N.n_count = op.n_count, N.n_start = op.n_start, N.n_end = op.n_end, N.speed = op.speed, N.scale = op.scale;
        N.status_first = *status_next, N.n_ptiles = F.n_tiles - (F.n_vt_a + F.n_vt_b);
        *status_next += N.n_ptiles;
        N.ticket_base = ctx->nest_ticket_base[op.emit_slot], ctx->nest_ticket_base[op.emit_slot] += N.n_ptiles;
        N.tag = nest_tag, N.spin_limit = ctx->spin_limit;
        fa.n_nest = fr.n_fuse;
    }
    if (nest.child >= 0) {
        F.nest = ((uint32_t)nest.child + 1u) | FW_FIFO_NEST_CHILD;
        fa.nest[nest.child].child = fa.n_segs - 1u;
    }
}

fw_status launch_fifo(fw_ctx *ctx, FwFrame &fr) {
    const FwUpdateArgs &a = fr.a;
    const float dt = fr.dt;
    const uint32_t n_seg = fr.n_seg;
    // the ring launch(es) of this frame: on the side stream when a general launch runs next to them (fw_ctx: fifo_stream)
    // (never on a caller-supplied stream: work the caller orders behind fw_step on ITS stream must cover the whole
    // frame, as it did before the side stream existed)
    // (the wave-per-type launch of small types counts as "a general launch" here: it touches none of the rings either)
    bool side = ctx->use_fifo_stream && ctx->stream.owned() && (fr.total_tiles != 0 || ctx->census.n_small != 0) && ctx->live_ring == nullptr;
    // (... nor with a colliding ring: a new collider set travels in the MAIN stream, fw_ctx_set_colliders)
    for (const SegHost &S : ctx->segs) side &= !(S.in_use && S.fifo && (S.fifo_mat || S.inst != nullptr || S.collides));
    fw_status st = order_side(ctx, side, ctx->fifo_last_side);
    if (st) return st;
    // (a frame whose only GPU work is this one launch: no compacting, range or small segment, no separate pass, no colour fill, nobody
    // who wants a count or a time per frame)
    const bool quiet = fr.quiet && fr.spawn_form == FW_SPAWN_NONE && !side;
    if (!quiet && (st = flush_withheld(ctx))) return st;
    // (a group is only ever pending in a quiet frame, and a quiet frame is never `side`: a group an offer of this frame sends out goes
    // to the main stream through ff.stream, as flush_withheld's does)
    FifoFrame ff;
    ff.stream = side ? ctx->fifo_stream : ctx->stream;
    ff.small = !fr.ring_stats.fifo_dev && fr.ring_stats.fifo_parts < (uint64_t)ctx->fifo_small_tiles * FW_TILE;
    ff.coll_real = fr.ring_stats.fifo_coll;
    ff.coll = ff.coll_real || ff.small;
    FifoAccum acc{};
    FwFifoArgs &fa = acc.L.fa;
    uint32_t nest_status_next = 0;
    const uint32_t nest_tag = fr.fuse ? next_nest_seq(ctx) : 0u;
    // the accumulated launch is complete: offered to the withheld group, and what the offer leaves goes to the stream
    auto flush = [&]() -> fw_status {
        if (acc.sent || !fa.n_segs) return FW_OK;
        fa.parity = fr.p, fa.epoch = a.epoch, fa.dbg = ctx->dbg, fa.dt = dt;
        // (the pinned "frame F has started" word recycles host buffers the GENERAL launch reads: when the two launches
        // run on different streams only that one reports)
        fa.done_tag = side ? nullptr : a.done_tag, fa.done_value = a.done_value;
        fa.host_counts = a.host_counts;
        fa.live_out = a.live_out, fa.live_next = a.live_next;
        const FifoAccum::Words w = acc.derive(ctx, quiet);
        acc.n_launches++;
        fr.fifo_launched = true;
        fw_status fst = FW_OK;
        const FwOffered o = ctx->withheld.offer(acc.L, w.candidate, w.depth_max, ctx->frame);
        if (o.first && (fst = enqueue_fifo(ctx, *o.first, ff.stream, nullptr, nullptr))) {
            ctx->withheld.drop();  // (the frame went neither to the stream nor into a group)
            return fst;
        }
        ctx->spinless_launches += fa.spinless;  // (a candidate is spin-less: a withheld frame counts when it is withheld)
        // (a withheld frame arms no snapshot row and reports no counts: FwWithheld::keep)
        if (o.withheld) fr.snap = -1, fr.a.host_counts = nullptr;
        if (o.second) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (o.second->depth == 1u) next_timing_pair(ctx, fr, &e0, &e1);
            if ((fst = enqueue_fifo(ctx, *o.second, ff.stream, e0, e1))) return fst;
        }
        if (side) ctx->side_dirty = true;
        acc.sent = true;
        return FW_OK;
    };
    // (two passes: the rings that keep Q0 in planes -- SegHost::q0pl, the ones that may run under the age rule -- get a launch of their own,
    // behind everybody else's: the colliding and the Nested instantiations of the kernel never meet that layout)
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t si = 0; si < n_seg; si++) {
            const SegHost &S = ctx->segs[si];
            if (!S.in_use || !S.fifo || S.q0pl != (pass == 1)) continue;
            uint32_t k_ops = 0;
            for (const FwOp &op : ctx->fifo_ops) k_ops += op.seg == si ? 1u : 0u;
            if (k_ops > FW_INLINE_OPS)  // (build_spawner never makes such a type a ring)
                return poison_segment(ctx, si, "a FIFO ring with more spawn ops than its launch can carry");
            if ((fa.n_segs == FW_FIFO_PER_LAUNCH || acc.L.n_ops + k_ops > FW_INLINE_OPS) && (st = flush())) return st;
            if (acc.sent) acc.restart();
            const RingInput in = ring_input(S, fr);
            const NestRole nest = nest_role(fr, si);
            RingRules rules;
            uint32_t dead = 0;
            if ((st = ring_rules(ctx, si, dt, ff, in, nest.any(), rules))) return st;
            if ((st = age_cohorts(ctx, si, dt, rules.spin_from_new, &dead))) return st;
            ring_record(ctx, ff, acc, si, dt, in, rules, dead, nest.parent >= 0);
            wire_nest(ctx, fr, fa, nest, nest_tag, &nest_status_next);
        }
        if ((st = flush())) return st;
    }
    return FW_OK;
}

// Every provisioned workgroup of the range launch is dispatched every frame, active or not (~3 us of a slot each): small needs get
// one spare, large ones an eighth -- a re-sent table is a copy in the stream, an idle workgroup a cost in every frame.
// (the bound of the old part follows the snapshots in a sawtooth: a role grows at once, and shrinks only after its
// need has stayed far below what is provided for 64 frames in a row -- otherwise the table would be re-sent on
// every tooth)  true: `have` changed, the table must be re-sent
inline bool fit(uint32_t &have, uint32_t need, uint32_t spare, uint32_t &low) {
    if (need > have) {
        have = need + spare, low = 0;
        return true;
    }
    if (have > need + need / 4 + spare + 2) {
        if (++low > 64) {
            have = need + spare, low = 0;
            return true;
        }
    } else {
        low = 0;
    }
    return false;
}

// ---- range rings: in place, one launch for all of them (fw_kernels.h: FwRangeRec)
fw_status launch_range(fw_ctx *ctx, FwFrame &fr) {
    const FwUpdateArgs &a = fr.a;
    const float dt = fr.dt;
    const uint32_t n_seg = fr.n_seg;
    const int rslot = (int)(ctx->rring_seq++ % kParamRing);
    fw_status st = wait_slot_free(ctx, ctx->rslot_frame[rslot]);  // (the kernel reads the slot in place)
    if (st) return st;
    FwRangeRec *recs = (FwRangeRec *)ctx->h_rparam[rslot].get();
    FwOp *rops = (FwOp *)(ctx->h_rparam[rslot] + round_up((uint32_t)(ctx->max_seg * sizeof(FwRangeRec)), 64));
    std::vector<FwOp> &ops = ctx->range_ops;
    sort_by_segment(ops.data(), ops.data() + ops.size());
    if (!ops.empty()) memcpy(rops, ops.data(), ops.size() * sizeof(FwOp));
    bool dirty = ctx->r_force, all_nospin = true, range_inst = false, range_coll = false;
    {  // the tile size of this launch (fw_ctx::range_small)
        const uint64_t parts = fr.ring_stats.range_parts;
        const bool any_dev = fr.ring_stats.range_dev, any_coll_r = fr.ring_stats.range_coll;
        const uint64_t lim = (uint64_t)ctx->range_small_tiles * FW_TILE;
        const bool small = any_coll_r || (!any_dev && parts < (ctx->range_small ? lim + lim / 4 : lim));
        if (small != ctx->range_small) ctx->range_small = small, dirty = true;
        // ... and of its YOUNG workgroups (fw_ctx::range_young_rounds)
        const uint64_t mean = parts / std::max<uint32_t>(1u, ctx->census.n_range), big = ctx->range_young_big;
        uint32_t yr = ctx->range_young_rounds;
        if (small || any_dev || fr.ring_stats.range_inst || big == 0) yr = 4;
        else if (yr == 4 && mean >= big) yr = 2;
        else if (yr == 2 && mean < big - big / 4) yr = 4;
        if (yr != ctx->range_young_rounds) ctx->range_young_rounds = yr, dirty = true;
    }
    const uint32_t OT = ctx->range_small ? (uint32_t)FW_BLOCK : (uint32_t)FW_TILE;  // slots an OLD workgroup covers
    uint64_t r_bytes = 0;  // what the launch streams, roughly (the non-temporal form of the kernel: fw_ctx::nt_bytes)
    size_t oi = 0;
    for (uint32_t si = 0; si < n_seg; si++) {
        SegHost &S = ctx->segs[si];
        if (!S.in_use || !S.range) continue;
        all_nospin &= S.nospin;
        range_inst |= S.inst != nullptr;
        range_coll |= S.collides;
        r_bytes += (uint64_t)(S.range_dev ? S.capacity / 2 : S.ub) * (S.nospin ? 104u : 164u);
        S.dead_at_end = true;
        // cohorts that are no longer provably too young to die join the old part: the boundary moves, nothing is copied
        const bool mat_frame = S.range_mat && fr.nested_frame && !S.virt_parent;  // its Global particles of this frame already sit in the ring
        uint32_t grad = 0;
        if (!S.range_dev) {
            while (!S.ycoh.empty()) {
                const float an = birth_age_before(ctx, S.ycoh.front().frame) + dt;  // the device's own addition (core.rs:594)
                if (an < S.range_life_lo) break;
                grad += S.ycoh.front().n;
                S.ycoh.pop_front();
            }
            if (S.frame_spawn) S.ycoh.push_back(SegHost::YCohort{ctx->frame, S.frame_spawn});
        } else {
            // a type that receives Nested children: a cohort's size is whatever the device appended in its frame; the update
            // of that frame left it in the pinned ring, and it is only needed now, a lifetime.min later
            while (!S.dcoh.empty()) {
                SegHost::DCohort &c = S.dcoh.front();
                const float an = birth_age_before(ctx, c.frame) + dt;
                if (an < S.range_life_lo) break;
                if (!c.known && (st = take_report(ctx, si, c, "cohort report missing (range ring)"))) return st;
                grad += c.n;
                if (c.n) S.gcoh.push_back(SegHost::YCohort{c.frame, c.n}), S.gcoh_sum += c.n;
                S.dcoh.pop_front();
            }
            S.dcoh.push_back(SegHost::DCohort{ctx->frame, 0u, false});
            // graduated cohorts whose every particle an EARLIER update has destroyed (age >= lifetime.max before this frame)
            while (!S.gcoh.empty() && !(birth_age_before(ctx, S.gcoh.front().frame) < (float)S.life_bound)) {
                S.gcoh_sum -= S.gcoh.front().n;
                S.gcoh.pop_front();
            }
        }
        {  // (young_lo + grad) mod capacity without a 64-bit division: both terms are below the capacity
            uint64_t nb = (uint64_t)S.young_lo + grad;
            while (nb >= S.capacity) nb -= S.capacity;
            S.young_lo = (uint32_t)nb;
        }
        const uint32_t y_exist = S.range_dev ? 0u : S.young_n - std::min(S.young_n, grad);
        FwRangeRec Rc{};  // (built here, stored once below: the slot is written, never read, by the host)
        Rc.b = S.young_lo, Rc.y_exist = y_exist, Rc.n_spawn = (mat_frame || S.range_dev) ? 0u : S.frame_spawn;
        Rc.grad = grad, Rc.flags = (mat_frame ? FW_RREC_MAT : 0u) | (S.range_dev ? (FW_RREC_MAT | FW_RREC_DEV) : 0u);
        Rc.report = S.range_dev ? S.h_report + (ctx->frame % kReportRing) : nullptr, Rc.pad2 = 0;
        while (oi < ops.size() && ops[oi].seg < si) oi++;
        Rc.op0 = (uint32_t)oi, Rc.op_n = 0;
        while (oi < ops.size() && ops[oi].seg == si) oi++, Rc.op_n++;
        S.young_n = S.range_dev ? 0u : y_exist + S.frame_spawn;
        // workgroups of each role (bands: the table is re-sent only when a need leaves its band)
        const uint32_t YT = ctx->range_small ? (uint32_t)FW_BLOCK : ctx->range_young_rounds * (uint32_t)FW_BLOCK;
        const uint32_t ysh = (uint32_t)__builtin_ctz(YT), osh = (uint32_t)__builtin_ctz(OT);  // (powers of two: shifts, not divisions, per segment)
        uint32_t need_old, need_new, need_young;
        if (S.range_dev) {
            // the old part: at most the cohorts that have joined it and may still hold survivors (all sizes known); the young
            // part: somewhere behind b -- the grid covers the ring, a tile without young particles leaves at once
            need_old = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>((S.gcoh_sum + OT - 1) >> osh, (S.capacity >> osh) + 1));
            need_new = 0u;
            need_young = S.capacity >> ysh;
        } else {
            const uint32_t live_before_ub = std::min(S.ub - std::min(S.ub, S.frame_spawn), S.capacity);
            const uint32_t old_ub = live_before_ub - std::min(live_before_ub, y_exist);
            need_old = std::max(1u, (old_ub + OT - 1) >> osh);
            need_new = mat_frame ? 0u : (S.frame_spawn + FW_BLOCK - 1) / FW_BLOCK;
            need_young = std::min(S.capacity >> ysh, ((S.young_lo & (YT - 1u)) + y_exist + (mat_frame ? S.frame_spawn : 0u) + YT - 1) >> ysh);
        }
        S.r_need[0] = need_old, S.r_need[1] = need_new, S.r_need[2] = need_young;
        if (S.range_dev) {
            // the grid covers the ring, but how far behind b the young part reaches is roughly known: the count of the latest
            // snapshot row (+ a fifth, + what a few frames add).  Tiles beyond that are "probably idle" and go to the end of
            // the table, where they run while the launch drains (a tile that does hold particles simply updates them
            // there); the split follows the count in steps of an eighth
            const uint64_t est = (uint64_t)((double)S.dev_count * 1.2 + 8.0 * (double)S.dev_rate) + 2 * YT;
            const uint32_t likely = (uint32_t)std::min<uint64_t>(need_young, (est + YT - 1) >> ysh);
            if (likely > S.r_young_main || likely + likely / 4 + 8 < S.r_young_main) S.r_young_main = std::min(need_young, likely + likely / 8 + 2), dirty = true;
            S.r_need[2] = S.r_young_main;
        }
        dirty |= fit(S.r_old, need_old, need_old >= 8 ? need_old / 4 : 1u, S.r_low[0]);
        dirty |= fit(S.r_new, need_new, need_new ? (need_new >= 8 ? need_new / 8 : 1u) : 0u, S.r_low[1]);
        dirty |= fit(S.r_young, need_young, need_young >= 16 ? need_young / 8 : 1u, S.r_low[2]);
        S.r_young = std::min(S.r_young, S.capacity >> ysh);
        // (START tickets, fw_kernels.h: every OLD workgroup the table provides for the segment takes one per launch -- r_old of
        // them, whether the table is re-sent this frame or not: fit() changes the number only together with `dirty`)
        Rc.ticket_base = S.ticket_base, S.ticket_base += S.r_old;
        recs[si] = Rc;
    }
    if (dirty && (st = upload_range_table(ctx, n_seg))) return st;
    // the ages every later frame starts from
    for (auto &e : ctx->birth_age) e.age = e.age + dt;
    ctx->birth_age.push_back(fw_ctx::BirthAge{ctx->frame, 0.0f + dt});
    // (kept while some ring may still ask for the age: until lifetime.min for every ring, until lifetime.max for those that
    // bound their old part by the cohorts in it -- range_age_keep)
    while (!ctx->birth_age.empty() && !(ctx->birth_age.front().age < std::max(ctx->range_life_max, ctx->range_age_keep))) ctx->birth_age.pop_front();
    if (!ctx->r_total) return FW_OK;
    // (the records went through write-combining stores into device memory)
    if (ctx->param_bar) drain_bar_writes(recs);
    FwRangeArgs ra{};
    ra.desc = ctx->d_rdesc, ra.recs = recs, ra.ops = rops, ra.status = ctx->d_rstatus;
    ra.total_tiles = ctx->r_total, ra.parity = fr.p, ra.epoch = a.epoch, ra.spin_limit = ctx->spin_limit, ra.dbg = ctx->dbg;
    ra.dt = dt;
    ra.any_inst = range_inst ? 1u : 0u;
    ra.any_coll = range_coll ? 1u : 0u;
    ra.small_tiles = ctx->range_small ? 1u : 0u;
    ra.young_rounds = ctx->range_young_rounds;
    ra.done_tag = a.done_tag, ra.done_value = a.done_value;
    ra.host_counts = a.host_counts, ra.live_out = a.live_out, ra.live_next = a.live_next;
    ra.ts = ctx->d_rts;
    hipEvent_t e0, e1;
    next_timing_pair(ctx, fr, &e0, &e1);
    FW_HIP(ctx, fw_launch_update_range(ctx->stream, ctx->g, ra, all_nospin, r_bytes > ctx->nt_bytes ? 2 : r_bytes > ctx->nt_wo_bytes_range ? 1 : 0, e0, e1));
    ctx->rslot_frame[rslot] = ctx->frame + 1;
    fr.range_launched = true;
    return FW_OK;
}

// ---- small types: one wave each (fw_k_small.hip)
fw_status launch_small(fw_ctx *ctx, FwFrame &fr) {
    const FwUpdateArgs &a = fr.a;
    fw_status st = FW_OK;
    const bool list_resent = ctx->small_dirty;
    if (ctx->small_dirty) {  // the list changed (a spawner built or destroyed, a type that outgrew the mode): re-sent through the stream
        ctx->small_list.clear();
        for (int wide = 0; wide < 2; wide++) {  // narrow types first, then the wide ones (FwSmallArgs::n_narrow)
            for (uint32_t si = 0; si < fr.n_seg; si++)
                if (ctx->segs[si].in_use && ctx->segs[si].small && (int)(ctx->segs[si].wide && !ctx->wave_all_on) == wide) ctx->small_list.push_back(si);
            if (!wide) ctx->n_narrow = (uint32_t)ctx->small_list.size();
        }
        if (ctx->small_list.size() > ctx->small_cap) return poison_segment(ctx, kNoSeg, "small-type list overflow");
        if ((st = ctx->small_fence.wait(ctx))) return st;
        // the previous frame's small launch ran on the ring stream and may not have read the OLD list yet: the copy below
        // (main stream) comes after it (the join used to be enqueued only further down, after the copy)
        if (ctx->small_last_side && ctx->side_dirty && (st = main_waits_side(ctx))) return st;
        memcpy(ctx->h_small, ctx->small_list.data(), ctx->small_list.size() * sizeof(uint32_t));
        FW_HIP(ctx, hipMemcpyAsync(ctx->d_small, ctx->h_small, ctx->small_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if ((st = ctx->small_fence.mark(ctx, ctx->stream))) return st;
        ctx->small_dirty = false;
    }
    FwSmallArgs sa{};
    sa.list = ctx->d_small, sa.n = (uint32_t)ctx->small_list.size(), sa.n_narrow = ctx->n_narrow, sa.parity = fr.p, sa.epoch = a.epoch, sa.dt = fr.dt;
    sa.seg_op_first = fr.small_hdr, sa.ops = fr.small_ops;
    sa.force_colors = a.force_colors, sa.dbg = ctx->dbg;
    sa.any_inst = ctx->census.n_inst != 0 ? 1u : 0u;
    sa.any_coll = ctx->census.n_small_coll != 0 ? 1u : 0u;
    sa.done_tag = a.done_tag, sa.done_value = a.done_value;
    sa.host_counts = a.host_counts, sa.live_out = a.live_out, sa.live_next = a.live_next;
    // next to the collision passes of the frame, on the ring stream (fw_ctx::small_last_side)
    const bool small_side = fr.legacy && fr.frame_mode != FW_MODE_FUSED && sa.n != 0 && ctx->host_fast && ctx->use_fifo_stream && ctx->stream.owned() &&
                            ctx->live_ring == nullptr && ctx->census.n_small_coll == 0 && !list_resent;
    if (!sa.n) return FW_OK;
    if ((st = order_side(ctx, small_side, ctx->small_last_side))) return st;
    if (small_side) sa.done_tag = nullptr;  // (the "frame has started" word recycles buffers the MAIN stream's launches read)
    hipEvent_t e0, e1;
    next_timing_pair(ctx, fr, &e0, &e1);
    FW_HIP(ctx, fw_launch_update_small(small_side ? ctx->fifo_stream : ctx->stream, ctx->g, sa, e0, e1));
    if (small_side) ctx->side_dirty = true;
    if (fr.small_tslot >= 0) {
        if (small_side) {
            if ((st = ctx->consumed[fr.small_tslot].mark(ctx, ctx->fifo_stream))) return st;
        } else {
            ctx->slot_frame[fr.small_tslot] = ctx->frame + 1;  // free once a launch after this frame has started
        }
    }
    fr.small_launched = true;
    return FW_OK;
}

// ---- the compacting launch (update_particles + compaction, core.rs:577-670), and the colours a caller's write left behind
fw_status launch_general(fw_ctx *ctx, FwFrame &fr) {
    if (fr.total_tiles || !(fr.fifo_launched || fr.range_launched || fr.small_launched)) {
        hipEvent_t e0, e1;
        next_timing_pair(ctx, fr, &e0, &e1);
        FW_HIP(ctx, fw_launch_update(ctx->stream, ctx->g, fr.a, fr.spawn_form == FW_SPAWN_INLINE ? &fr.inl : nullptr, fr.spawn_form,
                                     fr.frame_mode, e0, e1));
    }
    if (fr.timed) ctx->tev_frames++;
    if (!ctx->colors_dirty) return FW_OK;
    // that update wrote every colour of its output; the buffer it read (next frame's output) may still hold the
    // caller's colours past the survivors: back to the fill value, after which constant planes are skipped again
    for (uint32_t i = 0; i < fr.n_seg; i++) {
        SegHost &S = ctx->segs[i];
        if (!S.in_use || !S.colors_dirty) continue;
        FW_HIP(ctx, fw_launch_fill_colors(ctx->stream, S.buf[ctx->parity], nullptr, S.capacity, S.fill_bc, S.fill_em));
        S.colors_dirty = false;
    }
    ctx->colors_dirty = false;
    // every particle has been through an update since the caller's write: scale and colours are functions of the age
    // again, a type with an attached instance buffer can stop storing them (FW_TYPE_DERIVED; waits for this frame: rare)
    // (the flag flips at the START of the next fw_step, before anything of that frame is enqueued: flipping it waits for
    // the stream -- the frame just enqueued still stores the planes -- and may fail; fw_step itself only enqueues, and
    // by now this frame must finish its bookkeeping whatever happens)
    for (uint32_t i = 0; i < fr.n_seg; i++)
        if (ctx->segs[i].in_use && ctx->segs[i].derive_pending) {
            ctx->segs[i].derive_pending = false;
            if (wants_derived(ctx, ctx->segs[i])) ctx->segs[i].derive_ready = true, ctx->derive_ready_any = true;
        }
    return FW_OK;
}

// ---- the frame's bookkeeping: recycled slot, armed snapshot row, what the next frame's forecast finds, the counters
fw_status end_frame(fw_ctx *ctx, FwFrame &fr) {
    fw_status st;
    if (fr.slot >= 0 && (st = ctx->consumed[fr.slot].mark(ctx, ctx->stream))) return st;
    if (fr.snap >= 0) {
        ctx->snap_pending[fr.snap] = true;
        ctx->snap_seen[fr.snap] = false;
        ctx->snap_epoch[fr.snap] = fr.a.epoch;
        ctx->snap_cum[fr.snap].resize(fr.n_seg);
        for (uint32_t i = 0; i < fr.n_seg; i++) ctx->snap_cum[fr.snap][i] = ctx->segs[i].cum_spawn;
    }

    ctx->fc_ok = fr.fc_frame;
    ctx->boxes_epoch = fr.a.boxes ? fr.a.epoch : 0u;
    ctx->fc_dt_bits = fr.dt_bits;
    ctx->fc_tab_seq = ctx->tab_seq;
    ctx->parity ^= 1u;
    ctx->frame++;
    ctx->sim_time += (double)fr.dt;
    fr.prof(ctx, 7);
    if (ctx->frame > ctx->host_prof_skip) ctx->prof_frames++;
    return FW_OK;
}

}  // namespace

namespace fwh {

fw_status enqueue_frame(fw_ctx *ctx, FwFrame &fr) {
    fr.p = ctx->parity;
    update_args(ctx, fr);
    // a frame whose only GPU work can be one FIFO launch (fw_ctx::withheld, launch_fifo): no compacting, range or small segment, no separate
    // pass, no colour fill, nobody who wants a count or a time per frame.  Any other frame puts a withheld one on the stream first.
    fr.quiet = ctx->use_fuse2 && ctx->census.n_fifo != 0 && ctx->census.n_in_use == ctx->census.n_fifo && !ctx->census.n_range && !ctx->census.n_small && !fr.total_tiles && !fr.legacy &&
               !fr.fuse && !ctx->colors_dirty && ctx->live_ring == nullptr && !ctx->timing;
    fw_status st = fr.quiet ? FW_OK : flush_withheld(ctx);
    if (!st) st = set_forecast(ctx, fr);
    if (st) return st;
    pick_snapshot(ctx, fr);
    fr.prof(ctx, 4);
    if ((st = fr.legacy ? spawn_passes(ctx, fr) : op_table(ctx, fr))) return st;
    if (ctx->h_done) fr.a.done_tag = ctx->h_done, fr.a.done_value = ctx->frame;
    fr.prof(ctx, 5);
    if (ctx->census.n_fifo && (st = launch_fifo(ctx, fr))) return st;
    if (ctx->census.n_range && (st = launch_range(ctx, fr))) return st;
    if (ctx->census.n_small && (st = launch_small(ctx, fr))) return st;
    if ((st = launch_general(ctx, fr))) return st;
    fr.prof(ctx, 6);
    return end_frame(ctx, fr);
}

}  // namespace fwh
