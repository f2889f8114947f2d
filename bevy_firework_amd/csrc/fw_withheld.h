// fw_withheld.h -- the withheld group: up to FW_FUSE_MAX - 1 frames (the far tier, round 32: FW_FUSE_FAR - 1) of unread FIFO rings whose launches wait for the frame that closes the
// group, or for somebody who reads (fw_fuse2.h: the rules).  A value with three transitions -- offer, take, drop -- and the
// one type everything that reaches the stream goes through, FwFifoLaunch.  Nothing outside this header writes a field of the group.
// Plain host C++: no HIP call, nothing of the engine (fw_ctx, SegHost).  The engine (fw_engine_launch.cpp: launch_fifo, flush_withheld)
// and two host tests that drive the group through random hosts beside a model of their own (tests/test_cpp_host_withheld.py,
// test_cpp_host_withheld_far.py; the model: tests/fuse_model.py) compile the same lines.
#pragma once
#include <string.h>
#include "fw_kernels.h"

// one FIFO launch ready for the stream: the kernel's arguments and what the host books when it goes
struct FwFifoLaunch {
    FwFifoArgs fa;   // depth 1: the frame's launch as built (fa.fused == 0); deeper: the fused launch (fa.fused == depth, fa.dt the last frame's)
    FwInlineOps fio;
    FwFuseRecords rec;  // depth >= 2: the dt and boundaries of the withheld frames 0 .. depth - 2, in the records the fused kernels take; depth 1: unused
                        // (but for the rings' constants, rec.fz.move, which every frame's launch carries)
    uint32_t tiles, n_ops;
    int nt;          // the non-temporal form the LAST frame's launch would have taken
    uint32_t depth;  // frames the launch runs: 1 .. FW_FUSE_MAX, the far tier's up to FW_FUSE_FAR
    bool held;       // some frame of it waited in the group
    uint64_t frame[FW_FUSE_FAR];                // fw_ctx::frame of each of them (what its cohorts carry)
    uint64_t spin_from[FW_FIFO_PER_LAUNCH];     // per ring: what a cohort of the LAST frame carries as its spin pointer (the eager rule's)
};

// what an offer leaves to enqueue, in this order: the group that was pending (first), the offered launch -- alone, or as the closing frame of
// the group, fused (second); either may be null.  withheld: the offered launch is kept, and is in neither.  `first` stays readable until
// the next offer, `second` is the caller's own record
struct FwOffered {
    const FwFifoLaunch *first, *second;
    bool withheld;
};

// One op for a run of identical frames (round 32).  fw_spawn_one takes nothing of a frame but the op's own fields and the RNG serial
// serial_base + (k - rel_base), and the spawning workgroups of a FIFO launch read no other field of an op (not head, first_block or
// range_ring: fw_update_fifo_body).  So op `b` of a later frame -- rel_base already shifted into the group's numbering -- that continues
// `last` in particles and in serials, from the same emitter record with bit-identical origin, parent velocity and modifiers, is `last`
// with b.n more particles: every new particle k gets the emitter record and the serial it would have got; which frame spawned it is
// decided by FwFuseArgs::spawn_end, not by the op.
inline bool fw_op_continues(const FwOp &last, const FwOp &b) {
    return b.seg == last.seg && b.emit == last.emit && b.serial_base == last.serial_base + last.n && b.rel_base == last.rel_base + last.n &&
           memcmp(b.origin_pos, last.origin_pos, sizeof b.origin_pos) == 0 && memcmp(b.origin_rot, last.origin_rot, sizeof b.origin_rot) == 0 &&
           memcmp(b.parent_vel, last.parent_vel, sizeof b.parent_vel) == 0 && memcmp(&b.speed, &last.speed, 4) == 0 && memcmp(&b.scale, &last.scale, 4) == 0;
}

class FwWithheld {
public:
    // B: the launch this frame has just built, complete (fa, fio, tiles, n_ops, nt, spin_from; depth, held and frame are set here).
    // candidate: it may wait, or take the waiting ones in (fw_fuse2_candidate); depth_max: how deep a group it may close or continue.
    // B joins the group when it is a candidate, the group is short of depth_max and join() admits it: the frame that completes depth_max
    // closes the group -- B has become the fused launch --, any other is withheld with it.  A declined B sends the group out first; then
    // it starts a new group if it is a candidate, and goes out alone otherwise.
    // depth_max > FW_FUSE_MAX: the far tier, and there alone a frame's first op of a ring that continues the group's last op of that ring
    // is merged into it (fw_op_continues) -- one ring with a still emitter then needs one op for the whole group; with depth_max <=
    // FW_FUSE_MAX the ops stay one per frame and everything the group does is what it did before the tier existed.
    FwOffered offer(FwFifoLaunch &B, bool candidate, uint32_t depth_max, uint64_t frame) {
        FwOffered o{nullptr, nullptr, false};
        B.depth = 1u, B.held = false, B.frame[0] = frame;
        if (on_ && candidate && slot_[at_].depth < depth_max && join(B, depth_max > FW_FUSE_MAX)) {
            if (B.depth >= depth_max) on_ = false, o.second = &B;
            else keep(slot_[at_], B), o.withheld = true;  // (the group so far is the fused launch, kept: what take() hands out)
            return o;
        }
        o.first = take();
        if (!candidate) {
            o.second = &B;
            return o;
        }
        at_ ^= 1u;  // (what `first` points at stays as it is)
        keep(slot_[at_], B);
        for (uint32_t j = 0; j < B.fa.n_segs; j++) grp_[j] = fw_fuse_begin(FwFifoFrame{B.fa.s[j].head, B.fa.s[j].n_in, B.fa.s[j].n_spawn, B.fa.s[j].dead});
        on_ = true, o.withheld = true;
        return o;
    }
    // the group so far as ONE launch -- one withheld frame exactly as it was built, two to FW_FUSE_MAX - 1 as the fused launch of that
    // depth: whoever reads first pays one launch --, or null: nothing is pending.  Readable until the next offer
    const FwFifoLaunch *take() {
        if (!on_) return nullptr;
        on_ = false;
        return &slot_[at_];
    }
    // the group goes with the particles it would have updated
    void drop() { on_ = false; }
    uint32_t depth() const { return on_ ? slot_[at_].depth : 0u; }  // withheld frames: 0 .. FW_FUSE_FAR - 1

private:
    // A withheld launch arms no snapshot row and reports no counts (the launch that runs the frame, fused or alone, leaves the device's
    // counters as they must be; a row nobody fills would stay armed)
    static void keep(FwFifoLaunch &P, const FwFifoLaunch &B) {
        P = B;
        P.fa.host_counts = nullptr, P.held = true;
    }
    // B joins the group P when every ring of B is the ring of the group at the same place, every ring's group takes B's frame in
    // (fw_fuse_push: the pair rule between the fused frame so far and B) and the ops of all frames fit (FW_INLINE_OPS = 8: one ring with one
    // op per frame reaches FW_FUSE_MAX frames, a launch that carries two ops per frame closes its groups at four).  The fused launch is B's
    // with the group's head, live count and input row in front; the group's ops first, in frame order, B's behind them (rel_base shifted by
    // the new particles in front of them); `rec`: the withheld frames' dt and boundaries (FwFuseRecords: whichever record holds the frame).
    // merge: B's first op of a ring may become part of the group's last op of that ring.  false: declined, nothing changed.
    bool join(FwFifoLaunch &B, bool merge) {
        const FwFifoLaunch &P = slot_[at_];
        FwFifoArgs &fa = B.fa;
        const uint32_t d = P.depth;  // (withheld frames: B is frame d of the group)
        if (d < 1u || d >= FW_FUSE_FAR) return false;
        if (P.fa.n_segs != fa.n_segs || P.fa.write_mask != fa.write_mask || P.n_ops > FW_INLINE_OPS || B.n_ops > FW_INLINE_OPS) return false;
        FwFuseGroup grp[FW_FIFO_PER_LAUNCH];
        uint32_t merged = 0;  // ops of B that become part of an op of the group
        for (uint32_t j = 0; j < fa.n_segs; j++) {
            const FwFifoSeg &A = P.fa.s[j], &F = fa.s[j];
            if (A.buf != F.buf || A.seg != F.seg || A.capacity != F.capacity || A.type_idx != F.type_idx || A.keys_off != F.keys_off ||
                A.keys_len != F.keys_len || A.life != F.life || A.mat || F.mat || A.destroyed || F.destroyed || A.nest || F.nest)
                return false;
            grp[j] = grp_[j];
            if (!fw_fuse_push(F.capacity, grp[j], FwFifoFrame{F.head, F.n_in, F.n_spawn, F.dead}, FW_FUSE_FAR)) return false;
            if (merge && A.op0 < A.op1 && F.op0 < F.op1) {
                FwOp b = B.fio.ops[F.op0];
                b.rel_base += grp[j].spawn_end[d - 1u];
                merged += fw_op_continues(P.fio.ops[A.op1 - 1u], b) ? 1u : 0u;
            }
        }
        if (P.n_ops + B.n_ops - merged > FW_INLINE_OPS) return false;
        B.rec.continue_from(d >= 2u ? &P.rec : nullptr);  // (one withheld frame: its records are unused, whatever they hold)
        const uint32_t w = d - 1u;  // (the withheld frame this join adds: the group's latest)
        B.rec.dt(w) = P.fa.dt;
        FwInlineOps ops;
        uint32_t n = 0, t = 0;
        for (uint32_t j = 0; j < fa.n_segs; j++) {
            const FwFifoSeg &A = P.fa.s[j];
            FwFifoSeg &F = fa.s[j];
            const FwFifoFrame &U = grp[j].U;
            const uint32_t o0 = n;
            for (uint32_t x = A.op0; x < A.op1; x++) ops.ops[n++] = P.fio.ops[x];
            for (uint32_t x = F.op0; x < F.op1; x++) {
                FwOp b = B.fio.ops[x];
                b.rel_base += grp[j].spawn_end[w];
                if (merge && x == F.op0 && n > o0 && fw_op_continues(ops.ops[n - 1u], b)) ops.ops[n - 1u].n += b.n;
                else ops.ops[n++] = b;
            }
            const FwFifoLayout L = fw_fifo_layout(F.capacity, FW_TILE, FW_BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
            F.head = U.head, F.n_in = U.n_in, F.n_spawn = U.n_spawn, F.dead = U.dead;
            B.rec.spawn_end(j, w) = grp[j].spawn_end[w], B.rec.dead(j, w) = grp[j].dead[w];
            F.op0 = o0, F.op1 = n;
            F.spawn_a = L.spawn_a, F.n_vt_a = L.n_vt_a, F.n_vt_b = L.n_vt_b, F.tile0 = L.tile0, F.n_tiles = L.n_tiles;
            F.tile_first = t;
            t += F.n_tiles;
            grp_[j] = grp[j];
        }
        for (uint32_t x = 0; x < n; x++) B.fio.ops[x] = ops.ops[x];
        fa.parity = P.fa.parity, fa.fused = d + 1u;
        B.tiles = t, B.n_ops = n;
        B.frame[d] = B.frame[0];
        for (uint32_t f = 0; f < d; f++) B.frame[f] = P.frame[f];
        B.depth = d + 1u, B.held = true;
        return true;
    }

    bool on_ = false;
    uint32_t at_ = 0;      // the slot the group lives in; the other one keeps what the latest offer sent out as `first`
    FwFifoLaunch slot_[2] = {};
    FwFuseGroup grp_[FW_FIFO_PER_LAUNCH];   // per ring of the group: the fused frame and every frame's share (fw_fuse2.h)
};
