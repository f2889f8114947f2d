// fw_withheld.h -- the withheld group: up to FW_FUSE_MAX - 1 frames of unread FIFO rings whose launches wait for the frame that closes the
// group, or for somebody who reads (fw_fuse2.h: the rules).  A value with three transitions -- offer, take, drop -- and the
// one type everything that reaches the stream goes through, FwFifoLaunch.  Nothing outside this header writes a field of the group.
// Plain host C++: no HIP call, nothing of the engine (fw_ctx, SegHost).  The engine (fw_engine_launch.cpp: launch_fifo, flush_withheld)
// and a host test that drives the group through random hosts beside a model of its own (tests/test_cpp_host_withheld.py) compile the same lines.
#pragma once
#include <string.h>
#include "fw_kernels.h"

// one FIFO launch ready for the stream: the kernel's arguments and what the host books when it goes
struct FwFifoLaunch {
    FwFifoArgs fa;   // depth 1: the frame's launch as built (fa.fused == 0); deeper: the fused launch (fa.fused == depth, fa.dt the last frame's)
    FwInlineOps fio;
    FwFuseArgs fz;   // depth >= 2: the fused kernels' fourth argument, the dt and boundaries of frames 0 .. depth - 2; depth 1: unused
    uint32_t tiles, n_ops;
    int nt;          // the non-temporal form the LAST frame's launch would have taken
    uint32_t depth;  // frames the launch runs: 1 .. FW_FUSE_MAX
    bool held;       // some frame of it waited in the group
    uint64_t frame[FW_FUSE_MAX];                // fw_ctx::frame of each of them (what its cohorts carry)
    uint64_t spin_from[FW_FIFO_PER_LAUNCH];     // per ring: what a cohort of the LAST frame carries as its spin pointer (the eager rule's)
};

// what an offer leaves to enqueue, in this order: the group that was pending (first), the offered launch -- alone, or as the closing frame of
// the group, fused (second); either may be null.  withheld: the offered launch is kept, and is in neither.  `first` stays readable until
// the next offer, `second` is the caller's own record
struct FwOffered {
    const FwFifoLaunch *first, *second;
    bool withheld;
};

class FwWithheld {
public:
    // B: the launch this frame has just built, complete (fa, fio, tiles, n_ops, nt, spin_from; depth, held and frame are set here).
    // candidate: it may wait, or take the waiting ones in (fw_fuse2_candidate); depth_max: how deep a group it may close or continue.
    // B joins the group when it is a candidate, the group is short of depth_max and join() admits it: the frame that completes depth_max
    // closes the group -- B has become the fused launch --, any other is withheld with it.  A declined B sends the group out first; then
    // it starts a new group if it is a candidate, and goes out alone otherwise.
    FwOffered offer(FwFifoLaunch &B, bool candidate, uint32_t depth_max, uint64_t frame) {
        FwOffered o{nullptr, nullptr, false};
        B.depth = 1u, B.held = false, B.frame[0] = frame;
        if (on_ && candidate && slot_[at_].depth < depth_max && join(B)) {
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
    uint32_t depth() const { return on_ ? slot_[at_].depth : 0u; }  // withheld frames: 0 .. FW_FUSE_MAX - 1

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
    // the new particles in front of them); `fz`: the withheld frames' dt and boundaries.  false: declined, nothing changed.
    bool join(FwFifoLaunch &B) {
        const FwFifoLaunch &P = slot_[at_];
        FwFifoArgs &fa = B.fa;
        const uint32_t d = P.depth;  // (withheld frames: B is frame d of the group)
        if (d < 1u || d >= FW_FUSE_MAX) return false;
        if (P.fa.n_segs != fa.n_segs || P.n_ops + B.n_ops > FW_INLINE_OPS || P.fa.write_mask != fa.write_mask) return false;
        FwFuseGroup grp[FW_FIFO_PER_LAUNCH];
        for (uint32_t j = 0; j < fa.n_segs; j++) {
            const FwFifoSeg &A = P.fa.s[j], &F = fa.s[j];
            if (A.buf != F.buf || A.seg != F.seg || A.capacity != F.capacity || A.type_idx != F.type_idx || A.keys_off != F.keys_off ||
                A.keys_len != F.keys_len || A.life != F.life || A.mat || F.mat || A.destroyed || F.destroyed || A.nest || F.nest)
                return false;
            grp[j] = grp_[j];
            if (!fw_fuse_push(F.capacity, grp[j], FwFifoFrame{F.head, F.n_in, F.n_spawn, F.dead})) return false;
        }
        {
            FwFuseArgs fz = d >= 2u ? P.fz : FwFuseArgs{};  // (one withheld frame: its record is unused, whatever it holds)
            memcpy(fz.move, B.fz.move, sizeof fz.move);     // (... but for the rings' constants, which every frame's launch carries: B's own)
            B.fz = fz;
        }
        B.fz.dt_pre[d - 1u] = P.fa.dt;
        FwInlineOps ops;
        uint32_t n = 0, t = 0;
        for (uint32_t j = 0; j < fa.n_segs; j++) {
            const FwFifoSeg &A = P.fa.s[j];
            FwFifoSeg &F = fa.s[j];
            const FwFifoFrame &U = grp[j].U;
            const uint32_t o0 = n;
            for (uint32_t x = A.op0; x < A.op1; x++) ops.ops[n++] = P.fio.ops[x];
            for (uint32_t x = F.op0; x < F.op1; x++) ops.ops[n] = B.fio.ops[x], ops.ops[n++].rel_base += grp[j].spawn_end[d - 1u];
            const FwFifoLayout L = fw_fifo_layout(F.capacity, FW_TILE, FW_BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
            F.head = U.head, F.n_in = U.n_in, F.n_spawn = U.n_spawn, F.dead = U.dead;
            B.fz.spawn_end[j][d - 1u] = grp[j].spawn_end[d - 1u], B.fz.dead[j][d - 1u] = grp[j].dead[d - 1u];
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
    FwFuseGroup grp_[FW_FIFO_PER_LAUNCH];  // per ring of the group: the fused frame and every frame's share (fw_fuse2.h)
};
