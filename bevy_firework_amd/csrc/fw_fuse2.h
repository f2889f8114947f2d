// fw_fuse2.h -- up to FW_FUSE_FAR frames of an unread FIFO ring in one launch (rounds 22 to 32, FwFifoArgs::fused, FwFuseArgs and FwFarArgs: fw_kernels.h,
// DESIGN.md 4.0).
// A particle of a FIFO ring never moves: frame n + 1 of a slot needs nothing but frame n of the same slot.  A ring whose spin is deferred is
// a ring nobody has looked at for a while, so the host may withhold the launch of a frame A -- all of its bookkeeping done -- and run it
// inside the launch of a frame that follows: one load and one store per plane for two to sixteen updates.  The group grows frame by
// frame: the withheld frames so far are ONE fused frame (fw_fuse2_frame, folded), and the pair rule between it and the next frame is the
// rule of the group (FwFuseGroup, fw_fuse_push).  Here: what a launch lays out for a ring (the arithmetic launch_fifo has always done),
// when a frame may join, and the fused frame with the per-frame boundaries the kernel needs.
// Plain C++ behind FW_HD, like fw_spin.h: the host (launch_fifo) and the host tests (tests/test_cpp_host_fuse2.py, test_cpp_host_fuse_deep.py,
// test_cpp_host_fuse_wide.py, test_cpp_host_fuse_far.py, test_cpp_host_fuse_ladder.py, test_cpp_host_whole_tiles.py, test_cpp_host_whole_span.py)
// compile the same lines -- and so does the kernel, for fw_fifo_tile_whole (round 26).
#pragma once
#include <stdint.h>

#ifndef FW_HD
#ifdef __HIPCC__
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

// one frame of a ring as its launch sees it (FwFifoSeg): slot of logical particle 0 and live particles BEFORE the frame, the particles the
// frame spawns behind them (logical indices [n_in, n_in + n_spawn)) and the number it destroys (logical indices [0, dead))
struct FwFifoFrame {
    uint32_t head, n_in, n_spawn, dead;
};

// the workgroups of a ring in a launch (FwFifoSeg: tile0, spawn_a, n_vt_a, n_vt_b, n_tiles): first the new particles, `block` each, in
// two groups of consecutive slots -- [0, spawn_a) up to the end of the buffer, the rest from slot 0 --, then `live_tiles` ring tiles of
// `tile` slots from tile0 on, which cover the logical indices [lo, n_old); at least one workgroup in all (it publishes the counts)
struct FwFifoLayout {
    uint32_t tile0, live_tiles, spawn_a, n_vt_a, n_vt_b, n_tiles;
};
// (head < capacity, a multiple of `tile`; lo <= n_old <= capacity; first_new: logical index of the first new particle)
FW_HD FwFifoLayout fw_fifo_layout(uint32_t capacity, uint32_t tile, uint32_t block, uint32_t head, uint32_t lo, uint32_t n_old, uint32_t first_new,
                                  uint32_t n_spawn) {
    FwFifoLayout L;
    const uint32_t cnt = n_old - lo;
    const uint32_t ps = (uint32_t)(((uint64_t)head + lo) % capacity), ring_tiles = capacity / tile;
    const uint32_t ns0 = (uint32_t)(((uint64_t)head + first_new) % capacity);  // slot of the first new particle
    L.spawn_a = n_spawn < capacity - ns0 ? n_spawn : capacity - ns0;
    L.n_vt_a = (L.spawn_a + block - 1) / block, L.n_vt_b = (n_spawn - L.spawn_a + block - 1) / block;
    L.tile0 = ps / tile;
    const uint32_t need = (ps % tile + cnt + tile - 1) / tile;
    L.live_tiles = cnt ? (ring_tiles < need ? ring_tiles : need) : 0u;
    L.n_tiles = L.n_vt_a + L.n_vt_b + L.live_tiles;
    if (L.n_tiles == 0u) L.n_tiles = 1u;
    return L;
}

// Is ring tile `pt` (slots [pt * tile, (pt + 1) * tile)) of a launch WHOLE: does every one of its slots hold a particle that was in the ring
// before the launch and lives through it -- a logical index, counted from the launch's head with the ring's wrap, in [dead, n_in)?  (round 26:
// such a tile's update has no divergent lane, fw_update_fifo_body; head / n_in / dead: FwFifoSeg's, the fused frame's in a fused launch.)
// The logical indices of a tile's slots are consecutive unless the head lies strictly inside the tile: then the slots in front of it carry
// the LAST indices of the ring and the tile is whole only in a ring that is full and loses nobody.
// (head < capacity, a multiple of `tile`; pt < capacity / tile; dead <= n_in <= capacity)
FW_HD bool fw_fifo_tile_whole(uint32_t capacity, uint32_t tile, uint32_t head, uint32_t n_in, uint32_t dead, uint32_t pt) {
    const uint32_t s0 = pt * tile;
    if (n_in > capacity || dead > n_in) return false;  // (a count only the device knows, FwFifoSeg::n_in = 0xFFFFFFFF: never whole)
    if (head > s0 && head - s0 < tile) return dead == 0u && n_in == capacity;
    const uint32_t i0 = s0 >= head ? s0 - head : s0 + (capacity - head);  // (<= capacity - tile)
    return i0 >= dead && i0 + tile <= n_in;
}

// The whole tiles of a launch without a walk over its tiles (round 30).  The ring tiles fw_fifo_tile_whole calls whole are ONE cyclic run of
// tile indices: every tile of a full ring that loses nobody (the tile its head lies inside included); otherwise the tiles between the first
// tile boundary at or behind slot head + dead and the last one at or before slot head + n_in -- the survivors' slots, counted past the
// ring's end without wrapping; the head's own tile is never among them.  first / len: that run, ring tiles first, first + 1, ... (mod
// capacity / tile); count: how many of them lie among the `live_tiles` ring tiles the launch dispatches from tile0 on (fw_fifo_layout) --
// all of them where the layout starts at or in front of the first survivor, as every launch's does: a whole tile holds survivors alone.
// (head < capacity, a multiple of `tile`; tile0 < capacity / tile; live_tiles <= capacity / tile)
struct FwWholeSpan {
    uint32_t count, first, len;
};
FW_HD uint32_t fw_overlap(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {  // of [a0, a1) and [b0, b1)
    const uint32_t lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0u;
}
FW_HD FwWholeSpan fw_fifo_whole_span(uint32_t capacity, uint32_t tile, uint32_t head, uint32_t n_in, uint32_t dead, uint32_t tile0, uint32_t live_tiles) {
    FwWholeSpan W{0u, 0u, 0u};
    const uint32_t ring_tiles = capacity / tile;
    if (n_in > capacity || dead > n_in) return W;  // (a count only the device knows, FwFifoSeg::n_in = 0xFFFFFFFF: never whole)
    if (dead == 0u && n_in == capacity) {
        W.len = ring_tiles;
    } else {
        const uint64_t lo = ((uint64_t)head + dead + tile - 1u) / tile, hi = ((uint64_t)head + n_in) / tile;  // (fewer than ring_tiles apart)
        W.first = (uint32_t)(lo % ring_tiles), W.len = hi > lo ? (uint32_t)(hi - lo) : 0u;
    }
    // the run as offsets from tile0, [off, off + len) with off < ring_tiles, against the dispatched offsets [0, live_tiles) and their next turn
    const uint32_t off = W.first >= tile0 ? W.first - tile0 : W.first + (ring_tiles - tile0);
    W.count = fw_overlap(off, off + W.len, 0u, live_tiles) + fw_overlap(off, off + W.len, ring_tiles, ring_tiles + live_tiles);
    return W;
}

// Is a frame's launch one that may be withheld, or take the withheld one in?  enabled: fw_ctx::use_fuse2 (FW_FUSE2); quiet: the frame's only
// GPU work is FIFO launches; only_launch: this is the one launch of the frame and holds every FIFO ring of the context; spinless: it takes
// the spin-less form; unread_and_large: every ring of it deferred its spin in it and holds fw_ctx::fuse2_min live particles
FW_HD bool fw_fuse2_candidate(bool enabled, bool quiet, bool only_launch, bool spinless, bool unread_and_large) {
    return enabled && quiet && only_launch && spinless && unread_and_large;
}

// May the launch of frame A wait for frame B and run inside B's?  (Both frames qualify by themselves -- launch_fifo's rule; this is what
// the PAIR adds.)  B continues A.  No particle spawned in A or B dies within the pair: every dead particle of either frame was in the ring
// before A, so "dead" stays a prefix of the logical indices the fused launch counts from A's head.  And the new particles of both frames
// fit behind A's live particles without reaching the slots of A's own dead, which the fused view has not vacated: declined, not grown.
FW_HD bool fw_fuse2_ok(uint32_t capacity, const FwFifoFrame &A, const FwFifoFrame &B) {
    if (A.head >= capacity || A.n_in > capacity || A.n_spawn > capacity - A.n_in) return false;
    if (A.dead > A.n_in) return false;  // (a newborn of A dies in A)
    if (B.head != (uint32_t)(((uint64_t)A.head + A.dead) % capacity) || B.n_in != A.n_in + A.n_spawn - A.dead) return false;
    if ((uint64_t)A.dead + B.dead > A.n_in) return false;
    if ((uint64_t)A.n_in + A.n_spawn + B.n_spawn > capacity) return false;
    return true;
}

// the fused frame: counted from A's head over A's live particles, both frames' new particles behind them (A's first: FwFifoArgs::fuse_spawn
// = A.n_spawn), both frames' dead in front (FwFifoArgs::fuse_dead = A.dead)
FW_HD FwFifoFrame fw_fuse2_frame(const FwFifoFrame &A, const FwFifoFrame &B) { return FwFifoFrame{A.head, A.n_in, A.n_spawn + B.n_spawn, A.dead + B.dead}; }

// ---- a group of up to FW_FUSE_FAR consecutive frames (round 23: four; round 24: eight; round 32: sixteen).  The frames fold from the left: the
// group so far is the fused frame U of its members, and frame B may join exactly when fw_fuse2_ok(capacity, U, B) -- B continues U, the
// summed dead stay within the FIRST frame's live particles (nobody born in the group dies in it), and the first frame's live particles
// plus every frame's spawns fit the ring.  What the kernel needs beside U: where each frame's new particles end among the group's
// (cumulative: new particle k belongs to the first frame f with k < spawn_end[f]) and how many each frame destroys.
// The depths of the ladder (fw_fuse_depth_max): FW_FUSE_NARROW where round 23's threshold alone holds (fw_ctx::fuse_deep_min); FW_FUSE_MAX,
// the first tier -- what its kernels and their argument record (FwFuseArgs) hold -- where every ring holds fw_ctx::fuse_wide_min as well;
// FW_FUSE_FAR, the far tier, whose kernels read frames FW_FUSE_MAX - 1 .. FW_FUSE_FAR - 2 from a record of their own (FwFarArgs, fw_kernels.h).
#define FW_FUSE_MAX 8
#define FW_FUSE_NARROW 4
#define FW_FUSE_FAR 16
// (what fw_ctx::fuse_far_depth starts at: FW_FUSE_MAX = the tier is off; profiles/r32/fuse_far_ab.txt says how it was chosen)
#define FW_FUSE_FAR_DEFAULT 16
struct FwFuseGroup {
    FwFifoFrame U;                   // the fused frame of the members so far
    uint32_t depth;                  // members: 1 .. FW_FUSE_FAR
    uint32_t spawn_end[FW_FUSE_FAR]; // new particles of frames 0 .. f (spawn_end[depth - 1] == U.n_spawn)
    uint32_t dead[FW_FUSE_FAR];      // per frame (their sum == U.dead)
};
FW_HD FwFuseGroup fw_fuse_begin(const FwFifoFrame &A) {
    FwFuseGroup G{};
    G.U = A, G.depth = 1u, G.spawn_end[0] = A.n_spawn, G.dead[0] = A.dead;
    return G;
}
// may frame B join the group?  limit: the depth the group may reach (never beyond FW_FUSE_FAR, the tables' length; a caller that names
// none gets FW_FUSE_MAX, the first tier's cap -- what the call meant before the far tier, and what the programs written then still
// mean by it).  true: joined (G is the longer group); false: declined, G unchanged
FW_HD bool fw_fuse_push(uint32_t capacity, FwFuseGroup &G, const FwFifoFrame &B, uint32_t limit = FW_FUSE_MAX) {
    if (G.depth < 1u || G.depth >= limit || G.depth >= FW_FUSE_FAR || !fw_fuse2_ok(capacity, G.U, B)) return false;
    G.U = fw_fuse2_frame(G.U, B);
    G.spawn_end[G.depth] = G.U.n_spawn, G.dead[G.depth] = B.dead;
    G.depth++;
    return true;
}

// ---- the depth ladder: how deep a group of a launch may go.  Four rungs, each a threshold on the live particles of every ring of the launch,
// taken in this order: fw_ctx::fuse2_min (two frames), fuse_deep_min (min(knob, FW_FUSE_NARROW)), fuse_wide_min (the knob, fw_ctx::fuse_depth)
// and fuse_far_min (fw_ctx::fuse_far_depth, the far tier).  A ring's rung is the FIRST threshold its live count does not meet, whatever
// the later ones say; a launch's is the lowest rung of any of its rings.
enum { FW_RUNG_NONE = 0, FW_RUNG_TWO = 1, FW_RUNG_NARROW = 2, FW_RUNG_WIDE = 3, FW_RUNG_FAR = 4 };
FW_HD uint32_t fw_fuse_rung(uint32_t n_in, uint32_t fuse2_min, uint32_t deep_min, uint32_t wide_min, uint32_t far_min) {
    const uint32_t mins[FW_RUNG_FAR] = {fuse2_min, deep_min, wide_min, far_min};
    uint32_t r = FW_RUNG_NONE;
    while (r < FW_RUNG_FAR && n_in >= mins[r]) r++;
    return r;
}
// the depth a launch on `rung` (FW_RUNG_TWO at least: a launch below it is no candidate, fw_fuse2_candidate) may reach.  fuse_depth and
// fuse_far_depth: the knobs as fw_ctx holds them; the far rung counts only with the knob at FW_FUSE_MAX and the forms that defer their
// newborns' spin in use (newborn_deferred: FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN] != 0 -- the far tier has no eager kernels)
FW_HD uint32_t fw_fuse_depth_max(uint32_t rung, uint32_t fuse_depth, uint32_t fuse_far_depth, bool newborn_deferred) {
    const uint32_t knob = fuse_depth < 2u ? 2u : fuse_depth > FW_FUSE_MAX ? (uint32_t)FW_FUSE_MAX : fuse_depth;
    if (rung >= FW_RUNG_FAR && fuse_depth == FW_FUSE_MAX && newborn_deferred && fuse_far_depth > FW_FUSE_MAX)
        return fuse_far_depth < FW_FUSE_FAR ? fuse_far_depth : (uint32_t)FW_FUSE_FAR;
    return rung >= FW_RUNG_WIDE ? knob : rung == FW_RUNG_NARROW ? (knob < FW_FUSE_NARROW ? knob : (uint32_t)FW_FUSE_NARROW) : 2u;
}
