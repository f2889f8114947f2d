"""Groups of nine to sixteen frames of a FIFO ring in one launch without a GPU: the far tier (csrc/fw_fuse2.h: FwFarGroup, fw_far_begin,
fw_far_push -- the lines FwWithheld::join compiles -- and csrc/fw_withheld.h: fw_op_continues).  A stand-alone
C++ program in the manner of tests/test_cpp_host_fuse_wide.py, compiled -- once plainly, once with -fsanitize=address,undefined -- and
run directly, walks a reduced model of the kernel's grid (tiles of 4 slots, spawning workgroups of 2) slot by slot over rings of 8 to
64 slots.  A seeded random walk draws mostly small frames, so that groups grow to sixteen, and now and then anything; every frame is
also stepped by itself over an explicit ring of slots.  The fold must admit a frame exactly when stepping it met none of: a particle born
in the group dying in it, a new particle landing on a slot that held a particle when the group began, a frame that does not continue the
one before, a seventeenth frame.  For every admitted group of nine to sixteen frames the fused launch -- the layout fw_fifo_layout gives
for the folded frame, each new particle's frame taken from the cumulative bounds, the counters by the kernel's arithmetic -- must agree
with the frames stepped one by one: the slots stored (each live slot exactly once, nothing else), the updates every slot's particle
received and their order (an order-sensitive hash of the frames), both count rows, the destroyed count and the statistics; and
fw_fifo_whole_span must count the tiles fw_fifo_tile_whole calls whole among the dispatched ones.  fw_fuse_push, the first tier's, still
refuses a ninth frame.
The merge predicate against brute force: random lists of ops, frame by frame, drawn from a small alphabet so that runs occur, are merged
the way the group merges them (a frame's first op into the list's last); every new particle k must get the same (emit, serial, origin,
parent velocity, modifiers) from the merged and from the unmerged list, by the kernel's own lookup.  A pair that merges no longer merges
with one bit flipped in any compared field or with serial_base off by one, and still merges with the fields no spawning workgroup of the
FIFO launch reads (head, first_block, range_ring) changed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "fw_withheld.h"
static_assert(FW_FUSE_MAX == 8 && FW_FUSE_FAR == 16, "this program walks groups of up to sixteen frames and tries a seventeenth");
static const uint32_t TILE = 4, BLOCK = 2;
struct Slot { int id, born, n_upd; uint64_t hist; int stores; };  // id -1: empty; born -1: in the ring before the group; hist: the frames that updated it, in order
struct Frame { uint32_t spawn, dead; };
static unsigned long long n_bad = 0, n_groups[FW_FUSE_FAR + 1], n_declined, n_newborn_dies, n_overflow, n_discont, n_seventeenth, n_ninth, n_wrapped_head, n_wrapped_spawn,
                          n_compared, n_whole_tiles, n_merged, n_unmerged, n_particles, n_flips;
static uint64_t upd(uint64_t h, uint32_t f) { return h * 0x100000001B3ull + (uint64_t)(f + 1u); }
static void bad(const char *what, uint32_t C, uint32_t head, uint32_t n_in, const Frame *fr, uint32_t d) {
    if (n_bad++ < 20) {
        printf("BAD %s: C %u head %u n_in %u depth %u frames", what, C, head, n_in, d);
        for (uint32_t f = 0; f < d; f++) printf(" {%u %u}", fr[f].spawn, fr[f].dead);
        printf("\n");
    }
}
// the frames one by one over an explicit ring.  `orig`: the slots that held a particle when the group began
struct Stepped {
    std::vector<Slot> ring;
    std::vector<char> orig;
    uint32_t C, head, count, rows[2], parity, ndestroyed;
    unsigned long long stats;
    bool newborn_dies, overflow;
};
static void step(Stepped &S, const Frame &F, int f) {
    const uint32_t n_in = S.count;
    for (uint32_t k = 0; k < F.spawn; k++) {
        const uint32_t s = (S.head + n_in + k) % S.C;
        if (S.orig[s] || S.ring[s].id >= 0) S.overflow = true;
        S.ring[s] = Slot{1000 * (f + 1) + (int)k, f, 0, 0, 0};
    }
    const uint32_t all = n_in + F.spawn;
    for (uint32_t i = 0; i < all; i++) {
        Slot &x = S.ring[(S.head + i) % S.C];
        x.n_upd++, x.hist = upd(x.hist, (uint32_t)f);
    }
    for (uint32_t i = 0; i < F.dead; i++) {
        Slot &x = S.ring[(S.head + i) % S.C];
        if (x.born >= 0) S.newborn_dies = true;
        x.id = -1;
    }
    // the counters of one launch: reads row `parity`, writes the other
    S.rows[S.parity ^ 1u] = all - F.dead, S.parity ^= 1u, S.ndestroyed = F.dead, S.stats += all;
    S.head = (S.head + F.dead) % S.C, S.count = all - F.dead;
}
static Stepped begin(uint32_t C, uint32_t head, uint32_t n_in) {
    Stepped S;
    S.ring.assign(C, Slot{-1, -1, 0, 0, 0}), S.orig.assign(C, 0);
    for (uint32_t i = 0; i < n_in; i++) S.ring[(head + i) % C] = Slot{(int)i, -1, 0, 0, 0}, S.orig[(head + i) % C] = 1;
    const uint32_t parity0 = (head + n_in) & 1u;
    S.C = C, S.head = head, S.count = n_in, S.parity = parity0, S.rows[parity0] = n_in, S.rows[parity0 ^ 1u] = 0xDEADu, S.ndestroyed = 0, S.stats = 0;
    S.newborn_dies = S.overflow = false;
    return S;
}
// the fused launch of a group of D frames: what the kernel's workgroups do with FwFifoSeg {U} and the boundaries {spawn_end, dead}
static bool fused(const FwFarGroup &G, uint32_t C, uint32_t D, std::vector<Slot> &ring, uint32_t rows[2], uint32_t parity, uint32_t *ndestroyed, unsigned long long *stats) {
    const FwFifoFrame &U = G.U;
    const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
    const uint32_t ring_tiles = C / TILE;
    if (L.live_tiles > ring_tiles || L.n_tiles < 1u) return false;
    uint32_t covered = 0, whole = 0;
    for (uint32_t t = 0; t < L.live_tiles; t++) {
        const uint32_t pt = (L.tile0 + t) % ring_tiles;
        const bool w = fw_fifo_tile_whole(C, TILE, U.head, U.n_in, U.dead, pt);
        whole += w ? 1u : 0u;
        for (uint32_t s = pt * TILE; s < (pt + 1) * TILE; s++) {
            const uint32_t i = (s + C - U.head) % C;
            if (!(i < U.n_in && i >= U.dead)) {
                if (w) return false;  // (every slot of a whole tile holds a survivor)
                continue;
            }
            Slot &x = ring[s];
            if (x.id < 0) return false;
            for (uint32_t f = 0; f < D; f++) x.n_upd++, x.hist = upd(x.hist, f);  // the withheld frames' dt in order, then dt
            x.stores++, covered++;
        }
    }
    if (covered != U.n_in - U.dead) return false;
    if (fw_fifo_whole_span(C, TILE, U.head, U.n_in, U.dead, L.tile0, L.live_tiles).count != whole) return false;
    n_whole_tiles += whole;
    if (L.spawn_a < U.n_spawn) n_wrapped_spawn++;
    for (uint32_t wg = 0; wg < L.n_vt_a + L.n_vt_b; wg++) {
        const uint32_t k0 = wg < L.n_vt_a ? wg * BLOCK : L.spawn_a + (wg - L.n_vt_a) * BLOCK, k_end = wg < L.n_vt_a ? L.spawn_a : U.n_spawn;
        const uint32_t sbase = (U.head + U.n_in + k0) % C;
        for (uint32_t tid = 0; tid < BLOCK; tid++) {
            const uint32_t k = k0 + tid, s = sbase + tid;
            if (k >= k_end) continue;
            if (s >= C) return false;  // (a group's slots are consecutive)
            if (U.n_in + k < U.dead) return false;  // (no newborn of the group is among its dead)
            Slot &x = ring[s];
            if ((s + C - U.head) % C < U.n_in || x.id >= 0) return false;  // (never a slot an old particle is read from)
            uint32_t f0 = 0;
            while (f0 < D - 1 && k >= G.spawn_end[f0]) f0++;  // the kernel: the update of frame f when k < spawn_end[f]
            x = Slot{1000 * ((int)f0 + 1) + (int)(k - (f0 ? G.spawn_end[f0 - 1] : 0u)), (int)f0, 0, 0, x.stores + 1};
            for (uint32_t f = f0; f < D; f++) x.n_upd++, x.hist = upd(x.hist, f);
        }
    }
    for (uint32_t i = 0; i < U.dead; i++) ring[(U.head + i) % C].id = -1;
    // workgroup 0's counters (fw_update_fifo_body, the FUSE arm)
    const uint32_t sidx = parity, oidx = parity ^ 1u;
    uint32_t nc_prev = U.n_in, nc = U.n_in, all_f = 0, sp_done = 0, dead_done = 0;
    unsigned long long all_sum = 0;
    for (uint32_t f = 0; f < D; f++) {
        const uint32_t sp_end = f < D - 1 ? G.spawn_end[f] : U.n_spawn, dead_f = f < D - 1 ? G.dead[f] : U.dead - dead_done;
        nc_prev = nc, all_f = nc_prev + (sp_end - sp_done);
        nc = all_f - std::min(dead_f, all_f);
        sp_done = sp_end, dead_done += dead_f, all_sum += all_f;
    }
    const uint32_t last = (D & 1u) ? oidx : sidx, other = (D & 1u) ? sidx : oidx;
    rows[other] = nc_prev, rows[last] = nc;
    *ndestroyed = all_f - nc, *stats += all_sum;
    return true;
}
static void compare(uint32_t C, uint32_t head, uint32_t n_in, const Frame *fr, uint32_t D, const FwFarGroup &G, const Stepped &S, uint32_t parity0) {
    std::vector<Slot> one(C, Slot{-1, -1, 0, 0, 0});
    for (uint32_t i = 0; i < n_in; i++) one[(head + i) % C] = Slot{(int)i, -1, 0, 0, 0};
    uint32_t rows[2] = {0, 0}, ndestroyed = 0;
    rows[parity0] = n_in, rows[parity0 ^ 1u] = 0xDEADu;
    unsigned long long stats = 0;
    n_compared++;
    if (G.depth != D || G.spawn_end[D - 1] != G.U.n_spawn) { bad("group record", C, head, n_in, fr, D); return; }
    if (!fused(G, C, D, one, rows, parity0, &ndestroyed, &stats)) { bad("fused launch", C, head, n_in, fr, D); return; }
    if ((G.U.head + G.U.dead) % C != S.head || G.U.n_in + G.U.n_spawn - G.U.dead != S.count) bad("head / count", C, head, n_in, fr, D);
    if (rows[0] != S.rows[0] || rows[1] != S.rows[1] || ndestroyed != S.ndestroyed || stats != S.stats) bad("counters", C, head, n_in, fr, D);
    for (uint32_t s = 0; s < C; s++) {
        const bool in = (s + C - S.head) % C < S.count;
        if (in != (S.ring[s].id >= 0) || in != (one[s].id >= 0)) { bad("live set", C, head, n_in, fr, D); return; }
        if (!in) {
            if (one[s].stores) { bad("a store outside the live set", C, head, n_in, fr, D); return; }
            continue;
        }
        if (one[s].id != S.ring[s].id || one[s].born != S.ring[s].born || one[s].n_upd != S.ring[s].n_upd || one[s].hist != S.ring[s].hist) { bad("particle", C, head, n_in, fr, D); return; }
        if (one[s].stores != 1) { bad("stored once", C, head, n_in, fr, D); return; }
    }
}
// frame d, {sp, dd}, behind the d frames of G (admitted; stepped: S).  true: it joined -- H the longer group, T the ring behind it --,
// and everything a group of d + 1 frames must satisfy was compared; false: declined (as stepping says it must be), or the rule was wrong
static bool one_frame(uint32_t C, uint32_t head0, uint32_t n_in0, uint32_t parity0, Frame *fr, uint32_t d, const FwFarGroup *G, const Stepped &S, uint32_t sp, uint32_t dd,
                      FwFarGroup &H, Stepped &T) {
    fr[d] = Frame{sp, dd};
    T = S;
    step(T, fr[d], (int)d);
    const FwFifoFrame B{S.head, S.count, sp, dd};
    bool ok;
    if (d == 0) H = fw_far_begin(B), ok = true;  // (a frame of its own: dd <= S.count, the caller's choice)
    else H = *G, ok = fw_far_push(C, H, B);
    const bool clean = !T.newborn_dies && !T.overflow;
    if (ok != clean) { bad("rule", C, head0, n_in0, fr, d + 1); return false; }
    n_newborn_dies += T.newborn_dies, n_overflow += T.overflow;
    if (!ok) { n_declined++; return false; }
    n_groups[d + 1]++;
    if (d + 1 > FW_FUSE_MAX) {
        if (T.head < head0) n_wrapped_head++;
        compare(C, head0, n_in0, fr, d + 1, H, T, parity0);
    }
    if (d + 1 == FW_FUSE_MAX) {  // the first tier's fold holds the same eight frames and refuses a ninth, whatever it carries
        FwFuseGroup X = fw_fuse_begin(FwFifoFrame{head0, n_in0, fr[0].spawn, fr[0].dead});
        Stepped R = begin(C, head0, n_in0);
        step(R, fr[0], 0);
        bool all = true;
        for (uint32_t f = 1; f <= d; f++) all = all && fw_fuse_push(C, X, FwFifoFrame{R.head, R.count, fr[f].spawn, fr[f].dead}), step(R, fr[f], (int)f);
        if (!all || X.depth != FW_FUSE_MAX || memcmp(&X.U, &H.U, sizeof X.U) != 0 || memcmp(X.spawn_end, H.spawn_end, sizeof X.spawn_end) != 0 ||
            memcmp(X.dead, H.dead, sizeof X.dead) != 0)
            bad("the first tier's fold of the same eight frames", C, head0, n_in0, fr, d + 1);
        if (fw_fuse_push(C, X, FwFifoFrame{T.head, T.count, 0, 0}) || X.depth != FW_FUSE_MAX) bad("a ninth frame through fw_fuse_push", C, head0, n_in0, fr, d + 1);
        n_ninth++;
    }
    if (d + 1 == FW_FUSE_FAR) {  // a seventeenth frame never joins, whatever it carries
        FwFarGroup X = H;
        if (fw_far_push(C, X, FwFifoFrame{T.head, T.count, 0, 0}) || X.depth != FW_FUSE_FAR) bad("a seventeenth frame", C, head0, n_in0, fr, d + 1);
        n_seventeenth++;
    } else {  // a frame that does not continue the group is declined whatever else holds
        FwFarGroup X = H;
        if (fw_far_push(C, X, FwFifoFrame{(T.head + 1) % C, T.count, 0, 0}) && C > 1) bad("discontinuous head", C, head0, n_in0, fr, d + 1);
        X = H;
        if (T.count + 1 <= C && fw_far_push(C, X, FwFifoFrame{T.head, T.count + 1, 0, 0})) bad("discontinuous count", C, head0, n_in0, fr, d + 1);
        n_discont += 2;
    }
    return true;
}
static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // 0 .. n - 1 (xorshift64*)
    rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
    return (uint32_t)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static uint32_t pick(uint32_t hi, uint32_t small) {  // mostly small, so that sixteen frames fit; now and then nothing, now and then anything
    const uint32_t r = rnd(16);
    if (r == 0) return rnd(hi + 1u);
    if (r <= 2) return 0u;
    return rnd(std::min(hi, small) + 1u);
}
static void random_walks(uint32_t C, uint32_t trials) {
    for (uint32_t t = 0; t < trials; t++) {
        const uint32_t head = rnd(C), n_in = rnd(4) ? C / 4 + rnd(C / 2) : rnd(C + 1u);
        Stepped S = begin(C, head, n_in);
        const uint32_t parity0 = S.parity;
        FwFarGroup G{};
        Frame fr[FW_FUSE_FAR];
        for (uint32_t d = 0; d < FW_FUSE_FAR; d++) {
            const uint32_t sp = pick(C - S.count, C / 24u + 1u);
            uint32_t dd = pick(S.count + sp, C / 24u + 1u);
            if (d == 0) dd = std::min(dd, S.count);
            FwFarGroup H;
            Stepped T;
            if (!one_frame(C, head, n_in, parity0, fr, d, &G, S, sp, dd, H, T)) break;
            G = H, S = T;
        }
    }
}

// ---- the merge predicate against brute force
struct Got { uint32_t emit; uint64_t serial; float v[14]; bool found; };
static Got lookup(const std::vector<FwOp> &ops, uint32_t k) {  // the spawning workgroup's own: the last op that holds k
    Got g{};
    for (const FwOp &op : ops)
        if (k >= op.rel_base && k - op.rel_base < op.n) {
            g.found = true, g.emit = op.emit, g.serial = op.serial_base + (k - op.rel_base);
            memcpy(g.v, op.origin_pos, 16), memcpy(g.v + 4, op.origin_rot, 16), memcpy(g.v + 8, op.parent_vel, 16), g.v[12] = op.speed, g.v[13] = op.scale;
        }
    return g;
}
// every bit of one field of b0 (a field `last` and b0 are compared in), flipped by itself: the pair must no longer merge
static void flip(const FwOp &last, const FwOp &b0, const void *field, uint32_t bytes) {
    const size_t off = (size_t)((const unsigned char *)field - (const unsigned char *)&b0);
    for (uint32_t bit = 0; bit < bytes * 8u; bit++) {
        FwOp x = b0;
        ((unsigned char *)&x)[off + bit / 8u] ^= (unsigned char)(1u << (bit % 8u));
        if (fw_op_continues(last, x)) { if (n_bad++ < 20) printf("BAD merge: a pair that differs in one bit of a compared field still merges (offset %zu bit %u)\n", off, bit); }
        n_flips++;
    }
}
static void merges(uint32_t trials) {
    for (uint32_t t = 0; t < trials; t++) {
        std::vector<FwOp> plain, merged;
        const uint32_t D = 1u + rnd(FW_FUSE_FAR);
        uint32_t spawned = 0;
        uint64_t serial = 1000u + rnd(1000);
        uint32_t emit = rnd(2);
        float pos = (float)rnd(2), vel = 0.0f, speed = 1.0f;
        for (uint32_t f = 0; f < D; f++) {
            const uint32_t k_ops = rnd(8) == 0u ? 2u : rnd(8) == 0u ? 0u : 1u;
            uint32_t rel = 0;  // within the frame
            for (uint32_t x = 0; x < k_ops; x++) {
                // (mostly the frame before continues; now and then something of the emitter changes, or the serial jumps)
                const uint32_t r = rnd(24);
                if (r == 0) emit ^= 1u;
                else if (r == 1) pos += 1.0f;
                else if (r == 2) vel += 0.5f;
                else if (r == 3) speed *= 2.0f;
                else if (r == 4) serial += 1u + rnd(3);
                FwOp op{};
                op.seg = 2u, op.emit = emit, op.n = rnd(6), op.rel_base = rel, op.serial_base = serial, op.first_block = rnd(100), op.head = rnd(100);
                op.origin_pos[0] = pos, op.origin_rot[3] = 1.0f, op.parent_vel[1] = vel, op.speed = speed, op.scale = 1.0f;
                rel += op.n, serial += op.n;
                FwOp b = op;
                b.rel_base += spawned;  // (the new particles of the earlier frames of this ring sit in front)
                plain.push_back(b);
                if (x == 0 && !merged.empty() && fw_op_continues(merged.back(), b)) merged.back().n += b.n, n_merged++;
                else merged.push_back(b), n_unmerged++;
                if (x == 0 && plain.size() >= 2u) {
                    const FwOp &last = plain[plain.size() - 2u];
                    if (fw_op_continues(last, b)) {
                        FwOp b0 = b;
                        flip(last, b0, &b0.seg, 4), flip(last, b0, &b0.emit, 4), flip(last, b0, &b0.rel_base, 4), flip(last, b0, &b0.serial_base, 8);
                        flip(last, b0, b0.origin_pos, 16), flip(last, b0, b0.origin_rot, 16), flip(last, b0, b0.parent_vel, 16);
                        flip(last, b0, &b0.speed, 4), flip(last, b0, &b0.scale, 4);
                        FwOp y = b0;
                        y.serial_base += 1u;
                        if (fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: serial_base + 1 still merges\n"); }
                        y = b0, y.serial_base -= 1u;
                        if (fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: serial_base - 1 still merges\n"); }
                        y = b0, y.head ^= 0xFFu, y.first_block ^= 0xFFu, y.range_ring ^= 1u, y.n += 3u;
                        if (!fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: a field no spawning workgroup reads keeps a pair from merging\n"); }
                    }
                }
            }
            spawned += rel;
        }
        for (uint32_t k = 0; k < spawned; k++) {
            const Got a = lookup(plain, k), b = lookup(merged, k);
            n_particles++;
            if (!a.found || !b.found || a.emit != b.emit || a.serial != b.serial || memcmp(a.v, b.v, sizeof a.v) != 0)
                if (n_bad++ < 20) printf("BAD merge: particle %u of %u gets another record from the merged list (trial %u)\n", k, spawned, t);
        }
        if (lookup(merged, spawned).found) { if (n_bad++ < 20) printf("BAD merge: the merged list holds a particle nobody spawned\n"); }
    }
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const bool quick = atoi(argv[1]) != 0;
    for (uint32_t C : {8u, 16u, 20u, 32u, 64u}) {
        random_walks(C, quick ? 10000u : 200000u);
        printf("C %u groups of d9 %llu d10 %llu d11 %llu d12 %llu d13 %llu d14 %llu d15 %llu d16 %llu\n", C, n_groups[9], n_groups[10], n_groups[11], n_groups[12], n_groups[13],
               n_groups[14], n_groups[15], n_groups[16]);
    }
    merges(quick ? 2000u : 40000u);
    printf("total d9 %llu d10 %llu d11 %llu d12 %llu d13 %llu d14 %llu d15 %llu d16 %llu compared %llu declined %llu newborn_dies %llu overflow %llu discontinuous %llu "
           "seventeenth %llu ninth %llu wrapped_head %llu wrapped_spawn %llu whole_tiles %llu merged %llu unmerged %llu particles %llu flips %llu bad %llu\n",
           n_groups[9], n_groups[10], n_groups[11], n_groups[12], n_groups[13], n_groups[14], n_groups[15], n_groups[16], n_compared, n_declined, n_newborn_dies, n_overflow,
           n_discont, n_seventeenth, n_ninth, n_wrapped_head, n_wrapped_spawn, n_whole_tiles, n_merged, n_unmerged, n_particles, n_flips, n_bad);
    return n_bad ? 1 : 0;
}
"""

DEPTHS = ["d%d" % d for d in range(9, 17)]


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    # (fw_withheld.h -- the merge predicate's header -- includes fw_kernels.h, which g++ -Wall -Werror does not take alone: compiled
    # host-side by the Makefile's hipcc as plain C++, no device code and no HIP call, as tests/test_cpp_host_withheld.py compiles its program)
    d = tmp_path_factory.mktemp("fuse_far")
    (d / "fuse_far.cpp").write_text(PROGRAM)
    exe = d / "fuse_far"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([_hipcc(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                           "-I", CSRC] + flags + [str(d / "fuse_far.cpp"), "-o", str(exe)])
    # (the sanitizer build runs a twentieth of the walks: every path of the program)
    return str(exe), ("0" if request.param == "plain" else "1")


def test_groups_of_nine_to_sixteen_frames_and_the_merge_predicate(program):
    exe, quick = program
    r = subprocess.run([exe, quick], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:20]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0
    # groups of each depth occurred and were compared with the frames stepped one by one ...
    for k in DEPTHS:
        assert total[k] > 100, (k, total)
    assert total["compared"] == sum(total[k] for k in DEPTHS)
    # ... in every ring (the counts are cumulative, ring after ring)
    per_ring = [dict(zip(ln.split()[4::2], map(int, ln.split()[5::2]))) for ln in lines[:-1]]
    assert len(per_ring) == 5
    for k in DEPTHS:
        assert per_ring[0][k] > 0 and all(b[k] > a[k] for a, b in zip(per_ring, per_ring[1:])), (k, per_ring)
    # everything the rule must decline occurred and was declined, a seventeenth frame was offered to full groups and never joined, a ninth
    # never joined through fw_fuse_push, and the admitted groups include wrapped heads, new particles that wrap the buffer's end, whole tiles
    for k in ("declined", "newborn_dies", "overflow", "discontinuous", "seventeenth", "ninth", "wrapped_head", "wrapped_spawn", "whole_tiles"):
        assert total[k] > 0, (k, total)
    # the merge predicate: lists that merged and lists that did not, every particle looked up in both, every compared bit flipped
    assert total["merged"] > 1000 and total["unmerged"] > 1000 and total["particles"] > 10000 and total["flips"] > 100000, total
