"""What the host tests of the fused FIFO launches share (tests/test_cpp_host_fuse_deep.py, test_cpp_host_fuse_wide.py,
test_cpp_host_fuse_far.py, test_cpp_host_withheld.py, test_cpp_host_withheld_far.py; csrc/fw_fuse2.h, csrc/fw_withheld.h):
two models in C++ text, each the front part of a stand-alone program that a test completes with the part that is its own -- the depth
range, the ring sizes, the checks only it makes --, and the fixture that compiles such a program, once plainly and once with
-fsanitize=address,undefined, and runs it directly: nothing is loaded into Python, nothing is preloaded.

GRID_MODEL: a reduced model of the kernel's grid (tiles of 4 slots, spawning workgroups of 2) walked slot by slot.  Every frame is
stepped by itself over an explicit ring of slots (Stepped, step, begin); the fold (FwFuseGroup, fw_fuse_begin, fw_fuse_push) must admit a
frame exactly when stepping it met none of: a particle born in the group dying in it, a new particle landing on a slot that held a
particle when the group began, a frame that does not continue the one before, a frame beyond the limit (one_frame).  For an admitted
group the fused launch (fused) -- the layout fw_fifo_layout gives for the folded frame, each new particle's frame taken from the
cumulative bounds, the counters by the kernel's arithmetic -- must agree with the frames stepped one by one (compare): the slots stored
(each live slot exactly once, nothing else), the updates every slot's particle received and their order, both count rows, the destroyed
count and the statistics; and fw_fifo_whole_span must count the tiles fw_fifo_tile_whole calls whole among the dispatched ones.  The walks
that offer frames: every value or the edge values of every frame (walk), and a seeded random walk of mostly small frames (random_walks).
A program says before the model which header it compiles (fw_fuse2.h, or fw_withheld.h) and may define FW_MODEL_HIST_BASE = its deepest
group + 1: the history of a slot is then the exact base-N number of its frames (9^8 fits in 64 bits, 17^16 does not: an order-sensitive hash).

WITHHELD_MODEL: the withheld group (FwWithheld -- offer, take, drop) beside a model in its own words -- the plain list of the frames offered
since the last launch, each as it was built, with the depth_max it was offered with -- which says what every offer must do (join, close,
decline and why: judge, offer) and what every launch that comes out must hold (check_launch): its frames, each exactly once and in order;
fused, dt, parity; the dt and boundaries of withheld frames 0 to 6 in FwFuseArgs and of frames 7 to 14 in FwFarArgs, word for word; per
ring the first frame's head and live count, the summed spawns and dead, the layout fw_fifo_layout gives for the sums, cumulative
tile_first, the ring's constants; the ops ring by ring in frame order with rel_base shifted by the earlier frames' new particles -- a
frame that joined under a depth_max above FW_FUSE_MAX has its first op of a ring merged into the ring's last op where the model's own
predicate says it continues it --; a withheld frame that goes alone memcmp-equal to the launch as built, apart from host_counts ==
nullptr.  The random host that draws the frames is each test's own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")

GRID_MODEL = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
static const uint32_t TILE = 4, BLOCK = 2;
struct Slot { int id, born, n_upd; uint64_t hist; int stores; };  // id -1: empty; born -1: in the ring before the group; hist: the frames that updated it, in order
struct Frame { uint32_t spawn, dead; };
static unsigned long long n_bad = 0, n_groups[FW_FUSE_FAR + 1], n_declined, n_newborn_dies, n_overflow, n_discont, n_full, n_wrapped_head, n_wrapped_spawn, n_compared,
                          n_whole_tiles, n_spawn0, n_dead0, n_no_tile;
#ifdef FW_MODEL_HIST_BASE
static uint64_t upd(uint64_t h, uint32_t f) { return h * FW_MODEL_HIST_BASE + (uint64_t)(f + 1u); }
#else
static uint64_t upd(uint64_t h, uint32_t f) { return h * 0x100000001B3ull + (uint64_t)(f + 1u); }
#endif
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
static bool fused(const FwFuseGroup &G, uint32_t C, uint32_t D, std::vector<Slot> &ring, uint32_t rows[2], uint32_t parity, uint32_t *ndestroyed, unsigned long long *stats) {
    const FwFifoFrame &U = G.U;
    const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
    const uint32_t ring_tiles = C / TILE;
    if (L.live_tiles > ring_tiles || L.n_tiles < 1u) return false;
    if (L.live_tiles == 0) n_no_tile++;
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
static void compare(uint32_t C, uint32_t head, uint32_t n_in, const Frame *fr, uint32_t D, const FwFuseGroup &G, const Stepped &S, uint32_t parity0) {
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
// what a program checks beside the model where a frame has joined (H: the group of `depth` frames, T: the ring behind it), or null
static void (*after_join)(uint32_t C, uint32_t head0, uint32_t n_in0, const Frame *fr, uint32_t depth, const FwFuseGroup &H, const Stepped &T) = nullptr;
// frame d, {sp, dd}, behind the d frames of G (admitted; stepped: S), in a fold that may reach `limit` frames.  true: it joined -- H the longer
// group, T the ring behind it --, and everything a group of d + 1 frames must satisfy was compared (groups of cmp_from frames and more:
// the fused launch as well); false: declined (as stepping says it must be), or the rule was wrong
static bool one_frame(uint32_t C, uint32_t head0, uint32_t n_in0, uint32_t parity0, Frame *fr, uint32_t d, const FwFuseGroup *G, const Stepped &S, uint32_t sp, uint32_t dd,
                      FwFuseGroup &H, Stepped &T, uint32_t limit, uint32_t cmp_from) {
    fr[d] = Frame{sp, dd};
    T = S;
    step(T, fr[d], (int)d);
    const FwFifoFrame B{S.head, S.count, sp, dd};
    bool ok;
    if (d == 0) H = fw_fuse_begin(B), ok = true;  // (a frame of its own: dd <= S.count, the caller's choice)
    else H = *G, ok = fw_fuse_push(C, H, B, limit);
    const bool clean = !T.newborn_dies && !T.overflow;
    if (ok != clean) { bad("rule", C, head0, n_in0, fr, d + 1); return false; }
    n_newborn_dies += T.newborn_dies, n_overflow += T.overflow;
    if (!ok) { n_declined++; return false; }
    n_groups[d + 1]++;
    n_spawn0 += sp == 0, n_dead0 += dd == 0;
    if (d + 1 >= cmp_from) {
        if (T.head < head0) n_wrapped_head++;
        compare(C, head0, n_in0, fr, d + 1, H, T, parity0);
    }
    if (after_join) after_join(C, head0, n_in0, fr, d + 1, H, T);
    if (d + 1 == limit) {  // one frame more never joins, whatever it carries
        FwFuseGroup X = H;
        if (fw_fuse_push(C, X, FwFifoFrame{T.head, T.count, 0, 0}, limit) || X.depth != limit) bad("a frame beyond the limit", C, head0, n_in0, fr, d + 1);
        n_full++;
    } else {  // a frame that does not continue the group is declined whatever else holds
        FwFuseGroup X = H;
        if (fw_fuse_push(C, X, FwFifoFrame{(T.head + 1) % C, T.count, 0, 0}, limit) && C > 1) bad("discontinuous head", C, head0, n_in0, fr, d + 1);
        X = H;
        if (T.count + 1 <= C && fw_fuse_push(C, X, FwFifoFrame{T.head, T.count + 1, 0, 0}, limit)) bad("discontinuous count", C, head0, n_in0, fr, d + 1);
        n_discont += 2;
    }
    return true;
}
static std::vector<uint32_t> values(uint32_t hi, bool all) {  // 0 .. hi, or the edges of it
    std::vector<uint32_t> v;
    if (all) { for (uint32_t x = 0; x <= hi; x++) v.push_back(x); return v; }
    const uint32_t c[] = {0, 1, TILE + 1, hi / 3, hi - std::min(hi, 1u), hi};
    for (uint32_t x : c) if (x <= hi) v.push_back(x);
    std::sort(v.begin(), v.end()), v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}
// (the walks are [[maybe_unused]]: a program that leaves one out compiles under -Wall -Werror)
// frame d continues the group so far (d frames, admitted): every {spawn, dead} a frame of the ring can carry by itself (all), or the edge
// values, down to groups of max_depth frames
[[maybe_unused]] static void walk(uint32_t C, uint32_t head0, uint32_t n_in0, uint32_t parity0, Frame *fr, uint32_t d, const FwFuseGroup *G, const Stepped &S, bool all, uint32_t max_depth,
                 uint32_t limit, uint32_t cmp_from) {
    for (uint32_t sp : values(C - S.count, all))
    for (uint32_t dd : values(S.count + sp, all)) {
        if (d == 0 && dd > S.count) continue;  // (a group needs its first frame's dead to be old particles)
        FwFuseGroup H;
        Stepped T;
        if (one_frame(C, head0, n_in0, parity0, fr, d, G, S, sp, dd, H, T, limit, cmp_from) && d + 1 < max_depth)
            walk(C, head0, n_in0, parity0, fr, d + 1, &H, T, all, max_depth, limit, cmp_from);
    }
}
static uint64_t rng = 0x9E3779B97F4A7C15ull;
[[maybe_unused]] static uint32_t rnd(uint32_t n) {  // 0 .. n - 1 (xorshift64*)
    rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
    return (uint32_t)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
// mostly small, so that `limit` frames fit; one time in `odds` anything, `zeros` times in `odds` nothing
[[maybe_unused]] static uint32_t pick(uint32_t hi, uint32_t small, uint32_t odds, uint32_t zeros) {
    const uint32_t r = rnd(odds);
    if (r == 0) return rnd(hi + 1u);
    if (r <= zeros) return 0u;
    return rnd(std::min(hi, small) + 1u);
}
// `trials` groups from random heads and live counts, each grown frame by frame to `limit` frames or to the first frame the rule declines;
// small frames: up to C / small_div + 1 particles
[[maybe_unused]] static void random_walks(uint32_t C, uint32_t trials, uint32_t limit, uint32_t cmp_from, uint32_t small_div, uint32_t odds, uint32_t zeros) {
    for (uint32_t t = 0; t < trials; t++) {
        const uint32_t head = rnd(C), n_in = rnd(4) ? C / 4 + rnd(C / 2) : rnd(C + 1u);
        Stepped S = begin(C, head, n_in);
        const uint32_t parity0 = S.parity;
        FwFuseGroup G{};
        Frame fr[FW_FUSE_FAR];
        for (uint32_t d = 0; d < limit; d++) {
            const uint32_t sp = pick(C - S.count, C / small_div + 1u, odds, zeros);
            uint32_t dd = pick(S.count + sp, C / small_div + 1u, odds, zeros);
            if (d == 0) dd = std::min(dd, S.count);
            FwFuseGroup H;
            Stepped T;
            if (!one_frame(C, head, n_in, parity0, fr, d, &G, S, sp, dd, H, T, limit, cmp_from)) break;
            G = H, S = T;
        }
    }
}
"""

WITHHELD_MODEL = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "fw_withheld.h"
static_assert(FW_FUSE_MAX == 8 && FW_FUSE_NARROW == 4 && FW_FUSE_FAR == 16 && FW_INLINE_OPS == 8, "the depths and the ops limit this program counts");
static const uint32_t FAR_FROM = FW_FUSE_MAX - 1;  // withheld frames 0 .. 6 travel in FwFuseArgs, 7 .. 14 in FwFarArgs (fw_kernels.h)
static uint64_t rng;
static uint32_t rnd(uint32_t n) {  // 0 .. n - 1 (xorshift64*)
    rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
    return (uint32_t)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static unsigned long long n_bad, n_offers, n_withheld_new, n_joined_withheld, n_closed[FW_FUSE_FAR + 1], n_decl_pair, n_decl_ops, n_decl_ring, n_decl_depth, n_far_decl_pair,
    n_far_decl_ops, n_far_decl_depth, n_noncand_flush, n_alone, n_take[FW_FUSE_FAR], n_take_empty, n_drop_pending, n_drop_empty, n_depth_changed_inside, n_launches, n_frames_run,
    n_ops_merged, n_ops_kept_far, n_far_words, n_grew_into_far;
static uint64_t cur_seed, cur_step;
static void bad(const char *what, long long x = 0, long long y = 0) {
    if (n_bad++ < 30) printf("BAD seed %llu step %llu: %s (%lld, %lld)\n", (unsigned long long)cur_seed, (unsigned long long)cur_step, what, x, y);
}
#define CHECK(cond, ...) do { if (!(cond)) bad(__VA_ARGS__); } while (0)

// the host: rings as a FIFO ring's host keeps them, each with its emitter (a host that draws its ops otherwise leaves the emitter alone)
struct Ring { uint32_t capacity, head, live, type_idx, keys_off, keys_len; float life; char *buf; uint32_t emit; uint64_t serial; float pos, vel, speed; };
// the model: the frames offered since the last launch, each as it was built
struct Offered { uint64_t frame; uint32_t depth_max; FwFifoLaunch built; };
static std::vector<Offered> pending;
static std::vector<int> ran;  // per frame number: launches that ran it; -1: dropped
static uint64_t last_run;     // the latest frame a launch ran (frames and launches stay in order)

// the model's own words for "b is `last` with more particles"
static bool continues_model(const FwOp &last, const FwOp &b) {
    if (b.seg != last.seg || b.emit != last.emit) return false;
    if (b.serial_base != last.serial_base + (uint64_t)last.n || b.rel_base != last.rel_base + last.n) return false;
    for (int c = 0; c < 4; c++) {
        if (memcmp(&b.origin_pos[c], &last.origin_pos[c], 4) || memcmp(&b.origin_rot[c], &last.origin_rot[c], 4) || memcmp(&b.parent_vel[c], &last.parent_vel[c], 4)) return false;
    }
    return memcmp(&b.speed, &last.speed, 4) == 0 && memcmp(&b.scale, &last.scale, 4) == 0;
}
// the ops ring j of a launch that runs the frames `m` must carry.  *merged: how many ops became part of another
static std::vector<FwOp> ops_of(const std::vector<Offered> &m, uint32_t j, uint32_t *merged) {
    std::vector<FwOp> out;
    uint32_t spawn = 0;
    for (size_t f = 0; f < m.size(); f++) {
        const FwFifoSeg &X = m[f].built.fa.s[j];
        for (uint32_t x = X.op0; x < X.op1; x++) {
            FwOp want = m[f].built.fio.ops[x];
            want.rel_base += spawn;  // (the new particles of the earlier frames of this ring sit in front)
            // (a frame that JOINED under a depth_max above FW_FUSE_MAX: its first op of the ring may continue the ring's last)
            if (f > 0 && m[f].depth_max > FW_FUSE_MAX && x == X.op0 && !out.empty() && continues_model(out.back(), want)) out.back().n += want.n, (*merged)++;
            else out.push_back(want);
        }
        spawn += X.n_spawn;
    }
    return out;
}

// what a launch that runs the frames `m` must hold.  from_group: it comes out of the group (take, or the `first` of an offer)
static void check_launch(const FwFifoLaunch &L, const std::vector<Offered> &m, bool from_group) {
    const uint32_t D = (uint32_t)m.size();
    n_launches++;
    CHECK(D >= 1u && D <= FW_FUSE_FAR && L.depth == D, "depth", L.depth, D);
    if (D < 1u || D > FW_FUSE_FAR) return;
    const FwFifoLaunch &first = m[0].built, &last = m[D - 1].built;
    for (uint32_t f = 0; f < D; f++) {
        CHECK(L.frame[f] == m[f].frame, "frame number", (long long)L.frame[f], (long long)m[f].frame);
        CHECK(m[f].frame > last_run && ran[m[f].frame] == 0, "a frame runs once, in order", (long long)m[f].frame, ran[m[f].frame]);
        ran[m[f].frame]++, last_run = m[f].frame, n_frames_run++;
    }
    CHECK(D <= m[D - 1].depth_max, "deeper than the depth_max offered with the last frame", D, m[D - 1].depth_max);
    CHECK(L.fa.fused == (D == 1u ? 0u : D), "fused", L.fa.fused, D);
    CHECK(memcmp(&L.fa.dt, &last.fa.dt, 4) == 0, "dt is the last frame's");
    for (uint32_t f = 0; f + 1 < D; f++) {
        const float *have = f < FAR_FROM ? &L.rec.fz.dt_pre[f] : &L.rec.far.dt[f - FAR_FROM];
        const float named = L.rec.dt(f);
        CHECK(memcmp(have, &m[f].built.fa.dt, 4) == 0 && memcmp(&named, have, 4) == 0, "dt of a withheld frame", f);
    }
    CHECK(L.fa.parity == first.fa.parity, "parity is the first frame's", L.fa.parity, first.fa.parity);
    CHECK(L.fa.n_segs == first.fa.n_segs && L.fa.write_mask == last.fa.write_mask && L.fa.epoch == last.fa.epoch, "launch words");
    CHECK(L.held == (from_group || D >= 2u), "held", L.held, D);
    CHECK(from_group ? L.fa.host_counts == nullptr : L.fa.host_counts == last.fa.host_counts, "host_counts: none for a withheld launch, the closing frame's otherwise");
    CHECK(L.nt == last.nt, "nt is the last frame's", L.nt, last.nt);
    uint32_t t = 0, o = 0;
    for (uint32_t j = 0; j < L.fa.n_segs; j++) {
        const FwFifoSeg &F = L.fa.s[j], &A = first.fa.s[j], &Z = last.fa.s[j];
        CHECK(L.spin_from[j] == last.spin_from[j], "spin_from is the last frame's", j);
        CHECK(F.buf == Z.buf && F.seg == Z.seg && F.capacity == Z.capacity && F.type_idx == Z.type_idx && F.keys_off == Z.keys_off && F.keys_len == Z.keys_len &&
              F.life == Z.life && F.mat == Z.mat && F.destroyed == Z.destroyed && F.nest == Z.nest, "the ring's own words", j);
        CHECK(F.head == A.head && F.n_in == A.n_in, "head and n_in are the first frame's", j);
        CHECK(memcmp(L.rec.fz.move[j], last.rec.fz.move[j], sizeof last.rec.fz.move[j]) == 0, "the ring's constants are the last frame's", j);
        uint32_t spawn = 0, dead = 0, merged = 0;
        CHECK(F.op0 == o, "ops are grouped per ring", F.op0, o);
        const std::vector<FwOp> want = ops_of(m, j, &merged);
        for (size_t x = 0; x < want.size() && o < FW_INLINE_OPS; x++, o++) CHECK(memcmp(&L.fio.ops[o], &want[x], sizeof want[x]) == 0, "op", j, o);
        if (D > FW_FUSE_MAX) n_ops_merged += merged, n_ops_kept_far += want.size();
        for (uint32_t f = 0; f < D; f++) {
            const FwFifoSeg &X = m[f].built.fa.s[j];
            spawn += X.n_spawn, dead += X.dead;
            if (f + 1 < D) {
                const uint32_t se = f < FAR_FROM ? L.rec.fz.spawn_end[j][f] : L.rec.far.spawn_end[j][f - FAR_FROM];
                const uint32_t de = f < FAR_FROM ? L.rec.fz.dead[j][f] : L.rec.far.dead[j][f - FAR_FROM];
                CHECK(se == spawn && de == X.dead, "the boundaries of a withheld frame", j, f);
                CHECK(L.rec.spawn_end(j, f) == se && L.rec.dead(j, f) == de, "the owner's accessors name the same words", j, f);
                if (f >= FAR_FROM) n_far_words++;
            }
        }
        CHECK(F.op1 == o, "op1", F.op1, o);
        CHECK(F.n_spawn == spawn && F.dead == dead, "n_spawn and dead are the sums over the group", j);
        if (D >= 2u) {
            const FwFifoLayout W = fw_fifo_layout(F.capacity, FW_TILE, FW_BLOCK, A.head, dead, A.n_in, A.n_in, spawn);
            CHECK(F.spawn_a == W.spawn_a && F.n_vt_a == W.n_vt_a && F.n_vt_b == W.n_vt_b && F.tile0 == W.tile0 && F.n_tiles == W.n_tiles, "layout of the fused frame", j);
        }
        CHECK(F.tile_first == t, "tile_first is cumulative", F.tile_first, t);
        t += F.n_tiles;
    }
    CHECK(L.tiles == t, "tiles", L.tiles, t);
    CHECK(L.n_ops == o && o <= FW_INLINE_OPS, "n_ops", L.n_ops, o);
    if (D == 1u) {  // exactly as built
        FwFifoArgs want = first.fa;
        if (from_group) want.host_counts = nullptr;
        CHECK(memcmp(&L.fa, &want, sizeof want) == 0 && memcmp(&L.fio, &first.fio, sizeof first.fio) == 0, "one frame goes exactly as it was built");
    }
}

// may `me` join the frames of `pending`?  Each of the four conditions by itself
struct Verdict { bool depth, rings, ops, pair; bool all() const { return depth && rings && ops && pair; } int failed() const { return !depth + !rings + !ops + !pair; } };
static Verdict judge(const Offered &me) {
    const FwFifoLaunch &B = me.built;
    Verdict v{true, true, true, true};
    const uint32_t d = (uint32_t)pending.size();
    v.depth = d < me.depth_max && d < FW_FUSE_FAR;
    const FwFifoLaunch &P = pending.back().built;
    v.rings = P.fa.n_segs == B.fa.n_segs && P.fa.write_mask == B.fa.write_mask;
    for (uint32_t j = 0; v.rings && j < B.fa.n_segs; j++) {
        const FwFifoSeg &A = P.fa.s[j], &F = B.fa.s[j];
        v.rings = A.buf == F.buf && A.seg == F.seg && A.capacity == F.capacity && A.type_idx == F.type_idx && A.keys_off == F.keys_off && A.keys_len == F.keys_len &&
                  A.life == F.life && !A.mat && !F.mat && !A.destroyed && !F.destroyed && !A.nest && !F.nest;
    }
    // the ops the launch would carry, with what merges merged
    std::vector<Offered> with = pending;
    with.push_back(me);
    size_t ops = 0;
    uint32_t merged = 0;
    for (uint32_t j = 0; j < std::min(B.fa.n_segs, P.fa.n_segs); j++) ops += ops_of(with, j, &merged).size();
    if (B.fa.n_segs != P.fa.n_segs) ops = 0;  // (judged by the rings alone)
    v.ops = ops <= FW_INLINE_OPS;
    // the pair rule, ring by ring: nobody born in the group dies in it -- all the dead, B's too, were in the ring before the first frame --
    // and the first frame's live particles with every frame's new ones fit the ring; B continues the frames before it
    for (uint32_t j = 0; j < std::min(B.fa.n_segs, P.fa.n_segs); j++) {
        const FwFifoSeg &A = pending[0].built.fa.s[j], &F = B.fa.s[j];
        uint64_t spawn = 0, dead = 0;
        for (const Offered &f : pending) spawn += f.built.fa.s[j].n_spawn, dead += f.built.fa.s[j].dead;
        const uint64_t C = A.capacity;
        v.pair = v.pair && A.head < C && A.n_in <= C && dead <= A.n_in && A.n_in + spawn + F.n_spawn <= C && dead + F.dead <= A.n_in &&
                 F.head == (A.head + dead) % C && F.n_in == A.n_in + spawn - dead;
    }
    return v;
}

// ---- the steps of a random host (which of them, how often and with what draws: the program's own `host`)
static void new_rings(std::vector<Ring> &rings, uint32_t n, bool emitters) {
    rings.resize(n);
    for (uint32_t j = 0; j < n; j++) {
        Ring &R = rings[j];
        R.capacity = (2u + rnd(3)) * FW_TILE, R.head = rnd(R.capacity), R.live = R.capacity / 4u + rnd(R.capacity / 2u);
        R.type_idx = rnd(16), R.keys_off = rnd(64), R.keys_len = 1u + rnd(8), R.life = 1.0f + (float)rnd(8);
        R.buf = (char *)(uintptr_t)(0x100000u * (1u + rnd(1000)) + j * 0x1000u);
        if (emitters) R.emit = rnd(100), R.serial = rnd(1000000), R.pos = (float)rnd(10), R.vel = 0.0f, R.speed = 1.0f;
    }
}
static void somebody_reads(FwWithheld &W) {
    const FwFifoLaunch *L = W.take();
    if (pending.empty()) {
        CHECK(L == nullptr, "take on an empty group yields nothing");
        n_take_empty++;
    } else {
        CHECK(L != nullptr, "take hands the group out");
        if (L) check_launch(*L, pending, true);
        n_take[pending.size()]++;
        pending.clear();
    }
    CHECK(W.depth() == 0u && W.take() == nullptr, "nothing is pending behind a take");
}
static void particles_go(FwWithheld &W, std::vector<Ring> &rings, bool emitters) {  // ... and a withheld frame with them
    W.drop();
    (pending.empty() ? n_drop_empty : n_drop_pending)++;
    for (const Offered &f : pending) ran[f.frame] = -1;
    pending.clear();
    new_rings(rings, (uint32_t)rings.size(), emitters);
    CHECK(W.depth() == 0u && W.take() == nullptr, "nothing is pending behind a drop");
}
static void record_changes(Ring &R) {  // for good (an axis rule that ends, a type that is rebuilt)
    switch (rnd(5)) {
    case 0: R.type_idx ^= 1u << rnd(8); break;
    case 1: R.keys_off += 1u; break;
    case 2: R.keys_len += 1u; break;
    case 3: R.life += 0.5f; break;
    default: R.buf += 0x10000; break;
    }
}
// a frame, built as launch_fifo builds it, all of its bookkeeping done: the launch-wide words first, then ring by ring -- the ring's ops
// (the program's own; F.op0 and B.n_ops around them) and ring_frame
static void begin_frame(FwFifoLaunch &B, uint64_t &frame, uint32_t n_rings, int32_t write_mask) {
    static unsigned long long counts_word;
    memset(&B, 0, sizeof B);
    FwFifoArgs &fa = B.fa;
    frame++;
    ran.resize(frame + 1u, 0);
    fa.n_segs = n_rings, fa.parity = (uint32_t)(frame & 1u), fa.epoch = (uint32_t)frame, fa.write_mask = write_mask, fa.spinless = 1u, fa.q0pl = 1u;
    fa.dt = (float)(1u + rnd(1000)) / 32768.0f + (float)rnd(1000) * 1e-7f;
    fa.host_counts = &counts_word;
    fa.fuse_pad[FW_FIFO_NEWBORN] = 1u;
    B.nt = (int)rnd(3);
}
// (mostly a few of the oldest die; one time in dead_odds anything up to everybody, the frame's own newborns included; one time in odd_odds a
// frame no group may hold: materialised spawns, destroyed records, a Nested entry)
static void ring_frame(FwFifoLaunch &B, uint32_t j, Ring &R, uint32_t n_spawn, uint32_t dead_odds, uint32_t odd_odds) {
    FwFifoSeg &F = B.fa.s[j];
    F.op1 = B.n_ops;
    const uint32_t all = R.live + n_spawn;
    const uint32_t dead = rnd(dead_odds) == 0u ? rnd(all + 1u) : std::min(all, rnd(3) ? 0u : rnd(5));
    F.buf = R.buf, F.seg = j, F.capacity = R.capacity, F.type_idx = R.type_idx, F.keys_off = R.keys_off, F.keys_len = R.keys_len, F.life = R.life;
    F.head = R.head, F.n_in = R.live, F.n_spawn = n_spawn, F.dead = dead;
    for (int c = 0; c < 4; c++) B.rec.fz.move[j][c] = (float)(R.type_idx + c);
    if (rnd(odd_odds) == 0u) {
        const uint32_t r = rnd(3);
        if (r == 0u) F.mat = 1u;
        else if (r == 1u) F.destroyed = R.buf + 64;
        else F.nest = 1u;
    }
    const FwFifoLayout Y = fw_fifo_layout(R.capacity, FW_TILE, FW_BLOCK, R.head, std::min(dead, R.live), R.live, R.live, n_spawn);
    F.spawn_a = Y.spawn_a, F.n_vt_a = Y.n_vt_a, F.n_vt_b = Y.n_vt_b, F.tile0 = Y.tile0, F.n_tiles = Y.n_tiles;
    F.tile_first = B.tiles, B.tiles += F.n_tiles;
    B.spin_from[j] = rnd(1000);
    R.head = (uint32_t)(((uint64_t)R.head + dead) % R.capacity), R.live = all - dead;
}
// the frame is offered: what the offer must do, from the model, and what comes out of it
static void offer(FwWithheld &W, FwFifoLaunch &B, bool candidate, uint32_t depth_max, uint64_t frame) {
    Offered me{frame, depth_max, B};
    const bool group = !pending.empty();
    Verdict v{true, true, true, true};
    if (group) v = judge(me);
    const bool joins = group && candidate && v.all();
    const uint32_t d = (uint32_t)pending.size();
    n_offers++;
    const FwOffered o = W.offer(B, candidate, depth_max, frame);
    if (joins) {
        if (d + 1u > FW_FUSE_MAX && pending[0].depth_max <= FW_FUSE_MAX) n_grew_into_far++;
        pending.push_back(me);
        CHECK(o.first == nullptr, "a frame that joins sends nothing out first");
        if (d + 1u >= depth_max) {
            CHECK(!o.withheld && o.second == &B, "the frame that completes depth_max closes the group");
            if (o.second) check_launch(*o.second, pending, false);
            n_closed[d + 1u]++;
            pending.clear();
        } else {
            CHECK(o.withheld && o.second == nullptr, "a frame that joins a group short of its depth is withheld with it");
            n_joined_withheld++;
        }
    } else {
        if (group && candidate && v.failed() == 1) {
            (!v.depth ? n_decl_depth : !v.rings ? n_decl_ring : !v.ops ? n_decl_ops : n_decl_pair)++;
            if (depth_max > FW_FUSE_MAX) (!v.depth ? n_far_decl_depth : !v.rings ? n_decl_ring : !v.ops ? n_far_decl_ops : n_far_decl_pair)++;
        }
        if (group && !candidate) n_noncand_flush++;
        CHECK((o.first != nullptr) == group, "a declined frame sends the group out first", d);
        if (o.first && group) check_launch(*o.first, pending, true);
        pending.clear();
        if (candidate) {
            CHECK(o.withheld && o.second == nullptr, "a candidate that did not join starts a group");
            pending.push_back(me);
            n_withheld_new++;
        } else {
            CHECK(!o.withheld && o.second == &B, "a non-candidate is never withheld");
            pending.push_back(me);
            if (o.second) check_launch(*o.second, pending, false);
            pending.clear();
            n_alone++;
        }
    }
    CHECK(W.depth() == pending.size(), "pending depth", W.depth(), (long long)pending.size());
}
static void last_take(FwWithheld &W) {  // the rest goes to whoever reads last
    const FwFifoLaunch *L = W.take();
    CHECK((L != nullptr) == !pending.empty(), "the last take");
    if (L && !pending.empty()) check_launch(*L, pending, true);
    pending.clear();
}

static void host(uint64_t seed, uint32_t steps, uint64_t &frame);  // the program's own
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const uint32_t seeds = (uint32_t)atoi(argv[1]), steps = (uint32_t)atoi(argv[2]);
    uint64_t frame = 0;
    ran.assign(1, 0);
    for (uint32_t s = 1; s <= seeds; s++) host(s, steps, frame);
    unsigned long long n_dropped = 0;
    for (uint64_t f = 1; f <= frame; f++) {
        if (ran[f] < 0) n_dropped++;
        else CHECK(ran[f] == 1, "every offered frame is run by exactly one launch", (long long)f, ran[f]);
    }
    CHECK(n_frames_run + n_dropped == frame, "frames", (long long)n_frames_run, (long long)frame);
    printf("total offers %llu launches %llu frames_run %llu dropped %llu withheld_new %llu joined_withheld %llu", n_offers, n_launches, n_frames_run, n_dropped, n_withheld_new,
           n_joined_withheld);
    for (uint32_t d = 2; d <= FW_FUSE_FAR; d++) printf(" closed%u %llu", d, n_closed[d]);
    for (uint32_t d = 1; d < FW_FUSE_FAR; d++) printf(" take%u %llu", d, n_take[d]);
    printf(" declined_pair %llu declined_ops %llu declined_ring %llu declined_depth %llu far_declined_pair %llu far_declined_ops %llu far_declined_depth %llu noncandidate_flush %llu "
           "alone %llu take_empty %llu drop_pending %llu drop_empty %llu depth_changed_inside %llu ops_merged %llu ops_kept_far %llu far_words %llu grew_into_far %llu bad %llu\n",
           n_decl_pair, n_decl_ops, n_decl_ring, n_decl_depth, n_far_decl_pair, n_far_decl_ops, n_far_decl_depth, n_noncand_flush, n_alone, n_take_empty, n_drop_pending,
           n_drop_empty, n_depth_changed_inside, n_ops_merged, n_ops_kept_far, n_far_words, n_grew_into_far, n_bad);
    return n_bad ? 1 : 0;
}
"""


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


def program_fixture(name, source, host_hipcc=False):
    """A module-scoped fixture that compiles `source` as a stand-alone program, once plainly and once with -fsanitize=address,undefined,
    and yields (path of the program, "0" for the plain build or "1" for the sanitizer build -- programs that take a `quick` argument walk
    less under the sanitizer: every path of the program).  host_hipcc: the program includes fw_withheld.h, whose fw_kernels.h g++ -Wall
    -Werror does not take alone (`#pragma unroll` in the device headers it includes): compiled host-side by the Makefile's hipcc as plain
    C++ (-x c++: no device code, no HIP call); otherwise g++."""

    @pytest.fixture(scope="module", params=["plain", "address,undefined"])
    def program(request, tmp_path_factory):
        d = tmp_path_factory.mktemp(name)
        (d / (name + ".cpp")).write_text(source)
        exe = d / name
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
        cc = [_hipcc(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] if host_hipcc else ["g++"]
        subprocess.check_call(cc + ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / (name + ".cpp")), "-o", str(exe)])
        return str(exe), ("0" if request.param == "plain" else "1")

    return program


def run(exe, args, timeout):
    """Run the program: no line says BAD, it exits with 0 and its last line's `bad` is 0.  -> (the lines, the last line's name / count pairs)"""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:30]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0
    return lines, total
