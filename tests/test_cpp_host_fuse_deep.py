"""Groups of three and four frames of a FIFO ring in one launch without a GPU (csrc/fw_fuse2.h: FwFuseGroup, fw_fuse_begin, fw_fuse_push --
the lines FwWithheld::join (csrc/fw_withheld.h) and launch_fifo compile).  A stand-alone C++ program, compiled with g++ -Wall -Werror -- once plainly,
once with -fsanitize=address,undefined --, walks a reduced model of the kernel's grid (tiles of 4 slots, spawning workgroups of 2) slot by
slot.  For rings of 8 to 64 slots it walks sequences of up to four frames {spawn, dead} from every head and live count -- all of them for
the small rings, a grid of values that keeps the edges (0, 1, a tile + 1, a third, all but one, everything that fits) for the larger ones --
and steps them one by one over an explicit ring of slots.  The fold must admit a frame exactly when stepping it met none of: a particle
born in the group dying in it, a new particle landing on a slot that held a particle when the group began (the fused view has not
vacated it), a frame that does not continue the one before.  For every admitted group of three and four frames the fused launch -- the
layout fw_fifo_layout gives for the folded frame, each new particle's frame taken from the cumulative bounds, the counters by the
kernel's arithmetic -- must agree with the frames stepped one by one: the slots stored (each live slot exactly once, nothing else), the
updates every slot's particle received and their dt sequence, both count rows, the destroyed count and the statistics.  Wrapped heads,
frames that spawn nothing and frames that destroy nothing are counted, and must all have occurred."""
import os
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
#include "fw_fuse2.h"
static const uint32_t TILE = 4, BLOCK = 2;
struct Slot { int id, born, n_upd; long hist; int stores; };  // id -1: empty; born -1: in the ring before the group; hist: the frames that updated it, base 5
struct Frame { uint32_t spawn, dead; };
static unsigned long long n_bad = 0, n_groups[5], n_declined[5], n_newborn_dies, n_overflow, n_discont, n_wrapped_head, n_wrapped_spawn, n_spawn0, n_dead0, n_no_tile;
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
        x.n_upd++, x.hist = x.hist * 5 + (f + 1);
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
// the fused launch of a group of D frames: what the kernel's workgroups do with FwFifoSeg {U} and FwFuseArgs {spawn_end, dead}
static bool fused(const FwFuseGroup &G, uint32_t C, uint32_t D, std::vector<Slot> &ring, uint32_t rows[2], uint32_t parity, uint32_t *ndestroyed, unsigned long long *stats) {
    const FwFifoFrame &U = G.U;
    const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
    const uint32_t ring_tiles = C / TILE;
    if (L.live_tiles > ring_tiles || L.n_tiles < 1u) return false;
    if (L.live_tiles == 0) n_no_tile++;
    uint32_t covered = 0;
    for (uint32_t t = 0; t < L.live_tiles; t++) {
        const uint32_t pt = (L.tile0 + t) % ring_tiles;
        for (uint32_t s = pt * TILE; s < (pt + 1) * TILE; s++) {
            const uint32_t i = (s + C - U.head) % C;
            if (!(i < U.n_in && i >= U.dead)) continue;
            Slot &x = ring[s];
            if (x.id < 0) return false;
            for (uint32_t f = 0; f < D; f++) x.n_upd++, x.hist = x.hist * 5 + (f + 1);  // dt_pre[0 .. D - 2] in order, then dt
            x.stores++, covered++;
        }
    }
    if (covered != U.n_in - U.dead) return false;
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
            for (uint32_t f = f0; f < D; f++) x.n_upd++, x.hist = x.hist * 5 + (f + 1);
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
static std::vector<uint32_t> values(uint32_t hi, bool all) {  // 0 .. hi, or the edges of it
    std::vector<uint32_t> v;
    if (all) { for (uint32_t x = 0; x <= hi; x++) v.push_back(x); return v; }
    const uint32_t c[] = {0, 1, TILE + 1, hi / 3, hi - std::min(hi, 1u), hi};
    for (uint32_t x : c) if (x <= hi) v.push_back(x);
    std::sort(v.begin(), v.end()), v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}
static void walk(uint32_t C, uint32_t head0, uint32_t n_in0, uint32_t parity0, Frame *fr, uint32_t d, const FwFuseGroup *G, const Stepped &S, bool all, uint32_t max_depth) {
    // frame d continues the group so far (d frames, admitted): every {spawn, dead} a frame of the ring can carry by itself
    for (uint32_t sp : values(C - S.count, all))
    for (uint32_t dd : values(S.count + sp, all)) {
        fr[d] = Frame{sp, dd};
        Stepped T = S;
        step(T, fr[d], (int)d);
        const FwFifoFrame B{S.head, S.count, sp, dd};
        FwFuseGroup H;
        bool ok;
        if (d == 0) H = fw_fuse_begin(B), ok = dd <= S.count;  // (a frame of its own: whatever the ring runs; a group needs its dead to be old particles)
        else H = *G, ok = fw_fuse_push(C, H, B);
        if (d == 0 && !ok) continue;
        const bool clean = !T.newborn_dies && !T.overflow;
        if (ok != clean) { bad("rule", C, head0, n_in0, fr, d + 1); continue; }
        n_newborn_dies += T.newborn_dies, n_overflow += T.overflow;
        if (!ok) { n_declined[d + 1]++; continue; }
        n_groups[d + 1]++;
        n_spawn0 += sp == 0, n_dead0 += dd == 0;
        if (d + 1 >= 3) {
            if (T.head < head0) n_wrapped_head++;
            compare(C, head0, n_in0, fr, d + 1, H, T, parity0);
        }
        if (d + 1 < max_depth) walk(C, head0, n_in0, parity0, fr, d + 1, &H, T, all, max_depth);
        else {  // a fifth frame never joins; a frame that does not continue the group is declined whatever else holds
            FwFuseGroup X = H;
            if (d + 1 == FW_FUSE_MAX && fw_fuse_push(C, X, FwFifoFrame{T.head, T.count, 0, 0})) bad("a fifth frame", C, head0, n_in0, fr, d + 1);
        }
        if (d + 1 < FW_FUSE_MAX) {
            FwFuseGroup X = H;
            if (fw_fuse_push(C, X, FwFifoFrame{(T.head + 1) % C, T.count, 0, 0}) && C > 1) bad("discontinuous head", C, head0, n_in0, fr, d + 1);
            X = H;
            if (T.count + 1 <= C && fw_fuse_push(C, X, FwFifoFrame{T.head, T.count + 1, 0, 0})) bad("discontinuous count", C, head0, n_in0, fr, d + 1);
            n_discont += 2;
        }
    }
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const bool quick = atoi(argv[1]) != 0;
    // every sequence for the smallest ring (three frames: 8 and 12 slots too); a grid of edge values for 16 to 64 slots
    struct Plan { uint32_t C; bool all; uint32_t depth; } plans[] = {{8, true, 4}, {12, true, 3}, {16, false, 4}, {20, false, 4}, {32, false, 4}, {64, false, 4}};
    for (const Plan &p : plans) {
        if (quick && (p.C == 12 || p.C == 32 || p.C == 64)) continue;
        const uint32_t C = p.C;
        for (uint32_t head : values(C - 1, p.all || C <= 20))
        for (uint32_t n_in : values(C, p.all)) {
            Stepped S;
            S.ring.assign(C, Slot{-1, -1, 0, 0, 0}), S.orig.assign(C, 0);
            for (uint32_t i = 0; i < n_in; i++) S.ring[(head + i) % C] = Slot{(int)i, -1, 0, 0, 0}, S.orig[(head + i) % C] = 1;
            const uint32_t parity0 = (head + n_in) & 1u;
            S.C = C, S.head = head, S.count = n_in, S.parity = parity0, S.rows[parity0] = n_in, S.rows[parity0 ^ 1u] = 0xDEADu, S.ndestroyed = 0, S.stats = 0;
            S.newborn_dies = S.overflow = false;
            Frame fr[FW_FUSE_MAX];
            walk(C, head, n_in, parity0, fr, 0, nullptr, S, p.all, p.depth);
        }
        printf("C %u groups of two %llu three %llu four %llu\n", C, n_groups[2], n_groups[3], n_groups[4]);
    }
    printf("total three %llu four %llu declined %llu newborn_dies %llu overflow %llu discontinuous %llu wrapped_head %llu wrapped_spawn %llu spawn0 %llu dead0 %llu no_tile %llu bad %llu\n",
           n_groups[3], n_groups[4], n_declined[2] + n_declined[3] + n_declined[4], n_newborn_dies, n_overflow, n_discont, n_wrapped_head, n_wrapped_spawn, n_spawn0, n_dead0, n_no_tile, n_bad);
    return n_bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("fuse_deep")
    (d / "fuse_deep.cpp").write_text(PROGRAM)
    exe = d / "fuse_deep"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "fuse_deep.cpp"), "-o", str(exe)])
    # (the sanitizer build walks half of the rings: every path of the program)
    return str(exe), ("0" if request.param == "plain" else "1")


def test_every_group_of_three_and_four_frames_of_small_rings(program):
    exe, quick = program
    r = subprocess.run([exe, quick], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:20]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0
    assert total["three"] > 10000 and total["four"] > 10000
    # everything the rule must decline occurred and was declined (the program compares rule and stepping frame by frame), and the
    # admitted groups include wrapped heads, new particles that wrap the buffer's end, frames that spawn or destroy nothing, and launches
    # without a ring tile (every old particle dies in the group)
    for k in ("declined", "newborn_dies", "overflow", "discontinuous", "wrapped_head", "wrapped_spawn", "spawn0", "dead0", "no_tile"):
        assert total[k] > 0, (k, total)
