"""The withheld group of FIFO launches without a GPU (csrc/fw_withheld.h: FwWithheld -- offer, take, drop -- and FwFifoLaunch; the lines
launch_fifo and flush_withheld compile).  A stand-alone C++ program with its own main drives the group through random hosts
from fixed seeds: 1, 2 and FW_FIFO_PER_LAUNCH rings of 2 to 4 FW_TILE slots, 0 to 3 ops per ring and frame, spawn and death counts that now
and then break the pair rule, rings whose record changes between two frames, candidates and non-candidates, a depth_max of 2,
FW_FUSE_NARROW or FW_FUSE_MAX (and, less often, any depth the FW_FUSE_DEPTH knob can ask for: a group closes at depth_max exactly, and
every depth from 2 to 8 must be seen to close) that sometimes changes inside a group, readers (take) and drops at random.  Beside the
group the program keeps a model in its own words -- the plain list of the frames offered since the last launch, each as it was built --
and says from it what every offer must do (join, close, decline and why) and what every launch that comes out must hold: its frames,
each exactly once and in order; fused, dt, dt_pre, parity; per ring the first frame's head and live count, the summed spawns and dead, the
boundaries of FwFuseArgs, the layout fw_fifo_layout gives for the sums, cumulative tile_first; the ops ring by ring in frame order with
rel_base shifted by the earlier frames' new particles; a withheld frame that goes alone memcmp-equal to the launch as built, apart from
host_counts == nullptr.  The run fails unless every outcome occurred: joined and withheld, closed at each depth 2 to 8, declined by the
pair rule alone, by the ops limit alone, by a ring mismatch alone, by depth_max alone, a non-candidate flushing a group, take at each
pending depth 1 to 7 and on an empty group, drop with a group pending.
fw_kernels.h does not compile alone under g++ -Wall -Werror (`#pragma unroll` in the device headers it includes), so the program is
compiled host-side by the Makefile's hipcc as plain C++ (-x c++: no device code, no HIP call) -- once plainly, once with
-fsanitize=address,undefined -- and run directly: nothing is loaded into Python, nothing is preloaded."""
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
static_assert(FW_FUSE_MAX == 8 && FW_FUSE_NARROW == 4 && FW_INLINE_OPS == 8, "the depths and the ops limit this program counts");
static uint64_t rng;
static uint32_t rnd(uint32_t n) {  // 0 .. n - 1 (xorshift64*)
    rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
    return (uint32_t)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static unsigned long long n_bad, n_offers, n_withheld_new, n_joined_withheld, n_closed[FW_FUSE_MAX + 1], n_decl_pair, n_decl_ops, n_decl_ring, n_decl_depth,
    n_noncand_flush, n_alone, n_take[FW_FUSE_MAX], n_take_empty, n_drop_pending, n_drop_empty, n_depth_changed_inside, n_launches, n_frames_run;
static uint64_t cur_seed, cur_step;
static void bad(const char *what, long long x = 0, long long y = 0) {
    if (n_bad++ < 30) printf("BAD seed %llu step %llu: %s (%lld, %lld)\n", (unsigned long long)cur_seed, (unsigned long long)cur_step, what, x, y);
}
#define CHECK(cond, ...) do { if (!(cond)) bad(__VA_ARGS__); } while (0)

// the host: rings as a FIFO ring's host keeps them
struct Ring { uint32_t capacity, head, live, type_idx, keys_off, keys_len; float life; char *buf; };
// the model: the frames offered since the last launch, each as it was built
struct Offered { uint64_t frame; uint32_t depth_max; FwFifoLaunch built; };
static std::vector<Offered> pending;
static std::vector<int> ran;  // per frame number: launches that ran it; -1: dropped
static uint64_t last_run;     // the latest frame a launch ran (frames and launches stay in order)

// what a launch that runs the frames `m` must hold.  held: it comes out of the group (take, or the `first` of an offer)
static void check_launch(const FwFifoLaunch &L, const std::vector<Offered> &m, bool from_group) {
    const uint32_t D = (uint32_t)m.size();
    n_launches++;
    CHECK(D >= 1u && D <= FW_FUSE_MAX && L.depth == D, "depth", L.depth, D);
    if (D < 1u || D > FW_FUSE_MAX) return;
    const FwFifoLaunch &first = m[0].built, &last = m[D - 1].built;
    for (uint32_t f = 0; f < D; f++) {
        CHECK(L.frame[f] == m[f].frame, "frame number", (long long)L.frame[f], (long long)m[f].frame);
        CHECK(m[f].frame > last_run && ran[m[f].frame] == 0, "a frame runs once, in order", (long long)m[f].frame, ran[m[f].frame]);
        ran[m[f].frame]++, last_run = m[f].frame, n_frames_run++;
    }
    CHECK(D <= m[D - 1].depth_max, "deeper than the depth_max offered with the last frame", D, m[D - 1].depth_max);
    CHECK(L.fa.fused == (D == 1u ? 0u : D), "fused", L.fa.fused, D);
    CHECK(memcmp(&L.fa.dt, &last.fa.dt, 4) == 0, "dt is the last frame's");
    for (uint32_t f = 0; f + 1 < D; f++) CHECK(memcmp(&L.fz.dt_pre[f], &m[f].built.fa.dt, 4) == 0, "dt_pre", f);
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
        uint32_t spawn = 0, dead = 0;
        CHECK(F.op0 == o, "ops are grouped per ring", F.op0, o);
        for (uint32_t f = 0; f < D; f++) {
            const FwFifoSeg &X = m[f].built.fa.s[j];
            for (uint32_t x = X.op0; x < X.op1 && o < FW_INLINE_OPS; x++, o++) {
                FwOp want = m[f].built.fio.ops[x];
                want.rel_base += spawn;  // (the new particles of the earlier frames of this ring sit in front)
                CHECK(memcmp(&L.fio.ops[o], &want, sizeof want) == 0, "op", j, o);
            }
            spawn += X.n_spawn, dead += X.dead;
            if (f + 1 < D) CHECK(L.fz.spawn_end[j][f] == spawn && L.fz.dead[j][f] == X.dead, "the boundaries of FwFuseArgs", j, f);
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

// may B join the frames of `pending`?  Each of the four conditions by itself
struct Verdict { bool depth, rings, ops, pair; bool all() const { return depth && rings && ops && pair; } int failed() const { return !depth + !rings + !ops + !pair; } };
static Verdict judge(const FwFifoLaunch &B, uint32_t depth_max) {
    Verdict v{true, true, true, true};
    const uint32_t d = (uint32_t)pending.size();
    v.depth = d < depth_max && d < FW_FUSE_MAX;
    const FwFifoLaunch &P = pending.back().built;
    uint32_t ops = B.n_ops;
    for (const Offered &f : pending) ops += f.built.n_ops;
    v.ops = ops <= FW_INLINE_OPS;
    v.rings = P.fa.n_segs == B.fa.n_segs && P.fa.write_mask == B.fa.write_mask;
    for (uint32_t j = 0; v.rings && j < B.fa.n_segs; j++) {
        const FwFifoSeg &A = P.fa.s[j], &F = B.fa.s[j];
        v.rings = A.buf == F.buf && A.seg == F.seg && A.capacity == F.capacity && A.type_idx == F.type_idx && A.keys_off == F.keys_off && A.keys_len == F.keys_len &&
                  A.life == F.life && !A.mat && !F.mat && !A.destroyed && !F.destroyed && !A.nest && !F.nest;
    }
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

static void new_rings(std::vector<Ring> &rings, uint32_t n) {
    rings.resize(n);
    for (uint32_t j = 0; j < n; j++) {
        Ring &R = rings[j];
        R.capacity = (2u + rnd(3)) * FW_TILE, R.head = rnd(R.capacity), R.live = R.capacity / 4u + rnd(R.capacity / 2u);
        R.type_idx = rnd(16), R.keys_off = rnd(64), R.keys_len = 1u + rnd(8), R.life = 1.0f + (float)rnd(8);
        R.buf = (char *)(uintptr_t)(0x100000u * (1u + rnd(1000)) + j * 0x1000u);
    }
}

static void host(uint64_t seed, uint32_t steps, uint64_t &frame) {
    rng = seed * 0x9E3779B97F4A7C15ull + 1u, cur_seed = seed;
    static FwWithheld W;
    W.drop(), pending.clear();
    const uint32_t ring_counts[3] = {1u, 2u, FW_FIFO_PER_LAUNCH};
    const uint32_t n_rings = ring_counts[seed % 3u];
    const uint32_t op_rate = 2u + rnd(4u * n_rings);  // one ring in op_rate carries ops in a frame
    std::vector<Ring> rings;
    new_rings(rings, n_rings);
    uint32_t depth_max = 2u;
    int32_t write_mask = 0;
    static unsigned long long counts_word;
    for (uint32_t step = 0; step < steps; step++) {
        cur_step = step;
        const uint32_t what = rnd(100);
        if (what < 5u) {  // somebody reads
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
            continue;
        }
        if (what < 7u) {  // the particles go, and a withheld frame with them
            W.drop();
            (pending.empty() ? n_drop_empty : n_drop_pending)++;
            for (const Offered &f : pending) ran[f.frame] = -1;
            pending.clear();
            new_rings(rings, n_rings);
            CHECK(W.depth() == 0u && W.take() == nullptr, "nothing is pending behind a drop");
            continue;
        }
        // ---- a frame: built as launch_fifo builds it, all of its bookkeeping done
        if (step == 0u || rnd(12) == 0u) {
            const uint32_t r = rnd(10);
            const uint32_t nd = r < 3u ? 2u : r < 5u ? (uint32_t)FW_FUSE_NARROW : r < 8u ? (uint32_t)FW_FUSE_MAX : 2u + rnd(FW_FUSE_MAX - 1u);
            if (nd != depth_max && !pending.empty()) n_depth_changed_inside++;
            depth_max = nd;
        }
        if (rnd(40) == 0u) write_mask = (int32_t)rnd(9) - 1;
        if (rnd(25) == 0u) {  // a ring's record changes for good (an axis rule that ends, a type that is rebuilt)
            Ring &R = rings[rnd(n_rings)];
            switch (rnd(5)) {
            case 0: R.type_idx ^= 1u << rnd(8); break;
            case 1: R.keys_off += 1u; break;
            case 2: R.keys_len += 1u; break;
            case 3: R.life += 0.5f; break;
            default: R.buf += 0x10000; break;
            }
        }
        static FwFifoLaunch B;
        memset(&B, 0, sizeof B);
        FwFifoArgs &fa = B.fa;
        frame++;
        ran.resize(frame + 1u, 0);
        fa.n_segs = n_rings, fa.parity = (uint32_t)(frame & 1u), fa.epoch = (uint32_t)frame, fa.write_mask = write_mask, fa.spinless = 1u, fa.q0pl = 1u;
        fa.dt = (float)(1u + rnd(1000)) / 32768.0f + (float)rnd(1000) * 1e-7f;
        fa.host_counts = &counts_word;
        fa.fuse_pad[FW_FIFO_NEWBORN] = 1u;
        B.nt = (int)rnd(3);
        for (uint32_t j = 0; j < n_rings; j++) {
            Ring &R = rings[j];
            FwFifoSeg &F = fa.s[j];
            const uint32_t room = R.capacity - R.live;
            uint32_t k_ops = rnd(op_rate) == 0u ? 1u + rnd(3) : 0u;
            k_ops = std::min(k_ops, FW_INLINE_OPS - B.n_ops);
            F.op0 = B.n_ops;
            uint32_t n_spawn = 0;
            for (uint32_t k = 0; k < k_ops; k++) {
                FwOp op{};
                // (mostly a few new particles, so that groups grow deep; now and then as many as the ring has room for, and more than a group can take)
                op.n = std::min(room - n_spawn, rnd(20) == 0u ? rnd(room + 1u) : rnd(6));
                op.seg = j, op.emit = rnd(100), op.rel_base = n_spawn, op.serial_base = frame << 16 | j << 8 | k, op.head = R.head;
                op.origin_pos[0] = (float)frame, op.speed = (float)k, op.scale = 1.0f;
                n_spawn += op.n;
                B.fio.ops[B.n_ops++] = op;
            }
            F.op1 = B.n_ops;
            const uint32_t all = R.live + n_spawn;
            // (mostly a few of the oldest die; now and then anything up to everybody, the frame's own newborns included)
            const uint32_t dead = rnd(25) == 0u ? rnd(all + 1u) : std::min(all, rnd(3) ? 0u : rnd(5));
            F.buf = R.buf, F.seg = j, F.capacity = R.capacity, F.type_idx = R.type_idx, F.keys_off = R.keys_off, F.keys_len = R.keys_len, F.life = R.life;
            F.head = R.head, F.n_in = R.live, F.n_spawn = n_spawn, F.dead = dead;
            // (now and then a frame no group may hold: materialised spawns, destroyed records, a Nested entry)
            if (rnd(60) == 0u) {
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
        const bool candidate = rnd(8) != 0u;
        Offered me{frame, depth_max, B};
        // ---- what the offer must do, from the model
        const bool group = !pending.empty();
        Verdict v{true, true, true, true};
        if (group) v = judge(B, depth_max);
        const bool joins = group && candidate && v.all();
        const uint32_t d = (uint32_t)pending.size();
        n_offers++;
        const FwOffered o = W.offer(B, candidate, depth_max, frame);
        if (joins) {
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
            if (group && candidate && v.failed() == 1) (!v.depth ? n_decl_depth : !v.rings ? n_decl_ring : !v.ops ? n_decl_ops : n_decl_pair)++;
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
    // the rest goes to whoever reads last
    const FwFifoLaunch *L = W.take();
    CHECK((L != nullptr) == !pending.empty(), "the last take");
    if (L && !pending.empty()) check_launch(*L, pending, true);
    pending.clear();
}

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
    printf("total offers %llu launches %llu frames_run %llu dropped %llu withheld_new %llu joined_withheld %llu closed2 %llu closed3 %llu closed4 %llu closed5 %llu closed6 %llu "
           "closed7 %llu closed8 %llu declined_pair %llu declined_ops %llu declined_ring %llu declined_depth %llu noncandidate_flush %llu alone %llu take1 %llu take2 %llu "
           "take3 %llu take4 %llu take5 %llu take6 %llu take7 %llu take_empty %llu drop_pending %llu drop_empty %llu depth_changed_inside %llu bad %llu\n",
           n_offers, n_launches, n_frames_run, n_dropped, n_withheld_new, n_joined_withheld, n_closed[2], n_closed[3], n_closed[4], n_closed[5], n_closed[6], n_closed[7],
           n_closed[8], n_decl_pair, n_decl_ops, n_decl_ring, n_decl_depth, n_noncand_flush, n_alone, n_take[1], n_take[2], n_take[3], n_take[4], n_take[5], n_take[6],
           n_take[7], n_take_empty, n_drop_pending, n_drop_empty, n_depth_changed_inside, n_bad);
    return n_bad ? 1 : 0;
}
"""

SEEDS, STEPS = 48, 4000  # (chosen on the CPU so that the model alone meets the coverage condition below, with a margin)


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("withheld")
    (d / "withheld.cpp").write_text(PROGRAM)
    exe = d / "withheld"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([_hipcc(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                           "-I", CSRC] + flags + [str(d / "withheld.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_withheld_group_under_random_hosts(program):
    r = subprocess.run([program, str(SEEDS), str(STEPS)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:30]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0
    assert total["frames_run"] + total["dropped"] == total["offers"] > 100000
    # every outcome occurred
    for k in (["withheld_new", "joined_withheld"] + ["closed%d" % d for d in range(2, 9)] +
              ["declined_pair", "declined_ops", "declined_ring", "declined_depth", "noncandidate_flush", "alone"] +
              ["take%d" % d for d in range(1, 8)] + ["take_empty", "drop_pending", "depth_changed_inside"]):
        assert total[k] >= 10, (k, total)
