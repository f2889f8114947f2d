"""Two frames of a FIFO ring in one launch without a GPU (csrc/fw_fuse2.h: the layout of a launch, the rule that admits a pair, the fused
frame -- the lines FwWithheld::join, csrc/fw_withheld.h, and launch_fifo compile): a stand-alone C++ program, compiled here with g++ -- once plainly, once with
-fsanitize=address,undefined --, walks a reduced model of the kernel's grid (tiles of 4 slots, spawning workgroups of 2) slot by slot.
For every capacity that is a multiple of the tile, every head, live count and every {spawn_A, dead_A, spawn_B, dead_B} two frames can
carry, it asks fw_fuse2_ok; for every pair the rule admits it runs frame A and frame B as two launches and the fused frame as one, and
compares: the same live slots, each holding the same particle with the same number of updates and the same dt sequence, each stored
exactly once by the fused launch, the same head and count, every live particle covered, and no slot both read as an old particle and
written as a new one.  The rule itself is stated a second time, in the test's own words, and must agree for every combination: a pair in
which a newborn dies, or whose newborns do not fit beside A's dead, is declined.  A Python brute force counts the small capacities again."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
TILE, BLOCK = 4, 2

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fw_fuse2.h"
static const uint32_t TILE = 4, BLOCK = 2;
struct Slot { int id, n_upd, hist, stores; };  // id -1: no live particle; hist: the dt sequence in base 3 (1 = dt_A, 2 = dt_B)
static unsigned long long n_bad = 0;
static void bad(const char *what, uint32_t C, const FwFifoFrame &A, const FwFifoFrame &B) {
    if (n_bad++ < 20) printf("BAD %s: C %u A {%u %u %u %u} B {%u %u %u %u}\n", what, C, A.head, A.n_in, A.n_spawn, A.dead, B.head, B.n_in, B.n_spawn, B.dead);
}
// one launch over the ring, the way fw_k_update_fifo walks it: ring tiles from tile0, then (in the model: order does not matter, the
// slots are disjoint or the run is BAD) the two groups of spawning workgroups.  split: new particles [0, split) are frame A's and get
// dt_first too (the fused launch); id_a / id_b: what the new particles of either frame are called.  false: the walk broke a rule
static bool launch(std::vector<Slot> &ring, uint32_t C, const FwFifoFrame &F, uint32_t split, int dt_first, int dt, int id_a, int id_b, bool fused) {
    const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, F.head, F.dead < F.n_in ? F.dead : F.n_in, F.n_in, F.n_in, F.n_spawn);
    const uint32_t ring_tiles = C / TILE;
    if (L.live_tiles > ring_tiles || L.n_tiles < 1u) return false;
    uint32_t covered = 0;
    for (uint32_t t = 0; t < L.live_tiles; t++) {
        const uint32_t pt = (L.tile0 + t) % ring_tiles;
        for (uint32_t s = pt * TILE; s < (pt + 1) * TILE; s++) {
            const uint32_t i = (s + C - F.head) % C;
            if (!(i < F.n_in && i >= F.dead)) continue;
            Slot &x = ring[s];
            if (x.id < 0) return false;  // (a live index without a particle)
            if (fused) x.n_upd++, x.hist = x.hist * 3 + dt_first;
            x.n_upd++, x.hist = x.hist * 3 + dt, x.stores++;
            covered++;
        }
    }
    if (covered != F.n_in - (F.dead < F.n_in ? F.dead : F.n_in)) return false;  // every survivor, once
    for (uint32_t wg = 0; wg < L.n_vt_a + L.n_vt_b; wg++) {
        const uint32_t k0 = wg < L.n_vt_a ? wg * BLOCK : L.spawn_a + (wg - L.n_vt_a) * BLOCK, k_end = wg < L.n_vt_a ? L.spawn_a : F.n_spawn;
        const uint32_t sbase = (F.head + F.n_in + k0) % C;
        for (uint32_t tid = 0; tid < BLOCK; tid++) {
            const uint32_t k = k0 + tid, s = sbase + tid;
            if (k >= k_end) continue;
            if (s >= C) return false;  // (a group's slots are consecutive: the split at the ring's end)
            if (F.n_in + k < F.dead) continue;  // born and destroyed in the frame
            Slot &x = ring[s];
            // (no slot both read as an old particle and written as a new one: the slot's logical index lies behind the old particles)
            if ((s + C - F.head) % C < F.n_in || x.id >= 0) return false;
            x = Slot{k < split ? id_a + (int)k : id_b + (int)(k - split), 0, 0, x.stores + 1};
            if (k < split) x.n_upd++, x.hist = x.hist * 3 + dt_first;
            x.n_upd++, x.hist = x.hist * 3 + dt;
        }
    }
    for (uint32_t i = 0; i < F.dead && i < F.n_in + F.n_spawn; i++) ring[(F.head + i) % C].id = -1;
    return true;
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const uint32_t max_cap = (uint32_t)atoi(argv[1]);
    unsigned long long admitted = 0, declined = 0, newborn_dies = 0, no_room = 0;
    for (uint32_t C = TILE; C <= max_cap; C += TILE) {
        unsigned long long adm_c = 0, dec_c = 0;
        for (uint32_t head = 0; head < C; head++)
        for (uint32_t n_in = 0; n_in <= C; n_in++)
        for (uint32_t sa = 0; n_in + sa <= C; sa++)
        for (uint32_t da = 0; da <= n_in + sa; da++) {
            const FwFifoFrame A{head, n_in, sa, da};
            const uint32_t nb = n_in + sa - da, hb = (head + da) % C;
            for (uint32_t sb = 0; nb + sb <= C; sb++)
            for (uint32_t db = 0; db <= nb + sb; db++) {
                const FwFifoFrame B{hb, nb, sb, db};
                const bool ok = fw_fuse2_ok(C, A, B);
                // the rule in the test's own words: nobody born in the pair dies in it; both frames' newborns fit behind A's live
                // particles without reaching a slot A's dead still occupy in the fused view
                const bool dies = da + db > n_in, room = n_in + sa + sb <= C;
                if (ok != (!dies && room)) bad("rule", C, A, B);
                newborn_dies += dies, no_room += !room;
                if (!ok) { dec_c++; continue; }
                adm_c++;
                std::vector<Slot> two(C, Slot{-1, 0, 0, 0}), one(C, Slot{-1, 0, 0, 0});
                for (uint32_t i = 0; i < n_in; i++) two[(head + i) % C] = one[(head + i) % C] = Slot{(int)i, 0, 0, 0};
                if (!launch(two, C, A, 0, 0, 1, 0, 1000, false) || !launch(two, C, B, 0, 0, 2, 0, 2000, false)) { bad("two launches", C, A, B); continue; }
                const FwFifoFrame U = fw_fuse2_frame(A, B);
                if (!launch(one, C, U, sa, 1, 2, 1000, 2000, true)) { bad("fused launch", C, A, B); continue; }
                const uint32_t head2 = (hb + db) % C, n2 = nb + sb - db;
                if ((U.head + U.dead) % C != head2 || U.n_in + U.n_spawn - U.dead != n2) bad("head / count", C, A, B);
                uint32_t live = 0;
                for (uint32_t s = 0; s < C; s++) {
                    const bool in = (s + C - head2) % C < n2;
                    if (in != (two[s].id >= 0) || in != (one[s].id >= 0)) { bad("live set", C, A, B); break; }
                    if (!in) {
                        if (one[s].stores) { bad("a store outside the live set", C, A, B); break; }
                        continue;
                    }
                    live++;
                    if (one[s].id != two[s].id || one[s].n_upd != two[s].n_upd || one[s].hist != two[s].hist) { bad("particle", C, A, B); break; }
                    if (one[s].stores != 1) { bad("stored once", C, A, B); break; }
                }
                if (live != n2) bad("count", C, A, B);
            }
        }
        printf("C %u admitted %llu declined %llu\n", C, adm_c, dec_c);
        admitted += adm_c, declined += dec_c;
    }
    // the rule's switch (fw_ctx::use_fuse2, FW_FUSE2=0): off, no launch is a candidate whatever else holds
    unsigned cand_on = 0, cand_off = 0;
    for (unsigned m = 0; m < 16; m++) {
        cand_on += fw_fuse2_candidate(true, m & 1, m & 2, m & 4, m & 8);
        cand_off += fw_fuse2_candidate(false, m & 1, m & 2, m & 4, m & 8);
    }
    printf("candidates on %u off %u\n", cand_on, cand_off);
    printf("total admitted %llu declined %llu newborn_dies %llu no_room %llu bad %llu\n", admitted, declined, newborn_dies, no_room, n_bad);
    return n_bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("fuse2")
    (d / "fuse2.cpp").write_text(PROGRAM)
    exe = d / "fuse2"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "fuse2.cpp"), "-o", str(exe)])
    # (the sanitizer build walks the capacities up to 16: every path of the program, a twentieth of the combinations)
    return str(exe), (32 if request.param == "plain" else 16)


def _brute(C):
    """admitted / declined pairs of a ring of C slots, counted from the rule's two sentences alone (the head does not enter them)"""
    adm = dec = 0
    for n_in in range(C + 1):
        for sa in range(C - n_in + 1):
            for da in range(n_in + sa + 1):
                nb = n_in + sa - da
                for sb in range(C - nb + 1):
                    for db in range(nb + sb + 1):
                        if da + db <= n_in and n_in + sa + sb <= C:
                            adm += 1
                        else:
                            dec += 1
    return adm * C, dec * C


def test_every_pair_of_frames_of_a_small_ring(program):
    exe, max_cap = program
    r = subprocess.run([exe, str(max_cap)], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:20]
    assert r.returncode == 0, r.stderr[-2000:]
    per_cap = {int(ln.split()[1]): (int(ln.split()[3]), int(ln.split()[5])) for ln in lines if ln.startswith("C ")}
    assert sorted(per_cap) == list(range(TILE, max_cap + 1, TILE))
    for C in (4, 8, 12):
        assert per_cap[C] == _brute(C), (C, per_cap[C])
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0 and total["admitted"] == sum(a for a, _ in per_cap.values()) > 10000
    # every kind of pair the rule must decline occurred, and all of them were declined (the program compares rule and model pair by pair)
    assert total["newborn_dies"] > 0 and total["no_room"] > 0 and total["declined"] >= max(total["newborn_dies"], total["no_room"])
    assert lines[-2] == "candidates on 1 off 0"  # (FW_FUSE2=0: no launch is ever withheld)
