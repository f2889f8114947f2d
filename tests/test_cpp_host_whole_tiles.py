"""Whole ring tiles without a GPU (csrc/fw_fuse2.h: fw_fifo_tile_whole -- the lines the FIFO ring kernel and launch_fifo compile;
DESIGN.md 4.0, round 26).  A stand-alone C++ program in the manner of tests/test_cpp_host_fuse_wide.py, compiled with g++ -Wall -Werror --
once plainly, once with -fsanitize=address,undefined --, over rings of 2 to 6 tiles of 8 slots: every head, every live count, every number
of dead, as a frame of its own and as the fused frame of groups built with fw_fuse_push.  Per case: the predicate is true for a ring tile
exactly when brute force over the tile's slots finds every logical index in [dead, n_in); the tiles fw_fifo_layout dispatches (from
tile0, live_tiles of them, the tile index wrapping at the ring's end) are distinct and cover every live slot; and a tile the launch does
not dispatch holds no particle that lives through it.  The totals must show both answers for dispatched ranges that wrap the ring's end
and for ranges that do not, a whole tile in a ring whose head lies inside it, and whole tiles in groups of two to eight frames."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fw_fuse2.h"
static const uint32_t TILE = 8, BLOCK = 4;
static unsigned long long n_bad, n_cases, n_whole[2], n_part[2], n_head_inside, n_group_whole[FW_FUSE_MAX + 1], n_groups;
static void bad(const char *what, uint32_t C, const FwFifoFrame &U, uint32_t pt) {
    if (n_bad++ < 20) printf("BAD %s: C %u head %u n_in %u spawn %u dead %u tile %u\n", what, C, U.head, U.n_in, U.n_spawn, U.dead, pt);
}
// one launch of the frame U (a frame of its own, or a group's fused frame of `depth` frames)
static void check(uint32_t C, const FwFifoFrame &U, uint32_t depth) {
    const uint32_t ring_tiles = C / TILE;
    const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, U.head, U.dead, U.n_in, U.n_in, U.n_spawn);
    n_cases++;
    if (L.live_tiles > ring_tiles || L.tile0 >= ring_tiles) { bad("layout", C, U, L.tile0); return; }
    const bool wrapped = L.tile0 + L.live_tiles > ring_tiles;  // the dispatched tile range passes the ring's end
    std::vector<char> dispatched(ring_tiles, 0);
    uint32_t covered = 0;
    for (uint32_t t = 0; t < L.live_tiles; t++) {
        const uint32_t pt = (L.tile0 + t) % ring_tiles;
        if (dispatched[pt]++) bad("a tile dispatched twice", C, U, pt);
    }
    for (uint32_t pt = 0; pt < ring_tiles; pt++) {
        uint32_t live = 0;
        for (uint32_t s = pt * TILE; s < (pt + 1) * TILE; s++) {
            const uint32_t i = (s + C - U.head) % C;  // brute force: the slot's logical index
            live += (i >= U.dead && i < U.n_in) ? 1u : 0u;
        }
        const bool whole = fw_fifo_tile_whole(C, TILE, U.head, U.n_in, U.dead, pt);
        if (whole != (live == TILE)) bad("predicate", C, U, pt);
        if (!dispatched[pt]) {
            if (live) bad("a live slot in a tile nobody runs", C, U, pt);
            continue;
        }
        covered += live;
        (whole ? n_whole : n_part)[wrapped]++;
        if (whole && U.head > pt * TILE && U.head < (pt + 1) * TILE) n_head_inside++;
        if (whole) n_group_whole[depth]++;
    }
    if (covered != U.n_in - U.dead) bad("coverage", C, U, L.tile0);
}
int main() {
    for (uint32_t tiles = 2; tiles <= 6; tiles++) {
        const uint32_t C = tiles * TILE;
        // every frame of its own
        for (uint32_t head = 0; head < C; head++)
        for (uint32_t n_in = 0; n_in <= C; n_in++)
        for (uint32_t dead = 0; dead <= n_in; dead++)
            check(C, FwFifoFrame{head, n_in, (C - n_in) / 2u, dead}, 1u);
        // groups: every start, then frames that spawn sp and destroy dd each until the rule declines one
        for (uint32_t head = 0; head < C; head += 3u)
        for (uint32_t n_in = 0; n_in <= C; n_in++)
        for (uint32_t sp = 0; sp <= 3u; sp++)
        for (uint32_t dd = 0; dd <= 3u; dd++) {
            if (dd > n_in) continue;
            FwFifoFrame A{head, n_in, sp, dd};
            FwFuseGroup G = fw_fuse_begin(A);
            for (;;) {
                const FwFifoFrame B{(uint32_t)((G.U.head + G.U.dead) % C), G.U.n_in + G.U.n_spawn - G.U.dead, sp, dd + (G.depth & 1u)};
                if (!fw_fuse_push(C, G, B)) break;
                n_groups++;
                check(C, G.U, G.depth);
            }
        }
    }
    unsigned long long deep = 0;
    for (uint32_t d = 2; d <= FW_FUSE_MAX; d++) deep += n_group_whole[d] ? 1u : 0u;
    printf("total cases %llu groups %llu whole_unwrapped %llu whole_wrapped %llu part_unwrapped %llu part_wrapped %llu head_inside %llu depths_with_whole %llu bad %llu\n",
           n_cases, n_groups, n_whole[0], n_whole[1], n_part[0], n_part[1], n_head_inside, deep, n_bad);
    return n_bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("whole_tiles")
    (d / "whole_tiles.cpp").write_text(PROGRAM)
    exe = d / "whole_tiles"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "whole_tiles.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_predicate_against_brute_force_over_small_rings(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:20]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0 and total["cases"] > 10000 and total["groups"] > 1000
    # both answers, for dispatched tile ranges that wrap the ring's end and for ranges that do not
    for k in ("whole_unwrapped", "whole_wrapped", "part_unwrapped", "part_wrapped"):
        assert total[k] > 0, (k, total)
    # a full ring that loses nobody is whole even in the tile its head lies in; groups of every depth from two to eight met whole tiles
    assert total["head_inside"] > 0 and total["depths_with_whole"] == 7, total
