"""The whole tiles of a launch in closed form, without a GPU (csrc/fw_fuse2.h: fw_fifo_whole_span -- what launch_fifo's count_whole_tiles
calls instead of a walk over the tiles).  A stand-alone C++ program in the manner of
tests/test_cpp_host_whole_tiles.py, compiled with g++ -Wall -Werror -- once plainly, once with -fsanitize=address,undefined --, exhaustive
over rings of 4, 8, 12 and 32 slots in tiles of 4: every head (heads inside a tile included), every dead <= n_in <= capacity, and for the
dispatched tiles both every layout fw_fifo_layout can give (its first slot anywhere from the head to the first survivor) and every other
tile0 / live_tiles of the ring.  Per case: `count` is the brute-force count of fw_fifo_tile_whole over the dispatched tiles, and the run
first / len names exactly the ring tiles the predicate calls whole.  A count only the device knows (0xFFFFFFFF) has no whole tile."""
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
static const uint32_t TILE = 4, BLOCK = 2;
static unsigned long long n_bad, n_cases, n_layouts, n_some, n_all, n_none, n_head_inside, n_run_wraps, n_partial;
static void bad(const char *what, uint32_t C, uint32_t head, uint32_t n_in, uint32_t dead, uint32_t tile0, uint32_t live) {
    if (n_bad++ < 20) printf("BAD %s: C %u head %u n_in %u dead %u tile0 %u live_tiles %u\n", what, C, head, n_in, dead, tile0, live);
}
static void check(uint32_t C, uint32_t head, uint32_t n_in, uint32_t dead, uint32_t tile0, uint32_t live) {
    const uint32_t ring_tiles = C / TILE;
    const FwWholeSpan W = fw_fifo_whole_span(C, TILE, head, n_in, dead, tile0, live);
    uint32_t brute = 0, ring_whole = 0;
    for (uint32_t t = 0; t < live; t++) brute += fw_fifo_tile_whole(C, TILE, head, n_in, dead, (tile0 + t) % ring_tiles) ? 1u : 0u;
    n_cases++;
    if (W.count != brute) bad("count", C, head, n_in, dead, tile0, live);
    // the run: exactly the ring's whole tiles
    std::vector<char> in_run(ring_tiles, 0);
    if (W.len > ring_tiles || (W.len && W.first >= ring_tiles)) { bad("run", C, head, n_in, dead, tile0, live); return; }
    for (uint32_t i = 0; i < W.len; i++) in_run[(W.first + i) % ring_tiles]++;
    for (uint32_t pt = 0; pt < ring_tiles; pt++) {
        const bool whole = fw_fifo_tile_whole(C, TILE, head, n_in, dead, pt);
        ring_whole += whole ? 1u : 0u;
        if ((in_run[pt] != 0) != whole || in_run[pt] > 1) { bad("run membership", C, head, n_in, dead, tile0, live); return; }
        if (whole && head > pt * TILE && head < (pt + 1) * TILE) n_head_inside++;
    }
    n_some += brute ? 1u : 0u, n_none += brute ? 0u : 1u, n_all += (brute == ring_tiles) ? 1u : 0u;
    n_run_wraps += (W.len && W.first + W.len > ring_tiles) ? 1u : 0u, n_partial += (brute && brute < ring_whole) ? 1u : 0u;
}
int main() {
    const uint32_t caps[] = {4, 8, 12, 32};
    for (uint32_t C : caps) {
        const uint32_t ring_tiles = C / TILE;
        for (uint32_t head = 0; head < C; head++)
        for (uint32_t n_in = 0; n_in <= C; n_in++)
        for (uint32_t dead = 0; dead <= n_in; dead++) {
            // what a layout can give: the dispatched tiles start at the tile of logical index lo, 0 <= lo <= dead
            for (uint32_t lo = 0; lo <= dead; lo++) {
                const FwFifoLayout L = fw_fifo_layout(C, TILE, BLOCK, head, lo, n_in, n_in, 0u);
                n_layouts++;
                check(C, head, n_in, dead, L.tile0, L.live_tiles);
                // (a layout dispatches every whole tile of the ring)
                if (fw_fifo_whole_span(C, TILE, head, n_in, dead, L.tile0, L.live_tiles).count != fw_fifo_whole_span(C, TILE, head, n_in, dead, 0u, ring_tiles).count)
                    bad("a whole tile the layout does not dispatch", C, head, n_in, dead, L.tile0, L.live_tiles);
            }
            // ... and every other range of dispatched tiles
            for (uint32_t tile0 = 0; tile0 < ring_tiles; tile0++)
            for (uint32_t live = 0; live <= ring_tiles; live++) check(C, head, n_in, dead, tile0, live);
        }
        // a count only the device knows: the launch covers the ring, nothing is whole
        for (uint32_t head = 0; head < C; head++)
        for (uint32_t dead = 0; dead <= C; dead++) {
            const FwWholeSpan W = fw_fifo_whole_span(C, TILE, head, 0xFFFFFFFFu, dead, 0u, ring_tiles);
            if (W.count != 0u || W.len != 0u) bad("a count only the device knows", C, head, 0xFFFFFFFFu, dead, 0u, ring_tiles);
            check(C, head, 0xFFFFFFFFu, dead, head / TILE, ring_tiles);
        }
    }
    printf("total cases %llu layouts %llu some %llu all %llu none %llu head_inside %llu run_wraps %llu partial %llu bad %llu\n",
           n_cases, n_layouts, n_some, n_all, n_none, n_head_inside, n_run_wraps, n_partial, n_bad);
    return n_bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("whole_span")
    (d / "whole_span.cpp").write_text(PROGRAM)
    exe = d / "whole_span"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "whole_span.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_closed_form_against_the_predicate_tile_by_tile(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:20]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    assert total["bad"] == 0 and total["cases"] > 1000000 and total["layouts"] > 50000, total
    # launches with whole tiles, without, with nothing but whole tiles; a whole tile the head lies inside; runs that pass the ring's end;
    # dispatched ranges that hold only a part of the run
    for k in ("some", "all", "none", "head_inside", "run_wraps", "partial"):
        assert total[k] > 0, (k, total)
