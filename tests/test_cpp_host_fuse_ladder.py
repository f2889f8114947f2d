"""The depth ladder of the fused FIFO launches without a GPU (csrc/fw_fuse2.h: fw_fuse_rung, fw_fuse_depth_max -- the lines launch_fifo
compiles: FifoAccum::rung, FifoAccum::derive).  A stand-alone C++ program, compiled with g++ -Wall -Werror -- once plainly,
once with -fsanitize=address,undefined --, enumerates the rule: launches of one ring and of two, each ring's live count at every
threshold, one below and one above it (and 0); fw_ctx::fuse_depth over 2 to 8 and fuse_far_depth over 8 to 16, each with a value
beyond its range on either side, which the function clamps as launch_fifo did; both newborn rules; the four thresholds in order, with
ties, and out of order (fuse_wide_min below fuse_deep_min, fuse_far_min below everything, all reversed).  Every case must equal the
expression the ladder replaced, written out here as launch_fifo had it: four flags, each the AND over the rings of one comparison, a
clamped knob, `go_far`, and a nest of conditionals.  Whether the launch may be fused at all (the first flag) must equal "the rung is at
least FW_RUNG_TWO" in every case; the depth must be equal in every case in which the launch may be fused -- FwWithheld::offer reads
depth_max behind `candidate` alone, and a launch below the first rung is no candidate.  A ring's rung must be the first threshold, taken
in order, that its live count does not meet, and a launch's the lowest of its rings'.  Every rung and every depth from 2 to 16 must
occur as a result."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include <algorithm>
#include "fw_fuse2.h"
static_assert(FW_FUSE_MAX == 8 && FW_FUSE_NARROW == 4 && FW_FUSE_FAR == 16, "the depths this program expects to see");
static unsigned long long n_bad, n_cases, n_candidates, n_rung[FW_RUNG_FAR + 1], n_depth[FW_FUSE_FAR + 1], n_out_of_order;
struct Knobs { uint32_t fuse2_min, deep_min, wide_min, far_min, fuse_depth, far_depth; bool newborn_spin; };
static void bad(const char *what, const Knobs &K, const uint32_t *n, uint32_t rings, uint32_t want, uint32_t got) {
    if (n_bad++ < 20)
        printf("BAD %s: mins %u %u %u %u depth %u far_depth %u newborn_spin %d rings %u counts %u %u: want %u got %u\n", what, K.fuse2_min, K.deep_min, K.wide_min, K.far_min,
               K.fuse_depth, K.far_depth, (int)K.newborn_spin, rings, n[0], rings > 1 ? n[1] : 0u, want, got);
}
static void launch(const Knobs &K, const uint32_t *n, uint32_t rings) {
    // ---- what launch_fifo did: ring_record's four `&=` lines, then FifoAccum::derive
    bool fusable = true, deep = true, wide = true, far = true;
    for (uint32_t j = 0; j < rings; j++) {
        fusable &= n[j] >= K.fuse2_min;
        deep &= n[j] >= K.deep_min;
        wide &= n[j] >= K.wide_min;
        far &= n[j] >= K.far_min;
    }
    const uint32_t newborn_word = K.newborn_spin ? 0u : 1u;  // (FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN])
    const uint32_t depth_knob = std::max(2u, std::min(K.fuse_depth, (uint32_t)FW_FUSE_MAX));
    const bool go_far = deep && wide && far && K.fuse_depth == (uint32_t)FW_FUSE_MAX && newborn_word != 0u && K.far_depth > (uint32_t)FW_FUSE_MAX;
    const uint32_t want = go_far ? std::min(K.far_depth, (uint32_t)FW_FUSE_FAR) : !deep ? 2u : !wide ? std::min(depth_knob, (uint32_t)FW_FUSE_NARROW) : depth_knob;
    // ---- the ladder
    uint32_t rung = FW_RUNG_FAR;
    for (uint32_t j = 0; j < rings; j++) {
        const uint32_t r = fw_fuse_rung(n[j], K.fuse2_min, K.deep_min, K.wide_min, K.far_min);
        const uint32_t mins[4] = {K.fuse2_min, K.deep_min, K.wide_min, K.far_min};
        uint32_t first_failed = 0;  // (in its own words: the first threshold, in order, the count does not meet)
        while (first_failed < 4u && n[j] >= mins[first_failed]) first_failed++;
        if (r != first_failed) bad("a ring's rung", K, n, rings, first_failed, r);
        rung = std::min(rung, r);
    }
    const uint32_t got = fw_fuse_depth_max(rung, K.fuse_depth, K.far_depth, newborn_word != 0u);
    n_cases++, n_rung[rung]++;
    if (fusable != (rung >= FW_RUNG_TWO)) bad("may the launch be fused", K, n, rings, fusable, rung);
    if (got < 2u || got > FW_FUSE_FAR) { bad("a depth out of range", K, n, rings, want, got); return; }
    if (!fusable) return;  // (no candidate: nobody reads its depth)
    n_candidates++, n_depth[got]++;
    if (got != want) bad("depth_max", K, n, rings, want, got);
}
int main() {
    const uint32_t mins[][4] = {{10, 20, 30, 40}, {1, 1, 1, 1}, {10, 20, 20, 40}, {10, 30, 20, 40}, {10, 20, 40, 30}, {30, 10, 40, 20}, {40, 30, 20, 10}, {20, 10, 30, 5}, {0, 0, 0, 0}};
    for (const auto &m : mins) {
        std::vector<uint32_t> counts{0u};
        for (uint32_t t : m) for (uint32_t x : {t - 1u, t, t + 1u}) if (t || x != 0xFFFFFFFFu) counts.push_back(x);
        std::sort(counts.begin(), counts.end()), counts.erase(std::unique(counts.begin(), counts.end()), counts.end());
        const bool ordered = m[0] <= m[1] && m[1] <= m[2] && m[2] <= m[3];
        for (uint32_t fuse_depth = 1; fuse_depth <= 9; fuse_depth++)      // (2 .. 8, and one beyond on either side)
        for (uint32_t far_depth = 7; far_depth <= 17; far_depth++)        // (8 .. 16, likewise)
        for (int newborn_spin = 0; newborn_spin < 2; newborn_spin++) {
            const Knobs K{m[0], m[1], m[2], m[3], fuse_depth, far_depth, newborn_spin != 0};
            for (uint32_t a : counts) {
                launch(K, &a, 1u);
                n_out_of_order += ordered ? 0u : 1u;
                for (uint32_t b : counts) {
                    const uint32_t two[2] = {a, b};
                    launch(K, two, 2u);
                }
            }
        }
    }
    printf("total cases %llu candidates %llu out_of_order %llu", n_cases, n_candidates, n_out_of_order);
    for (uint32_t r = 0; r <= FW_RUNG_FAR; r++) printf(" rung%u %llu", r, n_rung[r]);
    for (uint32_t d = 2; d <= FW_FUSE_FAR; d++) printf(" depth%u %llu", d, n_depth[d]);
    printf(" bad %llu\n", n_bad);
    return n_bad ? 1 : 0;
}
"""

program = fuse_model.program_fixture("fuse_ladder", PROGRAM)


def test_the_ladder_equals_the_flags_it_replaced(program):
    lines, total = fuse_model.run(program[0], [], 120)
    assert total["cases"] > 100000 and total["candidates"] > 50000 and total["out_of_order"] > 1000, total
    # every rung and every depth from 2 to 16 occurred as a result
    for r in range(0, 5):
        assert total["rung%d" % r] > 0, (r, total)
    for d in range(2, 17):
        assert total["depth%d" % d] > 0, (d, total)
