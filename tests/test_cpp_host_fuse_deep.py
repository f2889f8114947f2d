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
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

# (the model: tests/fuse_model.py.  Its own: every sequence for the smallest rings, a grid of edge values for the larger ones, to groups
# of three and four frames; the history of a slot in base 5)
PROGRAM = r"""
#include "fw_fuse2.h"
#define FW_MODEL_HIST_BASE 5u
""" + fuse_model.GRID_MODEL + r"""
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
            const Stepped S = begin(C, head, n_in);
            Frame fr[FW_FUSE_MAX];
            walk(C, head, n_in, S.parity, fr, 0, nullptr, S, p.all, p.depth, FW_FUSE_MAX, 3);
        }
        printf("C %u groups of two %llu three %llu four %llu\n", C, n_groups[2], n_groups[3], n_groups[4]);
    }
    printf("total three %llu four %llu declined %llu newborn_dies %llu overflow %llu discontinuous %llu wrapped_head %llu wrapped_spawn %llu spawn0 %llu dead0 %llu no_tile %llu bad %llu\n",
           n_groups[3], n_groups[4], n_declined, n_newborn_dies, n_overflow, n_discont, n_wrapped_head, n_wrapped_spawn, n_spawn0, n_dead0, n_no_tile, n_bad);
    return n_bad ? 1 : 0;
}
"""

# (the sanitizer build walks half of the rings: every path of the program)
program = fuse_model.program_fixture("fuse_deep", PROGRAM)


def test_every_group_of_three_and_four_frames_of_small_rings(program):
    exe, quick = program
    lines, total = fuse_model.run(exe, [quick], 600)
    assert total["three"] > 10000 and total["four"] > 10000
    # everything the rule must decline occurred and was declined (the program compares rule and stepping frame by frame), and the
    # admitted groups include wrapped heads, new particles that wrap the buffer's end, frames that spawn or destroy nothing, and launches
    # without a ring tile (every old particle dies in the group)
    for k in ("declined", "newborn_dies", "overflow", "discontinuous", "wrapped_head", "wrapped_spawn", "spawn0", "dead0", "no_tile"):
        assert total[k] > 0, (k, total)
