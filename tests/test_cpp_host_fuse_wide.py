"""Groups of five to eight frames of a FIFO ring in one launch without a GPU (csrc/fw_fuse2.h: FwFuseGroup, fw_fuse_begin, fw_fuse_push --
the lines FwWithheld::join (csrc/fw_withheld.h) and launch_fifo compile).  A stand-alone C++ program in the manner of tests/test_cpp_host_fuse_deep.py,
compiled with g++ -Wall -Werror -- once plainly, once with -fsanitize=address,undefined --, walks a reduced model of the kernel's grid
(tiles of 4 slots, spawning workgroups of 2) slot by slot.  Every sequence of eight frames is too many, so: for rings of 8 and 16 slots
each frame takes the edge values {0, 1, a tile + 1, a third, all but one, everything} for its spawns and its dead, to depth 8, from edge
heads and live counts (the 16-slot ring: from three nearly full starts, which keep the walk to seconds); for rings of 20, 32 and 64
slots a seeded random walk draws mostly small frames, so that groups grow deep, and now and then anything.  Every frame is also stepped by itself over an explicit ring of slots.  The fold must admit a frame exactly when
stepping it met none of: a particle born in the group dying in it, a new particle landing on a slot that held a particle when the group
began, a frame that does not continue the one before, a ninth frame.  For every admitted group of five to eight frames the fused launch
-- the layout fw_fifo_layout gives for the folded frame, each new particle's frame taken from the cumulative bounds, the counters by the
kernel's arithmetic -- must agree with the frames stepped one by one: the slots stored (each live slot exactly once, nothing else), the
updates every slot's particle received and their dt sequence (the update history in base 9: 9^8 fits in 64 bits), both count rows, the
destroyed count and the statistics.  Groups of each depth, each reason to decline, wrapped heads and wrapped spawns are counted and must
all have occurred."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

# (the model: tests/fuse_model.py.  Its own: a fold limited to FW_FUSE_MAX, groups of five to eight frames, the edge values of every frame
# for the small rings and random walks for the larger ones; the history of a slot in base 9)
PROGRAM = r"""
#include "fw_fuse2.h"
static_assert(FW_FUSE_MAX == 8, "this program walks groups of up to eight frames and tries a ninth");
#define FW_MODEL_HIST_BASE 9u
""" + fuse_model.GRID_MODEL + r"""
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const bool quick = atoi(argv[1]) != 0;
    // the edge values of every frame to depth 8: from the edge heads and live counts of the 8-slot ring (the sanitizer build: from a
    // wrapping head with a third and with all but one of the slots live), and from three starts of the 16-slot ring, whose walk from a
    // ring with more room takes tens of seconds -- a head at the buffer's end with two slots free, the full ring, all but one slot live
    struct Start { uint32_t C, head, n_in; };
    std::vector<Start> starts;
    for (uint32_t head : values(7, false))
    for (uint32_t n_in : values(8, false))
        if (!quick || (head == 7u && (n_in == 2u || n_in == 7u))) starts.push_back(Start{8u, head, n_in});
    if (!quick) starts.insert(starts.end(), {Start{16u, 15u, 14u}, Start{16u, 1u, 16u}, Start{16u, 14u, 15u}});
    for (uint32_t C : {8u, 16u}) {
        for (const Start &s : starts) {
            if (s.C != C) continue;
            Stepped S = begin(C, s.head, s.n_in);
            Frame fr[FW_FUSE_MAX];
            walk(C, s.head, s.n_in, S.parity, fr, 0, nullptr, S, false, FW_FUSE_MAX, FW_FUSE_MAX, 5);
        }
        printf("C %u groups of five %llu six %llu seven %llu eight %llu\n", C, n_groups[5], n_groups[6], n_groups[7], n_groups[8]);
    }
    for (uint32_t C : {20u, 32u, 64u}) {
        random_walks(C, quick ? 5000u : 100000u, FW_FUSE_MAX, 5, 12, 10, 1);
        printf("C %u groups of five %llu six %llu seven %llu eight %llu\n", C, n_groups[5], n_groups[6], n_groups[7], n_groups[8]);
    }
    // (ninth: a ninth frame was offered to a full group, and never joined)
    printf("total five %llu six %llu seven %llu eight %llu compared %llu declined %llu newborn_dies %llu overflow %llu discontinuous %llu ninth %llu wrapped_head %llu wrapped_spawn %llu bad %llu\n",
           n_groups[5], n_groups[6], n_groups[7], n_groups[8], n_compared, n_declined, n_newborn_dies, n_overflow, n_discont, n_full, n_wrapped_head, n_wrapped_spawn, n_bad);
    return n_bad ? 1 : 0;
}
"""

# (the sanitizer build walks the smallest ring from two starts and a twentieth of the random walks: every path of the program)
program = fuse_model.program_fixture("fuse_wide", PROGRAM)


def test_groups_of_five_to_eight_frames_of_small_rings(program):
    exe, quick = program
    lines, total = fuse_model.run(exe, [quick], 600)
    # groups of each depth occurred and were compared with the frames stepped one by one ...
    for k in ("five", "six", "seven", "eight"):
        assert total[k] > 1000, (k, total)
    assert total["compared"] == total["five"] + total["six"] + total["seven"] + total["eight"]
    # ... in the random walks of the larger rings as well (the counts are cumulative: the last ring's line against the 16-slot one's)
    per_ring = [dict(zip(ln.split()[4::2], map(int, ln.split()[5::2]))) for ln in lines[:-1]]
    for k in ("five", "six", "seven", "eight"):
        assert per_ring[-1][k] > per_ring[-4][k], (k, per_ring)
    # everything the rule must decline occurred and was declined (the program compares rule and stepping frame by frame), a ninth frame
    # was offered to full groups and never joined, and the admitted groups include wrapped heads and new particles that wrap the buffer's end
    for k in ("declined", "newborn_dies", "overflow", "discontinuous", "ninth", "wrapped_head", "wrapped_spawn"):
        assert total[k] > 0, (k, total)
