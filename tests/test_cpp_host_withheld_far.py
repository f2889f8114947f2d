"""The withheld group of FIFO launches in the far tier without a GPU (csrc/fw_withheld.h: FwWithheld with a depth_max of 9 to 16, the merge
of a frame's op into the group's last op of its ring -- fw_op_continues --, FwFuseRecords).  A stand-alone C++
program with its own main, in the manner of tests/test_cpp_host_withheld.py, drives the group through random hosts from fixed seeds: 1,
2 and FW_FIFO_PER_LAUNCH rings of 2 to 4 FW_TILE slots; per ring an emitter that mostly stands still -- its op continues the one of the
frame before in particles and serials, with the same origin: mergeable -- and now and then moves, changes its record or skips serials:
not mergeable; now and then a second and third op in a frame; spawn and death counts that now and then break the pair rule; a depth_max
of 9 to 16 most of the time and of 2, FW_FUSE_NARROW or FW_FUSE_MAX otherwise, which sometimes changes inside a group; readers (take) and
drops at random.  Beside the group the program keeps a model in its own words -- the plain list of the frames offered since the last
launch, each as it was built, with the depth_max it was offered with -- and says from it what every offer must do and what every launch
that comes out must hold: its frames, each exactly once and in order; fused, dt, parity; the dt and boundaries of withheld frames 0 to 6
in FwFuseArgs and of frames 7 to 14 in FwFarArgs, word for word; per ring the first frame's head and live count, the summed spawns and
dead, the layout fw_fifo_layout gives for the sums; the ops ring by ring: a frame that joined under a depth_max above FW_FUSE_MAX has its
first op of a ring merged into the ring's last op where the model's own predicate says it continues it, every other op stands by itself
with rel_base shifted -- memcmp against the model's list.  The run fails unless every outcome occurred: closed at each depth 9 to 16,
take at each pending depth 1 to 15, ops merged and ops not merged in far groups, a far group declined by the ops limit alone, by the pair
rule alone and by depth_max alone, a group that began below the far tier and continued in it.
Compiled host-side by the Makefile's hipcc as plain C++ (-x c++: no device code, no HIP call) -- once plainly, once with
-fsanitize=address,undefined -- and run directly: nothing is loaded into Python, nothing is preloaded."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

# (the model, the steps of a host and main: tests/fuse_model.py.  Its own: the host whose emitters mostly stand still, which draws a
# depth_max of 9 to 16 most of the time and reads seldom)
PROGRAM = fuse_model.WITHHELD_MODEL + r"""
static void host(uint64_t seed, uint32_t steps, uint64_t &frame) {
    rng = seed * 0x9E3779B97F4A7C15ull + 1u, cur_seed = seed;
    static FwWithheld W;
    W.drop(), pending.clear();
    const uint32_t ring_counts[3] = {1u, 2u, FW_FIFO_PER_LAUNCH};
    const uint32_t n_rings = ring_counts[seed % 3u];
    const uint32_t still = 6u + rnd(40);       // one op in `still` does not continue the one before
    const uint32_t every = 1u + rnd(n_rings);  // one ring in `every` spawns in a frame
    const uint32_t reads = (seed % 7u == 0u) ? 12u : 3u;  // (some hosts read often: the shallow pending depths; most seldom: the deep ones)
    std::vector<Ring> rings;
    new_rings(rings, n_rings, true);
    uint32_t depth_max = 9u + rnd(8);
    int32_t write_mask = 0;
    for (uint32_t step = 0; step < steps; step++) {
        cur_step = step;
        const uint32_t what = rnd(100);
        if (what < reads) { somebody_reads(W); continue; }
        if (what == 99u && rnd(3) == 0u) { particles_go(W, rings, true); continue; }
        if (step == 0u || rnd(40) == 0u) {
            const uint32_t r = rnd(12);
            const uint32_t nd = r == 0u ? 2u : r == 1u ? (uint32_t)FW_FUSE_NARROW : r <= 3u ? (uint32_t)FW_FUSE_MAX : 9u + rnd(8);
            if (nd != depth_max && !pending.empty()) n_depth_changed_inside++;
            depth_max = nd;
        }
        if (rnd(400) == 0u) write_mask = (int32_t)rnd(9) - 1;
        if (rnd(300) == 0u) record_changes(rings[rnd(n_rings)]);
        static FwFifoLaunch B;
        begin_frame(B, frame, n_rings, write_mask);
        for (uint32_t j = 0; j < n_rings; j++) {
            Ring &R = rings[j];
            const uint32_t room = R.capacity - R.live;
            uint32_t k_ops = rnd(every) == 0u ? (rnd(12) == 0u ? 2u + rnd(2) : 1u) : 0u;
            k_ops = std::min(k_ops, FW_INLINE_OPS - B.n_ops);
            B.fa.s[j].op0 = B.n_ops;
            uint32_t n_spawn = 0;
            for (uint32_t k = 0; k < k_ops; k++) {
                // (the emitter stands still most of the time; now and then it moves, its parent does, its modifier changes, serials are skipped)
                if (rnd(still) == 0u) {
                    switch (rnd(5)) {
                    case 0: R.pos += 1.0f; break;
                    case 1: R.vel += 0.5f; break;
                    case 2: R.speed *= 2.0f; break;
                    case 3: R.serial += 1u + rnd(3); break;
                    default: R.emit += 1u; break;
                    }
                }
                FwOp op{};
                // (mostly a few new particles, so that groups grow deep; now and then as many as the ring has room for, and more than a group can take)
                op.n = std::min(room - n_spawn, rnd(60) == 0u ? rnd(room + 1u) : rnd(6));
                op.seg = j, op.emit = R.emit + (k ? 1000u + k : 0u), op.rel_base = n_spawn, op.serial_base = R.serial, op.head = R.head, op.first_block = rnd(50);
                op.origin_pos[0] = R.pos, op.origin_rot[3] = 1.0f, op.parent_vel[1] = R.vel, op.speed = R.speed, op.scale = 1.0f;
                R.serial += op.n, n_spawn += op.n;
                B.fio.ops[B.n_ops++] = op;
            }
            ring_frame(B, j, R, n_spawn, 80u, 400u);
        }
        const bool candidate = rnd(40) != 0u;
        offer(W, B, candidate, depth_max, frame);
    }
    last_take(W);
}
"""

SEEDS, STEPS = 63, 6000  # (chosen on the CPU so that the model alone meets the coverage condition below, with a margin)

program = fuse_model.program_fixture("withheld_far", PROGRAM, host_hipcc=True)


def test_the_withheld_group_in_the_far_tier_under_random_hosts(program):
    lines, total = fuse_model.run(program[0], [SEEDS, STEPS], 300)
    assert total["frames_run"] + total["dropped"] == total["offers"] > 100000
    # every outcome occurred
    for k in (["withheld_new", "joined_withheld"] + ["closed%d" % d for d in range(9, 17)] + ["take%d" % d for d in range(1, 16)] +
              ["far_declined_pair", "far_declined_ops", "far_declined_depth", "declined_ring", "noncandidate_flush", "alone", "take_empty", "drop_pending",
               "depth_changed_inside", "grew_into_far"]):
        assert total[k] >= 10, (k, total)
    # ops merged and ops that stood by themselves in launches of more than eight frames; the far record's words were compared
    assert total["ops_merged"] > 10000 and total["ops_kept_far"] > 1000 and total["far_words"] > 10000, total
