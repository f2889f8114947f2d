"""The withheld group of FIFO launches without a GPU (csrc/fw_withheld.h: FwWithheld -- offer, take, drop -- and FwFifoLaunch; the lines
launch_fifo and flush_withheld compile).  A stand-alone C++ program with its own main drives the group through random hosts
from fixed seeds: 1, 2 and FW_FIFO_PER_LAUNCH rings of 2 to 4 FW_TILE slots, 0 to 3 ops per ring and frame, spawn and death counts that now
and then break the pair rule, rings whose record changes between two frames, candidates and non-candidates, a depth_max of 2,
FW_FUSE_NARROW or FW_FUSE_MAX (and, less often, any depth the FW_FUSE_DEPTH knob can ask for: a group closes at depth_max exactly, and
every depth from 2 to 8 must be seen to close) that sometimes changes inside a group, readers (take) and drops at random.  Beside the
group the program keeps a model in its own words -- the plain list of the frames offered since the last launch, each as it was built --
and says from it what every offer must do (join, close, decline and why) and what every launch that comes out must hold: its frames,
each exactly once and in order; fused, dt, dt_pre, parity; per ring the first frame's head and live count, the summed spawns and dead, the
boundaries of FwFuseArgs (FwFuseRecords), the layout fw_fifo_layout gives for the sums, cumulative tile_first; the ops ring by ring in frame order with
rel_base shifted by the earlier frames' new particles; a withheld frame that goes alone memcmp-equal to the launch as built, apart from
host_counts == nullptr.  The run fails unless every outcome occurred: joined and withheld, closed at each depth 2 to 8, declined by the
pair rule alone, by the ops limit alone, by a ring mismatch alone, by depth_max alone, a non-candidate flushing a group, take at each
pending depth 1 to 7 and on an empty group, drop with a group pending.
fw_kernels.h does not compile alone under g++ -Wall -Werror (`#pragma unroll` in the device headers it includes), so the program is
compiled host-side by the Makefile's hipcc as plain C++ (-x c++: no device code, no HIP call) -- once plainly, once with
-fsanitize=address,undefined -- and run directly: nothing is loaded into Python, nothing is preloaded."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

# (the model, the steps of a host and main: tests/fuse_model.py.  Its own: the host that draws a depth_max of 2 to FW_FUSE_MAX, 0 to 3
# ops per ring and frame, and reads and drops often)
PROGRAM = fuse_model.WITHHELD_MODEL + r"""
static void host(uint64_t seed, uint32_t steps, uint64_t &frame) {
    rng = seed * 0x9E3779B97F4A7C15ull + 1u, cur_seed = seed;
    static FwWithheld W;
    W.drop(), pending.clear();
    const uint32_t ring_counts[3] = {1u, 2u, FW_FIFO_PER_LAUNCH};
    const uint32_t n_rings = ring_counts[seed % 3u];
    const uint32_t op_rate = 2u + rnd(4u * n_rings);  // one ring in op_rate carries ops in a frame
    std::vector<Ring> rings;
    new_rings(rings, n_rings, false);
    uint32_t depth_max = 2u;
    int32_t write_mask = 0;
    for (uint32_t step = 0; step < steps; step++) {
        cur_step = step;
        const uint32_t what = rnd(100);
        if (what < 5u) { somebody_reads(W); continue; }
        if (what < 7u) { particles_go(W, rings, false); continue; }
        if (step == 0u || rnd(12) == 0u) {
            const uint32_t r = rnd(10);
            const uint32_t nd = r < 3u ? 2u : r < 5u ? (uint32_t)FW_FUSE_NARROW : r < 8u ? (uint32_t)FW_FUSE_MAX : 2u + rnd(FW_FUSE_MAX - 1u);
            if (nd != depth_max && !pending.empty()) n_depth_changed_inside++;
            depth_max = nd;
        }
        if (rnd(40) == 0u) write_mask = (int32_t)rnd(9) - 1;
        if (rnd(25) == 0u) record_changes(rings[rnd(n_rings)]);
        static FwFifoLaunch B;
        begin_frame(B, frame, n_rings, write_mask);
        for (uint32_t j = 0; j < n_rings; j++) {
            Ring &R = rings[j];
            const uint32_t room = R.capacity - R.live;
            uint32_t k_ops = rnd(op_rate) == 0u ? 1u + rnd(3) : 0u;
            k_ops = std::min(k_ops, FW_INLINE_OPS - B.n_ops);
            B.fa.s[j].op0 = B.n_ops;
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
            ring_frame(B, j, R, n_spawn, 25u, 60u);
        }
        const bool candidate = rnd(8) != 0u;
        offer(W, B, candidate, depth_max, frame);
    }
    last_take(W);
}
"""

SEEDS, STEPS = 48, 4000  # (chosen on the CPU so that the model alone meets the coverage condition below, with a margin)

program = fuse_model.program_fixture("withheld", PROGRAM, host_hipcc=True)


def test_the_withheld_group_under_random_hosts(program):
    lines, total = fuse_model.run(program[0], [SEEDS, STEPS], 300)
    assert total["frames_run"] + total["dropped"] == total["offers"] > 100000
    # every outcome occurred
    for k in (["withheld_new", "joined_withheld"] + ["closed%d" % d for d in range(2, 9)] +
              ["declined_pair", "declined_ops", "declined_ring", "declined_depth", "noncandidate_flush", "alone"] +
              ["take%d" % d for d in range(1, 8)] + ["take_empty", "drop_pending", "depth_changed_inside"]):
        assert total[k] >= 10, (k, total)
