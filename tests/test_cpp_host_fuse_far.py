"""Groups of nine to sixteen frames of a FIFO ring in one launch without a GPU: the far tier (csrc/fw_fuse2.h: FwFuseGroup, fw_fuse_begin,
fw_fuse_push with the limit FW_FUSE_FAR -- the lines FwWithheld::join compiles -- and csrc/fw_withheld.h: fw_op_continues).  A stand-alone
C++ program in the manner of tests/test_cpp_host_fuse_wide.py, compiled -- once plainly, once with -fsanitize=address,undefined -- and
run directly, walks a reduced model of the kernel's grid (tiles of 4 slots, spawning workgroups of 2) slot by slot over rings of 8 to
64 slots.  A seeded random walk draws mostly small frames, so that groups grow to sixteen, and now and then anything; every frame is
also stepped by itself over an explicit ring of slots.  The fold must admit a frame exactly when stepping it met none of: a particle born
in the group dying in it, a new particle landing on a slot that held a particle when the group began, a frame that does not continue the
one before, a seventeenth frame.  For every admitted group of nine to sixteen frames the fused launch -- the layout fw_fifo_layout gives
for the folded frame, each new particle's frame taken from the cumulative bounds, the counters by the kernel's arithmetic -- must agree
with the frames stepped one by one: the slots stored (each live slot exactly once, nothing else), the updates every slot's particle
received and their order (an order-sensitive hash of the frames), both count rows, the destroyed count and the statistics; and
fw_fifo_whole_span must count the tiles fw_fifo_tile_whole calls whole among the dispatched ones.  A fold limited to FW_FUSE_MAX, the first tier's cap, holds
the same eight frames as the unlimited one and refuses a ninth.
The merge predicate against brute force: random lists of ops, frame by frame, drawn from a small alphabet so that runs occur, are merged
the way the group merges them (a frame's first op into the list's last); every new particle k must get the same (emit, serial, origin,
parent velocity, modifiers) from the merged and from the unmerged list, by the kernel's own lookup.  A pair that merges no longer merges
with one bit flipped in any compared field or with serial_base off by one, and still merges with the fields no spawning workgroup of the
FIFO launch reads (head, first_block, range_ring) changed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_model  # noqa: E402

# (the model: tests/fuse_model.py.  Its own: a fold limited to FW_FUSE_FAR, groups of nine to sixteen frames from random walks, the first
# tier's limit beside it, and the merge predicate)
PROGRAM = r"""
#include "fw_withheld.h"
static_assert(FW_FUSE_MAX == 8 && FW_FUSE_FAR == 16, "this program walks groups of up to sixteen frames and tries a seventeenth");
""" + fuse_model.GRID_MODEL + r"""
static unsigned long long n_ninth, n_merged, n_unmerged, n_particles, n_flips;
// a fold limited to FW_FUSE_MAX, the first tier's cap, holds the same eight frames as the unlimited one and refuses a ninth, whatever it carries
static void first_tier(uint32_t C, uint32_t head0, uint32_t n_in0, const Frame *fr, uint32_t depth, const FwFuseGroup &H, const Stepped &T) {
    if (depth != FW_FUSE_MAX) return;
    FwFuseGroup X = fw_fuse_begin(FwFifoFrame{head0, n_in0, fr[0].spawn, fr[0].dead});
    Stepped R = begin(C, head0, n_in0);
    step(R, fr[0], 0);
    bool all = true;
    for (uint32_t f = 1; f < depth; f++) all = all && fw_fuse_push(C, X, FwFifoFrame{R.head, R.count, fr[f].spawn, fr[f].dead}, FW_FUSE_MAX), step(R, fr[f], (int)f);
    if (!all || X.depth != FW_FUSE_MAX || memcmp(&X.U, &H.U, sizeof X.U) != 0 || memcmp(X.spawn_end, H.spawn_end, sizeof X.spawn_end) != 0 ||
        memcmp(X.dead, H.dead, sizeof X.dead) != 0)
        bad("the first tier's fold of the same eight frames", C, head0, n_in0, fr, depth);
    if (fw_fuse_push(C, X, FwFifoFrame{T.head, T.count, 0, 0}, FW_FUSE_MAX) || X.depth != FW_FUSE_MAX) bad("a ninth frame through a fold limited to FW_FUSE_MAX", C, head0, n_in0, fr, depth);
    n_ninth++;
}

// ---- the merge predicate against brute force
struct Got { uint32_t emit; uint64_t serial; float v[14]; bool found; };
static Got lookup(const std::vector<FwOp> &ops, uint32_t k) {  // the spawning workgroup's own: the last op that holds k
    Got g{};
    for (const FwOp &op : ops)
        if (k >= op.rel_base && k - op.rel_base < op.n) {
            g.found = true, g.emit = op.emit, g.serial = op.serial_base + (k - op.rel_base);
            memcpy(g.v, op.origin_pos, 16), memcpy(g.v + 4, op.origin_rot, 16), memcpy(g.v + 8, op.parent_vel, 16), g.v[12] = op.speed, g.v[13] = op.scale;
        }
    return g;
}
// every bit of one field of b0 (a field `last` and b0 are compared in), flipped by itself: the pair must no longer merge
static void flip(const FwOp &last, const FwOp &b0, const void *field, uint32_t bytes) {
    const size_t off = (size_t)((const unsigned char *)field - (const unsigned char *)&b0);
    for (uint32_t bit = 0; bit < bytes * 8u; bit++) {
        FwOp x = b0;
        ((unsigned char *)&x)[off + bit / 8u] ^= (unsigned char)(1u << (bit % 8u));
        if (fw_op_continues(last, x)) { if (n_bad++ < 20) printf("BAD merge: a pair that differs in one bit of a compared field still merges (offset %zu bit %u)\n", off, bit); }
        n_flips++;
    }
}
static void merges(uint32_t trials) {
    for (uint32_t t = 0; t < trials; t++) {
        std::vector<FwOp> plain, merged;
        const uint32_t D = 1u + rnd(FW_FUSE_FAR);
        uint32_t spawned = 0;
        uint64_t serial = 1000u + rnd(1000);
        uint32_t emit = rnd(2);
        float pos = (float)rnd(2), vel = 0.0f, speed = 1.0f;
        for (uint32_t f = 0; f < D; f++) {
            const uint32_t k_ops = rnd(8) == 0u ? 2u : rnd(8) == 0u ? 0u : 1u;
            uint32_t rel = 0;  // within the frame
            for (uint32_t x = 0; x < k_ops; x++) {
                // (mostly the frame before continues; now and then something of the emitter changes, or the serial jumps)
                const uint32_t r = rnd(24);
                if (r == 0) emit ^= 1u;
                else if (r == 1) pos += 1.0f;
                else if (r == 2) vel += 0.5f;
                else if (r == 3) speed *= 2.0f;
                else if (r == 4) serial += 1u + rnd(3);
                FwOp op{};
                op.seg = 2u, op.emit = emit, op.n = rnd(6), op.rel_base = rel, op.serial_base = serial, op.first_block = rnd(100), op.head = rnd(100);
                op.origin_pos[0] = pos, op.origin_rot[3] = 1.0f, op.parent_vel[1] = vel, op.speed = speed, op.scale = 1.0f;
                rel += op.n, serial += op.n;
                FwOp b = op;
                b.rel_base += spawned;  // (the new particles of the earlier frames of this ring sit in front)
                plain.push_back(b);
                if (x == 0 && !merged.empty() && fw_op_continues(merged.back(), b)) merged.back().n += b.n, n_merged++;
                else merged.push_back(b), n_unmerged++;
                if (x == 0 && plain.size() >= 2u) {
                    const FwOp &last = plain[plain.size() - 2u];
                    if (fw_op_continues(last, b)) {
                        FwOp b0 = b;
                        flip(last, b0, &b0.seg, 4), flip(last, b0, &b0.emit, 4), flip(last, b0, &b0.rel_base, 4), flip(last, b0, &b0.serial_base, 8);
                        flip(last, b0, b0.origin_pos, 16), flip(last, b0, b0.origin_rot, 16), flip(last, b0, b0.parent_vel, 16);
                        flip(last, b0, &b0.speed, 4), flip(last, b0, &b0.scale, 4);
                        FwOp y = b0;
                        y.serial_base += 1u;
                        if (fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: serial_base + 1 still merges\n"); }
                        y = b0, y.serial_base -= 1u;
                        if (fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: serial_base - 1 still merges\n"); }
                        y = b0, y.head ^= 0xFFu, y.first_block ^= 0xFFu, y.range_ring ^= 1u, y.n += 3u;
                        if (!fw_op_continues(last, y)) { if (n_bad++ < 20) printf("BAD merge: a field no spawning workgroup reads keeps a pair from merging\n"); }
                    }
                }
            }
            spawned += rel;
        }
        for (uint32_t k = 0; k < spawned; k++) {
            const Got a = lookup(plain, k), b = lookup(merged, k);
            n_particles++;
            if (!a.found || !b.found || a.emit != b.emit || a.serial != b.serial || memcmp(a.v, b.v, sizeof a.v) != 0)
                if (n_bad++ < 20) printf("BAD merge: particle %u of %u gets another record from the merged list (trial %u)\n", k, spawned, t);
        }
        if (lookup(merged, spawned).found) { if (n_bad++ < 20) printf("BAD merge: the merged list holds a particle nobody spawned\n"); }
    }
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const bool quick = atoi(argv[1]) != 0;
    after_join = first_tier;
    for (uint32_t C : {8u, 16u, 20u, 32u, 64u}) {
        random_walks(C, quick ? 10000u : 200000u, FW_FUSE_FAR, FW_FUSE_MAX + 1, 24, 16, 2);
        printf("C %u groups of d9 %llu d10 %llu d11 %llu d12 %llu d13 %llu d14 %llu d15 %llu d16 %llu\n", C, n_groups[9], n_groups[10], n_groups[11], n_groups[12], n_groups[13],
               n_groups[14], n_groups[15], n_groups[16]);
    }
    merges(quick ? 2000u : 40000u);
    // (seventeenth: a seventeenth frame was offered to a full group, and never joined)
    printf("total d9 %llu d10 %llu d11 %llu d12 %llu d13 %llu d14 %llu d15 %llu d16 %llu compared %llu declined %llu newborn_dies %llu overflow %llu discontinuous %llu "
           "seventeenth %llu ninth %llu wrapped_head %llu wrapped_spawn %llu whole_tiles %llu merged %llu unmerged %llu particles %llu flips %llu bad %llu\n",
           n_groups[9], n_groups[10], n_groups[11], n_groups[12], n_groups[13], n_groups[14], n_groups[15], n_groups[16], n_compared, n_declined, n_newborn_dies, n_overflow,
           n_discont, n_full, n_ninth, n_wrapped_head, n_wrapped_spawn, n_whole_tiles, n_merged, n_unmerged, n_particles, n_flips, n_bad);
    return n_bad ? 1 : 0;
}
"""

DEPTHS = ["d%d" % d for d in range(9, 17)]

# (the sanitizer build runs a twentieth of the walks: every path of the program)
program = fuse_model.program_fixture("fuse_far", PROGRAM, host_hipcc=True)


def test_groups_of_nine_to_sixteen_frames_and_the_merge_predicate(program):
    exe, quick = program
    lines, total = fuse_model.run(exe, [quick], 600)
    # groups of each depth occurred and were compared with the frames stepped one by one ...
    for k in DEPTHS:
        assert total[k] > 100, (k, total)
    assert total["compared"] == sum(total[k] for k in DEPTHS)
    # ... in every ring (the counts are cumulative, ring after ring)
    per_ring = [dict(zip(ln.split()[4::2], map(int, ln.split()[5::2]))) for ln in lines[:-1]]
    assert len(per_ring) == 5
    for k in DEPTHS:
        assert per_ring[0][k] > 0 and all(b[k] > a[k] for a, b in zip(per_ring, per_ring[1:])), (k, per_ring)
    # everything the rule must decline occurred and was declined, a seventeenth frame was offered to full groups and never joined, a ninth
    # never joined a fold limited to FW_FUSE_MAX, and the admitted groups include wrapped heads, new particles that wrap the buffer's end, whole tiles
    for k in ("declined", "newborn_dies", "overflow", "discontinuous", "seventeenth", "ninth", "wrapped_head", "wrapped_spawn", "whole_tiles"):
        assert total[k] > 0, (k, total)
    # the merge predicate: lists that merged and lists that did not, every particle looked up in both, every compared bit flipped
    assert total["merged"] > 1000 and total["unmerged"] > 1000 and total["particles"] > 10000 and total["flips"] > 100000, total
