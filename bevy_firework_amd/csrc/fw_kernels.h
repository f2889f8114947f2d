// fw_kernels.h -- launch interface between the host engine (fw_engine.h, fw_engine_*.cpp) and the
// gfx950 kernels (fw_k_general.hip, fw_k_rings.hip, fw_k_nested.hip, fw_k_aux.hip, fw_k_refit.hip, fw_k_query.hip, fw_k_sort.hip; shared device
// helpers: fw_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include "fw_device.h"
#include "fw_collide.h"
#include "fw_refit.h"
#include "fw_mesh_bounds.h"
#include "fw_fuse2.h"

// The product build (the default `make`) carries no experiment surface: the FW_DEBUG profiling modes (kernel ablations, in-kernel
// timestamps) and the A/B switches of measured-and-rejected variants exist only in the `make ab` build (-DFW_AB,
// libfirework_hip_ab.so, loaded by the tools through FW_LIB_PATH).  FW_DBG(x, bit) is a compile-time 0 in the product: the
// branches fold away (an UNUSED timestamp branch was measured at 6 % of one GPU's share of configs[4], profiles/r03).
#ifdef FW_AB
#define FW_DBG(x, bit) (((x) & (bit)) != 0u)
#else
#define FW_DBG(x, bit) (false)
#endif

// pointers to the context's persistent device state (passed by value as a kernel argument)
#define FW_STAT_SLOTS 32
struct FwGlobals {
    FwSeg *segs;
    FwType *types;
    FwTypeColl *type_coll;  // [like types] collision settings per particle type
    float *keys;
    FwEmit *emits;
    uint32_t *count;     // [2][max_seg]  live particles per segment, by buffer parity
    uint32_t *spawned;   // [2][max_seg]  Global spawns appended this frame
    uint32_t *appended;  // [2][max_seg]  Nested children appended this frame
    uint32_t *ndestroyed;  // [max_seg]   particles destroyed by the last update
    // [2][max_seg], by buffer parity like `count`: survivors in the OLD part of a range ring (FwRangeRec) after the last update.
    // Particle 0 of such a ring sits `rold` slots before its first young particle -- the one fact about a range ring only the
    // device knows; everything that addresses its particles by list index (fw_k_spawn, fw_k_nest, fw_k_pack, the AABB query,
    // the host's readers) derives the slot of particle 0 from it
    uint32_t *rold;
    uint32_t max_seg;
    uint32_t seed;
    uint32_t *tile_cnt;              // split mode: survivors per tile
    uint32_t *tile_off;              // split mode: exclusive prefix per tile
    unsigned long long *tile_status; // fused mode: decoupled look-back words
    float *tile_box;                 // [tiles][8] {min.xyz, epoch, max.xyz, -} of the survivors each tile stored (FwUpdateArgs::boxes)
    uint32_t *err;                   // sticky FW_ERR_* flags
    // pinned host word: the first internal error of a kernel also lands here ({1 : 1 | check : 31 | segment : 32}, segment
    // 0xFFFFFFFF = not tied to one), so that the NEXT fw_step sees it without a synchronisation and stops stepping the
    // spawner it belongs to (fw_engine_mem.cpp: poll_device_error) -- an in-place ring update that went wrong cannot be redone
    unsigned long long *err_host;
    unsigned long long *stats;       // [FW_STAT_SLOTS] particles that entered update (running total = their sum; most kernels add to [0])
    unsigned long long *dbg_ts;      // FW_DEBUG & 8: 4 timestamps per tile of the last update (profiling)
    unsigned long long *emit_serial; // RNG serials of Nested emission entries
    unsigned long long *nest_status; // [nested tiles] look-back words of fw_k_nest, tagged with the launch's sequence number
    unsigned long long *nest_ticket; // [n_ops] {workgroups of the op that have finished, children of the op}: the last one commits, then zeroes
    // START tickets (round 5): a workgroup that will wait for workgroups of lower rank -- an OLD tile of a range ring, a tile of
    // parents of a Nested entry -- takes its rank from an atomic counter FIRST THING instead of from its workgroup index, so that
    // "whoever has a lower rank has started" (hence publishes its status word without waiting for anybody of higher rank) is a
    // fact of the program, not a habit of the dispatcher.  Counters only ever grow; the host, which knows how many workgroups of
    // each launch take a ticket, sends the value each counter has when the launch starts (FwRangeRec / FwNestOp / FwFifoNest::
    // ticket_base): no reset, no second pass.  range_ticket: one per segment; nest_start: one per Nested entry (emit slot).
    uint32_t *range_ticket;
    uint32_t *nest_start;
    // MEASURED AND NOT SHIPPED (profiles/r05/tickets_ab.txt, same box, interleaved): the ticket is one more dependent hop in front
    // of everything a latency-bound workgroup does -- configs[2] +1.0 %, one GPU's share of configs[4] +4.5 % (88.4 against 84.6 us),
    // configs[3] +8.6 % with the Nested entry inside the FIFO launch (62.9 against 57.9 us) and +14 % with the separate pass (76.7
    // against 67.0) -- far past the 2 % the guarantee was judged worth.  The product build takes ranks from workgroup indices
    // (FW_TICKETS = 0); the wait stays bounded by the dispatcher's habit of starting lower indices first, and a wait that does run
    // out raises the sticky per-spawner error of DESIGN.md section 11.  `tools/build_variant.sh tickets -DFW_TICKETS=1` builds the
    // guaranteed form (the whole GPU suite passes on it).
#ifndef FW_TICKETS
#define FW_TICKETS 0
#endif
    const FwCollider *colliders;         // the world particle_collision casts its rays into (fw_ctx_set_colliders)
    uint32_t n_colliders;
    const FwMeshInst *mesh_inst;         // ... and its mesh instances (fw_ctx_set_mesh_colliders)
    uint32_t n_mesh_inst;
};

struct FwUpdateArgs {
    const uint32_t *seg_tile_first;  // [n_seg + 1] first tile of each segment (device)
    const uint4 *tile_desc;          // [total_tiles] {segment, its first tile, its tile count, type index} (device)
    uint32_t n_seg;
    uint32_t total_tiles;
    uint32_t parity;       // read buf[parity], write buf[parity ^ 1]
    uint32_t epoch;        // frame number (look-back tag), never 0
    float dt;
    uint32_t spin_limit;   // look-back polls before the self-computed fallback
    uint32_t any_inst;    // some segment has an attached instance buffer: run the kernels that also write the records
    // pinned host word: workgroup 0 stores done_value at its START.  Launches of a stream run in order, so the host
    // reads "every launch before frame done_value has finished" without an event (recycling of per-frame host rings)
    unsigned long long *done_tag;
    unsigned long long done_value;
    uint32_t new_static;  // 1: every particle spawned this frame survives the step (host-proved), offsets are static
    unsigned long long *host_counts;  // pinned host snapshot row for this frame (or null): epoch << 32 | count
    // Global spawn ops fused into the update (virtual particles appended after the live ones);
    // sorted by destination segment, emission order inside a segment
    const FwOp *ops;               // table form (device memory), or null
    const uint4 *seg_op_first;     // [n_seg] per segment {first op, one past its last op, particles they spawn in all, 0} (table
                                   // form; pinned host memory: ONE bus round trip tells a tile its role -- summing the ops' counts
                                   // over the bus was a second, dependent one)
    uint32_t n_ops;                // ops this frame (inline form: entries of FwInlineOps used)
    uint32_t dbg;                  // FW_DEBUG (profiling only, results wrong): 1 = no look-back, 2 = no integrate
    // survivor forecast (fw_k_update header): table written last frame / table to write this frame
    uint32_t vt_rounds;            // new-particle tiles are vt_rounds * (threads per workgroup) particles
    uint32_t resident_slots;       // fw_k_update workgroups resident at once (256 CUs x 4)
    uint32_t seg0_type;            // type index of segment 0 (used when n_seg == 1)
    uint32_t use_stream;           // forecast frames: run fw_k_update_stream 
    uint32_t seg0_keys_off, seg0_keys_len;  // key pool window of segment 0's type (n_seg == 1)
    // n_seg == 1: the lone segment's record (FwSeg) for THIS frame's parity, so that a tile can address its input from
    // the kernel arguments alone (fw_k_update_stream<.., LONE>); seg0_ib == null: not provided
    const char *seg0_ib;
    char *seg0_ob, *seg0_destroyed, *seg0_inst;
    uint32_t seg0_capacity, seg0_n_lplanes, seg0_inst_cap;
    const uint2 *tile_keys;        // [n_seg] {keys_off, keys_len} of each segment's type (device)
    // optional per-frame total of live particles (feed of the RCCL all-reduce): every segment's finalizer adds its
    // new count to *live_out; workgroup 0 zeroes *live_next (the slot the next frame will use)
    unsigned long long *live_out, *live_next;
    // Survivor forecast, as per-tile sums: P[t] = {lo: particles that survive one more step of this dt and will sit in
    // input tile t of the next frame, counted by the tiles whose output starts in t; hi: those that spill into t + 1}
    // (global tile index); P2[g] = sum of P over tiles [64 g, 64 g + 64), one per 64-byte line from offset fc_s2; the
    // word at fc_tag holds the epoch of the frame that produced the buffer.  Three buffers rotate: read the previous
    // frame's (fc_in; null = not applicable this frame -> decoupled look-back), accumulate into fc_out with atomics,
    // clear fc_zero for the frame after.
    const unsigned long long *fc_in;
    unsigned long long *fc_out;
    unsigned long long *fc_zero;
    // Segments of up to FW_FC_DIRECT tiles keep the forecast as one plain entry per tile instead: {survivors landing in
    // output tile A, in A + 1, A, epoch} written with an ordinary store (no atomics: at 1M particles the thousand
    // atomics cost ~0.7 us of a 25 us kernel), summed by every tile of the segment (at most 4 entries per lane).
    const uint4 *fce_in;
    uint4 *fce_out;
    uint32_t force_colors;  // 1: write base / emissive colour even for constant gradients (the caller rewrote particles)
    uint32_t boxes;    // 1: every tile also leaves the box of position -/+ scale of its survivors in FwGlobals::tile_box
    uint32_t fc_sums;  // 1: some segment exceeds FW_FC_DIRECT tiles -> this launch uses the sums (all segments)
    uint32_t fc_s2, fc_tag;
    // Threshold forecast (round 6, per-tile entries only): the forecast above counts the survivors of ONE more step of the SAME dt.
    // With fc_theta > 0 every tile also leaves what the next frame needs to turn its entry into the forecast for ANY dt' < fc_theta:
    // fct_out[tile] = {survivors stored into output tile A, into A + 1, nA | nB << 16 (0xFFFFFFFF: more than FW_TF_K), first
    // output slot} and the (age, lifetime) pairs of the "risky" survivors -- those a step of fc_theta would destroy -- in
    // fcl_out[tile * FW_TF_K ..]: the ones stored into A from the front, those into A + 1 from the back.  fw_k_fc_resolve
    // (a wave per tile, launched in front of the next update when its dt differs) evaluates fw_survives(age, dt', lifetime) on
    // the pairs -- the update's own expression -- and rewrites the entry's two counts: the streaming schedule then runs as if
    // dt had repeated.  Everybody else survives any dt' < fc_theta (fp32 addition is monotone).
    float fc_theta;
    uint4 *fct_out;
    float2 *fcl_out;
};
#define FW_TF_K 256u  // (2 KB per tile and buffer; a tile of lifetimes in [0.8, 1.2] s lists ~100 at 60 Hz: 64 overflowed on every OLD tile)
// fw_k_fc_resolve: the previous frame's entries / headers / lists, this frame's dt and parity
struct FwResolveArgs {
    uint4 *fce;            // entries of the previous frame (this frame's fce_in): .x / .y are rewritten
    const uint4 *fct;
    const float2 *fcl;
    const uint4 *tile_desc;  // tile -> {segment, ...} (null: one segment)
    uint32_t total_tiles, parity, epoch;
    float dt;
};

// small frames carry their spawn ops in the kernel arguments: no H2D copy, no extra dependency
#define FW_INLINE_OPS 8
struct FwInlineOps {
    FwOp ops[FW_INLINE_OPS];
};

// ---- FIFO (ring) segments ----------------------------------------------------------------------------------------
// A particle type whose lifetime range is a single value destroys its particles in the order it received them: ages
// grow by the same dt for everybody (fp32 addition is monotone), new particles start at 0, so at every update the
// destroyed particles are a PREFIX of the list (reference order, core.rs:590-600 keeps survivors in order).  Nothing
// ever has to move: such a segment lives in ONE buffer used as a ring -- logical particle i sits in slot
// (head + i) mod capacity -- the update works in place (a particle is read and written by the same lane, planes that
// did not change are not written), and the host, which knows every spawn count and replays the fp32 age of each spawn
// cohort, knows head / live count / destroyed count of every frame exactly: no counting pass, no look-back, no
// forecast, whatever dt does.  One record per segment per frame, in the kernel arguments:
struct FwFifoSeg {
    char *buf;               // the ring (FwSeg::buf[0] == buf[1])
    char *destroyed, *inst;  // FwSeg::destroyed / inst (or null)
    uint32_t inst_cap, capacity, seg, type_idx;  // type_idx: | FW_TYPE_IDX_NOSPIN for a type that cannot turn
    uint32_t keys_off, keys_len;
    float life;  // the type's one lifetime value (a no-spin type's Q3 plane -- angular velocity 0, this lifetime -- is not read)
    uint32_t head;     // slot of logical particle 0 BEFORE this update
    uint32_t n_in;     // live particles before this frame's spawns
    uint32_t n_spawn;  // Global particles spawned this frame (logical indices [n_in, n_in + n_spawn))
    uint32_t dead;     // logical indices [0, dead) are destroyed by this update (may reach into the new ones)
    uint32_t op0, op1; // this segment's spawn ops in FwInlineOps
    // workgroups [tile_first, tile_first + n_tiles) of the launch: first n_vt_a + n_vt_b of FW_BLOCK new particles each
    // (new particles [0, spawn_a) occupy the slots up to the end of the buffer, [spawn_a, n_spawn) those from slot 0),
    // then one per ring tile (FW_TILE slots) from tile0 on, covering the particles that were there before
    uint32_t tile0;
    uint32_t tile_first, n_tiles;
    uint32_t spawn_a, n_vt_a, n_vt_b;
    // mat = 1: this frame's new particles of the segment were MATERIALISED in the ring before the update (frames with
    // Nested entries: Global ops by fw_k_spawn, children by fw_k_nest) -- n_spawn is 0, the live count is read from the
    // device counters (count + spawned + appended; n_in is the host's value, or 0xFFFFFFFF when only the device knows:
    // a type that receives Nested children) and the particles from index `count` on get their first update (every
    // plane written).  report (or null): pinned host word that receives {epoch << 32 | particles added this frame} --
    // how the host learns the size of each cohort of children, long before it needs it (when the cohort dies)
    uint32_t mat;
    uint32_t n_lplanes;  // FwSeg::n_lplanes (new particles spawned here initialise those planes: fw_init_last_emitted)
    // a Nested entry run INSIDE this launch (FwFifoNest, round 5): 0 = none; otherwise 1 + its index in FwFifoArgs::nest, with
    // FW_FIFO_NEST_CHILD set in the record of the ring that RECEIVES the children (the other one is the parents' ring)
    uint32_t nest;
    unsigned long long *report;
};
#define FW_FIFO_PER_LAUNCH 8
// Nested emission (core.rs:471-546) inside the FIFO launch (round 5; the frame of configs[3] used to be fw_k_nest -- 13.6 us of
// one dependent chain on 192 workgroups moving 4 % of the frame's bytes -- a launch gap, then the update).  When both rings of a
// Nested entry are FIFO rings of the same launch -- parents fed by Global entries only (the host knows their count), spawned
// inside the update kernel (SegHost::virt_parent); children received by a ring nothing else feeds -- the parents' ring tiles do
// the entry's per-parent pass for their own slots BEFORE they update them (no workgroup reads what another one overwrites):
// compute_emission_count per parent, the advanced last_emitted_age stored, the tile's child total published and its exclusive
// prefix taken from a decoupled look-back over the tiles of lower rank (rank = distance from the ring's head tile = list order,
// core.rs:488-544 keeps children parent-major), children spawned wave-cooperatively and given their FIRST UPDATE right there,
// stored once, in the slot they will live in (behind the child ring's live particles).  The child ring's own tiles never see
// them; its bookkeeping workgroup takes the entry's total from the same status words (one more look-back, over all the parent
// tiles -- they have lower workgroup indices) and books count, RNG serial and the cohort report.
struct FwFifoNest {
    uint32_t parent, child;      // indices into FwFifoArgs::s (parent < child: the parents' workgroups come first)
    uint32_t emit, emit_slot;    // -> FwEmit, -> FwGlobals::emit_serial
    uint32_t status_first;       // first look-back word of the entry in FwGlobals::nest_status (tile of rank r: status_first + r)
    uint32_t n_ptiles;           // ring tiles of the parents' ring that take part (ranks 0 .. n_ptiles - 1)
    uint32_t parent_lplane;      // which last_emitted_age plane of the parent type belongs to the entry
    uint32_t tag;                // tag of the look-back words of this launch (fw_ctx::nest_seq)
    uint32_t ticket_base;        // value of FwGlobals::nest_start[emit_slot] when this launch starts (the tile of rank r holds ticket_base + r)
    float n_count, n_start, n_end;  // CountOverDuration of the entry (core.rs:474-481)
    float speed, scale;          // EffectModifier
    uint32_t spin_limit, pad;
};
#define FW_FIFO_NEST_MAX 4
#define FW_FIFO_NEST_CHILD 0x80000000u
#define FW_LDS_OPS 4u  // ops of one segment fw_k_update_stream parks in LDS (table form: pinned host memory otherwise)
#define FW_FIFO_COLL_TILE FW_BLOCK  // ring tile of a FIFO launch with colliding types: one round per workgroup (fw_k_update_fifo: TR)
struct FwFifoArgs {
    FwFifoSeg s[FW_FIFO_PER_LAUNCH];
    uint32_t n_segs, parity, epoch, dbg;
    float dt;
    uint32_t any_inst;
    uint32_t any_coll;  // some segment's particle type has collision settings: the launch runs the COLL instantiation (fw_k_rings.hip: FwCollArm)
    uint32_t small_tiles;  // 1: the host laid the launch out on ring tiles of FW_FIFO_COLL_TILE slots (one round per workgroup):
                           // colliding launches, and launches too small to fill the chip with four-round workgroups
    // which optional planes the particle types of this launch write: bit 0 base colour (gradient not constant), bit 1
    // emissive colour, bit 2 scale (curve not constant) when all its segments agree -- the kernel is then compiled for
    // exactly that set of stores; -1: they differ, read the flags from each type
    int32_t write_mask;
    unsigned long long *done_tag;      // as in FwUpdateArgs
    unsigned long long done_value;
    unsigned long long *host_counts;
    unsigned long long *live_out, *live_next;
    uint32_t n_nest;                   // Nested entries run inside this launch (the NEST instantiations of fw_k_update_fifo)
    uint32_t q0pl;                     // 1: EVERY ring of the launch keeps Q0 (position, age) as four component planes (FwSeg::cpl bit 2,
                                       // SegHost::q0pl: the rings that may run under the age rule -- the host launches them by themselves,
                                       // never with a collider or a Nested entry: the Q0PL instantiations); 0: none does
    FwFifoNest nest[FW_FIFO_NEST_MAX];
    uint32_t spinless;                 // 1: EVERY ring of this q0pl launch carries FW_TYPE_IDX_NOSPIN in it (a type that cannot turn, or a spin
                                       // the launch defers), none has an instance buffer, four-round tiles: no ring tile touches Q2 / Q3 -- the
                                       // SPINLESS instantiations, compiled without registers for them (fw_k_rings.hip); 0: the workgroups find out
                                       // (behind everything else: no other field of the kernel argument moves)
    uint32_t fused;                    // 0, or the DEPTH of a fused launch, 2 .. FW_FUSE_MAX: it runs the frames the host withheld (parity: the first
                                       // one's input rows; their dt and boundaries: FwFuseArgs) and the frame after them (dt, epoch, done_tag,
                                       // host_counts) in one pass over the planes -- spin-less launches only, the fused instantiations
    // (round 22 kept the first frame's dt, spawns and dead of a pair in the 17 words that follow; a group's travel in a record of its own,
    // FwFuseArgs, a fourth kernel argument of the fused kernels alone.  The words stay: this record keeps its size.)
    // FwInlineOps follows this record in the kernel arguments (FwGlobals, FwFifoArgs, FwInlineOps) and began on a 64-byte line of the
    // scalar cache, which the spawning workgroups -- the launch's longest chain -- read their ops through.  Measured, round 22
    // (profiles/r22/fuse2_ab.txt): with 72 bytes more configs[0]'s launch took 1.2-1.4 % longer in three builds, with the
    // record grown by two whole lines it keeps the parent's time
    // (round 26: word FW_FIFO_WHOLE of them is 1 in a spin-less launch whose whole ring tiles may take the arm without a divergent lane --
    // fw_update_fifo_body, fw_fifo_tile_whole: fw_ctx::use_whole_tiles, and every ring of the launch is of a FW_TYPE_DERIVED type, the fact
    // write_mask == 0 travels with -- and 0 everywhere else; the fused forms alone look at it.  No argument moves.)
    // (round 27: word FW_FIFO_NEWBORN is 1 in a launch whose spawning workgroups defer the spin of the particles they spawn into every
    // ring whose spin the launch defers -- FW_TYPE_IDX_NOSPIN with an axis, not FwFifoSeg::mat: fw_spin_newborn_deferred, fw_spin.h -- and
    // 0 under FW_NEWBORN_SPIN=1.  The unfused forms for rings with Q0 in planes read it in their spawning workgroups; for a fused launch,
    // every ring of which defers, the launcher picks the set of kernels by it: fw_k_update_fifo2 or fw_k_update_fifo2_eager.)
    uint32_t fuse_pad[31];
};
#define FW_FIFO_WHOLE 0
#define FW_FIFO_NEWBORN 1
static_assert((sizeof(FwGlobals) + sizeof(FwFifoArgs)) % 64 == 0, "FwInlineOps starts on a 64-byte line of the kernel arguments");
static_assert(sizeof(FwFifoArgs) == 1440, "the size every form of the FIFO kernel was measured with (profiles/r22/fuse2_ab.txt)");
// What a fused launch of depth D = FwFifoArgs::fused knows beside FwFifoArgs (round 23): the FOURTH argument of the fused kernels, behind
// FwInlineOps -- no other kernel's arguments move.  Frames 0 .. D - 2 are the withheld ones, frame D - 1 is the launch's own (FwFifoArgs::dt).
// Per ring of the launch (FwFifoSeg: head / n_in are the first frame's, n_spawn and dead the sums over the group): new particle k of the
// ring was spawned by the first frame f with k < spawn_end[f] (cumulative; the last frame's bound is FwFifoSeg::n_spawn) and gets the
// updates of the frames f .. D - 1; frame f destroys dead[f] particles, all of them in the ring before the group (fw_fuse2.h).
struct FwFuseArgs {
    float dt_pre[FW_FUSE_MAX - 1];
    uint32_t pad;
    uint32_t spawn_end[FW_FIFO_PER_LAUNCH][FW_FUSE_MAX - 1];
    uint32_t dead[FW_FIFO_PER_LAUNCH][FW_FUSE_MAX - 1];
    // (round 30) per ring, the four words of its type's record a WHOLE ring tile computes with -- FwType::acc[0 .. 2], FwType::lin_drag:
    // constants of the type, copied where the ring's record is built (ring_record, like FwFifoSeg::life) -- so that such a tile loads
    // nothing of the record (fw_update_fifo_body: FwMoveK)
    float move[FW_FIFO_PER_LAUNCH][4];
};
// (round 24, FW_FUSE_MAX = 8: 480 bytes.  The record is the LAST argument, so its size moves nobody else's; FW_INLINE_OPS stays 8 -- FwInlineOps
// sits in front of it -- so a launch whose rings carry two ops per frame closes its groups at four frames: FwWithheld::join declines the fifth)
// (round 30: + 128 bytes, four words per ring)
static_assert(sizeof(FwFuseArgs) == 32 + 2 * FW_FIFO_PER_LAUNCH * (FW_FUSE_MAX - 1) * 4 + FW_FIFO_PER_LAUNCH * 16,
              "dt_pre and a pad word, two tables of FW_FUSE_MAX - 1 words per ring, four words per ring");
static_assert(sizeof(FwGlobals) + sizeof(FwFifoArgs) + sizeof(FwInlineOps) + sizeof(FwFuseArgs) <= 4096, "the fused kernels' arguments fit the 4096-byte kernel-argument limit");
// The far tier (round 32): a launch of depth 9 .. FW_FUSE_FAR.  Withheld frames 0 .. FW_FUSE_MAX - 2 stay where the first tier keeps them,
// FwFuseArgs -- no argument of anybody moves --; withheld frames FW_FUSE_MAX - 1 .. FW_FUSE_FAR - 2 travel here, a FIFTH argument of the
// far kernels alone (fw_k_rings_far.hip): index f - (FW_FUSE_MAX - 1).  fw_update_fifo_body reads a withheld frame through one accessor
// that picks the record by the frame's compile-time index.
#define FW_FAR_FIRST (FW_FUSE_MAX - 1)
struct FwFarArgs {
    float dt[FW_FUSE_FAR - FW_FUSE_MAX];
    uint32_t spawn_end[FW_FIFO_PER_LAUNCH][FW_FUSE_FAR - FW_FUSE_MAX];
    uint32_t dead[FW_FIFO_PER_LAUNCH][FW_FUSE_FAR - FW_FUSE_MAX];
};
static_assert(sizeof(FwFarArgs) == (FW_FUSE_FAR - FW_FUSE_MAX) * 4 * (1 + 2 * FW_FIFO_PER_LAUNCH), "one dt and, per ring, two boundaries per far frame");
static_assert(sizeof(FwGlobals) + sizeof(FwFifoArgs) + sizeof(FwInlineOps) + sizeof(FwFuseArgs) + sizeof(FwFarArgs) <= 4096,
              "the far kernels' arguments fit the 4096-byte kernel-argument limit");
// The two records' one owner on the host (FwFifoLaunch; fw_launch_update_fifo passes each kernel the record it takes): withheld frame w of a
// group -- 0 .. FW_FUSE_FAR - 2 -- through one accessor, whichever record holds it.  (The kernel has its own, by the frame's compile-time
// index: dt_w, spawn_end_w, dead_w, fw_k_rings.hip.)
struct FwFuseRecords {
    FwFuseArgs fz;
    FwFarArgs far;
    float &dt(uint32_t w) { return w < FW_FAR_FIRST ? fz.dt_pre[w] : far.dt[w - FW_FAR_FIRST]; }
    uint32_t &spawn_end(uint32_t j, uint32_t w) { return w < FW_FAR_FIRST ? fz.spawn_end[j][w] : far.spawn_end[j][w - FW_FAR_FIRST]; }
    uint32_t &dead(uint32_t j, uint32_t w) { return w < FW_FAR_FIRST ? fz.dead[j][w] : far.dead[j][w - FW_FAR_FIRST]; }
    float dt(uint32_t w) const { return const_cast<FwFuseRecords *>(this)->dt(w); }
    uint32_t spawn_end(uint32_t j, uint32_t w) const { return const_cast<FwFuseRecords *>(this)->spawn_end(j, w); }
    uint32_t dead(uint32_t j, uint32_t w) const { return const_cast<FwFuseRecords *>(this)->dead(j, w); }
    // what a frame that joins a group carries: the group's tables so far (null: no withheld frame has written one yet -- zeros) and the rings'
    // constants, which every frame's launch brings itself: its own `move` rows
    void continue_from(const FwFuseRecords *group) {
        FwFuseRecords r = group ? *group : FwFuseRecords{};
        for (uint32_t j = 0; j < FW_FIFO_PER_LAUNCH; j++)
            for (uint32_t c = 0; c < 4; c++) r.fz.move[j][c] = fz.move[j][c];
        *this = r;
    }
};

// ---- range rings: particle types whose lifetime is a RANGE, updated in place ---------------------------------------
// Ages never increase along the particle list (everybody is born with age 0 behind all older particles and every update
// adds the same dt, core.rs:523, 594) and nobody dies before `age + dt >= lifetime.min`: only a PREFIX of the list -- the
// OLD part -- can lose particles in an update; everybody younger is in the situation of a FIFO ring particle.  Such a type
// lives in ONE buffer used as a ring:   [ ... free ... | old survivors | young | free ... ]
//   * the YOUNG part is updated in place (a lane owns its slot from load to store; no counting, no look-back, any dt);
//     the host knows it exactly -- it made every spawn count and replays the fp32 age of every spawn cohort -- as
//     {b = slot of the first young particle, y = their number};
//   * the OLD part [b - n_old, b) is compacted IN PLACE towards the young part (order kept): a tile of 1024 holds its
//     whole input in registers before it publishes its survivor count, so the tiles further from b -- which need that
//     count for their offset, and whose survivors land in slots of the tiles nearer to b -- cannot overwrite anything
//     that is still to be read.  Tiles nearer to b have lower workgroup indices: whoever is waited for is resident or done;
//   * cohorts whose age reaches lifetime.min simply join the old part: b moves, nothing is copied;
//   * new particles are spawned at the tail, in the slot they will live in.
// The first particle of the list sits in slot b - n_old: `n_old` = count - y is known to the device only.
struct alignas(16) FwRangeRec {  // per segment, per frame: pinned host memory, read by the tiles in place
    uint32_t b;         // slot of the first young particle, after this frame's cohorts have joined the old part
    uint32_t y_exist;   // young particles before this frame's spawns (host-known; FW_RREC_DEV: unknown, the device derives it)
    uint32_t n_spawn;   // particles spawned this frame by the NEW workgroups (all of them outlive the step: dt < lifetime.min)
    uint32_t op0, op_n; // their spawn ops in FwRangeArgs::ops
    uint32_t grad;      // particles that joined the old part this frame (b moved by so many slots): old part = rold + grad
    uint32_t flags;     // FW_RREC_*
    uint32_t ticket_base;  // value of FwGlobals::range_ticket[segment] when this launch starts (its OLD workgroup of rank k holds ticket_base + k)
    unsigned long long *report;  // FW_RREC_DEV: pinned host word that receives {epoch << 32 | particles added this frame}
    unsigned long long pad2;
};
// Range rings of spawners WITH Nested entries (core.rs:471-546):
// FW_RREC_MAT  this frame's new particles of the segment were MATERIALISED behind the young part before the update (frames
//              with a Nested pass: Global ops by fw_k_spawn -- the per-parent pass must find them in memory, core.rs:488 --
//              children by fw_k_nest): n_spawn is 0, the device counters say how many (spawned + appended), and those
//              particles get their first update with every plane written;
// FW_RREC_DEV  the type receives Nested children: how many particles it holds is known to the device only -- the young
//              count is  count + spawned + appended - (rold + grad)  -- and the size of each frame's cohort reaches the host
//              through `report`, long before the host needs it (when the cohort joins the old part).
#define FW_RREC_MAT 1u
#define FW_RREC_DEV 2u
#define FW_RANGE_OLD 0u
#define FW_RANGE_NEW 1u
#define FW_RANGE_YOUNG 2u
struct alignas(16) FwRangeDesc {  // per workgroup (device table, re-sent only when a bound leaves its band)
    uint32_t seg;
    uint32_t role_k;     // role << 30 | index of the workgroup within its role and segment
    uint32_t old_first;  // index of the segment's first look-back word in FwRangeArgs::status (its OLD workgroup k uses word old_first + k)
    uint32_t type_idx;   // | FW_TYPE_IDX_NOSPIN
    uint32_t keys_off, keys_len;
    uint32_t n_old;      // OLD workgroups the table provides for the segment (the kernel checks the old part against it)
    uint32_t pad;
};
struct FwRangeArgs {
    const FwRangeDesc *desc;
    const FwRangeRec *recs;         // [max_seg] indexed by segment (pinned host)
    const FwOp *ops;                // this frame's spawn ops of range segments (pinned host)
    unsigned long long *status;     // look-back words of the OLD workgroups (FwRangeDesc::old_first + k)
    uint32_t total_tiles, parity, epoch, spin_limit, dbg;
    float dt;
    uint32_t any_inst;              // some segment has a windowed instance buffer attached: the kernels that also write records
    uint32_t any_coll;              // some segment's particle type has collision settings: the COLL instantiation (FwCollArm)
    uint32_t small_tiles;           // 1: OLD and YOUNG workgroups cover ONE round (256 slots) each: the host laid the launch out so
                                    // (colliding launches, and launches too small to fill the chip with four-round workgroups)
    uint32_t young_rounds;          // rounds of a YOUNG workgroup of a four-round launch: 4, or 2 (launches of large segments, no records)
    unsigned long long *done_tag;   // as in FwUpdateArgs
    unsigned long long done_value;
    unsigned long long *host_counts;
    unsigned long long *live_out, *live_next;
    unsigned long long *ts;         // FW_DEBUG & 8: 8 words per workgroup {start, 0, 0, end of wave 0, role_k, seg, 0, 0} (profiling)
};
#define FW_RANGE_MAX_CAPACITY 0x10000000u  // slots are addressed as 32-bit byte offsets into a float4 plane

// ---- small particle types: one WAVE per (spawner, particle type) (fw_k_small.hip, round 5) ---------------------------------
// A type of a few hundred particles needs no workgroup, no tile table, no look-back and no forecast: a wave walks its list in
// rounds of 64, a ballot + a running count give the stable compaction (core.rs:589-659), its uniform values live in the wave's own
// scalar registers -- four types per workgroup, thousands of emitters resident at once.  Same ping-pong layout as the compacting
// path: a type enters and leaves the mode by a host flag (SegHost::small).
struct FwSmallArgs {
    const uint32_t *list;          // [n] segments of the launch (device): n_narrow types a wave walks, then n - n_narrow WIDE ones
                                   // (up to a few thousand particles: a workgroup each)
    uint32_t n, n_narrow, parity, epoch;
    uint32_t any_inst;             // some type of the launch has an instance buffer attached (FwSeg::inst): the INST instantiation
    uint32_t any_coll;             // ... collision settings (FwTypeColl): the COLL instantiation
    float dt;
    const uint4 *seg_op_first;     // as FwUpdateArgs (table form: pinned host memory), or null: no virtual spawns this frame
    const FwOp *ops;
    uint32_t force_colors, dbg;
    unsigned long long *done_tag;  // as in FwUpdateArgs
    unsigned long long done_value;
    unsigned long long *host_counts;
    unsigned long long *live_out, *live_next;
};
hipError_t fw_launch_update_small(hipStream_t s, const FwGlobals &g, const FwSmallArgs &a, hipEvent_t ev_start = nullptr,
                                  hipEvent_t ev_stop = nullptr);

enum { FW_SPAWN_NONE = 0, FW_SPAWN_INLINE = 1, FW_SPAWN_TABLE = 2 };

enum { FW_MODE_FUSED = 0, FW_MODE_SPLIT = 1, FW_MODE_SPLIT_COLL = 2 };  // SPLIT_COLL: frames with colliding particle types

// d_ops: device table, or null -> the (at most FW_INLINE_OPS) ops at h_ops travel in the kernel arguments
hipError_t fw_launch_spawn(hipStream_t s, const FwGlobals &g, const FwOp *d_ops, const FwOp *h_ops, uint32_t n_ops,
                           uint32_t total_blocks, uint32_t parity);
hipError_t fw_launch_fc_resolve(hipStream_t s, const FwGlobals &g, const FwResolveArgs &a);
hipError_t fw_launch_update(hipStream_t s, const FwGlobals &g, const FwUpdateArgs &a, const FwInlineOps *inl,
                            int spawn_form, int mode, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// in-place update of up to FW_FIFO_PER_LAUNCH FIFO segments (their spawn ops in `inl`): the one entry of every FIFO launch.  `rec`: the
// withheld frames of a fused launch (FwFifoArgs::fused >= 2), wanted for such a launch and for no other; null: an unfused one
hipError_t fw_launch_update_fifo(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl,
                                 uint32_t total_tiles, int nt, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const FwFuseRecords *rec = nullptr);
// The units behind it, one per set of fused kernels -- fw_launch_update_fifo routes by FwFifoArgs::fused, nobody else calls them:
// fused = 2 .. FW_FUSE_MAX, fw_k_rings_fuse2.hip -- which forwards to fw_k_rings_fuse2_eager.hip, the forms whose spawning workgroups spin
// what they spawn (round 27), where FwFifoArgs::fuse_pad[FW_FIFO_NEWBORN] is 0 --; fused = FW_FUSE_MAX + 1 .. FW_FUSE_FAR, fw_k_rings_far.hip
// (no eager forms: under FW_NEWBORN_SPIN=1 the host closes its groups at FW_FUSE_MAX, and a launch that says otherwise is refused)
hipError_t fw_unit_update_fifo2(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                                uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1);
hipError_t fw_unit_update_fifo2_eager(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                                      uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1);
hipError_t fw_unit_update_fifo_far(hipStream_t s, const FwGlobals &g, const FwFifoArgs &a, const FwInlineOps &inl, const FwFuseArgs &fz,
                                   const FwFarArgs &far, uint32_t total_tiles, int nt, hipEvent_t e0, hipEvent_t e1);
uint32_t fw_range_young_tile(void);  // ring slots a YOUNG workgroup of fw_k_update_range covers (a build-time choice)
// in-place update of every range ring of the context (all_nospin: no segment of the launch keeps a rotation plane)
// nt: which form of the kernel (fw_dev.h: fw_ld4w): 0 plain, 1 the write-only planes non-temporal, 2 every plane access
hipError_t fw_launch_update_range(hipStream_t s, const FwGlobals &g, const FwRangeArgs &a, bool all_nospin, int nt,
                                  hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
hipError_t fw_launch_nested(hipStream_t s, const FwGlobals &g, const FwNestOp *d_ops, const FwNestOp *h_ops, uint32_t n_ops,
                            uint32_t total_tiles, uint32_t parity, uint32_t tag, uint32_t spin_limit, uint32_t dbg = 0);
// ---- the readers of a segment's particles outside the update kernels (fw_k_aux.hip) --------------------------------
// fw_k_gather (fw_particle records), fw_k_pack (ParticleInstance records), fw_k_aabb, fw_k_rederive and fw_k_restore_q3 all
// have to know how a segment stores its particles.  FwSegView says it once; the host fills it in ONE place (seg_view,
// fw_engine_mem.cpp: every field from SegHost) and the device reads it through ONE set of functions (fw_view_*, fw_k_aux.hip):
//   in which slot is particle 0?            head / d_rold       SegHost::enqueue_head(), or ring_head_exact (seg_view_exact)
//   Q1 / Q3 in component planes?  Q2?  Q0?  cpl                 SegHost::cpl_bits()
//   a rotation plane, or one rotation?      nospin / rot        SegHost::nospin, const_rot
//   where is the lifetime?                  life_plane / const  SegHost::life_plane(), fifo_life -- read under `nospin` only
//   scale and colours stored, or evaluated? derived / keys      SegHost::derived
//   which buffer, how many slots?           buf / capacity      SegHost::buf[parity], capacity
struct FwSegView {
    char *buf;
    uint32_t capacity;
    uint32_t head;           // slot of particle 0 -- or, d_rold set, of the ring's first YOUNG particle
    const uint32_t *d_rold;  // null, or -- a range ring -- the segment's word of FwGlobals::rold: particle 0 sits so many slots before `head`
    uint32_t cpl;            // FwSeg::cpl -- bit 0: a ring, its Q1 / Q3 regions are component planes; bit 1: a FIFO ring, Q2 as well; bit 2: ... and Q0 (fw_dev.h)
    uint32_t nospin;         // FW_TYPE_NOSPIN: the rotation plane is not maintained and Q3 is not read -- every particle has
    float4 rot;              //   this rotation, angular velocity 0,
    uint32_t life_plane;     //   and its lifetime in this plane behind the last_emitted_age planes, or -- 0xFFFFFFFF: a FIFO ring --
    float life_const;        //   this one value
    const FwType *derived;   // null, or the type's device record when it is FW_TYPE_DERIVED: scale and colours are evaluated, not read,
    const float *keys;       //   from the key pool
};
// SoA -> AoS gather of the first `n` particles of a segment into fw_particle records (device)
hipError_t fw_launch_gather(hipStream_t s, const FwSegView &v, uint32_t n, int32_t pbr, void *d_out);
// fills the scale / colour planes of every slot from age, lifetime and initial_scale (a type leaves FW_TYPE_DERIVED: v.derived is still set)
hipError_t fw_launch_rederive(hipStream_t s, const FwSegView &v);
// the age plane of a FIFO ring from its cohort table (fw_ages.h: n FwAgeEntry records in device memory), for logical particles [0, live)
hipError_t fw_launch_fifo_ages(hipStream_t s, char *buf, uint32_t capacity, uint32_t head, uint32_t live, const void *d_table, uint32_t n);
// the deferred spin of a FIFO ring replayed (fw_spin.h: n FwSpinEntry records, then log_n fp32 dt values, in device memory), for logical
// particles [0, live): rotation component axis - 1, rotation w and angular-velocity component axis - 1 of every particle with pending steps
hipError_t fw_launch_fifo_spin(hipStream_t s, char *buf, uint32_t capacity, uint32_t head, uint32_t live, const FwType *type, uint32_t axis,
                               const void *d_table, uint32_t n, uint32_t log_n);
hipError_t fw_launch_fill_plane1(hipStream_t s, char *buf0, char *buf1, size_t plane_off, uint32_t capacity, float v);
// A type leaves FW_TYPE_NOSPIN, in one (buf1 == nullptr) or both buffers of its segment: Q3 = {0, 0, 0, lifetime} again, and the
// rotation plane, which nobody maintained, filled with the type's one rotation.  cpl, life_plane, life_const: as in FwSegView
hipError_t fw_launch_restore_q3(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, uint32_t life_plane, float life_const, uint32_t cpl);
hipError_t fw_launch_fill_rotation(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, const float rot[4], uint32_t cpl);
hipError_t fw_launch_scatter(hipStream_t s, char *buf, uint32_t capacity, uint32_t n, uint32_t n_lplanes,
                             const void *d_in);
// fills the base / emissive colour planes of one (buf1 == nullptr) or both buffers of a segment (capacity slots each)
hipError_t fw_launch_fill_colors(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, const float bc[4], const float em[4]);
// ParticleInstance records of the first min(*d_count, n_upper) particles of a segment (the count is the device's: no synchronisation)
hipError_t fw_launch_pack_instances(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, void *d_out);
// Depth-sorted records (fw_sort.h; the sort itself: fw_k_sort.hip).  All three take n = min(*d_count, n_upper) from the device.
//   keys:   d_key[li] = sort key of list particle li under `sv`, d_idx[li] = li, for li < n
//   sort:   the n pairs at the start of `scratch` (keys at [0, n_upper), indices at [n_upper, 2 * n_upper); fw_sort_scratch_words(n_upper)
//           words in all) sorted by ascending key, ties in incoming order; the sorted indices end at scratch + n_upper or, d_idx_out
//           not null, there instead (n entries; nothing at or beyond n is written)
//   pack:   as fw_launch_pack_instances, record j that of list particle d_order[j]
struct FwSortView;
hipError_t fw_launch_depth_keys(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, const FwSortView &sv, uint32_t *d_key,
                                uint32_t *d_idx);
hipError_t fw_launch_sort_pairs(hipStream_t s, const uint32_t *d_count, uint32_t n_upper, uint32_t *scratch, uint32_t *d_idx_out);
hipError_t fw_launch_pack_instances_sorted(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, const uint32_t *d_order,
                                           void *d_out);
// box of position -/+ scale over up to eight segments: seg_ids, views: host arrays of n_segs (views[i] for buffer `parity` of
// seg_ids[i]); d_part: device scratch of 256 * 8 floats; h_out8: PINNED host {min.xyz, any, max.xyz, -}
hipError_t fw_launch_aabb(hipStream_t s, const FwGlobals &g, const uint32_t *seg_ids, const FwSegView *views, uint32_t n_segs,
                          uint32_t parity, float *d_part, float *h_out8);
// the same query answered from the per-tile boxes of the last update (epoch = that update's)
hipError_t fw_launch_aabb_from_tiles(hipStream_t s, const FwGlobals &g, const uint32_t *seg_ids, uint32_t n_segs,
                                     uint32_t parity, uint32_t epoch, const uint32_t *d_seg_tile_first, float *h_out8);
// The boxes of many spawners in two launches (fw_boxes.h; fw_k_boxes / fw_k_boxes_fold).  One entry per listed (spawner, type) segment:
struct FwBoxEntry {
    FwSegView v;
    const uint32_t *d_count;  // the segment's live count, as the kernels keep it (count_slot)
    uint32_t bound;           // host-known upper bound of that count: list positions at or beyond it are never read
    uint32_t chunk0;          // chunks of the entries in front of this one (fw_boxes_plan)
};
struct FwBoxPlace;
// d_tab, d_places: the two tables in device memory (n_entries, n_places records; total_chunks: the plan's); d_part: device scratch of
// total_chunks * 8 floats; out_records: n_places fw_aabb records, device memory or PINNED host memory.  *launches: kernels enqueued
hipError_t fw_launch_boxes(hipStream_t s, const FwBoxEntry *d_tab, uint32_t n_entries, const FwBoxPlace *d_places, uint32_t n_places,
                           uint32_t total_chunks, float *d_part, void *out_records, uint32_t *launches);
// The particles of many places inside many volumes in two launches (fw_volumes.h; fw_k_volumes / fw_k_volumes_fold).  The tables are the
// batched boxes'; d_volumes: n_volumes records in device memory; d_part: device scratch of total_chunks * n_volumes uint32, [volume][chunk];
// out_counts: n_places * n_volumes uint32, device or pinned host memory.  *launches: kernels enqueued -- two, or one where total_chunks == 0
hipError_t fw_launch_volumes(hipStream_t s, const FwBoxEntry *d_tab, uint32_t n_entries, const FwBoxPlace *d_places, uint32_t n_places, uint32_t total_chunks,
                             const FwCollider *d_volumes, uint32_t n_volumes, uint32_t *d_part, void *out_counts, uint32_t *launches);
hipError_t fw_launch_total(hipStream_t s, const uint32_t *counts, uint32_t n_seg, unsigned long long *d_out);
hipError_t fw_launch_copy_probe(hipStream_t s, const void *src, void *dst, size_t bytes);
// Refit of a deformable mesh (fw_k_refit.hip): the levels of R.order, lowest first -- one launch per level of more than
// FW_REFIT_TAIL nodes, then one launch of one workgroup for all the others.  level_off: n_levels + 1 words, on the device
// and (the same) on the host.  No workgroup waits for another; everything goes to stream s.
#define FW_REFIT_TAIL 4096u
hipError_t fw_launch_mesh_refit(hipStream_t s, const FwRefit &R, const uint32_t *d_level_off, const uint32_t *h_level_off,
                                uint32_t n_levels);
// Vertices that are already in device memory (fw_ctx_update_mesh_vertices_device; fw_mesh_bounds.h has the arithmetic).
// fw_launch_mesh_bounds: one launch of fw_mesh_bounds_partials(n_vertices) workgroups (capped: this is latency, not bandwidth)
// leaves a partial each in d_partials, a second launch of ONE workgroup folds them into the mesh's record and the pinned
// report.  seed (may be null): the box the record takes when this update is rejected (the host's, which held until now).
#define FW_BOUNDS_BLOCK 256
#define FW_BOUNDS_MAX_GRID 256u
struct FwMeshSeed {
    float lo[3], hi[3], pad;
};
uint32_t fw_mesh_bounds_partials(uint32_t n_vertices);
hipError_t fw_launch_mesh_bounds(hipStream_t s, const float *d_xyz, const uint8_t *d_referenced, uint32_t n_vertices, FwVtxAcc *d_partials,
                                 FwMeshRecord *d_rec, FwMeshReport *h_report, const FwMeshSeed *seed);
// the bounding spheres of the instances in d_inst[0 .. n_inst) whose tables start at `nodes`, rewritten from the record's box;
// after_update: nothing when the record says the latest update was rejected
hipError_t fw_launch_mesh_spheres(hipStream_t s, FwMeshInst *d_inst, uint32_t n_inst, const float4 *nodes, const FwMeshRecord *d_rec,
                                  bool after_update);
// The ray-cast query (fw_k_query.hip; fw_ctx_cast_rays[_device]): n fw_ray records at d_rays -> n fw_ray_hit records at d_hits, both
// device memory, against g's collider world as of the launch's place in stream s (launches of at most 2^30 rays each).
hipError_t fw_launch_cast_rays(hipStream_t s, const FwGlobals &g, const void *d_rays, uint64_t n, void *d_hits);
// The point query (fw_k_query.hip; fw_ctx_project_points[_device]): n fw_point records (16 bytes) at d_points -> n fw_point_projection
// records (32 bytes) at d_out, in the same way.
hipError_t fw_launch_project_points(hipStream_t s, const FwGlobals &g, const void *d_points, uint64_t n, void *d_out);
// The path query (fw_k_query.hip; fw_ctx_trace_paths[_device]): n fw_path records (32 bytes) at d_paths -> n fw_path_result records (80
// bytes) at d_out and, d_samples not null, settings.n_steps * n float4 {position, age} at d_samples[step * n + path]; settings
// (fw_trace.h) travel in the kernel arguments.
struct FwPathSettings;
hipError_t fw_launch_trace_paths(hipStream_t s, const FwGlobals &g, const FwPathSettings &settings, const void *d_paths, uint64_t n, void *d_out,
                                 void *d_samples);
