/*
 * firework_hip_debug.h -- measurement and debugging hooks of libfirework_hip.so.
 *
 * NOT part of the drop-in boundary (include/firework_hip.h is what a host binds): these entry points exist for bench.py,
 * the tools under tools/ and the tests -- kernel timing by events attached to the dispatches, the copy-bandwidth probe of
 * the measured roofline, in-kernel timestamps, and which update path a particle type is on.  They may change between
 * builds without an ABI version bump.
 *
 * Environment knobs.  The library reads A/B and debugging switches from the environment (FW_FIFO, FW_RANGE, FW_NOSPIN, FW_AXIS_SPIN, FW_AGELESS,
 * FW_FORECAST, FW_UPDATE_MODE, FW_DEBUG, ...; DESIGN.md section 7 lists them) ONLY when FW_ENABLE_KNOBS=1 is set: a
 * product process never changes behaviour because of a stray variable.  The tests and the tools set it.
 */
#ifndef FIREWORK_HIP_DEBUG_H
#define FIREWORK_HIP_DEBUG_H

#include "firework_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP-event timing of the dominant kernel on the context's stream: enable, run
 * steps, then read (sum of kernel durations in ms, number of launches).  The start / stop
 * events are attached to the update dispatch itself (hipExtLaunchKernel), so each pair
 * spans exactly the kernel's begin / end timestamps -- the duration rocprofv3 reports. */
fw_status fw_ctx_kernel_timing(fw_ctx *ctx, int32_t enable);
fw_status fw_ctx_kernel_timing_read(fw_ctx *ctx, double *ms_total, uint64_t *launches, uint64_t *particles);
/* cost of an empty hipEventRecord pair on the stream (informational; nothing is subtracted from the figure above) */
fw_status fw_ctx_kernel_timing_overhead(fw_ctx *ctx, double *ms_per_pair);
/* device-to-device copy bandwidth probe (bytes moved R+W per second) for the measured-roofline line */
fw_status fw_ctx_measure_copy_bandwidth(fw_ctx *ctx, uint64_t bytes, int32_t iters, double *bytes_per_s);

/* in-kernel timestamps of the update kernel when the context was created under FW_DEBUG=8 (tools/tile_timeline.py,
 * tools/launch_gaps.py): per tile {entry, after the count barrier, after the prefix, end, 4 more phase marks} of the
 * last launch (and of the one before it: `prev`); {~earliest start [64], latest end [64]} of the last 256 launches */
fw_status fw_debug_read_timestamps(fw_ctx *ctx, unsigned long long *out, uint64_t max_tiles, uint64_t *n_tiles);
fw_status fw_debug_read_timestamps2(fw_ctx *ctx, unsigned long long *out, unsigned long long *prev, uint64_t max_tiles,
                                    uint64_t *n_tiles);
fw_status fw_debug_read_launches(fw_ctx *ctx, unsigned long long *out32768, uint32_t *epoch);
/* ... and of the last range-ring launch (tools/range_timeline.py): 8 words per workgroup {start, 0, 0, end of its wave 0,
 * role << 30 | k, segment, 0, 0} */
fw_status fw_debug_read_range_timestamps(fw_ctx *ctx, unsigned long long *out, uint64_t max_tiles, uint64_t *n_tiles);
/* which update path a particle type is on (1 = FIFO ring updated in place, 2 = range ring: young part in place, old part
 * compacted in place, 0 = general compacting path), the bytes one
 * update of a live particle moves on it, and how many of those are algorithmic (bench.py's roofline accounting).  A FIFO ring
 * whose latest launch ran D = 2 .. 8 frames of it in one pass (fw_debug_fuse2) reports that launch's bytes divided by D */
fw_status fw_debug_update_path(fw_ctx *ctx, fw_spawner spawner, uint32_t type, int32_t *mode, uint32_t *moved_bytes,
                               uint32_t *algorithmic_bytes);
/* the context's segments by update path, as the host keeps the census (kept[11]) and as a recount over its segment records gives it
 * (recounted[11]): in use, FIFO rings, range rings, few-rings, spilled rings, on the wave-per-type kernel, eligible for it, colliding
 * ones on it, with an instance buffer, solo; then the few-segments hysteresis (1: blocked), which is history and the same in both.
 * The two halves are equal at all times.  Host state only: no synchronisation, a withheld launch stays withheld */
fw_status fw_debug_path_census(fw_ctx *ctx, uint32_t *kept, uint32_t *recounted);

/* frames with Nested entries stepped so far: those whose entries ran INSIDE the FIFO ring launch (one launch per frame, DESIGN.md
 * 4.0) and those that ran the separate fw_k_spawn / fw_k_nest passes first */
fw_status fw_debug_nest_frames(fw_ctx *ctx, uint64_t *fused, uint64_t *separate);

/* tiles of the compacting launch's tile table as of the last fw_step, and how many entries each per-tile array of the context (status
 * words, forecast entries, tile boxes) holds: the first never exceeds the second (fw_step refuses the frame otherwise) */
fw_status fw_debug_tile_scratch(fw_ctx *ctx, uint64_t *table_tiles, uint64_t *scratch_tiles);

/* rings that fw_step moved to the compacting path -- particles and order kept -- because the device's report of a cohort size was
 * still missing when the cohort was due (a failed check of the host's bookkeeping that is found BEFORE the frame is committed:
 * recoverable) */
fw_status fw_debug_recovered_rings(fw_ctx *ctx, uint64_t *n);

/* frames of the compacting launch that ran under a dt different from the previous frame's on the STREAMING schedule (threshold
 * forecast: fw_k_fc_resolve in front of fw_k_update_stream) instead of the decoupled look-back */
fw_status fw_debug_tf_frames(fw_ctx *ctx, uint64_t *n);

/* launches so far of the kernel that writes the ages of a FIFO ring under the age rule back from the host's spawn cohorts (DESIGN.md
 * 4.0): one per read or copy of such a ring's particles after frames that did not move the age plane, none for a call that only
 * asks for counts */
fw_status fw_debug_age_launches(fw_ctx *ctx, uint64_t *n);

/* *n = launches of the kernel that replays the deferred spin of a FIFO ring (fw_k_fifo_spin) so far: one per call that reads or copies
 * the particles of a ring whose latest frames left rotation and angular velocity alone, none for
 * fw_spawner_aabb or a call that only asks for counts */
fw_status fw_debug_spin_launches(fw_ctx *ctx, uint64_t *n);

/* *n = FIFO launches so far that ran the kernel form compiled for launches in which no ring tile touches rotation or angular velocity
 * (DESIGN.md 4.0, round 21): every ring of the launch cannot turn or has its spin deferred in it, none has an instance buffer attached,
 * four-round tiles.  FW_SPINLESS=0 (with FW_ENABLE_KNOBS) keeps such launches on the form that finds out per workgroup: 0 then */
fw_status fw_debug_spinless_launches(fw_ctx *ctx, uint64_t *n);

/* Whole ring tiles: a ring tile of a spin-less launch every slot of which holds a particle that was in the ring
 * before the launch and lives through it issues all of its loads first and never waits for a store.  *tiles = the ring tiles so far that
 * the host's evaluation of the kernel's predicate (fw_fifo_tile_whole) called whole, in launches that allow the arm (every ring of a type
 * whose scale and colours are left to its readers, new particles not materialised); *launches = the launches with at least one.
 * The kernels that run two to eight frames in one launch take the arm for exactly these tiles; a launch of one frame counts its whole
 * tiles too and keeps the streaming loop for them (measured: the arm loses there).
 * FW_WHOLE_TILES=0 (with FW_ENABLE_KNOBS) keeps every tile on the streaming loop: both stay 0.  Either pointer may be null */
fw_status fw_debug_whole_tiles(fw_ctx *ctx, uint64_t *launches, uint64_t *tiles);

/* The spin of newborn particles: a launch that defers a ring's spin defers it for the particles it spawns into
 * that ring as well -- its spawning workgroups store the spawn-time rotation and angular velocity, and the replay applies the frame's own
 * log entry to them.  *launches = the launches so far, of one frame or of several, that went to the stream with at least one ring under
 * the rule.  A ring of a type that cannot turn, a ring that does not defer and a ring whose new particles are materialised by another
 * kernel are not under it.  FW_NEWBORN_SPIN=1 (with FW_ENABLE_KNOBS) restores the eager rule -- a new particle gets its first update's
 * spin from the launch -- everywhere: 0 then */
fw_status fw_debug_newborn_spin(fw_ctx *ctx, uint64_t *launches);

/* Several frames of unread FIFO rings in one launch (rounds 22 to 24).  *fused = launches so far that ran one or more
 * withheld frames and the frame after them in one pass over the planes; *flushed = withheld frames that went to the stream alone,
 * because the next frame did not qualify, the pair was declined, or somebody touched the stream or the particles first.  A frame is
 * withheld only when its one launch is spin-less, every ring of it deferred its spin in it and holds FW_FUSE2_MIN particles (default
 * 384 tiles); a group grows beyond two frames, up to FW_FUSE_DEPTH (2 to 8, default 8), only where every ring holds FW_FUSE_DEEP_MIN
 * particles (default 768 tiles), and beyond four only where every ring holds FW_FUSE_WIDE_MIN as well (default 768 tiles).  A launch
 * whose rings carry more than one spawn op per frame closes its groups earlier: eight ops travel in a launch.  Round 32, the far
 * tier: with FW_FUSE_DEPTH unset or 8 a group grows up to FW_FUSE_FAR_DEPTH frames (8 to 16, 8 = off, default 16) where every ring holds
 * FW_FUSE_FAR_MIN particles too (default 768 tiles); there, consecutive frames' ops of an emitter that stands still travel as one op.
 * FW_FUSE2=0 (with
 * FW_ENABLE_KNOBS) withholds nothing: both stay 0.  Either pointer may be null */
fw_status fw_debug_fuse2(fw_ctx *ctx, uint64_t *fused, uint64_t *flushed);
/* *frames = the frames run by fused launches so far: a launch that ran D frames counts D (so *frames / *fused is the mean depth) */
fw_status fw_debug_fuse_frames(fw_ctx *ctx, uint64_t *frames);

/* *on = 1: the context keeps the per-frame records of its range launches and its small op tables in DEVICE memory that the host writes
 * through the large BAR; 0: in pinned host memory (the platform does not map device memory for the host, or
 * FW_PARAM_BAR=0) */
fw_status fw_debug_param_bar(fw_ctx *ctx, int32_t *on);

/* The batched boxes (firework_hip.h: BATCHED BOXES).  *launches = kernel launches fw_ctx_aabbs and fw_ctx_aabbs_device have enqueued so
 * far: two per call whatever n is (one where no listed particle type can hold a particle: there is nothing to read); *chunks = the
 * chunks -- waves of the first launch -- of the latest call; *chunk_size = list positions per chunk.  Any pointer may be null */
fw_status fw_debug_aabb_batch(fw_ctx *ctx, uint64_t *launches, uint64_t *chunks, uint32_t *chunk_size);

/* The volume queries (firework_hip.h: VOLUME QUERIES).  *launches = kernel launches fw_ctx_count_in_volumes and
 * fw_ctx_count_in_volumes_device have enqueued so far: two per call whatever the sizes (one where no listed particle type can hold a
 * particle); *chunks = the chunks -- waves of the first launch -- of the latest call; *chunk_size = list positions per chunk;
 * *volume_tile = volumes per tile of the first launch.  Any pointer may be null */
fw_status fw_debug_volume_query(fw_ctx *ctx, uint64_t *launches, uint64_t *chunks, uint32_t *chunk_size, uint32_t *volume_tile);

#ifdef __cplusplus
}
#endif
#endif /* FIREWORK_HIP_DEBUG_H */
