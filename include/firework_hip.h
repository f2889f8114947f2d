/*
 * firework_hip.h -- C ABI of libfirework_hip.so, the MI355X (gfx950) backend for
 * bevy_firework's per-frame particle simulation path.
 *
 * The reference has no FFI: the path sits behind Bevy's system registration
 *   (sync_spawner_data, spawn_particles, update_particles,
 *    notify_finished_particle_spawners).chain()        reference src/plugin.rs:46-60
 * operating on the components ParticleSpawner (src/core.rs:178-185, user-owned
 * settings) and ParticleSpawnerData (src/core.rs:269-303, plugin-owned state).
 * This header is what a Rust shim crate would bind (INTEGRATION.md shows the
 * `extern "C"` block and the exclusive system that replaces the two CPU systems).
 * Each entry point cites the reference item it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; all input descriptors are copied at the call.
 *  - every function returns fw_status (0 = ok, negative = error) unless noted;
 *    fw_last_error() gives a message.  The library never aborts the process; the
 *    reference's panics (zero-key curve curve.rs:45,61,211,227; out-of-range
 *    particle_index / target_particle_type core.rs:392,453,488) become FW_EINVAL
 *    at create time.
 *  - calls on ONE context must be serialised by the caller (the reference chain is sequential too).  Contexts share no
 *    state: different contexts -- on one GPU or on several -- may be driven from different threads at the same time.
 *    One context per GPU is the normal arrangement; a host with thousands of small emitters, whose frame is bound by the
 *    host half of fw_step (~30 ns per emitter on one thread), spreads them over a few contexts on the same GPU, one per
 *    worker thread -- the counterpart of the reference's par_iter_mut over spawners (core.rs:583-585); the device runs
 *    their launches side by side (examples/many_contexts.cpp).  fw_last_error(NULL) is per calling thread.
 *  - fw_step only ENQUEUES work on the
 *    context's HIP stream; readers synchronise that stream.  A context created on a CALLER-SUPPLIED stream keeps the
 *    whole frame on that stream: work the caller orders behind fw_step on it (or hipStreamSynchronize of it) covers
 *    the frame.  A context that owns its stream (stream = NULL at fw_ctx_create) may run part of a frame on a second,
 *    internal stream (the in-place update of ring segments next to the compacting launch): everything the library
 *    enqueues on the context's stream that looks at particle data -- attached instance buffers, the *_device entry
 *    points -- is ordered after it by the library itself, and fw_ctx_synchronize waits for both; wait for a frame of
 *    such a context with fw_ctx_synchronize, not hipStreamSynchronize(fw_ctx_stream(ctx)).
 *  - there is NO CPU fallback: without a usable HIP device fw_ctx_create fails
 *    with FW_ENODEV.
 */
#ifndef FIREWORK_HIP_H
#define FIREWORK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_ABI_VERSION 5
/* (no FW_MAX_TYPES / FW_MAX_EMISSIONS / FW_MAX_KEYS / FW_MAX_COLLIDERS: the reference's Vec<ParticleSettings>,
 * Vec<EmissionSettings> (core.rs:178-185), curve sample vectors (curve.rs:40-75) and collider world are unbounded, and so
 * are the descriptors below -- FW_EINVAL is for input the reference itself rejects.  Curves and gradients of up to
 * FW_FAST_KEYS samples are staged in LDS; longer ones are read from device memory by the feature kernels.) */
#define FW_FAST_KEYS 32

typedef enum fw_status {
    FW_OK = 0,
    FW_EINVAL = -1,    /* bad argument / descriptor (mirrors the reference's panics) */
    FW_ENOMEM = -2,    /* host or device allocation failed */
    FW_EHIP = -3,      /* a HIP call failed, or an internal consistency check of an update kernel did (fw_last_error) */
    FW_ECAPACITY = -4, /* a particle type overflowed its device capacity (nested emission) */
    FW_ENODEV = -5,    /* no usable HIP device / kernels not loadable */
    FW_ESMALL = -6     /* output buffer too small; required size reported */
} fw_status;

/* Internal errors are STICKY PER SPAWNER.  The update kernels check the host's bookkeeping against the particles they load
 * (which particles a step destroys, live counts, look-back waits).  A failed check means the library's own state is wrong;
 * where the type is updated in place (ring paths) the frame has overwritten its input and cannot be redone.  The library
 * then does not guess: the spawner the particle type belongs to is marked invalid, fw_step returns FW_EHIP without
 * enqueuing anything (for any spawner: the frame is all-or-nothing) and so does every call that reads or writes that
 * spawner's particles, until fw_spawner_update_settings rebuilds it -- sync_spawner_data (core.rs:343-365): emission state
 * reset, all particles dropped; the rebuilt spawner stays off the in-place paths -- or fw_spawner_destroy removes it.  Other
 * spawners keep their state. */
typedef struct fw_ctx fw_ctx;
typedef int32_t fw_spawner; /* handle, >= 0 */

/* bevy_utilitarian RandF32 / RandVec3 as used by core.rs:102,107,155,157,161 */
typedef struct fw_rand_f32 { float min, max; } fw_rand_f32;
typedef struct fw_rand_vec3 { fw_rand_f32 magnitude; float direction[3]; float spread; } fw_rand_vec3;

/* FireworkCurve<f32> (curve.rs:8-12) and FireworkGradient<LinearRgba> (curve.rs:171-175) */
enum { FW_CURVE_CONSTANT = 0, FW_CURVE_EVEN = 1, FW_CURVE_UNEVEN = 2 };
typedef struct fw_curve { int32_t kind; int32_t n; const float *times; const float *values; } fw_curve;
typedef struct fw_gradient { int32_t kind; int32_t n; const float *times; const float *rgba; } fw_gradient;

/* ParticleCollisionSettings (core.rs:240-248, feature physics_avian): `enabled` = the Option is Some.
 * `filter_mask` stands in for SpatialQueryFilter (core.rs:247, passed to cast_ray at core.rs:764): a collider takes part when
 * (filter_mask & collider.layers) != 0 -- avian's `mask` against the collider's `memberships`.
 * NOT SUPPORTED: `SpatialQueryFilter::excluded_entities`.  The device-resident set has no entity identity (the ray-cast query
 * names what it hit by its position in the set: fw_ray_hit.index, below): a host that needs
 * an exclusion keeps the excluded colliders out of the set it sends (fw_ctx_set_colliders; the set is per context, so this
 * excludes them for every particle type of the context) or gives them a membership bit no particle type's mask contains
 * (rust/src/hip/colliders.rs does the latter for entities listed in a `ParticleColliderExclusions` resource). */
typedef struct fw_collision_settings {
    int32_t enabled;
    float restitution, friction;
    int32_t destroy_on_collision;
    uint32_t filter_mask;
} fw_collision_settings;

/* ParticleSettings (core.rs:99-142), simulation-relevant fields only; textures,
 * fade_*, blend_mode stay on the host (they never enter update_particles). */
typedef struct fw_particle_settings {
    fw_rand_f32 lifetime;
    fw_curve scale_curve;
    fw_rand_f32 initial_scale;
    float acceleration[3];
    float angular_acceleration[3];
    float linear_drag, angular_drag;
    fw_gradient base_color, emissive_color;
    int32_t pbr;
    int32_t report_destroyed; /* event_handlers.particles_destroyed.is_some() (core.rs:164-167) */
    uint32_t capacity;        /* device slots for this type; 0 = derive from the emitters */
    fw_collision_settings collision; /* collision_settings: Option<ParticleCollisionSettings> (core.rs:137-138) */
} fw_particle_settings;

/* The world particle_collision (core.rs:744-800) casts its rays into.  The reference asks avian's SpatialQuery
 * (arbitrary colliders, CPU broadphase); this backend keeps a DEVICE-RESIDENT set of analytic colliders instead and
 * casts against them inside the update.  Ray-cast semantics (ours, modelled on parry's `solid = true` casts):
 *   PLANE   the half-space n.(x - position) <= 0 is solid; `normal` must be a unit vector
 *   SPHERE  |x - position| <= radius is solid
 *   BOX     |R^-1 (x - position)|_i <= half_extents_i is solid (R = rotation, xyzw)
 *   CYLINDER  avian's Collider::cylinder(radius, height) (examples/textures.rs:195): in the collider's frame (R, position) the
 *           axis is Y; |y| <= half_extents[1] (= height / 2) and x^2 + z^2 <= radius^2 is solid; a hit on a cap reports +-Y, a hit
 *           on the lateral surface the radial direction (both rotated by R)
 *   CONE    avian's Collider::cone(radius, height) (examples/textures.rs:211): base disc of `radius` at y = -half_extents[1], apex
 *           at y = +half_extents[1]; solid between them; the base reports -Y, the lateral surface its outward normal
 *   CAPSULE avian's Collider::capsule(radius, length) (parry's Capsule): in the collider's frame (R, position) the axis is Y; every
 *           point within `radius` of the segment from (0, -hl, 0) to (0, +hl, 0) is solid.  hl = half_extents[1] is half the length of
 *           the SEGMENT (parry's half_height), NOT half the total height; hl == 0 is a ball.  The cast, all fp32 with no fused a*b+c
 *           (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z), with o = R^-1 (origin - position), d = R^-1 dir (the identity rotation skips
 *           both products, as for the other framed kinds) and rr = radius * radius:
 *     INSIDE  yc = min(max(o.y, -hl), hl), evaluated as o.y < -hl ? -hl : (o.y > hl ? hl : o.y); dy = o.y - yc;
 *             xz = (o.x * o.x) + (o.z * o.z); the origin is inside or on the solid when ((xz + (dy * dy)) - rr) <= 0: distance 0, zero
 *             normal, like every solid.
 *     ENTRY   otherwise the solid is convex and its boundary three pieces; the hit is the smallest valid t over them, taken in the
 *             order lateral surface, bottom cap (cy = -hl), top cap (cy = +hl): a later piece replaces an earlier one only when its t
 *             is strictly smaller (<), so the earlier piece wins a tie.  Near roots suffice: each cap's whole ball lies inside the
 *             solid, so a ray from outside meets a cap's sphere first at its near root, and the far root of the lateral surface is an
 *             exit.
 *       lateral  the cylinder's quadratic: a = (d.x * d.x) + (d.z * d.z); b = (o.x * d.x) + (o.z * d.z); c2 = xz - rr; no root when
 *                a == 0 or disc = (b * b) - (a * c2) is not >= 0; t = (-b - sqrt(disc)) / a; valid when t >= 0 and
 *                |o.y + (d.y * t)| <= hl.
 *       cap      the sphere's quadratic about the cap's centre (0, cy, 0), operation by operation: w = (o.x, o.y - cy, o.z);
 *                A = dot(d, d); B = dot(w, d); C = dot(w, w) - rr; no root when B > 0 ("outside and moving away") or
 *                delta = (B * B) - (A * C) is not >= 0; t = (-B - sqrt(delta)) / A; valid when t >= 0 and the hit point lies on the
 *                outer hemisphere: y = o.y + (d.y * t) with y <= -hl for the bottom cap, y >= hl for the top cap.  (The sphere's own
 *                "inside" test is not repeated: INSIDE above has answered it for the whole solid.)
 *       a hit needs t <= max_distance.
 *     NORMAL  p = (o.x + (d.x * t), o.y + (d.y * t), o.z + (d.z * t)); v = (p.x, 0, p.z) on the lateral surface, (p.x, p.y - cy, p.z) on
 *             a cap; n = v * (1 / sqrt(dot(v, v))), rotated by R (not at all under the identity rotation).
 *     REACH   the sphere around `position` a wave may skip the collider by (fw_ctx_set_colliders computes it) has the radius
 *             (hl + radius) * 1.0001f; NaN or negative gives INFINITY (never skipped), as for every kind.
 *   a ray that starts inside a solid hits it at distance 0 with a ZERO normal (core.rs:762-771 handles that case);
 *   otherwise the hit is the entry point, its normal the outward surface normal; the nearest hit over all colliders
 *   that pass the filter wins (lowest index on ties). */
enum { FW_COLLIDER_PLANE = 0, FW_COLLIDER_SPHERE = 1, FW_COLLIDER_BOX = 2, FW_COLLIDER_CYLINDER = 3, FW_COLLIDER_CONE = 4, FW_COLLIDER_CAPSULE = 5 };
typedef struct fw_collider {
    int32_t kind;
    uint32_t layers;        /* collision layers (membership bits) */
    float position[3];
    float rotation[4];      /* xyzw; BOX, CYLINDER, CONE, CAPSULE */
    float normal[3];        /* PLANE only */
    float radius;           /* SPHERE, CYLINDER, CONE, CAPSULE */
    float half_extents[3];  /* BOX; [1] = half the height of a CYLINDER / CONE, half the SEGMENT of a CAPSULE */
} fw_collider;

/* Triangle meshes (avian's Collider::trimesh / heightfield / convex hulls, as triangles): a mesh is uploaded once and placed
 * any number of times by instances.  Ray-cast semantics (ours, like those of the analytic kinds; all fp32, no fused a*b+c):
 *   SURFACE   a mesh is a two-sided surface with no interior: no distance-0 "inside" hit, no push-out.
 *   FRAME     the ray is taken into the instance's frame once: o = R^-1 (origin - position), d = R^-1 dir (R = rotation, xyzw;
 *             the identity rotation skips both products).  The mesh is not scaled, so the distance t needs no conversion.
 *   TRIANGLE  v0 as given, e1 = v1 - v0, e2 = v2 - v0 (fp32, at creation); Moeller-Trumbore in this order:
 *               p = cross(d, e2); det = dot(e1, p); det == 0 is a miss; inv = 1 / det; s = o - v0; u = dot(s, p) * inv;
 *               q = cross(s, e1); v = dot(d, q) * inv; t = dot(e2, q) * inv
 *             (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross(a, b) = (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y));
 *             a hit needs u >= -m, v >= -m, u + v <= 1 + m and 0 <= t <= max_distance, with the margin m of WATERTIGHT.
 *   WATERTIGHT  two triangles that share an edge evaluate it with different operands (their own v0, e1, e2), so with m = 0 a
 *             ray near the edge can be rejected by both and pass through a closed surface.  The margin is the rounding of u and
 *             v stated in their own operands:
 *               m = min(((2^-21 * |s|_1) * (|e1|_1 + |e2|_1)) * |inv|, 2^-8),   |a|_1 = (|a.x| + |a.y|) + |a.z|
 *             (2^-21 = 8 * 2^-24: fifteen times the largest margin any ray that used to leak needed; fmin, so a NaN product gives
 *             the cap).  What it buys, against a float64 cast over every triangle: a ray whose line passes inside the mesh's
 *             silhouette by 0.05 of the mesh's largest |coordinate| and crosses the surface within max_distance reports a hit no
 *             later than t_ref + 2^-14 (t_ref + that coordinate) -- NO LEAK.  What it costs: a ray may hit a triangle it passes up
 *             to m of its edges outside of; a hit met at |cos| >= 0.5 still lies within 2^-13 (|o - v0| + |e1| + |e2|) of its
 *             triangle, and a ray farther than that from every triangle hits nothing -- NO INVENTION.  Every ray the rule with
 *             m = 0 hits is still hit, no later, and the same triangle gives the same distance and normal bit for bit.
 *             DOMAIN: the brute force over every triangle (the C oracle's) is held to NO LEAK for origins up to 1024 times the
 *             mesh's largest |coordinate| away.  The device walks a hierarchy of boxes and tests each box grown by 2^-6 of its
 *             own extent, which holds every ray the margin accepts while its rounding stays below the cap: the walk is held to
 *             NO LEAK, and to the brute force's result bit for bit, wherever |s|_1 (|e1|_1 + |e2|_1) <= 2^13 |det| for the
 *             triangle crossed (the margin is then below its cap) -- a well-shaped triangle of edge e met at angle cos from
 *             a distance of up to about 2^11 e cos.  (tests/test_mesh_watertight_cpu.py, tests/test_gpu_mesh_watertight.py)
 *   NORMAL   c = cross(e1, e2); n = c * (1 / sqrt(dot(c, c))), rotated by R, and negated when dot(n, dir) > 0.
 *   TIES      the nearest hit wins; at equal distance analytic colliders come before mesh instances, lower instance indices
 *             before higher ones, and within an instance the lower ORIGINAL triangle index (position in `indices`) wins.
 *   FILTER    an instance takes part when (filter_mask & layers) != 0, as a collider does.
 * Triangles whose c has dot(c, c) == 0 (or not finite) -- zero area -- are dropped at creation; no other triangle is.
 *
 * DEFORMABLE MESHES.  A mesh made by fw_ctx_create_deformable_mesh takes new vertex positions through
 * fw_ctx_update_mesh_vertices: same topology, same hierarchy shape, its boxes and triangles recomputed on the device.
 *   AS IF CREATED ANEW   after an update with xyz', every ray cast of every later fw_step gives, bit for bit -- hit or miss,
 *             distance, normal, ties -- what a mesh from fw_ctx_create_mesh(xyz', indices) would give in the same places.  The
 *             zero-area rule is evaluated again per update with the same fp32 operations: a triangle that collapses stops
 *             being hit, one that was degenerate (at creation too) and opens up starts being hit, and original triangle
 *             indices never change.
 *   ORDER     the call does not synchronise: the vertices are copied to pinned staging (double-buffered; the call waits only for
 *             the copy before the previous one), travel as one copy in the context's stream, and the refit runs behind it in
 *             the same stream -- frames enqueued before the call see the old shape, frames after it the new one.  Instances
 *             of the current set that place the mesh follow (their bounding spheres are restaged in the same order).
 *   ERRORS    all-or-nothing: FW_EINVAL and nothing changes for an unknown handle, a mesh not created as deformable, an
 *             n_vertices other than the creation's, a non-finite vertex.  Vertices that leave NO triangle of non-zero area are
 *             accepted: the mesh is hit by nothing until the next update (creation still rejects such a mesh).
 *   QUALITY   a refit keeps the tree the creation vertices gave: after large deformations boxes overlap more and casts get
 *             slower, never wrong.  A caller whose mesh has changed beyond recognition creates a new one.
 *   FROM DEVICE MEMORY   fw_ctx_update_mesh_vertices_device is the same update for vertices a GPU pass has just produced
 *             (skinning, cloth, a terrain that is dug into).  AS IF CREATED ANEW holds unchanged, and the result equals what
 *             fw_ctx_update_mesh_vertices gives for the same values, bit for bit.  The call never waits for the device and does
 *             no host work that grows with the vertex count; everything it enqueues goes to the context's stream
 *             (fw_ctx_stream).  The caller writes d_xyz on that stream, or orders its producer in front of the call itself.  The
 *             buffer is read ONLY by work enqueued inside the call -- no copy is made, the refit gathers straight from it -- so
 *             work the caller orders behind the call on that stream may overwrite it.  Frames enqueued before the call see the
 *             old shape, frames after it the new one.  A mesh's first such call allocates what the device side needs (a
 *             failure: FW_EHIP, everything released, the mesh usable by both forms) and uploads a byte per vertex, which may
 *             wait for that copy; later calls allocate nothing.
 *             Host-side errors are those of the host form, at once and with nothing changed (null pointer, unknown handle,
 *             not deformable, another vertex count).  A NON-FINITE vertex is something only the device can see: the update is
 *             then REJECTED ON THE DEVICE -- hierarchy, triangles and the bounding spheres of placed instances stay exactly
 *             what they were, frames go on casting against the previous shape, fw_step does not fail, and the next good
 *             update of either form applies normally.  fw_ctx_mesh_update_status reports, without waiting, how many device-form
 *             updates of the mesh the device has applied and rejected so far and the lowest non-finite vertex index of the
 *             latest rejected one (-1: none yet); the words are written by the device into pinned memory, so they lag the
 *             calls until fw_ctx_synchronize, after which they are exact.  The two forms may alternate freely on one mesh.
 * fw_ctx_destroy_mesh and fw_ctx_set_mesh_colliders treat a deformable mesh like any other. */
typedef int32_t fw_mesh; /* handle >= 0, per context */
typedef struct fw_mesh_collider { /* one placed instance of a mesh */
    fw_mesh mesh;
    uint32_t layers;   /* membership bits, as fw_collider.layers */
    float position[3];
    float rotation[4]; /* xyzw, a unit quaternion; scale is baked into the mesh's vertices */
} fw_mesh_collider;

/* RAY-CAST QUERIES (avian's SpatialQuery::cast_ray for everybody else: decals, impact sounds, "where will this spark land").  The
 * collider world lives on the device; fw_ctx_cast_rays[_device] casts a batch of rays into it, one nearest hit per ray.
 *   SAME CAST the cast is the one particle_collision runs (the same device function): hit or miss, `distance` and `normal` are, bit
 *             for bit, what a particle gets for the same origin, dir, max_distance and mask, in the world as of the call's place in
 *             the context's stream, with the same tie rule -- the nearest hit wins; at equal distance analytic colliders come
 *             before mesh instances, then the lower index, then the lower ORIGINAL triangle.  `dir` is used as given: the update
 *             passes a unit vector, the query does not normalise (`distance` is in units of |dir|).  A ray that starts inside a
 *             solid reports distance 0 with a zero normal and names that solid (the lowest index on ties there too).
 *   MISS      kind = FW_HIT_NONE, distance = 0, normal = 0, index = triangle = 0xFFFFFFFF.
 *   IDENTITY  `kind` says which set `index` counts in: the one last given to fw_ctx_set_colliders (FW_HIT_COLLIDER) or to
 *             fw_ctx_set_mesh_colliders (FW_HIT_MESH) before the query; `triangle` is the position in `indices` at the mesh's
 *             creation, whatever was dropped or reordered since.  The host built both sets, so it keeps the parallel vector
 *             of entities.
 *   ORDER     both forms enqueue on the context's main stream (fw_ctx_stream), where collider sets, instance sets, refits and every
 *             launch that casts rays already travel: a query sees every fw_ctx_set_colliders, fw_ctx_set_mesh_colliders and
 *             fw_ctx_update_mesh_vertices[_device] called before it and none called after it.  The device form never waits,
 *             allocates nothing, does no host work that grows with n, and reads d_rays / writes d_hits ONLY in work it enqueues
 *             itself (as fw_ctx_update_mesh_vertices_device does): the caller writes d_rays on that stream or orders its producer
 *             in front of the call, and reads d_hits behind it.  The host form stages through pinned memory (grown on demand,
 *             kept by the context) and waits for its result.
 *   ERRORS    a null pointer with n > 0: FW_EINVAL, nothing enqueued.  n == 0: FW_OK, nothing touched.  An empty world: every ray
 *             misses.  NaN or infinite rays give whatever the operations give, deterministically; the walk ends for any ray. */
typedef struct fw_ray { /* 32 bytes */
    float origin[3];
    float max_distance;
    float dir[3];
    uint32_t filter_mask; /* as fw_collision_settings.filter_mask */
} fw_ray;
enum { FW_HIT_NONE = 0, FW_HIT_COLLIDER = 1, FW_HIT_MESH = 2 };
typedef struct fw_ray_hit { /* 32 bytes */
    float distance;
    float normal[3];
    int32_t kind;      /* FW_HIT_* */
    uint32_t index;    /* position in the set given to fw_ctx_set_colliders / fw_ctx_set_mesh_colliders */
    uint32_t triangle; /* FW_HIT_MESH: ORIGINAL triangle index (position in `indices` at creation); else 0xFFFFFFFF */
    uint32_t reserved; /* 0 */
} fw_ray_hit;

/* POINT QUERIES (avian's SpatialQuery::project_point and point_intersections: an emitter snapped to the nearest surface, a decal
 * placed from an explosion's centre, "is this spawn position buried?").  fw_ctx_project_points[_device] projects a batch of points
 * onto the collider world: per point the nearest point of the world, its distance, who owns it, and whether the point lies inside
 * a solid.  All fp32, no fused a*b+c; dot and cross as under TRIANGLE above; clamp(x, h) = x < -h ? -h : (x > h ? h : x).
 *   FILTER    a collider or instance takes part when (filter_mask & layers) != 0.
 *   SOLID     analytic kinds are solids (parry's `solid = true`).  "inside or on" is, kind by kind, the expression the ray cast
 *             tests for its distance-0 case, so is_inside agrees bit for bit with "a ray from this point reports distance 0 with a
 *             zero normal" for that collider.  With c = the collider, x = position, o as under FRAME below:
 *               PLANE     dot(n, c.position - x) > 0
 *               SPHERE    dot(v, v) - radius * radius <= 0, v = x - c.position
 *               BOX       |o.x| <= hx and |o.y| <= hy and |o.z| <= hz
 *               CYLINDER  |o.y| <= hh and (o.x o.x + o.z o.z) - radius * radius <= 0
 *               CONE      o.y >= -hh and wy <= 0 and (o.x o.x + o.z o.z) - k2 * (wy * wy) <= 0, wy = o.y - hh, k = radius / (hh + hh), k2 = k * k
 *               CAPSULE   ((o.x o.x + o.z o.z) + dy * dy) - radius * radius <= 0, yc = clamp(o.y, hl), dy = o.y - yc
 *             The participating collider of the LOWEST index that contains the point answers, whatever else is near: point =
 *             position (the caller's bits), distance = 0, is_inside = 1, kind = FW_HIT_COLLIDER, index = that collider.
 *   FRAME     PLANE and SPHERE work in the world (o = x).  BOX, CYLINDER, CONE and CAPSULE work in the collider's frame:
 *             o = R^-1 (x - c.position), the identity rotation skipping the product, as in the cast.
 *   NEAREST   for a point outside the solid, q = the nearest point of the solid:
 *               PLANE     s = dot(n, x - c.position); q = x - n * s
 *               SPHERE    q = c.position + v * (radius / sqrt(dot(v, v)))
 *               BOX       q = (clamp(o.x, hx), clamp(o.y, hy), clamp(o.z, hz))
 *               CYLINDER  r = sqrt(o.x o.x + o.z o.z); profile point qr = r > radius ? radius : r, qy = clamp(o.y, hh)
 *               CONE      r as above; first the base segment: qr = r > radius ? radius : r, qy = -hh, db = (r - qr)^2 + (o.y - qy)^2;
 *                         then the slant segment from the rim (radius, -hh) to the apex (0, +hh): h = hh + hh,
 *                         t = ((o.y + hh) * h - (r - radius) * radius) / (radius * radius + h * h), clamped to [0, 1] (t < 0 ? 0 : (t > 1 ? 1 : t)),
 *                         sr = radius - radius * t, sy = h * t - hh, ds = (r - sr)^2 + (o.y - sy)^2; (qr, qy) = (sr, sy) only when ds < db
 *               CYLINDER and CONE take the profile point back as q = (qr * o.x / r, qy, qr * o.z / r), or (qr, qy, 0) when r == 0
 *               CAPSULE   v = (o.x, dy, o.z); s = radius / sqrt(dot(v, v)); q = (v.x * s, yc + v.y * s, v.z * s)
 *             then w = o - q and d2 = dot(w, w): candidates compete on this squared distance.
 *   MESHES    surfaces, as for rays: never inside.  The point is taken into the instance's frame once (o as under FRAME of the mesh
 *             block).  A triangle takes part only when c = cross(e1, e2) of its STORED edges has dot(c, c) > 0 and finite -- the
 *             zero-area rule of creation; a deformable mesh keeps its collapsed triangles as records with zero edges, and those do not
 *             answer.  Per triangle the closest point by regions (Ericson, Real-Time Collision Detection, 5.1.5) from v0, e1, e2:
 *               ap = o - v0; d1 = dot(e1, ap); d2 = dot(e2, ap); bp = ap - e1; d3 = dot(e1, bp); d4 = dot(e2, bp);
 *               cp = ap - e2; d5 = dot(e1, cp); d6 = dot(e2, cp); vc = d1 d4 - d3 d2; vb = d5 d2 - d1 d6; va = d3 d6 - d5 d4;
 *             the FIRST of these tests that holds gives the barycentric pair (v, w):
 *               d1 <= 0 and d2 <= 0: (0, 0);   d3 >= 0 and d4 <= d3: (1, 0);   vc <= 0 and d1 >= 0 and d3 <= 0: (d1 / (d1 - d3), 0);
 *               d6 >= 0 and d5 <= d6: (0, 1);   vb <= 0 and d2 >= 0 and d6 <= 0: (0, d2 / (d2 - d6));
 *               va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w;
 *               otherwise (the face): denom = 1 / ((va + vb) + vc); v = vb * denom; w = vc * denom;
 *             q = (v0 + e1 * v) + e2 * w per component, w' = o - q, d2 = dot(w', w').
 *   TIES      the smaller d2 wins; the best starts at +infinity and is replaced by strict <, so a candidate whose d2 is NaN or
 *             infinite never wins.  The analytic colliders compete in index order, then the instances in index order: at bit-equal
 *             d2 analytic colliders come before mesh instances and lower indices before higher ones.  Within an instance the lower
 *             ORIGINAL triangle index wins a bit-equal d2 (neighbouring triangles do tie, on shared edges and vertices).
 *   RESULT    only the winner's q goes back to the world (R q + position, the identity rotation skipping the product; PLANE and
 *             SPHERE are there already), and only the winner takes the root: distance = sqrt(d2).  kind / index / triangle name the
 *             winner as in fw_ray_hit.  Nobody took part, or nobody won: kind = FW_HIT_NONE, point = 0, distance = 0,
 *             index = triangle = 0xFFFFFFFF, is_inside = 0.
 *   ORDER     both forms enqueue on the context's main stream (fw_ctx_stream), where collider sets, instance sets, refits and every
 *             launch that casts rays already travel: a query sees every fw_ctx_set_colliders, fw_ctx_set_mesh_colliders and
 *             fw_ctx_update_mesh_vertices[_device] called before it and none called after it.  The device form never waits,
 *             allocates nothing, does no host work that grows with n, and reads d_points / writes d_out ONLY in work it enqueues
 *             itself.  The host form stages through pinned memory (grown on demand, kept by the context) and waits for its result.
 *   ERRORS    a null pointer with n > 0: FW_EINVAL, nothing enqueued.  n == 0: FW_OK, nothing touched.  NaN or infinite points give
 *             whatever the operations give, deterministically; the walk of a mesh ends for any point. */
typedef struct fw_point { /* 16 bytes */
    float position[3];
    uint32_t filter_mask; /* as fw_ray.filter_mask */
} fw_point;
typedef struct fw_point_projection { /* 32 bytes */
    float point[3];     /* nearest point of the world to `position` (position itself when is_inside) */
    float distance;     /* sqrt of the winning squared distance; 0 when is_inside */
    int32_t kind;       /* FW_HIT_NONE / FW_HIT_COLLIDER / FW_HIT_MESH */
    uint32_t index;     /* as fw_ray_hit.index */
    uint32_t triangle;  /* as fw_ray_hit.triangle */
    uint32_t is_inside; /* 1: position lies inside or on the analytic solid named; meshes never */
} fw_point_projection;

/* PATH QUERIES ("where will this spark land": an aim arc for a mortar shell, a decal or a light placed before the spark arrives, the
 * emitter direction that clears a wall).  A ray cannot answer that: a particle falls, slows under drag, bounces with restitution and
 * friction and lives for a limited time.  fw_ctx_trace_paths[_device] runs a batch of HYPOTHETICAL particles through n_steps frames of
 * dt each, off the frame's path -- nothing is spawned, no spawner's state is read or written -- with the arithmetic a real particle
 * gets.  All fp32, no fused a*b+c.  One fw_path_settings per call, shared by the batch.
 *   SAME STEP one step is update_particles (core.rs:594-643) restricted to age, position and velocity, in this order:
 *               1. age = age + dt;
 *               2. age >= lifetime: the path ends FW_PATH_EXPIRED; position and velocity stay as they were, age is the advanced one
 *                  (what a destroyed record carries);
 *               3. otherwise particle_collision(position, velocity, dt) (core.rs:744-800: up to four sub-steps, each a cast along the
 *                  velocity of length |velocity| * remaining time into the world under collision.filter_mask, the push-out of an
 *                  inside hit, the bounce with restitution and friction) when collision.enabled, else position = position +
 *                  velocity * dt per component;
 *               4. the collision said destroy (destroy_on_collision and a hit): the path ends FW_PATH_DESTROYED with the
 *                  position and velocity the collision left;
 *               5. otherwise velocity = velocity + (acceleration - velocity * linear_drag) * dt per component, and the step is
 *                  survived (`steps` counts these).
 *             The promise: take a particle of a type with these settings (acceleration, linear_drag, collision), written with
 *             fw_spawner_write_particles at the path's position, velocity, age and lifetime.  After k calls of fw_step(dt) in the same
 *             world its position, velocity and age hold, bit for bit, what the path holds after k steps; it is removed in the step in
 *             which the path ends, and its destroyed record holds the result's position, velocity and age.
 *   CONTACTS  every hit a sub-step's cast returns is a contact, the distance-0 "inside" hit included; n_contacts counts them over the
 *             path.  The FIRST fills contact_*: contact_step is the step it happened in, counted from 0; contact_normal is the cast's
 *             normal as reported (zero for an inside hit, before core.rs:767-774 replaces it); contact_point is, for distance > 0, the
 *             position after position += normalize_or_zero(velocity) * distance and before the + normal * 0.0001 nudge, for distance
 *             == 0 the position before the push-out; kind / index / triangle name what was hit as in fw_ray_hit.  No contact:
 *             contact_point = contact_normal = 0, kind = FW_HIT_NONE, index = triangle = contact_step = 0xFFFFFFFF, n_contacts = 0.
 *   RESULT    position, velocity and age after the last step taken; steps = the steps survived; status = FW_PATH_RUNNING when all
 *             n_steps were.  n_steps == 0 gives the inputs back: RUNNING, steps 0, no contact.
 *   SAMPLES   optional (NULL: none, and nothing is reserved, written or copied for them): n_steps * n records of four floats,
 *             samples[(step * n + i) * 4 ..] = {position, age} of path i after that step.  Steps after a path has ended repeat its
 *             final values (those of the result).
 *   FROZEN WORLD  the whole path runs in the world as of the call's place in the context's stream; colliders a host moves between
 *             frames are not predicted.
 *   ORDER     both forms enqueue on the context's main stream (fw_ctx_stream), where collider sets, instance sets, refits and every
 *             launch that casts rays already travel: a query sees every fw_ctx_set_colliders, fw_ctx_set_mesh_colliders and
 *             fw_ctx_update_mesh_vertices[_device] called before it and none called after it.  The device form never waits,
 *             allocates nothing, does no host work that grows with n or n_steps, and reads d_paths / writes d_out and d_samples ONLY
 *             in work it enqueues itself; the settings are read on the host inside the call and travel as kernel arguments.  The
 *             host form stages through pinned memory (grown on demand, kept by the context) and waits for its result.
 *   ERRORS    checked in this order, FW_EINVAL with nothing enqueued: a null settings pointer; a non-finite dt; n_steps >
 *             FW_PATH_MAX_STEPS (the cap bounds one launch's running time).  Then n == 0: FW_OK, nothing touched.  Then a null
 *             paths or out pointer: FW_EINVAL, nothing enqueued.  NaN or infinite paths give whatever the operations give,
 *             deterministically, and every path ends after at most n_steps steps. */
enum { FW_PATH_RUNNING = 0, FW_PATH_EXPIRED = 1, FW_PATH_DESTROYED = 2 };
#define FW_PATH_MAX_STEPS 4096u
typedef struct fw_path_settings { /* one per call, shared by the batch */
    float dt;
    uint32_t n_steps;
    float acceleration[3];
    float linear_drag;
    fw_collision_settings collision; /* enabled = 0: no casts, position += velocity * dt */
} fw_path_settings;
typedef struct fw_path { /* 32 bytes */
    float position[3];
    float age;
    float velocity[3];
    float lifetime;
} fw_path;
typedef struct fw_path_result { /* 80 bytes */
    float position[3];
    float age;
    float velocity[3];
    uint32_t steps;          /* steps survived */
    float contact_point[3];
    uint32_t contact_step;   /* 0xFFFFFFFF: the path met nothing */
    float contact_normal[3];
    uint32_t status;         /* FW_PATH_* */
    int32_t kind;            /* FW_HIT_* of the first contact */
    uint32_t index;          /* as fw_ray_hit.index */
    uint32_t triangle;       /* as fw_ray_hit.triangle */
    uint32_t n_contacts;
} fw_path_result;

enum { FW_PACING_ONESHOT = 0, FW_PACING_ONDEMAND = 1, FW_PACING_COUNT_OVER_DURATION = 2 }; /* core.rs:12-29 */
enum { FW_MODE_GLOBAL = 0, FW_MODE_NESTED = 1 };                                           /* core.rs:47-54 */
enum { FW_SHAPE_POINT = 0, FW_SHAPE_SPHERE = 1, FW_SHAPE_CIRCLE = 2 };                     /* emission_shape.rs:7-15 */

/* EmissionSettings (core.rs:144-162) */
typedef struct fw_emission_settings {
    int32_t particle_index;
    int32_t pacing_kind;
    uint64_t oneshot_count;
    float count, duration, offset_start, offset_end;
    int32_t mode;
    int32_t target_particle_type;
    int32_t shape_kind;
    float shape_radius;
    float shape_normal[3];
    fw_rand_vec3 initial_velocity;
    fw_rand_f32 initial_velocity_radial;
    int32_t inherit_parent_velocity;
    float initial_rotation[4]; /* xyzw */
    fw_rand_vec3 initial_angular_velocity;
} fw_emission_settings;

/* ParticleSpawner (core.rs:178-185).  spawn_transform_mode is resolved by the host:
 * it passes the chosen transform to fw_spawner_set_origin (core.rs:432-435). */
typedef struct fw_spawner_desc {
    const fw_particle_settings *particle_settings;
    uint32_t n_particle_settings;
    const fw_emission_settings *emission_settings;
    uint32_t n_emission_settings;
    int32_t starts_enabled;
    uint32_t uid; /* RNG stream id; keep it stable across GPUs when sharding */
} fw_spawner_desc;

/* ParticleData (core.rs:305-321) as an AoS record for readback / upload.
 * last_emitted_age is read separately (fw_spawner_read_last_emitted). */
typedef struct fw_particle {
    float position[3];
    float velocity[3];
    float rotation[4];
    float angular_velocity[3];
    float initial_scale, scale, age, lifetime;
    float base_color[4];
    float emissive_color[4];
    int32_t pbr;
} fw_particle;

/* ParticleInstance (render.rs:95-103): 64 B */
typedef struct fw_particle_instance {
    float position[3];
    float scale;
    float rotation[4];
    float base_color[4];
    float emissive_color[4];
} fw_particle_instance;

/* DEPTH-SORTED INSTANCES (an alpha-blended draw with depth writes off -- the reference's default BlendMode, render.rs:775-779 -- shows
 * its particles in the order of the buffer: every other hand-off delivers list order, that is spawn order, and the picture changes
 * with the camera angle).  fw_ctx_pack_instances_sorted[_device] deliver the ParticleInstance records of one particle type sorted by
 * view depth, fw_ctx_depth_order_device the permutation alone, for a host that already has the records.
 *   DEPTH     d = ((p.x - eye.x) * forward.x + (p.y - eye.y) * forward.y) + (p.z - eye.z) * forward.z in fp32: three subtractions, three
 *             products, the sum of the x and y products, then that sum plus the z product; every operation rounded, none fused.  p is
 *             the position the unsorted pack writes into the particle's record.  `forward` is used as given, not normalised (as
 *             fw_ray.dir is): a zero vector gives every particle depth 0.
 *   KEY       a uint32 k per particle; ascending k = drawn first.  b = the bits of d, with b = 0 when d == 0 (so -0 and +0 tie);
 *             a = (b >> 31) ? ~b : (b | 0x80000000), which ascends with d from -inf (0x007FFFFF) to +inf (0xFF800000);
 *             k = a for FW_SORT_FRONT_TO_BACK, k = ~a for FW_SORT_BACK_TO_FRONT.  A NaN depth has k = 0xFFFFFFFF in either order:
 *             drawn last; no other depth reaches that value.
 *   ORDER     ascending k, particles of equal k in particle-list order (a stable sort): the permutation is unique.  order[j] is the list
 *             index of the particle drawn j-th; sorted record j is the unsorted pack's record order[j], byte for byte.
 *   WHICH     exactly the particles fw_spawner_pack_instances_device writes for the same `cap`: the first min(count, cap) of the list,
 *             sorted among themselves.  *n_upper_bound means what it means there (the count is the device's; the host learns a bound).
 *             Records and order entries at and beyond min(count, cap) are not written.
 *   STREAM    the device forms enqueue on the context's main stream and answer for their place in it, as the unsorted device pack
 *             does: behind every fw_step called before, in front of every one called after.  They never wait -- with ONE exception,
 *             the one fw_ctx_set_colliders has: the sort's scratch (16 bytes per particle of the bound, plus a table) belongs to the
 *             context and only grows; a call that needs more than any call before it waits for the stream once and reallocates.
 *             The host form stages through the context's staging buffer and waits for its result.
 *   INDEXED   a host that keeps fused records (fw_spawner_attach_instances) draws them through the order: the record of list index i
 *             is d_out[i] there, and d_out[first + i] with the windowed attach (`first` of fw_spawner_instance_window).
 *   ERRORS    a null context, an unknown spawner or type, a null view or buffer, an `order` that is no FW_SORT_* value, reserved != 0:
 *             FW_EINVAL, nothing enqueued, nothing written.  (The host form takes out = NULL or cap = 0 to ask for the count alone.) */
enum { FW_SORT_BACK_TO_FRONT = 0, FW_SORT_FRONT_TO_BACK = 1 };
typedef struct fw_sort_view { /* 32 bytes */
    float eye[3];
    uint32_t order; /* FW_SORT_*; anything else: FW_EINVAL */
    float forward[3];
    uint32_t reserved; /* must be 0 */
} fw_sort_view;

/* ---- context ---------------------------------------------------------------- */
/* `stream` = an existing hipStream_t to enqueue on (e.g. torch's current stream),
 * or NULL to let the context create its own. */
int fw_abi_version(void);
fw_status fw_ctx_create(int device, uint32_t seed, void *stream, fw_ctx **out);
fw_status fw_ctx_destroy(fw_ctx *ctx);
const char *fw_last_error(const fw_ctx *ctx); /* ctx may be NULL: last create error */
void *fw_ctx_stream(const fw_ctx *ctx);       /* the hipStream_t in use */
fw_status fw_ctx_synchronize(fw_ctx *ctx);

/* replaces the context's collider set (copied; any n; n = 0 clears it).  Takes effect at the next fw_step.  Does NOT
 * synchronise: the set travels as one copy in the context's stream, behind the frames that read the old one (the
 * reference queries the live physics world every frame, core.rs:756-765 -- moving colliders cost one small copy per
 * frame).  Only a set larger than any before reallocates the device table, which waits for the frames in flight. */
fw_status fw_ctx_set_colliders(fw_ctx *ctx, const fw_collider *colliders, uint32_t n);

/* Meshes of the collider world (semantics next to fw_mesh_collider).  Creating one validates it -- FW_EINVAL for no vertices,
 * no triangles, an index >= n_vertices, a non-finite vertex, or no triangle left once the zero-area ones are dropped -- builds
 * its bounding-volume hierarchy on the host and uploads it once (synchronises).  xyz[n_vertices][3], indices[n_triangles][3]. */
fw_status fw_ctx_create_mesh(fw_ctx *ctx, const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                             fw_mesh *out);
/* like fw_ctx_create_mesh, but the mesh keeps what fw_ctx_update_mesh_vertices needs (its vertices and per-triangle vertex
 * indices on the device, pinned staging for new vertices); every triangle keeps a place in the hierarchy, zero-area ones marked */
fw_status fw_ctx_create_deformable_mesh(fw_ctx *ctx, const float *xyz, uint32_t n_vertices, const uint32_t *indices,
                                        uint32_t n_triangles, fw_mesh *out);
/* replaces the vertex positions of a deformable mesh (DEFORMABLE MESHES above); xyz[n_vertices][3] in host memory, n_vertices
 * as at creation.  Does not synchronise. */
fw_status fw_ctx_update_mesh_vertices(fw_ctx *ctx, fw_mesh mesh, const float *xyz, uint32_t n_vertices);
/* as fw_ctx_update_mesh_vertices, but d_xyz[n_vertices][3] (packed float) is DEVICE memory, read in the order of the context's
 * stream by the launches this call enqueues and by nothing later (DEFORMABLE MESHES: FROM DEVICE MEMORY).  Never synchronises;
 * a non-finite vertex is found by the device and reported through fw_ctx_mesh_update_status. */
fw_status fw_ctx_update_mesh_vertices_device(fw_ctx *ctx, fw_mesh mesh, const void *d_xyz, uint32_t n_vertices);
/* what the device has decided about the device-form updates of a deformable mesh so far: updates applied, updates rejected,
 * lowest non-finite vertex index of the latest rejected one (-1: none).  Any out pointer may be NULL.  Does not synchronise:
 * exact after fw_ctx_synchronize.  FW_EINVAL: unknown handle, mesh not deformable. */
fw_status fw_ctx_mesh_update_status(fw_ctx *ctx, fw_mesh mesh, uint64_t *n_applied, uint64_t *n_rejected, int64_t *first_bad_vertex);
/* FW_EINVAL while the current instance set places the mesh; otherwise waits for the frames in flight and frees it */
fw_status fw_ctx_destroy_mesh(fw_ctx *ctx, fw_mesh mesh);
/* replaces the context's mesh instances (copied; n = 0 clears them); all-or-nothing: an unknown mesh handle -> FW_EINVAL and
 * the previous set stays.  Like the analytic set it takes effect at the next fw_step and does not synchronise: the set travels
 * as one copy in the context's stream, and only a set larger than any before waits for the frames in flight. */
fw_status fw_ctx_set_mesh_colliders(fw_ctx *ctx, const fw_mesh_collider *instances, uint32_t n);
/* casts rays[n] into the collider world and writes hits[n] (RAY-CAST QUERIES above); host memory, synchronises */
fw_status fw_ctx_cast_rays(fw_ctx *ctx, const fw_ray *rays, uint64_t n, fw_ray_hit *hits);
/* the same for n fw_ray records at d_rays and n fw_ray_hit records at d_hits in DEVICE memory (16-byte aligned), read and written in
 * the order of the context's stream by the launches this call enqueues and by nothing else.  Never synchronises. */
fw_status fw_ctx_cast_rays_device(fw_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits);
/* projects points[n] onto the collider world and writes out[n] (POINT QUERIES above); host memory, synchronises */
fw_status fw_ctx_project_points(fw_ctx *ctx, const fw_point *points, uint64_t n, fw_point_projection *out);
/* the same for n fw_point records at d_points and n fw_point_projection records at d_out in DEVICE memory (16-byte aligned), read and
 * written in the order of the context's stream by the launches this call enqueues and by nothing else.  Never synchronises. */
fw_status fw_ctx_project_points_device(fw_ctx *ctx, const void *d_points, uint64_t n, void *d_out);
/* traces paths[n] through settings->n_steps steps and writes out[n] and, samples not NULL, samples[n_steps * n * 4] (PATH QUERIES
 * above); host memory, synchronises */
fw_status fw_ctx_trace_paths(fw_ctx *ctx, const fw_path_settings *settings, const fw_path *paths, uint64_t n, fw_path_result *out, float *samples);
/* the same for n fw_path records at d_paths, n fw_path_result records at d_out and (or NULL) n_steps * n float4 at d_samples in DEVICE
 * memory (16-byte aligned), read and written in the order of the context's stream by the launches this call enqueues and by nothing
 * else; settings is host memory, read inside the call.  Never synchronises. */
fw_status fw_ctx_trace_paths_device(fw_ctx *ctx, const fw_path_settings *settings, const void *d_paths, uint64_t n, void *d_out, void *d_samples);

/* ---- spawners ----------------------------------------------------------------- */
/* ParticleSpawner insertion + first sync_spawner_data (core.rs:343-365) */
fw_status fw_spawner_create(fw_ctx *ctx, const fw_spawner_desc *desc, fw_spawner *out);
/* Changed<ParticleSpawner>: sync_spawner_data again -- resets emission state, drops all particles */
fw_status fw_spawner_update_settings(fw_ctx *ctx, fw_spawner h, const fw_spawner_desc *desc);
fw_status fw_spawner_destroy(fw_ctx *ctx, fw_spawner h);

/* per-frame inputs the ECS owns */
fw_status fw_spawner_set_origin(fw_ctx *ctx, fw_spawner h, const float translation[3], const float rotation_xyzw[4]);
/* ... for ALL spawners in one call: spawn_particles walks every spawner entity in one system (core.rs:377), and a host with
 * thousands of them would otherwise cross the FFI once per spawner per frame.  handles[n], translations[n][3],
 * rotations_xyzw[n][4]; all-or-nothing: one invalid handle -> FW_EINVAL and no origin changes. */
fw_status fw_ctx_set_origins(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *translations,
                             const float *rotations_xyzw);
fw_status fw_spawner_set_parent_velocity(fw_ctx *ctx, fw_spawner h, const float v[3]); /* core.rs:276,444-448 */
fw_status fw_spawner_set_modifier(fw_ctx *ctx, fw_spawner h, float scale, float speed); /* EffectModifier core.rs:323-327 */
fw_status fw_spawner_queue(fw_ctx *ctx, fw_spawner h, uint64_t count);                  /* queue_particles core.rs:284-286 */
/* ... and the same three for MANY spawners in one call each (ABI 5).  The reference rewrites these inputs for whole sets of
 * spawners every frame -- sync_parent_velocity walks every spawner under a rigid body (core.rs:706-736),
 * propagate_particle_spawner_modifier every spawner under an EffectModifier (core.rs:690-703), a gameplay system queues
 * particles on every OnDemand spawner it owns -- and a host with thousands of emitters would cross the FFI once per spawner
 * per frame for each.  handles[n]; velocities[n][3]; scales[n], speeds[n]; counts[n] (added to what is queued, core.rs:284-286).
 * All-or-nothing like fw_ctx_set_origins: one invalid handle -> FW_EINVAL and nothing changes. */
fw_status fw_ctx_set_parent_velocities(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *velocities);
fw_status fw_ctx_set_modifiers(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *scales, const float *speeds);
fw_status fw_ctx_queue(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const uint64_t *counts);

/* ---- the frame: spawn_particles then update_particles for every spawner -------- */
fw_status fw_step(fw_ctx *ctx, float dt); /* core.rs:367-551 + 577-670 */

/* ---- outputs (synchronise the stream) ------------------------------------------- */
/* particles[i].len() for every type (core.rs:274) */
fw_status fw_spawner_counts(fw_ctx *ctx, fw_spawner h, uint32_t *per_type, uint32_t n_types);
/* ParticleSpawnerData::active (core.rs:288-302): *out = 0/1 */
fw_status fw_spawner_active(fw_ctx *ctx, fw_spawner h, int32_t *out);
/* notify_finished_particle_spawners (core.rs:674-688): *out = 1 exactly once */
fw_status fw_spawner_poll_finished(fw_ctx *ctx, fw_spawner h, int32_t *out);
/* copies min(count, cap) records; *n_out = count.  Order = reference Vec order. */
fw_status fw_spawner_read_particles(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle *out, uint64_t cap,
                                    uint64_t *n_out);
fw_status fw_spawner_read_last_emitted(fw_ctx *ctx, fw_spawner h, uint32_t type, uint32_t emission_index, float *out,
                                       uint64_t cap, uint64_t *n_out);
/* replaces the particle vector of `type` (`particles` is a pub field in the reference) */
fw_status fw_spawner_write_particles(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_particle *in, uint64_t n);
fw_status fw_spawner_write_last_emitted(fw_ctx *ctx, fw_spawner h, uint32_t type, uint32_t emission_index,
                                        const float *in, uint64_t n);
/* particles destroyed by the last fw_step for a type with report_destroyed (core.rs:588,596-599,660-667) */
fw_status fw_spawner_read_destroyed(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle *out, uint64_t cap,
                                    uint64_t *n_out);
/* ParticleInstance packing (render.rs:105-115,403) into a HOST buffer */
fw_status fw_spawner_pack_instances(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle_instance *out, uint64_t cap,
                                    uint64_t *n_out);
/* same, into a DEVICE buffer on the context's stream (no sync): the render hand-off */
fw_status fw_spawner_pack_instances_device(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap,
                                           uint64_t *n_upper_bound);
/* Render hand-off fused into the update (render.rs:403 builds these records on the CPU every frame): from the next
 * fw_step on, the update kernel itself also writes the ParticleInstance record of every particle of (spawner, type) that
 * survives the step into d_out[0 .. live count) -- device memory, `cap` records, particle order -- so the frame needs
 * no packing pass.  Records beyond `cap` are dropped.  Types that receive Nested children work too: children are spawned
 * before the update of the same frame (plugin.rs:46-60), so they are among the records.
 * d_out = NULL detaches; fw_spawner_update_settings (which rebuilds the particle types) detaches too.
 * Synchronises the DEVICE once (the segment record changes; and whatever the caller enqueued on its own streams to
 * initialise the buffer has completed before a frame writes into it -- the same holds for fw_ctx_live_count_ring). */
fw_status fw_spawner_attach_instances(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap);
/* The same hand-off for a host that can draw an instance SUB-RANGE (every graphics API can: firstInstance): the records of
 * the particles that survive a step are d_out[first, first + count), particle order, with `first` and `count` reported by
 * fw_spawner_instance_window after the step (one readback: the count has to be read anyway).  `first` is 0 on most update
 * paths; a particle type with a lifetime RANGE that the library keeps in a ring numbers its records from the particles the
 * step destroys (first = their number): with the plain attach above such a type is moved to the compacting path, with this
 * one it keeps its in-place update.  The buffer is indexed from 0, not from `first`: `cap` must cover first + count --
 * a buffer of the particle type's capacity always does (first + count never exceeds the live count before the step);
 * records at an index >= cap are dropped, so a buffer sized for the live count alone loses its last `first` records.
 * d_out = NULL detaches. */
fw_status fw_spawner_attach_instances_window(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap);
fw_status fw_spawner_instance_window(fw_ctx *ctx, fw_spawner h, uint32_t type, uint64_t *first, uint64_t *count);
/* DEPTH-SORTED INSTANCES above.  `view` is host memory, read inside the call.
 * order[j] = list index of the particle drawn j-th: uint32 in DEVICE memory, enqueued on the context's stream, never waits (but for
 * the growth of the scratch) */
fw_status fw_ctx_depth_order_device(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, void *d_order, uint64_t cap,
                                    uint64_t *n_upper_bound);
/* the ParticleInstance records in that order, into a DEVICE buffer (16-byte aligned); never waits (but for the growth of the scratch) */
fw_status fw_ctx_pack_instances_sorted_device(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, void *d_out, uint64_t cap,
                                              uint64_t *n_upper_bound);
/* the same into a HOST buffer; waits; copies min(count, cap) records, *n_out = count, as fw_spawner_pack_instances */
fw_status fw_ctx_pack_instances_sorted(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, fw_particle_instance *out,
                                       uint64_t cap, uint64_t *n_out);
/* update_aabbs reduction (render.rs:677-703), world space; *any = 0 when no particles */
fw_status fw_spawner_aabb(fw_ctx *ctx, fw_spawner h, float out_min[3], float out_max[3], int32_t *any);
/* AABB fused into the update: from the next fw_step on, every tile of the update kernel also leaves the box of
 * position -/+ scale of the survivors it stored (no extra pass over the particles, no extra launch in the frame);
 * fw_spawner_aabb then folds a few hundred 32-byte tile boxes instead of re-reading every particle.  Same result bit for
 * bit.  Frames with colliding particle types, and queries after the state was touched outside fw_step, fall back to the
 * two-pass reduction. */
fw_status fw_ctx_track_aabbs(fw_ctx *ctx, int32_t enable);
/* BATCHED BOXES (update_aabbs recomputes the box of EVERY spawner every frame, render.rs:677-703, and frustum culling reads them: a
 * host with thousands of emitters cannot cross the FFI, launch and wait once per spawner).  fw_ctx_aabbs answers the boxes of
 * handles[n] in one call, two kernel launches and one wait; fw_ctx_aabbs_device leaves the same records in DEVICE memory without
 * waiting, for a host that culls or builds indirect draws on the GPU.
 *   SAME BOX  out[i] is what fw_spawner_aabb(handles[i]) answers at the same place in the stream: min / max of position -/+ scale over
 *             every particle of every particle type, scale as every reader evaluates it; any = 1 exactly where that call sets *any.
 *             A spawner that holds no particle gets any = 0, min = {FLT_MAX, FLT_MAX, FLT_MAX} and max = {-FLT_MAX, -FLT_MAX,
 *             -FLT_MAX} (3.40282347e+38: the values the reduction starts from).  min / max skip a NaN as fminf / fmaxf do.  Equal means
 *             equal as floats: -0 and +0 are the same answer (the order of a min over the two is nobody's to promise).  `reserved` is
 *             written as 0.  The batched forms always read the particles: the answer is the same with fw_ctx_track_aabbs on or off.
 *   ORDER     out[i] belongs to handles[i]; a handle may appear more than once, and each place is answered.
 *   RULES     as fw_spawner_aabb: frames a FIFO ring withheld are enqueued first (once), stale ages of such a ring are written back, a
 *             deferred spin stays deferred -- a host that asks every frame keeps those rules.
 *   STREAM    the device form enqueues on the context's main stream (fw_ctx_stream), behind every fw_step called before it and in front
 *             of every one called after; its host work grows with the number of listed particle types, never with the particles.  It
 *             never waits -- with the ONE exception fw_ctx_depth_order_device has: the tables and the scratch (32 bytes per 512
 *             particles of the listed types' bounds) belong to the context and only grow; a call that needs more than any call before
 *             it waits for the stream once and reallocates.  d_out: n records, 16-byte aligned.  The host form has the records
 *             written to pinned memory the context keeps, waits once and copies; it reports FW_ECAPACITY as fw_spawner_aabb does: the
 *             boxes are written and the status is returned.
 *   ERRORS    a null context, n > 0 with null handles or a null (or misaligned) output, ONE invalid handle anywhere in the list
 *             (all-or-nothing, as fw_ctx_set_origins): FW_EINVAL, nothing enqueued, nothing written.  n == 0: FW_OK, nothing touched.
 *             A poisoned spawner in the list ends the call with the status fw_spawner_aabb gives for it, and nothing is written. */
typedef struct fw_aabb { /* 32 bytes */
    float min[3];
    int32_t any; /* 0: the spawner holds no particle */
    float max[3];
    uint32_t reserved; /* written as 0 */
} fw_aabb;
fw_status fw_ctx_aabbs(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, fw_aabb *out);
fw_status fw_ctx_aabbs_device(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, void *d_out);

/* ---- VOLUME QUERIES ------------------------------------------------------------------ */
/* How many particles lie inside analytic volumes -- "how many fire particles are in the player's capsule", "is this trigger box full of
 * smoke" (Unity's particle Triggers module; on the CPU reference a loop over ParticleSpawnerData::particles).  Every other query asks
 * about the collider world; this one asks about the particles, without moving them to the host and without ending an unread FIFO
 * ring's rules.  out[p * n_volumes + v] is the number of particles of places[p] whose position lies inside volumes[v], counted at the
 * call's place in the context's stream (modulo 2^32).
 *   INSIDE    a volume is an fw_collider record of any of the six kinds; `layers` is ignored.  A particle is inside exactly when the
 *             kind's INSIDE expression above holds for its position -- the expression the ray cast tests for its distance-0 case, and
 *             what fw_point_projection.is_inside reports in a world that holds this collider alone -- operation by operation, fp32, no
 *             fused a*b+c: PLANE dot(n, position - x) > 0; SPHERE (dot(v, v) - radius * radius) <= 0 with v = x - position; BOX
 *             |o.x| <= hx and |o.y| <= hy and |o.z| <= hz; CYLINDER |o.y| <= hh and (xz - rr) <= 0; CONE o.y >= -hh and wy <= 0 and
 *             (xz - k2 * (wy * wy)) <= 0; CAPSULE ((xz + (dy * dy)) - rr) <= 0, with o, xz, rr, k2, wy, dy as POINT QUERIES states them
 *             (the identity rotation skips the product).  A point ON the boundary is inside: a sphere of radius 1 at the origin
 *             contains (1, 0, 0).  The particle is a point: its scale plays no part.  A NaN position is inside nothing (every
 *             comparison is false).  A volume with NaN or negative extents gives whatever the operations give, deterministically.
 *             Meshes are surfaces and cannot be volumes.
 *   WHICH     list positions [0, min(device count, host bound)) of each listed segment; the bound is fw_ctx_aabbs's (the capacity for a
 *             type that Nested entries feed).  type = -1 lists every particle type of the spawner.  A spawner or type that holds
 *             nothing counts 0.
 *   ORDER     places may repeat and come in any order; every place is answered.
 *   RULES     as fw_spawner_aabb, frames a FIFO ring withheld are enqueued first, once.  Unlike the boxes the query reads POSITIONS
 *             only: stale ages of such a ring STAY stale (nothing is written back), a deferred spin stays deferred -- a host that asks
 *             every frame keeps every rule of an unread ring, the fusing of frames aside.
 *   STREAM    both forms enqueue on the context's main stream (fw_ctx_stream), behind every fw_step called before and in front of
 *             every one called after.  `places` and `volumes` are host memory, copied inside the call.  The device form's host work
 *             grows with the listed particle types plus the volumes, never with the particles; it never waits -- with the ONE exception
 *             fw_ctx_aabbs_device has: the tables and the scratch (4 bytes per volume and 512 particles of the listed types' bounds)
 *             belong to the context and only grow, and a call that needs more than any call before it waits for the stream once and
 *             reallocates.  d_out: n_places * n_volumes uint32, 4-byte aligned.  Two kernel launches per call whatever the sizes (one
 *             where no listed type can hold a particle: the answer is all zeros).  The host form has the counts written to pinned
 *             memory the context keeps, waits once and copies; it reports FW_ECAPACITY as fw_ctx_aabbs does.
 *   ERRORS    all-or-nothing: a null context; null places, volumes or output with n_places * n_volumes != 0; ONE invalid handle; a type
 *             that is neither -1 nor below its spawner's number of particle types; a kind that is none of the six; a misaligned d_out;
 *             n_places * n_volumes > FW_VOLUME_MAX_ANSWERS (every answer is a one-wave workgroup of the second launch): FW_EINVAL,
 *             nothing enqueued, nothing written.  n_places == 0 or n_volumes == 0: FW_OK, nothing touched.  A poisoned spawner in the
 *             list ends the call as it ends fw_ctx_aabbs. */
#define FW_VOLUME_MAX_ANSWERS 0x3FFFFFFull
typedef struct fw_volume_place { /* 8 bytes */
    fw_spawner spawner;
    int32_t type; /* -1: every particle type of the spawner */
} fw_volume_place;
fw_status fw_ctx_count_in_volumes(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes, const fw_collider *volumes,
                                  uint32_t *out);
fw_status fw_ctx_count_in_volumes_device(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes,
                                         const fw_collider *volumes, void *d_out);

/* ---- whole-context statistics ---------------------------------------------------- */
/* total live particles over all spawners (host value; synchronises) */
fw_status fw_ctx_live_count(fw_ctx *ctx, uint64_t *out);
/* enqueue a write of the total live count into a caller-owned DEVICE uint64 (no
 * sync): feed for the RCCL all-reduce of live counts across GPUs */
fw_status fw_ctx_live_count_device(fw_ctx *ctx, void *d_out_u64);
/* register a caller-owned DEVICE ring of n_slots (>= 2) uint64: from now on every fw_step leaves the total live
 * count of its frame in slot (k mod n_slots), k = frames stepped since registration, at no extra launch
 * (written by the update kernel itself).  NULL unregisters.  Bucketed RCCL all-reduce feed. */
fw_status fw_ctx_live_count_ring(fw_ctx *ctx, void *d_ring_u64, uint32_t n_slots);
/* running total of particles that entered update_particles (after spawn) since the context was created */
fw_status fw_ctx_last_step_updated(fw_ctx *ctx, uint64_t *out);

/* (measurement and debugging hooks -- kernel timing, the copy-bandwidth probe, in-kernel timestamps, which update path a
 * particle type is on -- are declared in firework_hip_debug.h: exported by the same library, not part of the surface a
 * host binds) */

/* ---- pure host helpers (no GPU needed; the bit-exact count arithmetic) ------------ */
/* compute_emission_count (core.rs:553-575) exactly as fw_step's host side evaluates it */
uint64_t fw_compute_emission_count(float time_passed_in_cycle, float last_emission, float cycle_duration,
                                   float offset_start, float offset_end, float particles_per_cycle,
                                   float *next_last_emission);

#ifdef __cplusplus
}
#endif
#endif /* FIREWORK_HIP_H */
