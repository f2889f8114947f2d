"""Host-side mirror of the reference's plugin surface over the HIP backend.

``ParticleSystem`` plays the role of ``ParticleSystemPlugin`` (reference
src/plugin.rs:22-61): it owns one GPU context and ``update(dt)`` runs the
chained per-frame systems -- sync_spawner_data, spawn_particles,
update_particles, notify_finished_particle_spawners -- for every spawner, on
the device, through the C ABI of include/firework_hip.h.

``SpawnerData`` mirrors ``ParticleSpawnerData`` (src/core.rs:269-303):
``queue_particles``, ``active`` and read access to ``particles``.

No simulation arithmetic happens in Python and there is no CPU fallback: the
shared library must be built (hipcc, gfx950) and a GPU must be present.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import numpy as np

from . import _ffi
from . import settings as S
from ._ffi import FwError


class SpawnerData:
    """Runtime state handle of one spawner (ParticleSpawnerData, core.rs:269-303)."""

    def __init__(self, system: "ParticleSystem", handle: int, spawner: S.ParticleSpawner, uid: int):
        self._sys = system
        self.handle = handle
        self.settings = spawner
        self.uid = uid
        self.transform = S.Transform()
        self.global_transform: Optional[S.Transform] = None
        self.on_finished: List[Callable[["SpawnerData"], None]] = []

    # -- inputs ---------------------------------------------------------------------
    def queue_particles(self, count: int) -> None:  # core.rs:284-286
        self._sys._check(self._sys._lib.fw_spawner_queue(self._sys._ctx, self.handle, int(count)))

    def set_transform(self, transform: S.Transform, global_transform: Optional[S.Transform] = None) -> None:
        self.transform = transform
        self.global_transform = global_transform

    def set_parent_velocity(self, v) -> None:  # core.rs:276
        arr = (C.c_float * 3)(*[float(c) for c in v])
        self._sys._check(self._sys._lib.fw_spawner_set_parent_velocity(self._sys._ctx, self.handle, arr))

    def set_modifier(self, m: S.EffectModifier) -> None:  # core.rs:323-327
        self._sys._check(self._sys._lib.fw_spawner_set_modifier(self._sys._ctx, self.handle, float(m.scale), float(m.speed)))

    def update_settings(self, spawner: S.ParticleSpawner) -> None:
        """Changed<ParticleSpawner>: sync_spawner_data resets state and drops particles (core.rs:343-365)."""
        desc, keep = _ffi.make_desc(spawner, self.uid)
        self._sys._check(self._sys._lib.fw_spawner_update_settings(self._sys._ctx, self.handle, C.byref(desc)))
        self.settings = spawner

    # -- outputs (synchronise) -----------------------------------------------------------
    def counts(self) -> List[int]:
        n = len(self.settings.particle_settings)
        out = (C.c_uint32 * max(n, 1))()
        self._sys._check(self._sys._lib.fw_spawner_counts(self._sys._ctx, self.handle, out, n))
        return [int(out[i]) for i in range(n)]

    def count(self, particle_type: int = 0) -> int:
        return self.counts()[particle_type]

    def active(self) -> bool:  # core.rs:288-302
        out = C.c_int32()
        self._sys._check(self._sys._lib.fw_spawner_active(self._sys._ctx, self.handle, C.byref(out)))
        return bool(out.value)

    def poll_finished(self) -> bool:  # core.rs:674-688
        out = C.c_int32()
        self._sys._check(self._sys._lib.fw_spawner_poll_finished(self._sys._ctx, self.handle, C.byref(out)))
        return bool(out.value)

    def particles(self, particle_type: int = 0) -> np.ndarray:
        """``data.particles[particle_type]`` as a structured array (settings.PARTICLE_DTYPE)."""
        n = C.c_uint64()
        L, ctx = self._sys._lib, self._sys._ctx
        self._sys._check(L.fw_spawner_read_particles(ctx, self.handle, particle_type, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=S.PARTICLE_DTYPE)
        if n.value:
            self._sys._check(L.fw_spawner_read_particles(ctx, self.handle, particle_type, out.ctypes.data_as(C.c_void_p),
                                                         n.value, C.byref(n)))
        return out

    def last_emitted(self, particle_type: int, emission_index: int) -> np.ndarray:
        n = C.c_uint64()
        L, ctx = self._sys._lib, self._sys._ctx
        self._sys._check(L.fw_spawner_read_last_emitted(ctx, self.handle, particle_type, emission_index, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float32)
        if n.value:
            self._sys._check(L.fw_spawner_read_last_emitted(ctx, self.handle, particle_type, emission_index,
                                                            out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def write_particles(self, particle_type: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr, dtype=S.PARTICLE_DTYPE)
        self._sys._check(self._sys._lib.fw_spawner_write_particles(self._sys._ctx, self.handle, particle_type,
                                                                   arr.ctypes.data_as(C.c_void_p), len(arr)))

    def write_last_emitted(self, particle_type: int, emission_index: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        self._sys._check(self._sys._lib.fw_spawner_write_last_emitted(self._sys._ctx, self.handle, particle_type,
                                                                      emission_index, arr.ctypes.data_as(C.c_void_p), len(arr)))

    def destroyed(self, particle_type: int = 0) -> np.ndarray:
        n = C.c_uint64()
        L, ctx = self._sys._lib, self._sys._ctx
        self._sys._check(L.fw_spawner_read_destroyed(ctx, self.handle, particle_type, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=S.PARTICLE_DTYPE)
        if n.value:
            self._sys._check(L.fw_spawner_read_destroyed(ctx, self.handle, particle_type, out.ctypes.data_as(C.c_void_p),
                                                         n.value, C.byref(n)))
        return out

    def instances(self, particle_type: int = 0) -> np.ndarray:
        """ParticleInstance records for the render extract (render.rs:95-115)."""
        n = C.c_uint64()
        L, ctx = self._sys._lib, self._sys._ctx
        self._sys._check(L.fw_spawner_pack_instances(ctx, self.handle, particle_type, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=S.INSTANCE_DTYPE)
        if n.value:
            self._sys._check(L.fw_spawner_pack_instances(ctx, self.handle, particle_type, out.ctypes.data_as(C.c_void_p),
                                                         n.value, C.byref(n)))
        return out

    def instances_sorted(self, view: S.SortView, particle_type: int = 0) -> np.ndarray:
        """``instances()`` sorted by view depth for an alpha-blended draw (include/firework_hip.h: DEPTH-SORTED INSTANCES): the same
        records, byte for byte, in ascending key order of ``view``, ties in particle-list order.  Synchronises."""
        n = C.c_uint64()
        L, ctx, v = self._sys._lib, self._sys._ctx, _ffi.make_sort_view(view)
        self._sys._check(L.fw_ctx_pack_instances_sorted(ctx, self.handle, particle_type, C.byref(v), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=S.INSTANCE_DTYPE)
        if n.value:
            self._sys._check(L.fw_ctx_pack_instances_sorted(ctx, self.handle, particle_type, C.byref(v), out.ctypes.data_as(C.c_void_p),
                                                            n.value, C.byref(n)))
        return out

    def attach_instances(self, device_ptr: int, capacity: int, particle_type: int = 0) -> None:
        """From the next step on the update kernel also writes this type's ParticleInstance records (render.rs:95-115)
        into the caller's device buffer (`capacity` 64-byte records); 0 detaches."""
        self._sys._check(self._sys._lib.fw_spawner_attach_instances(
            self._sys._ctx, self.handle, particle_type, C.c_void_p(device_ptr) if device_ptr else None, int(capacity)))

    def attach_instances_window(self, device_ptr: int, capacity: int, particle_type: int = 0) -> None:
        """The same for a host that can draw an instance sub-range: the records of a step's survivors are
        buffer[first : first + count] with (first, count) = ``instance_window()``; lets a lifetime-range type keep its ring."""
        self._sys._check(self._sys._lib.fw_spawner_attach_instances_window(
            self._sys._ctx, self.handle, particle_type, C.c_void_p(device_ptr) if device_ptr else None, int(capacity)))

    def instance_window(self, particle_type: int = 0):
        """(first, count) of the attached windowed buffer's live records after the last step (synchronises)"""
        first, count = C.c_uint64(), C.c_uint64()
        self._sys._check(self._sys._lib.fw_spawner_instance_window(self._sys._ctx, self.handle, particle_type, C.byref(first), C.byref(count)))
        return int(first.value), int(count.value)

    def update_path(self, particle_type: int = 0):
        """("fifo" | "range" | "general" | "small" (one wave per type, the compacting layout), bytes one update of a live particle moves, of which algorithmic) -- which kernel family
        updates this type and what it costs per particle (bench.py's roofline accounting)"""
        mode, moved, algo = C.c_int32(), C.c_uint32(), C.c_uint32()
        self._sys._check(self._sys._lib.fw_debug_update_path(self._sys._ctx, self.handle, particle_type, C.byref(mode),
                                                             C.byref(moved), C.byref(algo)))
        # (4: a WIDE small type -- a workgroup of the same kernel instead of a wave; update_mode() tells the two apart)
        return {0: "general", 1: "fifo", 2: "range", 3: "small", 4: "small"}[mode.value], int(moved.value), int(algo.value)

    def update_mode(self, particle_type: int = 0) -> int:
        """the raw mode of fw_debug_update_path: 0 compacting, 1 FIFO ring, 2 range ring, 3 small (a wave), 4 small (a workgroup)"""
        mode = C.c_int32()
        self._sys._check(self._sys._lib.fw_debug_update_path(self._sys._ctx, self.handle, particle_type, C.byref(mode), None, None))
        return int(mode.value)

    def aabb(self):
        """(any, min, max) of position -/+ scale over all particle types (render.rs:677-703)."""
        mn, mx, any_ = (C.c_float * 3)(), (C.c_float * 3)(), C.c_int32()
        self._sys._check(self._sys._lib.fw_spawner_aabb(self._sys._ctx, self.handle, mn, mx, C.byref(any_)))
        return bool(any_.value), np.array(mn[:], dtype=np.float32), np.array(mx[:], dtype=np.float32)


class ParticleSystem:
    """One GPU context + its spawners; ``update(dt)`` is one frame of the plugin's system chain."""

    def __init__(self, device: int = 0, seed: int = 0, stream: Optional[int] = None):
        self._lib = _ffi.load()
        ctx = C.c_void_p()
        st = self._lib.fw_ctx_create(int(device), int(seed) & 0xFFFFFFFF, C.c_void_p(stream) if stream else None, C.byref(ctx))
        if st != _ffi.FW_OK:
            msg = self._lib.fw_last_error(None)
            raise FwError(st, msg.decode() if msg else "fw_ctx_create failed")
        self._ctx = ctx
        self.device = device
        self.seed = seed
        self.spawners: Dict[int, SpawnerData] = {}
        self._next_uid = 0
        self._keep: List = []

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, status: int) -> None:
        if status != _ffi.FW_OK:
            msg = self._lib.fw_last_error(self._ctx)
            raise FwError(status, msg.decode() if msg else "")

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.fw_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def stream(self) -> int:
        return int(self._lib.fw_ctx_stream(self._ctx) or 0)

    def synchronize(self) -> None:
        self._check(self._lib.fw_ctx_synchronize(self._ctx))

    def set_colliders(self, colliders) -> None:
        """The world particle_collision casts its rays into (core.rs:744-800): a device-resident set of analytic
        colliders (settings.Collider) standing in for avian's SpatialQuery."""
        self._check(self._lib.fw_ctx_set_colliders(self._ctx, _ffi.make_colliders(colliders), len(colliders)))

    def create_mesh(self, vertices, indices) -> int:
        """Uploads a triangle mesh of the collider world (vertices [n, 3] float32, indices [m, 3] uint32) and returns its
        handle; place it with set_mesh_colliders.  Zero-area triangles are dropped; bad input raises FW_EINVAL."""
        xyz = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        h = C.c_int32(-1)
        self._check(self._lib.fw_ctx_create_mesh(self._ctx, xyz.ctypes.data_as(C.c_void_p), len(xyz),
                                                 idx.ctypes.data_as(C.c_void_p), len(idx), C.byref(h)))
        return int(h.value)

    def create_deformable_mesh(self, vertices, indices) -> int:
        """create_mesh for a mesh whose vertices will move: it takes new positions through update_mesh_vertices.  Every
        triangle keeps its place; zero-area ones are hit by nothing until an update opens them up."""
        xyz = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        h = C.c_int32(-1)
        self._check(self._lib.fw_ctx_create_deformable_mesh(self._ctx, xyz.ctypes.data_as(C.c_void_p), len(xyz),
                                                            idx.ctypes.data_as(C.c_void_p), len(idx), C.byref(h)))
        return int(h.value)

    def update_mesh_vertices(self, mesh: int, vertices) -> None:
        """Replaces the vertex positions of a deformable mesh ([n, 3] float32, n as at creation): later frames cast against the
        mesh as if it had been created from them.  All-or-nothing, no synchronisation (the array is copied before the call
        returns); placed instances follow."""
        xyz = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self._check(self._lib.fw_ctx_update_mesh_vertices(self._ctx, int(mesh), xyz.ctypes.data_as(C.c_void_p), len(xyz)))

    def update_mesh_vertices_device(self, mesh: int, data_ptr: int, n_vertices: int) -> None:
        """update_mesh_vertices for positions that are already in device memory: data_ptr is the device address of n_vertices
        packed float32 triples (a torch tensor's data_ptr(), as attach_instances takes one), written on this context's stream
        or ordered in front of it by the caller.  Never synchronises and copies nothing: the buffer is read by work enqueued
        inside the call only, so it may be overwritten by work ordered behind the call.  A non-finite vertex is found on the
        device: that update is rejected there and the mesh keeps its shape (mesh_update_status)."""
        self._check(self._lib.fw_ctx_update_mesh_vertices_device(self._ctx, int(mesh), C.c_void_p(int(data_ptr)), int(n_vertices)))

    def mesh_update_status(self, mesh: int):
        """-> (applied, rejected, first_bad_vertex) of the mesh's device-form updates as the device has reported them so far
        (first_bad_vertex: the lowest non-finite index of the latest rejected update, -1 for none).  Does not synchronise; exact
        after synchronize()."""
        a, r, b = C.c_uint64(0), C.c_uint64(0), C.c_int64(-1)
        self._check(self._lib.fw_ctx_mesh_update_status(self._ctx, int(mesh), C.byref(a), C.byref(r), C.byref(b)))
        return int(a.value), int(r.value), int(b.value)

    def destroy_mesh(self, mesh: int) -> None:
        """Frees a mesh the current instance set does not place (waits for the frames in flight)."""
        self._check(self._lib.fw_ctx_destroy_mesh(self._ctx, int(mesh)))

    def set_mesh_colliders(self, instances) -> None:
        """Replaces the placed meshes (settings.MeshCollider) of the collider world; all-or-nothing, no synchronisation."""
        self._check(self._lib.fw_ctx_set_mesh_colliders(self._ctx, _ffi.make_mesh_colliders(instances), len(instances)))

    def cast_rays(self, origins, dirs, max_distances, masks) -> np.ndarray:
        """SpatialQuery::cast_ray for a batch: origins [n, 3], dirs [n, 3] (used as given: pass unit vectors for distances in
        world units), max_distances [n] or a scalar, masks [n] or a scalar (as ParticleCollisionSettings.filter_mask) -> a
        structured array (settings.RAY_HIT_DTYPE) of the nearest hit of each ray in the collider world as it stands behind
        every call made so far: distance and normal are bit for bit what a particle's own cast gives, kind / index / triangle
        name what was hit (settings.HIT_*; index counts in the list given to set_colliders / set_mesh_colliders).
        Synchronises."""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        rays = np.zeros(len(o), dtype=S.RAY_DTYPE)
        rays["origin"] = o
        rays["dir"] = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
        rays["max_distance"] = np.asarray(max_distances, dtype=np.float32)
        rays["filter_mask"] = np.asarray(masks, dtype=np.uint32)
        return self.cast_ray_records(rays)

    def cast_ray_records(self, rays: np.ndarray) -> np.ndarray:
        """cast_rays for rays that are already settings.RAY_DTYPE records"""
        rays = np.ascontiguousarray(rays, dtype=S.RAY_DTYPE)
        hits = np.zeros(len(rays), dtype=S.RAY_HIT_DTYPE)
        self._check(self._lib.fw_ctx_cast_rays(self._ctx, rays.ctypes.data_as(C.c_void_p), len(rays), hits.ctypes.data_as(C.c_void_p)))
        return hits

    def cast_rays_device(self, rays_ptr: int, n: int, hits_ptr: int) -> None:
        """cast_rays for n settings.RAY_DTYPE records at device address rays_ptr into n settings.RAY_HIT_DTYPE records at
        hits_ptr (torch tensors' data_ptr()): enqueued on this context's stream, never synchronises; the buffers are read and
        written only by work enqueued inside the call."""
        self._check(self._lib.fw_ctx_cast_rays_device(self._ctx, C.c_void_p(int(rays_ptr)) if rays_ptr else None, int(n),
                                                      C.c_void_p(int(hits_ptr)) if hits_ptr else None))

    def project_points(self, positions, masks) -> np.ndarray:
        """SpatialQuery::project_point (solid = true) for a batch: positions [n, 3], masks [n] or a scalar -> a structured array
        (settings.POINT_PROJECTION_DTYPE): the nearest point of the collider world as it stands behind every call made so far,
        its distance, who owns it (kind / index / triangle as cast_rays reports them) and is_inside (1: the position lies inside
        or on the analytic solid named -- point_intersections' question; point is then the position, distance 0).  Synchronises."""
        p = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
        points = np.zeros(len(p), dtype=S.POINT_DTYPE)
        points["position"] = p
        points["filter_mask"] = np.asarray(masks, dtype=np.uint32)
        return self.project_point_records(points)

    def project_point_records(self, points: np.ndarray) -> np.ndarray:
        """project_points for points that are already settings.POINT_DTYPE records"""
        points = np.ascontiguousarray(points, dtype=S.POINT_DTYPE)
        out = np.zeros(len(points), dtype=S.POINT_PROJECTION_DTYPE)
        self._check(self._lib.fw_ctx_project_points(self._ctx, points.ctypes.data_as(C.c_void_p), len(points), out.ctypes.data_as(C.c_void_p)))
        return out

    def project_points_device(self, points_ptr: int, n: int, out_ptr: int) -> None:
        """project_points for n settings.POINT_DTYPE records at device address points_ptr into n settings.POINT_PROJECTION_DTYPE
        records at out_ptr: enqueued on this context's stream, never synchronises; the buffers are read and written only by work
        enqueued inside the call."""
        self._check(self._lib.fw_ctx_project_points_device(self._ctx, C.c_void_p(int(points_ptr)) if points_ptr else None, int(n),
                                                           C.c_void_p(int(out_ptr)) if out_ptr else None))

    def trace_paths(self, settings: S.PathSettings, positions, velocities, ages=0.0, lifetimes=np.inf, samples: bool = False):
        """Where particles WOULD go: positions [n, 3], velocities [n, 3], ages and lifetimes [n] or scalars, stepped settings.n_steps
        times by settings.dt with the arithmetic update_particles gives a particle of a type with these settings, in the collider
        world as it stands behind every call made so far (frozen for the whole path) -> a structured array
        (settings.PATH_RESULT_DTYPE): where each path ended and how (status: settings.PATH_*), its first contact and how many it had.
        samples=True: -> (results, samples[n_steps, n, 4]), {position, age} after every step.  Nothing is spawned.  Synchronises."""
        p = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
        paths = np.zeros(len(p), dtype=S.PATH_DTYPE)
        paths["position"] = p
        paths["velocity"] = np.asarray(velocities, dtype=np.float32).reshape(-1, 3)
        paths["age"] = np.asarray(ages, dtype=np.float32)
        paths["lifetime"] = np.asarray(lifetimes, dtype=np.float32)
        return self.trace_path_records(settings, paths, samples)

    def trace_path_records(self, settings: S.PathSettings, paths: np.ndarray, samples: bool = False):
        """trace_paths for paths that are already settings.PATH_DTYPE records"""
        paths = np.ascontiguousarray(paths, dtype=S.PATH_DTYPE)
        out = np.zeros(len(paths), dtype=S.PATH_RESULT_DTYPE)
        smp = np.zeros((int(settings.n_steps), len(paths), 4), dtype=np.float32) if samples else None
        self._check(self._lib.fw_ctx_trace_paths(self._ctx, C.byref(_ffi.make_path_settings(settings)), paths.ctypes.data_as(C.c_void_p), len(paths),
                                                 out.ctypes.data_as(C.c_void_p), smp.ctypes.data_as(C.c_void_p) if samples else None))
        return (out, smp) if samples else out

    def trace_paths_device(self, settings: S.PathSettings, paths_ptr: int, n: int, out_ptr: int, samples_ptr: int = 0) -> None:
        """trace_paths for n settings.PATH_DTYPE records at device address paths_ptr into n settings.PATH_RESULT_DTYPE records at
        out_ptr and, samples_ptr not 0, settings.n_steps * n float4 there ([step][path]): enqueued on this context's stream, never
        synchronises; the buffers are read and written only by work enqueued inside the call."""
        self._check(self._lib.fw_ctx_trace_paths_device(self._ctx, C.byref(_ffi.make_path_settings(settings)), C.c_void_p(int(paths_ptr)) if paths_ptr else None,
                                                        int(n), C.c_void_p(int(out_ptr)) if out_ptr else None,
                                                        C.c_void_p(int(samples_ptr)) if samples_ptr else None))

    def pack_instances_sorted_device(self, data: SpawnerData, view: S.SortView, out_ptr: int, capacity: int, particle_type: int = 0) -> int:
        """The depth-sorted ParticleInstance records of (data, particle_type) into `capacity` 64-byte records at device address out_ptr:
        the first min(count, capacity) particles of the list, sorted among themselves (SpawnerData.instances_sorted has the order).
        Enqueued on this context's stream; never synchronises, except once when the sort's scratch has to grow.  -> the host's upper
        bound of the number of records written (the count itself is the device's)."""
        ub = C.c_uint64()
        self._check(self._lib.fw_ctx_pack_instances_sorted_device(self._ctx, data.handle, int(particle_type), C.byref(_ffi.make_sort_view(view)),
                                                                  C.c_void_p(int(out_ptr)) if out_ptr else None, int(capacity), C.byref(ub)))
        return int(ub.value)

    def depth_order_device(self, data: SpawnerData, view: S.SortView, order_ptr: int, capacity: int, particle_type: int = 0) -> int:
        """The permutation alone: order[j] (uint32 at device address order_ptr, `capacity` entries) = list index of the particle drawn
        j-th -- for a host that draws fused records (attach_instances) through an index.  Same stream rule and return value as
        pack_instances_sorted_device."""
        ub = C.c_uint64()
        self._check(self._lib.fw_ctx_depth_order_device(self._ctx, data.handle, int(particle_type), C.byref(_ffi.make_sort_view(view)),
                                                        C.c_void_p(int(order_ptr)) if order_ptr else None, int(capacity), C.byref(ub)))
        return int(ub.value)

    # -- ECS-like surface ------------------------------------------------------------------------
    def spawn(self, spawner: S.ParticleSpawner, transform: Optional[S.Transform] = None,
              global_transform: Optional[S.Transform] = None, modifier: Optional[S.EffectModifier] = None,
              uid: Optional[int] = None) -> SpawnerData:
        """commands.spawn((ParticleSpawner {..}, Transform)): returns the ParticleSpawnerData handle."""
        if uid is None:
            uid = self._next_uid
        self._next_uid = max(self._next_uid, uid + 1)
        desc, keep = _ffi.make_desc(spawner, uid)
        h = C.c_int32(-1)
        self._check(self._lib.fw_spawner_create(self._ctx, C.byref(desc), C.byref(h)))
        data = SpawnerData(self, h.value, spawner, uid)
        if transform is not None:
            data.set_transform(transform, global_transform)
        if modifier is not None:
            data.set_modifier(modifier)
        self.spawners[h.value] = data
        return data

    def despawn(self, data: SpawnerData) -> None:
        self._check(self._lib.fw_spawner_destroy(self._ctx, data.handle))
        self.spawners.pop(data.handle, None)

    def _push_origins(self) -> None:
        """the transforms of ALL spawners in one call (fw_ctx_set_origins): spawn_particles reads them for every spawner
        entity of the query in one system (core.rs:377, 432-435)"""
        n = len(self.spawners)
        if not n:
            return
        handles = (C.c_int32 * n)()
        tr = (C.c_float * (3 * n))()
        ro = (C.c_float * (4 * n))()
        for i, d in enumerate(self.spawners.values()):
            # SpawnTransformMode (core.rs:432-435): Global -> GlobalTransform.compute_transform(), Local -> Transform
            t = d.transform
            if d.settings.spawn_transform_mode == S.SpawnTransformMode.Global and d.global_transform is not None:
                t = d.global_transform
            handles[i] = d.handle
            tr[3 * i:3 * i + 3] = [float(c) for c in t.translation]
            ro[4 * i:4 * i + 4] = [float(c) for c in t.rotation]
        self._check(self._lib.fw_ctx_set_origins(self._ctx, n, handles, tr, ro))

    # the other per-frame inputs of MANY spawners in one FFI call each (ABI 5): what sync_parent_velocity (core.rs:706-736),
    # propagate_particle_spawner_modifier (core.rs:690-703) and a gameplay system that queues on its OnDemand spawners write
    def set_parent_velocities(self, spawners, velocities) -> None:
        n = len(spawners)
        handles = (C.c_int32 * max(n, 1))(*[d.handle for d in spawners])
        v = (C.c_float * max(3 * n, 1))(*[float(c) for vel in velocities for c in vel])
        self._check(self._lib.fw_ctx_set_parent_velocities(self._ctx, n, handles, v))

    def set_modifiers(self, spawners, modifiers) -> None:
        n = len(spawners)
        handles = (C.c_int32 * max(n, 1))(*[d.handle for d in spawners])
        sc = (C.c_float * max(n, 1))(*[float(m.scale) for m in modifiers])
        sp = (C.c_float * max(n, 1))(*[float(m.speed) for m in modifiers])
        self._check(self._lib.fw_ctx_set_modifiers(self._ctx, n, handles, sc, sp))

    def queue_particles(self, spawners, counts) -> None:
        n = len(spawners)
        handles = (C.c_int32 * max(n, 1))(*[d.handle for d in spawners])
        cn = (C.c_uint64 * max(n, 1))(*[int(c) for c in counts])
        self._check(self._lib.fw_ctx_queue(self._ctx, n, handles, cn))

    def step(self, dt: float) -> None:
        """Enqueue one frame (spawn_particles + update_particles) without touching transforms or callbacks."""
        self._check(self._lib.fw_step(self._ctx, float(dt)))

    def update(self, dt: float) -> None:
        """One run of the plugin's chained systems (plugin.rs:46-60)."""
        self._push_origins()
        self.step(dt)
        for d in self.spawners.values():
            handlers = [(i, p.particles_destroyed) for i, p in enumerate(d.settings.particle_settings)
                        if p.particles_destroyed is not None]
            for i, fn in handlers:  # commands.run_system_with(handler, destroyed) (core.rs:660-667)
                dead = d.destroyed(i)
                if len(dead):
                    fn(dead)
            if d.on_finished and d.poll_finished():  # ParticleSpawnerFinished observers (core.rs:674-688)
                for fn in d.on_finished:
                    fn(d)

    def track_aabbs(self, enable: bool = True) -> None:
        """AABB fused into the update (render.rs:677-703): every tile leaves the box of its survivors; `aabb()` folds
        those instead of re-reading the particles."""
        self._check(self._lib.fw_ctx_track_aabbs(self._ctx, 1 if enable else 0))

    # the boxes of MANY spawners in one call (include/firework_hip.h: BATCHED BOXES): what update_aabbs (render.rs:677-703) computes
    # for every spawner every frame.  `spawners`: SpawnerData objects or raw handles, in any order, duplicates allowed
    @staticmethod
    def _handle_array(spawners):
        n = len(spawners)
        return n, (C.c_int32 * max(n, 1))(*[int(getattr(d, "handle", d)) for d in spawners])

    def aabb_records(self, spawners) -> np.ndarray:
        """records[i] (settings.AABB_DTYPE) = the box of spawners[i], as `SpawnerData.aabb()` answers it.  One wait for the batch."""
        n, handles = self._handle_array(spawners)
        out = np.zeros(n, dtype=S.AABB_DTYPE)
        self._check(self._lib.fw_ctx_aabbs(self._ctx, n, handles, out.ctypes.data_as(C.c_void_p) if n else None))
        return out

    def aabbs(self, spawners):
        """(any[n] bool, min[n, 3], max[n, 3]) of the spawners' boxes"""
        r = self.aabb_records(spawners)
        return r["any"] != 0, r["min"].copy(), r["max"].copy()

    def aabbs_device(self, spawners, out_ptr: int) -> None:
        """the same records into DEVICE memory at out_ptr (n x 32 bytes, 16-byte aligned), enqueued on the context's stream: no wait"""
        n, handles = self._handle_array(spawners)
        self._check(self._lib.fw_ctx_aabbs_device(self._ctx, n, handles, C.c_void_p(out_ptr) if out_ptr else None))

    def debug_aabb_batch(self):
        """(launches the batched box calls have enqueued so far, chunks of the latest call, list positions per chunk)"""
        launches, chunks, size = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self._lib.fw_debug_aabb_batch(self._ctx, C.byref(launches), C.byref(chunks), C.byref(size)))
        return int(launches.value), int(chunks.value), int(size.value)

    # how many particles lie inside analytic volumes (include/firework_hip.h: VOLUME QUERIES).  `places`: a settings.VOLUME_PLACE_DTYPE
    # array, or a sequence whose items are a SpawnerData / raw handle (every particle type) or a (spawner, type) pair (type -1: every
    # type); any order, duplicates allowed.  `volumes`: settings.Collider objects of any kind; their layers are ignored
    @staticmethod
    def _place_array(places) -> np.ndarray:
        if isinstance(places, np.ndarray) and places.dtype == S.VOLUME_PLACE_DTYPE:
            return np.ascontiguousarray(places)
        out = np.zeros(len(places), dtype=S.VOLUME_PLACE_DTYPE)
        for k, p in enumerate(places):
            d, t = p if isinstance(p, (tuple, list)) else (p, -1)
            out[k] = (int(getattr(d, "handle", d)), int(t))
        return out

    def count_in_volumes(self, places, volumes) -> np.ndarray:
        """counts[p, v] (uint32) = the particles of places[p] whose position lies inside volumes[v].  One wait for the call."""
        pl = self._place_array(places)
        out = np.zeros((len(pl), len(volumes)), dtype=np.uint32)
        self._check(self._lib.fw_ctx_count_in_volumes(self._ctx, len(pl), pl.ctypes.data_as(C.c_void_p) if len(pl) else None, len(volumes),
                                                      _ffi.make_colliders(volumes) if len(volumes) else None, out.ctypes.data_as(C.c_void_p) if out.size else None))
        return out

    def count_in_volumes_device(self, places, volumes, out_ptr: int) -> None:
        """the same counts into DEVICE memory at out_ptr (n_places x n_volumes uint32, 4-byte aligned), enqueued on the context's stream:
        no wait"""
        pl = self._place_array(places)
        self._check(self._lib.fw_ctx_count_in_volumes_device(self._ctx, len(pl), pl.ctypes.data_as(C.c_void_p) if len(pl) else None, len(volumes),
                                                             _ffi.make_colliders(volumes) if len(volumes) else None, C.c_void_p(out_ptr) if out_ptr else None))

    def debug_volume_query(self):
        """(launches the volume queries have enqueued so far, chunks of the latest call, list positions per chunk, volumes per tile)"""
        launches, chunks, size, tile = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.fw_debug_volume_query(self._ctx, C.byref(launches), C.byref(chunks), C.byref(size), C.byref(tile)))
        return int(launches.value), int(chunks.value), int(size.value), int(tile.value)

    # -- statistics / measurement ----------------------------------------------------------------
    def live_count(self) -> int:
        out = C.c_uint64()
        self._check(self._lib.fw_ctx_live_count(self._ctx, C.byref(out)))
        return int(out.value)

    def live_count_device(self, device_ptr: int) -> None:
        self._check(self._lib.fw_ctx_live_count_device(self._ctx, C.c_void_p(device_ptr)))

    def live_count_ring(self, device_ptr: int, n_slots: int) -> None:
        """Every later step leaves its frame's total live count in ring[k % n_slots] (device uint64), no extra launch."""
        self._check(self._lib.fw_ctx_live_count_ring(self._ctx, C.c_void_p(device_ptr) if device_ptr else None, int(n_slots)))

    def updated_total(self) -> int:
        out = C.c_uint64()
        self._check(self._lib.fw_ctx_last_step_updated(self._ctx, C.byref(out)))
        return int(out.value)

    def kernel_timing(self, enable: bool) -> None:
        self._check(self._lib.fw_ctx_kernel_timing(self._ctx, 1 if enable else 0))

    def kernel_timing_read(self):
        ms, n, parts = C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.fw_ctx_kernel_timing_read(self._ctx, C.byref(ms), C.byref(n), C.byref(parts)))
        return ms.value, int(n.value), int(parts.value)

    def kernel_timing_overhead_us(self) -> float:
        out = C.c_double()
        self._check(self._lib.fw_ctx_kernel_timing_overhead(self._ctx, C.byref(out)))
        return out.value * 1e3

    def param_bar(self) -> bool:
        """per-frame records and small op tables live in device memory the host writes through the large BAR (else: pinned host memory)"""
        on = C.c_int32()
        if not hasattr(self._lib, "fw_debug_param_bar"):
            return False
        self._check(self._lib.fw_debug_param_bar(self._ctx, C.byref(on)))
        return bool(on.value)

    def tile_scratch(self):
        """(tiles of the compacting launch's table, entries every per-tile array of the context holds)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.fw_debug_tile_scratch(self._ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def tf_frames(self) -> int:
        """frames whose dt differed from the previous one's and that ran fw_k_fc_resolve + the streaming schedule (threshold forecast)"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_tf_frames(self._ctx, C.byref(n)))
        return int(n.value)

    def age_launches(self) -> int:
        """launches of fw_k_fifo_ages so far: a FIFO ring under the age rule had its ages written back for a reader"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_age_launches(self._ctx, C.byref(n)))
        return int(n.value)

    def spin_launches(self) -> int:
        """launches of fw_k_fifo_spin so far: a FIFO ring whose spin was deferred had its log of frames replayed for a reader"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_spin_launches(self._ctx, C.byref(n)))
        return int(n.value)

    def spinless_launches(self) -> int:
        """FIFO launches so far that ran the kernel form compiled for launches whose ring tiles touch neither rotation nor angular
        velocity (every ring cannot turn or has its spin deferred)"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_spinless_launches(self._ctx, C.byref(n)))
        return int(n.value)

    PATH_CENSUS_FIELDS = ("n_in_use", "n_fifo", "n_range", "n_few", "n_spilled", "n_small", "n_small_ok", "n_small_coll", "n_inst", "n_solo",
                          "few_blocked")

    def path_census(self):
        """(kept, recounted): the context's segments by update path as the host keeps the census and as a recount over its segment
        records gives it, each a dict over PATH_CENSUS_FIELDS; equal at all times (csrc/fw_update_path.h).  Host state only: nothing is
        synchronised or flushed"""
        kept, again = (C.c_uint32 * 11)(), (C.c_uint32 * 11)()
        self._check(self._lib.fw_debug_path_census(self._ctx, kept, again))
        return dict(zip(self.PATH_CENSUS_FIELDS, map(int, kept))), dict(zip(self.PATH_CENSUS_FIELDS, map(int, again)))

    def whole_tiles(self):
        """(launches, tiles): spin-less FIFO launches so far in which the host found a whole ring tile -- every slot a particle that lives
        through the launch -- and those tiles: they take the arm that issues all loads first"""
        launches, tiles = C.c_uint64(), C.c_uint64()
        self._check(self._lib.fw_debug_whole_tiles(self._ctx, C.byref(launches), C.byref(tiles)))
        return int(launches.value), int(tiles.value)

    def newborn_spin_launches(self) -> int:
        """FIFO launches so far whose spawning workgroups deferred the spin of the particles they spawned into a ring that defers its
        spin: the replay applies the frame's own log entry to them"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_newborn_spin(self._ctx, C.byref(n)))
        return int(n.value)

    def fuse2_launches(self):
        """(fused, flushed): FIFO launches so far that ran two frames of unread rings in one pass, and withheld frames that went to the
        stream alone"""
        fused, flushed = C.c_uint64(), C.c_uint64()
        self._check(self._lib.fw_debug_fuse2(self._ctx, C.byref(fused), C.byref(flushed)))
        return int(fused.value), int(flushed.value)

    def fuse_frames(self) -> int:
        """frames run by fused launches so far: a launch that ran D frames of unread rings in one pass counts D"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_fuse_frames(self._ctx, C.byref(n)))
        return int(n.value)

    def recovered_rings(self) -> int:
        """rings moved to the compacting path (particles kept) because a cohort report was missing when it was due"""
        n = C.c_uint64()
        self._check(self._lib.fw_debug_recovered_rings(self._ctx, C.byref(n)))
        return int(n.value)

    def nest_frames(self):
        """(frames whose Nested entries ran inside the FIFO ring launch, frames that ran the separate fw_k_spawn / fw_k_nest passes)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.fw_debug_nest_frames(self._ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def measure_copy_bandwidth(self, nbytes: int = 1 << 30, iters: int = 20) -> float:
        out = C.c_double()
        self._check(self._lib.fw_ctx_measure_copy_bandwidth(self._ctx, int(nbytes), int(iters), C.byref(out)))
        return out.value


def compute_emission_count(t, last, duration, start, end, count):
    """compute_emission_count (core.rs:553-575) as the library's host side evaluates it."""
    nxt = C.c_float()
    n = _ffi.load().fw_compute_emission_count(t, last, duration, start, end, count, C.byref(nxt))
    return int(n), np.float32(nxt.value)
