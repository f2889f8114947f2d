"""What the C entry points share since they were folded (csrc/fw_engine_query.cpp: query_device / query_staged and the four staging
buffers of both queries; csrc/fw_engine_api.cpp: begin_call, the one opener of the spawner entry points).  The suites of the entry
points themselves pin what each computes; this file pins what a shared path can get wrong: one query's staging seen by the other,
regrowth between them, the order null ctx -> n == 0 -> null pointer, and an opener that lets a bad handle or particle type through,
or that disturbs a healthy spawner on its way out.

That the device forms wait for nothing is pinned where it always was: test_queries_see_the_world_of_their_place_in_the_stream of
tests/test_gpu_ray_query.py and tests/test_gpu_point_query.py; the last test here enqueues all three device forms behind a step with
one synchronisation at the end, with no clock involved.  The autouse fw_path fixture runs every test on the FIFO ring, range ring,
compacting and small paths: the healthy spawner below is a type of each.  Needs an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capsule_ref  # noqa: E402
import mesh_ref  # noqa: E402
import project_ref  # noqa: E402
from capsule_rays import unit_quat  # noqa: E402
from test_gpu_capsule import _assert_hits  # noqa: E402
from test_gpu_point_query import _project_device, _records  # noqa: E402
from test_gpu_ray_query import _cast_device, _ctx_stream, _ray_records  # noqa: E402
from test_point_query_cpu import assert_projections_equal  # noqa: E402

from bevy_firework_amd import _ffi, workloads  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL, FW_OK  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL = 0xFFFFFFFF
SEED = 1717
DT = f32(1.0 / 60.0)
N = 4097  # one more than the first reservation of the staging buffers holds as rays (8192 float4 = 4096 records of two)


def _system():
    from bevy_firework_amd.system import ParticleSystem

    return ParticleSystem(device=0, seed=SEED)


# ---- 1. both queries through the same four buffers -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world():
    """one box, one capsule, one mesh instance of two triangles"""
    analytic = [S.Collider.Box((1.5, 0.0, 0.0), (0.5, 0.75, 1.0), unit_quat(0.3, 0.0, 0.1, 0.9)),
                S.Collider.Capsule((-1.5, 0.5, 0.5), 0.4, 2.0, unit_quat(0.6, 0.1, -0.3, 0.7))]
    quad_v = np.array([[-2.0, 0.0, -2.0], [2.0, 0.0, -2.0], [2.0, 0.3, 2.0], [-2.0, 0.0, 2.0]], dtype=f32)
    quad_t = np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)
    inst = mesh_ref.Instance(mesh_ref.Mesh(quad_v, quad_t), (0.0, -1.5, 0.0), unit_quat(0.1, 0.0, 0.05, 0.99), 1)
    return analytic, (quad_v, quad_t), inst


@functools.lru_cache(maxsize=None)
def _inputs_and_references():
    """N rays and N points about the world, and what the numpy statements answer: computed once, read-only"""
    analytic, _, inst = _world()
    rng = np.random.default_rng(SEED)
    src, dst = rng.uniform(-4.0, 4.0, (N, 3)), rng.uniform(-2.0, 2.0, (N, 3))
    ln = np.linalg.norm(dst - src, axis=1)
    o, d, md = src.astype(f32), ((dst - src) / ln[:, None]).astype(f32), (ln * rng.uniform(0.5, 1.5, N)).astype(f32)
    pts = rng.uniform(-4.0, 4.0, (N, 3)).astype(f32)
    pts[:N // 4] = (np.asarray(analytic[1].position) + rng.normal(size=(N // 4, 3)) * 0.5).astype(f32)  # (inside and about the capsule)
    hits = capsule_ref.cast_ray_identity(mesh_ref.World(analytic, [inst]), ALL, o, d, md)
    proj = project_ref.project_points(analytic, [inst], pts, ALL)
    rays, points = _ray_records(o, d, md, ALL), _records(pts, ALL)
    for a in hits + (proj, rays, points):
        a.setflags(write=False)
    return rays, hits, points, proj


def test_the_two_queries_share_their_staging(fw_path):
    """project_points n = 1, cast_rays n = 4096 (exactly the first reservation), cast_rays n = 4097 (regrowth), project_points n =
    4097, project_points n = 1: after each call the host form equals the device form bit for bit and both equal capsule_ref /
    mesh_ref (rays: found, distance, normal, kind, index) and project_ref (points: every field)"""
    analytic, (quad_v, quad_t), inst = _world()
    rays, hits, points, proj = _inputs_and_references()
    assert (hits[3] == S.HIT_COLLIDER).sum() > 300 and (hits[3] == S.HIT_MESH).sum() > 300 and (~hits[0]).sum() > 300
    assert all(((hits[3] == S.HIT_COLLIDER) & (hits[4] == i)).sum() > 100 for i in (0, 1))
    assert (proj["kind"] == S.HIT_MESH).sum() > 300 and (proj["is_inside"] != 0).sum() > 100
    with _system() as system:
        system.set_colliders(analytic)
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(quad_v, quad_t), inst.position, inst.rotation, inst.layers)])
        for what, n in (("points", 1), ("rays", 4096), ("rays", N), ("points", N), ("points", 1)):
            if what == "rays":
                host = system.cast_ray_records(rays[:n])
                assert host.tobytes() == _cast_device(system, rays[:n]).tobytes(), (what, n)
                _assert_hits(host, tuple(a[:n] for a in hits), f"{what}, n = {n}")
            else:
                host = system.project_point_records(points[:n])
                assert host.tobytes() == _project_device(system, points[:n]).tobytes(), (what, n)
                assert_projections_equal(host, proj[:n], f"{what}, n = {n}")


def test_query_argument_checks_keep_their_order_and_their_names(fw_path):
    """n == 0 with null pointers is FW_OK for all four entry points; a null pointer with n > 0 is FW_EINVAL and fw_last_error names the
    entry point that was called"""
    import torch

    with _system() as system:
        L, ctx = system._lib, system._ctx
        host = np.zeros(64, dtype=np.uint8).ctypes.data_as(C.c_void_p)
        with _ctx_stream(system):
            dev = C.c_void_p(torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr())
        for name, buf in (("fw_ctx_cast_rays", host), ("fw_ctx_cast_rays_device", dev), ("fw_ctx_project_points", host),
                          ("fw_ctx_project_points_device", dev)):
            fn = getattr(L, name)
            assert fn(ctx, None, 0, None) == FW_OK, name
            assert fn(None, buf, 1, buf) == FW_EINVAL, name
            for a, b in ((None, buf), (buf, None), (None, None)):
                assert fn(ctx, a, 1, b) == FW_EINVAL, name
                assert L.fw_last_error(ctx).decode() == f"{name}: null pointer"
        system.synchronize()


# ---- 2. the opener of the spawner entry points ------------------------------------------------------------------------------------------
def _spawner():
    """256 particles on demand: the stress test's type (drag, a gradient, a cone of velocities), alive for all three steps"""
    sp, tf = workloads.stress_test()
    sp.emission_settings[0].emission_pacing = S.EmissionPacing.OnDemand()
    return sp, tf


def _f(*v):
    return (C.c_float * len(v))(*v)


def _entry_points():
    """every spawner entry point of _ffi.SYMBOLS -> (takes a particle type, call(L, ctx, handle, type, env)); every argument but the
    handle and the type is one the entry point accepts"""
    n, i32, u32 = C.c_uint64(), C.c_int32(), C.c_uint32()
    return {
        "fw_spawner_update_settings": (False, lambda L, c, h, t, e: L.fw_spawner_update_settings(c, h, C.byref(e["desc"]))),
        "fw_spawner_destroy": (False, lambda L, c, h, t, e: L.fw_spawner_destroy(c, h)),
        "fw_spawner_set_origin": (False, lambda L, c, h, t, e: L.fw_spawner_set_origin(c, h, _f(1, 2, 3), _f(0, 0, 0, 1))),
        "fw_spawner_set_parent_velocity": (False, lambda L, c, h, t, e: L.fw_spawner_set_parent_velocity(c, h, _f(1, 2, 3))),
        "fw_spawner_set_modifier": (False, lambda L, c, h, t, e: L.fw_spawner_set_modifier(c, h, 2.0, 3.0)),
        "fw_spawner_queue": (False, lambda L, c, h, t, e: L.fw_spawner_queue(c, h, 100)),
        "fw_spawner_counts": (False, lambda L, c, h, t, e: L.fw_spawner_counts(c, h, C.byref(u32), 1)),
        "fw_spawner_active": (False, lambda L, c, h, t, e: L.fw_spawner_active(c, h, C.byref(i32))),
        "fw_spawner_poll_finished": (False, lambda L, c, h, t, e: L.fw_spawner_poll_finished(c, h, C.byref(i32))),
        "fw_spawner_read_particles": (True, lambda L, c, h, t, e: L.fw_spawner_read_particles(c, h, t, None, 0, C.byref(n))),
        "fw_spawner_read_last_emitted": (True, lambda L, c, h, t, e: L.fw_spawner_read_last_emitted(c, h, t, 0, None, 0, C.byref(n))),
        "fw_spawner_write_particles": (True, lambda L, c, h, t, e: L.fw_spawner_write_particles(c, h, t, None, 0)),
        "fw_spawner_write_last_emitted": (True, lambda L, c, h, t, e: L.fw_spawner_write_last_emitted(c, h, t, 0, None, 0)),
        "fw_spawner_read_destroyed": (True, lambda L, c, h, t, e: L.fw_spawner_read_destroyed(c, h, t, None, 0, C.byref(n))),
        "fw_spawner_pack_instances": (True, lambda L, c, h, t, e: L.fw_spawner_pack_instances(c, h, t, None, 0, C.byref(n))),
        "fw_spawner_pack_instances_device": (True, lambda L, c, h, t, e: L.fw_spawner_pack_instances_device(c, h, t, e["d_out"], 256, C.byref(n))),
        "fw_spawner_attach_instances": (True, lambda L, c, h, t, e: L.fw_spawner_attach_instances(c, h, t, e["d_out"], 256)),
        "fw_spawner_attach_instances_window": (True, lambda L, c, h, t, e: L.fw_spawner_attach_instances_window(c, h, t, e["d_out"], 256)),
        "fw_spawner_instance_window": (True, lambda L, c, h, t, e: L.fw_spawner_instance_window(c, h, t, C.byref(n), C.byref(n))),
        "fw_spawner_aabb": (False, lambda L, c, h, t, e: L.fw_spawner_aabb(c, h, _f(0, 0, 0), _f(0, 0, 0), C.byref(i32))),
        "fw_debug_update_path": (True, lambda L, c, h, t, e: L.fw_debug_update_path(c, h, t, C.byref(i32), None, None)),
    }


ENTRY_POINTS = sorted(_entry_points())


def test_the_table_holds_every_spawner_entry_point_of_the_binding(fw_path):
    bound = {name for name, _, _ in _ffi.SYMBOLS if name.startswith("fw_spawner_") or name == "fw_debug_update_path"}
    assert bound - {"fw_spawner_create"} == set(ENTRY_POINTS)


def _three_steps(bad_call=None):
    """a context with a destroyed spawner (handle 0) and a healthy one of 256 particles (handle 1): [(its count, the context's, its
    particles)] after each of three steps; bad_call(system, victim handle, healthy handle, a device buffer) runs in front of every step"""
    import torch

    sp, tf = _spawner()
    frames = []
    with _system() as system:
        victim = system.spawn(sp, tf, uid=0)
        healthy = system.spawn(sp, tf, uid=1)
        system.despawn(victim)
        healthy.queue_particles(256)
        with _ctx_stream(system):
            d_out = torch.zeros((256, 64), dtype=torch.uint8, device="cuda")
        system.synchronize()
        for _ in range(3):
            if bad_call is not None:
                bad_call(system, victim.handle, healthy.handle, C.c_void_p(d_out.data_ptr()))
            system.update(DT)
            frames.append((healthy.count(0), system.live_count(), healthy.particles(0).tobytes()))
        assert not d_out.cpu().numpy().any(), "a refused call wrote to the caller's buffer"
    return frames


@functools.lru_cache(maxsize=None)
def _undisturbed(path):
    """(per path: the fixture's knobs are read when a context is created, and they follow the path and the test function's name)"""
    frames = _three_steps()
    assert [f[:2] for f in frames] == [(256, 256)] * 3 and len({f[2] for f in frames}) == 3
    return tuple(frames)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_bad_handles_and_types_are_refused_and_disturb_nobody(fw_path, name):
    """a handle that was never created (past the array, negative), a destroyed handle, and -- where the entry point takes one -- a
    particle type equal to the type count of a healthy spawner: FW_EINVAL each; the healthy spawner's live count and particles after
    each of three steps equal, bit for bit, those of an identical context that received none of these calls"""
    typed, call = _entry_points()[name]
    desc, keep = _ffi.make_desc(_spawner()[0], 1)

    def bad_call(system, victim, healthy, d_out):
        L, ctx = system._lib, system._ctx
        env = {"desc": desc, "d_out": d_out}
        for h in (7, -1, victim):
            assert call(L, ctx, h, 0, env) == FW_EINVAL, (name, h)
        if typed:
            assert call(L, ctx, healthy, 1, env) == FW_EINVAL, (name, "type == type count")

    assert tuple(_three_steps(bad_call)) == _undisturbed(fw_path), name


# ---- 3. the device forms behind a step, nothing waited for --------------------------------------------------------------------------------
def test_device_forms_enqueued_behind_a_step_answer_as_the_host_forms_do(fw_path):
    """a step, then fw_spawner_pack_instances_device and both _device queries with no wait in between and one synchronisation at the end:
    each result is its host form's"""
    import torch

    analytic, (quad_v, quad_t), inst = _world()
    rays, _, points, _ = _inputs_and_references()
    rays, points = rays[:1000], points[:1000]
    sp, tf = _spawner()
    with _system() as system:
        system.set_colliders(analytic)
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(quad_v, quad_t), inst.position, inst.rotation, inst.layers)])
        h = system.spawn(sp, tf, uid=1)
        h.queue_particles(256)
        with _ctx_stream(system):
            d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32).copy()).to("cuda")
            d_points = torch.from_numpy(points.view(np.uint8).reshape(-1, 16).copy()).to("cuda")
            d_hits, d_proj = (torch.zeros((1000, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
            d_inst = torch.zeros((256, 64), dtype=torch.uint8, device="cuda")
        system.update(DT)
        ub = C.c_uint64()
        system._check(system._lib.fw_spawner_pack_instances_device(system._ctx, h.handle, 0, C.c_void_p(d_inst.data_ptr()), 256, C.byref(ub)))
        system.cast_rays_device(d_rays.data_ptr(), 1000, d_hits.data_ptr())
        system.project_points_device(d_points.data_ptr(), 1000, d_proj.data_ptr())
        system.synchronize()
        assert ub.value == 256
        assert d_inst.cpu().numpy().tobytes() == h.instances(0).tobytes() and d_inst.cpu().numpy().any()
        assert d_hits.cpu().numpy().tobytes() == system.cast_ray_records(rays).tobytes()
        assert d_proj.cpu().numpy().tobytes() == system.project_point_records(points).tobytes()
