"""The path query on the device (include/firework_hip.h: PATH QUERIES; fw_ctx_trace_paths / fw_ctx_trace_paths_device): a batch of
hypothetical particles through n_steps frames in the device-resident collider world.  Every field must equal, bit for bit,
tests/trace_ref.py -- the header's text composed from golden/np_sim.py, capsule_ref and mesh_ref -- for the world and the paths of
tests/test_path_query_cpu.py (which runs the same code on the host), and must equal what the simulation itself does to particles
written at the paths' states, on every update path of the suite's matrix (the autouse fw_path fixture).  Device buffers are torch
tensors.  Needs an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_points as P  # noqa: E402
import test_path_query_cpu as T  # noqa: E402
from test_gpu_mesh import _falling_spawner, _particles, _terrain  # noqa: E402
from test_gpu_mesh_deform import deform  # noqa: E402
from test_gpu_point_query import _open  # noqa: E402
from test_gpu_ray_query import SENTINEL, _ctx_stream, _read, _system  # noqa: E402

from bevy_firework_amd import _ffi  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL, FW_OK  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = 0xFFFFFFFF
N_PATHS = 1000


def _to_device(system, records):
    import torch

    host = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, 32).copy())
    with _ctx_stream(system):
        return host.to("cuda")


def _buffer(system, n_records, size):
    import torch

    with _ctx_stream(system):
        return torch.full((n_records, size), SENTINEL, dtype=torch.uint8, device="cuda")


def _trace_device(system, settings, records, n=None, samples=True):
    """-> (results, samples or None); one sentinel record behind the results and one behind the samples must survive"""
    n = len(records) if n is None else n
    d_paths, d_out = _to_device(system, records), _buffer(system, n + 1, 80)
    d_smp = _buffer(system, settings.n_steps * n + 1, 16) if samples else None
    system.trace_paths_device(settings, d_paths.data_ptr(), n, d_out.data_ptr(), d_smp.data_ptr() if samples else 0)
    raw = _read(system, d_out)
    assert (raw[n:] == SENTINEL).all(), "the record behind the last result was written"
    out = raw[:n].reshape(-1).view(S.PATH_RESULT_DTYPE).copy()
    if not samples:
        return out, None
    raw = _read(system, d_smp)
    assert (raw[settings.n_steps * n:] == SENTINEL).all(), "the record behind the last sample was written"
    return out, raw[:settings.n_steps * n].reshape(-1).view(f32).reshape(settings.n_steps, n, 4).copy()


def _worlds():
    w = T.random_world()
    return {"analytic": P.World(w.colliders), "meshes": P.World([], w.meshes, w.placements), "mixed": w}


def _settings(n_steps, destroy=False, mask=0xFFFFFFFF):
    return S.PathSettings(1.0 / 60.0, n_steps, T.GRAVITY, 0.3, S.ParticleCollisionSettings(0.6, 0.2, destroy, mask))  # (T.random_settings' values)


@functools.lru_cache(maxsize=None)
def _reference(name, n_steps, destroy=False):
    out = T.reference(_worlds()[name], _settings(n_steps, destroy), T.random_paths(N_PATHS), samples=True)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. bit-exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [0, 1, 4, 37])
def test_paths_are_bit_exact(n_steps):
    """1000 paths (a third falling onto the meshes, some starting inside solids, lifetimes around the 37 steps) through the analytic
    colliders alone (the kernel without the mesh loop), the meshes alone and both, for 0, 1, 4 and 37 steps: every field of every
    result and every sample equals the reference"""
    paths = T.random_paths(N_PATHS)
    for name, w in _worlds().items():
        with _system() as system:
            _open(system, w)
            got, smp = _trace_device(system, _settings(n_steps), paths)
        want, want_s = _reference(name, n_steps)
        T.assert_results_equal(got, want, f"{name}, {n_steps} steps")
        T.assert_samples_equal(smp, want_s, f"{name}, {n_steps} steps")
        if n_steps == 0:
            assert got["position"].tobytes() == paths["position"].tobytes() and got["age"].tobytes() == paths["age"].tobytes()
            assert not got["status"].any() and not got["steps"].any() and (got["contact_step"] == NONE).all() and (got["index"] == NONE).all()
        if n_steps == 37:
            assert (got["n_contacts"] >= 2).sum() > 30 and (got["status"] == S.PATH_EXPIRED).sum() > 100 and (got["status"] == S.PATH_RUNNING).sum() > 100
            if name != "analytic":
                assert (got["kind"] == S.HIT_MESH).sum() > 100
    if n_steps == 37:
        with _system() as system:
            _open(system, _worlds()["mixed"])
            got, smp = _trace_device(system, _settings(37, True), paths)
        want, want_s = _reference("mixed", 37, True)
        T.assert_results_equal(got, want, "destroy_on_collision")
        T.assert_samples_equal(smp, want_s, "destroy_on_collision")
        assert (got["status"] == S.PATH_DESTROYED).sum() > 100


def test_engineered_cases_on_the_device():
    with _system() as system:
        for name, world, settings, paths, _ in T.engineered():
            system.set_colliders(world.colliders)
            got, smp = _trace_device(system, settings, paths)
            want, want_s = T.reference(world, settings, paths, samples=True)
            T.assert_results_equal(got, want, name)
            T.assert_samples_equal(smp, want_s, name)


# ---- 2. launch sizes ---------------------------------------------------------------------------------------------------------------
def test_sizes_around_the_wave_and_the_workgroup():
    """n in {1, 63, 64, 65, 255, 256, 257, 1000}, each a prefix of the same paths: the prefix of the large batch's results and of every
    row of its samples ([step][n]: the stride follows n), the records behind both untouched; n = 0 touches nothing"""
    paths = T.random_paths(N_PATHS)
    settings = _settings(37)
    want, want_s = _reference("mixed", 37)
    with _system() as system:
        _open(system, _worlds()["mixed"])
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            got, smp = _trace_device(system, settings, paths, n)  # (paths beyond n are there to be loaded by a kernel that gets n wrong)
            T.assert_results_equal(got, want[:n], f"n = {n}")
            T.assert_samples_equal(smp, want_s[:, :n], f"n = {n}")
        d_paths, d_out, d_smp = _to_device(system, paths[:64]), _buffer(system, 64, 80), _buffer(system, 64 * 37, 16)
        system.trace_paths_device(settings, d_paths.data_ptr(), 0, d_out.data_ptr(), d_smp.data_ptr())
        assert (_read(system, d_out) == SENTINEL).all() and (_read(system, d_smp) == SENTINEL).all()
        assert len(system.trace_path_records(settings, paths[:0])) == 0


# ---- 3. lanes that end apart -------------------------------------------------------------------------------------------------------
def _apart():
    """256 paths over a ground plane.  Wave 0: 64 lifetimes that expire in 64 different steps, dealt out so that neighbours end far
    apart; the 16 that end first sit inside or just above a ball 100 units away that nobody else comes near -- once they have ended
    no running lane of the wave can reach it.  Waves 1-3: lanes that bounce on the ground, lanes high above it that meet nothing, and
    more early enders next to them."""
    rng = np.random.default_rng(23)
    n, n_steps = 256, 70
    end = np.concatenate([rng.permutation(64), rng.integers(0, 90, n - 64)])  # the step each path expires in (>= 70: it does not)
    pos = np.stack([rng.uniform(-3, 3, n), rng.uniform(0.02, 0.6, n), rng.uniform(-3, 3, n)], axis=1)
    vel = rng.normal(0.0, 1.5, (n, 3))
    high = np.arange(n) % 3 == 2
    pos[high, 1] += 40.0
    early = np.flatnonzero(end[:64] < 16)
    pos[early] = np.array([100.0, 1.0, 0.0]) + rng.uniform(-0.3, 0.3, (len(early), 3))
    world = P.World([S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), S.Collider.Sphere((100.0, 1.0, 0.0), 0.5), S.Collider.Box((0.0, 0.0, 0.0), (9.0, 9.0, 9.0), P.ID, 2)])
    paths = T.path_records(pos, vel, 0.0, ((end + 1) * T.DT).astype(f32))
    return world, S.PathSettings(T.DT, n_steps, T.GRAVITY, 0.0, S.ParticleCollisionSettings(0.5, 0.25, False, 1)), paths, end


def test_lanes_that_end_in_different_steps():
    world, settings, paths, end = _apart()
    want, want_s = T.reference(world, settings, paths, samples=True)
    # (from the reference alone: the wave's 64 lanes end in 64 different steps; the early ones met the ball, nobody else did; the
    # other waves hold bouncing lanes and lanes that met nothing)
    assert sorted(want["steps"][:64].tolist()) == list(range(64)) and (want["status"][:64] == S.PATH_EXPIRED).all()
    ball = (want["kind"] == S.HIT_COLLIDER) & (want["index"] == 1)
    assert ball[:64].sum() >= 8 and (end[:64][ball[:64]] < 16).all() and not ball[64:].any()
    assert (want["n_contacts"][64:] >= 2).sum() > 30 and (want["n_contacts"][64:] == 0).sum() > 30 and (want["status"][64:] == S.PATH_RUNNING).sum() > 20
    with _system() as system:
        system.set_colliders(world.colliders)
        for samples in (True, False):
            got, smp = _trace_device(system, settings, paths, samples=samples)
            T.assert_results_equal(got, want, f"ending apart, samples {samples}")
            if samples:
                T.assert_samples_equal(smp, want_s, "ending apart")
        # a mask that sees nothing: the same lanes, no contact anywhere, everybody falls through the ground
        settings = S.PathSettings(settings.dt, settings.n_steps, T.GRAVITY, 0.0, S.ParticleCollisionSettings(0.5, 0.25, False, 4))
        got, _ = _trace_device(system, settings, paths, samples=False)
        T.assert_results_equal(got, T.reference(world, settings, paths), "a mask that sees nothing")
        assert not got["n_contacts"].any() and (got["kind"] == S.HIT_NONE).all() and (got["position"][got["status"] == S.PATH_RUNNING][:, 1] < 0).any()


# ---- 4. against the simulation itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("destroy", [False, True])
def test_paths_are_what_the_simulation_does(fw_path, destroy):
    """the paths' states written as particles of a type with the same settings (report_destroyed on, no emission), 37 frames: after
    1, 4 and 37 frames the survivors are, in order, the paths still RUNNING after as many steps -- position, velocity, age bit for
    bit -- and every frame's destroyed records are the paths that ended in that step"""
    n = 600
    paths = T.random_paths(N_PATHS)[:n]
    settings = _settings(37, destroy)
    ps = S.ParticleSettings(lifetime=S.RandF32(0.2, 1.5), acceleration=settings.acceleration, linear_drag=settings.linear_drag, angular_drag=0.0, capacity=1024,
                            collision_settings=settings.collision_settings)
    ps.particles_destroyed = lambda dead: None
    spawner = S.ParticleSpawner([ps], [S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand())])
    parts = _particles(paths["position"], paths["velocity"])
    parts["age"], parts["lifetime"] = paths["age"], paths["lifetime"]
    with _system() as system:
        _open(system, _worlds()["mixed"])
        traced = {k: _trace_device(system, _settings(k, destroy), paths, samples=False)[0] for k in (1, 4, 37)}
        final = traced[37]
        h = system.spawn(spawner, uid=5)
        h.write_particles(0, parts)
        for frame in range(37):
            system.update(settings.dt)
            dead = h.destroyed(0)
            ended = np.flatnonzero((final["status"] != S.PATH_RUNNING) & (final["steps"] == frame))
            assert len(dead) == len(ended), (frame, len(dead), len(ended))
            for k in ("position", "velocity", "age"):
                assert dead[k].tobytes() == final[k][ended].tobytes(), (frame, k)
            assert dead["lifetime"].tobytes() == paths["lifetime"][ended].tobytes(), frame
            if frame + 1 in traced:
                alive, want = h.particles(0), traced[frame + 1]
                run = want["status"] == S.PATH_RUNNING
                assert len(alive) == run.sum() and (want["steps"][run] == frame + 1).all(), frame
                for k in ("position", "velocity", "age"):
                    assert alive[k].tobytes() == want[k][run].tobytes(), (frame, k)
    assert (final["status"] == S.PATH_EXPIRED).sum() > 50 and (final["n_contacts"] > 0).sum() > 100
    assert ((final["status"] == S.PATH_DESTROYED).sum() > 50) == destroy


# ---- 5. stream order ---------------------------------------------------------------------------------------------------------------
def test_traces_see_the_world_of_their_place_in_the_stream():
    """device form, nothing waited for in between: a trace, both sets replaced, a trace, a device-form vertex update, a trace; one
    synchronisation at the end.  Each result is the reference's over the world of its moment"""
    import torch

    mixed = P.mixed_world()
    gv, gt, _ = mixed.meshes[0]
    gv2 = deform(gv)
    a = P.World(mixed.colliders, [(gv, gt, True), mixed.meshes[1]], mixed.placements[:2])
    b_colliders = [S.Collider.Sphere((2.0, -1.0, 1.0), 1.5), S.Collider.Capsule((-3.0, 0.0, -2.0), 0.5, 2.0, P.TILT)]
    b_place = [(1, (-1.0, 0.5, 1.0), P.ID, 1), (0, (0.0, -1.5, 0.5), P.unit_quat(0.0, 0.2, 0.05, 0.97), 3), (0, (0.0, -2.0, 0.0), P.ID, 1)]
    b = P.World(b_colliders, a.meshes, b_place)
    c = P.World(b_colliders, [(gv2, gt, True), mixed.meshes[1]], b_place)
    paths = T.random_paths(N_PATHS)[:400]
    settings = _settings(12)
    with _system() as system:
        grid, ball = _open(system, a)
        d_paths = _to_device(system, paths)
        out = [_buffer(system, len(paths), 80) for _ in range(3)]
        with _ctx_stream(system):
            d_v2 = torch.from_numpy(gv2.copy()).to("cuda")
        system.trace_paths_device(settings, d_paths.data_ptr(), len(paths), out[0].data_ptr())
        system.set_colliders(b.colliders)
        system.set_mesh_colliders([S.MeshCollider((grid, ball)[k], p, q, layers) for k, p, q, layers in b_place])
        system.trace_paths_device(settings, d_paths.data_ptr(), len(paths), out[1].data_ptr())
        system.update_mesh_vertices_device(grid, d_v2.data_ptr(), len(gv2))
        system.trace_paths_device(settings, d_paths.data_ptr(), len(paths), out[2].data_ptr())
        system.synchronize()
        got = [t.cpu().numpy().reshape(-1).view(S.PATH_RESULT_DTYPE).copy() for t in out]
        assert system.mesh_update_status(grid) == (1, 0, -1)
    for k, w in enumerate((a, b, c)):
        T.assert_results_equal(got[k], T.reference(w, settings, paths), f"trace {k}")
        assert (got[k]["kind"] == S.HIT_MESH).sum() > 20
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


# ---- 6. the two forms, errors ------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_errors_enqueue_nothing():
    from bevy_firework_amd.system import FwError

    paths = T.random_paths(N_PATHS)
    settings = _settings(37)
    want, want_s = _reference("mixed", 37)
    with _system() as system:
        _open(system, _worlds()["mixed"])
        dev, dev_s = _trace_device(system, settings, paths)
        host, host_s = system.trace_path_records(settings, paths, samples=True)
        assert host.tobytes() == dev.tobytes() and host_s.tobytes() == dev_s.tobytes()
        T.assert_results_equal(host, want, "host form")
        assert system.trace_path_records(settings, paths).tobytes() == host.tobytes()  # (without samples)
        assert _trace_device(system, settings, paths, samples=False)[0].tobytes() == host.tobytes()
        by_fields = system.trace_paths(settings, paths["position"], paths["velocity"], paths["age"], paths["lifetime"])
        assert by_fields.tobytes() == host.tobytes()
        # (the host forms of the three queries share their staging: a point query in between changes nothing)
        assert len(system.project_points(paths["position"][:100], 1)) == 100
        assert system.trace_path_records(settings, paths[:300], samples=True)[1].tobytes() == np.ascontiguousarray(host_s[:, :300]).tobytes()
        # errors: each FW_EINVAL, nothing enqueued -- the sentinels survive
        d_paths, d_out, d_smp = _to_device(system, paths[:256]), _buffer(system, 256, 80), _buffer(system, 256 * 37, 16)
        bad = [_settings(S.PATH_MAX_STEPS + 1)] + [S.PathSettings(dt, 37, T.GRAVITY, 0.3, T.BOUNCE) for dt in (float("nan"), float("inf"), float("-inf"))]
        for s in bad:
            with pytest.raises(FwError) as e:
                system.trace_paths_device(s, d_paths.data_ptr(), 256, d_out.data_ptr(), d_smp.data_ptr())
            assert e.value.status == FW_EINVAL
            with pytest.raises(FwError) as e:
                system.trace_path_records(s, paths[:256])
            assert e.value.status == FW_EINVAL
        for pp, op in ((0, d_out.data_ptr()), (d_paths.data_ptr(), 0), (0, 0)):
            with pytest.raises(FwError) as e:
                system.trace_paths_device(settings, pp, 256, op, d_smp.data_ptr())
            assert e.value.status == FW_EINVAL
        L, ctx, cs = system._lib, system._ctx, _ffi.make_path_settings(settings)
        vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        assert L.fw_ctx_trace_paths_device(ctx, None, vp(d_paths), 256, vp(d_out), vp(d_smp)) == FW_EINVAL
        out = np.full(256, SENTINEL, dtype=np.uint8).repeat(80).view(S.PATH_RESULT_DTYPE)
        recs = np.ascontiguousarray(paths[:256])
        assert L.fw_ctx_trace_paths(ctx, None, recs.ctypes.data_as(C.c_void_p), 256, out.ctypes.data_as(C.c_void_p), None) == FW_EINVAL
        assert L.fw_ctx_trace_paths(ctx, C.byref(cs), None, 256, out.ctypes.data_as(C.c_void_p), None) == FW_EINVAL
        assert L.fw_ctx_trace_paths(ctx, C.byref(cs), recs.ctypes.data_as(C.c_void_p), 256, None, None) == FW_EINVAL
        assert (out.view(np.uint8) == SENTINEL).all()
        system.synchronize()
        assert (_read(system, d_out) == SENTINEL).all() and (_read(system, d_smp) == SENTINEL).all()
        assert L.fw_ctx_trace_paths(ctx, C.byref(cs), None, 0, None, None) == FW_OK and L.fw_ctx_trace_paths_device(ctx, C.byref(cs), None, 0, None, None) == FW_OK
        # the cap itself is allowed
        top = system.trace_path_records(_settings(S.PATH_MAX_STEPS), paths[:64])
        ended = host[:64]["status"] != S.PATH_RUNNING
        assert (top["status"] != S.PATH_RUNNING).all() and ended.sum() > 10 and top[ended].tobytes() == host[:64][ended].tobytes()
        assert system.trace_path_records(settings, paths[:500]).tobytes() == host[:500].tobytes()


# ---- 7. the simulation does not notice ---------------------------------------------------------------------------------------------
def _falling_frames(with_traces):
    v, t = _terrain()
    spawner, _ = _falling_spawner(True)
    tf = S.Transform((0.5, 0.2, -0.3))
    paths = T.random_paths(N_PATHS)
    settings = _settings(20)
    dt = f32(1.0 / 60.0)
    with _system() as system:
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)])
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(v, t))])
        d_paths, d_out, d_smp = _to_device(system, paths), _buffer(system, len(paths), 80), _buffer(system, len(paths) * 20, 16)
        dead = []
        for fr in range(40):
            system.update(dt)
            dead.append(h.destroyed(0))
            if with_traces:
                system.trace_paths_device(settings, d_paths.data_ptr(), len(paths), d_out.data_ptr(), d_smp.data_ptr() if fr % 2 else 0)
                if fr % 4 == 0:
                    r = system.trace_path_records(settings, paths, samples=fr % 8 == 0)
                    assert ((r[0] if fr % 8 == 0 else r)["n_contacts"] > 0).any()
        return h.particles(0), np.concatenate(dead)


def test_the_simulation_does_not_notice_path_queries(fw_path):
    """a colliding spawner over a mesh world, 40 frames with traces of both forms between the frames and 40 without: particles and
    destroyed records identical, bit for bit"""
    p0, d0 = _falling_frames(False)
    p1, d1 = _falling_frames(True)
    assert len(p0) > 300 and len(d0) > 100, (len(p0), len(d0))
    assert p0.tobytes() == p1.tobytes() and d0.tobytes() == d1.tobytes()
