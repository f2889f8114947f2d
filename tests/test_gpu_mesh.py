"""Triangle-mesh colliders (include/firework_hip.h: fw_mesh_collider) against the brute-force numpy reference
(tests/mesh_ref.py: every triangle of every instance, no hierarchy) -- so the device's hierarchy walk must cull
conservatively as well as compute bit for bit.  The autouse fw_path fixture runs every test on the FIFO ring, range ring,
compacting and small paths.  Needs an MI355X."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402
from mesh_rays import ray_world as _ray_world, rays as _rays, unit_quat as _unit_quat  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 1234
MB = 1 << 20


def _still_settings(destroy=False, capacity=0, report=False):
    """a type that moves only by its velocity: no acceleration, no drag, no spin -- position and velocity after a step are
    particle_collision's alone"""
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(100.0), acceleration=(0.0, 0.0, 0.0), linear_drag=0.0, angular_drag=0.0,
                            capacity=capacity,
                            collision_settings=S.ParticleCollisionSettings(0.6, 0.3, destroy, 0xFFFFFFFF))
    if report:
        ps.particles_destroyed = lambda dead: None
    return S.ParticleSpawner([ps], [S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand())])


def _particles(pos, vel):
    p = np.zeros(len(pos), dtype=S.PARTICLE_DTYPE)
    p["position"], p["velocity"] = pos, vel
    p["rotation"][:, 3] = 1.0
    p["initial_scale"] = p["scale"] = 1.0
    p["age"], p["lifetime"] = 0.0, 100.0
    p["base_color"] = p["emissive_color"] = 1.0
    return p


def _np_state(p, n_em=1):
    d = {k: np.ascontiguousarray(p[k]).astype(f32) for k in np_sim.FIELDS}
    d["last_emitted_age"] = np.full((len(p), n_em), np_sim.F32_MIN, dtype=f32)
    return d


def _device_world(system, meshes, placements):
    handles = {name: system.create_mesh(v, t) for name, (v, t) in meshes.items()}
    system.set_mesh_colliders([S.MeshCollider(handles[n], p, q, layers) for n, p, q, layers in placements])
    return handles


def _ref_world(meshes, placements, analytic):
    ms = {name: mesh_ref.Mesh(v, t) for name, (v, t) in meshes.items()}
    return mesh_ref.World(list(analytic), [mesh_ref.Instance(ms[n], p, q, layers) for n, p, q, layers in placements])


def _assert_same(got, want, what):
    for k in ("position", "velocity"):
        g, w = got[k], want[k]
        bad = ~((g == w) | (np.isnan(g) & np.isnan(w))).all(axis=1)
        assert not bad.any(), (what, k, int(bad.sum()), np.flatnonzero(bad)[:5], g[bad][:3], w[bad][:3])


def test_mesh_ray_casts_are_bit_exact(monkeypatch, fw_path):
    """50k+ particles, one step: every position and velocity equals the brute-force reference's bit for bit (the filter
    mask 0b101 leaves out the instance of layer 2)"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    meshes, placements, analytic = _ray_world()
    pos, vel, dt = _rays(meshes, placements, n_random=22000)
    assert len(pos) >= 50000
    spawner = _still_settings(capacity=1 << 17)
    spawner.particle_settings[0].collision_settings = S.ParticleCollisionSettings(0.6, 0.3, False, 0b101)
    parts = _particles(pos, vel)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        system.set_colliders(analytic)
        _device_world(system, meshes, placements)
        h.write_particles(0, parts)
        system.update(dt)
        got = h.particles(0)
    ref = np_sim.Spawner(spawner, SEED, 1)
    ref.colliders = _ref_world(meshes, placements, analytic)
    ref.particles[0] = _np_state(parts)
    ref.update(dt)
    want = ref.particles[0]
    assert len(got) == len(want["age"]) == len(pos)
    moved = (want["velocity"] != vel).any(axis=1)
    assert moved.sum() > 5000, int(moved.sum())  # (plenty of bounces)
    _assert_same(got, want, "one step")


def _terrain(cells=12, extent=6.0):
    return mesh_ref.grid_mesh(cells, cells, extent=extent, height=lambda x, z: 0.4 * np.sin(0.8 * x) * np.cos(0.6 * z) - 0.2)


def _falling_spawner(destroy):
    d = np.array([0.3, 1.0, 0.2])
    d = tuple(float(x) for x in (d / np.linalg.norm(d)).astype(f32))
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(1.5), initial_scale=S.RandF32.constant(0.05), linear_drag=0.1,
                            collision_settings=S.ParticleCollisionSettings(0.6, 0.2, destroy, 0xFFFFFFFF))
    ps.particles_destroyed = lambda dead: None  # report_destroyed: the destroyed records are compared too
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(2000.0), emission_shape=S.EmissionShape.Point(),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), d, 0.0), inherit_parent_velocity=False)
    return S.ParticleSpawner([ps], [es]), S.Transform((0.5, 1.5, -0.3))


@pytest.mark.parametrize("destroy, moving", [(False, False), (True, False), (False, True)])
def test_mesh_trajectories_are_bit_exact(monkeypatch, fw_path, destroy, moving):
    """a trig-free spawner falls onto a terrain mesh for 120 frames (bouncing, or destroyed on contact with the records
    compared); the moving variant replaces the instance set every frame without a synchronisation"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = _terrain()
    spawner, tf = _falling_spawner(destroy)
    dt = f32(1.0 / 60.0)
    ball = S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)
    ref = np_sim.Spawner(spawner, SEED, 3, tf)
    mesh = mesh_ref.Mesh(v, t)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([ball])
        terrain = system.create_mesh(v, t)
        hits = 0
        for fr in range(120):
            if moving or fr == 0:
                p = (f32(0.01 * (fr % 17)), f32(-0.005 * (fr % 5)), f32(0.0))
                q = _unit_quat(0.0, 0.02 * (fr % 3), 0.0, 1.0) if moving else (0.0, 0.0, 0.0, 1.0)
                system.set_mesh_colliders([S.MeshCollider(terrain, p, q)])
                ref.colliders = mesh_ref.World([ball], [mesh_ref.Instance(mesh, p, q)])
            system.update(dt)
            ref.step(dt)
            if fr % 10 == 9 or fr == 119:
                got, want = h.particles(0), ref.particles[0]
                assert len(got) == len(want["age"]), (fr, len(got), len(want["age"]))
                _assert_same(got, want, f"frame {fr}")
                dead, wdead = h.destroyed(0), ref.destroyed[0]
                assert len(dead) == len(wdead["age"]), fr
                assert np.array_equal(dead["age"], wdead["age"]), fr
                _assert_same(dead, wdead, f"destroyed, frame {fr}")
                hits += int((got["velocity"][:, 1] > 0).sum()) if not destroy else len(dead)
        assert len(h.particles(0)) > 300 and hits > 100, hits


def test_mesh_errors_keep_the_previous_state(fw_path):
    from bevy_firework_amd.system import FwError, ParticleSystem

    v, t = mesh_ref.grid_mesh(4, 4, extent=2.0, y=0.0)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(_still_settings(), uid=1)
        for bad_v, bad_t in ((v[:0], t), (v, t[:0]), (v, np.where(t == 3, len(v), t)),
                             (np.where(np.arange(len(v))[:, None] == 4, np.nan, v), t),
                             (np.zeros((3, 3), dtype=f32), np.array([[0, 1, 2]], dtype=np.uint32))):
            with pytest.raises(FwError) as e:
                system.create_mesh(bad_v, bad_t)
            assert e.value.status == FW_EINVAL
        m = system.create_mesh(v, t)
        other = system.create_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m)])
        for inst in ([S.MeshCollider(m), S.MeshCollider(999)], [S.MeshCollider(-1)]):
            with pytest.raises(FwError) as e:
                system.set_mesh_colliders(inst)
            assert e.value.status == FW_EINVAL
        with pytest.raises(FwError) as e:
            system.destroy_mesh(m)  # (placed by the current set)
        assert e.value.status == FW_EINVAL
        system.destroy_mesh(other)
        with pytest.raises(FwError) as e:
            system.destroy_mesh(other)  # (gone)
        assert e.value.status == FW_EINVAL
        with pytest.raises(FwError) as e:
            system.set_mesh_colliders([S.MeshCollider(other)])  # (a destroyed handle is unknown)
        assert e.value.status == FW_EINVAL
        # the set of the first call still stands: a particle falling onto the grid bounces
        h.write_particles(0, _particles(np.array([[0.3, 0.1, 0.2]], dtype=f32), np.array([[0.0, -12.0, 0.0]], dtype=f32)))
        system.update(f32(1.0 / 60.0))
        p = h.particles(0)
        assert p["velocity"][0, 1] > 0 and p["position"][0, 1] > 0, p
        system.set_mesh_colliders([])
        system.destroy_mesh(m)
        h.write_particles(0, _particles(np.array([[0.3, 0.1, 0.2]], dtype=f32), np.array([[0.0, -12.0, 0.0]], dtype=f32)))
        system.update(f32(1.0 / 60.0))
        assert h.particles(0)["position"][0, 1] < 0  # (no world left: it falls through)


def test_mesh_create_destroy_cycles_give_memory_back(fw_path):
    import torch

    from bevy_firework_amd.system import ParticleSystem

    v, t = _terrain(48)
    with ParticleSystem(device=0, seed=SEED) as system:
        system.spawn(_still_settings(), uid=1)
        free = []
        for cycle in range(100):
            m = system.create_mesh(v, t)
            system.set_mesh_colliders([S.MeshCollider(m, (0.0, 0.1 * cycle, 0.0))])
            system.update(f32(1.0 / 60.0))
            system.set_mesh_colliders([])
            system.destroy_mesh(m)
            system.synchronize()
            free.append(torch.cuda.mem_get_info(0)[0])
        drift = free[0] - free[-1]
        print(f"free device memory after cycle 1 / 100: {free[0] / MB:.1f} / {free[-1] / MB:.1f} MB (drift {drift / MB:.2f} MB)")
        assert drift < MB, [f / MB for f in free[:3] + free[-3:]]


def test_mesh_allocation_failures_leave_the_context_usable():
    """the `ab` build's FW_FAIL_ALLOC=k for every allocation fw_ctx_create_mesh makes: the call fails with a status, the
    context stays usable (the same mesh is created again and a frame against it is right) and nothing leaks.  In a
    subprocess: the `ab` build and its knobs are per process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ab = os.path.join(root, "bevy_firework_amd", "csrc", "libfirework_hip_ab.so")
    assert os.path.exists(ab), "libfirework_hip_ab.so not built (make -C bevy_firework_amd/csrc)"
    code = textwrap.dedent("""
        import os, sys, traceback
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np, torch
        from bevy_firework_amd import settings as S
        from bevy_firework_amd.system import ParticleSystem, FwError
        import mesh_ref
        from test_gpu_mesh import _still_settings, _particles
        v, t = mesh_ref.grid_mesh(8, 8, extent=2.0, y=0.0)
        def frame(ps, h, m):
            ps.set_mesh_colliders([S.MeshCollider(m)])
            h.write_particles(0, _particles(np.array([[0.3, 0.1, 0.2]], dtype=np.float32), np.array([[0.0, -12.0, 0.0]], dtype=np.float32)))
            ps.update(np.float32(1.0 / 60.0))
            return h.particles(0)["velocity"][0, 1] > 0
        def run(k):
            # -> None when the k-th allocation is not one of fw_ctx_create_mesh's, else (its status, the frame was right)
            os.environ["FW_FAIL_ALLOC"] = str(k)
            try:
                ps = ParticleSystem(device=0, seed=1)
            except FwError:
                return None
            try:
                h = ps.spawn(_still_settings(), uid=1)
                h.write_particles(0, _particles(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)))
                ps.update(np.float32(1.0 / 60.0))
                ps.synchronize()
            except FwError:
                ps.close()
                return None
            try:
                m = ps.create_mesh(v, t)
                failed = None
            except FwError as e:
                failed = e.status
                m = ps.create_mesh(v, t)  # (the k-th allocation failed once: this one runs through)
            try:
                ok = frame(ps, h, m)
            except FwError:  # (the failure came after the mesh: the instance table)
                ok = frame(ps, h, m)
            ps.close()
            return failed, ok
        try:
            assert run(0) == (None, True)
            torch.cuda.empty_cache()
            free0 = torch.cuda.mem_get_info(0)[0]
            failures, k = [], 0
            for k in range(1, 1001):
                r = run(k)
                if r is None:
                    continue  # (the k-th allocation comes before the mesh)
                failed, ok = r
                assert ok, k
                if failed is not None:
                    failures.append((k, failed))
                elif failures:
                    break  # (past the mesh's allocations)
            free1 = torch.cuda.mem_get_info(0)[0]
            print("MESH-ALLOC-FAIL-OK", failures, "free %%.1f -> %%.1f MB" %% (free0 / 2**20, free1 / 2**20))
            assert len(failures) == 2 and all(st != 0 for _, st in failures), failures
            assert abs(free0 - free1) < 64 * 2**20
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            raise
    """) % (root, root)
    env = dict(os.environ, FW_ENABLE_KNOBS="1", FW_LIB_PATH=ab)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "MESH-ALLOC-FAIL-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_mesh_tie_rule_on_the_device(monkeypatch, fw_path):
    """equal distances, different normals (mesh_ref.tie_meshes): the analytic plane before a mesh, the lower instance, the
    lower original triangle -- the bounce shows which surface won, and matches the reference"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    tilted, flat, tilted_first, flat_first = mesh_ref.tie_meshes()
    plane = S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    # (analytic colliders, meshes of the instances in order, does the tilted triangle win)
    cases = [([plane], [tilted], False), ([], [tilted, flat], True), ([], [flat, tilted], False),
             ([], [tilted_first], True), ([], [flat_first], False)]
    spawner = _still_settings()
    dt = f32(1.0 / 60.0)
    parts = _particles(np.array([[0.0, 1.0, -0.5]], dtype=f32), np.array([[0.0, -120.0, 0.0]], dtype=f32))
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        for analytic, ms, tilted_wins in cases:
            system.set_colliders(analytic)
            hs = [system.create_mesh(v, t) for v, t in ms]
            system.set_mesh_colliders([S.MeshCollider(m) for m in hs])
            h.write_particles(0, parts)
            system.update(dt)
            got = h.particles(0)
            ref = np_sim.Spawner(spawner, SEED, 1)
            ref.colliders = mesh_ref.World(list(analytic), [mesh_ref.Instance(mesh_ref.Mesh(v, t)) for v, t in ms])
            ref.particles[0] = _np_state(parts)
            ref.update(dt)
            _assert_same(got, ref.particles[0], (len(analytic), tilted_wins))
            assert (got["velocity"][0, 0] != 0) == tilted_wins, got["velocity"]
            system.set_mesh_colliders([])
            for m in hs:
                system.destroy_mesh(m)
