"""Deformable collider meshes (include/firework_hip.h: DEFORMABLE MESHES): after fw_ctx_update_mesh_vertices(xyz') every ray cast
equals, bit for bit, the cast against a mesh created from xyz' -- checked against the brute-force numpy reference
(tests/mesh_ref.py over Mesh(xyz', indices)), the C oracle (a fresh fwo_mesh_create per frame) and the device's own static
meshes.  The autouse fw_path fixture runs every test on the FIFO ring, range ring, compacting and small paths.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402
from mesh_rays import ray_world as _ray_world, rays as _rays, unit_quat as _unit_quat  # noqa: E402
from test_gpu_mesh import (SEED, MB, _assert_same, _falling_spawner, _np_state, _particles, _ref_world,  # noqa: E402
                           _still_settings)

from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
DT = f32(1.0 / 60.0)


def deform(v, amount=0.15):
    """a smooth displacement of every vertex (fp32 in, fp32 out)"""
    v = np.asarray(v, dtype=np.float64)
    return (v + amount * np.sin(2.0 * v[:, [1, 2, 0]] + 0.7)).astype(f32)


def terrain(frame, cells=12, extent=6.0):
    """the terrain of test_mesh_trajectories_are_bit_exact with its heights moving: p = 0.05 x frame"""
    p = 0.05 * frame
    return mesh_ref.grid_mesh(cells, cells, extent=extent, height=lambda x, z: 0.4 * np.sin(0.8 * x + p) * np.cos(0.6 * z - 0.5 * p) - 0.2)


def test_deformed_mesh_ray_casts_are_bit_exact(monkeypatch, fw_path):
    """the 50k-ray world of tests/mesh_rays.py, its meshes created deformable and then updated to deformed vertices: one step,
    every position and velocity equals np_sim + mesh_ref over Mesh(v', t) bit for bit"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    meshes, placements, analytic = _ray_world()
    moved_meshes = {n: (deform(v), t) for n, (v, t) in meshes.items()}
    pos, vel, dt = _rays(moved_meshes, placements, n_random=22000)
    assert len(pos) >= 50000
    spawner = _still_settings(capacity=1 << 17)
    spawner.particle_settings[0].collision_settings = S.ParticleCollisionSettings(0.6, 0.3, False, 0b101)
    parts = _particles(pos, vel)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        system.set_colliders(analytic)
        handles = {n: system.create_deformable_mesh(v, t) for n, (v, t) in meshes.items()}
        system.set_mesh_colliders([S.MeshCollider(handles[n], p, q, layers) for n, p, q, layers in placements])
        for n, (v, _) in moved_meshes.items():
            system.update_mesh_vertices(handles[n], v)
        h.write_particles(0, parts)
        system.update(dt)
        got = h.particles(0)
    ref = np_sim.Spawner(spawner, SEED, 1)
    ref.colliders = _ref_world(moved_meshes, placements, analytic)
    ref.particles[0] = _np_state(parts)
    ref.update(dt)
    want = ref.particles[0]
    assert len(got) == len(want["age"]) == len(pos)
    moved = (want["velocity"] != vel).any(axis=1)
    print("bounces:", int(moved.sum()))
    assert moved.sum() > 5000, int(moved.sum())
    _assert_same(got, want, "one step over deformed meshes")


@pytest.mark.parametrize("destroy, moving", [(False, False), (True, False), (False, True)])
def test_trajectories_over_a_terrain_that_deforms_every_frame(monkeypatch, fw_path, destroy, moving):
    """120 frames (bouncing / destroyed on contact with the records compared / the instance moved every frame as well) over a
    terrain whose heights change EVERY frame with no synchronisation in between; the reference's world is rebuilt from the
    frame's vertices"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v0, t = terrain(0)
    spawner, tf = _falling_spawner(destroy)
    ball = S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)
    ref = np_sim.Spawner(spawner, SEED, 3, tf)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([ball])
        m = system.create_deformable_mesh(v0, t)
        p, q = (f32(0.0), f32(0.0), f32(0.0)), (0.0, 0.0, 0.0, 1.0)
        system.set_mesh_colliders([S.MeshCollider(m, p, q)])
        hits = 0
        for fr in range(120):
            v = terrain(fr)[0]
            system.update_mesh_vertices(m, v)
            if moving:
                p = (f32(0.01 * (fr % 17)), f32(-0.005 * (fr % 5)), f32(0.0))
                q = _unit_quat(0.0, 0.02 * (fr % 3), 0.0, 1.0)
                system.set_mesh_colliders([S.MeshCollider(m, p, q)])
            ref.colliders = mesh_ref.World([ball], [mesh_ref.Instance(mesh_ref.Mesh(v, t), p, q)])
            system.update(DT)
            ref.step(DT)
            if fr % 10 == 9 or fr == 119:
                got, want = h.particles(0), ref.particles[0]
                assert len(got) == len(want["age"]), (fr, len(got), len(want["age"]))
                _assert_same(got, want, f"frame {fr}")
                dead, wdead = h.destroyed(0), ref.destroyed[0]
                assert len(dead) == len(wdead["age"]), fr
                assert np.array_equal(dead["age"], wdead["age"]), fr
                _assert_same(dead, wdead, f"destroyed, frame {fr}")
                hits += int((got["velocity"][:, 1] > 0).sum()) if not destroy else len(dead)
        print("live / hits:", len(h.particles(0)), hits)
        assert len(h.particles(0)) > 300 and hits > 100, hits


def test_deforming_terrain_against_the_c_oracle(fw_path):
    """the same trajectory against the third implementation: the C oracle with a mesh created from each frame's vertices"""
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import Pair

    v0, t = terrain(0)
    spawner, tf = _falling_spawner(True)
    ball = S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)
    with ParticleSystem(device=0, seed=SEED) as system:
        pair = Pair(system, spawner, tf, seed=SEED, uid=3)
        system.set_colliders([ball])
        pair.cpu.set_colliders([ball])
        m = system.create_deformable_mesh(v0, t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, 0.0, 0.0))])
        dead_total = 0
        for fr in range(120):
            v = terrain(fr)[0]
            system.update_mesh_vertices(m, v)
            om = oracle.OracleMesh(v, t)
            pair.cpu.set_mesh_colliders([S.MeshCollider(om, (0.0, 0.0, 0.0))])
            system.update(DT)
            pair.step_cpu(DT)
            cd = pair.cpu.destroyed(0)
            dead_total += len(cd)
            if fr % 10 == 9:
                gd = pair.gpu.destroyed(0)
                assert len(gd) == len(cd), fr
                for f in ("age", "position", "velocity", "lifetime"):
                    assert np.array_equal(gd[f], cd[f]), (fr, f)
                pair.check(exact_all=True, what=f"frame {fr}")
        assert sum(pair.gpu.counts()) > 300 and dead_total > 100, (pair.gpu.counts(), dead_total)


def _one_step(system, h, parts, dt=DT):
    h.write_particles(0, parts)
    system.update(dt)
    return h.particles(0)


def _ref_step(spawner, parts, world, dt=DT):
    ref = np_sim.Spawner(spawner, SEED, 1)
    ref.colliders = world
    ref.particles[0] = _np_state(parts)
    ref.update(dt)
    return ref.particles[0]


def _rain(n=4000, seed=2, height=0.6, extent=2.5):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-extent, extent, n), np.full(n, height), rng.uniform(-extent, extent, n)], 1).astype(f32)
    vel = np.stack([rng.uniform(-3, 3, n), rng.uniform(-90, -20, n), rng.uniform(-3, 3, n)], 1).astype(f32)
    return _particles(pos, vel)


def test_triangles_collapse_and_reopen(monkeypatch, fw_path):
    """vertices driven onto one line (EVERY triangle flat: nothing is hit, the reference leaves the instance out), half the field
    collapsed, and back open again -- the zero-area rule is evaluated per update"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(10, 10, extent=3.0, height=lambda x, z: 0.2 * np.sin(x) * np.cos(z))
    flat = v.copy()
    flat[:, 2] = 0.0
    flat[:, 1] = 0.0  # every vertex on the x axis
    half = v.copy()
    half[v[:, 0] < 0] = (-0.5, 0.1, 0.0)  # the left half in one point
    spawner = _still_settings()
    parts = _rain()
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.2, 0.0))])
        seen = []
        for name, w in (("open", v), ("half", half), ("flat", flat), ("reopened", deform(v, 0.1)), ("flat again", flat), ("open again", v)):
            system.update_mesh_vertices(m, w)
            got = _one_step(system, h, parts)
            kept = mesh_ref.Mesh(w, t)
            insts = [mesh_ref.Instance(kept, (0.0, -0.2, 0.0))] if len(kept.orig) else []
            want = _ref_step(spawner, parts, mesh_ref.World([], insts))
            _assert_same(got, want, name)
            seen.append((name, len(kept.orig), int((want["velocity"][:, 1] > 0).sum())))
        print(seen)
        by = {n: (k, b) for n, k, b in seen}
        assert by["flat"] == (0, 0) and by["flat again"] == (0, 0)
        assert 0 < by["half"][0] < by["open"][0] == len(t) and 0 < by["half"][1] < by["open"][1]
        assert by["reopened"][1] > 1000 and by["open again"] == by["open"]


def test_a_refit_equals_a_rebuild(fw_path):
    """after k updates, particles stepped over the updated mesh equal particles stepped over fw_ctx_create_mesh(xyz_k) placed
    identically -- bit for bit, the device against itself"""
    from bevy_firework_amd.system import ParticleSystem

    v, t = mesh_ref.grid_mesh(24, 24, extent=3.0, height=lambda x, z: 0.3 * np.sin(1.1 * x) * np.cos(0.7 * z))
    spawner = _still_settings()
    parts = _rain(6000, seed=5)
    q = _unit_quat(0.05, 0.3, -0.1, 0.9)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        w = v
        for k in range(1, 6):
            w = deform(w, 0.05 * k)
            system.update_mesh_vertices(m, w)
            system.set_mesh_colliders([S.MeshCollider(m, (0.1, -0.3, 0.0), q)])
            a = _one_step(system, h, parts).copy()
            fresh = system.create_mesh(w, t)
            system.set_mesh_colliders([S.MeshCollider(fresh, (0.1, -0.3, 0.0), q)])
            b = _one_step(system, h, parts).copy()
            system.set_mesh_colliders([])
            system.destroy_mesh(fresh)
            assert (a["velocity"][:, 1] > 0).sum() > 1000, k
            _assert_same(a, b, f"update {k}")


def test_update_errors_keep_the_previous_state(monkeypatch, fw_path):
    from bevy_firework_amd.system import FwError, ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(6, 6, extent=2.5, height=lambda x, z: 0.1 * x)
    w = deform(v, 0.3)
    spawner = _still_settings()
    parts = _rain(1500, seed=7, extent=2.0)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        static = system.create_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m), S.MeshCollider(static, (0.0, -1.0, 0.0))])
        nan = w.copy()
        nan[7, 1] = np.nan
        inf = w.copy()
        inf[0, 0] = np.inf
        for handle, xyz in ((999, w), (-1, w), (static, w), (m, w[:-1]), (m, np.concatenate([w, w[:1]])), (m, nan), (m, inf)):
            with pytest.raises(FwError) as e:
                system.update_mesh_vertices(handle, xyz)
            assert e.value.status == FW_EINVAL, (handle, len(xyz))
        ref_m = mesh_ref.Mesh(v, t)
        world = mesh_ref.World([], [mesh_ref.Instance(ref_m), mesh_ref.Instance(ref_m, (0.0, -1.0, 0.0))])
        got = _one_step(system, h, parts)
        want = _ref_step(spawner, parts, world)
        assert (want["velocity"][:, 1] > 0).sum() > 300
        _assert_same(got, want, "after refused updates")
        # ... and a good one still goes through afterwards
        system.update_mesh_vertices(m, w)
        world = mesh_ref.World([], [mesh_ref.Instance(mesh_ref.Mesh(w, t)), mesh_ref.Instance(ref_m, (0.0, -1.0, 0.0))])
        _assert_same(_one_step(system, h, parts), _ref_step(spawner, parts, world), "after a good update")
        with pytest.raises(FwError):
            system.destroy_mesh(m)  # (placed: like any other mesh)
        system.set_mesh_colliders([])
        system.destroy_mesh(m)
        with pytest.raises(FwError) as e:
            system.update_mesh_vertices(m, w)  # (gone)
        assert e.value.status == FW_EINVAL
        m2 = system.create_deformable_mesh(v, t)  # the handle is used again
        assert m2 == m
        system.update_mesh_vertices(m2, w)


def test_unplaced_and_twice_placed_meshes_follow_their_updates(monkeypatch, fw_path):
    """an update of a mesh that no instance places is seen when it is placed later; a mesh placed twice with different rotations
    (and far from the origin: the bounding spheres of both instances must move with it) updates in both places"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(8, 8, extent=2.5, height=lambda x, z: 0.15 * np.sin(x + z))
    w = deform(v, 0.25)
    far = (w + np.array([0.0, 0.0, 40.0], dtype=f32)).astype(f32)  # the whole mesh moved 40 units in its own frame
    spawner = _still_settings()
    parts = _rain(3000, seed=11)
    qa, qb = (0.0, 0.0, 0.0, 1.0), _unit_quat(0.2, 0.1, 0.0, 0.95)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        system.update_mesh_vertices(m, w)  # (placed by nothing yet)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.1, 0.0), qa), S.MeshCollider(m, (0.3, -0.6, 0.0), qb)])
        rm = mesh_ref.Mesh(w, t)
        world = mesh_ref.World([], [mesh_ref.Instance(rm, (0.0, -0.1, 0.0), qa), mesh_ref.Instance(rm, (0.3, -0.6, 0.0), qb)])
        want = _ref_step(spawner, parts, world)
        assert (want["velocity"][:, 1] > 0).sum() > 1000
        _assert_same(_one_step(system, h, parts), want, "placed after its update")
        # moved far away inside its own frame, the instances moved back by as much: the same world up to rounding of the sum
        system.update_mesh_vertices(m, far)
        back = [(0.0, -0.1, -40.0), tuple(float(c) for c in np.array([0.3, -0.6, 0.0]) - np_sim.quat_mul_vec3(
            np.array([qb], dtype=f32), np.array([[0.0, 0.0, 40.0]], dtype=f32))[0].astype(np.float64))]
        system.set_mesh_colliders([S.MeshCollider(m, back[0], qa), S.MeshCollider(m, back[1], qb)])
        system.update_mesh_vertices(m, far)  # (... and once more with the set in place: the restaged spheres)
        rm = mesh_ref.Mesh(far, t)
        world = mesh_ref.World([], [mesh_ref.Instance(rm, back[0], qa), mesh_ref.Instance(rm, back[1], qb)])
        want = _ref_step(spawner, parts, world)
        assert (want["velocity"][:, 1] > 0).sum() > 1000
        _assert_same(_one_step(system, h, parts), want, "moved within its frame")


def test_deformable_mesh_cycles_give_memory_back(fw_path):
    import torch

    from bevy_firework_amd.system import ParticleSystem

    v, t = terrain(0, cells=48)
    with ParticleSystem(device=0, seed=SEED) as system:
        system.spawn(_still_settings(), uid=1)
        free = []
        for cycle in range(100):
            m = system.create_deformable_mesh(v, t)
            system.set_mesh_colliders([S.MeshCollider(m, (0.0, 0.1 * cycle, 0.0))])
            for k in range(3):
                system.update_mesh_vertices(m, terrain(cycle + k, cells=48)[0])
                system.update(DT)
            system.set_mesh_colliders([])
            system.destroy_mesh(m)
            system.synchronize()
            free.append(torch.cuda.mem_get_info(0)[0])
        drift = free[0] - free[-1]
        print(f"free device memory after cycle 1 / 100: {free[0] / MB:.1f} / {free[-1] / MB:.1f} MB (drift {drift / MB:.2f} MB)")
        assert drift < MB, [f / MB for f in free[:3] + free[-3:]]


def test_deformable_mesh_allocation_failures_leave_the_context_usable():
    """tests/test_gpu_mesh.py's test_mesh_allocation_failures_leave_the_context_usable for the deformable entry: the `ab` build's
    FW_FAIL_ALLOC=k for every allocation fw_ctx_create_deformable_mesh makes (nodes, triangles, slots, order, level offsets,
    vertices, two pinned staging buffers: eight) -- the call fails with a status, the context stays usable (the same mesh is
    created again, updated, and a frame against it is right) and nothing leaks.  In a subprocess: the build and its knobs are
    per process."""
    import subprocess
    import textwrap

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
        up = v.copy(); up[:, 1] = 0.05
        def frame(ps, h, m):
            # the grid raised to y = 0.05 by an update: a particle that starts at y = 0.03 falls away under it, one from 0.1 bounces
            ps.set_mesh_colliders([S.MeshCollider(m)])
            ps.update_mesh_vertices(m, up)
            h.write_particles(0, _particles(np.array([[0.3, 0.1, 0.2], [0.3, 0.03, 0.2]], dtype=np.float32),
                                            np.array([[0.0, -12.0, 0.0], [0.0, -12.0, 0.0]], dtype=np.float32)))
            ps.update(np.float32(1.0 / 60.0))
            p = h.particles(0)
            return p["velocity"][0, 1] > 0 and p["velocity"][1, 1] < 0
        def run(k):
            # -> None when the k-th allocation is not one of fw_ctx_create_deformable_mesh's, else (its status, the frame was right)
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
                m = ps.create_deformable_mesh(v, t)
                failed = None
            except FwError as e:
                failed = e.status
                m = ps.create_deformable_mesh(v, t)  # (the k-th allocation failed once: this one runs through)
            try:
                ok = frame(ps, h, m)
            except FwError:  # (the failure came after the mesh: the instance table or its staging)
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
            print("DEFORM-ALLOC-FAIL-OK", failures, "free %%.1f -> %%.1f MB" %% (free0 / 2**20, free1 / 2**20))
            assert len(failures) == 8 and all(st != 0 for _, st in failures), failures
            assert abs(free0 - free1) < 64 * 2**20
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            raise
    """) % (root, root)
    env = dict(os.environ, FW_ENABLE_KNOBS="1", FW_LIB_PATH=ab)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DEFORM-ALLOC-FAIL-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_large_mesh_runs_the_wide_levels(monkeypatch, fw_path):
    """a mesh whose lowest levels hold more nodes than the one-workgroup tail takes (fw_k_refit.hip: a launch per wide level):
    32 768 triangles, rays against the brute force over the deformed vertices"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(128, 128, extent=3.0, height=lambda x, z: 0.2 * np.sin(2 * x) * np.cos(1.5 * z))
    w = deform(v, 0.2)
    spawner = _still_settings()
    parts = _rain(4000, seed=13)  # (about half of a rain reaches the terrain within the step: _rain)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.3, 0.0))])
        for xyz in (w, v, w):
            system.update_mesh_vertices(m, xyz)
        got = _one_step(system, h, parts)
    want = _ref_step(spawner, parts, mesh_ref.World([], [mesh_ref.Instance(mesh_ref.Mesh(w, t), (0.0, -0.3, 0.0))]))
    assert (want["velocity"][:, 1] > 0).sum() > 1000
    _assert_same(got, want, "32k triangles")


# ---- one random suite: the mesh worlds of tests/test_gpu_fuzz.py with some meshes deformable and updated at random frames ----
DEFORM_SEED_BASE = 93000
DEFORM_CASES = 8


@pytest.mark.parametrize("case", range(DEFORM_CASES))
def test_random_mesh_worlds_with_deforming_meshes_match_the_oracle(case):
    """`_mesh_scene` of tests/test_gpu_fuzz.py (random colliding spawners, one to three mesh instances, the world replaced half
    way); the first mesh of each world and about half the others are created deformable and get new vertices at random frames -- the oracle's side is a fresh mesh
    of those vertices.  Every field of the live particles and of the destroyed records against the oracle, bit for bit."""
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import MeshPair, Pair
    from test_gpu_fuzz import _DESTROYED_FIELDS, _mesh_scene
    from test_gpu_fuzz import SEED as FSEED

    class DeformPair(MeshPair):
        """a MeshPair whose device mesh is deformable; update() moves both sides"""

        def __init__(self, system, vertices, indices):  # noqa: super().__init__ would create a static mesh
            self.system, self.indices = system, indices
            self.gpu = system.create_deformable_mesh(vertices, indices)
            self.cpu = oracle.OracleMesh(vertices, indices)
            self.stale = []  # oracle meshes of earlier vertex sets: closed once the oracle's instance set no longer places them

        def update(self, vertices):
            self.system.update_mesh_vertices(self.gpu, vertices)
            self.stale.append(self.cpu)
            self.cpu = oracle.OracleMesh(vertices, self.indices)

        def close_stale(self):
            for m in self.stale:
                m.close()
            self.stale = []

        def destroy(self):
            self.close_stale()
            super().destroy()

    sc = _mesh_scene(case, seed_base=DEFORM_SEED_BASE)
    rng = np.random.default_rng(DEFORM_SEED_BASE + 500 + case)
    n_types = len(sc["spawner"].particle_settings)
    updates = n_deformable = 0
    with ParticleSystem(device=0, seed=FSEED) as system:
        pair = Pair(system, sc["spawner"], sc["transform"], seed=FSEED, uid=sc["uid"])
        live, placed = {}, []
        for i, (dt, pv) in enumerate(zip(sc["dts"], sc["pvs"])):
            ev = sc["events"].get(i)
            if ev is not None:
                for name, _, _, _ in ev["placements"]:
                    if name not in live:
                        # (the first mesh of each world -- "a0-..." / "b0-..." in _mesh_placements' names -- always deforms, the
                        # others by a coin)
                        deformable = name[1] == "0" or rng.random() < 0.5
                        live[name] = (DeformPair if deformable else MeshPair)(system, *sc["meshes"][name])
                        n_deformable += deformable
                placed = ev["placements"]
                analytic = ev["analytic"]
                pair.set_world(analytic, [(live[name], p, q, layers) for name, p, q, layers in placed])
                for name in ev["destroy"]:
                    live.pop(name).destroy()
            moved = False
            for name in sorted(live):
                if isinstance(live[name], DeformPair) and rng.random() < 0.5:
                    v = sc["meshes"][name][0]
                    live[name].update((v + rng.normal(scale=0.08, size=v.shape) * (rng.random() < 0.8)).astype(f32))
                    moved, updates = True, updates + 1
            if moved:  # the oracle's instances point at the new meshes (the device's follow by themselves)
                pair.cpu.set_mesh_colliders([S.MeshCollider(live[name].cpu, p, q, layers) for name, p, q, layers in placed])
                for name in live:
                    if isinstance(live[name], DeformPair):
                        live[name].close_stale()
            pair.gpu.set_parent_velocity(pv)
            pair.cpu.set_parent_velocity(pv)
            system.update(dt)
            pair.step_cpu(dt)
            for ty in range(n_types):
                cd = pair.cpu.destroyed(ty)
                if i % 8 == 7:
                    gd = pair.gpu.destroyed(ty)
                    assert len(gd) == len(cd), f"case {case} frame {i} type {ty}: destroyed {len(gd)} != {len(cd)}"
                    for f in _DESTROYED_FIELDS:
                        assert np.array_equal(gd[f], cd[f]), f"case {case} frame {i} type {ty}: destroyed.{f}"
            if i % 8 == 7:
                pair.check(exact_all=True, what=f"case {case} frame {i}")
        print(f"case {case}: {updates} updates, {sum(pair.gpu.counts())} live particles")
        assert updates >= 5 and n_deformable > 0, (updates, n_deformable)
