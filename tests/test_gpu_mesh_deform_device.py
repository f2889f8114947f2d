"""Deformable collider meshes updated from DEVICE memory (include/firework_hip.h: DEFORMABLE MESHES, FROM DEVICE MEMORY): after
fw_ctx_update_mesh_vertices_device(d_xyz) every ray cast equals, bit for bit, the cast against a mesh created from what the
buffer held -- checked against the brute-force numpy reference (tests/mesh_ref.py), the C oracle and the host form; a
non-finite vertex rejects the update on the device and the previous shape stays.  Device buffers are torch tensors.  The
autouse fw_path fixture runs every test on the FIFO ring, range ring, compacting and small paths.  Needs an MI355X."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402
from mesh_rays import ray_world as _ray_world, rays as _rays, unit_quat as _unit_quat  # noqa: E402
from test_gpu_mesh import (SEED, MB, _assert_same, _falling_spawner, _np_state, _particles, _ref_world,  # noqa: E402,F401
                           _still_settings)
from test_gpu_mesh_deform import DT, _one_step, _rain, _ref_step, deform, terrain  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx_stream(system):
    """torch's view of the context's stream: what is enqueued under it is ordered with the context's frames"""
    import torch

    return torch.cuda.stream(torch.cuda.ExternalStream(system.stream))


def _dev(system, v):
    """v ([n, 3] float32) in a device tensor written on the context's stream"""
    import torch

    host = torch.from_numpy(np.ascontiguousarray(v, dtype=f32).reshape(-1, 3).copy())
    with _ctx_stream(system):
        return host.to("cuda")


def _update(system, m, t):
    system.update_mesh_vertices_device(m, t.data_ptr(), t.shape[0])


def test_ray_casts_after_a_device_update_are_bit_exact(monkeypatch, fw_path):
    """the 50k-ray world of tests/mesh_rays.py, its meshes created deformable and updated through the device form: one step, every
    position and velocity equals np_sim + mesh_ref over Mesh(v', t) with v' what the device buffers hold, read back"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    meshes, placements, analytic = _ray_world()
    spawner = _still_settings(capacity=1 << 17)
    spawner.particle_settings[0].collision_settings = S.ParticleCollisionSettings(0.6, 0.3, False, 0b101)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        system.set_colliders(analytic)
        handles = {n: system.create_deformable_mesh(v, t) for n, (v, t) in meshes.items()}
        system.set_mesh_colliders([S.MeshCollider(handles[n], p, q, layers) for n, p, q, layers in placements])
        bufs = {n: _dev(system, deform(v)) for n, (v, _) in meshes.items()}
        for n in meshes:
            _update(system, handles[n], bufs[n])
        with _ctx_stream(system):  # (read back in the stream that wrote them)
            moved_meshes = {n: (bufs[n].cpu().numpy(), meshes[n][1]) for n in meshes}
        pos, vel, dt = _rays(moved_meshes, placements, n_random=22000)
        assert len(pos) >= 50000
        parts = _particles(pos, vel)
        h.write_particles(0, parts)
        system.update(dt)
        got = h.particles(0)
        system.synchronize()
        for n in meshes:
            assert system.mesh_update_status(handles[n]) == (1, 0, -1), n
    ref = np_sim.Spawner(spawner, SEED, 1)
    ref.colliders = _ref_world(moved_meshes, placements, analytic)
    ref.particles[0] = _np_state(parts)
    ref.update(dt)
    want = ref.particles[0]
    assert len(got) == len(want["age"]) == len(pos)
    moved = (want["velocity"] != vel).any(axis=1)
    print("bounces:", int(moved.sum()))
    assert moved.sum() > 5000, int(moved.sum())
    _assert_same(got, want, "one step over meshes deformed on the device")


def _device_terrain_frames(system, frames=120, cells=12, extent=6.0):
    """-> (tensor [frames, n, 3] computed ON THE GPU on the context's stream, indices): the terrain of tests/test_gpu_mesh_deform.py
    with its heights moving, in the device's own fp32 arithmetic (the reference reads the tensor back: whatever it holds is v')"""
    import torch

    v0, t = terrain(0, cells=cells, extent=extent)
    with _ctx_stream(system):
        base = torch.from_numpy(v0.copy()).to("cuda")
        p = 0.05 * torch.arange(frames, dtype=torch.float32, device="cuda")[:, None]
        x, z = base[None, :, 0], base[None, :, 2]
        y = 0.4 * torch.sin(0.8 * x + p) * torch.cos(0.6 * z - 0.5 * p) - 0.2
        V = torch.stack([x.expand(frames, -1), y, z.expand(frames, -1)], dim=2).contiguous()
    return V, t


@pytest.mark.parametrize("destroy, moving", [(False, False), (True, False), (False, True)])
def test_trajectories_over_a_terrain_deformed_on_the_device_every_frame(monkeypatch, fw_path, destroy, moving):
    """120 frames (bouncing / destroyed on contact with the records compared / the instance moved every frame as well: staged
    as never skipped, its sphere fixed behind the copy) over a terrain whose vertices come from one [frames, n, 3] tensor
    computed on the GPU up front; nothing waits between a frame's update and its step"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    spawner, tf = _falling_spawner(destroy)
    ball = S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)
    ref = np_sim.Spawner(spawner, SEED, 3, tf)
    with ParticleSystem(device=0, seed=SEED) as system:
        V, t = _device_terrain_frames(system)
        with _ctx_stream(system):
            Vh = V.cpu().numpy()  # (read back once, for the reference)
        assert np.isfinite(Vh).all() and np.ptp(Vh[:, :, 1], axis=0).max() > 0.2
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([ball])
        m = system.create_deformable_mesh(Vh[0], t)
        p, q = (f32(0.0), f32(0.0), f32(0.0)), (0.0, 0.0, 0.0, 1.0)
        system.set_mesh_colliders([S.MeshCollider(m, p, q)])
        hits = 0
        for fr in range(120):
            _update(system, m, V[fr])
            if moving:
                p = (f32(0.01 * (fr % 17)), f32(-0.005 * (fr % 5)), f32(0.0))
                q = _unit_quat(0.0, 0.02 * (fr % 3), 0.0, 1.0)
                system.set_mesh_colliders([S.MeshCollider(m, p, q)])
            ref.colliders = mesh_ref.World([ball], [mesh_ref.Instance(mesh_ref.Mesh(Vh[fr], t), p, q)])
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
        system.synchronize()
        assert system.mesh_update_status(m) == (120, 0, -1)


def test_terrain_deformed_on_the_device_against_the_c_oracle(fw_path):
    """the same trajectory against the third implementation: the C oracle with a fresh mesh of each frame's vertices"""
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import Pair

    spawner, tf = _falling_spawner(True)
    ball = S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)
    with ParticleSystem(device=0, seed=SEED) as system:
        V, t = _device_terrain_frames(system)
        with _ctx_stream(system):
            Vh = V.cpu().numpy()
        pair = Pair(system, spawner, tf, seed=SEED, uid=3)
        system.set_colliders([ball])
        pair.cpu.set_colliders([ball])
        m = system.create_deformable_mesh(Vh[0], t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, 0.0, 0.0))])
        dead_total = 0
        for fr in range(120):
            _update(system, m, V[fr])
            om = oracle.OracleMesh(Vh[fr], t)
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


def _all_fields_equal(a, b, what):
    assert len(a) == len(b), what
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def test_the_device_form_equals_the_host_form(fw_path):
    """two contexts, the same vertices through either call: every particle field equal bit for bit after N frames; then the two
    forms alternating on ONE mesh against the host form alone"""
    from bevy_firework_amd.system import ParticleSystem

    spawner, tf = _falling_spawner(False)
    v0, t = terrain(0)
    q = _unit_quat(0.02, 0.1, -0.03, 0.99)
    for forms in ("dddddd", "dhdhhd"):
        with ParticleSystem(device=0, seed=SEED) as a, ParticleSystem(device=0, seed=SEED) as b:
            ha, hb = a.spawn(spawner, tf, uid=3), b.spawn(spawner, tf, uid=3)
            ma, mb = a.create_deformable_mesh(v0, t), b.create_deformable_mesh(v0, t)
            keep = []
            for fr in range(60):
                v = terrain(fr)[0]
                pos = (f32(0.01 * (fr % 7)), f32(-0.1), f32(0.0))
                if forms[fr % len(forms)] == "d":
                    keep.append(_dev(a, v))
                    _update(a, ma, keep[-1])
                else:
                    a.update_mesh_vertices(ma, v)
                b.update_mesh_vertices(mb, v)
                if fr % 3 == 0:  # (a new instance set now and then: both ways of getting a sphere for a device-updated mesh)
                    a.set_mesh_colliders([S.MeshCollider(ma, pos, q)])
                    b.set_mesh_colliders([S.MeshCollider(mb, pos, q)])
                a.update(DT)
                b.update(DT)
                if fr % 20 == 19:
                    _all_fields_equal(ha.particles(0), hb.particles(0), f"{forms} frame {fr}")
            assert len(ha.particles(0)) > 300 and (ha.particles(0)["velocity"][:, 1] > 0).sum() > 20
            a.synchronize()
            assert a.mesh_update_status(ma) == (60 * forms.count("d") // len(forms), 0, -1)


def test_a_buffer_overwritten_right_behind_the_call_does_not_change_the_result(monkeypatch, fw_path):
    """the vertices are read only by what the call enqueues: the caller may overwrite them on the context's stream at once"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(128, 128, extent=3.0, height=lambda x, z: 0.2 * np.sin(2 * x) * np.cos(1.5 * z))
    w = deform(v, 0.2)
    spawner = _still_settings()
    parts = _rain(4000, seed=13)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.3, 0.0))])
        buf = _dev(system, w)
        _update(system, m, buf)
        with _ctx_stream(system):
            buf.fill_(float("nan"))
            buf.mul_(2.0)
        got = _one_step(system, h, parts)
        system.synchronize()
        assert system.mesh_update_status(m) == (1, 0, -1)
    want = _ref_step(spawner, parts, mesh_ref.World([], [mesh_ref.Instance(mesh_ref.Mesh(w, t), (0.0, -0.3, 0.0))]))
    assert (want["velocity"][:, 1] > 0).sum() > 1000
    _assert_same(got, want, "buffer overwritten behind the call")


def test_a_non_finite_vertex_rejects_the_update_on_the_device(monkeypatch, fw_path):
    """NaN / inf at several indices: counts and the lowest index after a synchronisation, trajectories continue over the PREVIOUS
    shape bit for bit, fw_step keeps returning FW_OK, a following good update of either form applies; the host-side FW_EINVAL
    cases leave state and status untouched"""
    import torch

    from bevy_firework_amd.system import FwError, ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(40, 40, extent=2.5, height=lambda x, z: 0.1 * x)
    n = len(v)
    w = deform(v, 0.3)
    spawner = _still_settings()
    parts = _rain(1500, seed=7, extent=2.0)
    place = (0.0, -0.2, 0.0)

    def want_over(xyz):
        return _ref_step(spawner, parts, mesh_ref.World([], [mesh_ref.Instance(mesh_ref.Mesh(xyz, t), place)]))

    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        static = system.create_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m, place)])
        assert system.mesh_update_status(m) == (0, 0, -1)
        good = _dev(system, w)
        # rejected as a mesh's FIRST device-form update: the shape is still the creation's
        applied = rejected = 0
        shape = v
        cases = [({0: (0, np.nan)}, 0), ({n - 1: (2, np.inf)}, n - 1), ({n // 2: (1, -np.inf), n - 3: (0, np.nan)}, n // 2),
                 ({777: (1, np.nan), 5: (2, -np.inf), 1200: (0, np.inf)}, 5)]
        for k, (bad, lowest) in enumerate(cases):
            x = deform(v, 0.1 + 0.05 * k)
            for i, (c, val) in bad.items():
                x[i, c] = val
            buf = _dev(system, x)
            _update(system, m, buf)  # (accepted by the host: only the device can see the value)
            rejected += 1
            got = _one_step(system, h, parts)  # fw_step: FW_OK (the mirror raises otherwise)
            system.synchronize()
            assert system.mesh_update_status(m) == (applied, rejected, lowest), (k, system.mesh_update_status(m))
            _assert_same(got, want_over(shape), f"after rejected update {k}: the previous shape")
            if k == 0:
                # a new instance set while the first update was rejected: the spheres come from the seeded record
                system.set_mesh_colliders([S.MeshCollider(m, place), S.MeshCollider(static, (0.0, -50.0, 0.0))])
                _assert_same(_one_step(system, h, parts), want_over(shape), "new instance set after a rejected first update")
            if k == 1:
                _update(system, m, good)
                applied, shape = applied + 1, w
                _assert_same(_one_step(system, h, parts), want_over(shape), "a good device update after a rejected one")
            if k == 2:
                shape = deform(v, 0.22)
                system.update_mesh_vertices(m, shape)
                _assert_same(_one_step(system, h, parts), want_over(shape), "a good host update after a rejected one")
        assert (want_over(shape)["velocity"][:, 1] > 0).sum() > 300
        # host-side errors: at once, nothing changed
        system.synchronize()
        before = system.mesh_update_status(m)
        short = torch.zeros((n - 1, 3), dtype=torch.float32, device="cuda")
        for handle, ptr, cnt in ((999, good.data_ptr(), n), (-1, good.data_ptr(), n), (static, good.data_ptr(), n),
                                 (m, short.data_ptr(), n - 1), (m, good.data_ptr(), n + 1), (m, 0, n)):
            with pytest.raises(FwError) as e:
                system.update_mesh_vertices_device(handle, ptr, cnt)
            assert e.value.status == FW_EINVAL, (handle, cnt)
        for handle in (999, -1, static):
            with pytest.raises(FwError) as e:
                system.mesh_update_status(handle)
            assert e.value.status == FW_EINVAL
        _assert_same(_one_step(system, h, parts), want_over(shape), "after refused calls")
        system.synchronize()
        assert system.mesh_update_status(m) == before == (1, 4, 5)


def test_unplaced_and_twice_placed_meshes_follow_their_device_updates(monkeypatch, fw_path):
    """an update of a mesh that no instance places is seen when it is placed later; a mesh placed twice with different rotations
    (and far from the origin: the spheres of both instances must move with it) updates in both places"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(8, 8, extent=2.5, height=lambda x, z: 0.15 * np.sin(x + z))
    w = deform(v, 0.25)
    far = (w + np.array([0.0, 0.0, 40.0], dtype=f32)).astype(f32)
    spawner = _still_settings()
    parts = _rain(3000, seed=11)
    qa, qb = (0.0, 0.0, 0.0, 1.0), _unit_quat(0.2, 0.1, 0.0, 0.95)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        bw, bfar = _dev(system, w), _dev(system, far)
        _update(system, m, bw)  # (placed by nothing yet)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.1, 0.0), qa), S.MeshCollider(m, (0.3, -0.6, 0.0), qb)])
        rm = mesh_ref.Mesh(w, t)
        world = mesh_ref.World([], [mesh_ref.Instance(rm, (0.0, -0.1, 0.0), qa), mesh_ref.Instance(rm, (0.3, -0.6, 0.0), qb)])
        want = _ref_step(spawner, parts, world)
        assert (want["velocity"][:, 1] > 0).sum() > 1000
        _assert_same(_one_step(system, h, parts), want, "placed after its update")
        back = [(0.0, -0.1, -40.0), tuple(float(c) for c in np.array([0.3, -0.6, 0.0]) - np_sim.quat_mul_vec3(
            np.array([qb], dtype=f32), np.array([[0.0, 0.0, 40.0]], dtype=f32))[0].astype(np.float64))]
        rm = mesh_ref.Mesh(far, t)
        world = mesh_ref.World([], [mesh_ref.Instance(rm, back[0], qa), mesh_ref.Instance(rm, back[1], qb)])
        want = _ref_step(spawner, parts, world)
        assert (want["velocity"][:, 1] > 0).sum() > 1000
        # the instances first, the update behind them: the update's own sphere launch moves both spheres 40 units
        _update(system, m, bw)
        system.set_mesh_colliders([S.MeshCollider(m, back[0], qa), S.MeshCollider(m, back[1], qb)])
        _update(system, m, bfar)
        _assert_same(_one_step(system, h, parts), want, "moved within its frame, set first")
        # ... and the update first, the instances behind it: the set's sphere launch
        system.set_mesh_colliders([])
        _update(system, m, bw)
        _update(system, m, bfar)
        system.set_mesh_colliders([S.MeshCollider(m, back[0], qa), S.MeshCollider(m, back[1], qb)])
        _assert_same(_one_step(system, h, parts), want, "moved within its frame, update first")


def test_many_far_instances_next_to_one_that_is_hit_match_the_oracle(fw_path):
    """the test a stale or too-small sphere fails: forty small instances far from the particles (skipped by whole waves) and one
    whose deformation carries it from far outside its creation bounds into the particles' way -- the oracle culls nothing"""
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import Pair

    spawner, tf = _falling_spawner(False)
    v0, t = terrain(0, cells=10, extent=1.0)  # a small patch ...
    rng = np.random.default_rng(3)
    spots = [tuple(float(c) for c in rng.uniform(-60, 60, 3) + np.array([0.0, 150.0, 0.0])) for _ in range(40)]
    big, bt = terrain(0)
    with ParticleSystem(device=0, seed=SEED) as system:
        pair = Pair(system, spawner, tf, seed=SEED, uid=3)
        small = system.create_deformable_mesh(v0, t)
        # ... and the terrain, created 300 units away from where its vertices will be
        away = (big + np.array([300.0, 40.0, -200.0], dtype=f32)).astype(f32)
        m = system.create_deformable_mesh(away, bt)
        q = _unit_quat(0.1, 0.0, 0.05, 0.98)
        insts = [S.MeshCollider(small, s, q) for s in spots[:20]] + [S.MeshCollider(m, (0.0, 0.0, 0.0))] + \
                [S.MeshCollider(small, s, q) for s in spots[20:]]
        system.set_mesh_colliders(insts)
        keep, bounced = [], 0
        for fr in range(90):
            vs = (v0 * f32(1.0 + 0.01 * (fr % 9))).astype(f32)
            vb = terrain(fr)[0]
            keep += [_dev(system, vs), _dev(system, vb)]
            _update(system, small, keep[-2])
            _update(system, m, keep[-1])
            if fr % 4 == 1:
                system.set_mesh_colliders(insts)
            oms, omb = oracle.OracleMesh(vs, t), oracle.OracleMesh(vb, bt)
            pair.cpu.set_mesh_colliders([S.MeshCollider(oms, c.position, c.rotation) if c.mesh == small else S.MeshCollider(omb, (0.0, 0.0, 0.0))
                                         for c in insts])
            system.update(DT)
            pair.step_cpu(DT)
            if fr % 15 == 14:
                pair.check(exact_all=True, what=f"frame {fr}")
                bounced += int((pair.gpu.particles(0)["velocity"][:, 1] > 0).sum())
        assert sum(pair.gpu.counts()) > 300 and bounced > 50, (pair.gpu.counts(), bounced)


def test_large_mesh_runs_the_wide_levels_from_device_vertices(monkeypatch, fw_path):
    """a mesh whose lowest levels hold more nodes than the one-workgroup tail takes, and more vertices than one round of the
    bounds grid: 32 768 triangles, rays against the brute force over the deformed vertices"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setattr(np_sim, "cast_ray", mesh_ref.cast_ray)
    v, t = mesh_ref.grid_mesh(128, 128, extent=3.0, height=lambda x, z: 0.2 * np.sin(2 * x) * np.cos(1.5 * z))
    w = deform(v, 0.2)
    spawner = _still_settings()
    parts = _rain(4000, seed=13)
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, uid=1)
        m = system.create_deformable_mesh(v, t)
        system.set_mesh_colliders([S.MeshCollider(m, (0.0, -0.3, 0.0))])
        bufs = [_dev(system, x) for x in (w, v, w)]
        for b in bufs:
            _update(system, m, b)
        got = _one_step(system, h, parts)
    want = _ref_step(spawner, parts, mesh_ref.World([], [mesh_ref.Instance(mesh_ref.Mesh(w, t), (0.0, -0.3, 0.0))]))
    assert (want["velocity"][:, 1] > 0).sum() > 1000
    _assert_same(got, want, "32k triangles")


def test_device_updated_mesh_cycles_give_memory_back(fw_path):
    import torch

    from bevy_firework_amd.system import ParticleSystem

    v, t = terrain(0, cells=48)
    with ParticleSystem(device=0, seed=SEED) as system:
        system.spawn(_still_settings(), uid=1)
        bufs = [_dev(system, terrain(k, cells=48)[0]) for k in range(3)]
        free = []
        for cycle in range(100):
            m = system.create_deformable_mesh(v, t)
            system.set_mesh_colliders([S.MeshCollider(m, (0.0, 0.1 * cycle, 0.0))])
            for k in range(3):
                _update(system, m, bufs[k])
                system.update(DT)
            system.set_mesh_colliders([])
            system.destroy_mesh(m)
            system.synchronize()
            free.append(torch.cuda.mem_get_info(0)[0])
        drift = free[0] - free[-1]
        print(f"free device memory after cycle 1 / 100: {free[0] / MB:.1f} / {free[-1] / MB:.1f} MB (drift {drift / MB:.2f} MB)")
        assert drift < MB, [f / MB for f in free[:3] + free[-3:]]


def test_first_device_update_allocation_failures_leave_the_mesh_usable():
    """the `ab` build's FW_FAIL_ALLOC=k for every allocation the FIRST device-form update of a mesh makes (fw_ctx::kMeshDeviceAllocs
    in csrc/fw_engine.h says how many): the call fails with a status, the mesh keeps its shape, the same call then succeeds, a frame
    against the new shape is right and nothing leaks.  In a subprocess: the build and its knobs are per process."""
    import subprocess
    import textwrap

    ab = os.path.join(ROOT, "bevy_firework_amd", "csrc", "libfirework_hip_ab.so")
    assert os.path.exists(ab), "libfirework_hip_ab.so not built (make -C bevy_firework_amd/csrc)"
    n_allocs = int(re.search(r"kMeshDeviceAllocs\s*=\s*(\d+)", open(os.path.join(ROOT, "bevy_firework_amd", "csrc", "fw_engine.h")).read()).group(1))
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
        d_up = torch.from_numpy(up).to("cuda")
        torch.cuda.synchronize()
        def frame(ps, h):
            # a particle that starts at y = 0.03 and one from 0.1, both falling: -> (the first bounced, the second bounced)
            h.write_particles(0, _particles(np.array([[0.3, 0.1, 0.2], [0.3, 0.03, 0.2]], dtype=np.float32),
                                            np.array([[0.0, -12.0, 0.0], [0.0, -12.0, 0.0]], dtype=np.float32)))
            ps.update(np.float32(1.0 / 60.0))
            p = h.particles(0)
            return bool(p["velocity"][0, 1] > 0), bool(p["velocity"][1, 1] > 0)
        def frame2(ps, h):
            try:
                return frame(ps, h)
            except FwError:  # (the k-th allocation came after the update: a frame's own)
                return frame(ps, h)
        def run(k):
            # -> None when the k-th allocation comes before the first device-form update, else (its status, frames were right)
            os.environ["FW_FAIL_ALLOC"] = str(k)
            try:
                ps = ParticleSystem(device=0, seed=1)
            except FwError:
                return None
            try:
                h = ps.spawn(_still_settings(), uid=1)
                m = ps.create_deformable_mesh(v, t)
                ps.set_mesh_colliders([S.MeshCollider(m)])
                assert frame(ps, h) == (True, True)  # the grid at y = 0: both bounce
                ps.synchronize()
            except FwError:
                ps.close()
                return None
            ok = True
            try:
                ps.update_mesh_vertices_device(m, d_up.data_ptr(), len(up))
                failed = None
            except FwError as e:
                failed = e.status
                ok = ok and frame2(ps, h) == (True, True)  # the mesh kept its shape
                ps.update_mesh_vertices(m, v)              # ... and is usable by the host form
                ok = ok and frame2(ps, h) == (True, True)
                ps.update_mesh_vertices_device(m, d_up.data_ptr(), len(up))  # (the k-th allocation failed once: this one runs through)
            # the grid raised to y = 0.05: the particle from 0.03 falls away under it, the one from 0.1 bounces
            ok = ok and frame2(ps, h) == (True, False)
            ps.synchronize()
            ok = ok and ps.mesh_update_status(m) == (1, 0, -1)
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
                    continue
                failed, ok = r
                assert ok, k
                if failed is not None:
                    failures.append((k, failed))
                elif failures:
                    break  # (past the call's allocations)
            free1 = torch.cuda.mem_get_info(0)[0]
            print("DEVICE-FORM-ALLOC-FAIL-OK", failures, "free %%.1f -> %%.1f MB" %% (free0 / 2**20, free1 / 2**20))
            assert len(failures) == %d and all(st != 0 for _, st in failures), failures
            assert abs(free0 - free1) < 64 * 2**20
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            raise
    """) % (ROOT, ROOT, n_allocs)
    env = dict(os.environ, FW_ENABLE_KNOBS="1", FW_LIB_PATH=ab)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DEVICE-FORM-ALLOC-FAIL-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- one random suite: tests/test_gpu_mesh_deform.py's, its updates drawn from host form, device form and rejected ones ----
DEVICE_SEED_BASE = 97000
DEVICE_CASES = 8


@pytest.mark.parametrize("case", range(DEVICE_CASES))
def test_random_mesh_worlds_with_either_form_and_rejected_updates_match_the_oracle(case):
    """`_mesh_scene` of tests/test_gpu_fuzz.py; the first mesh of each world and about half the others are deformable and get new
    vertices at random frames -- through the host form, the device form, or a device-form update with a non-finite vertex, which
    must change nothing (the oracle's side keeps its mesh).  Every field of the live particles and of the destroyed records
    against the oracle, bit for bit; at the end every mesh's status counts what was drawn."""
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import MeshPair, Pair
    from test_gpu_fuzz import _DESTROYED_FIELDS, _mesh_scene
    from test_gpu_fuzz import SEED as FSEED

    class DeformPair(MeshPair):
        def __init__(self, system, vertices, indices):  # noqa: super().__init__ would create a static mesh
            self.system, self.indices = system, indices
            self.gpu = system.create_deformable_mesh(vertices, indices)
            self.cpu = oracle.OracleMesh(vertices, indices)
            self.stale, self.keep = [], []
            self.applied = self.rejected = 0
            self.bad = -1

        def update(self, vertices, form):
            if form == "host":
                self.system.update_mesh_vertices(self.gpu, vertices)
            else:
                self.keep.append(_dev(self.system, vertices))
                _update(self.system, self.gpu, self.keep[-1])
            if form == "rejected":
                self.rejected += 1
                self.bad = int(np.flatnonzero(~np.isfinite(vertices).all(axis=1))[0])
                return
            self.applied += form == "device"
            self.stale.append(self.cpu)
            self.cpu = oracle.OracleMesh(vertices, self.indices)

        def close_stale(self):
            for m in self.stale:
                m.close()
            self.stale = []

        def destroy(self):
            self.system.synchronize()
            assert self.system.mesh_update_status(self.gpu) == (self.applied, self.rejected, self.bad)
            self.close_stale()
            super().destroy()

    sc = _mesh_scene(case, seed_base=DEVICE_SEED_BASE)
    rng = np.random.default_rng(DEVICE_SEED_BASE + 500 + case)
    n_types = len(sc["spawner"].particle_settings)
    drawn = {"host": 0, "device": 0, "rejected": 0}
    with ParticleSystem(device=0, seed=FSEED) as system:
        pair = Pair(system, sc["spawner"], sc["transform"], seed=FSEED, uid=sc["uid"])
        live, placed = {}, []
        for i, (dt, pv) in enumerate(zip(sc["dts"], sc["pvs"])):
            ev = sc["events"].get(i)
            if ev is not None:
                for name, _, _, _ in ev["placements"]:
                    if name not in live:
                        deformable = name[1] == "0" or rng.random() < 0.5
                        live[name] = (DeformPair if deformable else MeshPair)(system, *sc["meshes"][name])
                placed = ev["placements"]
                analytic = ev["analytic"]
                pair.set_world(analytic, [(live[name], p, q, layers) for name, p, q, layers in placed])
                for name in ev["destroy"]:
                    live.pop(name).destroy()
            moved = False
            for name in sorted(live):
                if isinstance(live[name], DeformPair) and rng.random() < 0.6:
                    v = sc["meshes"][name][0]
                    x = (v + rng.normal(scale=0.08, size=v.shape) * (rng.random() < 0.8)).astype(f32)
                    form = ("host", "device", "device", "rejected")[int(rng.integers(4))]
                    if form == "rejected":
                        x[int(rng.integers(len(x))), int(rng.integers(3))] = (np.nan, np.inf, -np.inf)[int(rng.integers(3))]
                    live[name].update(x, form)
                    drawn[form] += 1
                    moved = moved or form != "rejected"
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
        system.synchronize()
        for name in live:
            if isinstance(live[name], DeformPair):
                assert system.mesh_update_status(live[name].gpu) == (live[name].applied, live[name].rejected, live[name].bad), name
        print(f"case {case}: {drawn}, {sum(pair.gpu.counts())} live particles")
        assert drawn["device"] >= 3 and drawn["host"] + drawn["rejected"] >= 2, drawn
