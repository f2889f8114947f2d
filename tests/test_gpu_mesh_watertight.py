"""The mesh ray cast on the device against geometry (include/firework_hip.h: fw_mesh_collider, WATERTIGHT): the properties of
tests/test_mesh_watertight_cpu.py -- no leak, no invention, a superset of the rule without the margin, the walk equal to the brute
force -- asserted of what the MI355X computes, three ways: the ray-cast query, the path query and the particles themselves, the last
two from inside a closed icosphere that nothing may leave.  The float64 reference and the brute force are those of the CPU file,
computed once per family and shared.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_exact as X  # noqa: E402
from test_gpu_mesh import SEED, _particles, _still_settings  # noqa: E402
from test_mesh_watertight_cpu import assert_same_cast, case, in_domain, oracle_cast  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
N_STEPS = 8
DT = f32(1.0 / 60.0)
SPEED = f32(45.0)  # three quarters of the sphere's radius per step: every path meets the surface within two steps, then again and again


def _system():
    from bevy_firework_amd.system import ParticleSystem

    return ParticleSystem(device=0, seed=SEED)


@pytest.mark.parametrize("name", X.GATED)
def test_query_casts_hold_the_properties(fw_path, name):
    """system.cast_rays over each family at every level: P1 inside the walk's domain, P2, P3, and P4 -- found, distance and normal
    equal the C oracle's brute force bit for bit, the triangle is the brute force's"""
    with _system() as system:
        F0 = case(name, X.LEVELS[0])
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(F0.vertices, F0.indices), F0.position, F0.rotation, 1)])
        for level in X.LEVELS:
            F = case(name, level)
            hits = system.cast_rays(F.origin, F.dir, F.max_distance, 1)
            hit = hits["kind"] == S.HIT_MESH
            assert ((hits["kind"] == S.HIT_NONE) | hit).all() and (hits["index"][hit] == 0).all()
            t = np.where(hit, hits["distance"], f32(np.inf)).astype(f32)
            assert len(F.inst.mesh.orig) == len(F.indices)  # (no triangle dropped: original indices are the kept ones')
            k = np.where(hit, hits["triangle"], 0).astype(np.int64)
            leak = X.leaks(F, hit, t)
            off, ghost = X.inventions(F, hit, t, k)
            lost = X.not_superset(F.strict, (hit, t, hits["normal"], k))
            print(f"{name} {level}: P1 {int(leak.sum())} ({int((leak & in_domain(F)).sum())} inside the domain), P2 {int(off.sum())} + {int(ghost.sum())}, "
                  f"P3 {int(lost.sum())}")
            assert not (leak & in_domain(F)).any(), ("P1", level, np.flatnonzero(leak)[:10])
            assert not off.any() and not ghost.any(), ("P2", level, np.flatnonzero(off)[:10], np.flatnonzero(ghost)[:10])
            assert not lost.any(), ("P3", level, np.flatnonzero(lost)[:10])
            assert_same_cast((hit, t, hits["normal"]), oracle_cast(F), f"P4, {name} {level}")
            assert np.array_equal(k[hit], F.new[3][hit]), ("P4, the triangle", level)
            assert not leak.any(), ("P1 (the brute force holds it everywhere)", level)


def _sealed_ball():
    """the closed icosphere and the 20 000 states that start inside it aimed at its vertices and edges"""
    F = case("ico", "inside")
    vel = (F.dir * SPEED).astype(f32)
    radius = float(np.linalg.norm(F.vertices.astype(np.float64), axis=1).max())
    return F, vel, radius


def test_no_path_leaves_a_closed_mesh(fw_path):
    """trace_paths: restitution 1, no friction, no gravity, 8 steps -- after every step every path is within the circumradius + 1e-3
    of the centre (a path that gets through the surface is half a radius outside one step later and never comes back)"""
    F, vel, radius = _sealed_ball()
    settings = S.PathSettings(float(DT), N_STEPS, (0.0, 0.0, 0.0), 0.0, S.ParticleCollisionSettings(1.0, 0.0, False, 1))
    with _system() as system:
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(F.vertices, F.indices))])
        out, smp = system.trace_paths(settings, F.origin, vel, samples=True)
    assert (out["status"] == S.PATH_RUNNING).all() and (out["steps"] == N_STEPS).all()
    assert (out["n_contacts"] >= 2).all(), int(out["n_contacts"].min())
    far = np.linalg.norm(smp[:, :, :3].astype(np.float64), axis=2)
    assert np.isfinite(far).all()
    outside = (far > radius + 1e-3).any(axis=0) | (np.linalg.norm(out["position"].astype(np.float64), axis=1) > radius + 1e-3)
    assert not outside.any(), (int(outside.sum()), np.flatnonzero(outside)[:10], float(far.max()))


def test_no_particle_leaves_a_closed_mesh(fw_path):
    """the same states written into a colliding type with write_particles: after 8 frames nobody is outside -- on every update path"""
    F, vel, radius = _sealed_ball()
    spawner = _still_settings(capacity=1 << 15)
    spawner.particle_settings[0].collision_settings = S.ParticleCollisionSettings(1.0, 0.0, False, 1)
    with _system() as system:
        h = system.spawn(spawner, uid=1)
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(F.vertices, F.indices))])
        h.write_particles(0, _particles(F.origin, vel))
        for _ in range(N_STEPS):
            system.update(DT)
        got = h.particles(0)
    assert len(got) == len(vel)
    far = np.linalg.norm(got["position"].astype(np.float64), axis=1)
    moved = (got["velocity"] != vel).any(axis=1)
    assert np.isfinite(far).all() and moved.all()  # (everybody has bounced)
    assert not (far > radius + 1e-3).any(), (int((far > radius + 1e-3).sum()), float(far.max()))
