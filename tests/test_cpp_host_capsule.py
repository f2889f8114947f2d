"""The `capsule` scenario of examples/mirror_check.cpp -- a small fixed world of capsules built with both constructors of
include/firework.hpp (Collider::capsule, Collider::capsule_endpoints), a colliding spawner above it and a batch of rays every tenth
frame -- against the same calls through the Python mirror (settings.Collider.Capsule / CapsuleEndpoints): the same library, so every
digest must be identical.  A constructor that marshals a capsule differently in the two mirrors (the arc of the endpoint form, half
the segment against half the height) moves the bounces and the hit records."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_host import ROOT, _fnv, build  # noqa: E402


def _python_mirror_lines():
    import numpy as np

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    f32 = np.float32
    world = [S.Collider.Box((0.0, -0.5, 0.0), (4.0, 0.5, 4.0)),
             S.Collider.Capsule((0.25, 0.875, 0.125), 0.375, 1.0),
             S.Collider.Capsule((-0.75, 1.0, 0.5), 0.25, 1.5, (0.30151135, 0.0, 0.30151135, 0.90453404), 3),
             S.Collider.CapsuleEndpoints((-1.0, 0.25, -1.0), (1.5, 0.5, -0.375), 0.1875),
             S.Collider.CapsuleEndpoints((1.0, 2.0, 1.0), (1.125, 0.75, 1.0), 0.125, 2),
             S.Collider.CapsuleEndpoints((2.0, 0.5, 0.0), (2.0, 0.5, 0.0), 0.5)]
    ps0 = S.ParticleSettings(lifetime=S.RandF32.constant(0.75), linear_drag=0.125,
                             collision_settings=S.ParticleCollisionSettings(0.5, 0.25, False, 1))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(2000.0), emission_shape=S.EmissionShape.Sphere(0.75),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, -1.0, 0.0), 0.0))
    i = np.arange(256)
    rays = np.zeros(256, dtype=S.RAY_DTYPE)
    rays["origin"][:, 0] = f32(-2.0) + (i % 16).astype(f32) * f32(0.25)
    rays["origin"][:, 1] = 3.0
    rays["origin"][:, 2] = f32(-1.5) + (i // 16).astype(f32) * f32(0.1875)
    rays["max_distance"] = 6.0
    rays["dir"][:, 0] = np.where(i % 2, f32(0.6), f32(0.0))
    rays["dir"][:, 1] = np.where(i % 2, f32(-0.8), f32(-1.0))
    rays["filter_mask"] = 1 + i % 3
    lines = []
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ps.set_colliders(world)
        d = ps.spawn(S.ParticleSpawner([ps0], [e0]), S.Transform((0.25, 3.0, 0.125)), uid=7)
        dt = f32(1.0 / 60.0)
        for fr in range(40):
            ps.update(dt)
            if fr % 10 != 9:
                continue
            hits = ps.cast_ray_records(rays)
            per = [int(((hits["kind"] == S.HIT_COLLIDER) & (hits["index"] == k)).sum()) for k in range(6)]
            lines.append(f"frame {fr} count {d.counts()[0]} {_fnv(d.particles(0).tobytes()):016x} hits {' '.join(str(p) for p in per)} "
                         f"{_fnv(hits.tobytes()):016x}")
    return lines


def test_mirror_check_knows_the_capsule_scenario():
    """(no GPU) the example builds against the header's constructors and its source has the scenario"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"capsule"' in src and "Collider::capsule(" in src and "Collider::capsule_endpoints(" in src


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_place_capsules_identically():
    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "capsule"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines = _python_mirror_lines()
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    last = cpp_lines[-1].split()
    assert len(cpp_lines) == 4 and int(last[3]) > 1000
    assert all(int(x) > 0 for x in last[6:12]), last  # (the slab and every capsule stop some ray)
    assert len({ln.split()[4] for ln in cpp_lines}) == 4  # (the particles move)
