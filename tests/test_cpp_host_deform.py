"""The `deform` scenario of examples/mirror_check.cpp -- the scenario of tests/test_cpp_host.py with its two meshes created
deformable and their vertices moved every fifth frame through include/firework.hpp (create_deformable_mesh /
update_mesh_vertices) -- against the same calls through the Python mirror: the same library, so every digest must be identical."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_host import ROOT, _fnv, _run_both_mirrors, build  # noqa: E402


def _python_mirror_lines():
    """the scenario of test_cpp_host._run_both_mirrors(True) with the deformable calls of `mirror_check deform`"""
    import numpy as np

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    f32 = np.float32
    seen = [0]
    p0 = S.ParticleSettings(lifetime=S.RandF32.constant(0.4), initial_scale=S.RandF32(0.5, 2.0),
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]),
                            base_color=S.FireworkGradient.uneven_samples([(0.0, (10, 7, 1, 1)), (0.7, (3, 1, 1, 1)),
                                                                          (1.0, (0.1, 0.1, 0.1, 0))]),
                            linear_drag=0.3, particles_destroyed=lambda dead: seen.__setitem__(0, seen[0] + len(dead)))
    p1 = S.ParticleSettings(lifetime=S.RandF32(0.2, 0.6), acceleration=(0.0, 0.5, 0.0),
                            scale_curve=S.FireworkCurve.uneven_samples([(0.0, 1.0), (0.8, 1.2), (1.0, 0.0)]),
                            emissive_color=S.FireworkGradient.even_samples([(4, 2, 0, 1), (0, 0, 0, 1)]),
                            angular_drag=0.1, angular_acceleration=(0.1, 0.0, -0.2))
    p2 = S.ParticleSettings(lifetime=S.RandF32(0.5, 0.9), pbr=True,
                            collision_settings=S.ParticleCollisionSettings(0.6, 0.2, False, 3))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(5000.0),
                            emission_shape=S.EmissionShape.Sphere(0.5),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.0),
                            initial_velocity_radial=S.RandF32(1.0, 2.0))
    e1 = S.EmissionSettings(particle_index=1, emission_pacing=S.EmissionPacing.CountOverDuration(8.0, 1.0, 0.1, 0.9),
                            emission_mode=S.EmissionMode.Nested(0), inherit_parent_velocity=False)
    e2 = S.EmissionSettings(particle_index=2, emission_pacing=S.EmissionPacing.OnDemand(),
                            emission_shape=S.EmissionShape.Circle((0.0, 0.0, 1.0), 2.0),
                            initial_velocity=S.RandVec3(S.RandF32(0.0, 3.0), (0.0, -1.0, 0.0), 0.0),
                            initial_rotation=(0.0, 0.38941834, 0.0, 0.92106099))
    e3 = S.EmissionSettings(particle_index=2, emission_pacing=S.EmissionPacing.OneShot(700))
    ramp_v = lambda y: np.array([[-2.0, -0.25, -2.0], [2.0, -0.25, -2.0], [2.0, y, 2.0], [-2.0, y, 2.0]], dtype=f32)  # noqa: E731
    sheet_v = lambda y: np.array([[-3.0, 0.0, -3.0], [3.0, 0.0, -3.0], [0.0, y, 3.0]], dtype=f32)  # noqa: E731
    lines = []
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ps.track_aabbs(True)
        ps.set_colliders([S.Collider.Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), S.Collider.Sphere((1.0, 0.5, 0.0), 0.75, 2),
                          S.Collider.Box((-2.0, 0.0, 0.0), (0.5, 1.0, 0.5), (0.0, 0.38268343, 0.0, 0.92387953))])
        ramp = ps.create_deformable_mesh(ramp_v(0.25), np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32))
        ps.set_mesh_colliders([S.MeshCollider(ramp, (0.0, -0.25, 0.0), (0.0, 0.0, 0.0, 1.0), 1),
                               S.MeshCollider(ramp, (0.5, 0.25, 0.0), (0.0, 0.38268343, 0.0, 0.92387953), 2)])
        d = ps.spawn(S.ParticleSpawner([p0, p1, p2], [e0, e1, e2, e3]), S.Transform((0.0, 1.0, 0.0)), uid=42,
                     modifier=S.EffectModifier(2.0, 0.5))
        d.set_parent_velocity((0.5, 0.0, -0.25))
        dt = f32(1.0 / 60.0)
        sheet = None
        for fr in range(60):
            if fr in (0, 7, 8, 31):
                d.queue_particles(500 + 10 * fr)
            if fr % 5 == 0 and fr < 30:
                ps.update_mesh_vertices(ramp, ramp_v(0.25 + 0.125 * (fr // 5)))
            if fr % 5 == 0 and fr > 30:
                ps.update_mesh_vertices(sheet, sheet_v(0.5 + 0.25 * (fr // 5 - 6)))
            if fr == 30:
                sheet = ps.create_deformable_mesh(sheet_v(0.5), np.array([[0, 2, 1]], dtype=np.uint32))
                ps.set_mesh_colliders([S.MeshCollider(sheet, (1.0, 1.5, 3.0), (0.0, 0.0, 0.19509032, 0.98078528), 3)])
                ps.destroy_mesh(ramp)
            if fr == 20:
                d.set_transform(S.Transform((1.0, 2.0, 3.0), (0.0, 0.0, 0.38268343, 0.92387953)))
            ps.update(dt)
            if fr % 10 != 9:
                continue
            c = d.counts()
            digests = " ".join(f"{_fnv(d.particles(t).tobytes()):016x}" for t in range(3))
            any_, mn, mx = d.aabb()
            box = np.concatenate([mn, mx]).astype(f32).tobytes()
            lines.append(f"frame {fr} counts {c[0]} {c[1]} {c[2]} {digests} aabb {int(any_)} {_fnv(box):016x} "
                         f"active {int(d.active())}")
    lines.append(f"destroyed reported {seen[0]}")
    return lines


def test_mirror_check_knows_the_deform_scenario():
    """(no GPU) the example builds against the header's new calls and its source has the scenario"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"deform"' in src and "create_deformable_mesh(" in src and "update_mesh_vertices(" in src


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_deform_meshes_identically():
    """`mirror_check deform` against the Python mirror: identical lines; and the deformation matters -- the counts are those of
    the `mesh` scenario (a bounce destroys nothing) while the pebbles' digests under the moved ramp (frame 29) and under the
    moved sheet (frame 59) differ from it.  The `mesh` and no-argument scenarios themselves are tests/test_cpp_host.py's."""
    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "deform"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines = _python_mirror_lines()
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    static = _run_both_mirrors(True)
    assert [ln.split()[:6] for ln in cpp_lines] == [ln.split()[:6] for ln in static]
    for k in (2, 5):
        assert cpp_lines[k].split()[8] != static[k].split()[8], (cpp_lines[k], static[k])
