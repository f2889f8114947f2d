"""The pinned staging slots of the collider world (fw_engine.h: Fence, Staging) through the public API: a set that is replaced five times
in a row, with no step and no synchronisation in between, wraps its two slots twice -- every call from the third on finds the fence of its
slot pending -- and crosses a growth of the staging and of the device table on the way.  What the device then sees must be the LAST set
and nothing else: every case compares, byte for byte, with a second context that only ever received that one.  The results are
deterministic; the cases catch a wrong slot, a turn used up by a refused call, a fence forgotten on growth and a table read from the wrong
buffer (they cannot prove the absence of a race, and do not try to provoke one).  Product defaults, one run each.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from mesh_rays import unit_quat  # noqa: E402
from test_gpu_mesh import SEED, _particles, _still_settings  # noqa: E402
from test_gpu_mesh_deform import deform  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
DT = f32(1.0 / 60.0)


def _system():
    from bevy_firework_amd.system import ParticleSystem

    return ParticleSystem(device=0, seed=SEED)


def _rays(n_side=40, extent=2.4):
    """a fixed batch: a grid of origins above the world, pointing down and a little sideways"""
    x, z = np.meshgrid(np.linspace(-extent, extent, n_side), np.linspace(-extent, extent, n_side))
    rays = np.zeros(x.size, dtype=S.RAY_DTYPE)
    rays["origin"] = np.stack([x.ravel(), np.full(x.size, 3.0), z.ravel()], axis=1)
    d = np.stack([0.07 * np.sin(3.0 * x.ravel()), np.full(x.size, -1.0), 0.05 * np.cos(2.0 * z.ravel())], axis=1)
    rays["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["max_distance"], rays["filter_mask"] = 10.0, 0xFFFFFFFF
    return rays


def _collider_sets():
    """five different sets; the fourth holds 70 colliders: past the 64 entries the staging slots and the device table start with"""
    ball = lambda k, y=0.0: S.Collider.Sphere((-2.0 + 0.06 * k, y, 0.3 * np.sin(1.0 * k)), 0.25)  # noqa: E731
    return [[S.Collider.Plane((0.0, 0.3, 0.0), (0.0, 1.0, 0.0))],
            [S.Collider.Box((0.0, 0.0, 0.0), (1.5, 0.2, 1.5)), ball(3, 0.4)],
            [ball(k, 0.2) for k in range(9)],
            [ball(k, 0.1) for k in range(70)],
            [S.Collider.Plane((0.0, 0.15, 0.0), (0.1, 1.0, 0.0))] + [ball(k) for k in range(0, 66, 6)]]


def test_collider_sets_replaced_in_a_row():
    sets = _collider_sets()
    assert len(sets) == 5 and len(sets[3]) == 70 and len({len(s) for s in sets}) == 5
    rng = np.random.default_rng(11)
    n = 400
    pos = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(0.3, 0.7, n), rng.uniform(-1.0, 1.0, n)], axis=1).astype(f32)
    vel = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-6.0, -3.0, n), rng.uniform(-0.5, 0.5, n)], axis=1).astype(f32)
    parts = _particles(pos, vel)

    def run(given, destroy):
        out = []
        with _system() as system:
            h = system.spawn(_still_settings(destroy=destroy, report=True), uid=1)
            h.write_particles(0, parts)
            for s in given:
                system.set_colliders(s)
            for _ in range(6):
                system.update(DT)
                out.append((h.counts(), h.particles(0).tobytes(), h.destroyed(0).tobytes()))
            return out, h.particles(0)

    for destroy in (True, False):
        got, last = run(sets, destroy)
        want, _ = run(sets[-1:], destroy)
        for fr, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0], (destroy, fr, g[0], w[0])
            assert g[1] == w[1], (destroy, fr, "particles")
            assert g[2] == w[2], (destroy, fr, "destroyed records")
        if destroy:  # (the world was met: some particles died on it, some are still falling)
            assert 50 < len(last) < n - 50, len(last)
            assert sum(len(g[2]) for g in got) > 0
        else:
            assert 50 < int((last["velocity"][:, 1] > 0).sum()), "bounces"


def _mesh_sets(a, b):
    """five different instance sets over two meshes; the fourth places 20 instances: past the 16 entries the staging slots and the
    device table start with"""
    row = lambda m, k, y: S.MeshCollider(m, (-2.2 + 0.23 * k, y, 0.2 * np.cos(1.0 * k)), unit_quat(0.0, 0.05 * k, 0.0, 1.0))  # noqa: E731
    return [[S.MeshCollider(a)],
            [S.MeshCollider(b, (0.0, 0.5, 0.0)), S.MeshCollider(a, (0.3, -0.2, 0.0))],
            [row(a, k, 0.4) for k in range(5)],
            [row(a if k % 3 else b, k, 0.05 * k) for k in range(20)],
            [row(b, 2 * k, -0.3) for k in range(7)] + [S.MeshCollider(a, (0.0, 0.6, 0.1), unit_quat(0.1, 0.0, 0.0, 1.0))]]


def test_mesh_instance_sets_replaced_in_a_row():
    va, ta = mesh_ref.grid_mesh(4, 4, extent=1.2, height=lambda x, z: 0.2 * np.sin(2.0 * x) * np.cos(1.5 * z))
    vb, tb = mesh_ref.grid_mesh(3, 5, extent=0.8, height=lambda x, z: 0.1 * x - 0.2 * z)
    rays = _rays()

    def run(which):
        with _system() as system:
            a, b = system.create_mesh(va, ta), system.create_mesh(vb, tb)
            sets = _mesh_sets(a, b)
            assert len(sets) == 5 and len(sets[3]) == 20
            for s in (sets if which is None else sets[which:which + 1]):
                system.set_mesh_colliders(s)
            return system.cast_ray_records(rays)

    got, want = run(None), run(4)
    assert got.tobytes() == want.tobytes()
    assert (got["kind"] == S.HIT_MESH).sum() > 100
    assert got.tobytes() != run(3).tobytes()  # (the rays tell the sets apart)


def test_vertex_updates_in_a_row_with_a_refused_one():
    """five fw_ctx_update_mesh_vertices on a placed deformable mesh; the third carries a non-finite vertex, is refused (FW_EINVAL) and
    must not use up its slot's turn.  The hits equal those of a mesh created from the last accepted vertices, bit for bit: the rule of
    tests/test_gpu_mesh_deform.py for a refit against a build"""
    from bevy_firework_amd.system import FwError

    v, t = mesh_ref.grid_mesh(4, 4, extent=2.0, height=lambda x, z: 0.3 * np.sin(1.1 * x) * np.cos(0.7 * z))
    assert 24 <= len(t) <= 64
    place = lambda m: [S.MeshCollider(m, (0.1, -0.3, 0.0), unit_quat(0.05, 0.3, -0.1, 0.9))]  # noqa: E731
    rays = _rays(extent=1.8)
    shapes, w = [], v
    for k in range(1, 6):
        w = deform(w, 0.05 * k)
        shapes.append(w)
    shapes[2] = shapes[2].copy()
    shapes[2][7, 1] = np.nan
    with _system() as system:
        m = system.create_deformable_mesh(v, t)
        system.set_mesh_colliders(place(m))
        for k, xyz in enumerate(shapes):
            if k == 2:
                with pytest.raises(FwError) as e:
                    system.update_mesh_vertices(m, xyz)
                assert e.value.status == FW_EINVAL
            else:
                system.update_mesh_vertices(m, xyz)
        got = system.cast_ray_records(rays)
    with _system() as system:
        system.set_mesh_colliders(place(system.create_mesh(shapes[4], t)))
        want = system.cast_ray_records(rays)
        system.set_mesh_colliders(place(system.create_mesh(shapes[3], t)))
        before = system.cast_ray_records(rays)
    assert got.tobytes() == want.tobytes()
    assert (got["kind"] == S.HIT_MESH).sum() > 100 and want.tobytes() != before.tobytes()
