"""The ray families of the mesh ray-cast tests: one world (triangle soup, a rotated icosphere, a height field placed twice, an
instance on another layer, analytic colliders on top) and 50k+ rays into it -- random, aimed at vertices and edge midpoints,
starting on a face, axis-parallel, grazing.  tests/test_gpu_mesh.py casts them on the device, tests/test_oracle_mesh_cpu.py in
the C oracle; both compare with tests/mesh_ref.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32


def unit_quat(*q):
    q = np.array(q, dtype=np.float64)
    return tuple(float(x) for x in (q / np.linalg.norm(q)).astype(f32))


def ray_world():
    """the meshes of the ray-cast test: triangle soup, a closed icosphere (rotated), a height field with shared edges and vertices
    placed twice (overlapping: instance ties), and analytic colliders on top (analytic-before-mesh ties)"""
    rng = np.random.default_rng(5)
    soup_v = rng.uniform(-2.5, 2.5, size=(3 * 120, 3)).astype(f32)
    soup_t = np.arange(3 * 120, dtype=np.uint32).reshape(-1, 3)
    ico_v, ico_t = mesh_ref.icosphere(1, 1.25)
    grid_v, grid_t = mesh_ref.grid_mesh(12, 12, extent=5.0, height=lambda x, z: 0.25 * np.sin(1.3 * x) * np.cos(0.9 * z))
    meshes = {"soup": (soup_v, soup_t), "ico": (ico_v, ico_t), "grid": (grid_v, grid_t),
              "grid_flip": (grid_v, grid_t[:, ::-1].copy())}
    placements = [("soup", (0.0, 0.5, 0.0), unit_quat(0.1, 0.2, -0.3, 0.9), 1),
                  ("ico", (3.5, 0.0, -1.0), unit_quat(0.5, -0.1, 0.2, 0.8), 1),
                  ("grid", (0.0, -2.0, 0.0), (0.0, 0.0, 0.0, 1.0), 1),
                  ("grid_flip", (0.0, -2.0, 0.0), (0.0, 0.0, 0.0, 1.0), 1),
                  ("ico", (-3.0, 1.0, 2.0), (0.0, 0.0, 0.0, 1.0), 2)]   # (layer 2: filtered out by a mask of 1)
    analytic = [S.Collider.Sphere((-3.0, 1.0, 2.0), 1.25), S.Collider.Plane((0.0, -2.5, 0.0), (0.0, 1.0, 0.0)),
                S.Collider.Box((3.5, 0.0, -1.0), (0.5, 0.5, 0.5), unit_quat(0.3, 0.0, 0.1, 0.9))]
    return meshes, placements, analytic


def rays(meshes, placements, n_random=30000, seed=9):
    """origins and velocities: random, aimed at vertices and edge midpoints, axis-parallel, grazing, starting on a face"""
    rng = np.random.default_rng(seed)
    dt = 0.05
    pos, vel = [], []

    def unit(n):
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    pos.append(rng.uniform(-5.5, 5.5, size=(n_random, 3)))
    vel.append(unit(n_random) * rng.uniform(1.0, 80.0, size=(n_random, 1)))
    for name, p0, q, _ in placements[:3]:
        v, t = meshes[name]
        qv = np.broadcast_to(np.array(q, dtype=f32), (len(v), 4))
        world_v = (np_sim.quat_mul_vec3(qv, v).astype(np.float64) + np.array(p0))
        tri = world_v[t.astype(np.int64)]
        for targets in (world_v, 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2])):
            k = 2000 // len(targets) + 1
            tg = np.repeat(targets, k, axis=0)
            d = unit(len(tg))
            speed = rng.uniform(5.0, 60.0, size=(len(tg), 1))
            back = rng.uniform(0.05, 0.95, size=(len(tg), 1)) * speed * dt
            pos.append(tg - d * back), vel.append(d * speed)
        # starting on a face: a point of the triangle computed in fp32, any direction
        m = 1500
        ti = rng.integers(0, len(t), m)
        a, b = rng.uniform(0, 1, (2, m))
        sw = a + b > 1
        a[sw], b[sw] = 1 - a[sw], 1 - b[sw]
        on = tri[ti, 0] + a[:, None] * (tri[ti, 1] - tri[ti, 0]) + b[:, None] * (tri[ti, 2] - tri[ti, 0])
        pos.append(on), vel.append(unit(m) * rng.uniform(1.0, 30.0, size=(m, 1)))
    # axis-parallel
    m = 3000
    ax = np.zeros((m, 3))
    ax[np.arange(m), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0], m) * rng.uniform(5.0, 60.0, m)
    pos.append(rng.uniform(-5.0, 5.0, size=(m, 3))), vel.append(ax)
    # grazing the height field: nearly horizontal, just above it
    m = 3000
    xz = rng.uniform(-4.5, 4.5, size=(m, 2))
    hgt = -2.0 + 0.25 * np.sin(1.3 * xz[:, 0]) * np.cos(0.9 * xz[:, 1]) + rng.uniform(1e-4, 2e-2, m)
    g = np.stack([rng.normal(size=m), -rng.uniform(1e-4, 0.05, m), rng.normal(size=m)], 1)
    pos.append(np.stack([xz[:, 0], hgt, xz[:, 1]], 1)), vel.append(g / np.linalg.norm(g, axis=1, keepdims=True) * 20.0)
    return np.concatenate(pos).astype(f32), np.concatenate(vel).astype(f32), f32(dt)
