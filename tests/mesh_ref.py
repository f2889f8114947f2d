"""Brute-force numpy reference for triangle-mesh colliders (include/firework_hip.h: fw_mesh_collider has the semantics).

Every triangle of every instance is tested against every ray -- no hierarchy -- in the header's operation order, numpy
float32 (numpy never fuses a*b+c).  ``cast_ray`` has the signature of ``np_sim.cast_ray`` and merges the two by the
header's tie rule: the nearest hit wins; at equal distance the analytic colliders, then lower instances, then lower
original triangle indices.  ``np_sim.particle_collision`` / ``np_sim.Spawner.update`` look ``cast_ray`` up when they are
called and pass the spawner's ``colliders`` through unchanged, so a test that monkeypatches ``np_sim.cast_ray`` with this one
and hands the spawner a ``World`` gets whole trajectories against meshes.  Because the reference tests every triangle, a
device result that matches it also shows that the device's hierarchy culls conservatively.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field
from typing import List

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_sim  # noqa: E402

f32 = np.float32
ONE, ZERO = f32(1.0), f32(0.0)
_ANALYTIC = np_sim.cast_ray  # (held before any test replaces the module's own)
dot3, cross3, quat_mul_vec3 = np_sim.dot3, np_sim.cross3, np_sim.quat_mul_vec3


class Mesh:
    """A mesh as fw_ctx_create_mesh keeps it: v0, e1 = v1 - v0, e2 = v2 - v0 (fp32), zero-area triangles dropped."""

    def __init__(self, vertices, indices):
        xyz = np.asarray(vertices, dtype=f32).reshape(-1, 3)
        idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
        v0 = xyz[idx[:, 0]]
        e1 = (xyz[idx[:, 1]] - v0).astype(f32)
        e2 = (xyz[idx[:, 2]] - v0).astype(f32)
        c = cross3(e1, e2)
        with np.errstate(over="ignore", invalid="ignore"):
            cc = dot3(c, c)
        keep = np.isfinite(cc) & (cc > 0)
        self.vertices, self.indices = xyz, idx
        self.v0, self.e1, self.e2, self.orig = v0[keep], e1[keep], e2[keep], np.flatnonzero(keep)
        self.ee = (abs1(self.e1) + abs1(self.e2)).astype(f32)  # WATERTIGHT: |e1|_1 + |e2|_1
        with np.errstate(divide="ignore", invalid="ignore"):
            self.normal = (c[keep] * (ONE / np.sqrt(cc[keep]).astype(f32)).astype(f32)[:, None]).astype(f32)


@dataclass
class Instance:
    mesh: Mesh
    position: tuple = (0.0, 0.0, 0.0)
    rotation: tuple = (0.0, 0.0, 0.0, 1.0)
    layers: int = 1


@dataclass
class World:
    colliders: List = field(default_factory=list)   # settings.Collider (np_sim.cast_ray)
    instances: List[Instance] = field(default_factory=list)


WT_K = f32(2.0 ** -21)  # WATERTIGHT: 8 * 2^-24, the margin's factor
WT_CAP = f32(2.0 ** -8)  # ... and its cap


def abs1(a):
    """(|a.x| + |a.y|) + |a.z|, fp32"""
    a = np.abs(a)
    return ((a[..., 0] + a[..., 1]).astype(f32) + a[..., 2]).astype(f32)


def into_frame(inst: Instance, origin, d):
    """the header's FRAME: o = R^-1 (origin - position), d = R^-1 dir; the identity rotation skips both products"""
    q = np.asarray(inst.rotation, dtype=f32)
    pos = np.asarray(inst.position, dtype=f32)
    if q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1:
        return (origin - pos).astype(f32), d.astype(f32)
    qi = np.broadcast_to(np.array([-q[0], -q[1], -q[2], q[3]], dtype=f32), (len(origin), 4))
    return quat_mul_vec3(qi, (origin - pos).astype(f32)), quat_mul_vec3(qi, d)


def cast_instance(inst: Instance, origin, d, max_distance, chunk_elems=1 << 21):
    """-> (hit, t, normal) of the nearest triangle of one instance for each ray (lowest original index on ties)"""
    return cast_instance_full(inst, origin, d, max_distance, chunk_elems)[:3]


def cast_instance_full(inst: Instance, origin, d, max_distance, chunk_elems=1 << 21, watertight=True):
    """-> (hit, t, normal, k): cast_instance and the index k, among the KEPT triangles, of the one that was hit.  watertight=False:
    the header's TRIANGLE without its WATERTIGHT margin (u >= 0, v >= 0, u + v <= 1) -- the rule before the margin, kept so that
    the two can be compared (tests/mesh_exact.py: strict_cast)"""
    n = len(origin)
    q = np.asarray(inst.rotation, dtype=f32)
    aligned = q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1
    ol, dl = into_frame(inst, origin, d)
    m = inst.mesh
    hit = np.zeros(n, dtype=bool)
    best_t = np.full(n, np.inf, dtype=f32)
    best_j = np.zeros(n, dtype=np.int64)
    T = len(m.v0)
    step = max(1, chunk_elems // max(T, 1))
    md = np.asarray(max_distance, dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(0, n, step):
            b = min(n, a + step)
            O, D = ol[a:b, None, :], dl[a:b, None, :]
            p = cross3(np.broadcast_to(D, (b - a, T, 3)), m.e2[None])
            det = dot3(m.e1[None], p)
            inv = (ONE / det).astype(f32)
            s = (O - m.v0[None]).astype(f32)
            u = (dot3(s, p) * inv).astype(f32)
            qv = cross3(s, np.broadcast_to(m.e1[None], s.shape))
            v = (dot3(np.broadcast_to(D, qv.shape), qv) * inv).astype(f32)
            t = (dot3(np.broadcast_to(m.e2[None], qv.shape), qv) * inv).astype(f32)
            mdc = md[a:b, None] if md.ndim else md
            if watertight:
                mg = np.fmin((((WT_K * abs1(s)).astype(f32) * m.ee[None]).astype(f32) * np.abs(inv)).astype(f32), WT_CAP)
            else:
                mg = ZERO
            ok = (det != 0) & (u >= -mg) & (v >= -mg) & ((u + v).astype(f32) <= (ONE + mg).astype(f32)) & (t >= 0) & (t <= mdc)
            tt = np.where(ok, t, f32(np.inf))
            j = np.argmin(tt, axis=1)  # the first minimum: the lowest original index (kept triangles are in input order)
            hit[a:b] = ok.any(axis=1)
            best_t[a:b] = tt[np.arange(b - a), j]
            best_j[a:b] = j
        nrm = m.normal[best_j]
        if not aligned:
            nrm = quat_mul_vec3(np.broadcast_to(q, (n, 4)), nrm)
        flip = dot3(nrm, d) > 0
        nrm = np.where(flip[:, None], (-nrm).astype(f32), nrm).astype(f32)
    return hit, best_t, nrm, best_j


def cast_ray(world, mask, origin, d, max_distance):
    """np_sim.cast_ray over a World (analytic colliders, then mesh instances) -- or a plain collider list"""
    if not isinstance(world, World):
        return _ANALYTIC(world, mask, origin, d, max_distance)
    found, best_t, best_n = _ANALYTIC(world.colliders, mask, origin, d, max_distance)
    for inst in world.instances:
        if not (int(inst.layers) & int(mask)):
            continue
        hit, t, nrm = cast_instance(inst, origin, d, max_distance)
        better = hit & (~found | (t < best_t))
        best_t = np.where(better, t, best_t).astype(f32)
        best_n = np.where(better[:, None], nrm, best_n).astype(f32)
        found |= hit
    return found, best_t, best_n


# ---- meshes the tests use -----------------------------------------------------------------------------------------------
def box_mesh(half_extents):
    """the 12 triangles of an axis-aligned box around the origin (outward winding)"""
    hx, hy, hz = (float(h) for h in half_extents)
    v = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], dtype=f32)
    # vertex index = 4 * (x > 0) + 2 * (y > 0) + (z > 0)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, c, e in quads:
        tris += [(a, b, c), (a, c, e)]
    return v, np.array(tris, dtype=np.uint32)


def grid_mesh(nx, nz, extent=4.0, height=None, y=0.0):
    """a height field of nx * nz cells over [-extent, extent]^2 (two triangles per cell, shared vertices and edges)"""
    xs = np.linspace(-extent, extent, nx + 1, dtype=np.float64)
    zs = np.linspace(-extent, extent, nz + 1, dtype=np.float64)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    Y = np.full_like(X, y) if height is None else height(X, Z)
    v = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(f32)
    i = np.arange((nx + 1) * (nz + 1)).reshape(nx + 1, nz + 1)
    a, b, c, e = i[:-1, :-1].ravel(), i[1:, :-1].ravel(), i[1:, 1:].ravel(), i[:-1, 1:].ravel()
    tris = np.concatenate([np.stack([a, e, c], 1), np.stack([a, c, b], 1)]).astype(np.uint32)
    return v, tris


def icosphere(subdiv=2, radius=1.0):
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(f32), np.array(f, dtype=np.uint32)


def tie_meshes():
    """two surfaces through the point (0, 0, -0.5) that a ray from (0, 1, -0.5) straight down meets at t = 1 exactly (all
    operands exact in fp32): a triangle tilted onto the plane y = x, whose normal turned to the ray is (-1, 1, 0) / sqrt(2), and a
    flat quad in y = 0 (normal (0, 1, 0)) -- the same distance, different normals: which one won is visible"""
    tilted_v = np.array([[-1, -1, -1], [1, 1, -1], [-1, -1, 1]], dtype=f32)
    flat_v = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=f32)
    tilted_t = np.array([[0, 1, 2]], dtype=np.uint32)
    flat_t = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    both_v = np.concatenate([tilted_v, flat_v])
    tilted_first = (both_v, np.concatenate([tilted_t, flat_t + 3]))
    flat_first = (both_v, np.concatenate([flat_t + 3, tilted_t]))
    return (tilted_v, tilted_t), (flat_v, flat_t), tilted_first, flat_first


TILTED_N = np.array([-1, 1, 0], dtype=f32) * f32(1 / np.sqrt(2))
