"""The capsule collider (include/firework_hip.h: CAPSULE under fw_collider) in numpy float32, vectorised over rays, written from
the header's text -- INSIDE, ENTRY (lateral, bottom cap, top cap, strict <), NORMAL, the identity-rotation shortcut -- and not
from csrc/fw_collide.h; and a cast_ray with np_sim.cast_ray's signature for worlds that mix capsules with the kinds np_sim
knows.  A helper, not a test: tests that need whole frames put cast_ray in np_sim.cast_ray's place with monkeypatch, so that
np_sim.particle_collision and np_sim.Spawner run unchanged.

The same functions take float64 arrays (dtype=np.float64): the definition evaluated in double precision, which
tests/test_capsule_cpu.py holds against the geometry of a capsule."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import np_sim  # noqa: E402

f32 = np.float32
COLLIDER_CAPSULE = 5
_ANALYTIC = np_sim.cast_ray  # (held before any test puts cast_ray below in its place)


def _dot(a, b, ft):  # the header's dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z
    m = lambda p, q: (p * q).astype(ft)  # noqa: E731
    return ((m(a[0], b[0]) + m(a[1], b[1])).astype(ft) + m(a[2], b[2])).astype(ft)


def _quat_mul_vec3(q, v, ft):
    """Quat * Vec3 as every framed kind rotates: v (w^2 - b.b) + b (2 v.b) + (b x v) (2 w), columns of arrays"""
    m = lambda p, r: (p * r).astype(ft)  # noqa: E731
    b = [ft(q[0]), ft(q[1]), ft(q[2])]
    w = ft(q[3])
    b2 = ft(ft(ft(b[0] * b[0]) + ft(b[1] * b[1])) + ft(b[2] * b[2]))
    k0 = ft(ft(w * w) - b2)
    k1 = (_dot(v, b, ft) * ft(2.0)).astype(ft)
    c = [(m(b[1], v[2]) - m(v[1], b[2])).astype(ft), (m(b[2], v[0]) - m(v[2], b[0])).astype(ft), (m(b[0], v[1]) - m(v[0], b[1])).astype(ft)]
    k2 = ft(w * ft(2.0))
    return [((m(v[i], k0) + m(b[i], k1)).astype(ft) + m(c[i], k2)).astype(ft) for i in range(3)]


def cast_capsule(c, origin, d, max_distance, dtype=f32):
    """one capsule against rays origin[n, 3] + t d[n, 3], t in [0, max_distance[n]] -> (hit[n], t[n], normal[n, 3]), every operation
    rounded to `dtype`"""
    ft = dtype
    m = lambda p, r: (p * r).astype(ft)  # noqa: E731
    origin, d, md = np.asarray(origin, dtype=ft), np.asarray(d, dtype=ft), np.asarray(max_distance, dtype=ft)
    n = len(origin)
    pos = np.asarray(c.position, dtype=f32).astype(ft)
    q = np.asarray(c.rotation, dtype=f32).astype(ft)
    hl = ft(f32(c.half_extents[1]))
    r = ft(f32(c.radius))
    rr = ft(r * r)
    with np.errstate(all="ignore"):
        rel = [(origin[:, i] - pos[i]).astype(ft) for i in range(3)]
        dd = [d[:, i] for i in range(3)]
        aligned = q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1
        if aligned:  # the identity rotation skips both products
            o, dl = rel, dd
        else:
            qi = [-q[0], -q[1], -q[2], q[3]]
            o, dl = _quat_mul_vec3(qi, rel, ft), _quat_mul_vec3(qi, dd, ft)
        # INSIDE
        yc = np.where(o[1] < -hl, -hl, np.where(o[1] > hl, hl, o[1])).astype(ft)
        dy = (o[1] - yc).astype(ft)
        xz = (m(o[0], o[0]) + m(o[2], o[2])).astype(ft)
        inside = ((xz + m(dy, dy)).astype(ft) - rr).astype(ft) <= 0
        # ENTRY: lateral, bottom cap, top cap; a later piece replaces an earlier one only when strictly nearer
        best = np.full(n, np.inf, dtype=ft)
        cy_best = np.zeros(n, dtype=ft)
        piece = np.full(n, -1, dtype=np.int64)
        a = (m(dl[0], dl[0]) + m(dl[2], dl[2])).astype(ft)
        b = (m(o[0], dl[0]) + m(o[2], dl[2])).astype(ft)
        c2 = (xz - rr).astype(ft)
        disc = (m(b, b) - m(a, c2)).astype(ft)
        t = (((-b).astype(ft) - np.sqrt(disc).astype(ft)).astype(ft) / a).astype(ft)
        y = (o[1] + m(dl[1], t)).astype(ft)
        ok = (a != 0) & (disc >= 0) & (t >= 0) & (np.abs(y) <= hl)
        best = np.where(ok, t, best).astype(ft)
        piece = np.where(ok, 0, piece)
        A = _dot(dl, dl, ft)
        for k, cy in ((1, ft(-hl)), (2, hl)):
            w = [o[0], (o[1] - cy).astype(ft), o[2]]
            B = _dot(w, dl, ft)
            C = (_dot(w, w, ft) - rr).astype(ft)
            delta = (m(B, B) - m(A, C)).astype(ft)
            t = (((-B).astype(ft) - np.sqrt(delta).astype(ft)).astype(ft) / A).astype(ft)
            y = (o[1] + m(dl[1], t)).astype(ft)
            ok = ~(B > 0) & (delta >= 0) & (t >= 0) & ((y <= -hl) if k == 1 else (y >= hl)) & (t < best)
            best = np.where(ok, t, best).astype(ft)
            piece = np.where(ok, k, piece)
            cy_best = np.where(ok, cy, cy_best).astype(ft)
        entered = ~inside & (piece >= 0) & (best <= md)
        # NORMAL
        p = [(o[i] + m(dl[i], best)).astype(ft) for i in range(3)]
        v = [p[0], np.where(piece == 0, ft(0.0), (p[1] - cy_best).astype(ft)).astype(ft), p[2]]
        inv = (ft(1.0) / np.sqrt(_dot(v, v, ft)).astype(ft)).astype(ft)
        nl = [m(v[i], inv) for i in range(3)]
        nw = nl if aligned else _quat_mul_vec3(q, nl, ft)
        hit = inside | entered
        dist = np.where(inside, ft(0.0), best).astype(ft)
        nrm = np.where(entered[:, None], np.stack(nw, axis=1), ft(0.0)).astype(ft)
    return hit, dist, nrm


def _members(world):
    """(analytic colliders, mesh instances) of a plain collider list or of a mesh_ref.World"""
    if hasattr(world, "instances"):
        return list(world.colliders), list(world.instances)
    return list(world), []


def cast_ray_identity(world, mask, origin, d, max_distance):
    """the nearest `solid = true` hit over a set that may hold capsules -- a list of settings.Collider, or a mesh_ref.World whose
    instances follow the analytic colliders -> (found, distance, normal, kind, index).  Every member is cast ALONE, in index order
    (kinds 0-4 by np_sim, kind 5 above, an instance by mesh_ref.cast_instance), and a hit is kept only when strictly nearer: the
    product's tie rule, which also says WHO holds the hit (kind 1 a collider, 2 a mesh instance, 0 nobody; index -1 for nobody)"""
    origin, d = np.asarray(origin, dtype=f32), np.asarray(d, dtype=f32)
    n = len(origin)
    md = np.broadcast_to(np.asarray(max_distance, dtype=f32), (n,))
    best_t = np.full(n, np.inf, dtype=f32)
    best_n = np.zeros((n, 3), dtype=f32)
    kind = np.zeros(n, dtype=np.int32)
    index = np.full(n, -1, dtype=np.int64)
    colliders, instances = _members(world)
    members = [(1, i, c) for i, c in enumerate(colliders)] + [(2, i, m) for i, m in enumerate(instances)]
    for k, i, c in members:
        if not (int(c.layers) & int(mask)):
            continue
        if k == 2:
            import mesh_ref

            hit, t, nrm = mesh_ref.cast_instance(c, origin, d, md)
        elif c.kind == COLLIDER_CAPSULE:
            hit, t, nrm = cast_capsule(c, origin, d, md)
        else:
            hit, t, nrm = _ANALYTIC([c], mask, origin, d, md.copy())
        better = hit & ((kind == 0) | (t < best_t))
        best_t = np.where(better, t, best_t).astype(f32)
        best_n = np.where(better[:, None], nrm, best_n).astype(f32)
        kind = np.where(better, k, kind).astype(np.int32)
        index = np.where(better, i, index)
    return kind != 0, best_t, best_n, kind, index


def cast_ray(world, mask, origin, d, max_distance):
    """np_sim.cast_ray's signature and result for such a set: what tests put in np_sim.cast_ray's place"""
    return cast_ray_identity(world, mask, origin, d, max_distance)[:3]
