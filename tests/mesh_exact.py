"""The geometry the mesh ray cast is held to (include/firework_hip.h: fw_mesh_collider, WATERTIGHT) -- a helper, not a test.

Everything the other mesh references hold is the header's rule restated in fp32: they prove that the device computes what the header
says.  This file asks whether the rule is right: a float64 Moeller-Trumbore over every triangle of the placed mesh (products of fp32
values are exact in float64, so its rounding is ten orders below the fp32 cast's), the distance from a point or a segment to a
triangle, the rule as it stood before the margin (`strict_cast`), and the ray families that find the rays which used to pass between
two triangles: aimed at vertices and along edges, from inside a closed surface and from 4 and 16 times the mesh's size away.
numpy only; every family comes from a fixed seed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402

f32, f64 = np.float32, np.float64
MARGIN = 1e-9


# ---- float64 geometry ------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def rotate(q, v):
    """glam's Quat * Vec3 (np_sim.quat_mul_vec3's expression) in float64, on the quaternion's fp32 components as they are"""
    q = np.asarray(q, dtype=f32).astype(f64)
    b, w = q[:3], q[3]
    v = np.asarray(v, dtype=f64)
    return v * (w * w - b @ b) + b * (2.0 * (v @ b))[..., None] + np.cross(b, v) * (2.0 * w)


def placed_triangles(vertices, indices, position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0)):
    """(T, 3, 3) float64: the world-space corners of every triangle of non-zero area, and their original indices"""
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3).astype(f64)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    w = rotate(rotation, v) + np.asarray(position, dtype=f32).astype(f64)
    tri = w[idx]
    area2 = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    keep = area2 > 0
    return tri[keep], np.flatnonzero(keep)


def _uvt(tri, o, d):
    """Moeller-Trumbore of every ray against every triangle -> u, v, t, det of shape (n, T).  The triple products are expanded into
    matrix products (w = o x d per ray): u det = e2.w - d.(e2 x v0), v det = -e1.w - d.(v0 x e1), t det = (o - v0).(e1 x e2),
    det = -d.(e1 x e2)"""
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    w = np.cross(o, d)
    det = -(d @ nrm.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        u = (w @ e2.T - d @ np.cross(e2, v0).T) * inv
        v = (-(w @ e1.T) - d @ np.cross(v0, e1).T) * inv
        t = (o @ nrm.T - _dot(v0, nrm)[None]) * inv
    return u, v, t, det


def nearest_crossing(tri, origin, direction, max_distance, margin=MARGIN, chunk=20000):
    """the nearest crossing of each ray origin + t direction, 0 <= t <= max_distance, with the triangles `tri` (placed_triangles):
    -> (t, k) float64 / int64, t = inf and k = -1 where there is none.  Every triangle is tested, in float64, with `margin` on the
    barycentric coordinates (a ray exactly through a shared edge meets both of its triangles)"""
    o, d = np.asarray(origin, dtype=f64), np.asarray(direction, dtype=f64)
    md = np.broadcast_to(np.asarray(max_distance, dtype=f64), (len(o),))
    best_t, best_k = np.full(len(o), np.inf), np.full(len(o), -1, dtype=np.int64)
    for a in range(0, len(o), chunk):
        b = min(len(o), a + chunk)
        u, v, t, det = _uvt(tri, o[a:b], d[a:b])
        ok = (det != 0) & (u >= -margin) & (v >= -margin) & (u + v <= 1 + margin) & (t >= 0) & (t <= md[a:b, None])
        tt = np.where(ok, t, np.inf)
        k = np.argmin(tt, axis=1)
        best_t[a:b] = tt[np.arange(b - a), k]
        best_k[a:b] = np.where(ok.any(axis=1), k, -1)
    return best_t, best_k


def inside_silhouette(tri, origin, direction, offset, chunk=20000):
    """True where the ray's LINE passes at least `offset` inside the silhouette of the mesh: each of the eight parallel lines at
    that distance from it (45 degrees apart) crosses some triangle too"""
    o, d = np.asarray(origin, dtype=f64), np.asarray(direction, dtype=f64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    helper = np.where((np.abs(d[:, 0]) < 0.6)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    a1 = np.cross(d, helper)
    a1 /= np.linalg.norm(a1, axis=1, keepdims=True)
    a2 = np.cross(d, a1)
    ok = np.ones(len(o), dtype=bool)
    for k in range(8):
        shift = (np.cos(k * np.pi / 4) * a1 + np.sin(k * np.pi / 4) * a2) * offset
        for a in range(0, len(o), chunk):
            b = min(len(o), a + chunk)
            u, v, _, det = _uvt(tri, o[a:b] + shift[a:b], d[a:b])
            ok[a:b] &= ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)).any(axis=1)
    return ok


def _point_segment(p, a, b):
    ab = b - a
    s = np.clip(_dot(p - a, ab) / _dot(ab, ab), 0.0, 1.0)
    return np.linalg.norm(p - (a + ab * s[..., None]), axis=-1)


def point_triangle_distance(p, tri):
    """the distance from each point p[...] to the closest point of its triangle tri[..., 3, 3] (they broadcast), float64"""
    p, tri = np.asarray(p, dtype=f64), np.asarray(tri, dtype=f64)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    w = p - a
    # barycentric coordinates of the projection onto the plane
    u = _dot(np.cross(w, c - a), n) / nn
    v = _dot(np.cross(b - a, w), n) / nn
    inside = (u >= 0) & (v >= 0) & (u + v <= 1)
    plane = np.abs(_dot(w, n)) / np.sqrt(nn)
    edges = np.minimum(np.minimum(_point_segment(p, a, b), _point_segment(p, b, c)), _point_segment(p, c, a))
    return np.where(inside, plane, edges)


def _segment_segment(p1, q1, p2, q2):
    """the distance between the segments p1 q1 and p2 q2 (neither of length zero)"""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    den = a * e - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0, np.clip((b * f - c * e) / den, 0.0, 1.0), 0.0)
        t = (b * s + f) / e
        s = np.where(t < 0, np.clip(-c / a, 0.0, 1.0), np.where(t > 1, np.clip((b - c) / a, 0.0, 1.0), s))
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm((p1 + d1 * s[..., None]) - (p2 + d2 * t[..., None]), axis=-1)


def segment_triangle_distance(origin, direction, max_distance, tri):
    """the distance from the segment origin + t direction, 0 <= t <= max_distance, to each triangle -- for segments that do NOT
    cross the triangle (a crossing one is at distance 0, which this does not look for): the nearer of its two ends and of the
    triangle's three edges.  origin (n, 3) against tri (T, 3, 3) -> (n, T)"""
    o = np.asarray(origin, dtype=f64)[:, None, :]
    e = o + np.asarray(direction, dtype=f64)[:, None, :] * np.asarray(max_distance, dtype=f64).reshape(-1, 1, 1)
    T = np.asarray(tri, dtype=f64)[None]
    best = np.minimum(point_triangle_distance(o, T), point_triangle_distance(e, T))
    for i, j in ((0, 1), (1, 2), (2, 0)):
        best = np.minimum(best, _segment_segment(o, e, T[..., i, :], T[..., j, :]))
    return best


def triangle_scale(origin, tri):
    """|o - v0| + |e1| + |e2| of each ray's own triangle (tri (n, 3, 3)): what a bound on a hit point's error is stated in"""
    nrm = lambda a: np.linalg.norm(a, axis=-1)  # noqa: E731
    return nrm(np.asarray(origin, dtype=f64) - tri[..., 0, :]) + nrm(tri[..., 1, :] - tri[..., 0, :]) + nrm(tri[..., 2, :] - tri[..., 0, :])


def conditioning(inst, origin, direction, k):
    """|s|_1 (|e1|_1 + |e2|_1) / |det| of each ray against the KEPT triangle k[i] of inst.mesh, in float64 in the mesh's frame:
    the quantity WATERTIGHT states its margin and the walk's domain in"""
    m = inst.mesh
    qi = np.asarray(inst.rotation, dtype=f32) * np.array([-1, -1, -1, 1], dtype=f32)
    ol = rotate(qi, np.asarray(origin, dtype=f64) - np.asarray(inst.position, dtype=f32).astype(f64))
    dl = rotate(qi, np.asarray(direction, dtype=f64))
    e1, e2 = m.e1[k].astype(f64), m.e2[k].astype(f64)
    det = np.abs(_dot(e1, np.cross(dl, e2)))
    s1 = np.abs(ol - m.v0[k].astype(f64)).sum(axis=1)
    with np.errstate(divide="ignore"):
        return s1 * (np.abs(e1).sum(axis=1) + np.abs(e2).sum(axis=1)) / det


# ---- the rule before the margin --------------------------------------------------------------------------------------------
def strict_cast(inst, origin, direction, max_distance):
    """the cast of one mesh_ref.Instance by the rule as it stood before WATERTIGHT (u >= 0, v >= 0, u + v <= 1), fp32 in the
    header's operation order -> (hit, t, normal, k), k the index among the kept triangles"""
    return mesh_ref.cast_instance_full(inst, origin, direction, max_distance, watertight=False)


# ---- the ray families ------------------------------------------------------------------------------------------------------
def unit_quat(x, y, z, w):
    q = np.array([x, y, z, w], dtype=f64)
    return tuple((q / np.linalg.norm(q)).astype(f32))


def _field():
    return mesh_ref.grid_mesh(8, 8, extent=4.0, height=lambda x, z: 0.3 * np.sin(1.1 * x) * np.cos(0.8 * z))


def _scaled(scale, subdiv=2):
    v, t = mesh_ref.icosphere(subdiv, 1.0)
    return (v.astype(f64) * np.array(scale)).astype(f32), t


IDENT = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
#           name          mesh                                        (position, rotation)                                   aimed
FAMILIES = {"ico": (lambda: mesh_ref.icosphere(2, 1.0), IDENT, True),
            "ico_placed": (lambda: mesh_ref.icosphere(2, 1.0), ((0.5, 1.0, -0.25), unit_quat(0.2, -0.4, 0.1, 0.9)), True),
            "box": (lambda: mesh_ref.box_mesh((0.8, 0.5, 1.2)), ((0.0, 0.0, 0.0), unit_quat(0.3, 0.1, -0.2, 0.9)), True),
            "ico_scaled": (lambda: _scaled((2.0, 0.5, 1.0)), IDENT, True),
            "field": (_field, IDENT, True),
            "random_ico": (lambda: mesh_ref.icosphere(2, 1.0), IDENT, False),
            "random_field": (_field, IDENT, False),
            # reported, not gated
            "sliver": (lambda: _scaled((1.0, 0.01, 1.0)), IDENT, True)}
GATED = ("ico", "ico_placed", "box", "ico_scaled", "field", "random_ico", "random_field")
LEVELS = ("inside", 4, 16)  # where the rays start: inside the surface (above the field), or L x the mesh's largest coordinate away
N_RAYS = 20000


class Family:
    """one family at one level: the mesh, its placement, and the rays in world space as the device gets them (fp32)"""


def _aims(v, t):
    """vertices, edge midpoints, and the points 1/4 and 1/10 along every edge (float64, mesh frame)"""
    v = v.astype(f64)
    tri = v[t.astype(np.int64)]
    out = [v]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        for w in (0.5, 0.25, 0.1):
            out.append(tri[:, i] + (tri[:, j] - tri[:, i]) * w)
    return np.concatenate(out)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def family(name, level, n=N_RAYS, seed=0):
    """the rays of family `name` starting at `level` ("inside", or L: L x maxabs away).  Directions are normalised in float64 from
    the origin AS ROUNDED to fp32 towards the aim, then rounded to fp32"""
    make, (position, rotation), aimed = FAMILIES[name]
    v, t = make()
    rng = np.random.default_rng([list(FAMILIES).index(name), 0 if level == "inside" else int(level), seed])
    F = Family()
    F.name, F.level, F.vertices, F.indices, F.position, F.rotation = name, level, v, t, position, rotation
    F.maxabs = float(np.abs(v).max())
    half = np.abs(v.astype(f64)).max(axis=0)
    is_field = "field" in name
    lo, hi = v.astype(f64).min(axis=0), v.astype(f64).max(axis=0)
    if aimed:
        A = _aims(v, t)
        aim = A[rng.integers(0, len(A), n)]
    elif is_field:  # uniformly random points of the field's footprint
        aim = np.stack([rng.uniform(lo[0], hi[0], n), np.zeros(n), rng.uniform(lo[2], hi[2], n)], 1)
    else:
        aim = rng.uniform(lo, hi, (n, 3))
    if level == "inside":
        o = rng.uniform(-0.3, 0.3, (n, 3)) * (np.array([F.maxabs, F.maxabs, F.maxabs]) if is_field else half)
        if is_field:
            o[:, 1] += 0.5 * F.maxabs
        if not aimed and not is_field:
            aim = o + _unit(rng.normal(size=(n, 3)))
    else:
        L = float(level) * F.maxabs
        if aimed:
            inward = np.broadcast_to(np.array([0.0, -1.0, 0.0]), (n, 3)) if is_field else -_unit(aim)
            d0 = _unit(inward + 0.4 * rng.normal(size=(n, 3)))
        else:
            d0 = _unit(rng.normal(size=(n, 3)))
            if is_field:
                d0[:, 1] = -np.abs(d0[:, 1]) - 0.2
                d0 = _unit(d0)
        o = aim - L * d0
    pos = np.asarray(position, dtype=f32).astype(f64)
    o32 = (rotate(rotation, o) + pos).astype(f32)
    d = _unit((rotate(rotation, aim) + pos) - o32.astype(f64)).astype(f32)
    far = 0.0 if level == "inside" else float(level)
    F.origin, F.dir = o32, d
    F.max_distance = np.full(n, max(100.0, 2.0 * far) * F.maxabs, dtype=f32)
    F.tri, F.orig = placed_triangles(v, t, position, rotation)
    for a in (F.origin, F.dir, F.max_distance, F.tri):
        a.setflags(write=False)
    return F


def instance(F):
    return mesh_ref.Instance(mesh_ref.Mesh(F.vertices, F.indices), F.position, F.rotation)


# ---- the properties (tests/test_mesh_watertight_cpu.py and tests/test_gpu_mesh_watertight.py assert them) ---------------------
WALK_DOMAIN = 2.0 ** 13  # the header's WATERTIGHT: the conditioning up to which the margin is not capped and the walk is exact


def reference(F):
    """(t_ref, k_ref, inside) of a family's rays, computed once: the float64 nearest crossing, its triangle (index among
    placed_triangles), and whether the ray's line passes at least 0.05 maxabs inside the silhouette"""
    if not hasattr(F, "_ref"):
        t_ref, k_ref = nearest_crossing(F.tri, F.origin, F.dir, F.max_distance)
        F._ref = (t_ref, k_ref, inside_silhouette(F.tri, F.origin, F.dir, 0.05 * F.maxabs))
    return F._ref


def leaks(F, hit, t):
    """P1, no leak: the rays (bool) that the float64 reference has cross the surface within max_distance, well inside the
    silhouette, and that report nothing or a distance beyond t_ref + 2^-14 (t_ref + maxabs)"""
    t_ref, _, inside = reference(F)
    need = np.isfinite(t_ref) & inside
    with np.errstate(invalid="ignore"):
        late = t.astype(f64) > t_ref + 2.0 ** -14 * (t_ref + F.maxabs)
    return need & (~hit | late)


def inventions(F, hit, t, k):
    """P2, no invention -> (off, ghost): hits whose triangle k (index among the kept ones) the ray meets at |cos| >= 0.5 and whose
    point origin + t dir lies farther than 2^-13 (|o - v0| + |e1| + |e2|) from that triangle; and hits of rays that miss in float64
    and whose segment is farther than that bound from EVERY triangle"""
    assert len(F.tri) == len(F.indices), "a family's mesh has no triangle of zero area"
    o, d = F.origin.astype(f64), F.dir.astype(f64)
    tri = F.tri[np.where(hit, k, 0)]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    cos = np.abs(_dot(nrm, d)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
    p = o + d * np.where(hit, t, 0).astype(f64)[:, None]
    off = hit & (cos >= 0.5) & (point_triangle_distance(p, tri) > 2.0 ** -13 * triangle_scale(o, tri))
    t_ref, _, _ = reference(F)
    cand = np.flatnonzero(hit & ~np.isfinite(t_ref))
    ghost = np.zeros(len(o), dtype=bool)
    if len(cand):
        dist = segment_triangle_distance(o[cand], d[cand], F.max_distance[cand], F.tri)
        bound = 2.0 ** -13 * triangle_scale(o[cand][:, None, :], F.tri[None])
        ghost[cand] = (dist > bound).all(axis=1)
    return off, ghost


def not_superset(strict, new):
    """P3, superset: (hit, t, normal, k) of strict_cast against the new rule's -> the rays strict_cast hits that are no longer hit,
    or later, or -- where both name the same triangle -- with another distance or normal"""
    (sh, st, sn, sk), (nh, nt, nn, nk) = strict, new
    same = sh & nh & (sk == nk)
    return sh & (~nh | (nt > st) | (same & ((nt != st) | (nn != sn).any(axis=1))))
