"""The worlds and points of the point-query tests (a helper, not a test): engineered cases per analytic kind, each named; meshes of
1, 2, 5 and 200 triangles; engineered ties; a deformable build with a collapsed triangle; and a mixed scene -- one collider of
every kind plus three mesh instances -- with a seeded random point set.  All float32, computed once and read-only.
tests/test_point_query_cpu.py runs them through csrc/fw_project.h on the host, tests/test_gpu_point_query.py on the device; both
compare with tests/project_ref.py."""
import dataclasses
import functools
import os
import sys
from dataclasses import dataclass, field
from typing import List

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
from capsule_rays import ID, TILT, _rot64, unit_quat  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
SEED = 20262
ALL = 0xFFFFFFFF


@dataclass
class World:
    colliders: List = field(default_factory=list)    # settings.Collider
    meshes: List = field(default_factory=list)       # (vertices[nv, 3] f32, indices[nt, 3] u32, deformable)
    placements: List = field(default_factory=list)   # (mesh index, position, rotation, layers)

    def instances(self):
        """the placements as mesh_ref.Instance (tests/project_ref.py)"""
        built = [mesh_ref.Mesh(v, t) for v, t, _ in self.meshes]
        return [mesh_ref.Instance(built[k], tuple(p), tuple(q), layers) for k, p, q, layers in self.placements]


def _frozen(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


# ---- engineered cases per analytic kind ---------------------------------------------------------------------------------------------
MOVED = (1.5, -0.75, 2.25)


def _kinds(position, rotation):
    return {"plane": S.Collider.Plane(position, _rot64(rotation) @ np.array([0.0, 1.0, 0.0])),
            "sphere": S.Collider.Sphere(position, 0.75),
            "box": S.Collider.Box(position, (1.0, 0.5, 0.25), rotation),
            "cylinder": S.Collider.Cylinder(position, 0.5, 2.0, rotation),
            "cone": S.Collider.Cone(position, 0.75, 2.0, rotation),
            "capsule": S.Collider.Capsule(position, 0.5, 2.0, rotation),
            "ball capsule": S.Collider.Capsule(position, 0.5, 0.0, rotation)}


# points in the collider's own frame (the plane's: normal +Y through the origin)
_LOCAL = {
    "plane": [("inside", (0.3, -0.5, 0.2)), ("on the surface", (0.25, 0.0, -0.5)), ("outside", (1.0, 2.0, -3.0)), ("far outside", (100.0, 250.0, 7.0))],
    "sphere": [("inside", (0.1, 0.2, -0.3)), ("the centre", (0.0, 0.0, 0.0)), ("on the surface", (0.75, 0.0, 0.0)), ("outside", (1.0, 2.0, -0.5)),
               ("outside on an axis", (0.0, -3.0, 0.0))],
    "box": [("inside", (0.5, 0.25, -0.125)), ("on a face", (1.0, 0.25, 0.0)), ("on a corner", (1.0, 0.5, 0.25)), ("outside a face", (2.0, 0.25, 0.125)),
            ("outside an edge", (2.0, 1.5, 0.125)), ("outside a corner", (-2.0, 1.5, -1.25)), ("outside the -y face, on the axis", (0.0, -3.0, 0.0))],
    "cylinder": [("inside", (0.25, 0.5, -0.125)), ("on the axis inside", (0.0, 0.25, 0.0)), ("on the side", (0.5, 0.25, 0.0)), ("on the cap", (0.25, 1.0, 0.0)),
                 ("on the rim", (0.5, 1.0, 0.0)), ("outside the cap", (0.25, 2.0, 0.125)), ("outside the cap, on the axis", (0.0, 2.5, 0.0)),
                 ("outside the rim", (1.5, 2.0, -1.0)), ("outside the side", (-1.5, 0.25, 1.0)), ("outside the bottom rim", (0.0, -2.0, 3.0)),
                 ("outside the bottom cap, on the axis", (0.0, -1.5, 0.0))],
    "cone": [("inside", (0.125, -0.5, 0.125)), ("on the axis inside", (0.0, 0.0, 0.0)), ("on the base", (0.25, -1.0, 0.25)), ("on the apex", (0.0, 1.0, 0.0)),
             ("outside the base", (0.25, -2.0, 0.125)), ("outside the base, on the axis", (0.0, -3.0, 0.0)), ("outside the rim", (2.0, -1.5, 1.0)),
             ("outside the slant", (1.5, 0.5, -1.0)), ("outside the apex", (0.125, 3.0, 0.0)), ("above the apex, on the axis", (0.0, 2.5, 0.0)),
             ("beside the slant, level with the base", (1.0, -1.0, 0.0)), ("just below the base, under the rim", (0.75, -1.25, 0.0))],
    "capsule": [("inside", (0.1, 0.3, -0.2)), ("inside a cap's ball", (0.1, 1.3, 0.0)), ("on the axis inside", (0.0, 0.5, 0.0)), ("on the side", (0.5, 0.25, 0.0)),
                ("on the top pole", (0.0, 1.5, 0.0)), ("outside the side", (2.0, 0.25, -1.0)), ("outside the top cap", (1.0, 3.0, 0.5)),
                ("outside the bottom cap", (-1.0, -3.0, 0.5)), ("above the top pole, on the axis", (0.0, 4.0, 0.0)), ("below, on the axis", (0.0, -2.0, 0.0)),
                ("level with the segment's top end", (3.0, 1.0, 0.0))],
    "ball capsule": [("inside", (0.1, 0.2, -0.3)), ("outside", (2.0, 1.0, -1.0)), ("outside on the axis", (0.0, 3.0, 0.0)), ("the centre", (0.0, 0.0, 0.0))],
}


@functools.lru_cache(maxsize=None)
def engineered():
    """-> (World, points[n, 3], masks[n], names[n], collider index[n]): every kind at the origin with the identity rotation and
    again moved and tilted (the points carried along in float64 and rounded), every collider on a layer bit of its own, every point
    with the mask of its collider alone"""
    colliders, points, masks, names, owner = [], [], [], [], []
    for frame, pos, rot in (("identity", (0.0, 0.0, 0.0), ID), ("rotated", MOVED, TILT)):
        R = _rot64(rot)
        for kind, c in _kinds(pos, rot).items():
            c = dataclasses.replace(c, layers=1 << len(colliders))
            colliders.append(c)
            for what, p in _LOCAL[kind]:
                points.append((R @ np.asarray(p, dtype=np.float64) + np.asarray(pos)).astype(f32))
                masks.append(c.layers)
                names.append(f"{kind}: {what} [{frame}]")
                owner.append(len(colliders) - 1)
    assert len(colliders) <= 32
    return World(colliders), _frozen(points, f32), _frozen(masks, np.uint32), tuple(names), _frozen(owner, np.int64)


# ---- meshes of 1, 2, 5 (the first interior node) and 200 triangles ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_sizes():
    """-> (World, points, masks): four meshes, one instance and one layer bit each (the 2-triangle one rotated); points above, beside
    and far from each, with the mask of that instance"""
    rng = np.random.default_rng(SEED + 1)
    gv, gt = mesh_ref.grid_mesh(10, 10, extent=2.0, height=lambda x, z: 0.2 * np.sin(2.0 * x) * np.cos(1.5 * z))
    quad_v = np.array([[-1, 0, -1], [1, 0, -1], [1, 0.5, 1], [-1, 0, 1]], dtype=f32)
    fan_v = np.array([[0, 0, 0], [1, 0, 0], [0.8, 0.1, 0.8], [0, 0.2, 1], [-0.9, 0, 0.7], [-1, -0.1, -0.2], [-0.3, 0.3, -1]], dtype=f32)
    meshes = [(quad_v[:3], np.array([[0, 1, 2]], dtype=np.uint32), False),
              (quad_v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), False),
              (fan_v, np.array([[0, k, k + 1] for k in range(1, 6)], dtype=np.uint32), False),
              (gv, gt, False)]
    assert [len(t) for _, t, _ in meshes] == [1, 2, 5, 200]
    placements = [(0, (0.0, 0.0, 0.0), ID, 1), (1, (0.5, -0.25, 1.0), TILT, 2), (2, (0.0, 0.0, 0.0), ID, 4), (3, (-1.0, 0.5, 0.25), unit_quat(0.1, 0.0, -0.2, 0.95), 8)]
    n = 300
    pts = np.concatenate([rng.uniform(-2.5, 2.5, (n, 3)), rng.uniform(-30.0, 30.0, (n // 3, 3))])
    points = np.tile(pts, (4, 1))
    masks = np.repeat(np.array([1, 2, 4, 8], dtype=np.uint32), len(pts))
    return World([], meshes, placements), _frozen(points, f32), _frozen(masks, np.uint32)


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
def tie_cases():
    """[(name, World, point, expected kind, index, triangle, expected d2-distance)]: all operands exact in fp32, so the competing
    squared distances are bit-equal and only the tie rule decides"""
    s_left, s_right = S.Collider.Sphere((-2.0, 0.0, 0.0), 1.0), S.Collider.Sphere((2.0, 0.0, 0.0), 1.0)
    b_left = S.Collider.Box((-2.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    # two triangles sharing the edge (0, 0, -1) - (0, 0, 1), folded like a roof: the point above the ridge is nearest to the edge
    roof_v = np.array([[0, 0, -1], [0, 0, 1], [-1, -1, 0], [1, -1, 0]], dtype=f32)
    left_first = np.array([[0, 1, 2], [1, 0, 3]], dtype=np.uint32)
    right_first = left_first[::-1].copy()
    flat_v = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], dtype=f32)  # a flat quad in y = 0: its diagonal is shared
    flat_t = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    plane = S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    up = (0.0, 1.0, 0.0)
    roof = lambda t: World([], [(roof_v, t, False)], [(0, (0.0, 0.0, 0.0), ID, 1)])  # noqa: E731
    two = World([], [(flat_v, flat_t, False), (flat_v, flat_t[::-1].copy(), False)], [(0, (0.0, 0.0, 0.0), ID, 1), (1, (0.0, 0.0, 0.0), ID, 1)])
    return [("two spheres, the lower index", World([s_left, s_right]), (0.0, 0.0, 0.0), S.HIT_COLLIDER, 0, 0xFFFFFFFF, 1.0),
            ("a box and a sphere", World([s_right, b_left]), (0.0, 0.0, 0.0), S.HIT_COLLIDER, 0, 0xFFFFFFFF, 1.0),
            ("a sphere and a box", World([b_left, s_right]), (0.0, 0.0, 0.0), S.HIT_COLLIDER, 0, 0xFFFFFFFF, 1.0),
            ("a shared edge", roof(left_first), (0.0, 1.0, 0.25), S.HIT_MESH, 0, 0, 1.0),
            ("a shared edge, the triangles reversed in indices", roof(right_first), (0.0, 1.0, 0.25), S.HIT_MESH, 0, 0, 1.0),
            ("a shared vertex", roof(left_first), (0.0, 0.5, 2.0), S.HIT_MESH, 0, 0, float(np.sqrt(f32(1.25)))),
            ("a shared diagonal of a flat quad", World([], [(flat_v, flat_t, False)], [(0, (0.0, 0.0, 0.0), ID, 1)]), (0.5, 2.0, 0.5), S.HIT_MESH, 0, 0, 2.0),
            ("two instances, the lower index", two, (0.25, 2.0, -0.5), S.HIT_MESH, 0, 0, 2.0),
            ("a plane before a mesh", World([plane], [(flat_v, flat_t, False)], [(0, (0.0, 0.0, 0.0), ID, 1)]), (0.5, 2.0, -0.25), S.HIT_COLLIDER, 0, 0xFFFFFFFF, 2.0),
            ("inside the second sphere, on the first", World([S.Collider.Plane((0.0, 0.0, 0.0), up), S.Collider.Sphere((0.0, 0.0, 0.0), 1.0)]), (0.25, 0.0, 0.5),
             S.HIT_COLLIDER, 1, 0xFFFFFFFF, 0.0)]


# ---- a deformable build with a collapsed triangle --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def collapsed():
    """-> (World, points, masks, the vertex the collapsed triangles sit on): a small height field built as DEFORMABLE whose `indices`
    also hold two zero-area triangles on a vertex well above it -- they keep a slot in the hierarchy (a record with zero edges) and must
    not answer that vertex; the original indices of the triangles behind them are shifted"""
    gv, gt = mesh_ref.grid_mesh(4, 4, extent=2.0, height=lambda x, z: 0.1 * x * z)
    peak = np.array([[0.25, 3.0, -0.5]], dtype=f32)
    k = len(gv)
    v = np.concatenate([gv, peak])
    t = np.concatenate([[[k, k, k]], gt[:10], [[k, 3, k]], gt[10:]]).astype(np.uint32)
    rng = np.random.default_rng(SEED + 2)
    points = np.concatenate([rng.uniform(-2.5, 2.5, (400, 3)) + [0.0, 1.0, 0.0], peak + rng.normal(size=(100, 3)) * 0.2, peak])
    return World([], [(v, t, True)], [(0, (0.0, 0.0, 0.0), ID, 1)]), _frozen(points, f32), _frozen(np.full(len(points), 1), np.uint32), peak[0]


# ---- the mixed scene ----------------------------------------------------------------------------------------------------------------------
EXTENT = 6.0


@functools.lru_cache(maxsize=None)
def mixed_world():
    """one collider of every kind, on layers 1, 2, 4 and combinations, and three mesh instances (a height field, a rotated icosphere, a
    rotated triangle soup on layer 2) in a scene of about [-6, 6]^3"""
    colliders = [S.Collider.Plane((0.0, -4.0, 0.0), (0.0, 1.0, 0.0), 1), S.Collider.Sphere((-3.0, 1.0, 2.0), 1.25, 4),
                 S.Collider.Box((3.5, 0.0, -1.0), (0.5, 0.75, 1.0), unit_quat(0.3, 0.0, 0.1, 0.9), 1),
                 S.Collider.Cylinder((0.0, 2.5, -3.0), 0.75, 1.5, ID, 2), S.Collider.Cone((-2.0, -1.0, -3.0), 1.0, 2.0, TILT, 5),
                 S.Collider.Capsule((2.0, 3.0, 3.0), 0.4, 2.0, unit_quat(0.6, 0.1, -0.3, 0.7), 3)]
    rng = np.random.default_rng(5)
    soup_v = rng.uniform(-1.5, 1.5, size=(3 * 60, 3)).astype(f32)
    soup_t = np.arange(3 * 60, dtype=np.uint32).reshape(-1, 3)
    ico_v, ico_t = mesh_ref.icosphere(1, 1.25)
    grid_v, grid_t = mesh_ref.grid_mesh(12, 12, extent=5.0, height=lambda x, z: 0.25 * np.sin(1.3 * x) * np.cos(0.9 * z))
    meshes = [(grid_v, grid_t, False), (ico_v, ico_t, False), (soup_v, soup_t, False)]
    placements = [(0, (0.0, -2.0, 0.0), ID, 1), (1, (3.0, 2.5, -3.5), unit_quat(0.5, -0.1, 0.2, 0.8), 4), (2, (-3.0, 3.5, -1.0), unit_quat(0.1, 0.2, -0.3, 0.9), 2)]
    return World(colliders, meshes, placements)


@functools.lru_cache(maxsize=None)
def mixed_points(n=3000):
    """points for mixed_world(): spread over the scene, near the analytic surfaces and the height field, inside the solids, a few far
    away, and the non-finite ones last (a NaN, an infinity): about n + 8"""
    rng = np.random.default_rng(SEED)
    w = mixed_world()
    spread = rng.uniform(-EXTENT, EXTENT, (n // 2, 3))
    near = []
    for c in w.colliders[1:]:
        size = max(c.radius, max(c.half_extents)) * 1.5
        near.append(np.asarray(c.position) + rng.normal(size=(n // 16, 3)) * size)
    xz = rng.uniform(-5.5, 5.5, (n // 8, 2))
    near.append(np.stack([xz[:, 0], -2.0 + rng.normal(size=len(xz)) * 0.3, xz[:, 1]], 1))
    near.append(np.stack([xz[:, 0], -4.0 + rng.normal(size=len(xz)) * 0.2, xz[:, 1]], 1))  # about the plane, inside and outside
    far = rng.uniform(-60.0, 60.0, (n // 16, 3))
    odd = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e30, 1e30, 1e30], [0.0, 0.0, 0.0]])
    pts = np.concatenate([spread] + near + [far, odd])
    return _frozen(pts, f32)
