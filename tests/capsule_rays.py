"""The capsules and rays tests/test_capsule_cpu.py casts (a helper, not a test): engineered cases, each named, and a seeded random
set of a few thousand; all float32, computed once and read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
SEED = 20261


def unit_quat(x, y, z, w):
    q = np.array([x, y, z, w], dtype=np.float64)
    return tuple(float(c) for c in (q / np.linalg.norm(q)).astype(f32))


TILT = unit_quat(0.3, -0.2, 0.5, 0.8)
ID = (0.0, 0.0, 0.0, 1.0)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(f32)


@functools.lru_cache(maxsize=None)
def engineered():
    """[(name, capsule, origin, dir, max_distance)] in the capsule's OWN frame for the identity cases; every case is cast a second
    time against the same capsule rotated by TILT and moved, the ray carried along in float64 and rounded"""
    r, hl = 0.5, 1.0
    cap = S.Collider.Capsule((0.0, 0.0, 0.0), r, 2.0 * hl)
    ball = S.Collider.Capsule((0.0, 0.0, 0.0), r, 0.0)
    inf = 100.0
    cases = [
        ("origin inside", cap, (0.1, 0.3, -0.2), (1, 0, 0), inf),
        ("origin inside a cap's ball", cap, (0.1, 1.3, 0.0), (0, -1, 0), inf),
        ("origin on the lateral surface", cap, (0.5, 0.25, 0.0), (1, 0, 0), inf),
        ("origin on the top pole", cap, (0.0, 1.5, 0.0), (0, 1, 0), inf),
        ("hl == 0: a ball, from +x", ball, (3.0, 0.0, 0.0), (-1, 0, 0), inf),
        ("hl == 0: a ball, from above, off centre", ball, (0.25, 3.0, 0.125), (0, -1, 0), inf),
        ("hl == 0: a ball, slanted", ball, (2.0, 1.0, -1.0), _unit((-2.0, -0.9, 1.1)), inf),
        ("hl == 0: a ball, missed", ball, (2.0, 1.0, -1.0), (0, 1, 0), inf),
        ("parallel to the axis, inside the footprint, from above", cap, (0.25, 4.0, 0.125), (0, -1, 0), inf),
        ("parallel to the axis, inside the footprint, from below", cap, (-0.25, -4.0, 0.0), (0, 1, 0), inf),
        ("parallel to the axis, on the axis", cap, (0.0, 4.0, 0.0), (0, -1, 0), inf),
        ("parallel to the axis, outside the footprint", cap, (0.75, 4.0, 0.0), (0, -1, 0), inf),
        ("parallel to the axis, on the footprint's rim", cap, (0.5, 4.0, 0.0), (0, -1, 0), inf),
        ("perpendicular through the segment's top end", cap, (3.0, 1.0, 0.0), (-1, 0, 0), inf),
        ("perpendicular through the segment's bottom end", cap, (0.0, -1.0, -3.0), (0, 0, 1), inf),
        ("perpendicular through the middle", cap, (3.0, 0.0, 0.25), (-1, 0, 0), inf),
        ("enters through the top cap", cap, (1.0, 3.0, 0.5), _unit((-0.9, -1.75, -0.45)), inf),
        ("enters through the bottom cap", cap, (-1.0, -3.0, 0.5), _unit((0.95, 1.8, -0.5)), inf),
        ("enters through the lateral surface, slanted", cap, (2.0, 1.5, 1.0), _unit((-2.0, -1.25, -0.9)), inf),
        ("inside the infinite cylinder, beyond the top end, going down", cap, (0.125, 2.5, 0.25), _unit((0.05, -1.0, -0.1)), inf),
        ("inside the infinite cylinder, beyond the top end, going sideways", cap, (0.125, 2.5, 0.25), (1, 0, 0), inf),
        ("inside the infinite cylinder, beyond the bottom end, going up", cap, (0.125, -2.5, 0.25), (0, 1, 0), inf),
        ("inside the infinite cylinder, beyond the top end, moving away", cap, (0.125, 2.5, 0.25), (0, 1, 0), inf),
        ("tangent to the lateral surface", cap, (0.5, 0.25, -3.0), (0, 0, 1), inf),
        ("tangent to the top cap", cap, (-3.0, 1.5, 0.0), (1, 0, 0), inf),
        ("tangent to the top cap's side", cap, (0.5, 3.0, -3.0), _unit((0.0, -1.75, 3.0)), inf),
        ("just outside a tangent", cap, (0.5005, 0.25, -3.0), (0, 0, 1), inf),
        ("max_distance exactly the hit distance", cap, (3.0, 0.0, 0.0), (-1, 0, 0), 2.5),
        ("max_distance one ulp below the hit distance", cap, (3.0, 0.0, 0.0), (-1, 0, 0), float(np.nextafter(f32(2.5), f32(0.0)))),
        ("max_distance exactly the hit distance on a cap", cap, (0.0, 4.0, 0.0), (0, -1, 0), 2.5),
        ("max_distance one ulp below the hit distance on a cap", cap, (0.0, 4.0, 0.0), (0, -1, 0), float(np.nextafter(f32(2.5), f32(0.0)))),
        ("max_distance zero from outside", cap, (3.0, 0.0, 0.0), (-1, 0, 0), 0.0),
        ("a direction that is not a unit vector", cap, (3.0, 0.5, 0.0), (-2, 0, 0), inf),
        ("a zero direction outside", cap, (3.0, 0.5, 0.0), (0, 0, 0), inf),
        ("a NaN origin", cap, (float("nan"), 0.5, 0.0), (-1, 0, 0), inf),
        ("a NaN direction", cap, (3.0, 0.5, 0.0), (float("nan"), 0, 0), inf),
        ("a NaN max_distance", cap, (3.0, 0.5, 0.0), (-1, 0, 0), float("nan")),
        ("an infinite origin", cap, (float("inf"), 0.5, 0.0), (-1, 0, 0), inf),
    ]
    out = []
    pos = np.array([1.5, -0.75, 2.25])
    for name, c, o, d, md in cases:
        out.append((name + " [identity]", c, np.asarray(o, dtype=f32), np.asarray(d, dtype=f32), f32(md)))
        turned = S.Collider.Capsule(tuple(pos), c.radius, 2.0 * c.half_extents[1], TILT)
        R = _rot64(TILT)
        with np.errstate(invalid="ignore"):
            o2 = (R @ np.asarray(o, dtype=np.float64) + pos).astype(f32)
            d2 = (R @ np.asarray(d, dtype=np.float64)).astype(f32)
        out.append((name + " [rotated]", turned, o2, d2, f32(md)))
    return out


def _rot64(q):
    """the rotation matrix of q, normalised in float64 first"""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def random_set():
    """[(capsule, origin[n, 3], dir[n, 3], max_distance[n])]: eight capsules -- fat, thin, a ball, long (hl = 50 r), identity and
    rotated, away from the world's origin -- with 500 rays each: origins in a box three times the capsule's size (a fifth of them
    close in, many of those inside the solid), aimed at points spread a little wider than the solid (most hit, a good part misses), unit directions, a max_distance
    that cuts a part of the hits short.  About 4000 rays."""
    rng = np.random.default_rng(SEED)
    shapes = [(0.5, 1.0, ID, (0, 0, 0)), (0.5, 1.0, TILT, (1.5, -0.75, 2.25)), (0.75, 0.0, TILT, (-2.0, 1.0, 0.5)),
              (0.1, 5.0, unit_quat(0.6, 0.1, -0.3, 0.7), (3.0, 2.0, -1.0)), (1.0, 0.25, unit_quat(-0.2, 0.7, 0.1, 0.4), (0.0, -3.0, 1.0)),
              (0.25, 0.75, unit_quat(0.0, 0.0, 0.70710678, 0.70710678), (10.0, 5.0, -7.0)), (2.0, 3.0, ID, (-4.0, 0.5, 6.0)),
              (0.3, 2.0, unit_quat(0.1, 0.9, 0.2, -0.3), (0.5, 0.5, 0.5))]
    out = []
    for r, hl, q, p in shapes:
        c = S.Collider.Capsule(p, r, 2.0 * hl, q)
        n = 500
        R = _rot64(q)
        size = hl + r
        ol = rng.uniform(-3.0, 3.0, (n, 3)) * size
        ol[:100] *= 0.2  # (a fifth of them close in: many of those start inside the solid)
        target = np.stack([rng.uniform(-1.4, 1.4, n) * r, rng.uniform(-1.15, 1.15, n) * size, rng.uniform(-1.4, 1.4, n) * r], axis=1)
        dl = target - ol
        ln = np.linalg.norm(dl, axis=1)
        dl /= ln[:, None]
        o = (ol @ R.T + np.asarray(p, dtype=np.float64)).astype(f32)
        d = (dl @ R.T).astype(f32)
        md = (ln * rng.uniform(0.5, 2.0, n)).astype(f32)
        for a in (o, d, md):
            a.setflags(write=False)
        out.append((c, o, d, md))
    return out
