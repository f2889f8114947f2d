"""The volume queries (include/firework_hip.h: VOLUME QUERIES) in numpy: counts[p, v] = how many particles of places[p] -- read back
through SpawnerData.particles, which the caller does AFTER the query under test -- the inside answer of tests/project_ref.py (the
header's text in float32, operation by operation) holds for against volumes[v].  A helper, not a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_ref  # noqa: E402


def inside(volume, positions):
    """project_ref's inside answer of one settings.Collider for positions[n, 3] -> bool[n]"""
    positions = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    if not len(positions):
        return np.zeros(0, dtype=bool)
    return np.asarray(project_ref.project_collider(volume, positions)[0], dtype=bool)


def normalise(places):
    """places as ParticleSystem.count_in_volumes takes them -> [(SpawnerData, type)] (type -1: every particle type)"""
    return [(p[0], int(p[1])) if isinstance(p, (tuple, list)) else (p, -1) for p in places]


def positions_of(places):
    """-> per place the positions [n, 3] of its particles, each (spawner, type) read back once"""
    seen = {}

    def one(h, t):
        if (h.handle, t) not in seen:
            seen[(h.handle, t)] = h.particles(t)["position"].astype(np.float32).reshape(-1, 3)
        return seen[(h.handle, t)]

    out = []
    for h, t in normalise(places):
        types = range(len(h.settings.particle_settings)) if t < 0 else [t]
        out.append(np.concatenate([one(h, k) for k in types] + [np.zeros((0, 3), dtype=np.float32)]))
    return out


def counts(places, volumes):
    """-> uint32[n_places, n_volumes]; a (positions, volume) pair that repeats is evaluated once"""
    pos = positions_of(places)
    out = np.zeros((len(pos), len(volumes)), dtype=np.uint32)
    memo = {}
    for p, x in enumerate(pos):
        kx = x.tobytes()
        for v, c in enumerate(volumes):
            key = (kx, id(c))
            if key not in memo:
                memo[key] = int(inside(c, x).sum())
            out[p, v] = memo[key]
    return out
