"""Point queries on the MI355X: what fw_ctx_project_points[_device] costs (profiles/r16/point_queries.txt,
next to the ray figures of profiles/r13/ray_queries.txt for the same worlds).

  python tools/point_queries.py all               every world below, both point sets: the device form, the host form at 1k / 64k
  python tools/point_queries.py one WORLD SET [N] the device form alone, 30 calls (the rocprofv3 --kernel-trace --stats target)

Worlds are those of tools/ray_queries.py: `analytic` (the two boxes of stress_test_collision), `terrain32` (2 048 triangles) and
`terrain256` (131 072 triangles; the cube stays analytic).  Point sets: `near` -- within 0.05 of the terrain's height range or of the
boxes, what an emitter snapped to a surface or a decal asks -- and `spread` -- uniform over the scene and well above it (up to 8), where
the first triangles a lane meets give it a poor bound and the unordered walk has the most left to visit.  The batch is sized by a probe
of 4 096 points so that one call stays near 50 ms at most (a far point on the large terrain costs thousands of triangles), up to 1M.
Device form: 3 warm-up calls, then the best of 5 windows of 10 calls, each ending in a synchronise.  No time is a pass condition."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
f32 = np.float32
WORLDS = ("analytic", "terrain32", "terrain256")
SETS = ("near", "spread")


def _points(n, which, seed=13):
    from bevy_firework_amd import settings as S

    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=S.POINT_DTYPE)
    y = rng.uniform(-0.6, 0.6, n) if which == "near" else rng.uniform(-0.5, 8.0, n)
    p["position"] = np.stack([rng.uniform(-4, 4, n), y, rng.uniform(-4, 4, n)], 1)
    p["filter_mask"] = 0xFFFFFFFF
    return p


def _timed(ps, d_points, n, d_out, windows, calls):
    best = float("inf")
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            ps.project_points_device(d_points.data_ptr(), n, d_out.data_ptr())
        ps.synchronize()
        best = min(best, (time.perf_counter() - t0) / calls)
    return best


def measure(world, which, n=None, host_sizes=(1000, 65536), windows=5, calls=10):
    import torch
    from ray_queries import _world

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    ps = ParticleSystem(seed=1)
    row = {"world": world, "set": which, "triangles": _world(ps, world)}
    points = _points(1000000, which)
    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        d_points = torch.from_numpy(points.view(np.uint8).reshape(-1, 16).copy()).to("cuda")
        d_out = torch.zeros((len(points), 32), dtype=torch.uint8, device="cuda")
    if n is None:
        probe = _timed(ps, d_points, 4096, d_out, 2, 1)  # (the second window: the first call carries the module load)
        n = int(min(1000000, max(4096, 4096 * (0.05 / probe) // 4096 * 4096)))
        row["probe_4096_us"] = round(probe * 1e6, 2)
    row["n"] = n
    for _ in range(3):
        ps.project_points_device(d_points.data_ptr(), n, d_out.data_ptr())
    ps.synchronize()
    best = _timed(ps, d_points, n, d_out, windows, calls)
    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        out = d_out[:n].cpu().numpy().reshape(-1).view(S.POINT_PROJECTION_DTYPE)
    row.update(us_per_call=round(best * 1e6, 2), points_per_s=round(n / best), mesh_fraction=round(float((out["kind"] == 2).mean()), 4),
               inside_fraction=round(float((out["is_inside"] == 1).mean()), 4), mean_distance=round(float(out["distance"].mean()), 4))
    host = {}
    for m in host_sizes:
        m = min(m, n)
        ps.project_point_records(points[:m])
        t = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            ps.project_point_records(points[:m])
            t = min(t, time.perf_counter() - t0)
        host[m] = round(t * 1e6, 2)
    row["host_form_us"] = host
    ps.close()
    return row


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "one":
        print(json.dumps(measure(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else None, host_sizes=(), windows=1, calls=30)), flush=True)
    elif mode == "all":
        for world in WORLDS:
            for which in SETS:
                r = measure(world, which)
                print(f"{world:10s} ({r['triangles']:6d} triangles) {which:6s} points: device form {r['us_per_call']:.2f} us per call of {r['n']} points, "
                      f"{r['points_per_s'] / 1e6:.2f} M points/s ({r['mesh_fraction'] * 100:.1f} % answered by the mesh, {r['inside_fraction'] * 100:.1f} % inside a "
                      f"solid, mean distance {r['mean_distance']:.3f}); host form whole call " + ", ".join(f"{m}: {us:.1f} us" for m, us in r["host_form_us"].items()), flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
