"""Ray-cast queries on the MI355X: what fw_ctx_cast_rays[_device] costs (profiles/r13/ray_queries.txt).

  python tools/ray_queries.py all                 every world below: the device form at 1M rays, the host form at 1k / 64k / 1M
  python tools/ray_queries.py one WORLD [N]       the device form alone, 30 calls (the rocprofv3 --kernel-trace --stats target)

Worlds are those of tools/mesh_colliders.py: `analytic` (the two boxes of stress_test_collision), `capsules` (the slab and six capsules of
stress_test_collision_capsules), `terrain32` (2 048 triangles)
and `terrain256` (131 072 triangles; the cube stays analytic).  Rays: origins uniform over the scene, unit directions, two
lengths -- `short` like a particle's step (max_distance in [0.02, 0.3], what the colliding update casts) and `long` (8: across
the scene).  Device form: 5 warm-up calls, then the best of 5 windows of 20 calls, each ending in a synchronise.  Host form: the
whole call, best of 5."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
f32 = np.float32


def _world(ps, world):
    from bevy_firework_amd import settings as S
    from bevy_firework_amd import workloads
    from mesh_colliders import _terrain

    _, _, colliders = workloads.stress_test_collision(rate=80000.0)
    if world == "analytic":
        ps.set_colliders(colliders)
        return 0
    if world == "capsules":  # the slab and the six capsules of workloads.stress_test_collision_capsules
        ps.set_colliders(workloads.stress_test_collision_capsules(rate=80000.0)[2])
        return 0
    v, t = _terrain(int(world[len("terrain"):]))
    ps.set_mesh_colliders([S.MeshCollider(ps.create_mesh(v, t))])
    ps.set_colliders(colliders[1:])
    return len(t)


def _rays(n, length, seed=11):
    from bevy_firework_amd import settings as S

    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=S.RAY_DTYPE)
    r["origin"] = np.stack([rng.uniform(-4, 4, n), rng.uniform(-0.5, 3.0, n), rng.uniform(-4, 4, n)], 1)
    d = rng.normal(size=(n, 3))
    r["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r["max_distance"] = rng.uniform(0.02, 0.3, n) if length == "short" else 8.0
    r["filter_mask"] = 0xFFFFFFFF
    return r


def measure(world, n=1000000, host_sizes=(1000, 65536, 1000000), windows=5, calls=20):
    import torch

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    ps = ParticleSystem(seed=1)
    rows = {"world": world, "triangles": _world(ps, world), "n": n}
    for length in ("short", "long"):
        rays = _rays(n, length)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32).copy()).to("cuda")
            d_hits = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        for _ in range(5):
            ps.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr())
        ps.synchronize()
        best = float("inf")
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(calls):
                ps.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr())
            ps.synchronize()
            best = min(best, (time.perf_counter() - t0) / calls)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            hits = d_hits.cpu().numpy().reshape(-1).view(S.RAY_HIT_DTYPE)
        rows[length] = {"us_per_call": round(best * 1e6, 2), "rays_per_s": round(n / best), "hit_fraction": round(float((hits["kind"] != 0).mean()), 4)}
        host = {}
        for m in host_sizes:
            ps.cast_ray_records(rays[:m])
            t = float("inf")
            for _ in range(5):
                t0 = time.perf_counter()
                ps.cast_ray_records(rays[:m])
                t = min(t, time.perf_counter() - t0)
            host[m] = round(t * 1e6, 2)
        rows[length]["host_form_us"] = host
    ps.close()
    return rows


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "one":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1000000, host_sizes=(), windows=1, calls=30)), flush=True)
    elif mode == "all":
        for world in ("analytic", "capsules", "terrain32", "terrain256"):
            r = measure(world)
            for length in ("short", "long"):
                x = r[length]
                print(f"{world:10s} ({r['triangles']:6d} triangles) {length:5s} rays: device form {x['us_per_call']:.2f} us per 1M-ray call, "
                      f"{x['rays_per_s'] / 1e9:.3f} G rays/s, {x['hit_fraction'] * 100:.1f} % hit; host form whole call "
                      + ", ".join(f"{m}: {us:.1f} us" for m, us in x["host_form_us"].items()), flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
