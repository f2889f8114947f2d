"""Path queries on the MI355X: what fw_ctx_trace_paths_device costs (profiles/r17/path_queries.txt).

  python tools/path_queries.py all                every world below, with and without samples
  python tools/path_queries.py one WORLD [N]      the device form alone, 30 calls (the rocprofv3 --kernel-trace --stats target)

Worlds are those of tools/mesh_colliders.py: `analytic` (the two boxes of stress_test_collision), `terrain32` (2 048 triangles) and
`terrain256` (131 072 triangles; the cube stays analytic).  Paths: 65 536 sparks from all over the scene (origins as tools/ray_queries.py's,
0.5 to 3 above the ground), thrown in every direction at speeds of 2 to 8 so that most of them land and bounce within the call, under
stress_test_collision's settings (gravity, restitution 0.6, friction 0.2), 64 steps of 1 / 60 s, lifetimes long enough to run them all.
The device form, the whole call: 5 warm-up calls, then the best of 5 windows of 20 calls, each ending in a synchronise.  No pass mark: each figure is set, per path-step, beside the colliding update's time per particle in
the same world (profiles/r07/mesh_colliders.txt, rate 80 000: frame time / 157 334 live particles)."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
f32 = np.float32
UPDATE_NS_PER_PARTICLE = {"analytic": 13.75e3 / 157334, "terrain32": 57.55e3 / 157334, "terrain256": 106.11e3 / 157334}  # profiles/r07


def _paths(n, seed=11):
    from bevy_firework_amd import settings as S

    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=S.PATH_DTYPE)
    p["position"] = np.stack([rng.uniform(-4, 4, n), rng.uniform(0.5, 3.0, n), rng.uniform(-4, 4, n)], 1)
    d = rng.normal(size=(n, 3))
    p["velocity"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 8.0, n)[:, None]
    p["lifetime"] = 1e9
    return p


def measure(world, n=65536, n_steps=64, windows=5, calls=20):
    import torch

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem
    from ray_queries import _world

    ps = ParticleSystem(seed=1)
    rows = {"world": world, "triangles": _world(ps, world), "n": n, "n_steps": n_steps}
    settings = S.PathSettings(1.0 / 60.0, n_steps, (0.0, -9.81, 0.0), 0.0, S.ParticleCollisionSettings(restitution=0.6, friction=0.2))
    paths = _paths(n)
    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        d_paths = torch.from_numpy(paths.view(np.uint8).reshape(-1, 32).copy()).to("cuda")
        d_out = torch.zeros((n, 80), dtype=torch.uint8, device="cuda")
        d_smp = torch.zeros((n_steps * n, 4), dtype=torch.float32, device="cuda")
    for name, smp in (("results", 0), ("samples", d_smp.data_ptr())):
        for _ in range(5):
            ps.trace_paths_device(settings, d_paths.data_ptr(), n, d_out.data_ptr(), smp)
        ps.synchronize()
        best = float("inf")
        for _ in range(windows):
            t0 = time.perf_counter()
            for _ in range(calls):
                ps.trace_paths_device(settings, d_paths.data_ptr(), n, d_out.data_ptr(), smp)
            ps.synchronize()
            best = min(best, (time.perf_counter() - t0) / calls)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            out = d_out.cpu().numpy().reshape(-1).view(S.PATH_RESULT_DTYPE)
        rows[name] = {"us_per_call": round(best * 1e6, 2), "ns_per_path_step": round(best * 1e9 / (n * n_steps), 4),
                      "contacts_per_path": round(float(out["n_contacts"].mean()), 3), "running": round(float((out["status"] == 0).mean()), 4)}
    ps.close()
    return rows


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "one":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 65536, windows=1, calls=30)), flush=True)
    elif mode == "all":
        for world in ("analytic", "terrain32", "terrain256"):
            r = measure(world)
            for name in ("results", "samples"):
                x = r[name]
                print(f"{world:10s} ({r['triangles']:6d} triangles) {r['n']} paths x {r['n_steps']} steps, {name:7s}: {x['us_per_call']:.2f} us per call, "
                      f"{x['ns_per_path_step']:.4f} ns per path-step ({x['contacts_per_path']:.2f} contacts per path, {x['running'] * 100:.1f} % still running); "
                      f"the colliding update in this world: {UPDATE_NS_PER_PARTICLE[world]:.4f} ns per particle", flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
