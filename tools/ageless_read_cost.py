#!/usr/bin/env python3
"""What a read costs a ring under the age rule: configs[1]'s 1M-particle ring, a stretch of frames nobody
reads, then fw_spawner_aabb / fw_spawner_read_particles -- with the rule (the read first writes the age plane back: fw_k_fifo_ages, one
launch over ~4 MB) and with FW_AGELESS=0.  Prints one JSON line per form."""
import os as _os; _os.environ.setdefault("FW_ENABLE_KNOBS", "1")
import json, os, sys, time
import numpy as np
import torch  # noqa: F401  (before the library: two HIP runtimes in one process must be loaded in this order)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevy_firework_amd import workloads
from bevy_firework_amd.system import ParticleSystem

dt = np.float32(1 / 60)
for rule in ("1", "0"):
    os.environ["FW_AGELESS"] = rule
    ps = ParticleSystem(seed=workloads.SEED)
    sp, tf = workloads.one_million()
    h = ps.spawn(sp, tf, uid=0)
    for _ in range(80):
        ps.step(dt)
    ps.synchronize()
    t_aabb, t_read = [], []
    for rep in range(7):
        for _ in range(20):
            ps.step(dt)
        ps.synchronize()
        t0 = time.perf_counter()
        h.aabb()
        t_aabb.append((time.perf_counter() - t0) * 1e6)
        for _ in range(20):
            ps.step(dt)
        ps.synchronize()
        t0 = time.perf_counter()
        n = len(h.particles(0))
        t_read.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps({"FW_AGELESS": rule, "live": n, "path": h.update_path(0), "aabb_us_median": float(np.median(t_aabb[1:])), "aabb_us": [round(x, 1) for x in t_aabb],
                      "read_particles_us_median": float(np.median(t_read[1:])), "read_particles_us": [round(x, 1) for x in t_read]}))
    ps.close()
