#!/usr/bin/env python3
"""What a read costs a ring whose spin is deferred: configs[1]'s 1M-particle ring, a stretch of 20 / 60 frames
nobody reads, then fw_spawner_read_particles / fw_spawner_pack_instances_device (+ a wait for the stream) -- with the rule deferring
from the third frame of the stretch (FW_SPIN_DEFER_AFTER=2: the read first replays the log, fw_k_fifo_spin, up to `unread - 2` steps per
particle) and with FW_SPIN_DEFER=0.  Medians of six.  Prints one JSON line per form."""
import os as _os; _os.environ.setdefault("FW_ENABLE_KNOBS", "1")
import json, os, sys, time
import numpy as np
import torch  # noqa: F401  (before the library: two HIP runtimes in one process must be loaded in this order)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevy_firework_amd import workloads
from bevy_firework_amd.system import ParticleSystem

dt = np.float32(1 / 60)
os.environ["FW_SPIN_DEFER_AFTER"] = "2"
for rule in ("1", "0"):
    os.environ["FW_SPIN_DEFER"] = rule
    ps = ParticleSystem(seed=workloads.SEED)
    sp, tf = workloads.one_million()
    h = ps.spawn(sp, tf, uid=0)
    buf = torch.empty(1 << 20, 16, dtype=torch.float32, device="cuda")
    for _ in range(80):
        ps.step(dt)
    ps.synchronize()
    row = {"FW_SPIN_DEFER": rule}
    for unread in (20, 60):
        t_read, t_pack = [], []
        for rep in range(7):
            for _ in range(unread):
                ps.step(dt)
            ps.synchronize()
            n0 = ps.spin_launches()
            t0 = time.perf_counter()
            n = len(h.particles(0))
            t_read.append((time.perf_counter() - t0) * 1e6)
            row[f"replays_per_read_{unread}"] = ps.spin_launches() - n0
            for _ in range(unread):
                ps.step(dt)
            ps.synchronize()
            t0 = time.perf_counter()
            ps._check(ps._lib.fw_spawner_pack_instances_device(ps._ctx, h.handle, 0, buf.data_ptr(), 1 << 20, None))
            ps.synchronize()
            t_pack.append((time.perf_counter() - t0) * 1e6)
        row[f"read_particles_us_median_{unread}"] = float(np.median(t_read[1:]))
        row[f"pack_instances_device_us_median_{unread}"] = float(np.median(t_pack[1:]))
        row[f"read_particles_us_{unread}"] = [round(x, 1) for x in t_read]
        row[f"pack_instances_device_us_{unread}"] = [round(x, 1) for x in t_pack]
    row["live"], row["path"] = n, h.update_path(0)
    print(json.dumps(row))
    ps.close()
