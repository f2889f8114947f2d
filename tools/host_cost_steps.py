#!/usr/bin/env python3
"""Host-side cost of the individual fw_step calls of an unread stretch (configs[1]), split by what the call did: W -- the frame was
withheld, bookkeeping alone (fw_ctx::withheld) -- and L -- the call enqueued a launch.  Small batches between waits, as in
tools/host_cost.py, so the hardware queue never fills; the two debug counters are read outside the timed region.  Prints one JSON line:
medians and means of W and L in us, the depth the launches ran at, and the projected host cost per step ((D-1) W + L) / D for D = 2 .. 16."""
import os as _os; _os.environ.setdefault("FW_ENABLE_KNOBS", "1")  # the A/B switches are honoured only with this set
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevy_firework_amd import workloads
from bevy_firework_amd.system import ParticleSystem

ps = ParticleSystem(seed=1)
sp, tf = workloads.one_million()
ps.spawn(sp, tf)
dt = np.float32(1 / 60)
ps.update(dt)
for _ in range(120):  # (32 unread launches earn the deferred spin; a multiple of 2, 3, 4, 5, 6 and 8: no frame is pending behind it)
    ps.step(dt)
ps.synchronize()
has_frames = hasattr(ps._lib, "fw_debug_fuse_frames")
W, L, depth = [], [], []
for _ in range(100):
    for _ in range(24):  # (whole groups at every depth but 5 and 7, whose remainder the wait flushes outside the timed calls)
        f0 = ps.fuse2_launches()[0]
        n0 = ps.fuse_frames() if has_frames else 2 * f0
        t0 = time.perf_counter()
        ps.step(dt)
        t = (time.perf_counter() - t0) * 1e6
        f1 = ps.fuse2_launches()[0]
        if f1 != f0:
            L.append(t)
            depth.append((ps.fuse_frames() if has_frames else 2 * f1) - n0)
        else:
            W.append(t)
    ps.synchronize()
W, L = np.array(W[48:]), np.array(L[12:])  # (the first batches: cold caches)
row = {"withheld_calls": len(W), "launching_calls": len(L), "depth_of_the_launches": sorted(set(depth)),
       "W_us_median": round(float(np.median(W)), 3), "W_us_mean": round(float(W.mean()), 3), "W_us_p10_p90": [round(float(x), 3) for x in np.percentile(W, [10, 90])],
       "L_us_median": round(float(np.median(L)), 3), "L_us_mean": round(float(L.mean()), 3), "L_us_p10_p90": [round(float(x), 3) for x in np.percentile(L, [10, 90])]}
for d in (2, 3, 4, 5, 6, 8, 10, 12, 16):
    row[f"projected_host_us_per_step_depth_{d}"] = round(float(((d - 1) * np.median(W) + np.median(L)) / d), 3)
print(json.dumps(row))
