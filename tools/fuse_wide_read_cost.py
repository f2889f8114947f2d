#!/usr/bin/env python3
"""What a first reader pays with SEVEN frames withheld: tools/fuse_deep_read_cost.py at a depth of eight.
configs[1]'s 1M-particle ring at product thresholds, 40 unread frames to earn the deferred spin, then stretches of about 21 and 61 unread
frames, stepped on until seven frames are pending (the counters say so), and fw_spawner_pack_instances_device + a wait for the stream.
The device is waited for before the clock starts WITHOUT going through the library (torch.cuda.synchronize: the group stays kept), so the
figure is the group's one fused launch, the replay of the spin and the pack.  FW_FUSE2=1 against FW_FUSE2=0, medians of six.  Prints
one JSON line per setting.
(round 32: FW_READ_PENDING=15 waits for fifteen pending frames instead -- the far tier at its default depth of sixteen.)"""
import os as _os; _os.environ.setdefault("FW_ENABLE_KNOBS", "1"); _os.environ.setdefault("FW_FUSE_DEPTH", "8")  # (seven pending needs a depth of eight, the default or not)
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevy_firework_amd import workloads
from bevy_firework_amd.system import ParticleSystem

dt = np.float32(1 / 60)
PENDING = int(os.environ.get("FW_READ_PENDING", "7"))
for rule in ("1", "0"):
    os.environ["FW_FUSE2"] = rule
    ps = ParticleSystem(seed=workloads.SEED)
    sp, tf = workloads.one_million()
    h = ps.spawn(sp, tf, uid=0)
    buf = torch.empty(1 << 20, 16, dtype=torch.float32, device="cuda")
    ps.update(dt)
    row = {"FW_FUSE2": rule}
    for unread in (21, 61):
        t_pack, did, pending_seen = [], [], []
        for rep in range(7):
            pending = 0
            for k in range(40 + unread + 16):
                f0 = ps.fuse2_launches()
                ps.step(dt)
                pending = pending + 1 if ps.fuse2_launches() == f0 else 0
                if k >= 40 + unread and (pending == PENDING or rule == "0"):
                    break
            torch.cuda.synchronize()
            f0, n0 = ps.fuse2_launches(), ps.fuse_frames()
            t0 = time.perf_counter()
            ps._check(ps._lib.fw_spawner_pack_instances_device(ps._ctx, h.handle, 0, buf.data_ptr(), 1 << 20, None))
            ps.synchronize()
            t_pack.append((time.perf_counter() - t0) * 1e6)
            f1 = ps.fuse2_launches()
            did.append([f1[0] - f0[0], f1[1] - f0[1], ps.fuse_frames() - n0])
            pending_seen.append(pending if rule == "1" else 0)
        row[f"pack_instances_device_us_median_{unread}"] = float(np.median(t_pack[1:]))
        row[f"pack_instances_device_us_{unread}"] = [round(x, 1) for x in t_pack]
        row[f"frames_pending_{unread}"] = pending_seen
        row[f"fused_launches_flushed_alone_frames_fused_by_the_pack_{unread}"] = did
    print(json.dumps(row))
    ps.close()
