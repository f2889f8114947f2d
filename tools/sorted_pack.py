"""Depth-sorted instance records on the MI355X: what fw_ctx_pack_instances_sorted_device and fw_ctx_depth_order_device cost
(DESIGN.md section 4.2 "Depth-sorted records", profiles/r20/sorted_pack.txt).

  python tools/sorted_pack.py all [OUT]          every size below; the report goes to stdout and, OUT given, to that file as well
  python tools/sorted_pack.py one SIZE           30 calls of each device form and nothing else (the rocprofv3 --kernel-trace --stats target:
                                                 kernel times come from a run of their own, never from the timed windows)

Sizes: `stress` (workloads.stress_test: about 157 k live particles), `million` (workloads.one_million, configs[1]: 983 333) and `ring16m`
(the same emitter at 16 M particles a second: a FIFO ring of about 16 M).  Each is stepped past its lifetime, then read by a camera that
stands inside the cloud.  Per device form -- the sorted pack, the order alone, and the unsorted fw_spawner_pack_instances_device in the
same run -- 5 warm-up calls, then 5 windows of 20 calls, each window ending in one synchronise: the best and the median window, in
microseconds per call (a host clock around work that ends in a device synchronise).  The sort phase is the order form (keys + the four
passes).  Beside it: rocprim::radix_sort_pairs on the same keys and the same indices (tools/sort_ref.hip, a tool only; device events
around 20 sorts, same warm-up and windows), whose result must equal the library's order, entry for entry.  No pass mark."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
f32 = np.float32
YARDSTICK = os.path.join(HERE, "tools", "sort_ref_bench")
SIZES = ("stress", "million", "ring16m")


def _spawner(size):
    from bevy_firework_amd import workloads

    return {"stress": workloads.stress_test, "million": workloads.one_million, "ring16m": lambda: workloads.one_million(rate=16.0e6)}[size]()


def _yardstick():
    if not os.path.exists(YARDSTICK):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(HERE, "tools", "sort_ref.hip"), "-o", YARDSTICK])
    return YARDSTICK


def _windows(ps, call, windows, calls):
    for _ in range(5):
        call()
    ps.synchronize()
    us = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        ps.synchronize()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    return {"best_us": round(min(us), 2), "median_us": round(sorted(us)[len(us) // 2], 2)}


def measure(size, windows=5, calls=20, yardstick=True):
    import ctypes as C

    import torch

    import sort_ref
    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    spawner, tf = _spawner(size)
    ps = ParticleSystem(seed=1)
    d = ps.spawn(spawner, tf, uid=0)
    ps._push_origins()
    for _ in range(75):  # lifetime 1 s at dt = 1 / 60: steady state, a ring's head has moved
        ps.step(1.0 / 60.0)
    n = d.count(0)
    view = S.SortView(eye=(0.0, 2.0, 0.0), forward=(0.3, -0.2, 1.0), order=S.SORT_BACK_TO_FRONT)
    cap = n + 1024
    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        d_rec = torch.zeros((cap, 64), dtype=torch.uint8, device="cuda")
        d_ord = torch.zeros((cap,), dtype=torch.int32, device="cuda")
    ub = C.c_uint64()
    forms = {
        "sorted_pack": lambda: ps.pack_instances_sorted_device(d, view, d_rec.data_ptr(), cap),
        "order": lambda: ps.depth_order_device(d, view, d_ord.data_ptr(), cap),
        "unsorted_pack": lambda: ps._check(ps._lib.fw_spawner_pack_instances_device(ps._ctx, d.handle, 0, C.c_void_p(d_rec.data_ptr()), cap, C.byref(ub))),
    }
    row = {"size": size, "n": n, "path": d.update_path(0)[0]}
    for name, call in forms.items():
        row[name] = _windows(ps, call, windows, calls)
    if yardstick:
        # the same keys (the header's arithmetic on the positions the pack writes) and the same values, in a process of its own
        ps.depth_order_device(d, view, d_ord.data_ptr(), cap)
        ps.synchronize()
        ours = d_ord.cpu().numpy().view(np.uint32)[:n]
        keys = sort_ref.keys(d.instances(0)["position"], view.eye, view.forward, view.order)
        with tempfile.TemporaryDirectory() as tmp:
            kp, op = os.path.join(tmp, "keys.u32"), os.path.join(tmp, "order.u32")
            keys.tofile(kp)
            out = subprocess.run([_yardstick(), kp, str(windows), str(calls), op], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("sort_ref_bench failed: " + out.stderr[-2000:])
            row["rocprim"] = json.loads(out.stdout.strip().splitlines()[-1])
            theirs = np.fromfile(op, dtype=np.uint32)
        row["order_equals_rocprim"] = bool(np.array_equal(ours, theirs))
        row["order_equals_numpy"] = bool(np.array_equal(ours, np.argsort(keys, kind="stable").astype(np.uint32)))
    ps.close()
    return row


def _report(row):
    s, o, u = row["sorted_pack"], row["order"], row["unsorted_pack"]
    lines = [f"{row['size']:8s} {row['n']:9d} particles ({row['path']} path), microseconds per call, best window (median):",
             f"    sorted pack    {s['best_us']:10.2f} ({s['median_us']:.2f})   = {s['best_us'] / u['best_us']:.2f} x the unsorted pack",
             f"    order alone    {o['best_us']:10.2f} ({o['median_us']:.2f})   the sort phase: keys + four passes, {o['best_us'] * 1e3 / max(row['n'], 1):.3f} ns per particle",
             f"    unsorted pack  {u['best_us']:10.2f} ({u['median_us']:.2f})"]
    if "rocprim" in row:
        r = row["rocprim"]
        lines.append(f"    rocprim::radix_sort_pairs, same keys and indices {r['best_us']:10.2f} ({r['median_us']:.2f}), {r['temp_bytes']} bytes of temporary storage"
                     f"   -> the order form takes {o['best_us'] / r['best_us']:.2f} x rocPRIM's time (it also computes the keys)")
        lines.append(f"    the library's order equals rocPRIM's: {row['order_equals_rocprim']}; numpy's stable argsort: {row['order_equals_numpy']}")
    return lines


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "one":
        print(json.dumps(measure(sys.argv[2], windows=1, calls=30, yardstick=False)), flush=True)
    elif mode == "all":
        out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
        for size in SIZES:
            for ln in _report(measure(size)):
                print(ln, flush=True)
                if out:
                    out.write(ln + "\n"), out.flush()
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
