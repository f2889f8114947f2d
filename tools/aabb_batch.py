"""The boxes of many spawners on the MI355X: what one fw_ctx_aabbs over N spawners, one fw_ctx_aabbs_device (its whole call) and the
loop of N fw_spawner_aabb cost (DESIGN.md section 4.2 "Batched boxes", profiles/r25/aabb_batch.txt).

  python tools/aabb_batch.py all PARENT_LIB [OUT [SHAPES [REPEATS]]]   every shape below (or the comma-separated SHAPES); PARENT_LIB: the
                                                     library of the commit before the batched call, which runs the loop leg.  The report
                                                     goes to stdout and, OUT given, is appended to that file too
  python tools/aabb_batch.py one SHAPE LEGS         the legs (comma-separated) of one shape on one context: JSON on the last line (`all` starts these)
  python tools/aabb_batch.py trace SHAPE            30 batched host calls and nothing else: the rocprofv3 --kernel-trace --stats target

Shapes: `1x983333` (workloads.one_million, configs[1]), `512x8192` (one GPU's share of configs[4]), `4096x8192` (the whole of configs[4]),
`2048x200` (examples/many_contexts), `64x733` (sparks.rs emitters).  Every context is stepped for 75 frames of 1/60 s (past every
lifetime: steady state) and left idle; then, per leg, 3 warm-up rounds and 5 timed windows, each a host clock around work that ends in a
device synchronise: the best and the median window.  Legs: `batch` (fw_ctx_aabbs: waits itself), `device` (fw_ctx_aabbs_device followed
by one synchronise), `loop` (N x fw_spawner_aabb: N waits).  `all` alternates a process of this library
(batch, device, loop on one context) and one of the parent's (loop, through FW_LIB_PATH) three times: the spread between the repeats is printed with the best.
FW_BOX_CHUNK builds (make EXTRA=-DFW_BOX_CHUNK=512 in a copy of csrc/: tools/build_variant.sh) are measured by pointing FW_LIB_PATH at them.
No pass mark but one: at 512x8192 the batched host call has to beat the parent's loop."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SHAPES = {"1x983333": (1, 983333), "512x8192": (512, 8192), "4096x8192": (4096, 8192), "2048x200": (2048, 200), "64x733": (64, 733)}


def _context(shape):
    from bevy_firework_amd import workloads
    from bevy_firework_amd.system import ParticleSystem

    n, per = SHAPES[shape]
    ps = ParticleSystem(seed=1)
    if n == 1:
        specs = [workloads.one_million()]
    elif per == 733:
        specs = [workloads.example_sparks() for _ in range(n)]
    else:
        specs = workloads.many_emitters(n, per)
    hs = [ps.spawn(sp, tf, uid=i) for i, (sp, tf) in enumerate(specs)]
    ps._push_origins()
    for _ in range(75):
        ps.step(1.0 / 60.0)
    ps.synchronize()
    return ps, hs


def _windows(round_, windows=5, rounds=None):
    for _ in range(3):
        round_()
    us = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(rounds):
            round_()
        us.append((time.perf_counter() - t0) / rounds * 1e6)
    return {"best_us": round(min(us), 2), "median_us": round(sorted(us)[len(us) // 2], 2)}


def one(shape, legs):
    """the legs (comma-separated) of one shape, one after the other on one context: a list of rows"""
    ps, hs = _context(shape)
    rows = [_leg(ps, hs, shape, leg) for leg in legs.split(",")]
    ps.close()
    return rows


def _leg(ps, hs, shape, leg):
    import ctypes as C

    import numpy as np

    n = len(hs)
    live = ps.live_count()
    handles = (C.c_int32 * n)(*[h.handle for h in hs])
    L, ctx = ps._lib, ps._ctx
    rounds = max(2, min(50, 4000 // n))
    row = {"shape": shape, "leg": leg, "n": n, "live": live, "lib": os.environ.get("FW_LIB_PATH", "this")}
    if leg == "loop":
        mn, mx, any_ = (C.c_float * 3)(), (C.c_float * 3)(), C.c_int32()

        def round_():
            for h in handles:
                st = L.fw_spawner_aabb(ctx, h, mn, mx, C.byref(any_))
                if st:
                    raise SystemExit(f"fw_spawner_aabb: {st}")
    elif leg == "batch":
        from bevy_firework_amd import settings as S

        out = np.zeros(n, dtype=S.AABB_DTYPE)
        optr = out.ctypes.data_as(C.c_void_p)

        def round_():
            st = L.fw_ctx_aabbs(ctx, n, handles, optr)
            if st:
                raise SystemExit(f"fw_ctx_aabbs: {st}")
    elif leg == "device":
        dptr = C.c_void_p()  # (the HIP runtime the library itself is linked against; the process ends with the measurement: never freed)
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        if hip.hipMalloc(C.byref(dptr), C.c_size_t(n * 32)) != 0:
            raise SystemExit("hipMalloc failed")

        def round_():
            st = L.fw_ctx_aabbs_device(ctx, n, handles, dptr)
            if st:
                raise SystemExit(f"fw_ctx_aabbs_device: {st}")
            ps.synchronize()
    else:
        raise SystemExit(__doc__)
    row.update(_windows(round_, rounds=rounds))
    if leg != "loop":
        launches, chunks, chunk = ps.debug_aabb_batch()
        row.update(chunks=chunks, chunk=chunk)
    return row


def _child(shape, legs, lib=None):
    env = dict(os.environ)
    env.pop("FW_LIB_PATH", None), env.pop("FW_ALLOW_OLD_ABI", None)
    if lib:
        env["FW_LIB_PATH"], env["FW_ALLOW_OLD_ABI"] = lib, "1"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "one", shape, legs], capture_output=True, text=True, timeout=900, env=env)
    if out.returncode != 0:
        raise SystemExit(f"{shape} {legs} failed ({out.returncode}): " + out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "one":
        print(json.dumps(one(sys.argv[2], sys.argv[3])), flush=True)
    elif mode == "trace":
        ps, hs = _context(sys.argv[2])
        for _ in range(30):
            ps.aabb_records(hs)
        ps.close()
    elif mode == "all":
        parent = os.path.abspath(sys.argv[2])
        out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
        shapes = sys.argv[4].split(",") if len(sys.argv) > 4 else list(SHAPES)
        repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 3

        def say(ln):
            print(ln, flush=True)
            if out:
                out.write(ln + "\n"), out.flush()

        for shape in shapes:
            legs = {"batch": [], "device": [], "loop": [], "parent loop": []}
            for _ in range(repeats):  # interleaved: this library and the parent's take turns, a process each
                for row in _child(shape, "batch,device,loop"):
                    legs[row["leg"]].append(row)
                legs["parent loop"] += _child(shape, "loop", parent)
            r = legs["batch"][0]
            say(f"{shape:10s} {r['n']} spawners, {r['live']} live particles, {r['chunks']} chunks of {r['chunk']}; microseconds per round over all spawners,"
                " best window of each process (median window):")
            for name, rows in legs.items():
                say(f"    {name:12s} " + "  ".join(f"{x['best_us']:11.2f} ({x['median_us']:.2f})" for x in rows))
            b, p = min(x["best_us"] for x in legs["batch"]), min(x["best_us"] for x in legs["parent loop"])
            say(f"    batched host call / parent's loop: {b / p:.4f}  ({'faster' if b < p else 'NOT faster'}; {b * 1e3 / max(r['live'], 1):.3f} ns per particle)")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
