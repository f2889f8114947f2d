"""The volume queries on the MI355X: what one fw_ctx_count_in_volumes_device (its whole call, up to the synchronise that follows it) costs
per shape and per volume, next to fw_ctx_aabbs_device over the same handles and next to the only way the commit before it can answer
the question: fw_spawner_read_particles of every listed spawner plus a numpy count (DESIGN.md section 4.2 "Volume queries",
profiles/r29/volume_queries.txt).

  python tools/volume_queries.py all PARENT_LIB [OUT [REPEATS]]   every shape below.  PARENT_LIB: the library of the commit before the query,
                                                     which runs the read leg.  The report goes to stdout and, OUT given, is appended to that file
  python tools/volume_queries.py one SHAPE LEGS      the legs (comma-separated) of one shape on one context: JSON on the last line (`all` starts these)

Shapes: `1x983333` (workloads.one_million, configs[1]) with 1 / 16 / 64 / 256 volumes, `512x8192` (one GPU's share of configs[4]) and
`64x733` (sparks.rs emitters) with 4.  Every context is stepped for 75 frames of 1/60 s (past every lifetime: steady state) and left idle;
then, per leg, 3 warm-up rounds and 5 timed windows (the read legs: 1 and 3), each a host clock around work that ends in a device synchronise: the best and the
median window.  Legs: `query:V` (fw_ctx_count_in_volumes_device over every spawner, type -1, and V volumes of all six kinds placed at the
emitters, then one synchronise), `boxes` (fw_ctx_aabbs_device over the same handles, then one synchronise; its windows alternate with
those of `query:1` in one process), `read:V` (SpawnerData.particles of every spawner, then per volume one vectorised numpy expression
over the positions -- a sphere test, the cheapest of the six, whatever the volume's kind: the baseline is not charged for numpy's
cost of a cone).  `all` alternates a process of this library (query legs, boxes) and one of the parent's (read legs, through
FW_LIB_PATH).  The one condition: at every shape the query is cheaper than the parent's read leg."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SHAPES = {"1x983333": ((1, 983333), (1, 16, 64, 256)), "512x8192": ((512, 8192), (4,)), "64x733": ((64, 733), (4,))}


def _context(shape):
    from bevy_firework_amd import workloads
    from bevy_firework_amd.system import ParticleSystem

    n, per = SHAPES[shape][0]
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


def _volumes(hs, n):
    """n volumes, the six kinds in turn, each at the transform of one of the spawners and raised into its cloud"""
    from bevy_firework_amd import settings as S

    rot = (0.5, 0.5, 0.5, 0.5)
    out = []
    for j in range(n):
        x, y, z = (float(c) for c in hs[j % len(hs)].transform.translation)
        c, s = (x, y + 0.5, z), 0.5 + 0.25 * ((j // 6) % 4)
        out.append([S.Collider.Plane(c, (0.0, 1.0, 0.0)), S.Collider.Sphere(c, s), S.Collider.Box(c, (s, 0.5 * s, s), rot), S.Collider.Cylinder(c, s, s, rot),
                    S.Collider.Cone(c, s, 2.0 * s), S.Collider.Capsule(c, 0.5 * s, s, rot)][j % 6])
    return out


def _time(rounds_by_leg, windows=5, rounds=10, warm=3):
    """the legs' windows by turns: {leg: {best_us, median_us}}"""
    for fn in rounds_by_leg.values():
        for _ in range(warm):
            fn()
    us = {k: [] for k in rounds_by_leg}
    for _ in range(windows):
        for k, fn in rounds_by_leg.items():
            t0 = time.perf_counter()
            for _ in range(rounds):
                fn()
            us[k].append((time.perf_counter() - t0) / rounds * 1e6)
    return {k: {"best_us": round(min(v), 2), "median_us": round(sorted(v)[len(v) // 2], 2)} for k, v in us.items()}


def one(shape, legs):
    import ctypes as C

    import numpy as np

    ps, hs = _context(shape)
    n, live = len(hs), ps.live_count()
    L, ctx = ps._lib, ps._ctx
    handles = (C.c_int32 * n)(*[h.handle for h in hs])
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    dptr = C.c_void_p()  # (the process ends with the measurement: never freed)
    if hip.hipMalloc(C.byref(dptr), C.c_size_t(max(n * 32, n * 256 * 4))) != 0:
        raise SystemExit("hipMalloc failed")
    rows, fast, slow = [], {}, {}
    for leg in legs.split(","):
        name, _, v = leg.partition(":")
        if name == "query":
            from bevy_firework_amd import _ffi
            from bevy_firework_amd import settings as S

            places = np.array([(h.handle, -1) for h in hs], dtype=S.VOLUME_PLACE_DTYPE)
            vols = _ffi.make_colliders(_volumes(hs, int(v)))

            def round_(places=places, vols=vols, nv=int(v)):
                st = L.fw_ctx_count_in_volumes_device(ctx, n, places.ctypes.data_as(C.c_void_p), nv, vols, dptr)
                if st:
                    raise SystemExit(f"fw_ctx_count_in_volumes_device: {st}")
                ps.synchronize()
            fast[leg] = round_
        elif name == "boxes":
            def round_():
                st = L.fw_ctx_aabbs_device(ctx, n, handles, dptr)
                if st:
                    raise SystemExit(f"fw_ctx_aabbs_device: {st}")
                ps.synchronize()
            fast[leg] = round_
        elif name == "read":
            spheres = [(np.asarray(c.position, dtype=np.float32), np.float32(max(c.radius, 0.5)) ** 2) for c in _volumes(hs, int(v))]

            def round_(spheres=spheres):
                out = np.zeros((n, len(spheres)), dtype=np.uint32)
                for i, h in enumerate(hs):
                    p = h.particles(0)["position"]
                    for j, (c, rr) in enumerate(spheres):
                        d = p - c
                        out[i, j] = np.count_nonzero((d * d).sum(axis=1) <= rr)
                return out
            slow[leg] = round_
        else:
            raise SystemExit(__doc__)
    rounds = max(2, min(50, 4000 // n))
    for group, kw in ((fast, dict(rounds=rounds)), (slow, dict(windows=3, warm=1, rounds=1 if n * SHAPES[shape][0][1] > 500000 else 3))):
        if group:
            for leg, t in _time(group, **kw).items():
                rows.append(dict(shape=shape, leg=leg, n=n, live=live, lib=os.environ.get("FW_LIB_PATH", "this"), **t))
    if fast:
        _, chunks, chunk, tile = ps.debug_volume_query()
        for r in rows:
            r.update(chunks=chunks, chunk=chunk, tile=tile)
    ps.close()
    return rows


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
    elif mode == "all":
        parent = os.path.abspath(sys.argv[2])
        out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
        repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 2

        def say(ln):
            print(ln, flush=True)
            if out:
                out.write(ln + "\n"), out.flush()

        ok = True
        for shape, (_, counts) in SHAPES.items():
            legs = {}
            for _ in range(repeats):  # interleaved: this library and the parent's take turns, a process each
                for row in _child(shape, ",".join([f"query:{v}" for v in counts] + ["boxes"])) + _child(shape, ",".join(f"read:{v}" for v in counts), parent):
                    legs.setdefault(row["leg"], []).append(row)
            r = legs[f"query:{counts[0]}"][0]
            say(f"{shape:10s} {r['n']} spawners, {r['live']} live particles, {r['chunks']} chunks of {r['chunk']} in the last query; microseconds per call over all "
                "spawners, best window of each process (median window):")
            for name, rows in legs.items():
                say(f"    {name:10s} " + "  ".join(f"{x['best_us']:12.2f} ({x['median_us']:.2f})" for x in rows) + ("   [parent's library]" if name.startswith("read") else ""))
            best = {name: min(x["best_us"] for x in rows) for name, rows in legs.items()}
            for v in counts:
                q, p = best[f"query:{v}"], best[f"read:{v}"]
                ok &= q < p
                say(f"    {v:3d} volumes: query / parent's read and count = {q / p:.6f}  ({'cheaper' if q < p else 'NOT cheaper'})")
            say(f"    query with {counts[0]} volume(s) / fw_ctx_aabbs_device over the same handles: {best[f'query:{counts[0]}'] / best['boxes']:.3f}")
            if len(counts) > 1:
                say("    per added volume: " + ", ".join(f"{a} -> {b}: {(best[f'query:{b}'] - best[f'query:{a}']) / (b - a):.3f} us" for a, b in zip(counts, counts[1:])))
        say("the one condition (the query is cheaper than the parent's read and count at every shape): " + ("met" if ok else "NOT met"))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
