"""Triangle-mesh colliders on the MI355X: what they cost and what they leave unchanged.

  python tools/mesh_colliders.py regression --parent DIR   stress_test_collision at product defaults (analytic boxes, no mesh):
                                                           this tree against the tree at DIR (the parent commit, built),
                                                           alternated in one call, 3 runs each, one subprocess per run
  python tools/mesh_colliders.py cost                      the same world with its two boxes as 12-triangle meshes against the
                                                           analytic boxes, same build
  python tools/mesh_colliders.py scaling                   a height-field terrain of 2 048 and of 131 072 triangles over the
                                                           same extent, at 157k and 1.26M particles
  python tools/mesh_colliders.py build                     fw_ctx_create_mesh time (host build + upload) and device bytes for
                                                           131k and 1M triangles
  python tools/mesh_colliders.py deform                    a terrain of 2 048 and of 131 072 triangles whose heights change EVERY frame:
                                                           fw_ctx_update_mesh_vertices + fw_step, pipelined (deformN), against the only way
                                                           before deformable meshes, destroy + create + set per frame (rebuildN: the set is
                                                           emptied first, a placed mesh cannot be destroyed); and the
                                                           cast cost over a refitted tree against a fresh build of the same vertices
  python tools/mesh_colliders.py device_vertices           the deformN rows next to devdeformN -- the same 16 vertex sets resident in device
                                                           memory, handed over by fw_ctx_update_mesh_vertices_device (no copy back, no
                                                           host pass, no upload) -- and to the static terrain: alternated, 3 rounds, one
                                                           subprocess per run; us per frame and the host time inside the call
  python tools/mesh_colliders.py one WORLD RATE [FRAMES]   one measurement (what the modes above run; also the rocprofv3 target)

Frame time: 150 warm-up frames (the 2 s lifetime fills), then the best of 3 windows of 300 frames, each ending in a
synchronise.  Every world keeps the example's emitter pose and its angled cube where the cube is not a mesh.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _box_mesh(h):
    hx, hy, hz = h
    v = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], dtype=f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, e in quads for t in ((a, b, c), (a, c, e))], dtype=np.uint32)


def _terrain(cells, extent=4.0, phase=0.0, amp=0.15):
    """cells x cells quads (2 triangles each) over [-extent, extent]^2, a gentle height field around y = 0"""
    xs = np.linspace(-extent, extent, cells + 1)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = amp * np.sin(1.7 * X + phase) * np.cos(1.3 * Z - 0.5 * phase)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(f32)
    i = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, e = i[:-1, :-1].ravel(), i[1:, :-1].ravel(), i[1:, 1:].ravel(), i[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, e, c], 1), np.stack([a, c, b], 1)]).astype(np.uint32)


def one(world, rate, frames=300):
    """-> dict: us per frame of stress_test_collision at `rate` against `world` (analytic | mesh_boxes | terrainN)"""
    sys.path.insert(0, os.environ.get("FW_TREE", HERE))
    from bevy_firework_amd import settings as S
    from bevy_firework_amd import workloads
    from bevy_firework_amd.system import ParticleSystem

    sp, tf, colliders = workloads.stress_test_collision(rate=rate)
    dt = f32(1.0 / 60.0)
    ps = ParticleSystem(seed=workloads.SEED)
    h = ps.spawn(sp, tf, uid=0)
    info = {"world": world, "rate": rate}
    if world == "analytic":
        ps.set_colliders(colliders)
    elif world == "mesh_boxes":  # the slab and the cube as 12-triangle meshes, same poses
        insts = []
        for c in colliders:
            m = ps.create_mesh(*_box_mesh(c.half_extents))
            insts.append(S.MeshCollider(m, c.position, c.rotation))
        ps.set_mesh_colliders(insts)
    elif world.startswith("terrain"):  # the slab's top face as a height field; the cube stays analytic
        v, t = _terrain(int(world[len("terrain"):]))
        t0 = time.perf_counter()
        m = ps.create_mesh(v, t)
        info["create_ms"] = (time.perf_counter() - t0) * 1e3
        info["triangles"] = len(t)
        ps.set_mesh_colliders([S.MeshCollider(m)])
        ps.set_colliders(colliders[1:])
    elif world.startswith(("devdeform", "deform", "rebuild", "refitted", "fresh")):
        # a terrain that moves: deformN updates a deformable mesh every frame, rebuildN destroys and creates a static one;
        # refittedN:A / freshN:A cast (no per-frame change) over a tree refitted to phase A against one built there
        # devdeformN is deformN with the vertex sets in device tensors (fw_ctx_update_mesh_vertices_device)
        kind = next(k for k in ("devdeform", "deform", "rebuild", "refitted", "fresh") if world.startswith(k))
        spec = world[len(kind):].split(":")
        cells, far = int(spec[0]), float(spec[1]) if len(spec) > 1 else 0.0
        t = _terrain(cells)[1]
        phases = [_terrain(cells, phase=0.05 * k)[0] for k in range(16)]
        ps.set_colliders(colliders[1:])
        info["triangles"] = len(t)
        if kind == "refitted":
            m = ps.create_deformable_mesh(phases[0], t)
            ps.update_mesh_vertices(m, _terrain(cells, phase=far, amp=0.15 + 0.2 * far)[0])
        elif kind == "fresh":
            m = ps.create_mesh(_terrain(cells, phase=far, amp=0.15 + 0.2 * far)[0], t)
        else:
            m = ps.create_deformable_mesh(phases[0], t) if kind in ("deform", "devdeform") else ps.create_mesh(phases[0], t)
        if kind == "devdeform":
            import torch

            with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
                d_phases = [torch.from_numpy(v.copy()).to("cuda") for v in phases]
            ptrs = [d.data_ptr() for d in d_phases]
        ps.set_mesh_colliders([S.MeshCollider(m)])
        state = {"m": m, "k": 0, "host": 0.0, "calls": 0}

        def per_frame():
            state["k"] += 1
            v = phases[state["k"] % len(phases)]
            t0 = time.perf_counter()
            if kind == "deform":
                ps.update_mesh_vertices(state["m"], v)
            elif kind == "devdeform":
                ps.update_mesh_vertices_device(state["m"], ptrs[state["k"] % len(phases)], len(v))
            elif kind == "rebuild":
                ps.set_mesh_colliders([])
                ps.destroy_mesh(state["m"])
                state["m"] = ps.create_mesh(v, t)
                ps.set_mesh_colliders([S.MeshCollider(state["m"])])
            state["host"] += time.perf_counter() - t0
            state["calls"] += 1
    else:
        raise SystemExit(f"unknown world {world}")
    if not world.startswith(("devdeform", "deform", "rebuild")):
        per_frame = None
    if world.startswith("rebuild"):
        frames = min(frames, 30)  # (tens of milliseconds each at 131k triangles)
    ps.update(dt)
    for _ in range(150):  # (every world alike: the rows compare the same particle state)
        if per_frame:
            per_frame()
        ps.step(dt)
    ps.synchronize()
    best = math.inf
    for _ in range(3):
        ps.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            if per_frame:
                per_frame()
            ps.step(dt)
        ps.synchronize()
        best = min(best, (time.perf_counter() - t0) / frames * 1e6)
    if per_frame:
        info["host_us_per_call"] = round(state["host"] / state["calls"] * 1e6, 2)
    if world.startswith("devdeform"):
        info["status"] = ps.mesh_update_status(state["m"])
    info.update(us_per_frame=round(best, 2), live=h.count(0), path=h.update_path(0)[0])
    ps.close()
    return info


def _run(world, rate, tree=HERE):
    env = dict(os.environ, FW_TREE=tree)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "one", world, str(rate)], env=env, capture_output=True,
                       text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{world} {rate} ({tree}) failed: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
    if mode == "one":
        print(json.dumps(one(sys.argv[2], float(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 300)), flush=True)
        return
    if mode == "regression":
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])
        rows = {"this": [], "parent": []}
        for rep in range(3):
            for name, tree in (("this", HERE), ("parent", parent)):
                r = _run("analytic", 80000.0, tree)
                rows[name].append(r["us_per_frame"])
                print(f"run {rep + 1} {name:6s}: {r['us_per_frame']:.2f} us per frame ({r['live']} live, {r['path']} path)", flush=True)
        a, b = min(rows["this"]), min(rows["parent"])
        print(f"stress_test_collision: this {rows['this']} / parent {rows['parent']} us per frame; best {a:.2f} / {b:.2f} "
              f"({(a / b - 1) * 100:+.1f} %)")
    elif mode == "cost":
        for rate in (80000.0, 640000.0):
            for world in ("analytic", "mesh_boxes", "analytic", "mesh_boxes"):
                r = _run(world, rate)
                print(f"{world:10s} rate {rate:8.0f}: {r['us_per_frame']:.2f} us per frame ({r['live']} live, {r['path']} path)", flush=True)
    elif mode == "scaling":
        for rate in (80000.0, 640000.0):
            for world in ("terrain32", "terrain256"):
                r = _run(world, rate)
                print(f"{world:10s} ({r['triangles']:6d} triangles) rate {rate:8.0f}: {r['us_per_frame']:.2f} us per frame "
                      f"({r['live']} live, {r['path']} path)", flush=True)
    elif mode == "deform":
        for rate in (80000.0, 640000.0):
            for world in ("terrain32", "deform32", "rebuild32", "terrain256", "deform256", "rebuild256"):
                r = _run(world, rate)
                print(f"{world:11s} ({r['triangles']:6d} triangles) rate {rate:8.0f}: {r['us_per_frame']:.2f} us per frame, "
                      f"{r.get('host_us_per_call', 0.0):.2f} us of host time per change ({r['live']} live, {r['path']} path)", flush=True)
        for far in (0.3, 3.0):  # a small and a large deformation: the tree quality a refit gives up
            for world in (f"refitted256:{far}", f"fresh256:{far}"):
                r = _run(world, 640000.0)
                print(f"{world:16s} rate   640000: {r['us_per_frame']:.2f} us per frame ({r['live']} live)", flush=True)
    elif mode == "device_vertices":
        rows = {}
        for rnd in range(3):
            for rate in (80000.0, 640000.0):
                for cells in (32, 256):
                    for world in (f"deform{cells}", f"devdeform{cells}", f"terrain{cells}"):
                        r = _run(world, rate)
                        rows.setdefault((rate, cells, world), []).append((r["us_per_frame"], r.get("host_us_per_call", 0.0)))
                        print(f"round {rnd + 1} {world:13s} ({r['triangles']:6d} triangles) rate {rate:8.0f}: {r['us_per_frame']:.2f} us per frame, "
                              f"{r.get('host_us_per_call', 0.0):.2f} us of host time per change ({r['live']} live, {r['path']} path"
                              f"{', status ' + str(r['status']) if 'status' in r else ''})", flush=True)
        for (rate, cells, world), v in rows.items():
            print(f"{world:13s} rate {rate:8.0f}: us per frame {[a for a, _ in v]} (best {min(a for a, _ in v):.2f}); host us per change "
                  f"{[b for _, b in v]}", flush=True)
    elif mode == "build":
        import torch

        sys.path.insert(0, HERE)
        from bevy_firework_amd.system import ParticleSystem

        ps = ParticleSystem()
        for cells in (256, 724):
            v, t = _terrain(cells)
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(0)[0]
            t0 = time.perf_counter()
            m = ps.create_mesh(v, t)
            ms = (time.perf_counter() - t0) * 1e3
            free1 = torch.cuda.mem_get_info(0)[0]
            # (device bytes: the hierarchy's 32-byte nodes and 48-byte triangles; free memory moves in the allocator's granules)
            print(f"{len(t):8d} triangles: fw_ctx_create_mesh {ms:.1f} ms (host build + upload); device free memory -{(free0 - free1) / 2**20:.1f} MB",
                  flush=True)
            ps.destroy_mesh(m)
        ps.close()
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
