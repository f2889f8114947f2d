"""The C oracle against the committed golden vectors (tests/golden/*.json):
the reference's own two unit tests, the published Philox KATs, and the
independent numpy-float32 restatement.  CPU only."""
import json
import os

import numpy as np
import pytest

import oracle
from bevy_firework_amd import settings as S

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)


def f(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def b(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def test_reference_emission_unit_test():
    """reference src/core.rs:806-834: total must be 23 or 22; trajectory bit-exact."""
    d = load("emission_kat.json")
    total = 0
    for age_b, last_b, n, next_b in d["steps"]:
        got_n, got_next = oracle.compute_emission_count(f(age_b), f(last_b), 3.0, 0.0, 1.0, 23.0)
        assert got_n == n and b(got_next) == next_b
        total += got_n
    assert total == d["total"] and total in (22, 23)


def test_emission_wrap_trajectories():
    d = load("emission_wrap.json")
    for case in d["cases"]:
        dt = f(case["dt_bits"])
        tpc, last = np.float32(0), np.float32(0)
        for tpc_b, n, last_b in case["frames"]:
            tpc = np.float32(oracle.lib().fwo_rem_euclid(np.float32(tpc + dt), case["duration"]))
            got_n, last = oracle.compute_emission_count(tpc, last, case["duration"], case["offset_start"],
                                                        case["offset_end"], case["count"])
            assert b(tpc) == tpc_b and got_n == n and b(last) == last_b
    assert d["per_cycle_160k"] == 157334 and d["per_cycle_1m"] == 983333


def test_nested_count_kat():
    d = load("nested_count_kat.json")
    for case in d["cases"]:
        last = np.float32(np.finfo(np.float32).min)
        for age_b, n, last_b in case["rows"]:
            got_n, last = oracle.compute_emission_count(f(age_b), last, case["lifetime"], case["offset_start"],
                                                        case["offset_end"], case["count"])
            assert got_n == n and b(last) == last_b


def test_emission_count_edge_semantics():
    # negative / NaN / saturating `as usize`
    assert oracle.compute_emission_count(0.0, 0.5, 1.0, 0.0, 1.0, 10.0)[0] == 0
    # f32::min ignores a NaN operand (IEEE minNum): NaN clock behaves like "end of window"
    assert oracle.compute_emission_count(float("nan"), 0.0, 1.0, 0.0, 1.0, 10.0)[0] == 10
    assert oracle.compute_emission_count(0.5, 0.0, float("nan"), 0.0, 1.0, 10.0)[0] == 10
    assert oracle.compute_emission_count(0.5, 0.0, 1.0, 0.0, 1.0, float("nan"))[0] == 0  # NaN as usize -> 0
    n, _ = oracle.compute_emission_count(1.0, 0.0, 1.0, 0.0, 1.0, float("inf"))  # between = 0 -> x/0 = inf
    assert n == 2**64 - 1
    assert oracle.lib().fwo_div_euclid(-7.0, 2.0) == -4.0 and oracle.lib().fwo_div_euclid(7.0, -2.0) == -3.0
    assert oracle.lib().fwo_rem_euclid(-0.25, 1.0) == 0.75


def test_reference_gradient_unit_test():
    """reference src/curve.rs:246-258"""
    d = load("curve_kat.json")["reference_test"]
    g = S.FireworkGradient.even_samples(d["colors"])
    for s in d["samples"]:
        got = oracle.gradient_sample(g, s["t"])
        assert [b(x) for x in got] == s["rgba_bits"]
    assert list(oracle.gradient_sample(g, 0.5)) == [0.0, 1.0, 0.0, 1.0]


def test_curves_against_numpy_restatement():
    d = load("curve_kat.json")
    sg = d["stress_gradient"]
    gu = S.FireworkGradient.uneven_samples(list(zip(sg["times"], sg["colors"])))
    ge = S.FireworkGradient.even_samples(sg["colors"])
    for s in sg["uneven"]:
        assert [b(x) for x in oracle.gradient_sample(gu, f(s["t_bits"]))] == s["rgba_bits"]
    for s in sg["even"]:
        assert [b(x) for x in oracle.gradient_sample(ge, f(s["t_bits"]))] == s["rgba_bits"]
    for key, mk in [("f32_even_2", lambda c: S.FireworkCurve.even_samples(c["values"])),
                    ("f32_even_3", lambda c: S.FireworkCurve.even_samples(c["values"])),
                    ("f32_uneven_3", lambda c: S.FireworkCurve.uneven_samples(list(zip(c["times"], c["values"])))),
                    ("f32_uneven_messy", lambda c: S.FireworkCurve.uneven_samples(
                        [(float(t), v) for t, v in zip(c["times"], c["values"])]))]:
        c = d[key]
        curve = mk(c)
        for s in c["samples"]:
            assert b(oracle.curve_sample(curve, f(s["t_bits"]))) == s["v_bits"], key


def test_curve_constructors_mirror_reference_panics():
    with pytest.raises(ValueError):
        S.FireworkCurve.even_samples([])
    with pytest.raises(ValueError):
        S.FireworkGradient.uneven_samples([])
    assert S.FireworkCurve.even_samples([3.0]).kind == S.CURVE_CONSTANT
    assert S.FireworkGradient.uneven_samples([(0.3, (1, 2, 3, 4))]).kind == S.CURVE_CONSTANT


def test_philox_published_kat_and_uniform_stream():
    d = load("philox_kat.json")
    for kat in d["published"]:
        assert [int(x) for x in oracle.philox(kat["ctr"], kat["key"])] == kat["out"]
    for u in d["spawn_uniforms"]:
        got = oracle.spawn_uniforms(u["seed"], u["uid"], u["emission_index"], u["serial"])
        assert [b(x) for x in got] == u["u_bits"]
        assert (got >= 0).all() and (got < 1).all()


def _spawner_for(case):
    st = case["settings"]

    def grad(g):
        kind, cols, times = g
        if kind == 0:
            return S.FireworkGradient.constant(cols[0])
        if kind == 1:
            return S.FireworkGradient.even_samples(cols)
        return S.FireworkGradient.uneven_samples(list(zip(times, cols)))

    kind, vals, times = st["scale_curve"]
    sc = (S.FireworkCurve.constant(vals[0]) if kind == 0 else S.FireworkCurve.even_samples(vals) if kind == 1
          else S.FireworkCurve.uneven_samples(list(zip(times, vals))))
    ps = S.ParticleSettings(scale_curve=sc, acceleration=tuple(st["acceleration"]), linear_drag=st["linear_drag"],
                            angular_drag=st["angular_drag"], base_color=grad(st["base_color"]),
                            emissive_color=grad(st["emissive_color"]))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand())
    return S.ParticleSpawner(particle_settings=[ps], emission_settings=[es])


def particle_from_kat(case):
    p = np.zeros(1, dtype=S.PARTICLE_DTYPE)
    p["rotation"][0] = (0, 0, 0, 1)
    for k, v in case["in"].items():
        p[k][0] = [f(x) for x in v] if isinstance(v, list) else f(v)
    return p


def test_update_kats():
    """hand-derived single-particle updates, reference src/core.rs:591-658"""
    d = load("update_kat.json")
    for case in d["cases"]:
        o = oracle.OracleSpawner(_spawner_for(case))
        o.write_particles(0, particle_from_kat(case))
        o.update(f(case["dt_bits"]))
        if not case["alive"]:
            assert o.count(0) == 0, case["name"]
            dead = o.destroyed(0)
            assert len(dead) == 1 and b(dead["age"][0]) == case["out"]["age"]
            # destroyed record keeps the previous frame's pose (core.rs:596-599)
            assert [b(x) for x in dead["position"][0]] == case["in"]["position"]
        else:
            assert o.count(0) == 1, case["name"]
            got = o.particles(0)[0]
            for k, want in case["out"].items():
                gb = [b(x) for x in np.atleast_1d(got[k])]
                assert gb == (want if isinstance(want, list) else [want]), (case["name"], k)
            assert list(got["rotation"]) == [0, 0, 0, 1]  # identity * rot when angular velocity is zero


# ---- multi-frame trajectories of the independent numpy restatement ------------------------------------------
def _scenarios():
    import sys

    sys.path.insert(0, G)
    import scenarios

    return scenarios


@pytest.mark.parametrize("name", ["rotation_cone_sphere", "two_types_circle_oneshot", "nested_sparks_smoke",
                                  "deaths_everywhere", "bouncing_colliders"])
def test_oracle_follows_the_numpy_trajectories(name):
    """tests/golden/trajectories.npz was produced by np_sim.py -- array-oriented numpy, written from the reference
    lines, a different libm -- over scenarios.py.  The C oracle, run over the same inputs, must give the same counts
    and order, bit-identical age / lifetime / scale / colours / last_emitted_age, and vector fields inside the
    tolerance of parity.py: spawn formula, shapes, RandVec3 cones, Nested counting, the quaternion path, destroyed
    records.  (The GPU suite compares the HIP path with the same file, without the oracle in between.)"""
    import parity

    sc_mod = _scenarios()
    sc = sc_mod.ALL[name]()
    o = oracle.OracleSpawner(sc["spawner"], seed=sc_mod.SEED, uid=sc["uid"], transform=sc["transform"])
    if sc["modifier"] is not None:
        o.set_modifier(sc["modifier"])
    o.set_parent_velocity(sc["parent_velocity"])
    o.set_colliders(sc.get("colliders", []))
    n_types = len(sc["spawner"].particle_settings)
    n_em = len(sc["spawner"].emission_settings)
    g = parity.golden()

    def check(fr):
        for t in range(n_types):
            want = parity.golden_particles(name, fr, t)
            got = o.particles(t)
            parity.assert_particles_match(got, want, exact_all=bool(sc.get("exact")), what=f"{name} frame {fr} type {t}")
            lea = g[f"{name}/f{fr}/t{t}/last_emitted_age"]
            for i in range(n_em):
                assert np.array_equal(o.last_emitted(t, i), lea[:, i]), (name, fr, t, i)
            dead = o.destroyed(t)
            assert np.array_equal(dead["age"], g[f"{name}/f{fr}/t{t}/destroyed_age"])
            if len(dead):
                for k in ("position", "velocity"):  # collision deaths carry the NEW position / velocity (core.rs:633-639)
                    ok, _ = parity.trig_field_errors(dead[k], g[f"{name}/f{fr}/t{t}/destroyed_{k}"])
                    assert ok.all() and (not sc.get("exact") or np.array_equal(dead[k], g[f"{name}/f{fr}/t{t}/destroyed_{k}"]))
                assert np.array_equal(dead["scale"], g[f"{name}/f{fr}/t{t}/destroyed_scale"])

    parity.run_scenario(sc, lambda: o.step, check)
    assert sum(o.counts()) > 500


@pytest.mark.parametrize("name", ["mesh_terrain_bouncing", "mesh_terrain_destroying"])
def test_oracle_follows_the_numpy_mesh_trajectories(name):
    """tests/golden/mesh_trajectories.npz: np_sim.py with the brute-force mesh cast of tests/mesh_ref.py over scenarios.MESH (a
    terrain mesh placed twice + an analytic ball).  The oracle's own brute force reproduces every stored field of the live particles
    and of the destroyed records bit for bit (no libm call in these scenes)."""
    import parity

    sc_mod = _scenarios()
    sc = sc_mod.MESH[name]()
    g = np.load(os.path.join(G, "mesh_trajectories.npz"))
    o = oracle.OracleSpawner(sc["spawner"], seed=sc_mod.SEED, uid=sc["uid"], transform=sc["transform"])
    o.set_parent_velocity(sc["parent_velocity"])
    ms = {k: oracle.OracleMesh(*vt) for k, vt in sc["meshes"].items()}
    o.set_colliders(sc["colliders"])
    o.set_mesh_colliders([S.MeshCollider(ms[k], p, q, layers) for k, p, q, layers in sc["mesh_instances"]])
    seen = {"live": 0, "bounced": 0, "dead on contact": 0}

    def check(fr):
        want = parity.golden_particles(name, fr, 0, g)
        got = o.particles(0)
        parity.assert_particles_match(got, want, exact_all=True, what=f"{name} frame {fr}")
        assert np.array_equal(o.last_emitted(0, 0), g[f"{name}/f{fr}/t0/last_emitted_age"][:, 0])
        dead = o.destroyed(0)
        for k in ("age", "position", "velocity", "scale"):
            assert np.array_equal(dead[k], g[f"{name}/f{fr}/t0/destroyed_{k}"]), (name, fr, k)
        seen["live"] = len(got)
        seen["bounced"] += int((got["velocity"][:, 1] > 0).sum())  # (emitted downwards, no acceleration: moving up means a bounce)
        seen["dead on contact"] += int((dead["age"] < dead["lifetime"]).sum())

    parity.run_scenario(sc, lambda: o.step, check)
    # the scene is not empty and the surfaces matter.  Bouncing destroys nothing, and the last checkpoint lies past the longest
    # lifetime, so at least rate x shortest lifetime = 240 x 0.8 = 192 particles live (one less for the emission's rounding);
    # contact deaths leave no such floor, there the records themselves must exist
    if name.endswith("destroying"):
        assert seen["live"] > 0 and seen["dead on contact"] > 0, seen
    else:
        assert seen["live"] >= 191 and seen["bounced"] > 0, seen


def test_mesh_fixture_is_reproducible():
    """the committed mesh trajectories are what np_sim.py + mesh_ref.py produce today"""
    import sys

    sys.path.insert(0, G)
    sys.path.insert(0, os.path.dirname(G))
    import mesh_ref
    import np_sim

    sc_mod = _scenarios()
    name = "mesh_terrain_bouncing"
    sc = sc_mod.MESH[name]()
    g = np.load(os.path.join(G, "mesh_trajectories.npz"))
    sim = np_sim.Spawner(sc["spawner"], sc_mod.SEED, sc["uid"], sc["transform"], sc["modifier"])
    sim.parent_velocity = np.asarray(sc["parent_velocity"], dtype=np.float32)
    ms = {k: mesh_ref.Mesh(*vt) for k, vt in sc["meshes"].items()}
    sim.colliders = mesh_ref.World(list(sc["colliders"]), [mesh_ref.Instance(ms[k], p, q, layers) for k, p, q, layers in sc["mesh_instances"]])
    analytic, np_sim.cast_ray = np_sim.cast_ray, mesh_ref.cast_ray
    try:
        fr = sc["checkpoints"][1]
        for k in range(fr + 1):
            sim.step(np.float32(sc["dts"][k % len(sc["dts"])]))
    finally:
        np_sim.cast_ray = analytic
    for k, v in sim.particles[0].items():
        assert np.array_equal(v.view(np.uint32), g[f"{name}/f{fr}/t0/{k}"].view(np.uint32)), k


def test_fixtures_are_reproducible():
    """the committed trajectories are what np_sim.py produces today (the generator is part of the repo)"""
    import sys

    sys.path.insert(0, G)
    import np_sim

    sc_mod = _scenarios()
    name = "nested_sparks_smoke"
    sc = sc_mod.ALL[name]()
    sim = np_sim.Spawner(sc["spawner"], sc_mod.SEED, sc["uid"], sc["transform"], sc["modifier"])
    sim.parent_velocity = np.asarray(sc["parent_velocity"], dtype=np.float32)
    g = np.load(os.path.join(G, "trajectories.npz"))
    for fr in range(sc["checkpoints"][2] + 1):
        sim.step(np.float32(sc["dts"][fr % len(sc["dts"])]))
    fr = sc["checkpoints"][2]
    for t, p in enumerate(sim.particles):
        for k, v in p.items():
            assert np.array_equal(v.view(np.uint32), g[f"{name}/f{fr}/t{t}/{k}"].view(np.uint32)), (t, k)


def test_particle_collision_against_the_numpy_restatement():
    """particle_collision (core.rs:744-800) + the analytic ray cast: the C oracle and the vectorised numpy restatement
    agree bit for bit on random rays against every collider kind, inside-solid starts, grazing rays, zero velocity,
    the 4-sub-step cap and destroy_on_collision"""
    import math
    import sys

    sys.path.insert(0, G)
    import np_sim

    rng = np.random.default_rng(11)
    cols = [S.Collider.Plane((0, -1, 0), (0.1, 1, 0.05)), S.Collider.Sphere((1, 0.5, 0), 0.8),
            S.Collider.Box((-1.5, 0.3, 0.5), (0.6, 0.4, 0.9), (0.0, math.sin(0.35), 0.0, math.cos(0.35))),
            S.Collider.Sphere((0, 3, 0), 0.5, layers=2)]
    n = 6000
    pos = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    vel = (rng.normal(size=(n, 3)) * rng.choice([0, 0.5, 5, 30], size=(n, 1))).astype(np.float32)
    hits = 0
    for cs in (S.ParticleCollisionSettings(0.6, 0.3), S.ParticleCollisionSettings(0.2, 0.9, True),
               S.ParticleCollisionSettings(1.0, 0.0, False, 2)):
        for dt in (1 / 60, 0.25, 0.0):
            p2, v2, k2 = np_sim.particle_collision(pos, vel, np.float32(dt), cs, cols)
            for i in range(0, n, 5):
                p, v, k = oracle.particle_collision(pos[i], vel[i], np.float32(dt), cs, cols)
                assert np.array_equal(p, p2[i]) and np.array_equal(v, v2[i]) and k == bool(k2[i]), (cs, dt, i)
            hits += int((np.abs(p2 - (pos + vel * np.float32(dt))) > 1e-6).any(axis=1).sum())
    assert hits > 5000
    # hand-checkable: straight down onto the plane y = 0 with restitution 0.5, friction 0.2
    p, v, k = oracle.particle_collision((0, 1, 0), (0, -10, 1), 0.2, S.ParticleCollisionSettings(0.5, 0.2),
                                        [S.Collider.Plane((0, 0, 0), (0, 1, 0))])
    assert np.allclose(v, (0, 5, 0.8), atol=1e-6) and abs(p[1] - 1e-4) < 1e-6 and not k
    # 4-sub-step cap: inside the half-space every sub-step pushes along the velocity, delta is never consumed
    p, v, k = oracle.particle_collision((0, -1, 0), (0, -10, 1), 0.2, S.ParticleCollisionSettings(0.5, 0.2),
                                        [S.Collider.Plane((0, 0, 0), (0, 1, 0))])
    assert np.allclose(p, (0, -9, 0.8), atol=1e-5) and np.array_equal(v, np.float32((0, -10, 1)))


def test_cylinder_and_cone_ray_casts_against_the_numpy_restatement():
    """the two collider kinds the reference's Nested example bounces off (examples/textures.rs:195 Collider::cylinder(4., 0.2),
    :211 Collider::cone(0.5, 1.)): the C oracle and the numpy restatement bit for bit on random rays -- long and short ones,
    starts inside the solids, rays along and across the axis, onto the caps / the base / the lateral surfaces / the apex --
    against upright and rotated instances, and the geometry itself: a hit point lies on the surface it names, its normal is
    the outward unit normal there, nothing is hit from inside out"""
    import math
    import sys

    sys.path.insert(0, G)
    import np_sim

    rng = np.random.default_rng(23)
    q = rng.normal(size=4)
    q = tuple(float(c) for c in (q / np.linalg.norm(q)).astype(np.float32))
    worlds = [[S.Collider.Cylinder((0.0, 0.0, 0.0), 4.0, 0.2)], [S.Collider.Cone((0.0, 0.5, 0.0), 0.5, 1.0)],  # the example's own
              [S.Collider.Cylinder((0.4, -0.2, 0.1), 0.7, 1.6, q)], [S.Collider.Cone((-0.3, 0.1, 0.2), 0.9, 1.3, q)],
              [S.Collider.Cylinder((0.4, -0.2, 0.1), 0.7, 1.6, q), S.Collider.Cone((-0.9, 0.3, 0.2), 0.9, 1.3, q, layers=3),
               S.Collider.Plane((0, -1.5, 0), (0, 1, 0)), S.Collider.Cone((1.5, 0.0, 0.0), 0.4, 0.8)]]
    n = 4000
    pos = rng.uniform(-2.5, 2.5, size=(n, 3)).astype(np.float32)
    pos[: n // 8] *= np.float32(0.2)  # a good share of the starts inside the solids
    vel = (rng.normal(size=(n, 3)) * rng.choice([0, 0.5, 5, 30], size=(n, 1))).astype(np.float32)
    vel[n // 8: n // 4, 0] = 0.0
    vel[n // 8: n // 4, 2] = 0.0          # along the axis of the upright ones
    vel[n // 4: n // 4 + n // 8, 1] = 0.0  # across it
    changed = 0
    for world in worlds:
        for cs in (S.ParticleCollisionSettings(0.6, 0.3), S.ParticleCollisionSettings(0.2, 0.9, True)):
            for dt in (1 / 60, 0.25):
                p2, v2, k2 = np_sim.particle_collision(pos, vel, np.float32(dt), cs, world)
                for i in range(0, n, 3):
                    p, v, k = oracle.particle_collision(pos[i], vel[i], np.float32(dt), cs, world)
                    assert np.array_equal(p, p2[i]) and np.array_equal(v, v2[i]) and k == bool(k2[i]), (world[0].kind, dt, i, p, p2[i], v, v2[i])
                changed += int((np.abs(p2 - (pos + vel * np.float32(dt))) > 1e-6).any(axis=1).sum())
    assert changed > 8000
    # ---- the geometry, on the first hit of single rays (numpy cast_ray: hit mask, distance, unit normal)
    m = 6000  # rays from a shell around the solids towards points near them, and a share of starts inside
    o = rng.normal(size=(m, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 3.0, size=(m, 1))
    o[: m // 6] = rng.uniform(-0.3, 0.3, size=(m // 6, 3))
    tgt = rng.uniform(-0.8, 0.8, size=(m, 3))
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = o.astype(np.float32)
    for c in (S.Collider.Cylinder((0.0, 0.0, 0.0), 0.7, 1.6), S.Collider.Cone((0.0, 0.0, 0.0), 0.9, 1.3)):
        hit, t, nrm = np_sim.cast_ray([c], 0xFFFFFFFF, o, d, np.float32(10.0))
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        pt = o64 + d64 * np.where(hit, t, 0.0).astype(np.float64)[:, None]
        hh, r = c.half_extents[1], c.radius
        rho = np.hypot(pt[:, 0], pt[:, 2])
        outside = hit & (t > 0)
        assert outside.sum() > 300 and (hit & (t == 0)).sum() > 50
        assert np.allclose(np.linalg.norm(nrm[outside], axis=1), 1.0, atol=1e-5)
        assert ((nrm[outside].astype(np.float64) * d64[outside]).sum(axis=1) < 1e-5).all()  # entered against the normal
        if c.kind == S.COLLIDER_CYLINDER:
            cap = outside & (np.abs(nrm[:, 1]) > 0.5)
            side = outside & ~cap
            assert cap.sum() > 50 and side.sum() > 50
            assert np.allclose(np.abs(pt[cap, 1]), hh, atol=1e-4) and (rho[cap] <= r + 1e-4).all()
            assert np.allclose(rho[side], r, atol=1e-4) and (np.abs(pt[side, 1]) <= hh + 1e-4).all()
            assert np.allclose(nrm[side][:, [0, 2]], pt[side][:, [0, 2]] / rho[side, None], atol=1e-4)
            inside = (np.abs(o64[:, 1]) <= hh) & (np.hypot(o64[:, 0], o64[:, 2]) <= r)
        else:
            base = outside & (nrm[:, 1] < -0.99)
            side = outside & ~base
            assert base.sum() > 30 and side.sum() > 50
            assert np.allclose(pt[base, 1], -hh, atol=1e-4) and (rho[base] <= r + 1e-4).all()
            assert np.allclose(rho[side], r * (hh - pt[side, 1]) / (2 * hh), atol=2e-4) and (np.abs(pt[side, 1]) <= hh + 1e-4).all()
            slope = np.array([2 * hh, r]) / math.hypot(2 * hh, r)  # outward normal of the lateral surface: (radial, y) components
            assert np.allclose(nrm[side][:, 1], slope[1], atol=1e-3)
            inside = (o64[:, 1] >= -hh) & (o64[:, 1] <= hh) & (np.hypot(o64[:, 0], o64[:, 2]) <= r * (hh - o64[:, 1]) / (2 * hh))
        assert (t[inside & hit] == 0).all() and (hit[inside]).all()            # solid = true: a start inside hits at distance 0
        assert (nrm[hit & (t == 0)] == 0).all()                                 # ... with a zero normal (core.rs:762-771)


def test_one_lifetime_value_means_the_destroyed_are_always_the_oldest():
    """the premise of the backend's in-place FIFO path, checked on the oracle: with lifetime.min ==
    lifetime.max and any sequence of dt >= 0 -- zero steps, steps longer than the lifetime, several entries feeding the
    type, bursts -- the particles an update destroys are exactly a PREFIX of the list (core.rs:589-600 keeps the
    survivors in order), and the survivors are the old list's tail followed by the frame's new particles"""
    import oracle
    from bevy_firework_amd import settings as S

    rng = np.random.default_rng(2024)
    for case in range(6):
        life = float(rng.uniform(0.05, 0.4))
        ps = S.ParticleSettings(lifetime=S.RandF32.constant(life), linear_drag=0.1, particles_destroyed=lambda dead: None)
        es = [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(float(rng.uniform(500.0, 4000.0)))),
              S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand(), emission_shape=S.EmissionShape.Sphere(1.0)),
              S.EmissionSettings(emission_pacing=S.EmissionPacing.CountOverDuration(300.0, 0.5, 0.2, 0.9))]
        o = oracle.OracleSpawner(S.ParticleSpawner([ps], es), seed=7, uid=case)
        prev = o.particles(0)
        total_dead = 0
        for fr in range(120):
            dt = np.float32(rng.choice([0.0, 1 / 240, 1 / 60, 1 / 30, life * 1.5], p=[0.1, 0.2, 0.5, 0.15, 0.05]))
            if rng.random() < 0.1:
                o.queue_particles(int(rng.integers(1, 800)))
            o.step(dt)
            cur, dead = o.particles(0), o.destroyed(0)
            # destroyed records keep the previous pose (core.rs:596-599): the old ones among them are prev's first entries
            n_old_dead = min(len(dead), len(prev))
            assert np.array_equal(dead["position"][:n_old_dead], prev["position"][:n_old_dead]), (case, fr)
            n_old_alive = len(prev) - n_old_dead
            # ... and the old survivors are prev's tail, in order (same lifetimes; velocities integrate from the same state)
            assert np.array_equal(cur["lifetime"][:n_old_alive], prev["lifetime"][n_old_dead:]), (case, fr)
            if n_old_alive:
                assert np.all(cur["age"][:n_old_alive] == (prev["age"][n_old_dead:] + dt).astype(np.float32))
                assert len(dead) == n_old_dead  # nobody younger died while an older one lived
            assert np.all(np.diff(cur["age"]) <= 0), (case, fr)  # ages never increase along the list
            total_dead += len(dead)
            prev = cur
        assert total_dead > 1000
