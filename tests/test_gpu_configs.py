"""BASELINE.json configs at (or near) full size on the GPU: direct oracle comparison where the oracle
finishes in seconds, size-independent properties everywhere (spawn-order => ages never increase along
the index, every age < lifetime, conservation of particles, finite state)."""
import json
import os

import numpy as np
import pytest

import oracle
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair, assert_particles_match

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture()
def system():
    from bevy_firework_amd.system import ParticleSystem

    with ParticleSystem(device=0, seed=SEED) as ps:
        yield ps


def check_properties(parts, what=""):
    assert np.isfinite(parts["position"]).all() and np.isfinite(parts["velocity"]).all(), what
    assert (parts["age"] < parts["lifetime"]).all(), what  # anything older was compacted away
    assert (np.diff(parts["age"]) <= 0).all(), what        # Vec order == spawn order (stable compaction)
    assert (parts["age"] > 0).all(), what                  # spawned particles are integrated in the same frame


def test_config2_one_million_full_size(system):
    """configs[1]: 1 emitter, rate 1e6, lifetime 1 s; full size, compared with the oracle bit-for-bit on every
    field that involves no trigonometry, 1e-5 on the rest"""
    spawner, tf = workloads.one_million()
    pair = Pair(system, spawner, tf, seed=SEED, uid=0)
    wrap = json.load(open(os.path.join(G, "emission_wrap.json")))["cases"][1]  # rate 1e6
    assert wrap["count"] == 1.0e6
    frames = 64
    entering = 0  # particles that entered update_particles (after spawn), summed over frames
    for fr in range(frames):
        system.update(DT)
        before = pair.cpu.count(0)
        pair.cpu.spawn(DT)
        assert pair.cpu.count(0) - before == wrap["frames"][fr][1]  # golden emission trajectory
        entering += pair.cpu.count(0)
        pair.cpu.update(DT)
    parts = pair.gpu.particles(0)
    cpu = pair.cpu.particles(0)
    assert len(parts) == len(cpu) > 900000
    assert_particles_match(parts, cpu, what="1M full size")
    check_properties(parts, "1M")
    assert system.updated_total() == entering


def test_config2_steady_state_count(system):
    """steady state of rate 1e6 x 1 s at dt 1/60 is 983 333 live (one emission frame lost per cycle wrap)"""
    spawner, tf = workloads.one_million()
    h = system.spawn(spawner, tf, uid=0)
    system.update(DT)
    for _ in range(200):
        system.step(DT)
    assert h.count(0) in (983333, 983334)
    parts = h.particles(0)
    check_properties(parts, "steady 1M")
    inst = h.instances(0)
    assert np.array_equal(inst["position"], parts["position"]) and np.array_equal(inst["scale"], parts["scale"])


def _oracle_emitters(ems, which, frames):
    """the oracle over the emitters `which` of `ems`, one spawner per host thread like par_iter_mut (core.rs:583-585;
    ctypes releases the GIL inside the oracle calls) -> {emitter: OracleSpawner after `frames` steps}"""
    from concurrent.futures import ThreadPoolExecutor

    def run(e):
        o = oracle.OracleSpawner(ems[e][0], seed=SEED, uid=e, transform=ems[e][1])
        for _ in range(frames):
            o.step(DT)
        return e, o

    with ThreadPoolExecutor(max_workers=max(1, min(len(which), os.cpu_count() or 1))) as ex:
        return dict(ex.map(run, which))


def _compare_all_emitters(handles, cpu, what):
    """EVERY emitter against its oracle run: count, order, exact fields bit for bit, vector fields inside the tolerance"""
    from concurrent.futures import ThreadPoolExecutor

    got = {e: handles[e].particles(0) for e in cpu}  # (GPU reads are serialised on the context)

    def cmp(e):
        assert_particles_match(got[e], cpu[e].particles(0), what=f"{what} emitter {e}")
        check_properties(got[e], f"{what} emitter {e}")
        return len(got[e])

    with ThreadPoolExecutor(max_workers=max(1, min(len(cpu), os.cpu_count() or 1))) as ex:
        return sum(ex.map(cmp, list(cpu)))


def test_config3_many_emitters_full_size(system):
    """configs[2]: 256 emitters x 64Ki, Sphere + radial velocity, per-emitter constants (table spawn path).
    Emitters are independent and RNG streams are keyed by uid: ALL 256 are compared with the oracle, run
    emitter-by-emitter on the host's threads (75 frames: the oldest particles, lifetimes 0.8-1.2 s, have been dying for
    27 frames in every tile)."""
    ems = workloads.many_emitters(256, 65536)
    handles = [system.spawn(sp, tf, uid=e) for e, (sp, tf) in enumerate(ems)]
    frames = 75
    system.update(DT)
    for _ in range(frames - 1):
        system.step(DT)
    cpu = _oracle_emitters(ems, list(range(256)), frames)
    total = 0
    for e, h in enumerate(handles):
        c = h.count(0)
        total += c
        assert 55000 < c < 72000, (e, c)
        assert c == cpu[e].count(0), (e, c, cpu[e].count(0))
    assert system.live_count() == total and total > 15_000_000
    assert _compare_all_emitters(dict(enumerate(handles)), cpu, "configs[2]") == total


def test_config5_shard_of_4096_emitters(system):
    """configs[4], one GPU's share: emitters 3, 11, 19, ... (rank 3 of 8) of the 4096 x 8192 workload -- all 512 of them
    against the oracle"""
    ems = workloads.many_emitters(4096, 8192)
    from bevy_firework_amd import sharding

    mine = sharding.local_indices(4096, 3, 8)
    assert len(mine) == 512
    handles = {e: system.spawn(ems[e][0], ems[e][1], uid=e) for e in mine}
    frames = 80
    system.update(DT)
    for _ in range(frames - 1):
        system.step(DT)
    cpu = _oracle_emitters(ems, mine, frames)
    total = _compare_all_emitters(handles, cpu, "configs[4] rank 3 of 8")
    assert system.live_count() == total and 3_500_000 < total < 4_700_000


def test_config4_nested_mid_size(system):
    """configs[3] shape: sparks -> smoke with ~0.8M live smoke, compared with the oracle"""
    spawner, tf = workloads.nested(spark_rate=20000.0, smoke_per_spark=20.0)
    pair = Pair(system, spawner, tf, seed=SEED, uid=2)
    for fr in range(130):
        system.update(DT)
        pair.step_cpu(DT)
    pair.check(what="nested mid")
    assert np.array_equal(pair.gpu.last_emitted(0, 1), pair.cpu.last_emitted(0, 1))
    c = pair.gpu.counts()
    assert c[0] > 35000 and c[1] > 300000


NESTED_FRAMES = 260                    # both lifetimes are 2.0 s = 120 frames: 140 frames of steady-state deaths
NESTED_FULL = (110, 125, 165, 259)     # whole state compared (before any death / first deaths / after the spark ring wrapped
                                       # and the smoke segment's reallocation / the 3.9M steady state)
NESTED_DIGEST = (69, 84, 140, 200, 230)  # counts + exact digests only
_nested_oracle = {}


def _digest(parts):
    """order-sensitive digest of the fields that involve no trigonometry (bit-exact by contract)"""
    import zlib

    return (len(parts),) + tuple(zlib.crc32(np.ascontiguousarray(parts[f]).tobytes()) for f in
                                 ("age", "lifetime", "initial_scale", "scale", "base_color", "emissive_color"))


def nested_full_oracle():
    """the oracle over configs[3] at its full rates for NESTED_FRAMES frames, run ONCE per session (a single spawner is
    serial on the CPU, core.rs:586: ~1.5 minutes) and shared by the two update paths of the test below"""
    if not _nested_oracle:
        spawner, tf = workloads.nested(spark_rate=100000.0, smoke_per_spark=20.0)
        o = oracle.OracleSpawner(spawner, seed=SEED, uid=2, transform=tf)
        for fr in range(NESTED_FRAMES):
            o.step(DT)
            if fr in NESTED_FULL or fr in NESTED_DIGEST:
                parts = [o.particles(t) for t in (0, 1)]
                _nested_oracle[fr] = {"counts": o.counts(), "digest": [_digest(p) for p in parts],
                                      "lea": o.last_emitted(0, 1).copy(),
                                      "parts": [p.copy() for p in parts] if fr in NESTED_FULL else None}
        o.close()
    return _nested_oracle


def test_config4_nested_full_rate_steady_state(system):
    """configs[3] at its full emission rates (100 000 sparks/s, 20 smoke per spark -> 3.93M live) THROUGH its steady state:
    260 frames, i.e. 140 frames past both lifetimes -- sparks and smoke die every frame, ring heads move and the spark
    ring wraps (ring path), the compacting path runs its SUMS forecast over > 2048 tiles with MATERIALISED new-particle
    tiles, the device-counted smoke segment passes its growth threshold.  The whole state of both types (counts, order,
    exact fields bit for bit, vector fields inside the tolerance, last_emitted_age) is compared with the oracle at four
    frames, counts and order-sensitive digests of the exact fields at five more."""
    want = nested_full_oracle()
    spawner, tf = workloads.nested(spark_rate=100000.0, smoke_per_spark=20.0)
    h = system.spawn(spawner, tf, uid=2)
    for fr in range(NESTED_FRAMES):
        system.update(DT)
        if fr not in want:
            continue
        w = want[fr]
        assert h.counts() == w["counts"], (fr, h.counts(), w["counts"])
        parts = [h.particles(t) for t in (0, 1)]
        assert [_digest(p) for p in parts] == w["digest"], f"frame {fr}: exact-field digests differ"
        assert np.array_equal(h.last_emitted(0, 1), w["lea"]), f"frame {fr}: last_emitted_age"
        for t in (0, 1):
            assert np.isfinite(parts[t]["position"]).all() and (parts[t]["age"] < parts[t]["lifetime"]).all(), (fr, t)
            assert (np.diff(parts[t]["age"]) <= 0).all(), (fr, t)  # parent-major children, spawn order kept
            if w["parts"] is not None:
                assert_particles_match(parts[t], w["parts"][t], what=f"nested full rate, frame {fr}, type {t}")
    c = h.counts()
    assert c[1] > 3_700_000 and c[0] > 190_000, c
    assert want[259]["counts"] == want[230]["counts"]  # the steady state was reached: deaths balance the spawns


def test_config4_nested_with_lifetime_ranges_on_range_rings(monkeypatch):
    """configs[3]'s spawner with lifetimes that are RANGES (1.6-2.4 s, sparks and smoke alike) at its full rates, with the
    PRODUCT'S DEFAULT thresholds: both types live in range rings (round 4) -- the sparks' ring is addressed by fw_k_nest
    through the size of its old part (FwGlobals::rold), its new particles are spawned inside the update kernel and carry the
    last_emitted_age the frame's Nested pass would have left (fw_init_last_emitted); the smoke ring's particle count is known
    to the device alone (FW_RREC_DEV), its cohorts join the old part by sizes read from the pinned report ring a lifetime.min
    later.  170 frames (26 past the longest lifetime: both types lose particles every frame, the old parts are compacted in
    place, last_emitted_age planes move with the surviving sparks) against the oracle: the whole state at two frames, counts
    and digests of the exact fields at three more, > 3M particles."""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setenv("FW_ENABLE_KNOBS", "1")
    for k in ("FW_FIFO", "FW_FIFO_MIN", "FW_RANGE", "FW_RANGE_MIN"):
        monkeypatch.delenv(k, raising=False)
    spawner, tf = workloads.nested(spark_rate=100000.0, smoke_per_spark=20.0)
    for ps in spawner.particle_settings:
        ps.lifetime = S.RandF32(1.6, 2.4)
    full, digest = (150, 169), (60, 100, 160)
    o = oracle.OracleSpawner(spawner, seed=SEED, uid=2, transform=tf)
    want = {}
    for fr in range(170):
        o.step(DT)
        if fr in full or fr in digest:
            parts = [o.particles(t) for t in (0, 1)]
            want[fr] = {"counts": o.counts(), "digest": [_digest(p) for p in parts], "lea": o.last_emitted(0, 1).copy(),
                        "parts": [p.copy() for p in parts] if fr in full else None}
    o.close()
    with ParticleSystem(device=0, seed=SEED) as system:
        h = system.spawn(spawner, tf, uid=2)
        assert [h.update_path(t)[0] for t in (0, 1)] == ["range", "range"]
        for fr in range(170):
            system.update(DT)
            if fr not in want:
                continue
            w = want[fr]
            assert h.counts() == w["counts"], (fr, h.counts(), w["counts"])
            parts = [h.particles(t) for t in (0, 1)]
            assert [_digest(p) for p in parts] == w["digest"], f"frame {fr}: exact-field digests differ"
            assert np.array_equal(h.last_emitted(0, 1), w["lea"]), f"frame {fr}: last_emitted_age"
            for t in (0, 1):
                assert (parts[t]["age"] < parts[t]["lifetime"]).all() and (np.diff(parts[t]["age"]) <= 0).all(), (fr, t)
                if w["parts"] is not None:
                    assert_particles_match(parts[t], w["parts"][t], what=f"nested lifetime ranges, frame {fr}, type {t}")
        assert [h.update_path(t)[0] for t in (0, 1)] == ["range", "range"]
        c = h.counts()
        assert c[1] > 3_000_000 and c[0] > 150_000, c


def test_single_segment_beyond_the_entry_table(system):
    """one particle type with more than FW_FC_DIRECT (2048) tiles: the survivor forecast switches from one plain entry
    per tile to atomic per-tile sums + group sums, and back when enough particles have died; counts, order and
    state must not notice (2.3M particles burst, lifetimes spread so that deaths hit every tile every frame)"""
    ps = S.ParticleSettings(lifetime=S.RandF32(0.05, 0.9), linear_drag=0.1, acceleration=(0.0, -9.81, 0.0))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.OneShot(2_300_000),
                            initial_velocity=S.RandVec3(S.RandF32(0.0, 3.0), (0.0, 1.0, 0.0), 0.0))
    trickle = S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(30000.0),
                                 initial_velocity=S.RandVec3(S.RandF32(0.0, 3.0), (0.0, 1.0, 0.0), 0.0))
    pair = Pair(system, S.ParticleSpawner([ps], [es, trickle]), seed=SEED, uid=77)
    counts = []
    for fr in range(34):
        system.update(DT)
        pair.step_cpu(DT)
        counts.append(pair.gpu.count(0))
        if fr in (1, 4, 9, 14, 20, 27, 33):
            pair.check(exact_all=True, what=f"frame {fr}")
    assert counts[0] > 2_200_000 and counts[-1] < 1_200_000  # crossed the 2048-tile boundary on the way down
    check_properties(pair.gpu.particles(0), "end")


@pytest.mark.parametrize("which", ["configs1", "configs3_nested", "stress_test"])
def test_the_two_update_paths_agree_bit_for_bit_at_full_size(which, monkeypatch):
    """the in-place ring paths (FIFO rings, range rings) and the compacting path are implementations of the same update: at BASELINE sizes, over a
    sequence of irregular steps, every field of every particle (trigonometry included: same device functions), the
    destroyed-particle stream's length and the AABB must be IDENTICAL between a context with rings and one without"""
    from bevy_firework_amd.system import ParticleSystem

    make = {"configs1": lambda: workloads.one_million(), "configs3_nested": lambda: workloads.nested(50000.0, 20.0),
            "stress_test": lambda: workloads.stress_test(160000.0)}[which]
    rng = np.random.default_rng(77)
    # (135 regular frames first: the 2.0 s lifetimes of configs[3] have passed, deaths and ring heads are in play)
    dts = [np.float32(1 / 60)] * 135 + [np.float32(x) for x in rng.uniform(0.004, 0.03, size=40)] + [np.float32(0.0), np.float32(1 / 60)] * 3
    states = {}
    for mode in ("fifo", "range", "general"):
        monkeypatch.setenv("FW_FIFO", "1" if mode == "fifo" else "0")
        monkeypatch.setenv("FW_FIFO_MIN", "0")
        monkeypatch.setenv("FW_RANGE", "1" if mode == "range" else "0")
        monkeypatch.setenv("FW_RANGE_MIN", "0")
        monkeypatch.setenv("FW_SMALL", "0")
        with ParticleSystem(device=0, seed=SEED) as ps:
            sp, tf = make()
            h = ps.spawn(sp, tf, uid=5)
            # (round 4: the types of a spawner with Nested entries live in range rings too -- parents addressed through the old
            # part's size the device keeps, children counted by the device alone)
            assert h.update_path(0)[0] == mode, (mode, h.update_path(0))
            if which == "configs3_nested":
                assert h.update_path(1)[0] == mode, (mode, h.update_path(1))
            snaps = []
            for fr, dt in enumerate(dts):
                ps.update(dt)
                if fr in (69, 134, 155, len(dts) - 1):
                    snaps.append([h.particles(t).copy() for t in range(len(sp.particle_settings))] + [h.aabb()])
            states[mode] = snaps
    for other in ("fifo", "range"):
        for a, b in zip(states[other], states["general"]):
            for pa, pb in zip(a[:-1], b[:-1]):
                assert len(pa) == len(pb) and len(pa) > 10000
                assert pa.tobytes() == pb.tobytes(), other
            assert a[-1][0] == b[-1][0] and np.array_equal(a[-1][1], b[-1][1]) and np.array_equal(a[-1][2], b[-1][2]), other


def _run_collision_example(monkeypatch, general, spawner, tf, world, frames, check_every, exact_all):
    """`frames` frames of a colliding spawner on the ring path (product defaults) or on the count -> scan -> fw_k_update_coll
    path, against the oracle at the checkpoints; returns the final particle state"""
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setenv("FW_ENABLE_KNOBS", "1")
    for k in ("FW_FIFO", "FW_FIFO_MIN", "FW_RANGE", "FW_RANGE_MIN"):
        monkeypatch.delenv(k, raising=False)
    if general:  # (... and not on the wave- / workgroup-per-type kernel either, whose COLL instantiation takes colliding types too)
        monkeypatch.setenv("FW_FIFO", "0"), monkeypatch.setenv("FW_RANGE", "0"), monkeypatch.setenv("FW_SMALL", "0")
    with ParticleSystem(device=0, seed=SEED) as system:
        system.set_colliders(world)
        pair = Pair(system, spawner, tf, seed=SEED, uid=0)
        pair.cpu.set_colliders(world)
        assert pair.gpu.update_path(0)[0] == ("general" if general else "fifo")
        for fr in range(frames):
            system.update(DT)
            pair.step_cpu(DT)
            if fr % check_every == check_every - 1 or fr == frames - 1:
                assert pair.gpu.counts() == pair.cpu.counts()
                g, c = pair.gpu.particles(0), pair.cpu.particles(0)
                if exact_all:
                    assert_particles_match(g, c, True, f"frame {fr}")
                else:  # fields without trigonometry in their history: bit-exact whatever the particle hit
                    for f in ("age", "lifetime", "initial_scale", "scale", "base_color", "emissive_color"):
                        assert np.array_equal(g[f], c[f]), (f, fr)
                check_properties(g, f"frame {fr}")
        return pair.gpu.particles(0), pair.cpu.particles(0)


def test_stress_test_collision_example(monkeypatch):
    """examples/stress_test_collision.rs:92-151 at full size (rate 80 000/s x 2 s = ~157k live): particles that bounce off the
    ground slab and the angled cube, destroy_on_collision false.  A bounce changes neither age, lifetime nor order
    (core.rs:607-643), so with the product's defaults the type lives in a FIFO ring and the frame is ONE launch
    (fw_k_update_fifo<.., COLL>).  Checked three ways: (1) the ring path and the count -> scan -> fw_k_update_coll path agree
    BIT FOR BIT on every field (same device, same arithmetic); (2) against the oracle every field whose history holds no
    trigonometry is bit-exact; (3) position and velocity against the oracle: the spawn cone goes through sin / cos (device
    OCML vs the oracle's glibc: a last-bit difference in the initial velocity), and a bounce amplifies that difference --
    the hit point moves along the face, a ray that grazes an edge of the angled cube may take the other face -- so for
    particles that have bounced the usual 1e-5 does not bound it for any two libm's; the trig-free variant below is the
    bit-exact statement about the collision arithmetic itself.  Here: 99.9 % of the particles inside 1e-4 (round 6,
    profiles/r06/parity_error_budget.txt: 68 of 472 002 position elements are outside 1e-5 relative to the vector's length, the worst by
    5.6e-4 absolute; rounds 4-5 allowed 1 %), all of the young ones
    (age < 0.3 s: nothing within reach yet) inside the allowance of tests/parity.py."""
    spawner, tf, world = workloads.stress_test_collision()
    ring, cpu = _run_collision_example(monkeypatch, False, spawner, tf, world, 150, 30, False)
    general, _ = _run_collision_example(monkeypatch, True, spawner, tf, world, 150, 30, False)
    assert len(ring) == len(general) == len(cpu) > 150000
    for f in ring.dtype.names:
        assert np.array_equal(ring[f].view(np.uint32) if ring[f].dtype == np.float32 else ring[f],
                              general[f].view(np.uint32) if general[f].dtype == np.float32 else general[f]), f
    young = cpu["age"] < 0.3
    assert_particles_match(ring[young], cpu[young], what="young particles")
    for f in ("position", "velocity"):
        want = cpu[f].astype(np.float64)
        err = np.abs(ring[f].astype(np.float64) - want).max(axis=1)
        allow = 1e-4 * np.maximum(np.sqrt((want * want).sum(axis=1)), 1.0)
        assert np.count_nonzero(err > allow) < 0.001 * len(cpu), (f, int(np.count_nonzero(err > allow)))
    # nobody fell through the slab (its top face is y = 0; a bounce leaves the particle 1e-4 above the face it hit)
    p = ring
    inside = (np.abs(p["position"][:, 0]) < 3.9) & (np.abs(p["position"][:, 2]) < 3.9)
    assert (p["position"][inside, 1] > -1e-3).all()
    # ... and a good part of the old particles is moving UP again: they have bounced
    assert np.count_nonzero((p["age"] > 1.2) & (p["velocity"][:, 1] > 0.0)) > 1000


@pytest.mark.parametrize("general", [False, True])
def test_stress_test_collision_without_trigonometry_is_bit_exact(monkeypatch, general):
    """the same scene with Point emission and a zero-spread velocity (random magnitude along the rotated emitter's axis, a
    sideways drift from the parent velocity): no sin / cos anywhere, and particle_collision itself calls no libm function --
    the WHOLE state is bit-exact against the oracle through two seconds of bounces, on the ring path and on the
    count -> scan -> fw_k_update_coll path"""
    spawner, tf, world = workloads.stress_test_collision()
    es = spawner.emission_settings[0]
    es = S.EmissionSettings(emission_pacing=es.emission_pacing, emission_shape=S.EmissionShape.Point(),
                            initial_velocity=S.RandVec3(S.RandF32(3.0, 9.0), (0.0, 1.0, 0.0), 0.0), inherit_parent_velocity=True)
    spawner = S.ParticleSpawner(spawner.particle_settings, [es])
    g, c = _run_collision_example(monkeypatch, general, spawner, tf, world, 150, 30, True)
    assert len(g) > 150000
    assert np.count_nonzero((g["age"] > 1.2) & (g["velocity"][:, 1] > 0.0)) > 1000  # they do bounce


@pytest.mark.parametrize("general", [False, True])
def test_stress_test_collision_with_the_boxes_as_meshes_is_bit_exact(monkeypatch, general):
    """the trig-free variant above with the example's two cuboids as 12-triangle meshes (tests/mesh_ref.py: box_mesh) at the boxes'
    positions and rotations: the whole state bit for bit against the oracle's brute force through two seconds of bounces, on the
    ring path (fw_k_update_fifo's mesh form) and on count -> scan -> fw_k_update_coll<MESH>; and a particle that has touched
    nothing in the analytic world -- it equals the same particle of a world without colliders -- is the same in all three runs"""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mesh_ref
    import oracle
    from bevy_firework_amd.system import ParticleSystem
    from parity import MeshPair

    spawner, tf, world = workloads.stress_test_collision(rate=20000.0)
    es = spawner.emission_settings[0]
    es = S.EmissionSettings(emission_pacing=es.emission_pacing, emission_shape=S.EmissionShape.Point(),
                            initial_velocity=S.RandVec3(S.RandF32(3.0, 9.0), (0.0, 1.0, 0.0), 0.0), inherit_parent_velocity=True)
    spawner = S.ParticleSpawner(spawner.particle_settings, [es])
    frames = 150
    analytic, _ = _run_collision_example(monkeypatch, general, spawner, tf, world, frames, 30, True)
    free = oracle.OracleSpawner(spawner, seed=SEED, uid=0, transform=tf)
    with ParticleSystem(device=0, seed=SEED) as system:  # (the knobs _run_collision_example set are still in place)
        pair = Pair(system, spawner, tf, seed=SEED, uid=0)
        boxes = [(MeshPair(system, *mesh_ref.box_mesh(c.half_extents)), c.position, c.rotation, c.layers) for c in world]
        pair.set_world([], boxes)
        assert pair.gpu.update_path(0)[0] == ("general" if general else "fifo")
        for fr in range(frames):
            system.update(DT)
            pair.step_cpu(DT)
            free.step(DT)
            if fr % 30 == 29:
                pair.check(exact_all=True, what=f"frame {fr}")
        g, f = pair.gpu.particles(0), free.particles(0)
    assert len(g) == len(analytic) == len(f) > 35000
    untouched = (analytic["position"] == f["position"]).all(axis=1) & (analytic["velocity"] == f["velocity"]).all(axis=1)
    assert 3000 < untouched.sum() < len(g) - 3000, int(untouched.sum())
    for k in g.dtype.names:
        assert np.array_equal(g[k][untouched], analytic[k][untouched]), k
    assert np.count_nonzero((g["age"] > 1.2) & (g["velocity"][:, 1] > 0.0)) > 250  # they do bounce off the triangles
