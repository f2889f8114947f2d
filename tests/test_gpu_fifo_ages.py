"""The age rule of FIFO rings (fw_device.h: FW_TYPE_IDX_AGELESS): a streaming launch of a ring fed by Global entries alone
neither loads nor stores the age plane, and fw_k_fifo_ages writes the host's cohort ages back before anybody looks.  Every case runs
the same system twice -- with the rule and with FW_AGELESS=0 -- against the CPU oracle (tests/parity.py), and every field of every
read, `age` first of all, must carry the same bits in both runs.  The four-round form is forced at small sizes (FW_FIFO_SMALL=1): a ring
built with 8192 slots (it grows to what its lifetime needs, 1.5 to 16 frames), ~5000 particles per spawn cohort -- one or two cohort
boundaries inside a tile -- whose head wraps every few frames.  Needs an MI355X."""
import dataclasses

import numpy as np
import pytest

import first_readers
import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
Y = (0.0, 1.0, 0.0)


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the age rule belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _spawner(life_frames=2.5, rate=300000.0, capacity=8192, spin=False, on_demand=False, **kw):
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(float(DT) * life_frames), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]), capacity=capacity,
                            base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT), **kw)
    es = [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(rate), initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), Y, 0.0),
                             initial_velocity_radial=S.RandF32(0.0, 1.0),
                             initial_angular_velocity=S.RandVec3(S.RandF32(1.0, 4.0) if spin else S.RandF32(0.0, 0.0), Y, 0.0))]
    if on_demand:
        es.append(S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand()))
    return S.ParticleSpawner([ps], es)


class Run:
    """one of the two runs of a case: the system, the spawner next to its oracle twin, and everything the case reads"""

    def __init__(self, system, pair, rule):
        self.system, self.pair, self.rule, self.reads, self.frame = system, pair, rule, [], 0

    def step(self, dt=DT, n=1):
        for _ in range(n):
            dt = np.float32(dt)
            self.system.update(dt)
            self.pair.step_cpu(dt)
            self.frame += 1

    def read(self, what="", exact=True, check=True):
        if check:
            self.pair.check(exact_all=exact, what=f"{what} frame {self.frame} rule={self.rule}")
        for t in range(self.pair.n_types):
            self.keep(f"{what} frame {self.frame} type {t}", self.pair.gpu.particles(t))

    def keep(self, what, arr):
        self.reads.append((what, np.ascontiguousarray(arr).tobytes()))

    def bytes_moved(self, t=0):
        return self.pair.gpu.update_path(t)


def both(monkeypatch, spawner, scenario, fifo_small="1", range_rings="0", transform=None, **env):
    """runs `scenario(run)` with the rule and without it; -> the two byte figures the scenario returned"""
    from bevy_firework_amd.system import ParticleSystem

    figures, reads = {}, {}
    for rule in (True, False):
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", range_rings), ("FW_SMALL", "0"),
                     ("FW_AGELESS", "1" if rule else "0")) + tuple(env.items()):
            monkeypatch.setenv(k, v)
        for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN"):  # (the product's choice, whatever the path matrix dealt this test)
            monkeypatch.delenv(k, raising=False)
        if fifo_small is None:
            monkeypatch.delenv("FW_FIFO_SMALL", raising=False)
        else:
            monkeypatch.setenv("FW_FIFO_SMALL", fifo_small)
        with ParticleSystem(device=0, seed=SEED) as system:
            run = Run(system, Pair(system, spawner, transform or S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=18), rule)
            figures[rule] = scenario(run)
            reads[rule] = run.reads
    assert [w for w, _ in reads[True]] == [w for w, _ in reads[False]] and len(reads[True]) > 0
    for (what, a), (_, b) in zip(reads[True], reads[False]):
        assert a == b, f"{what}: the bits differ between the run under the age rule and the run with FW_AGELESS=0"
    return figures[True], figures[False]


def _expect_rule(run, unflagged=None):
    """after a streaming frame: a FIFO ring, 8 bytes fewer than without the rule (`unflagged`: the figure of a ring that does not carry it)"""
    path = run.bytes_moved()
    assert path[0] == "fifo", path
    if unflagged is not None:
        assert path[1] == unflagged[1] - (8 if run.rule else 0), (path, unflagged, run.rule)
    return path


@pytest.mark.parametrize("spin", [False, True], ids=["cannot turn", "spins about y"])
@pytest.mark.parametrize("every, life_frames", [(1, 1.5), (7, 16.0), (0, 2.5)], ids=["every frame", "every 7th frame", "only at the end"])
def test_reads_at_any_rhythm(monkeypatch, every, life_frames, spin):
    def scenario(run):
        before = run.bytes_moved()
        for fr in range(30):
            run.step()
            if every and fr % every == every - 1:
                run.read(exact=not spin)
        path = _expect_rule(run, before)
        run.read("end", exact=not spin)
        assert 4000 < run.pair.gpu.count(0) < 5500 * life_frames
        assert _expect_rule(run, before) == path  # (a read writes the ages back; the figure is the latest launch's)
        return path

    on, off = both(monkeypatch, _spawner(life_frames=life_frames, spin=spin), scenario)
    assert on[1] == off[1] - 8 and on[0] == off[0] == "fifo"


def test_a_ring_at_product_defaults_keeps_its_figure(monkeypatch):
    """4500 particles are a handful of tiles: one-round workgroups, nothing bound by bandwidth -- the rule is not set and the ring
    reports what it reported before this round"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=12)
        run.read()
        assert 4000 < run.pair.gpu.count(0) < 5000 and run.bytes_moved() == before
        return before

    on, off = both(monkeypatch, _spawner(life_frames=1.5, rate=270000.0, capacity=8192), scenario, fifo_small=None)
    assert on == off and on[0] == "fifo"


def test_jittering_zero_and_denormal_dt(monkeypatch):
    """any dt >= 0 keeps the rule except one the two sides might add differently: a denormal drops it for its frame (the ages are
    written back first, the kernel adds for itself) and the next frame carries it again"""
    rng = np.random.default_rng(18)
    dts = [float(x) for x in rng.uniform(0.004, 0.02, size=10)] + [0.0, 0.0, 0.012, 0.0] + [float(x) for x in rng.uniform(0.004, 0.02, size=4)]
    tiny = np.float32(1e-40)
    assert tiny != 0 and tiny < np.finfo(np.float32).tiny

    def scenario(run):
        before = run.bytes_moved()
        for k, dt in enumerate(dts):
            run.step(dt)
            if k in (3, 11, 13):
                run.read(f"dt {dt}")
        flagged = _expect_rule(run, before)
        run.step(tiny)
        assert run.bytes_moved() == before  # (the rule dropped for this frame ...)
        run.step(0.011)
        assert run.bytes_moved() == flagged  # (... and is back)
        run.read("after the denormal")
        run.step(tiny)
        run.read("right after a denormal")
        run.step(0.0625)  # (longer than anybody lives: everything dies, the particles of that very frame included)
        run.read("after dt >= lifetime")
        assert run.pair.gpu.count(0) == 0
        run.step(n=3)
        run.read("refilled")
        return _expect_rule(run, before)

    both(monkeypatch, _spawner(), scenario)


def test_negative_dt_ends_the_mode_with_stale_ages(monkeypatch):
    """the ring leaves for the compacting path (unwrapped and transposed, fifo_to_general) after frames nobody read: the ages it takes
    along are the written-back ones"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=11)
        _expect_rule(run, before)
        run.step(-1.0 / 240.0)
        assert run.bytes_moved()[0] == "general"
        run.read("after the negative step")
        run.step(n=4)
        run.read("on the compacting path")

    both(monkeypatch, _spawner(), scenario)


def test_instance_buffer_attached_and_detached(monkeypatch):
    """records need the age (scale and colours): the rule is off while a buffer is attached and comes back when it goes"""
    import torch

    def scenario(run):
        before = run.bytes_moved()
        cap = 16384
        buf = torch.full((cap * 16,), float("nan"), dtype=torch.float32, device="cuda")
        run.step(n=9)
        flagged = _expect_rule(run, before)
        run.pair.gpu.attach_instances(buf.data_ptr(), cap)
        for k in range(6):
            run.step()
            n = run.pair.gpu.count(0)
            run.keep(f"records {k}", buf[: n * 16].cpu().numpy())
            assert np.array_equal(buf[: n * 16].cpu().numpy().view(np.uint32), run.pair.gpu.instances(0).view(np.uint32).reshape(-1))
        assert run.bytes_moved()[1] == before[1] + 64 + 4
        run.read("attached")
        run.pair.gpu.attach_instances(0, 0)
        run.read("right after detaching")
        run.step(n=8)
        assert run.bytes_moved() == flagged
        run.read("detached")

    both(monkeypatch, _spawner(), scenario)


def test_caller_written_particles(monkeypatch):
    """fw_spawner_write_particles after an unread stretch: the ages are written back, the ring unwrapped, then the caller's records land"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        _expect_rule(run, before)
        parts = run.pair.cpu.particles(0)[::2].copy()
        run.pair.gpu.write_particles(0, parts)
        run.pair.cpu.write_particles(0, parts)
        run.read("right after the write")
        run.step(n=3)
        run.read("after the write")

    both(monkeypatch, _spawner(), scenario)


def test_growth_with_stale_ages(monkeypatch):
    """a burst far beyond the capacity while the ages are stale and the head sits in the middle of the buffer: the larger ring receives
    the written-back plane"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        _expect_rule(run, before)
        run.pair.queue(40000)
        run.step()
        run.step(n=2)
        _expect_rule(run, before)
        run.read("grown")
        assert run.pair.gpu.count(0) > 40000
        run.step(n=3)
        run.read("after the burst died")

    both(monkeypatch, _spawner(life_frames=3.5, on_demand=True), scenario)


def test_ring_becomes_a_range_ring_where_it_stands(monkeypatch):
    """the ninth one-lifetime type of a context takes a range ring and the FIFO rings follow it where they stand (fifo_to_range,
    fw_ctx::n_spilled): position + age are transposed in place, after the ages have been written back"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        _expect_rule(run, before)
        small = S.ParticleSpawner([S.ParticleSettings(lifetime=S.RandF32.constant(0.2), capacity=1024)],
                                  [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(600.0))])
        others = [run.system.spawn(small, uid=200 + k) for k in range(8)]
        assert run.bytes_moved()[0] == "range", (run.bytes_moved(), [o.update_path(0)[0] for o in others])
        run.read("right after the change")
        run.step(n=5)
        run.read("as a range ring")

    both(monkeypatch, _spawner(), scenario, range_rings="1", FW_RANGE_MIN="0")


def test_nested_entry_never_sets_the_rule(monkeypatch):
    """a ring other particles' entries emit from, and the ring that receives the children: the unflagged figure, before and after"""
    # (the spawner of tests/test_gpu_fifo.py's Nested cases: derived capacities, both rings grow on their own)
    sparks = S.ParticleSettings(lifetime=S.RandF32.constant(0.5), initial_scale=S.RandF32(0.01, 0.03), linear_drag=0.3,
                                base_color=S.FireworkGradient.even_samples([(8.0, 4.0, 1.0, 1.0), (1.0, 0.2, 0.0, 0.0)]))
    smoke = S.ParticleSettings(lifetime=S.RandF32.constant(0.4), initial_scale=S.RandF32(0.05, 0.1), acceleration=(0.0, 0.5, 0.0))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(3000.0), initial_velocity=S.RandVec3(S.RandF32(2.0, 6.0), Y, 0.0))
    e1 = S.EmissionSettings(particle_index=1, emission_pacing=S.EmissionPacing.rate(20.0), emission_mode=S.EmissionMode.Nested(0),
                            inherit_parent_velocity=False)

    def scenario(run):
        before = [run.bytes_moved(t) for t in (0, 1)]
        assert [b[0] for b in before] == ["fifo", "fifo"]
        run.step(n=40)
        assert [run.bytes_moved(t) for t in (0, 1)] == before
        run.read("nested")
        assert run.pair.gpu.count(0) > 1400 and run.pair.gpu.count(1) > 5000
        return before

    on, off = both(monkeypatch, S.ParticleSpawner([sparks, smoke], [e0, e1]), scenario)
    assert on == off


def test_queries_right_after_an_unread_stretch(monkeypatch):
    """the AABB query (which evaluates every particle's scale from its age) and one ray, nearest-point and path query, first thing after
    twelve frames nobody read"""
    world = [S.Collider.Sphere((1.0, 4.0, 3.0), 1.5), S.Collider.Plane((0.0, 0.0, 0.0), Y)]
    path_settings = S.PathSettings(0.03125, 8, (0.0, -9.75, 0.0), 0.125, S.ParticleCollisionSettings(0.5, 0.25, False, 0xFFFFFFFF))

    def scenario(run):
        before = run.bytes_moved()
        run.system.set_colliders(world)
        run.step(n=12)
        _expect_rule(run, before)
        any_, mn, mx = run.pair.gpu.aabb()
        parts = run.pair.cpu.particles(0)
        assert any_ and np.array_equal(mn, (parts["position"] - parts["scale"][:, None]).min(axis=0))
        assert np.array_equal(mx, (parts["position"] + parts["scale"][:, None]).max(axis=0))
        run.keep("aabb", np.concatenate([mn, mx]))
        o = np.array([[1.0, 9.0, 3.0]], dtype=np.float32)
        run.keep("ray", run.system.cast_rays(o, np.array([[0.0, -1.0, 0.0]], dtype=np.float32), 100.0, 0xFFFFFFFF))
        run.keep("point", run.system.project_points(o, 0xFFFFFFFF))
        run.keep("path", run.system.trace_paths(path_settings, o, np.array([[0.5, 0.0, 0.0]], dtype=np.float32), 0.0, 1.0))
        run.read("after the queries")

    both(monkeypatch, _spawner(), scenario)


def test_polling_calls_leave_the_ages_alone(monkeypatch):
    """what a host asks every frame -- counts, active, poll_finished -- reads no particle: the ring stays under the rule, frame after
    frame, and nothing writes the ages back until somebody reads them (fw_debug_age_launches)"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        flagged = _expect_rule(run, before)
        launches = run.system.age_launches()
        for _ in range(12):
            run.step()
            assert run.pair.gpu.counts() == run.pair.cpu.counts()
            assert run.pair.gpu.active() and not run.pair.gpu.poll_finished()
            assert run.bytes_moved() == flagged
        assert run.system.age_launches() == launches
        run.read("after the polled frames")
        assert run.system.age_launches() == launches + (1 if run.rule else 0)
        return flagged

    on, off = both(monkeypatch, _spawner(), scenario)
    assert on[1] == off[1] - 8


def test_ring_drains_below_one_tile_and_fills_again(monkeypatch):
    """a ring built for the rule (Q0 in planes) whose particles run out: below one four-round tile the launch takes one-round
    workgroups, reads the ages -- written back first -- and moves the unflagged figure; the rule returns with the particles"""
    def scenario(run):
        before = run.bytes_moved()
        for _ in range(8):
            run.pair.queue(5000)
            run.step()
        flagged = _expect_rule(run, before)
        assert run.pair.gpu.count(0) > 10000
        run.step(n=2)  # (nothing queued: the bursts die; no read in between -- the first small launch finds stale ages)
        run.step(n=4)
        assert 0 < run.pair.gpu.count(0) < 1024 and run.bytes_moved() == before
        run.read("drained")
        run.step(n=2)
        run.read("still small")
        for _ in range(5):
            run.pair.queue(5000)
            run.step()
        assert run.bytes_moved() == flagged
        run.read("filled again")

    both(monkeypatch, _spawner(rate=6000.0, on_demand=True), scenario)


@pytest.mark.parametrize("knob", ["FW_NT_MB", "FW_NT_WO_MB"])
def test_non_temporal_forms(monkeypatch, knob):
    """the launch forms of rings beyond the Infinity Cache (fully non-temporal; non-temporal stores of the write-only planes), forced at
    this size: the same rule, the same bits"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=6)
        run.read("early", exact=False)  # (spinning particles: the rotation's trigonometry is not bit-exact against the oracle)
        run.step(n=7)
        path = _expect_rule(run, before)
        run.read("end", exact=False)
        return path

    on, off = both(monkeypatch, _spawner(spin=True), scenario, **{knob: "0"})
    assert on[1] == off[1] - 8


# ---- the packed and the depth-sorted forms as the first reader of stale ages ------------------------------------------------------------
@pytest.mark.parametrize("spin", [False, True], ids=["cannot turn", "spins about y"])
@pytest.mark.parametrize("name", list(first_readers.PACK_READERS))
def test_a_pack_is_the_first_reader_of_stale_ages(monkeypatch, name, spin):
    """twelve frames nobody read (2.5-frame lifetimes: the head has wrapped, particles died unread), then ONE call that packs records:
    scale and colours are evaluated from the age, so the ages are written back first, exactly once, and the particles() read behind
    it writes nothing again.  The records are those of the run without the rule, whose own unsorted pack -- permuted by
    tests/sort_ref.py where the reader sorts -- they must equal byte for byte"""
    reader, is_sorted = first_readers.PACK_READERS[name]

    def scenario(run):
        before = run.bytes_moved()
        run.step(n=12)
        _expect_rule(run, before)
        launches = run.system.age_launches()
        first = reader(run)
        assert run.system.age_launches() == launches + (1 if run.rule else 0), (name, "the first reader", run.rule)
        run.keep(f"records of {name}", first)
        run.read("behind the first reader", exact=not spin)
        assert run.system.age_launches() == launches + (1 if run.rule else 0), (name, "the read behind it wrote the ages again", run.rule)
        unsorted = run.pair.gpu.instances(0)
        run.keep("unsorted", unsorted)
        return first, unsorted, run.pair.gpu.particles(0)

    on, off = both(monkeypatch, _spawner(spin=spin), scenario)
    for first, _, _ in (on, off):
        first_readers.check_records(first, off[1], is_sorted, name)
    first_readers.stale_planes_would_show(off[2], off[1], (0.0, 0.0, 0.0, 1.0) if spin else None, DT)


@pytest.mark.parametrize("spin", [False, True], ids=["cannot turn", "spins about y"])
def test_the_depth_order_every_frame_leaves_the_ages_alone(monkeypatch, spin):
    """the order reads positions, which every launch moves: twelve frames of fw_ctx_depth_order_device write no age back and the ring
    stays under the rule; the particles() read behind them writes them once.  (The run without the rule also takes the unsorted pack
    of every frame: what each order is checked against.)"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        flagged = _expect_rule(run, before)
        launches = run.system.age_launches()
        buf = first_readers.order_buffer(run, 16384)
        orders, unsorted = [], []
        for k in range(12):
            run.step()
            orders.append(first_readers.depth_order(run, buf, 16384))
            run.keep(f"order {k}", orders[-1])
            assert run.bytes_moved() == flagged and run.system.age_launches() == launches
            if not run.rule:
                unsorted.append(run.pair.gpu.instances(0))
        run.read("behind the orders", exact=not spin)
        assert run.system.age_launches() == launches + (1 if run.rule else 0)
        run.read("again", exact=not spin)
        assert run.system.age_launches() == launches + (1 if run.rule else 0)
        return orders, unsorted, run.pair.gpu.instances(0), run.pair.gpu.particles(0)

    on, off = both(monkeypatch, _spawner(spin=spin), scenario)
    assert len(off[1]) == 12
    for orders in (on[0], off[0]):
        for k, (got, u) in enumerate(zip(orders, off[1])):
            assert np.array_equal(got, first_readers.want_order(u)) and not np.array_equal(got, np.arange(len(u))), f"order {k}"
    first_readers.stale_planes_would_show(off[3], off[2], (0.0, 0.0, 0.0, 1.0) if spin else None, DT)


def _two_rings(make, long_frames, per_frame=4.0):
    """one spawner, two types of `make`, each fed by its own Global entry at `per_frame` particles per frame of dt / 64: 320 frames of
    life and `long_frames` -- as many spawn cohorts each"""
    rate = per_frame * 64.0 * 60.0
    a, b = make(life_frames=5.0, rate=rate), make(life_frames=long_frames / 64.0, rate=rate)
    return S.ParticleSpawner(a.particle_settings + b.particle_settings,
                             a.emission_settings + [dataclasses.replace(e, particle_index=1) for e in b.emission_settings])


def test_two_rings_are_read_back_to_back(monkeypatch):
    """two rings of one context after an unread stretch of 1200 frames of dt / 64: the reads write both cohort tables back one right
    after the other through the ONE staging buffer and the one device table (fw_engine.h: Staging), the second waiting for the fence
    behind the first's kernel -- and with 1152 cohorts behind 320 it needs more than the 1024 entries the pair starts with: the table
    grows in between.  Then the same inside a launch: a denormal dt drops the rule for both rings in one frame"""
    small, tiny = np.float32(DT / 64), np.float32(1e-40)

    def scenario(run):
        run.step(small, n=1200)
        launches = run.system.age_launches()
        run.read("both rings")
        assert run.system.age_launches() == launches + (2 if run.rule else 0)
        counts = run.pair.gpu.counts()
        assert 1150 < counts[0] < 1400 and 4300 < counts[1] < 4900, counts
        run.step(small, n=5)
        run.step(tiny)
        assert run.system.age_launches() == launches + (4 if run.rule else 0)
        run.read("after the denormal")
        assert run.system.age_launches() == launches + (4 if run.rule else 0)

    both(monkeypatch, _two_rings(_spawner, 1152), scenario)
