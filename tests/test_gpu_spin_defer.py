"""The deferred spin of FIFO rings nobody reads (fw_device.h: FW_TYPE_IDX_NOSPIN with FW_TYPE_IDX_AXIS; fw_spin.h): a
launch under the age rule and the axis rule leaves rotation and angular velocity of the particles it did not spawn alone, the host logs
its dt, and fw_k_fifo_spin replays the log per particle before anybody looks.  Every case runs the same system twice -- FW_SPIN_DEFER=1
and FW_SPIN_DEFER=0 -- next to the CPU oracle (tests/parity.py, its tolerances), and every field of every read must carry the same bits
in both runs.  The machinery is forced at small sizes: FW_FIFO_SMALL=1 (four-round tiles), FW_SPIN_DEFER_MIN=1, FW_SPIN_DEFER_AFTER=2;
a ring of 8192 slots, 4000 to 12000 live particles, lifetimes of 2.5 and 16 frames -- particles die unread, the head wraps, the log is
trimmed.  Needs an MI355X."""
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
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
AFTER = 2  # FW_SPIN_DEFER_AFTER of these tests: the third qualifying launch in a row is the first deferred one
# what a deferred launch moves less: 4 B of rotation component k, 4 B of rotation w, 4 B of angular velocity, read and written
# (angular_drag != 0: the angular velocity changes every frame)
SPIN_BYTES = 24


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the deferred spin belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _rot_about(axis, angle):
    s, c = float(np.sin(angle / 2)), float(np.cos(angle / 2))
    return (axis[0] * s, axis[1] * s, axis[2] * s, c)


def _spawner(life_frames=2.5, axis=Y, sign=1.0, spread=0.0, on_demand=False, rot_angle=0.7, ang_acc=(0.0, 0.0, 0.0), drag=0.2, rate=None, capacity=8192,
             **kw):
    """~10 000 live particles at either lifetime, spinning about `axis` (sign -1: the direction points the other way; the rotation
    plane's sign follows the angular velocity's), born with a rotation about that axis that is not the identity.  The ring is built
    with 8192 slots and grows, once, to what its lifetime needs (a copy: the spin is replayed and has to be earned again); the cases
    that count replays frame by frame over 16-frame lifetimes build it with 16384, which it keeps."""
    rate = rate if rate is not None else (270000.0 if life_frames < 8 else 40000.0)
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(float(DT) * life_frames), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]), capacity=capacity, angular_drag=drag, angular_acceleration=ang_acc,
                            base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT), **kw)
    direction = tuple(sign * a + 0.0 for a in axis)  # (+ 0.0: no negative zero in the two components the axis rule wants +0)
    es = [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(rate), initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), Y, 0.0),
                             initial_velocity_radial=S.RandF32(0.0, 1.0), initial_rotation=_rot_about(axis, rot_angle),
                             initial_angular_velocity=S.RandVec3(S.RandF32(1.0, 4.0), direction, spread))]
    if on_demand:
        es.append(S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand(), initial_rotation=_rot_about(axis, rot_angle),
                                     initial_angular_velocity=S.RandVec3(S.RandF32(1.0, 4.0), direction, spread)))
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

    def read(self, what="", check=True):
        if check:  # (spinning particles: the rotation's trigonometry is not bit-exact against the oracle -- parity.py's tolerances)
            self.pair.check(exact_all=False, what=f"{what} frame {self.frame} rule={self.rule}")
        for t in range(self.pair.n_types):
            self.keep(f"{what} frame {self.frame} type {t}", self.pair.gpu.particles(t))

    def keep(self, what, arr):
        self.reads.append((what, np.ascontiguousarray(arr).tobytes()))

    def bytes_moved(self, t=0):
        return self.pair.gpu.update_path(t)

    def spins(self):
        return self.system.spin_launches()

    def expect(self, before, deferred=True, t=0):
        """after a streaming frame: a FIFO ring under the age rule (8 B fewer than `before`, the figure at build time), and -- in the
        run with the rule, when the latest launch deferred the spin -- SPIN_BYTES fewer again"""
        path = self.bytes_moved(t)
        assert path[0] == "fifo", path
        assert path[1] == before[1] - 8 - (SPIN_BYTES if (self.rule and deferred) else 0), (path, before, self.rule, deferred)
        return path


def both(monkeypatch, spawner, scenario, fifo_small="1", range_rings="0", product=False, **env):
    """runs `scenario(run)` with the rule and with FW_SPIN_DEFER=0; every read of the two runs must carry the same bits"""
    from bevy_firework_amd.system import ParticleSystem

    figures, reads = {}, {}
    knobs = () if product else (("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", str(AFTER)))
    for rule in (True, False):
        for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_DEFER_MIN", "FW_SPIN_DEFER_AFTER", "FW_SPIN_LOG"):
            monkeypatch.delenv(k, raising=False)  # (the product's choice, whatever the path matrix dealt this test)
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", range_rings), ("FW_SMALL", "0"),
                     ("FW_SPIN_DEFER", "1" if rule else "0")) + knobs + tuple(env.items()):
            monkeypatch.setenv(k, v)
        if fifo_small is None:
            monkeypatch.delenv("FW_FIFO_SMALL", raising=False)
        else:
            monkeypatch.setenv("FW_FIFO_SMALL", fifo_small)
        with ParticleSystem(device=0, seed=SEED) as system:
            run = Run(system, Pair(system, spawner, S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=19), rule)
            figures[rule] = scenario(run)
            reads[rule] = run.reads
            if not rule:
                assert run.spins() == 0
    assert [w for w, _ in reads[True]] == [w for w, _ in reads[False]] and len(reads[True]) > 0
    for (what, a), (_, b) in zip(reads[True], reads[False]):
        assert a == b, f"{what}: the bits differ between the run that defers the spin and the run with FW_SPIN_DEFER=0"
    return figures[True], figures[False]


@pytest.mark.parametrize("every, life_frames, frames", [(0, 2.5, 30), (0, 16.0, 40), (7, 16.0, 35), (7, 2.5, 35), (1, 2.5, 12)],
                         ids=["only at the end", "only at the end, after 2.5 long lifetimes", "every 7th frame", "every 7th frame, short lives", "every frame"])
def test_reads_at_any_rhythm(monkeypatch, every, life_frames, frames):
    def scenario(run):
        before = run.bytes_moved()
        for fr in range(frames):
            run.step()
            # (a launch defers once AFTER launches in a row qualified with nobody asking: frames AFTER + 1 .. of every unread stretch;
            # the very first frame finds an empty ring and does not qualify -- looked at from the first read on)
            if every and fr >= every:
                run.expect(before, deferred=fr % every + 1 > AFTER)
            if every and fr % every == every - 1:
                n = run.spins()
                run.read()
                assert run.spins() == n + (1 if (run.rule and every > AFTER) else 0)
        if not every:
            run.expect(before)
        n = run.spins()
        run.read("end")
        stale = run.rule and (frames if not every else frames % every) > AFTER
        assert run.spins() == n + (1 if stale else 0)
        run.read("again")  # (nothing pending any more)
        assert run.spins() == n + (1 if stale else 0)
        assert 4000 < run.pair.gpu.count(0) < 12500
        if every == 1:
            assert run.spins() == 0  # (a host that reads every frame never defers and never pays a replay)
        return run.bytes_moved()

    # (read frame by frame over long lifetimes: a ring that does not grow on the way, see _spawner)
    on, off = both(monkeypatch, _spawner(life_frames=life_frames, capacity=16384 if (every and life_frames > 8) else 8192), scenario)
    assert on[0] == off[0] == "fifo"


@pytest.mark.parametrize("axis, sign", [(X, 1.0), (Y, -1.0), (Z, 1.0)], ids=["+x", "-y", "z"])
def test_every_axis(monkeypatch, axis, sign):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=14)
        run.expect(before)
        run.read("end")
        assert run.spins() == (1 if run.rule else 0)
        parts = run.pair.gpu.particles(0)
        k = axis.index(1.0)
        assert np.all(np.sign(parts["angular_velocity"][:, k]) == sign) and np.all(parts["rotation"][:, k] != 0)
        others = [a for a in range(3) if a != k]
        assert not parts["angular_velocity"][:, others].view(np.uint32).any() and not parts["rotation"][:, others].view(np.uint32).any()

    both(monkeypatch, _spawner(axis=axis, sign=sign, rot_angle=1.1), scenario)


def test_angular_acceleration_along_the_axis_never_defers(monkeypatch):
    """the axis rule does not cover a type that accelerates its spin (axis_spin_rule, C3): no launch of it defers"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=12)
        assert run.bytes_moved()[1] == before[1] - 8
        run.read("end")
        assert run.spins() == 0

    both(monkeypatch, _spawner(ang_acc=(0.0, 0.75, 0.0)), scenario)


def test_jittering_dt(monkeypatch):
    rng = np.random.default_rng(19)
    dts = [float(x) for x in rng.uniform(0.004, 0.02, size=26)]

    def scenario(run):
        before = run.bytes_moved()
        for k, dt in enumerate(dts):
            run.step(dt)
            if k in (9, 10, 25):
                run.expect(before, deferred=k != 10)
                run.read(f"dt {dt}")

    both(monkeypatch, _spawner(life_frames=16.0), scenario)


def test_zero_denormal_and_negative_dt_inside_a_stretch(monkeypatch):
    """a frame of +0 (its cohort would take the next spawn in), a denormal (the age rule drops it) and a negative one (the ring leaves
    for the compacting path) run undeferred: the spin is replayed first, and the ring earns the rule again afterwards"""
    tiny = np.float32(1e-40)
    assert tiny != 0 and tiny < np.finfo(np.float32).tiny

    def scenario(run):
        before = run.bytes_moved()
        run.step(n=8)
        run.expect(before)
        for odd in (0.0, tiny):
            n = run.spins()
            run.step(odd)
            assert run.spins() == n + (1 if run.rule else 0)
            assert run.bytes_moved()[1] >= before[1] - 8  # (not deferred; a denormal also drops the age rule)
            run.step(n=AFTER)
            run.expect(before, deferred=False)
            run.step(n=3)
            run.expect(before)
        run.step(0.0)
        run.read("right after a frame of zero")
        run.step(n=6)
        run.expect(before)
        n = run.spins()
        run.step(-1.0 / 240.0)
        assert run.bytes_moved()[0] == "general" and run.spins() == n + (1 if run.rule else 0)
        run.read("after the negative step")
        run.step(n=3)
        run.read("on the compacting path")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_a_dt_the_axis_rule_does_not_cover(monkeypatch):
    """angular_drag * dt > 1 voids the axis rule's proof for good: the log is replayed under the rule (every logged dt passed it), the
    frame runs with every plane loaded, and no later launch defers"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        run.expect(before)
        n = run.spins()
        run.step(0.04)  # 30 * 0.04 > 1
        assert run.spins() == n + (1 if run.rule else 0)
        after = run.bytes_moved()
        assert after[1] > before[1]  # (the figure of a ring that spins generally)
        run.read("right after")
        run.step(n=10)
        assert run.bytes_moved() == after and run.spins() == n + (1 if run.rule else 0)
        run.read("ten frames later")
        return after

    on, off = both(monkeypatch, _spawner(life_frames=16.0, drag=30.0), scenario)
    assert on == off


def test_instance_buffer_attached_and_detached(monkeypatch):
    import torch

    def scenario(run):
        before = run.bytes_moved()
        cap = 16384
        buf = torch.full((cap * 16,), float("nan"), dtype=torch.float32, device="cuda")
        run.step(n=9)
        run.expect(before)
        n0 = run.spins()
        run.pair.gpu.attach_instances(buf.data_ptr(), cap)
        assert run.spins() == n0 + (1 if run.rule else 0)
        for k in range(5):
            run.step()
            n = run.pair.gpu.count(0)
            run.keep(f"records {k}", buf[: n * 16].cpu().numpy())
        assert run.bytes_moved()[1] == before[1] + 64 + 4
        run.read("attached")
        run.pair.gpu.attach_instances(0, 0)
        run.read("right after detaching")
        run.step(n=AFTER + 8)
        run.expect(before)
        run.read("detached")

    both(monkeypatch, _spawner(), scenario)


def test_caller_written_particles(monkeypatch):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        run.expect(before)
        parts = run.pair.cpu.particles(0)[::2].copy()
        run.pair.gpu.write_particles(0, parts)
        run.pair.cpu.write_particles(0, parts)
        run.read("right after the write")
        run.step(n=3)
        run.read("after the write")

    both(monkeypatch, _spawner(), scenario)


def test_growth_with_a_stale_spin(monkeypatch):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        run.expect(before)
        n = run.spins()
        run.pair.queue(40000)
        run.step()
        assert run.spins() == n + (1 if run.rule else 0)  # (the larger ring receives the replayed planes)
        run.step(n=2)
        run.read("grown")
        assert run.pair.gpu.count(0) > 40000
        run.step(n=4)
        run.read("after the burst died")

    both(monkeypatch, _spawner(life_frames=3.5, on_demand=True, rate=200000.0), scenario)


def test_ring_becomes_a_range_ring_where_it_stands(monkeypatch):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=10)
        run.expect(before)
        small = S.ParticleSpawner([S.ParticleSettings(lifetime=S.RandF32.constant(0.2), capacity=1024)],
                                  [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(600.0))])
        others = [run.system.spawn(small, uid=200 + k) for k in range(8)]
        assert run.bytes_moved()[0] == "range", (run.bytes_moved(), [o.update_path(0)[0] for o in others])
        run.read("right after the change")
        run.step(n=5)
        run.read("as a range ring")

    both(monkeypatch, _spawner(), scenario, range_rings="1", FW_RANGE_MIN="0")


def test_settings_change_mid_stretch(monkeypatch):
    """fw_spawner_update_settings with another angular_drag, and with destroyed records wanted, inside an unread stretch: the spawner
    starts over (core.rs:343-365) and nothing of the old log reaches the new particles; a ring that reports destroyed particles never
    defers"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        run.expect(before)
        changed = _spawner(drag=0.45)
        run.pair.gpu.update_settings(changed)
        run.pair = _Twin(run.pair, changed)
        assert run.pair.gpu.counts() == [0]
        run.step(n=9)
        run.expect(before)
        run.read("another drag")
        wanted = _spawner(drag=0.45, particles_destroyed=lambda dead: None)
        run.step(n=5)
        run.pair.gpu.update_settings(wanted)
        run.pair = _Twin(run.pair, wanted)
        run.step(n=7)
        assert run.bytes_moved()[1] > before[1] - 8 - SPIN_BYTES
        run.read("destroyed records subscribed")
        return run.spins()

    both(monkeypatch, _spawner(), scenario)


class _Twin:
    """a Pair whose spawner got new settings: the device side keeps its handle, the oracle starts a spawner with the new settings
    (sync_spawner_data drops the particles and restarts the clocks; the RNG serials go on, which only the device's two runs have to
    agree on: the oracle is not consulted after the change)"""

    def __init__(self, pair, spawner):
        self.gpu, self.system, self.spawner, self.n_types = pair.gpu, pair.system, spawner, pair.n_types

    def step_cpu(self, dt):
        pass

    def check(self, exact_all=False, what=""):
        pass


def test_log_at_its_cap(monkeypatch):
    """FW_SPIN_LOG=4 under 16-frame lifetimes: the ring is replayed every fourth deferred frame and goes on deferring"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=8)  # (the first frames find less than a tile of particles and do not count)
        run.read("start")  # (nothing pending from here on, and the rule to be earned again)
        n = run.spins()
        run.step(n=AFTER)
        run.expect(before, deferred=False)
        for k in range(22):
            run.step()
            run.expect(before)  # (the streak is not reset: every launch after the first AFTER defers)
            assert run.spins() == n + (k // 4 if run.rule else 0)
        run.read("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_SPIN_LOG="4")


def test_aabb_and_polling_calls_leave_the_spin_deferred(monkeypatch):
    """what a culling host asks every frame -- the box, counts, active, poll_finished -- needs no rotation: the ages are written back for
    the box, the spin stays deferred, frame after frame"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        flagged = run.expect(before)
        n = run.spins()
        for k in range(12):
            run.step()
            any_, mn, mx = run.pair.gpu.aabb()
            parts = run.pair.cpu.particles(0)
            assert any_ and np.array_equal(mn, (parts["position"] - parts["scale"][:, None]).min(axis=0))
            assert np.array_equal(mx, (parts["position"] + parts["scale"][:, None]).max(axis=0))
            run.keep(f"aabb {k}", np.concatenate([mn, mx]))
            assert run.pair.gpu.counts() == run.pair.cpu.counts()
            assert run.pair.gpu.active() and not run.pair.gpu.poll_finished()
            assert run.bytes_moved() == flagged and run.spins() == n
        run.read("after the polled frames")
        assert run.spins() == n + (1 if run.rule else 0)
        return flagged

    on, off = both(monkeypatch, _spawner(), scenario)
    assert on[1] == off[1] - SPIN_BYTES


def test_ring_drains_below_one_tile_and_fills_again(monkeypatch):
    def scenario(run):
        before = run.bytes_moved()
        for _ in range(8):
            run.pair.queue(5000)
            run.step()
        run.expect(before)
        assert run.pair.gpu.count(0) > 10000
        run.step(n=6)  # (nothing queued: the bursts die unread; the first one-round launch finds a stale spin)
        assert 0 < run.pair.gpu.count(0) < 1024 and run.bytes_moved()[1] == before[1]
        run.read("drained")
        run.step(n=2)
        run.read("still small")
        for _ in range(AFTER + 6):
            run.pair.queue(5000)
            run.step()
        run.expect(before)
        run.read("filled again")

    both(monkeypatch, _spawner(rate=6000.0, on_demand=True), scenario)


def test_two_rings_in_one_launch_one_deferred(monkeypatch):
    """two particle types of one spawner, both FIFO rings of the same launch: one spins about y and defers, the other's angular
    velocities fan out (spread > 0: no axis) and it keeps loading every plane"""
    a, b = _spawner(), _spawner(spread=0.5)
    pa, pb = a.particle_settings[0], b.particle_settings[0]
    ea, eb = a.emission_settings[0], dataclasses.replace(b.emission_settings[0], particle_index=1)
    spawner = S.ParticleSpawner([pa, pb], [ea, eb])

    def scenario(run):
        before = [run.bytes_moved(t) for t in (0, 1)]
        run.step(n=12)
        run.expect(before[0], t=0)
        run.expect(before[1], deferred=False, t=1)
        run.read("end")
        assert run.spins() == (1 if run.rule else 0)

    both(monkeypatch, spawner, scenario)


@pytest.mark.parametrize("knob", ["FW_NT_MB", "FW_NT_WO_MB"])
def test_non_temporal_forms(monkeypatch, knob):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=6)
        run.read("early")
        run.step(n=7)
        path = run.expect(before)
        run.read("end")
        return path

    on, off = both(monkeypatch, _spawner(), scenario, **{knob: "0"})
    assert on[1] == off[1] - SPIN_BYTES


def test_a_ring_that_spins_generally_never_defers(monkeypatch):
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=12)
        path = run.expect(before, deferred=False)
        run.read("end")
        assert run.spins() == 0
        return path

    on, off = both(monkeypatch, _spawner(spread=0.5), scenario)
    assert on == off


def test_a_small_ring_at_product_defaults_keeps_its_figure(monkeypatch):
    """10 000 particles are far below spin_defer_min (and below the size at which a launch streams at all): nothing defers, and the
    ring reports what it reported before this round"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=80)
        assert run.bytes_moved() == before and run.spins() == 0
        run.read("end")
        return before

    on, off = both(monkeypatch, _spawner(), scenario, fifo_small=None, product=True)
    assert on == off and on[0] == "fifo"


# ---- the packed and the depth-sorted forms as the first reader of a deferred spin -------------------------------------------------------
@pytest.mark.parametrize("name", list(first_readers.PACK_READERS))
def test_a_pack_is_the_first_reader_of_a_deferred_spin(monkeypatch, name):
    """fourteen frames nobody read (2.5-frame lifetimes: the head has wrapped, particles died unread), then ONE call that packs
    records: it replays the spin (and writes the ages back: both runs are under the age rule) before it packs, exactly once, and
    the particles() read behind it finds nothing left to replay.  The records are those of the run without the rule, whose own
    unsorted pack -- permuted by tests/sort_ref.py where the reader sorts -- they must equal byte for byte"""
    reader, is_sorted = first_readers.PACK_READERS[name]

    def scenario(run):
        before = run.bytes_moved()
        run.step(n=14)
        run.expect(before)
        spins, ages = run.spins(), run.system.age_launches()
        first = reader(run)
        after = (spins + (1 if run.rule else 0), ages + 1)
        assert (run.spins(), run.system.age_launches()) == after, (name, "the first reader", run.rule)
        run.keep(f"records of {name}", first)
        run.read("behind the first reader")
        assert (run.spins(), run.system.age_launches()) == after, (name, "the read behind it replayed again", run.rule)
        unsorted = run.pair.gpu.instances(0)
        run.keep("unsorted", unsorted)
        return first, unsorted, run.pair.gpu.particles(0)

    on, off = both(monkeypatch, _spawner(), scenario)
    for first, _, _ in (on, off):
        first_readers.check_records(first, off[1], is_sorted, name)
    first_readers.stale_planes_would_show(off[2], off[1], _rot_about(Y, 0.7), DT)


def test_the_depth_order_every_frame_leaves_the_spin_deferred(monkeypatch):
    """a host that draws through an index asks for the order every frame: it reads positions, which no launch defers -- neither the
    spin nor the ages are written back, the ring keeps the deferred figure frame after frame, and the particles() read behind the
    twelve frames causes the one replay.  (The run without the rule also takes the unsorted pack of every frame: what each order is
    checked against.)"""
    def scenario(run):
        before = run.bytes_moved()
        run.step(n=9)
        flagged = run.expect(before)
        spins, ages = run.spins(), run.system.age_launches()
        buf = first_readers.order_buffer(run, 16384)
        orders, unsorted = [], []
        for k in range(12):
            run.step()
            orders.append(first_readers.depth_order(run, buf, 16384))
            run.keep(f"order {k}", orders[-1])
            assert run.bytes_moved() == flagged and run.spins() == spins
            if run.rule:
                assert run.system.age_launches() == ages
            else:
                unsorted.append(run.pair.gpu.instances(0))
        ages = run.system.age_launches()  # (both runs are under the age rule, and the run without this rule has read this frame already)
        after = (spins + 1, ages + 1) if run.rule else (spins, ages)
        run.read("behind the orders")
        assert (run.spins(), run.system.age_launches()) == after
        run.read("again")
        assert (run.spins(), run.system.age_launches()) == after
        return orders, unsorted, run.pair.gpu.instances(0), run.pair.gpu.particles(0)

    on, off = both(monkeypatch, _spawner(), scenario)
    assert len(off[1]) == 12
    for orders in (on[0], off[0]):
        for k, (got, u) in enumerate(zip(orders, off[1])):
            assert np.array_equal(got, first_readers.want_order(u)) and not np.array_equal(got, np.arange(len(u))), f"order {k}"
    first_readers.stale_planes_would_show(off[3], off[2], _rot_about(Y, 0.7), DT)


def test_two_rings_are_read_back_to_back(monkeypatch):
    """two rings of one context whose spin nobody asked for over 2300 frames of dt / 64 (the log reaches its cap on the way: replays inside
    fw_step), then both read back to back: two tables and logs through the ONE staging buffer and the one device table (fw_engine.h:
    Staging), the second waiting for the fence behind the first's kernel -- and with 2176 cohorts behind 320 the pair outgrows the
    16 KiB it starts with while the first's fence is pending.  Then the same inside a launch: a denormal dt ends the deferral of both rings"""
    from test_gpu_fifo_ages import _two_rings

    small, tiny = np.float32(DT / 64), np.float32(1e-40)

    def scenario(run):
        run.step(small, n=2300)
        n = run.spins()
        assert (n > 0) == run.rule
        run.read("both rings")
        assert run.spins() == n + (2 if run.rule else 0)
        counts = run.pair.gpu.counts()
        assert 550 < counts[0] < 720 and 4200 < counts[1] < 4500, counts
        run.step(small, n=5)
        run.step(tiny)
        assert run.spins() == n + (4 if run.rule else 0)
        run.read("after the denormal")
        assert run.spins() == n + (4 if run.rule else 0)

    both(monkeypatch, _two_rings(_spawner, 2176, per_frame=2.0), scenario)
