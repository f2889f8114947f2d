"""Two frames of an unread FIFO ring in one launch (fw_ctx::withheld, FwFifoArgs::fused, the FUSE2 instantiations of fw_k_update_fifo;
csrc/fw_fuse2.h): a frame whose only GPU work is one spin-less launch of rings that all deferred their spin is
withheld -- its bookkeeping done, its launch kept --, and the next frame's launch runs both: one load and one store per plane for two
updates.  Whoever touches the stream or the particles first puts the kept launch on the stream as it was built.
Every case runs the same system twice, FW_FUSE2=0 and FW_FUSE2=1, next to the CPU oracle (tests/parity.py); every field of every read,
the counts, updated_total and the particle total of kernel_timing_read must carry the same bits and values in both runs, and
fw_debug_fuse2 must say, call by call, which frames were fused and which withheld frames went out alone (a frame was withheld exactly
when the next call fuses or flushes it).  The machinery is forced at small sizes as in test_gpu_spin_defer.py, whose spawner and Run
this file borrows: FW_FIFO_SMALL=1, FW_SPIN_DEFER_MIN=1, FW_SPIN_DEFER_AFTER=2, FW_FUSE2_MIN=1; rings of 8192 to 32768 slots (4500 new
particles per frame over 2.5-frame lifetimes need 18000 slots for a pair: at 16384 the rule declines, which is a case of its own).
Needs an MI355X."""
import numpy as np
import pytest

import first_readers
import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from parity import Pair
from test_gpu_fifo_spinless import _two_types
from test_gpu_spin_defer import AFTER, DT, SEED, SPIN_BYTES, Run, _spawner, _Twin

pytestmark = pytest.mark.gpu
W, F, X = (0, 0), (1, 0), (0, 1)  # what one call did to (fused launches, withheld frames flushed alone): nothing, fused a pair, flushed


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


class Run2(Run):
    """a Run that asks fw_debug_fuse2 around every step and every other call it makes"""

    def __init__(self, system, pair, rule):
        super().__init__(system, pair, rule)
        self.log = []

    def did(self, fn, *a, **kw):
        c0 = self.system.fuse2_launches()
        out = fn(*a, **kw)
        c1 = self.system.fuse2_launches()
        self.log.append((c1[0] - c0[0], c1[1] - c0[1]))
        if not self.rule:
            assert self.log[-1] == W, (self.frame, self.log[-8:])
        return out

    def step(self, dt=DT, n=1):
        for _ in range(n):
            self.did(Run.step, self, dt)

    def quiesce(self):
        """nothing pending afterwards, and no ring has lost its streak: synchronize is no request for the planes"""
        self.system.synchronize()
        self.log.append(None)

    def pairs(self, n, dt=DT):
        """n frames nobody reads, starting with nothing pending: withheld, fused, withheld, fused ..."""
        self.step(dt, n)
        if self.rule:
            assert self.log[-n:] == [W, F] * (n // 2) + [W] * (n % 2), (self.frame, self.log[-n - 2:])

    def never(self, n, dt=DT):
        """n frames none of which may be withheld: each goes out with its own launch (a call that finds nothing pending flushes nothing)"""
        self.step(dt, n)
        self.did(self.system.synchronize)
        assert self.log[-n - 1:] == [W] * (n + 1), (self.frame, self.log[-n - 3:])

    def totals(self, what=""):
        self.keep(f"{what} counts", np.array(self.pair.gpu.counts(), dtype=np.int64))
        self.keep(f"{what} updated_total", np.array([self.system.updated_total()], dtype=np.int64))


def both(monkeypatch, spawner, scenario, fifo_small="1", oracle_twin=True, **env):
    """runs `scenario(run)` with FW_FUSE2=1 and with FW_FUSE2=0; every read of the two runs must carry the same bits"""
    from bevy_firework_amd.system import ParticleSystem

    reads, logs, out = {}, {}, {}
    for rule in (True, False):
        for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB", "FW_SPINLESS", "FW_SPIN_DEFER",
                  "FW_SPIN_DEFER_MIN", "FW_SPIN_DEFER_AFTER", "FW_FUSE2_MIN", "FW_FIFO_SMALL"):
            monkeypatch.delenv(k, raising=False)  # (the product's choice, whatever the path matrix dealt this test)
        knobs = (("FW_FIFO_SMALL", fifo_small), ("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", str(AFTER)), ("FW_FUSE2_MIN", "1")) if fifo_small else ()
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0"),
                     ("FW_FUSE2", "1" if rule else "0")) + knobs + tuple(env.items()):
            monkeypatch.setenv(k, v)
        with ParticleSystem(device=0, seed=SEED) as system:
            pair = Pair(system, spawner, S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=22)
            run = Run2(system, pair if oracle_twin else _Twin(pair, spawner), rule)
            out[rule] = scenario(run)
            reads[rule], logs[rule] = run.reads, run.log
    assert [w for w, _ in reads[True]] == [w for w, _ in reads[False]] and len(reads[True]) > 0
    for (what, a), (_, b) in zip(reads[True], reads[False]):
        assert a == b, f"{what}: the bits differ between the run that fuses pairs of frames and the run with FW_FUSE2=0"
    assert not any(e not in (None, W) for e in logs[False])
    return logs[True], out[True]


def _fused(log):
    return sum(e[0] for e in log if e)


def _flushed(log):
    return sum(e[1] for e in log if e)


@pytest.mark.parametrize("frames", [20, 21], ids=["even", "odd"])
def test_an_unread_stretch_read_at_its_end(monkeypatch, frames):
    def scenario(run):
        run.step(n=8)  # (the ring qualifies from its fourth launch on)
        run.quiesce()
        run.pairs(frames)
        run.did(run.read, "end")
        assert not run.rule or run.log[-1] == (X if frames % 2 else W)  # (an odd stretch leaves a frame withheld: the read flushes it)
        run.totals("end")
        run.step(n=AFTER)  # (the read asked for the planes: the rule is earned again, and until then nothing is withheld)
        run.did(run.system.synchronize)
        assert run.log[-AFTER - 1:] == [W] * (AFTER + 1)
        run.pairs(4)
        run.read("after four more")

    log, _ = both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)
    assert _fused(log) == frames // 2 + 2 + sum(1 for e in log[:8] if e == F)


def test_a_host_that_reads_every_seventh_frame(monkeypatch):
    def scenario(run):
        for fr in range(35):
            run.step()
            if fr % 7 == 6:
                run.did(run.read, f"frame {fr}")
                run.totals(f"frame {fr}")

    log, _ = both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)
    assert _fused(log) >= 4 and _flushed(log) >= 1  # (7 frames: AFTER + 1 to earn the rule, then two pairs -- or one and a flush)


@pytest.mark.parametrize("rate, capacity", [(270000.0, 32768), (240000.0, 16384), (150000.0, 16384)],
                         ids=["4500 per frame", "4000 per frame: every old particle dies inside the pair", "2500 per frame"])
def test_the_head_goes_round_under_pairs(monkeypatch, rate, capacity):
    """2.5-frame lifetimes: two cohorts live before a frame, one dies in it.  The ring's head goes round several times, the new particles
    of two frames straddle the ring's end in some pairs (two groups of spawning workgroups), and the boundary between the first frame's
    new particles and the second's falls inside a workgroup (4500, 4000 and 2500 are no multiples of 256).  At 4000 per frame in 16384
    slots the pair's dead are ALL the old particles: the fused launch has spawning workgroups and no ring tile at all"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(41)
        run.did(run.read, "end")
        assert not run.rule or run.log[-1] == X
        run.totals("end")
        assert 41 * (rate / 60.0) > 3 * capacity

    both(monkeypatch, _spawner(rate=rate, capacity=capacity), scenario)


def test_lives_of_a_frame_and_a_half_are_declined(monkeypatch):
    """every particle born in a frame dies in the next one: a pair in which a newborn dies is never fused -- each withheld frame goes out
    alone, in front of the next frame's launch, which is then withheld itself"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.step(n=12)
        if run.rule:
            assert run.log[-12:] == [W] + [X] * 11, run.log[-14:]
        run.did(run.read, "end")
        run.totals("end")

    log, _ = both(monkeypatch, _spawner(life_frames=1.5, rate=270000.0, capacity=16384), scenario)
    assert _fused(log) == 0 and _flushed(log) >= 12


def test_a_ring_without_room_for_two_frames_of_newborns_is_declined(monkeypatch):
    """9000 live particles and 4500 new ones per frame in 16384 slots: one frame fits, a pair would put the second frame's new
    particles on slots the first frame's dead have not left in the fused view.  Declined, not grown"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.step(n=10)
        if run.rule:
            assert run.log[-10:] == [W] + [X] * 9, run.log[-12:]
        assert run.pair.gpu.update_path(0)[0] == "fifo"
        run.did(run.read, "end")
        run.totals("end")

    log, _ = both(monkeypatch, _spawner(rate=270000.0, capacity=16384), scenario)
    assert _fused(log) == 0


def test_two_different_dt_in_every_pair(monkeypatch):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        for k in range(24):
            run.step(np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k))))
        if run.rule:
            assert run.log[-24:] == [W, F] * 12
        run.read("end")
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


@pytest.mark.parametrize("odd", ["zero", "denormal", "negative"])
def test_a_frame_that_does_not_qualify_flushes_the_withheld_one(monkeypatch, odd):
    dt = {"zero": np.float32(0.0), "denormal": np.float32(1e-40), "negative": np.float32(-1.0 / 240.0)}[odd]

    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(3)  # (... and one frame is withheld)
        run.step(dt)
        assert not run.rule or run.log[-1] == X
        run.read("right after")
        run.step(n=AFTER + 4)
        run.read("later")
        run.totals("later")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_frames_that_spawn_nothing_and_frames_that_kill_nothing(monkeypatch):
    """a trickle of one particle every other frame next to three bursts: most frames spawn nothing, and for the first sixteen nobody dies"""
    def scenario(run):
        for _ in range(3):
            run.pair.queue(3000)
            run.step()
        run.step(n=5)
        run.quiesce()
        run.pairs(4)   # (nobody dies yet; the trickle alone spawns, in every other frame)
        run.pair.queue(3000)  # (... so that the ring still streams when the three bursts have died)
        run.pairs(12)  # (the bursts die here, in frames 16 to 18)
        run.read("end")
        run.totals("end")
        assert 3000 <= run.pair.gpu.count(0) < 3200

    both(monkeypatch, _spawner(life_frames=16.0, rate=30.0, on_demand=True, capacity=16384), scenario)


def _ray(run):
    return run.system.cast_rays(np.array([[1.0, 9.0, 3.0]], np.float32), np.array([[0.0, -1.0, 0.0]], np.float32), np.array([100.0], np.float32),
                                np.array([0xFFFFFFFF], np.uint32))


def _attach(run):
    import torch

    run.buf = torch.zeros((16384 * 16,), dtype=torch.float32, device="cuda")
    run.pair.gpu.attach_instances(run.buf.data_ptr(), 16384)


def _write(run):
    parts = run.pair.cpu.particles(0)[::2].copy()
    run.pair.gpu.write_particles(0, parts)
    run.pair.cpu.write_particles(0, parts)


def _settings(run):
    changed = _spawner(life_frames=16.0, capacity=16384, drag=0.45)
    run.pair.gpu.update_settings(changed)
    run.pair = _Twin(run.pair, changed)


# name -> the call (on a Run)
FIRST_CALLERS = {
    "read_particles": lambda run: run.keep("first", run.pair.gpu.particles(0)),
    "pack_instances": lambda run: run.keep("first", first_readers.unsorted_host(run)),
    "pack_instances_device": lambda run: run.keep("first", first_readers.unsorted_device(run)),
    "pack_instances_sorted": lambda run: run.keep("first", first_readers.sorted_host(run)),
    "pack_instances_sorted_device": lambda run: run.keep("first", first_readers.sorted_device(run)),
    "aabb": lambda run: run.keep("first", np.concatenate(run.pair.gpu.aabb()[1:])),
    "counts": lambda run: run.keep("first", np.array(run.pair.gpu.counts())),
    "poll_finished": lambda run: run.keep("first", np.array([run.pair.gpu.poll_finished(), run.pair.gpu.active()])),
    "updated_total": lambda run: run.keep("first", np.array([run.system.updated_total()])),
    "synchronize": lambda run: run.system.synchronize(),
    "write_particles": _write,
    "attach_instances": _attach,
    "set_colliders": lambda run: run.system.set_colliders([]),
    "cast_rays": lambda run: run.keep("first", _ray(run)),
    "update_settings": _settings,
}


@pytest.mark.parametrize("name", list(FIRST_CALLERS))
def test_every_entry_point_as_the_first_caller_with_a_frame_withheld(monkeypatch, name):
    """three unread frames from a state with nothing pending: the third is withheld when `name` is called.  The call puts it on the stream
    first (the counting and polling calls too: they read the device's count rows) and sees what the run with FW_FUSE2=0 sees"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(3)
        run.did(FIRST_CALLERS[name], run)
        assert not run.rule or run.log[-1] == X, (name, run.log[-4:])
        if name == "attach_instances":
            run.step(n=2)
            run.keep("records", run.buf[: run.pair.gpu.count(0) * 16].cpu().numpy())
            run.pair.gpu.attach_instances(0, 0)
        run.step(n=5)
        run.read("behind it", check=name != "update_settings")
        run.totals("behind it")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_a_context_closed_with_a_frame_withheld(monkeypatch):
    def scenario(run):
        run.step(n=8)
        run.read("early")
        run.quiesce()
        run.step(n=AFTER + 1)
        run.quiesce()
        run.pairs(3)  # (the context manager closes the context with the third frame withheld: dropped with the particles)

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_a_burst_grows_the_ring_with_a_frame_withheld(monkeypatch):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(3)
        run.pair.queue(40000)
        run.step()
        assert not run.rule or run.log[-1] == X  # (the growth copies the ring: the withheld frame first)
        run.step(n=2)
        run.read("grown")
        assert run.pair.gpu.count(0) > 40000
        run.step(n=6)
        run.read("after the burst died")
        run.totals("end")

    # (3333 new particles per frame over 3.5-frame lifetimes: 10000 live before a frame, a pair needs 16666 slots -- 32768, which the burst outgrows)
    both(monkeypatch, _spawner(life_frames=3.5, on_demand=True, rate=200000.0, capacity=32768), scenario)


def test_two_rings_in_one_launch(monkeypatch):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(13)
        run.did(run.read, "end")
        assert not run.rule or run.log[-1] == X
        run.totals("end")

    both(monkeypatch, _two_types(_spawner(life_frames=16.0, capacity=16384), _spawner(life_frames=5.0, rate=100000.0, capacity=16384)), scenario)


def test_a_ring_that_does_not_qualify_next_to_one_that_does(monkeypatch):
    """type 1's angular velocities fan out (no axis: its spin is never deferred): the launch of the two is never withheld"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.never(9)
        run.read("end")

    log, _ = both(monkeypatch, _two_types(_spawner(life_frames=16.0, capacity=16384), _spawner(life_frames=16.0, spread=0.5, capacity=16384)), scenario)
    assert _fused(log) == 0 and _flushed(log) == 0


def test_a_compacting_segment_in_the_context(monkeypatch):
    """a second spawner whose lifetimes are a range runs on the compacting kernels (FW_RANGE=0): the frame has a general launch, and no
    frame of the context is withheld"""
    def scenario(run):
        other = S.ParticleSpawner([S.ParticleSettings(lifetime=S.RandF32(0.1, 0.3), capacity=4096)], [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(6000.0))])
        h = run.system.spawn(other, uid=300)
        run.step(n=8)
        assert h.update_path(0)[0] == "general" and run.pair.gpu.update_path(0)[0] == "fifo"
        run.quiesce()
        run.never(9)
        run.read("end")
        run.keep("the other spawner", h.particles(0))

    log, _ = both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)
    assert _fused(log) == 0 and _flushed(log) == 0


def test_a_context_that_keeps_a_ring_of_live_counts(monkeypatch):
    """what the sharded system attaches when its ranks exchange live counts (fw_ctx_live_count_ring): a count per frame is wanted, and
    no frame is withheld; detached, the pairs come back"""
    import torch

    def scenario(run):
        ring = torch.zeros((8,), dtype=torch.int64, device="cuda")
        run.step(n=8)
        run.system.live_count_ring(ring.data_ptr(), 8)
        run.never(9)
        run.keep("live counts", ring.cpu().numpy())
        run.system.live_count_ring(0, 0)
        run.pairs(6)
        run.read("end")

    log, _ = both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)
    assert _fused(log) >= 3


def test_the_sharded_system_with_its_exchange_on(monkeypatch):
    """bevy_firework_amd.sharding with exchange=True (one rank: the ring of live counts and the buckets without a collective): every
    frame's total is wanted, so no frame is withheld -- and the history of totals is the run's with FW_FUSE2=0"""
    from bevy_firework_amd import sharding
    from bevy_firework_amd.system import ParticleSystem

    spawner, tf = _spawner(life_frames=16.0, capacity=16384), S.Transform((1.0, 2.0, 3.0))
    seen = {}
    for rule in ("1", "0"):
        for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB", "FW_SPINLESS", "FW_SPIN_DEFER"):
            monkeypatch.delenv(k, raising=False)  # (the product's choice, whatever the path matrix dealt this test)
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0"), ("FW_FIFO_SMALL", "1"),
                     ("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", str(AFTER)), ("FW_FUSE2_MIN", "1"), ("FW_FUSE2", rule)):
            monkeypatch.setenv(k, v)
        sh = sharding.ShardedParticleSystem(lambda: ParticleSystem(device=0, seed=SEED), [(spawner, tf)], exchange=True, reduce_every=4)
        with sh.system:
            sh.update(DT)
            for _ in range(23):
                sh.step(DT)
            assert sh.system.fuse2_launches() == (0, 0)
            assert sh.handles[0].update_path(0)[0] == "fifo" and sh.system.spinless_launches() > 12  # (the launches would have qualified)
            sh.flush()
            seen[rule] = (list(sh.global_live_history), sh.handles[0].particles(0).tobytes())
    assert seen["1"] == seen["0"] and len(seen["1"][0]) == 24 and seen["1"][0][-1] > 9000


def test_the_bytes_a_particle_update_moves_after_a_fused_launch(monkeypatch):
    """fw_debug_update_path: position and velocity in and out, 48 B, for a launch that leaves age and spin alone -- and 24 B per
    particle-update when the latest launch ran two frames; 48 again once a withheld frame has gone out alone"""
    def scenario(run):
        built = run.bytes_moved()
        run.step(n=8)
        run.quiesce()
        run.step()
        run.did(run.system.synchronize)  # (a frame that went out alone: the latest launch ran one frame)
        one = run.bytes_moved()[1]
        assert one == built[1] - 8 - SPIN_BYTES == 48, (built, one)  # (the age rule and the deferred spin: test_gpu_spin_defer.py)
        run.pairs(4)
        moved = run.bytes_moved()
        assert moved[0] == "fifo" and moved[1] == (24 if run.rule else 48), moved
        run.step()
        run.did(run.system.synchronize)  # (the fifth frame, withheld, goes out alone)
        assert run.bytes_moved()[1] == 48
        run.read("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_kernel_timing_counts_every_particle_update(monkeypatch):
    """with events on every dispatch nothing is withheld (a launch per frame is what is timed); switching them on flushes a withheld frame"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.pairs(3)
        run.did(run.system.kernel_timing, True)
        assert not run.rule or run.log[-1] == X
        run.never(6)
        _, launches, particles = run.system.kernel_timing_read()
        run.keep("timed", np.array([launches, particles], dtype=np.int64))
        run.system.kernel_timing(False)
        run.pairs(4)
        run.read("end")
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_the_product_thresholds_at_524289_particles(monkeypatch):
    """no knob but FW_FUSE2: a ring of 2^19 + 1 live particles (16-frame lifetimes, 34952.6 new ones per frame) earns the
    deferred spin after 32 unread launches and runs in pairs from then on; read after an odd and after an even number of them"""
    per_frame = 524289.0 / 15.0  # (a particle dies in its sixteenth update: fifteen cohorts are alive after a frame)

    def scenario(run):
        run.step(n=16 + 32 + 2)
        run.quiesce()
        assert 524289 - 16 <= run.pair.gpu.count(0) <= 524289 + 16  # (34952 or 34953 a frame)
        run.pairs(9)
        run.did(run.read, "odd", check=False)
        assert not run.rule or run.log[-1] == X
        run.totals("odd")
        run.step(n=32 + 1)  # (the read asked for the planes: 32 launches to earn the rule again)
        run.quiesce()
        run.pairs(4)
        run.did(run.read, "even", check=False)
        assert not run.rule or run.log[-1] == W
        run.totals("even")

    log, _ = both(monkeypatch, _spawner(life_frames=16.0, rate=per_frame * 60.0, capacity=1 << 20), scenario, fifo_small=None, oracle_twin=False)
    assert _fused(log) >= 6
