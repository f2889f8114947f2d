"""The spin of the particles a deferring launch spawns (fw_spin_newborn_deferred, csrc/fw_spin.h; nb_defer in fw_update_fifo_body; DESIGN.md
4.0, round 27): a launch that defers a ring's spin defers it for its newborns too -- the spawning workgroups run no spin step, store the
spawn-time rotation and angular velocity, and the cohort points at the frame's own log entry, which fw_k_fifo_spin applies when somebody
reads.  Every case drives two contexts with the same calls, one under the rule and one with FW_NEWBORN_SPIN=1 (the eager rule of rounds
19 to 26), next to the CPU oracle (tests/parity.py: rotation at the project's 1e-5).  Every plane a reader sees -- all four rotation
components, angular velocity, position, velocity, age and the rest of the record -- must carry the same bits in both; fw_debug_fuse2 and
fw_debug_fuse_frames must say the same thing call by call (the rule changes no launch, only what its spawning workgroups compute); and
fw_debug_newborn_spin must be non-zero exactly where the rule applies.

The ring: 4096 slots, 197 new particles per frame (no multiple of 64: the boundaries between the birth frames of a fused launch fall
inside waves) over 9.5-frame lifetimes -- about 1870 live, eight frames' spawns fit (3446) and their dead are old particles, so groups
reach depth 8; 50 to 60 frames spawn three times the ring's slots: the head goes round, groups of spawning workgroups split at the
buffer's end, and cohorts born under the rule die under it.  One-axis angular velocity (1 to 4 rad/s: |w| dt is far below the bound of
fw_quat_step's polynomial arm, whose choice is per wave) with an angular drag of 0.2.  An angular ACCELERATION along the axis is a case
of its own: the axis rule refuses such a type (axis_spin_rule, C3), so none of its launches defers and the rule never applies.
The thresholds are lowered as in tests/test_gpu_fifo_fuse_wide.py.  Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from parity import Pair
from test_gpu_fifo import _nested_rings
from test_gpu_fifo_fuse2 import Run2
from test_gpu_fifo_spinless import _still, _two_types
from test_gpu_spin_defer import AFTER, DT, SEED, _spawner

pytestmark = pytest.mark.gpu
PER_FRAME, LIFE, CAPACITY = 197, 9.5, 4096
CLEARED = ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB", "FW_SPINLESS", "FW_SPIN_DEFER",
           "FW_SPIN_DEFER_MIN", "FW_SPIN_DEFER_AFTER", "FW_FUSE2", "FW_FUSE2_MIN", "FW_FIFO_SMALL", "FW_FUSE_DEPTH", "FW_FUSE_DEEP_MIN", "FW_FUSE_WIDE_MIN",
           "FW_WHOLE_TILES", "FW_NEWBORN_SPIN")


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the deferred spin belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _ring(**kw):
    kw.setdefault("life_frames", LIFE)
    kw.setdefault("rate", PER_FRAME * 60.0)
    kw.setdefault("capacity", CAPACITY)
    return _spawner(**kw)


def _dt(k):
    return np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k)))


def twice(monkeypatch, spawner, scenario, fuse2="1", **env):
    """`scenario(run)` under the rule and under FW_NEWBORN_SPIN=1.  Returns, of the run under the rule: fw_debug_newborn_spin, the frames
    fused launches ran call by call, and what the scenario returned"""
    from bevy_firework_amd.system import ParticleSystem

    reads, logs, frames, counted, out = {}, {}, {}, {}, {}
    for newborn in (True, False):
        for k in CLEARED:
            monkeypatch.delenv(k, raising=False)
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0"), ("FW_FIFO_SMALL", "1"),
                     ("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", str(AFTER)), ("FW_FUSE2_MIN", "1"), ("FW_FUSE_DEEP_MIN", "1"), ("FW_FUSE_WIDE_MIN", "1"),
                     ("FW_FUSE2", fuse2), ("FW_NEWBORN_SPIN", "0" if newborn else "1")) + tuple(env.items()):
            monkeypatch.setenv(k, v)
        with ParticleSystem(device=0, seed=SEED) as system:
            run = Run2(system, Pair(system, spawner, S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=27), fuse2 == "1")
            run.newborn, run.frames = newborn, []
            did = run.did

            def tracked(fn, *a, _did=did, _run=run, **kw):
                n0 = _run.system.fuse_frames()
                got = _did(fn, *a, **kw)
                _run.frames.append(_run.system.fuse_frames() - n0)
                return got

            run.did = tracked
            out[newborn] = scenario(run)
            reads[newborn], logs[newborn], frames[newborn], counted[newborn] = run.reads, run.log, run.frames, system.newborn_spin_launches()
    assert [w for w, _ in reads[True]] == [w for w, _ in reads[False]] and len(reads[True]) > 0
    for (what, a), (_, b) in zip(reads[True], reads[False]):
        assert a == b, f"{what}: the bits differ between the run that defers its newborns' spin and the run with FW_NEWBORN_SPIN=1"
    assert logs[True] == logs[False] and frames[True] == frames[False], "the rule changed which frames were fused"
    assert counted[False] == 0, counted
    return counted[True], frames[True], out[True]


@pytest.mark.parametrize("depth", [2, 4, 8])
def test_groups_that_close_at_their_depth(monkeypatch, depth):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.step(n=48)
        live = run.pair.gpu.count(0)
        run.did(run.read, "end")
        run.totals("end")
        run.step(n=5)
        run.read("behind it")
        return live

    counted, frames, live = twice(monkeypatch, _ring(), scenario, FW_FUSE_DEPTH=str(depth))
    assert max(frames) == depth and frames.count(depth) >= 48 // depth - 1, frames
    assert counted >= 48 // depth, counted
    assert 61 * PER_FRAME > 2 * CAPACITY and 1500 < live < 2300, live  # (the head went round; cohorts born under the rule died under it)


@pytest.mark.parametrize("pending", [1, 2, 3, 4, 5, 6, 7])
def test_a_reader_arrives_with_frames_withheld(monkeypatch, pending):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        run.step(n=24 + pending)
        run.did(run.read, "the reader")
        flushed = run.frames[-1]
        run.totals("the reader")
        run.step(n=8)
        run.read("behind it")
        return flushed

    counted, frames, flushed = twice(monkeypatch, _ring(), scenario, FW_FUSE_DEPTH="8")
    assert flushed == (pending if pending >= 2 else 0), (pending, frames[-12:])  # (one withheld frame goes out alone, as it was built)
    assert counted >= 4, counted


def test_unfused_deferring_launches(monkeypatch):
    def scenario(run):
        run.step(n=50)
        run.read("end")
        run.totals("end")
        run.step(n=AFTER + 4)
        run.read("behind it")

    counted, frames, _ = twice(monkeypatch, _ring(), scenario, fuse2="0")
    assert not any(frames) and counted >= 40, (counted, frames)  # (every launch from the one that earns the rule on: 50 less AFTER and the first few)


def test_a_dt_that_changes_every_frame(monkeypatch):
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        for k in range(45):
            run.step(_dt(k))
        run.did(run.read, "end")
        run.totals("end")

    counted, frames, _ = twice(monkeypatch, _ring(), scenario, FW_FUSE_DEPTH="8")
    assert max(frames) == 8 and counted >= 5, (counted, frames)


@pytest.mark.parametrize("fuse2", ["1", "0"], ids=["fused", "unfused"])
def test_a_log_cap_below_the_lifetime(monkeypatch, fuse2):
    """FW_SPIN_LOG=5 under 9.5-frame lifetimes: the log fills every five frames, is replayed mid-stretch -- the newborns' own entries
    with it -- and the ring goes on deferring"""
    def scenario(run):
        run.step(n=8)
        run.quiesce()
        for k in range(42):
            run.step(_dt(k))
        replays = run.spins()
        run.read("end")
        run.totals("end")
        return replays

    counted, _, replays = twice(monkeypatch, _ring(), scenario, fuse2=fuse2, FW_FUSE_DEPTH="8", FW_SPIN_LOG="5")
    assert replays >= 6 and counted >= 30 // (8 if fuse2 == "1" else 1), (replays, counted)


def test_a_stretch_that_ends_and_a_second_one(monkeypatch):
    """a read ends the first stretch (every pending entry replayed, the rule earned again), a frame of dt +0 the second one (the launch
    does not defer: replayed in front of it), and a third one runs to the end"""
    def scenario(run):
        run.step(n=20)
        run.read("first")
        run.step(n=17)
        run.step(np.float32(0.0))
        run.step(n=19)
        run.read("end")
        run.totals("end")
        return run.spins()

    counted, _, replays = twice(monkeypatch, _ring(), scenario, FW_FUSE_DEPTH="4")
    assert replays >= 3 and counted >= 8, (replays, counted)


def test_a_ring_that_cannot_turn_beside_one_that_defers(monkeypatch):
    """two rings in one launch: the one that cannot turn has nothing to defer, the other one's newborns are under the rule"""
    def scenario(run):
        run.step(n=45)
        run.read("end")
        run.totals("end")

    counted, _, _ = twice(monkeypatch, _two_types(_ring(), _still(life_frames=LIFE, rate=PER_FRAME * 60.0)), scenario, FW_FUSE_DEPTH="4")
    assert counted >= 5, counted


def test_a_ring_that_keeps_its_spin_beside_one_that_defers(monkeypatch):
    """... and beside a ring that accelerates its spin, which never defers: the launch takes the form that finds out per workgroup"""
    def scenario(run):
        run.step(n=45)
        run.read("end")
        run.totals("end")

    counted, frames, _ = twice(monkeypatch, _two_types(_ring(), _ring(ang_acc=(0.0, 0.75, 0.0))), scenario)
    assert counted >= 30 and not any(frames), (counted, frames)


@pytest.mark.parametrize("spawner", ["cannot turn", "accelerates its spin", "materialised"])
def test_rings_the_rule_does_not_apply_to(monkeypatch, spawner):
    """a type that cannot turn (nothing to defer), a type with an angular acceleration along its axis (the axis rule refuses it: no launch
    defers) and sparks that emit smoke, both in FIFO rings (the sparks are materialised before the update, the smoke is appended on the
    device): the counter stays at zero and the switch changes nothing"""
    sp = {"cannot turn": lambda: _still(life_frames=LIFE, rate=PER_FRAME * 60.0), "accelerates its spin": lambda: _ring(ang_acc=(0.0, 0.75, 0.0)),
          "materialised": lambda: _nested_rings(spark_rate=31400.0, per_spark=12.0)}[spawner]()
    if spawner == "materialised":
        sp.particle_settings[0].capacity = 16384  # (what its sparks need: the ring does not grow on the way)

    def scenario(run):
        for k in range(40):
            run.step(_dt(k))
            if k % 16 == 15:
                run.read(f"frame {k}")
        run.read("end")
        run.totals("end")
        assert all(run.pair.gpu.update_path(t)[0] == "fifo" for t in range(run.pair.n_types))

    counted, _, _ = twice(monkeypatch, sp, scenario)
    assert counted == 0, counted
