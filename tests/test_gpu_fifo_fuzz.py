"""Random rings under random hosts (tests/fifo_fuzz.py: the generator): spawners every type of which is a FIFO ring whose
ages are derived, whose spin and whose newborns' spin are deferred and whose unread frames run fused -- up to sixteen in a launch, whole
tiles first, ops merged in the far tier -- with everything the rules leave free drawn at random: one or two rings, one to three entries
per ring (rates, windows that emit nothing in some frames, bursts on demand), shapes, cones, accelerations, drags, curves, every spin
axis and sign; and hosts that step irregularly, move the emitter, change parent velocity and modifier, queue bursts, and read -- with
every entry point that reads -- after stretches of 1 to 40 frames, so that a reader meets every pending depth.
Every case runs the same spawner, script and seed in three contexts, each beside its own oracle twin: (A) the drawn knobs with FW_FUSE2=1,
(B) the same with FW_FUSE2=0, (C) with FW_FUSE2=0 FW_SPIN_DEFER=0 FW_AGELESS=0.  Every read of every reader carries the same bytes in the
three, every full read matches the oracle within tests/parity.py's tolerances, B and C fuse nothing, C replays nothing, and in A every
frame ran exactly once, no launch is deeper than the knobs allow and nothing is pending behind a reader.  Which frames fuse is recorded,
not predicted: the hand-written files (test_gpu_fifo_fuse2.py .. test_gpu_fifo_fuse_far.py, test_gpu_fifo_whole_*.py) own the exact logs.
FW_FUZZ_EXTRA=n runs n more cases, FW_FUZZ_OFFSET=k other ones (the case number is the seed), as in tests/test_gpu_fuzz.py.
Needs an MI355X."""
import hashlib
import os
import time

import numpy as np
import pytest

import fifo_fuzz as ff
import first_readers
import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from parity import Pair
from test_gpu_fifo_fuse2 import W, Run2, _ray
from test_gpu_fifo_fuse_deep import _accounted, _tail, _track
from test_gpu_spin_defer import SEED, Run

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("FW_FUZZ_EXTRA", "0"))  # more random cases than the committed suite runs (spare GPU time)
OFF = int(os.environ.get("FW_FUZZ_OFFSET", "0"))  # ... and other ones: the case numbers (= the seeds) start here
CONTEXTS = {"A": {"FW_FUSE2": "1"}, "B": {"FW_FUSE2": "0"}, "C": {"FW_FUSE2": "0", "FW_SPIN_DEFER": "0", "FW_AGELESS": "0"}}
CLEARED = ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB", "FW_SPINLESS", "FW_SPIN_DEFER",
           "FW_SPIN_DEFER_MIN", "FW_SPIN_DEFER_AFTER", "FW_FUSE2_MIN", "FW_FIFO_SMALL", "FW_WHOLE_TILES", "FW_NEWBORN_SPIN", "FW_FUSE_DEPTH",
           "FW_FUSE_FAR_DEPTH", "FW_FUSE_DEEP_MIN", "FW_FUSE_WIDE_MIN", "FW_FUSE_FAR_MIN")
STATS = {}  # case -> what its A run did (test_the_random_cases_reached_the_machinery)


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _call(run, kind, fn, *a):
    """every call a run makes goes through Run2.did (under _track): what it did to the withheld group is logged beside its kind"""
    run.kinds.append(kind)
    return run.did(fn, *a)


def _write(run, t, stride):
    parts = run.pair.cpu.particles(t)[::stride].copy()
    run.pair.gpu.write_particles(t, parts)
    run.pair.cpu.write_particles(t, parts)


def _attach(run):
    import torch

    run.records = 4 * max(p.capacity for p in run.pair.spawner.particle_settings)  # (a ring that grows under a burst stays inside)
    run.buf = torch.zeros((run.records * 16,), dtype=torch.float32, device="cuda")
    run.pair.gpu.attach_instances(run.buf.data_ptr(), run.records)
    run.detach_in = 2


def _detach(run, what):
    n = run.pair.gpu.count(0)
    assert n <= run.records
    run.keep(f"{what} attached records", run.buf[: n * 16].cpu().numpy())
    run.pair.gpu.attach_instances(0, 0)
    run.buf = None


def _volume(run, centre):
    return run.system.count_in_volumes([run.pair.gpu], [S.Collider.Sphere(centre, 2.5)])


def _reader(run, name, t, stride, what, centre):
    keep = lambda arr: run.keep(f"{what} {name}", arr)
    if name == "read_particles":
        run.read(what)
    elif name == "pack_instances":
        keep(first_readers.unsorted_host(run))
    elif name == "pack_instances_device":
        keep(first_readers.unsorted_device(run))
    elif name == "pack_instances_sorted":
        keep(first_readers.sorted_host(run))
    elif name == "pack_instances_sorted_device":
        keep(first_readers.sorted_device(run))
    elif name == "aabb":
        box = run.pair.gpu.aabb()
        keep(np.concatenate([[np.float32(box[0])], box[1], box[2]]))
    elif name == "counts":
        keep(np.array(run.pair.gpu.counts(), dtype=np.int64))
    elif name == "poll_finished":
        keep(np.array([run.pair.gpu.poll_finished(), run.pair.gpu.active()]))
    elif name == "updated_total":
        keep(np.array([run.system.updated_total()], dtype=np.int64))
    elif name == "synchronize":
        run.system.synchronize()
    elif name == "write_particles":
        _write(run, t, stride)
    elif name == "attach_instances":
        if getattr(run, "buf", None) is None:
            _attach(run)
    elif name == "set_colliders":
        run.system.set_colliders([])
    elif name == "cast_rays":
        keep(_ray(run))
    elif name == "count_in_volumes":
        keep(_volume(run, centre))
    else:
        raise AssertionError(name)


def _play(run, case, c):
    """the script of case `c` on one run and its oracle twin"""
    pair, steps, centre = run.pair, 0, c["transform"].translation
    _track(run)
    run.kinds, run.detach_in = [], 0
    for action in c["script"]:
        kind = action[0]
        what = f"case {case} frame {steps}"
        if kind == "step":
            _call(run, "step", Run.step, run, action[1])
            steps += 1
            if run.detach_in:
                run.detach_in -= 1
                if not run.detach_in:
                    _call(run, "read", _detach, run, what)
        elif kind == "set_transform":
            _call(run, "keep", pair.gpu.set_transform, S.Transform(action[1], action[2]))
            pair.cpu.set_origin(action[1], action[2])
        elif kind == "set_parent_velocity":
            _call(run, "keep", pair.gpu.set_parent_velocity, action[1])
            pair.cpu.set_parent_velocity(action[1])
        elif kind == "set_modifier":
            _call(run, "keep", pair.gpu.set_modifier, S.EffectModifier(action[1], action[2]))
            pair.cpu.set_modifier(S.EffectModifier(action[1], action[2]))
        elif kind == "queue":
            _call(run, "keep", pair.gpu.queue_particles, action[1])
            pair.cpu.queue_particles(action[1])
        elif kind == "read":
            _call(run, "read", _reader, run, action[1], action[2], action[3], what, centre)
            _call(run, "after", run.system.synchronize)
            if run.rule:  # nothing is pending behind a reader
                assert _tail(run, 1) == [W + (0,)], (what, action[1], _tail(run, 3))
        else:
            for t in range(pair.n_types):
                run.keep(f"{what} final path of type {t}", np.array([pair.gpu.update_mode(t)]))
            run.totals(what)
    return steps


def _groups(run, limit, what):
    """the A run's log by kind of call -> (depths of the fused launches frames put on the stream, the depth each reader found pending,
    the depth anything else -- a keeper -- found pending and flushed)"""
    closed, flushed, other = [], [], []
    for kind, (fused, alone, frames) in zip(run.kinds, _tail(run, len(run.kinds))):
        assert 2 * fused <= frames <= fused * limit, (what, kind, fused, alone, frames, limit)
        assert fused + alone <= 1 or kind == "step", (what, kind, fused, alone)  # (a call finds ONE group pending)
        depth = frames if fused == 1 else None
        if kind == "step":
            closed += [depth] if fused == 1 else ["?"] * fused
        elif kind == "read":
            flushed.append(depth if fused else alone)
        elif fused or alone:
            other.append(depth if fused else alone)
    return closed, flushed, other


def _one_case(monkeypatch, case):
    from bevy_firework_amd.system import ParticleSystem

    c = ff.draw_case(case)
    limit = ff.depth_limit(c["env"])
    reads, t0 = {}, time.perf_counter()
    for name, own in CONTEXTS.items():
        for k in CLEARED:
            monkeypatch.delenv(k, raising=False)  # (the product's choice, whatever the path matrix dealt this test)
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0")) + tuple(c["env"].items()) + tuple(own.items()):
            monkeypatch.setenv(k, v)
        with ParticleSystem(device=0, seed=SEED) as system:
            pair = Pair(system, c["spawner"], c["transform"], seed=SEED, uid=c["uid"], modifier=c["modifier"])
            run = Run2(system, pair, name == "A")  # (rule False: Run2.did asserts that the call fused and flushed nothing)
            assert all(pair.gpu.update_path(t)[0] == "fifo" for t in range(pair.n_types))
            steps = _play(run, case, c)
            reads[name] = run.reads
            if name == "C":
                assert system.spin_launches() == 0
            if name == "A":
                fused_frames, alone = _accounted(run, steps)
                closed, flushed, other = _groups(run, limit, f"case {case}")
                assert fused_frames == system.fuse_frames() and alone == system.fuse2_launches()[1]
                stats = dict(steps=steps, fused=system.fuse2_launches()[0], fused_frames=fused_frames, alone=alone, closed=closed, flushed=flushed,
                             other=other, whole=system.whole_tiles(), spins=system.spin_launches(), newborn=system.newborn_spin_launches(),
                             rings=pair.n_types, limit=limit, live=pair.gpu.counts())
            pair.cpu.close()
    names = [w for w, _ in reads["A"]]
    assert names == [w for w, _ in reads["B"]] == [w for w, _ in reads["C"]] and len(names) > 2
    digest = hashlib.sha256()
    for (what, a), (_, b), (_, cc) in zip(reads["A"], reads["B"], reads["C"]):
        assert a == b, f"{what}: the bits differ between the run that fuses (A) and the run with FW_FUSE2=0 (B)"
        assert a == cc, f"{what}: the bits differ between the run that fuses (A) and the run without fusing, deferred spin and derived ages (C)"
        digest.update(a)
    stats.update(seconds=time.perf_counter() - t0, reads=len(names), bytes=sum(len(a) for _, a in reads["A"]), digest=digest.hexdigest()[:16])
    STATS[case] = stats
    print(f"[fifo fuzz] case {case}: {stats['seconds']:.2f} s, {stats['rings']} ring(s) live {stats['live']}, depth limit {limit}, {steps} frames: "
          f"{stats['fused_frames']} in {stats['fused']} fused launches, {alone} alone; closed {closed}; readers found pending {flushed}; keepers "
          f"flushed {other}; whole tiles {stats['whole']}, spin replays {stats['spins']}, newborn-spin launches {stats['newborn']}; {stats['reads']} reads, "
          f"{stats['bytes']} bytes, identical in A, B and C (sha256 {stats['digest']})")


@pytest.mark.parametrize("case", list(range(OFF, OFF + ff.CASES + EXTRA)))
def test_random_ring_under_a_random_host(monkeypatch, case):
    _one_case(monkeypatch, case)


def test_the_random_cases_reached_the_machinery():
    """bookkeeping over the A runs of the cases above: conditions that keep the suite from passing without work"""
    if len(STATS) < ff.CASES:
        pytest.skip("the random ring cases did not run in this session")
    n = len(STATS)
    closed, flushed = {}, {}
    for s in STATS.values():
        for d in s["closed"]:
            closed[d] = closed.get(d, 0) + 1
        for d in s["flushed"]:
            flushed[d] = flushed.get(d, 0) + 1
    figures = dict(
        cases=n, fused_once=sum(s["fused"] >= 1 for s in STATS.values()), a_third_fused=sum(3 * s["fused_frames"] >= s["steps"] for s in STATS.values()),
        whole_tiles=sum(s["whole"][1] > 0 for s in STATS.values()), spin_replays=sum(s["spins"] > 0 for s in STATS.values()),
        newborn_spin=sum(s["newborn"] > 0 for s in STATS.values()), two_rings_fused=sum(s["rings"] == 2 and s["fused"] >= 1 for s in STATS.values()),
        closed_depths=dict(sorted(closed.items(), key=str)), pending_depths_readers_found=dict(sorted(flushed.items())),
        seconds_max=round(max(s["seconds"] for s in STATS.values()), 2), seconds_total=round(sum(s["seconds"] for s in STATS.values()), 1))
    print(f"[fifo fuzz] suite: {figures}")
    assert 4 * figures["fused_once"] >= 3 * n, figures
    assert 2 * figures["a_third_fused"] >= n, figures
    assert all(closed.get(d, 0) >= 1 for d in range(2, 17)), figures
    assert all(flushed.get(d, 0) >= 1 for d in range(1, 16)), figures
    assert figures["whole_tiles"] >= 10 and figures["spin_replays"] >= 10 and figures["two_rings_fused"] >= 5, figures
