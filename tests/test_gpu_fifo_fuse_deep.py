"""Up to four frames of an unread FIFO ring in one launch (fw_ctx::withheld as a group, FwFuseArgs, the depth-3 and depth-4 instantiations of
fw_k_update_fifo2; csrc/fw_fuse2.h).  The cases, the two runs of each (FW_FUSE2=1 against FW_FUSE2=0, next to
the CPU oracle) and the knobs that force the machinery at small sizes are tests/test_gpu_fifo_fuse2.py's, whose `both` and Run2 this
file borrows; on top of them FW_FUSE_DEEP_MIN=1 (a group may be deeper than two frames at any size) and FW_FUSE_DEPTH.  Every field of
every read, the counts and updated_total carry the same bits in both runs, and the call-by-call log of fw_debug_fuse2 AND
fw_debug_fuse_frames says what each call did: W nothing (the frame was withheld), X a withheld frame went out alone, F a fused launch --
of how many frames, the second counter says.  Needs an MI355X."""
import numpy as np
import pytest

import first_readers
import oracle  # noqa: F401
from test_gpu_fifo_fuse2 import F, W, X, Run2, _flushed, _fused, both
from test_gpu_fifo_spinless import _two_types
from test_gpu_spin_defer import DT, _spawner

pytestmark = pytest.mark.gpu
DEEP = {"FW_FUSE_DEEP_MIN": "1"}


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _track(run):
    """from here on every call the run logs also logs the frames fused launches ran in it (fw_debug_fuse_frames): run.frames, entry
    for entry next to the tail of run.log"""
    run.frames = []

    def did(fn, *a, **kw):
        n0 = run.system.fuse_frames()
        out = Run2.did(run, fn, *a, **kw)
        run.frames.append(run.system.fuse_frames() - n0)
        return out

    run.did = did


def _start(run):
    """the ring has earned the rule and nothing is pending"""
    run.step(n=8)
    run.quiesce()
    _track(run)


def _tail(run, n):
    """what the last n calls did: (fused launches, frames flushed alone, frames run by fused launches)"""
    return [e + (f,) for e, f in zip(run.log[-n:], run.frames[-n:])]


def _groups(depth, n):
    """n unread frames from nothing pending at that depth: withheld ... fused, and the remainder withheld"""
    return ([W + (0,)] * (depth - 1) + [F + (depth,)]) * (n // depth) + [W + (0,)] * (n % depth)


def _flush_of(pending):
    """what the call that finds `pending` frames withheld does first: nothing, the kept launch, or ONE fused launch of that depth"""
    return (W + (0,), X + (0,), F + (2,), F + (3,))[pending]


def _accounted(run, stepped):
    """every frame since _start ran exactly once: in a fused launch or alone (nothing is pending when this is asked)"""
    if run.rule:
        fused_frames = sum(run.frames)
        alone = sum(e[1] for e in run.log[-len(run.frames):] if e)
        launched = stepped - fused_frames - alone  # (frames that were never withheld: their own launch)
        assert launched >= 0 and fused_frames + alone + launched == stepped, (fused_frames, alone, stepped)
        return fused_frames, alone
    return 0, 0


@pytest.mark.parametrize("stretch", [12, 13, 14, 15])
@pytest.mark.parametrize("depth", [3, 4])
def test_an_unread_stretch_read_at_its_end(monkeypatch, depth, stretch):
    def scenario(run):
        _start(run)
        run.step(n=stretch)
        if run.rule:
            assert _tail(run, stretch) == _groups(depth, stretch), (run.frame, _tail(run, stretch))
        run.did(run.read, "end")
        if run.rule:  # (the read flushes the remainder as one launch: the kept one, or a fused launch of depth 2 or 3)
            assert _tail(run, 1) == [_flush_of(stretch % depth)], _tail(run, 3)
            assert _accounted(run, stretch) == (stretch - (1 if stretch % depth == 1 else 0), 1 if stretch % depth == 1 else 0)
        run.totals("end")
        run.step(n=5)
        run.read("behind it")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH=str(depth), **DEEP)


def test_the_death_rule_closes_a_group_early(monkeypatch):
    """2.5-frame lifetimes: two cohorts live before a frame, one dies in each.  Two frames' dead are all the old particles; a third
    frame's would be particles born in the group: a group never exceeds two frames, whatever the depth allows"""
    def scenario(run):
        _start(run)
        run.step(n=21)
        if run.rule:
            assert all(f in (0, 2) for f in run.frames), run.frames
            # (the third frame is declined: the pair goes out as one fused launch in front of it, and it begins the next group)
            assert _tail(run, 21) == [W + (0,), W + (0,)] + [F + (2,), W + (0,)] * 9 + [F + (2,)], _tail(run, 21)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)]
            assert _accounted(run, 21) == (20, 1)
        run.totals("end")

    both(monkeypatch, _spawner(rate=270000.0, capacity=32768), scenario, FW_FUSE_DEPTH="4", **DEEP)


def test_the_capacity_closes_a_group_early(monkeypatch):
    """900 new particles per frame over 16-frame lifetimes in 16384 slots: 15 cohorts, 13500 particles, live before a frame.  The rule
    (fw_fuse2.h) wants the first frame's live particles and every frame's spawns inside the ring: three frames' do (16200), four
    frames' do not (17100) -- the fourth frame is declined, the three go out as one launch, and the ring is not grown"""
    per_frame, capacity = 900, 16384
    assert 15 * (per_frame + 1) + 3 * (per_frame + 1) <= capacity < 15 * (per_frame - 1) + 4 * (per_frame - 1)  # (a rate spawns n or n +- 1)

    def scenario(run):
        run.step(n=12)  # (with _start's eight: twenty frames, the ring is as full as it gets)
        _start(run)
        assert abs(run.pair.gpu.count(0) - 15 * per_frame) <= 15
        run.step(n=16)
        if run.rule:
            assert _tail(run, 16) == [W + (0,)] * 3 + [F + (3,), W + (0,), W + (0,)] * 4 + [F + (3,)], _tail(run, 16)
        assert run.pair.gpu.update_path(0)[0] == "fifo"
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)] and 4 not in run.frames
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, rate=per_frame * 60.0, capacity=capacity), scenario, FW_FUSE_DEPTH="4", **DEEP)


def test_the_head_goes_round_under_groups_of_three(monkeypatch):
    """2000 new particles per frame over 5.5-frame lifetimes in 16384 slots: 10000 live before a frame, three frames fit (16000) and
    their dead (6000) are old particles.  The head goes round five times in 41 frames: it wraps inside some groups, and the new
    particles of some groups straddle the buffer's end (two groups of spawning workgroups: spawn_a < n_spawn); the boundaries between
    the frames' new particles fall inside workgroups (2000 is no multiple of 256)"""
    def scenario(run):
        _start(run)
        run.step(n=41)
        if run.rule:
            assert _tail(run, 41) == _groups(3, 41), _tail(run, 41)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [_flush_of(2)]
        run.totals("end")
        assert 41 * 2000 > 5 * 16384

    both(monkeypatch, _spawner(life_frames=5.5, rate=120000.0, capacity=16384), scenario, FW_FUSE_DEPTH="3", **DEEP)


def test_three_different_dt_in_every_group(monkeypatch):
    def scenario(run):
        _start(run)
        for k in range(24):
            run.step(np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k))))
        if run.rule:
            assert _tail(run, 24) == _groups(3, 24)
        run.read("end")
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH="3", **DEEP)


def test_a_dt_of_zero_in_the_middle_of_a_stretch(monkeypatch):
    """a dt that defers no spin does not qualify: the two frames withheld so far go out as one fused launch, the frame runs alone"""
    def scenario(run):
        _start(run)
        run.step(n=6)  # (a group of four, and two frames withheld)
        run.step(np.float32(0.0))
        if run.rule:
            assert _tail(run, 7) == _groups(4, 6) + [F + (2,)], _tail(run, 7)
        run.did(run.system.synchronize)
        assert _tail(run, 1) == [W + (0,)]  # (the frame itself was not withheld)
        run.read("right after")
        run.step(n=9)
        run.read("later")
        run.totals("later")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH="4", **DEEP)


FIRST_READERS = {
    "read_particles": lambda run: run.keep("first", run.pair.gpu.particles(0)),
    "pack_instances": lambda run: run.keep("first", first_readers.unsorted_host(run)),
    "pack_instances_device": lambda run: run.keep("first", first_readers.unsorted_device(run)),
    "pack_instances_sorted": lambda run: run.keep("first", first_readers.sorted_host(run)),
    "pack_instances_sorted_device": lambda run: run.keep("first", first_readers.sorted_device(run)),
}


@pytest.mark.parametrize("pending", [1, 2, 3])
@pytest.mark.parametrize("name", list(FIRST_READERS))
def test_first_readers_with_one_two_and_three_frames_withheld(monkeypatch, name, pending):
    """the reader puts the group on the stream first -- one launch, whatever its depth -- and sees what the run with FW_FUSE2=0 sees"""
    def scenario(run):
        _start(run)
        run.step(n=4 + pending)
        if run.rule:
            assert _tail(run, 4 + pending) == _groups(4, 4 + pending)
        run.did(FIRST_READERS[name], run)
        if run.rule:
            assert _tail(run, 1) == [_flush_of(pending)], (name, _tail(run, 4))
        run.step(n=5)
        run.read("behind it")
        run.totals("behind it")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH="4", **DEEP)


def test_two_rings_in_one_launch(monkeypatch):
    def scenario(run):
        _start(run)
        run.step(n=13)
        run.did(run.read, "end")
        if run.rule:
            fused_frames, alone = _accounted(run, 13)
            assert fused_frames + alone == 13 and max(run.frames) >= 3, _tail(run, 14)
        run.totals("end")

    both(monkeypatch, _two_types(_spawner(life_frames=16.0, capacity=16384), _spawner(life_frames=8.0, rate=60000.0, capacity=16384)), scenario,
         FW_FUSE_DEPTH="4", **DEEP)


def test_depth_two_set_explicitly_against_the_default_depth(monkeypatch):
    """FW_FUSE_DEPTH=2 is round 22's rule: pairs.  The default depth runs the same frames in groups of four; every read carries the
    same bits under both"""
    def scenario(run):
        _start(run)
        run.step(n=14)
        depth = max(run.frames) if run.rule else 0
        run.did(run.read, "end")
        run.totals("end")
        run.step(n=7)
        run.read("later")
        return depth, list(run.reads)

    spawner = _spawner(life_frames=16.0, capacity=16384)
    _, (depth_2, reads_2) = both(monkeypatch, spawner, scenario, FW_FUSE_DEPTH="2", **DEEP)
    monkeypatch.delenv("FW_FUSE_DEPTH", raising=False)
    _, (depth_default, reads_default) = both(monkeypatch, spawner, scenario, **DEEP)
    assert depth_2 == 2 and depth_default == 4
    assert [w for w, _ in reads_2] == [w for w, _ in reads_default] and len(reads_2) > 3
    for (what, a), (_, b) in zip(reads_2, reads_default):
        assert a == b, f"{what}: the bits differ between FW_FUSE_DEPTH=2 and the default depth"
