"""Nine to sixteen frames of an unread FIFO ring in one launch: the far tier (fw_ctx::fuse_far_depth / fuse_far_min, FwFarArgs, the depth-9
to depth-16 instantiations fw_k_update_fifo_far, one op for a run of identical frames -- fw_op_continues; csrc/fw_fuse2.h, fw_withheld.h,
fw_k_rings_far.hip).  The cases, the two runs of each (FW_FUSE2=1 against FW_FUSE2=0, next to the CPU oracle) and
the knobs that force the machinery at small sizes are tests/test_gpu_fifo_fuse_wide.py's, whose helpers this file borrows the way that
file borrows them; on top of its WIDE pair FW_FUSE_FAR_MIN=1 (a group may be deeper than eight frames at any size) and FW_FUSE_FAR_DEPTH.
Every field of every read, the counts and updated_total carry the same bits in both runs, and the call-by-call log of fw_debug_fuse2 AND
fw_debug_fuse_frames says what each call did: W nothing (the frame was withheld), X a withheld frame went out alone, F a fused launch --
of how many frames, the second counter says.  A launch carries eight spawn ops: a group of more than eight frames of a ring that spawns
in every frame exists only where the frames' ops were merged, so every log with a depth above eight is a statement about the merge too.
The smallest shape: ~380 new particles per frame over 24-frame lifetimes in 16384 slots -- 23 cohorts live before a frame, sixteen
frames' spawns fit ((24 + 16) x 381 = 15 240) and sixteen frames' dead are all old particles.  Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from test_gpu_fifo_fuse2 import F, W, X, both
from test_gpu_fifo_fuse_deep import FIRST_READERS, _accounted, _groups, _start, _tail
from test_gpu_fifo_spinless import _two_types
from test_gpu_spin_defer import DT, _spawner

pytestmark = pytest.mark.gpu
WIDE = {"FW_FUSE_DEEP_MIN": "1", "FW_FUSE_WIDE_MIN": "1"}
FAR = dict(WIDE, FW_FUSE_DEPTH="8", FW_FUSE_FAR_MIN="1")
PER_FRAME, CAPACITY = 380, 16384
assert (24 + 16) * (PER_FRAME + 1) <= CAPACITY


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _ring(life_frames=24.0, per_frame=PER_FRAME, capacity=CAPACITY):
    return _spawner(life_frames=life_frames, rate=per_frame * 60.0, capacity=capacity)


def _cohorts_before_a_frame(life_frames):
    """the cohorts a ring in its steady state holds before a frame: the host's own arithmetic -- a cohort ages by fp32 additions of DT and
    dies in the update that takes its age to the lifetime"""
    age, life, k = np.float32(0.0), np.float32(float(DT) * life_frames), 0
    while True:
        age, k = np.float32(age + DT), k + 1
        if age >= life:
            return k - 1


def _flush_of(pending):
    """what the call that finds `pending` frames withheld does first: nothing, the kept launch, or ONE fused launch of that depth"""
    return W + (0,) if pending == 0 else X + (0,) if pending == 1 else F + (pending,)


def _closed_early(depth, groups):
    """a stretch in which every group is closed by the frame behind it being declined: `depth` frames withheld, then -- `groups` times --
    the call that puts them on the stream as one launch and withholds its own frame; one frame is pending at the end"""
    return [W + (0,)] * depth + ([F + (depth,)] + [W + (0,)] * (depth - 1)) * (groups - 1) + [F + (depth,)]


def _move(run, k):
    """the emitter's transform from here on: both sides"""
    tf = S.Transform((1.0 + 0.25 * k, 2.0, 3.0 - 0.125 * k))
    run.pair.gpu.set_transform(tf)
    run.pair.cpu.set_origin(tf.translation, tf.rotation)


@pytest.mark.parametrize("stretch", [32, 33, 34, 35])
@pytest.mark.parametrize("depth", [9, 12, 15, 16])
def test_an_unread_stretch_read_at_its_end(monkeypatch, depth, stretch):
    """(a)"""
    def scenario(run):
        _start(run)
        run.step(n=stretch)
        if run.rule:
            assert _tail(run, stretch) == _groups(depth, stretch), (run.frame, _tail(run, stretch))
        run.did(run.read, "end")
        rest = stretch % depth
        if run.rule:  # (the read flushes the remainder as ONE launch: the kept one for one frame, a fused launch for two to fifteen)
            assert _tail(run, 1) == [_flush_of(rest)], _tail(run, 3)
            assert _accounted(run, stretch) == (stretch - (1 if rest == 1 else 0), 1 if rest == 1 else 0)
        run.totals("end")
        run.step(n=5)
        run.read("behind it")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH=str(depth), **FAR)


@pytest.mark.parametrize("pending", [8, 9, 15])
@pytest.mark.parametrize("name", list(FIRST_READERS))
def test_first_readers_with_eight_nine_and_fifteen_frames_withheld(monkeypatch, name, pending):
    """(b) the reader puts the group on the stream first -- one launch, whatever its depth -- and sees what the run with FW_FUSE2=0 sees"""
    def scenario(run):
        _start(run)
        run.step(n=16 + pending)
        if run.rule:
            assert _tail(run, 16 + pending) == _groups(16, 16 + pending)
        run.did(FIRST_READERS[name], run)
        if run.rule:
            assert _tail(run, 1) == [_flush_of(pending)], (name, _tail(run, 16))
        run.step(n=5)
        run.read("behind it")
        run.totals("behind it")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_sixteen_different_dt_in_every_group(monkeypatch):
    """(c)"""
    def scenario(run):
        _start(run)
        for k in range(48):
            run.step(np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k))))
        if run.rule:
            assert _tail(run, 48) == _groups(16, 48), _tail(run, 48)
        run.read("end")
        run.totals("end")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_the_capacity_closes_a_group_early(monkeypatch):
    """(d) 460 new particles per frame over 24-frame lifetimes in 16384 slots: 23 cohorts live before a frame.  The rule (fw_fuse2.h) wants
    the first frame's live particles and every frame's spawns inside the ring: twelve frames' do (35 x 461 = 16 135), thirteen frames' do
    not (36 x 459 = 16 524) -- the thirteenth frame is declined, the twelve go out as one launch, and the ring is not grown.  (The case
    ends before the emitter's one-second cycle does, at frame 60: the frame that wraps the cycle spawns another count.)"""
    per_frame, live = 460, _cohorts_before_a_frame(24.0)
    assert live == 23
    assert (live + 12) * (per_frame + 1) <= CAPACITY < (live + 13) * (per_frame - 1)  # (a rate spawns n or n +- 1)

    def scenario(run):
        run.step(n=17)  # (with _start's eight: twenty-five frames, the ring is as full as it gets)
        _start(run)
        assert abs(run.pair.gpu.count(0) - live * per_frame) <= live
        run.step(n=25)
        assert run.frame < 60
        if run.rule:
            assert _tail(run, 25) == _closed_early(12, 2), _tail(run, 25)
        assert run.pair.gpu.update_path(0)[0] == "fifo"
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)] and not {13, 14, 15, 16} & set(run.frames)
        run.totals("end")

    both(monkeypatch, _ring(per_frame=per_frame), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_the_death_rule_closes_a_group_early(monkeypatch):
    """(e) 12.5-frame lifetimes: twelve cohorts live before a frame, one dies in each.  Twelve frames' dead are all the old particles; a
    thirteenth frame's would be particles born in the group: a group never exceeds twelve frames, whatever the depth allows (the ring
    has room for sixteen frames' spawns)"""
    assert _cohorts_before_a_frame(12.5) == 12 and (12 + 16) * (PER_FRAME + 1) <= CAPACITY

    def scenario(run):
        run.step(n=8)  # (with _start's eight: the ring is in its steady state)
        _start(run)
        run.step(n=37)
        if run.rule:
            assert all(f in (0, 12) for f in run.frames), run.frames
            assert _tail(run, 37) == _closed_early(12, 3), _tail(run, 37)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)]
            assert _accounted(run, 37) == (36, 1)
        run.totals("end")

    both(monkeypatch, _ring(life_frames=12.5), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_the_head_goes_round_under_groups_of_sixteen(monkeypatch):
    """(f) 480 new particles per frame over 16.5-frame lifetimes in 16384 slots: sixteen cohorts live before a frame, sixteen frames fit
    (32 x 481 = 15 392, and one more frame's worth beside them: the frame that wraps the emitter's one-second cycle spawns another
    count) and their dead are old particles.  40 320 spawns in 84 frames: the head goes round more than twice, it wraps inside some
    groups, and the new particles of some groups straddle the buffer's end (two groups of spawning workgroups: spawn_a < n_spawn); the
    boundaries between the frames' new particles fall inside workgroups (480 is no multiple of 256)"""
    per_frame = 480
    assert _cohorts_before_a_frame(16.5) == 16 and (16 + 16 + 1) * (per_frame + 1) <= CAPACITY and per_frame % 256 != 0

    def scenario(run):
        _start(run)
        run.step(n=84)
        if run.rule:
            assert _tail(run, 84) == _groups(16, 84), _tail(run, 84)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [_flush_of(4)]
        run.totals("end")
        assert 84 * per_frame > 2 * CAPACITY

    both(monkeypatch, _ring(life_frames=16.5, per_frame=per_frame), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_a_transform_that_changes_once_inside_a_group(monkeypatch):
    """(g) the frame behind the change brings an op that continues nobody's: the group holds two ops and still reaches sixteen frames"""
    def scenario(run):
        _start(run)
        run.step(n=5)
        _move(run, 1)
        run.step(n=27)
        if run.rule:
            assert _tail(run, 32) == _groups(16, 32), _tail(run, 32)
        run.did(run.read, "end")
        run.totals("end")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_a_transform_that_changes_every_frame_closes_groups_at_eight(monkeypatch):
    """(g) no op continues the one before it: eight ops travel in a launch, the ninth frame is declined and begins the next group"""
    def scenario(run):
        _start(run)
        for k in range(25):
            _move(run, k + 1)
            run.step()
        if run.rule:
            assert _tail(run, 25) == _closed_early(8, 3), _tail(run, 25)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)]
            assert _accounted(run, 25) == (24, 1)
        run.totals("end")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


def test_two_rings_with_still_emitters_reach_sixteen(monkeypatch):
    """(h) one op per ring for the whole group (below the far threshold the same two rings close their groups at four frames:
    tests/test_gpu_fifo_fuse_wide.py)"""
    def scenario(run):
        _start(run)
        run.step(n=35)
        if run.rule:
            assert _tail(run, 35) == _groups(16, 35), _tail(run, 35)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [_flush_of(3)]
            assert _accounted(run, 35) == (35, 0)
        run.totals("end")

    both(monkeypatch, _two_types(_ring(), _ring(life_frames=20.0)), scenario, FW_FUSE_FAR_DEPTH="16", **FAR)


@pytest.mark.parametrize("knob, depth", [({"FW_WHOLE_TILES": "0"}, 16), ({"FW_WHOLE_TILES": "1"}, 16), ({"FW_NEWBORN_SPIN": "1"}, 8)],
                         ids=["no whole-tile arm", "whole-tile arm", "eager newborns: no far tier"])
def test_depth_sixteen_under_the_other_switches(monkeypatch, knob, depth):
    """(i) the ring is full before the stretch: 23 cohorts live, sixteen die in a group, the survivors' slots hold whole tiles"""
    def scenario(run):
        run.step(n=16)
        _start(run)
        run.step(n=35)
        if run.rule:
            assert _tail(run, 35) == _groups(depth, 35), _tail(run, 35)
        run.did(run.read, "end")
        run.totals("end")

    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", **knob, **FAR)


def test_without_the_far_threshold_the_small_ring_stays_at_eight(monkeypatch):
    """(j)"""
    def scenario(run):
        _start(run)
        run.step(n=35)
        if run.rule:
            assert _tail(run, 35) == _groups(8, 35), _tail(run, 35)
        run.did(run.read, "end")
        run.totals("end")

    monkeypatch.delenv("FW_FUSE_FAR_MIN", raising=False)
    both(monkeypatch, _ring(), scenario, FW_FUSE_FAR_DEPTH="16", FW_FUSE_DEPTH="8", **WIDE)
