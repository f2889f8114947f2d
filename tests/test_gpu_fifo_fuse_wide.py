"""Up to eight frames of an unread FIFO ring in one launch (fw_ctx::withheld as a group of up to seven withheld frames, FwFuseArgs, the depth-5
to depth-8 instantiations of fw_k_update_fifo2; csrc/fw_fuse2.h).  The cases, the two runs of each (FW_FUSE2=1
against FW_FUSE2=0, next to the CPU oracle) and the knobs that force the machinery at small sizes are tests/test_gpu_fifo_fuse2.py's,
whose `both` and Run2 this file borrows as tests/test_gpu_fifo_fuse_deep.py does (and that file's bookkeeping of the second counter);
on top of them FW_FUSE_DEEP_MIN=1 and FW_FUSE_WIDE_MIN=1 (a group may be deeper than two, and than four, frames at any size) and
FW_FUSE_DEPTH.  Every field of every read, the counts and updated_total carry the same bits in both runs, and the call-by-call log of
fw_debug_fuse2 AND fw_debug_fuse_frames says what each call did: W nothing (the frame was withheld), X a withheld frame went out alone,
F a fused launch -- of how many frames, the second counter says.
The smallest shapes: ~667 new particles per frame over 16-frame lifetimes, 10 000 live, in 16384 slots -- eight frames' spawns reach
15 336 slots and fit, a ninth would not.  Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from test_gpu_fifo_fuse2 import F, W, X, both
from test_gpu_fifo_fuse_deep import FIRST_READERS, _accounted, _groups, _start, _tail
from test_gpu_fifo_spinless import _two_types
from test_gpu_spin_defer import DT, _spawner

pytestmark = pytest.mark.gpu
WIDE = {"FW_FUSE_DEEP_MIN": "1", "FW_FUSE_WIDE_MIN": "1"}


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _flush_of(pending):
    """what the call that finds `pending` frames withheld does first: nothing, the kept launch, or ONE fused launch of that depth"""
    return W + (0,) if pending == 0 else X + (0,) if pending == 1 else F + (pending,)


def _closed_early(depth, groups):
    """a stretch in which every group is closed by the frame behind it being declined: `depth` frames withheld, then -- `groups` times --
    the call that puts them on the stream as one launch and withholds its own frame; one frame is pending at the end"""
    return [W + (0,)] * depth + ([F + (depth,)] + [W + (0,)] * (depth - 1)) * (groups - 1) + [F + (depth,)]


@pytest.mark.parametrize("stretch", [16, 17, 18, 19])
@pytest.mark.parametrize("depth", [5, 6, 7, 8])
def test_an_unread_stretch_read_at_its_end(monkeypatch, depth, stretch):
    def scenario(run):
        _start(run)
        run.step(n=stretch)
        if run.rule:
            assert _tail(run, stretch) == _groups(depth, stretch), (run.frame, _tail(run, stretch))
        run.did(run.read, "end")
        rest = stretch % depth
        if run.rule:  # (the read flushes the remainder as one launch: the kept one for one frame, a fused launch for two to seven)
            assert _tail(run, 1) == [_flush_of(rest)], _tail(run, 3)
            assert _accounted(run, stretch) == (stretch - (1 if rest == 1 else 0), 1 if rest == 1 else 0)
        run.totals("end")
        run.step(n=5)
        run.read("behind it")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH=str(depth), **WIDE)


@pytest.mark.parametrize("pending", [4, 5, 6, 7])
@pytest.mark.parametrize("name", list(FIRST_READERS))
def test_first_readers_with_four_to_seven_frames_withheld(monkeypatch, name, pending):
    """the reader puts the group on the stream first -- one launch, whatever its depth -- and sees what the run with FW_FUSE2=0 sees"""
    def scenario(run):
        _start(run)
        run.step(n=8 + pending)
        if run.rule:
            assert _tail(run, 8 + pending) == _groups(8, 8 + pending)
        run.did(FIRST_READERS[name], run)
        if run.rule:
            assert _tail(run, 1) == [_flush_of(pending)], (name, _tail(run, 8))
        run.step(n=5)
        run.read("behind it")
        run.totals("behind it")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH="8", **WIDE)


def test_eight_different_dt_in_every_group(monkeypatch):
    def scenario(run):
        _start(run)
        for k in range(24):
            run.step(np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k))))
        if run.rule:
            assert _tail(run, 24) == _groups(8, 24), _tail(run, 24)
        run.read("end")
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario, FW_FUSE_DEPTH="8", **WIDE)


def test_the_capacity_closes_a_group_early(monkeypatch):
    """760 new particles per frame over 16-frame lifetimes in 16384 slots: 15 cohorts, 11 400 particles, live before a frame.  The rule
    (fw_fuse2.h) wants the first frame's live particles and every frame's spawns inside the ring: six frames' do (15 960), seven
    frames' do not (16 720) -- the seventh frame is declined, the six go out as one launch, and the ring is not grown"""
    per_frame, capacity = 760, 16384
    assert 15 * (per_frame + 1) + 6 * (per_frame + 1) <= capacity < 15 * (per_frame - 1) + 7 * (per_frame - 1)  # (a rate spawns n or n +- 1)

    def scenario(run):
        run.step(n=12)  # (with _start's eight: twenty frames, the ring is as full as it gets)
        _start(run)
        assert abs(run.pair.gpu.count(0) - 15 * per_frame) <= 15
        run.step(n=19)
        if run.rule:
            assert _tail(run, 19) == _closed_early(6, 3), _tail(run, 19)
        assert run.pair.gpu.update_path(0)[0] == "fifo"
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)] and not {7, 8} & set(run.frames)
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=16.0, rate=per_frame * 60.0, capacity=capacity), scenario, FW_FUSE_DEPTH="8", **WIDE)


def test_the_death_rule_closes_a_group_early(monkeypatch):
    """6.5-frame lifetimes: six cohorts live before a frame, one dies in each.  Six frames' dead are all the old particles; a seventh
    frame's would be particles born in the group: a group never exceeds six frames, whatever the depth allows (the ring has room for
    seven frames' spawns: 10 000 live + 7 x 1667 in 32768 slots)"""
    def scenario(run):
        _start(run)
        run.step(n=19)
        if run.rule:
            assert all(f in (0, 6) for f in run.frames), run.frames
            assert _tail(run, 19) == _closed_early(6, 3), _tail(run, 19)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)]
            assert _accounted(run, 19) == (18, 1)
        run.totals("end")

    both(monkeypatch, _spawner(life_frames=6.5, rate=100000.0, capacity=32768), scenario, FW_FUSE_DEPTH="8", **WIDE)


def test_the_head_goes_round_under_groups_of_eight(monkeypatch):
    """700 new particles per frame over 9.5-frame lifetimes in 16384 slots: 6300 live before a frame, eight frames fit (11 900) and
    their dead (5600) are old particles.  42 000 spawns in 60 frames: the head goes round more than twice, it wraps inside some
    groups, and the new particles of some groups straddle the buffer's end (two groups of spawning workgroups: spawn_a < n_spawn); the
    boundaries between the frames' new particles fall inside workgroups (700 is no multiple of 256)"""
    def scenario(run):
        _start(run)
        run.step(n=60)
        if run.rule:
            assert _tail(run, 60) == _groups(8, 60), _tail(run, 60)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [_flush_of(4)]
        run.totals("end")
        assert 60 * 700 > 2 * 16384

    both(monkeypatch, _spawner(life_frames=9.5, rate=42000.0, capacity=16384), scenario, FW_FUSE_DEPTH="8", **WIDE)


def test_two_rings_in_one_launch_close_their_groups_at_four_frames(monkeypatch):
    """eight spawn ops travel in a launch (FW_INLINE_OPS): two rings with one op per frame each fill them in four frames.  The fifth
    frame is declined whatever the depth allows: the four go out as one launch, and it begins the next group"""
    def scenario(run):
        _start(run)
        run.step(n=17)
        if run.rule:
            assert max(run.frames) == 4 and all(f in (0, 4) for f in run.frames), run.frames
            assert _tail(run, 17) == _closed_early(4, 4), _tail(run, 17)
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)]
            assert _accounted(run, 17) == (16, 1)
        run.totals("end")

    both(monkeypatch, _two_types(_spawner(life_frames=16.0, capacity=16384), _spawner(life_frames=8.0, rate=60000.0, capacity=16384)), scenario,
         FW_FUSE_DEPTH="8", **WIDE)


def test_the_wide_threshold_against_the_narrow_one(monkeypatch):
    """without FW_FUSE_WIDE_MIN the small ring holds round 23's threshold alone (FW_FUSE_DEEP_MIN=1): groups of four, FW_FUSE_NARROW.  With
    it the default depth applies, somewhere from four to eight.  Every read carries the same bits under both"""
    def scenario(run):
        _start(run)
        run.step(n=17)
        depth = max(run.frames) if run.rule else 0
        run.did(run.read, "end")
        run.totals("end")
        run.step(n=7)
        run.read("later")
        return depth, list(run.reads)

    spawner = _spawner(life_frames=16.0, capacity=16384)
    monkeypatch.delenv("FW_FUSE_DEPTH", raising=False)
    monkeypatch.delenv("FW_FUSE_WIDE_MIN", raising=False)
    _, (depth_narrow, reads_narrow) = both(monkeypatch, spawner, scenario, FW_FUSE_DEEP_MIN="1")
    _, (depth_wide, reads_wide) = both(monkeypatch, spawner, scenario, **WIDE)
    assert depth_narrow == 4 and 4 <= depth_wide <= 8
    assert [w for w, _ in reads_narrow] == [w for w, _ in reads_wide] and len(reads_narrow) > 3
    for (what, a), (_, b) in zip(reads_narrow, reads_wide):
        assert a == b, f"{what}: the bits differ between groups of four and the default depth"
