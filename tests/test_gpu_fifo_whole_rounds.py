"""The whole-tile arm of the fused FIFO forms as round 30 left it (fw_update_fifo_body; FwFuseArgs::move; csrc/fw_kernels.h):
a whole tile's loads are issued round by round and each round waits for its own, acceleration and drag come per ring from the kernel
arguments instead of the type record, the arm ends its workgroup -- the one with index 0 in its segment publishes the counts from
there --, and it asks for the age rule.  None of it changes what a reader sees.  Every case is tests/test_gpu_fifo_whole_tiles.py's
`on_and_off`: tests/test_gpu_fifo_fuse2.py's `both` -- the same system with FW_FUSE2=1 and FW_FUSE2=0 next to the CPU oracle, every read
bit-equal between the two and checked against the oracle -- run with FW_WHOLE_TILES=1 and with FW_WHOLE_TILES=0: every field of every
read, the counts and updated_total must carry the same bits under both, and fw_debug_whole_tiles must be zero with the switch off.
FW_FUSE_DEEP_MIN=1 and FW_FUSE_WIDE_MIN=1 as there; rings of 16384 slots: 16 tiles; groups of two and of eight frames.

A ring that keeps its age -- a type that reports its destroyed particles -- is never part of a fused launch: the host withholds a frame
only of rings that defer their spin in it, only a ring under the age rule does (launch_fifo: ring_rules), and FwWithheld::join declines a
ring with a destroyed-records buffer.  So no fused launch loads an age plane, and the arm holds none; the last case keeps such a ring
next to one under the age rule and asks that nothing of it was ever fused.  Needs an MI355X."""
import dataclasses

import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from test_gpu_fifo_fuse_deep import _start, _track
from test_gpu_fifo_spinless import _two_types
from test_gpu_fifo_whole_tiles import CAPACITY, WIDE, _bursts, _dt, on_and_off
from test_gpu_spin_defer import DT, _spawner

pytestmark = pytest.mark.gpu
DEPTHS = [2, 8]


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the whole-tile arm belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


@pytest.mark.parametrize("depth", DEPTHS)
def test_new_particles_that_straddle_the_rings_end(monkeypatch, depth):
    """500 new particles in every frame over 20.5-frame lifetimes: 10 250 live before a frame, the head in mid-tile nearly always.  In 76
    frames 38 000 slots are handed out, the ring's 16 384 more than twice over: twice the new particles of a launch -- 500 alone, or a
    group's 1000 to 4000 -- cross the ring's end, so both groups of spawning workgroups exist, beside whole tiles and the partly filled
    ones at both ends of the live range."""
    def scenario(run):
        for k in range(76):
            run.pair.queue(500)
            run.step(_dt(k) if k >= 30 else DT)
            if k == 29:
                run.quiesce()
            if k in (45, 59):
                run.read(f"frame {k}")
        run.read("end")
        run.totals("end")
        assert run.pair.gpu.update_path(0)[0] == "fifo" and 9000 <= run.pair.gpu.count(0) <= 11000

    launches, tiles = on_and_off(monkeypatch, _bursts(20.5), scenario, FW_FUSE_DEPTH=str(depth), **WIDE)
    assert launches >= 6 and tiles >= 5 * 6, (launches, tiles)


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_group_whose_first_frame_finds_the_ring_empty(monkeypatch, depth):
    """two rings in one launch.  The first keeps the launch on four-round tiles and has whole tiles; the second, fed on demand alone, is
    empty while it earns the rule with it (every threshold at 0: an empty ring defers, and joins a group).  Then, with nothing pending, it
    is handed 700 particles: the group that frame begins lays the ring out without a live tile -- three spawning workgroups, the first of
    which publishes the ring's counts -- next to a ring whose whole tiles end their workgroups in the arm.  (That group carries nine spawn
    ops at depth 8, one more than a launch holds, and closes a frame early; the groups behind it reach the depth.)"""
    steady, burst = _spawner(life_frames=16.0, capacity=CAPACITY), _bursts(40.0)

    def scenario(run):
        run.step(n=8)
        run.quiesce()
        _track(run)
        run.whole_base = run.system.whole_tiles()
        run.pair.queue(700)
        run.step(n=3 * depth + 1)
        if run.rule:
            # (the frame that found the ring empty was withheld and ran in the first fused launch, depth - 1 calls later)
            assert max(run.frames) == depth and run.frames[:depth - 1] == [0] * (depth - 1) and run.frames[depth - 1] >= min(depth, 7), run.frames
        run.read("end")
        run.totals("end")
        assert run.pair.gpu.count(1) == 700

    empty = {"FW_SPIN_DEFER_MIN": "0", "FW_FUSE2_MIN": "0", "FW_FUSE_DEEP_MIN": "0", "FW_FUSE_WIDE_MIN": "0"}
    launches, tiles = on_and_off(monkeypatch, _two_types(steady, burst), scenario, FW_FUSE_DEPTH=str(depth), **empty)
    assert launches >= 2 and tiles >= 4 * launches, (launches, tiles)  # (5280 or more live in the first ring, nobody dies yet)


@pytest.mark.parametrize("depth", DEPTHS)
def test_a_group_in_which_no_frame_spawns(monkeypatch, depth):
    """1400 particles in each of ten frames over 60-frame lifetimes, then nothing: the launches behind them hold ring tiles alone --
    thirteen whole ones and one partly filled --, and the workgroup with index 0, the launch's first, is a whole tile: the arm publishes
    the ring's counts, the launch's live_next and done_tag."""
    def scenario(run):
        for k in range(10):
            run.pair.queue(1400)
            run.step()
        run.quiesce()
        _track(run)
        run.whole_base = run.system.whole_tiles()
        for k in range(2 * depth + 1):
            run.step(_dt(k))
        if run.rule:
            assert max(run.frames) == depth, run.frames
        run.read("end")
        run.totals("end")
        assert run.pair.gpu.count(0) == 14000

    launches, tiles = on_and_off(monkeypatch, _bursts(60.0), scenario, FW_FUSE_DEPTH=str(depth), **WIDE)
    assert launches >= 2 and tiles == 13 * launches, (launches, tiles)


@pytest.mark.parametrize("depth", DEPTHS)
def test_two_rings_of_different_types_in_one_launch(monkeypatch, depth):
    """two types whose accelerations differ in all three components, none of them zero, and whose drags differ: a whole tile of either
    ring computes with its own row of FwFuseArgs::move, component by component -- the oracle and the unfused run say which.  The second
    ring is filled on demand before the groups begin (1300 in each of eight frames over 60-frame lifetimes: ten whole tiles), so that a
    frame of a group carries one spawn op and the groups reach eight frames."""
    a, b = _spawner(life_frames=16.0, capacity=CAPACITY), _bursts(60.0)
    pa = dataclasses.replace(a.particle_settings[0], acceleration=(0.5, -9.81, 1.25), linear_drag=0.2)
    pb = dataclasses.replace(b.particle_settings[0], acceleration=(-1.5, 2.0, -0.75), linear_drag=0.65)
    spawner = _two_types(S.ParticleSpawner([pa], a.emission_settings), S.ParticleSpawner([pb], b.emission_settings))

    def scenario(run):
        for k in range(8):
            run.pair.queue(1300)
            run.step()
        run.quiesce()
        _track(run)
        run.whole_base = run.system.whole_tiles()
        for k in range(2 * depth + 1):
            run.step(_dt(k))
        if run.rule:
            assert max(run.frames) == depth, run.frames
        run.read("end")
        run.totals("end")
        assert [run.pair.gpu.update_path(t)[0] for t in (0, 1)] == ["fifo", "fifo"]

    launches, tiles = on_and_off(monkeypatch, spawner, scenario, FW_FUSE_DEPTH=str(depth), **WIDE)
    # (5280 or more live in the first ring, four whole tiles or more, and the second ring's ten, in each launch)
    assert launches >= 2 and tiles >= 14 * launches, (launches, tiles)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("destroyed", [False, True], ids=["the age rule", "the age kept"])
def test_the_age_kept_next_to_the_age_rule(monkeypatch, depth, destroyed):
    """the same spinning particles under the age rule and, in a type that reports its destroyed particles, with the age kept.  The first
    fuses and takes the arm.  The second is never withheld (this file's head): every frame has its own launch, and the bits and the
    oracle hold all the same."""
    def scenario(run):
        _start(run)
        run.whole_base = run.system.whole_tiles()
        for k in range(2 * depth + 1):
            run.step(_dt(k))
        if run.rule:
            assert max(run.frames) == (0 if destroyed else depth), run.frames
        run.read("end")
        run.totals("end")

    sp = _spawner(life_frames=16.0, capacity=CAPACITY, **({"particles_destroyed": lambda dead: None} if destroyed else {}))
    launches, tiles = on_and_off(monkeypatch, sp, scenario, FW_FUSE_DEPTH=str(depth), **WIDE)
    if not destroyed:  # (a ring that spins and keeps its age runs no spin-less launch: nothing is counted for it)
        assert launches >= 2 and tiles >= 4 * launches, (launches, tiles)  # (5280 or more live, nobody dies yet)
