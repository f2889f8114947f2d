"""Whole ring tiles of spin-less FIFO launches (fw_fifo_tile_whole, the whole-tile arm of fw_update_fifo_body, FwFifoArgs::fuse_pad
[FW_FIFO_WHOLE]; csrc/fw_fuse2.h): a ring tile every slot of which holds a particle that lives through the launch
issues all of its loads first, runs its rounds without a divergent lane and stores unconditionally.  The same bits as the streaming loop.
Every case is tests/test_gpu_fifo_fuse2.py's `both` -- the same system with FW_FUSE2=1 and FW_FUSE2=0 next to the CPU oracle, every read
bit-equal between the two -- run twice, with FW_WHOLE_TILES=1 and with FW_WHOLE_TILES=0: every field of every read, the counts and
updated_total must carry the same bits under both, and fw_debug_whole_tiles must be non-zero with the switch on where the case has whole
tiles and zero with it off.  FW_FUSE_DEEP_MIN=1 and FW_FUSE_WIDE_MIN=1 as in tests/test_gpu_fifo_fuse_wide.py; rings of 16384 slots: 16
tiles.  Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from test_gpu_fifo import _nested_rings
from test_gpu_fifo_fuse2 import both
from test_gpu_fifo_fuse_deep import _start
from test_gpu_fifo_spinless import _still
from test_gpu_spin_defer import DT, Y, _rot_about, _spawner

pytestmark = pytest.mark.gpu
WIDE = {"FW_FUSE_DEEP_MIN": "1", "FW_FUSE_WIDE_MIN": "1"}
CAPACITY, TILE = 16384, 1024


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the whole-tile arm belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _bursts(life_frames):
    """_spawner's particles, spinning about Y, spawned on demand alone: the case decides every frame's number, so heads and live ranges
    fall where it wants them"""
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(float(DT) * life_frames), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]), capacity=CAPACITY, angular_drag=0.2,
                            base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT))
    es = [S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand(), initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), Y, 0.0),
                             initial_velocity_radial=S.RandF32(0.0, 1.0), initial_rotation=_rot_about(Y, 0.7),
                             initial_angular_velocity=S.RandVec3(S.RandF32(1.0, 4.0), Y, 0.0))]
    return S.ParticleSpawner([ps], es)


def on_and_off(monkeypatch, spawner, scenario, **env):
    """`scenario(run)` under `both`, with the switch on and off.  Returns fw_debug_whole_tiles of the run that fuses with the switch on,
    counted from where the scenario set `run.whole_base` (from the start where it did not)"""
    seen = {}

    def wrapped(run):
        scenario(run)
        (l1, t1), (l0, t0) = run.system.whole_tiles(), getattr(run, "whole_base", (0, 0))
        return (l1 - l0, t1 - t0), list(run.reads)

    for switch in ("1", "0"):
        _, seen[switch] = both(monkeypatch, spawner, wrapped, FW_WHOLE_TILES=switch, **env)
    (on, reads_on), (off, reads_off) = seen["1"], seen["0"]
    assert [w for w, _ in reads_on] == [w for w, _ in reads_off] and len(reads_on) > 0
    for (what, a), (_, b) in zip(reads_on, reads_off):
        assert a == b, f"{what}: the bits differ between FW_WHOLE_TILES=1 and FW_WHOLE_TILES=0"
    assert off == (0, 0), off
    return on


def _dt(k):
    return np.float32(DT * (1.0 + 0.3 * np.sin(0.7 * k)))


@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6, 7, 8])
def test_every_depth_with_a_different_dt_in_every_frame(monkeypatch, depth):
    """~667 new particles per frame over 16-frame lifetimes, from the ninth frame on: 5280 or more live before a launch and nobody dies
    yet -- a contiguous range of L particles holds at least L // 1024 - 1 whole tiles: four"""
    def scenario(run):
        _start(run)
        run.whole_base = run.system.whole_tiles()
        for k in range(2 * depth + 1):
            run.step(_dt(k))
        if run.rule:
            assert max(run.frames) == depth, run.frames
        run.read("end")
        run.totals("end")

    launches, tiles = on_and_off(monkeypatch, _spawner(life_frames=16.0, capacity=CAPACITY), scenario, FW_FUSE_DEPTH=str(depth), **WIDE)
    assert launches >= 2 and tiles >= 4 * launches, (launches, tiles)


def test_heads_and_ends_on_tile_boundaries_and_ranges_that_wrap(monkeypatch):
    """512 new particles in every frame over 20.5-frame lifetimes: 10 240 live before a frame.  The head advances by 512 slots a frame: on
    a tile boundary in every other frame and in mid-tile in the others; with the head on a boundary the live range ends on one (ten tiles
    exactly); the ring's 32 half-tiles go round once in 32 frames, so in 76 frames the live range wraps the ring's end for twenty frames,
    twice.  Groups of eight (their dead: 4096, four tiles) and, with FW_FUSE2=0, every frame by itself"""
    def scenario(run):
        for k in range(76):
            run.pair.queue(512)
            run.step(_dt(k) if k >= 30 else DT)
            if k == 29:
                run.quiesce()
            if k in (45, 59):
                run.read(f"frame {k}")
        run.read("end")
        run.totals("end")
        assert run.pair.gpu.update_path(0)[0] == "fifo" and 9000 <= run.pair.gpu.count(0) <= 11000

    launches, tiles = on_and_off(monkeypatch, _bursts(20.5), scenario, FW_FUSE_DEPTH="8", **WIDE)
    # (the launches behind frame 29 alone: 10 240 live, at most 4096 of them dead in a group -- five whole tiles or more in each)
    assert launches >= 6 and tiles >= 5 * 6, (launches, tiles)


def test_one_partly_filled_live_tile(monkeypatch):
    """128 new particles in every frame over 8.5-frame lifetimes: 1024 live before a frame, of which 128 die in it -- the 896 that live
    through a launch never fill a tile, wherever the head stands: no tile is whole, and the switch changes nothing"""
    def scenario(run):
        for k in range(40):
            run.pair.queue(128)
            run.step()
            if k == 25:
                run.quiesce()
        run.read("end")
        run.totals("end")
        assert run.system.spinless_launches() > 0 and run.pair.gpu.count(0) == 1024

    assert on_and_off(monkeypatch, _bursts(8.5), scenario, FW_FUSE_DEPTH="8", **WIDE) == (0, 0)


@pytest.mark.parametrize("destroyed", [False, True], ids=["the age rule", "the age kept"])
def test_a_type_that_cannot_turn_read_every_frame(monkeypatch, destroyed):
    """nothing is withheld from a host that reads every frame: the unfused spin-less form, with the age plane left alone (the age rule)
    and loaded, advanced and stored -- a type that reports its destroyed particles never runs under the age rule, and keeps the layout
    the spin-less forms ask for (FW_AGELESS=0 would take that away: no spin-less launch at all).  The host counts the whole tiles; the
    kernel keeps the streaming loop for them (the arm was measured slower in the unfused forms), so the switch must change nothing"""
    def scenario(run):
        run.step(n=20)
        for k in range(6):
            run.step(_dt(k))
            run.read(f"frame {k}", check=True)
        run.totals("end")
        assert run.system.spinless_launches() >= 6 and run.system.fuse2_launches() == (0, 0)

    sp = _still(life_frames=16.0, rate=40000.0, **({"particles_destroyed": lambda dead: None} if destroyed else {}))
    sp.particle_settings[0].capacity = CAPACITY
    launches, tiles = on_and_off(monkeypatch, sp, scenario, **WIDE)
    # (~10 000 live before a frame, ~667 of them die in it: 9300 live through it -- eight whole tiles or more; the launches before
    # the ring filled hold fewer)
    assert launches >= 6 and tiles >= 8 * 6, (launches, tiles)


@pytest.mark.parametrize("knob", [{"FW_NT_MB": "0"}, {"FW_NT_WO_MB": "0", "FW_NT_MB": "4096"}], ids=["non-temporal", "write-only non-temporal"])
def test_non_temporal_forms(monkeypatch, knob):
    def scenario(run):
        _start(run)
        run.whole_base = run.system.whole_tiles()
        for k in range(11):
            run.step(_dt(k))
        run.read("end")
        run.totals("end")

    launches, tiles = on_and_off(monkeypatch, _spawner(life_frames=16.0, capacity=CAPACITY), scenario, FW_FUSE_DEPTH="4", **knob, **WIDE)
    assert launches >= 2 and tiles >= 4 * launches, (launches, tiles)  # (5280 or more live, nobody dies: as above)


def test_materialised_new_particles_decline_the_arm(monkeypatch):
    """sparks that emit smoke, both in FIFO rings: the sparks of a frame are materialised in their ring before the update, and only the
    device knows how many children the smoke ring holds.  Neither ring's launch may take the arm -- the counter stays at zero -- and the
    switch changes nothing"""
    sp = _nested_rings(spark_rate=31400.0, per_spark=12.0)
    sp.particle_settings[0].capacity = CAPACITY

    def scenario(run):
        for k in range(40):
            run.step(_dt(k))
            if k % 8 == 7:
                run.read(f"frame {k}")
        run.totals("end")
        assert [run.pair.gpu.update_path(t)[0] for t in (0, 1)] == ["fifo", "fifo"] and run.pair.gpu.count(0) > 12 * TILE

    assert on_and_off(monkeypatch, sp, scenario, **WIDE) == (0, 0)
