"""Round 11: the in-place update tests every component plane of the angular velocity by itself and stores only the ones a wave
changed (fw_integrate_store<INPLACE>, fw_dev.h).  A component that is skipped when it should have been written shows as stale bits
in the slot, so every case here compares the ANGULAR VELOCITY BIT FOR BIT (sign of zero included) with the C oracle, frame by frame,
and the rotation -- which is integrated from it -- under the rule of tests/parity.py.  The path matrix of tests/conftest.py runs each
case on FIFO rings and on range rings (and on the compacting kernels, which write everything: the same expectations).
Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair, assert_particles_match

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
Y = (0.0, 1.0, 0.0)


@pytest.fixture()
def system(fw_path):
    from bevy_firework_amd.system import ParticleSystem

    with ParticleSystem(device=0, seed=SEED) as ps:
        ps.path = fw_path
        yield ps


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: {g.shape} != {w.shape}"
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} differ in their bits, indices {i}..{int(bad[-1])}; "
                             f"first: got {np.asarray(got)[i]!r} want {np.asarray(want)[i]!r}")


def _match(gpu, cpu, what):
    """one list of particles (live or destroyed) against the oracle's: angular velocity bit for bit, the rest under parity.py"""
    assert_particles_match(gpu, cpu, False, what)
    _same_bits(gpu["angular_velocity"], cpu["angular_velocity"], f"{what}: angular_velocity")


def _check(pair, what):
    assert pair.gpu.counts() == pair.cpu.counts(), f"{what}: counts {pair.gpu.counts()} != {pair.cpu.counts()}"
    for t in range(pair.n_types):
        _match(pair.gpu.particles(t), pair.cpu.particles(t), f"{what} type {t} [path {pair.gpu.update_path(t)}]")


def _expect_ring(system, pair, t=0):
    if system.path in ("fifo", "range"):
        assert pair.gpu.update_path(t)[0] == system.path, (pair.gpu.update_path(t), system.path)


def _spinner(**kw):
    base = dict(lifetime=S.RandF32.constant(0.4), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, angular_drag=0.2, capacity=16384)
    base.update(kw)
    return S.ParticleSettings(**base)


def _entry(axis=Y, spread=0.0, rate=24000.0, mag=(1.0, 9.0), **kw):
    return S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(rate),
                              initial_velocity=S.RandVec3(S.RandF32(1.0, 5.0), Y, 0.0),
                              initial_angular_velocity=S.RandVec3(S.RandF32(*mag), axis, spread), **kw)


def _run(system, pair, frames, what):
    for fr in range(frames):
        system.update(DT)
        pair.step_cpu(DT)
        _check(pair, f"{what}, frame {fr}")


def test_fixed_axis_spin(system):
    """(a) the headline workload's shape: direction (0,1,0), spread 0, no angular acceleration -- x and z of the angular velocity
    and of the rotation stay +0 for a particle's whole life; y decays under the drag and must be written every frame"""
    pair = Pair(system, S.ParticleSpawner([_spinner()], [_entry()]), S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=41)
    _expect_ring(system, pair)
    _run(system, pair, 60, "fixed axis")
    g = pair.gpu.particles(0)
    assert len(g) > 8000
    assert not _bits(g["angular_velocity"])[:, (0, 2)].any() and _bits(g["angular_velocity"])[:, 1].all()
    assert not _bits(g["rotation"])[:, (0, 2)].any()


@pytest.mark.parametrize("axis", [(0.0, -1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -0.6, 0.8), (-0.6, 0.0, -0.8)],
                         ids=["-y", "-x", "-y+z", "-x-z"])
def test_negative_axes_and_negative_zero(system, axis):
    """(b) a direction with negative components: magnitude * -0.0... the spawn value of a component the axis does not have may be a
    zero of either sign, and the first update turns a -0 into +0 (w + (0 - drag * w) * dt): that one change must reach the slot"""
    pair = Pair(system, S.ParticleSpawner([_spinner()], [_entry(axis=axis)]), seed=SEED, uid=42)
    _expect_ring(system, pair)
    _run(system, pair, 45, f"axis {axis}")
    assert pair.gpu.count(0) > 8000


def test_component_starts_constant_and_then_moves(system):
    """(c) no initial spin, an angular acceleration along x: x moves from the first update on, y and z stay zero"""
    ps = _spinner(angular_acceleration=(0.7, 0.0, 0.0))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(24000.0), initial_velocity=S.RandVec3(S.RandF32(1.0, 5.0), Y, 0.0))
    pair = Pair(system, S.ParticleSpawner([ps], [es]), seed=SEED, uid=43)
    _expect_ring(system, pair)
    _run(system, pair, 45, "angular acceleration along x")
    g = pair.gpu.particles(0)
    assert len(g) > 8000 and _bits(g["angular_velocity"])[:, 0].all() and not _bits(g["angular_velocity"])[:, 1:].any()


def test_waves_mix_lanes_that_change_a_component_with_lanes_that_do_not(system):
    """(d) two entries feed one type, one with a fixed axis and one with a cone around another: within a wave some lanes change x / z
    and some do not -- the test is per wave, the store per lane's own value.
    The particles of the fixed-axis entry are compared bit for bit like everywhere in this file.  The cone entry's are not: their
    INITIAL angular velocity comes out of sincosf, the device's and the oracle's libm differ in the last bit there (tests/parity.py,
    DESIGN.md 5), and w + (acc - drag * w) * dt carries that bit along -- no build of the library, the parent's included, can match
    them bit for bit.  They are held to the rule of tests/parity.py in every frame, which a stale component cannot pass: a plane that
    was not written keeps the previous frame's value, off by drag * dt = 3e-3 of it against an allowance of 1e-5."""
    es = [_entry(rate=13000.0), _entry(axis=(0.6, 0.0, 0.8), spread=0.5, rate=11000.0, emission_shape=S.EmissionShape.Sphere(0.5))]
    pair = Pair(system, S.ParticleSpawner([_spinner()], es), seed=SEED, uid=45)
    _expect_ring(system, pair)
    for fr in range(50):
        system.update(DT)
        pair.step_cpu(DT)
        assert pair.gpu.counts() == pair.cpu.counts(), fr
        g, c = pair.gpu.particles(0), pair.cpu.particles(0)
        assert_particles_match(g, c, False, f"fixed axis + cone, frame {fr}")
        fixed = ~_bits(c["angular_velocity"])[:, (0, 2)].any(axis=1)  # (the oracle's particles of the first entry: x and z are +0)
        assert fixed.any() and not fixed.all()
        _same_bits(g["angular_velocity"][fixed], c["angular_velocity"][fixed], f"frame {fr}: angular_velocity of the fixed-axis entry")
    assert pair.gpu.count(0) > 8000


def test_recycled_slots_take_the_new_particles_bits(system):
    """(e) a small ring that wraps every ~0.3 s, fed by an entry that spins about y and one that spins about x: a recycled slot holds
    an old particle's x / y / z, and the new particle's first update must overwrite all three whatever the wave's other lanes do"""
    ps = _spinner(lifetime=S.RandF32.constant(0.25), capacity=4096)
    es = [_entry(rate=6000.0), _entry(axis=(1.0, 0.0, 0.0), rate=5000.0)]
    pair = Pair(system, S.ParticleSpawner([ps], es), S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=46)
    _expect_ring(system, pair)
    _run(system, pair, 200, "wrapping ring")
    assert 2500 < pair.gpu.count(0) < 3000
    _expect_ring(system, pair)


def test_fifo_ring_becomes_a_range_ring_with_spinning_particles(fw_path, monkeypatch):
    """(f) a ninth large one-lifetime type moves the eight FIFO rings of a context to range rings where they stand (fifo_to_range):
    rotation and angular velocity are the same bits before and after, and the oracle's in the frames that follow"""
    from bevy_firework_amd.system import ParticleSystem

    if fw_path != "fifo":
        pytest.skip("a conversion of FIFO rings")
    monkeypatch.setenv("FW_RANGE", "1"), monkeypatch.setenv("FW_RANGE_MIN", "0")
    with ParticleSystem(device=0, seed=SEED) as system:
        pairs = []

        def add(k):
            ps = _spinner(lifetime=S.RandF32.constant(0.3 + 0.02 * k), capacity=0)
            axis = [Y, (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.6, 0.8)][k % 4]
            pairs.append(Pair(system, S.ParticleSpawner([ps], [_entry(axis=axis, rate=4000.0 + 500.0 * k)]), S.Transform((float(k), 0.0, 0.0)),
                              seed=SEED, uid=400 + k))

        def run(n, what):
            for fr in range(n):
                system.update(DT)
                for k, p in enumerate(pairs):
                    p.step_cpu(DT)
                    _check(p, f"{what}, frame {fr} spawner {k}")

        for k in range(8):
            add(k)
        assert [p.gpu.update_path(0)[0] for p in pairs] == ["fifo"] * 8
        run(27, "eight FIFO rings")
        before = [p.gpu.particles(0) for p in pairs[:8]]
        add(8)
        assert [p.gpu.update_path(0)[0] for p in pairs] == ["range"] * 9
        for k, (p, b) in enumerate(zip(pairs, before)):
            after = p.gpu.particles(0)
            for f in ("rotation", "angular_velocity", "position", "velocity", "age", "lifetime"):
                _same_bits(after[f], b[f], f"fifo_to_range, spawner {k}: {f}")
        run(30, "nine range rings")
        assert all(p.gpu.count(0) > 1000 for p in pairs)


def test_fifo_ring_becomes_a_compacting_segment_with_spinning_particles(system):
    """(f) fw_spawner_write_particles ends the ring mode (fifo_to_general; a range ring leaves the same way): what the caller wrote is
    what the segment holds -- rotation and angular velocity bit for bit -- and the oracle's state from there on"""
    pair = Pair(system, S.ParticleSpawner([_spinner(capacity=8192)], [_entry(rate=18000.0)]), seed=SEED, uid=47)
    _run(system, pair, 30, "before write")
    _expect_ring(system, pair)
    parts = pair.gpu.particles(0)[::2].copy()
    parts["lifetime"] = np.linspace(0.05, 0.6, len(parts)).astype(np.float32)  # no longer one lifetime
    pair.gpu.write_particles(0, parts)
    pair.cpu.write_particles(0, parts)
    assert pair.gpu.update_path(0)[0] in ("general", "small")
    back = pair.gpu.particles(0)
    for f in ("rotation", "angular_velocity"):
        _same_bits(back[f], parts[f], f"read back after write_particles: {f}")
    _run(system, pair, 40, "after write")
    assert pair.gpu.count(0) > 3000


@pytest.mark.parametrize("windowed", [False, True], ids=["plain attach", "windowed attach"])
def test_readers_of_a_spinning_ring_type(system, windowed):
    """(g) everything that reads a ring's rotation and angular velocity: particles(), the instance records the update writes into an
    attached buffer (plain and windowed) and the packing pass, and the destroyed records -- on a ring that wraps"""
    import torch

    ps = _spinner(lifetime=S.RandF32.constant(0.2), capacity=4096, particles_destroyed=lambda dead: None)
    pair = Pair(system, S.ParticleSpawner([ps], [_entry(rate=17000.0)]), seed=SEED, uid=48)
    _expect_ring(system, pair)
    path = pair.gpu.update_path(0)[0]
    cap, guard = 8192, 64
    buf = torch.full(((cap + guard) * 16,), float("nan"), dtype=torch.float32, device="cuda")
    (pair.gpu.attach_instances_window if windowed else pair.gpu.attach_instances)(buf.data_ptr(), cap)
    for fr in range(100):
        system.update(DT)
        pair.step_cpu(DT)
        _check(pair, f"frame {fr}")
        _match(pair.gpu.destroyed(0), pair.cpu.destroyed(0), f"destroyed, frame {fr}")
        n = pair.gpu.count(0)
        first = pair.gpu.instance_window(0)[0] if windowed else 0
        if windowed:
            assert first == (len(pair.cpu.destroyed(0)) if path == "range" else 0), (fr, first, path)
        ref = pair.gpu.instances(0)  # packing pass
        got = buf[first * 16: (first + n) * 16].cpu().numpy().view(np.uint32).reshape(n, 16)
        assert np.array_equal(got, ref.view(np.uint32).reshape(n, 16)), f"frame {fr}: attached records differ from packed ones"
        _same_bits(got.view(np.float32)[:, 4:8], pair.gpu.particles(0)["rotation"], f"frame {fr}: rotation of the records")
        assert bool(torch.isnan(buf[cap * 16:]).all()), "wrote past the attached buffer"
    assert 3000 < pair.gpu.count(0) < 4000
