"""The boxes of many spawners in one call (include/firework_hip.h: BATCHED BOXES; fw_ctx_aabbs / fw_ctx_aabbs_device; csrc/fw_boxes.h,
fw_k_boxes / fw_k_boxes_fold).  The contract is SAME BOX: record i is what fw_spawner_aabb(handles[i]) answers at the same place in
the stream -- compared as floats, `any` included -- and both are numpy's min / max of position -/+ scale over the particles read back
(the very fp32 subtraction and addition the kernels make: equality, no tolerance).  The sizes sit around the wave (63, 64, 65) and
around the chunk one wave owns (chunk - 1, chunk, chunk + 1, 2 x chunk + 1; the chunk size comes from fw_debug_aabb_batch).  Every
case runs on the four update paths of tests/conftest.py; the two cases about rules of the FIFO ring kernel set their own knobs, as
tests/test_gpu_spin_defer.py and tests/test_gpu_fifo_fuse2.py do, and run once.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from bevy_firework_amd import _ffi
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
FLT_MAX = np.float32(3.40282347e+38)


@pytest.fixture()
def system(fw_path):
    from bevy_firework_amd.system import ParticleSystem

    with ParticleSystem(device=0, seed=SEED) as ps:
        ps.path = fw_path
        yield ps


def _type(life=10.0, **kw):
    base = dict(lifetime=S.RandF32.constant(life), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    base.update(kw)
    return S.ParticleSettings(**base)


def _on_demand(t=0):
    return S.EmissionSettings(particle_index=t, emission_pacing=S.EmissionPacing.OnDemand(), emission_shape=S.EmissionShape.Sphere(0.75),
                              initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.5))


def _rate(rate, t=0):
    return S.EmissionSettings(particle_index=t, emission_pacing=S.EmissionPacing.rate(rate), emission_shape=S.EmissionShape.Sphere(0.75),
                              initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.5))


def _numpy_box(h):
    p = np.concatenate([h.particles(t) for t in range(len(h.settings.particle_settings))])
    if not len(p):
        return False, None, None
    lo, hi = p["position"] - p["scale"][:, None], p["position"] + p["scale"][:, None]
    return True, np.fmin.reduce(lo, axis=0), np.fmax.reduce(hi, axis=0)  # (fminf / fmaxf: a NaN is skipped)


def _check(ps, hs, what=""):
    """the batched call FIRST (it is what has to cope with whatever state the frames left), then the per-spawner call, then numpy"""
    rec = ps.aabb_records(hs)
    any_, mn, mx = ps.aabbs(hs)
    assert (rec["reserved"] == 0).all() and set(np.unique(rec["any"])) <= {0, 1}
    assert np.array_equal(any_, rec["any"] != 0) and np.array_equal(mn, rec["min"]) and np.array_equal(mx, rec["max"])
    seen = {}
    for i, h in enumerate(hs):
        if h.handle not in seen:
            seen[h.handle] = h.aabb() + _numpy_box(h)
        a, lo, hi, na, nlo, nhi = seen[h.handle]
        ctx = (what, i, h.handle, mn[i], lo, nlo, mx[i], hi, nhi)
        assert bool(any_[i]) == a == na, ctx
        assert np.array_equal(mn[i], lo) and np.array_equal(mx[i], hi), ctx  # (as floats: -0 == +0)
        if a:
            assert np.array_equal(mn[i], nlo) and np.array_equal(mx[i], nhi), ctx
        else:  # what the header promises for a spawner without particles
            assert (mn[i] == FLT_MAX).all() and (mx[i] == -FLT_MAX).all(), ctx
    return rec


def _zoo(ps, chunk):
    """on-demand spawners of the sizes around a wave and around a chunk -- long lives: nothing dies inside a test --, one with three
    types whose middle one stays empty, one whose second type receives Nested children (its bound is its capacity), one with nine
    types (fw_spawner_aabb answers it in two passes of eight and one)"""
    sizes = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    hs = []
    for k, n in enumerate(sizes):
        h = ps.spawn(S.ParticleSpawner([_type()], [_on_demand()]), S.Transform((3.0 * k, 1.0, -2.0 * k)), uid=100 + k)
        if n:
            h.queue_particles(n)
        hs.append(h)
    # (what is queued goes to the spawner's first OnDemand entry: the other types are fed by rate emitters)
    three = ps.spawn(S.ParticleSpawner([_type(), _type(), _type()], [_on_demand(0), _rate(6000.0, 2)]), S.Transform((-5.0, 0.0, 4.0)), uid=200)
    three.queue_particles(chunk + 3)
    child = _type(life=2.0, initial_scale=S.RandF32(0.05, 0.1), acceleration=(0.0, 0.5, 0.0))
    nested = ps.spawn(S.ParticleSpawner([_type(life=0.5), child],
                                        [_on_demand(0), S.EmissionSettings(particle_index=1, emission_mode=S.EmissionMode.Nested(0),
                                                                           emission_pacing=S.EmissionPacing.CountOverDuration(20.0, 0.0, 0.0, 0.5),
                                                                           inherit_parent_velocity=False)]), S.Transform((-9.0, 2.0, 0.0)), uid=201)
    nested.queue_particles(65)
    nine = ps.spawn(S.ParticleSpawner([_type() for _ in range(9)], [_on_demand(0), _rate(3000.0, 4), _rate(4200.0, 8)]), S.Transform((7.0, -3.0, 9.0)), uid=202)
    nine.queue_particles(65)
    late = ps.spawn(S.ParticleSpawner([_type(), _type()], [_on_demand(1)]), S.Transform((0.0, 8.0, -6.0)), uid=203)  # (its FIRST type stays empty)
    late.queue_particles(64)
    return hs + [three, nested, nine, late], sizes


def test_sizes_around_the_wave_and_the_chunk(system):
    chunk = system.debug_aabb_batch()[2]
    assert chunk in (512, 1024, 2048)
    hs, sizes = _zoo(system, chunk)
    _check(system, hs, "before the first step")  # (nothing anywhere: every box is the empty one)
    step = 0
    for upto in (1, 2, 5):
        while step < upto:
            system.update(DT)
            step += 1
        rec = _check(system, hs, f"after {upto} steps")
        assert [int(h.counts()[0]) for h in hs[:len(sizes)]] == sizes
        assert list(rec["any"][:len(sizes)]) == [1 if n else 0 for n in sizes]
    three, nested, nine, late = hs[-4:]
    assert list(late.counts()) == [0, 64] and rec["any"][-1] == 1
    c3, c9 = list(three.counts()), list(nine.counts())
    assert c3[0] == chunk + 3 and c3[1] == 0 and c3[2] > 300 and nested.counts()[1] > 0
    assert c9[0] == 65 and c9[4] > 100 and c9[8] > 100 and sum(c9) == c9[0] + c9[4] + c9[8]


def test_order_and_duplicates_follow_the_list(system):
    chunk = system.debug_aabb_batch()[2]
    hs, _ = _zoo(system, chunk)
    for _ in range(2):
        system.update(DT)
    base = _check(system, hs)
    perm = np.random.default_rng(5).permutation(len(hs))
    got = _check(system, [hs[i] for i in perm], "permuted")
    assert got.tobytes() == base[perm].tobytes()  # (the same kernels over the same particles: the same bits, place by place)
    dup = [hs[8], hs[2], hs[8], hs[0], hs[-1], hs[2], hs[8]]
    got = _check(system, dup, "duplicates")
    assert got[0].tobytes() == got[2].tobytes() == got[6].tobytes() == base[8].tobytes() and got[1].tobytes() == got[5].tobytes()
    assert got[3]["any"] == 0 and not np.array_equal(got[0]["min"], got[1]["min"])


def test_ring_heads_that_are_not_slot_zero(system):
    """a FIFO ring that has wrapped and a lifetime-range ring whose particle 0 is not in slot 0 (tests/test_gpu_fifo.py, tests/test_gpu_range.py:
    rings of 4096 slots that turn over every third of a second), next to a small emitter; on the other paths the same types are
    compacting segments or small types"""
    ring = S.ParticleSettings(lifetime=S.RandF32.constant(0.25), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, capacity=4096,
                              scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    rng = S.ParticleSettings(lifetime=S.RandF32(0.2, 0.5), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, capacity=8192,
                             scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    hs = [system.spawn(S.ParticleSpawner([ring], [_rate(11000.0)]), S.Transform((1.0, 2.0, 3.0)), uid=3),
          system.spawn(S.ParticleSpawner([rng], [_rate(9000.0)]), S.Transform((-4.0, 0.0, 1.0)), uid=4),
          system.spawn(S.ParticleSpawner([_type(life=0.4)], [_rate(700.0)]), S.Transform((0.0, 5.0, 0.0)), uid=5)]
    for fr in range(60):  # (one second: the FIFO head has gone round the 4096 slots more than twice)
        system.update(DT)
        if fr in (20, 41, 59):
            _check(system, hs, f"frame {fr}")
    assert hs[0].counts()[0] > 2000
    if system.path == "fifo":
        assert hs[0].update_path(0)[0] == "fifo"
    if system.path == "range":
        assert hs[1].update_path(0)[0] == "range"


def _device_buffer(ps, n):
    import torch

    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        return torch.full(((n + 2) * 32,), 0xAB, dtype=torch.uint8, device="cuda")


def test_device_form_behind_a_step_without_a_wait(system):
    chunk = system.debug_aabb_batch()[2]
    hs, _ = _zoo(system, chunk)
    buf = _device_buffer(system, len(hs))
    for k in range(3):
        system.update(DT)
        system.aabbs_device(hs, buf.data_ptr() + 32)  # (enqueued right behind fw_step: nothing waits in between)
        host = system.aabb_records(hs)
        system.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[:32] == 0xAB).all() and (raw[-32:] == 0xAB).all(), "a guard record was written"
        dev = raw[32:-32].view(S.AABB_DTYPE)
        assert (dev["reserved"] == 0).all() and np.array_equal(dev["any"], host["any"])
        assert np.array_equal(dev["min"], host["min"]) and np.array_equal(dev["max"], host["max"])  # (as floats: -0 == +0)
        same = (dev.view(np.uint32) == host.view(np.uint32))
        zeros = (dev.view(np.float32) == 0.0) & (host.view(np.float32) == 0.0)
        assert (same | zeros).all(), "the two forms differ in more than the sign of a zero"
        _check(system, hs, f"frame {k}")


def _fifo_knobs(monkeypatch, **env):
    """the FIFO ring rules forced at small sizes, whatever the path matrix dealt this test (tests/test_gpu_spin_defer.py: both)"""
    for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB", "FW_SPINLESS", "FW_SPIN_DEFER",
              "FW_SPIN_DEFER_MIN", "FW_SPIN_DEFER_AFTER", "FW_FUSE2_MIN", "FW_FIFO_SMALL", "FW_FUSE2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0"), ("FW_FIFO_SMALL", "1"),
                 ("FW_SPIN_DEFER", "1"), ("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", "2")) + tuple(env.items()):
        monkeypatch.setenv(k, v)


def test_stale_ages_are_written_back_and_the_spin_stays_deferred(fw_path, monkeypatch):
    if fw_path != "fifo":
        pytest.skip("the age rule and the deferred spin belong to the FIFO ring kernel: one run, under the path matrix's fifo entry")
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    _fifo_knobs(monkeypatch, FW_FUSE2="0")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(), S.Transform((1.0, 2.0, 3.0)), uid=19)
        for _ in range(9):
            ps.update(DT)
        flagged = h.update_path(0)
        assert flagged[0] == "fifo"
        ages, spins = ps.age_launches(), ps.spin_launches()
        first = ps.aabb_records([h, h])  # first thing after the unread frames: the ages in memory are nine frames old
        assert ps.age_launches() == ages + 1 and ps.spin_launches() == spins
        a, lo, hi = h.aabb()
        assert a and first["any"][0] == 1 and np.array_equal(first["min"][0], lo) and np.array_equal(first["max"][0], hi)
        assert first[0].tobytes() == first[1].tobytes() and (lo < hi).all()
        for k in range(3):  # ... and a host that asks every frame keeps the rule: the spin is still deferred, the ring in its mode
            ps.update(DT)
            assert h.update_path(0) == flagged
            ps.aabbs([h])
            assert ps.spin_launches() == spins
        any_, mn, mx = ps.aabbs([h])
        a, lo, hi = h.aabb()
        assert ps.spin_launches() == spins
        na, nlo, nhi = _numpy_box(h)  # (reads the particles: the one call here that replays the spin)
        assert ps.spin_launches() == spins + 1
        assert list(any_) == [True] and a and na
        assert np.array_equal(mn[0], lo) and np.array_equal(mx[0], hi) and np.array_equal(mn[0], nlo) and np.array_equal(mx[0], nhi)


def _fused_run(monkeypatch, ask):
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    _fifo_knobs(monkeypatch, FW_FUSE2="1", FW_FUSE2_MIN="1")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(life_frames=16.0, capacity=16384), S.Transform((1.0, 2.0, 3.0)), uid=22)
        for _ in range(8):
            ps.update(DT)
        ps.synchronize()
        for _ in range(3):  # (withheld, fused, withheld: tests/test_gpu_fifo_fuse2.py)
            ps.update(DT)
        fused, flushed = ps.fuse2_launches()
        box = None
        if ask:
            any_, mn, mx = ps.aabbs([h])
            assert ps.fuse2_launches() == (fused, flushed + 1), "the withheld frame goes to the stream once, in front of the boxes"
            box = (bool(any_[0]), mn[0], mx[0])
            ps.aabbs([h, h])
            assert ps.fuse2_launches() == (fused, flushed + 1)
        for _ in range(4):
            ps.update(DT)
        return fused, box, h.particles(0)


def test_a_withheld_group_is_flushed_once_and_the_particles_are_the_same(fw_path, monkeypatch):
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    fused, box, asked = _fused_run(monkeypatch, True)
    assert fused >= 1
    _, _, never = _fused_run(monkeypatch, False)
    assert len(asked) > 4000 and asked.tobytes() == never.tobytes()
    # the boxes after the 11 frames: a context that fuses nothing, read back in full
    _fifo_knobs(monkeypatch, FW_FUSE2="0")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(life_frames=16.0, capacity=16384), S.Transform((1.0, 2.0, 3.0)), uid=22)
        for _ in range(11):
            ps.update(DT)
        na, nlo, nhi = _numpy_box(h)
    assert box[0] and na and np.array_equal(box[1], nlo) and np.array_equal(box[2], nhi)


def test_scratch_grows_and_shrinking_calls_stay_right(system):
    chunk = system.debug_aabb_batch()[2]
    hs, _ = _zoo(system, chunk)
    system.update(DT)
    system.update(DT)
    _check(system, [hs[2], hs[5]], "two")
    assert system.debug_aabb_batch()[1] >= 1
    _check(system, hs, "all")
    big = system.debug_aabb_batch()[1]
    _check(system, [hs[8], hs[1]], "two again")
    assert 3 <= system.debug_aabb_batch()[1] < big
    _check(system, hs + hs, "twice all")
    assert system.debug_aabb_batch()[1] == 2 * big


def test_two_launches_per_call_whatever_n(system):
    chunk = system.debug_aabb_batch()[2]
    hs, sizes = _zoo(system, chunk)
    sparks = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=300)
    sparks.queue_particles(733)
    system.update(DT)
    n0 = system.debug_aabb_batch()[0]
    system.aabb_records([sparks])
    n1, chunks, _ = system.debug_aabb_batch()
    assert n1 == n0 + 2
    assert -(-733 // chunk) <= chunks < 256, "a 733-particle emitter occupies waves, not a 256-workgroup grid"
    system.aabb_records(hs + [sparks])
    n2, chunks, _ = system.debug_aabb_batch()
    assert n2 == n1 + 2 and chunks >= sum(-(-n // chunk) for n in sizes)
    buf = _device_buffer(system, len(hs))
    system.aabbs_device(hs, buf.data_ptr() + 32)
    assert system.debug_aabb_batch()[0] == n2 + 2
    system.synchronize()


def test_nan_positions_are_skipped_and_a_negative_zero_is_a_zero(system):
    h = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), S.Transform((20.0, 30.0, 40.0)), uid=7)
    other = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), S.Transform((-3.0, 0.0, 0.0)), uid=8)
    h.queue_particles(70), other.queue_particles(5)
    system.update(DT)
    p = h.particles(0).copy()
    assert len(p) == 70 and (p["position"] - p["scale"][:, None]).min() > 1.0
    p["position"][3] = np.nan
    p["position"][66] = (np.float32(-0.0), np.float32(-0.0), np.float32(-0.0))
    p["scale"][66] = p["initial_scale"][66] = 0.0  # position - scale == -0.0, position + scale == +0.0: the box's min
    h.write_particles(0, p)
    rec = _check(system, [other, h], "written")
    assert rec["any"][1] == 1 and (rec["min"][1] == 0.0).all() and np.isfinite(rec["max"][1]).all()
    system.update(DT)
    rec = _check(system, [h, other], "one step later")
    assert np.isfinite(rec["min"][0]).all() and np.isfinite(rec["max"][0]).all()


def test_tile_boxes_do_not_change_the_answer(system):
    big, tf = workloads.stress_test(rate=40000.0)
    hs = [system.spawn(big, tf, uid=1), system.spawn(S.ParticleSpawner([_type(life=0.4)], [_rate(300.0)]), S.Transform((5.0, 0.0, 1.0)), uid=3),
          system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=4)]
    system.track_aabbs(True)
    for fr in range(12):
        system.update(DT)
        if fr % 4 == 3:
            on = system.aabb_records(hs)
            _check(system, hs, f"tracking, frame {fr}")
            system.track_aabbs(False)
            off = system.aabb_records(hs)
            system.track_aabbs(True)
            assert on.tobytes() == off.tobytes()


def test_errors_write_nothing_and_enqueue_nothing(system):
    hs = [system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=10 + k) for k in range(4)]
    gone = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=20)
    hs[1].queue_particles(9)
    system.update(DT)
    system.despawn(gone)
    L, ctx = system._lib, system._ctx
    out = np.zeros(4, dtype=S.AABB_DTYPE)
    out.view(np.uint8)[:] = 0xCD
    poison = out.tobytes()
    optr = out.ctypes.data_as(C.c_void_p)
    buf = _device_buffer(system, 4)
    dptr = C.c_void_p(buf.data_ptr() + 32)
    system.synchronize()
    launches = system.debug_aabb_batch()[0]

    def arr(*v):
        return (C.c_int32 * len(v))(*v)

    good = arr(*[h.handle for h in hs])
    assert L.fw_ctx_aabbs(None, 4, good, optr) == _ffi.FW_EINVAL and L.fw_ctx_aabbs_device(None, 4, good, dptr) == _ffi.FW_EINVAL
    for form, dst in ((L.fw_ctx_aabbs, optr), (L.fw_ctx_aabbs_device, dptr)):
        assert form(ctx, 4, None, dst) == _ffi.FW_EINVAL
        assert form(ctx, 4, good, None) == _ffi.FW_EINVAL
        for bad in (-1, 1 << 20, gone.handle):
            for at in (0, 2, 3):  # (first, in the middle of a valid list, last)
                v = [h.handle for h in hs]
                v[at] = bad
                assert form(ctx, 4, arr(*v), dst) == _ffi.FW_EINVAL, (bad, at)
                assert b"invalid spawner handle" in L.fw_last_error(ctx) and L.fw_last_error(ctx).startswith(b"fw_ctx_aabbs")
        assert form(ctx, 0, None, None) == _ffi.FW_OK and form(ctx, 0, good, dst) == _ffi.FW_OK
    assert L.fw_ctx_aabbs_device(ctx, 4, good, C.c_void_p(buf.data_ptr() + 36)) == _ffi.FW_EINVAL  # (not 16-byte aligned)
    system.synchronize()
    assert out.tobytes() == poison and (buf.cpu().numpy() == 0xAB).all()
    assert system.debug_aabb_batch()[0] == launches
    # ... and the same arguments with every handle valid are answered
    assert L.fw_ctx_aabbs(ctx, 4, good, optr) == _ffi.FW_OK and list(out["any"]) == [0, 1, 0, 0]
    _check(system, hs)
