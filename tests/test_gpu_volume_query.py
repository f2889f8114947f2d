"""How many particles lie inside analytic volumes (include/firework_hip.h: VOLUME QUERIES; fw_ctx_count_in_volumes[_device];
csrc/fw_volumes.h, fw_k_volumes / fw_k_volumes_fold).  The answers are integers and the contract is exact: counts[p, v] equals the number
of particles of places[p] -- read back AFTER the query -- for which tests/project_ref.py's inside answer holds against volumes[v]
(tests/volume_ref.py).  The spawners are those of tests/test_gpu_aabb_batch.py: sizes around the wave (63, 64, 65) and around the chunk
one wave owns (chunk - 1, chunk, chunk + 1, 2 x chunk + 1; the chunk size comes from fw_debug_volume_query); the volume counts sit
around the tile of 64 (1, 63, 64, 65, 129).  Every case runs on the four update paths of tests/conftest.py; the two cases about rules of
the FIFO ring kernel set their own knobs and run once.  Needs an MI355X.

Builds altered on purpose (not committed) and what each turns red:
  a chunk that stops one position early (fw_k_volumes: `li < end - 1`)      every case that holds a particle: the half-space that holds
                                                                            everything no longer equals counts()
  a fold that skips a place's last chunk (fw_k_volumes_fold: `c < P.c1 - 1`) the same cases; sizes <= chunk count 0
  volume tile 64 treated as 63 (the tile loop steps by 63)                  the cases with 64, 65 and 129 volumes: volume 63 onwards is
                                                                            answered with its neighbour's count or not at all"""
import ctypes as C

import numpy as np
import pytest

import volume_ref
from test_gpu_aabb_batch import _fifo_knobs, _on_demand, _rate, _type, _zoo

from bevy_firework_amd import _ffi
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
KINDS = (S.COLLIDER_PLANE, S.COLLIDER_SPHERE, S.COLLIDER_BOX, S.COLLIDER_CYLINDER, S.COLLIDER_CONE, S.COLLIDER_CAPSULE)
EVERYTHING, NOTHING = 1, 2  # (places in _volumes' list)


@pytest.fixture()
def system(fw_path):
    from bevy_firework_amd.system import ParticleSystem

    with ParticleSystem(device=0, seed=SEED) as ps:
        ps.path = fw_path
        yield ps


def _quat(x, y, z, w):
    q = np.array([x, y, z, w], dtype=np.float64)
    return tuple(float(c) for c in (q / np.linalg.norm(q)).astype(np.float32))


ROT = _quat(0.3, 0.5, -0.2, 0.78)


def _volumes(n, centres):
    """n volumes: a sphere that cuts the first centre's cloud, a half-space that holds everything, a sphere that holds nothing, then
    every kind, unrotated and rotated, cutting that cloud (the emitters fill a ball of radius 0.75 around their transform and rise); from
    the fifteenth on the same shapes at the other centres, in other sizes"""
    out = []
    rng = np.random.default_rng(29)
    k = 0
    while len(out) < n:
        c = tuple(float(x) for x in centres[k % len(centres)])
        s = 1.0 if k == 0 else float(rng.uniform(0.5, 1.6))
        up = (c[0], c[1] + 0.3, c[2])
        out += [S.Collider.Sphere(up, 0.6 * s),
                S.Collider.Plane((0.0, 1000.0, 0.0), (0.0, 1.0, 0.0)),
                S.Collider.Sphere((1000.0, 1000.0, 1000.0), 1.0),
                S.Collider.Plane(up, (0.0, 1.0, 0.0)), S.Collider.Plane(up, (0.6, -0.5, 0.3)),
                S.Collider.Sphere((c[0] + 0.4, c[1], c[2] - 0.2), 0.5 * s),
                S.Collider.Box(up, (0.5 * s, 0.6 * s, 0.4 * s)), S.Collider.Box(up, (0.5 * s, 0.6 * s, 0.4 * s), ROT),
                S.Collider.Cylinder(up, 0.6 * s, 1.0 * s), S.Collider.Cylinder(up, 0.6 * s, 1.0 * s, ROT),
                S.Collider.Cone(up, 0.8 * s, 1.5 * s), S.Collider.Cone(up, 0.8 * s, 1.5 * s, ROT),
                S.Collider.Capsule(up, 0.4 * s, 0.8 * s), S.Collider.Capsule(up, 0.4 * s, 0.8 * s, ROT)]
        k += 1
    return out[:n]


def _centres(hs):
    """the transforms of the spawners, the largest plain one first"""
    return [hs[8].transform.translation] + [h.transform.translation for h in hs]


def _check(ps, places, volumes, what=""):
    """the query FIRST (it is what has to cope with whatever state the frames left), then the particles read back and numpy"""
    got = ps.count_in_volumes(places, volumes)
    assert got.dtype == np.uint32 and got.shape == (len(places), len(volumes))
    want = volume_ref.counts(places, volumes)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, [(int(p), int(v), int(got[p, v]), int(want[p, v]), volumes[v].kind) for p, v in bad[:8]])
    return got, want


def test_sizes_around_the_wave_and_the_chunk_volumes_around_the_tile(system):
    launches, _, chunk, tile = system.debug_volume_query()
    assert chunk in (512, 1024, 2048) and tile == 64 and launches == 0
    hs, sizes = _zoo(system, chunk)
    vols = _volumes(129, _centres(hs))
    got, _ = _check(system, hs, vols[:14], "before the first step")
    assert not got.any()
    step = 0
    for upto, counts in ((1, (14,)), (2, (1, 63)), (5, (64, 65, 129))):
        while step < upto:
            system.update(DT)
            step += 1
        for n in counts:
            got, want = _check(system, hs, vols[:n], f"after {upto} steps, {n} volumes")
            if n > NOTHING:
                totals = [int(sum(h.counts())) for h in hs]
                assert list(got[:, EVERYTHING]) == totals and totals[:len(sizes)] == sizes and not got[:, NOTHING].any()
            if n >= 14:  # on the reference: every kind cuts the largest plain spawner's cloud
                for kind in KINDS:
                    cut = [v for v in range(n) if vols[v].kind == kind and 0 < want[8, v] < sizes[8]]
                    assert cut, kind
                    assert any(tuple(vols[v].rotation) != S.QUAT_IDENTITY for v in cut) or kind in (S.COLLIDER_PLANE, S.COLLIDER_SPHERE), kind


def test_one_type_every_type_an_empty_middle_type_nested_children_nine_types(system):
    chunk = system.debug_volume_query()[2]
    hs, _ = _zoo(system, chunk)
    three, nested, nine, late = hs[-4:]
    vols = _volumes(14, [h.transform.translation for h in (three, nested, nine, late)]) + _volumes(14, [nested.transform.translation])
    for _ in range(5):
        system.update(DT)
    places = []
    for h in (three, nested, nine, late):
        places += [(h, -1)] + [(h, t) for t in range(len(h.settings.particle_settings))]
    got, want = _check(system, places, vols)
    at = 0
    for h in (three, nested, nine, late):
        nt = len(h.settings.particle_settings)
        assert np.array_equal(got[at], got[at + 1:at + 1 + nt].sum(axis=0, dtype=np.uint32)), h.handle
        assert list(got[at + 1:at + 1 + nt, EVERYTHING]) == [int(c) for c in h.counts()]
        at += 1 + nt
    assert got[2, EVERYTHING] == 0 and got[1, EVERYTHING] == chunk + 3 and got[3, EVERYTHING] > 300  # (three: its middle type is empty)
    assert nested.counts()[1] > 0 and got[6].any() and (want[6] < nested.counts()[1]).any()      # (nested's children: cut by some volume)
    assert got[7 + 1 + 4, EVERYTHING] > 100 and got[7 + 1 + 8, EVERYTHING] > 100


def test_order_and_duplicates_follow_the_list(system):
    chunk = system.debug_volume_query()[2]
    hs, _ = _zoo(system, chunk)
    vols = _volumes(65, _centres(hs))
    for _ in range(2):
        system.update(DT)
    places = [(h, -1) for h in hs] + [(hs[-2], 4), (hs[-4], 2)]
    base, _ = _check(system, places, vols)
    perm = np.random.default_rng(5).permutation(len(places))
    got, _ = _check(system, [places[i] for i in perm], vols, "permuted")
    assert got.tobytes() == base[perm].tobytes()
    dup = [places[8], places[2], places[8], places[0], places[-1], places[2], places[8]]
    got, _ = _check(system, dup, vols, "duplicates")
    assert got[0].tobytes() == got[2].tobytes() == got[6].tobytes() == base[8].tobytes() and got[1].tobytes() == got[5].tobytes() == base[2].tobytes()
    assert not got[3].any() and got[4].tobytes() == base[-1].tobytes() and got[0].tobytes() != got[1].tobytes()
    # ... and the volumes permuted: the same counts, column by column
    vperm = np.random.default_rng(6).permutation(len(vols))
    got, _ = _check(system, places, [vols[i] for i in vperm], "volumes permuted")
    assert np.array_equal(got, base[:, vperm])


def test_ring_heads_that_are_not_slot_zero(system):
    """a FIFO ring that has wrapped and a lifetime-range ring whose particle 0 is not in slot 0 (tests/test_gpu_aabb_batch.py), next to a
    small emitter; on the other paths the same types are compacting segments or small types"""
    ring = S.ParticleSettings(lifetime=S.RandF32.constant(0.25), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, capacity=4096,
                              scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    rng = S.ParticleSettings(lifetime=S.RandF32(0.2, 0.5), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, capacity=8192,
                             scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    hs = [system.spawn(S.ParticleSpawner([ring], [_rate(11000.0)]), S.Transform((1.0, 2.0, 3.0)), uid=3),
          system.spawn(S.ParticleSpawner([rng], [_rate(9000.0)]), S.Transform((-4.0, 0.0, 1.0)), uid=4),
          system.spawn(S.ParticleSpawner([_type(life=0.4)], [_rate(700.0)]), S.Transform((0.0, 5.0, 0.0)), uid=5)]
    vols = _volumes(28, [h.transform.translation for h in hs])
    for fr in range(60):  # (one second: the FIFO head has gone round the 4096 slots more than twice)
        system.update(DT)
        if fr in (20, 41, 59):
            got, want = _check(system, [(hs[0], 0), (hs[1], -1), hs[2]], vols, f"frame {fr}")
            assert list(got[:, EVERYTHING]) == [int(h.counts()[0]) for h in hs]
            assert ((want[0] > 0) & (want[0] < want[0, EVERYTHING])).sum() >= 3 and ((want[1] > 0) & (want[1] < want[1, EVERYTHING])).sum() >= 3
    assert hs[0].counts()[0] > 2000
    if system.path == "fifo":
        assert hs[0].update_path(0)[0] == "fifo"
    if system.path == "range":
        assert hs[1].update_path(0)[0] == "range"


def test_particles_on_a_boundary_one_ulp_outside_and_nan(system):
    """positions written with write_particles: ON the boundary of every kind (inside, by <= 0 -- the half-space alone is strict), the
    next float outside, and NaN (inside nothing)"""
    f = np.float32
    h = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), S.Transform((0.0, 0.0, 0.0)), uid=7)
    other = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), S.Transform((-300.0, 0.0, 0.0)), uid=8)
    h.queue_particles(70), other.queue_particles(5)
    system.update(DT)
    p = h.particles(0).copy()
    assert len(p) == 70
    p["position"] = np.array([100.0, 100.0, 100.0], dtype=f) + np.arange(70, dtype=f)[:, None]
    up = lambda x: np.nextafter(f(x), f(np.inf))  # noqa: E731
    pts = [(1.0, 0.0, 0.0), (up(1.0), 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (np.nan, np.nan, np.nan),   # sphere r 1 at the origin
           (10.5, 0.25, -0.5), (up(10.5), 0.25, -0.5), (10.5, 0.25, -up(0.5)),                                       # box at (10, 0, 0), half 0.5
           (0.0, -50.0, 0.0), (0.0, -up(50.0), 0.0), (3.0, np.nextafter(f(-50.0), f(0.0)), 0.0),                      # half-space y < -50, strict
           (20.0, 1.0, 0.0), (20.0, up(1.0), 0.0), (20.5, 0.25, 0.0), (up(20.5), 0.25, 0.0),                          # capsule at (20, 0, 0): r 0.5, segment 1
           (30.5, 0.5, 0.0), (30.5, up(0.5), 0.0), (up(30.5), 0.5, 0.0),                                              # cylinder at (30, 0, 0): r 0.5, height 1
           (40.0, 0.5, 0.0), (40.0, up(0.5), 0.0), (40.5, -0.5, 0.0), (40.5, -up(0.5), 0.0), (up(40.5), -0.5, 0.0)]   # cone at (40, 0, 0): r 0.5, height 1
    p["position"][:len(pts)] = np.array(pts, dtype=f)
    h.write_particles(0, p)
    vols = [S.Collider.Sphere((0.0, 0.0, 0.0), 1.0), S.Collider.Box((10.0, 0.0, 0.0), (0.5, 0.5, 0.5)), S.Collider.Plane((0.0, -50.0, 0.0), (0.0, 1.0, 0.0)),
            S.Collider.Capsule((20.0, 0.0, 0.0), 0.5, 1.0), S.Collider.Cylinder((30.0, 0.0, 0.0), 0.5, 1.0), S.Collider.Cone((40.0, 0.0, 0.0), 0.5, 1.0),
            S.Collider.Plane((0.0, 1e6, 0.0), (0.0, 1.0, 0.0))]
    got, want = _check(system, [other, h], vols, "written")
    # the reference's own answers, spelled out: one point on each boundary counts, its neighbours do not, a NaN is in nothing
    assert list(want[1]) == [1, 1, 1, 2, 1, 2, 67] and list(want[0]) == [0, 0, 0, 0, 0, 0, 5]
    back = h.particles(0)["position"]
    assert back[:len(pts)].tobytes() == np.array(pts, dtype=f).tobytes()
    # the same points against rotated frames: whatever the operations give, the same on both sides
    _check(system, [h], [S.Collider.Box((10.0, 0.0, 0.0), (0.5, 0.5, 0.5), ROT), S.Collider.Capsule((20.0, 0.0, 0.0), 0.5, 1.0, ROT),
                         S.Collider.Cylinder((30.0, 0.0, 0.0), 0.5, 1.0, ROT), S.Collider.Cone((40.0, 0.0, 0.0), 0.5, 1.0, ROT),
                         S.Collider.Box((10.0, 0.0, 0.0), (np.nan, 0.5, -0.5)), S.Collider.Sphere((0.0, 0.0, 0.0), -1.0)], "rotated, NaN and negative extents")


def _device_words(ps, n):
    import torch

    with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
        return torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")


def test_device_form_behind_a_step_without_a_wait(system):
    chunk = system.debug_volume_query()[2]
    hs, _ = _zoo(system, chunk)
    vols = _volumes(65, _centres(hs))
    n = len(hs) * len(vols)
    buf = _device_words(system, n)
    for k in range(3):
        system.update(DT)
        system.count_in_volumes_device(hs, vols, buf.data_ptr() + 4)  # (enqueued right behind fw_step: nothing waits in between)
        host = system.count_in_volumes(hs, vols)
        system.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[:4] == 0xAB).all() and (raw[-4:] == 0xAB).all(), "a guard word was written"
        assert raw[4:-4].view(np.uint32).reshape(len(hs), len(vols)).tobytes() == host.tobytes()
        _check(system, hs, vols, f"frame {k}")


def test_two_launches_per_call_whatever_the_sizes(system):
    chunk = system.debug_volume_query()[2]
    hs, sizes = _zoo(system, chunk)
    vols = _volumes(129, _centres(hs))
    sparks = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=300)
    sparks.queue_particles(733)
    system.update(DT)
    n0 = system.debug_volume_query()[0]
    system.count_in_volumes([sparks], vols[:1])
    n1, chunks, _, _ = system.debug_volume_query()
    assert n1 == n0 + 2
    assert -(-733 // chunk) <= chunks < 256, "a 733-particle emitter occupies waves"
    system.count_in_volumes(hs + [sparks], vols)
    n2, chunks, _, _ = system.debug_volume_query()
    assert n2 == n1 + 2 and chunks >= sum(-(-n // chunk) for n in sizes)
    system.count_in_volumes(hs, vols)
    big = system.debug_volume_query()[1]
    system.count_in_volumes([(hs[5], 0), hs[1]], vols[:64])  # (a smaller call in the scratch the larger one grew)
    n3, chunks, _, _ = system.debug_volume_query()
    assert n3 == n2 + 4 and 2 <= chunks < big
    buf = _device_words(system, 2 * len(hs) * len(vols))
    system.count_in_volumes_device(hs + hs, vols, buf.data_ptr() + 4)
    assert system.debug_volume_query()[:2] == (n3 + 2, 2 * big)
    system.synchronize()
    _check(system, hs + hs, vols, "twice all")
    _check(system, [(hs[5], 0), hs[1]], vols[:64], "two again")
    assert system.aabb_records(hs)["any"].sum() > 8  # (the boxes share the tables: still answered)


def test_an_unread_ring_keeps_its_rules(fw_path, monkeypatch):
    if fw_path != "fifo":
        pytest.skip("the age rule and the deferred spin belong to the FIFO ring kernel: one run, under the path matrix's fifo entry")
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    _fifo_knobs(monkeypatch, FW_FUSE2="0")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(), S.Transform((1.0, 2.0, 3.0)), uid=19)
        vols = _volumes(14, [h.transform.translation]) + [S.Collider.Plane((1.0, 2.1, 3.0), (0.0, 1.0, 0.0))]  # (the last: through the young cloud)
        for _ in range(9):
            ps.update(DT)
        flagged = h.update_path(0)
        assert flagged[0] == "fifo"
        ages, spins = ps.age_launches(), ps.spin_launches()
        first = ps.count_in_volumes([h, (h, 0)], vols)  # first thing after the unread frames: the ages in memory are nine frames old, and stay so
        assert ps.age_launches() == ages and ps.spin_launches() == spins
        assert first[0].tobytes() == first[1].tobytes() and first[0, EVERYTHING] == h.counts()[0] and 0 < first[0, -1] < first[0, EVERYTHING]
        for k in range(3):  # ... and a host that asks every frame keeps every rule
            ps.update(DT)
            assert h.update_path(0) == flagged
            got = ps.count_in_volumes([h], vols)
            assert ps.age_launches() == ages and ps.spin_launches() == spins and h.update_path(0) == flagged
        want = volume_ref.counts([h], vols)  # (reads the particles: the one call here that writes ages back and replays the spin)
        assert ps.age_launches() == ages + 1 and ps.spin_launches() == spins + 1
        assert np.array_equal(got, want)


def _fused_run(monkeypatch, ask):
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    _fifo_knobs(monkeypatch, FW_FUSE2="1", FW_FUSE2_MIN="1")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(life_frames=16.0, capacity=16384), S.Transform((1.0, 2.0, 3.0)), uid=22)
        vols = _volumes(14, [h.transform.translation])
        for _ in range(8):
            ps.update(DT)
        ps.synchronize()
        for _ in range(3):  # (withheld, fused, withheld: tests/test_gpu_fifo_fuse2.py)
            ps.update(DT)
        fused, flushed = ps.fuse2_launches()
        got = None
        if ask:
            ages, spins = ps.age_launches(), ps.spin_launches()
            got = ps.count_in_volumes([h], vols)
            assert ps.fuse2_launches() == (fused, flushed + 1), "the withheld frame goes to the stream once, in front of the query"
            again = ps.count_in_volumes([h, h], vols)
            assert ps.fuse2_launches() == (fused, flushed + 1) and again[0].tobytes() == again[1].tobytes() == got[0].tobytes()
            assert ps.age_launches() == ages and ps.spin_launches() == spins
        for _ in range(4):
            ps.update(DT)
        return fused, got, h.particles(0)


def test_a_withheld_group_is_flushed_once_and_the_particles_are_the_same(fw_path, monkeypatch):
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")
    from bevy_firework_amd.system import ParticleSystem
    from test_gpu_spin_defer import _spawner

    fused, got, asked = _fused_run(monkeypatch, True)
    assert fused >= 1
    _, _, never = _fused_run(monkeypatch, False)
    assert len(asked) > 4000 and asked.tobytes() == never.tobytes()
    # the counts after the 11 frames: a context that fuses nothing, read back in full
    _fifo_knobs(monkeypatch, FW_FUSE2="0")
    with ParticleSystem(device=0, seed=SEED) as ps:
        h = ps.spawn(_spawner(life_frames=16.0, capacity=16384), S.Transform((1.0, 2.0, 3.0)), uid=22)
        vols = _volumes(14, [h.transform.translation])
        for _ in range(11):
            ps.update(DT)
        want = volume_ref.counts([h], vols)
    assert np.array_equal(got, want) and 0 < want[0, 0] < want[0, EVERYTHING]


def test_errors_write_nothing_and_enqueue_nothing(system):
    hs = [system.spawn(S.ParticleSpawner([_type(), _type()], [_on_demand()]), uid=10 + k) for k in range(4)]
    gone = system.spawn(S.ParticleSpawner([_type()], [_on_demand()]), uid=20)
    hs[1].queue_particles(9)
    system.update(DT)
    system.despawn(gone)
    L, ctx = system._lib, system._ctx
    vols = _volumes(4, [(0.0, 0.0, 0.0)])
    out = np.zeros((4, 4), dtype=np.uint32)
    out.view(np.uint8)[:] = 0xCD
    poison = out.tobytes()
    optr = out.ctypes.data_as(C.c_void_p)
    buf = _device_words(system, 16)
    dptr = C.c_void_p(buf.data_ptr() + 4)
    system.synchronize()
    launches = system.debug_volume_query()[0]

    def places(*v):
        a = np.array([tuple(x) for x in v], dtype=S.VOLUME_PLACE_DTYPE)
        return a, a.ctypes.data_as(C.c_void_p)

    def volumes(kinds=None):
        a = _ffi.make_colliders(vols)
        for k, kind in enumerate(kinds or []):
            a[k].kind = kind
        return a

    valid = [(h.handle, t) for h, t in zip(hs, (-1, 0, 1, -1))]
    keep, good = places(*valid)
    gv = volumes()
    assert L.fw_ctx_count_in_volumes(None, 4, good, 4, gv, optr) == _ffi.FW_EINVAL
    assert L.fw_ctx_count_in_volumes_device(None, 4, good, 4, gv, dptr) == _ffi.FW_EINVAL
    for form, dst in ((L.fw_ctx_count_in_volumes, optr), (L.fw_ctx_count_in_volumes_device, dptr)):
        assert form(ctx, 4, None, 4, gv, dst) == _ffi.FW_EINVAL
        assert form(ctx, 4, good, 4, None, dst) == _ffi.FW_EINVAL
        assert form(ctx, 4, good, 4, gv, None) == _ffi.FW_EINVAL
        for at in (0, 2, 3):  # (first, in the middle of a valid list, last)
            for bad in (-1, 1 << 20, gone.handle):
                v = list(valid)
                v[at] = (bad, -1)
                k, ptr = places(*v)
                assert form(ctx, 4, ptr, 4, gv, dst) == _ffi.FW_EINVAL, (bad, at)
                assert b"invalid spawner handle" in L.fw_last_error(ctx) and L.fw_last_error(ctx).startswith(b"fw_ctx_count_in_volumes")
            for bad in (2, -2, 1 << 30):  # (neither -1 nor one of the spawner's two types)
                v = list(valid)
                v[at] = (v[at][0], bad)
                k, ptr = places(*v)
                assert form(ctx, 4, ptr, 4, gv, dst) == _ffi.FW_EINVAL and b"no such particle type" in L.fw_last_error(ctx), (bad, at)
            for bad in (-1, 6, 1 << 20):
                kinds = [c.kind for c in vols]
                kinds[at] = bad
                assert form(ctx, 4, good, 4, volumes(kinds), dst) == _ffi.FW_EINVAL and b"unknown volume kind" in L.fw_last_error(ctx), (bad, at)
        # more answers than the indices hold: refused before either list is looked at beyond its first records
        assert form(ctx, 1 << 20, good, 1 << 20, gv, dst) == _ffi.FW_EINVAL and b"FW_VOLUME_MAX_ANSWERS" in L.fw_last_error(ctx)
        assert form(ctx, 0x4000000, good, 1, gv, dst) == _ffi.FW_EINVAL and form(ctx, 1, good, 0x4000000, gv, dst) == _ffi.FW_EINVAL
        for a, b in ((0, 4), (4, 0), (0, 0)):  # nothing to answer: nothing touched, null lists or not
            assert form(ctx, a, None, b, None, None) == _ffi.FW_OK and form(ctx, a, good, b, gv, dst) == _ffi.FW_OK
    assert L.fw_ctx_count_in_volumes_device(ctx, 4, good, 4, gv, C.c_void_p(buf.data_ptr() + 6)) == _ffi.FW_EINVAL  # (not 4-byte aligned)
    system.synchronize()
    assert out.tobytes() == poison and (buf.cpu().numpy() == 0xAB).all()
    assert system.debug_volume_query()[0] == launches
    # ... and the same arguments made valid are answered
    assert L.fw_ctx_count_in_volumes(ctx, 4, good, 4, gv, optr) == _ffi.FW_OK
    assert list(out[:, EVERYTHING]) == [0, 9, 0, 0] and not out[:, NOTHING].any()
    assert L.fw_ctx_count_in_volumes_device(ctx, 4, good, 4, gv, dptr) == _ffi.FW_OK
    system.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:4] == 0xAB).all() and (raw[-4:] == 0xAB).all() and raw[4:-4].tobytes() == out.tobytes()
    _check(system, [(hs[0], -1), (hs[1], 0), (hs[2], 1), (hs[3], -1)], vols)
