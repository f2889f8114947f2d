"""Depth-sorted instance records on the device (include/firework_hip.h: DEPTH-SORTED INSTANCES; csrc/fw_k_sort.hip, fw_k_depth_keys and
fw_k_pack<true> of csrc/fw_k_aux.hip): fw_ctx_depth_order_device, fw_ctx_pack_instances_sorted_device and fw_ctx_pack_instances_sorted
against tests/sort_ref.py -- numpy written from the header's text.  The expected sorted records are the UNSORTED pack's records
(SpawnerData.instances(), pinned by the existing suites) taken in the reference's order, so every comparison is of bytes and no
tolerance exists.  The autouse fw_path fixture runs every test on the FIFO ring, the range ring, the compacting path and the small
path.  Needs an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref  # noqa: E402
from test_gpu_fuzz import _spawner as _fuzz_spawner  # noqa: E402
from test_gpu_fuzz import _steps as _fuzz_steps  # noqa: E402
from test_gpu_ray_query import _ctx_stream  # noqa: E402

from bevy_firework_amd import _ffi, workloads  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 2020
DT = f32(1.0 / 60.0)
T = 2048  # elements per workgroup of the sort: FW_SORT_TILE of csrc/fw_sort.h (FW_SORT_WG 256 lanes x FW_SORT_ROUNDS 8)
POISON = 0xA5
PAD = 64  # entries of every device buffer behind `cap`: must stay poisoned
ORDERS = (S.SORT_BACK_TO_FRONT, S.SORT_FRONT_TO_BACK)


def _system(seed=SEED):
    from bevy_firework_amd.system import ParticleSystem

    return ParticleSystem(device=0, seed=seed)


def _on_demand():
    """the stress test's type (drag, a gradient, a cone of velocities, lifetime 1 s), fed on demand: exact counts"""
    sp, tf = workloads.stress_test()
    sp.emission_settings[0].emission_pacing = S.EmissionPacing.OnDemand()
    return sp, tf


def _poisoned(system, n_bytes):
    import torch

    with _ctx_stream(system):
        return torch.full((n_bytes,), POISON, dtype=torch.uint8, device="cuda")


def _host_form(system, d, view, cap, ptype=0):
    """fw_ctx_pack_instances_sorted with its own cap -> (records written, count reported, the poisoned tail)"""
    n = C.c_uint64()
    out = np.full((cap + PAD) * 64, POISON, dtype=np.uint8).view(S.INSTANCE_DTYPE)
    system._check(system._lib.fw_ctx_pack_instances_sorted(system._ctx, d.handle, ptype, C.byref(_ffi.make_sort_view(view)),
                                                           out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    m = min(int(n.value), cap)
    return out[:m], int(n.value), out[m:]


def _check_all_forms(system, d, view, cap=None, ptype=0, what="", min_slack=0):
    """all three forms of one (spawner, type, view, cap) against the unsorted pack of the same state permuted by sort_ref; -> the order
    (min_slack: by how much the bound both device forms return has to exceed the count at least)"""
    unsorted = d.instances(ptype)
    n = len(unsorted)
    cap = n + 7 if cap is None else cap
    m = min(n, cap)
    want_order = sort_ref.order_of(unsorted["position"], view.eye, view.forward, view.order, cap=m)
    want = unsorted[:m][want_order]
    d_ord, d_rec = _poisoned(system, (cap + PAD) * 4), _poisoned(system, (cap + PAD) * 64)
    ub_o = system.depth_order_device(d, view, d_ord.data_ptr(), cap, ptype)
    ub_r = system.pack_instances_sorted_device(d, view, d_rec.data_ptr(), cap, ptype)
    system.synchronize()
    assert m <= ub_o <= cap and m <= ub_r <= cap, (what, n, cap, ub_o, ub_r)
    assert not min_slack or (ub_o >= n + min_slack and ub_r >= n + min_slack), (what, "the bound is closer to the count than this case needs", n, cap, ub_o, ub_r)
    got_ord = d_ord.cpu().numpy().view(np.uint32)
    got_rec = d_rec.cpu().numpy().view(S.INSTANCE_DTYPE)
    assert np.array_equal(got_ord[:m], want_order), (what, "order", n, cap)
    assert (got_ord[m:].view(np.uint8) == POISON).all(), (what, "order entries at and beyond min(count, cap) were written")
    assert got_rec[:m].tobytes() == want.tobytes(), (what, "device records", n, cap)
    assert (got_rec[m:].view(np.uint8) == POISON).all(), (what, "records at and beyond min(count, cap) were written")
    host, count, tail = _host_form(system, d, view, cap, ptype)
    assert count == n and host.tobytes() == want.tobytes(), (what, "host records", n, cap)
    assert (tail.view(np.uint8) == POISON).all(), (what, "host records beyond min(count, cap) were written")
    if cap >= n:
        assert d.instances_sorted(view, ptype).tobytes() == want.tobytes(), (what, "instances_sorted")
    assert d.instances(ptype).tobytes() == unsorted.tobytes(), (what, "a sorted call changed the particles")
    return want_order


def _inside_view(positions, rng, order):
    """the eye inside the cloud, so depths have both signs; a forward vector that is not normalised"""
    p = np.asarray(positions, dtype=f32).reshape(-1, 3)
    eye = p.mean(axis=0).astype(f32) if len(p) else np.zeros(3, dtype=f32)
    fwd = (rng.normal(size=3) * rng.uniform(0.5, 3.0)).astype(f32)
    return S.SortView(eye=tuple(float(c) for c in eye), forward=tuple(float(c) for c in fwd), order=order)


# ---- 1. counts: one element, a wave, a round, a workgroup, several workgroups and rows ------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 70001])
def test_every_form_sorts_n_particles_in_both_orders(fw_path, n):
    sp, tf = _on_demand()
    rng = np.random.default_rng(SEED + n)
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(n)
        for _ in range(4):
            system.update(DT)
        assert d.count(0) == n
        pos = d.instances(0)["position"]
        for order in ORDERS:
            view = _inside_view(pos, rng, order)
            got = _check_all_forms(system, d, view, what=f"n={n} order={order}")
            if n > 64:
                depth = sort_ref.depth(pos, view.eye, view.forward)
                assert (depth < 0).any() and (depth > 0).any()  # (the eye is inside the cloud)
                assert not np.array_equal(got, np.arange(n))     # (and the order is not the list's)


# ---- 2. stability through every pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 2 * T + 1])
def test_a_zero_forward_vector_returns_the_unsorted_pack(fw_path, n):
    """every depth is 0, every key ties in all four digits: the identity, byte for byte"""
    sp, tf = _on_demand()
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(n)
        for _ in range(3):
            system.update(DT)
        for order in ORDERS:
            view = S.SortView(eye=(0.25, 0.5, -0.125), forward=(0.0, 0.0, 0.0), order=order)
            got = _check_all_forms(system, d, view, what=f"zero forward n={n}")
            assert np.array_equal(got, np.arange(n)) and d.instances_sorted(view).tobytes() == d.instances(0).tobytes()


def test_thousands_of_ties_in_a_few_groups_keep_list_order(fw_path):
    """a Point emitter that gives no velocity, moved between five batches: four heights (one used twice), so four keys, in an order that is not
    the batches'; inside a group the list order survives all four passes"""
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(2.0), initial_scale=S.RandF32(0.02, 0.08), acceleration=(0.0, 0.0, 0.0))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand(), emission_shape=S.EmissionShape.Point(),
                            initial_velocity=S.RandVec3(S.RandF32.constant(0.0), (0.0, 1.0, 0.0), 0.0))
    heights = (0.5, -1.25, 3.0, -1.25, 0.0)
    with _system() as system:
        d = system.spawn(S.ParticleSpawner([ps], [es]), S.Transform((0.0, 0.0, 0.0)), uid=5)
        for k, y in enumerate(heights):
            d.set_transform(S.Transform((0.125, y, -0.5)))
            d.queue_particles(1500 + 77 * k)
            system.update(DT)
        pos = d.instances(0)["position"]
        assert len(pos) == sum(1500 + 77 * k for k in range(5)) and len(np.unique(pos[:, 1])) == 4 and len(np.unique(pos[:, 0])) == 1
        for order in ORDERS:
            view = S.SortView(eye=(0.0, 0.25, 0.0), forward=(0.0, 1.0, 0.0), order=order)
            got = _check_all_forms(system, d, view, what="ties")
            assert len(np.unique(sort_ref.keys(pos, view.eye, view.forward, order))) == 4
            assert not np.array_equal(got, np.arange(len(pos)))


# ---- 3. ring state: a head that is not 0, an old part ------------------------------------------------------------------------------------
def test_a_rate_emitter_past_its_lifetime_sorts_on_its_path(fw_path):
    sp, tf = workloads.stress_test(rate=3000.0)
    rng = np.random.default_rng(SEED)
    with _system() as system:
        d = system.spawn(sp, tf, uid=2)
        for fr in range(80):  # lifetime 1 s: the first particles died twenty frames ago
            system.update(DT)
        assert d.update_path(0)[0] == fw_path
        assert 2500 < d.count(0) < 3100
        for order in ORDERS:
            _check_all_forms(system, d, _inside_view(d.instances(0)["position"], rng, order), what=f"ring {fw_path}")
        system.update(DT)  # ... and the frame after a reader
        assert d.update_path(0)[0] == fw_path
        _check_all_forms(system, d, _inside_view(d.instances(0)["position"], rng, S.SORT_BACK_TO_FRONT), what=f"ring {fw_path}, next frame")


# ---- 4. special values (written particles: the compacting path by design) ---------------------------------------------------------------
def test_special_depths_sort_as_the_header_says(fw_path):
    """positions along x whose depths from eye 0 along +x are +-0, +-inf, NaN, denormals of both signs and many exact ties"""
    sp, tf = _on_demand()
    rng = np.random.default_rng(SEED + 4)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800123, 0x00000001, 0x80000001, 0x007FFFFF,
                         0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(f32)
    x = np.concatenate([np.tile(specials, 40), rng.integers(-3, 4, 3000).astype(f32) * f32(0.5), rng.normal(size=700).astype(f32)])
    rng.shuffle(x)
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(16)
        system.update(DT)
        rec = np.zeros(len(x), dtype=S.PARTICLE_DTYPE)
        rec[:] = d.particles(0)[0]
        rec["position"] = 0.0
        rec["position"][:, 0] = x
        rec["position"][:, 1] = rng.normal(size=len(x)).astype(f32)  # (times forward.y = 0: no part of the depth ... unless x is NaN or inf)
        d.write_particles(0, rec)
        assert d.instances(0)["position"][:, 0].tobytes() == x.tobytes()
        for order in ORDERS:
            view = S.SortView(eye=(0.0, 0.0, 0.0), forward=(1.0, 0.0, 0.0), order=order)
            got = _check_all_forms(system, d, view, what=f"special values order={order}")
            k = sort_ref.keys(rec["position"], view.eye, view.forward, order)[got]
            assert (np.diff(k.astype(np.int64)) >= 0).all() and (k[-40 * 3:] == 0xFFFFFFFF).all() and (k[:-40 * 3] != 0xFFFFFFFF).all()


# ---- 5. cap ---------------------------------------------------------------------------------------------------------------------------------
def test_cap_below_the_count_sorts_the_first_cap_particles_only(fw_path):
    sp, tf = _on_demand()
    n = T + 300
    rng = np.random.default_rng(SEED + 5)
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(n)
        for _ in range(4):
            system.update(DT)
        view = _inside_view(d.instances(0)["position"], rng, S.SORT_BACK_TO_FRONT)
        for cap in (1, 64, n - 1, n, n + 1):
            got = _check_all_forms(system, d, view, cap=cap, what=f"cap={cap}")
            assert len(got) == min(cap, n) and (not len(got) or int(got.max()) < cap)


# ---- 6. scratch regrowth and reuse ---------------------------------------------------------------------------------------------------------
def test_the_scratch_grows_and_is_reused_between_types_and_spawners(fw_path):
    sp, tf = _on_demand()
    rng = np.random.default_rng(SEED + 6)
    with _system() as system:
        small, large, other = (system.spawn(sp, tf, uid=u) for u in (1, 2, 3))
        small.queue_particles(300), large.queue_particles(3 * T + 5), other.queue_particles(T + 1)
        for _ in range(3):
            system.update(DT)
        for k, d in enumerate((small, large, small, other, large)):
            _check_all_forms(system, d, _inside_view(d.instances(0)["position"], rng, ORDERS[k & 1]), what=f"scratch call {k}")


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------------------
def test_device_forms_answer_for_their_place_in_the_stream(fw_path):
    """a step, the sorted pack, another step, the order, ONE synchronisation at the end: the records are those of the first step's
    state and the order that of the second's (a twin context, stepped and read frame by frame, says what those are)"""
    sp, tf = _on_demand()
    view = S.SortView(eye=(0.0, 1.0, 0.0), forward=(0.3, -0.5, 0.8), order=S.SORT_BACK_TO_FRONT)
    with _system() as twin:
        h = twin.spawn(sp, tf, uid=1)
        h.queue_particles(256)
        states = []
        for _ in range(2):
            twin.update(DT)
            states.append(h.instances(0).copy())
    assert states[0].tobytes() != states[1].tobytes()
    with _system() as system:
        h = system.spawn(sp, tf, uid=1)
        h.queue_particles(256)
        d_rec, d_ord = _poisoned(system, 256 * 64), _poisoned(system, 256 * 4)
        system.pack_instances_sorted_device(h, view, d_rec.data_ptr(), 1, 0)  # (the scratch's one wait happens here, in front of everything)
        system.update(DT)
        ub1 = system.pack_instances_sorted_device(h, view, d_rec.data_ptr(), 256)
        system.update(DT)
        ub2 = system.depth_order_device(h, view, d_ord.data_ptr(), 256)
        system.synchronize()
        assert (ub1, ub2) == (256, 256)
        o1 = sort_ref.order_of(states[0]["position"], view.eye, view.forward, view.order)
        o2 = sort_ref.order_of(states[1]["position"], view.eye, view.forward, view.order)
        assert d_rec.cpu().numpy().tobytes() == states[0][o1].tobytes()
        assert np.array_equal(d_ord.cpu().numpy().view(np.uint32), o2)
        assert h.instances(0).tobytes() == states[1].tobytes()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def _three_steps(bad_call=None):
    """a context with a destroyed spawner (handle 0) and a healthy one of 256 particles (handle 1): [(its count, the context's, its
    particles)] after each of three steps; bad_call(system, victim handle, healthy handle, a poisoned device buffer) runs in front of
    every step (the pattern of tests/test_gpu_entry_points.py)"""
    sp, tf = _on_demand()
    frames = []
    with _system(1717) as system:
        victim = system.spawn(sp, tf, uid=0)
        healthy = system.spawn(sp, tf, uid=1)
        system.despawn(victim)
        healthy.queue_particles(256)
        d_out = _poisoned(system, 256 * 64)
        system.synchronize()
        for _ in range(3):
            if bad_call is not None:
                bad_call(system, victim.handle, healthy.handle, C.c_void_p(d_out.data_ptr()))
            system.update(DT)
            frames.append((healthy.count(0), system.live_count(), healthy.particles(0).tobytes()))
        assert (d_out.cpu().numpy() == POISON).all(), "a refused call wrote to the caller's buffer"
    return frames


@functools.lru_cache(maxsize=None)
def _undisturbed(path, test_name):
    """(per path and per test function: the fixture's knobs follow both)"""
    frames = _three_steps()
    assert [f[:2] for f in frames] == [(256, 256)] * 3 and len({f[2] for f in frames}) == 3
    return tuple(frames)


@pytest.mark.parametrize("name", ["fw_ctx_depth_order_device", "fw_ctx_pack_instances_sorted_device", "fw_ctx_pack_instances_sorted"])
def test_refused_calls_write_nothing_and_disturb_nobody(fw_path, name):
    good = _ffi.make_sort_view(S.SortView(eye=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0)))
    bad_order, bad_reserved = _ffi.make_sort_view(S.SortView(order=2)), _ffi.make_sort_view(S.SortView(reserved=1))
    huge_order = _ffi.make_sort_view(S.SortView(order=0xFFFFFFFF))
    host = name == "fw_ctx_pack_instances_sorted"

    def bad_call(system, victim, healthy, d_out):
        fn, ctx = getattr(system._lib, name), system._ctx
        host_out = np.full(256 * 64, POISON, dtype=np.uint8)
        out = host_out.ctypes.data_as(C.c_void_p) if host else d_out
        n = C.c_uint64(12345)
        assert fn(None, healthy, 0, C.byref(good), out, 256, C.byref(n)) == FW_EINVAL, (name, "null ctx")
        for h in (7, -1, victim):
            assert fn(ctx, h, 0, C.byref(good), out, 256, C.byref(n)) == FW_EINVAL, (name, h)
        assert fn(ctx, healthy, 1, C.byref(good), out, 256, C.byref(n)) == FW_EINVAL, (name, "type == type count")
        assert fn(ctx, healthy, 0, None, out, 256, C.byref(n)) == FW_EINVAL, (name, "null view")
        if not host:  # (the host form takes out = NULL to ask for the count alone, as fw_spawner_pack_instances does)
            assert fn(ctx, healthy, 0, C.byref(good), None, 256, C.byref(n)) == FW_EINVAL, (name, "null buffer")
        for v, why in ((bad_order, "order = 2"), (huge_order, "order = 0xFFFFFFFF"), (bad_reserved, "reserved = 1")):
            assert fn(ctx, healthy, 0, C.byref(v), out, 256, C.byref(n)) == FW_EINVAL, (name, why)
        assert n.value == 12345 and (host_out == POISON).all(), (name, "a refused call wrote to its outputs")

    assert tuple(_three_steps(bad_call)) == _undisturbed(fw_path, "test_refused_calls_write_nothing_and_disturb_nobody"), name


def test_accepted_calls_disturb_nobody_either(fw_path):
    """the three forms in front of every step: the healthy spawner's frames are those of a context that never sorted"""
    view = S.SortView(eye=(0.0, 1.0, 0.0), forward=(0.3, 0.2, 1.0))

    def calls(system, victim, healthy, d_out):
        d = system.spawners[healthy]
        d_tmp = _poisoned(system, 256 * 64)
        system.depth_order_device(d, view, d_tmp.data_ptr(), 256)
        system.pack_instances_sorted_device(d, view, d_tmp.data_ptr(), 256)
        d.instances_sorted(view)

    assert tuple(_three_steps(calls)) == _undisturbed(fw_path, "test_accepted_calls_disturb_nobody_either")


# ---- 9. a random suite -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(36))
def test_random_spawners_views_orders_and_caps(fw_path, case):
    rng = np.random.default_rng(202000 + case)
    spawner = _fuzz_spawner(rng, scale=0.15, const_p=0.5)
    tf = S.Transform(tuple(float(c) for c in rng.uniform(-2.0, 2.0, size=3)), tuple(float(c) for c in (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))))
    on_demand = any(e.emission_pacing.kind == S.PACING_ONDEMAND for e in spawner.emission_settings)
    with _system(SEED + case) as system:
        d = system.spawn(spawner, tf, uid=case)
        for i, dt in enumerate(_fuzz_steps(rng, 24)):
            if on_demand and i % 5 == 0:
                d.queue_particles(int(rng.integers(0, 1500)))
            system.update(f32(dt))
            if i % 8 != 7:
                continue
            for t in range(len(spawner.particle_settings)):
                pos = d.instances(t)["position"]
                view = _inside_view(pos, rng, int(rng.integers(0, 2)))
                if rng.random() < 0.3:  # an eye far outside: one sign, small relative differences
                    view.eye = tuple(float(c) for c in rng.uniform(-50.0, 50.0, size=3))
                cap = None if rng.random() < 0.5 else int(rng.integers(1, max(2, len(pos) + 10)))
                _check_all_forms(system, d, view, cap=cap, ptype=t, what=f"case {case} frame {i} type {t}")
        assert len(d.counts()) == len(spawner.particle_settings)


# ---- 10. the sizes at which the kernels change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256 * T + 1, 2097152 + 300])
def test_every_form_sorts_counts_beyond_one_column_per_lane_and_one_trip_of_the_grid(fw_path, n):
    """256 * T + 1 particles are 257 tiles: fw_k_sort_scan gives a lane two columns of a histogram row for the first time (every smaller
    case gives it one).  2 097 152 + 300 are more than the 8192 workgroups of 256 lanes fw_k_depth_keys and fw_k_pack<true> launch at
    the most: both go round their grid-stride loop a second time (the gather with its two barriers and the LDS transpose inside)."""
    if fw_path not in ("fifo", "general"):
        pytest.skip("the sort's launches depend on the count alone: the FIFO ring and the compacting path stand for the four "
                    "(the small entry would put two million particles on one wave)")
    sp, tf = _on_demand()
    rng = np.random.default_rng(SEED + n)
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(n)
        for _ in range(4):
            system.update(DT)
        assert d.count(0) == n and d.update_path(0)[0] == fw_path
        large = n > 8192 * 256
        assert large or -(-n // T) > 256
        pos = d.instances(0)["position"]
        for order in ORDERS[:1] if large else ORDERS:
            view = _inside_view(pos, rng, order)
            got = _check_all_forms(system, d, view, what=f"n={n} order={order}")
            assert not np.array_equal(got, np.arange(n))


# ---- 11. a bound far above the count -------------------------------------------------------------------------------------------------------
def _nested_children(capacity):
    """150 parents queued once (0.5 s), each emitting 12 children a second (0.2 s): a few hundred children in a segment of `capacity` slots"""
    parents = S.ParticleSettings(lifetime=S.RandF32.constant(0.5), initial_scale=S.RandF32(0.01, 0.03), linear_drag=0.3)
    children = S.ParticleSettings(lifetime=S.RandF32.constant(0.2), initial_scale=S.RandF32(0.05, 0.1), acceleration=(0.0, 0.5, 0.0), capacity=capacity,
                                  base_color=S.FireworkGradient.even_samples([(8.0, 4.0, 1.0, 1.0), (1.0, 0.2, 0.0, 0.0)]))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.OnDemand(), emission_shape=S.EmissionShape.Sphere(0.5),
                            initial_velocity=S.RandVec3(S.RandF32(2.0, 6.0), (0.0, 1.0, 0.0), 0.4))
    e1 = S.EmissionSettings(particle_index=1, emission_pacing=S.EmissionPacing.rate(12.0), emission_mode=S.EmissionMode.Nested(0),
                            inherit_parent_velocity=False)
    return S.ParticleSpawner([parents, children], [e0, e1])


def _device_forms_write_nothing(system, d, view, cap, ptype, what):
    d_ord, d_rec = _poisoned(system, (cap + PAD) * 4), _poisoned(system, (cap + PAD) * 64)
    ub_o = system.depth_order_device(d, view, d_ord.data_ptr(), cap, ptype)
    ub_r = system.pack_instances_sorted_device(d, view, d_rec.data_ptr(), cap, ptype)
    system.synchronize()
    assert (d_ord.cpu().numpy() == POISON).all() and (d_rec.cpu().numpy() == POISON).all(), (what, "no particle lives, yet something was written")
    return ub_o, ub_r


def test_nested_children_sort_under_a_bound_of_their_whole_capacity(fw_path):
    """a type fed by Nested entries: the host does not know its count, the bound is the segment's capacity -- trailing tiles that hold
    no element (fw_k_sort_hist writes columns of zeros, fw_k_sort_scatter returns early), and in the end a count of 0 under a bound
    of thousands"""
    capacity = 8 * T
    rng = np.random.default_rng(SEED + 11)
    with _system() as system:
        d = system.spawn(_nested_children(capacity), S.Transform((0.5, 1.0, -0.25)), uid=4)
        d.queue_particles(150)
        seen = []
        for fr in range(60):
            system.update(DT)
            if fr in (9, 20, 33):  # (33: the parents are gone, the last children are dying)
                n = d.count(1)
                seen.append(n)
                for order in ORDERS:
                    _check_all_forms(system, d, _inside_view(d.instances(1)["position"], rng, order), cap=capacity, ptype=1,
                                     what=f"nested frame {fr}", min_slack=2 * T)
        assert 100 < seen[0] < 1000 and 100 < seen[1] < 1000 and 0 < seen[2] < seen[1], seen
        view = S.SortView(eye=(0.0, 1.0, 0.0), forward=(0.3, -0.5, 0.8))
        ub_o, ub_r = _device_forms_write_nothing(system, d, view, capacity, 1, "nested, drained")  # (in front of any call that reads the count)
        assert ub_o >= 2 * T and ub_r >= 2 * T, (ub_o, ub_r)
        assert d.counts() == [0, 0]
        for order in ORDERS:
            view.order = order
            assert len(_check_all_forms(system, d, view, cap=capacity, ptype=1, what="nested, drained", min_slack=2 * T)) == 0


def _check_device_forms_first(system, d, view, cap, ptype=0, what="", min_slack=0):
    """both device forms in front of any call that tells the host the count (its bound is what the frames since the last such call left
    it), then the unsorted pack they must agree with; -> the count"""
    d_ord, d_rec = _poisoned(system, (cap + PAD) * 4), _poisoned(system, (cap + PAD) * 64)
    ub_o = system.depth_order_device(d, view, d_ord.data_ptr(), cap, ptype)
    ub_r = system.pack_instances_sorted_device(d, view, d_rec.data_ptr(), cap, ptype)
    system.synchronize()
    unsorted = d.instances(ptype)
    n = len(unsorted)
    assert n <= cap, (what, n, cap)
    print(f"[{what}] count {n} cap {cap} bounds {ub_o} {ub_r}")
    assert n + min_slack <= ub_o <= cap and n + min_slack <= ub_r <= cap, (what, n, cap, ub_o, ub_r, min_slack)
    want_order = sort_ref.order_of(unsorted["position"], view.eye, view.forward, view.order)
    got_ord, got_rec = d_ord.cpu().numpy().view(np.uint32), d_rec.cpu().numpy().view(S.INSTANCE_DTYPE)
    assert np.array_equal(got_ord[:n], want_order), (what, "order", n, cap)
    assert (got_ord[n:].view(np.uint8) == POISON).all(), (what, "order entries at and beyond the count were written")
    assert got_rec[:n].tobytes() == unsorted[want_order].tobytes(), (what, "device records", n, cap)
    assert (got_rec[n:].view(np.uint8) == POISON).all(), (what, "records at and beyond the count were written")
    return n


def test_a_cap_four_tiles_above_the_count_on_the_compacting_path(fw_path):
    """a caller that passes its buffer's size: a rate-fed type with a lifetime range (0.05 .. 1 s, 12 000 a second: about 6300 live), read
    after thirty frames in which nobody asked for a count.  On the compacting path the host's bound then lies above the count by the
    spawns since the last device count it has seen (200 a frame; which frame that was depends on when the snapshot landed, so the
    excess -- thousands, printed -- is not asserted; the Nested-fed case above has a fixed one), and cap = count + 4 tiles does not
    clip it.  Then one frame longer than anybody lives, and both device forms in front of any call that tells the host that nobody
    is left"""
    ps = S.ParticleSettings(lifetime=S.RandF32(0.05, 1.0), initial_scale=S.RandF32(0.02, 0.08), linear_drag=0.2,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(12000.0), emission_shape=S.EmissionShape.Sphere(0.75),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.5))
    rng = np.random.default_rng(SEED + 12)
    compacting = fw_path in ("fifo", "general")  # (a lifetime range: no FIFO ring; the other two entries run it on their own layout)
    with _system() as system:
        d = system.spawn(S.ParticleSpawner([ps], [es]), S.Transform((0.0, 1.0, 0.0)), uid=6)
        for _ in range(65):
            system.update(DT)
        count = d.count(0)
        assert 5500 < count < 7000, count
        if compacting:
            assert d.update_path(0)[0] == "general"
        for k, order in enumerate(ORDERS):
            for _ in range(30):
                system.update(DT)
            view = _inside_view(np.zeros((1, 3)), rng, order)
            view.eye = (0.25, 2.0, -0.125)
            count = _check_device_forms_first(system, d, view, count + 4 * T, what=f"cap = count + 4 tiles, stretch {k}")
            _check_all_forms(system, d, view, cap=count + 4 * T, what=f"cap = count + 4 tiles, after stretch {k}")
        system.update(f32(1.0625))  # longer than anybody lives: everything dies, the particles of this very frame included
        view = S.SortView(eye=(0.0, 1.0, 0.0), forward=(0.3, -0.5, 0.8))
        assert _check_device_forms_first(system, d, view, 4 * T, what="everybody died") == 0
        for order in ORDERS:
            view.order = order
            assert len(_check_all_forms(system, d, view, cap=4 * T, what="everybody died")) == 0


# ---- 12. keys the engine's clouds never make (written particles: the compacting path by design) -------------------------------------------
def _bits_to_sort(rng, name, n):
    """position.x as bit patterns: with eye 0 and forward +x the depth is x and the key a bijection of its bits.  No NaN and no zero
    (test_special_depths_sort_as_the_header_says has those): bytes are drawn from 1 .. 255, the top byte from 1 .. 127 (one sign: a negative
    depth's key is the complement of its bits, which would put two values into the other three digits as well)"""
    if name == "eight":
        while True:
            eight = rng.integers(0, 1 << 32, size=8, dtype=np.uint64).astype(np.uint32)
            if np.isfinite(eight.view(f32)).all() and (eight.view(f32) != 0).all() and len(np.unique(eight)) == 8:
                return eight[rng.integers(0, 8, size=n)]
    b = int(name)
    byte = rng.integers(1, 256, size=n, dtype=np.uint64).astype(np.uint32)
    if b == 3:
        byte = np.uint32(1) + (byte - np.uint32(1)) % np.uint32(127)
    return byte << np.uint32(8 * b)


@pytest.mark.parametrize("name", ["0", "1", "2", "3", "eight"], ids=["byte 0", "byte 1", "byte 2", "byte 3", "eight distinct keys"])
def test_one_pass_carries_the_whole_order_through_the_engine(fw_path, name):
    """one byte of the key varies and the other three are the same everywhere: one pass of the four sorts, three have every element in
    one digit and must be the identity.  And eight distinct depths with replacement: hundreds of ties per key, stability is the answer"""
    sp, tf = _on_demand()
    n = 3 * T + 5
    rng = np.random.default_rng([SEED, 12, ["0", "1", "2", "3", "eight"].index(name)])
    bits = _bits_to_sort(rng, name, n)
    x = bits.view(f32)
    assert np.isfinite(x).all() and (x != 0).all()
    with _system() as system:
        d = system.spawn(sp, tf, uid=3)
        d.queue_particles(16)
        system.update(DT)
        rec = np.zeros(n, dtype=S.PARTICLE_DTYPE)
        rec[:] = d.particles(0)[0]
        rec["position"] = 0.0
        rec["position"][:, 0] = x
        d.write_particles(0, rec)
        assert d.instances(0)["position"][:, 0].tobytes() == x.tobytes()
        for order in ORDERS:
            view = S.SortView(eye=(0.0, 0.0, 0.0), forward=(1.0, 0.0, 0.0), order=order)
            k = sort_ref.keys(rec["position"], view.eye, view.forward, order)
            assert len(np.unique(k)) == len(np.unique(bits))  # (a bijection of the bits)
            digits = [len(np.unique((k >> np.uint32(8 * p)) & np.uint32(0xFF))) for p in range(4)]
            assert name == "eight" or sorted(digits)[:3] == [1, 1, 1], digits
            got = _check_all_forms(system, d, view, what=f"bits {name} order={order}")
            assert not np.array_equal(got, np.arange(n))
