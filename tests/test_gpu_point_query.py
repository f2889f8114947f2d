"""The point query on the device (include/firework_hip.h: POINT QUERIES; fw_ctx_project_points / fw_ctx_project_points_device): a batch
of points onto the device-resident collider world, per point the nearest point, its distance, its owner and is_inside.  Every field
must equal, bit for bit, tests/project_ref.py -- the header's text in numpy, a brute force over all triangles -- for the worlds and
points of tests/project_points.py (what tests/test_point_query_cpu.py runs through the same code on the host).  Device buffers are
torch tensors.  Needs an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
import project_points as P  # noqa: E402
import project_ref  # noqa: E402
from test_gpu_mesh import _falling_spawner, _terrain  # noqa: E402
from test_gpu_mesh_deform import deform  # noqa: E402
from test_gpu_ray_query import SENTINEL, _ctx_stream, _read, _system  # noqa: E402
from test_point_query_cpu import assert_projections_equal  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL, FW_OK  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = 0xFFFFFFFF
MASKS = (0xFFFFFFFF, 0b101, 0)


def _records(points, masks):
    r = np.zeros(len(points), dtype=S.POINT_DTYPE)
    r["position"], r["filter_mask"] = points, masks
    return r


def _to_device(system, records):
    import torch

    host = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, 16).copy())
    with _ctx_stream(system):
        return host.to("cuda")


def _out_buffer(system, n_records):
    import torch

    with _ctx_stream(system):
        return torch.full((n_records, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _project_device(system, records, n=None):
    n = len(records) if n is None else n
    d_points, d_out = _to_device(system, records), _out_buffer(system, n + 2)
    system.project_points_device(d_points.data_ptr(), n, d_out.data_ptr())
    raw = _read(system, d_out)
    assert (raw[n:] == SENTINEL).all(), "the 64 bytes behind the last record were written"
    return raw[:n].reshape(-1).view(S.POINT_PROJECTION_DTYPE).copy()


def _open(system, world):
    """the world on the device: the analytic set, the meshes (deformable where the world says so), the instance set -> mesh handles"""
    system.set_colliders(world.colliders)
    handles = [(system.create_deformable_mesh if deformable else system.create_mesh)(v, t) for v, t, deformable in world.meshes]
    system.set_mesh_colliders([S.MeshCollider(handles[k], p, q, layers) for k, p, q, layers in world.placements])
    return handles


def _worlds():
    w = P.mixed_world()
    return {"analytic": P.World(w.colliders), "meshes": P.World([], w.meshes, w.placements), "mixed": w}


@functools.lru_cache(maxsize=None)
def _reference(name, mask):
    w = _worlds()[name]
    out = project_ref.project_points(w.colliders, w.instances(), P.mixed_points(), mask)
    out.setflags(write=False)
    return out


# ---- 1. bit-exact ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
def test_projections_are_bit_exact(mask):
    """~3400 points (spread over the scene, near the surfaces, inside the solids, far away, a NaN, an infinity) onto the analytic
    colliders alone (the kernel without the mesh loop), the mesh instances alone and both; the engineered cases per kind and the
    meshes of 1, 2, 5 and 200 triangles under the mask of each"""
    pts = P.mixed_points()
    for name, w in _worlds().items():
        with _system() as system:
            _open(system, w)
            got = _project_device(system, _records(pts, mask))
        want = _reference(name, mask)
        assert_projections_equal(got, want, f"{name}, mask {mask:#x}")
        if mask == 0:
            assert (got["kind"] == S.HIT_NONE).all() and (got["index"] == NONE).all() and not got["point"].any()
        else:
            assert (got["kind"] != S.HIT_NONE).sum() > 3000
    if mask == MASKS[0]:
        for w, p, m in (P.engineered()[:3], P.mesh_sizes()):
            with _system() as system:
                _open(system, w)
                got = _project_device(system, _records(p, m))
            assert_projections_equal(got, project_ref.project_points(w.colliders, w.instances(), p, m), "engineered / mesh sizes")
            assert (got["kind"] != S.HIT_NONE).all()


# ---- 2. launch sizes, masks mixed inside a wave ------------------------------------------------------------------------------------
def test_sizes_around_the_wave_and_the_workgroup_with_masks_mixed_inside_a_wave():
    """n in {1, 63, 64, 65, 255, 256, 257, 1000}, each a prefix of the same points: the prefix of the large batch's result, the 64
    bytes behind the last record untouched, n = 0 touches nothing; the three masks dealt out point by point (every wave holds all
    three) and in runs of 5: each point equals the uniform-mask reference for its mask"""
    pts = P.mixed_points()
    n_all = len(pts)
    cycle = np.array(MASKS, dtype=np.uint32)
    with _system() as system:
        _open(system, P.mixed_world())
        for deal in (np.arange(n_all) % 3, (np.arange(n_all) // 5) % 3):
            recs = _records(pts, cycle[deal])
            big = _project_device(system, recs)
            for k, m in enumerate(MASKS):
                assert_projections_equal(big[deal == k], _reference("mixed", m)[deal == k], f"dealt, mask {m:#x}")
            assert (big["kind"][deal == 2] == S.HIT_NONE).all() and (big["kind"][deal != 2] != S.HIT_NONE).sum() > 2000
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            got = _project_device(system, recs[:n + 300], n)  # (points beyond n are there to be loaded by a kernel that gets n wrong)
            assert got.tobytes() == big[:n].tobytes(), n
        d_points, d_out = _to_device(system, recs[:64]), _out_buffer(system, 66)
        system.project_points_device(d_points.data_ptr(), 0, d_out.data_ptr())
        assert (_read(system, d_out) == SENTINEL).all()
        assert len(system.project_point_records(recs[:0])) == 0


# ---- 3. identity and ties ----------------------------------------------------------------------------------------------------------
def test_engineered_ties_dropped_and_collapsed_triangles():
    """bit-equal squared distances resolve to the analytic collider, the lower index, the lower ORIGINAL triangle; a mesh that lost
    zero-area triangles at creation reports original indices; the collapsed triangles of a deformable mesh do not answer"""
    with _system() as system:
        for name, w, point, kind, index, triangle, dist in P.tie_cases():
            handles = _open(system, w)
            r = system.project_points([point], 1)[0]
            assert (r["kind"], r["index"], r["triangle"], r["distance"]) == (kind, index, triangle, f32(dist)), (name, r)
            assert_projections_equal(np.array([r]), project_ref.project_points(w.colliders, w.instances(), [point], 1), name)
            system.set_mesh_colliders([])
            for h in handles:
                system.destroy_mesh(h)
        w, pts, masks, peak = P.collapsed()
        want = project_ref.project_points([], w.instances(), pts, masks)
        for deformable in (True, False):  # (kept as records with zero edges; dropped at creation)
            _open(system, P.World([], [(w.meshes[0][0], w.meshes[0][1], deformable)], w.placements))
            got = system.project_points(pts, masks)
            assert_projections_equal(got, want, f"collapsed, deformable {deformable}")
        assert not np.isin(got["triangle"], (0, 11)).any() and (got["triangle"] <= 10).any() and (got["triangle"] >= 12).any()
        assert got["distance"][-1] > 2.0  # (the point ON the collapsed triangles is answered by the terrain below)


# ---- 4. stream order ---------------------------------------------------------------------------------------------------------------
def test_queries_see_the_world_of_their_place_in_the_stream():
    """device form, nothing waited for in between: a query, both sets replaced, a query, a device-form vertex update, a query; one
    synchronisation at the end.  Each result is the reference's over the world of its moment, and the third is also that of a static
    mesh created from the new vertices"""
    import torch

    mixed = P.mixed_world()
    gv, gt, _ = mixed.meshes[0]
    gv2 = deform(gv)
    a = P.World(mixed.colliders, [(gv, gt, True), mixed.meshes[1]], mixed.placements[:2])
    b_colliders = [S.Collider.Sphere((2.0, -1.0, 1.0), 1.5), S.Collider.Capsule((-3.0, 0.0, -2.0), 0.5, 2.0, P.TILT)]
    b_place = [(1, (-1.0, 0.5, 1.0), P.ID, 1), (0, (0.0, -1.5, 0.5), P.unit_quat(0.0, 0.2, 0.05, 0.97), 3), (0, (0.0, -2.0, 0.0), P.ID, 1)]
    b = P.World(b_colliders, a.meshes, b_place)
    c = P.World(b_colliders, [(gv2, gt, True), mixed.meshes[1]], b_place)
    pts = P.mixed_points()[::2]
    recs = _records(pts, 0xFFFFFFFF)
    with _system() as system:
        grid, ball = _open(system, a)
        d_points = _to_device(system, recs)
        out = [_out_buffer(system, len(recs)) for _ in range(3)]
        with _ctx_stream(system):
            d_v2 = torch.from_numpy(gv2.copy()).to("cuda")
        system.project_points_device(d_points.data_ptr(), len(recs), out[0].data_ptr())
        system.set_colliders(b.colliders)
        system.set_mesh_colliders([S.MeshCollider((grid, ball)[k], p, q, layers) for k, p, q, layers in b_place])
        system.project_points_device(d_points.data_ptr(), len(recs), out[1].data_ptr())
        system.update_mesh_vertices_device(grid, d_v2.data_ptr(), len(gv2))
        system.project_points_device(d_points.data_ptr(), len(recs), out[2].data_ptr())
        system.synchronize()
        got = [t.cpu().numpy().reshape(-1).view(S.POINT_PROJECTION_DTYPE).copy() for t in out]
        assert system.mesh_update_status(grid) == (1, 0, -1)
        static = system.create_mesh(gv2, gt)
        system.set_mesh_colliders([S.MeshCollider((static, ball)[k], p, q, layers) for k, p, q, layers in b_place])
        anew = system.project_point_records(recs)
    for k, w in enumerate((a, b, c)):
        assert_projections_equal(got[k], project_ref.project_points(w.colliders, w.instances(), pts, 0xFFFFFFFF), f"query {k}")
        assert (got[k]["kind"] == S.HIT_MESH).sum() > 200
    assert got[2].tobytes() == anew.tobytes()
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


# ---- 5. the two forms, errors, the empty world -------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_errors_enqueue_nothing():
    from bevy_firework_amd.system import FwError

    pts = P.mixed_points()
    recs = _records(pts, 0b101)
    none = np.zeros(1, dtype=S.POINT_PROJECTION_DTYPE)
    none["index"] = none["triangle"] = NONE
    with _system() as system:
        empty = system.project_point_records(recs[:1000])  # (no world yet: FW_HIT_NONE a thousand times)
        assert empty.tobytes() == none.tobytes() * 1000
        assert _project_device(system, recs[:1000]).tobytes() == empty.tobytes()
        _open(system, P.mixed_world())
        host = system.project_point_records(recs)
        assert host.tobytes() == _project_device(system, recs).tobytes()
        assert_projections_equal(host, _reference("mixed", 0b101), "host form")
        assert system.project_points(pts, 0b101).tobytes() == host.tobytes()
        # (the host forms of the two queries share their staging: a ray query in between changes nothing)
        assert len(system.cast_rays(pts[:100], np.tile(f32([0, -1, 0]), (100, 1)), 5.0, 1)) == 100
        assert system.project_point_records(recs[:5000]).tobytes() == host[:5000].tobytes()
        d_points, d_out = _to_device(system, recs[:256]), _out_buffer(system, 256)
        for pp, op in ((0, d_out.data_ptr()), (d_points.data_ptr(), 0), (0, 0)):
            with pytest.raises(FwError) as e:
                system.project_points_device(pp, 256, op)
            assert e.value.status == FW_EINVAL
        system.synchronize()
        assert (_read(system, d_out) == SENTINEL).all()
        out = np.full(256, SENTINEL, dtype=np.uint8).repeat(32).view(S.POINT_PROJECTION_DTYPE)
        L, ctx = system._lib, system._ctx
        assert L.fw_ctx_project_points(ctx, None, 256, out.ctypes.data_as(C.c_void_p)) == FW_EINVAL
        assert L.fw_ctx_project_points(ctx, recs.ctypes.data_as(C.c_void_p), 256, None) == FW_EINVAL
        assert (out.view(np.uint8) == SENTINEL).all()
        assert L.fw_ctx_project_points(ctx, None, 0, None) == FW_OK and L.fw_ctx_project_points_device(ctx, None, 0, None) == FW_OK
        assert system.project_point_records(recs[:3000]).tobytes() == host[:3000].tobytes()
        system.set_colliders([])
        system.set_mesh_colliders([])
        assert system.project_point_records(recs[:1000]).tobytes() == empty.tobytes()


# ---- 6. the simulation does not notice ---------------------------------------------------------------------------------------------
def _falling_frames(with_queries):
    v, t = _terrain()
    spawner, _ = _falling_spawner(True)
    tf = S.Transform((0.5, 0.2, -0.3))
    recs = _records(P.mixed_points()[:2000], 0xFFFFFFFF)
    dt = f32(1.0 / 60.0)
    with _system() as system:
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)])
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(v, t))])
        d_points, d_out = _to_device(system, recs), _out_buffer(system, len(recs))
        dead = []
        for fr in range(40):
            system.update(dt)
            dead.append(h.destroyed(0))
            if with_queries:
                system.project_points_device(d_points.data_ptr(), len(recs), d_out.data_ptr())
                if fr % 4 == 0:
                    assert (system.project_point_records(recs)["kind"] != S.HIT_NONE).all()
        return h.particles(0), np.concatenate(dead)


def test_the_simulation_does_not_notice_point_queries(fw_path):
    """a colliding spawner over a mesh world, 40 frames with point queries of both forms between the frames and 40 without: particles
    and destroyed records identical, bit for bit"""
    p0, d0 = _falling_frames(False)
    p1, d1 = _falling_frames(True)
    assert len(p0) > 300 and len(d0) > 100, (len(p0), len(d0))
    assert p0.tobytes() == p1.tobytes() and d0.tobytes() == d1.tobytes()
