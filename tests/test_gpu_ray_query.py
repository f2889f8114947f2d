"""The public ray-cast query (include/firework_hip.h: RAY-CAST QUERIES; fw_ctx_cast_rays / fw_ctx_cast_rays_device): a batch of
rays into the device-resident collider world, nearest hits out.  Distance and normal must equal, bit for bit, the C oracle's
fwo_cast_rays and the numpy brute force (tests/mesh_ref.py) -- the cast a particle runs -- and kind / index / triangle must name
what was hit by the cast's own tie rule (expected values built here from numpy alone: the oracle reports no identity).  Device
buffers are torch tensors.  The autouse fw_path fixture runs every test on the FIFO ring, range ring, compacting and small
paths.  Needs an MI355X."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rays  # noqa: E402
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402
from test_gpu_mesh import SEED, _device_world, _falling_spawner, _particles, _ref_world, _still_settings, _terrain  # noqa: E402
from test_gpu_mesh_deform import deform  # noqa: E402

import oracle  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402
from bevy_firework_amd._ffi import FW_EINVAL, FW_OK  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
MASKS = (0b101, 0b10, 0xFFFFFFFF)  # (those of tests/test_oracle_mesh_cpu.py)
NONE = 0xFFFFFFFF
SENTINEL = 0xA5


# ---- the rays and their references: computed once, shared, read-only ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _world_and_rays():
    """the world of mesh_rays.ray_world() and about 20k of its rays -- every second one of each family (aimed at vertices and
    edges, starting on faces, axis-parallel, grazing, inside the analytic solids) and of 8000 random ones -- as a particle casts
    them: origin = pos, dir = vel / |vel| (numpy float32, as Dir3::new), max_distance = |vel| * dt"""
    meshes, placements, analytic = mesh_rays.ray_world()
    pos, vel, dt = mesh_rays.rays(meshes, placements, n_random=8000)
    pos, vel = pos[::2].copy(), vel[::2].copy()
    ln = np.sqrt(mesh_ref.dot3(vel, vel)).astype(f32)
    d = (vel / ln[:, None]).astype(f32)
    md = (ln * dt).astype(f32)
    assert 15000 < len(pos) < 25000, len(pos)
    for a in (pos, vel, d, md):
        a.setflags(write=False)
    return meshes, placements, analytic, pos, vel, dt, d, md


def _oracle_cast(analytic, mesh_list, placements, mask, o, d, md):
    """fwo_cast_rays over analytic + [(vertices, indices)] placed by placements [(k, position, rotation, layers)]"""
    om = [oracle.OracleMesh(v, t) for v, t in mesh_list]
    got = oracle.cast_rays(analytic, [S.MeshCollider(om[k], p, q, layers) for k, p, q, layers in placements], mask, o, d, md)
    for m in om:
        m.close()
    return got


@functools.lru_cache(maxsize=None)
def _reference(mask):
    """(found, distance, normal) of the shared rays under `mask`: the C oracle's, checked here against the numpy brute force"""
    meshes, placements, analytic, pos, _, _, d, md = _world_and_rays()
    names = list(meshes)
    got = _oracle_cast(analytic, [meshes[n] for n in names], [(names.index(n), p, q, layers) for n, p, q, layers in placements], mask, pos, d, md)
    want = mesh_ref.cast_ray(_ref_world(meshes, placements, analytic), mask, pos, d, md.copy())
    _assert_cast_equal(got, want, f"oracle against numpy, mask {mask:#x}")
    for a in got:
        a.setflags(write=False)
    return got


def _assert_cast_equal(got, want, what):
    (gf, gt, gn), (wf, wt, wn) = got, want
    assert np.array_equal(gf, wf), (what, "found", np.flatnonzero(gf != wf)[:10])
    bad = np.flatnonzero(gf & ~((gt == wt) | (np.isnan(gt) & np.isnan(wt))))
    assert not len(bad), (what, "distance", bad[:10], gt[bad][:3], wt[bad][:3])
    bad = np.flatnonzero(gf & ~((gn == wn) | (np.isnan(gn) & np.isnan(wn))).all(axis=1))
    assert not len(bad), (what, "normal", bad[:10], gn[bad][:3], wn[bad][:3])


def _assert_hits_equal_cast(hits, ref, what):
    """fw_ray_hit records against (found, distance, normal), bit for bit; misses carry the exact miss record"""
    found = hits["kind"] != S.HIT_NONE
    _assert_cast_equal((found, hits["distance"], hits["normal"]), ref, what)
    miss = hits[~found]
    assert (miss["distance"].view(np.uint32) == 0).all() and (miss["normal"].view(np.uint32) == 0).all(), what
    assert (miss["index"] == NONE).all() and (miss["triangle"] == NONE).all(), what
    assert (hits["reserved"] == 0).all() and np.isin(hits["kind"], (S.HIT_NONE, S.HIT_COLLIDER, S.HIT_MESH)).all(), what
    assert (hits["triangle"][hits["kind"] == S.HIT_COLLIDER] == NONE).all(), what


def _ray_records(o, d, md, masks):
    r = np.zeros(len(o), dtype=S.RAY_DTYPE)
    r["origin"], r["dir"], r["max_distance"], r["filter_mask"] = o, d, md, masks
    return r


def _shared_records(masks):
    _, _, _, pos, _, _, d, md = _world_and_rays()
    return _ray_records(pos, d, md, masks)


# ---- the device side -------------------------------------------------------------------------------------------------------
def _ctx_stream(system):
    import torch

    return torch.cuda.stream(torch.cuda.ExternalStream(system.stream))


def _to_device(system, records):
    """ray records in a device tensor written on the context's stream"""
    import torch

    host = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1, 32).copy())
    with _ctx_stream(system):
        return host.to("cuda")


def _hit_buffer(system, n_records):
    import torch

    with _ctx_stream(system):
        return torch.full((n_records, 32), SENTINEL, dtype=torch.uint8, device="cuda")


def _read(system, t):
    """the buffer's bytes, read back in the stream that wrote them"""
    with _ctx_stream(system):
        return t.cpu().numpy()


def _cast_device(system, records, n=None):
    n = len(records) if n is None else n
    d_rays, d_hits = _to_device(system, records), _hit_buffer(system, n + 2)
    system.cast_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr())
    raw = _read(system, d_hits)
    assert (raw[n:] == SENTINEL).all(), "the 64 bytes behind the last hit record were written"
    return raw[:n].reshape(-1).view(S.RAY_HIT_DTYPE).copy()


def _open_ray_world(system):
    meshes, placements, analytic = _world_and_rays()[:3]
    system.set_colliders(analytic)
    return _device_world(system, meshes, placements)


def _system():
    from bevy_firework_amd.system import ParticleSystem

    return ParticleSystem(device=0, seed=SEED)


# ---- 1. the cast ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
def test_query_casts_are_bit_exact(fw_path, mask):
    """about 20k rays into the world of mesh_rays.ray_world(): found, distance and normal equal fwo_cast_rays and mesh_ref.cast_ray
    bit for bit (NaN equals NaN), misses carry the exact miss record; thousands hit and thousands miss"""
    ref = _reference(mask)
    with _system() as system:
        _open_ray_world(system)
        hits = _cast_device(system, _shared_records(mask))
    _assert_hits_equal_cast(hits, ref, f"mask {mask:#x}")
    n_hit = int((hits["kind"] != S.HIT_NONE).sum())
    print(f"mask {mask:#x}: {n_hit} of {len(hits)} rays hit, {int((hits['kind'] == S.HIT_MESH).sum())} of them a mesh")
    if mask == 0b10:  # (layer 2 holds one icosphere: few rays reach it)
        assert n_hit > 20 and len(hits) - n_hit > 2000
    else:
        assert n_hit > 2000 and len(hits) - n_hit > 2000, n_hit
        assert (hits["kind"] == S.HIT_MESH).sum() > 1000 and (hits["kind"] == S.HIT_COLLIDER).sum() > 1000
        assert ((hits["kind"] != S.HIT_NONE) & (hits["distance"] == 0)).sum() > 100  # (rays that start inside a solid)


# ---- 2. launch sizes ----------------------------------------------------------------------------------------------------------
def test_query_sizes_around_the_wave_and_the_workgroup(fw_path):
    """n in {1, 63, 64, 65, 255, 256, 257, 1000}, each a prefix of the same rays: the prefix of the large batch's result, the 64
    bytes behind the last record untouched; n = 0 leaves the whole buffer untouched"""
    rays = _shared_records(MASKS[2])
    with _system() as system:
        _open_ray_world(system)
        big = _cast_device(system, rays[:4096])
        assert (big["kind"] != S.HIT_NONE).sum() > 300
        for n in (1, 63, 64, 65, 255, 256, 257, 1000):
            got = _cast_device(system, rays[:n + 300], n)  # (rays beyond n are there to be loaded by a kernel that gets n wrong)
            assert got.tobytes() == big[:n].tobytes(), n
        d_rays, d_hits = _to_device(system, rays[:64]), _hit_buffer(system, 66)
        system.cast_rays_device(d_rays.data_ptr(), 0, d_hits.data_ptr())
        assert (_read(system, d_hits) == SENTINEL).all()
        assert len(system.cast_ray_records(rays[:0])) == 0


# ---- 3. masks mixed inside a wave ---------------------------------------------------------------------------------------------
def test_query_masks_mixed_inside_a_wave(fw_path):
    """the three masks and mask 0 dealt out ray by ray (every wave holds all four; then in runs of 5, so that the lanes that take part
    change from wave to wave): each ray equals the uniform-mask result for its mask, mask-0 rays miss"""
    n = len(_shared_records(0))
    cycle = np.array(MASKS + (0,), dtype=np.uint32)
    for deal in (np.arange(n) % 4, (np.arange(n) // 5) % 4):
        masks = cycle[deal]
        with _system() as system:
            _open_ray_world(system)
            hits = _cast_device(system, _shared_records(masks))
            uniform = {m: _cast_device(system, _shared_records(m)) for m in MASKS}
        for k, m in enumerate(MASKS):
            sel = deal == k
            ref = tuple(a[sel] for a in _reference(m))
            _assert_hits_equal_cast(hits[sel], ref, f"mixed, mask {m:#x}")
            assert hits[sel].tobytes() == uniform[m][sel].tobytes(), f"identity under mixed masks, mask {m:#x}"
        zero = hits[deal == 3]
        assert len(zero) > 1000 and (zero["kind"] == S.HIT_NONE).all() and (zero["index"] == NONE).all()
        assert (hits[deal != 3]["kind"] != S.HIT_NONE).sum() > 3000


# ---- 4. identity ----------------------------------------------------------------------------------------------------------------
def _dot(a, b):  # the header's: (a.x b.x + a.y b.y) + a.z b.z
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32)).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)


def _cross(a, b):  # the header's: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)
    return np.stack([(a[..., 1] * b[..., 2]).astype(f32) - (b[..., 1] * a[..., 2]).astype(f32),
                     (a[..., 2] * b[..., 0]).astype(f32) - (b[..., 2] * a[..., 0]).astype(f32),
                     (a[..., 0] * b[..., 1]).astype(f32) - (b[..., 0] * a[..., 1]).astype(f32)], axis=-1).astype(f32)


def _moller_trumbore(o, d, v0, e1, e2, md):
    """the header's TRIANGLE, operation by operation, broadcasting rays against triangles -> (hit, t)"""
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        det = _dot(e1, p).astype(f32)
        inv = (f32(1.0) / det).astype(f32)
        s = (o - v0).astype(f32)
        u = (_dot(s, p).astype(f32) * inv).astype(f32)
        q = _cross(s, e1)
        v = (_dot(d, q).astype(f32) * inv).astype(f32)
        t = (_dot(e2, q).astype(f32) * inv).astype(f32)
        # WATERTIGHT: the margin 8 * 2^-24 |s|_1 (|e1|_1 + |e2|_1) / |det|, at most 2^-8
        a1 = lambda a: ((np.abs(a[..., 0]) + np.abs(a[..., 1])).astype(f32) + np.abs(a[..., 2])).astype(f32)  # noqa: E731
        m = np.fmin((((f32(2.0 ** -21) * a1(s)).astype(f32) * (a1(e1) + a1(e2)).astype(f32)).astype(f32) * np.abs(inv)).astype(f32), f32(2.0 ** -8))
        hit = (det != 0) & (u >= -m) & (v >= -m) & ((u + v).astype(f32) <= (f32(1.0) + m).astype(f32)) & (t >= 0) & (t <= md)
    return hit, t


def _into_frame(o, d, position, rotation):
    """the header's FRAME: o = R^-1 (origin - position), d = R^-1 dir; the identity rotation skips both products"""
    q = np.asarray(rotation, dtype=f32)
    ol = (o - np.asarray(position, dtype=f32)).astype(f32)
    if q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1:
        return ol, d
    qi = np.broadcast_to(np.array([-q[0], -q[1], -q[2], q[3]], dtype=f32), (len(o), 4))
    return np_sim.quat_mul_vec3(qi, ol), np_sim.quat_mul_vec3(qi, d)


def _expected_identity(analytic, instances, mask, o, d, md):
    """(kind, index, distance): every analytic collider and every instance cast ALONE, the first strict minimum in the order
    analytic 0.., instance 0.. -- the tie rule, from numpy alone"""
    n = len(o)
    kind, index = np.zeros(n, dtype=np.int32), np.full(n, NONE, dtype=np.uint32)
    best = np.full(n, np.inf, dtype=f32)
    found = np.zeros(n, dtype=bool)
    alone = [(S.HIT_COLLIDER, i, c.layers, lambda c=c: np_sim.cast_ray([c], 0xFFFFFFFF, o, d, md.copy())[:2]) for i, c in enumerate(analytic)]
    alone += [(S.HIT_MESH, i, inst.layers, lambda inst=inst: mesh_ref.cast_instance(inst, o, d, md)[:2]) for i, inst in enumerate(instances)]
    for k, i, layers, cast in alone:
        if not (int(layers) & int(mask)):
            continue
        hit, t = cast()
        better = hit & (~found | (t < best))
        kind[better], index[better], best[better] = k, i, t[better]
        found |= hit
    return kind, index, np.where(found, best, f32(0)).astype(f32)


def _assert_identity(hits, analytic, instances, mask, o, d, md, what):
    kind, index, dist = _expected_identity(analytic, instances, mask, o, d, md)
    assert np.array_equal(hits["kind"], kind), (what, "kind", np.flatnonzero(hits["kind"] != kind)[:10])
    assert np.array_equal(hits["index"], index), (what, "index", np.flatnonzero(hits["index"] != index)[:10])
    assert hits["distance"].tobytes() == dist.tobytes(), (what, "distance")
    # the reported triangle, evaluated ALONE, reproduces the distance exactly -- and is the lowest original index that does
    for i, inst in enumerate(instances):
        sel = np.flatnonzero((hits["kind"] == S.HIT_MESH) & (hits["index"] == i))
        if not len(sel):
            continue
        m = inst.mesh
        ol, dl = _into_frame(o[sel], d[sel], inst.position, inst.rotation)
        tri = hits["triangle"][sel].astype(np.int64)
        assert np.isin(tri, m.orig).all(), (what, i, "a triangle the mesh does not keep")
        k = np.searchsorted(m.orig, tri)
        hit, t = _moller_trumbore(ol, dl, m.v0[k], m.e1[k], m.e2[k], md[sel])
        assert hit.all() and t.tobytes() == hits["distance"][sel].tobytes(), (what, i, "the reported triangle alone")
        hit_all, t_all = _moller_trumbore(ol[:, None, :], dl[:, None, :], m.v0[None], m.e1[None], m.e2[None], md[sel][:, None])
        first = np.argmax(hit_all & (t_all == hits["distance"][sel][:, None]), axis=1)
        assert np.array_equal(m.orig[first], tri), (what, i, "not the lowest original triangle at that distance")


@pytest.mark.parametrize("mask", [0xFFFFFFFF, 0b101])
def test_query_identity_follows_the_tie_rule(fw_path, mask):
    """a few thousand rays: kind and index are the first strict minimum over the colliders and instances cast alone, the triangle
    reproduces the distance"""
    meshes, placements, analytic, pos, _, _, d, md = _world_and_rays()
    o, d, md = pos[::5], d[::5], md[::5]
    world = _ref_world(meshes, placements, analytic)
    with _system() as system:
        _open_ray_world(system)
        hits = system.cast_rays(o, d, md, mask)
    assert len(hits) > 3000 and (hits["kind"] == S.HIT_MESH).sum() > 300 and (hits["kind"] == S.HIT_COLLIDER).sum() > 300
    assert len(set(hits["index"][hits["kind"] == S.HIT_MESH].tolist())) >= 3
    _assert_identity(hits, analytic, world.instances, mask, o, d, md, f"mask {mask:#x}")


def test_query_identity_on_engineered_ties_and_dropped_triangles(fw_path):
    """mesh_ref.tie_meshes(): equal distances resolve to the analytic collider, the lower instance, the lower original triangle;
    a mesh that lost zero-area triangles at creation still reports ORIGINAL indices"""
    tilted, flat, tilted_first, flat_first = mesh_ref.tie_meshes()
    o = np.array([[0.0, 1.0, -0.5]], dtype=f32)
    d = np.array([[0.0, -1.0, 0.0]], dtype=f32)
    md = np.array([5.0], dtype=f32)
    plane = S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    up = np.array([0, 1, 0], dtype=f32)
    #        analytic  meshes           kind            index triangle  normal (None: the tilted triangle's)
    cases = [([plane], [tilted], S.HIT_COLLIDER, 0, NONE, up), ([], [tilted, flat], S.HIT_MESH, 0, 0, None),
             ([], [flat, tilted], S.HIT_MESH, 0, 0, up), ([], [tilted_first], S.HIT_MESH, 0, 0, None),
             ([], [flat_first], S.HIT_MESH, 0, 0, up), ([], [flat, flat], S.HIT_MESH, 0, 0, up)]
    gv, gt = mesh_ref.grid_mesh(4, 4, extent=2.0, height=lambda x, z: 0.1 * x * z)
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], dtype=f32)
    n0 = len(gv)
    dropped = (np.concatenate([gv, line]), np.concatenate([[[0, 0, 1], [n0, n0 + 1, n0 + 2]], gt[:10], [[n0 + 2, n0 + 1, n0]], gt[10:]]).astype(np.uint32))
    rng = np.random.default_rng(3)
    go = np.stack([rng.uniform(-1.9, 1.9, 600), np.full(600, 2.0), rng.uniform(-1.9, 1.9, 600)], 1).astype(f32)
    gd = np.broadcast_to(np.array([0.0, -1.0, 0.0], dtype=f32), go.shape).copy()
    gmd = np.full(600, 5.0, dtype=f32)
    with _system() as system:
        for k, (analytic, ms, kind, index, triangle, normal) in enumerate(cases):
            system.set_colliders(analytic)
            hs = [system.create_mesh(v, t) for v, t in ms]
            system.set_mesh_colliders([S.MeshCollider(m) for m in hs])
            h = system.cast_rays(o, d, md, 1)[0]
            assert (h["kind"], h["index"], h["triangle"], h["distance"]) == (kind, index, triangle, 1.0), (k, h)
            if normal is None:
                assert np.allclose(h["normal"], mesh_ref.TILTED_N, atol=1e-6) and h["normal"][0] < 0, (k, h)
            else:
                assert (h["normal"] == normal).all(), (k, h)
            system.set_mesh_colliders([])
            for m in hs:
                system.destroy_mesh(m)
        system.set_colliders([])
        whole, lossy = system.create_mesh(gv, gt), system.create_mesh(*dropped)
        system.set_mesh_colliders([S.MeshCollider(whole)])
        a = system.cast_rays(go, gd, gmd, 1)
        system.set_mesh_colliders([S.MeshCollider(lossy)])
        b = system.cast_rays(go, gd, gmd, 1)
    assert (a["kind"] == S.HIT_MESH).all() and a["distance"].tobytes() == b["distance"].tobytes() and a["normal"].tobytes() == b["normal"].tobytes()
    want = np.where(a["triangle"] < 10, a["triangle"] + 2, a["triangle"] + 3)  # (two dropped in front, a third behind the first ten)
    assert np.array_equal(b["triangle"], want) and (a["triangle"] < 10).any() and (a["triangle"] >= 10).any()
    _assert_identity(b, [], [mesh_ref.Instance(mesh_ref.Mesh(*dropped))], 1, go, gd, gmd, "dropped triangles")


# ---- 5. stream order -------------------------------------------------------------------------------------------------------------
def test_queries_see_the_world_of_their_place_in_the_stream(fw_path):
    """device form, nothing waited for in between: a query, then both sets replaced, a query, then a device-form vertex update, a
    query; one synchronisation at the end.  Each result is the oracle's over the world of its moment, and the third also that of a
    static mesh created from the new vertices"""
    import torch

    meshes, placements, analytic, pos, _, _, d, md = _world_and_rays()
    rays = _shared_records(0xFFFFFFFF)[::4]
    o, dd, mdd = pos[::4], d[::4], md[::4]
    gv, gt = meshes["grid"]
    gv2 = deform(gv)
    a_inst = [(0, (0.0, -2.0, 0.0), (0.0, 0.0, 0.0, 1.0), 1), (1, (3.5, 0.0, -1.0), mesh_rays.unit_quat(0.5, -0.1, 0.2, 0.8), 1)]
    b_inst = [(1, (-1.0, 0.5, 1.0), (0.0, 0.0, 0.0, 1.0), 1), (0, (0.0, -1.5, 0.5), mesh_rays.unit_quat(0.0, 0.2, 0.05, 0.97), 3),
              (0, (0.0, -2.0, 0.0), (0.0, 0.0, 0.0, 1.0), 1)]
    a_analytic, b_analytic = analytic, [S.Collider.Sphere((2.0, -1.0, 1.0), 1.5), S.Collider.Box((-3.0, 0.0, -2.0), (1.0, 2.0, 1.0), mesh_rays.unit_quat(0.0, 0.3, 0.1, 0.9))]
    ico = meshes["ico"]
    with _system() as system:
        grid = system.create_deformable_mesh(gv, gt)
        ball = system.create_mesh(*ico)
        hs = (grid, ball)
        system.set_colliders(a_analytic)
        system.set_mesh_colliders([S.MeshCollider(hs[k], p, q, layers) for k, p, q, layers in a_inst])
        d_rays = _to_device(system, rays)
        out = [_hit_buffer(system, len(rays)) for _ in range(3)]
        with _ctx_stream(system):
            d_v2 = torch.from_numpy(gv2.copy()).to("cuda")
        system.cast_rays_device(d_rays.data_ptr(), len(rays), out[0].data_ptr())
        system.set_colliders(b_analytic)
        system.set_mesh_colliders([S.MeshCollider(hs[k], p, q, layers) for k, p, q, layers in b_inst])
        system.cast_rays_device(d_rays.data_ptr(), len(rays), out[1].data_ptr())
        system.update_mesh_vertices_device(grid, d_v2.data_ptr(), len(gv2))
        system.cast_rays_device(d_rays.data_ptr(), len(rays), out[2].data_ptr())
        system.synchronize()
        got = [t.cpu().numpy().reshape(-1).view(S.RAY_HIT_DTYPE).copy() for t in out]
        assert system.mesh_update_status(grid) == (1, 0, -1)
        static = system.create_mesh(gv2, gt)
        system.set_mesh_colliders([S.MeshCollider((static, ball)[k], p, q, layers) for k, p, q, layers in b_inst])
        anew = system.cast_ray_records(rays)
    worlds = [(a_analytic, [(gv, gt), ico], a_inst), (b_analytic, [(gv, gt), ico], b_inst), (b_analytic, [(gv2, gt), ico], b_inst)]
    for k, (an, ml, inst) in enumerate(worlds):
        _assert_hits_equal_cast(got[k], _oracle_cast(an, ml, inst, 0xFFFFFFFF, o, dd, mdd), f"query {k}")
        assert (got[k]["kind"] != S.HIT_NONE).sum() > 500
    assert got[2].tobytes() == anew.tobytes()
    assert got[0].tobytes() != got[1].tobytes() and got[1].tobytes() != got[2].tobytes()


# ---- 6. the two forms, errors, the empty world ------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_errors_enqueue_nothing(fw_path):
    from bevy_firework_amd.system import FwError

    rays = _shared_records(0b101)
    with _system() as system:
        empty = system.cast_ray_records(rays[:1000])  # (no world yet: the exact miss record, a thousand times)
        miss = np.zeros(1, dtype=S.RAY_HIT_DTYPE)
        miss["index"] = miss["triangle"] = NONE
        assert empty.tobytes() == miss.tobytes() * 1000
        assert _cast_device(system, rays[:1000]).tobytes() == empty.tobytes()
        _open_ray_world(system)
        host = system.cast_ray_records(rays)
        assert host.tobytes() == _cast_device(system, rays).tobytes()
        _assert_hits_equal_cast(host, _reference(0b101), "host form")
        by_arrays = system.cast_rays(rays["origin"], rays["dir"], rays["max_distance"], 0b101)
        assert by_arrays.tobytes() == host.tobytes()
        # null pointers: FW_EINVAL, and the buffers that were passed stay as they are
        d_rays, d_hits = _to_device(system, rays[:256]), _hit_buffer(system, 256)
        for rp, hp in ((0, d_hits.data_ptr()), (d_rays.data_ptr(), 0), (0, 0)):
            with pytest.raises(FwError) as e:
                system.cast_rays_device(rp, 256, hp)
            assert e.value.status == FW_EINVAL
        system.synchronize()
        assert (_read(system, d_hits) == SENTINEL).all()
        out = np.full(256, SENTINEL, dtype=np.uint8).repeat(32).view(S.RAY_HIT_DTYPE)
        L, ctx = system._lib, system._ctx
        assert L.fw_ctx_cast_rays(ctx, None, 256, out.ctypes.data_as(C.c_void_p)) == FW_EINVAL
        assert L.fw_ctx_cast_rays(ctx, rays.ctypes.data_as(C.c_void_p), 256, None) == FW_EINVAL
        assert (out.view(np.uint8) == SENTINEL).all()
        assert L.fw_ctx_cast_rays(ctx, None, 0, None) == FW_OK and L.fw_ctx_cast_rays_device(ctx, None, 0, None) == FW_OK
        # ... and the next query is right
        assert system.cast_ray_records(rays[:3000]).tobytes() == host[:3000].tobytes()
        system.set_colliders([])
        system.set_mesh_colliders([])
        assert system.cast_ray_records(rays[:1000]).tobytes() == empty.tobytes()


# ---- 7. the simulation does not notice ----------------------------------------------------------------------------------------------
def _falling_frames(with_queries):
    v, t = _terrain()
    spawner, _ = _falling_spawner(True)
    tf = S.Transform((0.5, 0.2, -0.3))  # (just above the terrain: what goes up slowly is back down, and destroyed, within the 40 frames)
    rays = _shared_records(0xFFFFFFFF)[:2000]
    dt = f32(1.0 / 60.0)
    with _system() as system:
        h = system.spawn(spawner, tf, uid=3)
        system.set_colliders([S.Collider.Sphere((2.0, -0.5, 1.0), 0.6)])
        system.set_mesh_colliders([S.MeshCollider(system.create_mesh(v, t))])
        d_rays, d_hits = _to_device(system, rays), _hit_buffer(system, len(rays))
        dead = []
        for fr in range(40):
            system.update(dt)
            dead.append(h.destroyed(0))
            if with_queries:
                system.cast_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
                if fr % 4 == 0:
                    assert (system.cast_ray_records(rays)["kind"] != S.HIT_NONE).sum() > 100
        return h.particles(0), np.concatenate(dead)


def test_the_simulation_does_not_notice_queries(fw_path):
    """a colliding spawner over a mesh world, 40 frames with queries of both forms between the frames and 40 without: particles and
    destroyed records identical, bit for bit"""
    p0, d0 = _falling_frames(False)
    p1, d1 = _falling_frames(True)
    assert len(p0) > 300 and len(d0) > 100, (len(p0), len(d0))
    assert p0.tobytes() == p1.tobytes() and d0.tobytes() == d1.tobytes()


# ---- 8. one cast for particles and queries --------------------------------------------------------------------------------------------
def test_particles_and_queries_run_one_cast(fw_path):
    """the one-step particle set-up of the cast test: a particle whose query misses ends at pos + vel * dt, one whose query hits at
    distance > 0 has left that line"""
    meshes, placements, analytic, pos, vel, dt, d, md = _world_and_rays()
    spawner = _still_settings(capacity=1 << 15)
    spawner.particle_settings[0].collision_settings = S.ParticleCollisionSettings(0.6, 0.3, False, 0b101)
    with _system() as system:
        h = system.spawn(spawner, uid=1)
        _open_ray_world(system)
        hits = system.cast_rays(pos, d, md, 0b101)
        h.write_particles(0, _particles(pos, vel))
        system.update(dt)
        got = h.particles(0)
    straight = (pos + (vel * dt).astype(f32)).astype(f32)
    on_line = (got["position"] == straight).all(axis=1)
    miss = hits["kind"] == S.HIT_NONE
    bounced = ~miss & (hits["distance"] > 0)
    assert miss.sum() > 2000 and bounced.sum() > 2000
    assert on_line[miss].all(), np.flatnonzero(miss & ~on_line)[:10]
    assert (got["velocity"][miss] == vel[miss]).all()
    assert not on_line[bounced].any(), np.flatnonzero(bounced & on_line)[:10]
