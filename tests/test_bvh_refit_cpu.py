"""Deformable collider meshes without a GPU: the builder's deformable entry (bevy_firework_amd/csrc/fw_bvh.cpp) and the refit
arithmetic the kernel runs per node (csrc/fw_refit.h), both compiled here with g++, against the static build, the brute-force
numpy reference (tests/mesh_ref.py) and the numpy replay of the device's walk (tests/test_bvh_cpu.py: device_walk)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
import test_bvh_cpu as static  # noqa: E402
from test_bvh_cpu import _rays, device_walk, lib, random_soup, u32  # noqa: E402,F401  (lib: the static builder's fixture)

f32 = np.float32
WRAPPER = r"""
#include "fw_bvh.h"
#include "fw_refit.h"
#include <cstring>
extern "C" int bvh_build_deformable(const float *xyz, uint32_t nv, const uint32_t *idx, uint32_t nt, float *nodes, float *tris,
                                    uint32_t *slots, int32_t *parent, uint32_t *order, uint32_t *level_off, uint32_t *counts,
                                    float *box_pad, char *err, uint32_t err_cap) {
    FwBvh b;
    std::string e;
    const int r = fw_bvh_build_deformable(xyz, nv, idx, nt, &b, &e);
    strncpy(err, e.c_str(), err_cap - 1);
    if (r) return r;
    counts[0] = b.n_nodes, counts[1] = b.n_tris, counts[2] = (uint32_t)b.level_off.size();
    if (b.n_nodes > 2 * nt || b.n_tris != nt || b.level_off.size() > 2 * (size_t)nt + 2) return -9;
    if (b.slots.size() != 4 * (size_t)nt || b.parent.size() != b.n_nodes || b.order.size() != b.n_nodes) return -8;
    memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(float));
    memcpy(tris, b.tris.data(), b.tris.size() * sizeof(float));
    memcpy(slots, b.slots.data(), b.slots.size() * sizeof(uint32_t));
    memcpy(parent, b.parent.data(), b.parent.size() * sizeof(int32_t));
    memcpy(order, b.order.data(), b.order.size() * sizeof(uint32_t));
    memcpy(level_off, b.level_off.data(), b.level_off.size() * sizeof(uint32_t));
    for (int k = 0; k < 3; k++) box_pad[k] = b.lo[k], box_pad[3 + k] = b.hi[k];
    box_pad[6] = b.pad;
    return 0;
}
// the kernel's work, one node after the other in the schedule's order (fw_k_refit.hip runs a level's nodes side by side)
extern "C" void bvh_refit(float *nodes, float *tris, const uint32_t *slots, const float *xyz, const uint32_t *order,
                          uint32_t n_nodes, float pad) {
    static_assert(sizeof(FwR4) == 16 && sizeof(FwSlotIdx) == 16, "layout");
    FwRefit R{reinterpret_cast<FwR4 *>(nodes), reinterpret_cast<FwR4 *>(tris), reinterpret_cast<const FwSlotIdx *>(slots), xyz, order, pad};
    for (uint32_t j = 0; j < n_nodes; j++) fw_refit_node(R, order[j]);
}
extern "C" void bvh_bounds(const float *xyz, const uint8_t *referenced, uint32_t nv, float *box_pad) {
    fw_bvh_bounds(xyz, referenced, nv, box_pad, box_pad + 3, box_pad + 6);
}
"""
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def rlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "librefit.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(CSRC, "fw_bvh.cpp"), str(d / "wrap.cpp"), "-o", str(so)])
    return C.CDLL(str(so))


class Tables:
    pass


def _aligned(shape, dtype):
    """(the refit reads and writes 16-byte records)"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n].view(dtype).reshape(shape)


def build_deformable(rlib, v, t):
    v = np.ascontiguousarray(v, dtype=f32).reshape(-1, 3)
    t = np.ascontiguousarray(t, dtype=np.uint32).reshape(-1, 3)
    nt = max(len(t), 1)
    T = Tables()
    T.v, T.t = v, t
    nodes, tris, slots = _aligned((2 * nt, 8), f32), _aligned((nt, 12), f32), _aligned((nt, 4), np.uint32)
    parent, order = np.zeros(2 * nt, dtype=np.int32), np.zeros(2 * nt, dtype=np.uint32)
    level_off = np.zeros(2 * nt + 2, dtype=np.uint32)
    counts, box_pad = np.zeros(3, dtype=np.uint32), np.zeros(7, dtype=f32)
    err = C.create_string_buffer(256)
    r = rlib.bvh_build_deformable(P(v), C.c_uint32(len(v)), P(t), C.c_uint32(len(t)), P(nodes), P(tris), P(slots), P(parent), P(order),
                                  P(level_off), P(counts), P(box_pad), err, C.c_uint32(256))
    if r:
        return r, err.value.decode(), None
    n = int(counts[0])
    T.nodes, T.tris, T.slots = nodes[:n], tris, slots
    T.parent, T.order, T.level_off = parent[:n], order[:n], level_off[:counts[2]]
    T.lo, T.hi, T.pad = box_pad[0:3].copy(), box_pad[3:6].copy(), f32(box_pad[6])
    T.referenced = np.zeros(len(v), dtype=np.uint8)
    T.referenced[t.astype(np.int64).ravel()] = 1
    return 0, "", T


def refit(rlib, T, v_new):
    """-> (nodes, tris) of T refitted to v_new, as fw_ctx_update_mesh_vertices does it: the host's bounds and pad, then every node"""
    v_new = np.ascontiguousarray(v_new, dtype=f32).reshape(-1, 3)
    assert v_new.shape == T.v.shape
    box_pad = np.zeros(7, dtype=f32)
    rlib.bvh_bounds(P(v_new), P(T.referenced), C.c_uint32(len(v_new)), P(box_pad))
    nodes, tris = _aligned(T.nodes.shape, f32), _aligned(T.tris.shape, f32)
    nodes[:], tris[:] = T.nodes, T.tris
    rlib.bvh_refit(P(nodes), P(tris), P(T.slots), P(v_new), P(T.order), C.c_uint32(len(nodes)), C.c_float(box_pad[6]))
    return nodes, tris, box_pad


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def check_tables(v, t, T, nodes, tris):
    """the invariants of a deformable mesh's tables over the vertices v: every original triangle in exactly one slot with its
    vertices; live records equal mesh_ref.Mesh's, the dropped set is its complement and marked e1 = e2 = 0; escapes as in the
    static build; every box holds its triangles' vertices (dropped ones too) and its children"""
    v = np.asarray(v, dtype=f32)
    ref = mesh_ref.Mesh(v, t)
    n_nodes = len(nodes)
    orig = u32(tris[:, 3])
    assert sorted(orig.tolist()) == list(range(len(t)))
    assert np.array_equal(T.slots[:, 3], orig) and np.array_equal(T.slots[:, 0:3], t[orig.astype(np.int64)])
    assert np.array_equal(u32(tris[:, 7]), np.zeros(len(t), np.uint32)) and np.array_equal(u32(tris[:, 11]), np.zeros(len(t), np.uint32))
    live = np.isin(orig, ref.orig)
    pos = {o: k for k, o in enumerate(ref.orig.tolist())}
    k = np.array([pos[o] for o in orig[live].tolist()], dtype=np.int64)
    assert same_bits(tris[live, 0:3], ref.v0[k]) and same_bits(tris[live, 4:7], ref.e1[k]) and same_bits(tris[live, 8:11], ref.e2[k])
    dead = tris[~live]
    assert (u32(dead[:, 4:7]) == 0).all() and (u32(dead[:, 8:11]) == 0).all()  # (+0.0: what no ray hits)
    assert same_bits(dead[:, 0:3], v[t[orig[~live].astype(np.int64), 0].astype(np.int64)])
    esc, leaf = u32(nodes[:, 3]), u32(nodes[:, 7])
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    assert (esc > np.arange(n_nodes)).all() and esc[0] == n_nodes
    covered = np.zeros(len(tris), dtype=np.int64)
    for i in range(n_nodes):
        if leaf[i]:
            first, cnt = int(leaf[i] >> 4), int(leaf[i] & 15)
            assert 1 <= cnt <= 8 and esc[i] == i + 1
            covered[first:first + cnt] += 1
            p = v[T.slots[first:first + cnt, 0:3].astype(np.int64)].reshape(-1, 3)
            assert (p >= lo[i]).all() and (p <= hi[i]).all(), i
        else:
            a, b = i + 1, int(esc[i + 1])
            assert b < esc[i] and esc[b] == esc[i]
            assert T.parent[a] == i and T.parent[b] == i
            for c in (a, b):
                assert (lo[c] >= lo[i]).all() and (hi[c] <= hi[i]).all(), (i, c)
    assert (covered == 1).all() and T.parent[0] == -1
    return ref, live


def check_schedule(T):
    """order: every node once, by height; an interior node's children on lower levels; level sizes never grow"""
    n = len(T.nodes)
    assert sorted(T.order.tolist()) == list(range(n))
    assert T.level_off[0] == 0 and T.level_off[-1] == n
    sizes = np.diff(T.level_off.astype(np.int64))
    assert (sizes > 0).all() and (np.diff(sizes) <= 0).all()
    level = np.zeros(n, dtype=np.int64)
    for h in range(len(sizes)):
        level[T.order[T.level_off[h]:T.level_off[h + 1]]] = h
    esc, leaf = u32(T.nodes[:, 3]), u32(T.nodes[:, 7])
    assert ((leaf != 0) == (level == 0)).all()
    inner = np.flatnonzero(leaf == 0)
    a, b = inner + 1, esc[inner + 1].astype(np.int64)
    assert (level[inner] == np.maximum(level[a], level[b]) + 1).all()


# ---- the meshes and their deformations ---------------------------------------------------------------------------------------
def waving_grid(phase, cells=48, extent=3.0):
    return mesh_ref.grid_mesh(cells, cells, extent=extent, height=lambda x, z: 0.35 * np.sin(1.7 * x + phase) * np.cos(1.2 * z - 0.5 * phase) + 0.1 * phase)


def squashed_ico(subdiv=3, radius=2.0):
    """an icosphere whose cap (y > 0.6 r) is pulled into one point: the triangles with two or three vertices there collapse"""
    v, t = mesh_ref.icosphere(subdiv, radius)
    w = v.copy()
    w[v[:, 1] > 0.6 * radius] = (0.0, 0.6 * radius, 0.0)
    w[:, 1] *= f32(0.7)
    return v, w.astype(f32), t


def pinched_grid(cells=24, extent=3.0):
    """a height field created with a patch of its vertices in ONE point (degenerate at creation), and the vertices that open it"""
    v, t = mesh_ref.grid_mesh(cells, cells, extent=extent, height=lambda x, z: 0.3 * np.cos(x) * np.sin(1.5 * z))
    w = v.copy()
    patch = (np.abs(v[:, 0]) < 1.0) & (np.abs(v[:, 2] - 0.5) < 1.2)
    w[patch] = (0.0, 0.25, 0.5)
    return w.astype(f32), v, t


def deformations():
    rng = np.random.default_rng(21)
    gv, gt = waving_grid(0.0)
    sv, st = random_soup(rng, 1500)
    iv, iw, it = squashed_ico()
    pv, pw, pt = pinched_grid()
    return {"grid": (gv, waving_grid(1.3)[0], gt),
            "soup": (sv, (sv + rng.normal(scale=0.4, size=sv.shape)).astype(f32), st),
            "ico": (iv, iw, it),
            "reopen": (pv, pw, pt)}


def ray_families(rng, v, t, n=6000):
    """the families of test_device_walk_culls_nothing_the_brute_force_hits: random, at vertices and edge midpoints, grazing,
    axis-parallel"""
    o, d = _rays(rng, n, np.zeros(3), 4.0)
    tri = v[t.astype(np.int64)].astype(np.float64)
    aims = np.concatenate([v.astype(np.float64), 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2])])
    aims = aims[rng.integers(0, len(aims), n)]
    back = rng.uniform(0.05, 2.0, (n, 1))
    d2 = rng.normal(size=(n, 3))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    o2 = aims - d2 * back
    g = np.stack([rng.normal(size=n), rng.uniform(-1e-3, 1e-3, n), rng.normal(size=n)], 1)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    o3 = np.stack([rng.uniform(-3, 3, n), rng.uniform(-0.25, 0.25, n), rng.uniform(-3, 3, n)], 1)
    ax = np.zeros((n, 3))
    ax[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    O = np.concatenate([o, o2, o3, rng.uniform(-4, 4, (n, 3))]).astype(f32)
    D = np.concatenate([d, d2, g, ax]).astype(f32)
    return O, D, rng.uniform(0.1, 6.0, len(O)).astype(f32)


# ---- tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["soup1", "soup1000", "grid", "ico", "degenerate", "reopen"])
def test_deformable_build_keeps_every_triangle(rlib, kind):
    if kind.startswith("soup"):
        v, t = random_soup(np.random.default_rng(4), int(kind[4:]))
    elif kind == "grid":
        v, t = waving_grid(0.0, cells=64)
    elif kind == "ico":
        v, t = mesh_ref.icosphere(3, 2.0)
    elif kind == "reopen":
        v, _, t = pinched_grid()
    else:  # duplicated triangles with collinear and repeated-vertex ones mixed in (tests/test_bvh_cpu.py's)
        bv, bt = mesh_ref.box_mesh((1.0, 1.0, 1.0))
        v = np.concatenate([bv, np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], dtype=f32)])
        t = np.concatenate([bt, [[8, 9, 10], [0, 0, 1]], bt] * 5, axis=0).astype(np.uint32)
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0, err
    ref, live = check_tables(v, t, T, T.nodes, T.tris)
    check_schedule(T)
    assert live.sum() == len(ref.orig)
    if kind in ("degenerate", "reopen"):
        assert 0 < live.sum() < len(t)


@pytest.mark.parametrize("kind", ["soup", "grid", "ico"])
def test_deformable_build_equals_the_static_build_without_degenerates(lib, rlib, kind):
    v, t = {"soup": lambda: random_soup(np.random.default_rng(8), 700), "grid": lambda: waving_grid(0.4, cells=40),
            "ico": lambda: mesh_ref.icosphere(3, 1.5)}[kind]()
    r, err, nodes, tris = static.build(lib, v, t)
    assert r == 0, err
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0, err
    assert same_bits(T.nodes, nodes) and same_bits(T.tris, tris)


def test_deformable_build_rejects_what_the_static_build_rejects(rlib):
    v, t = mesh_ref.box_mesh((1.0, 1.0, 1.0))
    assert build_deformable(rlib, v, t[:0])[0] == -1
    bad = t.copy()
    bad[3, 1] = len(v)
    assert build_deformable(rlib, v, bad)[0] == -1
    vn = v.copy()
    vn[5, 2] = np.nan
    assert build_deformable(rlib, vn, t)[0] == -1
    r, err, _ = build_deformable(rlib, np.zeros((3, 3), dtype=f32), np.array([[0, 1, 2]], dtype=np.uint32))
    assert r == -1 and "area" in err


@pytest.mark.parametrize("kind", ["grid", "soup", "ico", "reopen"])
def test_refit_with_the_creation_vertices_reproduces_the_tables(rlib, kind):
    v, _, t = deformations()[kind]
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0, err
    nodes, tris, box_pad = refit(rlib, T, v)
    assert same_bits(nodes, T.nodes) and same_bits(tris, T.tris)
    assert same_bits(box_pad, np.concatenate([T.lo, T.hi, [T.pad]]).astype(f32))  # the host's bounds: the root's box and the pad


@pytest.mark.parametrize("kind", ["grid", "soup", "ico", "reopen"])
def test_refit_with_deformed_vertices(rlib, kind):
    v, w, t = deformations()[kind]
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0, err
    nodes, tris, box_pad = refit(rlib, T, w)
    ref, live = check_tables(w, t, T, nodes, tris)
    assert same_bits(box_pad[0:3], nodes[0, 0:3]) and same_bits(box_pad[3:6], nodes[0, 4:7])
    before = mesh_ref.Mesh(v, t)
    if kind == "ico":
        assert 0 < len(ref.orig) < len(before.orig) == len(t)  # some collapsed
    if kind == "reopen":
        assert len(before.orig) < len(ref.orig) == len(t)      # every creation-time degenerate opened up
    # ... and back again: the tables of the creation, bit for bit (nothing of an update survives the next one)
    T2 = Tables()
    T2.__dict__.update(T.__dict__)
    T2.nodes, T2.tris = nodes, tris
    nodes2, tris2, _ = refit(rlib, T2, v)
    assert same_bits(nodes2, T.nodes) and same_bits(tris2, T.tris)


def test_refit_of_a_single_leaf_and_of_an_all_flat_mesh(rlib):
    """N = 1 (the root is a leaf); vertices that leave no triangle of non-zero area are accepted by a refit: every record is marked"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], dtype=f32)
    t = np.array([[0, 1, 2]], dtype=np.uint32)
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0 and len(T.nodes) == 1 and list(T.level_off) == [0, 1], err
    w = (v * f32(2.5) + f32(1.0)).astype(f32)
    nodes, tris, _ = refit(rlib, T, w)
    check_tables(w, t, T, nodes, tris)
    gv, gt = waving_grid(0.0, cells=6)
    r, err, T = build_deformable(rlib, gv, gt)
    assert r == 0, err
    flat = np.zeros_like(gv)
    flat[:, 0] = gv[:, 0]  # every vertex on one line
    nodes, tris, _ = refit(rlib, T, flat)
    assert (u32(tris[:, 4:7]) == 0).all() and (u32(tris[:, 8:11]) == 0).all()
    O, D, md = ray_families(np.random.default_rng(1), gv, gt, n=500)
    hit, _, _ = device_walk(nodes, tris, O, D, md)
    assert not hit.any()


@pytest.mark.parametrize("kind", ["grid", "soup", "ico"])
def test_device_walk_over_refitted_tables_matches_the_brute_force(rlib, kind):
    """the numpy replay of the kernels' walk over the REFITTED hierarchy against the brute-force reference over a mesh made of
    the new vertices: same hit, distance, normal -- on every ray family of the static test"""
    v, w, t = deformations()[kind]
    r, err, T = build_deformable(rlib, v, t)
    assert r == 0, err
    nodes, tris, _ = refit(rlib, T, w)
    O, D, md = ray_families(np.random.default_rng({"grid": 1, "soup": 2, "ico": 3}[kind]), w, t)
    hit, dist, nrm = device_walk(nodes, tris, O, D, md)
    rh, rt, rn = mesh_ref.cast_instance(mesh_ref.Instance(mesh_ref.Mesh(w, t)), O, D, md)
    assert rh.sum() > len(O) // 10, rh.sum()
    assert np.array_equal(hit, rh), np.flatnonzero(hit != rh)[:10]
    assert np.array_equal(dist[hit], rt[hit]) and np.array_equal(nrm[hit], rn[hit])


def test_the_new_calls_are_bound():
    from bevy_firework_amd import _ffi, system

    bound = {name for name, _, _ in _ffi.SYMBOLS}
    assert {"fw_ctx_create_deformable_mesh", "fw_ctx_update_mesh_vertices"} <= bound
    lib_ = _ffi.load()
    assert hasattr(lib_, "fw_ctx_create_deformable_mesh") and hasattr(lib_, "fw_ctx_update_mesh_vertices")
    assert callable(system.ParticleSystem.create_deformable_mesh) and callable(system.ParticleSystem.update_mesh_vertices)
    assert lib_.fw_abi_version() == 5
