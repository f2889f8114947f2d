"""Vertices from device memory, without a GPU: the reduction fw_k_mesh_bounds / fw_k_mesh_bounds_fold run (csrc/fw_mesh_bounds.h:
the per-vertex step, the combine step, the finish) compiled here with g++ and folded over random partitions and orders of the
vertices, against the host's one pass (fw_bvh_stage_vertices, csrc/fw_bvh.cpp) -- bit for bit; and the instance sphere the
device computes from the record's box (fw_mesh_inst_sphere) against the placed box it has to contain."""
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

f32 = np.float32
FLT_MAX = np.finfo(f32).max
WRAPPER = r"""
#include "fw_bvh.h"
#include "fw_mesh_bounds.h"
#include <vector>
// the host's pass: returns the first non-finite vertex or -1; out = lo[3] hi[3] pad
extern "C" long long host_bounds(const float *xyz, const uint8_t *referenced, uint32_t nv, float *out) {
    return (long long)fw_bvh_stage_vertices(xyz, referenced, nv, nullptr, out, out + 3, out + 6);
}
// the device's reduction: the vertices visited in the order perm[], vertex perm[i] going to the partial group[i] (a lane, a
// workgroup); the partials then combined in the order corder[], one after the other (tree == 0) or pairwise, halving (tree != 0)
extern "C" long long fold_bounds(const float *xyz, const uint8_t *referenced, uint32_t nv, const uint32_t *perm, const uint32_t *group,
                                 uint32_t n_groups, const uint32_t *corder, int tree, float *out) {
    std::vector<FwVtxAcc> acc(n_groups, fw_bounds_empty());
    for (uint32_t i = 0; i < nv; i++) {
        const uint32_t v = perm[i];
        fw_bounds_vertex(acc[group[i]], v, xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2], referenced[v] != 0);
    }
    std::vector<FwVtxAcc> q(n_groups);
    for (uint32_t g = 0; g < n_groups; g++) q[g] = acc[corder[g]];
    FwVtxAcc total = fw_bounds_empty();
    if (!tree) {
        for (uint32_t g = 0; g < n_groups; g++) total = fw_bounds_combine(total, q[g]);
    } else {
        while (q.size() > 1) {
            std::vector<FwVtxAcc> h;
            for (size_t g = 0; g + 1 < q.size(); g += 2) h.push_back(fw_bounds_combine(q[g + 1], q[g]));
            if (q.size() & 1) h.push_back(q.back());
            q.swap(h);
        }
        total = q[0];
    }
    if (total.bad != FW_MESH_NO_BAD) return (long long)total.bad;
    fw_bounds_finish(total, out, out + 3, out + 6);
    return -1;
}
extern "C" void inst_sphere(const float *lo, const float *hi, const float *position, const float *rotation, float *out4) {
    fw_mesh_inst_sphere(lo, hi, position, rotation, out4, out4 + 3);
}
"""
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def blib(tmp_path_factory):
    d = tmp_path_factory.mktemp("bounds")
    (d / "wrap.cpp").write_text(WRAPPER)
    so = d / "libbounds.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(CSRC, "fw_bvh.cpp"), str(d / "wrap.cpp"), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.host_bounds.restype = C.c_longlong
    lib.fold_bounds.restype = C.c_longlong
    return lib


def host(blib, v, ref):
    out = np.zeros(7, dtype=f32)
    bad = blib.host_bounds(P(v), P(ref), C.c_uint32(len(v)), P(out))
    return int(bad), out


def folds(blib, v, ref, rng, rounds=12):
    """the reduction over `rounds` random (order, partition, combine order, combine shape) choices, the kernel's own among them:
    vertex i to lane i % (64 x workgroups), the partials in index order"""
    n = len(v)
    for r in range(rounds):
        if r == 0:
            n_groups = min(n, 64 * 4)
            perm, group, corder, tree = np.arange(n), np.arange(n) % n_groups, np.arange(n_groups), 1
        else:
            n_groups = int(rng.integers(1, min(n, 300) + 1))
            perm, group = rng.permutation(n), rng.integers(0, n_groups, n)
            corder, tree = rng.permutation(n_groups), int(rng.integers(0, 2))
        out = np.zeros(7, dtype=f32)
        bad = blib.fold_bounds(P(v), P(ref), C.c_uint32(n), P(perm.astype(np.uint32)), P(group.astype(np.uint32)), C.c_uint32(n_groups),
                               P(corder.astype(np.uint32)), C.c_int(tree), P(out))
        yield int(bad), out


def referenced_of(n, t):
    ref = np.zeros(n, dtype=np.uint8)
    ref[np.asarray(t, dtype=np.int64).ravel()] = 1
    return ref


def _cases():
    rng = np.random.default_rng(77)
    out = {}
    v, t = mesh_ref.grid_mesh(17, 13, extent=5.0, height=lambda x, z: 0.7 * np.sin(x) * np.cos(2 * z))
    out["terrain"] = (v.astype(f32), referenced_of(len(v), t))
    for k in range(4):
        n = int(rng.integers(3, 3000))
        v = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 6)).astype(f32)
        ref = (rng.random(n) < rng.uniform(0.05, 1.0)).astype(np.uint8)
        ref[int(rng.integers(n))] = 1
        out[f"random {k}"] = (v, ref)
    # unreferenced vertices with larger coordinates than any referenced one: they must not enter lo / hi / pad
    v = rng.normal(size=(500, 3)).astype(f32)
    ref = np.ones(500, dtype=np.uint8)
    ref[::7] = 0
    v[::7] *= f32(1e6)
    out["large unreferenced"] = (v, ref)
    out["all equal"] = (np.full((300, 3), f32(-3.25)), np.ones(300, dtype=np.uint8))
    den = (rng.integers(1, 1 << 22, size=(400, 3)).astype(np.uint32) | (rng.integers(0, 2, size=(400, 3)).astype(np.uint32) << 31)).view(f32)
    out["denormals"] = (den, np.ones(400, dtype=np.uint8))
    z = np.zeros((200, 3), dtype=f32)
    z[rng.random((200, 3)) < 0.5] = f32(-0.0)
    out["signed zeros"] = (z, np.ones(200, dtype=np.uint8))
    mz = rng.normal(size=(200, 3)).astype(f32)
    mz[:, 1] = np.where(rng.random(200) < 0.5, f32(-0.0), f32(0.0))  # a flat mesh at y = +-0: lo / hi of y are zeros of either sign
    out["zeros in one axis"] = (mz, np.ones(200, dtype=np.uint8))
    big = (rng.uniform(-1, 1, size=(300, 3)) * FLT_MAX).astype(f32)
    big[0], big[1] = FLT_MAX, -FLT_MAX
    out["near FLT_MAX"] = (big, np.ones(300, dtype=np.uint8))
    out["all zero"] = (np.zeros((64, 3), dtype=f32), np.ones(64, dtype=np.uint8))  # (the 1e-30f arm of the pad)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_any_partition_and_order_folds_to_the_hosts_bits(blib, name):
    v, ref = CASES[name]
    v = np.ascontiguousarray(v, dtype=f32)
    bad, want = host(blib, v, ref)
    assert bad == -1
    if name == "all zero":
        assert want[6] == f32(1e-30)
    rng = np.random.default_rng(len(name))
    n = 0
    for got_bad, got in folds(blib, v, ref, rng):
        assert got_bad == -1
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, got, want)
        n += 1
    assert n == 12


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_the_lowest_non_finite_vertex_is_reported(blib, value):
    rng = np.random.default_rng(5)
    v0 = rng.normal(size=(777, 3)).astype(f32)
    ref = (rng.random(777) < 0.6).astype(np.uint8)
    ref[[0, 776]] = 1
    mid_ref, mid_unref = int(np.flatnonzero(ref)[200]), int(np.flatnonzero(ref == 0)[100])
    for where in ([0], [776], [mid_ref], [mid_unref], [mid_unref, 776], [mid_ref, mid_unref, 500], [0, 776]):
        for comp in range(3):
            v = v0.copy()
            for i in where:
                v[i, comp] = value
            bad, _ = host(blib, v, ref)
            assert bad == min(where)  # (the host form rejects an unreferenced non-finite vertex too)
            for got_bad, _ in folds(blib, v, ref, rng, rounds=6):
                assert got_bad == min(where), (where, comp)


def _rot(q, p):
    """R(q) p in double for a unit quaternion xyzw"""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return p @ R.T


def test_the_instance_sphere_contains_the_placed_box(blib):
    rng = np.random.default_rng(9)
    for k in range(300):
        c = rng.normal(size=3) * 10.0 ** rng.integers(-2, 4)
        h = np.abs(rng.normal(size=3)) * 10.0 ** rng.integers(-3, 3)
        lo, hi = (c - h).astype(f32), (c + h).astype(f32)
        pos = (rng.normal(size=3) * 10.0 ** rng.integers(-1, 3)).astype(f32)
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q)).astype(f32) if k % 5 else np.array([0, 0, 0, 1], dtype=f32)
        out = np.zeros(4, dtype=f32)
        blib.inst_sphere(P(lo), P(hi), P(pos), P(q), P(out))
        q64 = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
        corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[m][2]] for i in (0, 1) for j in (0, 1) for m in (0, 1)], dtype=np.float64)
        world = _rot(q64, corners) + pos.astype(np.float64)
        d = np.linalg.norm(world - out[:3].astype(np.float64), axis=1).max()
        assert np.isfinite(out).all() and d <= float(out[3]), (k, d, out)
        assert float(out[3]) < 1.01 * np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)) / 2 + 1e-3 * (1 + np.abs(world).max()), (k, out)
    # a degenerate rotation, an overflowing box: never skipped, around the position
    for lo, hi, q in (((-1, -1, -1), (1, 1, 1), (0, 0, 0, 0)), ((-FLT_MAX,) * 3, (FLT_MAX,) * 3, (0, 0, 0, 1)),
                      ((-1, -1, -1), (1, 1, 1), (np.nan, 0, 0, 1))):
        out = np.zeros(4, dtype=f32)
        pos = np.array([1.0, 2.0, 3.0], dtype=f32)
        blib.inst_sphere(P(np.array(lo, dtype=f32)), P(np.array(hi, dtype=f32)), P(pos), P(np.array(q, dtype=f32)), P(out))
        assert out[3] == np.inf and np.array_equal(out[:3], pos), (lo, q, out)
