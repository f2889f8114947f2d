"""The mesh ray cast against geometry (include/firework_hip.h: fw_mesh_collider, WATERTIGHT), without a GPU.  Every other mesh test
compares the device with the header's rule restated in fp32; these compare the rule with a float64 reference over every triangle
(tests/mesh_exact.py), on rays aimed at the vertices and edges two triangles share -- the rays that used to be rejected by both:

  P1  no leak        a ray the float64 reference has cross the surface, well inside the silhouette, reports a hit no later than
                     t_ref + 2^-14 (t_ref + maxabs)                                                        (violations allowed: 0)
  P2  no invention   a hit met at |cos| >= 0.5 lies within 2^-13 (|o - v0| + |e1| + |e2|) of its triangle; a float64 miss
                     farther than that from every triangle stays a miss
  P3  superset       what the rule without the margin (mesh_exact.strict_cast) hits is still hit, no later; the same triangle
                     gives the same distance and normal, bit for bit
  P4  walk = brute   the numpy replay of the kernels' walk (tests/test_bvh_cpu.py: device_walk) over the hierarchy fw_bvh.cpp builds
                     equals the brute force bit for bit

twice: through the C oracle's brute force (oracle.cast_rays, which must equal tests/mesh_ref.py bit for bit) and through the walk,
over a static build and over a deformable build refitted to moved vertices (csrc/fw_refit.h)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_exact as X  # noqa: E402
import mesh_ref  # noqa: E402
from test_bvh_cpu import build as bvh_build, device_walk, lib  # noqa: E402,F401  (lib: the g++ fixture)
from test_bvh_refit_cpu import build_deformable, refit, rlib  # noqa: E402,F401

import oracle  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
CASES = [(name, level) for name in X.GATED for level in X.LEVELS]
FAR = [(name, level) for name in X.GATED for level in (64, 1024)]
SLIVER = [("sliver", level) for level in X.LEVELS + (64, 1024)]
AIMED = [c for c in CASES if X.FAMILIES[c[0]][2]]
ids = lambda cases: [f"{n}-{l}" for n, l in cases]  # noqa: E731


@functools.lru_cache(maxsize=None)
def case(name, level):
    """one family at one level with what every property needs, computed once and read-only: the instance, the brute force by the
    new rule and by the rule without the margin -- (hit, t, normal, k) each"""
    F = X.family(name, level)
    F.inst = X.instance(F)
    F.new = mesh_ref.cast_instance_full(F.inst, F.origin, F.dir, F.max_distance)
    F.strict = X.strict_cast(F.inst, F.origin, F.dir, F.max_distance)
    for a in F.new + F.strict:
        a.setflags(write=False)
    return F


def oracle_cast(F):
    om = oracle.OracleMesh(F.vertices, F.indices)
    got = oracle.cast_rays([], [S.MeshCollider(om, F.position, F.rotation, 1)], 1, F.origin, F.dir, F.max_distance)
    om.close()
    return got


def walk(nodes, tris, inst, o, d, md):
    """the walk of one placed instance as fw_cast_ray runs it: into the frame, device_walk, the normal of the best slot taken back
    -> (hit, t, normal, k) like mesh_ref.cast_instance_full"""
    ol, dl = mesh_ref.into_frame(inst, o, d)
    hit, t, slot = device_walk(nodes, tris, ol, dl, md, slots=True)
    orig = np.ascontiguousarray(tris[:, 3]).view(np.uint32).astype(np.int64)
    k = np.searchsorted(inst.mesh.orig, orig[np.where(hit, slot, 0)])
    nrm = inst.mesh.normal[k]
    q = np.asarray(inst.rotation, dtype=f32)
    if not (q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1):
        nrm = mesh_ref.quat_mul_vec3(np.broadcast_to(q, (len(o), 4)), nrm)
    flip = mesh_ref.dot3(nrm, d) > 0
    nrm = np.where(flip[:, None], (-nrm).astype(f32), nrm).astype(f32)
    return hit, np.where(hit, t, f32(np.inf)).astype(f32), nrm, k


def assert_same_cast(got, want, what):
    (gh, gt, gn), (wh, wt, wn) = got[:3], want[:3]
    assert np.array_equal(gh, wh), (what, "hit", np.flatnonzero(gh != wh)[:10])
    assert np.array_equal(gt[gh], wt[gh]) and np.array_equal(gn[gh], wn[gh]), (what, np.flatnonzero(gh & ((gt != wt) | (gn != wn).any(axis=1)))[:10])


def in_domain(F):
    """the rays the header's WATERTIGHT holds the WALK to: those whose float64 crossing has a conditioning of at most 2^13"""
    _, k_ref, _ = X.reference(F)
    return (k_ref >= 0) & (X.conditioning(F.inst, F.origin, F.dir, np.maximum(k_ref, 0)) <= X.WALK_DOMAIN)


# ---- the brute force ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, level", CASES, ids=ids(CASES))
def test_brute_force_holds_the_properties(name, level):
    F = case(name, level)
    got = oracle_cast(F)
    assert_same_cast(got, F.new, "the C oracle against tests/mesh_ref.py")
    hit, t, _, k = F.new
    leak = X.leaks(F, hit, t)
    off, ghost = X.inventions(F, hit, t, k)
    lost = X.not_superset(F.strict, F.new)
    n_ref = int(np.isfinite(X.reference(F)[0]).sum())
    print(f"{name} {level}: {n_ref} crossings, P1 {int(leak.sum())}, P2 {int(off.sum())} + {int(ghost.sum())}, P3 {int(lost.sum())}; "
          f"without the margin P1 {int(X.leaks(F, F.strict[0], F.strict[1]).sum())}")
    assert n_ref > len(hit) // 2
    assert not leak.any(), ("P1", np.flatnonzero(leak)[:10])
    assert not off.any() and not ghost.any(), ("P2", np.flatnonzero(off)[:10], np.flatnonzero(ghost)[:10])
    assert not lost.any(), ("P3", np.flatnonzero(lost)[:10])


@pytest.mark.parametrize("name, level", AIMED, ids=ids(AIMED))
def test_the_aimed_families_find_the_leaks_of_the_rule_without_the_margin(name, level):
    """(the families are sharp: u >= 0, v >= 0, u + v <= 1 lets hundreds of each through -- and holds P2 as well)"""
    F = case(name, level)
    hit, t, _, k = F.strict
    assert X.leaks(F, hit, t).sum() > 100
    off, ghost = X.inventions(F, hit, t, k)
    assert not off.any() and not ghost.any()


@pytest.mark.parametrize("name, level", FAR, ids=ids(FAR))
def test_brute_force_holds_p1_from_far_away(name, level):
    """64 and 1024 times the mesh's size away the margin is at its cap for most rays: the brute force still lets nothing through"""
    F = X.family(name, level)
    hit, t, _ = oracle_cast(F)
    leak = X.leaks(F, hit, t)
    print(f"{name} {level}: P1 {int(leak.sum())} of {int(np.isfinite(X.reference(F)[0]).sum())}")
    assert not leak.any(), np.flatnonzero(leak)[:10]


# ---- the walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, level", CASES, ids=ids(CASES))
def test_walk_equals_the_brute_force_and_holds_p1(lib, name, level):  # noqa: F811
    F = case(name, level)
    r, err, nodes, tris = bvh_build(lib, F.vertices, F.indices)
    assert r == 0, err
    got = walk(nodes, tris, F.inst, F.origin, F.dir, F.max_distance)
    leak = X.leaks(F, got[0], got[1]) & in_domain(F)
    assert not leak.any(), ("P1 inside the walk's domain", np.flatnonzero(leak)[:10])
    assert_same_cast(got, F.new, "P4")
    assert np.array_equal(got[3][got[0]], F.new[3][got[0]])


@pytest.mark.parametrize("level", X.LEVELS)
def test_walk_over_a_refitted_hierarchy(rlib, level):  # noqa: F811
    """a deformable build of the unit icosphere refitted to the vertices of the scaled one: the walk over the refitted tables
    against the brute force over a mesh made of the new vertices, on the scaled family's rays"""
    F = case("ico_scaled", level)
    v0, t0 = mesh_ref.icosphere(2, 1.0)
    assert np.array_equal(t0, F.indices)
    r, err, T = build_deformable(rlib, v0, t0)
    assert r == 0, err
    nodes, tris, _ = refit(rlib, T, F.vertices)
    got = walk(nodes, tris, F.inst, F.origin, F.dir, F.max_distance)
    leak = X.leaks(F, got[0], got[1]) & in_domain(F)
    assert not leak.any(), ("P1", np.flatnonzero(leak)[:10])
    assert_same_cast(got, F.new, "P4, refitted")


# ---- reported, not gated ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, level", FAR + SLIVER, ids=ids(FAR + SLIVER))
def test_report_the_walk_far_away_and_on_slivers(lib, name, level):  # noqa: F811
    """P1 of the walk 64 and 1024 sizes away and on a mesh of slivers (an icosphere scaled by (1, 0.01, 1)): counted and printed,
    inside and outside the walk's domain; only the domain is asserted -- and P4, which holds out here only because the walk grows
    its boxes (without FW_WT_BOX: 22 rays of `box 1024` and 12 of `sliver 64` differ)"""
    F = X.family(name, level)
    F.inst = X.instance(F)
    r, err, nodes, tris = bvh_build(lib, F.vertices, F.indices)
    assert r == 0, err
    got = walk(nodes, tris, F.inst, F.origin, F.dir, F.max_distance)
    brute = mesh_ref.cast_instance_full(F.inst, F.origin, F.dir, F.max_distance)
    leak, dom = X.leaks(F, got[0], got[1]), in_domain(F)
    differ = (got[0] != brute[0]) | (got[0] & (got[1] != brute[1]))
    print(f"{name} {level}: walk P1 {int(leak.sum())} ({int((leak & dom).sum())} inside the domain, which holds {int(dom.sum())} rays), "
          f"brute force P1 {int(X.leaks(F, brute[0], brute[1]).sum())}, walk != brute force on {int(differ.sum())} rays")
    assert not (leak & dom).any()
    assert_same_cast(got, brute, "P4")
