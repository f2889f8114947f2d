"""The point query (include/firework_hip.h: POINT QUERIES; fw_ctx_project_points[_device]) without a GPU: fw_point /
fw_point_projection as the C compiler lays them out against the numpy dtypes and the ctypes mirrors, the two entry points in every
mirror; the product's own arithmetic -- csrc/fw_project.h's fw_project_point, host side, over hierarchies built by fw_bvh.cpp -- bit
for bit against the numpy statement of the header's text (tests/project_ref.py, a brute force over all triangles); is_inside against
the ray cast's distance-0 case; and that statement against the geometry of the shapes in float64."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_points as P  # noqa: E402
import project_ref  # noqa: E402
from capsule_rays import _rot64  # noqa: E402
from test_capsule_cpu import COLLIDER_DTYPE, _makefile_flags  # noqa: E402

from bevy_firework_amd import _ffi  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
f32 = np.float32
NONE = 0xFFFFFFFF
POINT_FIELDS = ("position", "filter_mask")
PROJECTION_FIELDS = ("point", "distance", "kind", "index", "triangle", "is_inside")


# ---- 1. layout and mirrors -----------------------------------------------------------------------------------------------------------
def test_point_and_projection_layouts_and_entry_points_in_every_mirror(tmp_path):
    exprs = ["sizeof(fw_point)", "sizeof(fw_point_projection)"] + [f"offsetof(fw_point,{k})" for k in POINT_FIELDS] \
        + [f"offsetof(fw_point_projection,{k})" for k in PROJECTION_FIELDS] + ["(size_t)FW_ABI_VERSION"]
    src = tmp_path / "point.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "firework_hip.h"\nint main(void){printf("' + " ".join(["%zu"] * len(exprs))
                   + '\\n",' + ",".join(exprs) + ");return 0;}\n")
    exe = tmp_path / "point"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [16, 32] and got[-1] == 5
    for dtype, mirror, fields, size in ((S.POINT_DTYPE, _ffi.Point, POINT_FIELDS, 16), (S.POINT_PROJECTION_DTYPE, _ffi.PointProjection, PROJECTION_FIELDS, 32)):
        assert dtype.names == fields and [name for name, _ in mirror._fields_] == list(fields)
        assert dtype.itemsize == C.sizeof(mirror) == size
    want = [16, 32] + [S.POINT_DTYPE.fields[k][1] for k in POINT_FIELDS] + [S.POINT_PROJECTION_DTYPE.fields[k][1] for k in PROJECTION_FIELDS]
    assert got[:-1] == want, (got, want)
    assert got[:-1] == [16, 32] + [getattr(_ffi.Point, k).offset for k in POINT_FIELDS] + [getattr(_ffi.PointProjection, k).offset for k in PROJECTION_FIELDS]
    assert S.POINT_DTYPE["filter_mask"] == "u4" and S.POINT_PROJECTION_DTYPE["kind"] == "i4" and S.POINT_PROJECTION_DTYPE["is_inside"] == "u4"
    names = ("fw_ctx_project_points", "fw_ctx_project_points_device")
    lib = _ffi.load()
    bound = {name for name, _, _ in _ffi.SYMBOLS}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert "POINT QUERIES" in header and header.index("RAY-CAST QUERIES") < header.index("POINT QUERIES")
    for name in names:
        assert hasattr(lib, name) and name in bound, name
        assert re.search(rf" T {name}$", exported, re.M), name
        assert re.search(rf"fw_status {name}\(fw_ctx \*ctx, ", header), name
        for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
            assert re.search(rf"pub fn {name}\(ctx: \*mut fw_ctx, ", open(os.path.join(ROOT, mirror)).read()), (mirror, name)
        assert f"{name}(ctx_" in open(os.path.join(ROOT, "include", "firework.hpp")).read(), name
    for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
        text = open(os.path.join(ROOT, mirror)).read()
        assert "pub struct fw_point {" in text and "pub struct fw_point_projection {" in text, mirror
        assert re.search(r"pub position: \[f32; 3\], pub filter_mask: u32", text), mirror
        assert re.search(r"pub point: \[f32; 3\], pub distance: f32, pub kind: i32, pub index: u32, pub triangle: u32, pub is_inside: u32", text), mirror
    from bevy_firework_amd.system import ParticleSystem

    assert callable(ParticleSystem.project_points) and callable(ParticleSystem.project_points_device)
    src = open(os.path.join(CSRC, "fw_k_query.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "fw_project_point(" in code and "fw_k_project_points" in code


# ---- 2. the product's arithmetic on the CPU ---------------------------------------------------------------------------------------
PROGRAM = r"""
// projects points read from a file onto a world read from the same file through csrc/fw_project.h's fw_project_point (the host side
// of FW_HD: no device is touched; the hierarchies are fw_bvh.cpp's) and writes one fw_point_projection per point; then, per point
// and analytic collider, whether fw_project_collider says inside and whether fw_ray_collider with max_distance 0 reports a hit
// with a zero normal
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "fw_project.h"
#include "fw_bvh.h"
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, n, 1, f) == 1; }
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nc = 0, nm = 0, ni = 0, np = 0;
    if (!rd(f, &nc, 4)) return 4;
    std::vector<FwCollider> cs(nc);
    if (!rd(f, cs.data(), nc * sizeof(FwCollider)) || !rd(f, &nm, 4)) return 4;
    std::vector<FwBvh> bvh(nm);
    for (uint32_t m = 0; m < nm; m++) {
        uint32_t h[3];
        if (!rd(f, h, 12)) return 4;
        std::vector<float> xyz(3 * (size_t)h[1]);
        std::vector<uint32_t> idx(3 * (size_t)h[2]);
        if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, idx.data(), idx.size() * 4)) return 4;
        std::string err;
        const int rc = h[0] ? fw_bvh_build_deformable(xyz.data(), h[1], idx.data(), h[2], &bvh[m], &err)
                            : fw_bvh_build(xyz.data(), h[1], idx.data(), h[2], &bvh[m], &err);
        if (rc != 0) {
            std::fprintf(stderr, "mesh %u: %s\n", m, err.c_str());
            return 5;
        }
    }
    if (!rd(f, &ni, 4)) return 4;
    std::vector<FwMeshInst> inst(ni);
    for (uint32_t i = 0; i < ni; i++) {
        uint32_t h[2];
        float pr[7];
        if (!rd(f, h, 8) || !rd(f, pr, 28) || h[0] >= nm) return 4;
        FwMeshInst M{};
        std::memcpy(M.position, pr, 12), std::memcpy(M.rotation, pr + 3, 16);
        M.nodes = reinterpret_cast<const float4 *>(bvh[h[0]].nodes.data()), M.tris = reinterpret_cast<const float4 *>(bvh[h[0]].tris.data());
        M.n_nodes = bvh[h[0]].n_nodes, M.layers = h[1];
        inst[i] = M;
    }
    if (!rd(f, &np, 4)) return 4;
    std::vector<fw_v3> pts(np);
    std::vector<uint32_t> masks(np);
    for (uint32_t k = 0; k < np; k++)
        if (!rd(f, &pts[k], 12) || !rd(f, &masks[k], 4)) return 4;
    std::fclose(f);
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    for (uint32_t k = 0; k < np; k++) {
        FwProjection p;
        FwHitId id;
        fw_project_point(cs.data(), nc, inst.data(), ni, masks[k], pts[k], &p, id);
        uint32_t out[8];
        std::memcpy(out, &p.point, 12), std::memcpy(out + 3, &p.distance, 4), std::memcpy(out + 4, &id.kind, 4);
        out[5] = id.index, out[6] = id.tri, out[7] = p.is_inside;
        std::fwrite(out, sizeof out, 1, f);
    }
    for (uint32_t k = 0; k < np; k++)
        for (uint32_t i = 0; i < nc; i++) {
            fw_v3 q;
            float d2;
            FwRayHit h{1.0f, fw_v3{1.0f, 1.0f, 1.0f}};
            const bool hit = fw_ray_collider(cs[i], pts[k], fw_v3{0.0f, 1.0f, 0.0f}, 0.0f, &h);
            const unsigned char two[2] = {(unsigned char)fw_project_collider(cs[i], pts[k], &q, &d2),
                                          (unsigned char)(hit && h.distance == 0.0f && h.normal.x == 0.0f && h.normal.y == 0.0f && h.normal.z == 0.0f)};
            std::fwrite(two, 2, 1, f);
        }
    std::fclose(f);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _program():
    """the stand-alone program, compiled once with the Makefile's flags"""
    d = tempfile.mkdtemp(prefix="fw_project_")
    src, exe = os.path.join(d, "project.cpp"), os.path.join(d, "project")
    open(src, "w").write(PROGRAM)
    hipcc, flags = _makefile_flags()
    subprocess.check_call([hipcc] + flags + ["-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "hip", src, os.path.join(CSRC, "fw_bvh.cpp"), "-o", exe])
    return d, exe


def _run_host(world, points, masks):
    """-> (projections, inside[n, colliders], cast says distance 0 with a zero normal[n, colliders]) from the product's code"""
    d, exe = _program()
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    masks = np.broadcast_to(np.asarray(masks, dtype=np.uint32), (len(points),))
    cs = np.zeros(len(world.colliders), dtype=COLLIDER_DTYPE)
    for k, c in enumerate(world.colliders):
        cs[k]["kind"], cs[k]["layers"], cs[k]["radius"] = c.kind, c.layers, c.radius
        cs[k]["position"][:3], cs[k]["rotation"], cs[k]["half_extents"][:3], cs[k]["normal"][:3] = c.position, c.rotation, c.half_extents, c.normal
    blob = [struct.pack("<I", len(cs)), cs.tobytes(), struct.pack("<I", len(world.meshes))]
    for v, t, deformable in world.meshes:
        v, t = np.ascontiguousarray(v, dtype=f32), np.ascontiguousarray(t, dtype=np.uint32)
        blob += [struct.pack("<III", int(deformable), len(v), len(t)), v.tobytes(), t.tobytes()]
    blob.append(struct.pack("<I", len(world.placements)))
    for k, p, q, layers in world.placements:
        blob.append(struct.pack("<II7f", k, layers, *[float(f32(x)) for x in p], *[float(f32(x)) for x in q]))
    rec = np.zeros(len(points), dtype=S.POINT_DTYPE)
    rec["position"], rec["filter_mask"] = points, masks
    blob += [struct.pack("<I", len(rec)), rec.tobytes()]
    fd, path = tempfile.mkstemp(dir=d, suffix=".world")
    with os.fdopen(fd, "wb") as f:
        f.write(b"".join(blob))
    subprocess.check_call([exe, path, path + ".out"], timeout=120)
    raw = np.fromfile(path + ".out", dtype=np.uint8)
    os.remove(path), os.remove(path + ".out")
    n = len(points)
    got = raw[:32 * n].view(S.POINT_PROJECTION_DTYPE).copy()
    flags = raw[32 * n:].reshape(n, len(cs), 2) if len(cs) else np.zeros((n, 0, 2), dtype=np.uint8)
    return got, flags[:, :, 0] == 1, flags[:, :, 1] == 1


def assert_projections_equal(got, want, what, names=None):
    """every field, bit for bit -- except that a NaN equals a NaN"""
    for k in PROJECTION_FIELDS:
        g, w = got[k], want[k]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if g.dtype == f32 else g == w
        bad = np.flatnonzero(~(same.all(axis=1) if same.ndim == 2 else same))
        assert not len(bad), (what, k, [(names[i] if names else int(i), got[i], want[i]) for i in bad[:5]])


@functools.lru_cache(maxsize=None)
def _mixed_reference(mask):
    w = P.mixed_world()
    out = project_ref.project_points(w.colliders, w.instances(), P.mixed_points(), mask)
    out.setflags(write=False)
    return out


def test_engineered_cases_per_kind_equal_the_header_in_numpy():
    w, pts, masks, names, owner = P.engineered()
    got, inside, _ = _run_host(w, pts, masks)
    want = project_ref.project_points(w.colliders, [], pts, masks)
    assert_projections_equal(got, want, "engineered", names)
    by = {n: got[i] for i, n in enumerate(names)}
    assert (got["kind"] == S.HIT_COLLIDER).all() and np.array_equal(got["index"], owner) and (got["triangle"] == NONE).all()
    for n, r in by.items():
        what = n.split(": ")[1].split(" [")[0]
        if "[identity]" in n and (what.startswith("inside") or what.startswith("on ") or what == "the centre") and n != "plane: on the surface [identity]":
            assert r["is_inside"] == 1 and r["distance"] == 0, n
        if what.startswith("inside"):  # (in both frames: well inside)
            assert r["is_inside"] == 1 and r["distance"] == 0, n
        if "outside" in what or what.startswith(("above", "below", "beside", "level", "just")):
            assert r["is_inside"] == 0 and r["distance"] > 0, n
    # an inside point answers with the caller's bits
    ins = got["is_inside"] == 1
    assert got["point"][ins].tobytes() == pts[ins].tobytes() and ins.sum() > 30
    # regions, where the operands are exact
    for n, point, dist in (("box: outside a face", (1.0, 0.25, 0.125), 1.0), ("box: outside a corner", (-1.0, 0.5, -0.25), float(np.sqrt(f32(3.0)))),
                           ("cylinder: outside the cap, on the axis", (0.0, 1.0, 0.0), 1.5), ("cylinder: outside the bottom rim", (0.0, -1.0, 0.5), None),
                           ("cone: above the apex, on the axis", (0.0, 1.0, 0.0), 1.5), ("cone: outside the base, on the axis", (0.0, -1.0, 0.0), 2.0),
                           ("cone: just below the base, under the rim", (0.75, -1.0, 0.0), 0.25), ("capsule: above the top pole, on the axis", (0.0, 1.5, 0.0), 2.5),
                           ("capsule: level with the segment's top end", (0.5, 1.0, 0.0), 2.5), ("ball capsule: outside on the axis", (0.0, 0.5, 0.0), 2.5),
                           ("plane: outside", (1.0, 0.0, -3.0), 2.0), ("sphere: outside on an axis", (0.0, -0.75, 0.0), 2.25)):
        r = by[n + " [identity]"]
        assert tuple(r["point"]) == point and (dist is None or r["distance"] == f32(dist)), (n, r)


MIXED_MASKS = (0xFFFFFFFF, 0b101, 0)


def test_the_mixed_world_equals_the_brute_force_over_all_triangles():
    """one collider of every kind and three mesh instances, ~3400 points (spread, near the surfaces, inside the solids, far away, a NaN,
    an infinity), under the masks 0xFFFFFFFF, 0b101, 0 and all three dealt out point by point: every field equals the reference, which
    tests every triangle -- the walk left out nothing that could win or tie; the NaN point ends"""
    w, pts = P.mixed_world(), P.mixed_points()
    for mask in MIXED_MASKS:
        got, _, _ = _run_host(w, pts, mask)
        assert_projections_equal(got, _mixed_reference(mask), f"mask {mask:#x}")
        if mask == 0:
            none = np.zeros(1, dtype=S.POINT_PROJECTION_DTYPE)
            none["index"] = none["triangle"] = NONE
            assert got.tobytes() == none.tobytes() * len(pts)
        else:
            assert (got["kind"] == S.HIT_MESH).sum() > 300 and (got["kind"] == S.HIT_COLLIDER).sum() > 1000 and (got["is_inside"] == 1).sum() > 100
            assert len(set(got["index"][got["kind"] == S.HIT_MESH].tolist())) >= 2 and len(set(got["index"][got["kind"] == S.HIT_COLLIDER].tolist())) >= 4
            assert got["kind"][np.isnan(pts).any(axis=1)].tolist() == [S.HIT_NONE]
            assert (got["triangle"][got["kind"] != S.HIT_MESH] == NONE).all() and (got["is_inside"][got["kind"] != S.HIT_COLLIDER] == 0).all()
    deal = np.arange(len(pts)) % 3
    got, _, _ = _run_host(w, pts, np.array(MIXED_MASKS, dtype=np.uint32)[deal])
    for k, mask in enumerate(MIXED_MASKS):
        assert_projections_equal(got[deal == k], _mixed_reference(mask)[deal == k], f"dealt, mask {mask:#x}")
    # a mask that excludes the winner: under 0b101 the capsule (layers 3) still answers, the cylinder (layer 2) and the soup do not
    full, part = _mixed_reference(0xFFFFFFFF), _mixed_reference(0b101)
    lost = (full["kind"] == S.HIT_COLLIDER) & (full["index"] == 3)
    assert lost.sum() > 50 and not ((part["kind"] == S.HIT_COLLIDER) & (part["index"] == 3)).any() and (part["kind"][lost] != S.HIT_NONE).all()
    assert (part["distance"][lost & (full["is_inside"] == 0)] >= full["distance"][lost & (full["is_inside"] == 0)]).all()


def test_meshes_of_one_two_five_and_two_hundred_triangles():
    """a single leaf, the first interior node, a real hierarchy: each against the brute force; every triangle of the fan answers
    somewhere"""
    w, pts, masks = P.mesh_sizes()
    got, _, _ = _run_host(w, pts, masks)
    want = project_ref.project_points([], w.instances(), pts, masks)
    assert_projections_equal(got, want, "mesh sizes")
    assert (got["kind"] == S.HIT_MESH).all() and np.array_equal(got["index"], np.log2(masks).astype(np.uint32))
    assert set(got["triangle"][got["index"] == 2].tolist()) == {0, 1, 2, 3, 4} and len(set(got["triangle"][got["index"] == 3].tolist())) > 100


def test_ties_follow_the_rule():
    """bit-equal squared distances: the analytic collider before the mesh, the lower index, the lower ORIGINAL triangle whatever the
    order in `indices`; a containing solid beats a lower collider at distance 0"""
    for name, w, point, kind, index, triangle, dist in P.tie_cases():
        got, _, _ = _run_host(w, [point], 1)
        assert_projections_equal(got, project_ref.project_points(w.colliders, w.instances(), [point], 1), name)
        r = got[0]
        assert (r["kind"], r["index"], r["triangle"], r["distance"]) == (kind, index, triangle, f32(dist)), (name, r)


def test_a_collapsed_triangle_of_a_deformable_build_does_not_answer():
    w, pts, masks, peak = P.collapsed()
    got, _, _ = _run_host(w, pts, masks)
    assert_projections_equal(got, project_ref.project_points([], w.instances(), pts, masks), "collapsed")
    assert (got["kind"] == S.HIT_MESH).all() and (got["point"][-1] != peak).any() and got["distance"][-1] > 2.0  # (the point ON the collapsed triangles)
    assert not np.isin(got["triangle"], (0, 11)).any() and (got["triangle"] <= 10).any() and (got["triangle"] >= 12).any()  # original indices
    static = P.World([], [(w.meshes[0][0], w.meshes[0][1], False)], w.placements)  # creation drops them: the same answers
    assert _run_host(static, pts, masks)[0].tobytes() == got.tobytes()


# ---- 3. is_inside against the cast ---------------------------------------------------------------------------------------------------------
def test_is_inside_is_the_casts_distance_zero_case():
    """every analytic collider against every point of the engineered and the mixed set: fw_project_collider says inside exactly when
    fw_ray_collider with max_distance = 0 reports a hit at distance 0 with a zero normal"""
    for w, pts in ((P.engineered()[0], P.engineered()[1]), (P.mixed_world(), P.mixed_points())):
        got, inside, cast = _run_host(P.World(w.colliders), pts, 0xFFFFFFFF)
        assert inside.shape == (len(pts), len(w.colliders)) and np.array_equal(inside, cast), np.argwhere(inside != cast)[:10]
        assert inside.any(axis=0).all() and (~inside).any(axis=0).all()  # (every collider contains some points and not others)
        assert np.array_equal(got["is_inside"] == 1, inside.any(axis=1))
        first = np.argmax(inside, axis=1)
        assert np.array_equal(got["index"][inside.any(axis=1)], first[inside.any(axis=1)])  # the lowest containing index


# ---- 4. the reference against geometry in float64 ---------------------------------------------------------------------------------------------
def _solid_distance64(c, x):
    """float64 closed forms: the distance from x[n, 3] to the solid (0 inside)"""
    pos = np.asarray(c.position, dtype=np.float64)
    if c.kind == 0:
        nrm = np.asarray(c.normal, dtype=np.float64)
        return np.maximum((x - pos) @ (nrm / np.linalg.norm(nrm)), 0.0)
    if c.kind == 1:
        return np.maximum(np.linalg.norm(x - pos, axis=1) - float(f32(c.radius)), 0.0)
    o = (x - pos) @ _rot64(c.rotation)  # R^T (x - pos)
    r, hh = float(f32(c.radius)), float(f32(c.half_extents[1]))
    rad = np.hypot(o[:, 0], o[:, 2])
    if c.kind == 2:
        return np.linalg.norm(np.maximum(np.abs(o) - np.asarray([float(f32(h)) for h in c.half_extents]), 0.0), axis=1)
    if c.kind == 3:
        return np.hypot(np.maximum(rad - r, 0.0), np.maximum(np.abs(o[:, 1]) - hh, 0.0))
    if c.kind == 5:
        return np.maximum(np.hypot(rad, o[:, 1] - np.clip(o[:, 1], -hh, hh)) - r, 0.0)
    # the cone's profile: the triangle (0, -hh), (r, -hh), (0, +hh) in (rad, y); outside it the nearer of the base and the slant segment
    def seg(ax, ay, bx, by):
        dx, dy = bx - ax, by - ay
        t = np.clip(((rad - ax) * dx + (o[:, 1] - ay) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
        return np.hypot(rad - (ax + t * dx), o[:, 1] - (ay + t * dy))
    inside = (o[:, 1] >= -hh) & (o[:, 1] <= hh) & (rad <= r * (hh - o[:, 1]) / (2.0 * hh))
    return np.where(inside, 0.0, np.minimum(seg(0.0, -hh, r, -hh), seg(r, -hh, 0.0, hh)))


def _mesh_distance64(inst, x):
    """float64: the distance from x[n, 3] to the nearest triangle of a placed mesh -- the foot of the perpendicular where it falls inside
    the triangle, else the nearest of the three edges (not the region walk of the header)"""
    o = (x - np.asarray(inst.position, dtype=np.float64)) @ _rot64(inst.rotation)
    a = inst.mesh.v0.astype(np.float64)
    b, c = a + inst.mesh.e1.astype(np.float64), a + inst.mesh.e2.astype(np.float64)
    best = np.full(len(x), np.inf)
    for k in range(0, len(x), 512):
        p = o[k:k + 512, None, :]
        def edge(u, v):
            d = v - u
            t = np.clip(((p - u) * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
            return np.linalg.norm(p - (u + t[..., None] * d), axis=-1)
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        h = ((p - a) * n).sum(-1)
        foot = p - h[..., None] * n
        inside = np.ones(h.shape, dtype=bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(v - u, foot - u) * n).sum(-1) >= 0.0
        d = np.minimum(np.minimum(edge(a, b), edge(b, c)), edge(c, a))
        best[k:k + 512] = np.where(inside, np.abs(h), d).min(axis=1)
    return best


MARGIN = 1e-4 * P.EXTENT
# Measured over the fixed set below (P.mixed_points(), seed P.SEED, under the mask 0xFFFFFFFF; profiles/r16/project_error.txt): the
# worst deviation of tests/project_ref.py -- the fp32 statement, not the library -- from the float64 closed forms, each relative to
# max(EXTENT, |position|): the reported distance against the least distance over all participants, the distance from the reported
# point to the collider it names, and |position - point| against the reported distance.  The bounds are four times these figures.
MEASURED = {"distance": 1.685e-07, "on_surface": 8.048e-08, "consistent": 1.991e-07}  # (over the 3371 chosen points)


@functools.lru_cache(maxsize=None)
def _geometry():
    """-> the three deviations per point (relative), is_inside of the reference and of float64, the margin of every point"""
    w, pts = P.mixed_world(), P.mixed_points()
    pts = pts[np.isfinite(pts).all(axis=1) & (np.abs(pts).max(axis=1) < 1e6)]
    ref = project_ref.project_points(w.colliders, w.instances(), pts, 0xFFFFFFFF)
    x = pts.astype(np.float64)
    insts = w.instances()
    each = [_solid_distance64(c, x) for c in w.colliders] + [_mesh_distance64(i, x) for i in insts]
    # how far float64 puts a point from every SURFACE: outside a solid its distance; inside, the distance to the complement
    # (sampled: the distance 0 of a step of MARGIN in 26 directions) is replaced by a direct statement -- the point moved by MARGIN in
    # any of 26 directions is still inside
    steps = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], dtype=np.float64)
    steps *= MARGIN / np.linalg.norm(steps, axis=1, keepdims=True)
    clear = np.ones(len(x), dtype=bool)
    for c, d in zip(w.colliders, each[:len(w.colliders)]):
        deep = np.all([_solid_distance64(c, x + s) == 0.0 for s in steps], axis=0)
        clear &= (d >= MARGIN) | deep
    for d in each[len(w.colliders):]:
        clear &= d >= MARGIN
    inside64 = np.any([d == 0.0 for d in each[:len(w.colliders)]], axis=0)
    dmin = np.where(inside64, 0.0, np.min(each, axis=0))
    scale = np.maximum(P.EXTENT, np.abs(x).max(axis=1))
    q = ref["point"].astype(np.float64)
    on = np.zeros(len(x))
    for i, c in enumerate(w.colliders):
        sel = (ref["kind"] == S.HIT_COLLIDER) & (ref["index"] == i)
        on[sel] = _solid_distance64(c, q[sel])
    for i, inst in enumerate(insts):
        sel = (ref["kind"] == S.HIT_MESH) & (ref["index"] == i)
        on[sel] = _mesh_distance64(inst, q[sel])
    dev = {"distance": np.abs(ref["distance"].astype(np.float64) - dmin) / scale, "on_surface": on / scale,
           "consistent": np.abs(np.linalg.norm(x - q, axis=1) - ref["distance"].astype(np.float64)) / scale}
    return dev, ref, inside64, clear, pts


def test_the_definition_is_the_nearest_point_in_float64():
    """every finite point of the mixed set that float64 puts at least 1e-4 of the scene's extent away from every surface (the set is
    chosen so: at least nine in ten of the candidates, and none of those is left out): the reference names somebody, is_inside is
    float64's, the reported point lies on the named collider, no participant has anything nearer than the reported distance, and
    |position - point| is that distance -- each within four times the deviation measured on this very set"""
    dev, ref, inside64, clear, pts = _geometry()
    assert clear.sum() > 0.9 * len(pts) and clear.sum() > 2500, (clear.sum(), len(pts))
    print(f"{clear.sum()} of {len(pts)} points clear of every surface by {MARGIN:g}; worst deviations relative to max(extent, |position|): "
          + ", ".join(f"{k} {dev[k][clear].max():.3e}" for k in dev))
    assert (ref["kind"][clear] != S.HIT_NONE).all()
    assert np.array_equal(ref["is_inside"][clear] == 1, inside64[clear])
    for k, worst in MEASURED.items():
        assert dev[k][clear].max() <= 4.0 * worst, (k, dev[k][clear].max(), worst)
