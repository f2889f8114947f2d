"""The path query (include/firework_hip.h: PATH QUERIES; fw_ctx_trace_paths[_device]) without a GPU: fw_path_settings / fw_path /
fw_path_result as the C compiler lays them out against the numpy dtypes and the ctypes mirrors, the two entry points in every mirror;
and the product's own arithmetic -- csrc/fw_trace.h's fw_trace_path, host side, over hierarchies built by fw_bvh.cpp -- bit for bit,
every field, against tests/trace_ref.py (the header's text composed from golden/np_sim.py, capsule_ref and mesh_ref)."""
import atexit
import ctypes as C
import functools
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_points as P  # noqa: E402
import trace_ref  # noqa: E402
from test_capsule_cpu import COLLIDER_DTYPE, _makefile_flags  # noqa: E402

from bevy_firework_amd import _ffi  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
f32 = np.float32
NONE = 0xFFFFFFFF
SETTINGS_FIELDS = ("dt", "n_steps", "acceleration", "linear_drag", "collision")
PATH_FIELDS = ("position", "age", "velocity", "lifetime")
RESULT_FIELDS = ("position", "age", "velocity", "steps", "contact_point", "contact_step", "contact_normal", "status", "kind", "index", "triangle", "n_contacts")


# ---- 1. layout and mirrors -----------------------------------------------------------------------------------------------------------
def test_path_layouts_and_entry_points_in_every_mirror(tmp_path):
    exprs = ["sizeof(fw_path_settings)", "sizeof(fw_path)", "sizeof(fw_path_result)"] + [f"offsetof(fw_path_settings,{k})" for k in SETTINGS_FIELDS] \
        + [f"offsetof(fw_path,{k})" for k in PATH_FIELDS] + [f"offsetof(fw_path_result,{k})" for k in RESULT_FIELDS] \
        + ["(size_t)FW_PATH_RUNNING", "(size_t)FW_PATH_EXPIRED", "(size_t)FW_PATH_DESTROYED", "(size_t)FW_PATH_MAX_STEPS", "(size_t)FW_ABI_VERSION"]
    src = tmp_path / "path.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "firework_hip.h"\nint main(void){printf("' + " ".join(["%zu"] * len(exprs))
                   + '\\n",' + ",".join(exprs) + ");return 0;}\n")
    exe = tmp_path / "path"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [44, 32, 80] and got[-5:] == [S.PATH_RUNNING, S.PATH_EXPIRED, S.PATH_DESTROYED, S.PATH_MAX_STEPS, 5] == [0, 1, 2, 4096, 5]
    for dtype, mirror, fields, size in ((S.PATH_DTYPE, _ffi.Path, PATH_FIELDS, 32), (S.PATH_RESULT_DTYPE, _ffi.PathResult, RESULT_FIELDS, 80)):
        assert dtype.names == fields and [name for name, _ in mirror._fields_] == list(fields)
        assert dtype.itemsize == C.sizeof(mirror) == size
    assert [name for name, _ in _ffi.PathSettings._fields_] == list(SETTINGS_FIELDS) and C.sizeof(_ffi.PathSettings) == 44
    assert got[3:-5] == [getattr(_ffi.PathSettings, k).offset for k in SETTINGS_FIELDS] + [S.PATH_DTYPE.fields[k][1] for k in PATH_FIELDS] \
        + [S.PATH_RESULT_DTYPE.fields[k][1] for k in RESULT_FIELDS]
    assert got[3:-5] == [getattr(_ffi.PathSettings, k).offset for k in SETTINGS_FIELDS] + [getattr(_ffi.Path, k).offset for k in PATH_FIELDS] \
        + [getattr(_ffi.PathResult, k).offset for k in RESULT_FIELDS]
    for k in ("steps", "contact_step", "status", "index", "triangle", "n_contacts"):
        assert S.PATH_RESULT_DTYPE[k] == "u4", k
    assert S.PATH_RESULT_DTYPE["kind"] == "i4"
    d = _ffi.make_path_settings(S.PathSettings(0.25, 7, (1.0, -2.0, 3.0), 0.5, S.ParticleCollisionSettings(0.75, 0.125, True, 0b110)))
    assert (d.dt, d.n_steps, list(d.acceleration), d.linear_drag) == (0.25, 7, [1.0, -2.0, 3.0], 0.5)
    assert (d.collision.enabled, d.collision.restitution, d.collision.friction, d.collision.destroy_on_collision, d.collision.filter_mask) == (1, 0.75, 0.125, 1, 6)
    assert _ffi.make_path_settings(S.PathSettings(0.25, 7)).collision.enabled == 0
    names = ("fw_ctx_trace_paths", "fw_ctx_trace_paths_device")
    lib = _ffi.load()
    bound = {name for name, _, _ in _ffi.SYMBOLS}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert "PATH QUERIES" in header and header.index("POINT QUERIES") < header.index("PATH QUERIES")
    for name in names:
        assert hasattr(lib, name) and name in bound, name
        assert re.search(rf" T {name}$", exported, re.M), name
        assert re.search(rf"fw_status {name}\(fw_ctx \*ctx, const fw_path_settings \*settings, ", header), name
        for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
            assert re.search(rf"pub fn {name}\(ctx: \*mut fw_ctx, settings: \*const fw_path_settings, ", open(os.path.join(ROOT, mirror)).read()), (mirror, name)
        assert f"{name}(ctx_, &settings" in open(os.path.join(ROOT, "include", "firework.hpp")).read(), name
    for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
        text = open(os.path.join(ROOT, mirror)).read()
        assert "pub struct fw_path_settings {" in text and "pub struct fw_path {" in text and "pub struct fw_path_result {" in text, mirror
        assert re.search(r"pub dt: f32, pub n_steps: u32, pub acceleration: \[f32; 3\], pub linear_drag: f32, pub collision: fw_collision_settings", text), mirror
        assert re.search(r"pub position: \[f32; 3\], pub age: f32, pub velocity: \[f32; 3\], pub lifetime: f32", text), mirror
        assert re.search(r"pub position: \[f32; 3\], pub age: f32, pub velocity: \[f32; 3\], pub steps: u32,\s+pub contact_point: \[f32; 3\], pub contact_step: u32, "
                         r"pub contact_normal: \[f32; 3\], pub status: u32,\s+pub kind: i32, pub index: u32, pub triangle: u32, pub n_contacts: u32", text), mirror
        assert "pub const FW_PATH_MAX_STEPS: u32 = 4096;" in text, mirror
    from bevy_firework_amd.system import ParticleSystem

    assert callable(ParticleSystem.trace_paths) and callable(ParticleSystem.trace_paths_device)
    src = open(os.path.join(CSRC, "fw_k_query.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "fw_trace_path(" in code and "fw_k_trace_paths" in code and "fw_particle_collision" not in code  # (the response is stated once, elsewhere)


# ---- 2. the product's arithmetic on the CPU ---------------------------------------------------------------------------------------
PROGRAM = r"""
// traces paths read from a file through a world read from the same file with csrc/fw_trace.h's fw_trace_path (the host side of FW_HD:
// no device is touched; the hierarchies are fw_bvh.cpp's) and writes one fw_path_result per path, then the samples [step][path];
// every path is traced a second time without samples and must end the same
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "fw_trace.h"
#include "fw_bvh.h"
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, n, 1, f) == 1; }
struct Samples {
    static constexpr bool on = true;
    float *at;
    size_t n;
    void operator()(uint32_t k, fw_v3 pos, float age) const {
        float *p = at + 4 * (size_t)k * n;
        p[0] = pos.x, p[1] = pos.y, p[2] = pos.z, p[3] = age;
    }
};
static void pack(uint32_t *out, const FwPathEnd &e, const FwPathContacts &c) {
    std::memcpy(out, &e.pos, 12), std::memcpy(out + 3, &e.age, 4), std::memcpy(out + 4, &e.vel, 12), out[7] = e.steps;
    std::memcpy(out + 8, &c.point, 12), out[11] = c.step, std::memcpy(out + 12, &c.normal, 12), out[15] = e.status;
    std::memcpy(out + 16, &c.who.kind, 4), out[17] = c.who.index, out[18] = c.who.tri, out[19] = c.n;
}
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
        uint32_t h[2];
        if (!rd(f, h, 8)) return 4;
        std::vector<float> xyz(3 * (size_t)h[0]);
        std::vector<uint32_t> idx(3 * (size_t)h[1]);
        if (!rd(f, xyz.data(), xyz.size() * 4) || !rd(f, idx.data(), idx.size() * 4)) return 4;
        std::string err;
        if (fw_bvh_build(xyz.data(), h[0], idx.data(), h[1], &bvh[m], &err) != 0) {
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
    FwPathSettings s;
    static_assert(sizeof(FwPathSettings) == 44, "eleven words");
    if (!rd(f, &s, sizeof s) || !rd(f, &np, 4)) return 4;
    std::vector<float> paths(8 * (size_t)np);
    if (!rd(f, paths.data(), paths.size() * 4)) return 4;
    std::fclose(f);
    std::vector<uint32_t> out(20 * (size_t)np);
    std::vector<float> samples(4 * (size_t)s.n_steps * np);
    for (uint32_t k = 0; k < np; k++) {
        const float *p = &paths[8 * (size_t)k];
        FwPathContacts c, c2;
        const FwPathEnd e = fw_trace_path(cs.data(), nc, inst.data(), ni, s, fw_v3{p[0], p[1], p[2]}, fw_v3{p[4], p[5], p[6]}, p[3], p[7], c,
                                          Samples{samples.data() + 4 * (size_t)k, np});
        const FwPathEnd e2 = fw_trace_path(cs.data(), nc, inst.data(), ni, s, fw_v3{p[0], p[1], p[2]}, fw_v3{p[4], p[5], p[6]}, p[3], p[7], c2, FwNoSamples{});
        uint32_t again[20];
        pack(&out[20 * (size_t)k], e, c), pack(again, e2, c2);
        if (std::memcmp(&out[20 * (size_t)k], again, sizeof again) != 0) return 6;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), 4, out.size(), f), std::fwrite(samples.data(), 4, samples.size(), f);
    std::fclose(f);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _program():
    """the stand-alone program, compiled once with the Makefile's flags"""
    d = tempfile.mkdtemp(prefix="fw_trace_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)  # (kept for the session: the GPU tests run the same program)
    src, exe = os.path.join(d, "trace.cpp"), os.path.join(d, "trace")
    open(src, "w").write(PROGRAM)
    hipcc, flags = _makefile_flags()
    subprocess.check_call([hipcc] + flags + ["-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "hip", src, os.path.join(CSRC, "fw_bvh.cpp"), "-o", exe])
    return d, exe


def run_host(world, settings, paths):
    """-> (results, samples[n_steps, n, 4]) of a P.World from the product's code"""
    d, exe = _program()
    paths = np.ascontiguousarray(paths, dtype=S.PATH_DTYPE)
    cs = np.zeros(len(world.colliders), dtype=COLLIDER_DTYPE)
    for k, c in enumerate(world.colliders):
        cs[k]["kind"], cs[k]["layers"], cs[k]["radius"] = c.kind, c.layers, c.radius
        cs[k]["position"][:3], cs[k]["rotation"], cs[k]["half_extents"][:3], cs[k]["normal"][:3] = c.position, c.rotation, c.half_extents, c.normal
    blob = [struct.pack("<I", len(cs)), cs.tobytes(), struct.pack("<I", len(world.meshes))]
    for v, t, _ in world.meshes:
        v, t = np.ascontiguousarray(v, dtype=f32), np.ascontiguousarray(t, dtype=np.uint32)
        blob += [struct.pack("<II", len(v), len(t)), v.tobytes(), t.tobytes()]
    blob.append(struct.pack("<I", len(world.placements)))
    for k, p, q, layers in world.placements:
        blob.append(struct.pack("<II7f", k, layers, *[float(f32(x)) for x in p], *[float(f32(x)) for x in q]))
    c = settings.collision_settings
    blob.append(struct.pack("<fI3ffIIIff", settings.dt, settings.n_steps, *settings.acceleration, settings.linear_drag, int(c is not None),
                            int(bool(c and c.destroy_on_collision)), (c.filter_mask if c else 0) & NONE, c.restitution if c else 0.0, c.friction if c else 0.0))
    blob += [struct.pack("<I", len(paths)), paths.tobytes()]
    fd, path = tempfile.mkstemp(dir=d, suffix=".world")
    with os.fdopen(fd, "wb") as f:
        f.write(b"".join(blob))
    subprocess.check_call([exe, path, path + ".out"], timeout=120)
    raw = np.fromfile(path + ".out", dtype=np.uint8)
    os.remove(path), os.remove(path + ".out")
    n = len(paths)
    return raw[:80 * n].view(S.PATH_RESULT_DTYPE).copy(), raw[80 * n:].view(f32).reshape(settings.n_steps, n, 4).copy()


def assert_results_equal(got, want, what):
    """every field, bit for bit -- except that a NaN equals a NaN"""
    for k in RESULT_FIELDS:
        g, w = got[k], want[k]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if g.dtype == f32 else g == w
        bad = np.flatnonzero(~(same.all(axis=1) if same.ndim == 2 else same))
        assert not len(bad), (what, k, [(int(i), got[i], want[i]) for i in bad[:3]])


def assert_samples_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, np.argwhere(~same)[:5])


def reference(world, settings, paths, samples=False):
    return trace_ref.trace_paths(trace_ref.world_of(world.colliders, world.instances()), settings, paths, samples)


def path_records(position, velocity, age=0.0, lifetime=np.inf):
    p = np.asarray(position, dtype=f32).reshape(-1, 3)
    r = np.zeros(len(p), dtype=S.PATH_DTYPE)
    r["position"], r["velocity"], r["age"], r["lifetime"] = p, np.asarray(velocity, dtype=f32).reshape(-1, 3), age, lifetime
    return r


GRAVITY = (0.0, -9.8, 0.0)
DT = 1.0 / 64.0  # (exact in fp32: k steps give an age of exactly k / 64)
BOUNCE = S.ParticleCollisionSettings(restitution=0.5, friction=0.25)
GROUND = P.World([S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))])


def engineered():
    """[(name, P.World, PathSettings, paths, check(result) -> bool)]: the check is asked of the REFERENCE's result, before anything is compared"""
    box = P.World([S.Collider.Box((0.0, 0.0, 0.0), (1.0, 0.5, 1.0), P.TILT)])
    ball = P.World([S.Collider.Sphere((0.0, 0.0, 0.0), 1.0)])
    n = 37
    return [
        ("free fall onto a plane, three bounces", GROUND, S.PathSettings(DT, 37, GRAVITY, 0.0, BOUNCE), path_records((0.25, 0.05, -0.5), (0.5, 0.0, 0.25)),
         lambda r: r["n_contacts"][0] >= 3 and r["status"][0] == S.PATH_RUNNING and r["contact_step"][0] > 0 and r["contact_normal"][0].tolist() == [0, 1, 0]),
        ("start inside a box", box, S.PathSettings(DT, 8, GRAVITY, 0.0, BOUNCE), path_records([(0.1, 0.0, 0.2), (0.0, 0.1, 0.0)], [(1.0, 2.0, 0.5), (0.0, 0.0, 0.0)]),
         lambda r: (r["contact_step"] == 0).all() and not r["contact_normal"].any() and (r["kind"] == S.HIT_COLLIDER).all() and (r["n_contacts"] >= 4).all()),
        ("destroy_on_collision", GROUND, S.PathSettings(DT, 37, GRAVITY, 0.0, S.ParticleCollisionSettings(0.5, 0.25, True)),
         path_records([(0.0, 0.05, 0.0), (0.0, 50.0, 0.0), (0.0, -1.0, 0.0)], [(1.0, 0.0, 0.0)] * 3),
         lambda r: r["status"].tolist() == [S.PATH_DESTROYED, S.PATH_RUNNING, S.PATH_DESTROYED] and r["n_contacts"].tolist() == [1, 0, 1] and r["steps"][2] == 0
         and 0 < r["steps"][0] < 37 and r["contact_step"][0] == r["steps"][0]),
        ("collision disabled", GROUND, S.PathSettings(DT, 37, GRAVITY, 0.125), path_records((0.0, 0.05, 0.0), (1.0, 0.0, 0.0)),
         lambda r: r["n_contacts"][0] == 0 and r["kind"][0] == S.HIT_NONE and r["position"][0][1] < -1.0 and r["steps"][0] == 37),
        ("a mask that sees nothing", GROUND, S.PathSettings(DT, 37, GRAVITY, 0.0, S.ParticleCollisionSettings(0.5, 0.25, False, 2)), path_records((0.0, 0.05, 0.0), (1.0, 0.0, 0.0)),
         lambda r: r["n_contacts"][0] == 0 and r["position"][0][1] < -1.0),
        ("expiry in step 0, in the last step, one step past it", GROUND, S.PathSettings(DT, n, GRAVITY, 0.0, BOUNCE),
         path_records([(0.0, 1.0, 0.0)] * 4, [(1.0, 2.0, 3.0)] * 4, [0.0, 0.0, 0.0, 0.5], [DT, n * DT, (n + 1) * DT, 0.25]),
         lambda r: r["status"].tolist() == [S.PATH_EXPIRED, S.PATH_EXPIRED, S.PATH_RUNNING, S.PATH_EXPIRED] and r["steps"].tolist() == [0, n - 1, n, 0]
         and r["age"].tolist() == [DT, n * DT, n * DT, 0.5 + DT] and r["position"][0].tolist() == [0, 1, 0] and r["velocity"][3].tolist() == [1, 2, 3]),
        ("n_steps 0", GROUND, S.PathSettings(DT, 0, GRAVITY, 0.0, BOUNCE), path_records([(0.0, 1.0, 0.0), (0.0, -1.0, 0.0)], [(1.0, 2.0, 3.0)] * 2, 0.5, [0.25, 9.0]),
         lambda r: (r["status"] == S.PATH_RUNNING).all() and not r["steps"].any() and (r["age"] == 0.5).all() and (r["contact_step"] == NONE).all()
         and r["position"].tolist() == [[0, 1, 0], [0, -1, 0]] and (r["velocity"] == [1, 2, 3]).all()),
        ("n_steps 1", GROUND, S.PathSettings(DT, 1, GRAVITY, 0.0, BOUNCE), path_records([(0.0, 1.0, 0.0), (0.0, -1.0, 0.0)], [(1.0, 2.0, 3.0)] * 2),
         lambda r: r["steps"].tolist() == [1, 1] and r["n_contacts"].tolist() == [0, 4]),
        ("drag only", P.World(), S.PathSettings(DT, 37, (0.0, 0.0, 0.0), 0.5, BOUNCE), path_records((0.0, 0.0, 0.0), (4.0, -2.0, 1.0)),
         lambda r: 0 < r["velocity"][0][0] < 4.0 and r["n_contacts"][0] == 0),
        ("zero velocity: above the ground, inside a ball", ball, S.PathSettings(DT, 5, (0.0, 0.0, 0.0), 0.0, BOUNCE), path_records([(0.0, 3.0, 0.0), (0.25, 0.0, 0.0)], [(0.0, 0.0, 0.0)] * 2),
         lambda r: r["n_contacts"][0] == 0 and r["position"][0].tolist() == [0, 3, 0] and r["n_contacts"][1] >= 4 and r["position"][1][1] > 0
         and r["contact_point"][1].tolist() == [0.25, 0, 0] and not r["velocity"].any()),
    ]


def test_engineered_cases_equal_the_header_in_numpy():
    for name, world, settings, paths, check in engineered():
        want, want_s = reference(world, settings, paths, samples=True)
        assert check(want), (name, want)
        got, got_s = run_host(world, settings, paths)
        assert_results_equal(got, want, name)
        assert_samples_equal(got_s, want_s, name)


# ---- the random set: all six analytic kinds, meshes of 5 and 200 triangles, 500 paths of 37 steps ---------------------------------------------
SEED = 17
N_RANDOM, N_STEPS = 500, 37


@functools.lru_cache(maxsize=None)
def random_world():
    meshes = P.mesh_sizes()[0].meshes
    fan, grid = meshes[2], meshes[3]
    assert len(fan[1]) == 5 and len(grid[1]) == 200
    return P.World(P.mixed_world().colliders, [fan, grid], [(0, (3.0, -2.0, 3.0), P.TILT, 1), (1, (0.0, -2.5, 0.5), P.ID, 3)])


@functools.lru_cache(maxsize=None)
def random_paths(n=N_RANDOM, seed=SEED):
    """spread over the scene, a third above the height field and the fan falling onto them, some starting inside the ball, the box and
    the cylinder; lifetimes around the 37 steps"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform((-5.0, -3.5, -5.0), (5.0, 5.0, 5.0), (n, 3))
    vel = rng.normal(0.0, 3.0, (n, 3))
    k = n // 3
    pos[:k] = rng.uniform((-2.0, -2.2, -1.5), (2.0, -1.5, 2.5), (k, 3))
    pos[k:k + n // 10] = rng.uniform((2.3, -1.9, 2.3), (3.7, -1.4, 3.7), (n // 10, 3))
    vel[:k + n // 10, 1] = -np.abs(vel[:k + n // 10, 1])
    inside = [c.position for c in P.mixed_world().colliders[1:4]]
    for j in range(n // 20):
        pos[n - 1 - j] = np.asarray(inside[j % 3]) + rng.uniform(-0.3, 0.3, 3)
    r = path_records(pos, vel, rng.uniform(0.0, 0.2, n), rng.uniform(0.2, 1.5, n))
    r.setflags(write=False)
    return r


def random_settings(destroy):
    return S.PathSettings(1.0 / 60.0, N_STEPS, GRAVITY, 0.3, S.ParticleCollisionSettings(0.6, 0.2, destroy, 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def random_reference(destroy):
    out = reference(random_world(), random_settings(destroy), random_paths(), samples=True)
    for a in out:
        a.setflags(write=False)
    return out


def assert_the_random_set_covers(bounce, destroy):
    """from the reference's results alone: all three statuses, a path with two contacts or more, an inside contact, a mesh contact"""
    assert set(bounce["status"].tolist()) == {S.PATH_RUNNING, S.PATH_EXPIRED} and (bounce["status"] == S.PATH_EXPIRED).sum() > 50
    assert (destroy["status"] == S.PATH_DESTROYED).sum() > 50 and (destroy["status"] == S.PATH_RUNNING).sum() > 20 and (destroy["status"] == S.PATH_EXPIRED).sum() > 20
    assert (bounce["n_contacts"] >= 2).sum() > 20
    hit = bounce["contact_step"] != NONE
    inside = hit & ~bounce["contact_normal"].any(axis=1)
    assert inside.sum() >= 5 and (bounce["kind"][inside] == S.HIT_COLLIDER).all()
    assert (bounce["kind"] == S.HIT_MESH).sum() > 50 and set(bounce["index"][bounce["kind"] == S.HIT_MESH].tolist()) == {0, 1}
    assert len(set(bounce["index"][bounce["kind"] == S.HIT_COLLIDER].tolist())) >= 4
    assert (bounce["contact_step"][hit] > 0).sum() > 50 and (~hit).sum() > 20


def test_a_world_of_every_kind_and_two_meshes_with_random_paths():
    (bounce, bounce_s), (destroy, destroy_s) = random_reference(False), random_reference(True)
    assert_the_random_set_covers(bounce, destroy)
    for kill, want, want_s in ((False, bounce, bounce_s), (True, destroy, destroy_s)):
        got, got_s = run_host(random_world(), random_settings(kill), random_paths())
        assert_results_equal(got, want, f"random, destroy_on_collision {kill}")
        assert_samples_equal(got_s, want_s, f"random samples, destroy_on_collision {kill}")


def test_samples_are_step_major_and_repeat_the_end():
    """samples[step][path] = {position, age} after that step; the last row is the result; a path that ended in step k holds its final
    values from row k on, and moved before"""
    settings, paths = random_settings(True), random_paths()
    got, smp = run_host(random_world(), settings, paths)
    assert smp.shape == (N_STEPS, len(paths), 4)
    assert smp[-1, :, :3].tobytes() == got["position"].tobytes() and smp[-1, :, 3].tobytes() == got["age"].tobytes()
    ended = np.flatnonzero(got["status"] != S.PATH_RUNNING)
    assert len(ended) > 100
    for i in ended:
        k = int(got["steps"][i])  # the step the path ended in
        assert (smp[k:, i].view(np.uint32) == smp[k, i].view(np.uint32)).all(), i
        if k > 0:
            assert smp[k - 1, i, 3] < smp[k, i, 3] and (got["status"][i] == S.PATH_DESTROYED or smp[k - 1, i, :3].tobytes() == smp[k, i, :3].tobytes())
    one = run_host(random_world(), settings, paths[7:8])
    assert one[0].tobytes() == got[7:8].tobytes() and one[1][:, 0].tobytes() == smp[:, 7].tobytes()
