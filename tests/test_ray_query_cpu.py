"""The ray-cast query's ABI without a GPU: fw_ray / fw_ray_hit as the C compiler lays them out against the numpy dtypes and the
ctypes mirrors, the two entry points exported by the library and declared in every mirror, and the kernel unit in the build."""
import ctypes as C
import os
import re
import subprocess

from bevy_firework_amd import _ffi
from bevy_firework_amd import settings as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_FIELDS = ("origin", "max_distance", "dir", "filter_mask")
HIT_FIELDS = ("distance", "normal", "kind", "index", "triangle", "reserved")


def test_ray_and_hit_layouts_match_the_header(tmp_path):
    """sizeof and the offset of every field, the C compiler's against RAY_DTYPE / RAY_HIT_DTYPE and the ctypes mirrors"""
    exprs = ["sizeof(fw_ray)", "sizeof(fw_ray_hit)"] + [f"offsetof(fw_ray,{k})" for k in RAY_FIELDS] + [f"offsetof(fw_ray_hit,{k})" for k in HIT_FIELDS] \
        + ["(size_t)FW_HIT_NONE", "(size_t)FW_HIT_COLLIDER", "(size_t)FW_HIT_MESH", "(size_t)FW_ABI_VERSION"]
    src = tmp_path / "ray.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "firework_hip.h"\nint main(void){printf("' + " ".join(["%zu"] * len(exprs))
                   + '\\n",' + ",".join(exprs) + ");return 0;}\n")
    exe = tmp_path / "ray"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [32, 32]
    for dtype, mirror, fields in ((S.RAY_DTYPE, _ffi.Ray, RAY_FIELDS), (S.RAY_HIT_DTYPE, _ffi.RayHit, HIT_FIELDS)):
        assert dtype.names == fields and [name for name, _ in mirror._fields_] == list(fields)
        assert dtype.itemsize == C.sizeof(mirror) == 32
    want = [32, 32] + [S.RAY_DTYPE.fields[k][1] for k in RAY_FIELDS] + [S.RAY_HIT_DTYPE.fields[k][1] for k in HIT_FIELDS]
    assert got[:-4] == want, (got, want)
    assert got[:-4] == [32, 32] + [getattr(_ffi.Ray, k).offset for k in RAY_FIELDS] + [getattr(_ffi.RayHit, k).offset for k in HIT_FIELDS]
    assert got[-4:] == [S.HIT_NONE, S.HIT_COLLIDER, S.HIT_MESH, 5]
    assert S.RAY_DTYPE["filter_mask"] == "u4" and S.RAY_HIT_DTYPE["kind"] == "i4" and S.RAY_HIT_DTYPE["triangle"] == "u4"


def test_query_entry_points_are_exported_and_declared_in_every_mirror():
    names = ("fw_ctx_cast_rays", "fw_ctx_cast_rays_device")
    lib = _ffi.load()
    bound = {name for name, _, _ in _ffi.SYMBOLS}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in bound, name
        assert re.search(rf" T {name}$", exported, re.M), name
        assert re.search(rf"fw_status {name}\(fw_ctx \*ctx, ", header), name
        for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
            assert re.search(rf"pub fn {name}\(ctx: \*mut fw_ctx, ", open(os.path.join(ROOT, mirror)).read()), (mirror, name)
        assert f"{name}(ctx_" in open(os.path.join(ROOT, "include", "firework.hpp")).read(), name
    for mirror in ("INTEGRATION.md", os.path.join("rust", "src", "hip", "ffi.rs")):
        text = open(os.path.join(ROOT, mirror)).read()
        assert "pub struct fw_ray {" in text and "pub struct fw_ray_hit {" in text, mirror
        assert re.search(r"pub origin: \[f32; 3\], pub max_distance: f32, pub dir: \[f32; 3\], pub filter_mask: u32", text), mirror
        assert re.search(r"pub distance: f32, pub normal: \[f32; 3\], pub kind: i32, pub index: u32, pub triangle: u32, pub reserved: u32", text), mirror
    from bevy_firework_amd.system import ParticleSystem

    assert callable(ParticleSystem.cast_rays) and callable(ParticleSystem.cast_rays_device)


def test_query_kernel_is_a_unit_of_the_build_and_runs_the_shared_cast():
    """fw_k_query.hip is built into every form of the library and calls fw_collide.h's cast: no arithmetic of its own"""
    mk = open(os.path.join(ROOT, "bevy_firework_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\bfw_k_query\.hip\b", mk, re.M) and re.search(r"^KUNITS\s*:=.*\bfw_k_query\b", mk, re.M)
    assert re.search(r"^UNITS\s*:=.*\bfw_engine_query\.cpp\b", mk, re.M) and re.search(r"^HOSTUNITS\s*:=.*\bfw_engine_query\b", mk, re.M)
    src = open(os.path.join(ROOT, "bevy_firework_amd", "csrc", "fw_k_query.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "fw_cast_ray(" in code and "FwHitId" in code
    assert not re.search(r"\b(sqrtf|fw_cross|fw_dot3|fw_ray_collider)\b", code), "the query kernel must not copy the cast's arithmetic"
