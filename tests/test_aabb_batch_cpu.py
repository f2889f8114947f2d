"""The batched boxes (include/firework_hip.h: BATCHED BOXES; fw_ctx_aabbs / fw_ctx_aabbs_device) without a GPU: the fw_aabb record has
one layout in the header, the ctypes mirror, the numpy dtype, the Rust source and the C++ mirror; the two entry points and the debug
hook appear in every mirror; and the chunk arithmetic host and device share (csrc/fw_boxes.h: the plan and the locate function) is
checked by a stand-alone C++ program, run plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import subprocess

import pytest

from bevy_firework_amd import _ffi
from bevy_firework_amd import settings as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
FIELDS = ("min", "any", "max", "reserved")
OFFSETS = [0, 12, 16, 28]


def _compile_and_run(tmp_path, name, text, compiler, extra):
    src = tmp_path / name
    src.write_text(text)
    exe = tmp_path / (name + ".exe")
    subprocess.check_call([compiler, "-I", os.path.join(ROOT, "include")] + extra + [str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


def test_fw_aabb_has_one_layout_in_every_mirror(tmp_path):
    want = [32] + OFFSETS
    text = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu\\n",sizeof(fw_aabb),'
            + ",".join(f"offsetof(fw_aabb,{k})" for k in FIELDS) + ");return 0;}\n")
    # the header, through the C compiler; the C++ mirror, which takes the record from the header (through the C++ compiler)
    assert _compile_and_run(tmp_path, "aabb.c", text % "firework_hip.h", "gcc", []) == want
    assert _compile_and_run(tmp_path, "aabb.cpp", text % "firework.hpp", "g++", ["-std=c++17"]) == want
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "std::vector<fw_aabb> aabbs(" in hpp and "void aabbs_device(" in hpp
    # ctypes and numpy
    A = _ffi.Aabb
    assert [n for n, _ in A._fields_] == list(FIELDS)
    assert [C.sizeof(A)] + [getattr(A, k).offset for k in FIELDS] == want
    assert S.AABB_DTYPE.names == FIELDS and [S.AABB_DTYPE.itemsize] + [S.AABB_DTYPE.fields[k][1] for k in FIELDS] == want
    assert S.AABB_DTYPE["min"].shape == (3,) and S.AABB_DTYPE["any"] == "int32" and S.AABB_DTYPE["reserved"] == "uint32"
    # the Rust source: #[repr(C)], the same fields in the same order with the same types (no padding between 4-byte fields)
    rs = open(os.path.join(ROOT, "rust", "src", "hip", "ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\][^\n]*pub struct fw_aabb \{[^\n]*\n\s*([^\n]*)\n\}", rs)
    assert m, "fw_aabb is missing from ffi.rs"
    got = [(n, t) for n, t in re.findall(r"pub (\w+): ([^,]+),", m.group(1))]
    assert got == [("min", "[f32; 3]"), ("any", "i32"), ("max", "[f32; 3]"), ("reserved", "u32")], got


def test_the_entry_points_appear_in_every_mirror():
    """fails where the feature is missing: the header, the library, ctypes, the Rust source, INTEGRATION.md, the C++ mirror, the Python class"""
    from bevy_firework_amd import system

    entry = {"fw_ctx_aabbs", "fw_ctx_aabbs_device"}
    header = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    assert "BATCHED BOXES" in header
    assert entry <= set(re.findall(r"\b(fw_[a-z0-9_]+)\s*\(", header))
    assert "fw_debug_aabb_batch" in open(os.path.join(ROOT, "include", "firework_hip_debug.h")).read()
    bound = {name: args for name, _, args in _ffi.SYMBOLS}
    assert entry | {"fw_debug_aabb_batch"} <= set(bound)
    assert len(bound["fw_ctx_aabbs"]) == 4 and len(bound["fw_ctx_aabbs_device"]) == 4 and len(bound["fw_debug_aabb_batch"]) == 4
    lib = _ffi.load()
    for name in entry | {"fw_debug_aabb_batch"}:
        assert hasattr(lib, name), name
    for path in (("rust", "src", "hip", "ffi.rs"), ("INTEGRATION.md",)):
        assert entry <= set(re.findall(r"pub fn (fw_[a-z0-9_]+)\(", open(os.path.join(ROOT, *path)).read())), path
    assert "fw_ctx_aabbs(" in open(os.path.join(ROOT, "rust", "src", "hip", "render.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "fw_ctx_aabbs(ctx_," in hpp and "fw_ctx_aabbs_device(ctx_," in hpp
    for method in ("aabbs", "aabb_records", "aabbs_device"):
        assert callable(getattr(system.ParticleSystem, method, None)), method
    # a null context is refused before anything is looked at; no GPU is needed to ask
    assert lib.fw_ctx_aabbs(None, 0, None, None) == _ffi.FW_EINVAL and lib.fw_ctx_aabbs_device(None, 0, None, None) == _ffi.FW_EINVAL
    assert lib.fw_debug_aabb_batch(None, None, None, None) == _ffi.FW_EINVAL


# The plan and the locate function of csrc/fw_boxes.h, checked against the definition of a chunk: random lists of bounds (the edge
# sizes around a chunk among them), random partitions of the entries into output places (places without entries among them).
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fw_boxes.h"

struct Entry {
    uint32_t bound, chunk0;
};
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return (uint32_t)(s >> 32);
}
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);       \
            return 1;                                                \
        }                                                            \
    } while (0)

int main() {
    const uint32_t K = FW_BOX_CHUNK;
    const uint32_t edge[] = {0u, 1u, K - 1u, K, K + 1u, 3u * K + 7u, 63u, 64u, 65u, 2u * K, 2u * K + 1u};
    const uint32_t n_edge = (uint32_t)(sizeof edge / sizeof edge[0]);
    unsigned long long lists = 0, chunks_seen = 0;
    for (uint32_t round = 0; round < 400; round++) {
        const uint32_t n = round < 4 ? round : rnd() % 40u;  // (the empty list, one entry, ...)
        std::vector<Entry> tab(n);
        for (uint32_t e = 0; e < n; e++) {
            const uint32_t pick = rnd() % 4u;
            tab[e].bound = round == 4 ? edge[e % n_edge] : pick == 0 ? 0u : pick == 1 ? edge[rnd() % n_edge] : rnd() % (5u * K);
            tab[e].chunk0 = 0xDEADBEEFu;
        }
        // places: a random non-decreasing sequence of first entries, 0 first and n last; repeated values are places without entries
        const uint32_t n_places = 1u + rnd() % 12u;
        std::vector<uint32_t> first(n_places + 1);
        first[0] = 0, first[n_places] = n;
        for (uint32_t p = 1; p < n_places; p++) first[p] = n ? rnd() % (n + 1u) : 0u;
        for (uint32_t p = 1; p < n_places; p++)
            for (uint32_t q = p + 1; q < n_places; q++)
                if (first[q] < first[p]) std::swap(first[p], first[q]);
        std::vector<FwBoxPlace> places(n_places, FwBoxPlace{0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu});
        const uint64_t total = fw_boxes_plan(tab.data(), n, first.data(), n_places, places.data());
        // the running sum; empty entries own no chunk
        uint64_t sum = 0;
        for (uint32_t e = 0; e < n; e++) {
            CHECK(tab[e].chunk0 == sum);
            CHECK(fw_boxes_chunks(tab[e].bound) == (tab[e].bound + K - 1u) / K);
            CHECK((fw_boxes_chunks(tab[e].bound) == 0u) == (tab[e].bound == 0u));
            sum += fw_boxes_chunks(tab[e].bound);
        }
        CHECK(sum == total);
        // every list position of every entry lies in exactly one chunk, and locate(chunk) names that entry and first position
        std::vector<std::vector<uint8_t>> covered(n);
        for (uint32_t e = 0; e < n; e++) covered[e].assign(tab[e].bound, 0);
        for (uint32_t c = 0; c < total; c++) {
            uint32_t f = 0xFFFFFFFFu;
            const uint32_t e = fw_boxes_locate(tab.data(), n, c, &f);
            CHECK(e < n && tab[e].bound > 0u);
            CHECK(c >= tab[e].chunk0 && c - tab[e].chunk0 < fw_boxes_chunks(tab[e].bound));
            CHECK(f == (c - tab[e].chunk0) * K && f < tab[e].bound);
            for (uint32_t li = f; li < f + K && li < tab[e].bound; li++) covered[e][li]++;
            chunks_seen++;
        }
        for (uint32_t e = 0; e < n; e++)
            for (uint32_t li = 0; li < tab[e].bound; li++) CHECK(covered[e][li] == 1);
        // the places tile the entries and the chunks, in order
        uint32_t e_at = 0, c_at = 0;
        for (uint32_t p = 0; p < n_places; p++) {
            CHECK(places[p].e0 == e_at && places[p].c0 == c_at);
            CHECK(places[p].e0 == first[p] && places[p].e1 == first[p + 1]);
            CHECK(places[p].e1 >= places[p].e0 && places[p].c1 >= places[p].c0);
            uint64_t own = 0;
            for (uint32_t e = places[p].e0; e < places[p].e1; e++) own += fw_boxes_chunks(tab[e].bound);
            CHECK(places[p].c1 - places[p].c0 == own);
            CHECK(places[p].e0 == places[p].e1 || places[p].c0 == tab[places[p].e0].chunk0);
            e_at = places[p].e1, c_at = places[p].c1;
        }
        CHECK(e_at == n && c_at == total);
        lists++;
    }
    std::printf("ok %llu lists %llu chunks chunk %u\n", lists, chunks_seen, K);
    return 0;
}
"""


@pytest.mark.parametrize("build", ["plain", "address,undefined"])
def test_plan_and_locate_cover_every_list_position_once(tmp_path, build):
    (tmp_path / "boxes.cpp").write_text(PROGRAM)
    exe = tmp_path / "boxes"
    flags = ["-O1"] if build == "plain" else ["-O1", "-g", "-fsanitize=" + build, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + flags + [str(tmp_path / "boxes.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok 400 lists"), out.stdout + out.stderr
    assert int(out.stdout.split()[3]) > 1000 and int(out.stdout.split()[6]) in (512, 1024, 2048)
