"""Depth-sorted instance records without a GPU (include/firework_hip.h: DEPTH-SORTED INSTANCES): the layout of fw_sort_view and the
three entry points in every mirror, and the depth and key arithmetic of csrc/fw_sort.h -- the statements fw_k_depth_keys runs per
lane -- compiled into a stand-alone C++ program with the host flags of csrc/Makefile (-ffp-contract=off -fno-fast-math; once plainly,
once with -fsanitize=address,undefined) and compared bit for bit with tests/sort_ref.py, which is written from the header's text."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref  # noqa: E402

from bevy_firework_amd import _ffi  # noqa: E402
from bevy_firework_amd import settings as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
NAMES = ("fw_ctx_depth_order_device", "fw_ctx_pack_instances_sorted_device", "fw_ctx_pack_instances_sorted")
f32 = np.float32


def test_sort_view_layout_and_entry_points_in_every_mirror(tmp_path):
    """sizeof(fw_sort_view) == 32 and the offset of every field, the C compiler's against the ctypes mirror's; the enum's values; the
    three names in the header, rust/src/hip/ffi.rs, _ffi.SYMBOLS, include/firework.hpp and the library's exports"""
    fields = ("eye", "order", "forward", "reserved")
    src = tmp_path / "sortview.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "firework_hip.h"\nint main(void){printf("%zu %d %d ' + "%zu " * len(fields)
                   + '\\n",sizeof(fw_sort_view),(int)FW_SORT_BACK_TO_FRONT,(int)FW_SORT_FRONT_TO_BACK,'
                   + ",".join(f"offsetof(fw_sort_view,{k})" for k in fields) + ");return 0;}\n")
    exe = tmp_path / "sortview"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    V = _ffi.SortView
    assert [name for name, _ in V._fields_] == list(fields)
    assert got == [32, 0, 1, 0, 12, 16, 28], got
    assert got == [C.sizeof(V), S.SORT_BACK_TO_FRONT, S.SORT_FRONT_TO_BACK] + [getattr(V, k).offset for k in fields]
    assert (sort_ref.SORT_BACK_TO_FRONT, sort_ref.SORT_FRONT_TO_BACK) == (0, 1)
    header = open(os.path.join(ROOT, "include", "firework_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    bound = {name for name, _, _ in _ffi.SYMBOLS}
    exported = set(re.findall(r" T (fw_[a-z0-9_]+)$", subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH], text=True), re.M))
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert f"pub fn {name}(" in rust, name
        assert name + "(" in hpp, name
        assert name in bound and name in exported, name
    assert "pub struct fw_sort_view" in rust and "DEPTH-SORTED INSTANCES" in header
    # the Python mirror marshals field by field
    v = _ffi.make_sort_view(S.SortView(eye=(1.0, 2.0, 3.0), forward=(4.0, 5.0, 6.0), order=S.SORT_FRONT_TO_BACK))
    assert bytes(v) == np.array([1, 2, 3], dtype=f32).tobytes() + np.uint32(1).tobytes() + np.array([4, 5, 6], dtype=f32).tobytes() + np.uint32(0).tobytes()
    assert S.SortView().order == S.SORT_BACK_TO_FRONT and S.SortView().reserved == 0


PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fw_sort.h"
static float bits_f(unsigned b) { float f; memcpy(&f, &b, 4); return f; }
static unsigned f_bits(float f) { unsigned b; memcpy(&b, &f, 4); return b; }
// input: "k <order> <n>" then n depth words -> one key per line; "p <order> eye[3] forward[3] <n>" then n positions of three words ->
// "depth key" per line (all words hex)
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char what = 0;
    unsigned order = 0, n = 0;
    if (fscanf(f, " %c %u", &what, &order) != 2) return 2;
    if (what == 'k') {
        if (fscanf(f, "%u", &n) != 1) return 2;
        std::vector<float> d(n);  // (exactly n on the heap: the sanitizer build sees a read that leaves it)
        for (unsigned i = 0; i < n; i++) {
            unsigned b = 0;
            if (fscanf(f, "%x", &b) != 1) return 2;
            d[i] = bits_f(b);
        }
        for (unsigned i = 0; i < n; i++) printf("%08x\n", fw_sort_key_of_depth(d[i], order));
    } else {
        FwSortView v{};
        v.order = order;
        unsigned w[6];
        for (int c = 0; c < 6; c++)
            if (fscanf(f, "%x", &w[c]) != 1) return 2;
        for (int c = 0; c < 3; c++) v.eye[c] = bits_f(w[c]), v.forward[c] = bits_f(w[3 + c]);
        if (fscanf(f, "%u", &n) != 1) return 2;
        for (unsigned i = 0; i < n; i++) {
            unsigned p[3];
            if (fscanf(f, "%x %x %x", &p[0], &p[1], &p[2]) != 3) return 2;
            const float d = fw_sort_depth(bits_f(p[0]), bits_f(p[1]), bits_f(p[2]), v);
            printf("%08x %08x\n", f_bits(d), fw_sort_key(bits_f(p[0]), bits_f(p[1]), bits_f(p[2]), v));
        }
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("sortkey")
    (d / "sortkey.cpp").write_text(PROGRAM)
    exe = d / "sortkey"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "sortkey.cpp"), "-o", str(exe)])
    return str(exe), d


def _hex(a):
    return " ".join(f"{int(x):08x}" for x in np.ascontiguousarray(a, dtype=f32).reshape(-1).view(np.uint32))


def _keys(program, depths, order, name):
    exe, d = program
    path = d / (name + ".txt")
    path.write_text(f"k {order} {len(depths)}\n{_hex(depths)}\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.array([int(x, 16) for x in r.stdout.split()], dtype=np.uint32)


def _special_depths():
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,  # +-0, denormals, FLT_MIN
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,  # +-FLT_MAX, +-inf
            0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5, 0xFFDEAD00,  # NaNs: both signs, payloads
            0x3F800000, 0xBF800000]
    return np.array(bits, dtype=np.uint32).view(f32)


@pytest.mark.parametrize("order", [sort_ref.SORT_BACK_TO_FRONT, sort_ref.SORT_FRONT_TO_BACK])
def test_keys_of_special_depths_match_the_header(program, order):
    d = _special_depths()
    got = _keys(program, d, order, f"special{order}")
    want = sort_ref.keys_of_depths(d, order)
    assert np.array_equal(got, want), [(f"{a:08x}", f"{b:08x}") for a, b in zip(got, want)]
    assert got[0] == got[1]  # -0 and +0 tie
    nan = np.isnan(d)
    assert (got[nan] == 0xFFFFFFFF).all() and (got[~nan] != 0xFFFFFFFF).all()
    # the header's own figures, not only the helper's: -inf and +inf are the ends of the image of `a`
    a = got if order == sort_ref.SORT_FRONT_TO_BACK else ~got
    assert a[11] == 0x007FFFFF and a[10] == 0xFF800000 and a[0] == 0x80000000


@pytest.mark.parametrize("order", [sort_ref.SORT_BACK_TO_FRONT, sort_ref.SORT_FRONT_TO_BACK])
def test_keys_of_random_depths_are_monotonic_and_only_nan_is_last(program, order):
    """a few thousand floats drawn as BIT PATTERNS (every exponent, denormals, infinities and NaNs among them) and a few thousand drawn as
    values: bit for bit the reference's; k never descends as d ascends (never ascends, back to front), strictly where d differs"""
    rng = np.random.default_rng(2020 + order)
    d = np.concatenate([rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(f32), rng.normal(size=2048).astype(f32) * f32(100.0),
                        _special_depths()])
    got = _keys(program, d, order, f"random{order}")
    assert np.array_equal(got, sort_ref.keys_of_depths(d, order))
    nan = np.isnan(d)
    assert nan.any() and (got[nan] == 0xFFFFFFFF).all() and (got[~nan] != 0xFFFFFFFF).all()
    dd, kk = d[~nan], got[~nan].astype(np.int64)
    by_depth = np.argsort(dd, kind="stable")
    dd, kk = dd[by_depth], kk[by_depth]
    step = np.diff(kk) if order == sort_ref.SORT_FRONT_TO_BACK else -np.diff(kk)
    assert (step >= 0).all()
    assert ((step > 0) == (np.diff(dd) > 0)).all()  # equal depths (+-0 among them) tie, different depths never do


def test_depth_is_rounded_operation_by_operation(program):
    """positions and views whose products and sums round differently when fused or reassociated: the bits of d and of k, both orders"""
    rng = np.random.default_rng(77)
    exe, tmp = program
    for case in range(6):
        p = (rng.normal(size=(512, 3)) * 10.0 ** rng.integers(-3, 4)).astype(f32)
        eye = (rng.normal(size=3) * 3.0).astype(f32) if case else p[:100].mean(axis=0).astype(f32)
        fwd = rng.normal(size=3).astype(f32) if case != 1 else np.zeros(3, dtype=f32)
        if case == 2:
            p[::7] = eye  # exact zeros of both signs after the products
            p[::11, 0] = np.inf
            p[::13, 1] = np.nan
        order = case & 1
        path = tmp / f"depth{case}.txt"
        path.write_text(f"p {order} {_hex(eye)} {_hex(fwd)} {len(p)}\n" + "\n".join(_hex(row) for row in p) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [ln.split() for ln in r.stdout.strip().splitlines()]
        got_d = np.array([int(a, 16) for a, _ in rows], dtype=np.uint32)
        got_k = np.array([int(b, 16) for _, b in rows], dtype=np.uint32)
        want_d = sort_ref.depth(p, eye, fwd)
        same = (got_d == want_d.view(np.uint32)) | (np.isnan(want_d) & np.isnan(got_d.view(f32)))  # (a NaN's payload is not part of the definition)
        assert same.all(), case
        assert np.array_equal(got_k, sort_ref.keys(p, eye, fwd, order)), case
