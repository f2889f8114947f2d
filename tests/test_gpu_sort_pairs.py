"""fw_launch_sort_pairs (csrc/fw_k_sort.hip) against its own contract (csrc/fw_kernels.h: "sort: the n pairs at the start of `scratch` ...
sorted by ascending key, ties in incoming order; the sorted indices end at scratch + n_upper or, d_idx_out not null, there instead (n
entries; nothing at or beyond n is written)"), without the engine: tests/sort_pairs_check.hip is built with csrc/fw_k_sort.hip alone and
sorts the pairs of one case file per process.  The reference is numpy's stable argsort and nothing else; every word of every output and
of every guard is compared, no tolerance exists.  The shapes are those at which the kernels change: fw_k_sort_scan gives each of its 256
lanes ceil(tiles / 256) columns (tiles = ceil(n_upper / 2048)), so 524 289 elements are the first at which a lane carries a running sum
over two columns; a device count far below n_upper leaves whole tiles empty; and the key patterns make single passes, single waves,
rounds and tiles carry the whole order.  Needs an MI355X (the build-only test does not)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
EXE = os.path.join(HERE, "sort_pairs_check")
SEED = 2121  # every case draws from np.random.default_rng([SEED, its own number])
T = 2048  # FW_SORT_TILE of csrc/fw_sort.h
POISON = 0xA5A5A5A5
# seconds per harness process: three times what tests/test_cpp_host_sorted.py::test_cpp_mirror_and_python_mirror_sort_identically takes at the
# commit before this suite (its slowest entry: 0.53 s on an MI355X, 0.46 s in profiles/r20/sort_gpu_tests.txt) is 1.59 s, rounded up
TIMEOUT = 2
u32 = np.uint32


def build():
    """tests/sort_pairs_check from tests/sort_pairs_check.hip + csrc/fw_k_sort.hip with the FLAGS of csrc/Makefile (when older than a source)"""
    srcs = [os.path.join(HERE, "sort_pairs_check.hip"), os.path.join(CSRC, "fw_k_sort.hip")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("fw_kernels.h", "fw_sort.h", "fw_device.h", "Makefile")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return EXE
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags, flags
    subprocess.check_call([hipcc] + flags + ["-I", CSRC, "-x", "hip"] + srcs + ["-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def exe():
    return build()


def reference(keys, values, count, n_upper):
    """-> n = min(count, n_upper), the first n values and the first n keys in the stable ascending order of those keys"""
    n = min(int(count), int(n_upper))
    order = np.argsort(keys[:n], kind="stable")
    return n, values[:n][order], keys[:n][order]


def run_case(exe, tmp_path, keys, values, count, with_out):
    """one process, one case -> (returncode, stderr, the OUT file's sections or None)"""
    n_upper = len(keys)
    assert keys.dtype == u32 and values.dtype == u32 and len(values) == n_upper
    case, out = str(tmp_path / "case.u32"), str(tmp_path / "out.u32")
    with open(case, "wb") as f:
        np.array([n_upper, count, int(with_out)], dtype=u32).tofile(f)
        keys.tofile(f)
        values.tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=TIMEOUT)
    os.remove(case)
    if r.returncode != 0:
        return r.returncode, r.stderr, None
    w = np.fromfile(out, dtype=u32)
    os.remove(out)
    g = int(w[0])
    assert g >= 4096 and len(w) == 1 + 2 * n_upper + 2 * g + (n_upper + 2 * g)
    cut = np.cumsum([1, n_upper, n_upper, g, g])
    got = {"keys": w[cut[0]:cut[1]], "idx": w[cut[1]:cut[2]], "guard_lo": w[cut[2]:cut[3]], "guard_hi": w[cut[3]:cut[4]], "out_all": w[cut[4]:], "g": g}
    return 0, r.stderr, got


def check_case(exe, tmp_path, keys, values, count, with_out, what=""):
    n_upper = len(keys)
    rc, err, got = run_case(exe, tmp_path, keys, values, count, with_out)
    assert rc == 0, (what, rc, err)
    n, want_idx, want_keys = reference(keys, values, count, n_upper)
    g = got["g"]
    assert np.array_equal(got["idx"][:n], want_idx), (what, "sorted indices", n, n_upper, np.flatnonzero(got["idx"][:n] != want_idx)[:8])
    assert (got["guard_lo"] == POISON).all() and (got["guard_hi"] == POISON).all(), (what, "a guard of the scratch was written")
    out_all = got["out_all"]
    if with_out:
        assert np.array_equal(out_all[g:g + n], want_idx), (what, "d_idx_out")
        assert (out_all[g + n:] == POISON).all() and (out_all[:g] == POISON).all(), (what, "d_idx_out was written at or beyond n, or in front of 0")
    else:
        assert np.array_equal(got["keys"][:n], want_keys), (what, "sorted keys", n, n_upper)
        assert (out_all == POISON).all(), (what, "a buffer that was not passed was written")


def _only_once(fw_path):
    if fw_path != "fifo":
        pytest.skip("no context is created, the update path means nothing to the sort: one run, under the path matrix's fifo entry")


def _values(rng, n_upper, random_words):
    """the list indices the engine passes, or arbitrary words (values >= n_upper, repeats): the sort carries values, it never rebuilds them"""
    if not random_words:
        return np.arange(n_upper, dtype=u32)
    v = rng.integers(0, 1 << 32, size=n_upper, dtype=np.uint64).astype(u32)
    v[::7] = v[0]
    v[1::11] = u32(0xFFFFFFFF)
    return v


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
N_PER2 = 256 * T + 1  # 524 289: 257 tiles, per = 2 (lane 128 holds one column, the lanes above it none)
SHAPES = ([(n, n) for n in (1, 64, T - 1, T, T + 1, 256 * T, N_PER2, 513 * T + 1, 700 * T + 77)]  # count == n_upper; 700 tiles: per = 3
          + [(3 * T + 5, c) for c in (0, 1, 255, T - 1, T + 1, 2 * T)] + [(600 * T, c) for c in (0, T + 1, N_PER2)]  # count < n_upper
          + [(n, c) for n in (5000, N_PER2) for c in (n + 1, 0xFFFFFFFF)])  # count > n_upper


@pytest.mark.gpu
@pytest.mark.parametrize("with_out", [False, True], ids=["in the scratch", "d_idx_out"])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"n_upper={n}-count={c}" for n, c in SHAPES])
def test_shapes(fw_path, exe, tmp_path, k, with_out):
    _only_once(fw_path)
    n_upper, count = SHAPES[k]
    rng = np.random.default_rng([SEED, k])
    keys = rng.integers(0, 1 << 32, size=n_upper, dtype=np.uint64).astype(u32)
    check_case(exe, tmp_path, keys, _values(rng, n_upper, (k + with_out) & 1), count, with_out, what=f"n_upper={n_upper} count={count}")


# ---- key patterns ------------------------------------------------------------------------------------------------------------------------
def _byte(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint64).astype(u32)


def _cloud(rng, n):
    """a normal cloud seen from an eye far outside: one sign, a few values in the two high digits"""
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    k = sort_ref.keys(pos, (40.0, -30.0, 25.0), (0.3, -0.5, 0.8), sort_ref.SORT_BACK_TO_FRONT)
    assert len(np.unique(k >> u32(31))) == 1 and len(np.unique(k >> u32(16))) < 64
    return k


def _one_tile(e, inside, outside):
    return np.where((e >> u32(11)) == 1, u32(inside), u32(outside)).astype(u32)


PATTERNS = {
    "uniform": lambda rng, e: rng.integers(0, 1 << 32, size=len(e), dtype=np.uint64).astype(u32),
    "all 0": lambda rng, e: np.zeros(len(e), dtype=u32),
    "all 0xFFFFFFFF": lambda rng, e: np.full(len(e), 0xFFFFFFFF, dtype=u32),
    "ascending": lambda rng, e: e.copy(),
    "descending": lambda rng, e: ~e,
    **{f"byte {b} alone": (lambda rng, e, b=b: _byte(rng, len(e)) << u32(8 * b)) for b in range(4)},  # one pass carries the order, three are the identity
    **{f"byte {b} random, the others 255": (lambda rng, e, b=b: (~(u32(0xFF) << u32(8 * b))) & u32(0xFFFFFFFF) | (_byte(rng, len(e)) << u32(8 * b))) for b in range(4)},
    "eight distinct keys": lambda rng, e: rng.integers(0, 1 << 32, size=8, dtype=np.uint64).astype(u32)[rng.integers(0, 8, size=len(e))],
    "low digit = lane": lambda rng, e: e & u32(63),  # 64 distinct digits in every wave: every peer group is one lane
    "low digit = wave": lambda rng, e: (e >> u32(6)) & u32(3),  # whole waves in one digit
    "low digit = round": lambda rng, e: (e >> u32(8)) & u32(7),  # whole rounds in one digit
    "one tile of digit 255 among 0": lambda rng, e: _one_tile(e, 255, 0),
    "one tile of digit 0 among 255": lambda rng, e: _one_tile(e, 0, 255),
    "a cloud from far outside": lambda rng, e: _cloud(rng, len(e)),
}
assert len(PATTERNS) == 20


@pytest.mark.gpu
@pytest.mark.parametrize("with_out", [False, True], ids=["in the scratch", "d_idx_out"])
@pytest.mark.parametrize("n_upper", [3 * T + 5, N_PER2])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_key_patterns(fw_path, exe, tmp_path, name, n_upper, with_out):
    _only_once(fw_path)
    k = list(PATTERNS).index(name)
    rng = np.random.default_rng([SEED, 1000 + k, n_upper])
    keys = np.ascontiguousarray(PATTERNS[name](rng, np.arange(n_upper, dtype=u32)), dtype=u32)
    assert keys.dtype == u32 and len(keys) == n_upper
    if name.startswith("byte") and "alone" in name:
        b = int(name.split()[1])
        assert not (keys & ~(u32(0xFF) << u32(8 * b))).any() and len(np.unique(keys)) == 256
    if "the others 255" in name:
        b = int(name.split()[1])
        assert ((keys | (u32(0xFF) << u32(8 * b))) == 0xFFFFFFFF).all() and len(np.unique(keys)) == 256
    if name == "eight distinct keys":
        assert len(np.unique(keys)) == 8
    check_case(exe, tmp_path, keys, _values(rng, n_upper, (k + with_out + (n_upper & 1)) & 1), n_upper, with_out, what=f"{name} n_upper={n_upper}")


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_sort_pairs_check_builds(tmp_path):
    """the program builds for gfx950; without a device it says so and exits 1 (with one, it sorts the twelve pairs); and the reference the
    GPU cases trust, on twelve pairs with ties written out by hand"""
    exe = build()
    keys = np.array([5, 3, 5, 0, 0xFFFFFFFF, 3, 3, 0, 5, 0x80000000, 3, 0], dtype=u32)
    values = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111], dtype=u32)
    by_hand = [103, 107, 111, 101, 105, 106, 110, 100, 102, 108, 109, 104]
    n, idx, srt = reference(keys, values, 12, 12)
    assert n == 12 and idx.tolist() == by_hand and srt.tolist() == [0, 0, 0, 3, 3, 3, 3, 5, 5, 5, 0x80000000, 0xFFFFFFFF]
    n, idx, srt = reference(keys, values, 5, 12)  # (a count below n_upper: the first five pairs alone)
    assert n == 5 and idx.tolist() == [103, 101, 100, 102, 104] and srt.tolist() == [0, 3, 5, 5, 0xFFFFFFFF]
    n, idx, _ = reference(keys, values, 0xFFFFFFFF, 12)
    assert n == 12 and idx.tolist() == by_hand
    import torch

    if torch.cuda.is_available():
        check_case(exe, tmp_path, keys, values, 12, False, what="twelve pairs")
        return
    rc, err, got = run_case(exe, tmp_path, keys, values, 12, False)
    assert rc == 1 and got is None and "no CPU fallback" in err, (rc, err)
    r = subprocess.run([exe, str(tmp_path / "missing"), str(tmp_path / "out")], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 2 and "not a case file" in r.stderr
