"""What the compiler makes of every form of the far tier of the fused FIFO ring kernel (no GPU: hipcc cross-compiles for gfx950), built the
way tests/test_fuse_wide_occupancy.py builds the first tier's.  For every depth D = 9 .. 16 (FW_FUSE_MAX + 1 .. FW_FUSE_FAR) a translation
unit that includes fw_k_rings.hip for its templates alone (FW_RINGS_TEMPLATES_ONLY) and instantiates fw_k_update_fifo_far<D, WM, NT> over
the four forms of the spin-less launch is compiled for the device with the library's flags and -Rpass-analysis=kernel-resource-usage.
Every form must keep the fifth workgroup per CU the spin-less launch has (five waves per SIMD) and use no scratch (DESIGN.md 4.0, round
32): the figures come from the compiler's remarks alone."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the library's flags (csrc/Makefile: FLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function", "-Wno-unused-value",
         "-Wno-unused-result"]
DEPTHS = list(range(9, 17))
# <WM, NT>: write mask 0, generic, write-only non-temporal, fully non-temporal (fw_k_rings_far.hip: fw_launch_fifo_far_depth)
FORMS = [(0, 0), (-1, 0), (-1, 1), (-1, 2)]


def _int(v):
    return f"Li{'n' if v < 0 else ''}{abs(v)}E"


def _mangled(d, wm, nt):
    """_Z20fw_k_update_fifo_farILi9ELi0ELi0EEv9FwGlobals10FwFifoArgs11FwInlineOps10FwFuseArgs9FwFarArgs for <9, 0, 0>"""
    return "_Z20fw_k_update_fifo_farI" + _int(d) + _int(wm) + _int(nt) + "Ev9FwGlobals10FwFifoArgs11FwInlineOps10FwFuseArgs9FwFarArgs"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("fuse_far_occupancy")

    def compile_depth(D):  # (a unit per depth, side by side: eight short compilations instead of one long one)
        tu = d / f"far_forms_{D}.hip"
        tu.write_text('#define FW_RINGS_TEMPLATES_ONLY\n#include "fw_k_rings.hip"\n' +
                      "".join(f"template __global__ void fw_k_update_fifo_far<{D}, {wm}, {nt}>(FwGlobals, FwFifoArgs, FwInlineOps, FwFuseArgs, FwFarArgs);\n"
                              for wm, nt in FORMS))
        return subprocess.run([HIPCC] + FLAGS + ["-I", CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-x", "hip", str(tu), "-o",
                                                 str(d / f"far_forms_{D}.o")], capture_output=True, text=True)

    with concurrent.futures.ThreadPoolExecutor(max_workers=len(DEPTHS)) as pool:
        done = list(pool.map(compile_depth, DEPTHS))
    for p in done:
        assert p.returncode == 0, p.stderr[-4000:]
    out, name = {}, None
    for line in "".join(p.stderr for p in done).splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_the_header_allows_the_depths_this_file_instantiates():
    text = open(os.path.join(CSRC, "fw_fuse2.h")).read()
    assert re.search(r"#define\s+FW_FUSE_MAX\s+%d\b" % (DEPTHS[0] - 1), text)
    assert re.search(r"#define\s+FW_FUSE_FAR\s+%d\b" % DEPTHS[-1], text)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"WM{f[0]}-NT{f[1]}")
@pytest.mark.parametrize("depth", DEPTHS)
def test_a_far_form_fits_five_workgroups_per_cu(remarks, depth, form):
    r = remarks[_mangled(depth, *form)]
    assert r["Occupancy"] >= 5 and r["ScratchSize"] == 0, r
