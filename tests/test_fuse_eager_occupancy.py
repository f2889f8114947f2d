"""What the compiler makes of the second set of fused forms of the FIFO ring kernel, fw_k_update_fifo2_eager<D, WM, NT> (round 27: the forms
whose spawning workgroups spin what they spawn, launched under FW_NEWBORN_SPIN=1; csrc/fw_k_rings_fuse2_eager.hip), built the way
tests/test_fuse_wide_occupancy.py builds fw_k_update_fifo2, whose depths, forms and flags this file borrows: every form must keep five
waves per SIMD and use no scratch, so that the switch compares two kernels of one occupancy.  No GPU: hipcc cross-compiles for gfx950."""
import concurrent.futures
import os
import re
import subprocess

import pytest

from test_fuse_wide_occupancy import CSRC, DEPTHS, FLAGS, FORMS, HIPCC, _int


def _mangled(d, wm, nt):
    return "_Z23fw_k_update_fifo2_eagerI" + _int(d) + _int(wm) + _int(nt) + "Ev9FwGlobals10FwFifoArgs11FwInlineOps10FwFuseArgs"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("fuse_eager_occupancy")

    def compile_depth(D):
        tu = d / f"eager_forms_{D}.hip"
        tu.write_text('#define FW_RINGS_TEMPLATES_ONLY\n#include "fw_k_rings.hip"\n' +
                      "".join(f"template __global__ void fw_k_update_fifo2_eager<{D}, {wm}, {nt}>(FwGlobals, FwFifoArgs, FwInlineOps, FwFuseArgs);\n" for wm, nt in FORMS))
        return subprocess.run([HIPCC] + FLAGS + ["-I", CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-x", "hip", str(tu), "-o",
                                                 str(d / f"eager_forms_{D}.o")], capture_output=True, text=True)

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


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"WM{f[0]}-NT{f[1]}")
@pytest.mark.parametrize("depth", DEPTHS)
def test_an_eager_fused_form_fits_five_workgroups_per_cu(remarks, depth, form):
    r = remarks[_mangled(depth, *form)]
    assert r["Occupancy"] >= 5 and r["ScratchSize"] == 0, r
