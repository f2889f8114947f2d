"""What the compiler makes of the FIFO ring kernel's headline forms (no GPU: hipcc cross-compiles for gfx950).  A translation unit that
includes fw_k_rings.hip for its templates alone (FW_RINGS_TEMPLATES_ONLY) and instantiates five forms of fw_k_update_fifo is compiled for the
device with the library's flags and -Rpass-analysis=kernel-resource-usage.  The SPINLESS forms exist to fit five
workgroups of four waves on a CU -- five waves per SIMD, at most 102 VGPRs -- without scratch; the form that finds out per workgroup must
stay what it was: four waves, no scratch."""
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
# <INST, WM, NT, COLL, TR, Q0PL, SPINLESS>: the headline form of configs[1] as it was, and the four spin-less ones
OLD = "false, 0, 0, 0, FW_ROUNDS, true, false"
SPINLESS = ["false, 0, 0, 0, FW_ROUNDS, true, true", "false, -1, 0, 0, FW_ROUNDS, true, true", "false, -1, 1, 0, FW_ROUNDS, true, true",
            "false, -1, 2, 0, FW_ROUNDS, true, true"]


def _mangled(args):
    """_Z16fw_k_update_fifoILb0ELi0ELi0ELi0ELi4ELb1ELb1EEv9FwGlobals10FwFifoArgs11FwInlineOps for "false, 0, 0, 0, FW_ROUNDS, true, true" """
    parts = []
    for a in (x.strip() for x in args.split(",")):
        if a in ("true", "false"):
            parts.append("Lb1E" if a == "true" else "Lb0E")
        else:
            v = 4 if a == "FW_ROUNDS" else int(a)
            parts.append(f"Li{'n' if v < 0 else ''}{abs(v)}E")
    return "_Z16fw_k_update_fifoI" + "".join(parts) + "Ev9FwGlobals10FwFifoArgs11FwInlineOps"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("rings_occupancy")
    tu = d / "rings_forms.hip"
    tu.write_text('#define FW_RINGS_TEMPLATES_ONLY\n#include "fw_k_rings.hip"\n' +
                  "".join(f"template __global__ void fw_k_update_fifo<{a}>(FwGlobals, FwFifoArgs, FwInlineOps);\n" for a in [OLD] + SPINLESS))
    p = subprocess.run([HIPCC] + FLAGS + ["-I", CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-x", "hip", str(tu), "-o",
                                          str(d / "rings_forms.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def test_fw_rounds_is_four():
    text = open(os.path.join(CSRC, "fw_dev.h")).read() + open(os.path.join(CSRC, "fw_kernels.h")).read() + open(os.path.join(CSRC, "fw_device.h")).read()
    assert re.search(r"#define\s+FW_ROUNDS\s+4\b", text), "the mangled names of this test spell the four-round tile"


@pytest.mark.parametrize("args", SPINLESS)
def test_a_spinless_form_fits_five_workgroups_per_cu(remarks, args):
    r = remarks[_mangled(args)]
    assert r["Occupancy"] >= 5 and r["ScratchSize"] == 0, r


def test_the_form_that_finds_out_per_workgroup_is_what_it_was(remarks):
    r = remarks[_mangled(OLD)]
    assert r["Occupancy"] == 4 and r["ScratchSize"] == 0, r
