"""The host engine holds every HIP resource of a context in an owning handle (fw_engine.h: HipBuf, HipEvent, HipStream) and
(re)allocates buffers through alloc_buf / grow_buf only: no translation unit allocates, creates or releases one by hand.
A source check, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")
RAW = re.compile(r"\b(hipMalloc\w*|hipExtMallocWithFlags|hipHostMalloc|hipFree|hipHostFree|hipEventCreate\w*|hipEventDestroy|"
                 r"hipStreamCreate\w*|hipStreamDestroy)\s*\(")


def test_engine_units_make_no_raw_resource_calls():
    units = sorted(glob.glob(os.path.join(CSRC, "fw_engine_*.cpp")))
    assert len(units) >= 6, units
    found = []
    for u in units:
        for n, line in enumerate(open(u), 1):
            if RAW.search(line):
                found.append(f"{os.path.basename(u)}:{n}: {line.strip()}")
    assert not found, "\n".join(found)


def test_raw_resource_calls_live_in_the_owners_and_helpers():
    """in fw_engine.h the calls sit inside the owner types (from `enum class Mem` to the end of HipStream) and hip_alloc"""
    src = open(os.path.join(CSRC, "fw_engine.h")).read()
    owners = (src.index("enum class Mem"), src.index("class HipStream"))
    owners = (owners[0], src.index("\n};\n", owners[1]))
    helper = (src.index("inline hipError_t hip_alloc("), src.index("\n}\n", src.index("inline hipError_t hip_alloc(")))
    seen = set()
    for m in RAW.finditer(src):
        assert owners[0] <= m.start() < owners[1] or helper[0] <= m.start() < helper[1], \
            f"{m.group(1)} outside the owners: line {src.count(chr(10), 0, m.start()) + 1}"
        seen.add(m.group(1))
    assert {"hipMalloc", "hipExtMallocWithFlags", "hipHostMalloc", "hipFree", "hipHostFree", "hipEventCreateWithFlags",
            "hipEventDestroy", "hipStreamCreateWithFlags", "hipStreamDestroy"} <= seen, seen
