"""The host engine holds every HIP resource of a context in an owning handle (fw_engine.h: HipBuf, HipEvent, HipStream) and
(re)allocates buffers through alloc_buf / grow_buf only: no translation unit allocates, creates or releases one by hand.
What is in flight on top of them -- a pinned staging slot whose copy may still be running -- has one owner as well (Fence, Staging):
no unit waits for an event or keeps a pending flag by hand.  A source check, no GPU."""
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


TIMING = re.compile(r"fw_ctx_measure_\w+|fw_ctx_kernel_timing\w*|fw_debug_\w+")  # (fw_engine_api.cpp: kernel timing)
ENTRY = re.compile(r"^(?:static\s+)?[\w:]+[ \*]+(\w+)\(", re.M)  # a function definition: starts in column 0


def test_only_the_fence_waits_for_an_event():
    """what is in flight has one owner (fw_engine.h: Fence): no translation unit waits for an event by hand, except the kernel-timing
    entry points of fw_engine_api.cpp, which measure with events of their own"""
    found = []
    for u in sorted(glob.glob(os.path.join(CSRC, "fw_engine_*.cpp"))):
        src = open(u).read()
        for m in re.finditer(r"hipEventSynchronize\s*\(", src):
            names = [e.group(1) for e in ENTRY.finditer(src, 0, m.start())]
            if os.path.basename(u) == "fw_engine_api.cpp" and names and TIMING.fullmatch(names[-1]):
                continue
            found.append(f"{os.path.basename(u)}:{src.count(chr(10), 0, m.start()) + 1} (in {names[-1] if names else '?'})")
    assert not found, "\n".join(found)
    header = open(os.path.join(CSRC, "fw_engine.h")).read()
    assert len(re.findall(r"hipEventSynchronize\s*\(", header)) == 1, "fw_engine.h: the one wait is Fence's"


def test_no_pending_flag_is_kept_by_hand():
    """fw_ctx / MeshHost keep no `*_pending` flag, `*_busy` stream or event of their own for the staging sites: the Fence of each
    does.  (snap_pending is something else: pinned rows recognised by their tag; derive_pending is a segment's mode)"""
    src = open(os.path.join(CSRC, "fw_engine.h")).read()
    body = src[src.index("struct fw_ctx {"):src.index("\n};\n", src.index("struct fw_ctx {"))]
    assert "struct MeshHost {" in body
    flags = set(re.findall(r"\b(\w+_pending)\b", body))
    assert flags <= {"snap_pending"}, flags
    for gone in ("ev_coll", "ev_mesh", "ev_xyz", "ev_tab", "ev_rtab", "ev_small", "ev_consumed", "ages_busy", "spin_busy", "ages_cap",
                 "spin_cap", "coll_seq", "mesh_seq", "xyz_seq"):
        assert not re.search(rf"\b{gone}\b", src), gone
