"""The depth sort of include/firework_hip.h (DEPTH-SORTED INSTANCES) in numpy, written from the header's text: the depth in np.float32
one operation at a time, the key mapping, np.argsort(kind="stable").  The reference of tests/test_depth_sort_cpu.py,
tests/test_gpu_depth_sort.py and tests/test_cpp_host_sorted.py; nothing here reads the library."""
import numpy as np

SORT_BACK_TO_FRONT, SORT_FRONT_TO_BACK = 0, 1
f32 = np.float32


def depth(positions, eye, forward):
    """d = ((p.x - eye.x) * forward.x + (p.y - eye.y) * forward.y) + (p.z - eye.z) * forward.z, every operation rounded to fp32"""
    p = np.asarray(positions, dtype=f32).reshape(-1, 3)
    e, f = np.asarray(eye, dtype=f32), np.asarray(forward, dtype=f32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - e[0], p[:, 1] - e[1], p[:, 2] - e[2]
        xx, yy, zz = dx * f[0], dy * f[1], dz * f[2]
        xy = xx + yy
        d = xy + zz
    assert d.dtype == f32
    return d


def keys_of_depths(d, order):
    """b = bits(d), 0 when d == 0; a = (b >> 31) ? ~b : (b | 0x80000000); k = a front to back, ~a back to front; NaN: 0xFFFFFFFF"""
    d = np.ascontiguousarray(d, dtype=f32)
    b = d.view(np.uint32).copy()
    b[d == 0] = 0
    a = np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k = a if order == SORT_FRONT_TO_BACK else ~a
    assert order in (SORT_BACK_TO_FRONT, SORT_FRONT_TO_BACK)
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def keys(positions, eye, forward, order):
    return keys_of_depths(depth(positions, eye, forward), order)


def order_of(positions, eye, forward, order, cap=None):
    """order[j] = list index of the particle drawn j-th among the first min(count, cap) of the list"""
    p = np.asarray(positions, dtype=f32).reshape(-1, 3)
    if cap is not None:
        p = p[:cap]
    return np.argsort(keys(p, eye, forward, order), kind="stable").astype(np.uint32)
