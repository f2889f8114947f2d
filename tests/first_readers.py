"""The packed and the depth-sorted forms as the FIRST reader of a FIFO ring whose ages are stale (tests/test_gpu_fifo_ages.py) or whose
spin is deferred (tests/test_gpu_spin_defer.py): what the two suites share.  Every reader takes a Run of either suite (run.system,
run.pair.gpu) and returns what it read; none of them asks for anything else first except the count, which writes nothing back
(fw_engine_api.cpp: Ages::leave).  The independent check takes the unsorted instances() of the run WITHOUT the rule, permutes them by
tests/sort_ref.py and compares bytes, so a first reader is never judged by the other run's first reader alone."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref  # noqa: E402
from test_gpu_ray_query import _ctx_stream  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

PAD = 64
POISON = 0xA5
# (the spawners of both suites stand at (1, 2, 3) and throw their particles upwards: an eye inside the cloud, a forward vector that is not normalised)
VIEW = S.SortView(eye=(1.0, 2.5, 3.0), forward=(0.3, -0.5, 0.8), order=S.SORT_BACK_TO_FRONT)


def _device_buffer(system, n_bytes):
    import torch

    with _ctx_stream(system):
        return torch.full((n_bytes,), POISON, dtype=torch.uint8, device="cuda")


def _records_of(system, buf, n, cap, ub):
    system.synchronize()
    assert n <= ub <= cap, (n, ub, cap)
    got = buf.cpu().numpy()
    assert (got[n * 64:] == POISON).all(), "records at and beyond the count were written"
    return got[:n * 64].view(S.INSTANCE_DTYPE).copy()


def sorted_device(run):
    """fw_ctx_pack_instances_sorted_device"""
    d, system = run.pair.gpu, run.system
    n = d.count(0)
    buf = _device_buffer(system, (n + PAD) * 64)
    ub = system.pack_instances_sorted_device(d, VIEW, buf.data_ptr(), n + PAD)
    return _records_of(system, buf, n, n + PAD, ub)


def sorted_host(run):
    """fw_ctx_pack_instances_sorted"""
    return run.pair.gpu.instances_sorted(VIEW)


def unsorted_device(run):
    """fw_spawner_pack_instances_device, as tools/sorted_pack.py calls it"""
    d, system = run.pair.gpu, run.system
    n = d.count(0)
    buf = _device_buffer(system, (n + PAD) * 64)
    ub = C.c_uint64()
    system._check(system._lib.fw_spawner_pack_instances_device(system._ctx, d.handle, 0, C.c_void_p(buf.data_ptr()), n + PAD, C.byref(ub)))
    return _records_of(system, buf, n, n + PAD, int(ub.value))


def unsorted_host(run):
    """fw_spawner_pack_instances"""
    return run.pair.gpu.instances(0)


# name -> (the reader, whether its records come depth-sorted)
PACK_READERS = {"fw_ctx_pack_instances_sorted_device": (sorted_device, True), "fw_ctx_pack_instances_sorted": (sorted_host, True),
                "fw_spawner_pack_instances_device": (unsorted_device, False), "fw_spawner_pack_instances": (unsorted_host, False)}


def depth_order(run, buf, cap):
    """fw_ctx_depth_order_device into a poisoned buffer of `cap` entries -> the order"""
    d, system = run.pair.gpu, run.system
    n = d.count(0)
    assert n <= cap
    buf.fill_(POISON)
    ub = system.depth_order_device(d, VIEW, buf.data_ptr(), cap)
    system.synchronize()
    assert n <= ub <= cap, (n, ub, cap)
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[n:].view(np.uint8) == POISON).all(), "order entries at and beyond the count were written"
    return got[:n].copy()


def order_buffer(run, cap):
    return _device_buffer(run.system, cap * 4)


def want_order(unsorted):
    return sort_ref.order_of(unsorted["position"], VIEW.eye, VIEW.forward, VIEW.order)


def check_records(first, unsorted_without_rule, is_sorted, what):
    """the first reader's records against the unsorted pack of the run without the rule, same frame"""
    u = unsorted_without_rule
    want = u[want_order(u)] if is_sorted else u
    assert len(first) == len(u) and first.tobytes() == want.tobytes(), what
    if is_sorted:
        assert first.tobytes() != u.tobytes(), (what, "the depth order is the list's: the case sorts nothing")


def stale_planes_would_show(parts, unsorted, spawn_rotation, dt):
    """the particles of the frame behind a first reader: several cohorts of different ages (scale and colours follow the age), and -- a
    spinning type, spawn_rotation given -- everybody older than a frame has left the rotation it was born with"""
    assert len(parts) == len(unsorted) and len(np.unique(parts["age"])) >= 2
    assert len(np.unique(unsorted["scale"] / parts["initial_scale"])) >= 2  # (the scale curve is not flat)
    if spawn_rotation is not None:
        old = parts["age"] > np.float32(dt)
        assert old.sum() > len(parts) // 4
        assert (unsorted["rotation"][old] != np.asarray(spawn_rotation, dtype=np.float32)).any(axis=1).all()
