"""The `sorted` scenario of examples/mirror_check.cpp -- one spawner whose instance records are sorted by view depth every tenth frame,
in both orders, through ParticleSpawnerData::instances_sorted, ParticleSystemPlugin::pack_instances_sorted_device and ::depth_order_device
of include/firework.hpp -- against the same calls through the Python mirror (SpawnerData.instances_sorted,
ParticleSystem.pack_instances_sorted_device / depth_order_device): the same library, so every digest must be identical.  A mirror that
marshals fw_sort_view differently (eye and forward swapped, the order dropped) sorts for another camera."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref  # noqa: E402
from test_cpp_host import ROOT, _fnv, build  # noqa: E402

EYE, FORWARD = (0.25, 3.5, 0.125), (0.5, -0.25, 1.0)
CAP = 4096


def _python_mirror_lines():
    import numpy as np
    import torch

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    ps0 = S.ParticleSettings(lifetime=S.RandF32.constant(0.75), linear_drag=0.125)
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(2000.0), emission_shape=S.EmissionShape.Sphere(0.75),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.5))
    lines, checks = [], []
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        d = ps.spawn(S.ParticleSpawner([ps0], [e0]), S.Transform((0.25, 3.0, 0.125)), uid=7)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_rec = torch.zeros((CAP, 64), dtype=torch.uint8, device="cuda")
            d_ord = torch.zeros((CAP,), dtype=torch.int32, device="cuda")
        dt = np.float32(1.0 / 60.0)
        for fr in range(40):
            ps.update(dt)
            if fr % 10 != 9:
                continue
            unsorted = d.instances(0)
            for order in (S.SORT_BACK_TO_FRONT, S.SORT_FRONT_TO_BACK):
                view = S.SortView(eye=EYE, forward=FORWARD, order=order)
                host = d.instances_sorted(view, 0)
                ps.pack_instances_sorted_device(d, view, d_rec.data_ptr(), CAP)
                ps.depth_order_device(d, view, d_ord.data_ptr(), CAP)
                ps.synchronize()
                n = len(host)
                rec = d_rec.cpu().numpy().reshape(-1)[:n * 64].tobytes()
                idx = d_ord.cpu().numpy().view(np.uint32)[:n]
                lines.append(f"frame {fr} order {order} count {n} unsorted {_fnv(unsorted.tobytes()):016x} host {_fnv(host.tobytes()):016x} "
                             f"device {_fnv(rec):016x} index {_fnv(idx.tobytes()):016x}")
                checks.append((unsorted, order, host, idx))
    return lines, checks


def test_mirror_check_knows_the_sorted_scenario():
    """(no GPU) the example builds against the header's three calls, and both mirrors hand the view over field by field"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"sorted"' in src and "instances_sorted(" in src and "pack_instances_sorted_device(" in src and "depth_order_device(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    for call in ("fw_ctx_pack_instances_sorted(raw_(), handle, particle_type, &view,", "fw_ctx_pack_instances_sorted_device(ctx_, data.handle, particle_type, &view, d_out, cap, &ub)",
                 "fw_ctx_depth_order_device(ctx_, data.handle, particle_type, &view, d_order, cap, &ub)"):
        assert call in hpp, call
    from bevy_firework_amd import _ffi
    from bevy_firework_amd import settings as S

    v = _ffi.make_sort_view(S.SortView(eye=EYE, forward=FORWARD, order=S.SORT_FRONT_TO_BACK))
    assert tuple(v.eye) == EYE and tuple(v.forward) == FORWARD and (v.order, v.reserved) == (1, 0)


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_sort_identically():
    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "sorted"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines, checks = _python_mirror_lines()
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert len(cpp_lines) == 8 and int(cpp_lines[-1].split()[5]) > 1000
    for ln in cpp_lines:
        w = ln.split()
        assert w[9] == w[11] and w[7] != w[9], ln  # host form == device form, and sorted is not the list's order
    assert len({ln.split()[13] for ln in cpp_lines}) == 8  # (every frame and order has a permutation of its own)
    for unsorted, order, host, idx in checks:  # ... and what both mirrors agree on is the header's order
        want = sort_ref.order_of(unsorted["position"], EYE, FORWARD, order)
        assert (idx == want).all() and host.tobytes() == unsorted[want].tobytes()
