"""The `aabbs` scenario of examples/mirror_check.cpp -- three spawners (two sphere emitters, one OnDemand spawner fed in frame 15) whose
boxes are asked for every tenth frame through ParticleSpawnerData::aabb, ParticleSystemPlugin::aabbs and ::aabbs_device of
include/firework.hpp over a list that names one spawner twice -- against the same calls through the Python mirror (SpawnerData.aabb,
ParticleSystem.aabb_records / aabbs_device): the same library, so every line must be identical.  A mirror that marshals the handle list
or the fw_aabb record differently (min and max swapped, `any` dropped, the list reordered) prints other digests."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_host import ROOT, _fnv, build  # noqa: E402


def _python_mirror_lines():
    import numpy as np
    import torch

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    lines, checks = [], []
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ds = []
        for k in range(3):
            ps0 = S.ParticleSettings(lifetime=S.RandF32.constant(0.75), linear_drag=0.125)
            pacing = S.EmissionPacing.OnDemand() if k == 2 else S.EmissionPacing.rate(2000.0 if k == 0 else 150.0)
            e0 = S.EmissionSettings(particle_index=0, emission_pacing=pacing, emission_shape=S.EmissionShape.Sphere(0.75),
                                    initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.5))
            ds.append(ps.spawn(S.ParticleSpawner([ps0], [e0]), S.Transform((0.25 + 4.0 * k, 3.0, 0.125)), uid=7 + k))
        order = [ds[2], ds[0], ds[1], ds[0]]
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_rec = torch.zeros((len(order), 32), dtype=torch.uint8, device="cuda")
        dt = np.float32(1.0 / 60.0)
        for fr in range(40):
            if fr == 15:
                ds[2].queue_particles(33)
            ps.update(dt)
            if fr % 10 != 9:
                continue
            ps.aabbs_device(order, d_rec.data_ptr())
            host = ps.aabb_records(order)
            ps.synchronize()
            dev = d_rec.cpu().numpy().reshape(-1).view(S.AABB_DTYPE)
            single = np.zeros(len(order), dtype=S.AABB_DTYPE)
            for i, d in enumerate(order):
                any_, single["min"][i], single["max"][i] = d.aabb()
                single["any"][i] = 1 if any_ else 0
            lines.append(f"frame {fr} any {''.join(str(int(a)) for a in host['any'])} host {_fnv(host.tobytes()):016x} "
                         f"device {_fnv(dev.tobytes()):016x} single {_fnv(single.tobytes()):016x}")
            checks.append((host.copy(), dev.copy(), single))
    return lines, checks


def test_mirror_check_knows_the_aabbs_scenario():
    """(no GPU) the example builds against the header's two calls, and both mirrors hand the list and the records over as they are"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"aabbs"' in src and "app.aabbs(" in src and "app.aabbs_device(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    for call in ("fw_ctx_aabbs(ctx_, (uint32_t)h.size(), h.data(), out.data())", "fw_ctx_aabbs_device(ctx_, (uint32_t)h.size(), h.data(), d_out)"):
        assert call in hpp, call


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_answer_the_same_boxes():
    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "aabbs"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines, checks = _python_mirror_lines()
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert [ln.split()[3] for ln in cpp_lines] == ["0111", "1111", "1111", "1111"]  # the OnDemand spawner, first in the list: empty until it is fed in frame 15
    assert len({ln.split()[5] for ln in cpp_lines}) == 4  # (every frame has boxes of its own)
    for host, dev, single in checks:
        for f in ("min", "max", "any", "reserved"):  # (as floats: -0 == +0)
            assert (host[f] == dev[f]).all() and (host[f] == single[f]).all(), f
        assert (host["min"][1] == host["min"][3]).all() and (host["max"][1] == host["max"][3]).all()  # the spawner listed twice
        assert not (host["min"][1] == host["min"][2]).all()
