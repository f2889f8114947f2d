"""The `volumes` scenario of examples/mirror_check.cpp -- the three spawners of its `aabbs` scenario and, every tenth frame, how many of
their particles lie inside six volumes (a half-space that holds everything, one of every other kind, three of them rotated) through
ParticleSystemPlugin::count_in_volumes and ::count_in_volumes_device of include/firework.hpp, over a list that names one spawner twice --
against the same calls through the Python mirror (ParticleSystem.count_in_volumes / count_in_volumes_device): the same library, so every
line must be identical.  A mirror that marshals the places or the volumes differently (type dropped, a field of the record in another
place, the list reordered) prints other counts."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_host import ROOT, _fnv, build  # noqa: E402


def _python_mirror_lines():
    import numpy as np
    import torch

    import volume_ref
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
        places = [(ds[2], -1), (ds[0], 0), (ds[1], -1), (ds[0], -1)]
        q = (0.5, 0.5, 0.5, 0.5)
        volumes = [S.Collider.Plane((0.0, 1000.0, 0.0), (0.0, 1.0, 0.0)), S.Collider.Sphere((0.25, 3.25, 0.125), 0.625),
                   S.Collider.Box((4.25, 3.25, 0.125), (0.5, 0.625, 0.375), q), S.Collider.Cylinder((0.25, 3.25, 0.125), 0.625, 1.0),
                   S.Collider.Cone((0.25, 3.25, 0.125), 0.75, 1.5, q), S.Collider.Capsule((8.25, 3.25, 0.125), 0.375, 0.75, q)]
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_cnt = torch.zeros((len(places) * len(volumes), 4), dtype=torch.uint8, device="cuda")
        dt = np.float32(1.0 / 60.0)
        for fr in range(40):
            if fr == 15:
                ds[2].queue_particles(33)
            ps.update(dt)
            if fr % 10 != 9:
                continue
            ps.count_in_volumes_device(places, volumes, d_cnt.data_ptr())
            host = ps.count_in_volumes(places, volumes)
            ps.synchronize()
            dev = d_cnt.cpu().numpy().reshape(-1).view(np.uint32).reshape(host.shape)
            lines.append(f"frame {fr} all {' '.join(str(int(c)) for c in host[:, 0])} host {_fnv(host.tobytes()):016x} device {_fnv(dev.tobytes()):016x}")
            checks.append((host.copy(), dev.copy(), volume_ref.counts(places, volumes)))
    return lines, checks


def test_mirror_check_knows_the_volumes_scenario():
    """(no GPU) the example builds against the header's two calls, and the C++ mirror hands places and volumes over as they are"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"volumes"' in src and "app.count_in_volumes(" in src and "app.count_in_volumes_device(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    for call in ("fw_ctx_count_in_volumes(ctx_, (uint32_t)p.size(), p.data(), (uint32_t)v.size(), v.data(), out.data())",
                 "fw_ctx_count_in_volumes_device(ctx_, (uint32_t)p.size(), p.data(), (uint32_t)v.size(), v.data(), d_out)"):
        assert call in hpp, call


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_count_the_same():
    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "volumes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines, checks = _python_mirror_lines()
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert [ln.split()[3] for ln in cpp_lines] == ["0", "33", "33", "33"]  # the OnDemand spawner, first in the list: empty until it is fed in frame 15
    assert len({ln.split()[8] for ln in cpp_lines}) == 4  # (every frame has counts of its own)
    for host, dev, want in checks:
        assert host.tobytes() == dev.tobytes() and (host == want).all()
        assert (host[1] == host[3]).all() and host[1, 0] > 300  # the spawner listed twice: by its one type and by -1
        assert ((host > 0) & (host < host[:, :1])).sum() >= 5    # (volumes that cut the clouds)
