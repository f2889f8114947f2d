"""The `project` scenario of examples/mirror_check.cpp -- a fixed small world (one collider of each kind plus one mesh instance) and a
fixed list of points projected onto it through include/firework.hpp (project_points / project_points_device) -- against the same
calls through the Python mirror: the same library, so every field of every projection must carry the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_ref  # noqa: E402
from mesh_ref import Instance, Mesh  # noqa: E402
from test_cpp_host import ROOT, _fnv, build  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
TURN_Y, TURN_Z, TILT = (0.0, 0.38268343, 0.0, 0.92387953), (0.0, 0.0, 0.19509032, 0.98078528), (0.30151135, 0.0, 0.30151135, 0.90453404)
RAMP = (np.array([[-2, -0.25, -2], [2, -0.25, -2], [2, 0.25, 2], [-2, 0.25, 2]], dtype=f32), np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32))
RAMP_AT = ((0.5, 1.75, 0.0), TURN_Y, 3)


def _world():
    return [S.Collider.Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), S.Collider.Sphere((1.0, 0.5, 0.0), 0.75, 2),
            S.Collider.Box((-2.0, 0.0, 0.0), (0.5, 1.0, 0.5), TURN_Y), S.Collider.Cylinder((0.0, 0.5, -2.0), 0.5, 1.5, S.QUAT_IDENTITY, 3),
            S.Collider.Cone((2.0, 0.0, 2.0), 0.75, 2.0, TURN_Z), S.Collider.Capsule((-0.75, 1.0, 1.5), 0.25, 1.5, TILT, 2)]


def _points():
    i = np.arange(96)
    p = np.zeros(96, dtype=S.POINT_DTYPE)
    p["position"][:, 0] = f32(-3.0) + (i % 8).astype(f32) * f32(0.875)
    p["position"][:, 1] = f32(-1.5) + ((i // 8) % 4).astype(f32) * f32(1.125)
    p["position"][:, 2] = f32(-2.5) + (i // 32).astype(f32) * f32(2.25)
    p["filter_mask"] = 1 + i % 3
    return p


def _lines(out, from_device):
    words = out.view(np.uint32).reshape(-1, 8)
    return [f"point {i} " + " ".join(f"{w:08x}" for w in row) for i, row in enumerate(words)] + [f"host {_fnv(out.tobytes()):016x} device {_fnv(from_device.tobytes()):016x}"]


def test_mirror_check_knows_the_project_scenario():
    """(no GPU) the example builds against the header's new calls and its source has the scenario; the scenario's points meet every
    kind of answer in the reference: inside a solid, a collider's surface, the mesh, nobody"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"project"' in src and "project_points(" in src and "project_points_device(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "fw_ctx_project_points(" in hpp and "fw_ctx_project_points_device(" in hpp
    p = _points()
    want = project_ref.project_points(_world(), [Instance(Mesh(*RAMP), *RAMP_AT)], p["position"], p["filter_mask"])
    assert (want["is_inside"] == 1).sum() >= 5 and (want["kind"] == S.HIT_MESH).sum() >= 5 and (want["kind"] != S.HIT_NONE).all()
    assert len(set(want["index"][want["kind"] == S.HIT_COLLIDER].tolist())) >= 5


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_project_points_identically():
    import torch

    from bevy_firework_amd.system import ParticleSystem

    build()
    run = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "project"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    cpp_lines = run.stdout.strip().splitlines()
    p = _points()
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ps.set_colliders(_world())
        ps.set_mesh_colliders([S.MeshCollider(ps.create_mesh(*RAMP), *RAMP_AT)])
        host = ps.project_point_records(p)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_points = torch.from_numpy(p.view("u1").reshape(-1, 16).copy()).to("cuda")
            d_out = torch.zeros((len(p), 32), dtype=torch.uint8, device="cuda")
        ps.project_points_device(d_points.data_ptr(), len(p), d_out.data_ptr())
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            from_device = d_out.cpu().numpy()
    lines = _lines(host, from_device)
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert cpp_lines[-1].split()[1] == cpp_lines[-1].split()[3]  # (host form == device form)
    want = project_ref.project_points(_world(), [Instance(Mesh(*RAMP), *RAMP_AT)], p["position"], p["filter_mask"])
    assert host.tobytes() == want.tobytes()
