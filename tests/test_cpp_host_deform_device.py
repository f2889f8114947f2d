"""The `deform_device` scenario of examples/mirror_check.cpp -- `deform` with every new vertex set handed over in device memory
through include/firework.hpp (update_mesh_vertices_device / mesh_update_status) -- against the same calls through the Python
mirror: the same library, so every digest must be identical; and against the `deform` scenario itself, whose vertices take
the host form: the two forms give the same bits."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpp_host import ROOT, build  # noqa: E402
import test_cpp_host_deform as host_form  # noqa: E402


def _python_mirror_lines(monkeypatch):
    """test_cpp_host_deform's scenario with every update_mesh_vertices going through a device tensor and the device form"""
    import numpy as np
    import torch

    from bevy_firework_amd.system import ParticleSystem

    keep, last = [], {}

    def via_device(self, mesh, vertices):
        host = torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3).copy())
        with torch.cuda.stream(torch.cuda.ExternalStream(self.stream)):
            keep.append(host.to("cuda"))
        self.update_mesh_vertices_device(mesh, keep[-1].data_ptr(), keep[-1].shape[0])
        last["mesh"] = mesh

    close = ParticleSystem.close

    def close_with_status(self):
        if getattr(self, "_ctx", None) and "mesh" in last:
            self.synchronize()
            last["status"] = self.mesh_update_status(last.pop("mesh"))
        close(self)

    monkeypatch.setattr(ParticleSystem, "update_mesh_vertices", via_device)
    monkeypatch.setattr(ParticleSystem, "close", close_with_status)
    lines = host_form._python_mirror_lines()
    return lines + ["sheet device updates %d %d %d" % last["status"]]


def test_mirror_check_knows_the_deform_device_scenario():
    """(no GPU) the example builds against the header's new calls and its source has the scenario"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"deform_device"' in src and "update_mesh_vertices_device(" in src and "mesh_update_status(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "fw_ctx_update_mesh_vertices_device(" in hpp and "fw_ctx_mesh_update_status(" in hpp


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_deform_meshes_from_device_memory_identically(monkeypatch):
    build()
    exe = os.path.join(ROOT, "examples", "mirror_check")
    out = subprocess.run([exe, "deform_device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()
    lines = _python_mirror_lines(monkeypatch)
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert cpp_lines[-1] == "sheet device updates 5 0 -1", cpp_lines[-1]  # (frames 35, 40, 45, 50, 55)
    # the host form of the same scenario: the same bits
    ref = subprocess.run([exe, "deform"], capture_output=True, text=True, timeout=120)
    assert ref.returncode == 0, ref.stderr
    assert cpp_lines[:-1] == ref.stdout.strip().splitlines()
