"""The `paths` scenario of examples/mirror_check.cpp -- the fixed small world of its `project` scenario (one collider of each kind plus
one mesh instance) and a fixed list of hypothetical particles traced through it by include/firework.hpp (trace_paths with samples /
trace_paths_device) -- against the same calls through the Python mirror: the same library, so every field of every result must carry
the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_ref  # noqa: E402
from mesh_ref import Instance, Mesh  # noqa: E402
from test_cpp_host import ROOT, _fnv, build  # noqa: E402
from test_cpp_host_project import RAMP, RAMP_AT, _world  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
SETTINGS = S.PathSettings(0.03125, 24, (0.0, -9.75, 0.0), 0.125, S.ParticleCollisionSettings(0.5, 0.25, False, 3))


def _paths():
    i = np.arange(96)
    p = np.zeros(96, dtype=S.PATH_DTYPE)
    p["position"][:, 0] = f32(-3.0) + (i % 8).astype(f32) * f32(0.875)
    p["position"][:, 1] = f32(-1.5) + ((i // 8) % 4).astype(f32) * f32(1.125)
    p["position"][:, 2] = f32(-2.5) + (i // 32).astype(f32) * f32(2.25)
    p["velocity"][:, 0] = f32(1.5) - (i % 5).astype(f32) * f32(0.75)
    p["velocity"][:, 1] = f32(-0.5) * (i % 4).astype(f32)
    p["velocity"][:, 2] = (i % 3).astype(f32) - f32(1.0)
    p["age"] = f32(0.0625) * (i % 2).astype(f32)
    p["lifetime"] = f32(0.25) + f32(0.125) * (i % 7).astype(f32)
    return p


def _reference():
    return trace_ref.trace_paths(trace_ref.world_of(_world(), [Instance(Mesh(*RAMP), *RAMP_AT)]), SETTINGS, _paths(), samples=True)


def _lines(out, samples, from_device, samples_from_device):
    words = out.view(np.uint32).reshape(-1, 20)
    return [f"path {i} " + " ".join(f"{w:08x}" for w in row) for i, row in enumerate(words)] + [
        f"host {_fnv(out.tobytes()):016x} device {_fnv(from_device.tobytes()):016x} samples {_fnv(samples.tobytes()):016x} device {_fnv(samples_from_device.tobytes()):016x}"]


def test_mirror_check_knows_the_paths_scenario():
    """(no GPU) the example builds against the header's new calls and its source has the scenario; the scenario's paths meet every
    kind of end in the reference: running, expired, bounced off a collider, off the mesh, started inside a solid"""
    build()
    src = open(os.path.join(ROOT, "examples", "mirror_check.cpp")).read()
    assert '"paths"' in src and "trace_paths(" in src and "trace_paths_device(" in src
    hpp = open(os.path.join(ROOT, "include", "firework.hpp")).read()
    assert "fw_ctx_trace_paths(" in hpp and "fw_ctx_trace_paths_device(" in hpp
    want, _ = _reference()
    assert (want["status"] == S.PATH_RUNNING).sum() >= 5 and (want["status"] == S.PATH_EXPIRED).sum() >= 5
    assert (want["kind"] == S.HIT_MESH).sum() >= 3 and len(set(want["index"][want["kind"] == S.HIT_COLLIDER].tolist())) >= 3
    hit = want["contact_step"] != 0xFFFFFFFF
    assert (hit & ~want["contact_normal"].any(axis=1)).sum() >= 3 and (want["n_contacts"] >= 2).sum() >= 5 and (~hit).sum() >= 5


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_trace_paths_identically():
    import torch

    from bevy_firework_amd.system import ParticleSystem

    build()
    run = subprocess.run([os.path.join(ROOT, "examples", "mirror_check"), "paths"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    cpp_lines = run.stdout.strip().splitlines()
    p = _paths()
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ps.set_colliders(_world())
        ps.set_mesh_colliders([S.MeshCollider(ps.create_mesh(*RAMP), *RAMP_AT)])
        host, samples = ps.trace_path_records(SETTINGS, p, samples=True)
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            d_paths = torch.from_numpy(p.view("u1").reshape(-1, 32).copy()).to("cuda")
            d_out = torch.zeros((len(p), 80), dtype=torch.uint8, device="cuda")
            d_samples = torch.zeros((SETTINGS.n_steps, len(p), 4), dtype=torch.float32, device="cuda")
        ps.trace_paths_device(SETTINGS, d_paths.data_ptr(), len(p), d_out.data_ptr(), d_samples.data_ptr())
        with torch.cuda.stream(torch.cuda.ExternalStream(ps.stream)):
            from_device, samples_from_device = d_out.cpu().numpy(), d_samples.cpu().numpy()
    lines = _lines(host, samples, from_device, samples_from_device)
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    last = cpp_lines[-1].split()
    assert last[1] == last[3] and last[5] == last[7]  # (host form == device form, results and samples)
    want, want_s = _reference()
    assert host.tobytes() == want.tobytes() and samples.tobytes() == want_s.tobytes()
