"""Every reader of a segment outside the update kernels -- fw_k_gather (particles), fw_k_pack (instances), fw_k_aabb, and the two
kernels that put a segment back into its plain form, fw_k_rederive and fw_k_restore_q3 (+ fw_k_fill_rotation) -- over every
combination of what a segment's view (FwSegView) can say: rotation plane or one rotation, lifetime in Q3 / in a plane / one
value, scale and colours stored or evaluated, float4 planes or component planes, particle 0 in slot 0 / at a FIFO ring's head /
an old part before a range ring's young part.  Runs on all four paths; asserts on whatever path the type is on.  Needs an MI355X."""
import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
INSTANCE_FIELDS = ("position", "scale", "rotation", "base_color", "emissive_color")


def _settings(lifetime):
    # (a scale curve and both gradients that change with age: what a derived type's readers must evaluate)
    return S.ParticleSettings(lifetime=lifetime, capacity=4096, initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                              scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]),
                              base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT),
                              emissive_color=S.FireworkGradient.even_samples([(4.0, 2.0, 0.0, 1.0), (0.0, 0.0, 0.0, 1.0)]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_readers(pair, what):
    pair.check(what=what)  # gather against the oracle
    lo, hi = [], []
    for t in range(2):
        parts, inst = pair.gpu.particles(t), pair.gpu.instances(t)
        assert len(parts) == len(inst) > 3000, (what, t, len(parts), len(inst))
        for f in INSTANCE_FIELDS:  # pack against gather
            assert np.array_equal(_bits(inst[f]), _bits(parts[f])), f"{what} type {t} ({pair.gpu.update_path(t)[0]}): instances.{f} != particles.{f}"
        lo.append((parts["position"] - parts["scale"][:, None]).min(axis=0))
        hi.append((parts["position"] + parts["scale"][:, None]).max(axis=0))
    any_g, mn_g, mx_g = pair.gpu.aabb()
    assert any_g, what
    assert np.array_equal(_bits(mn_g), _bits(np.min(lo, axis=0))), f"{what}: aabb min {mn_g} != {np.min(lo, axis=0)}"
    assert np.array_equal(_bits(mx_g), _bits(np.max(hi, axis=0))), f"{what}: aabb max {mx_g} != {np.max(hi, axis=0)}"


# FW_DERIVED 0: scale and colours always stored; 2: never (every reader evaluates them).  1 -- stored unless an instance buffer is
# attached -- is the one form in which detaching the buffer takes the type out of the derived mode, i.e. runs fw_k_rederive
@pytest.mark.parametrize("derived", ["0", "2", "1"])
@pytest.mark.parametrize("turns", [True, False], ids=["can turn", "cannot turn"])
def test_every_reader_agrees_on_every_view(fw_path, monkeypatch, turns, derived):
    """two types of ~3400 live particles in buffers of 4096 slots: a ring's head passes the end of the buffer after ~15 frames, so
    the gather / AABB tiles and the 256-record pack blocks straddle it.  Type 0 has one lifetime value (a FIFO ring where the
    path has them), type 1 a lifetime range (a range ring where the path has those)."""
    import torch
    from bevy_firework_amd.system import ParticleSystem

    monkeypatch.setenv("FW_DERIVED", derived)
    spin = dict(initial_angular_velocity=S.RandVec3(S.RandF32(0.0, 5.0), (0.0, 1.0, 0.0), 0.0)) if turns else {}
    entries = [S.EmissionSettings(particle_index=t, emission_pacing=S.EmissionPacing.rate(17000.0),
                                  initial_velocity=S.RandVec3(S.RandF32(0.0, 4.0), (0.0, 1.0, 0.0), 0.0), **spin) for t in range(2)]
    types = [_settings(S.RandF32.constant(0.2)), _settings(S.RandF32(0.15, 0.25))]
    with ParticleSystem(device=0, seed=SEED) as system:
        pair = Pair(system, S.ParticleSpawner(types, entries), S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=14)
        for fr in range(1, 41):
            system.update(DT)
            pair.step_cpu(DT)
            if fr in (20, 40):
                _check_readers(pair, f"frame {fr}")

        # an instance buffer comes and goes on type 0 (FW_DERIVED=1: the type enters the derived mode, then fw_k_rederive)
        buf = torch.zeros(4096 * 16, dtype=torch.float32, device="cuda")
        pair.gpu.attach_instances(buf.data_ptr(), 4096, 0)
        system.update(DT), pair.step_cpu(DT)
        _check_readers(pair, "buffer attached")
        pair.gpu.attach_instances(0, 0, 0)
        _check_readers(pair, "buffer detached")
        system.update(DT), pair.step_cpu(DT)
        _check_readers(pair, "a step after the buffer")

        # the caller's particles: type 1 leaves its ring and the no-spin mode (fw_k_fill_rotation, fw_k_restore_q3)
        parts = pair.gpu.particles(1)
        pair.gpu.write_particles(1, parts), pair.cpu.write_particles(1, parts)
        assert pair.gpu.update_path(1)[0] in ("general", "small")
        _check_readers(pair, "particles written")
        system.update(DT), pair.step_cpu(DT)
        _check_readers(pair, "a step after the write")
