"""Resource handling of a context (fw_engine.h: the HipBuf / HipEvent / HipStream owners).  Contexts that grow every kind of
buffer and are then destroyed give their device memory back, and a simulated allocation failure (the `ab` build's
FW_FAIL_ALLOC=k: the context's k-th allocation fails) at any point of such a run ends in a status -- after which
fw_ctx_destroy releases what the context holds.  Needs an MI355X."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from bevy_firework_amd import settings as S

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
MB = 1 << 20
DRIFT = 64 * MB  # free device memory a run may leave behind (a margin, not a measured figure)


def scenario(ps, scale):
    """a FIFO-ring type and a range-ring type that bursts make grow, a Nested spawner, a colliding type; then a caller write
    that sends the FIFO ring to the compacting path and a collider set larger than the first"""
    od = S.EmissionSettings(emission_pacing=S.EmissionPacing.OnDemand())
    fifo = ps.spawn(S.ParticleSpawner([S.ParticleSettings(lifetime=S.RandF32.constant(1.0), capacity=65536)], [od]), uid=1)
    rr = ps.spawn(S.ParticleSpawner([S.ParticleSettings(lifetime=S.RandF32(0.6, 1.0), capacity=16384)], [od]), uid=2)
    sparks = S.ParticleSettings(lifetime=S.RandF32(0.5, 0.8), linear_drag=0.2)
    smoke = S.ParticleSettings(lifetime=S.RandF32.constant(0.5), acceleration=(0.0, 0.5, 0.0))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(4000.0),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 5.0), (0.0, 1.0, 0.0), 0.0))
    e1 = S.EmissionSettings(particle_index=1, emission_mode=S.EmissionMode.Nested(0), inherit_parent_velocity=False,
                            emission_pacing=S.EmissionPacing.CountOverDuration(6.0, 0.0, 0.0, 0.5))
    ps.spawn(S.ParticleSpawner([sparks, smoke], [e0, e1]), uid=3)
    coll = S.ParticleSettings(lifetime=S.RandF32(0.5, 1.0), collision_settings=S.ParticleCollisionSettings(0.6, 0.2, True, 3))
    ps.spawn(S.ParticleSpawner([coll], [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(5000.0),
                                                          initial_velocity=S.RandVec3(S.RandF32(1.0, 3.0), (0.0, -1.0, 0.0), 0.0))]),
             S.Transform((0.0, 1.0, 0.0)), uid=4)
    ps.set_colliders([S.Collider.Plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))])
    paths = [fifo.update_path(0)[0], rr.update_path(0)[0]]
    for fr in range(12):
        if fr in (2, 5):
            fifo.queue_particles(int(1_200_000 * scale))
            rr.queue_particles(int(400_000 * scale))
        ps.update(DT)
    grown = fifo.count(0) > 65536 and rr.count(0) > 16384
    parts = np.zeros(1000, dtype=S.PARTICLE_DTYPE)
    parts["rotation"][:, 3] = 1.0
    parts["initial_scale"] = parts["scale"] = 1.0
    parts["lifetime"] = np.linspace(0.2, 0.9, len(parts), dtype=np.float32)  # (no longer one lifetime: the ring ends)
    fifo.write_particles(0, parts)
    paths.append(fifo.update_path(0)[0])
    ps.set_colliders([S.Collider.Sphere((0.1 * i, 0.0, 0.0), 0.05) for i in range(100)])
    for _ in range(2):
        ps.update(DT)
    ps.synchronize()
    return paths, grown


@pytest.fixture()
def ring_knobs(monkeypatch):
    for k, v in {"FW_ENABLE_KNOBS": "1", "FW_FIFO": "1", "FW_FIFO_MIN": "0", "FW_RANGE": "1", "FW_RANGE_MIN": "0"}.items():
        monkeypatch.setenv(k, v)


def test_contexts_give_their_device_memory_back(ring_knobs):
    """ten contexts in a row, each allocating hundreds of MB in the library: free device memory after the tenth is where it was
    after the first"""
    import torch

    from bevy_firework_amd.system import ParticleSystem

    torch.cuda.empty_cache()
    free = []
    for cycle in range(10):
        ps = ParticleSystem(device=0, seed=cycle)
        paths, grown = scenario(ps, 1.0)
        held = torch.cuda.mem_get_info(0)[0]
        ps.close()
        free.append(torch.cuda.mem_get_info(0)[0])
        assert paths == ["fifo", "range", "general"] and grown, (cycle, paths, grown)
        assert free[-1] - held >= 256 * MB, (cycle, (free[-1] - held) / MB)
    drift = free[0] - free[-1]
    print(f"free device memory after cycle 1 / 10: {free[0] / MB:.1f} / {free[-1] / MB:.1f} MB (drift {drift / MB:.1f} MB)")
    assert drift < DRIFT, [f / MB for f in free]


def test_every_allocation_failure_ends_in_a_status():
    """FW_FAIL_ALLOC=k for k = 1, 2, ... until a run no longer reaches its k-th allocation: every call returns FW_OK or a
    failure status, the first failure is followed by nothing but fw_ctx_destroy (FW_OK), and device memory is back at the
    end.  In a subprocess: the `ab` build and its knobs are per process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ab = os.path.join(root, "bevy_firework_amd", "csrc", "libfirework_hip_ab.so")
    assert os.path.exists(ab), "libfirework_hip_ab.so not built (make -C bevy_firework_amd/csrc)"
    code = textwrap.dedent("""
        import os, sys, tempfile, traceback
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import torch
        from bevy_firework_amd import _ffi
        from bevy_firework_amd.system import ParticleSystem, FwError
        from test_gpu_resources import scenario, DRIFT, MB
        # (the library says on stderr when the injected failure happens: that is how a run that never gets there is told apart
        # from one whose failure was absorbed -- the large-BAR probe, for one)
        log = tempfile.TemporaryFile()
        os.dup2(log.fileno(), 2)
        def run(k):
            log.seek(0), log.truncate()
            os.environ["FW_FAIL_ALLOC"] = str(k)
            try:
                ps = ParticleSystem(device=0, seed=k)
            except FwError as e:
                return e.status
            try:
                scenario(ps, 0.1)
                st = None
            except FwError as e:
                st = e.status
            ctx, ps._ctx = ps._ctx, None
            assert ps._lib.fw_ctx_destroy(ctx) == _ffi.FW_OK
            return st
        try:
            assert run(0) is None  # (the scenario itself runs through; the runtime's own allocations happen here)
            torch.cuda.empty_cache()
            free0 = torch.cuda.mem_get_info(0)[0]
            failures = {}
            for k in range(1, 1001):
                st = run(k)
                log.seek(0)
                if b"FW_FAIL_ALLOC" not in log.read():
                    assert st is None, (k, st)
                    break
                failures[k] = st
            else:
                raise AssertionError("the run makes more than 1000 allocations")
            assert k > 20 and any(st is not None for st in failures.values()), failures
            free1 = torch.cuda.mem_get_info(0)[0]
            print("ALLOC-FAIL-OK", k - 1, "allocations", sum(st is not None for st in failures.values()), "failed runs,",
                  "free device memory %%.1f -> %%.1f MB" %% (free0 / MB, free1 / MB))
            assert abs(free0 - free1) < DRIFT, (free0 / MB, free1 / MB)
        except BaseException:
            traceback.print_exc(file=sys.stdout)
            raise
    """) % (root, root)
    env = dict(os.environ, FW_ENABLE_KNOBS="1", FW_LIB_PATH=ab, FW_FIFO="1", FW_FIFO_MIN="0", FW_RANGE="1", FW_RANGE_MIN="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "ALLOC-FAIL-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
