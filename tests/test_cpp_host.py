"""The C++ host mirror (include/firework.hpp): compiles everywhere, runs the reference's stress_test
parameters on the GPU and must land on the count the emission arithmetic predicts."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    return os.path.join(ROOT, "examples", "stress_test")


def test_cpp_example_builds_and_fails_loudly_without_gpu():
    exe = build()
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "examples", "sharded"), "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr  # the native multi-GPU host: same rule


@pytest.mark.gpu
def test_cpp_stress_test_counts():
    exe = build()
    out = subprocess.run([exe, "160000", "300"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    n = int(re.search(r"Particles: (\d+)", out.stdout).group(1))
    assert n in (157333, 157334, 157335)  # examples/stress_test.rs load: 157 334 per 1 s cycle


def _fnv(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _run_both_mirrors(meshes):
    """examples/mirror_check (with the argument `mesh`: triangle meshes in its collider world) and the same scenario through the
    Python mirror; asserts that the lines are identical and returns them"""
    import numpy as np

    from bevy_firework_amd import settings as S
    from bevy_firework_amd.system import ParticleSystem

    build()
    out = subprocess.run([os.path.join(ROOT, "examples", "mirror_check")] + (["mesh"] if meshes else []), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    cpp_lines = out.stdout.strip().splitlines()

    seen = [0]
    p0 = S.ParticleSettings(lifetime=S.RandF32.constant(0.4), initial_scale=S.RandF32(0.5, 2.0),
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]),
                            base_color=S.FireworkGradient.uneven_samples([(0.0, (10, 7, 1, 1)), (0.7, (3, 1, 1, 1)),
                                                                          (1.0, (0.1, 0.1, 0.1, 0))]),
                            linear_drag=0.3, particles_destroyed=lambda dead: seen.__setitem__(0, seen[0] + len(dead)))
    p1 = S.ParticleSettings(lifetime=S.RandF32(0.2, 0.6), acceleration=(0.0, 0.5, 0.0),
                            scale_curve=S.FireworkCurve.uneven_samples([(0.0, 1.0), (0.8, 1.2), (1.0, 0.0)]),
                            emissive_color=S.FireworkGradient.even_samples([(4, 2, 0, 1), (0, 0, 0, 1)]),
                            angular_drag=0.1, angular_acceleration=(0.1, 0.0, -0.2))
    p2 = S.ParticleSettings(lifetime=S.RandF32(0.5, 0.9), pbr=True,
                            collision_settings=S.ParticleCollisionSettings(0.6, 0.2, False, 3))
    e0 = S.EmissionSettings(particle_index=0, emission_pacing=S.EmissionPacing.rate(5000.0),
                            emission_shape=S.EmissionShape.Sphere(0.5),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.0),
                            initial_velocity_radial=S.RandF32(1.0, 2.0))
    e1 = S.EmissionSettings(particle_index=1, emission_pacing=S.EmissionPacing.CountOverDuration(8.0, 1.0, 0.1, 0.9),
                            emission_mode=S.EmissionMode.Nested(0), inherit_parent_velocity=False)
    e2 = S.EmissionSettings(particle_index=2, emission_pacing=S.EmissionPacing.OnDemand(),
                            emission_shape=S.EmissionShape.Circle((0.0, 0.0, 1.0), 2.0),
                            initial_velocity=S.RandVec3(S.RandF32(0.0, 3.0), (0.0, -1.0, 0.0), 0.0),
                            initial_rotation=(0.0, 0.38941834, 0.0, 0.92106099))
    e3 = S.EmissionSettings(particle_index=2, emission_pacing=S.EmissionPacing.OneShot(700))
    lines = []
    with ParticleSystem(device=0, seed=0x00C0FFEE) as ps:
        ps.track_aabbs(True)
        ps.set_colliders([S.Collider.Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), S.Collider.Sphere((1.0, 0.5, 0.0), 0.75, 2),
                          S.Collider.Box((-2.0, 0.0, 0.0), (0.5, 1.0, 0.5), (0.0, 0.38268343, 0.0, 0.92387953))])
        if meshes:
            ramp = ps.create_mesh(np.array([[-2.0, -0.25, -2.0], [2.0, -0.25, -2.0], [2.0, 0.25, 2.0], [-2.0, 0.25, 2.0]], dtype=np.float32),
                                  np.array([[0, 2, 1], [0, 3, 2]], dtype=np.uint32))
            ps.set_mesh_colliders([S.MeshCollider(ramp, (0.0, -0.25, 0.0), (0.0, 0.0, 0.0, 1.0), 1),
                                   S.MeshCollider(ramp, (0.5, 0.25, 0.0), (0.0, 0.38268343, 0.0, 0.92387953), 2)])
        d = ps.spawn(S.ParticleSpawner([p0, p1, p2], [e0, e1, e2, e3]), S.Transform((0.0, 1.0, 0.0)), uid=42,
                     modifier=S.EffectModifier(2.0, 0.5))
        d.set_parent_velocity((0.5, 0.0, -0.25))
        dt = np.float32(1.0 / 60.0)
        for fr in range(60):
            if fr in (0, 7, 8, 31):
                d.queue_particles(500 + 10 * fr)
            if meshes and fr == 30:
                sheet = ps.create_mesh(np.array([[-3.0, 0.0, -3.0], [3.0, 0.0, -3.0], [0.0, 0.5, 3.0]], dtype=np.float32),
                                       np.array([[0, 2, 1]], dtype=np.uint32))
                ps.set_mesh_colliders([S.MeshCollider(sheet, (1.0, 1.5, 3.0), (0.0, 0.0, 0.19509032, 0.98078528), 3)])
                ps.destroy_mesh(ramp)
            if fr == 20:
                d.set_transform(S.Transform((1.0, 2.0, 3.0), (0.0, 0.0, 0.38268343, 0.92387953)))
            ps.update(dt)
            if fr % 10 != 9:
                continue
            c = d.counts()
            digests = " ".join(f"{_fnv(d.particles(t).tobytes()):016x}" for t in range(3))
            any_, mn, mx = d.aabb()
            box = np.concatenate([mn, mx]).astype(np.float32).tobytes()
            lines.append(f"frame {fr} counts {c[0]} {c[1]} {c[2]} {digests} aabb {int(any_)} {_fnv(box):016x} "
                         f"active {int(d.active())}")
    lines.append(f"destroyed reported {seen[0]}")
    assert cpp_lines == lines, "\n".join(["C++:"] + cpp_lines + ["Python:"] + lines)
    assert int(cpp_lines[-2].split()[3]) > 1000 and seen[0] > 2000
    return cpp_lines


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_drive_the_library_identically():
    """examples/mirror_check.cpp (three particle types, Global / OnDemand / OneShot / Nested entries, all curve kinds,
    modifier, transforms, parent velocity, destroyed handler, colliders, fused AABB) through include/firework.hpp, and
    the same scenario through bevy_firework_amd/: the same library, so every digest must be identical -- a field either
    mirror marshals differently (or forgets) shows up here"""
    _run_both_mirrors(False)


@pytest.mark.gpu
def test_cpp_mirror_and_python_mirror_place_meshes_identically():
    """the same scenario with the mesh entry points of both mirrors (`mirror_check mesh`): one small mesh of literal vertices placed
    twice -- one instance rotated, one on layer 2 -- then the set replaced by another mesh and the first one destroyed.  A slip in
    either mirror's marshalling of fw_mesh_collider (mesh, layers, position, rotation) changes where the pebbles bounce and so the
    digests; and the meshes do change them: the lines differ from those of the scenario without meshes"""
    with_meshes = _run_both_mirrors(True)
    without = _run_both_mirrors(False)
    assert [ln.split()[:6] for ln in with_meshes] == [ln.split()[:6] for ln in without]  # (a bounce destroys nothing: the same counts)
    for k in (2, 5):  # frames 29 and 59: the pebbles' digest under the first and under the second instance set
        assert with_meshes[k].split()[8] != without[k].split()[8], (with_meshes[k], without[k])


@pytest.mark.gpu
def test_native_sharded_host_matches_the_python_sharding(tmp_path):
    """examples/sharded.cpp -- N contexts, the live-count device ring, ncclAllReduce of bucketed per-frame totals, all from
    C++ over include/firework.hpp -- against bevy_firework_amd.sharding.ShardedParticleSystem on the same workload (one GPU
    here: one rank; the RCCL calls are made all the same): the per-frame global live totals and the per-emitter counts must be
    identical, in the single-process form and in the one-process-per-GPU form"""
    import numpy as np
    import torch

    from bevy_firework_amd import sharding, workloads
    from bevy_firework_amd.system import ParticleSystem

    build()
    exe = os.path.join(ROOT, "examples", "sharded")
    common = ["--emitters", "48", "--live", "2048", "--frames", "44", "--reduce-every", "8"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = []
    for how in (["--gpus", "1"], ["--rank", "0", "--world", "1", "--id-file", str(tmp_path / "nccl_id")]):
        try:
            r = subprocess.run([exe] + how + common, capture_output=True, text=True, timeout=120, env=env)
        except subprocess.TimeoutExpired:  # (RCCL's communicator set-up has hung once on a fresh box: one more try)
            r = subprocess.run([exe] + how + common, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines())
    assert outs[0][:45] == outs[1][:45]
    cpp_hist = [int(ln.split()[3]) for ln in outs[0] if ln.startswith("frame ")]
    cpp_digest = re.search(r"counts_digest ([0-9a-f]{16})", "\n".join(outs[0])).group(1)
    assert len(cpp_hist) == 44 and cpp_hist[-1] > 60000

    stream = torch.cuda.Stream()
    dt = np.float32(1.0 / 60.0)
    sh = sharding.ShardedParticleSystem(lambda: ParticleSystem(device=0, seed=workloads.SEED, stream=stream.cuda_stream),
                                        workloads.many_emitters(48, 2048), 0, 1, reduce_every=8, torch_stream=stream, exchange=True)
    sh.update(dt)
    for _ in range(43):
        sh.step(dt)
    sh.flush()
    assert sh.global_live_history == cpp_hist
    h = 1469598103934665603
    for e, d in zip(sh.global_indices, sh.handles):
        for x in np.array([e, d.count(0)], dtype=np.uint32).tobytes():
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert f"{h:016x}" == cpp_digest
    sh.system.close()
    # round 6: the rehearsal of N ranks on ONE device (N contexts, N host threads, host-side sum of the buckets instead of
    # ncclAllReduce): emitter e in context e mod 4 -- the per-frame global totals do not depend on how the emitters are spread
    r = subprocess.run([exe, "--ranks-on-one-device", "4"] + common, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert [int(ln.split()[3]) for ln in lines if ln.startswith("frame ")] == cpp_hist
    per_ctx = [ln for ln in lines if ln.startswith("context ")]
    assert len(per_ctx) == 4 and all("12 emitters" in ln for ln in per_ctx)
    assert re.search(r"ranks_on_one_device 4 emitters 48 live_total (\d+)", r.stdout).group(1) == str(cpp_hist[-1])


@pytest.mark.gpu
def test_cpp_many_contexts_one_per_thread():
    """examples/many_contexts.cpp: emitters spread over contexts, one per worker thread, stepped frame-synchronously -- the same
    emitters end up with the same live total however many contexts (and threads) hold them (emitter e keeps uid e)"""
    build()
    exe = os.path.join(ROOT, "examples", "many_contexts")
    totals = []
    for threads in ("1", "2", "3"):
        r = subprocess.run([exe, "96", "400", threads, "150"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"on (\d+) context\(s\).*?([\d.]+) us per frame, (\d+) live", r.stdout)
        assert m and m.group(1) == threads, r.stdout
        totals.append(int(m.group(3)))
    assert totals[0] > 30000 and totals[0] == totals[1] == totals[2], totals


def test_cpp_many_contexts_fails_loudly_without_gpu():
    build()
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([os.path.join(ROOT, "examples", "many_contexts"), "8", "100", "2", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
