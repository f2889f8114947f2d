"""The census of a context's segments by update path (csrc/fw_update_path.h: FwPathCensus; fw_engine.h: SegPathEdit) on the device's
host: ONE context walks through every transition that moves a segment from one path to another, and after every call the census the
host keeps equals the census recounted from its segment records (fw_debug_path_census), the counts are the ones the situation asks
for, and fw_debug_update_path names the path tests/test_gpu_range.py promises for it.  A dozen frames between the steps, every spawner
against the oracle.  Thresholds as in the few-rings test there (FW_RANGE_FEW=5), with FW_FIFO_MIN = FW_RANGE_MIN = 2048 and
FW_SMALL_MIN=3 so that types of one and two tiles of capacity reach every path: one tile -- a few-ring, or the compacting layout (a
wave per type from three of them on); two tiles -- a FIFO ring (one lifetime value) or a range ring by size.  Needs an MI355X."""
import numpy as np
import pytest

import oracle
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair

pytestmark = pytest.mark.gpu
DT = np.float32(1.0 / 60.0)
SEED = workloads.SEED
ZERO = dict.fromkeys(("n_in_use", "n_fifo", "n_range", "n_few", "n_spilled", "n_small", "n_small_ok", "n_small_coll", "n_inst", "n_solo", "few_blocked"), 0)


@pytest.fixture(autouse=True)
def one_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; this one sets its own knobs and runs once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the walk sets its own thresholds: one run, under the path matrix's fifo entry")


def _spawner(life, capacity, rate):
    ps = S.ParticleSettings(lifetime=life, initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2, capacity=capacity,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]),
                            base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT))
    es = S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(rate),
                            initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), (0.0, 1.0, 0.0), 0.0), initial_velocity_radial=S.RandF32(0.0, 1.0))
    return S.ParticleSpawner([ps], [es])


def test_the_census_follows_every_transition(monkeypatch):
    import torch

    from bevy_firework_amd.system import ParticleSystem

    for k in ("FW_FIFO", "FW_RANGE", "FW_FIFO_SMALL", "FW_RANGE_SMALL", "FW_NOSPIN", "FW_SMALL", "FW_SMALL_MAX", "FW_WIDE_MAX", "FW_WIDE_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(FW_ENABLE_KNOBS="1", FW_RANGE_FEW="5", FW_FIFO_MIN="2048", FW_RANGE_MIN="2048", FW_SMALL_MIN="3").items():
        monkeypatch.setenv(k, v)
    with ParticleSystem(device=0, seed=SEED) as system:
        pairs, uid = [], [900]

        def census(what, **want):
            kept, recounted = system.path_census()
            assert kept == recounted, (what, kept, recounted)
            if want:
                assert kept == dict(ZERO, **want), (what, kept)
            return kept

        def add(life, capacity, rate, what):
            uid[0] += 1
            p = Pair(system, _spawner(life, capacity, rate), S.Transform((float(uid[0] % 7), 0.5, 0.0)), seed=SEED, uid=uid[0])
            pairs.append(p)
            census(what)
            return p

        def small(what, life=S.RandF32(0.2, 0.5)):  # one tile, ~300 live: eligible for the wave-per-type kernel once it is off a ring
            return add(life, 1024, 500.0, what)

        def remove(p, what):
            system.despawn(p.gpu)
            p.cpu.close()
            pairs.remove(p)
            census(what)

        def paths(ps):
            return [p.gpu.update_path(0)[0] for p in ps]

        def run(what, n=12):
            for fr in range(n):
                system.update(DT)
                census(f"{what}, frame {fr}")
                for p in pairs:
                    p.step_cpu(DT)
            for k, p in enumerate(pairs):
                p.check(exact_all=True, what=f"{what}, spawner {k}")
            census(f"{what}, after the reads")

        # 1. small types onto few-rings, a one-lifetime one among them (below FW_FIFO_MIN: a range ring too)
        few = [small(f"few-ring {k}", S.RandF32.constant(0.4) if k == 3 else S.RandF32(0.2, 0.5)) for k in range(5)]
        assert paths(few) == ["range"] * 5
        census("five few-rings", n_in_use=5, n_range=5, n_few=5)
        run("five few-rings")
        # 2. the sixth segment: the rings leave (drop_few_rings), and with three eligible types the wave-per-type kernel takes them
        few.append(small("the sixth segment"))
        assert paths(few) == ["small"] * 6
        census("the sixth segment", n_in_use=6, n_small_ok=6, n_small=6, few_blocked=1)
        run("six small types")
        assert census("six small types have had a frame begin")["n_solo"] == 6  # (one Global feeder each: fw_step's pass made them solo)
        # 3. nine one-lifetime types of two tiles: eight FIFO rings, the ninth spills and the eight follow it (fifo_to_range)
        big = [add(S.RandF32.constant(0.4 + 0.01 * k), 2048, 3000.0, f"FIFO ring {k}") for k in range(8)]
        assert paths(big) == ["fifo"] * 8 and paths(few) == ["small"] * 6
        census("eight FIFO rings", n_in_use=14, n_fifo=8, n_small_ok=6, n_small=6, n_solo=6, few_blocked=1)
        run("eight FIFO rings")
        big.append(add(S.RandF32.constant(0.5), 2048, 3000.0, "the ninth one-lifetime type"))
        assert paths(big) == ["range"] * 9
        census("nine spilled rings", n_in_use=15, n_range=9, n_spilled=9, n_small_ok=6, n_small=6, n_solo=6, few_blocked=1)
        run("nine spilled rings")
        # 4. the caller writes a ring's particles: it continues on the compacting path (fifo_to_general)
        parts = big[0].cpu.particles(0)[::2].copy()
        big[0].gpu.write_particles(0, parts), big[0].cpu.write_particles(0, parts)
        assert paths(big[:2]) == ["general", "range"]
        census("a ring the caller wrote", n_in_use=15, n_range=8, n_spilled=8, n_small_ok=6, n_small=6, n_solo=6, few_blocked=1)
        run("a ring the caller wrote")
        # 5. instance buffers: a windowed one keeps the ring, a plain one sends it to the compacting path; a small type keeps its kernel
        bufs = [torch.zeros(2048 * 16, dtype=torch.float32, device="cuda") for _ in range(3)]
        big[1].gpu.attach_instances_window(bufs[0].data_ptr(), 2048, particle_type=0)
        big[2].gpu.attach_instances(bufs[1].data_ptr(), 2048, particle_type=0)
        few[0].gpu.attach_instances(bufs[2].data_ptr(), 2048, particle_type=0)
        assert paths(big[1:3]) == ["range", "general"] and paths(few[:1]) == ["small"]
        census("three instance buffers", n_in_use=15, n_range=7, n_spilled=7, n_small_ok=6, n_small=6, n_solo=6, n_inst=3, few_blocked=1)
        run("three instance buffers", n=4)
        for p in (big[1], big[2], few[0]):
            p.gpu.attach_instances(0, 0, particle_type=0)
        assert paths(big[1:3]) == ["range", "general"] and paths(few[:1]) == ["small"]
        census("detached", n_in_use=15, n_range=7, n_spilled=7, n_small_ok=6, n_small=6, n_solo=6, few_blocked=1)
        run("detached")
        # 6. types leave the wave-per-type kernel when fewer than three are eligible, and enter it again with the third
        for p in few[2:]:
            remove(p, "a small type goes")
        del few[2:]
        assert paths(few) == ["general"] * 2
        census("two eligible types", n_in_use=11, n_range=7, n_spilled=7, n_small_ok=2, few_blocked=1)
        run("two eligible types")
        few.append(small("the third eligible type"))
        assert paths(few) == ["small"] * 3
        census("three eligible types", n_in_use=12, n_range=7, n_spilled=7, n_small_ok=3, n_small=3, few_blocked=1)
        run("three eligible types")
        # 7. new settings that change a type's path: two tiles and a lifetime range -- a range ring by size -- become one tile; and the
        # same settings again for a type with live particles (core.rs:343-365: particles dropped, clocks reset)
        moved = add(S.RandF32(0.2, 0.5), 2048, 3000.0, "a range ring by size")
        assert paths([moved]) == ["range"]
        census("a range ring by size", n_in_use=13, n_range=8, n_spilled=7, n_small_ok=3, n_small=3, n_solo=3, few_blocked=1)
        smaller = _spawner(S.RandF32(0.2, 0.5), 1024, 500.0)
        moved.gpu.update_settings(smaller)  # (nothing spawned yet: a fresh oracle with the new settings is its twin)
        moved.cpu.close()
        moved.cpu, moved.spawner = oracle.OracleSpawner(smaller, seed=SEED, uid=uid[0], transform=moved.cpu_transform), smaller
        assert paths([moved]) == ["small"]
        census("one tile now", n_in_use=13, n_range=7, n_spilled=7, n_small_ok=4, n_small=4, n_solo=3, few_blocked=1)
        big[3].gpu.update_settings(big[3].spawner)
        big[3].cpu.reset()
        assert paths(big[3:4]) == ["range"]  # (while spilled rings exist a one-lifetime type joins them)
        census("a ring rebuilt", n_in_use=13, n_range=7, n_spilled=7, n_small_ok=4, n_small=4, n_solo=3, few_blocked=1)
        run("after the new settings")
        # 8. destroy: everybody goes, one by one; at two segments the few-segments rule is free again, and a new small type is a ring
        while len(pairs) > 2:
            remove(pairs[-1], "destroy")
        assert census("two segments left")["few_blocked"] == 0
        last = small("a few-ring again")
        assert paths([last]) == ["range"]
        run("three segments", n=4)
        while pairs:
            remove(pairs[-1], "destroy")
        census("empty", **ZERO)
