"""The FIFO launches compiled for "no ring tile touches rotation or angular velocity" (FwFifoArgs::spinless, the SPINLESS instantiations of
fw_k_update_fifo): a launch all of whose rings cannot turn or have their spin deferred in it, without an instance
buffer, on four-round tiles, runs a form of the kernel in which that is a fact of the code -- 88 registers instead of 110, a fifth workgroup
per CU -- and must compute exactly what the form that finds out per workgroup computes.  Every case runs the same system three times: with
FW_SPIN_DEFER=0 and FW_SPINLESS=0 (no launch defers, no launch takes the new form), with the deferred spin and FW_SPINLESS=0, and with the
deferred spin and FW_SPINLESS=1 (the product).  Every field of every read must carry the same bits in all three, and
fw_debug_spinless_launches says, frame by frame, that the third run took the new form in the frames it should and in no others (the other two:
never).  Knobs, sizes and lifetimes as in test_gpu_spin_defer.py, whose spawner and Run this file borrows.  Needs an MI355X."""
import dataclasses

import numpy as np
import pytest

import oracle  # noqa: F401
from bevy_firework_amd import settings as S
from bevy_firework_amd import workloads
from parity import Pair
from test_gpu_spin_defer import AFTER, DT, SEED, SPIN_BYTES, X, Y, Z, Run, _rot_about, _spawner

pytestmark = pytest.mark.gpu
RUNS = (("no rule", "0", "0"), ("old form", "1", "0"), ("spinless", "1", "1"))  # (name, FW_SPIN_DEFER, FW_SPINLESS)


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the spin-less forms belong to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _still(life_frames=2.5, rate=270000.0, rot=None, **kw):
    """the same particles as _spawner's, but born without angular velocity and all with one rotation: a type that cannot turn"""
    ps = S.ParticleSettings(lifetime=S.RandF32.constant(float(DT) * life_frames), initial_scale=S.RandF32(0.5, 2.0), linear_drag=0.2,
                            scale_curve=S.FireworkCurve.even_samples([1.0, 2.0, 0.5]), capacity=8192,
                            base_color=S.FireworkGradient.uneven_samples(workloads.STRESS_GRADIENT), **kw)
    es = [S.EmissionSettings(emission_pacing=S.EmissionPacing.rate(rate), initial_velocity=S.RandVec3(S.RandF32(1.0, 6.0), Y, 0.0),
                             initial_velocity_radial=S.RandF32(0.0, 1.0), initial_rotation=rot or _rot_about(Z, 0.4))]
    return S.ParticleSpawner([ps], es)


def _two_types(a, b, entry_b=0):
    """the types of two one-type spawners as types 0 and 1 of one spawner: two FIFO rings of the same launch"""
    ea, eb = a.emission_settings[0], dataclasses.replace(b.emission_settings[entry_b], particle_index=1)
    return S.ParticleSpawner([a.particle_settings[0], b.particle_settings[0]], [ea, eb])


class Run3(Run):
    """a Run that asks the counter after every frame.  What the frame's launch should have been is worked out from what the host reports
    through another door -- fw_debug_update_path: the bytes a particle of each ring moved in the latest launch, SPIN_BYTES fewer when the
    launch deferred the ring's spin -- and from what the case itself did (an instance buffer attached)."""

    def __init__(self, system, pair, rule, form, still):
        super().__init__(system, pair, rule)
        self.form, self.still, self.inst, self.taken = form, still, False, []
        self.base = [pair.gpu.update_path(t) for t in range(pair.n_types)]

    def ring_leaves_spin_alone(self, t):
        path = self.pair.gpu.update_path(t)
        if path[0] != "fifo":
            return False
        return t in self.still or path[1] == self.base[t][1] - 8 - SPIN_BYTES

    def step(self, dt=DT, n=1):
        for _ in range(n):
            n0, held = self.system.spinless_launches(), sum(self.pair.gpu.counts())
            super().step(dt)
            self.taken.append(self.system.spinless_launches() - n0)
            # (a context that held fewer than 1024 particles when the frame began runs it on one-round tiles, FW_FIFO_SMALL=1: never the new form)
            want = (self.form and not self.inst and held >= 1024
                    and all(self.ring_leaves_spin_alone(t) for t in range(self.pair.n_types)))
            assert self.taken[-1] == (1 if want else 0), (self.frame, self.rule, self.form, self.taken[-8:], [self.pair.gpu.update_path(t) for t in range(self.pair.n_types)])

    def took(self, new_form, frames=1):
        """the latest `frames` launches: the new form (in the run that has it), or not -- what the CASE knows about its own frames"""
        assert self.taken[-frames:] == [1 if (new_form and self.form) else 0] * frames, (self.frame, self.rule, self.form, self.taken)


def three(monkeypatch, spawner, scenario, still=(), **env):
    """runs `scenario(run)` under the three settings of RUNS; every read of the three runs must carry the same bits"""
    from bevy_firework_amd.system import ParticleSystem

    reads, taken = {}, {}
    for name, rule, form in RUNS:
        for k in ("FW_DERIVED", "FW_PARAM_BAR", "FW_NOSPIN", "FW_AXIS_SPIN", "FW_AGELESS", "FW_SPIN_LOG", "FW_NT_MB", "FW_NT_WO_MB"):
            monkeypatch.delenv(k, raising=False)  # (the product's choice, whatever the path matrix dealt this test)
        for k, v in (("FW_ENABLE_KNOBS", "1"), ("FW_FIFO", "1"), ("FW_FIFO_MIN", "0"), ("FW_RANGE", "0"), ("FW_SMALL", "0"), ("FW_FIFO_SMALL", "1"),
                     ("FW_SPIN_DEFER_MIN", "1"), ("FW_SPIN_DEFER_AFTER", str(AFTER)), ("FW_SPIN_DEFER", rule), ("FW_SPINLESS", form)) + tuple(env.items()):
            monkeypatch.setenv(k, v)
        with ParticleSystem(device=0, seed=SEED) as system:
            run = Run3(system, Pair(system, spawner, S.Transform((1.0, 2.0, 3.0)), seed=SEED, uid=21), rule == "1", form == "1", set(still))
            scenario(run)
            reads[name], taken[name] = run.reads, run.taken
    assert not any(taken["no rule"]) and not any(taken["old form"]) and any(taken["spinless"]), taken
    for name in ("old form", "spinless"):
        assert [w for w, _ in reads[name]] == [w for w, _ in reads["no rule"]] and len(reads[name]) > 0
        for (what, a), (_, b) in zip(reads[name], reads["no rule"]):
            assert a == b, f"{what}: the bits of the run `{name}` differ from those of the run without either rule"
    return taken["spinless"]


@pytest.mark.parametrize("every, life_frames, frames", [(1, 2.5, 12), (7, 16.0, 35), (7, 2.5, 35), (0, 16.0, 40)],
                         ids=["every frame", "every 7th frame", "every 7th frame, short lives", "only at the end"])
def test_deferred_and_replayed_launches_alternate(monkeypatch, every, life_frames, frames):
    def scenario(run):
        for fr in range(frames):
            run.step()
            if every and fr >= every:  # (a launch defers from the third qualifying one of an unread stretch on: test_gpu_spin_defer.py)
                run.took(fr % every + 1 > AFTER)
            if every and fr % every == every - 1:
                run.read()
        if not every:
            run.took(True, frames=frames - AFTER - 2)
        run.read("end")
        run.step(n=AFTER)  # (the read replayed the spin: the rule is earned again, launch by launch)
        run.took(False, frames=AFTER)
        run.step(n=2)
        run.took(True, frames=2)
        run.read("after two more spin-less launches")

    taken = three(monkeypatch, _spawner(life_frames=life_frames, capacity=16384 if life_frames > 8 else 8192), scenario)  # (long lives: a ring that does not grow on the way)
    if every == 1:
        assert taken[:frames] == [0] * frames  # (a host that reads every frame: its launches load every plane, none of them takes the new form)


def test_new_particles_split_over_the_rings_end(monkeypatch):
    """forty unread frames of 4500 new particles each with 2.5-frame lifetimes: the ring's head goes round several times, and in the frames
    in which the new particles straddle the ring's end they come in two groups of spawning workgroups (FwFifoSeg::n_vt_a / n_vt_b) in front
    of the spin-less tiles"""
    def scenario(run):
        born = 0
        for _ in range(40):
            before = run.pair.cpu.counts()[0]
            run.step()
            born = max(born, run.pair.cpu.counts()[0] - before)  # (the first frame's growth: what one frame spawns)
        run.took(True, frames=30)
        live = run.pair.gpu.count(0)
        assert 4000 < live < 12500 and born >= 4000  # (many spawning workgroups of 256 per frame: a straddling frame has them on both sides)
        # (40 frames x 4500 new particles go round a ring of at most 32768 slots -- what 12500 live particles can have grown it to -- five times)
        assert 40 * 4500 > 5 * 32768
        run.read("end")

    three(monkeypatch, _spawner(), scenario)


@pytest.mark.parametrize("derived", [True, False], ids=["derived", "scale and colour planes stored: the generic write mask"])
def test_a_type_that_cannot_turn(monkeypatch, derived):
    """no deferral involved: FW_TYPE_NOSPIN is the type's own, every launch of at least one four-round tile takes the new form, reads in
    between or not.  With FW_DERIVED=0 the type stores scale and base colour: write mask 5, the form with the mask read from the type"""
    def scenario(run):
        run.step(n=6)
        run.took(True, frames=5)
        run.read("early")
        run.step(n=9)
        run.took(True, frames=9)
        run.read("end")
        parts = run.pair.gpu.particles(0)
        assert np.array_equal(parts["rotation"], np.broadcast_to(np.float32(_rot_about(Z, 0.4)), parts["rotation"].shape))
        assert not parts["angular_velocity"].view(np.uint32).any()

    three(monkeypatch, _still(), scenario, still=(0,), **({} if derived else {"FW_DERIVED": "0"}))


def test_a_ring_that_cannot_turn_next_to_a_deferred_ring(monkeypatch):
    def scenario(run):
        run.step(n=AFTER + 1)
        run.took(False, frames=AFTER + 1)  # (the spinning ring has not earned its rule yet: its tiles load rotation and angular velocity)
        run.step(n=10)
        run.took(True, frames=10)
        run.read("end")
        run.step(n=AFTER)
        run.took(False, frames=AFTER)
        run.step(n=3)
        run.took(True, frames=3)
        run.read("again")

    three(monkeypatch, _two_types(_still(), _spawner()), scenario, still=(0,))


def test_a_deferred_ring_next_to_a_ring_that_has_not_qualified_yet(monkeypatch):
    """type 0 spins about y and defers from its fourth frame on; type 1 spins about y as well but holds nothing until frame 10, when 5000
    particles are queued for it -- an empty ring does not qualify, a ring in its first launches has not yet: the launch of the two is not
    spin-less until BOTH rings leave their spin alone"""
    def scenario(run):
        run.step(n=10)
        run.took(False, frames=10)
        run.expect(run.base[0], t=0)  # (type 0 defers all the same)
        run.pair.queue(5000)
        run.step(n=AFTER + 1)  # (the launch that spawns them finds an empty ring; then AFTER qualifying ones)
        run.took(False, frames=AFTER + 1)
        run.step(n=6)
        run.took(True, frames=5)
        run.read("end")
        assert run.pair.gpu.counts()[1] == 5000

    three(monkeypatch, _two_types(_spawner(), _spawner(life_frames=16.0, on_demand=True), entry_b=1), scenario)


@pytest.mark.parametrize("axis, sign", [(X, 1.0), (Y, -1.0), (Z, 1.0)], ids=["+x", "-y", "z"])
def test_every_axis(monkeypatch, axis, sign):
    def scenario(run):
        run.step(n=14)
        run.took(True, frames=10)
        run.read("end")
        parts = run.pair.gpu.particles(0)
        k = axis.index(1.0)
        assert np.all(np.sign(parts["angular_velocity"][:, k]) == sign) and np.all(parts["rotation"][:, k] != 0)

    three(monkeypatch, _spawner(axis=axis, sign=sign, rot_angle=1.1), scenario)


def test_jittering_dt(monkeypatch):
    rng = np.random.default_rng(21)
    dts = [float(x) for x in rng.uniform(0.004, 0.02, size=26)]

    def scenario(run):
        for k, dt in enumerate(dts):
            run.step(dt)
            if k in (9, 10, 25):
                run.took(k != 10)
                run.read(f"dt {dt}")

    three(monkeypatch, _spawner(life_frames=16.0), scenario)


def test_zero_and_negative_dt_inside_a_stretch(monkeypatch):
    """a frame of +0 runs undeferred -- the old form, every plane loaded -- and the ring earns the new form again; a negative one sends the
    ring to the compacting path: no FIFO launch at all from then on"""
    def scenario(run):
        run.step(n=8)
        run.took(True, frames=4)
        run.step(0.0)
        run.took(False)
        run.step(n=AFTER)
        run.took(False, frames=AFTER)
        run.step(n=3)
        run.took(True, frames=3)
        run.step(0.0)
        run.read("right after a frame of zero")
        run.step(n=6)
        run.took(True, frames=3)
        run.step(-1.0 / 240.0)
        run.took(False)
        assert run.bytes_moved()[0] == "general"
        run.read("after the negative step")
        run.step(n=3)
        run.took(False, frames=3)
        run.read("on the compacting path")

    three(monkeypatch, _spawner(life_frames=16.0, capacity=16384), scenario)


def test_instance_buffer_attached_mid_stretch(monkeypatch):
    import torch

    def scenario(run):
        cap = 16384
        buf = torch.full((cap * 16,), float("nan"), dtype=torch.float32, device="cuda")
        run.step(n=9)
        run.took(True, frames=5)
        run.pair.gpu.attach_instances(buf.data_ptr(), cap)
        run.inst = True
        for k in range(5):
            run.step()
            run.took(False)  # (a launch that writes records: the instance-writing form, which evaluates the rotation)
            run.keep(f"records {k}", buf[: run.pair.gpu.count(0) * 16].cpu().numpy())
        run.read("attached")
        run.pair.gpu.attach_instances(0, 0)
        run.inst = False
        run.step(n=AFTER + 6)
        run.took(True, frames=5)
        run.read("detached")

    three(monkeypatch, _spawner(), scenario)


@pytest.mark.parametrize("knob", ["FW_NT_MB", "FW_NT_WO_MB"])
@pytest.mark.parametrize("still", [False, True], ids=["deferred", "cannot turn"])
def test_non_temporal_forms(monkeypatch, knob, still):
    """FW_NT_MB=0: every launch takes the fully non-temporal form (NT = 2); FW_NT_WO_MB=0: the one with non-temporal stores of the
    write-only planes (NT = 1)"""
    def scenario(run):
        run.step(n=6)
        run.read("early")
        run.step(n=7)
        run.took(True, frames=4)
        run.read("end")

    three(monkeypatch, _still() if still else _spawner(), scenario, still=(0,) if still else (), **{knob: "0"})
