"""The generator of the random ring suite (tests/test_fifo_fuzz_cpu.py, tests/test_gpu_fifo_fuzz.py): random spawners whose every type is
a FIFO ring under the age rule and the axis rule BY CONSTRUCTION -- so its spin is deferred, its newborns' too, and its unread frames run
fused, up to sixteen in a launch -- with everything the rules leave free drawn at random, and random hosts: irregular steps, moves,
parent velocities, modifiers and bursts that keep a stretch unread, and every kind of reader at the end of stretches of 1 to 40 frames.
The hand-written fused files (test_gpu_fifo_fuse2.py .. test_gpu_fifo_fuse_far.py) turn one spawner family; tests/test_gpu_fuzz.py draws
everything but never meets the rules (cones on the angular velocity, product thresholds, a read every sixth frame).
No GPU module is imported here: the CPU twin runs every committed case on the oracle alone and asserts that the inputs are what this
docstring says.  All draws of a case come from np.random.default_rng(SEED_BASE + case), in the order spawner, placement, knobs, script."""
import math

import numpy as np

from bevy_firework_amd import settings as S
from test_gpu_fuzz import _curve, _gradient, _unit

SEED_BASE = 330000
CASES = 48
DT = np.float32(1.0 / 60.0)
DT_MAX = 0.03            # the longest frame a script draws
TILE = 1024              # FW_TILE: the slots of a four-round ring tile
CAP_MIN, CAP_MAX = 4096, 65536
HEADROOMS = (3, 9, 20, 40)
ODD_DTS = (np.float32(0.0), np.float32(1e-40), np.float32(-1.0 / 240.0))  # zero, a denormal, a negative one: no rule holds in such a frame
# the knobs that force the machinery at these sizes: tests/test_gpu_fifo_fuse_far.py's FAR on top of test_gpu_fifo_fuse2.py's set
FORCING = {"FW_FIFO_SMALL": "1", "FW_SPIN_DEFER_MIN": "1", "FW_SPIN_DEFER_AFTER": "2", "FW_FUSE2_MIN": "1", "FW_FUSE_DEEP_MIN": "1",
           "FW_FUSE_WIDE_MIN": "1", "FW_FUSE_FAR_MIN": "1"}
KEEPERS = ("set_transform", "set_parent_velocity", "set_modifier", "queue")
# the entry points that ask for the particles or the stream (test_gpu_fifo_fuse2.FIRST_CALLERS without update_settings) and the volume query
READERS = ("read_particles", "pack_instances", "pack_instances_device", "pack_instances_sorted", "pack_instances_sorted_device", "aabb", "counts",
           "poll_finished", "updated_total", "synchronize", "write_particles", "attach_instances", "set_colliders", "cast_rays", "count_in_volumes")


def _f32(x):
    return float(np.float32(x))


def _quat(rng):
    q = rng.normal(size=4)
    return tuple(float(c) for c in q / np.linalg.norm(q))


def _pow2_at_least(n):
    return 1 << max(0, int(math.ceil(n)) - 1).bit_length()


def _about(k, angle):
    """a rotation about coordinate axis k: the other two components +0 whatever the angle's sign (0.0 * negative would be -0)"""
    q = [0.0, 0.0, 0.0, float(np.cos(angle / 2))]
    q[k] = float(np.sin(angle / 2))
    return tuple(q)


def _velocity(rng):
    lo = float(rng.uniform(0.0, 3.0))
    return S.RandVec3(S.RandF32(lo, float(lo + rng.uniform(0.0, 6.0))), _unit(rng), float(rng.uniform(0.0, math.pi)))


def _shape(rng):
    return [S.EmissionShape.Point(), S.EmissionShape.Sphere(float(rng.uniform(0.1, 2.0))),
            S.EmissionShape.Circle(_unit(rng), float(rng.uniform(0.1, 2.0)))][int(rng.integers(0, 3))]


def ring_spawner(rng):
    """one type, or two in about a third of the draws; every type eligible for every rule (`eligible`), everything else drawn.
    P new particles per frame (the sum of the type's peak rates) over a constant lifetime of L frames, L no integer, in the smallest power
    of two from 4096 to 65536 that holds (L + h) * P: a small h makes the capacity close groups, a small L the death rule, large ones
    leave the depth limit.  The first entry of a type is a `rate`; at most one entry of the spawner is OnDemand (the first one takes the
    whole queue)."""
    n_types = 2 if rng.random() < 1.0 / 3.0 else 1
    types, entries, on_demand = [], [], False
    for t in range(n_types):
        L = float(rng.uniform(2.5, 30.0))
        L = math.floor(L) + min(max(L - math.floor(L), 0.06), 0.94)  # (an integer number of frames would die on an fp32 rounding)
        h = int(rng.choice(HEADROOMS, p=(0.15, 0.15, 0.35, 0.35)))
        P = float(rng.uniform(150.0, 1200.0))
        P = min(P, math.floor(CAP_MAX / (L + h)))
        capacity = max(CAP_MIN, _pow2_at_least((L + h) * P))
        k, sign = int(rng.integers(0, 3)), (1.0 if rng.random() < 0.5 else -1.0)
        direction = [0.0, 0.0, 0.0]
        direction[k] = sign
        types.append(S.ParticleSettings(
            lifetime=S.RandF32.constant(_f32(float(DT) * L)), scale_curve=_curve(rng), initial_scale=S.RandF32(0.01, float(rng.uniform(0.02, 0.2))),
            acceleration=tuple(float(c) for c in rng.uniform(-10.0, 10.0, size=3)), angular_acceleration=(0.0, 0.0, 0.0),
            linear_drag=0.0 if rng.random() < 0.25 else float(rng.uniform(0.0, 1.0)),
            angular_drag=0.0 if rng.random() < 0.35 else float(rng.uniform(0.0, 1.0)),
            base_color=_gradient(rng), emissive_color=_gradient(rng), pbr=bool(rng.random() < 0.5), capacity=capacity))
        # (a launch carries eight ops and only a ring's first op of a frame may continue its last one: a ring with two entries that emit
        # in every frame closes its groups at four frames, one with three at two -- most rings have one entry)
        n_entries = int(rng.choice([1, 2, 3], p=(0.7, 0.18, 0.12)))
        kinds = ["rate"] + [str(rng.choice(["rate", "cod", "cod", "demand"])) for _ in range(n_entries - 1)]
        for i, kind in enumerate(kinds):  # (one OnDemand entry in the spawner)
            if kind == "demand":
                kinds[i], on_demand = ("rate" if on_demand else "demand"), True
        paced = [i for i, kind in enumerate(kinds) if kind != "demand"]
        share = rng.uniform(0.2, 1.0, size=len(paced))
        share[0] += 0.6  # (the `rate` entry never starves the ring)
        share = share / share.sum() * P
        for i, kind in enumerate(kinds):
            if kind == "rate":
                pacing = S.EmissionPacing.rate(float(share[paced.index(i)] * 60.0))
            elif kind == "cod":  # a window inside its duration: the entry emits nothing in some frames, at its share of P in the others
                dur = float(rng.uniform(0.3, 1.5))
                a = float(rng.uniform(0.0, 0.6))
                b = float(min(1.0, a + rng.uniform(0.2, 0.8)))
                pacing = S.EmissionPacing.CountOverDuration(float(share[paced.index(i)] * 60.0 * dur * (b - a)), dur, a, b)
            else:
                pacing = S.EmissionPacing.OnDemand()
            lo = float(rng.uniform(0.2, 4.0))
            entries.append(S.EmissionSettings(
                particle_index=t, emission_pacing=pacing, emission_shape=_shape(rng), initial_velocity=_velocity(rng),
                initial_velocity_radial=S.RandF32(0.0, float(rng.uniform(0.0, 3.0))), inherit_parent_velocity=bool(rng.random() < 0.5),
                initial_rotation=_about(k, float(rng.uniform(-math.pi, math.pi))),
                initial_angular_velocity=S.RandVec3(S.RandF32(lo, float(lo + rng.uniform(0.1, 6.0))), tuple(direction), 0.0)))
    order = rng.permutation(len(entries))  # (entries of two types interleave: a ring's ops are not the first ops of the frame)
    return S.ParticleSpawner(types, [entries[i] for i in order])


def per_frame(spawner, t):
    """P of type t: what its paced entries spawn in a frame of DT at their peak"""
    total = 0.0
    for e in spawner.emission_settings:
        p = e.emission_pacing
        if e.particle_index == t and p.kind == S.PACING_COUNT_OVER_DURATION:
            total += p.count / (p.duration * (p.offset_end - p.offset_start)) * float(DT)
    return total


def life_frames(spawner, t):
    return spawner.particle_settings[t].lifetime.min / float(DT)


def headroom(spawner, t):
    """the slots of type t beyond what its paced entries can ever hold: rate x lifetime and one long frame's spawns (three frames of DT)"""
    return spawner.particle_settings[t].capacity - int(math.ceil((life_frames(spawner, t) + 3.0) * per_frame(spawner, t)))


def _zero_bits(x):
    return np.float32(x).view(np.uint32) == 0


def eligible(spawner):
    """fw_engine_launch.cpp: ring_rules and fw_engine_build.cpp: axis_spin_rule, from the settings alone -> one list of broken conditions
    per type (empty: a FIFO ring under the age rule whose spin is deferred, in every frame of a positive normal dt up to DT_MAX)"""
    out = []
    fin = lambda x: bool(np.isfinite(np.float32(x)))
    pos = lambda x: fin(x) and not np.signbit(np.float32(x))
    for t, p in enumerate(spawner.particle_settings):
        bad = []
        feeders = [e for e in spawner.emission_settings if e.particle_index == t]
        # a FIFO ring with position and age in planes (fw_update_path.h): one finite lifetime, Global entries alone that fit the launch's
        # arguments, no collisions, large enough for a four-round tile under FW_FIFO_SMALL=1
        if not (p.lifetime.min == p.lifetime.max and fin(p.lifetime.min) and p.lifetime.min > 0.0):
            bad.append("one lifetime value")
        if any(e.emission_mode.kind != S.MODE_GLOBAL for e in spawner.emission_settings):
            bad.append("Global entries only")
        if not 1 <= len(feeders) <= 8:
            bad.append("one to eight feeding entries")
        if p.collision_settings is not None or p.particles_destroyed is not None:
            bad.append("no collisions, no destroyed stream")
        if not (TILE <= p.capacity < 0x40000000):
            bad.append("a capacity of a tile or more")
        # the axis rule, C1 to C4, for some axis k
        axis = None
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            acc = p.angular_acceleration
            if not (_zero_bits(acc[a]) and _zero_bits(acc[b]) and np.float32(acc[k]) == 0.0 and pos(p.angular_drag)):  # (C3)
                continue
            ok, wmax = bool(feeders), 0.0
            for e in feeders:
                w, r = e.initial_angular_velocity, e.initial_rotation
                ok = ok and not w.spread > 0.0 and _zero_bits(w.direction[a]) and _zero_bits(w.direction[b]) and fin(w.direction[k]) \
                    and pos(w.magnitude.min) and pos(w.magnitude.max) \
                    and _zero_bits(r[a]) and _zero_bits(r[b]) and fin(r[k]) and fin(r[3])  # (C1, C2)
                wmax = max(wmax, abs(w.direction[k]) * max(w.magnitude.min, w.magnitude.max))
            if ok and fin(wmax):  # (C4)
                axis = (k, wmax)
                break
        if axis is None:
            bad.append("the axis rule")
        else:  # axis_dt_ok for every dt a script draws
            v = np.float32(axis[1]) * np.float32(DT_MAX)
            if not (np.float32(0.25) * (v * v) < np.float32(0.6) and np.float32(p.angular_drag) * np.float32(DT_MAX) <= 1.0):
                bad.append("axis_dt_ok at the longest frame")
        out.append(bad)
    return out


def knobs(rng):
    """the environment of a case on top of FORCING.  The far tier applies at FW_FUSE_DEPTH=8 (and with deferred newborns) only, so 8 is
    drawn more often than 2, 3 and 4, and 16 more often than the other far depths: each depth of 9 to 16 needs its own cases"""
    env = dict(FORCING)
    env["FW_FUSE_FAR_DEPTH"] = str(16 if rng.random() < 0.55 else int(rng.integers(8, 17)))
    env["FW_FUSE_DEPTH"] = str(8 if rng.random() < 0.8 else int(rng.choice([2, 3, 4])))
    env["FW_WHOLE_TILES"] = str(int(rng.random() < 0.6))
    env["FW_NEWBORN_SPIN"] = str(int(rng.random() < 0.08))
    # (a log at its cap is replayed, and the replay puts the withheld group on the stream first: a cap of 4 closes every group at four frames)
    env["FW_SPIN_LOG"] = str(int(rng.choice([4, 16, 256], p=(0.15, 0.35, 0.5))))
    env["FW_PARAM_BAR"] = str(int(rng.random() < 0.7))
    return env


def depth_limit(env):
    """the deepest fused launch the knobs allow (tests/test_gpu_fifo_fuse_far.py: eager newborns keep a ring off the far tier)"""
    if env["FW_FUSE_DEPTH"] == "8" and env["FW_NEWBORN_SPIN"] == "0":
        return int(env["FW_FUSE_FAR_DEPTH"])
    return int(env["FW_FUSE_DEPTH"])


def _stretch(rng):
    """the frames up to the next reader: 1 to 40, those of 12 to 34 -- behind which a reader finds a deep group pending -- more often"""
    return int(rng.integers(1, 41)) if rng.random() < 0.4 else int(rng.integers(12, 35))


def host_script(rng, spawner, frames):
    """-> a list of actions, applied alike to every run and to the oracle:
    ("step", dt) | ("set_transform", translation, rotation) | ("set_parent_velocity", v) | ("set_modifier", scale, speed) |
    ("queue", n, last frame of the growth burst or -1) | ("read", name, particle type, stride) | ("totals",)
    The keepers act in front of a frame with small probabilities -- each host has its own -- and leave a stretch unread; a reader
    follows the last frame of a stretch of 1 to 40 frames."""
    demand = next((e.particle_index for e in spawner.emission_settings if e.emission_pacing.kind == S.PACING_ONDEMAND), None)
    # a quarter of the hosts move the emitter in nearly every frame of one phase: no op continues the one before it there
    busy_from = int(rng.integers(0, frames)) if rng.random() < 0.25 else frames
    busy_to, p_busy = busy_from + int(rng.integers(10, 31)), float(rng.uniform(0.4, 1.0))
    p_keep = {"set_transform": float(rng.uniform(0.0, 0.06)), "set_parent_velocity": float(rng.uniform(0.0, 0.05)),
              "set_modifier": float(rng.uniform(0.0, 0.04)), "queue": float(rng.uniform(0.03, 0.15))}
    grows = demand is not None and rng.random() < 0.25  # (at most one case in eight grows a ring: tests/test_fifo_fuzz_cpu.py counts)
    grow_at = int(rng.integers(30, frames - 20)) if grows else -1
    out, now, queued = [], 0.0, []
    left = _stretch(rng)
    for f in range(frames):
        for name in KEEPERS:
            if name == "queue":
                if demand is None or not (rng.random() < p_keep[name] or f == grow_at):
                    continue
                life, room = spawner.particle_settings[demand].lifetime.min, headroom(spawner, demand)
                queued = [(t, n) for t, n in queued if now - t < life + 2.0 * DT_MAX]  # (bursts that may still be alive)
                room -= sum(n for _, n in queued)
                if f == grow_at:  # a growth burst: more than the ring has room for -- it grows, with whatever is withheld
                    n = int(spawner.particle_settings[demand].capacity * rng.uniform(0.6, 1.2))
                    out.append(("queue", n, f + int(math.ceil(life / float(DT))) + 2))
                elif room >= 8:
                    n = int(rng.integers(1, max(2, min(room, 6000))))
                    queued.append((now, n))
                    out.append(("queue", n, -1))
            elif rng.random() < (p_busy if name == "set_transform" and busy_from <= f < busy_to else p_keep[name]):
                if name == "set_transform":
                    out.append((name, tuple(float(c) for c in rng.uniform(-3.0, 3.0, size=3)), _quat(rng)))
                elif name == "set_parent_velocity":
                    out.append((name, tuple(float(c) for c in rng.uniform(-2.0, 2.0, size=3))))
                else:
                    out.append((name, float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))))
        r = rng.random()
        dt = DT if r < 0.85 else (np.float32(rng.uniform(0.004, DT_MAX)) if r < 0.98 else ODD_DTS[int(rng.integers(0, len(ODD_DTS)))])
        # (a negative dt voids the axis rule's proof for good, ring_record: the ring never defers again -- late, when the case has worked)
        if np.signbit(dt) and f < frames - 25:
            dt = ODD_DTS[0]
        out.append(("step", dt))
        now += max(float(dt), 0.0)
        left -= 1
        if left == 0 and f < frames - 1:
            name = READERS[int(rng.integers(0, len(READERS)))]
            if name == "write_particles" and (f < 50 or rng.random() < 0.5):
                name = "read_particles"  # (a rewritten ring has to earn its rules again: late and seldom)
            out.append(("read", name, int(rng.integers(0, len(spawner.particle_settings))), int(rng.integers(2, 4))))
            left = _stretch(rng)
    out.append(("read", "read_particles", 0, 1))
    out.append(("totals",))
    return out


def draw_case(case, seed_base=SEED_BASE):
    """-> dict(spawner, transform, modifier, env, script, uid): everything the runs of a case share"""
    rng = np.random.default_rng(seed_base + case)
    spawner = ring_spawner(rng)
    transform = S.Transform(tuple(float(c) for c in rng.uniform(-2.0, 2.0, size=3)), _quat(rng))
    modifier = S.EffectModifier(float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))) if rng.random() < 0.5 else None
    env = knobs(rng)
    script = host_script(rng, spawner, int(rng.integers(80, 111)))
    return dict(spawner=spawner, transform=transform, modifier=modifier, env=env, script=script, uid=33000 + case)


def apply_to_oracle(o, action):
    """one action of a script on an oracle.OracleSpawner; readers read nothing there except write_particles, which both sides apply"""
    kind = action[0]
    if kind == "step":
        o.step(np.float32(action[1]))
    elif kind == "set_transform":
        o.set_origin(action[1], action[2])
    elif kind == "set_parent_velocity":
        o.set_parent_velocity(action[1])
    elif kind == "set_modifier":
        o.set_modifier(S.EffectModifier(action[1], action[2]))
    elif kind == "queue":
        o.queue_particles(action[1])
    elif kind == "read" and action[1] == "write_particles":
        o.write_particles(action[2], o.particles(action[2])[:: action[3]].copy())
