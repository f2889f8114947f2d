"""The inputs of the random ring suite (tests/fifo_fuzz.py, tests/test_gpu_fifo_fuzz.py) on the oracle alone: every committed case builds
its spawner and its script and runs the script on oracle.OracleSpawner.  Conditions on the INPUTS, not on the library: every type is
eligible for every rule from its settings, no ring outgrows the capacity the generator gave it (a growth burst is the one exception, and
rare), and the rings are large enough for whole tiles, wraps and sixteen frames of headroom to exist.  No GPU."""
import functools

import numpy as np
import pytest

import fifo_fuzz as ff
import oracle
from bevy_firework_amd import settings as S

SEED = 0x5EED
CASE_NUMBERS = list(range(ff.CASES))


@functools.lru_cache(maxsize=None)
def _run(case):
    """-> (the case, live[frame][type] after every step, the frames inside a growth burst, per type the counts at the final read)"""
    c = ff.draw_case(case)
    o = oracle.OracleSpawner(c["spawner"], seed=SEED, uid=c["uid"], transform=c["transform"])
    if c["modifier"] is not None:
        o.set_modifier(c["modifier"])
    live, bursting, burst_until = [], set(), -1
    for action in c["script"]:
        if action[0] == "queue" and action[2] >= 0:
            burst_until = max(burst_until, action[2])
        ff.apply_to_oracle(o, action)
        if action[0] == "step":
            if len(live) <= burst_until:
                bursting.add(len(live))
            live.append(o.counts())
    final = o.counts()
    o.close()
    return c, live, bursting, final


@pytest.mark.parametrize("case", CASE_NUMBERS)
def test_every_type_is_eligible_and_stays_inside_its_ring(case):
    c, live, bursting, final = _run(case)
    sp = c["spawner"]
    assert ff.eligible(sp) == [[] for _ in sp.particle_settings]
    assert 80 <= len(live) <= 110
    for t, p in enumerate(sp.particle_settings):
        L = ff.life_frames(sp, t)
        assert 2.5 <= L <= 30.0 and 0.05 < L - np.floor(L) < 0.95
        assert 149.0 <= ff.per_frame(sp, t) <= 1201.0
        assert ff.CAP_MIN <= p.capacity <= ff.CAP_MAX and p.capacity & (p.capacity - 1) == 0
        assert any(L + h <= p.capacity / ff.per_frame(sp, t) + 1e-3 for h in ff.HEADROOMS)
        for f, counts in enumerate(live):
            assert counts[t] <= p.capacity or f in bursting, (case, t, f, counts, p.capacity)
        assert final[t] >= 100, (case, final)
    assert c["script"][-2][:2] == ("read", "read_particles") and c["script"][-1] == ("totals",)
    stretch, longest = 0, 0
    for action in c["script"]:
        stretch = stretch + 1 if action[0] == "step" else (0 if action[0] == "read" else stretch)
        longest = max(longest, stretch)
    assert longest <= 40


def test_the_cases_do_real_work():
    runs = [_run(case) for case in CASE_NUMBERS]
    # from frame 40 on, some ring of the case holds four tiles of live particles at every frame: in at least half of the cases
    large = [min(max(counts) for counts in live[40:]) >= 4 * ff.TILE for _, live, _, _ in runs]
    assert sum(large) * 2 >= len(runs), sum(large)
    assert sum(bool(bursting) for _, _, bursting, _ in runs) * 8 <= len(runs)
    two = [len(c["spawner"].particle_settings) == 2 for c, _, _, _ in runs]
    assert len(runs) // 6 <= sum(two) <= len(runs) // 2, sum(two)


def test_the_draws_cover_what_the_suite_is_about():
    """every axis with each sign, angular drag zero and not, every pacing and shape, every headroom's rings, every knob value, every
    keeper, every reader, the three odd frames"""
    cases = [ff.draw_case(case) for case in CASE_NUMBERS]
    axes, drags, pacings, shapes = set(), set(), set(), set()
    for c in cases:
        sp = c["spawner"]
        drags |= {p.angular_drag == 0.0 for p in sp.particle_settings}
        for e in sp.emission_settings:
            d = e.initial_angular_velocity.direction
            axes.add(tuple(int(x) for x in d))
            p = e.emission_pacing
            pacings.add("demand" if p.kind == S.PACING_ONDEMAND else "rate" if (p.duration, p.offset_start, p.offset_end) == (1.0, 0.0, 1.0) else "cod")
            shapes.add(e.emission_shape.kind)
    assert len(axes) == 6 and drags == {True, False} and pacings == {"rate", "cod", "demand"} and len(shapes) == 3
    for key, values in (("FW_FUSE_DEPTH", (2, 3, 4, 8)), ("FW_WHOLE_TILES", (0, 1)), ("FW_NEWBORN_SPIN", (0, 1)), ("FW_SPIN_LOG", (4, 16, 256)),
                        ("FW_PARAM_BAR", (0, 1))):
        assert {c["env"][key] for c in cases} == {str(v) for v in values}, key
    far = {int(c["env"]["FW_FUSE_FAR_DEPTH"]) for c in cases}  # (nine values, 16 the most frequent: most of them, and both ends)
    assert far <= set(range(8, 17)) and len(far) >= 7 and {8, 16} <= far, far
    assert all(c["env"][k] == v for c in cases for k, v in ff.FORCING.items())
    acts = [a for c in cases for a in c["script"]]
    assert {a[0] for a in acts} == {"step", "read", "totals"} | set(ff.KEEPERS)
    assert {a[1] for a in acts if a[0] == "read"} == set(ff.READERS)
    odd = {np.float32(a[1]).tobytes() for a in acts if a[0] == "step"} & {d.tobytes() for d in ff.ODD_DTS}
    assert len(odd) == len(ff.ODD_DTS)
