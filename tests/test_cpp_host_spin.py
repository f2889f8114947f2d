"""The deferred spin of a FIFO ring without a GPU (csrc/fw_spin.h: the lookup fw_k_fifo_spin runs per lane and the log the host keeps):
a stand-alone C++ program, compiled here with g++ -- once plainly, once with -fsanitize=address,undefined --, drives FwSpinBook through
schedules of frames the way launch_fifo (ring_rules, age_cohorts) and ensure_spin do (a deferred frame logs its dt, a cohort spawned in it points behind that entry,
dead cohorts leave and the log is trimmed, a full log or a reader replays) and prints, at every replay, which log entries fw_spin_steps
hands every single live index.  The dt of frame k is the number k, so an entry names its frame.  A brute-force Python model -- one list
of pending frames PER PARTICLE -- says what every line must be: exactly the frames the particle lived through, and was not integrated
in, since it was last current."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>
#include "fw_spin.h"
struct Cohort { uint32_t n; uint64_t spin_from; };
static size_t max_log = 0;
// what ensure_spin does: the table and the log in ONE block of exactly their size (the sanitizer build sees a lookup that leaves it),
// then, per live index, the entries the kernel's loop would run through
static void replay(FwSpinBook &book, std::deque<Cohort> &coh, unsigned frame) {
    if (!book.stale) return;
    const size_t log_n = book.log.size();
    std::vector<FwSpinEntry> tab(coh.size() + 1);
    uint64_t live = 0;
    const uint32_t n = book.table(coh, tab.data(), &live);
    char *blk = (char *)malloc(n * sizeof(FwSpinEntry) + log_n * sizeof(float) + 1);
    FwSpinEntry *t = (FwSpinEntry *)blk;
    float *log = (float *)(t + n);
    if (n) memcpy(t, tab.data(), n * sizeof(FwSpinEntry));
    for (size_t k = 0; k < log_n; k++) log[k] = book.log[k];
    printf("M %u %llu\n", frame, (unsigned long long)live);
    for (uint32_t i = 0; i < (uint32_t)live; i++) {
        uint32_t from = 0;
        const uint32_t steps = fw_spin_steps(t, n, (uint32_t)live, (uint32_t)log_n, i, &from);
        printf("%u", i);
        for (uint32_t e = from; e < from + steps; e++) printf(" %d", (int)log[e]);
        printf("\n");
    }
    uint32_t from = 0;
    if (fw_spin_steps(t, n, (uint32_t)live, (uint32_t)log_n, (uint32_t)live, &from) || fw_spin_steps(t, n, (uint32_t)live, (uint32_t)log_n, 0xFFFFFFFFu, &from) ||
        fw_spin_steps(t, 0, (uint32_t)live, (uint32_t)log_n, 0, &from))
        printf("BAD index past the ring\n");
    free(blk);
    book.current(coh);
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n_sched = 0;
    if (fscanf(f, "%u", &n_sched) != 1) return 2;
    for (unsigned s = 0; s < n_sched; s++) {
        unsigned cap = 0, n_ops = 0;
        if (fscanf(f, "%u %u", &cap, &n_ops) != 2) return 2;
        printf("S %u\n", s);
        FwSpinBook book;
        std::deque<Cohort> coh;
        unsigned frame = 0;
        for (unsigned o = 0; o < n_ops; o++) {
            char kind = 0;
            unsigned n_spawn = 0, n_dead = 0, push_empty = 0;
            if (fscanf(f, " %c %u %u %u", &kind, &n_spawn, &n_dead, &push_empty) != 4) return 2;
            if (kind == 'R') {  // a reader
                replay(book, coh, frame);
                continue;
            }
            frame++;
            const float dt = (float)frame;
            uint64_t from;
            if (kind == 'D') {  // a deferred launch (launch_fifo)
                if (fw_spin_full(book.log.size(), cap)) replay(book, coh, frame);
                from = book.defer(coh, dt);
            } else {  // a launch that does not defer
                replay(book, coh, frame);
                from = book.end();
            }
            if (n_spawn || push_empty) coh.push_back(Cohort{n_spawn, from});
            for (unsigned k = 0; k < n_dead && !coh.empty(); k++) coh.pop_front();
            if (book.stale) book.trim(coh);
            max_log = book.log.size() > max_log ? book.log.size() : max_log;
            if (book.log.size() > cap) printf("BAD log above its cap\n");
        }
        replay(book, coh, frame);
    }
    printf("max_log %zu\n", max_log);
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("spin")
    (d / "spin.cpp").write_text(PROGRAM)
    exe = d / "spin"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "spin.cpp"), "-o", str(exe)])
    return str(exe), d


class Model:
    """every particle by itself: the list of frames whose spin step it still lacks.  Cohorts exist only to know who dies together
    (and to carry the pending frames of a cohort without particles, which the log's trim looks at as well)."""

    def __init__(self, cap):
        self.cap, self.frame, self.stale = cap, 0, False
        self.cohorts = []  # oldest first: {"parts": [pending list per particle], "pend": pending list of the cohort itself}
        self.log = []      # frames logged and not trimmed
        self.out = []
        self.max_log = 0

    def replay(self):
        if not self.stale:
            return
        parts = [p for c in self.cohorts for p in c["parts"]]
        self.out.append(f"M {self.frame} {len(parts)}")
        for i, p in enumerate(parts):
            self.out.append(" ".join([str(i)] + [str(k) for k in p]))
            p.clear()
        for c in self.cohorts:
            c["pend"].clear()
        self.log, self.stale = [], False

    def op(self, kind, n_spawn, n_dead, push_empty):
        if kind == "R":
            self.replay()
            return
        self.frame += 1
        if kind == "D":
            if len(self.log) + 1 > self.cap:
                self.replay()
            self.stale = True
            self.log.append(self.frame)
            for c in self.cohorts:  # everybody who is here lacks this frame's step ...
                c["pend"].append(self.frame)
                for p in c["parts"]:
                    p.append(self.frame)
        else:
            self.replay()
        if n_spawn or push_empty:  # ... the particles the frame spawns got it from the launch itself
            self.cohorts.append({"parts": [[] for _ in range(n_spawn)], "pend": []})
        del self.cohorts[:n_dead]
        if self.stale:  # the trim: a logged frame stays while somebody in the ring lacks it
            lacking = {k for c in self.cohorts for k in c["pend"]}
            self.log = [k for k in self.log if k in lacking]
        self.max_log = max(self.max_log, len(self.log))


def _run(program, schedules, name):
    exe, d = program
    lines = [str(len(schedules))]
    want = []
    max_log = 0
    for s, (cap, ops) in enumerate(schedules):
        lines.append(f"{cap} {len(ops)}")
        lines += [f"{k} {a} {b} {c}" for k, a, b, c in ops]
        m = Model(cap)
        for o in ops:
            m.op(*o)
        m.replay()
        want += [f"S {s}"] + m.out
        max_log = max(max_log, m.max_log)
        assert m.max_log <= cap
    want.append(f"max_log {max_log}")
    path = d / (name + ".txt")
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.strip().splitlines()
    assert not [ln for ln in got if ln.startswith("BAD")]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k, g, w)
    return max_log


def _random_schedule(rng, cap, n_ops, p_defer, p_read, life):
    ops = []
    for _ in range(n_ops):
        u = rng.random()
        if u < p_read:
            ops.append(("R", 0, 0, 0))
            continue
        kind = "D" if rng.random() < p_defer else "U"
        n_spawn = int(rng.integers(0, 6)) if rng.random() < 0.8 else 0
        push_empty = int(n_spawn == 0 and rng.random() < 0.5)
        # cohorts die roughly `life` frames after they came, sometimes two at once, sometimes none for a while
        n_dead = int(rng.random() < 1.0 / max(1.0, life) * 3.0) * int(rng.integers(1, 3)) if len(ops) > life else 0
        ops.append((kind, n_spawn, n_dead, push_empty))
    return cap, ops


def test_random_schedules(program):
    """3000 schedules: deferred stretches of every length, launches that do not defer, readers, cohorts that die unread (alone and in
    pairs), frames that spawn nothing, cohorts without particles, caps from 1 to 16"""
    rng = np.random.default_rng(19)
    schedules = []
    for k in range(3000):
        schedules.append(_random_schedule(rng, cap=int(rng.integers(1, 17)), n_ops=int(rng.integers(1, 40)), p_defer=float(rng.choice([0.5, 0.9, 1.0])),
                                          p_read=float(rng.choice([0.0, 0.05, 0.3])), life=float(rng.choice([1.5, 4.0, 12.0]))))
    _run(program, schedules, "random")


def test_ring_drains_and_fills_again(program):
    """every cohort dies inside a stretch (the log is trimmed to nothing while the ring stays deferred), then the ring fills again"""
    ops = [("D", 3, 0, 0)] * 4 + [("D", 0, 2, 0)] * 2 + [("D", 0, 0, 0)] * 3 + [("D", 2, 0, 0)] * 3 + [("R", 0, 0, 0)] + [("D", 1, 1, 0)] * 5
    assert _run(program, [(64, ops)], "drain") >= 3


def test_empty_cohorts_and_an_empty_ring(program):
    """cohorts without particles between cohorts with some (no table entry; the trim still honours their pointer), a stretch over a
    ring that never held a particle, a reader with nothing stale"""
    a = [("D", 2, 0, 0), ("D", 0, 0, 1), ("D", 0, 0, 1), ("D", 3, 0, 0), ("D", 0, 1, 1), ("D", 1, 0, 0), ("R", 0, 0, 0), ("R", 0, 0, 0)]
    b = [("D", 0, 0, 0)] * 5 + [("R", 0, 0, 0)]
    c = [("D", 0, 0, 1)] * 5 + [("U", 2, 0, 0), ("R", 0, 0, 0)]
    _run(program, [(8, a), (8, b), (8, c)], "hollow")


def test_log_at_its_cap(program):
    """a ring nobody reads whose particles live longer than the cap: replayed every `cap` frames, never a log above it; the same ring
    with lifetimes below the cap never replays before its reader"""
    long_lived = [("D", 2, 0, 0)] * 40
    short_lived = [("D", 2, 0, 0)] * 3 + [("D", 2, 1, 0)] * 37
    assert _run(program, [(4, long_lived)], "cap_long") == 4
    assert _run(program, [(4, short_lived)], "cap_short") <= 4
    assert _run(program, [(1, long_lived)], "cap_one") == 1
