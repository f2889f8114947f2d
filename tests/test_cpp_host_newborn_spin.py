"""The spin pointer of the cohort a deferring launch spawns, without a GPU (csrc/fw_spin.h: fw_spin_newborn_deferred, FwSpinBook::
defer_spawn; round 27).  A stand-alone C++ program, compiled here with g++ -- once plainly, once with -fsanitize=address,undefined --,
drives FwSpinBook the way launch_fifo (ring_rules, age_cohorts), group_launched and ensure_spin do, over random hosts: deferring launches and stretches that end and
begin again, frames withheld into groups of depth 1 to FW_FUSE_MAX that close by depth or are flushed early (by a reader, a launch that
does not defer, a full log), cohorts that die and trim the log, a small log cap, frames whose ring falls back to the eager rule (somebody
else writes its new particles), and whole hosts under the switch (FW_NEWBORN_SPIN=1).

What is checked, per live particle and at every replay: the log entries the table assigns it (fw_spin_steps) are exactly the frames whose
spin step no launch gave it, kept by a brute force PER PARTICLE inside the program.  Under the rule that is every deferring frame the
particle has lived through since it was last current, its birth frame included; under the eager rule the birth frame is the launch's --
and so is every later frame of the group the birth frame was withheld into: one entry fewer for a frame that went out alone.  The dt of
frame k is the number k, so an entry names its frame.  A Python model of the same hosts counts the same totals on its own."""
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
#include "fw_fuse2.h"
struct Cohort {
    uint32_t n;
    uint64_t spin_from;
    unsigned frame;
    std::vector<std::vector<int>> lacks;  // the brute force: per particle, the frames whose spin step nobody gave it
};
struct Host {
    FwSpinBook book;
    std::deque<Cohort> coh;
    unsigned frame = 0;
    bool eager = false;  // FW_NEWBORN_SPIN=1
    // the withheld frames of the group so far (fw_ctx::withheld): their numbers, and the pointer a cohort of the last one carries
    unsigned held[FW_FUSE_MAX] = {}, depth = 0;
    uint64_t held_from = 0;
    unsigned long long total = 0;
};
// group_launched: the group goes to the stream.  Under the eager rule the launch spins the newborns of every withheld frame through
// every later frame of the group: their pointer is the last frame's, and the brute force drops those frames
static void launch_group(Host &h) {
    if (!h.depth) return;
    const unsigned last = h.held[h.depth - 1];
    if (h.eager)
        for (auto &c : h.coh)
            for (unsigned f = 0; f + 1 < h.depth; f++)
                if (c.frame == h.held[f]) {
                    c.spin_from = h.held_from;
                    for (auto &p : c.lacks) {
                        std::vector<int> keep;
                        for (int k : p)
                            if ((unsigned)k > last) keep.push_back(k);
                        p = keep;
                    }
                }
    h.depth = 0;
}
// ensure_spin: whoever is withheld goes out first; then the table and the log in ONE block of exactly their size, and per live index
// the entries the kernel's loop would run through against the brute force
static void replay(Host &h) {
    launch_group(h);
    if (!h.book.stale) return;
    const size_t log_n = h.book.log.size();
    std::vector<FwSpinEntry> tab(h.coh.size() + 1);
    uint64_t live = 0;
    const uint32_t n = h.book.table(h.coh, tab.data(), &live);
    char *blk = (char *)malloc(n * sizeof(FwSpinEntry) + log_n * sizeof(float) + 1);
    FwSpinEntry *t = (FwSpinEntry *)blk;
    float *log = (float *)(t + n);
    if (n) memcpy(t, tab.data(), n * sizeof(FwSpinEntry));
    for (size_t k = 0; k < log_n; k++) log[k] = h.book.log[k];
    unsigned long long steps_all = 0;
    uint32_t i = 0;
    for (auto &c : h.coh)
        for (auto &p : c.lacks) {
            uint32_t from = 0;
            const uint32_t steps = fw_spin_steps(t, n, (uint32_t)live, (uint32_t)log_n, i, &from);
            bool same = steps == p.size();
            for (uint32_t e = 0; same && e < steps; e++) same = (int)log[from + e] == p[e];
            if (!same) printf("BAD frame %u particle %u born %u: the table says %u entries, the brute force %zu\n", h.frame, i, c.frame, steps, p.size());
            steps_all += steps;
            p.clear();
            i++;
        }
    if ((uint64_t)i != live) printf("BAD live count\n");
    printf("M %u %llu %llu\n", h.frame, (unsigned long long)live, steps_all);
    h.total += steps_all;
    free(blk);
    h.book.current(h.coh);
}
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned n_sched = 0;
    if (fscanf(f, "%u", &n_sched) != 1) return 2;
    for (unsigned s = 0; s < n_sched; s++) {
        unsigned cap = 0, n_ops = 0, eager = 0, dmax = 0;
        if (fscanf(f, "%u %u %u %u", &cap, &eager, &dmax, &n_ops) != 4 || dmax < 1 || dmax > FW_FUSE_MAX) return 2;
        printf("S %u\n", s);
        Host h;
        h.eager = eager != 0;
        for (unsigned o = 0; o < n_ops; o++) {
            char kind = 0;
            unsigned n_spawn = 0, n_dead = 0, hold = 0;
            if (fscanf(f, " %c %u %u %u", &kind, &n_spawn, &n_dead, &hold) != 4) return 2;
            if (kind == 'R') {  // a reader
                replay(h);
                continue;
            }
            h.frame++;
            const float dt = (float)h.frame;
            // 'D': a deferring launch that spawns for itself; 'F': a deferring launch of a ring somebody else writes the newborns of
            // (the eager rule for this frame, decided when the cohort is pushed; such a frame is never withheld); 'U': no deferral
            const bool deferring = kind == 'D' || kind == 'F';
            const bool rule = fw_spin_newborn_deferred(deferring, kind == 'D', h.eager);
            if (kind != 'D' || !hold) launch_group(h);  // (a frame that is no candidate flushes whoever waits)
            uint64_t from;
            if (deferring) {
                if (fw_spin_full(h.book.log.size(), cap)) replay(h);
                from = h.book.defer_spawn(h.coh, dt, rule);
                if (from != (rule ? h.book.end() - 1u : h.book.end())) printf("BAD pointer\n");
                for (auto &c : h.coh)
                    for (auto &p : c.lacks) p.push_back((int)h.frame);
            } else {
                replay(h);
                from = h.book.end();
            }
            if (n_spawn) {
                Cohort c{n_spawn, from, h.frame, {}};
                c.lacks.assign(n_spawn, rule ? std::vector<int>{(int)h.frame} : std::vector<int>{});
                h.coh.push_back(c);
            }
            for (unsigned k = 0; k < n_dead && !h.coh.empty(); k++) h.coh.pop_front();
            if (h.book.stale) h.book.trim(h.coh);
            if (h.book.log.size() > cap) printf("BAD log above its cap\n");
            // the newest entry is the one a newborn under the rule points at: the trim never takes it while the cohort lives
            if (n_spawn && rule && !h.coh.empty() && (h.book.log.empty() || h.book.log.back() != dt)) printf("BAD the newborn's entry was trimmed\n");
            if (kind == 'D' && hold) {  // withheld, or the frame that completes the group
                h.held[h.depth++] = h.frame, h.held_from = from;
                if (h.depth >= dmax) launch_group(h);
            } else if (deferring) {
                h.held[0] = h.frame, h.depth = 1, h.held_from = from;
                launch_group(h);
            }
        }
        replay(h);
        printf("T %llu\n", h.total);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("newborn_spin")
    (d / "newborn_spin.cpp").write_text(PROGRAM)
    exe = d / "newborn_spin"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I", CSRC] + flags + [str(d / "newborn_spin.cpp"), "-o", str(exe)])
    return str(exe), d


class Model:
    """counts, not lists: per cohort the number of steps each of its particles lacks (they are born together and treated alike), written
    from the rule's wording and not from the table's arithmetic"""

    def __init__(self, cap, eager, dmax):
        self.cap, self.eager, self.dmax = cap, bool(eager), dmax
        self.frame, self.stale, self.log = 0, False, 0
        self.cohorts = []  # oldest first: [n, frames lacked (a list), birth frame]
        self.held = []
        self.out, self.total = [], 0

    def launch_group(self):
        if self.held and self.eager:
            last = self.held[-1]
            for c in self.cohorts:
                if c[2] in self.held[:-1]:
                    c[1] = [k for k in c[1] if k > last]
        self.held = []

    def replay(self):
        self.launch_group()
        if not self.stale:
            return
        steps = sum(c[0] * len(c[1]) for c in self.cohorts)
        self.out.append(f"M {self.frame} {sum(c[0] for c in self.cohorts)} {steps}")
        self.total += steps
        for c in self.cohorts:
            c[1] = []
        self.stale, self.log = False, 0

    def op(self, kind, n_spawn, n_dead, hold):
        if kind == "R":
            self.replay()
            return
        self.frame += 1
        deferring = kind in "DF"
        rule = kind == "D" and not self.eager
        if kind != "D" or not hold:
            self.launch_group()
        if deferring:
            if self.stale and self.log + 1 > self.cap:
                self.replay()
            self.stale = True
            self.log += 1
            for c in self.cohorts:
                c[1].append(self.frame)
        else:
            self.replay()
        if n_spawn:
            self.cohorts.append([n_spawn, [self.frame] if rule else [], self.frame])
        del self.cohorts[:n_dead]
        if self.stale:  # the trim: as many entries as the neediest cohort lacks (none left: none)
            self.log = max((len(c[1]) for c in self.cohorts), default=0)
        if kind == "D" and hold:
            self.held.append(self.frame)
            if len(self.held) >= self.dmax:
                self.launch_group()
        elif deferring:
            self.held = [self.frame]
            self.launch_group()


def _run(program, schedules, name):
    exe, d = program
    lines = [str(len(schedules))]
    want = []
    for s, (cap, eager, dmax, ops) in enumerate(schedules):
        lines.append(f"{cap} {int(eager)} {dmax} {len(ops)}")
        lines += [f"{k} {a} {b} {c}" for k, a, b, c in ops]
        m = Model(cap, eager, dmax)
        for o in ops:
            m.op(*o)
        m.replay()
        want += [f"S {s}"] + m.out + [f"T {m.total}"]
    path = d / (name + ".txt")
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.strip().splitlines()
    assert not [ln for ln in got if ln.startswith("BAD")], [ln for ln in got if ln.startswith("BAD")][:5]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k, g, w)
    return [int(ln.split()[1]) for ln in got if ln.startswith("T ")]


def _random_host(rng, cap, eager, dmax, n_ops, p_defer, p_read, p_fallback, p_hold, life):
    ops = []
    for _ in range(n_ops):
        if rng.random() < p_read:
            ops.append(("R", 0, 0, 0))
            continue
        kind = ("F" if rng.random() < p_fallback else "D") if rng.random() < p_defer else "U"
        n_spawn = int(rng.integers(1, 6)) if rng.random() < 0.85 else 0
        n_dead = int(rng.random() < 3.0 / max(1.0, life)) * int(rng.integers(1, 3)) if len(ops) > life else 0
        ops.append((kind, n_spawn, n_dead, int(kind == "D" and dmax > 1 and rng.random() < p_hold)))
    return cap, eager, dmax, ops


def test_random_hosts(program):
    """3000 hosts: stretches of every length that end and begin again, groups of depth 1 to 8 closed by depth or flushed early, readers,
    cohorts that die unread, frames that spawn nothing, log caps from 1 to 16, frames that fall back to the eager rule, and a third of the
    hosts under the switch"""
    rng = np.random.default_rng(27)
    hosts = []
    for k in range(3000):
        hosts.append(_random_host(rng, cap=int(rng.integers(1, 17)), eager=k % 3 == 2, dmax=int(rng.integers(1, 9)), n_ops=int(rng.integers(1, 60)),
                                  p_defer=float(rng.choice([0.6, 0.9, 1.0])), p_read=float(rng.choice([0.0, 0.05, 0.25])),
                                  p_fallback=float(rng.choice([0.0, 0.0, 0.2])), p_hold=float(rng.choice([0.5, 0.9, 1.0])),
                                  life=float(rng.choice([1.5, 4.0, 12.0, 40.0]))))
    _run(program, hosts, "random")


@pytest.mark.parametrize("depth", [1, 2, 4, 8])
def test_one_entry_more_than_the_eager_rule(program, depth):
    """twenty deferring frames of three newborns each, nobody dies, groups of one depth: under the rule a particle born in frame b lacks
    frames b .. 20; under the eager rule frames behind the group its birth frame went out in.  Unfused that is exactly one entry fewer
    per particle"""
    ops = [("D", 3, 0, 1)] * 20
    rule, = _run(program, [(64, False, depth, ops)], f"more_{depth}")
    eager, = _run(program, [(64, True, depth, ops)], f"more_eager_{depth}")
    assert rule == 3 * sum(20 - b + 1 for b in range(1, 21))
    # (frame b goes out with the group that ends at frame e(b) = the next multiple of the depth)
    assert eager == 3 * sum(20 - min(20, -(-b // depth) * depth) for b in range(1, 21))
    if depth == 1:
        assert rule - eager == 3 * 20


def test_a_reader_arrives_with_frames_withheld(program):
    """groups of eight flushed by a reader at every depth from 1 to 7, then a stretch that begins again"""
    ops = []
    for held in range(1, 8):
        ops += [("D", 2, 0, 1)] * held + [("R", 0, 0, 0)]
    ops += [("U", 2, 0, 0)] + [("D", 2, 1, 1)] * 9
    _run(program, [(64, False, 8, ops), (64, True, 8, ops)], "reader")


def test_small_cap_and_dying_cohorts(program):
    """a cap of three with groups of four: the log fills inside a group (the group is flushed, the log replayed, the ring goes on
    deferring); cohorts born under the rule die under it and the trim follows them"""
    ops = [("D", 2, 0, 1)] * 10 + [("D", 2, 1, 1)] * 30
    _run(program, [(3, False, 4, ops), (3, True, 4, ops), (1, False, 8, ops), (2, False, 2, ops)], "cap")


def test_fallback_frames_keep_the_eager_pointer(program):
    """a ring whose new particles somebody else writes in some frames: those cohorts point at the next entry whatever the switch says"""
    ops = [("D", 2, 0, 0), ("F", 2, 0, 0), ("D", 2, 0, 1), ("D", 2, 0, 1), ("F", 3, 0, 0), ("D", 1, 0, 1), ("R", 0, 0, 0)]
    t, = _run(program, [(64, False, 4, ops)], "fallback")
    # births at frames 1..6, read after frame 6: rule frames lack 6 - b + 1, fallback frames 6 - b
    assert t == 2 * 6 + 2 * 4 + 2 * 4 + 2 * 3 + 3 * 1 + 1 * 1
