"""The update-path rule and the census of segments by path without a GPU (csrc/fw_update_path.h: fw_choose_path, fw_type_facts,
FwPathCensus; the lines build_spawner, fifo_may_become_range and SegPathEdit compile).  A stand-alone C++ program with its
own main does three things.
The rule: beside fw_choose_path it keeps a model in its own words -- the clauses build_spawner held before the rule had a header of its own,
as straight-line booleans -- and compares every output field over a grid: every combination of the seven boolean facts; seven lifetimes
(one value, a range, min > max, infinite, NaN, a range and a single value whose life_lo_safe is not positive); 0, 1, 8 and 9 Global
feeders; 0 to 3 last_emitted_age planes; capacities one below, at and one above fifo_min, 8 fifo_min, range_min, 32 range_min,
fifo_small_tiles FW_TILE, FW_RANGE_MAX_CAPACITY and 2^30; censuses with n_in_use at and one past range_few, n_fifo 0, 1, kMaxFifoSegs - 1
and kMaxFifoSegs, n_spilled 0 and 1, few_blocked both ways; the product's default policy, each of its switches flipped alone, the two
rules that have no switch set to 0, and one policy with the thresholds of the GPU tests (at the defaults 8 fifo_min == 32 range_min, and
the two clauses of the few-nested exception could hide behind each other).  The run fails unless every outcome occurred: a FIFO ring with
and without Q0 in planes, materialised and device-counted ones, a range ring by size, as a few-ring, by the few-nested exception, a
spilled one, a spill that ends on the compacting path, and the compacting path for each single reason that alone sends a type there.
fw_type_facts is held against the three loops over the emission entries it replaces, on random descriptors.
The census: an FwPathCensus is driven through random sequences of add, flag edits (remove + add) and remove over up to 300 segments from
fixed seeds and compared with FwPathCensus::recount after every operation; the hysteresis is walked both ways with range_few = 5 -- blocked
at the sixth segment, still blocked at four, free at two (the numbers of tests/test_gpu_range.py's few-rings test), and blocked by a FIFO
ring that meets a few-ring --; a remove of bits that were never added must be refused and leave every count as it was.
Compiled host-side by the Makefile's hipcc as plain C++ (-x c++: fw_kernels.h does not compile alone under g++ -Wall -Werror) -- once
plainly, once with -fsanitize=address,undefined -- and run directly: nothing is loaded into Python, nothing is preloaded."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_firework_amd", "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fw_update_path.h"
static_assert(FW_INLINE_OPS == 8 && FW_FIFO_PER_LAUNCH == 8 && FW_RANGE_MAX_CAPACITY == 0x10000000u, "the limits this program's model spells out");
static uint64_t rng;
static uint32_t rnd(uint32_t n) {  // 0 .. n - 1 (xorshift64*)
    rng ^= rng >> 12, rng ^= rng << 25, rng ^= rng >> 27;
    return (uint32_t)(((rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static unsigned long long n_bad;
static void bad(const char *what, long long x = 0, long long y = 0) {
    if (n_bad++ < 30) printf("BAD %s (%lld, %lld)\n", what, x, y);
}
#define CHECK(cond, ...) do { if (!(cond)) bad(__VA_ARGS__); } while (0)

// ---- the model: the clauses of the segment loop, one after the other, as the loop held them
struct Model {
    bool fifo, range, few_ring, spilled, fifo_mat, fifo_dev, range_mat, range_dev, q0pl, win_ok;
    bool few_nested, spill;             // (how it got there)
    int range_failed, range_which;      // conjuncts of the range clause that are false, and the last of them
    bool life_not_finite;
};
enum { R_USE_RANGE, R_NO_RINGS, R_SELF_NESTED, R_MIXED_FEED, R_LPLANES, R_COLLISION, R_LIFETIME, R_SIZE, R_MAX_CAPACITY, R_N };
static Model model(const FwPathPolicy &P, const FwPathCensus &C, const FwTypeFacts &F) {
    Model m{};
    const double life_bound = (double)std::max(F.life_min, F.life_max);
    m.win_ok = !F.nested_fed && std::isfinite(life_bound);
    m.fifo = P.use_fifo && !F.no_rings && !F.self_nested && !F.mixed_feed && (!F.collides || F.coll_inplace) && F.life_min == F.life_max &&
             F.n_global_feed <= 8u && std::isfinite(F.life_min) && F.capacity >= P.fifo_min && F.capacity < 0x40000000u && (!F.any_nested || P.fifo_nested);
    m.spill = m.fifo && (C.n_spilled != 0 || C.n_fifo >= 8u);
    if (m.spill) m.fifo = false;
    if (m.fifo && F.nested_fed && P.use_range && P.range_few != 0 && !C.few_blocked && C.n_in_use <= P.range_few && C.n_fifo == 0 &&
        F.capacity < 8u * P.fifo_min && F.capacity < P.range_min * 32u && F.n_lplanes <= 2 && F.life_lo_safe > 0.0f && F.capacity <= 0x10000000u)
        m.fifo = false, m.few_nested = true;
    if (m.fifo) {
        m.win_ok = false;
        m.fifo_mat = F.any_nested;
        m.fifo_dev = F.nested_fed;
        m.q0pl = P.use_ageless && P.fifo_small_tiles != 0u && !F.any_nested && !F.nested_fed && F.n_lplanes == 0 && !F.collides &&
                 (uint64_t)F.capacity >= (uint64_t)P.fifo_small_tiles * FW_TILE;
    }
    m.life_not_finite = !(std::isfinite(F.life_min) && std::isfinite(F.life_max));
    const bool conj[R_N] = {
        P.use_range,
        !F.no_rings,
        !F.self_nested,
        !F.mixed_feed,
        F.n_lplanes <= 2,
        !F.collides || F.coll_inplace,
        std::isfinite(F.life_min) && std::isfinite(F.life_max) && F.life_lo_safe > 0.0f,
        F.capacity >= P.range_min || (P.range_few != 0 && !C.few_blocked && C.n_in_use <= P.range_few && C.n_fifo == 0),
        F.capacity <= 0x10000000u,
    };
    m.range = !m.fifo;
    for (int k = 0; k < R_N; k++) {
        m.range = m.range && conj[k];
        if (!conj[k]) m.range_failed++, m.range_which = k;
    }
    if (m.range) {
        if (F.capacity < P.range_min || m.few_nested) m.few_ring = true;
        if (m.spill) m.spilled = true;
        m.range_mat = F.n_lplanes != 0;
        m.range_dev = F.nested_fed;
        if (m.range_dev) m.win_ok = false;
    }
    return m;
}

static unsigned long long n_cases, n_fifo_q0pl, n_fifo_float4, n_fifo_mat, n_fifo_dev, n_range_by_size, n_range_few_ring, n_few_nested, n_spilled, n_spill_compacting,
    n_compact_alone[R_N], n_compact_life_not_finite, n_compact_life_lo_safe;

static void rule_grid() {
    std::vector<FwPathPolicy> policies;
    {
        const FwPathPolicy def;
        policies.push_back(def);
        FwPathPolicy p;
        p = def, p.use_fifo = false, policies.push_back(p);
        p = def, p.fifo_nested = false, policies.push_back(p);
        p = def, p.use_ageless = false, policies.push_back(p);
        p = def, p.use_range = false, policies.push_back(p);
        p = def, p.range_few = 0u, policies.push_back(p);
        p = def, p.fifo_small_tiles = 0u, policies.push_back(p);
        p = def, p.fifo_min = 2048u, p.range_min = 4096u, p.range_few = 5u, p.fifo_small_tiles = 2u, policies.push_back(p);  // (the GPU tests' kind of thresholds)
    }
    const float inf = INFINITY, nan = NAN;
    const float lifetimes[7][2] = {{1.0f, 1.0f}, {0.5f, 2.0f}, {2.0f, 0.5f}, {inf, inf}, {nan, nan}, {0.0f, 1.0f}, {0.0f, 0.0f}};
    const uint32_t feeds[4] = {0u, 1u, 8u, 9u};
    for (const FwPathPolicy &P : policies) {
        std::vector<uint32_t> caps;
        const uint64_t thresholds[7] = {P.fifo_min, 8ull * P.fifo_min, P.range_min, 32ull * P.range_min, (uint64_t)P.fifo_small_tiles * FW_TILE, FW_RANGE_MAX_CAPACITY, 1ull << 30};
        for (uint64_t thr : thresholds)
            for (int d = -1; d <= 1; d++)
                if (thr + d >= 1u && thr + d <= 0xFFFFFFFFull) caps.push_back((uint32_t)(thr + d));
        std::vector<FwPathCensus> censuses;
        for (uint32_t over = 0; over < 2; over++)
            for (uint32_t nf : {0u, 1u, (uint32_t)FW_FIFO_PER_LAUNCH - 1u, (uint32_t)FW_FIFO_PER_LAUNCH})
                for (uint32_t ns = 0; ns < 2; ns++)
                    for (int blocked = 0; blocked < 2; blocked++) {
                        // (the rule is a function of these four words alone; n_in_use counts the type being built)
                        FwPathCensus C;
                        C.n_in_use = P.range_few + over, C.n_fifo = nf, C.n_spilled = ns, C.n_range = ns, C.few_blocked = blocked != 0;
                        censuses.push_back(C);
                    }
        for (uint32_t b = 0; b < 128u; b++)
            for (const auto &life : lifetimes)
                for (uint32_t feed : feeds)
                    for (uint32_t lp = 0; lp < 4u; lp++)
                        for (uint32_t cap : caps) {
                            FwTypeFacts F;
                            F.collides = b & 1u, F.coll_inplace = b & 2u, F.nested_fed = b & 4u, F.any_nested = b & 8u, F.self_nested = b & 16u, F.mixed_feed = b & 32u,
                            F.no_rings = b & 64u;
                            F.life_min = life[0], F.life_max = life[1], F.life_lo_safe = fw_life_lo_safe(life[0], life[1]);
                            F.n_global_feed = feed, F.n_feeders = feed + (F.nested_fed ? 1u : 0u), F.n_lplanes = lp, F.capacity = cap;
                            for (const FwPathCensus &C : censuses) {
                                const FwPathChoice r = fw_choose_path(P, C, F);
                                const Model m = model(P, C, F);
                                n_cases++;
                                if (r.fifo != m.fifo || r.range != m.range || r.few_ring != m.few_ring || r.spilled != m.spilled || r.fifo_mat != m.fifo_mat ||
                                    r.fifo_dev != m.fifo_dev || r.range_mat != m.range_mat || r.range_dev != m.range_dev || r.q0pl != m.q0pl || r.win_ok != m.win_ok)
                                    bad("fw_choose_path differs from the model", (long long)b, (long long)cap);
                                CHECK(!(m.fifo && m.range), "one path at most");
                                n_fifo_q0pl += m.fifo && m.q0pl, n_fifo_float4 += m.fifo && !m.q0pl, n_fifo_mat += m.fifo && m.fifo_mat, n_fifo_dev += m.fifo && m.fifo_dev;
                                n_range_by_size += m.range && !m.few_ring && !m.spilled, n_range_few_ring += m.range && m.few_ring && !m.few_nested;
                                n_few_nested += m.few_nested && m.range, n_spilled += m.range && m.spilled, n_spill_compacting += m.spill && !m.range;
                                CHECK(!m.few_nested || (m.range && m.few_ring), "the few-nested exception does qualify for a range ring");
                                if (!m.fifo && !m.range && m.range_failed == 1) {
                                    n_compact_alone[m.range_which]++;
                                    if (m.range_which == R_LIFETIME) (m.life_not_finite ? n_compact_life_not_finite : n_compact_life_lo_safe)++;
                                }
                            }
                        }
    }
}

// ---- fw_type_facts against the loops over the emission entries it replaces
static void facts_of_random_descriptors(uint32_t rounds) {
    rng = 0x1234567ull;
    for (uint32_t round = 0; round < rounds; round++) {
        const uint32_t nt = 1u + rnd(4), ne = rnd(7);
        std::vector<fw_particle_settings> ps(nt);
        std::vector<fw_emission_settings> es(ne);
        memset(ps.data(), 0, nt * sizeof ps[0]);
        if (ne) memset(es.data(), 0, ne * sizeof es[0]);
        for (auto &p : ps) {
            p.lifetime.min = (float)rnd(4), p.lifetime.max = rnd(3) ? p.lifetime.min : (float)rnd(4);
            p.collision.enabled = rnd(3) == 0u, p.collision.destroy_on_collision = rnd(2);
        }
        for (auto &e : es) e.particle_index = (int32_t)rnd(nt), e.mode = rnd(2) ? FW_MODE_GLOBAL : FW_MODE_NESTED, e.target_particle_type = (int32_t)rnd(nt);
        fw_spawner_desc d{};
        d.particle_settings = ps.data(), d.n_particle_settings = nt, d.emission_settings = es.data(), d.n_emission_settings = ne;
        for (uint32_t t = 0; t < nt; t++) {
            const bool bigkeys = rnd(4) == 0u, no_rings = rnd(4) == 0u;
            const uint32_t cap = 1u + rnd(100000);
            const FwTypeFacts f = fw_type_facts(&d, t, cap, bigkeys, no_rings);
            uint32_t n_lplanes = 0, feeders = 0, global_feeders = 0;
            bool nested_fed = false;
            for (uint32_t i = 0; i < ne; i++) {
                if (es[i].mode == FW_MODE_NESTED && (uint32_t)es[i].target_particle_type == t) n_lplanes++;
                if (es[i].mode == FW_MODE_NESTED && (uint32_t)es[i].particle_index == t) nested_fed = true;
            }
            bool any_nested = false, self_nested = false, mixed_feed = false;
            uint32_t n_global_feed = 0;
            for (uint32_t i = 0; i < ne; i++) {
                n_global_feed += (es[i].mode == FW_MODE_GLOBAL && (uint32_t)es[i].particle_index == t) ? 1u : 0u;
                any_nested |= es[i].mode == FW_MODE_NESTED;
                self_nested |= es[i].mode == FW_MODE_NESTED && es[i].target_particle_type == es[i].particle_index;
                mixed_feed |= nested_fed && es[i].mode == FW_MODE_GLOBAL && (uint32_t)es[i].particle_index == t;
            }
            for (uint32_t i = 0; i < ne; i++)
                if ((uint32_t)es[i].particle_index == t) feeders++, global_feeders += es[i].mode == FW_MODE_GLOBAL ? 1u : 0u;
            const fw_particle_settings &p = ps[t];
            const float lls = std::nextafterf(std::nextafterf(std::min(p.lifetime.min, p.lifetime.max), -INFINITY), -INFINITY);
            CHECK(f.capacity == cap && f.no_rings == no_rings && f.life_min == p.lifetime.min && f.life_max == p.lifetime.max && f.life_lo_safe == lls, "facts: the type's own");
            CHECK(f.collides == (p.collision.enabled != 0 || bigkeys) && f.coll_inplace == (p.collision.enabled != 0 && p.collision.destroy_on_collision == 0 && !bigkeys),
                  "facts: collisions");
            CHECK(f.n_lplanes == n_lplanes && f.nested_fed == nested_fed && f.n_global_feed == n_global_feed && f.any_nested == any_nested && f.self_nested == self_nested &&
                  f.mixed_feed == mixed_feed, "facts: the feed", round, t);
            CHECK((f.n_feeders == 1 && f.n_global_feed == 1) == (feeders == 1 && global_feeders == 1), "facts: one feeder", round, t);
        }
    }
    CHECK(std::isnan(fw_life_lo_safe(INFINITY, 1.0f)) && std::isnan(fw_life_lo_safe(1.0f, NAN)), "life_lo_safe of a range that is not finite");
}

// ---- the census
static unsigned long long n_census_ops;
static void census_random(uint64_t seed, uint32_t ops) {
    rng = seed * 0x9E3779B97F4A7C15ull + 1u;
    FwPathCensus C;
    std::vector<uint32_t> bits;
    const bool blocked = seed & 1u;
    C.few_blocked = blocked;
    for (uint32_t op = 0; op < ops; op++, n_census_ops++) {
        const uint32_t what = rnd(10);
        if ((what < 4u && bits.size() < 300u) || bits.empty()) {
            bits.push_back(FW_PATH_IN_USE | rnd(1024));
            C.add(bits.back());
        } else if (what < 8u) {  // a flag edit: out with the old bits, in with the new
            uint32_t &b = bits[rnd((uint32_t)bits.size())];
            CHECK(C.remove(b), "remove of bits that are in", b);
            b = rnd(8) ? b ^ (1u << rnd(10)) : rnd(1024);
            C.add(b);
        } else {
            const uint32_t k = rnd((uint32_t)bits.size());
            CHECK(C.remove(bits[k]), "remove of a segment that is in", bits[k]);
            bits[k] = bits.back(), bits.pop_back();
        }
        CHECK(C == FwPathCensus::recount(bits.data(), bits.size(), blocked), "the census is its recount", (long long)seed, op);
    }
    for (uint32_t b : bits) CHECK(C.remove(b), "the last removes");
    CHECK(C == FwPathCensus::recount(nullptr, 0, blocked), "empty at the end");
}

static void census_hysteresis() {
    const uint32_t few = 5u;
    FwPathCensus C;
    for (uint32_t n = 1; n <= 6u; n++) {
        C.add(FW_PATH_IN_USE);
        const bool drop = C.spawner_built(few);
        CHECK(!drop, "no few-ring: nothing to drop", n);
        CHECK(C.few_blocked == (n >= 6u), "blocked at the sixth segment", n, C.few_blocked);
    }
    for (uint32_t left = 6u; left-- > 0u;) {  // 5, 4, .. 0 segments left
        CHECK(C.remove(FW_PATH_IN_USE), "release");
        C.segment_released(few);
        CHECK(C.few_blocked == (left > 2u), "still blocked at four, free at two", left, C.few_blocked);
    }
    // a few-ring, then a sixth segment: the small rings leave
    FwPathCensus D;
    D.add(FW_PATH_IN_USE | FW_PATH_RANGE | FW_PATH_FEW_RING);
    CHECK(!D.spawner_built(few) && !D.few_blocked, "a few-ring alone stays");
    for (uint32_t n = 2; n <= 6u; n++) D.add(FW_PATH_IN_USE);
    CHECK(D.spawner_built(few) && D.few_blocked, "past range_few with a few-ring: drop");
    // a FIFO ring meets a few-ring: blocked as well, whatever the number of segments
    FwPathCensus E;
    E.add(FW_PATH_IN_USE | FW_PATH_RANGE | FW_PATH_FEW_RING);
    E.add(FW_PATH_IN_USE | FW_PATH_FIFO);
    CHECK(E.spawner_built(few) && E.few_blocked, "a FIFO ring meets a few-ring: drop");
    FwPathCensus G;  // ... but a FIFO ring alone blocks nothing
    G.add(FW_PATH_IN_USE | FW_PATH_FIFO);
    CHECK(!G.spawner_built(few) && !G.few_blocked, "a FIFO ring alone");
}

static void census_refuses() {
    FwPathCensus C;
    const FwPathCensus empty;
    for (uint32_t k = 0; k < 10u; k++) {
        const uint32_t b = 1u << k;
        if (b == FW_PATH_COLLIDES) continue;  // (counts only together with FW_PATH_SMALL)
        CHECK(!C.remove(b) && C == empty, "remove from an empty census is refused", b);
    }
    CHECK(!C.remove(FW_PATH_SMALL | FW_PATH_COLLIDES) && C == empty, "small + collides from an empty census");
    C.add(FW_PATH_IN_USE | FW_PATH_SMALL);
    const FwPathCensus before = C;
    CHECK(!C.remove(FW_PATH_IN_USE | FW_PATH_SMALL | FW_PATH_COLLIDES) && C == before, "a colliding small type was never added: refused, nothing changed");
    CHECK(!C.remove(FW_PATH_IN_USE | FW_PATH_FIFO) && C == before, "one count short: refused whole, nothing changed");
    CHECK(C.remove(FW_PATH_IN_USE | FW_PATH_SMALL) && C == empty, "what was added goes");
    CHECK(C.n_in_use == 0u && C.n_small == 0u && C.n_small_coll == 0u && C.n_fifo == 0u, "no counter wrapped");
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const uint32_t seeds = (uint32_t)atoi(argv[1]), ops = (uint32_t)atoi(argv[2]);
    rule_grid();
    facts_of_random_descriptors(20000);
    for (uint32_t s = 1; s <= seeds; s++) census_random(s, ops);
    census_hysteresis();
    census_refuses();
    printf("total cases %llu fifo_q0pl %llu fifo_float4 %llu fifo_mat %llu fifo_dev %llu range_by_size %llu range_few_ring %llu few_nested %llu spilled %llu "
           "spill_compacting %llu alone_use_range %llu alone_no_rings %llu alone_self_nested %llu alone_mixed_feed %llu alone_lplanes %llu alone_collision %llu "
           "alone_life_not_finite %llu alone_life_lo_safe %llu alone_size %llu alone_max_capacity %llu census_ops %llu bad %llu\n",
           n_cases, n_fifo_q0pl, n_fifo_float4, n_fifo_mat, n_fifo_dev, n_range_by_size, n_range_few_ring, n_few_nested, n_spilled, n_spill_compacting,
           n_compact_alone[R_USE_RANGE], n_compact_alone[R_NO_RINGS], n_compact_alone[R_SELF_NESTED], n_compact_alone[R_MIXED_FEED], n_compact_alone[R_LPLANES],
           n_compact_alone[R_COLLISION], n_compact_life_not_finite, n_compact_life_lo_safe, n_compact_alone[R_SIZE], n_compact_alone[R_MAX_CAPACITY], n_census_ops, n_bad);
    return n_bad ? 1 : 0;
}
"""

SEEDS, OPS = 8, 4000

OUTCOMES = ["fifo_q0pl", "fifo_float4", "fifo_mat", "fifo_dev", "range_by_size", "range_few_ring", "few_nested", "spilled", "spill_compacting",
            "alone_use_range", "alone_no_rings", "alone_self_nested", "alone_mixed_feed", "alone_lplanes", "alone_collision", "alone_life_not_finite",
            "alone_life_lo_safe", "alone_size", "alone_max_capacity"]


def _hipcc():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "address,undefined"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("update_path")
    (d / "update_path.cpp").write_text(PROGRAM)
    exe = d / "update_path"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=" + request.param, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([_hipcc(), "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror",
                           "-I", CSRC] + flags + [str(d / "update_path.cpp"), "-o", str(exe)])
    return str(exe)


def test_the_rule_is_the_model_and_the_census_its_recount(program):
    r = subprocess.run([program, str(SEEDS), str(OPS)], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert not [ln for ln in lines if ln.startswith("BAD")], lines[:30]
    assert r.returncode == 0, r.stderr[-2000:]
    total = dict(zip(lines[-1].split()[1::2], map(int, lines[-1].split()[2::2])))
    print(lines[-1])
    assert total["bad"] == 0
    assert total["cases"] > 10_000_000 and total["census_ops"] == SEEDS * OPS
    for k in OUTCOMES:  # every outcome occurred
        assert total[k] >= 1, (k, total)
