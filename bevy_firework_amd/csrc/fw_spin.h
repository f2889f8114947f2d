// fw_spin.h -- the deferred spin of a FIFO ring nobody reads (round 19, FW_TYPE_IDX_NOSPIN together with FW_TYPE_IDX_AXIS: fw_device.h).
// A launch under the rule neither loads nor integrates nor stores rotation and angular velocity of the particles that were in the ring
// before it; the host logs the frame's dt instead (FwSpinBook::log, oldest first) and remembers, per spawn cohort, the first log entry
// its particles have not had applied.  fw_k_fifo_spin (fw_k_aux.hip) replays the entries per particle before anybody looks: a table of
// one entry per cohort that holds particles -- the logical index of its first particle, its first pending log entry -- and the log.
// Plain C++ behind FW_HD, like fw_ages.h: the kernel, the host bookkeeping (launch_fifo, ensure_spin) and a host test
// (tests/test_cpp_host_spin.py) compile the same lines.
#pragma once
#include <stdint.h>

#ifndef FW_HD
#ifdef __HIPCC__
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

struct FwSpinEntry {
    uint32_t first;  // logical index of the cohort's first particle (ascending; entry 0: index 0)
    uint32_t pend;   // position in the uploaded log of the first step the cohort's particles have not had applied (== log_n: none)
};

// entry of particle i: the largest k in [0, n) with tab[k].first <= i   (n >= 1; the lookup of fw_age_entry, fw_ages.h)
FW_HD uint32_t fw_spin_entry(const FwSpinEntry *tab, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid].first <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the pending steps of particle i of a ring of `live` particles: log entries [*from, log_n), oldest first.  Returns their number;
// 0: nothing to replay (no such particle, an empty table, a cohort that is current, a table entry that points past the log)
FW_HD uint32_t fw_spin_steps(const FwSpinEntry *tab, uint32_t n, uint32_t live, uint32_t log_n, uint32_t i, uint32_t *from) {
    if (n == 0u || i >= live) return 0u;
    const uint32_t p = tab[fw_spin_entry(tab, n, i)].pend;
    *from = p;
    return p < log_n ? log_n - p : 0u;
}

// ---- the log's arithmetic.  Positions are absolute: entry number `base` is the oldest one still held, `base + size` the next one
// to be written; a cohort's pointer (`from`) is such a position.
// entries in front of the oldest pointer any live cohort holds are dropped (min_from: that pointer; base + size where no cohort is left)
FW_HD uint64_t fw_spin_trim(uint64_t base, uint64_t size, uint64_t min_from) {
    if (min_from <= base) return 0u;
    return min_from - base < size ? min_from - base : size;
}
// one more entry would exceed the cap: the ring is materialised before the launch
FW_HD bool fw_spin_full(uint64_t size, uint32_t cap) { return size + 1u > (uint64_t)cap; }
// a cohort's pointer as a position in the uploaded log (which starts at `base`); a pointer in front of it cannot exist after a trim
FW_HD uint32_t fw_spin_rel(uint64_t base, uint64_t size, uint64_t from) {
    if (from <= base) return 0u;
    return (uint32_t)(from - base < size ? from - base : size);
}

#include <deque>
// The host's half: the log of one ring and what its launches do to it.  Cohorts: any sequence of records, oldest first, with the
// members `n` (particles) and `spin_from` (absolute log position); SegHost::coh in the engine, a test's own type in the host test.
struct FwSpinBook {
    std::deque<float> log;  // dt of every deferred frame some live cohort has not had applied, oldest first
    uint64_t base = 0;      // absolute position of log[0]
    bool stale = false;     // some particle of the ring may have pending steps: the planes are not to be read
    uint64_t end() const { return base + log.size(); }

    // before a launch: dead cohorts have left `coh`; entries nobody points at any more go
    template <class Cohorts>
    void trim(const Cohorts &coh) {
        uint64_t mn = end();
        for (const auto &c : coh) mn = c.spin_from < mn ? c.spin_from : mn;
        for (uint64_t k = fw_spin_trim(base, log.size(), mn); k; k--) log.pop_front(), base++;
    }
    // a deferred launch with this dt: the cohorts that exist get no step (the first launch of a stretch points all of them at this
    // frame's entry).  Returns the pointer of a cohort SPAWNED by this launch, whose particles the launch integrates itself: the next entry.
    template <class Cohorts>
    uint64_t defer(Cohorts &coh, float dt) {
        if (!stale) {
            log.clear();
            for (auto &c : coh) c.spin_from = end();
            stale = true;
        }
        log.push_back(dt);
        return end();
    }
    // every particle has been brought up to date (or the ring holds none that matter any more)
    template <class Cohorts>
    void current(Cohorts &coh) {
        base = end(), log.clear(), stale = false;
        for (auto &c : coh) c.spin_from = base;
    }
    // the replay's table: one entry per cohort that holds particles; returns their number, *live the particles they hold
    template <class Cohorts>
    uint32_t table(const Cohorts &coh, FwSpinEntry *tab, uint64_t *live) const {
        uint32_t n = 0;
        uint64_t at = 0;
        for (const auto &c : coh) {
            if (!c.n) continue;
            tab[n++] = FwSpinEntry{(uint32_t)at, fw_spin_rel(base, log.size(), c.spin_from)};
            at += c.n;
        }
        *live = at;
        return n;
    }
};
