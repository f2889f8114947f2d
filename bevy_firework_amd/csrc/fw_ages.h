// fw_ages.h -- the age of a particle of a FIFO ring from the host's spawn cohorts (round 18, FW_TYPE_IDX_AGELESS: fw_device.h).
// The live particles of a FIFO ring are its cohorts laid end to end, oldest first (SegHost::coh); a launch under the age rule does
// not store the age plane, and fw_k_fifo_ages (fw_k_aux.hip) writes it back from a table of one entry per cohort -- the logical index
// of its first particle and the fp32 running sum the host kept for it: the bits the update would have stored.  Plain C++ behind
// FW_HD: the kernel and a host test (tests/test_cpp_host_ages.py) compile the same lines, as with fw_refit.h.
#pragma once
#include <stdint.h>

#ifndef FW_HD
#ifdef __HIPCC__
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

struct FwAgeEntry {
    uint32_t first;  // logical index of the cohort's first particle (ascending; entry 0: index 0)
    float age;
};

// entry of particle i: the largest k in [0, n) with tab[k].first <= i   (n >= 1; cohorts without a particle share their `first` with
// the next one and are never the answer's predecessor: the LAST entry with first <= i is the one that holds i)
FW_HD uint32_t fw_age_entry(const FwAgeEntry *tab, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid].first <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// age of particle i of a ring of `live` particles; false: no such particle (an empty table, i past the last cohort)
FW_HD bool fw_age_of(const FwAgeEntry *tab, uint32_t n, uint32_t live, uint32_t i, float *age) {
    if (n == 0u || i >= live) return false;
    *age = tab[fw_age_entry(tab, n, i)].age;
    return true;
}
