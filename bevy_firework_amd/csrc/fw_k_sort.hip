// fw_k_sort.hip -- the stable radix sort behind the depth-sorted instance records (fw_ctx_depth_order_device,
// fw_ctx_pack_instances_sorted[_device]; fw_sort.h has the key and the shape): (key, index) pairs of 32 bits each, ascending key, ties in
// the order they came in.  The keys come from fw_k_depth_keys and the sorted indices go to fw_k_pack<true> (both fw_k_aux.hip, where
// the segment decoders live).
//
// FW_SORT_PASSES passes of FW_SORT_BITS bits, least significant digit first, between two (key, idx) buffer pairs.  A pass is three
// launches of the context's stream:
//   fw_k_sort_hist     workgroup w counts the digits of elements [w * FW_SORT_TILE, (w + 1) * FW_SORT_TILE) into column w of the
//                      digit-major table: entry [digit][w]
//   fw_k_sort_scan     workgroup d turns row d into its exclusive prefix sums and leaves the row's total in totals[d]
//   fw_k_sort_scatter  workgroup w scans the 256 totals itself (where digit d starts), adds its entry of row d (how many elements of
//                      digit d sit in earlier workgroups) and ranks its own elements behind that, stably: rounds of one element per
//                      lane, so (round, wave, lane) is the incoming order; within a wave the lanes of equal digit find each other with
//                      eight 64-bit ballots and a lane's rank is the population count of its peers below it; the waves of a round add
//                      their counts through LDS.
// What one workgroup wrote is read by another only across a kernel boundary, and no workgroup ever waits for another: nothing here
// spins, polls, looks back or counts arrivals (fw_k_refit.hip's rule), so a sort cannot hang whatever else the device runs.
// n = min(*d_count, n_upper) is the device's, read by every launch from the same word (no launch of the stream in between changes
// it): the host never learns it.  Every address is formed from n, n_upper and values these kernels wrote themselves; a store is
// skipped, not trusted, where the position would not be below n.
#include <hip/hip_runtime.h>

#include "fw_kernels.h"
#include "fw_sort.h"

// exclusive prefix sum of one value per lane over a workgroup of FW_SORT_WG lanes; *total: the sum of all of them
__device__ __forceinline__ uint32_t fw_sort_block_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t s_wave[FW_SORT_WG / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < FW_SORT_WG / 64; w++) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();  // (s_wave may be written again by the caller's next scan)
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(FW_SORT_WG) void fw_k_sort_hist(const uint32_t *d_count, uint32_t n_upper, const uint32_t *key, uint32_t shift,
                                                             uint32_t *table, uint32_t tiles) {
    __shared__ uint32_t s_h[FW_SORT_DIGITS];
    const uint32_t n = min(*d_count, n_upper);
    const uint32_t tid = threadIdx.x, base = blockIdx.x * FW_SORT_TILE;
    s_h[tid] = 0u;
    __syncthreads();
    for (uint32_t r = 0; r < FW_SORT_ROUNDS && base + r * FW_SORT_WG < n; r++) {  // (uniform bounds: n_upper <= 0xF0000000, nothing wraps)
        const uint32_t e = base + r * FW_SORT_WG + tid;
        if (e < n) atomicAdd(&s_h[(key[e] >> shift) & (FW_SORT_DIGITS - 1u)], 1u);
    }
    __syncthreads();
    table[(size_t)tid * tiles + blockIdx.x] = s_h[tid];  // (a workgroup past n writes its zeros: the scan reads every column)
}

__global__ __launch_bounds__(FW_SORT_WG) void fw_k_sort_scan(uint32_t *table, uint32_t tiles, uint32_t *totals) {
    uint32_t *row = table + (size_t)blockIdx.x * tiles;
    const uint32_t per = (tiles + FW_SORT_WG - 1u) / FW_SORT_WG;
    const uint32_t lo = min(threadIdx.x * per, tiles), hi = min(lo + per, tiles);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += row[i];
    uint32_t total;
    uint32_t run = fw_sort_block_scan(sum, &total);
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = row[i];
        row[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(FW_SORT_WG) void fw_k_sort_scatter(const uint32_t *d_count, uint32_t n_upper, const uint32_t *key_in, const uint32_t *idx_in,
                                                                uint32_t shift, const uint32_t *table, uint32_t tiles, const uint32_t *totals,
                                                                uint32_t *key_out, uint32_t *idx_out) {
    __shared__ uint32_t s_base[FW_SORT_DIGITS];               // where the next element of digit d goes
    __shared__ uint32_t s_w[FW_SORT_WG / 64][FW_SORT_DIGITS];  // this round: elements of digit d in wave w
    const uint32_t n = min(*d_count, n_upper);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, base = blockIdx.x * FW_SORT_TILE;
    if (base >= n) return;  // (uniform, before any barrier)
    uint32_t all;
    const uint32_t first = fw_sort_block_scan(totals[tid], &all);
    s_base[tid] = first + table[(size_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < FW_SORT_WG / 64; w++) s_w[w][tid] = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < FW_SORT_ROUNDS && base + r * FW_SORT_WG < n; r++) {
        const uint32_t e = base + r * FW_SORT_WG + tid;
        const bool valid = e < n;
        const uint32_t k = valid ? key_in[e] : 0u, v = valid ? idx_in[e] : 0u;
        const uint32_t d = (k >> shift) & (FW_SORT_DIGITS - 1u);
        unsigned long long peers = __ballot(valid);  // the lanes of this wave that hold an element of my digit
#pragma unroll
        for (uint32_t bit = 0; bit < FW_SORT_BITS; bit++) {
            const bool set = ((d >> bit) & 1u) != 0u;
            const unsigned long long bal = __ballot(set);
            peers &= set ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0u) s_w[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = s_base[d] + rank;
#pragma unroll
            for (uint32_t w = 0; w < FW_SORT_WG / 64; w++) pos += w < wave ? s_w[w][d] : 0u;
            if (pos < n) key_out[pos] = k, idx_out[pos] = v;
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (uint32_t w = 0; w < FW_SORT_WG / 64; w++) add += s_w[w][tid], s_w[w][tid] = 0u;
        s_base[tid] += add;
        __syncthreads();
    }
}

hipError_t fw_launch_sort_pairs(hipStream_t s, const uint32_t *d_count, uint32_t n_upper, uint32_t *scratch, uint32_t *d_idx_out) {
    if (!n_upper) return hipSuccess;
    if (n_upper > 0xF0000000u || !scratch) return hipErrorInvalidValue;
    const uint32_t tiles = fw_sort_tiles(n_upper);
    uint32_t *key[2] = {scratch, scratch + (size_t)n_upper * 2u}, *idx[2] = {key[0] + n_upper, key[1] + n_upper};
    uint32_t *table = scratch + (size_t)n_upper * 4u, *totals = table + (size_t)tiles * FW_SORT_DIGITS;
    for (uint32_t p = 0; p < FW_SORT_PASSES; p++) {
        const uint32_t in = p & 1u, out = in ^ 1u, shift = p * FW_SORT_BITS;
        uint32_t *idx_out = (p + 1u == FW_SORT_PASSES && d_idx_out) ? d_idx_out : idx[out];
        hipLaunchKernelGGL(fw_k_sort_hist, dim3(tiles), dim3(FW_SORT_WG), 0, s, d_count, n_upper, (const uint32_t *)key[in], shift, table, tiles);
        hipLaunchKernelGGL(fw_k_sort_scan, dim3(FW_SORT_DIGITS), dim3(FW_SORT_WG), 0, s, table, tiles, totals);
        hipLaunchKernelGGL(fw_k_sort_scatter, dim3(tiles), dim3(FW_SORT_WG), 0, s, d_count, n_upper, (const uint32_t *)key[in], (const uint32_t *)idx[in],
                           shift, (const uint32_t *)table, tiles, (const uint32_t *)totals, key[out], idx_out);
    }
    return hipGetLastError();
}
