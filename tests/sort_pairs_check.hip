// sort_pairs_check.hip -- one call of fw_launch_sort_pairs (csrc/fw_k_sort.hip; its contract: fw_kernels.h) on the pairs of one case file,
// for tests/test_gpu_sort_pairs.py.  Built with csrc/fw_k_sort.hip and the FLAGS of csrc/Makefile; no context, no particles, no timing.
//
//   sort_pairs_check CASE OUT
//
// CASE (uint32 words): n_upper, the device count word, with_out (0: d_idx_out = null, 1: a buffer of its own), n_upper keys, n_upper values.
// The scratch is fw_sort_scratch_words(n_upper) words between two guards of GUARD words; d_idx_out is n_upper words between two guards as
// well; every word of both allocations starts as POISON.  Keys go to scratch[0, n_upper), values to scratch[n_upper, 2 * n_upper).
// OUT (uint32 words): GUARD; the first n_upper words of the scratch (keys); the n_upper index words from where the contract leaves them
// (d_idx_out when one was passed, scratch + n_upper otherwise); the scratch's low guard; its high guard; all of d_idx_out's allocation
// (GUARD + n_upper + GUARD words).
// Exit: 0 done; 1 no HIP device (no CPU fallback); 2 usage or a file that is not a case; 3 a HIP error, its text on stderr.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fw_kernels.h"
#include "fw_sort.h"

static const uint32_t GUARD = 4096u, POISON = 0xA5A5A5A5u;

#define CHECK(call)                                                                                       \
    do {                                                                                                  \
        const hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                           \
            fprintf(stderr, "sort_pairs_check: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
            return 3;                                                                                     \
        }                                                                                                 \
    } while (0)

static bool put(FILE *f, const uint32_t *p, size_t n) { return fwrite(p, 4, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: sort_pairs_check CASE OUT\n");
        return 2;
    }
    uint32_t head[3];
    FILE *in = fopen(argv[1], "rb");
    if (!in || fread(head, 4, 3, in) != 3 || !head[0] || head[0] > 0x10000000u || head[2] > 1u) {
        fprintf(stderr, "sort_pairs_check: %s is not a case file\n", argv[1]);
        return 2;
    }
    const uint32_t n_upper = head[0], count = head[1];
    const bool with_out = head[2] != 0u;
    std::vector<uint32_t> pairs((size_t)n_upper * 2u);
    if (fread(pairs.data(), 4, pairs.size(), in) != pairs.size() || fgetc(in) != EOF) {
        fprintf(stderr, "sort_pairs_check: %s does not hold %u keys and %u values\n", argv[1], n_upper, n_upper);
        return 2;
    }
    fclose(in);

    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) {
        fprintf(stderr, "sort_pairs_check: no HIP device: the sort runs on a gfx950 GPU only, no CPU fallback\n");
        return 1;
    }
    CHECK(hipSetDevice(0));
    const size_t words = fw_sort_scratch_words(n_upper), s_all = words + 2u * GUARD, o_all = (size_t)n_upper + 2u * GUARD;
    uint32_t *d_scratch = nullptr, *d_out = nullptr, *d_count = nullptr;
    CHECK(hipMalloc(&d_scratch, s_all * 4u));
    CHECK(hipMalloc(&d_out, o_all * 4u));
    CHECK(hipMalloc(&d_count, 4u));
    CHECK(hipMemsetD32(d_scratch, (int)POISON, s_all));
    CHECK(hipMemsetD32(d_out, (int)POISON, o_all));
    uint32_t *const scratch = d_scratch + GUARD, *const idx_out = d_out + GUARD;
    CHECK(hipMemcpy(scratch, pairs.data(), pairs.size() * 4u, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_count, &count, 4u, hipMemcpyHostToDevice));
    CHECK(hipDeviceSynchronize());

    hipStream_t s;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    CHECK(fw_launch_sort_pairs(s, d_count, n_upper, scratch, with_out ? idx_out : nullptr));
    CHECK(hipStreamSynchronize(s));

    std::vector<uint32_t> h_scratch(s_all), h_out(o_all);
    CHECK(hipMemcpy(h_scratch.data(), d_scratch, s_all * 4u, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h_out.data(), d_out, o_all * 4u, hipMemcpyDeviceToHost));
    CHECK(hipStreamDestroy(s));
    CHECK(hipFree(d_scratch));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_count));

    FILE *out = fopen(argv[2], "wb");
    const uint32_t *const sc = h_scratch.data() + GUARD;
    if (!out || !put(out, &GUARD, 1) || !put(out, sc, n_upper) || !put(out, with_out ? h_out.data() + GUARD : sc + n_upper, n_upper) ||
        !put(out, h_scratch.data(), GUARD) || !put(out, sc + words, GUARD) || !put(out, h_out.data(), o_all) || fclose(out) != 0) {
        fprintf(stderr, "sort_pairs_check: cannot write %s\n", argv[2]);
        return 2;
    }
    return 0;
}
