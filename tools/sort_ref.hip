// sort_ref.hip -- the yardstick of tools/sorted_pack.py: rocprim::radix_sort_pairs on the keys the library's depth sort ordered, with
// the same values (the indices 0 .. n-1).  A tool only: never linked into libfirework_hip.so, never used by a test.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/sort_ref.hip -o tools/sort_ref_bench
//   tools/sort_ref_bench KEYS.u32 [windows] [calls] [ORDER.u32]
//
// KEYS.u32: n little-endian uint32 keys.  Prints one JSON line: n, the best and the median window's microseconds per sort (device
// events around `calls` sorts, after 5 warm-up sorts), and writes the sorted indices to ORDER.u32 -- radix_sort_pairs is stable, so they
// equal the library's order.
#include <cstring>  // (rocprim's texture iterator calls memset without including it)

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                          \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const int windows = argc > 2 ? std::atoi(argv[2]) : 5, calls = argc > 3 ? std::atoi(argv[3]) : 20;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / 4;
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> keys(n), idx(n);
    if (n && std::fread(keys.data(), 4, n, f) != n) return 2;
    std::fclose(f);
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    uint32_t *d_k = nullptr, *d_v = nullptr, *d_ko = nullptr, *d_vo = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    CHECK(hipMalloc(&d_k, std::max<size_t>(n, 1) * 4));
    CHECK(hipMalloc(&d_v, std::max<size_t>(n, 1) * 4));
    CHECK(hipMalloc(&d_ko, std::max<size_t>(n, 1) * 4));
    CHECK(hipMalloc(&d_vo, std::max<size_t>(n, 1) * 4));
    CHECK(hipMemcpy(d_k, keys.data(), n * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_v, idx.data(), n * 4, hipMemcpyHostToDevice));
    hipStream_t s;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_k, d_ko, d_v, d_vo, n, 0, 32, s));
    CHECK(hipMalloc(&d_tmp, std::max<size_t>(tmp_bytes, 16)));
    for (int i = 0; i < 5; i++) CHECK(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_k, d_ko, d_v, d_vo, n, 0, 32, s));
    CHECK(hipStreamSynchronize(s));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<double> us;
    for (int w = 0; w < windows; w++) {
        CHECK(hipEventRecord(e0, s));
        for (int i = 0; i < calls; i++) CHECK(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_k, d_ko, d_v, d_vo, n, 0, 32, s));
        CHECK(hipEventRecord(e1, s));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.0f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        us.push_back((double)ms * 1e3 / calls);
    }
    CHECK(hipMemcpy(idx.data(), d_vo, n * 4, hipMemcpyDeviceToHost));
    if (argc > 4) {
        FILE *o = std::fopen(argv[4], "wb");
        if (!o || (n && std::fwrite(idx.data(), 4, n, o) != n)) return 2;
        std::fclose(o);
    }
    std::sort(us.begin(), us.end());
    std::printf("{\"n\": %zu, \"best_us\": %.2f, \"median_us\": %.2f, \"temp_bytes\": %zu}\n", n, us.front(), us[us.size() / 2], tmp_bytes);
    return 0;
}
