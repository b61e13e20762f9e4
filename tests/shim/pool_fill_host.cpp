// The device pool's fill knob (csrc/pool.cpp, FHELIN_POOL_FILL) as a stand-alone host program: no GPU, no HIP runtime.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I$ROCM/include \
//       tests/shim/pool_fill_host.cpp fhe-linformer_amd/csrc/pool.cpp -o pool_fill_host
//
// The pool runs over host malloc with a host fill function, so every word the self-test reads or writes is memory the sanitizers see:
// a fill that ran one word past its block, or a check that read past a slab, ends the program.  The few HIP entry points the pool
// names are defined here and abort: the host path must never reach the runtime.  tests/test_pool_fill_host.py builds and runs the
// program without the sanitizers; with them it prints the same lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../fhe-linformer_amd/csrc/pool.h"

static void unreachable(const char* what) {
    std::fprintf(stderr, "pool_fill_host: the host path called %s\n", what);
    std::abort();
}
extern "C" {
hipError_t hipMalloc(void**, size_t) { unreachable("hipMalloc"); return hipErrorUnknown; }
hipError_t hipFree(void*) { unreachable("hipFree"); return hipErrorUnknown; }
hipError_t hipGetLastError(void) { unreachable("hipGetLastError"); return hipErrorUnknown; }
const char* hipGetErrorString(hipError_t) { return "hip stub"; }
hipError_t hipEventDestroy(hipEvent_t) { unreachable("hipEventDestroy"); return hipErrorUnknown; }
hipError_t hipEventCreateWithFlags(hipEvent_t*, unsigned) { unreachable("hipEventCreateWithFlags"); return hipErrorUnknown; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { unreachable("hipEventRecord"); return hipErrorUnknown; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { unreachable("hipStreamWaitEvent"); return hipErrorUnknown; }
hipError_t hipDeviceSynchronize(void) { unreachable("hipDeviceSynchronize"); return hipErrorUnknown; }
hipError_t hipStreamSynchronize(hipStream_t) { unreachable("hipStreamSynchronize"); return hipErrorUnknown; }
hipError_t hipMemsetD32Async(hipDeviceptr_t, int, size_t, hipStream_t) { unreachable("hipMemsetD32Async"); return hipErrorUnknown; }
}

int main(int argc, char** argv) {
    using fhelin::DevicePool;
    const int n_ops = argc > 1 ? std::atoi(argv[1]) : 1500;
    int bad = 0;
    for (uint64_t seed = 1; seed <= 3; ++seed)
        for (uint32_t w : {0u, 1u, 2u, 4095u}) {
            uint64_t out[6] = {};
            try {
                fhelin::pool_fill_selftest(seed, n_ops, w, out, 6);
            } catch (const fhelin::Error& e) {
                std::printf("FAIL seed %llu w %u: %s\n", (unsigned long long)seed, w, e.what());
                ++bad;
                continue;
            }
            const bool ok = w ? (out[2] == out[0] && out[3] == out[1]) : (out[2] == 0 && out[3] == 0);
            std::printf("%s seed %llu w %u: %llu blocks (%llu at 4 KiB granules), %llu rounded bytes, filled %llu blocks %llu bytes, %llu slabs\n",
                        ok ? "ok" : "FAIL", (unsigned long long)seed, w, (unsigned long long)out[0], (unsigned long long)out[5],
                        (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[4]);
            bad += !ok;
        }
    // the knob's text
    const struct { const char* text; int want; } cases[] = {{nullptr, 0}, {"", 0}, {"0", 0}, {"1", 1}, {"2", 2}, {"4095", 4095}, {"4096", -1},
        {"4294967295", -1}, {"0xFFFFFFFF", -1}, {"-1", -1}, {"one", -1}, {"7x", -1}, {" 7", -1}, {"99999999999999999999999", -1}};
    for (const auto& c : cases) {
        int got;
        try {
            got = (int)DevicePool::parse_fill(c.text);
        } catch (const fhelin::Error& e) {
            got = e.code == FHELIN_ERR_ARG ? -1 : -2;
        }
        if (got != c.want) {
            std::printf("FAIL parse '%s': %d, want %d\n", c.text ? c.text : "(unset)", got, c.want);
            ++bad;
        }
    }
    std::printf("%s\n", bad ? "pool_fill_host: FAILED" : "pool_fill_host: all ok");
    return bad ? 1 : 0;
}
