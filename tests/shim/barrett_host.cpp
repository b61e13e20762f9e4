// barrett_reduce128 (fhe-linformer_amd/csrc/modarith.h) as compiled for the host: reads lines "q lo hi" (decimal) from standard input and
// prints the reduced value of hi * 2^64 + lo modulo q, one per line.  Driver of tests/test_dot_kernels_host.py.
#include <cinttypes>
#include <cstdio>
#include "../../fhe-linformer_amd/csrc/modarith.h"

int main() {
    uint64_t q, lo, hi;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &q, &lo, &hi) == 3) {
        const fhelin::Barrett b = fhelin::h_barrett(q);
        std::printf("%" PRIu64 "\n", fhelin::barrett_reduce128(lo, hi, b));
    }
    return 0;
}
