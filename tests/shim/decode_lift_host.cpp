// decode_lift (fhe-linformer_amd/csrc/decode_lift.h) as compiled for the host: reads lines "nl q0 q1 x0 x1 ms es" (decimal; q1 and x1 are
// 0 when nl = 1) from standard input and prints the IEEE bits of the decoded double in hexadecimal, one per line.  The constants of the
// lift (q0^-1 mod q1 and its Shoup companion) are made here as Client::decrypt_batch makes them.  Driver of tests/test_decode_lift_host.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../fhe-linformer_amd/csrc/decode_lift.h"

int main() {
    int nl, es;
    uint64_t q0, q1, x0, x1, ms;
    while (std::scanf("%d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &nl, &q0, &q1, &x0, &x1, &ms, &es) == 7) {
        fhelin::DecodeLift p;
        p.q0 = q0;
        p.q1 = nl > 1 ? q1 : 1;
        p.inv = nl > 1 ? fhelin::h_invmod(q0 % q1, q1) : 0;
        p.inv_shoup = nl > 1 ? fhelin::h_shoup(p.inv, q1) : 0;
        p.ms = ms;
        p.es = es;
        p.nl = nl;
        const double d = fhelin::decode_lift(x0, x1, p);
        uint64_t bits;
        std::memcpy(&bits, &d, sizeof bits);
        std::printf("%016" PRIx64 "\n", bits);
    }
    return 0;
}
