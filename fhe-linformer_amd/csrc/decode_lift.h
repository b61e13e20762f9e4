// The decoder's number conversion, host/device like modarith.h: the one or two phase residues of a coefficient -> the double that
// Client::decrypt_physical's `(double)(lift(idx) / ct->scale)` gives on x87, in integer code only (no long double on the device).
//
//   RNE53( RNE64( RNE64(|centred CRT lift|) / S ) ),   S = ms * 2^es with 2^63 <= ms < 2^64
//
// stated from its definitions in tests/encode_model.py decode_double and held to it bit for bit (tests/test_decode_lift_host.py on the
// host build of this header, tests/test_decrypt_batch_gpu.py on the device):
//   * CRT over (q0, q1): x = x0 + q0 * ((x1 - x0 mod q1) * q0^-1 mod q1), below M = q0 q1 < 2^116; one limb: x = x0, M = q0
//   * centring with the host's rule: x > floor(M / 2) is the negative M - x
//   * the magnitude (up to 107 bits with two limbs) rounded to a 64-bit significand, ties to even: the host's
//     (long double)hi * 2^64 + (long double)lo
//   * the quotient of the two 64-bit significands rounded to 64 bits, with the carry to the next binade: the x87 division
//   * that quotient rounded to 53 bits, ties to even, assembled as IEEE bits with the sign: the conversion to double
// Zero gives +0.0.  The result must be a normal double (true for every scale the engine makes: |es| stays far below 900).
#pragma once
#include "modarith.h"

namespace fhelin {

// per-call constants of the lift: nl = 1 reads q0 and the scale only
struct DecodeLift {
    u64 q0, q1;
    u64 inv, inv_shoup;   // q0^-1 mod q1 and floor(inv * 2^64 / q1)
    u64 ms;               // the scale's 64-bit significand (top bit set)
    int32_t es;           // scale = ms * 2^es
    int32_t nl;           // limbs read: 1 or 2
};

FHE_HD int decode_clz64(u64 x) {   // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

FHE_HD double decode_bits_to_double(u64 bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)bits);
#else
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
#endif
}

// x0 in [0, q0), x1 in [0, q1) (ignored when p.nl == 1)
FHE_HD double decode_lift(u64 x0, u64 x1, const DecodeLift& p) {
    // ---- centred lift: magnitude (hi:lo) and sign
    u64 lo, hi = 0;
    bool neg;
    if (p.nl == 1) {
        neg = x0 > p.q0 / 2;
        lo = neg ? p.q0 - x0 : x0;
    } else {
        const u64 d = mul_shoup(sub_mod(x1, x0 % p.q1, p.q1), p.inv, p.inv_shoup, p.q1);
        lo = p.q0 * d;
        hi = mulhi64(p.q0, d);
        lo += x0;
        hi += lo < x0;
        const u64 Qlo = p.q0 * p.q1, Qhi = mulhi64(p.q0, p.q1);
        const u64 Hlo = (Qlo >> 1) | (Qhi << 63), Hhi = Qhi >> 1;   // floor(M / 2)
        neg = hi > Hhi || (hi == Hhi && lo > Hlo);
        if (neg) {
            const u64 l = Qlo - lo;
            hi = Qhi - hi - (Qlo < lo);
            lo = l;
        }
    }
    if ((lo | hi) == 0) return 0.0;
    // ---- first rounding: the magnitude as m * 2^e with 2^63 <= m < 2^64, ties to even
    u64 m;
    int e;
    if (hi) {
        const int sh = 64 - decode_clz64(hi);                 // bits above 64: 1..52
        m = (lo >> sh) | (hi << (64 - sh));
        const u64 rem = lo & ((1ull << sh) - 1), half = 1ull << (sh - 1);
        e = sh;
        if (rem > half || (rem == half && (m & 1))) {
            ++m;
            if (m == 0) {                                     // carried out of 64 bits
                m = 1ull << 63;
                ++e;
            }
        }
    } else {
        const int z = decode_clz64(lo);                       // exact: normalised only
        m = lo << z;
        e = -z;
    }
    // ---- second rounding: m / ms in (1/2, 2) as a 64-bit significand q.  Long division, one quotient bit per shift-subtract step
    // (the device has no 128-by-64 division to link against); r < ms throughout, so 2r needs its carry bit
    u64 r = m, q = 0;
    int steps = 64;
    e -= p.es + 64;
    if (m >= p.ms) {                                          // quotient in [1, 2): its leading one first
        r -= p.ms;
        q = 1;
        steps = 63;
        ++e;
    }
    for (int i = 0; i < steps; ++i) {
        const u64 top = r >> 63;
        r <<= 1;
        const u64 bit = (top | (r >= p.ms)) ? 1 : 0;
        if (bit) r -= p.ms;
        q = (q << 1) | bit;
    }
    {
        // remainder against one half of the divisor: 2r ? ms.  A tie cannot occur - the quotient of two 64-bit significands is never a
        // 65-bit midpoint: m * 2^x = ms * t with t odd would force ms = 2^63, and then the quotient is m itself - so the ties-to-even
        // branch below is unreachable; it is coded so that the function is the model's
        const u64 top = r >> 63, r2 = r << 1;
        const bool above = top || r2 > p.ms, tie = !top && r2 == p.ms;
        if (above || (tie && (q & 1))) {
            ++q;
            if (q == 0) {                                     // carry to the next binade
                q = 1ull << 63;
                ++e;
            }
        }
    }
    // ---- third rounding: 64 -> 53 bits, ties to even; value = q * 2^e
    u64 m53 = q >> 11;
    const u64 rem = q & 0x7FF;
    e += 11;
    if (rem > 0x400 || (rem == 0x400 && (m53 & 1))) {
        ++m53;
        if (m53 == (1ull << 53)) {
            m53 = 1ull << 52;
            ++e;
        }
    }
    const u64 bits = ((u64)neg << 63) | ((u64)(e + 52 + 1023) << 52) | (m53 & 0xFFFFFFFFFFFFFull);
    return decode_bits_to_double(bits);
}

}  // namespace fhelin
