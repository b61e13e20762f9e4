#include "client.h"
#include "kernels_seeded.h"
#include <time.h>
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <map>
#include <mutex>

namespace fhelin {

// ------------------------------------------------------------------------------------------------ PRNG
// ChaCha20 over GCC vector types: lane j of every state word belongs to block (counter + j), so one pass of the
// 20 rounds yields LANES blocks (lowered to SSE2/AVX2 by the compiler; no intrinsics).
namespace {
typedef u32 vw __attribute__((vector_size(4 * Prng::LANES)));
#define FHELIN_ROTL(x, k) (((x) << (k)) | ((x) >> (32 - (k))))
inline void quarter(vw& a, vw& b, vw& c, vw& d) {  // vectors travel by reference only (no vector ABI involved)
    a += b; d ^= a; d = FHELIN_ROTL(d, 16);
    c += d; b ^= c; b = FHELIN_ROTL(b, 12);
    a += b; d ^= a; d = FHELIN_ROTL(d, 8);
    c += d; b ^= c; b = FHELIN_ROTL(b, 7);
}
void chacha20_blocks(const u32 key[8], u64 counter, u64 stream, u32* out /* [LANES][16] */) {
    static const u32 sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};  // "expand 32-byte k"
    vw init[16], x[16];
    for (int i = 0; i < 4; ++i) init[i] = vw{} + sigma[i];
    for (int i = 0; i < 8; ++i) init[4 + i] = vw{} + key[i];
    for (int j = 0; j < Prng::LANES; ++j) {
        const u64 c = counter + (u64)j;
        init[12][j] = (u32)c;
        init[13][j] = (u32)(c >> 32);
    }
    init[14] = vw{} + (u32)stream;
    init[15] = vw{} + (u32)(stream >> 32);
    for (int i = 0; i < 16; ++i) x[i] = init[i];
    for (int r = 0; r < 10; ++r) {
        quarter(x[0], x[4], x[8], x[12]);
        quarter(x[1], x[5], x[9], x[13]);
        quarter(x[2], x[6], x[10], x[14]);
        quarter(x[3], x[7], x[11], x[15]);
        quarter(x[0], x[5], x[10], x[15]);
        quarter(x[1], x[6], x[11], x[12]);
        quarter(x[2], x[7], x[8], x[13]);
        quarter(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 16; ++i) {
        x[i] += init[i];
        for (int j = 0; j < Prng::LANES; ++j) out[j * 16 + i] = x[i][j];
    }
}
void load_key(const uint8_t seed[32], u32 key[8]) {
    for (int i = 0; i < 8; ++i)
        key[i] = (u32)seed[4 * i] | ((u32)seed[4 * i + 1] << 8) | ((u32)seed[4 * i + 2] << 16) | ((u32)seed[4 * i + 3] << 24);
}
}  // namespace

Prng::Prng(const uint8_t seed[32], u64 stream) : stream_(stream) { load_key(seed, key_); }

void Prng::refill() {
    chacha20_blocks(key_, counter_, stream_, buf_);
    counter_ += LANES;
    pos_ = 0;
}
void Prng::block(const uint8_t seed[32], u64 counter, u64 stream, uint8_t out[64]) {
    u32 key[8], buf[16 * LANES];
    load_key(seed, key);
    chacha20_blocks(key, counter, stream, buf);
    for (int i = 0; i < 16; ++i)
        for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(buf[i] >> (8 * b));
}
u64 Prng::next() {
    if (pos_ + 2 > 16 * LANES) refill();
    const u64 r = (u64)buf_[pos_] | ((u64)buf_[pos_ + 1] << 32);
    pos_ += 2;
    return r;
}
u64 Prng::uniform(u64 q) {  // multiply-shift with rejection of the biased low range (exactly uniform)
    const u64 thresh = (0 - q) % q;  // 2^64 mod q
    for (;;) {
        const u128 m = (u128)next() * q;
        if ((u64)m >= thresh) return (u64)(m >> 64);
    }
}
double Prng::normal() {
    if (have_spare) {
        have_spare = false;
        return spare;
    }
    double u1, u2;
    do {
        u1 = (next() >> 11) * (1.0 / 9007199254740992.0);
    } while (u1 <= 0.0);
    u2 = (next() >> 11) * (1.0 / 9007199254740992.0);
    const double r = std::sqrt(-2.0 * std::log(u1)), th = 6.283185307179586476925 * u2;
    spare = r * std::sin(th);
    have_spare = true;
    return r * std::cos(th);
}

// ------------------------------------------------------------------------------------------------ special FFT
namespace {
struct FftTables {
    std::vector<u32> rot;                         // 5^j mod 4*slots
    std::vector<std::complex<double>> ksi;        // exp(2 pi i k / (4*slots)), k in [0, 4*slots]
};
std::map<int, FftTables> g_fft;
std::mutex g_fft_mu;
const FftTables& fft_tables(int slots) {
    std::lock_guard<std::mutex> lk(g_fft_mu);
    auto it = g_fft.find(slots);
    if (it != g_fft.end()) return it->second;
    FftTables t;
    const u32 m = 4u * slots;
    t.rot.resize(slots);
    u32 p = 1;
    for (int j = 0; j < slots; ++j) {
        t.rot[j] = p;
        p = (u32)(((u64)p * 5) % m);
    }
    t.ksi.resize(m + 1);
    for (u32 k = 0; k <= m; ++k) {
        const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)m;
        t.ksi[k] = {(double)cosl(a), (double)sinl(a)};
    }
    return g_fft.emplace(slots, std::move(t)).first->second;
}
void bit_reverse(std::vector<std::complex<double>>& v) {
    const size_t n = v.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j >= bit; bit >>= 1) j -= bit;
        j += bit;
        if (i < j) std::swap(v[i], v[j]);
    }
}
}  // namespace

// canonical embedding restricted to the rotation group <5>: forward = decode direction
void ckks_fft_special(std::vector<std::pair<double, double>>& pv, bool inverse) {
    const int size = (int)pv.size();
    const FftTables& t = fft_tables(size);
    const int m = 4 * size;
    std::vector<std::complex<double>> v(size);
    for (int i = 0; i < size; ++i) v[i] = {pv[i].first, pv[i].second};
    if (!inverse) {
        bit_reverse(v);
        for (int len = 2; len <= size; len <<= 1) {
            const int lenh = len >> 1, lenq = len << 2, gap = m / lenq;
            for (int i = 0; i < size; i += len)
                for (int j = 0; j < lenh; ++j) {
                    const int idx = (t.rot[j] % lenq) * gap;
                    const auto u = v[i + j], w = v[i + j + lenh] * t.ksi[idx];
                    v[i + j] = u + w;
                    v[i + j + lenh] = u - w;
                }
        }
    } else {
        for (int len = size; len >= 2; len >>= 1) {
            const int lenh = len >> 1, lenq = len << 2, gap = m / lenq;
            for (int i = 0; i < size; i += len)
                for (int j = 0; j < lenh; ++j) {
                    const int idx = (lenq - (t.rot[j] % lenq)) * gap;
                    const auto u = v[i + j] + v[i + j + lenh];
                    const auto w = (v[i + j] - v[i + j + lenh]) * t.ksi[idx];
                    v[i + j] = u;
                    v[i + j + lenh] = w;
                }
        }
        bit_reverse(v);
        const double inv = 1.0 / size;
        for (auto& x : v) x *= inv;
    }
    for (int i = 0; i < size; ++i) pv[i] = {v[i].real(), v[i].imag()};
}

void ckks_fft_tables(int slots, std::vector<u32>& rot, std::vector<std::pair<double, double>>& ksi) {
    const FftTables& t = fft_tables(slots);
    rot = t.rot;
    ksi.resize(t.ksi.size());
    for (size_t i = 0; i < t.ksi.size(); ++i) ksi[i] = {t.ksi[i].real(), t.ksi[i].imag()};
}

static void ld_to_i128(long double v, u64& lo, u64& hi) {
    if (v > -9.0e18L && v < 9.0e18L) {  // fits 64 bits: same rounding (half away from zero), no 128-bit split
        const long long r = llroundl(v);
        lo = (u64)r;
        hi = r < 0 ? ~0ull : 0;
        return;
    }
    const bool neg = v < 0;
    long double mag = roundl(fabsl(v));
    const long double two64 = 18446744073709551616.0L;
    u64 h = (u64)floorl(mag / two64);
    u64 l = (u64)(mag - (long double)h * two64);
    if (neg) {
        l = ~l + 1;
        h = ~h + (l == 0);
    }
    lo = l;
    hi = h;
}

static const Context::FftDev& fft_dev_tables(Context& c, int slots) {
    auto it = c.fft_dev.find(slots);
    if (it != c.fft_dev.end()) return it->second;
    const FftTables& t = fft_tables(slots);
    std::vector<double> k(2 * t.ksi.size());
    for (size_t i = 0; i < t.ksi.size(); ++i) {
        k[2 * i] = t.ksi[i].real();
        k[2 * i + 1] = t.ksi[i].imag();
    }
    Context::FftDev d;
    d.rot = c.upload_table(t.rot);
    d.ksi = c.upload_table(k);
    return c.fft_dev.emplace(slots, d).first->second;
}

// The encoder's domain (include/fhelin.h fhelin_encode): finite slot values, and max|v| * scale below 2^125 - tested on the exponents
// alone: floor(log2 max|v|) + floor(log2 scale) <= 123 guarantees it (each factor is below twice its power of two), needs no product
// that could round, and refuses everything that reaches 2^125.  reduce_i128_kernel takes |x| < 2^126 and x87_mul_round < 2^127; a
// coefficient is an average of slot values, so max|v| bounds it up to the FFT's rounding.  A NaN or an infinity would reach the
// rounding code as exponent 0x7FF (device) or as (u64)floorl(NaN) (host) and leave arbitrary residues.
void encode_domain_check(double max_abs, long double scale) {
    if (!std::isfinite(max_abs)) throw Error(FHELIN_ERR_ARG, "encode: a slot value is NaN or infinite");
    if (!(scale > 0) || !std::isfinite(scale)) throw Error(FHELIN_ERR_ARG, "encode: the scale must be positive and finite");
    if (max_abs != 0.0 && std::ilogb(max_abs) + std::ilogb(scale) > 123)
        throw Error(FHELIN_ERR_ARG, "encode: max|value| * scale may reach 2^125 (floor(log2 max|value|) + floor(log2 scale) > 123)");
}

void encode_batch_device(Context& c, u64* dst, const double* re, const double* im, int n_vec, int n_per, int slots, int ell, long double scale,
                         int stride, int lanes, int ell_q) {
    c.require_device();
    if (slots < 2 || (slots & (slots - 1)) || slots > c.N / 2) throw Error(FHELIN_ERR_ARG, "encode: slots must be a power of two in [2, N/2]");
    if (stride < 1 || (stride & (stride - 1)) || (long)slots * stride > c.N / 2 || (lanes != 1 && lanes != stride))
        throw Error(FHELIN_ERR_ARG, "encode: the interleaved packing (slots x stride) must be a power of two <= N/2");
    // ell = L + 1 + k: the encoding over the FULL key basis (limb ids 0..L+k: Q limbs, then the special limbs), for plaintexts
    // folded into rotation keys (Evaluator::folded_key); the leveled operations only ever ask for ell <= L + 1
    if (ell < 1 || ell > c.L + 1 + c.K) throw Error(FHELIN_ERR_ARG, "encode: level out of range");
    if (ell_q && (ell_q < 1 || ell_q > c.L + 1 || ell != ell_q + c.K)) throw Error(FHELIN_ERR_ARG, "encode: limb split out of range");
    if (n_vec < 1) return;
    const size_t words = (size_t)2 * slots;                 // one complex vector, in doubles
    const int n_staged = n_vec * lanes;                     // interleaved samples: re / im [n_vec][lanes][n_per], uploads at logical size
    Scratch<double> dv = c.scratch<double>(words * n_staged);
    std::vector<u64> host(words);
    for (int b = 0; b < n_staged; ++b) {                    // through the pinned staging ring: no stream drain
        double* h = reinterpret_cast<double*>(host.data());
        double mx = 0.0;                                    // the encoder's domain (encode_domain_check), on the values as they pass
        for (int i = 0; i < slots; ++i) {
            const double x = i < n_per ? re[(size_t)b * n_per + i] : 0.0;
            const double y = (im && i < n_per) ? im[(size_t)b * n_per + i] : 0.0;
            h[2 * i] = x;
            h[2 * i + 1] = y;
            const double ax = std::fabs(x), ay = std::fabs(y);
            if (ax > mx || ax != ax) mx = ax;               // a NaN takes over mx and stays: nothing compares greater than it
            if (ay > mx || ay != ay) mx = ay;
        }
        encode_domain_check(mx, scale);
        c.upload_async(reinterpret_cast<u64*>(dv.get()) + words * b, host.data(), words);
    }
    if (stride > 1) {   // the staged vectors are logical: the physical ones are made on the device, in front of the FFT
        Scratch<double> phys = c.scratch<double>(words * stride * n_vec);
        launch_interleave_slots(phys, dv, slots, stride, lanes, n_vec, c.stream);
        encode_complex_on_device(c, dst, phys, n_vec, slots * stride, ell, scale, ell_q);
        return;
    }
    encode_complex_on_device(c, dst, dv, n_vec, slots, ell, scale, ell_q);
}

// dv [n_vec][slots][2] complex slot values already on the device (overwritten) -> dst [n_vec][ell][N] encodings, NTT form
void encode_complex_on_device(Context& c, u64* dst, double* dv, int n_vec, int slots, int ell, long double scale, int ell_q) {
    const Context::FftDev& tab = fft_dev_tables(c, slots);
    launch_fft_special_inv(dv, tab.rot, tab.ksi, slots, n_vec, c.stream);
    // scale = mant * 2^exp with a 64-bit significand, exactly (the host code multiplies in x87 extended precision)
    int e2 = 0;
    const long double m = frexpl(scale, &e2);               // scale = m * 2^e2, m in [0.5, 1)
    const u64 mant = (u64)ldexpl(m, 64);
    c.stats.encode += (u64)n_vec;
    if (ell_q) {    // rows = the limbs a key switch at ell_q limbs reads: the forward transform takes their ids from the level's table
        launch_encode_round_reduce_split(c.dt, dst, dv, slots, ell_q, c.K, c.L + 1, mant, e2 - 64, n_vec, c.stream);
        c.ntt(LimbBatch{dst, n_vec * ell, c.lvl[ell_q].key_limb_tab, 0, 1, nullptr, ell}, false);
    } else {
        launch_encode_round_reduce(c.dt, dst, dv, slots, ell, mant, e2 - 64, n_vec, c.stream);
        c.ntt(LimbBatch{dst, n_vec * ell, nullptr, 0, ell}, false);
    }
    hip_check(hipGetLastError(), "encode kernels (device)");
}

std::shared_ptr<Encoding> encode_to_device(Context& c, const std::vector<double>& values, const std::vector<double>& imag, int slots,
                                           int ell, long double scale, int stride, int ell_q) {
    c.require_device();
    if (stride > 1 && (c.host_encode || slots < 2)) {   // the host encoder takes the physical vector: every value in all of its lanes
        if ((long)slots * stride > c.N / 2) throw Error(FHELIN_ERR_ARG, "encode: slots x stride must be <= N/2");
        std::vector<double> re((size_t)slots * stride, 0.0), im(imag.empty() ? 0 : (size_t)slots * stride, 0.0);
        for (int i = 0; i < slots && i < (int)values.size(); ++i)
            for (int k = 0; k < stride; ++k) re[(size_t)i * stride + k] = values[i];
        for (int i = 0; i < slots && i < (int)imag.size(); ++i)
            for (int k = 0; k < stride; ++k) im[(size_t)i * stride + k] = imag[i];
        return encode_to_device(c, re, im, slots * stride, ell, scale, 1, ell_q);
    }
    if (slots < 1 || (slots & (slots - 1)) || slots > c.N / 2) throw Error(FHELIN_ERR_ARG, "encode: slots must be a power of two <= N/2");
    if (ell < 1 || ell > c.L + 1 + c.K) throw Error(FHELIN_ERR_ARG, "encode: level out of range");   // L + 1 + k: full key basis (see above)
    if (ell_q && (ell_q < 1 || ell_q > c.L + 1 || ell != ell_q + c.K)) throw Error(FHELIN_ERR_ARG, "encode: limb split out of range");
    if (!c.host_encode && slots >= 2) {
        auto e = std::make_shared<Encoding>();
        e->ctx = &c;
        e->ell = ell;
        e->ell_q = ell_q;
        e->scale = scale;
        e->d = c.dalloc<u64>((size_t)ell * c.N);
        std::vector<double> re(slots, 0.0), im(slots, 0.0);
        for (int i = 0; i < slots && i < (int)values.size(); ++i) re[i] = values[i];
        for (int i = 0; i < slots && i < (int)imag.size(); ++i) im[i] = imag[i];
        encode_batch_device(c, e->d, re.data(), imag.empty() ? nullptr : im.data(), 1, slots, slots, ell, scale, stride, 1, ell_q);
        return e;
    }
    std::vector<std::pair<double, double>> v(slots, {0.0, 0.0});
    for (int i = 0; i < slots && i < (int)values.size(); ++i) v[i].first = values[i];
    for (int i = 0; i < slots && i < (int)imag.size(); ++i) v[i].second = imag[i];
    ckks_fft_special(v, true);
    const size_t N = c.N;
    const size_t gap = (N / 2) / slots;
    std::vector<u64> coeffs(2 * N, 0);
    for (int i = 0; i < slots; ++i) {
        ld_to_i128((long double)v[i].first * scale, coeffs[2 * (i * gap)], coeffs[2 * (i * gap) + 1]);
        ld_to_i128((long double)v[i].second * scale, coeffs[2 * (i * gap + N / 2)], coeffs[2 * (i * gap + N / 2) + 1]);
    }
    Scratch<u64> dco = c.scratch<u64>(2 * N);
    c.upload_async(dco, coeffs.data(), 2 * N);  // pinned staging: no stream drain (the GPU keeps its queue)
    auto e = std::make_shared<Encoding>();
    e->ctx = &c;
    e->ell = ell;
    e->ell_q = ell_q;
    e->scale = scale;
    e->d = c.dalloc<u64>((size_t)ell * N);
    c.stats.encode += 1;
    if (ell_q) {
        launch_reduce_i128(c.dt, e->d, dco, 0, ell_q, c.stream);
        if (c.K > 0) launch_reduce_i128(c.dt, e->d + (size_t)ell_q * N, dco, c.L + 1, c.K, c.stream);
        c.ntt(LimbBatch{e->d, ell, c.lvl[ell_q].key_limb_tab, 0, 1, nullptr, ell}, false);
    } else {
        launch_reduce_i128(c.dt, e->d, dco, 0, ell, c.stream);
        c.ntt(LimbBatch{e->d, ell, nullptr, 0, ell}, false);
    }
    hip_check(hipGetLastError(), "encode kernels");
    return e;
}

std::shared_ptr<Encoding> Plaintext::at_sliced(int ell_q, long double scale) {
    if (ell_q < 1 || ell_q > ctx->L + 1) throw Error(FHELIN_ERR_ARG, "encode: limb split out of range");
    return at(ell_q + ctx->K, scale, ell_q);
}

std::shared_ptr<Encoding> Plaintext::at(int ell, long double scale, int ell_q) {
    // an encoding is made on the stream that first asks for it; a DIFFERENT lane that uses it later orders its stream behind the event
    // recorded after the encode (no host wait: with two lanes fed by one host thread a host-side synchronisation of one lane starves the
    // other - 2.9 s of host time per 16 samples before this, tools: FHELIN_HOST_WAITS=1)
    auto order = [&](const std::shared_ptr<Encoding>& e) {
        const int lane = ctx->pool.cur_lane;
        if (e->ready && lane != e->made_lane && !(e->lanes_ordered & (1u << lane))) {
            hip_check(hipStreamWaitEvent(ctx->stream, e->ready, 0), "hipStreamWaitEvent(encoding)");
            e->lanes_ordered |= 1u << lane;
        }
    };
    // the encodings over the full key basis (ell = L + 1 + k, fhelin_hoisted_dot's folded keys) are asked for at a level's exact scale:
    // matched exactly, since neighbouring levels' scales can lie within 1e-12 of each other (~60-bit scaling primes)
    // ... and so are the limb-sliced ones (ell_q > 0: the same residues on the rows present), which never match a plain encoding of as many rows
    const bool full = ell > ctx->L + 1 || ell_q > 0;
    for (size_t i = 0; i < cache.size(); ++i)
        if (cache[i]->ell == ell && cache[i]->ell_q == ell_q && (full ? cache[i]->scale == scale : fabsl(cache[i]->scale / scale - 1.0L) < 1e-12L)) {
            if (i) std::rotate(cache.begin(), cache.begin() + i, cache.begin() + i + 1);   // most recently used first
            order(cache[0]);
            return cache[0];
        }
    auto sync_all = [&]() {
        hip_check(hipStreamSynchronize(ctx->main_stream), "encoding eviction sync");
        for (int k = 1; k <= ctx->n_lanes; ++k) hip_check(hipStreamSynchronize(ctx->lane_stream[k]), "encoding eviction sync (lane)");
    };
    if (fixed) throw Error(FHELIN_ERR_STATE, "a plaintext made from residues holds one encoding only: asked for another limb count or scale");
    std::shared_ptr<Encoding> e;
    if (shared)   // an earlier handle of the same values has made exactly this encoding: nothing to launch
        for (size_t i = 0; i < shared->cache.size() && !e; ++i)
            if (shared->cache[i]->ell == ell && shared->cache[i]->ell_q == ell_q && shared->cache[i]->scale == scale) {
                if (i) std::rotate(shared->cache.begin(), shared->cache.begin() + i, shared->cache.begin() + i + 1);
                e = shared->cache[0];
                order(e);
            }
    if (!e) {
        encode_domain_check(max_abs, scale);   // before anything is launched: a refused encoding leaves the plaintext and its cache as they were
        e = encode_to_device(*ctx, values, imag, slots, ell, scale, stride, ell_q);
        e->made_lane = ctx->pool.cur_lane;
        e->lanes_ordered = 1u << e->made_lane;
        if (ctx->n_lanes > 0) {
            hip_check(hipEventCreateWithFlags(&e->ready, hipEventDisableTiming), "hipEventCreate(encoding)");
            hip_check(hipEventRecord(e->ready, ctx->stream), "hipEventRecord(encoding)");
        }
        if (shared) {
            shared->cache.insert(shared->cache.begin(), e);
            if (shared->cache.size() > MAX_SHARED_ENCODINGS) {   // as below: the copy that goes may still be read by work in flight
                sync_all();
                shared->cache.pop_back();
            }
        }
    }
    cache.insert(cache.begin(), e);
    // one entry per (limb count, scale) the plaintext has been used at: bounded by the chain length in principle, capped here
    // so that a long-lived mask or bootstrap diagonal cannot pin more than MAX_ENCODINGS device copies (least recently used
    // goes; callers hold their own reference while they enqueue work on it)
    if (cache.size() > MAX_ENCODINGS) {
        // the evicted copy may still be read by work in flight on any stream: its block must not go back to a pool before that
        // work is done (rare: more than MAX_ENCODINGS distinct levels for one plaintext)
        sync_all();
        cache.pop_back();
    }
    return e;
}

// ------------------------------------------------------------------------------------------------ Client
Client::Client(Evaluator& ev, const uint8_t seed[32]) : ev_(ev), c_(ev.ctx()), rng_(seed) {}
Client::~Client() {
    try {
        if (s_all) c_.pool.free(s_all);
        if (s_sparse) c_.pool.free(s_sparse);
        if (pk) c_.pool.free(pk);
    } catch (...) {
    }
}

// sample a small polynomial on the host, reduce it into `nl` limbs on the GPU and transform to NTT form
void Client::draw_small_host(std::vector<u64>& co, int kind) {
    const size_t N = c_.N;
    co.resize(2 * N);
    for (size_t i = 0; i < N; ++i) {
        long v;
        if (kind == 0) v = lround(rng_.normal() * 3.19);
        else v = (long)(rng_.next() % 3) - 1;
        co[2 * i] = (u64)v;
        co[2 * i + 1] = v < 0 ? ~0ull : 0;
    }
}

void Client::sample_small_to_ntt(u64* dst, int nlimbs_q, bool with_p, int kind) {
    const size_t N = c_.N;
    std::vector<u64> co;
    draw_small_host(co, kind);
    Scratch<u64> dco = c_.scratch<u64>(2 * N);
    c_.upload_async(dco, co.data(), 2 * N);
    launch_reduce_i128(c_.dt, dst, dco, 0, nlimbs_q, c_.stream);
    launch_ntt(c_.dt, LimbBatch{dst, nlimbs_q, nullptr, 0, nlimbs_q}, false, c_.stream);
    if (with_p && c_.K > 0) {
        u64* dp = dst + (size_t)nlimbs_q * N;
        launch_reduce_i128(c_.dt, dp, dco, c_.L + 1, c_.K, c_.stream);
        launch_ntt(c_.dt, LimbBatch{dp, c_.K, nullptr, c_.L + 1, c_.K}, false, c_.stream);
    }
}

void Client::install_public_key(u64* d_pk, bool seeded) {
    if (pk) c_.pool.free(pk);
    pk = d_pk;
    pk_seeded_ = seeded;
    eval_only_ = true;
    c_.stride_locked = true;
}

void Client::place_sparse_ternary(std::vector<u64>& co, int h) {
    const size_t N = c_.N;
    int placed = 0;
    while (placed < h) {
        size_t pos = rng_.uniform(N);
        if (co[2 * pos] | co[2 * pos + 1]) continue;
        if (rng_.next() & 1) {
            co[2 * pos] = 1;
        } else {
            co[2 * pos] = ~0ull;
            co[2 * pos + 1] = ~0ull;
        }
        ++placed;
    }
}

void Client::keygen() {
    if (eval_only_) throw Error(FHELIN_ERR_KEY, "keygen: an evaluation context holds no secret and cannot make one");
    c_.require_device();
    keygen_run_ = true;
    c_.stride_locked = true;
    const size_t N = c_.N;
    const int L1 = c_.L + 1, nl = L1 + c_.K;
    // sparse ternary secret of Hamming weight h (reference SetSecretKeyDist(SPARSE_TERNARY), :8)
    std::vector<u64> co(2 * N, 0);
    place_sparse_ternary(co, std::min<int>(c_.prm.hamming, (int)N));
    if (seeded_keys_ && L1 > KEYGEN_MAX_Q) throw Error(FHELIN_ERR_ARG, "seeded keys: more than 64 Q limbs");
    if (seeded_keys_) {   // the public key-set seed: the next four words of the stream, bytes as begin_call
        for (int i = 0; i < 4; ++i) {
            const u64 w = rng_.next();
            for (int b = 0; b < 8; ++b) key_seed_[8 * i + b] = (uint8_t)(w >> (8 * b));
        }
        has_key_seed_ = true;
    }
    if (!s_all) s_all = c_.dalloc<u64>((size_t)nl * N);
    Scratch<u64> dco = c_.scratch<u64>(2 * N);
    hip_check(hipMemcpyAsync(dco, co.data(), 2 * N * 8, hipMemcpyHostToDevice, c_.stream), "secret upload");
    hip_check(hipStreamSynchronize(c_.stream), "secret sync");
    launch_reduce_i128(c_.dt, s_all, dco, 0, nl, c_.stream);
    launch_ntt(c_.dt, LimbBatch{s_all, nl, nullptr, 0, nl}, false, c_.stream);
    dco.reset();
    if (!pk) pk = c_.dalloc<u64>((size_t)2 * L1 * N);
    if (seeded_keys_) {
        // b = e - a s with a the expansion of (key-set seed, nonce of the public key) on the Q limbs, made in registers
        Scratch<u64> e = c_.scratch<u64>((size_t)L1 * N);
        sample_small_device(e, 1, L1, 0);
        c_.ntt(LimbBatch{e, L1, nullptr, 0, L1}, false);
        launch_seeded_keygen_combine(c_.dt, pk, s_all, nullptr, e, L1, 1, c_.alpha, L1, nullptr, key_seed_words(), 0, 0, c_.stream);
        hip_check(hipGetLastError(), "seeded keygen kernels");
        hip_check(hipMemsetAsync(e, 0, (size_t)L1 * N * sizeof(u64), c_.stream), "hipMemsetAsync(key noise)");
        e.reset();
        pk_seeded_ = true;
        return;
    }
    pk_seeded_ = false;
    // public key over Q: a uniform (sampled directly in NTT form), b = e - a s
    std::vector<u64> a((size_t)L1 * N);
    for (int l = 0; l < L1; ++l)
        for (size_t i = 0; i < N; ++i) a[(size_t)l * N + i] = rng_.uniform(c_.chain.q[l]);
    u64* pa = pk + (size_t)L1 * N;
    hip_check(hipMemcpyAsync(pa, a.data(), a.size() * 8, hipMemcpyHostToDevice, c_.stream), "pk upload");
    hip_check(hipStreamSynchronize(c_.stream), "pk sync");
    Scratch<u64> e = c_.scratch<u64>((size_t)L1 * N);
    sample_small_to_ntt(e, L1, false, 0);
    launch_ew_mul(c_.dt, pk, pa, s_all, L1, L1, 0, L1, c_.stream);
    launch_ew_sub(c_.dt, pk, e, pk, L1, L1, 0, L1, c_.stream);
    hip_check(hipGetLastError(), "keygen kernels");
}

SamplerKey Client::key_seed_words() const {
    SamplerKey k;
    for (int i = 0; i < 8; ++i)
        k.w[i] = (u32)key_seed_[4 * i] | ((u32)key_seed_[4 * i + 1] << 8) | ((u32)key_seed_[4 * i + 2] << 16) | ((u32)key_seed_[4 * i + 3] << 24);
    return k;
}

void Client::install_key_seed(const uint8_t seed[32]) {
    std::memcpy(key_seed_, seed, 32);
    has_key_seed_ = true;
}

void Client::set_key_caps(const std::vector<KeyCap>& table) {
    key_caps_.clear();
    for (const KeyCap& e : table) key_caps_[{e.kind, e.galois}] = e.max_ell;
}

int Client::key_cap(int kind, u64 galois) const {
    auto it = key_caps_.find({kind, galois});
    return it == key_caps_.end() ? c_.L + 1 : it->second;
}

// Level-capped keys (include/fhelin.h "Level-capped keys"): a key with an entry in the cap table is made with its present rows only - the
// Q limbs 0 .. cap-1 and the special limbs of the digits_at(cap) digits a switch at <= cap limbs reads - and those are, residue for
// residue, the rows of the key this call would have made uncapped: the generator and the device sampler are consumed exactly as for the
// uncapped key (so every later key is unchanged too), and only transforms, products and uploads of absent rows are left out.
KeyPtr Client::make_switch_key(const u64* s_from_all, const u64* s_to_all, u64 kind, u64 galois, int force_cap) {
    c_.require_device();
    if (c_.K < 1) throw Error(FHELIN_ERR_STATE, "key switching keys need special primes (n_p >= 1)");
    const size_t N = c_.N;
    const int L1 = c_.L + 1, nl = L1 + c_.K;
    const int cap = force_cap > 0 ? std::min(force_cap, L1) : key_cap((int)kind, galois), all_digits = c_.digits_at(L1);
    const bool capped = cap < L1;
    KeyPtr key = ev_.new_key(cap);
    key->kind = (int)kind;
    key->galois = galois;
    if (seeded_keys_) {
        if (!has_key_seed_) throw Error(FHELIN_ERR_STATE, "seeded keys: keygen() draws the key-set seed and has not run");
        if (L1 > KEYGEN_MAX_Q) throw Error(FHELIN_ERR_ARG, "seeded keys: more than 64 Q limbs");
        // every digit in one launch: e [digits][nl][N] from the device sampler, one forward NTT, then the fused combination.  A capped key
        // samples the same e (the sampler's stream positions depend on the shape) and transforms the present rows of its digits only
        const size_t en = (size_t)all_digits * nl * N;
        Scratch<u64> e = c_.scratch<u64>(en);
        sample_small_device(e, all_digits, nl, 0);
        if (!capped) c_.ntt(LimbBatch{e, all_digits * nl, nullptr, 0, nl}, false);
        else
            for (int j = 0; j < key->digits; ++j) {
                u64* ej = e + (size_t)j * nl * N;
                c_.ntt(LimbBatch{ej, cap, nullptr, 0, cap}, false);
                c_.ntt(LimbBatch{ej + (size_t)L1 * N, c_.K, nullptr, L1, c_.K}, false);
            }
        std::vector<u64> pm(L1);
        for (int t = 0; t < L1; ++t) {
            const u64 qt = c_.chain.q[t];
            u64 m = 1;
            for (u64 p : c_.chain.p) m = h_mulmod(m, p % qt, qt);
            pm[t] = m;
        }
        if (!capped)
            launch_seeded_keygen_combine(c_.dt, key->d, s_to_all, s_from_all, e, nl, key->digits, c_.alpha, L1, pm.data(), key_seed_words(), kind,
                                         galois, c_.stream);
        else
            launch_seeded_keygen_combine_capped(c_.dt, key->d, s_to_all, s_from_all, e, nl, key->digits, c_.alpha, L1, cap, pm.data(),
                                                key_seed_words(), kind, galois, c_.stream);
        hip_check(hipGetLastError(), "seeded keygen kernels");
        hip_check(hipMemsetAsync(e, 0, en * sizeof(u64), c_.stream), "hipMemsetAsync(key noise)");
        e.reset();
        key->seeded = true;
        return key;
    }
    std::vector<u64> a((size_t)nl * N);
    Scratch<u64> e = c_.scratch<u64>((size_t)nl * N);
    Scratch<u64> tmp = c_.scratch<u64>((size_t)nl * N);
    // the Q rows in use and where the special rows of e / tmp lie: a capped key keeps its noise and products dense, [cap + k][N]
    const int nq = capped ? cap : L1;
    for (int j = 0; j < all_digits; ++j) {
        for (int l = 0; l < nl; ++l) {
            const u64 m = c_.moduli[l];
            for (size_t i = 0; i < N; ++i) a[(size_t)l * N + i] = rng_.uniform(m);
        }
        if (j >= key->digits) {   // a digit the capped key does not hold: its draws are consumed, nothing is computed
            std::vector<u64> co;
            draw_small_host(co, 0);
            continue;
        }
        u64* kb = key->d + (size_t)(2 * j) * nl * N;
        u64* ka = key->d + (size_t)(2 * j + 1) * nl * N;
        if (!capped) {
            hip_check(hipMemcpyAsync(ka, a.data(), a.size() * 8, hipMemcpyHostToDevice, c_.stream), "evk upload");
        } else {
            hip_check(hipMemcpyAsync(ka, a.data(), (size_t)nq * N * 8, hipMemcpyHostToDevice, c_.stream), "evk upload");
            hip_check(hipMemcpyAsync(ka + (size_t)L1 * N, a.data() + (size_t)L1 * N, (size_t)c_.K * N * 8, hipMemcpyHostToDevice, c_.stream),
                      "evk upload");
        }
        hip_check(hipStreamSynchronize(c_.stream), "evk sync");
        sample_small_to_ntt(e, nq, true, 0);
        if (!capped) {
            launch_ew_mul(c_.dt, tmp, ka, s_to_all, nl, nl, 0, nl, c_.stream);
            launch_ew_sub(c_.dt, kb, e, tmp, nl, nl, 0, nl, c_.stream);
        } else {
            const size_t pq = (size_t)nq * N, pl = (size_t)L1 * N;   // special rows: dense in e / tmp, at row L1 in the key and the secrets
            launch_ew_mul(c_.dt, tmp, ka, s_to_all, nq, nq, 0, nq, c_.stream);
            launch_ew_sub(c_.dt, kb, e, tmp, nq, nq, 0, nq, c_.stream);
            launch_ew_mul(c_.dt, tmp + pq, ka + pl, s_to_all + pl, c_.K, c_.K, L1, c_.K, c_.stream);
            launch_ew_sub(c_.dt, kb + pl, e + pq, tmp + pq, c_.K, c_.K, L1, c_.K, c_.stream);
        }
        // + P * (Q/Q_j) * [(Q/Q_j)^{-1}]_{Q_j} * s_from  ==  (P mod q_t) * s_from on the limbs of digit j, 0 elsewhere
        const int lo = j * c_.alpha, hi = std::min((j + 1) * c_.alpha, nq);
        ScalarSet sc;
        for (int t = lo; t < hi; ++t) {
            const u64 qt = c_.chain.q[t];
            u64 pm = 1;
            for (u64 p : c_.chain.p) pm = h_mulmod(pm, p % qt, qt);
            sc.v[2 * (t - lo)] = pm;
            sc.v[2 * (t - lo) + 1] = h_shoup(pm, qt);
        }
        launch_ew_scalar(c_.dt, tmp, s_from_all + (size_t)lo * N, sc, hi - lo, lo, hi - lo, c_.stream);
        launch_ew_add(c_.dt, kb + (size_t)lo * N, kb + (size_t)lo * N, tmp, hi - lo, hi - lo, lo, hi - lo, c_.stream);
    }
    hip_check(hipGetLastError(), "make_switch_key kernels");
    return key;
}

void Client::gen_relin_key() {
    if (!s_all) {
        if (ev_.relin_key) return;   // without the secret: a key that is present is all this call can confirm
        throw Error(FHELIN_ERR_KEY, eval_only_ ? "relinearisation key not in the evaluation-key set" : "keygen() has not been called");
    }
    const int nl = c_.L + 1 + c_.K;
    Scratch<u64> s2 = c_.scratch<u64>((size_t)nl * c_.N);
    launch_ew_mul(c_.dt, s2, s_all, s_all, nl, nl, 0, nl, c_.stream);
    ev_.relin_key = make_switch_key(s2, s_all, 1, 0);
}

void Client::gen_rotation_key(int index) {
    const u64 g = c_.rot_element(index);   // a logical index (bootstrapping asks for its physical ones under a PhysicalScope)
    if (!s_all) {
        auto it = ev_.rot_keys.find(g);
        if (it != ev_.rot_keys.end() && it->second) return;
        throw Error(FHELIN_ERR_KEY, eval_only_ ? "rotation key for index " + std::to_string(index) + " not in the evaluation-key set"
                                              : "keygen() has not been called");
    }
    if (ev_.rot_keys.count(g)) return;
    const int nl = c_.L + 1 + c_.K;
    // key switches from s to sigma_{g^-1}(s); applying sigma_g afterwards restores s (oracle orc_rotate)
    const u64 ginv = c_.rot_element(-index);
    Scratch<u64> sp = c_.scratch<u64>((size_t)nl * c_.N);
    launch_automorph(c_.dt, sp, s_all, c_.automorph_map(ginv), nl, c_.stream);
    KeyPtr key = make_switch_key(s_all, sp, 2, g);
    key->has_index = true;
    key->index = index;
    ev_.rot_keys[g] = key;
}

void Client::gen_conj_key() {
    if (!s_all) {
        if (ev_.conj_key) return;
        throw Error(FHELIN_ERR_KEY, eval_only_ ? "conjugation key not in the evaluation-key set" : "keygen() has not been called");
    }
    const u64 g = 2ull * c_.N - 1;  // X -> X^{-1}; its own inverse
    const int nl = c_.L + 1 + c_.K;
    Scratch<u64> sp = c_.scratch<u64>((size_t)nl * c_.N);
    launch_automorph(c_.dt, sp, s_all, c_.automorph_map(g), nl, c_.stream);
    ev_.conj_key = make_switch_key(s_all, sp, 3, g);
    ev_.rot_keys[g] = ev_.conj_key;
}

void Client::gen_sparse_keys(int hamming) {
    if (!s_all) {
        const char* missing = !ev_.to_sparse_key ? "to-sparse key" : !ev_.from_sparse_key ? "from-sparse key" : nullptr;
        if (!missing) return;
        throw Error(FHELIN_ERR_KEY, eval_only_ ? std::string(missing) + " not in the evaluation-key set (it was saved without sparse-secret bootstrapping)"
                                              : "keygen() has not been called");
    }
    if (s_sparse && ev_.to_sparse_key && ev_.from_sparse_key) return;   // once per context, as the conjugation key
    const size_t N = c_.N;
    const int nl = c_.L + 1 + c_.K;
    if (hamming < 1 || hamming > (int)N) throw Error(FHELIN_ERR_ARG, "sparse-secret bootstrapping: Hamming weight outside 1 .. N");
    std::vector<u64> co(2 * N, 0);
    place_sparse_ternary(co, hamming);
    sparse_coeffs_.assign(N, 0);
    for (size_t i = 0; i < N; ++i) sparse_coeffs_[i] = co[2 * i + 1] ? -1 : (int8_t)co[2 * i];
    if (!s_sparse) s_sparse = c_.dalloc<u64>((size_t)nl * N);
    Scratch<u64> dco = c_.scratch<u64>(2 * N);
    hip_check(hipMemcpyAsync(dco, co.data(), 2 * N * 8, hipMemcpyHostToDevice, c_.stream), "sparse secret upload");
    hip_check(hipStreamSynchronize(c_.stream), "sparse secret sync");
    launch_reduce_i128(c_.dt, s_sparse, dco, 0, nl, c_.stream);
    launch_ntt(c_.dt, LimbBatch{s_sparse, nl, nullptr, 0, nl}, false, c_.stream);
    hip_check(hipMemsetAsync(dco, 0, 2 * N * sizeof(u64), c_.stream), "hipMemsetAsync(sparse secret staging)");
    dco.reset();
    // a switch from s to s~ encrypts s under s~ (s_from = s, s_to = s~), and back
    ev_.to_sparse_key = make_switch_key(s_all, s_sparse, 4, 0, 2);
    ev_.from_sparse_key = make_switch_key(s_sparse, s_all, 5, 0);
}

PtPtr Client::encode(const double* vals, int n, int level, int slots) {
    if (slots <= 0) slots = 1 << c_.prm.log_slots;
    if (slots & (slots - 1)) throw Error(FHELIN_ERR_ARG, "encode: slots must be a power of two");
    if (c_.stride > 1 && (long)slots * c_.stride > c_.N / 2) throw Error(FHELIN_ERR_ARG, "encode: slots x interleave stride must be <= N/2");
    if (level < 0 || level > c_.L) throw Error(FHELIN_ERR_ARG, "encode: level out of range");
    auto p = std::make_shared<Plaintext>();
    p->ctx = &c_;
    p->slots = slots;
    p->stride = c_.stride;
    c_.stride_locked = true;
    p->level = level;
    p->values.assign(slots, 0.0);
    double mx = 0.0;
    for (int i = 0; i < n && i < slots; ++i) {
        p->values[i] = vals[i];
        const double a = std::fabs(vals[i]);
        if (a > mx || a != a) mx = a;                       // a NaN takes over mx and stays: nothing compares greater than it
    }
    if (!std::isfinite(mx)) throw Error(FHELIN_ERR_ARG, "encode: a slot value is NaN or infinite");
    p->max_abs = mx;
    return p;
}

void Client::sample_small_device(u64* dst, int n_poly, int ell, int kind) {
    SamplerKey key;   // a fresh ChaCha20 key per call, drawn from the client's own (secret-seeded) stream
    for (int i = 0; i < 4; ++i) {
        const u64 w = rng_.next();
        key.w[2 * i] = (u32)w;
        key.w[2 * i + 1] = (u32)(w >> 32);
    }
    launch_sample_small(c_.dt, dst, key, (sample_calls_++) << 32, kind, ell, n_poly, c_.stream);
}

SamplerKey Client::draw_sampler_key() {
    SamplerKey key;   // as sample_small_device: a fresh ChaCha20 key per call from the context's own generator
    for (int i = 0; i < 4; ++i) {
        const u64 w = rng_.next();
        key.w[2 * i] = (u32)w;
        key.w[2 * i + 1] = (u32)(w >> 32);
    }
    return key;
}

void Client::debug_sampler_peek(int n_keys, u32* key_words, u64* sample_calls) const {
    Prng copy = rng_;   // the draws below advance the copy only
    for (int k = 0; k < n_keys; ++k)
        for (int i = 0; i < 4; ++i) {   // as draw_sampler_key
            const u64 w = copy.next();
            key_words[8 * k + 2 * i] = (u32)w;
            key_words[8 * k + 2 * i + 1] = (u32)(w >> 32);
        }
    if (sample_calls) *sample_calls = sample_calls_;
}

void Client::sample_flood_device(u64* dst, int n_poly, int ell, int flood_bits, bool gauss) {
    const SamplerKey key = draw_sampler_key();
    const u64 flood_stream = (sample_calls_++) << 32, gauss_stream = (sample_calls_++) << 32;   // two distinct stream ranges
    launch_sample_flood(c_.dt, dst, key, flood_stream, gauss_stream, flood_bits, gauss, ell, n_poly, c_.stream);
}

void Client::check_flood(int flood_bits, int nl, const char* who) const {
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, std::string(who) + ": flood_bits must lie in [0, 62]");
    long double bits = 0;
    for (int l = 0; l < nl; ++l) bits += log2l((long double)c_.chain.q[l]);
    if (flood_bits > 0 && !((long double)(flood_bits + 2) < bits))
        throw Error(FHELIN_ERR_ARG, std::string(who) + ": 2^(flood_bits + 2) must stay below the product of the limbs kept");
}

std::vector<u64> Client::debug_flood(const uint8_t key[32], u64 stream, int flood_bits, int ell) {
    c_.require_device();
    if (flood_bits < 1 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "debug_flood: flood_bits must lie in [1, 62]");
    if (ell < 1 || ell > c_.L + 1) throw Error(FHELIN_ERR_ARG, "debug_flood: limb count out of range");
    SamplerKey k;
    for (int i = 0; i < 8; ++i)
        k.w[i] = (u32)key[4 * i] | ((u32)key[4 * i + 1] << 8) | ((u32)key[4 * i + 2] << 16) | ((u32)key[4 * i + 3] << 24);
    const size_t n = (size_t)ell * c_.N;
    Scratch<u64> d = c_.scratch<u64>(n);
    launch_sample_flood(c_.dt, d, k, stream, 0, flood_bits, false, ell, 1, c_.stream);
    hip_check(hipGetLastError(), "flood sampler");
    std::vector<u64> h(n);
    hip_check(hipMemcpyAsync(h.data(), d, n * 8, hipMemcpyDeviceToHost, c_.stream), "flood download");
    hip_check(hipStreamSynchronize(c_.stream), "flood sync");
    return h;
}

std::vector<CtPtr> Client::sanitize(const std::vector<CtPtr>& vin, const PtPtr& mask, int flood_bits, int out_ell) {
    Context& c = c_;
    c.require_device();
    if (!pk) throw Error(FHELIN_ERR_KEY, "sanitize: the context holds no public key (keygen, or an evaluation-key set)");
    if (out_ell <= 0) out_ell = 2;
    if (out_ell > c.L + 1) throw Error(FHELIN_ERR_ARG, "sanitize: out_ell above the chain's limbs");
    check_flood(flood_bits, out_ell, "sanitize");
    // every refusal before any device work
    for (const CtPtr& ct : vin) {
        if (!ct || ct->wrapped()) throw Error(FHELIN_ERR_ARG, "sanitize: a wrapped input ciphertext is not a result");
        if (ct->npoly != 2) throw Error(FHELIN_ERR_ARG, "sanitize: a 3-component ciphertext must be relinearised first");
        const int left = ct->ell - std::max(0, ct->deg - 1) - (mask ? 1 : 0);
        if (left < out_ell) throw Error(FHELIN_ERR_ARG, "sanitize: too few limbs for the rescale, the mask and out_ell");
    }
    std::vector<CtPtr> x = vin;
    auto rescale_where = [&](int min_deg) {   // batched, every ciphertext above degree 1 (as decrypt rescales its input)
        for (;;) {
            std::vector<CtPtr> need;
            std::vector<size_t> at;
            for (size_t i = 0; i < x.size(); ++i)
                if (x[i]->deg >= min_deg) {
                    need.push_back(x[i]);
                    at.push_back(i);
                }
            if (need.empty()) return;
            std::vector<CtPtr> r = ev_.rescale_batch(need);
            for (size_t k = 0; k < at.size(); ++k) x[at[k]] = r[k];
        }
    };
    rescale_where(2);
    if (mask) {
        x = ev_.mult_plain_batch(x, mask);
        rescale_where(2);
    }
    const size_t N = c.N, pn = (size_t)out_ell * N;
    const int L1 = c.L + 1;
    std::vector<CtPtr> out;
    const int CHUNK = 32;                                    // bounds the temporaries (3 polynomials per ciphertext in flight)
    for (size_t lo = 0; lo < x.size(); lo += CHUNK) {
        const int n = (int)std::min<size_t>(CHUNK, x.size() - lo);
        std::vector<CtPtr> cts = ev_.new_ct_batch(n, 2, out_ell, 1, x[lo]->scale, x[lo]->slots);
        std::vector<RerandItem> tab(n);
        for (int b = 0; b < n; ++b) {
            const Ciphertext& in = *x[lo + b];
            cts[b]->scale = in.scale;
            cts[b]->slots = in.slots;
            tab[b].in = in.d;
            tab[b].out = cts[b]->d;
            tab[b].in_ell = in.ell;
        }
        Scratch<RerandItem> d_tab = c.scratch<RerandItem>((size_t)n);
        hip_check(hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(RerandItem), hipMemcpyHostToDevice, c.stream), "sanitize item table");
        Scratch<u64> rnd = c.scratch<u64>((size_t)3 * n * pn);           // u | e0 + f | e1, each [n][out_ell][N]
        sample_small_device(rnd, n, out_ell, 1);
        if (flood_bits > 0) sample_flood_device(rnd + (size_t)n * pn, n, out_ell, flood_bits, true);
        else sample_small_device(rnd + (size_t)n * pn, n, out_ell, 0);
        sample_small_device(rnd + (size_t)2 * n * pn, n, out_ell, 0);
        c.ntt(LimbBatch{rnd, 3 * n * out_ell, nullptr, 0, out_ell}, false);
        launch_rerandomize_combine(c.dt, d_tab, pk, rnd, rnd + (size_t)n * pn, rnd + (size_t)2 * n * pn, out_ell, L1, n, c.stream);
        hip_check(hipGetLastError(), "sanitize kernels");
        // the randomness (u, e0 + f, e1) does not stay behind in a recycled pool block
        hip_check(hipMemsetAsync(rnd, 0, (size_t)3 * n * pn * sizeof(u64), c.stream), "hipMemsetAsync(sanitize randomness)");
        rnd.reset();
        for (auto& ct : cts) out.push_back(ct);
    }
    return out;
}

std::vector<long> Client::debug_sample(int kind, int n_poly) {
    c_.require_device();
    const size_t N = c_.N;
    Scratch<u64> d = c_.scratch<u64>((size_t)n_poly * N);
    sample_small_device(d, n_poly, 1, kind);
    std::vector<u64> h((size_t)n_poly * N);
    hip_check(hipMemcpyAsync(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost, c_.stream), "sample download");
    hip_check(hipStreamSynchronize(c_.stream), "sample sync");
    d.reset();
    const u64 q0 = c_.chain.q[0];
    std::vector<long> out(h.size());
    for (size_t i = 0; i < h.size(); ++i) out[i] = h[i] > q0 / 2 ? -(long)(q0 - h[i]) : (long)h[i];
    return out;
}

void Client::set_seeded(bool on) {
    if (on && eval_only_) throw Error(FHELIN_ERR_KEY, "seeded encryption needs the secret key: an evaluation context holds none");
    seeded_ = on;
}

void Client::begin_call() {
    if (!seeded_) return;
    for (int i = 0; i < 4; ++i) {   // a fresh public seed per call, drawn from the client's own stream
        const u64 w = rng_.next();
        for (int b = 0; b < 8; ++b) call_seed_[8 * i + b] = (uint8_t)(w >> (8 * b));
    }
}

// c0 = b u + e0 + m, c1 = a u + e1 for n_vec encodings enc [n_vec][ell][N] (stride enc_stride words; 0 = one shared encoding);
// seeded mode: c0 = m - a s + e, c1 = a with a the expansion of (call seed, nonces[b])
void Client::encrypt_encoded(const u64* enc, size_t enc_stride, int n_vec, int ell, long double scale, int slots, std::vector<CtPtr>& out,
                             const u64* nonces) {
    Context& c = c_;
    const size_t N = c.N, pn = (size_t)ell * N;
    const int L1 = c.L + 1;
    std::vector<CtPtr> cts = ev_.new_ct_batch(n_vec, 2, ell, 1, scale, slots);
    if (seeded_) {
        if (!s_all) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
        SamplerKey key;
        for (int i = 0; i < 8; ++i)
            key.w[i] = (u32)call_seed_[4 * i] | ((u32)call_seed_[4 * i + 1] << 8) | ((u32)call_seed_[4 * i + 2] << 16) |
                       ((u32)call_seed_[4 * i + 3] << 24);
        Scratch<u64> e = c.scratch<u64>((size_t)n_vec * pn);              // e [n_vec][ell][N]
        sample_small_device(e, n_vec, ell, 0);
        c.ntt(LimbBatch{e, n_vec * ell, nullptr, 0, ell}, false);
        launch_sk_encrypt_combine(c.dt, cts[0]->d, s_all, e, enc, enc_stride, ell, key, nonces, n_vec, c.stream);
        hip_check(hipGetLastError(), "secret-key encrypt kernels");
        // the encryption noise does not stay behind in a recycled pool block
        hip_check(hipMemsetAsync(e, 0, (size_t)n_vec * pn * sizeof(u64), c.stream), "hipMemsetAsync(encryption noise)");
        e.reset();
        for (int b = 0; b < n_vec; ++b) {
            cts[b]->seeded = true;
            cts[b]->nonce = nonces[b];
            std::memcpy(cts[b]->seed, call_seed_, 32);
        }
        for (auto& ct : cts) out.push_back(ct);
        return;
    }
    Scratch<u64> rnd = c.scratch<u64>((size_t)3 * n_vec * pn);       // u | e0 | e1, each [n_vec][ell][N]
    sample_small_device(rnd, n_vec, ell, 1);
    sample_small_device(rnd + (size_t)n_vec * pn, 2 * n_vec, ell, 0);
    c.ntt(LimbBatch{rnd, 3 * n_vec * ell, nullptr, 0, ell}, false);
    launch_encrypt_combine(c.dt, cts[0]->d, pk, rnd, rnd + (size_t)n_vec * pn, rnd + (size_t)2 * n_vec * pn, enc, ell, L1, enc_stride, n_vec,
                           c.stream);
    hip_check(hipGetLastError(), "encrypt kernels");
    // the encryption randomness (u, e0, e1) does not stay behind in a recycled pool block
    hip_check(hipMemsetAsync(rnd, 0, (size_t)3 * n_vec * pn * sizeof(u64), c.stream), "hipMemsetAsync(encryption randomness)");
    rnd.reset();
    for (auto& ct : cts) out.push_back(ct);
}

CtPtr Client::encrypt(const PtPtr& p, int drop) {
    if (seeded_ ? !s_all : !pk) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    const int level = std::min(c_.L, p->level + std::max(0, drop));   // level plan: start `drop` limbs lower
    const int ell = c_.L + 1 - level;
    auto enc = p->at(ell, c_.sf_real[level]);
    std::vector<CtPtr> out;
    begin_call();
    const u64 nonce = 0;
    encrypt_encoded(enc->d, 0, 1, ell, enc->scale, p->slots, out, &nonce);
    return out[0];
}

std::vector<CtPtr> Client::encrypt_batch(const double* vals, int n_vec, int n_per, int level, int slots, const int* nonce_of, bool per_lane) {
    if (seeded_ ? !s_all : !pk) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    if (slots <= 0) slots = 1 << c_.prm.log_slots;
    // interleaved samples: every vector replicated into all lanes, or (per_lane) vals [n_vec][stride][n_per], one vector per sample
    const int lanes = per_lane ? c_.stride : 1;
    if (level < 0 || level > c_.L) throw Error(FHELIN_ERR_ARG, "encrypt: level out of range");
    if (n_vec < 0 || n_per < 0) throw Error(FHELIN_ERR_ARG, "encrypt_batch: negative count");
    const int ell = c_.L + 1 - level;
    const size_t pn = (size_t)ell * c_.N;
    const long double scale = c_.sf_real[level];
    std::vector<CtPtr> out;
    if (!nonce_of) begin_call();
    const int CHUNK = 32;                                    // bounds the temporaries (4 polynomials per vector in flight)
    for (int lo = 0; lo < n_vec; lo += CHUNK) {
        const int n = std::min(CHUNK, n_vec - lo);
        Scratch<u64> enc = c_.scratch<u64>((size_t)n * pn);
        encode_batch_device(c_, enc, vals + (size_t)lo * lanes * n_per, nullptr, n, n_per, slots, ell, scale, c_.stride, lanes);
        u64 nonces[CHUNK];
        for (int k = 0; k < n; ++k) nonces[k] = nonce_of ? (u64)nonce_of[lo + k] : (u64)(lo + k);
        encrypt_encoded(enc, pn, n, ell, scale, slots, out, nonces);
    }
    return out;
}

// Wrapped inputs, the parts ingest_sample and ingest_interleaved share.  wrap_groups: groups of <= 128 inputs that share a target, in read
// order (runs of one target follow its first input); group_ell per wrapped vector: the inputs' limbs; pos [n_w][128] input positions
// (-1 = none).
void Client::wrap_groups(const std::vector<int>& wrap_ell, int n_vec, std::vector<int>& group_ell, std::vector<int>& pos) const {
    if ((int)wrap_ell.size() != n_vec) throw Error(FHELIN_ERR_ARG, "ingest: one target per input");
    for (int v : wrap_ell)
        if (v < 1 || v > c_.L + 1) throw Error(FHELIN_ERR_ARG, "ingest: wrapped target limbs out of range [1, n_q]");
    std::vector<char> taken(n_vec, 0);
    for (int i = 0; i < n_vec; ++i) {
        if (taken[i]) continue;
        int t = 128;
        for (int j = i; j < n_vec; ++j) {
            if (taken[j] || wrap_ell[j] != wrap_ell[i]) continue;
            if (t == 128) {
                group_ell.push_back(wrap_ell[i]);
                pos.resize(pos.size() + 128, -1);
                t = 0;
            }
            pos[pos.size() - 128 + t++] = j;
            taken[j] = 1;
        }
    }
}

// encrypt_wrapped: dv [n_w][phys] complex (phys = slots x the interleave stride) -> the wrapped ciphertexts.  Seeded secret-key encryption
// over the first ell + 1 moduli of Q then P at the scale of a fresh encryption at ell limbs; wrapped vectors of one target are
// consecutive (wrap_groups) and share the batched encoder and encryptor.  get: the caller's wiped temporaries.
std::vector<CtPtr> Client::encrypt_wrapped(double* dv, int phys, int slots, int n_vec, const std::vector<int>& group_ell,
                                           const std::vector<int>& pos, const std::function<void*(size_t)>& get) {
    struct SeededMode {
        bool& f;
        bool was;
        ~SeededMode() { f = was; }
    } mode{seeded_, seeded_};
    seeded_ = true;
    begin_call();
    const int n_w = (int)group_ell.size();
    std::vector<CtPtr> out;
    for (int w0 = 0; w0 < n_w;) {
        const int ell = group_ell[w0], ell1 = ell + 1;
        int n = 0;
        while (w0 + n < n_w && n < 32 && group_ell[w0 + n] == ell) ++n;
        const size_t pn = (size_t)ell1 * c_.N;
        const long double scale = c_.sf_real[c_.L + 1 - ell];
        u64* enc = (u64*)get((size_t)n * pn * sizeof(u64));
        encode_complex_on_device(c_, enc, dv + (size_t)w0 * phys * 2, n, phys, ell1, scale);
        std::vector<CtPtr> part;
        u64 nonces[32];
        for (int k = 0; k < n; ++k) nonces[k] = (u64)(w0 + k);
        encrypt_encoded(enc, pn, n, ell1, scale, slots, part, nonces);
        for (int k = 0; k < n; ++k) {
            Ciphertext& ct = *part[k];
            for (int t = 0; t < 128 && pos[(size_t)(w0 + k) * 128 + t] >= 0; ++t) ct.wrap_pos.push_back(pos[(size_t)(w0 + k) * 128 + t]);
            ct.wrap_total = n_vec;
            out.push_back(part[k]);
        }
        w0 += n;
    }
    return out;
}

// One sample's client side on the device (kernels_client.h "sample ingestion"): embedding rows (given, or gathered from a table by
// token id) + positional embedding, the two Linformer projections, the expanded packing, encoding and encryption.  drop[v]:
// limbs vector v starts lower by (level plan); vectors of one level share the batched encryptor.
std::vector<CtPtr> Client::ingest_sample(const double* emb, const int* tokens, const double* table, int vocab, int S, const double* cls,
                                         const double* pos, const double* E_w, const double* E_b, const double* F_w, const double* F_b,
                                         int w_cols, int level, const std::vector<int>& drop, std::vector<double>* proj_out,
                                         const std::vector<int>* wrap_ell) {
    if (wrap_ell && eval_only_) throw Error(FHELIN_ERR_KEY, "wrapped inputs are secret-key encryptions: an evaluation context holds no secret");
    if ((seeded_ || wrap_ell) ? !s_all : !pk) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    const int slots = 1 << c_.prm.log_slots, S1 = S + 1, n_vec = 64 + S1;
    if (c_.stride > 1) throw Error(FHELIN_ERR_STATE, "ingest: a context with interleaved samples takes its samples through ingest_interleaved");
    if (slots != 16384) throw Error(FHELIN_ERR_ARG, "ingest: the expanded layout needs 16384 slots (128 x 128)");
    if (S < 1 || S1 > w_cols || (!emb && !(tokens && table && vocab > 0))) throw Error(FHELIN_ERR_ARG, "ingest: bad token count / inputs");
    if (level < 0 || level > c_.L || (int)drop.size() != n_vec) throw Error(FHELIN_ERR_ARG, "ingest: level out of range");
    std::vector<int> wrap_group_ell, wrap_pos;   // per wrapped vector: the inputs' limbs; [n_w][128] input positions (-1 = none)
    if (wrap_ell) wrap_groups(*wrap_ell, n_vec, wrap_group_ell, wrap_pos);
    hipStream_t s = c_.stream;
    // every temporary of the sample - the embeddings, x_in, the projections, the expanded packing: the client's PLAINTEXT - is wiped
    // before its block goes back to the recycled pool, and freed on every path out of this function (an exception included)
    struct Temps {
        Context& c;
        hipStream_t s;
        std::vector<std::pair<Scratch<char>, size_t>> blocks;
        void* get(size_t bytes) {
            blocks.emplace_back(c.scratch<char>(bytes), bytes);
            return blocks.back().first.get();
        }
        ~Temps() {   // the wipes are queued first; the blocks' owners free them behind
            for (auto& b : blocks) (void)hipMemsetAsync(b.first.get(), 0, b.second, s);
        }
    } tmp{c_, s, {}};
    auto up = [&](const void* h, size_t bytes) {
        void* d = tmp.get(bytes);
        hip_check(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "ingest upload");
        return d;
    };
    if (tokens)
        for (int t = 0; t < S; ++t)
            if (tokens[t] < 0 || tokens[t] >= vocab) throw Error(FHELIN_ERR_ARG, "ingest: token id outside the embedding table");
    double* d_emb = emb ? (double*)up(emb, (size_t)S * 128 * 8) : nullptr;
    int* d_tok = tokens ? (int*)up(tokens, (size_t)S * 4) : nullptr;
    double* d_tab = tokens ? (double*)up(table, (size_t)vocab * 128 * 8) : nullptr;
    double* d_cls = (double*)up(cls, 128 * 8);
    double* d_pos = (double*)up(pos, (size_t)S * 128 * 8);
    double* d_Ew = (double*)up(E_w, (size_t)32 * w_cols * 8);
    double* d_Fw = (double*)up(F_w, (size_t)32 * w_cols * 8);
    double* d_Eb = (double*)up(E_b, 32 * 8);
    double* d_Fb = (double*)up(F_b, 32 * 8);
    double* x_in = (double*)tmp.get((size_t)S1 * 128 * 8);
    double* proj = (double*)tmp.get((size_t)64 * 128 * 8);
    launch_ingest_xin(x_in, d_emb, d_tok, d_tab, d_cls, d_pos, S, s);
    launch_ingest_project(proj, x_in, d_Ew, d_Eb, d_Fw, d_Fb, w_cols, S1, s);
    double* dv = nullptr;
    const int n_w = (int)wrap_group_ell.size();
    if (!wrap_ell) {
        dv = (double*)tmp.get((size_t)n_vec * slots * 16);
        launch_ingest_expand(dv, proj, x_in, S1, slots, s);
    } else {
        dv = (double*)tmp.get((size_t)n_w * slots * 16);
        const int* d_pos = (const int*)up(wrap_pos.data(), wrap_pos.size() * sizeof(int));
        launch_ingest_wrap(dv, proj, x_in, d_pos, n_w, slots, s);
    }
    hip_check(hipGetLastError(), "ingest kernels");
    if (proj_out) {   // test hook: x_in rows then the 64 projected rows, as computed on the device
        proj_out->resize((size_t)(S1 + 64) * 128);
        hip_check(hipMemcpyAsync(proj_out->data(), x_in, (size_t)S1 * 128 * 8, hipMemcpyDeviceToHost, s), "ingest download");
        hip_check(hipMemcpyAsync(proj_out->data() + (size_t)S1 * 128, proj, (size_t)64 * 128 * 8, hipMemcpyDeviceToHost, s), "ingest download");
    }
    hip_check(hipStreamSynchronize(s), "ingest sync");   // the host buffers are the caller's: done with them
    if (wrap_ell)
        return encrypt_wrapped(dv, slots, slots, n_vec, wrap_group_ell, wrap_pos, [&](size_t bytes) { return tmp.get(bytes); });
    begin_call();
    std::vector<CtPtr> out(n_vec);
    std::vector<char> seen(n_vec, 0);
    for (int i = 0; i < n_vec; ++i) {
        if (seen[i]) continue;
        const int lvl = std::min(c_.L, level + std::max(0, drop[i]));
        const int ell = c_.L + 1 - lvl;
        const size_t pn = (size_t)ell * c_.N;
        const long double scale = c_.sf_real[lvl];
        // runs of consecutive vectors that start at this level, in chunks of 32 (bounds the temporaries)
        int j = i;
        while (j < n_vec) {
            if (seen[j] || std::min(c_.L, level + std::max(0, drop[j])) != lvl) {
                ++j;
                continue;
            }
            int hi = j;
            while (hi < n_vec && hi - j < 32 && !seen[hi] && std::min(c_.L, level + std::max(0, drop[hi])) == lvl) ++hi;
            const int n = hi - j;
            u64* enc = (u64*)tmp.get((size_t)n * pn * sizeof(u64));   // the encoded plaintext: wiped and freed with the other temporaries
            encode_complex_on_device(c_, enc, dv + (size_t)j * slots * 2, n, slots, ell, scale);
            std::vector<CtPtr> part;
            u64 nonces[32];
            for (int k = 0; k < n; ++k) nonces[k] = (u64)(j + k);
            encrypt_encoded(enc, pn, n, ell, scale, slots, part, nonces);
            for (int k = 0; k < n; ++k) {
                out[j + k] = part[k];
                seen[j + k] = 1;
            }
            j = hi;
        }
    }
    return out;   // ~Temps wipes and frees
}

// ingest_sample for `stride` samples of one length S that share a ciphertext (include/fhelin.h "Interleaved samples"): x_in and the
// projections run per sample with ingest_sample's own kernels (so proj_out[i] is ingest_sample's, bit for bit), the expand step writes
// sample i into lane i of the shared [n_vec][slots * stride] buffer, and the 64 + S + 1 vectors are encoded and encrypted once for the
// group: the sampler draws of ONE ingest_sample.  wrap_ell: as ingest_sample's, the group's WRAPPED ciphertexts - the same inputs of
// every sample in one ciphertext (ingest_wrap_interleaved_kernel), the draws of one wrapped ingest_sample.
std::vector<CtPtr> Client::ingest_interleaved(const double* const* emb, const int* const* tokens, const double* table, int vocab, int S,
                                              const double* cls, const double* pos, const double* E_w, const double* E_b, const double* F_w,
                                              const double* F_b, int w_cols, int level, const std::vector<int>& drop,
                                              std::vector<std::vector<double>>* proj_out, const std::vector<int>* wrap_ell) {
    if (wrap_ell && eval_only_) throw Error(FHELIN_ERR_KEY, "wrapped inputs are secret-key encryptions: an evaluation context holds no secret");
    if ((seeded_ || wrap_ell) ? !s_all : !pk) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    const int st = c_.stride, slots = 1 << c_.prm.log_slots, S1 = S + 1, n_vec = 64 + S1, phys = slots * st;
    if (slots != 16384) throw Error(FHELIN_ERR_ARG, "ingest: the expanded layout needs 16384 slots (128 x 128)");
    if ((long)slots * st > c_.N / 2) throw Error(FHELIN_ERR_ARG, "ingest: slots x interleave stride must be <= N/2");
    if (S < 1 || S1 > w_cols || (!emb && !(tokens && table && vocab > 0))) throw Error(FHELIN_ERR_ARG, "ingest: bad token count / inputs");
    if (level < 0 || level > c_.L || (int)drop.size() != n_vec) throw Error(FHELIN_ERR_ARG, "ingest: level out of range");
    for (int i = 0; i < st; ++i) {
        if (emb ? !emb[i] : !tokens[i]) throw Error(FHELIN_ERR_ARG, "ingest: a sample of the group has no input");
        if (!emb)
            for (int t = 0; t < S; ++t)
                if (tokens[i][t] < 0 || tokens[i][t] >= vocab) throw Error(FHELIN_ERR_ARG, "ingest: token id outside the embedding table");
    }
    std::vector<int> wrap_group_ell, wrap_pos;
    if (wrap_ell) wrap_groups(*wrap_ell, n_vec, wrap_group_ell, wrap_pos);
    hipStream_t s = c_.stream;
    // as ingest_sample: every temporary is the client's plaintext - wiped, then freed, on every path out
    struct Temps {
        Context& c;
        hipStream_t s;
        std::vector<std::pair<Scratch<char>, size_t>> blocks;
        void* get(size_t bytes) {
            blocks.emplace_back(c.scratch<char>(bytes), bytes);
            return blocks.back().first.get();
        }
        ~Temps() {
            for (auto& b : blocks) (void)hipMemsetAsync(b.first.get(), 0, b.second, s);
        }
    } tmp{c_, s, {}};
    auto up = [&](const void* h, size_t bytes) {
        void* d = tmp.get(bytes);
        hip_check(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "ingest upload");
        return d;
    };
    double* d_tab = emb ? nullptr : (double*)up(table, (size_t)vocab * 128 * 8);
    double* d_cls = (double*)up(cls, 128 * 8);
    double* d_pos = (double*)up(pos, (size_t)S * 128 * 8);
    double* d_Ew = (double*)up(E_w, (size_t)32 * w_cols * 8);
    double* d_Fw = (double*)up(F_w, (size_t)32 * w_cols * 8);
    double* d_Eb = (double*)up(E_b, 32 * 8);
    double* d_Fb = (double*)up(F_b, 32 * 8);
    double* x_in = (double*)tmp.get((size_t)st * S1 * 128 * 8);     // [stride][S1][128]
    double* proj = (double*)tmp.get((size_t)st * 64 * 128 * 8);     // [stride][64][128]
    for (int i = 0; i < st; ++i) {
        double* d_emb = emb ? (double*)up(emb[i], (size_t)S * 128 * 8) : nullptr;
        int* d_tok = emb ? nullptr : (int*)up(tokens[i], (size_t)S * 4);
        launch_ingest_xin(x_in + (size_t)i * S1 * 128, d_emb, d_tok, d_tab, d_cls, d_pos, S, s);
        launch_ingest_project(proj + (size_t)i * 64 * 128, x_in + (size_t)i * S1 * 128, d_Ew, d_Eb, d_Fw, d_Fb, w_cols, S1, s);
    }
    double* dv = nullptr;
    if (!wrap_ell) {
        dv = (double*)tmp.get((size_t)n_vec * phys * 16);
        launch_ingest_expand_interleaved(dv, proj, x_in, S1, slots, st, s);
    } else {
        const int n_w = (int)wrap_group_ell.size();
        dv = (double*)tmp.get((size_t)n_w * phys * 16);
        const int* d_wpos = (const int*)up(wrap_pos.data(), wrap_pos.size() * sizeof(int));
        launch_ingest_wrap_interleaved(dv, proj, x_in, d_wpos, n_w, S1, slots, st, s);
    }
    hip_check(hipGetLastError(), "ingest kernels");
    if (proj_out) {   // per sample: x_in rows then the 64 projected rows, as ingest_sample reports them
        proj_out->assign(st, std::vector<double>((size_t)(S1 + 64) * 128));
        for (int i = 0; i < st; ++i) {
            double* h = (*proj_out)[i].data();
            hip_check(hipMemcpyAsync(h, x_in + (size_t)i * S1 * 128, (size_t)S1 * 128 * 8, hipMemcpyDeviceToHost, s), "ingest download");
            hip_check(hipMemcpyAsync(h + (size_t)S1 * 128, proj + (size_t)i * 64 * 128, (size_t)64 * 128 * 8, hipMemcpyDeviceToHost, s),
                      "ingest download");
        }
    }
    hip_check(hipStreamSynchronize(s), "ingest sync");   // the host buffers are the caller's: done with them
    if (wrap_ell)
        return encrypt_wrapped(dv, phys, slots, n_vec, wrap_group_ell, wrap_pos, [&](size_t bytes) { return tmp.get(bytes); });
    begin_call();
    std::vector<CtPtr> out(n_vec);
    std::vector<char> seen(n_vec, 0);
    for (int i = 0; i < n_vec; ++i) {   // runs of one level in chunks of 32, exactly as ingest_sample forms them
        if (seen[i]) continue;
        const int lvl = std::min(c_.L, level + std::max(0, drop[i]));
        const int ell = c_.L + 1 - lvl;
        const size_t pn = (size_t)ell * c_.N;
        const long double scale = c_.sf_real[lvl];
        int j = i;
        while (j < n_vec) {
            if (seen[j] || std::min(c_.L, level + std::max(0, drop[j])) != lvl) {
                ++j;
                continue;
            }
            int hi = j;
            while (hi < n_vec && hi - j < 32 && !seen[hi] && std::min(c_.L, level + std::max(0, drop[hi])) == lvl) ++hi;
            const int n = hi - j;
            u64* enc = (u64*)tmp.get((size_t)n * pn * sizeof(u64));
            encode_complex_on_device(c_, enc, dv + (size_t)j * phys * 2, n, phys, ell, scale);
            std::vector<CtPtr> part;
            u64 nonces[32];
            for (int k = 0; k < n; ++k) nonces[k] = (u64)(j + k);
            encrypt_encoded(enc, pn, n, ell, scale, slots, part, nonces);
            for (int k = 0; k < n; ++k) {
                out[j + k] = part[k];
                seen[j + k] = 1;
            }
            j = hi;
        }
    }
    return out;   // ~Temps wipes and frees
}

CtPtr Client::phase(const CtPtr& ct, int nl) {
    if (!s_all) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    if (nl < 1 || nl > ct->ell || ct->npoly < 2) throw Error(FHELIN_ERR_ARG, "phase: bad limb count / component count");
    const size_t pn = (size_t)ct->ell * c_.N;
    CtPtr o = ev_.new_ct(1, nl, ct->deg, ct->scale, ct->slots);
    u64* m = o->d;
    // m = c0 + c1 s (+ c2 s^2) on the first nl limbs
    launch_ew_muladd(c_.dt, m, ct->d, ct->d + pn, s_all, nl, nl, 0, nl, c_.stream);
    if (ct->npoly == 3) {
        Scratch<u64> s2 = c_.scratch<u64>((size_t)nl * c_.N);
        launch_ew_mul(c_.dt, s2, s_all, s_all, nl, nl, 0, nl, c_.stream);
        launch_ew_muladd(c_.dt, m, m, ct->d + 2 * pn, s2, nl, nl, 0, nl, c_.stream);
    }
    hip_check(hipGetLastError(), "phase kernels");
    return o;
}

std::vector<double> Client::decrypt(const CtPtr& cin, int slots, int flood_bits) {
    if (c_.stride == 1) return decrypt_physical(cin, slots, flood_bits, 1);
    const std::vector<double> v = decrypt_physical(cin, slots, flood_bits, c_.stride);   // lane 0 of the physical vector
    std::vector<double> out(v.size() / c_.stride);
    for (size_t k = 0; k < out.size(); ++k) out[k] = v[k * c_.stride];
    return out;
}

std::vector<double> Client::decrypt_interleaved(const CtPtr& cin, int slots, int flood_bits) {
    const int s = c_.stride;
    const std::vector<double> v = decrypt_physical(cin, slots, flood_bits, s);
    const size_t n = v.size() / s;
    std::vector<double> out(v.size());
    for (int i = 0; i < s; ++i)
        for (size_t k = 0; k < n; ++k) out[(size_t)i * n + k] = v[k * s + i];
    return out;
}

// slots: logical (<= 0: the ciphertext's); the decoded packing has slots * mult physical slots
std::vector<double> Client::decrypt_physical(const CtPtr& cin, int slots, int flood_bits, int mult) {
    if (!s_all) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "decrypt_flooded: flood_bits must lie in [0, 62]");
    CtPtr ct = cin;
    while (ct->deg > 1 && ct->ell > 2) ct = ev_.rescale(ct);
    if (slots <= 0) slots = ct->slots > 0 ? ct->slots : (1 << c_.prm.log_slots);
    if (mult > 1) {
        if ((slots & (slots - 1)) || (long)slots * mult > c_.N / 2) throw Error(FHELIN_ERR_ARG, "decrypt: slots x interleave stride must be a power of two <= N/2");
        slots *= mult;
    }
    const size_t N = c_.N;
    const int ell = ct->ell - (ct->wrapped() ? 1 : 0), nl = std::min(ell, 2);   // a wrapped input's extra limb is left out
    CtPtr ph = phase(ct, nl);
    u64* m = ph->d;
    c_.ntt(LimbBatch{m, nl, nullptr, 0, nl}, true);
    if (flood_bits > 0) {   // noise-flooding decryption: phase + f in coefficient form, on the limbs that are read
        check_flood(flood_bits, nl, "decrypt_flooded");
        Scratch<u64> f = c_.scratch<u64>((size_t)nl * N);
        sample_flood_device(f, 1, nl, flood_bits, false);
        launch_ew_add(c_.dt, m, m, f, nl, nl, 0, nl, c_.stream);
        hip_check(hipGetLastError(), "decrypt flood kernels");
        hip_check(hipMemsetAsync(f, 0, (size_t)nl * N * sizeof(u64), c_.stream), "hipMemsetAsync(decrypt flood)");
    }
    std::vector<u64> h((size_t)nl * N);
    hip_check(hipMemcpyAsync(h.data(), m, h.size() * 8, hipMemcpyDeviceToHost, c_.stream), "decrypt download");
    hip_check(hipStreamSynchronize(c_.stream), "decrypt sync");
    ph.reset();
    const u64 q0 = c_.chain.q[0];
    const size_t gap = (N / 2) / slots;
    std::vector<std::pair<double, double>> v(slots);
    const u64 q1 = nl > 1 ? c_.chain.q[1] : 1;
    const u64 inv = nl > 1 ? h_invmod(q0 % q1, q1) : 0;     // q0^-1 mod q1, once (not per coefficient)
    const u128 Q = (u128)q0 * q1;
    auto lift = [&](size_t idx) -> long double {
        if (nl == 1) {
            u64 x = h[idx];
            return x > q0 / 2 ? -(long double)(q0 - x) : (long double)x;
        }
        const u64 x0 = h[idx], x1 = h[N + idx];
        const u64 d = h_mulmod(sub_mod(x1, x0 % q1, q1), inv, q1);
        const u128 x = (u128)x0 + (u128)q0 * d;
        if (x > Q / 2) {
            const u128 mag = Q - x;
            return -((long double)(u64)(mag >> 64) * 18446744073709551616.0L + (long double)(u64)mag);
        }
        return (long double)(u64)(x >> 64) * 18446744073709551616.0L + (long double)(u64)x;
    };
    for (int i = 0; i < slots; ++i) {
        v[i].first = (double)(lift(i * gap) / ct->scale);
        v[i].second = (double)(lift(i * gap + N / 2) / ct->scale);
    }
    ckks_fft_special(v, false);
    std::vector<double> out(slots);
    for (int i = 0; i < slots; ++i) out[i] = v[i].first;
    return out;
}

// The decoder on the device for a whole batch (client.h): what decrypt_physical does per ciphertext on the host after its download -
// CRT lift in long double, division by the scale, forward special FFT - runs in decode_lift_kernel and the forward FFT kernels, held to
// the host code bit for bit; the batch then costs one download of the slots asked for and one drain of the stream.
void Client::decrypt_batch(const std::vector<CtPtr>& cin, int slots, int flood_bits, bool all_lanes, const int* idx, int n_idx, double* out) {
    c_.require_device();
    if (!s_all) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "decrypt_batch: flood_bits must lie in [0, 62]");
    const int n = (int)cin.size();
    if (n == 0) return;
    if (!out) throw Error(FHELIN_ERR_ARG, "decrypt_batch: null output");
    if (cin.size() > 65535) throw Error(FHELIN_ERR_ARG, "decrypt_batch: at most 65535 ciphertexts per call");
    if (idx && n_idx <= 0) throw Error(FHELIN_ERR_ARG, "decrypt_batch: an index list needs at least one entry");
    // every refusal before any device work and before the sampler is touched
    for (const CtPtr& ct : cin)
        if (!ct || ct->npoly < 2 || ct->npoly > 3) throw Error(FHELIN_ERR_ARG, "decrypt_batch: a ciphertext has 2 or 3 components");
    if (slots <= 0) {
        for (const CtPtr& ct : cin) {
            const int own = ct->slots > 0 ? ct->slots : (1 << c_.prm.log_slots);
            if (slots > 0 && own != slots) throw Error(FHELIN_ERR_ARG, "decrypt_batch: the ciphertexts' slot counts disagree (pass slots)");
            slots = own;
        }
    }
    const int st = c_.stride;
    if ((slots & (slots - 1)) || (long)slots * st > c_.N / 2)
        throw Error(FHELIN_ERR_ARG, "decrypt_batch: slots x interleave stride must be a power of two <= N/2");
    if (idx)
        for (int k = 0; k < n_idx; ++k)
            if (idx[k] < 0 || idx[k] >= slots) throw Error(FHELIN_ERR_ARG, "decrypt_batch: slot index outside [0, slots)");
    std::vector<int> nl(n);
    int nl_max = 1, nl_sum = 0;
    for (int b = 0; b < n; ++b) {   // the limbs read once the pending rescales have run, a wrapped input's extra limb left out
        int ell = cin[b]->ell, deg = cin[b]->deg;
        while (deg > 1 && ell > 2) --ell, --deg;
        ell -= cin[b]->wrapped() ? 1 : 0;
        if (ell < 1) throw Error(FHELIN_ERR_ARG, "decrypt_batch: a ciphertext has no limb to read");
        nl[b] = std::min(ell, 2);
        nl_max = std::max(nl_max, nl[b]);
        nl_sum += nl[b];
        if (flood_bits > 0) check_flood(flood_bits, nl[b], "decrypt_batch");
    }
    std::vector<CtPtr> x = cin;
    for (;;) {   // ONE rescale_batch per pending degree (as decrypt rescales its input)
        std::vector<CtPtr> need;
        std::vector<size_t> at;
        for (size_t i = 0; i < x.size(); ++i)
            if (x[i]->deg > 1 && x[i]->ell > 2) {
                need.push_back(x[i]);
                at.push_back(i);
            }
        if (need.empty()) break;
        std::vector<CtPtr> r = ev_.rescale_batch(need);
        for (size_t k = 0; k < at.size(); ++k) x[at[k]] = r[k];
    }
    const size_t N = c_.N;
    const int phys = slots * st;
    const int lanes = all_lanes ? st : 1, width = idx ? n_idx : slots;
    hipStream_t s = c_.stream;
    // device tables of the call in one upload: the items, the inverse NTT's limb table (-1: a row the item does not read), the slot list
    const size_t off_limb = (size_t)n * sizeof(DecodeItem), off_idx = off_limb + (size_t)n * nl_max * sizeof(int);
    std::vector<char> host(off_idx + (idx ? (size_t)n_idx * sizeof(int) : 0));
    DecodeItem* items = reinterpret_cast<DecodeItem*>(host.data());
    int* limb_tab = reinterpret_cast<int*>(host.data() + off_limb);
    for (int b = 0; b < n; ++b) {
        const Ciphertext& ct = *x[b];
        const size_t pn = (size_t)ct.ell * N;
        int e2 = 0;
        const long double m = frexpl(ct.scale, &e2);         // scale = m * 2^e2, m in [0.5, 1): a 64-bit significand, exactly
        items[b].c0 = ct.d;
        items[b].c1 = ct.d + pn;
        items[b].c2 = ct.npoly == 3 ? ct.d + 2 * pn : nullptr;
        items[b].ms = (u64)ldexpl(m, 64);
        items[b].es = e2 - 64;
        items[b].deg = ct.npoly - 1;
        items[b].limb_stride = (int32_t)N;
        items[b].nl = nl[b];
        for (int l = 0; l < nl_max; ++l) limb_tab[b * nl_max + l] = l < nl[b] ? l : -1;
    }
    if (idx) std::memcpy(host.data() + off_idx, idx, (size_t)n_idx * sizeof(int));
    Scratch<char> d_tab = c_.scratch<char>(host.size());
    hip_check(hipMemcpyAsync(d_tab, host.data(), host.size(), hipMemcpyHostToDevice, s), "decrypt_batch tables");
    const DecodeItem* d_items = reinterpret_cast<const DecodeItem*>(d_tab.get());
    const int* d_limb = reinterpret_cast<const int*>(d_tab.get() + off_limb);
    const int* d_idx = idx ? reinterpret_cast<const int*>(d_tab.get() + off_idx) : nullptr;
    const size_t words = (size_t)n * nl_max * N;
    Scratch<u64> ph = c_.scratch<u64>(words);
    launch_phase_batch(c_.dt, ph, d_items, s_all, nl_max, n, s);
    c_.ntt(LimbBatch{ph, n * nl_max, d_limb, 0, nl_max}, true, nl_sum);
    if (flood_bits > 0) {   // noise-flooding decryption: phase + f in coefficient form, one sampler call for the batch
        Scratch<u64> f = c_.scratch<u64>(words);
        sample_flood_device(f, n, nl_max, flood_bits, false);
        launch_ew_add(c_.dt, ph, ph, f, n * nl_max, n * nl_max, 0, nl_max, s);
        hip_check(hipGetLastError(), "decrypt_batch flood kernels");
        hip_check(hipMemsetAsync(f, 0, words * sizeof(u64), s), "hipMemsetAsync(decrypt_batch flood)");
    }
    const u64 q0 = c_.chain.q[0], q1 = nl_max > 1 ? c_.chain.q[1] : 1;
    const u64 inv = nl_max > 1 ? h_invmod(q0 % q1, q1) : 0;
    Scratch<double> v = c_.scratch<double>((size_t)n * phys * 2);
    launch_decode_lift(c_.dt, v, ph, d_items, inv, nl_max > 1 ? h_shoup(inv, q1) : 0, nl_max, phys, n, s);
    if (phys >= 2) {
        const Context::FftDev& tab = fft_dev_tables(c_, phys);
        launch_fft_special_fwd(v, tab.rot, tab.ksi, phys, n, s);
    }
    Scratch<double> o = c_.scratch<double>((size_t)n * lanes * width);
    launch_decode_gather(o, v, d_idx, slots, st, lanes, width, n, s);
    hip_check(hipGetLastError(), "decrypt_batch kernels");
    hip_check(hipMemcpyAsync(out, o, (size_t)n * lanes * width * sizeof(double), hipMemcpyDeviceToHost, s), "decrypt_batch download");
    hip_check(hipStreamSynchronize(s), "decrypt_batch sync");
}

void Client::export_secret(u64* out) {
    if (!s_all) throw Error(FHELIN_ERR_KEY, "keygen() has not been called");
    const size_t n = (size_t)(c_.L + 1 + c_.K) * c_.N;
    hip_check(hipMemcpyAsync(out, s_all, n * 8, hipMemcpyDeviceToHost, c_.stream), "export secret");
    hip_check(hipStreamSynchronize(c_.stream), "sync");
}

void Client::import_secret(const u64* in) {
    if (eval_only_) throw Error(FHELIN_ERR_KEY, "import_secret: an evaluation context holds no secret");
    c_.require_device();
    keygen_run_ = true;
    c_.stride_locked = true;
    const size_t n = (size_t)(c_.L + 1 + c_.K) * c_.N;
    if (!s_all) s_all = c_.dalloc<u64>(n);
    hip_check(hipMemcpyAsync(s_all, in, n * 8, hipMemcpyHostToDevice, c_.stream), "import secret");
    hip_check(hipStreamSynchronize(c_.stream), "sync");
}

}  // namespace fhelin
