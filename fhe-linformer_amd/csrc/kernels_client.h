// Launchers of the client-side kernels (kernels_client.hip): batched CKKS encoding and public-key encryption.
#pragma once
#include "kernels.h"

namespace fhelin {

struct SamplerKey {
    u32 w[8];  // ChaCha20 key words of one sampling call (drawn from the client's generator)
};

// Interleaved samples (include/fhelin.h): out [n_vec][slots * stride] complex, physical slot stride * k + i = in [b][lanes == 1 ? 0 : i][k];
// in [n_vec][lanes][slots] with lanes = stride (one staged vector per sample) or 1 (one vector replicated).  stride a power of two >= 2
void launch_interleave_slots(double* out, const double* in, int slots, int stride, int lanes, int n_vec, hipStream_t s);
// data [n_vec][slots] complex (re, im): all stages of the inverse special FFT (without the bit reversal and the 1/n scaling,
// which launch_encode_round_reduce applies while reading).  rot [slots] = 5^j mod 4 slots, ksi [4 slots + 1] = e^{2 pi i k / (4 slots)}
void launch_fft_special_inv(double* data, const u32* rot, const double* ksi, int slots, int n_vec, hipStream_t s);
// out [n_vec][ell][N] (coefficient form) <- round(v * scale) mod q_l with scale = scale_mant * 2^scale_exp (64-bit significand)
void launch_encode_round_reduce(const DeviceTables& t, u64* out, const double* fftdata, int slots, int ell, u64 scale_mant, int scale_exp,
                                int n_vec, hipStream_t s);
// the limb-sliced form (Plaintext::at_sliced): out [n_vec][ell_q + k][N], the first ell_q rows modulo q_0..q_{ell_q-1}, then k rows modulo
// the limbs from id L1 on (the special limbs) - the rows of the full-basis encoding that a key switch at ell_q limbs reads, dense
void launch_encode_round_reduce_split(const DeviceTables& t, u64* out, const double* fftdata, int slots, int ell_q, int k, int L1, u64 scale_mant,
                                      int scale_exp, int n_vec, hipStream_t s);
// out [n_poly][ell][N] (coefficient form): kind 0 rounded Gaussian sigma 3.19, kind 1 uniform ternary; polynomial p uses
// ChaCha20 stream stream_base + p
void launch_sample_small(const DeviceTables& t, u64* out, const SamplerKey& key, u64 stream_base, int kind, int ell, int n_poly, hipStream_t s);
// ct [n_vec][2][ell][N] <- (pk_b u + e0 + m, pk_a u + e1); u, e0, e1 [n_vec][ell][N]; m at m + b * m_stride; pk [2][L1][N]
void launch_encrypt_combine(const DeviceTables& t, u64* ct, const u64* pk, const u64* u, const u64* e0, const u64* e1, const u64* m, int ell,
                            int L1, size_t m_stride, int n_vec, hipStream_t s);

// out [n_poly][ell][N] (coefficient form): coefficient i of polynomial p = (W >> (63 - flood_bits)) - 2^flood_bits reduced into
// [0, q_l), W = little-endian u64 word i % 8 of ChaCha20 block i / 8 of stream stream_base + p; 1 <= flood_bits <= 62.
// gauss: plus a rounded Gaussian (sigma 3.19, launch_sample_small kind 0) from stream gauss_stream_base + p
void launch_sample_flood(const DeviceTables& t, u64* out, const SamplerKey& key, u64 stream_base, u64 gauss_stream_base, int flood_bits,
                         bool gauss, int ell, int n_poly, hipStream_t s);
// one ciphertext of a re-randomised batch: in [2][in_ell][N], out [2][out_ell][N] with out_ell <= in_ell (device table entry)
struct RerandItem {
    const u64* in;
    u64* out;
    int32_t in_ell;
    int32_t pad_ = 0;
};
static_assert(sizeof(RerandItem) == 24, "RerandItem is 24 bytes");
// out_b = first out_ell limbs of in_b + (pk_b u_b + w_b, pk_a u_b + e1_b) for b < n_ct (<= 65535) in one launch; tab [n_ct] on the
// device; u, w, e1 [n_ct][out_ell][N] and pk [2][L1][N] in NTT form
void launch_rerandomize_combine(const DeviceTables& t, const RerandItem* tab, const u64* pk, const u64* u, const u64* w, const u64* e1,
                                int out_ell, int L1, int n_ct, hipStream_t s);

// ---- batched decryption (include/fhelin.h "Batched decryption"): phase, lift, forward special FFT and slot gather on the device
// one ciphertext of a decrypted batch (device table entry): components [ell][N] each, NTT form; the first nl limbs are read
struct DecodeItem {
    const u64* c0;
    const u64* c1;
    const u64* c2;          // null: a 2-component ciphertext
    u64 ms;                 // scale = ms * 2^es (64-bit significand, as launch_encode_round_reduce takes it)
    int32_t es;
    int32_t deg;            // components - 1: 1 or 2
    int32_t limb_stride;    // words between two limbs of a component (N)
    int32_t nl;             // limbs read: 1 or 2
};
static_assert(sizeof(DecodeItem) == 48, "DecodeItem is 48 bytes");
// out [n][nl_max][N] (NTT form) <- c0 + c1 s (+ c2 s^2) on the first nl limbs of item b = tab[b]; rows nl..nl_max-1 of an item are
// zeroed.  s [..][N] the secret's Q limbs, NTT form; tab [n] on the device; n <= 65535
void launch_phase_batch(const DeviceTables& t, u64* out, const DecodeItem* tab, const u64* s, int nl_max, int n, hipStream_t st);
// v [n][slots] complex <- the decoded coefficients of phase [n][nl_max][N] (coefficient form), element bitrev(i) = (lift(i * gap),
// lift(i * gap + N/2)) / scale with gap = (N/2) / slots: csrc/decode_lift.h per coefficient, the forward FFT's bit reversal in the store.
// q0inv = q_0^-1 mod q_1 and its Shoup companion (unused when no item reads two limbs)
void launch_decode_lift(const DeviceTables& t, double* v, const u64* phase, const DecodeItem* tab, u64 q0inv, u64 q0inv_shoup, int nl_max,
                        int slots, int n, hipStream_t st);
// data [n_vec][slots] complex, bit-reversed input: all stages of the forward special FFT in place, bit-identical to the host loop
// ckks_fft_special(forward).  Stages up to len 512 in ONE launch over 512-element LDS tiles, every later stage one launch.
// rot / ksi as launch_fft_special_inv.  slots = 1: nothing to do
void launch_fft_special_fwd(double* data, const u32* rot, const double* ksi, int slots, int n_vec, hipStream_t st);
// out [n][lanes][width] <- Re v[b][(idx ? idx[k] : k) * stride + lane]; v [n][slots * stride] complex; lanes = 1 (lane 0) or stride;
// width = n_idx when idx (device, logical slot numbers) is given, else slots
void launch_decode_gather(double* out, const double* v, const int* idx, int slots, int stride, int lanes, int width, int n, hipStream_t st);

// ---- client-side ingestion of one sample (reference src/python/dimReduce.py:141-160 and the read_expanded_input packing,
// src/FHEController.cpp:623-650), all in fp64 with the operation order of the NumPy statement and FMA contraction off:
//   x_in[0] = cls, x_in[t] = emb[t-1] + pos[t-1] / 3   (emb row = table[token[t-1]] when a token-id list is given)
//   X[i]    = (...((W[i][0] x_in[0]) + W[i][1] x_in[1]) + ...) + b[i]      for the 32 rows of E and of F (sequential sums)
//   slot j*128 + i of vector v = v[j]  (i < 128; "expanded" layout), written as complex doubles for the encoder's inverse FFT
// x_in [S1][128]; proj [64][128] (E rows then F rows); out [(64 + S1)][slots][2] in the order E rows, F rows, tokens.
void launch_ingest_xin(double* x_in, const double* emb, const int* tokens, const double* table, const double* cls, const double* pos,
                       int S, hipStream_t s);
void launch_ingest_project(double* proj, const double* x_in, const double* E_w, const double* E_b, const double* F_w, const double* F_b,
                           int w_cols, int S1, hipStream_t s);
void launch_ingest_expand(double* out, const double* proj, const double* x_in, int S1, int slots, hipStream_t s);
// `stride` samples of one length S1 - 1: proj [stride][64][128], x_in [stride][S1][128]; out [(64 + S1)][slots * stride][2], sample i in
// the physical slots = i mod stride
void launch_ingest_expand_interleaved(double* out, const double* proj, const double* x_in, int S1, int slots, int stride, hipStream_t s);
// the wrapped layout (include/fhelin.h "Wrapped inputs"): out [n_w][slots][2], slot j*128 + t of vector w = input pos[w][t] [j]
// (inputs numbered as in launch_ingest_expand: E rows, F rows, tokens); pos [n_w][128] on the device, -1 = empty column
void launch_ingest_wrap(double* out, const double* proj, const double* x_in, const int* pos, int n_w, int slots, hipStream_t s);
// the wrapped layout of `stride` samples of one length S1 - 1 (proj, x_in as launch_ingest_expand_interleaved; pos shared by the samples):
// out [n_w][slots * stride][2], physical slot stride * (j*128 + t) + i of vector w = input pos[w][t] [j] of sample i
void launch_ingest_wrap_interleaved(double* out, const double* proj, const double* x_in, const int* pos, int n_w, int S1, int slots, int stride,
                                    hipStream_t s);
}  // namespace fhelin
