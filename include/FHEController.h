/*
 * FHEController.h — source-compatible shim of the reference's `class FHEController`
 * (reference src/FHEController.h:22-161) on top of the MI355X-native engine's C ABI (fhelin.h).
 *
 * Same method names, argument meaning and error behaviour as the reference class, so that the reference's
 * drivers (src/main.cpp, src/main_2.cpp) compile against this header unchanged:
 *   - `Ctxt` / `Ptxt` are nullable, copyable shared handles (reference :19-20); `ct->GetLevel()`,
 *     `ct->Clone()`, `ct->GetSlots()`, `pt->SetLength()`, `pt->GetRealPackedValue()` are provided.
 *   - like reference src/FHEController.h:13-17 and src/Utils.h:15-17 this header leaks
 *     `using namespace std; std::chrono; lbcrypto; utils` — main.cpp relies on that.
 *   - I/O failure -> message + exit(1) (reference :59-71,:192-220); missing ciphertext file -> message and
 *     a null handle (:1383-1394); engine failures -> uncaught std::runtime_error (OpenFHE throws likewise).
 * Every arithmetic instruction runs in libfhelin_amd.so on the GPU; this header only marshals handles,
 * parses the reference's text files into its three packing layouts, and fits Chebyshev coefficients.
 *
 * Persistence: OpenFHE's cereal BINARY files are out of scope.  `generate_context(true)` writes the
 * PUBLIC parameter set to ../<parameters_folder>/crypto-context.txt and — separately, like the reference's
 * secret-key.txt (:80-86) — the client's 256-bit SECRET seed to ../<parameters_folder>/secret-key.txt.  All key material
 * derives from that seed through a ChaCha20 stream, so `load_context` (which, like the reference :208-214, reads the
 * secret key file) + `load_bootstrapping_and_rotation_keys` regenerate bit-identical keys.  Whoever holds secret-key.txt
 * can decrypt, so it never goes to an evaluation server: the client writes an evaluation-key set instead
 * (`save_evaluation_keys`: the public key and every switching key, no secret) and the server opens it with
 * `load_evaluation_context`, which never reads secret-key.txt ("Client / server split").  On such a server
 * decrypt and the debug prints throw.  Ciphertexts are saved in the engine's own little-endian limb format.
 */
#ifndef FHELIN_FHECONTROLLER_SHIM_H
#define FHELIN_FHECONTROLLER_SHIM_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fcntl.h>
#include <fstream>
#include <sys/stat.h>
#include <unistd.h>
#include <functional>
#include <iomanip>
#include <iostream>
#include <iterator>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fhelin.h"

namespace lbcrypto {}  // the reference header does `using namespace lbcrypto;`

using namespace lbcrypto;
using namespace std;
using namespace std::chrono;

/* ---- the subset of reference src/Utils.h that FHEController and main.cpp use (:21-42, :61-87) ---------- */
namespace utils {
typedef chrono::time_point<steady_clock, nanoseconds> tick_t;
static inline tick_t start_time() { return steady_clock::now(); }
static duration<long long, ratio<1, 1000>> total_time;
// "(title): s:ms (Total: Ns)" like the reference's stopwatch, minutes shown once a step exceeds 60 s
static inline void print_duration(tick_t start, const string& title) {
    const long long ms_all = duration_cast<milliseconds>(steady_clock::now() - start).count();
    total_time += milliseconds(ms_all);
    const long long mins = ms_all / 60000, secs = (ms_all / 1000) % 60, ms = ms_all % 1000;
    cout << "(" << title << "): ";
    if (mins > 0) cout << mins << "." << secs << ":" << ms << endl;
    else cout << secs << ":" << ms << "s (Total: " << duration_cast<seconds>(total_time).count() << "s)" << endl;
}
// comma- and newline-separated decimal numbers (the format written by extract_parameters_numeric.py): one strtod
// sweep over the whole file; unparsable tokens are reported and skipped; a missing file yields an empty vector
static inline vector<double> read_values_from_file(const string& filename, double scale = 1) {
    vector<double> values;
    ifstream file(filename, ios::in | ios::binary);
    if (!file.is_open()) {
        std::cerr << "Can not open " << filename << std::endl;
        return values;
    }
    const string text((istreambuf_iterator<char>(file)), istreambuf_iterator<char>());
    const char* p = text.c_str();
    const char* const last = p + text.size();
    while (p < last) {
        while (p < last && (*p == ',' || *p == '\n' || *p == '\r' || *p == ' ' || *p == '\t')) ++p;
        if (p >= last) break;
        char* stop = nullptr;
        const double v = std::strtod(p, &stop);
        if (stop == p) {
            const char* q = p;
            while (q < last && *q != ',' && *q != '\n') ++q;
            cerr << "Can not convert: " << string(p, q) << endl;
            p = q;
            continue;
        }
        values.push_back(v * scale);
        p = stop;
    }
    return values;
}
}  // namespace utils
using namespace utils;

/* ---- handles ------------------------------------------------------------------------------------------ */
namespace fhelin_shim {
inline void check(int rc, const char* what) {
    if (rc != FHELIN_OK) throw std::runtime_error(string(what) + ": " + fhelin_last_error());
}
class CiphertextImpl;
class PlaintextImpl;
}  // namespace fhelin_shim

using Ctxt = std::shared_ptr<fhelin_shim::CiphertextImpl>;
using Ptxt = std::shared_ptr<fhelin_shim::PlaintextImpl>;

namespace fhelin_shim {
class CiphertextImpl {
public:
    fhelin_ctx* ctx;
    fhelin_ct* h;
    CiphertextImpl(fhelin_ctx* c, fhelin_ct* x) : ctx(c), h(x) {}
    ~CiphertextImpl() { fhelin_ct_free(h); }
    CiphertextImpl(const CiphertextImpl&) = delete;
    CiphertextImpl& operator=(const CiphertextImpl&) = delete;
    size_t GetLevel() const {
        int32_t lv = 0;
        fhelin_ct_info(h, nullptr, nullptr, &lv, nullptr, nullptr, nullptr);
        return (size_t)lv;
    }
    uint32_t GetSlots() const {
        int32_t s = 0;
        fhelin_ct_info(h, nullptr, nullptr, nullptr, nullptr, nullptr, &s);
        return (uint32_t)s;
    }
    size_t GetNoiseScaleDeg() const {
        int32_t d = 0;
        fhelin_ct_info(h, nullptr, nullptr, nullptr, &d, nullptr, nullptr);
        return (size_t)d;
    }
    Ctxt Clone() const {
        fhelin_ct* o = nullptr;
        check(fhelin_ct_clone(ctx, h, &o), "Clone");
        return std::make_shared<CiphertextImpl>(ctx, o);
    }
};
class PlaintextImpl {
public:
    fhelin_ctx* ctx;
    fhelin_pt* h;          // null for a decryption result
    vector<double> values;  // slot values
    size_t length;
    PlaintextImpl(fhelin_ctx* c, fhelin_pt* x, vector<double> v) : ctx(c), h(x), values(std::move(v)), length(values.size()) {}
    ~PlaintextImpl() { fhelin_pt_free(h); }
    PlaintextImpl(const PlaintextImpl&) = delete;
    PlaintextImpl& operator=(const PlaintextImpl&) = delete;
    void SetLength(size_t n) { length = n; }
    void SetSlots(uint32_t) {}
    vector<double> GetRealPackedValue() const {
        vector<double> v(values.begin(), values.begin() + std::min(length, values.size()));
        v.resize(length, 0.0);
        return v;
    }
};
}  // namespace fhelin_shim

/* ---- the controller ------------------------------------------------------------------------------------ */
class FHEController {
    fhelin_ctx* context = nullptr;

public:
    int circuit_depth = 0;
    int num_slots = 0;

    FHEController() {}
    ~FHEController() {
        save_level_plan();
        fhelin_ctx_destroy(context);
    }
    FHEController(const FHEController&) = delete;
    FHEController& operator=(const FHEController&) = delete;

    /* Context generating/loading (reference :3-235).  The reference's parameters: N=2^15, depth 27 = 28 Q limbs, dnum 4
     * (:6-35), hence 7 special limbs by OpenFHE's rule — used as they are; FHELIN_PRESET=bench selects BASELINE.json's
     * ring N=2^16. */
    void generate_context(bool serialize = false, bool secure = false) {
        (void)secure;  // parsed but ignored by the reference as well (:3,:10)
        num_slots = 1 << 14;
        level_budget = {3, 3};
        fhelin_params p = default_params();
        circuit_depth = 1 + 12 + 14;  // 1 + levelsUsedBeforeBootstrap + GetBootstrapDepth(8, {3,3}, SPARSE_TERNARY)  (:27-31)
        cout << endl << "Ciphertexts depth: " << circuit_depth << ", available multiplications: " << 12 - 2 << endl;
        create(p);
        cout << "Context built, generating keys..." << endl;
        apply_seeded_keys();
        fhelin_shim::check(fhelin_keygen(context), "KeyGen");
        fhelin_shim::check(fhelin_gen_relin_key(context), "EvalMultKeyGen");
        cout << "Generated." << endl;
        if (!serialize) return;
        cout << "Now serializing keys ..." << endl;
        ofstream f("../" + parameters_folder + "/crypto-context.txt", ios::out | ios::binary);
        if (!f.is_open()) {
            cerr << "Error serializing the crypto context in \"" << "../" + parameters_folder + "/crypto-context.txt" << "\"" << endl;
            exit(1);
        }
        f << "fhelin-context 2\n" << p.log_n << ' ' << p.n_q << ' ' << p.first_bits << ' ' << p.scale_bits << ' ' << p.n_p << ' '
          << p.special_bits << ' ' << p.dnum << ' ' << p.log_slots << ' ' << p.hamming << '\n';
        cout << "Crypto Context have been serialized" << std::endl;
        // the secret goes to its own file, as in the reference (:80-86)
        uint8_t seed[32];
        fhelin_shim::check(fhelin_ctx_secret_seed(context, seed), "Serialize(secret)");
        const string sk_path = "../" + parameters_folder + "/secret-key.txt";
        {   // owner-only from the start (the reference leaves its secret-key.txt to the umask)
            const int fd = ::open(sk_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
            if (fd >= 0) {
                (void)::fchmod(fd, 0600);
                ::close(fd);
            }
        }
        ofstream sk(sk_path, ios::out | ios::binary);
        if (!sk.is_open()) {
            cerr << "Error writing serialization of private key to secret-key.txt" << endl;
            exit(1);
        }
        sk << "fhelin-secret-seed ";
        for (int i = 0; i < 32; i++) sk << hex << setw(2) << setfill('0') << (int)seed[i];
        sk << dec << '\n';
        cout << "The secret key has been serialized." << std::endl;
    }
    void generate_context(int log_ring, int log_scale, int log_primes, int digits_hks, int cts_levels, int stc_levels, int relu_deg,
                          bool serialize = false) {
        (void)serialize;
        num_slots = 1 << 14;
        level_budget = {(uint32_t)cts_levels, (uint32_t)stc_levels};
        relu_degree = relu_deg;
        fhelin_params p = default_params();
        p.log_n = log_ring;
        p.first_bits = log_scale;
        p.scale_bits = log_primes;
        p.dnum = digits_hks;
        circuit_depth = p.n_q - 1;
        create(p);
        apply_seeded_keys();
        fhelin_shim::check(fhelin_keygen(context), "KeyGen");
        fhelin_shim::check(fhelin_gen_relin_key(context), "EvalMultKeyGen");
    }
    void load_context(bool verbose = true) {
        fhelin_params p = read_crypto_context();
        ifstream sk("../" + parameters_folder + "/secret-key.txt", ios::in | ios::binary);
        if (!sk.is_open()) {
            cerr << "I cannot read serialization from ../" << parameters_folder << "/secret-key.txt" << endl;
            exit(1);
        }
        string smagic, hexseed;
        sk >> smagic >> hexseed;
        uint8_t seed[32];
        if (!sk || smagic != "fhelin-secret-seed" || hexseed.size() != 64) {
            cerr << "Could not read secret key" << endl;
            exit(1);
        }
        for (int i = 0; i < 32; i++) seed[i] = (uint8_t)std::stoul(hexseed.substr(2 * i, 2), nullptr, 16);
        num_slots = 1 << 14;
        level_budget = {3, 3};
        circuit_depth = 12 + 14;  // the reference recomputes the depth without the +1 here (:226-230, quirk Q2)
        fhelin_ctx_destroy(context);
        context = nullptr;
        fhelin_shim::check(fhelin_ctx_create_seeded(&p, seed, &context), "GenCryptoContext");
        start_level_plan();
        apply_seeded_keys();
        fhelin_shim::check(fhelin_keygen(context), "KeyGen");
        fhelin_shim::check(fhelin_gen_relin_key(context), "EvalMultKeyGen");
        if (verbose) cout << "CtoS: " << level_budget[0] << ", StoC: " << level_budget[1] << endl;
    }

    /* Client / server split (include/fhelin.h "Evaluation-key sets").  The client, after generate_context and
     * generate_bootstrapping_and_rotation_keys, writes its public key and every switching key to ../<parameters_folder>/<filename>;
     * the server reads crypto-context.txt and that set and never opens secret-key.txt.  load_bootstrapping_and_rotation_keys then
     * works unchanged on the server (the keys it asks for are present); decrypt and the print* helpers throw, as OpenFHE does
     * without a secret key.
     * Seeded keys (include/fhelin.h "Seeded evaluation keys"): set_seeded_keys(true) before generate_context / load_context makes
     * every key's uniform half the expansion of a public key-set seed; save_evaluation_keys(filename, true) then writes the compact
     * set (b halves and the seed, half the bytes), which load_evaluation_context reads as it reads the full one. */
    void set_seeded_keys(bool on) { seeded_keys = on; }
    /* Level-capped keys (include/fhelin.h "Level-capped keys"), optional: set_key_caps(kind, galois, max_ell) before generate_context /
     * load_context hands the table to fhelin_ctx_set_key_caps ahead of the first key, so every key the reference's call sequence then
     * generates is made only as deep as the table says.  Nothing else changes: the same methods in the same order. */
    void set_key_caps(const vector<int32_t>& kind, const vector<uint64_t>& galois, const vector<int32_t>& max_ell) {
        if (kind.size() != galois.size() || kind.size() != max_ell.size()) throw std::runtime_error("set_key_caps: three arrays of one length");
        cap_kind = kind;
        cap_galois = galois;
        cap_max_ell = max_ell;
    }
    /* Interleaved samples (include/fhelin.h "Interleaved samples"): set_interleave(s) before generate_context / load_context /
     * load_evaluation_context makes every ciphertext carry s samples (s = 2, 4, ... with num_slots * s <= N/2).  The circuit, its
     * rotation indices and num_slots stay as they are (logical); encode / encrypt replicate their values into every sample (model
     * plaintexts, masks), encrypt_interleaved packs one vector per sample and decrypt_tovector_lanes returns every sample's slots
     * (decrypt_tovector: sample 0).  An evaluation-key set records the stride; load_evaluation_context adopts it. */
    void set_interleave(int stride) { interleave_stride = stride; }
    int interleave() const {
        int32_t s = interleave_stride > 0 ? interleave_stride : 1;
        if (context) fhelin_shim::check(fhelin_ctx_interleave(context, &s), "GetInterleave");
        return s;
    }
    Ctxt encrypt_interleaved(const vector<vector<double>>& samples, int level = 0, int plaintext_num_slots = 0) {
        if (plaintext_num_slots == 0) plaintext_num_slots = num_slots;
        if ((int)samples.size() != interleave()) throw std::runtime_error("encrypt_interleaved: one vector per sample (the interleave stride)");
        size_t n_per = 0;
        for (const auto& v : samples) n_per = std::max(n_per, v.size());
        vector<double> flat(samples.size() * n_per, 0.0);
        for (size_t i = 0; i < samples.size(); i++) std::copy(samples[i].begin(), samples[i].end(), flat.begin() + i * n_per);
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_encrypt_interleaved_batch(context, flat.data(), 1, (int32_t)n_per, level, plaintext_num_slots, &o),
                           "Encrypt (interleaved)");
        return wrap(o);
    }
    vector<vector<double>> decrypt_tovector_lanes(const Ctxt& c, int slots = 0) {
        if (slots == 0) slots = num_slots;
        const int s = interleave();
        vector<double> flat((size_t)s * slots);
        fhelin_shim::check(fhelin_decrypt_interleaved(context, c->h, 0, flat.data(), slots), "Decrypt (interleaved)");
        vector<vector<double>> out;
        for (int i = 0; i < s; i++) out.emplace_back(flat.begin() + (size_t)i * slots, flat.begin() + (size_t)(i + 1) * slots);
        return out;
    }
    void save_evaluation_keys(const string& filename, bool compact = false, bool packed = false) {
        const string path = "../" + parameters_folder + "/" + filename;
        fhelin_shim::check(packed    ? fhelin_evalkeys_save_packed(context, path.c_str(), compact ? 1 : 0)
                           : compact ? fhelin_evalkeys_save_compact(context, path.c_str())
                                     : fhelin_evalkeys_save(context, path.c_str()),
                           "Serialize(evaluation keys)");
    }
    void load_evaluation_context(const string& filename, bool verbose = true) {
        fhelin_params p = read_crypto_context();
        num_slots = 1 << 14;
        level_budget = {3, 3};
        circuit_depth = 12 + 14;  // as load_context
        create(p);                // this context's own generator (public-key encryption randomness): OS entropy
        apply_interleave();       // only when set_interleave was called: the set's own stride is adopted otherwise
        const string path = "../" + parameters_folder + "/" + filename;
        fhelin_shim::check(fhelin_evalkeys_load(context, path.c_str()), "Deserialize(evaluation keys)");
        if (verbose) cout << "Evaluation keys loaded from " << path << "; CtoS: " << level_budget[0] << ", StoC: " << level_budget[1] << endl;
    }

    /* rotation / bootstrapping keys (reference :237-343) */
    void generate_bootstrapping_keys(int bootstrap_slots) {
        fhelin_shim::check(fhelin_bootstrap_setup(context, (int)level_budget[0], (int)level_budget[1], bootstrap_slots), "EvalBootstrapSetup");
    }
    void generate_rotation_keys(vector<int> rotations, bool serialize = false, string filename = "") {
        if (serialize && filename.size() == 0) {
            cout << "Filename cannot be empty when serializing rotation keys." << endl;
            return;
        }
        // the reference's list (src/main.cpp:84) omits indices the circuit uses (quirk Q3): generate the union, plus the
        // 3*2^i (and 5s, 7s) rotations that let the engine run two (three) steps of a rotate-and-sum tree as one merged key switch
        vector<int32_t> all(rotations.begin(), rotations.end());
        for (int i = 0; i < 14; i++) {
            all.push_back(1 << i);
            all.push_back(-(1 << i));
        }
        for (int i = 0; i < 13; i++) {
            all.push_back(3 << i);
            all.push_back(-(3 << i));
        }
        for (int s : {1, 8, 128, 512, 1024})  // with s..7s three tree steps run as one merged key switch (6s = 3 * 2s is above)
            for (int m : {5, 7}) {
                all.push_back(m * s);
                all.push_back(-m * s);
            }
        fhelin_shim::check(fhelin_gen_rotation_keys(context, all.data(), (int32_t)all.size()), "EvalRotateKeyGen");
        if (serialize) {
            ofstream f("../" + parameters_folder + "/rot_" + filename, ios::out | ios::binary);
            if (!f.is_open()) {
                cerr << "Error serializing Rotation keys" << "../" + parameters_folder + "/rot_" + filename << std::endl;
                exit(1);
            }
            f << "fhelin-rotations " << all.size();
            for (int r : all) f << ' ' << r;
            f << '\n';
        }
    }
    void generate_bootstrapping_and_rotation_keys(vector<int> rotations, int bootstrap_slots, bool serialize, const string& filename) {
        if (serialize && filename.empty()) {
            cout << "Filename cannot be empty when serializing bootstrapping and rotation keys." << endl;
            return;
        }
        generate_bootstrapping_keys(bootstrap_slots);
        generate_rotation_keys(rotations, serialize, filename);
    }
    void load_bootstrapping_and_rotation_keys(const string& filename, int bootstrap_slots, bool verbose) {
        auto start = start_time();
        generate_bootstrapping_keys(bootstrap_slots);
        load_rotation_keys(filename, false);
        if (verbose) print_duration(start, "Loading bootstrapping pre-computations + rotations");
    }
    void load_rotation_keys(const string& filename, bool verbose) {
        auto start = start_time();
        ifstream f("../" + parameters_folder + "/rot_" + filename, ios::in | ios::binary);
        if (!f.is_open()) {
            cerr << "Cannot read serialization from " << "../" + parameters_folder + "/rot_" + filename << std::endl;
            exit(1);
        }
        string magic;
        size_t n = 0;
        f >> magic >> n;
        vector<int32_t> idx(n);
        for (auto& r : idx) f >> r;
        if (!f || magic != "fhelin-rotations") {
            cerr << "Could not deserialize eval rot key file" << std::endl;
            exit(1);
        }
        fhelin_shim::check(fhelin_gen_rotation_keys(context, idx.data(), (int32_t)idx.size()), "EvalRotateKeyGen");
        if (verbose) print_duration(start, "Loading rotation keys");
    }
    void clear_bootstrapping_and_rotation_keys(int) {}
    void clear_rotation_keys() {}
    void clear_context(int) {}

    /* CKKS encoding / encryption (reference :348-404) */
    Ptxt encode(const vector<double>& vec, int level, int plaintext_num_slots) {
        if (plaintext_num_slots == 0) plaintext_num_slots = num_slots;
        fhelin_pt* h = nullptr;
        fhelin_shim::check(fhelin_encode(context, vec.data(), (int32_t)vec.size(), level, plaintext_num_slots, &h), "MakeCKKSPackedPlaintext");
        vector<double> v(vec);
        v.resize(plaintext_num_slots, 0.0);
        return std::make_shared<fhelin_shim::PlaintextImpl>(context, h, std::move(v));
    }
    Ptxt encode(double val, int level, int plaintext_num_slots) {
        if (plaintext_num_slots == 0) plaintext_num_slots = num_slots;
        return encode(vector<double>(plaintext_num_slots, val), level, plaintext_num_slots);
    }
    Ctxt encrypt(const vector<double>& vec, int level = 0, int plaintext_num_slots = 0) {
        return encrypt_ptxt(encode(vec, level, plaintext_num_slots));
    }
    Ctxt encrypt_ptxt(const Ptxt& p) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_encrypt(context, p->h, &o), "Encrypt");
        return wrap(o);
    }
    Ptxt decrypt(const Ctxt& c) {
        int slots = c->GetSlots() ? (int)c->GetSlots() : num_slots;
        vector<double> v(slots);
        fhelin_shim::check(fhelin_decrypt(context, c->h, v.data(), slots), "Decrypt");
        return std::make_shared<fhelin_shim::PlaintextImpl>(context, nullptr, std::move(v));
    }
    vector<double> decrypt_tovector(const Ctxt& c, int slots) {
        if (slots == 0) slots = num_slots;
        vector<double> v(slots);
        fhelin_shim::check(fhelin_decrypt(context, c->h, v.data(), slots), "Decrypt");
        return v;
    }
    /* noise-flooding decryption (fhelin.h "Sanitised replies"): a uniform term on [-2^flood_bits, 2^flood_bits) per coefficient is added
     * to the phase before it leaves the device, so that values the client shares do not expose the exact noise.  flood_bits = 0:
     * decrypt_tovector. */
    vector<double> decrypt_tovector_flooded(const Ctxt& c, int slots, int flood_bits) {
        if (slots == 0) slots = num_slots;
        vector<double> v(slots);
        fhelin_shim::check(fhelin_decrypt_flooded(context, c->h, flood_bits, v.data(), slots), "Decrypt (flooded)");
        return v;
    }
    /* The reply form of a result (fhelin.h "Sanitised replies"): only keep_slots survive (every other slot is masked out; empty = no
     * mask), out_ell limbs remain, a fresh public-key encryption of zero and a flood term of flood_bits bits are added.  Runs on a
     * server without the secret key; nothing else in this class calls it. */
    Ctxt sanitize(const Ctxt& c, const vector<int>& keep_slots, int flood_bits, int out_ell = 2) {
        fhelin_pt* m = nullptr;
        Ptxt mask;
        if (!keep_slots.empty()) {
            const int slots = c->GetSlots() ? (int)c->GetSlots() : num_slots;
            vector<double> v(slots, 0.0);
            for (int k : keep_slots) {
                if (k < 0 || k >= slots) throw std::runtime_error("sanitize: slot index outside the ciphertext's slots");
                v[k] = 1.0;
            }
            mask = encode(v, 0, slots);
            m = mask->h;
        }
        const fhelin_ct* in = c->h;
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_sanitize(context, &in, 1, m, flood_bits, out_ell, &o), "Sanitize");
        return wrap(o);
    }

    /* homomorphic operations (reference :409-469) */
    Ctxt add(const Ctxt& c1, const Ctxt& c2) { return bin(fhelin_add, c1, c2, "EvalAdd"); }
    Ctxt add(const Ctxt& c1, const Ptxt& c2) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_add_plain(context, c1->h, c2->h, &o), "EvalAdd");
        return wrap(o);
    }
    Ctxt add(vector<Ctxt> c) {
        auto hs = handles(c);
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_fc_add_many(context, hs.data(), (int32_t)hs.size(), &o), "EvalAddMany");
        return wrap(o);
    }
    Ctxt mult(const Ctxt& c1, const Ctxt& c2) { return bin(fhelin_mult, c1, c2, "EvalMult"); }
    Ctxt mult(const Ctxt& c, double d) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_fc_mult_const(context, c->h, d, &o), "EvalMult");
        return wrap(o);
    }
    Ctxt mult(const Ctxt& c, const Ptxt& p) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_mult_plain(context, c->h, p->h, &o), "EvalMult");
        return wrap(o);
    }
    Ctxt rotate(const Ctxt& c, int index) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_rotate(context, c->h, index, &o), "EvalRotate");
        return wrap(o);
    }
    Ctxt bootstrap(const Ctxt& c, bool timing = false) {
        auto start = start_time();
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_bootstrap(context, c->h, &o), "EvalBootstrap");
        if (timing) print_duration(start, "Bootstrapping " + to_string(c->GetSlots()) + " slots");
        return wrap(o);
    }
    // paired bootstrapping (include/fhelin.h fhelin_ctx_set_bootstrap_pairing; off by default), once the context exists: bootstrap(c) calls on
    // real ciphertexts that are evaluated together travel two per pipeline
    void set_bootstrap_pairing(bool on) { fhelin_shim::check(fhelin_ctx_set_bootstrap_pairing(context, on ? 1 : 0), "SetBootstrapPairing"); }
    // EvalBootstrap(c, 2, precision): the iterative bootstrap (include/fhelin.h fhelin_bootstrap_iter), one limb fewer than bootstrap(c)
    Ctxt bootstrap(const Ctxt& c, int precision, bool timing = false) {
        if (static_cast<int>(c->GetLevel()) + 2 < circuit_depth)
            cout << "You are bootstrapping with remaining levels! You are at " << to_string(c->GetLevel()) << "/" << circuit_depth - 2 << endl;
        auto start = start_time();
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_bootstrap_iter(context, c->h, precision, &o), "EvalBootstrap");
        if (timing) print_duration(start, "Double Bootstrapping " + to_string(c->GetSlots()) + " slots");
        return wrap(o);
    }
    Ctxt relu(const Ctxt& c, double scale, bool timing = false) {
        auto start = start_time();
        Ctxt res = chebyshev([scale](double x) -> double { return x < 0 ? 0 : (1 / scale) * x; }, c, -1, 1, relu_degree);
        if (timing) print_duration(start, "ReLU d = " + to_string(relu_degree) + " evaluation");
        return res;
    }

    /* text I/O and packing layouts (reference :501-698) */
    Ctxt read_input(const string& filename, double scale = 1) {
        vector<double> input = read_values_from_file(filename);
        for (auto& v : input) v *= scale;
        return encrypt(input, circuit_depth - 10, num_slots);
    }
    Ctxt read_repeated_input(const string& filename, double scale = 1) {
        vector<double> input = read_values_from_file(filename);  // the reference encrypts `input`, not `repeated` (quirk Q7)
        for (auto& v : input) v *= scale;
        return encrypt(input, 0, num_slots);
    }
    Ctxt read_expanded_input(const string& filename, double scale = 1) { return encrypt(expanded(filename, scale, 128), 0, num_slots); }
    Ptxt read_plain_input(const string& filename, int level = 0, double scale = 1) {
        vector<double> input = read_values_from_file(filename);
        for (auto& v : input) v *= scale;
        return encode(input, level, num_slots);
    }
    vector<Ptxt> read_plain_256_input(const string& filename, int level = 0, double scale = 1) {
        vector<double> input = read_values_from_file(filename);
        need(input, 256, filename);
        for (auto& v : input) v *= scale;
        vector<double> a(input.begin(), input.begin() + 128), b(input.begin() + 128, input.begin() + 256);
        return {encode(a, level, num_slots), encode(b, level, num_slots)};
    }
    Ptxt read_plain_repeated_input(const string& filename, int level = 0, double scale = 1) {
        vector<double> input = read_values_from_file(filename);
        need(input, 128, filename);
        vector<double> rep;
        for (int j = 0; j < 128; j++)
            for (int i = 0; i < 128; i++) rep.push_back(input[i] * scale);
        return encode(rep, level, num_slots);
    }
    Ptxt read_plain_repeated_512_input(const string& filename, int level = 0, double scale = 1) {
        vector<double> input = read_values_from_file(filename);
        need(input, 512, filename);
        vector<double> rep;
        for (int j = 0; j < 32; j++)
            for (int i = 0; i < 512; i++) rep.push_back(input[i] * scale);
        return encode(rep, level, num_slots);
    }
    Ptxt read_plain_expanded_input(const string& filename, int level = 0, double scale = 1) {
        return encode(expanded(filename, scale, 128), level, num_slots);
    }
    Ptxt read_plain_expanded_input(const string& filename, int level, double scale, int num_inputs) {
        return encode(expanded(filename, scale, num_inputs), level, num_slots);
    }

    /* debug printing: decrypts with the secret key on the "server", as the reference does (:700-826, quirk Q5) */
    void print(const Ctxt& c, int slots = 0, string prefix = "") {
        if (slots == 0) slots = num_slots;
        cout << prefix << " (Lv. " << c->GetLevel() << ") ";
        vector<double> v = decrypt_tovector(c, num_slots);
        cout << setprecision(4) << fixed << "[ ";
        for (int i = 0; i < slots; i++) print_slot(v[i], i == slots - 1, " 0.0000");
        cout << endl;
    }
    void print_padded(const Ctxt& c, int slots = 0, int padding = 1, string prefix = "") {
        if (slots == 0) slots = num_slots;
        cout << prefix;
        vector<double> v = decrypt_tovector(c, num_slots);
        cout << setprecision(10) << fixed << "[ ";
        for (int i = 0; i < slots * padding && i < (int)v.size(); i += padding) print_slot(v[i], i == slots - 1, " 0.000");
        cout << endl;
    }
    void print_expanded(const Ctxt& c, int slots = 0, int expansion_factor = 1, string prefix = "") {
        if (slots == 0) slots = num_slots;
        cout << prefix << " (Lv. " << c->GetLevel() << ") ";
        vector<double> v = decrypt_tovector(c, num_slots);
        cout << setprecision(4) << fixed << "[ ";
        for (int i = 0; i < slots; i++)
            if (i % expansion_factor == 0) print_slot(v[i], i == slots - 1, " 0.000");
        cout << " ]" << endl;
    }
    void print_min_max(const Ctxt& c) {
        vector<double> v = decrypt_tovector(c, (int)c->GetSlots() ? (int)c->GetSlots() : num_slots);
        cout << "min: " << *min_element(v.begin(), v.end()) << ", max: " << *max_element(v.begin(), v.end()) << endl;
    }

    /* rotate-and-sum reductions and matmuls (reference :829-1058) */
    Ctxt rotsum(const Ctxt& in, int slots, int padding) { return un2(fhelin_fc_rotsum, in, slots, padding, "rotsum"); }
    Ctxt rotsum_padded(const Ctxt& in, int slots) { return un2(fhelin_fc_rotsum, in, slots, slots, "rotsum_padded"); }
    Ctxt repeat(const Ctxt& in, int slots) { return un2(fhelin_fc_repeat, in, slots, 1, "repeat"); }
    Ctxt repeat(const Ctxt& in, int slots, int padding) { return un2(fhelin_fc_repeat, in, slots, padding, "repeat"); }

    vector<Ctxt> matmulRE(vector<Ctxt> rows, const Ptxt& weight, const Ptxt& bias) { return mm_pt(rows, weight, bias, 128, 128); }
    vector<Ctxt> matmulRE(vector<Ctxt> rows, const Ptxt& weight, const Ptxt& bias, int row_size, int padding) {
        return mm_pt(rows, weight, bias, row_size, padding);
    }
    vector<Ctxt> matmulRE(vector<Ctxt> rows, const Ctxt& weight, int row_size, int padding) { return mm_ct(rows, weight, row_size, padding); }
    vector<Ctxt> matmulRElarge(vector<Ctxt>& rows, const vector<Ptxt>& weight, const Ptxt& bias, double mask_value = 1) {
        auto hs = handles(rows);
        vector<const fhelin_pt*> ws;
        for (auto& w : weight) ws.push_back(w->h);
        vector<fhelin_ct*> outs(rows.size());
        fhelin_shim::check(fhelin_fc_matmulRElarge(context, hs.data(), (int32_t)hs.size(), ws.data(), (int32_t)ws.size(),
                                                   bias ? bias->h : nullptr, mask_value, outs.data()), "matmulRElarge");
        return wrap_all(outs);
    }
    vector<Ctxt> matmulCR(vector<Ctxt> rows, const Ptxt& weight, const Ptxt& bias) { return mm_pt(rows, weight, bias, 128, 1); }
    vector<Ctxt> matmulCR(vector<Ctxt> rows, const Ctxt& matrix) { return mm_ct(rows, matrix, 64, 1); }
    vector<Ctxt> matmulCR_128(vector<Ctxt> rows, const Ctxt& matrix) { return mm_ct(rows, matrix, 128, 1); }
    Ctxt matmulCR_128(Ctxt row, const Ctxt& matrix) { return mm_ct({row}, matrix, 128, 1)[0]; }
    vector<Ctxt> matmulCRlarge(vector<vector<Ctxt>> rows, vector<Ptxt> weights, const Ptxt& bias) {
        vector<const fhelin_ct*> hs;
        for (auto& r : rows)
            for (int j = 0; j < 4; j++) hs.push_back(r.at(j)->h);
        vector<const fhelin_pt*> ws;
        for (auto& w : weights) ws.push_back(w->h);
        if (ws.size() < 4) throw std::runtime_error("matmulCRlarge: need 4 weight blocks");
        vector<fhelin_ct*> outs(rows.size());
        fhelin_shim::check(fhelin_fc_matmulCRlarge(context, hs.data(), (int32_t)rows.size(), ws.data(), bias ? bias->h : nullptr, outs.data()),
                           "matmulCRlarge");
        return wrap_all(outs);
    }
    Ctxt matmulScores(vector<Ctxt> queries, const Ctxt& key) {
        auto hs = handles(queries);
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_fc_matmulScores(context, hs.data(), (int32_t)hs.size(), key->h, &o), "matmulScores");
        return wrap(o);
    }
    Ctxt matmulScores(Ctxt query, const Ctxt& key) { return matmulScores(vector<Ctxt>{query}, key); }

    /* layout shuffles (reference :1060-1205) */
    Ctxt wrapUpRepeated(vector<Ctxt> vectors) { return many(fhelin_fc_wrapUpRepeated, vectors, "wrapUpRepeated"); }
    Ctxt wrapUpExpanded(vector<Ctxt> vectors) { return many(fhelin_fc_wrapUpExpanded, vectors, "wrapUpExpanded"); }
    vector<Ctxt> unwrapExpanded(Ctxt c, int inputs_num) {
        vector<fhelin_ct*> outs(inputs_num);
        fhelin_shim::check(fhelin_fc_unwrapExpanded(context, c->h, inputs_num, outs.data()), "unwrapExpanded");
        return wrap_all(outs);
    }
    vector<Ctxt> unwrapScoresExpanded(Ctxt c, int inputs_num) {
        vector<fhelin_ct*> outs(inputs_num);
        fhelin_shim::check(fhelin_fc_unwrapScoresExpanded(context, c->h, inputs_num, outs.data()), "unwrapScoresExpanded");
        return wrap_all(outs);
    }
    vector<Ctxt> unwrap_512_in_4_128(const Ctxt& c, int index) {
        vector<fhelin_ct*> outs(4);
        fhelin_shim::check(fhelin_fc_unwrap_512_in_4_128(context, c->h, index, outs.data()), "unwrap_512_in_4_128");
        return wrap_all(outs);
    }
    vector<vector<Ctxt>> unwrapRepeatedLarge(vector<Ctxt> c, int input_number) {
        auto hs = handles(c);
        vector<fhelin_ct*> outs((size_t)4 * input_number);
        fhelin_shim::check(fhelin_fc_unwrapRepeatedLarge(context, hs.data(), (int32_t)hs.size(), input_number, outs.data()), "unwrapRepeatedLarge");
        vector<vector<Ctxt>> res;
        for (int i = 0; i < input_number; i++) {
            vector<Ctxt> four;
            for (int j = 0; j < 4; j++) four.push_back(wrap(outs[4 * i + j]));
            res.push_back(four);
        }
        return res;
    }
    vector<Ctxt> generate_containers(vector<Ctxt> inputs, const Ptxt& bias) {
        cout << "inputs.size(): " << inputs.size() << endl;
        auto hs = handles(inputs);
        vector<fhelin_ct*> outs((inputs.size() + 31) / 32);
        int32_t n = 0;
        fhelin_shim::check(fhelin_fc_generate_containers(context, hs.data(), (int32_t)hs.size(), bias ? bias->h : nullptr, outs.data(), &n),
                           "generate_containers");
        outs.resize(n);
        return wrap_all(outs);
    }
    Ctxt wrap_containers(vector<Ctxt> inputs, int inputs_number) {
        auto hs = handles(inputs);
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_fc_wrap_containers(context, hs.data(), (int32_t)hs.size(), inputs_number, &o), "wrap_containers");
        return wrap(o);
    }

    /* masks (reference :1207-1286) */
    Ctxt mask_block(const Ctxt& c, int from, int to, double mask_value = 1) { return mask(c, 0, from, to, mask_value); }
    Ctxt mask_heads(const Ctxt& c, double mask_value = 1) { return mask(c, 1, 0, 0, mask_value); }
    Ctxt mask_heads_128(const Ctxt& c, double mask_value = 1) { return mask(c, 2, 0, 0, mask_value); }
    Ctxt mask_mod_n(const Ctxt& c, int n) { return mask(c, 3, n, 0, 1); }
    Ctxt mask_mod_n(const Ctxt& c, int n, int padding, int max_slots) {
        (void)max_slots;  // ignored by the reference too (:1262-1273, quirk Q7)
        return mask(c, 3, n, padding, 1);
    }
    Ctxt mask_first_n(const Ctxt& c, int n, double mask_value = 1) { return mask(c, 4, n, 0, mask_value); }

    /* polynomial / Chebyshev activations (reference :1289-1336) */
    Ctxt eval_exp(const Ctxt& c, int inputs_number) {
        const double coeffs[7] = {1, 1, 1 / 2.0, 1 / 6.0, 1 / 24.0, 1 / 120.0, 1 / 720.0};
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_eval_poly(context, c->h, coeffs, 7, &o), "EvalPoly");
        Ctxt res = wrap(o);
        if ((int)res->GetLevel() + 4 > circuit_depth) res = bootstrap(res);
        vector<const fhelin_ct*> eight(8, res->h);
        fhelin_shim::check(fhelin_mult_many(context, eight.data(), 8, &o), "EvalMultMany");
        res = wrap(o);
        vector<double> m;
        for (int i = 0; i < num_slots; i++) m.push_back((i % 128 < inputs_number && i < (128 * inputs_number)) ? 0 : -1);
        return add(res, encode(m, (int)res->GetLevel(), num_slots));
    }
    Ctxt eval_inverse(const Ctxt& c, double min, double max) {
        double middle = (max - min) / 2;
        Ctxt res = add(c, encode(-middle - min, (int)c->GetLevel(), num_slots));
        res = mult(res, encode(1 / middle, (int)res->GetLevel(), num_slots));
        return chebyshev([](double x) -> double { return 1 / ((x * 9895) + 9995); }, res, -1, 1, 200);
    }
    Ctxt eval_inverse_naive(const Ctxt& c, double min, double max) {
        return chebyshev([](double x) -> double { return 1 / x; }, c, min, max, 119);
    }
    Ctxt eval_inverse_naive_2(const Ctxt& c, double min, double max, double mult) {
        return chebyshev([mult](double x) -> double { return mult / x; }, c, min, max, 200);
    }
    Ctxt eval_gelu_function(const Ctxt& c, double min, double max, double mult, int degree) {
        return chebyshev([mult](double x) -> double { return (0.5 * (x * (1 / mult)) * (1 + erf((x * (1 / mult)) / 1.41421356237))); }, c, min,
                         max, degree);
    }
    Ctxt eval_tanh_function(const Ctxt& c, double min, double max, double mult, int degree) {
        return chebyshev([mult](double x) -> double { return tanh(x * (1 / mult)); }, c, min, max, degree);
    }

    vector<Ctxt> slicing(vector<Ctxt>& arr, int X, int Y) {
        if (Y - X >= (int)arr.size()) return arr;
        if (Y > (int)arr.size()) Y = (int)arr.size();
        return vector<Ctxt>(arr.begin() + X, arr.begin() + Y);
    }

    /* ciphertext checkpoint (reference :1360-1394) in the engine's own format */
    void save(Ctxt v, string filename) { save(vector<Ctxt>{v}, filename); }
    void save(vector<Ctxt> v, string filename) {
        ofstream f(filename, ios::out | ios::binary);
        if (!f.is_open()) return;
        uint64_t magic = 0x46484C4E43543031ull, n = v.size();
        f.write((const char*)&magic, 8);
        f.write((const char*)&n, 8);
        for (auto& c : v) {
            int32_t npoly, ell, level, deg, slots;
            double scale;
            fhelin_ct_info(c->h, &npoly, &ell, &level, &deg, &scale, &slots);
            fhelin_params p;
            fhelin_ctx_info(context, &p, nullptr, nullptr);
            vector<uint64_t> limbs((size_t)npoly * ell << p.log_n);
            fhelin_shim::check(fhelin_ct_export(context, c->h, limbs.data(), limbs.size()), "Serialize");
            int32_t hdr[5] = {npoly, ell, deg, slots, p.log_n};
            f.write((const char*)hdr, sizeof hdr);
            f.write((const char*)&scale, 8);
            f.write((const char*)limbs.data(), (streamsize)(limbs.size() * 8));
        }
    }
    /* Compact inputs (include/fhelin.h "Compact ciphertexts"): with seeded encryption on, encrypt / read_expanded_input encrypt with
     * the secret key and c1 expanded from a public seed, and save_compact writes c0, the seed and the nonce of each, half the bytes
     * of save().  File: magic, count, then per ciphertext a u64 byte length and the blob.  load_vector / load_ciphertext read both
     * formats; a compact file is imported in one batched call (all or nothing).  The server needs no secret to load one. */
    void set_seeded_encryption(bool on) { fhelin_shim::check(fhelin_ctx_set_seeded_encryption(context, on ? 1 : 0), "SetSeededEncryption"); }
    void save_compact(vector<Ctxt> v, string filename) {
        ofstream f(filename, ios::out | ios::binary);
        if (!f.is_open()) throw std::runtime_error("save_compact: cannot create " + filename);
        uint64_t magic = COMPACT_FILE_MAGIC, n = v.size();
        f.write((const char*)&magic, 8);
        f.write((const char*)&n, 8);
        vector<uint8_t> blob;
        for (auto& c : v) {
            size_t bytes = 0;
            fhelin_shim::check(fhelin_ct_compact_bytes(c->h, &bytes), "Serialize(compact)");
            blob.resize(bytes);
            fhelin_shim::check(fhelin_ct_export_compact(context, c->h, blob.data(), bytes), "Serialize(compact)");
            const uint64_t len = bytes;
            f.write((const char*)&len, 8);
            f.write((const char*)blob.data(), (streamsize)bytes);
        }
        if (!f) throw std::runtime_error("save_compact: write to " + filename + " failed");
    }
    /* Packed ciphertexts (include/fhelin.h "Packed formats"): every residue at its modulus width, the exact 80-bit scale and a digest.
     * Each blob takes the seeded form when the handle has one (an unmodified seeded encryption, a wrapped input) and the full form
     * otherwise.  File: a magic of its own, count, then per ciphertext a u64 byte length and the blob; load_vector reads it through
     * one batched import (all or nothing). */
    void save_packed(vector<Ctxt> v, string filename) {
        ofstream f(filename, ios::out | ios::binary);
        if (!f.is_open()) throw std::runtime_error("save_packed: cannot create " + filename);
        uint64_t magic = PACKED_FILE_MAGIC, n = v.size();
        f.write((const char*)&magic, 8);
        f.write((const char*)&n, 8);
        vector<uint8_t> blob;
        try {
            for (auto& c : v) {
                // the seeded form where the handle has one: asking for its size is the test (FHELIN_ERR_STATE otherwise, which only
                // leaves a message in fhelin_last_error that the next failing call overwrites); any other handle takes the full form
                size_t bytes = 0;
                const int32_t seeded = fhelin_ct_packed_bytes(context, c->h, 1, &bytes) == FHELIN_OK ? 1 : 0;
                if (!seeded) fhelin_shim::check(fhelin_ct_packed_bytes(context, c->h, 0, &bytes), "Serialize(packed)");
                blob.resize(bytes);
                fhelin_shim::check(fhelin_ct_export_packed(context, c->h, seeded, blob.data(), bytes), "Serialize(packed)");
                const uint64_t len = bytes;
                f.write((const char*)&len, 8);
                f.write((const char*)blob.data(), (streamsize)bytes);
            }
            if (!f) throw std::runtime_error("save_packed: write to " + filename + " failed");
        } catch (...) {   // no partial file stays behind
            f.close();
            std::remove(filename.c_str());
            throw;
        }
    }
    vector<Ctxt> load_vector(string filename) {
        vector<Ctxt> result;
        ifstream f(filename, ios::in | ios::binary);
        uint64_t magic = 0, n = 0;
        if (f.is_open()) {
            f.read((char*)&magic, 8);
            f.read((char*)&n, 8);
        }
        if (f && (magic == COMPACT_FILE_MAGIC || magic == PACKED_FILE_MAGIC)) {
            const bool packed = magic == PACKED_FILE_MAGIC;
            vector<vector<uint8_t>> blobs;
            for (uint64_t i = 0; i < n; i++) {
                uint64_t len = 0;
                f.read((char*)&len, 8);
                if (!f || len > ((uint64_t)1 << 36)) throw std::runtime_error("Deserialize(compact): truncated " + filename);
                blobs.emplace_back(len);
                f.read((char*)blobs.back().data(), (streamsize)len);
                if (!f) throw std::runtime_error("Deserialize(compact): truncated " + filename);
            }
            vector<const uint8_t*> ptrs;
            vector<size_t> sizes;
            for (auto& b : blobs) {
                ptrs.push_back(b.data());
                sizes.push_back(b.size());
            }
            vector<fhelin_ct*> outs(blobs.size(), nullptr);
            fhelin_shim::check(packed ? fhelin_ct_import_packed(context, ptrs.data(), sizes.data(), (int32_t)blobs.size(), outs.data())
                                      : fhelin_ct_import_compact(context, ptrs.data(), sizes.data(), (int32_t)blobs.size(), outs.data()),
                               packed ? "Deserialize(packed)" : "Deserialize(compact)");
            for (fhelin_ct* o : outs) result.push_back(wrap(o));
            return result;
        }
        if (!f || magic != 0x46484C4E43543031ull) {
            cerr << "Could not find \"" << filename << "\"" << endl;
            return result;
        }
        for (uint64_t i = 0; i < n; i++) {
            int32_t hdr[5];
            double scale;
            f.read((char*)hdr, sizeof hdr);
            f.read((char*)&scale, 8);
            vector<uint64_t> limbs((size_t)hdr[0] * hdr[1] << hdr[4]);
            f.read((char*)limbs.data(), (streamsize)(limbs.size() * 8));
            if (!f) break;
            fhelin_ct* o = nullptr;
            fhelin_shim::check(fhelin_ct_import(context, limbs.data(), hdr[0], hdr[1], hdr[2], scale, hdr[3], &o), "Deserialize");
            result.push_back(wrap(o));
        }
        return result;
    }
    Ctxt load_ciphertext(string filename) {
        vector<Ctxt> v = load_vector(filename);
        return v.empty() ? Ctxt() : v[0];
    }

    static constexpr uint64_t COMPACT_FILE_MAGIC = 0x46484C4E43433031ull;
    static constexpr uint64_t PACKED_FILE_MAGIC = 0x46484C4E43503031ull;

    int relu_degree = 119;
    string parameters_folder = "keys";

    /* not part of the reference API: the engine handle, for tests and benchmarks */
    fhelin_ctx* engine() { return context; }

    /* EvalChebyshevCoefficients + EvalChebyshevSeries: coefficients fitted on the host (fp64), series on the GPU */
    Ctxt chebyshev(std::function<double(double)> func, const Ctxt& c, double a, double b, int degree) {
        const int n = degree + 1;
        const double pi = 3.14159265358979323846, bma = 0.5 * (b - a), bpa = 0.5 * (b + a);
        vector<double> fx(n), coeff(n);
        for (int i = 0; i < n; i++) fx[i] = func(std::cos(pi * (i + 0.5) / n) * bma + bpa);
        for (int k = 0; k < n; k++) {
            double s = 0;
            for (int j = 0; j < n; j++) s += fx[j] * std::cos(pi * k * (j + 0.5) / n);
            coeff[k] = 2.0 * s / n;
        }
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_eval_chebyshev(context, c->h, coeff.data(), n, a, b, &o), "EvalChebyshevFunction");
        return wrap(o);
    }

private:
    vector<uint32_t> level_budget = {4, 4};

    fhelin_params read_crypto_context() {
        ifstream f("../" + parameters_folder + "/crypto-context.txt", ios::in | ios::binary);
        if (!f.is_open()) {
            cerr << "I cannot find ../" << parameters_folder << "/crypto-context.txt" << endl;
            exit(1);
        }
        string magic;
        int ver = 0;
        fhelin_params p = default_params();
        f >> magic >> ver >> p.log_n >> p.n_q >> p.first_bits >> p.scale_bits >> p.n_p >> p.special_bits >> p.dnum >> p.log_slots >>
            p.hamming;
        if (!f || magic != "fhelin-context" || ver != 2) {
            cerr << "Error reading serialization of the crypto context from crypto-context.txt" << endl;
            exit(1);
        }
        return p;
    }
    static fhelin_params default_params() {
        fhelin_params p;
        const char* preset = std::getenv("FHELIN_PRESET");
        const bool bench = preset && string(preset) == "bench";
        p.log_n = bench ? 16 : 15;
        p.n_q = 28;  // circuit_depth 27 + 1, the reference's chain (:27-31)
        p.first_bits = 55;
        p.scale_bits = 52;
        p.n_p = -1;  // OpenFHE's sizeP rule: 7 special limbs for this chain (367-bit digit / 60)
        p.special_bits = 60;
        p.dnum = 4;
        p.log_slots = 14;
        p.hamming = 192;
        const char* dev = std::getenv("FHELIN_DEVICE");
        p.device = dev ? std::atoi(dev) : 0;
        const char* seed = std::getenv("FHELIN_SEED");   // explicit deterministic TEST seed; default 0 = OS entropy
        p.seed = seed ? std::strtoull(seed, nullptr, 10) : 0ull;
        return p;
    }
    bool seeded_keys = false;   // set_seeded_keys: applied between context creation and keygen
    int interleave_stride = 0;  // set_interleave: applied there too (0: not set, the context's default of 1 or a key set's own)
    vector<int32_t> cap_kind, cap_max_ell;   // set_key_caps: applied there too
    vector<uint64_t> cap_galois;
    void apply_seeded_keys() {   // the settings a fresh context takes before its first key: seeded keys, interleaved samples
        if (seeded_keys) fhelin_shim::check(fhelin_ctx_set_seeded_keys(context, 1), "SetSeededKeys");
        if (!cap_kind.empty())
            fhelin_shim::check(fhelin_ctx_set_key_caps(context, cap_kind.data(), cap_galois.data(), cap_max_ell.data(), (int32_t)cap_kind.size()),
                               "SetKeyCaps");
        apply_interleave();
    }
    void apply_interleave() {
        if (interleave_stride > 0) fhelin_shim::check(fhelin_ctx_set_interleave(context, interleave_stride), "SetInterleave");
    }
    void create(const fhelin_params& p) {
        fhelin_ctx_destroy(context);
        context = nullptr;
        fhelin_shim::check(fhelin_ctx_create(&p, &context), "GenCryptoContext");
        start_level_plan();
    }
    /* Level plan (include/fhelin.h fhelin_level_plan_*), opt-in: FHELIN_LEVEL_PLAN=<file>.  A driver process is ONE pass of a
     * straight-line program (src/main.cpp:145-475): the first run with the variable set records the pass and writes the plan
     * when the controller goes away; later runs of the same driver find the file and apply it — fresh encryptions and
     * bootstrap outputs then start with the limbs their consumers read.  Delete the file when the driver changes. */
    string level_plan_file;
    bool level_plan_recording = false;
    void start_level_plan() {
        const char* f = std::getenv("FHELIN_LEVEL_PLAN");
        if (!f || !*f) return;
        level_plan_file = f;
        ifstream in(level_plan_file);
        string magic;
        int n = 0;
        if (in.is_open() && (in >> magic >> n) && magic == "fhelin-level-plan" && n >= 0) {
            vector<int32_t> t(n);
            for (int i = 0; i < n; i++) in >> t[i];
            if (in) {
                fhelin_shim::check(fhelin_level_plan_set(context, t.data(), n), "level plan (load)");
                fhelin_shim::check(fhelin_level_plan_begin(context, 2), "level plan (apply)");
                cout << "Level plan " << level_plan_file << " applied (" << n << " sources)." << endl;
                return;
            }
        }
        fhelin_shim::check(fhelin_level_plan_begin(context, 1), "level plan (record)");
        level_plan_recording = true;
    }
    void save_level_plan() {
        if (!context || !level_plan_recording) return;
        level_plan_recording = false;
        int32_t n = 0;
        if (fhelin_level_plan_end(context, &n) != FHELIN_OK || n <= 0) return;
        vector<int32_t> t(n);
        if (fhelin_level_plan_get(context, t.data(), n, &n) != FHELIN_OK) return;
        ofstream out(level_plan_file);
        out << "fhelin-level-plan " << n << '\n';
        for (int i = 0; i < n; i++) out << t[i] << (i + 1 < n ? ' ' : '\n');
        cout << "Level plan recorded to " << level_plan_file << " (" << n << " sources)." << endl;
    }
    Ctxt wrap(fhelin_ct* h) { return std::make_shared<fhelin_shim::CiphertextImpl>(context, h); }
    vector<Ctxt> wrap_all(const vector<fhelin_ct*>& hs) {
        vector<Ctxt> v;
        for (auto* h : hs) v.push_back(wrap(h));
        return v;
    }
    static vector<const fhelin_ct*> handles(const vector<Ctxt>& v) {
        vector<const fhelin_ct*> hs;
        for (auto& c : v) hs.push_back(c->h);
        return hs;
    }
    template <class F> Ctxt bin(F f, const Ctxt& a, const Ctxt& b, const char* what) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(f(context, a->h, b->h, &o), what);
        return wrap(o);
    }
    template <class F> Ctxt un2(F f, const Ctxt& a, int x, int y, const char* what) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(f(context, a->h, x, y, &o), what);
        return wrap(o);
    }
    template <class F> Ctxt many(F f, const vector<Ctxt>& v, const char* what) {
        auto hs = handles(v);
        fhelin_ct* o = nullptr;
        fhelin_shim::check(f(context, hs.data(), (int32_t)hs.size(), &o), what);
        return wrap(o);
    }
    Ctxt mask(const Ctxt& c, int kind, int x, int y, double v) {
        fhelin_ct* o = nullptr;
        fhelin_shim::check(fhelin_fc_mask(context, c->h, kind, x, y, v, &o), "mask");
        return wrap(o);
    }
    vector<Ctxt> mm_pt(const vector<Ctxt>& rows, const Ptxt& w, const Ptxt& bias, int slots, int padding) {
        auto hs = handles(rows);
        vector<fhelin_ct*> outs(rows.size());
        fhelin_shim::check(fhelin_fc_matmul_pt(context, hs.data(), (int32_t)hs.size(), w->h, bias ? bias->h : nullptr, slots, padding, outs.data()),
                           "matmul");
        return wrap_all(outs);
    }
    vector<Ctxt> mm_ct(const vector<Ctxt>& rows, const Ctxt& w, int slots, int padding) {
        auto hs = handles(rows);
        vector<fhelin_ct*> outs(rows.size());
        fhelin_shim::check(fhelin_fc_matmul_ct(context, hs.data(), (int32_t)hs.size(), w->h, slots, padding, outs.data()), "matmul");
        return wrap_all(outs);
    }
    static void need(const vector<double>& v, size_t n, const string& filename) {
        if (v.size() < n) {
            cerr << "\"" << filename << "\" holds " << v.size() << " values, " << n << " expected" << endl;
            exit(1);
        }
    }
    vector<double> expanded(const string& filename, double scale, int num_inputs) {
        vector<double> input = read_values_from_file(filename);
        need(input, 128, filename);
        vector<double> rep;
        for (int j = 0; j < 128; j++) {
            for (int i = 0; i < num_inputs; i++) rep.push_back(input[j] * scale);
            for (int i = 0; i < 128 - num_inputs; i++) rep.push_back(0);
        }
        return rep;
    }
    static void print_slot(double v, bool last, const char* zero) {
        string segno = v > 0 ? " " : "-";
        double a = std::fabs(v);
        if (last) cout << segno << a << " ]";
        else if (a < 0.00000001) cout << zero << ", ";
        else cout << segno << a << ", ";
    }
};

#endif /* FHELIN_FHECONTROLLER_SHIM_H */
