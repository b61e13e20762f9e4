// Sanitised replies through include/FHEController.h: a server without the secret key evaluates on the client's inputs and hands back
// the reply form of its result - the answer slots only, two limbs, re-randomised and flooded.  Run from a directory whose ../keys/ is
// the key folder:
//   shim_sanitize client   generate_context(true), rotation keys, save_evaluation_keys("evk.bin"), two encryptions to ../keys/in.bin
//   shim_sanitize server   load_evaluation_context("evk.bin") + load_rotation_keys; rotate, multiply, then
//                          sanitize(keep = {0..19}, flood_bits = 24): the raw result to ../keys/raw.bin, the reply to ../keys/reply.bin;
//                          prints "bytes raw <n> reply <n> limbs <ell> ring <N>"
//   shim_sanitize check    load_context() (the secret), decrypts reply.bin: prints "err <max abs error of the kept slots> other <largest
//                          magnitude of any other slot>"
#include <cmath>
#include <cstring>
#include "FHEController.h"

FHEController controller;

static const int KEEP = 20;

static vector<double> input(int k) {
    vector<double> x(1 << 14);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.5 * std::sin(0.37 * (double)i + 0.1 * (double)(i % 7) + k);
    return x;
}

static long long file_bytes(const char* path) {
    std::ifstream f(path, ios::binary | ios::ate);
    return (long long)f.tellg();
}

int main(int argc, char** argv) {
    const string mode = argc > 1 ? argv[1] : "";
    const vector<int> rotations = {1, -1, 2, 4, 8};
    if (mode == "client") {
        controller.generate_context(true);
        controller.generate_rotation_keys(rotations, true, "rk.txt");
        controller.save_evaluation_keys("evk.bin");
        // 5 and 7 limbs: the product has 5, and its rescale, the mask's product and rescale and the reply's two limbs need 4
        vector<Ctxt> in = {controller.encrypt(input(0), controller.circuit_depth - 4, 1 << 14),
                           controller.encrypt(input(1), controller.circuit_depth - 6, 1 << 14)};
        controller.save(in, "../keys/in.bin");
        cout << "client done" << endl;
        return 0;
    }
    if (mode == "server") {
        controller.load_evaluation_context("evk.bin");
        controller.load_rotation_keys("rk.txt", false);
        vector<Ctxt> v = controller.load_vector("../keys/in.bin");
        if (v.size() != 2) {
            cerr << "inputs not loaded" << endl;
            return 1;
        }
        Ctxt raw = controller.mult(controller.rotate(v[0], 1), v[1]);
        vector<int> keep;
        for (int i = 0; i < KEEP; i++) keep.push_back(i);
        Ctxt reply = controller.sanitize(raw, keep, 24);
        controller.save(raw, "../keys/raw.bin");
        controller.save(reply, "../keys/reply.bin");
        int32_t npoly, ell, level, deg, slots;
        double scale;
        fhelin_ct_info(reply->h, &npoly, &ell, &level, &deg, &scale, &slots);
        fhelin_params p;
        fhelin_ctx_info(controller.engine(), &p, nullptr, nullptr);
        cout << "bytes raw " << file_bytes("../keys/raw.bin") << " reply " << file_bytes("../keys/reply.bin") << " limbs " << ell << " ring "
             << (1 << p.log_n) << endl;
        return 0;
    }
    if (mode == "check") {
        controller.load_context(false);
        Ctxt c = controller.load_ciphertext("../keys/reply.bin");
        vector<double> x = input(0), y = input(1), got = controller.decrypt_tovector(c, 1 << 14);
        double kept = 0, other = 0;
        for (size_t i = 0; i < x.size(); i++) {
            if ((int)i < KEEP) kept = std::max(kept, std::fabs(got[i] - x[(i + 1) % x.size()] * y[i]));
            else other = std::max(other, std::fabs(got[i]));
        }
        cout << "err " << kept << " other " << other << endl;
        return 0;
    }
    cerr << "usage: shim_sanitize client|server|check" << endl;
    return 2;
}
