// Compact inputs through include/FHEController.h: the client encrypts with seeded (secret-key) encryption and writes its inputs with
// save_compact; a separate server process that has no secret-key.txt reads them with load_ciphertext / load_vector, evaluates with
// the client's evaluation-key set, and the client decrypts.  Run from a directory whose ../keys/ is the key folder:
//   shim_compact client   generate_context(true), rotation keys, save_evaluation_keys("evk.bin"), two seeded encryptions saved to
//                         ../keys/in.cc (save_compact) and ../keys/in_full.bin (save), the client's own rotate + mult of them to
//                         ../keys/own.bin; prints the two files' sizes
//   shim_compact server   load_evaluation_context("evk.bin") + load_rotation_keys, the same steps on in.cc, result to ../keys/out.bin
//   shim_compact check    load_context() (the secret), decrypts out.bin: prints "err <max abs error>"
// tests/test_shim_compact_gpu.py compares out.bin and own.bin byte for byte.
#include <cmath>
#include <cstring>
#include "FHEController.h"

FHEController controller;

static vector<double> input(int k) {
    vector<double> x(1 << 14);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.5 * std::sin(0.37 * (double)i + 0.1 * (double)(i % 7) + k);
    return x;
}

static Ctxt steps(const Ctxt& a, const Ctxt& b) { return controller.mult(controller.rotate(a, 1), b); }

int main(int argc, char** argv) {
    const string mode = argc > 1 ? argv[1] : "";
    const vector<int> rotations = {1, -1, 2, 4, 8};
    if (mode == "client") {
        controller.generate_context(true);
        controller.generate_rotation_keys(rotations, true, "rk.txt");
        controller.save_evaluation_keys("evk.bin");
        controller.set_seeded_encryption(true);
        vector<Ctxt> in = {controller.encrypt(input(0), controller.circuit_depth - 2, 1 << 14),
                           controller.encrypt(input(1), controller.circuit_depth - 4, 1 << 14)};
        controller.save_compact(in, "../keys/in.cc");
        controller.save(in, "../keys/in_full.bin");
        controller.save(steps(in[0], in[1]), "../keys/own.bin");
        std::ifstream a("../keys/in.cc", ios::binary | ios::ate), b("../keys/in_full.bin", ios::binary | ios::ate);
        cout << "bytes compact " << (long long)a.tellg() << " full " << (long long)b.tellg() << endl;
        return 0;
    }
    if (mode == "server") {
        controller.load_evaluation_context("evk.bin");
        controller.load_rotation_keys("rk.txt", false);
        Ctxt a = controller.load_ciphertext("../keys/in.cc");
        vector<Ctxt> v = controller.load_vector("../keys/in.cc");
        if (!a || v.size() != 2) {
            cerr << "compact inputs not loaded" << endl;
            return 1;
        }
        controller.save(steps(a, v[1]), "../keys/out.bin");
        cout << "server done" << endl;
        return 0;
    }
    if (mode == "check") {
        controller.load_context(false);
        Ctxt c = controller.load_ciphertext("../keys/out.bin");
        vector<double> x = input(0), y = input(1), got = controller.decrypt_tovector(c, 1 << 14);
        double m = 0;
        for (size_t i = 0; i < x.size(); i++) m = std::max(m, std::fabs(got[i] - x[(i + 1) % x.size()] * y[i]));
        cout << "err " << m << endl;
        return 0;
    }
    cerr << "usage: shim_compact client|server|check" << endl;
    return 2;
}
