// Seeded evaluation keys through include/FHEController.h: the client makes its keys in seeded-key mode and writes the compact
// evaluation-key set (b halves and the key-set seed); a separate server process that has no secret-key.txt loads it, and the
// client decrypts.  Run from a directory whose ../keys/ is the key folder:
//   shim_seeded_keys client   set_seeded_keys(true), generate_context(true), bootstrapping + rotation keys,
//                             save_evaluation_keys("evk.cmp", true) and save_evaluation_keys("evk.bin") (the full set, for its
//                             size), one encrypted input to ../keys/in.bin, the client's own bootstrap + rotate + mult of it to
//                             ../keys/own.bin
//   shim_seeded_keys server   load_evaluation_context("evk.cmp") + load_bootstrapping_and_rotation_keys, the same steps on in.bin,
//                             result to ../keys/out.bin; prints "decrypt refused" when decrypt throws there
//   shim_seeded_keys check    set_seeded_keys(true), load_context() (the secret), decrypts out.bin: prints "err <max abs error>"
// tests/test_shim_seeded_keys_gpu.py compares out.bin and own.bin byte for byte.
#include <cmath>
#include <cstring>
#include "FHEController.h"

FHEController controller;

static vector<double> input() {
    vector<double> x(1 << 14);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.5 * std::sin(0.23 * (double)i + 0.1 * (double)(i % 5));
    return x;
}

static Ctxt steps(const Ctxt& c) {
    Ctxt b = controller.bootstrap(c);
    Ctxt r = controller.rotate(b, 1);
    return controller.mult(b, r);
}

int main(int argc, char** argv) {
    const string mode = argc > 1 ? argv[1] : "";
    const vector<int> rotations = {1, -1, 2, 4, 8};
    if (mode == "client") {
        controller.set_seeded_keys(true);
        controller.generate_context(true);
        controller.generate_bootstrapping_and_rotation_keys(rotations, 1 << 14, true, "rk.txt");
        controller.save_evaluation_keys("evk.cmp", true);
        controller.save_evaluation_keys("evk.bin");
        Ctxt c = controller.encrypt(input(), controller.circuit_depth - 2, 1 << 14);
        controller.save(c, "../keys/in.bin");
        controller.save(steps(c), "../keys/own.bin");
        cout << "client done" << endl;
        return 0;
    }
    if (mode == "server") {
        controller.load_evaluation_context("evk.cmp");
        controller.load_bootstrapping_and_rotation_keys("rk.txt", 1 << 14, true);
        Ctxt c = controller.load_ciphertext("../keys/in.bin");
        Ctxt out = steps(c);
        controller.save(out, "../keys/out.bin");
        try {
            controller.decrypt_tovector(out, 16);
            cout << "decrypt succeeded" << endl;
        } catch (const std::exception& e) {
            cout << "decrypt refused: " << e.what() << endl;
        }
        return 0;
    }
    if (mode == "check") {
        controller.set_seeded_keys(true);
        controller.load_context(false);
        Ctxt c = controller.load_ciphertext("../keys/out.bin");
        vector<double> x = input(), got = controller.decrypt_tovector(c, 1 << 14);
        double m = 0;
        for (size_t i = 0; i < x.size(); i++) m = std::max(m, std::fabs(got[i] - x[i] * x[(i + 1) % x.size()]));
        cout << "err " << m << endl;
        return 0;
    }
    cerr << "usage: shim_seeded_keys client|server|check" << endl;
    return 2;
}
