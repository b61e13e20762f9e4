// The reference's two bootstrap overloads through include/FHEController.h: bootstrap(c) and bootstrap(c, precision), the
// iterative EvalBootstrap(c, 2, precision) (reference src/FHEController.cpp:438-469), on one encrypted vector at N=2^15 with
// 16384 slots.  Prints one line "single_err <e> iter_err <e> single_level <l> iter_level <l>" for
// tests/test_shim_bootstrap_iter_gpu.py.
#include <cmath>
#include "FHEController.h"

FHEController controller;

static double max_err(const vector<double>& got, const vector<double>& want) {
    double m = 0;
    for (size_t i = 0; i < want.size(); i++) m = std::max(m, std::fabs(got[i] - want[i]));
    return m;
}

int main(int argc, char** argv) {
    const int precision = argc > 1 ? std::atoi(argv[1]) : 12;
    controller.generate_context(15, 55, 52, 4, 3, 3, 59);
    controller.generate_bootstrapping_keys(1 << 14);
    vector<double> x(1 << 14);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.9 * std::sin(0.37 * (double)i + 0.1 * (double)(i % 7));
    Ctxt c = controller.encrypt(x, controller.circuit_depth - 2, 1 << 14);
    Ctxt once = controller.bootstrap(c);
    Ctxt twice = controller.bootstrap(c, precision, true);
    const double e1 = max_err(controller.decrypt_tovector(once, 1 << 14), x);
    const double e2 = max_err(controller.decrypt_tovector(twice, 1 << 14), x);
    cout << setprecision(6) << "single_err " << e1 << " iter_err " << e2 << " single_level " << once->GetLevel() << " iter_level "
         << twice->GetLevel() << endl;
    return 0;
}
