// Host-only check of the bootstrap's linear-stage splits (Bootstrapper::prepare): for n = 2^10 and 2^11 slots, level
// budgets {3, 3}, every CoeffsToSlots / SlotsToCoeffs stage (the packed ones over 2n slots included) is prepared with the default split
// and with the linear-transform engine's split at n1 = 0 (planner), 4, 16 and 32, and the terms of each must reassemble - diag_{g+b} =
// rot(V_{g,b}, +g) - to the same diagonal map, value for value.  Also checked: at most 32 baby steps, baby[b] = b * g0, ascending giant
// steps, pts [n2][n1] holding exactly the terms.  Prints the split per stage and the rotation-key lists; exit status 0 = all equal.
// No device is touched (a host-only context).  Build, from the repository root, after the library:
//   g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/boot_lt_split_check.cpp -Lfhe-linformer_amd -lfhelin_amd \
//       -Wl,-rpath,$PWD/fhe-linformer_amd -o /tmp/boot_lt_split_check
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <numeric>
#include <set>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#define private public   // Bootstrapper::prepare and the knob's fields; the standard headers above are already in
#include "../fhe-linformer_amd/csrc/bootstrap.cpp"
#undef private

using namespace fhelin;

static DiagMap reassemble(const LinStage& st, int n) {
    DiagMap m;
    for (const auto& t : st.terms) {
        std::vector<cplx> d(n);
        for (int i = 0; i < n; ++i) {
            const int j = (i + t.giant) % n;
            d[i] = cplx(t.diag->values[j], t.diag->imag[j]);
        }
        if (!m.emplace((t.giant + t.baby) % n, d).second) {
            std::printf("FAIL: two terms at index %d\n", (t.giant + t.baby) % n);
            std::exit(1);
        }
    }
    return m;
}

int main() {
    int bad = 0;
    for (int logn : {10, 11}) {
        Params p;
        p.log_n = 12;
        p.n_q = 22;
        p.n_p = 6;
        p.dnum = 4;
        p.log_slots = logn;
        p.hamming = 64;
        p.seed = 1;
        p.device = -1;
        Context ctx(p);
        Evaluator ev(ctx);
        Client cl(ev, ctx.prm.seed_bytes);
        const int n = 1 << logn, budget = 3;
        std::vector<u32> rot;
        std::vector<std::pair<double, double>> ksi;
        ckks_fft_tables(n, rot, ksi);
        const bool packed = (ctx.N / 2) / n >= 2;
        // the stage maps as Bootstrapper::setup composes them (radix levels per stage: the remainder goes to the later stages)
        std::vector<std::pair<DiagMap, int>> maps;
        for (int inverse = 1; inverse >= 0; --inverse) {
            std::vector<int> lens;
            if (inverse) for (int len = n; len >= 2; len >>= 1) lens.push_back(len);
            else for (int len = 2; len <= n; len <<= 1) lens.push_back(len);
            size_t pos = 0;
            for (int g = 0; g < budget; ++g) {
                const int cnt = logn / budget + (budget - 1 - g < logn % budget ? 1 : 0);
                DiagMap m = stage_map(n, lens[pos], inverse, rot, ksi);
                for (int i = 1; i < cnt; ++i) m = compose(stage_map(n, lens[pos + i], inverse, rot, ksi), m, n);
                pos += cnt;
                if (packed && inverse && g == budget - 1) maps.push_back({pack_last_c2s(m, n), 2 * n});
                else if (packed && !inverse && g == 0) maps.push_back({unpack_first_s2c(m, n), 2 * n});
                else maps.push_back({m, n});
            }
        }
        Bootstrapper off(ev, cl);
        std::set<int> keys_off;
        std::vector<DiagMap> want;
        for (auto& e : maps) {
            const LinStage st = off.prepare(e.first, e.second);
            want.push_back(reassemble(st, e.second));
            for (const auto& t : st.terms) keys_off.insert({t.giant, t.baby});
        }
        keys_off.erase(0);
        for (int n1 : {0, 4, 16, 32}) {
            Bootstrapper on(ev, cl);
            on.set_lt(true, n1);
            std::set<int> keys;
            std::printf("slots 2^%d n1=%d:", logn, n1);
            for (size_t s = 0; s < maps.size(); ++s) {
                const int ns = maps[s].second;
                const LinStage st = on.prepare(maps[s].first, ns);
                const int n2 = (int)st.lt_giant.size();
                std::printf("  %s%zu n1=%d n2=%d terms=%zu", s < 3 ? "c2s" : "s2c", s % 3, st.bsz, n2, st.terms.size());
                bool ok = st.bsz >= 1 && st.bsz <= LtDot::MAX_STEPS && (int)st.lt_baby.size() == st.bsz && (int)st.lt_pts.size() == n2;
                for (int b = 0; ok && b < st.bsz; ++b) ok = st.lt_baby[b] == b * st.g0;
                for (int g = 1; ok && g < n2; ++g) ok = st.lt_giant[g] > st.lt_giant[g - 1];
                size_t held = 0;
                for (const auto& row : st.lt_pts)
                    for (const PtPtr& q : row) held += q ? 1 : 0;
                ok = ok && held == st.terms.size();
                for (const auto& t : st.terms) {
                    ok = ok && t.baby % st.g0 == 0 && t.baby / st.g0 < st.bsz && t.giant % st.g0 == 0 && t.giant + t.baby < ns;
                    const auto it = std::find(st.lt_giant.begin(), st.lt_giant.end(), t.giant);
                    ok = ok && it != st.lt_giant.end() && st.lt_pts[it - st.lt_giant.begin()][t.baby / st.g0] == t.diag;
                    keys.insert({t.giant, t.baby});
                }
                const DiagMap got = reassemble(st, ns);
                ok = ok && got.size() == want[s].size();
                for (const auto& e : want[s]) {
                    const auto it = got.find(e.first);
                    ok = ok && it != got.end() && it->second == e.second;
                }
                if (!ok) {
                    std::printf(" FAIL");
                    ++bad;
                }
            }
            keys.erase(0);
            std::vector<int> missing;
            std::set_difference(keys_off.begin(), keys_off.end(), keys.begin(), keys.end(), std::back_inserter(missing));
            std::printf("\n  rotation keys: %zu (default split: %zu, of which %zu are not in this list)\n", keys.size(), keys_off.size(),
                        missing.size());
        }
    }
    std::printf(bad ? "FAILED: %d stage(s)\n" : "all stages reassemble to the default split's diagonal map%.0d\n", bad);
    return bad ? 1 : 0;
}
