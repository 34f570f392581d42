// tools/asan_tdt_total_host.cpp -- stand-alone sanitizer exercise of the HOST code of the TDT total / rescoring entry points: the planning and the
// refusals of pk_tdt_total, the grouping of hypotheses (pk_diag_tdt_total_groups) and the ordering rule (pk_diag_rescore_order).  No device is
// needed: every call here returns before one is looked for.  Build and run against the sanitizer build of the library (make -C csrc asan):
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -I include tools/asan_tdt_total_host.cpp \
//       -L parakeet.cpp_amd -lparakeet_amd_asan -Wl,-rpath,$PWD/parakeet.cpp_amd -o asan_tdt_total_host && ASAN_OPTIONS=detect_leaks=0 ./asan_tdt_total_host
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "parakeet_amd.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    std::mt19937 rng(7);
    const int32_t dur[5] = {0, 1, 2, 3, 4};
    // grouping: random shapes, every cap of the group width; groups are consecutive and cover every hypothesis
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rng() % 700), max_hyps = (int)(rng() % 5) == 0 ? 0 : 1 + (int)(rng() % 300);
        std::vector<int32_t> T(n), off(n + 1, 0), g(n, -1);
        for (int i = 0; i < n; ++i) { T[i] = 1 + (int32_t)(rng() % 4000); off[i + 1] = off[i] + (int32_t)(rng() % 1536); }
        int ng = 0;
        CHECK(pk_diag_tdt_total_groups(T.data(), off.data(), n, dur, 5, 1025, 640, max_hyps, g.data(), &ng) == PK_OK);
        CHECK(g[0] == 0 && g[n - 1] == ng - 1);
        int width = 0;
        for (int i = 1; i < n; ++i) { CHECK(g[i] == g[i - 1] || g[i] == g[i - 1] + 1); }
        for (int i = 0, run = 0; i < n; ++i) { run = (i && g[i] == g[i - 1]) ? run + 1 : 1; width = run > width ? run : width; }
        CHECK(width <= (max_hyps > 0 ? max_hyps : 256));
    }
    {   // refusals: past the token limit, past the scratch cap alone, a duration of 9, D = 9, decreasing offsets
        int32_t T1[1] = {10}, g1[1], offb[2] = {0, 1536}, offc[2] = {0, 1500}, Tc[1] = {30000}, offd[2] = {0, -1}, d9[2] = {0, 9}, dd[9] = {};
        CHECK(pk_diag_tdt_total_groups(T1, offb, 1, dur, 5, 1025, 640, 0, g1, nullptr) == PK_ERR_UNSUPPORTED);
        CHECK(pk_diag_tdt_total_groups(Tc, offc, 1, dur, 5, 1025, 640, 0, g1, nullptr) == PK_ERR_UNSUPPORTED);
        CHECK(pk_diag_tdt_total_groups(T1, offc, 1, d9, 2, 1025, 640, 0, g1, nullptr) == PK_ERR_UNSUPPORTED);
        CHECK(pk_diag_tdt_total_groups(T1, offc, 1, dd, 9, 1025, 640, 0, g1, nullptr) == PK_ERR_UNSUPPORTED);
        CHECK(pk_diag_tdt_total_groups(T1, offd, 1, dur, 5, 1025, 640, 0, g1, nullptr) == PK_ERR_INVALID);
        float z[8] = {}, tot[1];
        int32_t ok[1], T3[1] = {3}, o1[2] = {0, 1}, T6[1] = {60000};
        CHECK(pk_tdt_total(z, z, z, d9, 2, T3, 1, o1, tot, ok) == PK_ERR_UNSUPPORTED);
        CHECK(pk_tdt_total(z, z, z, dd, 9, T3, 1, o1, tot, ok) == PK_ERR_UNSUPPORTED);
        CHECK(pk_tdt_total(z, z, z, dur, 2, T3, 1, offb, tot, ok) == PK_ERR_UNSUPPORTED);
        CHECK(pk_tdt_total(z, z, z, dur, 2, T6, 1, offc, tot, ok) == PK_ERR_UNSUPPORTED);
        CHECK(pk_tdt_total(z, z, z, dur, 2, T3, 0, o1, tot, ok) == PK_ERR_INVALID);
        CHECK(pk_tdt_total(z, z, z, dur, 2, T3, 1, offd, tot, ok) == PK_ERR_INVALID);
    }
    // the ordering rule: a permutation; scored slots first and descending, ties in beam order; unscored filled slots next; unfilled last
    for (int round = 0; round < 2000; ++round) {
        const int N = 1 + (int)(rng() % 32), filled = (int)(rng() % (N + 1)), bad = filled ? (int)(rng() % (filled + 1)) : 0;
        const float w = (float)(rng() % 5) / 4.0f, inf = INFINITY;
        std::vector<int32_t> lens(N, 0), ok(N, 0), order(N);
        std::vector<float> ctc(N, -inf), tdt(N, -inf), comb(N);
        for (int j = 0; j < filled; ++j) { lens[j] = (int32_t)(rng() % 9); ctc[j] = -(float)(rng() % 7); }
        for (int j = 0; j < filled - bad; ++j) { ok[j] = 1; tdt[j] = -(float)(rng() % 7); }
        CHECK(pk_diag_rescore_order(lens.data(), ctc.data(), tdt.data(), ok.data(), N, w, order.data(), comb.data()) == PK_OK);
        std::vector<int> seen(N, 0);
        for (int p = 0; p < N; ++p) { CHECK(order[p] >= 0 && order[p] < N && !seen[order[p]]); seen[order[p]] = 1; }
        const int good = filled - bad;
        for (int p = 0; p < N; ++p) {
            if (p < good) CHECK(order[p] < good);
            else CHECK(order[p] == p);
            if (p + 1 < good) CHECK(comb[order[p]] > comb[order[p + 1]] || (comb[order[p]] == comb[order[p + 1]] && order[p] < order[p + 1]));
        }
    }
    CHECK(pk_diag_rescore_order(nullptr, nullptr, nullptr, nullptr, 1, 0.5f, nullptr, nullptr) == PK_ERR_INVALID);
    std::puts("asan_tdt_total_host: ok");
    return 0;
}
