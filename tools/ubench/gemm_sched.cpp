// tools/ubench/gemm_sched.cpp -- A/B of the single-buffered K loop of gemm_pipe_kernel (gemm_pipe.hpp): SCHED = 0 (compiler-placed staging)
// against the hand-placed loop SCHED = 1..3, on the PRODUCT header (no instrumented copy) and the production tiles of the encoder products.
//   gemm_sched <reps>       per production shape: us per launch of every loop form, bit-compared with SCHED = 0
//   gemm_sched <reps> ml    main-loop TF (slope of the time over K) and fixed us (intercept) of every loop form on every production tile
// Build: make -C tools/ubench gemm_sched ; run on the GPU box.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../parakeet.cpp_amd/csrc/kernels/gemm.hip"
#include "../../parakeet.cpp_amd/csrc/kernels/gemm_smallm.hip"        // (launch_gemm links against the small-M kernels)
#include "../../parakeet.cpp_amd/csrc/kernels/gemm_smallm_bf16.hip"

using namespace pk;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

typedef void (*LaunchFn)(const GemmArgs &, hipStream_t);

// one production tile + epilogue, every loop form
struct Prod {
    const char *name;
    int N, K, Klo, Khi, epi;
    bool lna;
    LaunchFn run[4];
};
template <int WGM, int WGN, int TM, int TN, int EPI, bool LNA>
static Prod prod(const char *name, int N, int K, int Klo, int Khi) {
    return {name, N, K, Klo, Khi, EPI, LNA,
            {launch_gemm_pipe<WGM, WGN, TM, TN, 32, EPI, 1, LNA, 0>, launch_gemm_pipe<WGM, WGN, TM, TN, 32, EPI, 1, LNA, 1>,
             launch_gemm_pipe<WGM, WGN, TM, TN, 32, EPI, 1, LNA, 2>, launch_gemm_pipe<WGM, WGN, TM, TN, 32, EPI, 1, LNA, 3>}};
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 20;
    const bool ml = argc > 2 && strcmp(argv[2], "ml") == 0;
    CK(hipSetDevice(0));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    // the encoder products of tdt-ctc-110m at 64 x 10 s (M = 8064); fc2 / sub_proj take the long-K 128x128 tile of 64 x 32 waves
    const std::vector<Prod> prods = {
        prod<4, 2, 1, 2, EPI_SILU, true>("fc1+silu (LN folded) 8064x2048x512", 2048, 512, 512, 2048),
        prod<4, 2, 1, 2, EPI_SILU, false>("fc1+silu 8064x2048x512", 2048, 512, 512, 2048),
        prod<2, 4, 2, 1, EPI_RESID, false>("fc2+resid 8064x512x2048", 512, 2048, 1024, 4096),
        prod<4, 2, 1, 2, EPI_NONE, true>("qkv (LN folded) 8064x1536x512", 1536, 512, 512, 2048),
        prod<4, 2, 1, 2, EPI_NONE, false>("qkv 8064x1536x512", 1536, 512, 512, 2048),
        prod<4, 2, 1, 2, EPI_GLU, true>("pw1+glu (LN folded) 8064x512(x2)x512", 512, 512, 512, 2048),
        prod<4, 2, 1, 2, EPI_GLU, false>("pw1+glu 8064x512(x2)x512", 512, 512, 512, 2048),
        prod<4, 2, 1, 2, EPI_RESID, false>("out_proj/pw2+resid 8064x512x512", 512, 512, 512, 2048),
    };
    const int M = 8064, maxN = 2 * 2048, maxK = 4096;
    std::vector<float> h((size_t)M * maxK);
    unsigned st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) * (1.0f / 16777216.0f)) * 2.0f - 1.0f; };
    float *dA, *dW, *dB, *dO, *dR, *dS, *dG, *dBe;
    CK(hipMalloc(&dA, (size_t)M * maxK * 4));
    CK(hipMalloc(&dW, (size_t)maxN * maxK * 4));
    CK(hipMalloc(&dB, (size_t)maxN * 4));
    CK(hipMalloc(&dO, (size_t)M * maxN * 4));
    CK(hipMalloc(&dR, (size_t)M * maxN * 4));
    CK(hipMalloc(&dS, (size_t)M * 2 * 4));
    CK(hipMalloc(&dG, (size_t)maxK * 4));
    CK(hipMalloc(&dBe, (size_t)maxK * 4));
    for (auto &v : h) v = rnd();
    CK(hipMemcpy(dA, h.data(), (size_t)M * maxK * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dR, h.data(), (size_t)M * maxN * 4, hipMemcpyHostToDevice));
    for (size_t i = 0; i < (size_t)maxN * maxK; i += h.size()) {
        for (auto &v : h) v = 0.05f * rnd();
        CK(hipMemcpy(dW + i, h.data(), std::min(h.size(), (size_t)maxN * maxK - i) * 4, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < maxN; ++i) h[i] = rnd();
    CK(hipMemcpy(dB, h.data(), (size_t)maxN * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < maxK; ++i) h[i] = 1.0f + 0.1f * rnd();
    CK(hipMemcpy(dG, h.data(), (size_t)maxK * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dBe, h.data() + maxK, (size_t)maxK * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < M; ++i) { h[2 * i] = 0.01f * rnd(); h[2 * i + 1] = 1.5f + 0.2f * rnd(); }
    CK(hipMemcpy(dS, h.data(), (size_t)M * 2 * 4, hipMemcpyHostToDevice));

    auto args = [&](const Prod &p, int K) {
        GemmArgs g{dA, K, dW, K, dB, dO, p.N, dR, p.N, 0.5f, M, p.N, K};
        if (p.lna) { g.ln_stats = dS; g.ln_g = dG; g.ln_b = dBe; }
        return g;
    };
    auto time_us = [&](LaunchFn f, const GemmArgs &g) {
        for (int i = 0; i < 2; ++i) f(g, s);
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) f(g, s);
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        return ms / reps * 1e3;
    };
    std::vector<unsigned> ref, out;
    for (const Prod &p : prods) {
        printf("== %s\n", p.name);
        const double flop_k = 2.0 * M * p.N * (p.epi == EPI_GLU ? 2 : 1);   // per unit of K
        const size_t no = (size_t)M * p.N;
        for (int v = 0; v < 4; ++v) {
            GemmArgs g = args(p, p.K);
            CK(hipMemsetAsync(dO, 0xff, no * 4, s));
            p.run[v](g, s);
            CK(hipStreamSynchronize(s));
            CK(hipGetLastError());
            out.resize(no);
            CK(hipMemcpy(out.data(), dO, no * 4, hipMemcpyDeviceToHost));
            if (v == 0) ref = out;
            size_t bad = 0;
            for (size_t i = 0; i < no; ++i) bad += out[i] != ref[i];
            if (ml) {
                const double tlo = time_us(p.run[v], args(p, p.Klo)), thi = time_us(p.run[v], args(p, p.Khi));
                const double slope = (thi - tlo) / (p.Khi - p.Klo);                       // us per unit of K
                printf("   SCHED=%d  K=%d %7.1f us  K=%d %7.1f us  | main loop %6.1f TF, fixed %6.1f us  %s\n", v, p.Klo, tlo, p.Khi, thi,
                       flop_k / slope * 1e-6, tlo - slope * p.Klo, bad ? "MISMATCH" : "bit-equal");
            } else {
                const double t = time_us(p.run[v], g);
                printf("   SCHED=%d  %7.1f us  %6.1f TF  %s\n", v, t, flop_k * p.K / t * 1e-6, bad ? "MISMATCH" : "bit-equal");
            }
            if (bad) printf("      (%zu of %zu elements differ)\n", bad, no);
        }
        fflush(stdout);
    }
    return 0;
}
