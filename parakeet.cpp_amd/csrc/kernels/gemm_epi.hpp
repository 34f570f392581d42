// parakeet.cpp_amd/csrc/kernels/gemm_epi.hpp -- what every GEMM family of this directory does to a finished accumulator, written once:
// the epilogue function of one value, the remap / sigma-column store, the scalar epilogue of the 32x32 MFMA tiles, and the streaming conv
// module's depthwise-conv tail (kernels.hpp: DwTail).  No state; everything inlines into the kernel that calls it.
#ifndef PK_GEMM_EPI_HPP
#define PK_GEMM_EPI_HPP
#include "../pk_devmath.h"
#include "kernels.hpp"

namespace pk {

// One output value: bias (only where the product has one), then the epilogue function.  EPI_RESID is resid + v * alpha with the product rounded
// on its own (unfused); EPI_GLU adds the gate's bias before the sigmoid.  `fast` (GemmArgs::fast_act, bf16 mode) selects the hardware exp / rcp
// activations; the fp32-contract kernels pass a literal false and the branch folds away.
template <int EPI>
__device__ __forceinline__ float epi_finish(float v, bool has_bias, float bias, float gate, float bias_g, float resid, float alpha, bool fast) {
    if (has_bias) v = v + bias;
    if constexpr (EPI == EPI_RELU) {
        v = v > 0.0f ? v : 0.0f;
    } else if constexpr (EPI == EPI_SILU) {
        v = fast ? fast_siluf(v) : dsiluf(v);
    } else if constexpr (EPI == EPI_RESID) {
        const float y = v * alpha;
        v = resid + y;
    } else if constexpr (EPI == EPI_GLU) {
        if (has_bias) gate = gate + bias_g;
        v = v * (fast ? fast_sigmoidf(gate) : dsigmoidf(gate));
    }
    return v;
}

// The scalar store of out[row][col]: through the output re-mapping, or row-major with the columns below sigma_cols in the sigma layout.
__device__ __forceinline__ void gemm_store(const GemmArgs &g, int row, int col, float v) {
    if (g.remap_rows) g.out[(int64_t)(row / g.remap_rows) * g.remap_gs + (int64_t)(row % g.remap_rows) * g.remap_rs + (int64_t)col * g.remap_cs] = v;
    else g.out[(int64_t)row * g.ldo + (col < g.sigma_cols ? sigma_col(col) : col)] = v;
}

// Scalar epilogue of wave (wm, wn) holding TM x TN accumulators of the 32x32 MFMA (GLU: tiles [0, TN/2) the values, [TN/2, TN) the gates of the
// same columns).  C/D layout: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
template <int TM, int TN, int WN, int EPI>
__device__ __forceinline__ void epilogue_scalar_32x32(const GemmArgs &g, float __attribute__((ext_vector_type(16))) (&acc)[TM][TN], int m0, int n0,
                                                      int wm, int wn, int lane, bool fast) {
    constexpr int WM = TM * 32, TNO = (EPI == EPI_GLU) ? TN / 2 : TN;
    const int lc = lane & 31, lr = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < TNO; ++j) {
        const int col = n0 + wn * (EPI == EPI_GLU ? WN / 2 : WN) + j * 32 + lc;
        if (col >= g.N) continue;
        const float bias = g.bias ? g.bias[col] : 0.0f;
        float bias_g = 0.0f;
        if constexpr (EPI == EPI_GLU) bias_g = g.bias ? g.bias[g.N + col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + lr;
                if (row >= g.M) continue;
                float gate = 0.0f, resid = 0.0f;
                if constexpr (EPI == EPI_GLU) gate = acc[i][j + TN / 2][r];
                if constexpr (EPI == EPI_RESID) resid = g.resid[(int64_t)row * g.ldr + col];
                gemm_store(g, row, col, epi_finish<EPI>(acc[i][j][r], g.bias != nullptr, bias, gate, bias_g, resid, g.alpha, fast));
            }
        }
    }
}

// The conv tail of a GLU tile of the 16x16 MFMA (kernels.hpp: DwTail): the lane that finishes rows m0 + 4 kq .. + 3 of channel `col` -- 4 / c
// streams of c new frames -- holds the streams' 8 cached rows, the 9 taps and the channel's bias / BatchNorm parameters.  load() requests them
// (in front of the weight stream); finish() runs the conv over [cache ; new rows] with dwconv_point -- what stream_dwconv_kernel calls --,
// stores the activations and the streams' next cache.  The caller guards both with the same predicate.  (gemm_smallm_ln_kernel keeps the same
// lines written out: through this struct its K = 1024 instantiation spilled 8 VGPRs instead of 4.)
struct DwTailRegs {
    float dpre[4][8], dwk[9], dbs, dmu, drs, dbg, dbb;

    __device__ __forceinline__ void load(const DwTail &dw, const GemmArgs &g, int m0, int kq, int col) {
        const int nstr = 4 / dw.c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int rw = m0 + 4 * kq + j * dw.c;
            const bool on = j < nstr && rw < g.M && dw.has_cache;
            const int64_t sidx = on ? rw / dw.c : 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) dpre[j][q] = on ? dw.cache_in[(sidx * 8 + q) * g.N + col] : 0.0f;   // (first chunk: zero left padding)
        }
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) dwk[kk] = dw.w[kk * g.N + col];
        dbs = dw.bias[col]; dmu = dw.bn_mean[col]; drs = dw.bn_rstd[col]; dbg = dw.bn_g[col]; dbb = dw.bn_b[col];
    }

    template <int C>
    __device__ __forceinline__ void finish_c(const DwTail &dw, const GemmArgs &g, int m0, int kq, int col, const float (&glu)[4]) const {
        const int ocol = dw.out_sigma ? sigma_col(col) : col;
#pragma unroll
        for (int j = 0; j < 4 / C; ++j) {
            const int rw = m0 + 4 * kq + j * C;
            if (rw >= g.M) continue;
            const int64_t sidx = rw / C;
            float cat[8 + C];
#pragma unroll
            for (int q = 0; q < 8; ++q) cat[q] = dpre[j][q];
#pragma unroll
            for (int f = 0; f < C; ++f) cat[8 + f] = glu[j * C + f];
#pragma unroll
            for (int f = 0; f < C; ++f) g.out[(int64_t)(rw + f) * g.ldo + ocol] = dwconv_point<9>(dwk, cat + f, dbs, dmu, drs, dbg, dbb);
#pragma unroll
            for (int q = 0; q < 8; ++q) dw.cache_out[(sidx * 8 + q) * g.N + col] = cat[q + C];   // the last 8 rows of the concatenation
        }
    }
    __device__ __forceinline__ void finish(const DwTail &dw, const GemmArgs &g, int m0, int kq, int col, const float (&glu)[4]) const {
        if (dw.c == 1) finish_c<1>(dw, g, m0, kq, col, glu);
        else if (dw.c == 2) finish_c<2>(dw, g, m0, kq, col, glu);
        else finish_c<4>(dw, g, m0, kq, col, glu);
    }
};

}  // namespace pk
#endif  // PK_GEMM_EPI_HPP
