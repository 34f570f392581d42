// parakeet.cpp_amd/csrc/kernels/gemm_smallm.hip -- the fp32 MFMA GEMM for a HANDFUL of rows (M <= kSmallMRows): the streaming
// encoder's products (16 streams x 1-3 frames per chunk against the full 600M-parameter weight set) and the single-clip path.
//
// out[M][N] = epi(A[M][K] * W[N][K]^T + bias), natural-k fma chains (bit-identical to the oracle and to the big-tile kernels).
// With so few rows the problem is a latency-bound weight stream, not a tile problem: ONE dependent chain of K / 4
// v_mfma_f32_16x16x4_f32 (8 passes = 32 clocks each) per 16x16 output tile is the floor -- 13.7 us for fc2 of the 600M model
// (K = 4096) at 2.4 GHz -- so everything else has to stay off that chain:
//  * one WAVEFRONT per 16x16 output tile, no LDS and no barrier in the K loop.  The first generation of this kernel parked every
//    64-k chunk k-planar in LDS (ds_write x 32, fence, ds_read_b128 x 8) in front of its 16 MFMAs; with a single wave per
//    workgroup that round trip sits ON the chain: 1390 clocks per chunk against the 512 of the MFMAs
//    (profiles/r03_rocprofv3_stream_kernel_stats.md: fc2 37 us).
//  * operands straight from L2 / HBM with 16-byte loads in the NATURAL layouts: lane (row r = lane & 15, quarter q = lane >> 4) loads
//    A[r][16 f + 4 q .. + 3] and W[n0 + r][16 f + 4 q .. + 3] -- 64-byte row segments per 16 lanes.  The MFMA wants lane (r, q) to
//    supply k = 4 s + q for step s, i.e. element e of the four consecutive steps 4 f + e is natural k = 16 f + 4 e + q: the 4 x 4
//    transpose of what the four lanes (r, 0..3) hold in their four registers.  gfx950 has the instruction for exactly that:
//    v_permlane16_swap / v_permlane32_swap exchange the odd 16-lane rows of one register with the even rows of another -- two
//    swaps per register pair, four per float4, eight per 16-k block, issued beside the block's four MFMAs (128 clocks).
//    (Semantics pinned on the hardware by tools/ubench/permlane_probe.cpp.)
//  * a register ring of DEPTH = 8 chunks of 64 k (8 loads per chunk and lane; 2 when K / 64 is even but no multiple of 8 -- K = 256 runs
//    depth 2 --, 1 when it is odd; gemm_smallm_form): 7 x 512 chain clocks of cover for the weight stream, 56 loads in flight -- below vmcnt's 6-bit limit.
//  * one wave per workgroup -- with a few hundred waves on 1024 SIMDs every chain gets a SIMD and an L1 of its own (four row-tile waves in
//    one workgroup, sharing the W lines through one L1, lost: the L1 is at its 64 B/clk with four chains); GLU: the value and the gate
//    tile of the same 16 columns are the two waves of a workgroup (two chains side by side instead of one of double length), the gate sums
//    cross through LDS once at the end.
//  * SIG (GemmArgs::a_sigma + W_sig): both operands already in MFMA order -- no transposes at all; the weights TILED so that a load
//    instruction reads 1 KB of consecutive addresses (the streaming encoder, csrc/stream.cpp; Model::sigma_weights).
#include "../pk_devmath.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "kernels.hpp"
#include "gemm_epi.hpp"

namespace pk {

typedef float sm_f32x4 __attribute__((ext_vector_type(4)));

// 4 x 4 transpose between the four 16-lane rows of a wave and the four components of v: afterwards component e of row q holds what
// was component q of row e.  permlane16_swap(a, b): rows 1, 3 of a <-> rows 0, 2 of b; permlane32_swap(a, b): rows 2, 3 of a <-> rows 0, 1 of b.
__device__ __forceinline__ void sm_tr4x4(float4 &v) {
    unsigned c0 = __builtin_bit_cast(unsigned, v.x), c1 = __builtin_bit_cast(unsigned, v.y);
    unsigned c2 = __builtin_bit_cast(unsigned, v.z), c3 = __builtin_bit_cast(unsigned, v.w);
    auto s01 = __builtin_amdgcn_permlane16_swap(c0, c1, false, false);
    auto s23 = __builtin_amdgcn_permlane16_swap(c2, c3, false, false);
    auto t02 = __builtin_amdgcn_permlane32_swap(s01[0], s23[0], false, false);
    auto t13 = __builtin_amdgcn_permlane32_swap(s01[1], s23[1], false, false);
    v.x = __builtin_bit_cast(float, (unsigned)t02[0]);
    v.y = __builtin_bit_cast(float, (unsigned)t13[0]);
    v.z = __builtin_bit_cast(float, (unsigned)t02[1]);
    v.w = __builtin_bit_cast(float, (unsigned)t13[1]);
}

template <int EPI, int DEPTH /* chunks in the register ring; K / 64 is a multiple of it */, bool SIG /* A in the sigma K layout, W_sig tiled in load order */>
__global__ __launch_bounds__(128) void gemm_smallm_kernel(GemmArgs g) {
    constexpr int KC = 64;                       // k per chunk (GLU: two waves per output tile, value + gate)
    __shared__ float gate[64][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = wave;                       // GLU: wave 0 = value tile, wave 1 = gate tile
    const int r = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const bool active = m0 < g.M;                // wave-uniform
    sm_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    // epilogue operands first (bias, residual rows): their round trips hide under the chain instead of following it
    const int col = n0 + r;
    float bias = 0.0f, bias_g = 0.0f, res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active && half == 0 && col < g.N) {
        if (g.bias) bias = g.bias[col];
        if constexpr (EPI == EPI_GLU) bias_g = g.bias ? g.bias[g.N + col] : 0.0f;
        if constexpr (EPI == EPI_RESID) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + 4 * kq + i;
                if (row < g.M) res[i] = g.resid[(int64_t)row * g.ldr + col];
            }
        }
    }
    if (active) {
        int arow = m0 + r;
        arow = arow < g.M ? arow : g.M - 1;
        int wrow = n0 + r;
        wrow = wrow < g.N ? wrow : g.N - 1;
        const float *ap = g.A + (int64_t)arow * g.lda + 4 * kq;
        // SIG: W_sig is TILED -- the 16 rows x 64 k of (column tile, chunk) are one contiguous 4 KB block in load order [q][lane][4], so a wave's
        // load instruction reads 1 KB of consecutive addresses and its whole weight stream is one contiguous run of 16 K floats
        const float *wp = SIG ? g.W_sig + (int64_t)((half * g.N + n0) >> 4) * 16 * g.K + 4 * lane : g.W + (int64_t)(half * g.N + wrow) * g.ldw + 4 * kq;
        float4 ra[DEPTH][4], rw[DEPTH][4];
        auto gload = [&](int kc, int set) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rw[set][q] = *reinterpret_cast<const float4 *>(SIG ? wp + kc * (16 * KC) + 256 * q : wp + kc * KC + 16 * q);
                ra[set][q] = *reinterpret_cast<const float4 *>(ap + kc * KC + 16 * q);
            }
            __builtin_amdgcn_sched_barrier(0);   // the loads stay HERE, DEPTH - 1 chunks ahead of their use (the scheduler would sink them)
        };
        // No branch inside the unrolled group: a conditional load makes the compiler's s_waitcnt bookkeeping drain the ring to vmcnt(0)
        // every chunk.  The loads past the end re-read the last chunk (hot lines, never consumed).
        const int nkc = g.K / KC, last = nkc - 1;
#pragma unroll
        for (int j = 0; j < DEPTH - 1; ++j) gload(j < last ? j : last, j);
        for (int kc0 = 0; kc0 < nkc; kc0 += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                const int nx = kc0 + j + DEPTH - 1;
                if (DEPTH > 1) gload(nx < last ? nx : last, (j + DEPTH - 1) % DEPTH);
                else gload(kc0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 a = ra[j][q], w = rw[j][q];
                    if (!SIG) {
                        sm_tr4x4(a);
                        sm_tr4x4(w);
                    }
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc, 0, 0, 0);
                }
            }
        }
    }
    if constexpr (EPI == EPI_GLU) {
        if (active && half == 1) *reinterpret_cast<sm_f32x4 *>(&gate[lane][0]) = acc;
        __syncthreads();
        if (half == 1) return;
    }
    if (!active) return;
    // epilogue: C/D layout of 16x16x4: column = lane & 15, row = 4 * (lane >> 4) + i
    if (col >= g.N) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + 4 * kq + i;
        if (row >= g.M) continue;
        float gt = 0.0f;
        if constexpr (EPI == EPI_GLU) gt = gate[lane][i];
        gemm_store(g, row, col, epi_finish<EPI>(acc[i], g.bias != nullptr, bias, gt, bias_g, res[i], g.alpha, false));
    }
}

// Two 16-row tiles per wave (SIG operands only): the tiles share the W operand and their two independent chains are issued alternately -- 64 clocks
// per MFMA pair instead of 44 per single MFMA, so each chain is ~1.45x slower, but the launch has half the waves and reads W once per pair.
// For the shapes where one wave per tile would put more waves on the chip than it has SIMDs (a whole 10-30 s utterance against a wide product:
// fc1 of tdt-ctc-110m at M = 126 is 1024 waves asking L2 for 64 MB), which are bound by L2 traffic and not by the chain.
template <int EPI>
__global__ __launch_bounds__(64) void gemm_smallm_rt2_kernel(GemmArgs g) {
    constexpr int KC = 64, DEPTH = 4;
    const int lane = threadIdx.x, r = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 32;
    sm_f32x4 acc[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    const int col = n0 + r;
    float bias = 0.0f, res[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    if (col < g.N) {
        if (g.bias) bias = g.bias[col];
        if constexpr (EPI == EPI_RESID) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = m0 + 16 * t + 4 * kq + i;
                    if (row < g.M) res[t][i] = g.resid[(int64_t)row * g.ldr + col];
                }
        }
    }
    const float *ap[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int arow = m0 + 16 * t + r;
        arow = arow < g.M ? arow : g.M - 1;
        ap[t] = g.A + (int64_t)arow * g.lda + 4 * kq;
    }
    const float *wp = g.W_sig + (int64_t)(n0 >> 4) * 16 * g.K + 4 * lane;
    float4 ra[DEPTH][2][4], rw[DEPTH][4];
    auto gload = [&](int kc, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rw[set][q] = *reinterpret_cast<const float4 *>(wp + kc * (16 * KC) + 256 * q);
            ra[set][0][q] = *reinterpret_cast<const float4 *>(ap[0] + kc * KC + 16 * q);
            ra[set][1][q] = *reinterpret_cast<const float4 *>(ap[1] + kc * KC + 16 * q);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    const int nkc = g.K / KC, last = nkc - 1;
#pragma unroll
    for (int j = 0; j < DEPTH - 1; ++j) gload(j < last ? j : last, j);
    for (int kc0 = 0; kc0 < nkc; kc0 += DEPTH) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            const int nx = kc0 + j + DEPTH - 1;
            gload(nx < last ? nx : last, (j + DEPTH - 1) % DEPTH);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 w = rw[j][q], a0 = ra[j][0][q], a1 = ra[j][1][q];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, w.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, w.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, w.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, w.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, w.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, w.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, w.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, w.w, acc[1], 0, 0, 0);
            }
        }
    }
    if (col >= g.N) return;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + 16 * t + 4 * kq + i;
            if (row >= g.M) continue;
            gemm_store(g, row, col, epi_finish<EPI>(acc[t][i], g.bias != nullptr, bias, 0.0f, 0.0f, res[t][i], g.alpha, false));   // (no GLU form: two row tiles share W)
        }
}

// The chain kernel with the LayerNorm of its input rows folded in (GemmArgs::ln_g / ln_b / ln_eps; A = the UN-normalised rows x[M][K], K = the
// row length, 512 or 1024): out = epi(LayerNorm(x) W^T + bias), bit for bit what layernorm_kernel followed by gemm_smallm_kernel<.., SIG> give.
// Round 3 folded the norm into the one-wave-per-tile kernel and lost (every wave re-derived the statistics of its 16 rows alone: 3-4 us in front
// of its chain).  Here a workgroup is FOUR waves: each normalises four of the tile's 16 rows the way layernorm_kernel does (one wave per row,
// lane l holds elements l + 64 j, ln_row_stats of pk_devmath.h, y = fma((x - mean) rstd, gamma, beta)) and stores them to LDS in the sigma K
// order at a pitch of K + 4 floats; after one barrier waves 0 and 1 run the dependent MFMA chains of two column tiles (GLU: the value and the
// gate tile of the same 16 columns) with their A fragments from LDS (one chunk ahead of the chain, conflict-free ds_read_b128) and the tiled
// weight stream in the same 8-chunk register ring as gemm_smallm_kernel -- requested BEFORE the rows, so the weights' HBM round trip covers the
// normalisation.  Saves the LayerNorm launch (~5 us of a 32-row streaming chunk's ~360) for ~1 us in front of the chain.
// DW (EPI_GLU; kernels.hpp DwTail): the streaming conv module's depthwise conv + BatchNorm + SiLU run by the lane that finishes (stream, channel) --
// every point is the dwconv_point (pk_devmath.h) that stream_dwconv_kernel (kernels/stream.hip) calls; one launch less per block.
// PRE (GemmArgs::pre_g): another LayerNorm in front of the folded one.  Both are template parameters: as run-time branches they cost every
// instantiation 64 VGPRs (K = 1024: 240 -> 304, one workgroup per CU instead of two -- 64 sessions ran 14 % slower for it).
template <int EPI, int PER_LANE /* K / 64 */, bool DW = false, bool PRE = false>
__global__ __launch_bounds__(256) void gemm_smallm_ln_kernel(GemmArgs g, DwTail dw = DwTail{}) {
    static_assert(!DW || EPI == EPI_GLU, "the conv tail finishes a GLU tile");
    constexpr int K = 64 * PER_LANE, PITCH = K + 4, KC = 64, NKC = PER_LANE, DEPTH = 8;
    static_assert(NKC % DEPTH == 0, "the ring walks whole groups of 8 chunks");
    extern __shared__ __attribute__((aligned(16))) float At[];     // [16][PITCH]: the normalised rows of the tile, K in the sigma order
    __shared__ float gate[64][4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.y * 16;
    const int half = (EPI == EPI_GLU) ? (wave & 1) : 0;            // GLU: wave 0 = value tile, wave 1 = gate tile
    const int n0 = (EPI == EPI_GLU) ? blockIdx.x * 16 : (2 * blockIdx.x + (wave & 1)) * 16;
    const bool chain = wave < 2 && n0 < g.N;                        // (wave-uniform)
    // ---- chain waves: epilogue operands and the head of the weight stream first ----
    const int col = n0 + r;
    float bias = 0.0f, bias_g = 0.0f;
    float4 rw[DEPTH][4];
    const float *wp = g.W_sig + (int64_t)((half * g.N + (chain ? n0 : 0)) >> 4) * 16 * K + 4 * lane;
    auto wload = [&](int kc, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rw[set][q] = *reinterpret_cast<const float4 *>(wp + kc * (16 * KC) + 256 * q);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (chain) {
        if (half == 0 && col < g.N && g.bias) {
            bias = g.bias[col];
            if constexpr (EPI == EPI_GLU) bias_g = g.bias[g.N + col];
        }
#pragma unroll
        for (int j = 0; j < DEPTH - 1; ++j) wload(j, j);
    }
    // conv tail: the cached rows of this lane's streams (rows m0 + 4 kq .. + 3 = 4 / c streams of c frames) and the conv's parameters of its channel
    // (mirrors DwTailRegs::load / finish of gemm_epi.hpp, written out here: through the struct the K = 1024 instantiation spills 8 VGPRs instead of 4)
    [[maybe_unused]] float dpre[4][8], dwk[9], dbs = 0.0f, dmu = 0.0f, drs = 0.0f, dbg = 0.0f, dbb = 0.0f;
    if constexpr (DW) {
        if (chain && half == 0 && col < g.N) {
            const int nstr = 4 / dw.c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rw0 = m0 + 4 * kq + j * dw.c;
                const bool on = j < nstr && rw0 < g.M && dw.has_cache;
                const int64_t sidx = on ? rw0 / dw.c : 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) dpre[j][q] = on ? dw.cache_in[(sidx * 8 + q) * g.N + col] : 0.0f;   // (first chunk: zero left padding)
            }
#pragma unroll
            for (int kk = 0; kk < 9; ++kk) dwk[kk] = dw.w[kk * g.N + col];
            dbs = dw.bias[col]; dmu = dw.bn_mean[col]; drs = dw.bn_rstd[col]; dbg = dw.bn_g[col]; dbb = dw.bn_b[col];
        }
    }
    // ---- every wave: LayerNorm of rows m0 + 4 wave .. + 3, one wave per row with layernorm_kernel's ln_row_stats ----
    {
        float gv[PER_LANE], bv[PER_LANE], v[4][PER_LANE];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int row = m0 + 4 * wave + rr;
            row = row < g.M ? row : g.M - 1;                        // (rows past the end repeat the last one; their outputs are never stored)
            const float *xr = g.A + (int64_t)row * g.lda;
#pragma unroll
            for (int j = 0; j < PER_LANE; ++j) v[rr][j] = xr[lane + 64 * j];
        }
        // A norm in front of the folded one (GemmArgs::pre_g: a block's final_norm_ riding on the next block's first product; streaming): the wave
        // normalises its rows (ln_row_stats, layernorm_kernel's fma: the bits of the separate launch), keeps them in
        // registers, and the first K / 64 column-tile workgroups write them out, one 64-element chunk of every row each: the residual stream of the block that starts here.
        if constexpr (PRE) {
#pragma unroll
            for (int j = 0; j < PER_LANE; ++j) {
                gv[j] = g.pre_g[lane + 64 * j];
                bv[j] = g.pre_b[lane + 64 * j];
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                float mean, rstd;
                ln_row_stats<PER_LANE>(v[rr], lane, K, g.ln_eps, mean, rstd);
                const int row = m0 + 4 * wave + rr;
                const bool put = g.pre_out && row < g.M;
#pragma unroll
                for (int j = 0; j < PER_LANE; ++j) {
                    v[rr][j] = __builtin_fmaf((v[rr][j] - mean) * rstd, gv[j], bv[j]);
                    if (put && (int)blockIdx.x == j) g.pre_out[(int64_t)row * g.pre_ldo + lane + 64 * j] = v[rr][j];   // (column tile j writes chunk j: gridDim.x >= PER_LANE)
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            gv[j] = g.ln_g[lane + 64 * j];
            bv[j] = g.ln_b[lane + 64 * j];
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            float mean, rstd;
            ln_row_stats<PER_LANE>(v[rr], lane, K, g.ln_eps, mean, rstd);
            float *yr = At + (4 * wave + rr) * PITCH;
#pragma unroll
            for (int j = 0; j < PER_LANE; ++j) yr[sigma_col(lane + 64 * j)] = __builtin_fmaf((v[rr][j] - mean) * rstd, gv[j], bv[j]);
        }
    }
    __syncthreads();
    if (!chain) return;
    // ---- the chain of this wave's tile: A fragments from LDS one chunk ahead, W from the ring ----
    sm_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const float *arow = At + r * PITCH + 4 * kq;
    float4 ra[2][4];
    auto aload = [&](int kc, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ra[set][q] = *reinterpret_cast<const float4 *>(arow + kc * KC + 16 * q);
    };
    aload(0, 0);
    constexpr int last = NKC - 1;
    for (int kc0 = 0; kc0 < NKC; kc0 += DEPTH) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            const int kc = kc0 + j, nx = kc + DEPTH - 1;
            wload(nx < last ? nx : last, (j + DEPTH - 1) % DEPTH);
            aload(kc + 1 < NKC ? kc + 1 : last, (j + 1) & 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = ra[j & 1][q], w = rw[j][q];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc, 0, 0, 0);
            }
        }
    }
    if constexpr (EPI == EPI_GLU) {
        if (half == 1) *reinterpret_cast<sm_f32x4 *>(&gate[lane][0]) = acc;
        __syncthreads();                                            // (waves 2 and 3 have ended: the barrier counts the two chain waves)
        if (half == 1) return;
    }
    if (col >= g.N) return;
    [[maybe_unused]] float glu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // epilogue: C/D layout of 16x16x4: column = lane & 15, row = 4 * (lane >> 4) + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + 4 * kq + i;
        if (row >= g.M) continue;
        float gt = 0.0f;
        if constexpr (EPI == EPI_GLU) gt = gate[lane][i];
        const float v = epi_finish<EPI>(acc[i], g.bias != nullptr, bias, gt, bias_g, 0.0f, 0.0f, false);   // (no residual form)
        if constexpr (DW) glu[i] = v;
        else gemm_store(g, row, col, v);
    }
    if constexpr (DW) {
        const int ocol = dw.out_sigma ? sigma_col(col) : col;
        auto tail = [&](auto cc) {
            constexpr int C = decltype(cc)::value;
#pragma unroll
            for (int j = 0; j < 4 / C; ++j) {
                const int rw0 = m0 + 4 * kq + j * C;
                if (rw0 >= g.M) continue;
                const int64_t sidx = rw0 / C;
                float cat[8 + C];
#pragma unroll
                for (int q = 0; q < 8; ++q) cat[q] = dpre[j][q];
#pragma unroll
                for (int f = 0; f < C; ++f) cat[8 + f] = glu[j * C + f];
#pragma unroll
                for (int f = 0; f < C; ++f) g.out[(int64_t)(rw0 + f) * g.ldo + ocol] = dwconv_point<9>(dwk, cat + f, dbs, dmu, drs, dbg, dbb);
#pragma unroll
                for (int q = 0; q < 8; ++q) dw.cache_out[(sidx * 8 + q) * g.N + col] = cat[q + C];
            }
        };
        if (dw.c == 1) tail(std::integral_constant<int, 1>{});
        else if (dw.c == 2) tail(std::integral_constant<int, 2>{});
        else tail(std::integral_constant<int, 4>{});
    }
}

// The two fusions lengthen the chain kernel (a second normalisation in front, the conv behind) and cost it registers (K = 1024: one workgroup per
// CU instead of two): they pay while the launch is a single round of workgroups -- 16 sessions x 2 frames: -1 % per fusion -- and lose beyond
// (64 sessions: +3 %, 128: +5 %; profiles/r05_stream_fusions_by_streams.txt).
static bool smallm_ln_one_round(const GemmArgs &a, int epi) {
    const int tiles = a.N / 16;
    return (int64_t)(epi == EPI_GLU ? tiles : (tiles + 1) / 2) * ((a.M + 15) / 16) <= 256;
}
bool gemm_smallm_pre_applies(const GemmArgs &a, int epi) {
    if (epi != EPI_SILU || !a.pre_g || !a.pre_b || (a.pre_out && (a.pre_out == a.A || a.pre_ldo < a.K)) || a.N < 32 * 16) return false;   // (>= 16 column-tile pairs share the write-out)
    return gemm_smallm_ln_applies(a, epi) && smallm_ln_one_round(a, epi);
}
bool gemm_smallm_dw_applies(const GemmArgs &a, int epi, int c, int kc) {
    if (epi != EPI_GLU || !stream_dwconv_tail_fusable(c, kc) || a.M % c != 0 || a.remap_rows != 0 || a.sigma_cols != 0) return false;
    return gemm_smallm_ln_applies(a, epi) && smallm_ln_one_round(a, epi);
}
bool gemm_smallm_ln_applies(const GemmArgs &a, int epi) {
    if (!a.ln_g || !a.ln_b || !a.W_sig || a.a_bf16 || a.a_sigma) return false;
    if (a.M <= 0 || a.M > kSmallMRows || (a.K != 512 && a.K != 1024) || a.N % 16 != 0 || a.lda < a.K) return false;
    return epi == EPI_NONE || epi == EPI_RELU || epi == EPI_SILU || epi == EPI_GLU;
}

// Which instantiation a product takes (kernels.hpp: GemmSmallmForm).  The launchers below switch on this function's result and pk_diag_gemm_smallm
// reports it: every threshold of the family lives here and nowhere else.
GemmSmallmForm gemm_smallm_form(const GemmArgs &a, int epi) {
    const int nkc = a.K / 64;
    if (a.ln_g)                                                     // LayerNorm folded in (the caller checked gemm_smallm_ln_applies: K = 512 / 1024)
        return gemm_smallm_form_of(SMALLM_LN, epi, a.K == 512 ? 8 : 16, true, epi == EPI_GLU && a.dw_tail, epi == EPI_SILU && a.pre_g);
    const bool sig = a.a_sigma && a.W_sig;
    // more waves than SIMDs (1024): two row tiles per wave (gemm_smallm_rt2_kernel)
    const int64_t col_tiles = (a.N + 15) / 16, row_tiles = (a.M + 15) / 16;
    if (sig && epi != EPI_GLU && nkc % 4 == 0 && row_tiles >= 4 && col_tiles * row_tiles >= 768) return gemm_smallm_form_of(SMALLM_RT2, epi, 4, true);
    return gemm_smallm_form_of(SMALLM_CHAIN, epi, nkc % 8 == 0 ? 8 : nkc % 2 == 0 ? 2 : 1, sig);
}
[[noreturn]] static void smallm_no_form(int form) {
    fprintf(stderr, "parakeet_amd: internal error: launch_gemm_smallm has no kernel for form %d\n", form);
    abort();
}

template <int EPI, int PER_LANE, bool DW, bool PRE>
static void launch_smallm_ln_inst(const GemmArgs &a, hipStream_t s) {
    const int tiles = a.N / 16;
    const dim3 grid(EPI == EPI_GLU ? tiles : (tiles + 1) / 2, (a.M + 15) / 16), block(256);
    const size_t lds = (size_t)16 * (a.K + 4) * sizeof(float);
    static DynLdsSlots slots;                                       // (one per instantiation)
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(&gemm_smallm_ln_kernel<EPI, PER_LANE, DW, PRE>), lds);
    hipLaunchKernelGGL((gemm_smallm_ln_kernel<EPI, PER_LANE, DW, PRE>), grid, block, lds, s, a, DW ? *a.dw_tail : DwTail{});
}
template <int EPI>
static void launch_smallm_ln(const GemmArgs &a, hipStream_t s) {
    const int form = gemm_smallm_form(a, EPI), per_lane = gemm_smallm_form_ring(form);
    if (per_lane != 8 && per_lane != 16) smallm_no_form(form);
    if constexpr (EPI == EPI_SILU) {
        if (gemm_smallm_form_pre(form)) {
            if (per_lane == 8) launch_smallm_ln_inst<EPI, 8, false, true>(a, s);
            else launch_smallm_ln_inst<EPI, 16, false, true>(a, s);
            return;
        }
    }
    if constexpr (EPI == EPI_GLU) {
        if (gemm_smallm_form_dw(form)) {
            if (per_lane == 8) launch_smallm_ln_inst<EPI, 8, true, false>(a, s);
            else launch_smallm_ln_inst<EPI, 16, true, false>(a, s);
            return;
        }
    }
    if (per_lane == 8) launch_smallm_ln_inst<EPI, 8, false, false>(a, s);
    else launch_smallm_ln_inst<EPI, 16, false, false>(a, s);
}

// W_sig of GemmArgs: dst[tile = row / 16][chunk = k / 64][q][lane = (row % 16) + 16 kq][e] = src[row][64 chunk + 16 q + 4 e + kq]
__global__ void sigma_copy_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t rows, int K, int64_t ld) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // destination index
    if (idx >= rows * K) return;
    const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63), q = (int)((idx >> 8) & 3);
    const int64_t blk = idx >> 10;                                         // (tile, chunk)
    const int nkc = K / 64;
    const int64_t tile = blk / nkc;
    const int kc = (int)(blk % nkc);
    dst[idx] = src[(tile * 16 + (lane & 15)) * ld + 64 * kc + 16 * q + 4 * e + (lane >> 4)];
}
void launch_sigma_copy(const float *src, float *dst, int64_t rows, int K, int64_t ld, hipStream_t s) {
    const int64_t n = rows * K;                                            // rows % 16 == 0, K % 64 == 0
    hipLaunchKernelGGL(sigma_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, K, ld);
}

template <int EPI>
static void launch_smallm_epi(const GemmArgs &a, hipStream_t s) {
    constexpr int NB = (EPI == EPI_GLU) ? 2 : 1;
    // one wave per workgroup (GLU: the value / gate pair): with a few hundred waves on 1024 SIMDs every chain gets a SIMD and an L1 of its own
    const dim3 grid((a.N + 15) / 16, (a.M + 15) / 16), block(64 * NB);
    const int form = gemm_smallm_form(a, EPI), ring = gemm_smallm_form_ring(form);
    if constexpr (EPI != EPI_GLU) {
        if (gemm_smallm_form_kernel(form) == SMALLM_RT2) {
            hipLaunchKernelGGL((gemm_smallm_rt2_kernel<EPI>), dim3(grid.x, (grid.y + 1) / 2), dim3(64), 0, s, a);
            return;
        }
    }
    if (gemm_smallm_form_kernel(form) != SMALLM_CHAIN) smallm_no_form(form);
    if (gemm_smallm_form_sig(form)) {
        if (ring == 8) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 8, true>), grid, block, 0, s, a);
        else if (ring == 2) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 2, true>), grid, block, 0, s, a);
        else if (ring == 1) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 1, true>), grid, block, 0, s, a);
        else smallm_no_form(form);
    } else {
        if (ring == 8) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 8, false>), grid, block, 0, s, a);
        else if (ring == 2) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 2, false>), grid, block, 0, s, a);
        else if (ring == 1) hipLaunchKernelGGL((gemm_smallm_kernel<EPI, 1, false>), grid, block, 0, s, a);
        else smallm_no_form(form);
    }
}

void launch_gemm_smallm(const GemmArgs &a, int epi, hipStream_t s) {
    if (a.ln_g) {                                                   // LayerNorm folded in (the caller checked gemm_smallm_ln_applies)
        switch (epi) {
        case EPI_NONE: launch_smallm_ln<EPI_NONE>(a, s); break;
        case EPI_RELU: launch_smallm_ln<EPI_RELU>(a, s); break;
        case EPI_SILU: launch_smallm_ln<EPI_SILU>(a, s); break;
        case EPI_GLU: launch_smallm_ln<EPI_GLU>(a, s); break;
        default: break;
        }
        return;
    }
    switch (epi) {
    case EPI_NONE: launch_smallm_epi<EPI_NONE>(a, s); break;
    case EPI_RELU: launch_smallm_epi<EPI_RELU>(a, s); break;
    case EPI_SILU: launch_smallm_epi<EPI_SILU>(a, s); break;
    case EPI_RESID: launch_smallm_epi<EPI_RESID>(a, s); break;
    case EPI_GLU: launch_smallm_epi<EPI_GLU>(a, s); break;
    default: break;
    }
}

}  // namespace pk
