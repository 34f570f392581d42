// parakeet.cpp_amd/csrc/kernels/gemm.hip -- fp32 MFMA GEMM with fused epilogues (gfx950).
//
// out[M][N] = epi(A[M][K] * W[N][K]^T + bias).  This one kernel template carries ~93 % of the
// encoder's arithmetic: every nn::Linear / 1x1 Conv call site of the reference
// (src/encoder.cpp:41-45 FFN, :120-122 QKV, :148 pos_proj, :177 out_proj, :63/:70 pointwise convs,
// :227/:231 subsampling 1x1 convs, :240 proj_; src/ctc.cpp:19; src/tdt.cpp:17 enc_proj_).
//
// Design for CDNA4:
//  * v_mfma_f32_32x32x2_f32: exact fp32, bit-identical to a k-ordered fmaf chain (64 FLOP/clk/SIMD,
//    157 TF peak).  Lanes 0-31 feed k = 2s, lanes 32-63 feed k = 2s+1, so the accumulation order is
//    the natural k = 0,1,2,... order the CPU oracle uses: results are bit-identical to the oracle.
//  * 256-thread workgroup = 4 wavefronts in a 2x2 grid; each wave owns a (BM/2)x(BN/2) sub-tile held
//    as TMxTN 32x32 accumulators (16 VGPRs each).
//  * K is tiled by 32: A and W tiles are staged global -> registers (float4, 128-B rows, coalesced)
//    -> LDS with a 33-float row pitch, so the per-lane scalar ds_read_b32 fragment reads
//    (32 different rows, same k) hit 32 different banks.  fp32 MFMA is slow enough (64 cycles per
//    32x32x2) that 2 LDS reads per MFMA use <15 % of the LDS issue rate.
//  * Double-buffered LDS: the global loads of tile k+1 are issued before the MFMAs of tile k and
//    written to the other buffer after them -> one __syncthreads per K tile.
//  * XCD-aware block swizzle: consecutive tiles (sharing A rows / W rows) stay on one XCD's L2.
//  * Epilogues (bias, ReLU, SiLU, residual + alpha*y, GLU) are applied to the accumulator registers:
//    no separate elementwise passes over HBM.
#include "../pk_devmath.h"
#include "kernels.hpp"
#include <cstdio>
#include <cstdlib>
#include "gemm_pipe.hpp"
#include "gemm_bf16.hpp"
#include "gemm_bf16_glds.hpp"

namespace pk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static constexpr int BK = 32;
static constexpr int LDP = BK + 1;  // LDS row pitch in floats

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g, int tiles_n, int n_tiles) {
    constexpr int WM = BM / 2, WN = BN / 2;      // wave sub-tile
    constexpr int TM = WM / 32, TN = WN / 32;    // 32x32 accumulators per wave
    constexpr int A_CH = BM * 8 / 256, W_CH = BN * 8 / 256;
    constexpr int NOUT = (EPI == EPI_GLU) ? BN / 2 : BN;  // output columns per block
    static_assert(EPI != EPI_GLU || (TN % 2 == 0), "GLU needs an even number of column tiles per wave");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    // XCD-aware bijective remap (block b runs on XCD b % 8): XCD x gets a contiguous range of tiles.
    int bid = blockIdx.x;
    {
        const int q = n_tiles >> 3, r = n_tiles & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * NOUT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // per-thread global source rows of the staging chunks
    const float *a_src[A_CH];
    const float *w_src[W_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int c = tid + 256 * i, row = c >> 3, c4 = c & 7;
        int gr = m0 + row;
        gr = gr < g.M ? gr : g.M - 1;
        a_src[i] = g.A + (int64_t)gr * g.lda + c4 * 4;
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
        const int c = tid + 256 * i, v = c >> 3, c4 = c & 7;
        int wr;
        if constexpr (EPI == EPI_GLU) {
            // virtual column v -> (wave column, tile, lane column); tiles [0,TN/2) are the value half,
            // tiles [TN/2,TN) the gate half of the SAME output columns, so one lane holds both.
            constexpr int HT = TN / 2;
            const int vw = v / WN, rem = v % WN, tn = rem >> 5, cc = rem & 31;
            int col = n0 + vw * (WN / 2) + (tn % HT) * 32 + cc;
            col = col < g.N ? col : g.N - 1;
            wr = (tn / HT) * g.N + col;
        } else {
            wr = n0 + v;
            wr = wr < g.N ? wr : g.N - 1;
        }
        w_src[i] = g.W + (int64_t)wr * g.ldw + c4 * 4;
    }

    float4 ra[A_CH], rw[W_CH];
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < A_CH; ++i) ra[i] = *reinterpret_cast<const float4 *>(a_src[i] + kt * BK);
#pragma unroll
        for (int i = 0; i < W_CH; ++i) rw[i] = *reinterpret_cast<const float4 *>(w_src[i] + kt * BK);
    };
    auto lstore = [&](int buf) {
        float *As = smem + buf * (BM + BN) * LDP;
        float *Ws = As + BM * LDP;
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            const int c = tid + 256 * i;
            float *d = As + (c >> 3) * LDP + (c & 7) * 4;
            d[0] = ra[i].x; d[1] = ra[i].y; d[2] = ra[i].z; d[3] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < W_CH; ++i) {
            const int c = tid + 256 * i;
            float *d = Ws + (c >> 3) * LDP + (c & 7) * 4;
            d[0] = rw[i].x; d[1] = rw[i].y; d[2] = rw[i].z; d[3] = rw[i].w;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int nk = g.K / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    const int frag = (lane & 31) * LDP + (lane >> 5);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const float *Ab = smem + cur * (BM + BN) * LDP + wm * WM * LDP + frag;
        const float *Wb = smem + cur * (BM + BN) * LDP + BM * LDP + wn * WN * LDP + frag;
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Ab[i * 32 * LDP + 2 * kk];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Wb[j * 32 * LDP + 2 * kk];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
    }

    epilogue_scalar_32x32<TM, TN, WN, EPI>(g, acc, m0, n0, wm, wn, lane, false);   // (an fp32-contract kernel: the polynomial activations)
}

template <int BM, int BN, int EPI>
static void launch_one(const GemmArgs &a, hipStream_t s) {
    constexpr int NOUT = (EPI == EPI_GLU) ? BN / 2 : BN;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + NOUT - 1) / NOUT;
    const int n_tiles = tiles_m * tiles_n;
    constexpr size_t lds = 2 * (size_t)(BM + BN) * LDP * sizeof(float);
    static DynLdsSlots slots;
    ensure_dyn_lds(slots, reinterpret_cast<const void *>(&gemm_nt_kernel<BM, BN, EPI>), lds);
    hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, EPI>), dim3(n_tiles), dim3(256), lds, s, a, tiles_n, n_tiles);
}

// Tile choice, from tools/ubench/gemm_sweep on MI355X (profiles/r01_gemm_sweep.txt): the pipelined kernels win where
// the K loop is short (most of the encoder is K = 512); wide outputs like 128x128 tiles on 8 waves, long-K / narrow-N
// products 128x64, everything else 64x64 (more resident workgroups to overlap one tile's epilogue with another's MFMAs).
// The tile table of the round-2 and round-6 engine measurements (profiles/r02_gemm_variant_ab.txt: step 20.44 -> 19.73 ms; r06_gemm_sweep_fc2_variants.txt).
// Variants measured and not kept (up to 4fb176f a run-time mask of EXPERIMENTAL builds, PK_GEMM_VARIANT): out_proj / pw2 on single-buffered
// 64x128 tiles (level), wide outputs on BK 64 (behind), 192x128 tiles where they make a whole round of workgroups (profiles/r04_gemm_tile192_ab.txt:
// qkv 1.97 -> 1.99 ms per step -- workgroups are handed out as slots free up, so a CU never idles for a 'round'), and the double-buffered forms of
// the single-buffered tiles below.
// Every single-buffered tile runs the hand-placed K loop (gemm_pipe_kernel SCHED = 2: staging spread over the MFMA gaps of the last sub-step,
// its last two k-steps after the second barrier under the next K tile's first fragment reads).  tools/ubench/gemm_sched on MI355X
// (profiles/r07_gemm_sched_sweep.txt), bit-equal everywhere: per launch fc1 + LayerNorm fold 181.7 -> 167.3 us, fc2 144.7 -> 128.8, qkv + fold
// 127.6 -> 123.7, GLU + fold 87.3 -> 76.4, out_proj / pw2 40.2 -> 39.1; main loop e.g. fc1 + fold 120.9 -> 131.7 TF.  SCHED = 1 and 3 are
// behind SCHED = 2 or level on every shape; the GLU product without the fold is the only level one (139.0 / 139.2 TF).  One exception, from the
// kernel trace of the bench (profiles/r07_kernel_stats_ab.txt): the long-K tile without an epilogue function (sub_proj, once per step) is
// slower with it (172 -> 185 us), so that product keeps the compiler-placed loop.
constexpr int kSbSched = kGemmTileSched;
// Which instantiation a product takes (kernels.hpp: GemmTileForm).  launch_gemm switches on this function's result and pk_diag_gemm_tile reports it:
// every threshold of the tile kernels lives here and nowhere else.
GemmTileForm gemm_tile_form(const GemmArgs &a, int epi) {
    const bool lna = a.ln_stats != nullptr;
    if (epi == EPI_GLU) {
        if (a.K < 64) return gemm_tile_nt_form(128, 128, EPI_GLU);
        return gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, lna, kSbSched, EPI_GLU);
    }
    if (a.K < 64) return gemm_tile_nt_form(64, 64, epi);                // pipelined kernels need >= 2 K tiles
    // measured table: profiles/r01_gemm_sweep_v5.txt (128x128 tile on 8 waves of 32x64 wins for every wide output and for the
    // 321k-row subsampling products; long-K / narrow-N products like fc2 of the 110M model take 128x64)
    // long-K products whose 128x128 tiles fill the chip exactly once (fc2 / sub_proj of the 110M model: 252 tiles for 256 CUs): one
    // 8-wave workgroup per CU, single-buffered -- 8 waves of 64 x 32, BK 32 (round 6): 2-3 % ahead of the BK 64 tile of 32 x 64 waves in the sweep
    // (profiles/r06_gemm_sweep_fc2_variants.txt: 137 vs 140.5 us), which was itself -6 % against two 128x64 workgroups
    const int64_t tiles128 = (int64_t)((a.M + 127) / 128) * ((a.N + 127) / 128);
    if (a.M >= 1024 && a.N >= 256 && a.K >= 1024 && a.K % 64 == 0 && tiles128 <= 256)
        return gemm_tile_form_of(TILE_PIPE, 2, 4, 2, 1, 1, false, epi == EPI_NONE ? 0 : kSbSched, epi);
    // round 2: the SINGLE-buffered loop (template parameter NBUF = 1: half the LDS, two barriers per K tile) is ahead of the double-buffered
    // one on every large shape, in the micro-benchmark (tools/ubench/gemm_sweep ml: main loop 130-135 vs 118-125 TF) and, by less, in the
    // engine (fc2 -8 %, fc1 -3.6 %, qkv -5 %, GLU -3 %).
    const GemmTileForm wide = gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, false, kSbSched, epi);
    if (lna && epi != EPI_RESID) return gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, true, kSbSched, epi);   // (gemm_ln_stats_applies: the wide-output tile, LayerNorm applied while staging A)
    if (a.M >= 1024 && (a.N >= 1024 || (a.M >= 65536 && a.N >= 256))) return wide;
    if (a.M >= 1024 && a.N >= 256 && a.K >= 1024) return gemm_tile_form_of(TILE_PIPE, 2, 2, 2, 1, 2, false, 0, epi);
    if (a.M >= 1024 && a.N >= 256) return wide;                         // out_proj / pw2 on 128x128 / 8 waves (0.81 -> 0.77 ms per step)
    return gemm_tile_form_of(TILE_PIPE, 2, 2, 1, 1, 2, false, 0, epi);
}
[[noreturn]] static void tile_no_form(int form, int epi) {
    fprintf(stderr, "parakeet_amd: internal error: launch_gemm has no tile kernel for form %d with epilogue %d\n", form, epi);
    abort();
}
// One case per tile geometry and loop; the `if constexpr` beside it names the epilogues that geometry is instantiated for (kGemmTileForms).
template <int EPI>
static void launch_tile(const GemmArgs &a, GemmTileForm f, hipStream_t s) {
    if (gemm_tile_form_epi(f) != EPI) tile_no_form(f, EPI);
    switch (gemm_tile_form_shape(f)) {
    case gemm_tile_form_shape(gemm_tile_nt_form(64, 64, 0)):
        if constexpr (EPI != EPI_GLU) { launch_one<64, 64, EPI>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_nt_form(128, 128, 0)):
        if constexpr (EPI == EPI_GLU) { launch_one<128, 128, EPI>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 2, 4, 2, 1, 1, false, 0, 0)):
        if constexpr (EPI == EPI_NONE) { launch_gemm_pipe<2, 4, 2, 1, 32, EPI, 1, false, 0>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 2, 4, 2, 1, 1, false, kSbSched, 0)):
        if constexpr (EPI == EPI_RELU || EPI == EPI_SILU || EPI == EPI_RESID) { launch_gemm_pipe<2, 4, 2, 1, 32, EPI, 1, false, kSbSched>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, false, kSbSched, 0)):
        launch_gemm_pipe<4, 2, 1, 2, 32, EPI, 1, false, kSbSched>(a, s);
        return;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, true, kSbSched, 0)):
        if constexpr (EPI != EPI_RESID) { launch_gemm_pipe<4, 2, 1, 2, 32, EPI, 1, true, kSbSched>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 2, 2, 2, 1, 2, false, 0, 0)):
        if constexpr (EPI != EPI_GLU) { launch_gemm_pipe<2, 2, 2, 1, 32, EPI>(a, s); return; }
        break;
    case gemm_tile_form_shape(gemm_tile_form_of(TILE_PIPE, 2, 2, 1, 1, 2, false, 0, 0)):
        if constexpr (EPI != EPI_GLU) { launch_gemm_pipe<2, 2, 1, 1, 32, EPI>(a, s); return; }
        break;
    default: break;
    }
    tile_no_form(f, EPI);
}

void launch_gemm_smallm(const GemmArgs &a, int epi, hipStream_t s);   // kernels/gemm_smallm.hip

// The products whose LayerNorm can ride on the A staging of the fp32 tile kernel (GemmArgs::ln_stats): exactly the shapes gemm_tile_form
// sends to the single-buffered 128 x 128 / BK 32 tile -- wide outputs of large batches (fc1, qkv) and the GLU product.
bool gemm_ln_stats_applies(const GemmArgs &a, int epi) {
    if (!a.ln_g || !a.ln_b || !a.ln_stats || a.a_bf16 || a.out_bf16 || a.fast_act || a.a_sigma || a.W_sig) return false;
    if (a.M <= kSmallMRows || a.K < 64 || a.K % 32 != 0 || (a.lda & 3) != 0 || (a.ldw & 3) != 0) return false;
    if (epi == EPI_GLU) return true;
    if (epi != EPI_NONE && epi != EPI_RELU && epi != EPI_SILU) return false;
    const int64_t tiles128 = (int64_t)((a.M + 127) / 128) * ((a.N + 127) / 128);
    if (a.K >= 1024 && a.K % 64 == 0 && tiles128 <= 256 && a.N >= 256) return false;     // (the long-K single-round tile has no LNA instantiation)
    return a.M >= 1024 && a.N >= 1024;
}

bool gemm_tile_applies(const GemmArgs &a) { return !(a.M <= kSmallMRows && a.K % 64 == 0); }

const char *gemm_tile_refusal(const GemmArgs &a, int epi) {
    if (epi == EPI_GLU && a.sigma_cols != 0) return "a GLU product with sigma_cols on a tile kernel (the wide epilogue reads the sigma columns without the GLU column mapping)";
    if (epi == EPI_RESID && a.sigma_cols != 0) return "a residual product with sigma_cols on a tile kernel (the wide epilogue adds the residual by output position, the scalar one by natural column)";
    if (a.K < 32 || a.K % 32 != 0) return "K is no positive multiple of 32 (the tile kernels run K / 32 whole K tiles)";
    if ((a.lda & 3) != 0 || (a.ldw & 3) != 0) return "lda or ldw is no multiple of 4 (the tile kernels stage their operands with 16-byte loads)";
    return nullptr;
}

// A product on the tile kernels (gemm_tile_applies).  Returns the form it launched: the one value both the dispatch below and pk_diag_gemm_tile's report come from.
GemmTileForm launch_gemm_tile(const GemmArgs &a, int epi, hipStream_t s) {
    if (const char *why = gemm_tile_refusal(a, epi)) { fprintf(stderr, "parakeet_amd: internal error: %s\n", why); abort(); }
    const GemmTileForm f = gemm_tile_form(a, epi);
    switch (epi) {
    case EPI_NONE: launch_tile<EPI_NONE>(a, f, s); break;
    case EPI_RELU: launch_tile<EPI_RELU>(a, f, s); break;
    case EPI_SILU: launch_tile<EPI_SILU>(a, f, s); break;
    case EPI_RESID: launch_tile<EPI_RESID>(a, f, s); break;
    case EPI_GLU: launch_tile<EPI_GLU>(a, f, s); break;
    default: break;
    }
    return f;
}

void launch_gemm(const GemmArgs &a, int epi, hipStream_t s) {
    if (a.ln_stats && !gemm_ln_stats_applies(a, epi)) { fprintf(stderr, "parakeet_amd: internal error: GemmArgs::ln_stats on a product the tile kernel does not fold it into\n"); abort(); }
    // up to a few hundred rows (streaming chunks, ONE utterance of up to a minute -- the reference's own benchmark protocol is batch 1):
    // one wavefront per 16x16 tile ((M/16)(N/16) independent waves) instead of a few dozen fat workgroups with a long K loop each.
    // Measured with tools/bench_reference_protocol.py: 10 s clip (M = 126) 6.3 -> 2.9 ms, 30 s (M = 376) 6.7 -> 4.3 ms per encoder pass.
    if (!gemm_tile_applies(a)) { launch_gemm_smallm(a, epi, s); return; }
    launch_gemm_tile(a, epi, s);
}

// bf16 operands / fp32 accumulate (a.W points to bf16 weights [N][K]); K % 64 == 0
// The direct-to-LDS bf16 kernel (gemm_bf16_glds.hpp; activations already bf16 in HBM), 256x256 macro tiles.  Measured inside the engine on
// tdt-600m (profiles/r03_bf16_tile_ab.txt): it is ahead of the register-staged 128x128 kernel where one operand is large -- fc1 (N = 4096:
// 6.70 -> 6.60 ms per step) and fc2 (K = 4096: 6.51 -> 6.11) -- and behind on qkv (2.50 -> 2.70), the GLU product (1.75 -> 2.03) and the
// N = 1024 / K = 1024 products; 256x128 and 128x128-on-4-waves variants lose everywhere.  The second pass (tools/ubench/gemm_bf16_k.cpp) found
// why: the 256-row tile count of those products falls between two rounds of the 256 CUs; with the tile height chosen per product (below) the
// kernel is ahead everywhere.  (Up to 4fb176f, EXPERIMENTAL builds selected the other tile forms -- 256x128, 128x128 on 4 waves of 64x64, 256x256
// or 192x256 everywhere -- with PK_BF16_TILE.)
// Forms of the direct-to-LDS kernel measured and not kept (up to 4fb176f selected in EXPERIMENTAL builds by PK_BF16_PERSIST / PK_BF16_FLAGS):
//  * persistent with the LDS epilogue (round 4, profiles/r04_bf16_persist_ab.txt, interleaved A/B on one box, tdt-600m 32 x 30 s): bit-for-bit
//    the same results, qkv 2.45 -> 2.41 ms and GLU 1.82 -> 1.77 ms per step, but fc1 6.75 -> 7.17 (140 -> 150 us) and the step 27.62 -> 27.94 ms:
//    inside one launch the next tile cannot start before `s_waitcnt vmcnt(0)` has ALSO drained the epilogue's stores (gfx950 counts loads and
//    stores in one counter, and they complete out of order relative to each other), which costs more than the cold prologue and the re-dispatch
//    it removes; and the epilogue, confined to one 64 KB buffer, needs 8 row bands instead of 4;
//  * the continuous-stream kernel (ring of four 32-k slots, counted vmcnt; plain, STAGGER, PHASED, PHASED + s_setprio): correct and NOT faster
//    than the persistent form -- the K loop is not bound by the DMA's latency (r05_bf16_ring_ab.txt, r05_bf16_phased_ab.txt; SQ counters
//    r05_pmc_sq_600m_bf16_p*.md: the matrix pipe is busy 31-33 % of the launch in every form): it is bound by what a CU can pull from L2 into
//    LDS (64 KB per 64-k tile at ~14 B/clock against the 32 B/clock the MFMAs could use), not by how the pulls are scheduled;
//  * STAGGER (half the waves of a SIMD issue their DMA after the first MFMA group, profiles/r05_bf16_stagger_template_ab.txt) and the row-block walk of
//    the persistent form (XCD x owns a block of tile rows: fetch bytes per fc1 launch 176 -> 150 MB, time +1.5 %, profiles/r05_bf16_rowblock_ab.txt);
//  * residual products accumulated onto the residual in the un-swapped MFMA layout (GemmArgs::resid_init, profiles/r05_bf16_resid_init_ab.txt):
//    fc2 123 -> 144 us, out_proj / pw2 24.5 -> 34.5 us -- the residual arrived as 96 four-byte loads per wave in front of the first MFMA, dearer
//    than the coalesced float4 reads of the LDS epilogue.  The register residual epilogue of round 6 does the same arithmetic with 16-byte accesses.
// What production runs (launch_gemm_bf16_glds): the persistent form with the DIRECT register epilogue (round 5) for the products without a residual
// read whose tiles exceed one round of the CUs -- bit-identical results, fc1 142 -> 134 us, qkv / GLU -4 %, the tdt-600m step 27.11 -> 26.73 ms
// (profiles/r05_bf16_direct_epilogue_ab.txt, r05_bf16_ring_ab.txt: three interleaved repetitions each) -- the direct epilogue on one tile per
// workgroup otherwise, the register residual epilogue for the residual products (round 6), and hand-counted fragment reads (ASMFRAG: bit-identical,
// -0.7 % per tdt-600m step, profiles/r05_bf16_asmfrag_ab.txt).

// the one rule both gemm_bf16_form and gemm_bf16_blocked_handoff apply: the product runs on the tile-height-per-product direct-to-LDS kernels
static bool bf16_glds_rule(int M, int N, int K) {
    return M >= 8192 && N >= 512 && K >= 128 && (int64_t)N * K >= (int64_t)1024 * 1024 && (N & 3) == 0;
}
bool gemm_bf16_blocked_handoff(int M, int N, int K, int epi, bool producer) {
    if (!bf16_glds_rule(M, N, K) || (N % 16) != 0 || (K % 64) != 0) return false;
    if (!producer) return true;                                     // every gemm_bf16_glds_kernel form reads the blocked A
    return epi != EPI_RESID && (int64_t)(M + 31) * N < ((int64_t)1 << 31);   // the register epilogue writes it (callers set fast_act: bf16 mode)
}

// Which instantiation a product takes (kernels.hpp: GemmBf16Form).  launch_gemm_bf16 switches on this function's result and pk_diag_gemm_bf16_tile reports
// it: every threshold of the bf16 tile kernels lives here (the register epilogues' predicates: gl_epilogue_form) and nowhere else.
GemmBf16Form gemm_bf16_form(const GemmArgs &a, int epi) {
    const bool a16 = a.a_bf16 != 0;
    if (a.one_form && epi != EPI_GLU) return gemm_bf16_form_of(BF16_REG, 2, 2, 1, 1, a16, BF16_EPI_LDS, epi);   // (GemmArgs::one_form: no threshold in M)
    if (a16 && bf16_glds_rule(a.M, a.N, a.K) && (a.lda % 8) == 0 && (a.ldw % 8) == 0 && a.remap_rows == 0 && (a.ldo & 3) == 0) {
        // One tile per CU and round (128 KB of LDS): the kernel's time is rounds x (tile's K loop + ~12 us of prologue / epilogue), so the tile
        // HEIGHT is chosen per product for the fewest, fullest rounds of the 256 CUs (tools/ubench/gemm_bf16_k.cpp, profiles/r03_gemm_bf16_k.txt:
        // main loop 1.3 PF on either tile).  tdt-600m (M = 12032): fc1 (N 4096) 752 tiles of 256 rows = 2.94 rounds; fc2 / out / pw2 (N 1024) 252
        // tiles of 192 rows = ONE round (188 of 256 rows leave 68 CUs idle: 113 -> 99 us); qkv (N 3072) 756 of 192 = 2.95 rounds (564 of 256 = 2.2).
        const int NOUT = (epi == EPI_GLU) ? 128 : 256;
        auto est = [&](int R) {
            const int64_t tiles = (int64_t)((a.M + R - 1) / R) * ((a.N + NOUT - 1) / NOUT);
            return (double)((tiles + 255) / 256) * ((double)R * a.K * 1.008e-4 + 12.0);
        };
        if (est(192) < est(256)) return gemm_bf16_form_of(BF16_GLDS, 2, 4, 3, 2, true, gl_epilogue_form(a, epi, 192), epi);
        return gemm_bf16_form_of(BF16_GLDS, 4, 2, 2, 4, true, gl_epilogue_form(a, epi, 256), epi);
    }
    // round 2: the staging stores decide the rate of this kernel.  As 16-byte ds_write_b128 the 128x128 tile ran at 320-340 TF and 256x256
    // macro tiles were the way to 450 (profiles/r02_gemm_bf16_tiles.txt); the SAME 16 bytes written as a ds_write2_b64 pair
    // (gemm_bf16.hpp, lstore) take the 128x128 tile to 580 TF in the sweep and 510-600 TF in the engine (profiles/r02_gemm_bf16_ablation.txt)
    // -- the 16-byte LDS store is pathologically slow next to fragment reads on gfx950, as the fp32 kernel had already shown.
    if (epi == EPI_GLU || (a.M >= 1024 && (a.N >= 1024 || (a.M >= 65536 && a.N >= 256))))
        return gemm_bf16_form_of(BF16_REG, 4, 2, 1, 2, a16, BF16_EPI_LDS, epi);      // 128x128 on 8 waves of 32x64 (also the 1.4 M-row subsampling products)
    if (a.M >= 1024 && a.N >= 256) return gemm_bf16_form_of(BF16_REG, 2, 2, 2, 1, a16, BF16_EPI_LDS, epi);
    return gemm_bf16_form_of(BF16_REG, 2, 2, 1, 1, a16, BF16_EPI_LDS, epi);
}
static const char *bf16_form_refusal(const GemmArgs &a, GemmBf16Form f) {
    if ((f >> 18) == BF16_REG)
        return (a.out_blocked || a.a_blocked) ? "blocked activation layout requested for the register-staged bf16 kernel (GemmArgs::out_blocked / a_blocked on a kernel that does not implement it)" : nullptr;
    const int efo = (f >> 3) & 3;                                  // (only gl_epilogue_direct writes the blocked layout)
    return (a.out_blocked && efo != BF16_EPI_DIRECT && efo != BF16_EPI_PERSIST) ? "blocked output on the LDS epilogue" : nullptr;
}
const char *gemm_bf16_refusal(const GemmArgs &a, int epi) { return bf16_form_refusal(a, gemm_bf16_form(a, epi)); }
[[noreturn]] static void bf16_no_form(int form, int epi) {
    fprintf(stderr, "parakeet_amd: internal error: launch_gemm_bf16 has no tile kernel for form %d with epilogue %d\n", form, epi);
    abort();
}
// One case per kernel, geometry and A type; the `if constexpr` beside it names the epilogue functions that geometry is instantiated for (kGemmBf16Forms).
template <int EPI>
static void launch_bf16_tile(const GemmArgs &a, GemmBf16Form f, hipStream_t s) {
    if (gemm_bf16_form_epi(f) != EPI) bf16_no_form(f, EPI);
    const int efo = (f >> 3) & 3;
    switch (gemm_bf16_form_shape(f) & ~(3 << 3)) {
    case gemm_bf16_form_of(BF16_GLDS, 2, 4, 3, 2, true, 0, 0):
        if (launch_gemm_bf16_glds<2, 4, 3, 2, EPI>(a, efo, s)) return;
        break;
    case gemm_bf16_form_of(BF16_GLDS, 4, 2, 2, 4, true, 0, 0):
        if (launch_gemm_bf16_glds<4, 2, 2, 4, EPI>(a, efo, s)) return;
        break;
    case gemm_bf16_form_of(BF16_REG, 4, 2, 1, 2, false, 0, 0):
        if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<4, 2, 1, 2, EPI, false>(a, s); return; }
        break;
    case gemm_bf16_form_of(BF16_REG, 4, 2, 1, 2, true, 0, 0):
        if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<4, 2, 1, 2, EPI, true>(a, s); return; }
        break;
    case gemm_bf16_form_of(BF16_REG, 2, 2, 2, 1, false, 0, 0):
        if constexpr (EPI != EPI_GLU) { if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<2, 2, 2, 1, EPI, false>(a, s); return; } }
        break;
    case gemm_bf16_form_of(BF16_REG, 2, 2, 2, 1, true, 0, 0):
        if constexpr (EPI != EPI_GLU) { if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<2, 2, 2, 1, EPI, true>(a, s); return; } }
        break;
    case gemm_bf16_form_of(BF16_REG, 2, 2, 1, 1, false, 0, 0):
        if constexpr (EPI != EPI_GLU) { if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<2, 2, 1, 1, EPI, false>(a, s); return; } }
        break;
    case gemm_bf16_form_of(BF16_REG, 2, 2, 1, 1, true, 0, 0):
        if constexpr (EPI != EPI_GLU) { if (efo == BF16_EPI_LDS) { launch_gemm_bf16_t<2, 2, 1, 1, EPI, true>(a, s); return; } }
        break;
    default: break;
    }
    bf16_no_form(f, EPI);
}
// A product on the bf16 tile kernels.  Returns the form it launched: the one value both the dispatch above and pk_diag_gemm_bf16_tile's report come from.
GemmBf16Form launch_gemm_bf16_tile(const GemmArgs &a, int epi, hipStream_t s) {
    const GemmBf16Form f = gemm_bf16_form(a, epi);
    if (const char *why = bf16_form_refusal(a, f)) { fprintf(stderr, "parakeet_amd: internal error: %s\n", why); abort(); }
    switch (epi) {
    case EPI_NONE: launch_bf16_tile<EPI_NONE>(a, f, s); break;
    case EPI_RELU: launch_bf16_tile<EPI_RELU>(a, f, s); break;
    case EPI_SILU: launch_bf16_tile<EPI_SILU>(a, f, s); break;
    case EPI_RESID: launch_bf16_tile<EPI_RESID>(a, f, s); break;
    case EPI_GLU: launch_bf16_tile<EPI_GLU>(a, f, s); break;
    default: break;
    }
    return f;
}
void launch_gemm_bf16(const GemmArgs &a, int epi, hipStream_t s) {
    // (a bf16 output goes through the wide epilogue only -- row-major, 4-column groups: Model::run_gemm checks)
    // a handful of rows (the streaming encoder's chunks): the weight-stream kernel of gemm_smallm_bf16.hip
    if (gemm_smallm_bf16_applies(a, epi)) { launch_gemm_smallm_bf16(a, epi, s); return; }
    launch_gemm_bf16_tile(a, epi, s);
}

double gemm_flops(const GemmArgs &a, int epi) {
    return 2.0 * (double)a.M * (double)a.N * (double)a.K * (epi == EPI_GLU ? 2.0 : 1.0);
}

}  // namespace pk
