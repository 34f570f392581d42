// parakeet.cpp_amd/csrc/kernels/gemm_smallm_bf16.hip -- the bf16 MFMA GEMM for a HANDFUL of rows (M <= kSmallMRowsBf16): the products of a
// streaming chunk (16 lock-step streams x 2 encoder frames against the 600M-parameter weight set) in the TOLERANCE-class mode
// (pk_config.gemm_bf16; BASELINE configs[4] with bf16 weights).
//
// out[M][N] = epi(bf16(A)[M][K] * W16[N][K]^T + bias), fp32 accumulation on v_mfma_f32_16x16x32_bf16; optionally with the LayerNorm of the
// input rows folded in (GemmArgs::ln_g): out = epi(bf16(LN(A)) W16^T + bias).
//
// Why a kernel of its own.  The exact (fp32) streaming mode is bound by its numerics contract: a natural-k fp32 chain issues 4 k per ~33 clocks,
// so fc2 of nemotron-600m (K = 4096) is a 14 us dependent chain whatever the bandwidth (gemm_smallm.hip; DESIGN.md section 5: 1.19 ms of
// chain per chunk).  The tolerance-class mode has no k-order contract: one MFMA takes 32 k in the same 8 passes (8x the k rate), and K may
// be SPLIT over the waves of a workgroup -- what is left is data movement: 8.4 MB of bf16 weights per ffn product from HBM, and the activation
// rows, which EVERY workgroup needs, from L2.
//   * one WORKGROUP per (16 output columns, R rows), `split` waves; wave w owns the K slices w, w + split, ... of 32 * STEPS k each and
//     requests its whole slice UP FRONT (STEPS 16-byte loads per lane and operand tile, no ring, no branch between the loads): every byte of a
//     product is in flight a few hundred clocks after the launch.  GLU: the value and the gate rows of the same 16 columns are two weight
//     tiles of the SAME wave (one set of activation registers feeds both).
//   * R = 32 (two 16-row MFMA tiles per wave sharing the W registers), 16 or 8 (one tile; rows 8..15 of the MFMA repeat rows 0..7 and are not
//     stored).  What a product costs is the bytes its busiest CU has to pull through its L1 -- measured ~45 GB/s per CU in this access pattern
//     (profiles/r04_stream_bf16_kernel_stats_v1.md: 64 workgroups of 8 waves took 13.3 us for fc2, 384 KB per CU) -- so a product with few column
//     tiles (N = 1024: 64) is cut into more, smaller workgroups: with R rows and 16 columns a workgroup pulls 2 K (R + 16) bytes (bf16 rows), and
//     the workgroups of one column tile run on the same XCD (grid.x is a multiple of 8), so the tile's weights leave HBM once.
//   * operands in their NATURAL layouts: lane (r = lane & 15, q = lane >> 4) supplies k = 32 s + 8 q .. + 7 of MFMA step s for row / column r:
//     one 16-byte load of a bf16 row (weights; activations when the producer stored bf16: GemmArgs::a_bf16) or two 16-byte loads of an fp32
//     row rounded with v_cvt_pk_bf16_f32 (RNE -- the rounding the big-tile bf16 kernel applies while staging, gemm_bf16.hpp).
//   * the partial sums of the `split` waves meet in LDS and are added in wave order (fixed: run-to-run deterministic); the first RT waves
//     then run the epilogue (bias, SiLU / ReLU / residual / GLU; fp32 or bf16 rows out).
//   * LayerNorm folded in (LN): A = the UN-normalised fp32 rows.  A streaming chunk is ~360 dependent launches of which 96 are LayerNorms over
//     32 rows -- ~5 us each for a fraction of a microsecond of work; here the workgroup that needs the normalised rows derives their statistics
//     itself: every wave already holds its K slice of the rows in registers (two-pass mean / variance as the oracle's layer_norm: the slices'
//     partial sums meet in LDS, added in wave order), normalises with gamma / beta staged once per wave in LDS, rounds to bf16.  Slices of
//     256 k, ONE per wave: K = 256 * split, split <= 8.  (The exact fp32 mode tried this in round 3 and lost: one WAVE per 16x16 tile
//     re-derived the statistics over the whole K, 3-4 us on the dependent chain.  Here they cost two LDS exchanges.)
//   * weights in OPERAND TILES (GemmArgs::W_t16, round 5): a copy of W16 in the order the lanes load it -- per (16 output columns, 32 k) one KB
//     [lane][8 bf16], tiles ordered [N / 16][K / 32] -- so a load instruction reads ONE contiguous KB instead of 16 row segments of 64 bytes
//     (tools/ubench/cu_ingest.cpp, profiles/r05_cu_ingest_patterns.txt: out of L2 a CU pulls 14-18 B/clk in whole lines against 10-12 B/clk in
//     64-byte segments of 16 rows; what a product costs is what its busiest CU pulls).  Same values in the same lanes: bit-identical results.
// Specification = the oracle's gemm_bf16 mode (oracle/pk_oracle.c linear_t: both operands rounded to bf16, k-ordered fp32 accumulation);
// the accumulation ORDER differs (MFMA blocks of 32 k, K slices), so results are compared within the mode's tolerance
// (tests/test_gpu_bf16.py: against float64 of the same rounded operands; tests/test_gpu_stream.py: the streaming mode against the oracle's;
// tests/test_gpu_smallm_bf16_gemm.py: every launch form alone, at operand pitches, the whole of every output buffer handed back).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include "../pk_devmath.h"
#include "kernels.hpp"
#include "gemm_epi.hpp"

namespace pk {

typedef float sb_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sb_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kSbMaxWaves = 8;      // waves per workgroup (2 per SIMD: 256 VGPRs each -- the up-front slices need them)

// Phase stamps for tools/ubench/smallm_bf16_trace.cpp (-DSB_TRACE): shader clock of lane 0 of every wave -- [workgroup][wave][8]: 0 kernel entry,
// 1 every load of the slice issued, 2 activation rows arrived (first use), 3 LayerNorm applied / rows converted, 4 weights arrived + MFMAs issued,
// 5 partial sums exchanged (after the barrier), 6 epilogue stores issued.  Production builds: nothing.
#ifdef SB_TRACE
__device__ unsigned long long *sb_trace;
#define SB_STAMP(i) do { if (sb_trace && (threadIdx.x & 63) == 0) sb_trace[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSbMaxWaves + (threadIdx.x >> 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SB_STAMP(i) do { } while (0)
#endif

template <int EPI, int STEPS /* MFMA steps (32 k each) per K slice */, int RT /* 16-row MFMA tiles per wave */, bool A16 /* A is bf16 [M][lda] */,
          bool LN /* fold LayerNorm(A; ln_g, ln_b, ln_eps) in: A fp32, STEPS = 8 or 4, one slice per wave */,
          int CT = 1 /* 16-column tiles per wave: the activation registers of a K slice feed CT weight tiles (round 5) */,
          bool WT = false /* weights from the operand-tile copy GemmArgs::W_t16 */, bool DW = false /* EPI_GLU: the depthwise-conv tail (DwTail) */,
          bool AT = false /* A16: the rows in 8-row operand tiles (GemmArgs::a_t8) */,
          bool AL = false /* fp32 rows: the wave's K slice of the rows travels global -> LDS by DMA (1 KB of consecutive addresses per instruction) */,
          bool PRE = false /* LN: another LayerNorm in front of the folded one (GemmArgs::pre_g) */>
__global__ __launch_bounds__(64 * kSbMaxWaves) void gemm_smallm_bf16_kernel(GemmArgs g, int split /* waves = K slices in flight */,
                                                                            int rvalid /* rows of a 16-row tile that exist: 16, or 8 (RT = 1) */,
                                                                            DwTail dw = DwTail{}) {
    static_assert(!DW || (EPI == EPI_GLU && RT == 1 && CT == 1), "the conv tail finishes the GLU tile of one wave");
    static_assert(!PRE || (LN && RT == 1), "the norm in front of the folded norm: one row tile per wave");
    constexpr int NW = (EPI == EPI_GLU) ? 2 : 1;                    // weight tiles per column tile (GLU: value rows [0, N), gate rows [N, 2N))
    constexpr int SL = 32 * STEPS;
    static_assert(!LN || (!A16 && (STEPS == 8 || STEPS == 4)), "the folded LayerNorm reads fp32 rows in slices of 256 (128) k");
    static_assert(!AL || (!A16 && RT == 1 && STEPS == 8), "LDS-DMA rows: fp32, one row tile, slices of 256 k (1 KB per row)");
    // AL: every wave owns 16 row slots of 1 KB + 16 B (the pad makes the operand reads conflict-free: 16 lanes of one k group read 16 rows, 65
    // 16-byte chunks apart); once the rows are in registers the slot holds the wave's partial sums.
    constexpr int APITCH = 4 * SL + 16;
    extern __shared__ __attribute__((aligned(16))) char arows[];    // AL: [kSbMaxWaves][16][APITCH] (dynamic; 0 bytes otherwise)
    __shared__ sb_f32x4 part_s[AL ? 1 : kSbMaxWaves][NW][CT][RT][64];   // partial sums [wave][weight tile][column tile][row tile][lane]
    auto part = [&](int w, int h, int c, int t) -> sb_f32x4 * {
        if constexpr (AL) return reinterpret_cast<sb_f32x4 *>(arows + (size_t)w * 16 * APITCH) + ((h * CT + c) * RT + t) * 64;
        else return &part_s[w][h][c][t][0];
    };
    __shared__ __attribute__((aligned(16))) float gam[LN ? kSbMaxWaves : 1][LN ? SL : 4], bet[LN ? kSbMaxWaves : 1][LN ? SL : 4];
    __shared__ float st1[LN ? kSbMaxWaves : 1][RT][16], st2[LN ? kSbMaxWaves : 1][RT][16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    SB_STAMP(0);
    const int r = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16 * CT, m0 = blockIdx.y * (RT == 2 ? 32 : rvalid);
    const int nslices = g.K / SL;

    // epilogue operands of the waves that will finish the output tiles (wave e < RT * CT finishes row tile e % RT of column tile e / RT):
    // requested before the weight stream
    const int et = wave % RT, ec = wave / RT;
    const int col = n0 + 16 * ec + r;
    float bias = 0.0f, bias_g = 0.0f, res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wave < RT * CT && col < g.N) {
        if (g.bias) {
            bias = g.bias[col];
            if constexpr (EPI == EPI_GLU) bias_g = g.bias[g.N + col];
        }
        if constexpr (EPI == EPI_RESID) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + 16 * et + 4 * kq + i;
                if (4 * kq + i < rvalid && row < g.M) res[i] = g.resid[(int64_t)row * g.ldr + col];
            }
        }
    }
    // conv tail: the cached rows of this lane's streams (rows m0 + 4 kq .. + 3 = 4 / c streams of c frames) and the conv's parameters of its
    // channel, requested before the weight stream like the operands above
    [[maybe_unused]] DwTailRegs tail;
    if constexpr (DW) {
        if (wave == 0 && col < g.N && 4 * kq < rvalid) tail.load(dw, g, m0, kq, col);
    }

    sb_f32x4 acc[NW][CT][RT];
#pragma unroll
    for (int h = 0; h < NW; ++h)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[h][c][t] = sb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const __bf16 *wp[NW][CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        int wrow = n0 + 16 * c + r;
        wrow = wrow < g.N ? wrow : g.N - 1;
#pragma unroll
        for (int h = 0; h < NW; ++h) {
            if constexpr (WT) wp[h][c] = reinterpret_cast<const __bf16 *>(g.W_t16) + (int64_t)((h * g.N + n0 + 16 * c) >> 4) * (g.K >> 5) * 512 + 8 * lane;   // (N % 16 == 0)
            else wp[h][c] = reinterpret_cast<const __bf16 *>(g.W) + (int64_t)(h * g.N + wrow) * g.ldw + 8 * kq;
        }
    }
    const __bf16 *ap16[RT];
    const float *ap32[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        int arow = m0 + 16 * t + (r & (rvalid - 1));                // rvalid = 8: MFMA rows 8..15 repeat rows 0..7 (never stored)
        arow = arow < g.M ? arow : g.M - 1;
        if constexpr (AT) ap16[t] = reinterpret_cast<const __bf16 *>(g.A) + (int64_t)(arow >> 3) * (g.lda >> 5) * 256 + ((arow & 7) + 8 * kq) * 8;
        else ap16[t] = reinterpret_cast<const __bf16 *>(g.A) + (int64_t)arow * g.lda + 8 * kq;
        ap32[t] = g.A + (int64_t)arow * g.lda + 8 * kq;
    }

    // (one iteration for the shapes of the streaming encoder; LN: exactly one per wave, the host launches split = K / 256 waves -- the
    //  barriers below are executed by every wave once)
    for (int sl = wave; sl < nslices; sl += split) {
        const int k0 = sl * SL;
        sb_bf16x8 w[NW][CT][STEPS], a[RT][STEPS];
        float4 af[RT][STEPS][2];
        // activations first (L2 hits: they return ahead of the weight stream that follows in the same queue)
        if constexpr (AL) {
            // one instruction per row: 64 lanes x 16 bytes = the row's 256 k of this slice, into the wave's slot of that row
            // (inline asm, and inline-asm reads below: an LDS access the compiler can see after an LDS-DMA it can see is preceded by
            //  s_waitcnt vmcnt(0) -- the whole weight stream would have to land before the LayerNorm starts.  Unknown to the compiler, the DMAs are
            //  only OLDER entries of the in-order vmcnt queue: its counted waits for the loads behind them stay sufficient.)
            const unsigned slot0 = (unsigned)(size_t)(arows + (size_t)wave * 16 * APITCH);
            auto row_dma = [&](int q) {
                int arow = m0 + q;
                arow = arow < g.M ? arow : g.M - 1;
                const float *src = g.A + (int64_t)arow * g.lda + k0 + 4 * lane;
                const unsigned dst = __builtin_amdgcn_readfirstlane(slot0 + q * APITCH);
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"                      // (m0 is a reserved register: named so that the compiler knows it changes)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(dst), "v"(src) : "memory", "m0");
#pragma clang diagnostic pop
            };
#pragma unroll
            for (int q = 0; q < 8; ++q) row_dma(q);
            if (rvalid > 8) {                                       // (kernel argument: 8 or 16)
#pragma unroll
                for (int q = 8; q < 16; ++q) row_dma(q);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                if constexpr (AL) {
                    // (read from LDS below, once the DMA has landed)
                } else if constexpr (A16) {
                    a[t][s] = *reinterpret_cast<const sb_bf16x8 *>(AT ? ap16[t] + (k0 / 32 + s) * 256 : ap16[t] + k0 + 32 * s);
                } else {
                    af[t][s][0] = *reinterpret_cast<const float4 *>(ap32[t] + k0 + 32 * s);
                    af[t][s][1] = *reinterpret_cast<const float4 *>(ap32[t] + k0 + 32 * s + 4);
                }
            }
        float4 g4 = {0.0f, 0.0f, 0.0f, 0.0f}, b4 = {0.0f, 0.0f, 0.0f, 0.0f}, pg4 = {0.0f, 0.0f, 0.0f, 0.0f}, pb4 = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (LN) {
            if (4 * lane < SL) {
                g4 = *reinterpret_cast<const float4 *>(g.ln_g + k0 + 4 * lane);
                b4 = *reinterpret_cast<const float4 *>(g.ln_b + k0 + 4 * lane);
                // the norm in front of it (GemmArgs::pre_g)
                if constexpr (PRE) {
                    pg4 = *reinterpret_cast<const float4 *>(g.pre_g + k0 + 4 * lane);
                    pb4 = *reinterpret_cast<const float4 *>(g.pre_b + k0 + 4 * lane);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < NW; ++h)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const sb_bf16x8 *src = reinterpret_cast<const sb_bf16x8 *>(WT ? wp[h][c] + (k0 / 32 + s) * 512 : wp[h][c] + k0 + 32 * s);
                    w[h][c][s] = *src;
                }
        __builtin_amdgcn_sched_barrier(0);                          // every load of the slice is issued before anything waits
        SB_STAMP(1);
        if constexpr (AL) {
            // the rows were requested first: they have landed when only the loads issued after them are outstanding (gamma / beta, the weights)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((LN ? (PRE ? 4 : 2) : 0) + NW * CT * STEPS) : "memory");
            // (inline-asm reads: left to the compiler, an LDS read after an LDS-DMA write is preceded by s_waitcnt vmcnt(0) -- the whole weight
            //  stream would have to land before the LayerNorm starts)
            const unsigned ar = (unsigned)(size_t)(arows + ((size_t)wave * 16 + (r & (rvalid - 1))) * APITCH + 32 * kq);
            sb_f32x4 lo[STEPS], hi[STEPS];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(lo[s]) : "v"(ar), "n"(128 * s));
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(hi[s]) : "v"(ar), "n"(128 * s + 16));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                asm volatile("" : "+v"(lo[s]), "+v"(hi[s]));         // (the uses stay behind the wait)
                af[0][s][0] = float4{lo[s][0], lo[s][1], lo[s][2], lo[s][3]};
                af[0][s][1] = float4{hi[s][0], hi[s][1], hi[s][2], hi[s][3]};
            }
        }

        if constexpr (LN) {
            const float inv_k = 1.0f / (float)g.K;
            float mean[RT], rstd[RT];
            // gamma / beta of this wave's slice: wave-private LDS rows, read back after the barriers of row_stats
            auto stage_gb = [&](const float4 &gv, const float4 &bv) {
                if (4 * lane < SL) {
                    *reinterpret_cast<float4 *>(&gam[wave][4 * lane]) = gv;
                    *reinterpret_cast<float4 *>(&bet[wave][4 * lane]) = bv;
                }
            };
            // statistics of the rows, two passes over the registers; the slices' partial sums meet in LDS, added in wave order (two barriers,
            // executed by every wave).  A decomposition of its own (K slices across waves), not the one-wave-per-row ln_row_stats of the fp32 kernels:
            // the specification is layer_norm of oracle/pk_oracle.c (the mean, then the mean of the squared deviations), within the mode's tolerance.
            auto row_stats = [&]() {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    float p = 0.0f;
#pragma unroll
                    for (int s = 0; s < STEPS; ++s) {
                        const float4 lo = af[t][s][0], hi = af[t][s][1];
                        p += ((lo.x + lo.y) + (lo.z + lo.w)) + ((hi.x + hi.y) + (hi.z + hi.w));
                    }
                    p += __shfl_xor(p, 16);
                    p += __shfl_xor(p, 32);
                    if (kq == 0) st1[wave][t][r] = p;
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    float sum = st1[0][t][r];
                    for (int w2 = 1; w2 < split; ++w2) sum += st1[w2][t][r];
                    mean[t] = sum * inv_k;
                    float p = 0.0f;
#pragma unroll
                    for (int s = 0; s < STEPS; ++s) {
                        const float4 lo = af[t][s][0], hi = af[t][s][1];
                        const float c0 = lo.x - mean[t], c1 = lo.y - mean[t], c2 = lo.z - mean[t], c3 = lo.w - mean[t];
                        const float c4 = hi.x - mean[t], c5 = hi.y - mean[t], c6 = hi.z - mean[t], c7 = hi.w - mean[t];
                        p += ((c0 * c0 + c1 * c1) + (c2 * c2 + c3 * c3)) + ((c4 * c4 + c5 * c5) + (c6 * c6 + c7 * c7));
                    }
                    p += __shfl_xor(p, 16);
                    p += __shfl_xor(p, 32);
                    if (kq == 0) st2[wave][t][r] = p;
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    float sum = st2[0][t][r];
                    for (int w2 = 1; w2 < split; ++w2) sum += st2[w2][t][r];
                    rstd[t] = 1.0f / sqrtf(sum * inv_k + g.ln_eps);
                }
            };
            if constexpr (PRE) {
                // A norm in front of the folded one (a block's final_norm_ in front of the next block's first: GemmArgs::pre_g): the rows are
                // normalised in place (fp32) -- and written out, one k-step of every slice by each of the first STEPS column tiles: they are the
                // residual stream from here on
                stage_gb(pg4, pb4);
                row_stats();
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const float4 gl = *reinterpret_cast<const float4 *>(&gam[wave][32 * s + 8 * kq]), gh = *reinterpret_cast<const float4 *>(&gam[wave][32 * s + 8 * kq + 4]);
                    const float4 bl = *reinterpret_cast<const float4 *>(&bet[wave][32 * s + 8 * kq]), bh = *reinterpret_cast<const float4 *>(&bet[wave][32 * s + 8 * kq + 4]);
#pragma unroll
                    for (int t = 0; t < RT; ++t) {
                        const float4 lo = af[t][s][0], hi = af[t][s][1];
                        const float m = mean[t], rs = rstd[t];
                        const float4 ylo = {fmaf((lo.x - m) * rs, gl.x, bl.x), fmaf((lo.y - m) * rs, gl.y, bl.y), fmaf((lo.z - m) * rs, gl.z, bl.z), fmaf((lo.w - m) * rs, gl.w, bl.w)};
                        const float4 yhi = {fmaf((hi.x - m) * rs, gh.x, bh.x), fmaf((hi.y - m) * rs, gh.y, bh.y), fmaf((hi.z - m) * rs, gh.z, bh.z), fmaf((hi.w - m) * rs, gh.w, bh.w)};
                        af[t][s][0] = ylo; af[t][s][1] = yhi;
                        const int row = m0 + 16 * t + r;
                        if ((int)blockIdx.x == s && g.pre_out && r < rvalid && row < g.M) {   // (column tile s writes k-step s of every slice: gridDim.x >= STEPS)
                            float *dst = g.pre_out + (int64_t)row * g.pre_ldo + k0 + 32 * s + 8 * kq;
                            *reinterpret_cast<float4 *>(dst) = ylo;
                            *reinterpret_cast<float4 *>(dst + 4) = yhi;
                        }
                    }
                }
            }
            stage_gb(g4, b4);                                       // (wave-private rows, LDS operations of a wave complete in order)
            row_stats();
            SB_STAMP(2);
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const float4 gl = *reinterpret_cast<const float4 *>(&gam[wave][32 * s + 8 * kq]), gh = *reinterpret_cast<const float4 *>(&gam[wave][32 * s + 8 * kq + 4]);
                const float4 bl = *reinterpret_cast<const float4 *>(&bet[wave][32 * s + 8 * kq]), bh = *reinterpret_cast<const float4 *>(&bet[wave][32 * s + 8 * kq + 4]);
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const float4 lo = af[t][s][0], hi = af[t][s][1];
                    const float m = mean[t], rs = rstd[t];
                    sb_bf16x8 v;                                    // y = fma((x - mean) * rstd, gamma, beta), rounded to bf16 (RNE)
                    v[0] = (__bf16)fmaf((lo.x - m) * rs, gl.x, bl.x); v[1] = (__bf16)fmaf((lo.y - m) * rs, gl.y, bl.y);
                    v[2] = (__bf16)fmaf((lo.z - m) * rs, gl.z, bl.z); v[3] = (__bf16)fmaf((lo.w - m) * rs, gl.w, bl.w);
                    v[4] = (__bf16)fmaf((hi.x - m) * rs, gh.x, bh.x); v[5] = (__bf16)fmaf((hi.y - m) * rs, gh.y, bh.y);
                    v[6] = (__bf16)fmaf((hi.z - m) * rs, gh.z, bh.z); v[7] = (__bf16)fmaf((hi.w - m) * rs, gh.w, bh.w);
                    a[t][s] = v;
                }
            }
        } else if constexpr (!A16) {
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const float4 lo = af[t][s][0], hi = af[t][s][1];
                    sb_bf16x8 v;
                    v[0] = (__bf16)lo.x; v[1] = (__bf16)lo.y; v[2] = (__bf16)lo.z; v[3] = (__bf16)lo.w;
                    v[4] = (__bf16)hi.x; v[5] = (__bf16)hi.y; v[6] = (__bf16)hi.z; v[7] = (__bf16)hi.w;
                    a[t][s] = v;
                }
        }
        SB_STAMP(3);
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int h = 0; h < NW; ++h)
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[h][c][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][s], w[h][c][s], acc[h][c][t], 0, 0, 0);
    }

    SB_STAMP(4);
    // the K slices meet: partial sums through LDS, added in wave order
    if (split > 1) {
#pragma unroll
        for (int h = 0; h < NW; ++h)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int t = 0; t < RT; ++t) part(wave, h, c, t)[lane] = acc[h][c][t];
        __syncthreads();
    }
    SB_STAMP(5);
    if (wave >= RT * CT) return;                                    // (launched with split >= RT * CT whenever RT * CT > 1)
    const int t = et;                                               // this wave finishes row tile et of column tile ec
    sb_f32x4 v = acc[0][0][0], gt = acc[NW - 1][0][0];              // (split == 1: RT = CT = 1)
    if (split > 1) {
        v = part(0, 0, ec, t)[lane];
        for (int w2 = 1; w2 < split; ++w2) v += part(w2, 0, ec, t)[lane];
        if constexpr (EPI == EPI_GLU) {
            gt = part(0, 1, ec, t)[lane];
            for (int w2 = 1; w2 < split; ++w2) gt += part(w2, 1, ec, t)[lane];
        }
    }
    if (col >= g.N) return;
    [[maybe_unused]] float glu[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // C/D layout of 16x16: column = lane & 15, row = 4 * (lane >> 4) + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + 16 * t + 4 * kq + i;
        if (4 * kq + i >= rvalid || row >= g.M) continue;
        const float o = epi_finish<EPI>(v[i], g.bias != nullptr, bias, gt[i], bias_g, res[i], g.alpha, g.fast_act != 0);
        if constexpr (DW) { glu[i] = o; continue; }
        if (g.out_t8) reinterpret_cast<__bf16 *>(g.out)[((int64_t)(row >> 3) * (g.ldo >> 5) + (col >> 5)) * 256 + ((row & 7) + 8 * ((col & 31) >> 3)) * 8 + (col & 7)] = (__bf16)o;
        else if (g.out_bf16) reinterpret_cast<__bf16 *>(g.out)[(int64_t)row * g.ldo + col] = (__bf16)o;
        else g.out[(int64_t)row * g.ldo + col] = o;
    }
    if constexpr (DW) {
        // depthwise conv over [cached 8 rows ; the c new GLU rows] of (stream, channel), BatchNorm, SiLU; the last 8 rows of the concatenation
        // are the stream's cache for the next chunk (DwTailRegs, gemm_epi.hpp)
        if (4 * kq >= rvalid) return;
        tail.finish(dw, g, m0, kq, col, glu);
    }
    SB_STAMP(6);
}

// the shapes this kernel takes (everything else stays on the tile kernels of gemm_bf16.hpp)
bool gemm_smallm_bf16_applies(const GemmArgs &a, int epi) {
    if (a.M > kSmallMRowsBf16 || a.M <= 0 || a.K % 256 != 0 || a.remap_rows != 0 || a.sigma_cols != 0 || a.one_form) return false;
    if ((a.ldw % 8) != 0 || (a.lda % (a.a_bf16 ? 8 : 4)) != 0) return false;
    if (a.out_bf16 && (epi == EPI_RESID || epi == EPI_GLU)) return false;
    if (a.out_t8 && !(a.out_bf16 && a.M % 8 == 0 && a.N % 32 == 0 && a.ldo == a.N)) return false;
    if (a.a_t8 && !(a.a_bf16 && a.M % 8 == 0 && a.lda == a.K && epi == EPI_RESID)) return false;   // (instantiated for the product that takes them: fc2)
    return epi >= EPI_NONE && epi <= EPI_GLU;
}
bool gemm_smallm_bf16_pre_applies(const GemmArgs &a, int epi) {
    if (epi != EPI_SILU || !a.pre_g || !a.pre_b || a.K / 256 > kSbMaxWaves || a.K % 256 != 0 || a.N < 256) return false;   // (>= 8 column tiles share the write-out)
    if (a.pre_out && (a.pre_out == a.A || a.pre_ldo < a.K || (a.pre_ldo % 4) != 0)) return false;
    return gemm_smallm_bf16_ln_applies(a, epi);
}
bool gemm_smallm_bf16_dw_applies(const GemmArgs &a, int epi, int c, int kc) {
    if (epi != EPI_GLU || !stream_dwconv_tail_fusable(c, kc) || a.M % c != 0 || a.N % 16 != 0 || a.out_bf16) return false;
    return a.ln_g ? gemm_smallm_bf16_ln_applies(a, epi) : gemm_smallm_bf16_applies(a, epi);
}
bool gemm_smallm_bf16_ln_applies(const GemmArgs &a, int epi) {
    if (!a.ln_g || !a.ln_b || a.a_bf16) return false;
    if (!gemm_smallm_bf16_applies(a, epi)) return false;
    if (epi == EPI_GLU && a.K / 256 > 4) return false;              // GLU + folded LayerNorm: two weight tiles, fp32 AND bf16 rows per wave -- 4 slices (K <= 1024)
    return a.K / 256 <= kSbMaxWaves;                                // one slice of 256 k per wave
}

// rows per workgroup: the LARGEST of 32 (two MFMA row tiles per wave) / 16 / 8 that still gives (nearly) every CU a workgroup -- the bytes
// all workgroups pull together are tiles * ceil(M / R) * 2 K (R + 16), least for the largest R, but a product costs what its busiest CU pulls
// (header).  RT = 2 needs two waves to finish its two row tiles.  `tiles` = workgroups along N (column tiles / CT).
static int sb_rows_per_wg(const GemmArgs &a, int nslices, bool glu, int tiles) {
    // (GLU keeps one row tile per wave: two weight tiles AND two row tiles of fp32 rows do not fit 256 registers)
    if (!glu && a.M > 16 && nslices >= 2 && tiles * ((a.M + 31) / 32) >= 192) return 32;
    if (a.M > 8 && tiles * ((a.M + 15) / 16) >= 192) return 16;
    return 8;
}

// Launch forms measured and not kept (up to 4fb176f selected in EXPERIMENTAL builds by PK_SB_CT / PK_SB_NT / PK_SB_ROWS / PK_SB_WT / PK_SB_AL):
// forced column tiles per wave or rows per workgroup, non-temporal weight loads, the weights in their natural layout where the operand-tile copy
// exists, and fp32 rows by per-lane loads instead of LDS-DMA.

// Which instantiation a product takes, and with how many rows of a tile (kernels.hpp: GemmSmallmBf16Form).  launch_gemm_smallm_bf16 switches on this
// function's result and pk_diag_gemm_smallm_bf16 reports it: every threshold of the family lives here and nowhere else.
GemmSmallmBf16Form gemm_smallm_bf16_form(const GemmArgs &a, int epi) {
    const bool glu = epi == EPI_GLU;
    const bool ln = a.ln_g != nullptr;                              // LayerNorm folded in (the caller checked gemm_smallm_bf16_ln_applies): fp32 rows
    const bool a16 = !ln && a.a_bf16;
    // bf16 rows: 4 registers per MFMA operand -- slices of 512 k where 256 would leave more than kSbMaxWaves of them (fc2 of the 600M models:
    // K = 4096); not for GLU (two weight tiles per wave)
    const int steps = (a16 && !glu && a.K % 512 == 0 && a.K / 256 > kSbMaxWaves) ? 16 : 8;
    const bool wt = a.W_t16 && a.N % 16 == 0;
    const int nslices = a.K / (32 * steps);
    const int split = nslices < kSbMaxWaves ? nslices : kSbMaxWaves;
    const int tiles1 = (a.N + 15) / 16;
    int R = sb_rows_per_wg(a, nslices, glu, tiles1), ct = 1;
    // Two column tiles per wave (the activation registers of a K slice feed both) where that lowers what the busiest CU pulls: fp32 rows (4 bytes
    // per k and row against 2 per k and column) of products wide enough to keep every CU busy with 16 rows x 32 columns per workgroup -- fc1 and
    // qkv of the 600M models: K (16 * 4 + 32 * 2) = 128 KB per CU instead of K (32 * 4 + 16 * 2) = 160 KB.
    if (!a16 && !glu && R == 32 && split >= 2 && a.N % 32 == 0 && (tiles1 / 2) * ((a.M + 15) / 16) >= 192) { ct = 2; R = 16; }
    if (R == 32 && (glu || split < 2 || a.pre_g)) R = 16;           // two row tiles per wave: a wave per output tile; not in front of a second norm
    const int rt = R == 32 ? 2 : 1, rvalid = rt == 2 ? 16 : R;
    const bool at = epi == EPI_RESID && a16 && a.a_t8;              // (instantiated for the product that takes them: fc2)
    // a norm in front of the folded one (GemmArgs::pre_g; the caller checked gemm_smallm_bf16_pre_applies): fc1 of a streaming block
    const bool pre = rt == 1 && ln && epi == EPI_SILU && a.pre_g;
    const bool dw = rt == 1 && glu && a.dw_tail;
    // fp32 rows of one row tile: the wave's slice of the rows by LDS-DMA (template AL), with the operand-tiled weights
    const bool al = rt == 1 && !a16 && wt;
    return gemm_smallm_bf16_form_of(epi, steps, rt, rvalid, a16, ln, ct, wt, dw, at, al, pre);
}

// one instantiation: F = a form with its rvalid field cleared (the rows of a tile that exist are a kernel argument)
template <int F>
static void launch_sb_inst(const GemmArgs &a, hipStream_t s, int rvalid) {
    constexpr int EPI = gemm_smallm_bf16_form_epi(F), STEPS = gemm_smallm_bf16_form_steps(F), RT = gemm_smallm_bf16_form_rt(F), CT = gemm_smallm_bf16_form_ct(F);
    constexpr bool A16 = gemm_smallm_bf16_form_a16(F), LN = gemm_smallm_bf16_form_ln(F), WT = gemm_smallm_bf16_form_wt(F), DW = gemm_smallm_bf16_form_dw(F);
    constexpr bool AT = gemm_smallm_bf16_form_at(F), AL = gemm_smallm_bf16_form_al(F), PRE = gemm_smallm_bf16_form_pre(F);
    const int nslices = a.K / (32 * STEPS);
    const int split = nslices < kSbMaxWaves ? nslices : kSbMaxWaves;
    const int tiles = (a.N + 16 * CT - 1) / (16 * CT), R = RT == 2 ? 32 : rvalid;
    const dim3 grid(tiles, (a.M + R - 1) / R), block(64 * split);
    constexpr size_t lds = AL ? (size_t)kSbMaxWaves * 16 * (4 * 32 * STEPS + 16) : 0;
    if constexpr (AL) {
        static DynLdsSlots slots;                                   // (one per instantiation)
        ensure_dyn_lds(slots, reinterpret_cast<const void *>(&gemm_smallm_bf16_kernel<EPI, STEPS, RT, A16, LN, CT, WT, DW, AT, AL, PRE>), lds);
    }
    hipLaunchKernelGGL((gemm_smallm_bf16_kernel<EPI, STEPS, RT, A16, LN, CT, WT, DW, AT, AL, PRE>), grid, block, lds, s, a, split, rvalid, DW ? *a.dw_tail : DwTail{});
}
// the instantiations: the forms with their rvalid field cleared, each once (two forms that differ in the rows of a tile in use share a kernel)
constexpr int kSbRvalidBit = gemm_smallm_bf16_form_of(0, 8, 1, 16, false, false, 1, false, false, false, false, false);
struct SbInsts { int v[kGemmSmallmBf16FormCount]; int n; };
constexpr SbInsts sb_insts() {
    SbInsts t{};
    for (int i = 0; i < kGemmSmallmBf16Forms.n; ++i) {
        const int key = (int)kGemmSmallmBf16Forms.v[i] & ~kSbRvalidBit;
        bool seen = false;
        for (int j = 0; j < t.n; ++j) seen = seen || t.v[j] == key;
        if (!seen) t.v[t.n++] = key;
    }
    return t;
}
constexpr SbInsts kSbInsts = sb_insts();
static_assert(kSbInsts.n == 104, "the instantiations of gemm_smallm_bf16_kernel the launcher can take");
// launches the instantiation of `form`; false: the table has none (the form's rvalid goes to the kernel as an argument)
template <size_t... I>
static bool launch_sb_form(int form, const GemmArgs &a, hipStream_t s, std::index_sequence<I...>) {
    const int key = form & ~kSbRvalidBit, rvalid = gemm_smallm_bf16_form_rvalid(form);
    return ((key == kSbInsts.v[I] ? (launch_sb_inst<kSbInsts.v[I]>(a, s, rvalid), true) : false) || ...);
}
// W16 [rows][ld] (bf16) -> the operand tiles of GemmArgs::W_t16: per (16 rows, 32 k) one KB [lane = (row & 15) + 16 * (k / 8 & 3)][8 bf16]
__global__ __launch_bounds__(256) void tile_copy_bf16_kernel(const uint4 *src, uint4 *dst, int64_t n_chunks, int ksteps, int64_t ld8 /* ld / 8 */) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one 16-byte chunk (8 bf16) each
    if (i >= n_chunks) return;
    const int lane = (int)(i & 63);
    const int64_t ts = i >> 6, tile = ts / ksteps;
    const int st = (int)(ts - tile * ksteps);
    dst[i] = src[(tile * 16 + (lane & 15)) * ld8 + 4 * st + (lane >> 4)];
}
void launch_tile_copy_bf16(const float *src16, float *dst16, int64_t rows, int K, int64_t ld, hipStream_t s) {
    const int64_t n = rows * K / 8;
    hipLaunchKernelGGL(tile_copy_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(src16),
                       reinterpret_cast<uint4 *>(dst16), n, K / 32, ld / 8);
}

GemmSmallmBf16Form launch_gemm_smallm_bf16(const GemmArgs &a, int epi, hipStream_t s) {
    const int form = gemm_smallm_bf16_form(a, epi);
    if (epi < EPI_NONE || epi > EPI_GLU || !launch_sb_form(form, a, s, std::make_index_sequence<kSbInsts.n>{})) {
        fprintf(stderr, "parakeet_amd: internal error: launch_gemm_smallm_bf16 has no kernel for form %d\n", form);
        abort();
    }
    return (GemmSmallmBf16Form)form;
}

}  // namespace pk
