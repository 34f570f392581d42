// parakeet.cpp_amd/csrc/kernels/kernels.hpp -- host-side launchers of the gfx950 kernels.
// Every launcher enqueues on `s` and returns; none allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

namespace pk {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE setting and the launchers run on one host thread per device in a
// pk_group: the largest size set so far is kept per (launcher, device).  `slots` is the launcher's own static array.
constexpr int kMaxDevices = 16;
struct DynLdsSlots { std::atomic<size_t> set[kMaxDevices]; };
inline void ensure_dyn_lds(DynLdsSlots &slots, const void *kernel, size_t bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) {          // no slot for this device: set the attribute every time, never alias another device's slot
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        return;
    }
    std::atomic<size_t> &cur = slots.set[dev];
    if (bytes > cur.load(std::memory_order_acquire)) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        cur.store(bytes, std::memory_order_release);
    }
}

// ---- ragged (mixed-length, packed) batches -------------------------------------------------------------------------------------
// The reference's roadmap "batch inference: pad + length-mask" (README.md:513) done WITHOUT padding: utterance b of a packed tensor owns
// rows [off[b], off[b] + n[b]) -- GEMMs, LayerNorm and their epilogues are row-wise and never notice; kernels that look across rows (mel
// framing, the 3x3 / depthwise convolutions, attention, the greedy decoders) take the per-utterance extents below, so every utterance sees
// exactly the zero padding, position table and softmax extent of a single-clip run: bit-identical per clip.  A null pointer in the first
// member = uniform batch (the launchers' plain B / T arguments apply).
struct RagUnit { int b, r0; };                 // one strip of rows of ONE utterance: utterance b, first local row r0
struct RagUnits { const RagUnit *u = nullptr; int count = 0; };
struct MelRag { const int64_t *pcm_off = nullptr; const int *Tm = nullptr, *Tm_off = nullptr; int max_frames = 0;   // [B+1] samples, [B] mel frames, [B+1]
                const int *Tm_pad_off = nullptr; };   // [B+1] prefix sums of mel_logmel_pitch(Tm[b]): where clip b's log-mel block starts (in frames)
struct SubRag {                                 // conv subsampling: mel frames -> H2 = rows after conv1 / dw1 -> T rows after dw2
    RagUnits strips;                            // conv1_dw1: strips of strip_rows rows of H2 ; dw2: one unit per output row
    int strip_rows = 0;
    const int *Tm = nullptr, *Tm_off = nullptr, *H2 = nullptr, *H2_off = nullptr, *T = nullptr, *T_off = nullptr;
};
struct SeqRag {                                 // encoder frames: attention row blocks (32 rows) / depthwise-conv strips / decoders
    RagUnits units;
    const int *T = nullptr, *T_off = nullptr;  // [B], [B+1]
    int T_max = 0;                              // longest utterance of the batch (LDS sizing)
    int pos_T = 0;                              // the position table was built for pos_T >= T_max frames: utterance b reads it from row pos_T - T[b]
};

// ---- mel front end (src/audio.cpp:100-158) ----------------------------------------------------
constexpr int kMelMaxTaps = 768;      // packed filterbank taps staged in LDS by the mel kernel (sum of the band widths; 80 / 128 bins: ~590)
struct MelTables {
    const float *window;   // [512] symmetric Hann(400) zero-padded to n_fft, placed per switch A1 (pk_config.stft_window_centered)
    const float *window_left;  // [512] the same window left-aligned: the streaming preprocessor's frames (center=false)
    const float *tw_re;    // [256] cos(2 pi k / 512)
    const float *tw_im;    // [256] -sin(2 pi k / 512)
    const float *fb;       // [257][n_mels] Slaney filterbank (src/audio.cpp:40-94)
    const int *f_lo;       // [n_mels] first / last non-zero fft bin of each filter
    const int *f_hi;
    const float *fbc;      // the non-zero band of every filter, packed: fbc[fb_off[m] + f - f_lo[m]] = fb[f][m]
    const int *fb_off;     // [n_mels + 1]
    int fb_nnz;            // fb_off[n_mels] (<= kMelMaxTaps)
    int n_mels;
    int power_via_abs;     // switch A2
};
// rag set: clip b = pcm[rag.pcm_off[b] .. rag.pcm_off[b+1]), its log-mel [n_mels][pitch of rag.Tm[b]] at logmel + n_mels * rag.Tm_pad_off[b] (n_samples / n_frames ignored)
// The log-mel intermediate is [clip][n_mels][pitch], pitch = mel_logmel_pitch(n_frames) = n_frames rounded up to 16: every run of 16 frames a
// workgroup stores is then one aligned 64-byte segment (the un-padded rows -- 1001 floats for 10 s -- put every run across sector boundaries:
// 1.44x write traffic).  Only mel_normalize (and the debug read-outs of pk_mel) read it.
__host__ __device__ inline int mel_logmel_pitch(int n_frames) { return (n_frames + 15) & ~15; }
// Each launcher returns the grid it launched (x, y, threads per workgroup): what pk_diag_mel reports.
struct MelGrid { int x, y, threads; };
MelGrid launch_mel_logmel(const float *pcm, int B, int64_t n_samples, int n_frames, const MelTables &t, float *logmel, hipStream_t s, const MelRag &rag = MelRag());
// StreamingAudioPreprocessor::process_chunk (src/audio.cpp:222-252) on pre-emphasised buffers pre[B][n_samples]:
// n_frames = (n_samples - 400) / 160 + 1 frames -> log-mel [B][n_frames][n_mels] (no normalisation)
MelGrid launch_mel_stream(const float *pre, int B, int64_t n_samples, int n_frames, const MelTables &t, float *logmel_tf, hipStream_t s);
MelGrid launch_mel_normalize(const float *logmel, int B, int n_mels, int n_frames, int normalize, float *feats, hipStream_t s, const MelRag &rag = MelRag());

// ---- fp32 MFMA GEMM: out = epi(A[M][K] * W[N][K]^T + bias), natural-k fma chains ----------------
enum GemmEpi { EPI_NONE = 0, EPI_RELU = 1, EPI_SILU = 2, EPI_RESID = 3, EPI_GLU = 4 };
// Streaming conv module: the causal depthwise conv (kernel 9) + BatchNorm + SiLU of
// CausalConformerConvModule::forward_cached (src/streaming_encoder.cpp:41-78) run in the GLU epilogue of pw1 (tolerance-class mode:
// gemm_smallm_bf16.hip; exact mode: gemm_smallm_ln_kernel of gemm_smallm.hip): the lane that
// finishes column ch of a stream's c new frames holds everything the conv of (stream, ch) needs next to the stream's cached 8 frames -- no
// exchange, one launch less per block.  Rows of the product = [S][c] stream-major; GemmArgs::out receives the conv module's activations
// (the GLU values themselves are not stored).  Both tails (gemm_epi.hpp: DwTailRegs) call the dwconv_point that stream_dwconv_kernel calls.
struct DwTail {
    const float *cache_in = nullptr; float *cache_out = nullptr;     // [S][8][d]: the last 8 GLU rows of every stream before / after this chunk
    int has_cache = 0, c = 0;                                        // first chunk: zero left padding; c = new frames per stream (1, 2 or 4)
    const float *w = nullptr /* [9][d] */, *bias = nullptr, *bn_mean = nullptr, *bn_rstd = nullptr, *bn_g = nullptr, *bn_b = nullptr;
    int out_sigma = 0;                                               // the activations' columns in the sigma layout (exact mode: pw2 reads a_sigma rows)
};

struct GemmArgs {
    const float *A; int64_t lda;
    const float *W; int64_t ldw;
    const float *bias;          // [N] (GLU: [2N]) or nullptr
    float *out; int64_t ldo;
    const float *resid; int64_t ldr; float alpha;   // EPI_RESID: out = resid + alpha * (acc + bias)
    int M, N, K;                // N = output width (GLU: W has 2N rows, a-part rows [0,N), gate rows [N,2N))
    // optional output re-mapping (0 = off): offset = (row / remap_rows) * remap_gs + (row % remap_rows) * remap_rs + col * remap_cs
    // (used to write the last subsampling conv straight into the permute(0,2,1,3)+reshape layout, src/encoder.cpp:235-238)
    int remap_rows = 0; int64_t remap_gs = 0, remap_rs = 0, remap_cs = 0;
    // output columns < sigma_cols (a multiple of 16) are written in the "sigma" layout: inside every block of 16 columns the
    // 4x4 index matrix is transposed (col -> (col & ~15) | ((col & 3) << 2) | ((col >> 2) & 3)).  The attention kernel reads
    // Q, K and the projected position table that way: a lane's float4 then holds its operands of 4 consecutive MFMA steps.
    int sigma_cols = 0;
    // bf16 mode (launch_gemm_bf16 / gemm_bf16.hpp) only: A points to bf16 activations [M][lda] the producer already rounded (RNE, the
    // rounding the staging path would apply -- same operand values, half the bytes); out points to a bf16 buffer [M][ldo] (the next
    // product's A operand; row-major wide outputs only).
    int a_bf16 = 0, out_bf16 = 0;
    // bf16 mode, direct-to-LDS kernels (gemm_bf16_glds.hpp) only: the bf16 activation tensor between a producer's register epilogue and the
    // next product's LDS-DMA lives in BLOCKS of 32 rows x 16 columns (1 KB, row-major inside; blocks ordered [row / 32][col / 16]): one store
    // instruction of the producer's epilogue (32 rows x 2 x 16 bytes) then writes ONE contiguous KB instead of 32 row slivers of 32 bytes,
    // and the consumer's DMA (which gathers 16-byte chunks by per-lane address anyway) reads it in 256-byte runs.  out_blocked: `out` is
    // written that way (ldo = the row length in elements, a multiple of 16; rows padded to a multiple of 32 by the allocation);
    // a_blocked: `A` is read that way (lda = its row length).  Set by the engine for fc1 -> fc2 when gemm_bf16_blocked_handoff() says both take
    // those kernels.
    int out_blocked = 0, a_blocked = 0;
    // small-M bf16 kernel only (gemm_smallm_bf16.hip): the bf16 activation rows between two of its products (fc1 -> fc2 of a streaming chunk) in
    // OPERAND TILES of 8 rows: per (8 rows, 32 k) 512 bytes [lane32 = (row & 7) + 8 * (k / 8 & 3)][8 bf16], tiles ordered [rows / 8][K / 32] -- the
    // consumer's load instruction reads whole lines (512 B, or two runs of 512 B for 16 rows) instead of 8 / 16 row segments of 64 bytes.
    // M % 8 == 0, row length % 32 == 0.  out_t8: `out` is written that way (ldo = the row length), a_t8: `A` is read that way (lda = the row length).
    int out_t8 = 0, a_t8 = 0;
    // bf16 mode only: SiLU / sigmoid of the epilogue on the hardware exp2 / rcp (1 ulp) instead of the fixed polynomial + IEEE division of the
    // numerics contract -- that mode is compared with the oracle within a bf16-epsilon-class tolerance, not bit for bit, and at bf16 MFMA rates
    // the 38-operation SiLU is as expensive as the product itself (fc1 of tdt-600m: ~48 us of VALU against 40 us of MFMA).
    int fast_act = 0;
    // bf16 mode only: the product runs on ONE kernel form whatever M is -- never the small-M bf16 kernel (with K > 256 it splits K over its waves and adds
    // the partial sums afterwards: not the fp32 sum the tile kernels form), always the register-staged 64 x 64 tile -- so that a row of the output has the
    // same bits at every M.  Set for products whose rows are read again under another M: the relative-position tables (Model::ensure_pos_tables), built
    // once for the longest sequence and read by windows.  Not for the hot path: the form is not the fastest one for most shapes.  (EPI_GLU: ignored.)
    int one_form = 0;
    // small-M kernel (gemm_smallm.hip, M <= kSmallMRows) only: W_sig = a copy of W (launch_sigma_copy; N % 16 == 0, K % 64 == 0) tiled in the kernel's load
    // order -- per (16-row tile, 64-k chunk) one 4 KB block [q][lane][4] with the K axis in the sigma layout; a_sigma = A's K axis is in the sigma
    // layout (its producer wrote it that way: sigma_cols, LayerNorm mode 2, the streaming attention / conv kernels).  Both set: a lane's 16-byte
    // load IS its operand of four consecutive MFMA steps -- no transposes on the chain -- and every weight load is 1 KB of consecutive addresses.
    const float *W_sig = nullptr; int a_sigma = 0;
    // small-M bf16 kernel (gemm_smallm_bf16.hip) only: a copy of the bf16 weights in the kernel's OPERAND TILES (launch_tile_copy_bf16: per
    // (16 rows, 32 k) one KB in lane order, tiles [rows / 16][K / 32]; rows % 16 == 0, K % 32 == 0) -- every weight load instruction reads one
    // contiguous KB.  W stays set (the natural layout: every other kernel reads that).
    const float *W_t16 = nullptr;
    // small-M kernels only (gemm_smallm_bf16.hip; gemm_smallm.hip with W_sig): A = the UN-normalised fp32 rows, the LayerNorm (gamma ln_g[K], beta
    // ln_b[K], ln_eps) of the product's input is applied while the rows are staged -- out = epi(LN(A) W^T + bias) (bf16 mode: bf16(LN(A)) W16^T).
    // Callers check gemm_smallm_bf16_ln_applies() / gemm_smallm_ln_applies().
    const float *ln_g = nullptr, *ln_b = nullptr; float ln_eps = 0.0f;
    // Tile kernel of the fp32 path (gemm_pipe.hpp, LNA; round 6): with ln_g / ln_b set, ln_stats = {mean, rstd} of every row of A (launch_layernorm_stats) and
    // the normalisation y = fma((x - mean) * rstd, gamma, beta) is applied while the A tile is staged -- bit for bit the rows launch_layernorm would have
    // written.  Callers check gemm_ln_stats_applies().
    const float *ln_stats = nullptr;
    // small-M kernels with ln_g set (gemm_smallm_bf16.hip; exact mode: gemm_smallm_ln_kernel, bit for bit the separate launch): ANOTHER LayerNorm in front of the folded one -- out = epi(bf16(LN(LN(A; pre_g, pre_b); ln_g, ln_b)) W16^T + bias):
    // a block's final_norm_ folded into the first product of the next block (streaming, tolerance-class mode: one launch less per block).  pre_out
    // (optional, fp32 [M][pre_ldo], NOT the buffer A lives in: other workgroups still read A) receives LN(A; pre_g, pre_b) -- the residual stream
    // of the block that starts here -- written by the first few column tiles, one k-step (chunk) of every row each.
    const float *pre_g = nullptr, *pre_b = nullptr; float *pre_out = nullptr; int64_t pre_ldo = 0;
    // small-M kernels with the LayerNorm folded in (exact mode) / small-M bf16 kernel, EPI_GLU only: HOST pointer to the depthwise-conv tail of
    // the epilogue (read during the launch call).  Callers check gemm_smallm_dw_applies() / gemm_smallm_bf16_dw_applies().
    const DwTail *dw_tail = nullptr;
};
constexpr int kSmallMRows = 1536;  // launch_gemm: products with M <= this (and K % 64 == 0) run on gemm_smallm.hip.  Measured with the two-row-tile
                                   // variant in place (110m encoder; reference protocol, batch 1: M = 626 5.6 ms on it vs 6.7 on the tile kernels,
                                   // M = 751 6.1 vs 6.9, M = 1251 12.4 vs 15.1; pipelined batches of 8 / 12 / 16 clips, M = 1008 / 1512 / 2016:
                                   // 6.75 vs 6.50, 9.14 vs 10.67, 11.35 vs 10.93 ms per step)
// src [rows][ld] -> dst rows x K floats in the W_sig tiling (rows % 16 == 0, K % 64 == 0)
void launch_sigma_copy(const float *src, float *dst, int64_t rows, int K, int64_t ld, hipStream_t s);
// bf16 src [rows][ld] -> dst rows x K bf16 in the W_t16 operand tiles (rows % 16 == 0, K % 32 == 0, ld % 8 == 0)
void launch_tile_copy_bf16(const float *src16, float *dst16, int64_t rows, int K, int64_t ld, hipStream_t s);
void launch_gemm(const GemmArgs &a, int epi, hipStream_t s);
// fp32 tile kernel with the LayerNorm of its input rows applied from per-row statistics (GemmArgs::ln_stats): large batches (M > kSmallMRows), K = the row
// length (a multiple of 32), wide outputs (the 128 x 128 single-buffered tile: fc1, qkv, pw1 + GLU), epilogues none / ReLU / SiLU / GLU
bool gemm_ln_stats_applies(const GemmArgs &a, int epi);
// bf16 mode: true when the product (M x N x K, bf16 A already in HBM, epilogue `epi`) runs on a direct-to-LDS kernel that can write
// (producer = true: register epilogue) / read (producer = false: LDS-DMA) the blocked activation layout of GemmArgs::out_blocked / a_blocked
bool gemm_bf16_blocked_handoff(int M, int N, int K, int epi, bool producer);
// fp32 small-M chain kernel with GemmArgs::ln_g set (kernels/gemm_smallm.hip: gemm_smallm_ln_kernel): A = the un-normalised rows, K = 512 / 1024 = the
// row length, tiled weights W_sig, epi none / relu / silu / glu -- bit for bit LayerNorm + product.  Callers check this first.
bool gemm_smallm_ln_applies(const GemmArgs &a, int epi);
bool gemm_smallm_pre_applies(const GemmArgs &a, int epi);                      // ... with GemmArgs::pre_g (a second norm in front, bit for bit the separate LayerNorm launch)
bool gemm_smallm_dw_applies(const GemmArgs &a, int epi, int c, int kc);        // ... with GemmArgs::dw_tail (GLU, conv kernel 9, c = 1 / 2 / 4 frames per stream)
// The form of a small-M launch (kernels/gemm_smallm.hip), by the function launch_gemm_smallm switches on: value = gemm_smallm_form_of(...).
//   kernel: gemm_smallm_kernel (one wave per 16 x 16 tile), gemm_smallm_rt2_kernel (two row tiles per wave), gemm_smallm_ln_kernel (LayerNorm folded in)
//   epi:    the epilogue the kernel is instantiated for (GemmEpi)
//   ring:   chain: DEPTH, the chunks of 64 k in the register ring -- 8 / 2 / 1 by K / 64; rt2: its fixed 4; ln: PER_LANE = K / 64, 8 or 16
//   sig:    the operands in the sigma K order, the weights tiled (a_sigma + W_sig; ln: W_sig only, the kernel writes the sigma rows itself)
//   dw:     ln + GLU with GemmArgs::dw_tail;  pre: ln + SiLU with GemmArgs::pre_g
enum GemmSmallmKernel { SMALLM_CHAIN = 0, SMALLM_RT2 = 1, SMALLM_LN = 2 };
enum GemmSmallmForm : int {};
constexpr GemmSmallmForm gemm_smallm_form_of(int kernel, int epi, int ring, bool sig, bool dw = false, bool pre = false) {
    return (GemmSmallmForm)(kernel * 4096 + epi * 512 + ring * 8 + (sig ? 4 : 0) + (dw ? 2 : 0) + (pre ? 1 : 0));
}
constexpr int gemm_smallm_form_kernel(int f) { return f >> 12; }
constexpr int gemm_smallm_form_epi(int f) { return (f >> 9) & 7; }
constexpr int gemm_smallm_form_ring(int f) { return (f >> 3) & 63; }
constexpr bool gemm_smallm_form_sig(int f) { return (f & 4) != 0; }
constexpr bool gemm_smallm_form_dw(int f) { return (f & 2) != 0; }
constexpr bool gemm_smallm_form_pre(int f) { return (f & 1) != 0; }
GemmSmallmForm gemm_smallm_form(const GemmArgs &a, int epi);   // of a product launch_gemm sends there (M <= kSmallMRows, K % 64 == 0; ln_g: gemm_smallm_ln_applies)
// Every form launch_gemm_smallm can take = every instantiation of the three kernels: chain 5 epilogues x 3 ring depths x natural / sigma; rt2 the four
// epilogues without GLU; ln none / relu / silu / glu x K = 512 / 1024, then SiLU with the norm in front and GLU with the conv tail at both K.
constexpr int kGemmSmallmFormCount = 5 * 3 * 2 + 4 + 4 * 2 + 2 + 2;
struct GemmSmallmForms { GemmSmallmForm v[kGemmSmallmFormCount]; int n; };
constexpr GemmSmallmForms gemm_smallm_forms() {
    GemmSmallmForms t{};
    constexpr int ring[3] = {8, 2, 1}, ln_epi[4] = {EPI_NONE, EPI_RELU, EPI_SILU, EPI_GLU};
    for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi)
        for (int r = 0; r < 3; ++r)
            for (int sig = 0; sig < 2; ++sig) t.v[t.n++] = gemm_smallm_form_of(SMALLM_CHAIN, epi, ring[r], sig != 0);
    for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_smallm_form_of(SMALLM_RT2, epi, 4, true);
    for (int per_lane = 8; per_lane <= 16; per_lane += 8) {
        for (int e = 0; e < 4; ++e) t.v[t.n++] = gemm_smallm_form_of(SMALLM_LN, ln_epi[e], per_lane, true);
        t.v[t.n++] = gemm_smallm_form_of(SMALLM_LN, EPI_SILU, per_lane, true, false, true);
        t.v[t.n++] = gemm_smallm_form_of(SMALLM_LN, EPI_GLU, per_lane, true, true, false);
    }
    return t;
}
constexpr GemmSmallmForms kGemmSmallmForms = gemm_smallm_forms();
static_assert(kGemmSmallmForms.n == kGemmSmallmFormCount, "kGemmSmallmForms must list every instantiation");
// The form of a tile-kernel launch (kernels/gemm.hip, gemm_pipe.hpp), by the function launch_gemm switches on for every product it does not send to
// the small-M kernels: value = gemm_tile_form_of(...).
//   kernel: gemm_nt_kernel (K < 64: one K tile) or gemm_pipe_kernel
//   wgm x wgn waves of tm x tn 32 x 32 accumulators: the tile is (32 wgm tm) x (32 wgn tn); gemm_nt_kernel<BM, BN> is 2 x 2 waves of (BM / 64) x (BN / 64)
//   nbuf:   LDS staging buffers (NBUF; gemm_nt_kernel: 2);  lna: the LayerNorm applied while A is staged (GemmArgs::ln_stats);  sched: SCHED of gemm_pipe_kernel
//   epi:    the epilogue the kernel is instantiated for (GemmEpi)
enum GemmTileKernel { TILE_NT = 0, TILE_PIPE = 1 };
enum GemmTileForm : int {};
constexpr GemmTileForm gemm_tile_form_of(int kernel, int wgm, int wgn, int tm, int tn, int nbuf, bool lna, int sched, int epi) {
    return (GemmTileForm)((kernel << 20) | (wgm << 17) | (wgn << 14) | (tm << 11) | (tn << 8) | (nbuf << 6) | ((lna ? 1 : 0) << 5) | (sched << 3) | epi);
}
constexpr GemmTileForm gemm_tile_nt_form(int bm, int bn, int epi) { return gemm_tile_form_of(TILE_NT, 2, 2, bm / 64, bn / 64, 2, false, 0, epi); }
constexpr int gemm_tile_form_epi(int f) { return f & 7; }
constexpr int gemm_tile_form_shape(int f) { return f & ~7; }       // everything but the epilogue: what launch_gemm's switch has one case for
GemmTileForm gemm_tile_form(const GemmArgs &a, int epi);          // of a product launch_gemm keeps (gemm_tile_applies; ln_stats: gemm_ln_stats_applies)
bool gemm_tile_applies(const GemmArgs &a);                        // launch_gemm does NOT send the product to the small-M kernels
// What no tile kernel can do (nullptr: nothing): a GLU or a residual product with sigma_cols (the wide epilogue's sigma read has no GLU column mapping,
// and it adds the residual by output position where the scalar epilogue and the small-M kernels add it by natural column), K < 32 or
// K % 32 != 0 (the K loop runs K / 32 whole tiles), lda / ldw no multiple of 4 (float4 staging loads).  launch_gemm aborts on these.
const char *gemm_tile_refusal(const GemmArgs &a, int epi);
// launch_gemm's tile branch alone: aborts on gemm_tile_refusal, launches, and returns the form it switched on (callers checked gemm_tile_applies and,
// with ln_stats, gemm_ln_stats_applies)
GemmTileForm launch_gemm_tile(const GemmArgs &a, int epi, hipStream_t s);
constexpr int kGemmTileSched = 2;                                 // SCHED of every single-buffered tile (gemm.hip: the measurements)
// Every form launch_gemm can take = every instantiation of the two kernels it launches: the 64 x 64 one-K-tile kernel without GLU and its 128 x 128 GLU
// form; the long-K single-round tile (2 x 4 waves of 2 x 1; SCHED 0 without an epilogue function) without GLU; the wide single-buffered tile (4 x 2 waves
// of 1 x 2) with every epilogue, and with the LayerNorm fold without the residual one; the double-buffered 128 x 64 and 64 x 64 tiles without GLU.
constexpr int kGemmTileFormCount = 4 + 1 + 4 + 5 + 4 + 4 + 4;
struct GemmTileForms { GemmTileForm v[kGemmTileFormCount]; int n; };
constexpr GemmTileForms gemm_tile_forms() {
    GemmTileForms t{};
    for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_tile_nt_form(64, 64, epi);
    t.v[t.n++] = gemm_tile_nt_form(128, 128, EPI_GLU);
    for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_tile_form_of(TILE_PIPE, 2, 4, 2, 1, 1, false, epi == EPI_NONE ? 0 : kGemmTileSched, epi);
    for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi) t.v[t.n++] = gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, false, kGemmTileSched, epi);
    for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi)
        if (epi != EPI_RESID) t.v[t.n++] = gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, true, kGemmTileSched, epi);
    for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_tile_form_of(TILE_PIPE, 2, 2, 2, 1, 2, false, 0, epi);
    for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_tile_form_of(TILE_PIPE, 2, 2, 1, 1, 2, false, 0, epi);
    return t;
}
constexpr GemmTileForms kGemmTileForms = gemm_tile_forms();
static_assert(kGemmTileForms.n == kGemmTileFormCount, "kGemmTileForms must list every instantiation");
// same contract with bf16 operands and fp32 accumulation: a.W points to bf16 weights [N][K] (rounded once at upload), A is
// rounded to bf16 while it is staged; K % 64 == 0.  Not bit-identical to the fp32 chain (kernels/gemm_bf16.hpp).
void launch_gemm_bf16(const GemmArgs &a, int epi, hipStream_t s);
// The form of a bf16 tile launch (kernels/gemm.hip, gemm_bf16.hpp, gemm_bf16_glds.hpp), by the function launch_gemm_bf16 switches on for every product it
// does not send to the small-M bf16 kernel: value = gemm_bf16_form_of(...).
//   kernel: gemm_bf16_kernel (register-staged) or gemm_bf16_glds_kernel (direct-to-LDS; A already bf16)
//   wgm x wgn waves of tm x tn 32 x 32 accumulators: the tile is (32 wgm tm) x (32 wgn tn)
//   a16:    A read as bf16 (GemmArgs::a_bf16); fp32 rows are rounded while they are staged (register-staged kernel only)
//   efo:    the epilogue form -- through LDS (gp_epilogue: wide or scalar), the register epilogue on one tile per workgroup, the persistent walk with the
//           register epilogue, the register residual epilogue.  The register-staged kernel has the LDS one only.
//   epi:    the epilogue function the kernel is instantiated for (GemmEpi)
enum GemmBf16Kernel { BF16_REG = 0, BF16_GLDS = 1 };
enum GemmBf16Epilogue { BF16_EPI_LDS = 0, BF16_EPI_DIRECT = 1, BF16_EPI_PERSIST = 2, BF16_EPI_RESID_REG = 3 };
enum GemmBf16Form : int {};
constexpr GemmBf16Form gemm_bf16_form_of(int kernel, int wgm, int wgn, int tm, int tn, bool a16, int efo, int epi) {
    return (GemmBf16Form)((kernel << 18) | (wgm << 15) | (wgn << 12) | (tm << 9) | (tn << 6) | ((a16 ? 1 : 0) << 5) | (efo << 3) | epi);
}
constexpr int gemm_bf16_form_epi(int f) { return f & 7; }
constexpr int gemm_bf16_form_shape(int f) { return f & ~7; }       // everything but the epilogue function: what the launcher's switch has one case for
GemmBf16Form gemm_bf16_form(const GemmArgs &a, int epi);          // of a product launch_gemm_bf16 keeps (gemm_smallm_bf16_applies goes first)
// What the kernel a product is sent to does not implement (nullptr: nothing): the blocked activation layout (GemmArgs::out_blocked / a_blocked) on the
// register-staged kernel, a blocked output on the LDS epilogue of the direct-to-LDS kernel.  launch_gemm_bf16 aborts on these.
const char *gemm_bf16_refusal(const GemmArgs &a, int epi);
// launch_gemm_bf16 behind the small-M branch: aborts on gemm_bf16_refusal, launches, and returns the form it switched on
GemmBf16Form launch_gemm_bf16_tile(const GemmArgs &a, int epi, hipStream_t s);
// Every form launch_gemm_bf16_tile can take = every instantiation of the two kernels: register-staged 128 x 128 (4 x 2 waves of 1 x 2) with every epilogue
// function, 128 x 64 (2 x 2 of 2 x 1) and 64 x 64 (2 x 2 of 1 x 1) without GLU, each with fp32 or bf16 A; direct-to-LDS 192 x 256 (2 x 4 of 3 x 2) and 256 x 256
// (4 x 2 of 2 x 4): none / relu / silu / glu on the LDS, the one-tile register and the persistent register epilogue, resid on the LDS and the register residual one.
constexpr int kGemmBf16FormCount = 2 * (5 + 4 + 4) + 2 * (4 * 3 + 2);
struct GemmBf16Forms { GemmBf16Form v[kGemmBf16FormCount]; int n; };
constexpr GemmBf16Forms gemm_bf16_forms() {
    GemmBf16Forms t{};
    for (int a16 = 0; a16 < 2; ++a16) {
        for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi) t.v[t.n++] = gemm_bf16_form_of(BF16_REG, 4, 2, 1, 2, a16 != 0, BF16_EPI_LDS, epi);
        for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_bf16_form_of(BF16_REG, 2, 2, 2, 1, a16 != 0, BF16_EPI_LDS, epi);
        for (int epi = EPI_NONE; epi <= EPI_RESID; ++epi) t.v[t.n++] = gemm_bf16_form_of(BF16_REG, 2, 2, 1, 1, a16 != 0, BF16_EPI_LDS, epi);
    }
    for (int tall = 0; tall < 2; ++tall)
        for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi)
            for (int efo = BF16_EPI_LDS; efo <= BF16_EPI_RESID_REG; ++efo)
                if (epi == EPI_RESID ? (efo == BF16_EPI_LDS || efo == BF16_EPI_RESID_REG) : efo != BF16_EPI_RESID_REG)
                    t.v[t.n++] = tall ? gemm_bf16_form_of(BF16_GLDS, 4, 2, 2, 4, true, efo, epi) : gemm_bf16_form_of(BF16_GLDS, 2, 4, 3, 2, true, efo, epi);
    return t;
}
constexpr GemmBf16Forms kGemmBf16Forms = gemm_bf16_forms();
static_assert(kGemmBf16Forms.n == kGemmBf16FormCount, "kGemmBf16Forms must list every instantiation");
// the same for a handful of rows (streaming chunks in the tolerance-class mode): kernels/gemm_smallm_bf16.hip -- one workgroup per 16 output
// columns, K split over its waves, every weight byte requested up front.  launch_gemm_bf16 routes the shapes gemm_smallm_bf16_applies() accepts
// (M <= kSmallMRowsBf16, K % 256 == 0, row-major output) there.
constexpr int kSmallMRowsBf16 = 128;
bool gemm_smallm_bf16_applies(const GemmArgs &a, int epi);
bool gemm_smallm_bf16_dw_applies(const GemmArgs &a, int epi, int c, int kc);   // ... with GemmArgs::dw_tail: GLU, conv kernel 9, c = 1 / 2 / 4 frames per stream
bool gemm_smallm_bf16_ln_applies(const GemmArgs &a, int epi);
bool gemm_smallm_bf16_pre_applies(const GemmArgs &a, int epi);    // ... and GemmArgs::pre_g (a second norm in front): SiLU products, slices of 256 k     // ... with GemmArgs::ln_g set: K = 256 * (1 .. 8 waves; GLU: 4), fp32 rows
// The form of a small-M bf16 launch, by the function launch_gemm_smallm_bf16 switches on: value = gemm_smallm_bf16_form_of(...) -- the template
// parameters of gemm_smallm_bf16_kernel and the one kernel argument that selects a path of its own:
//   epi:    the epilogue the kernel is instantiated for (GemmEpi);  steps: MFMA steps of 32 k per K slice, 8 or 16 (bf16 rows, K / 256 > 8 waves, K % 512 == 0)
//   rt:     16-row MFMA tiles per wave, 1 or 2 (32 rows per workgroup);  rvalid: the rows of a tile that exist, 16, or 8 (rt = 1: 8 rows per workgroup)
//   a16:    A read as bf16 rows (GemmArgs::a_bf16);  ln: the LayerNorm folded in (ln_g);  ct: 16-column tiles per wave, 1 or 2
//   wt:     the weights from the operand-tile copy (W_t16, N % 16 == 0);  dw: GLU with the conv tail (dw_tail);  at: A in 8-row operand tiles (a_t8)
//   al:     fp32 rows travel global -> LDS by DMA (rt = 1, fp32 rows, wt);  pre: the second norm in front of the folded one (pre_g)
enum GemmSmallmBf16Form : int {};
constexpr GemmSmallmBf16Form gemm_smallm_bf16_form_of(int epi, int steps, int rt, int rvalid, bool a16, bool ln, int ct, bool wt, bool dw, bool at, bool al,
                                                      bool pre) {
    return (GemmSmallmBf16Form)(epi | ((steps == 16 ? 1 : 0) << 3) | ((rt == 2 ? 1 : 0) << 4) | ((rvalid == 16 ? 1 : 0) << 5) | ((a16 ? 1 : 0) << 6) |
                                ((ln ? 1 : 0) << 7) | ((ct == 2 ? 1 : 0) << 8) | ((wt ? 1 : 0) << 9) | ((dw ? 1 : 0) << 10) | ((at ? 1 : 0) << 11) |
                                ((al ? 1 : 0) << 12) | ((pre ? 1 : 0) << 13));
}
constexpr int gemm_smallm_bf16_form_epi(int f) { return f & 7; }
constexpr int gemm_smallm_bf16_form_steps(int f) { return (f >> 3) & 1 ? 16 : 8; }
constexpr int gemm_smallm_bf16_form_rt(int f) { return (f >> 4) & 1 ? 2 : 1; }
constexpr int gemm_smallm_bf16_form_rvalid(int f) { return (f >> 5) & 1 ? 16 : 8; }
constexpr bool gemm_smallm_bf16_form_a16(int f) { return (f >> 6) & 1; }
constexpr bool gemm_smallm_bf16_form_ln(int f) { return (f >> 7) & 1; }
constexpr int gemm_smallm_bf16_form_ct(int f) { return (f >> 8) & 1 ? 2 : 1; }
constexpr bool gemm_smallm_bf16_form_wt(int f) { return (f >> 9) & 1; }
constexpr bool gemm_smallm_bf16_form_dw(int f) { return (f >> 10) & 1; }
constexpr bool gemm_smallm_bf16_form_at(int f) { return (f >> 11) & 1; }
constexpr bool gemm_smallm_bf16_form_al(int f) { return (f >> 12) & 1; }
constexpr bool gemm_smallm_bf16_form_pre(int f) { return (f >> 13) & 1; }
GemmSmallmBf16Form gemm_smallm_bf16_form(const GemmArgs &a, int epi);   // of a product gemm_smallm_bf16_applies accepts (ln_g / pre_g / dw_tail: their predicates)
GemmSmallmBf16Form launch_gemm_smallm_bf16(const GemmArgs &a, int epi, hipStream_t s);   // launches, and returns the form it switched on
// Every form launch_gemm_smallm_bf16 can take.  A form exists when its fields are consistent with the launcher's rules:
//   slices of 512 k: bf16 rows, no GLU (two weight tiles per wave);  a folded norm reads fp32 rows
//   two row tiles per wave: no GLU, one column tile, none of dw / al / pre;  two column tiles per wave: fp32 rows, no GLU, 16 rows per workgroup
//   a_t8: the residual product on bf16 rows;  the conv tail: GLU;  the second norm: SiLU with the folded norm, one row tile
//   LDS-DMA rows: exactly the fp32-row forms of one row tile on operand-tiled weights
constexpr bool gemm_smallm_bf16_form_exists(int epi, int steps, int rt, int rvalid, bool a16, bool ln, int ct, bool wt, bool dw, bool at, bool al, bool pre) {
    const bool glu = epi == EPI_GLU;
    if (steps == 16 && (!a16 || glu)) return false;
    if (ln && a16) return false;
    if (rt == 2 && (glu || ct != 1 || rvalid != 16 || dw || al || pre)) return false;
    if (ct == 2 && (a16 || glu || rt != 1 || rvalid != 16)) return false;
    if (at && !(epi == EPI_RESID && a16)) return false;
    if (dw && !glu) return false;
    if (pre && !(ln && epi == EPI_SILU)) return false;
    return al == (rt == 1 && !a16 && wt);
}
struct GemmSmallmBf16Forms { GemmSmallmBf16Form v[256]; int n; };
constexpr GemmSmallmBf16Forms gemm_smallm_bf16_forms() {
    GemmSmallmBf16Forms t{};
    for (int epi = EPI_NONE; epi <= EPI_GLU; ++epi)
        for (int bits = 0; bits < (1 << 11); ++bits) {
            const int steps = bits & 1 ? 16 : 8, rt = bits & 2 ? 2 : 1, rvalid = bits & 4 ? 16 : 8, ct = bits & 32 ? 2 : 1;
            const bool a16 = bits & 8, ln = bits & 16, wt = bits & 64, dw = bits & 128, at = bits & 256, al = bits & 512, pre = bits & 1024;
            if (gemm_smallm_bf16_form_exists(epi, steps, rt, rvalid, a16, ln, ct, wt, dw, at, al, pre))
                t.v[t.n++] = gemm_smallm_bf16_form_of(epi, steps, rt, rvalid, a16, ln, ct, wt, dw, at, al, pre);
        }
    return t;
}
constexpr GemmSmallmBf16Forms kGemmSmallmBf16Forms = gemm_smallm_bf16_forms();
// two row tiles: 4 epilogues x (fp32 / folded norm / bf16 rows in slices of 256 / 512 k) x wt = 32, + a_t8 on both slice lengths x wt = 4;
// one row tile, 8 or 16 rows per workgroup: fp32 / folded-norm rows 5 epilogues x 2 x wt x 2 = 40, + two column tiles 4 x 2 x wt = 16, + the second norm (one or
// two column tiles) 2 x wt + wt = 6, + the conv tail 2 x wt x 2 = 8; bf16 rows 5 x wt x 2 + 4 x wt x 2 (slices of 512 k) = 36, + a_t8 2 x wt x 2 = 8, + the conv tail
// wt x 2 = 4
constexpr int kGemmSmallmBf16FormCount = 32 + 4 + 40 + 16 + 6 + 8 + 36 + 8 + 4;
static_assert(kGemmSmallmBf16Forms.n == kGemmSmallmBf16FormCount, "kGemmSmallmBf16Forms must list every form the launcher can take");
double gemm_flops(const GemmArgs &a, int epi);

// ---- conv subsampling (src/encoder.cpp:219-241), channels-last ---------------------------------------
// rag set (strips = units of sub_conv1_dw1_strip_rows(...) rows of H2): packed feats [sum Tm][F] -> out [sum H2][W2][C]; B / Tm ignored
int sub_conv1_dw1_strip_rows(int64_t total_h2_rows);       // output rows per strip the launcher will use for a batch with that many H2 rows
// Which instantiation a launcher of this file's conv kernels takes.  The launchers switch on these functions' results and pk_diag_conv_variants
// reports them (tests/test_gpu_conv_variants.py asks instead of re-deriving a threshold); kConvInsts below lists every one of them.
enum SubC1d1Inst { C1D1_X20_Y2, C1D1_X16_Y2, C1D1_C2_X4_Y8, C1D1_X10_Y8, C1D1_X8_Y8, C1D1_N };   // sub_conv1_dw1_kernel<XC, YS> / sub_conv1_dw1_c2_kernel<XC, YS>
SubC1d1Inst sub_conv1_dw1_inst(int strip_rows /* sub_conv1_dw1_strip_rows(total H2 rows) */, int C, int W2);
enum SubDwInst { SUBDW_X5, SUBDW_X4, SUBDW_N };                                                  // sub_dw4_kernel<XO>
SubDwInst sub_dw_inst(int Wo);
void launch_sub_conv1_dw1(const float *feats, int B, int Tm, int F, int C, const float *w1, const float *b1, const float *wd,
                          const float *bd, float *out, hipStream_t s, const SubRag &rag = SubRag());
// rag set (strips = one unit per output row): packed in [sum H2][W][C] -> out [sum T][Wo][C]; B / H ignored
void launch_sub_dw(const float *in, int B, int H, int W, int C, const float *wd, const float *bd, float *out, hipStream_t s, const SubRag &rag = SubRag());

// ---- conformer pieces ---------------------------------------------------------------------------------
// qkv[B*T][3d]: q and k thirds in the sigma column layout.  pos == nullptr: plain multi-head attention (src/transformer.cpp:38),
// no position term, bias_u / bias_v ignored.  scale <= 0: 1/sqrt(d / n_heads).
size_t relpos_attention_lds_bytes(int T, int hd);     // 0: unsupported head size
int relpos_attention_max_frames(int hd);              // longest sequence one workgroup's LDS score block can hold
size_t relpos_attention_scratch_bytes(int B, int T, int n_heads, int hd);   // long sequences: score blocks in global scratch (hd 64 / 128)
// pos_row0: first row of the table to use (the table may have been built for a longer sequence: row p of a T-frame table is row
// p + T_table - T of the longer one, engine.cpp ensure_pos_tables).  rag set (units = 32-row blocks): qkv / ctx are packed [sum T] rows,
// utterance b attends over its own T[b] frames with table rows from rag.pos_T - T[b]; B / T / pos_row0 ignored, LDS sized by rag.T_max.
void launch_relpos_attention(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u,
                             const float *bias_v, float *ctx, hipStream_t s, float scale = 0.0f, float *scratch = nullptr, int ctx_bf16 = 0,
                             int pos_row0 = 0, const SeqRag &rag = SeqRag(), int form = 0);
// form: which fp32 kernel runs.  ATT_FORM_AUTO: relpos_attention_form decides; the other two ask for one (diagnostics, A/B).  The "strip" form
// (one wave per 16 query rows, the scores in registers) covers hd 32 / 64 with the longest sequence of the launch <= 128 frames, LDS only.
enum { ATT_FORM_AUTO = 0, ATT_FORM_BLOCK = 1, ATT_FORM_STRIP = 2 };
// -> the form the launch takes (ATT_FORM_BLOCK / ATT_FORM_STRIP), or -1 when `want` does not cover it.  t_longest: T, or rag.T_max.
int relpos_attention_form(int t_longest, int hd, bool scratch, int want);
size_t relpos_attention_scratch_bytes_units(int64_t n_units, int T_max, int n_heads, int hd);   // ragged form of relpos_attention_scratch_bytes
// Limited-context ("band") form, kernels/attention.hip (relpos_attention_kernel with BAND): query row i attends to keys [max(0, i - left), min(T - 1, i + right)] only.
// qkv as above (fp32, q / k sigma columns), pos = the layer's LOCAL table [left + right + 1][d] (sigma columns; row r = position i - j = left - r).
// rag set (units = 32-row blocks): packed rows, per-utterance T; the local table is the same for every utterance.  ctx_bf16: 0 fp32, 1 bf16, 2 fp32 sigma.
// Every block's score block is [32][<= left + right + 32] in LDS: left + right <= relpos_local_attention_max_span(hd) (-1: unsupported head size).
int relpos_local_attention_max_span(int hd);
void launch_relpos_local_attention(const float *qkv, int B, int T, int d, int n_heads, const float *pos, const float *bias_u, const float *bias_v,
                                   float *ctx, hipStream_t s, int ctx_bf16, int left, int right, const SeqRag &rag = SeqRag());
// Causal form (relpos_attention_kernel with BAND and CAUSAL; the Transformer LM of neural_lm.cpp): ctx_i = softmax_j<=i(scale q_i . k_j) V over PACKED
// sequences -- rag is required (units = 32-row blocks, rag.T[b] positions each, rag.T_max the longest) -- with no position term.  qkv [rows][3 d]
// (q / k sigma columns), ctx [rows][d] fp32 natural columns.  hd = d / n_heads in {32, 64, 96, 128}; the [32][T_max] score block lives in LDS:
// causal_attention_lds_bytes(T_max, hd) <= 160 KB (0: unsupported head size; 512 positions fit at every head size).
size_t causal_attention_lds_bytes(int T_max, int hd);
void launch_causal_attention(const float *qkv, int d, int n_heads, float scale, float *ctx, hipStream_t s, const SeqRag &rag);
// ---- Transformer LM (kernels/neural_lm.hip) ----
// Packed positions of n strings: row r belongs to string b = row_str[r] at position i = r - row_off[b]; its input token is bos at i = 0 and
// ids[id_off[b] + i - 1] behind it, its target ids[id_off[b] + i] for i < the string's length and eos at the end term.
// h[r][:] = tok_emb[input][:] + pos_emb[i][:] (one fp32 add; d a multiple of 4), tgt[r] = the target.
void launch_nlm_embed(const float *tok_emb, const float *pos_emb, const int32_t *ids, const int32_t *id_off, const int32_t *row_off, const int32_t *row_str,
                      int bos, int eos, int d, int64_t rows, float *h, int32_t *tgt, hipStream_t s);
// lp[r] = logit_r[tgt[r]] - logsumexp_c logit_r[c], logit_r[c] = the natural-k fma chain h_r . W_c from zero (+ bias[c], one add), c < V.  The logits
// are never stored.  d a multiple of 32, ldh / ldw multiples of 4, V >= 1, any rows >= 1, 0 <= tgt[r] < V.
void launch_nlm_head_logp(const float *h, int64_t ldh, const float *W, int64_t ldw, const float *bias, const int32_t *tgt, int64_t rows, int V, int d,
                          float *lp, hipStream_t s);
// The tolerance-class (pk_config.gemm_bf16) attention, kernels/attention_bf16.hip: q / k / v as bf16 [B*T][3d] (natural columns, written by the
// qkv GEMM), the projected position table of the layer as bf16 [2T-1][d], cvec[h][p] = (v_h - u_h) . P_p (fp32, launch_pos_cvec), ctx as bf16.
// Head sizes 64 and 128; relpos_attention_bf16_lds_bytes returns 0 for any other.
size_t relpos_attention_bf16_lds_bytes(int T, int hd);
void launch_pos_cvec(const void *pos_bf16, const float *bias_u, const float *bias_v, int P, int d, int n_heads, float *cvec, hipStream_t s);
// pos_T: sequence length the table / cvec were built for (>= T; 0 = T).  rag set (units = the kernel's query-row blocks,
// relpos_attention_bf16_block_rows()): packed rows, per-utterance T.
int relpos_attention_bf16_block_rows(int hd);
void launch_relpos_attention_bf16(const void *qkv_bf16, int B, int T, int d, int n_heads, const void *pos_bf16, const float *cvec, const float *bias_u,
                                  void *ctx_bf16, hipStream_t s, int pos_T = 0, const SeqRag &rag = SeqRag());
void launch_dwconv_bn_silu(const float *g, int B, int T, int d, int kc, const float *w, const float *bias, const float *bn_mean,
                           const float *bn_rstd, const float *bn_g, const float *bn_b, float *out, hipStream_t s, int out_bf16 = 0,
                           const SeqRag &rag = SeqRag());
int dwconv_strip_frames(int64_t total_rows);   // frames per strip launch_dwconv_bn_silu uses for a batch of that many rows (rag.units granularity)
enum DwconvInst { DWCONV_K9_T2, DWCONV_K9_T8, DWCONV_K31_T2, DWCONV_K31_T8, DWCONV_N };          // dwconv_bn_silu_kernel<KC, TT>; DWCONV_N: no kernel for that size
DwconvInst dwconv_inst(int64_t total_rows, int kc);
// the kernel's two bodies: every input row of the strip loaded before the first is used (true), or a window of KC rows sliding through registers
__host__ __device__ constexpr bool dwconv_loads_first(int kc, int tt) { return kc + tt - 1 <= 16; }

// ---- streaming encoder pieces (src/streaming_encoder.cpp) -----------------------------------------------------------------------
// StreamingConformerAttention::forward_cached (:162-272) core for S streams x c query rows: keys / values = nc cached rows
// followed by the c rows of this chunk (qkv_new[S*c][3d], natural columns); position scores are the rightmost kv = nc + c
// columns of (q+v) P^T WITHOUT rel_shift (:215-224), masked to the [left, right] context (:226-247).  ctx[S*c][d].
void launch_stream_attention(const float *qkv_new, const float *kcache, const float *vcache, int cache_rows, int S, int c, int nc, int d,
                             int n_heads, const float *pos /*[P][d]*/, int P, const float *bias_u, const float *bias_v, int att_left,
                             int att_right, float *ctx, hipStream_t s, float *cache_k_out = nullptr, float *cache_v_out = nullptr, int keep_max = 0,
                             int ctx_sigma = 0 /* ctx columns in the sigma layout (GemmArgs::a_sigma of the out-projection) */);
// cache_k_out / cache_v_out set and keep = min(keep_max, nc + c) > 0: the same launch also rotates the K / V caches of every (stream, head)
// into those buffers (:193-209) -- row r < keep of the new cache = row nc + c - keep + r of [cache(nc rows) ; new(c rows)], so with keep < c the
// whole new cache comes from the chunk.  The outputs must not alias the caches the attention blocks still read; their rows keep .. cache_rows - 1
// and everything else in them stay untouched.  Row stride of all four caches: cache_rows * d per stream (keep_max <= cache_rows).
// The form of a launch, by the function the launcher switches on: the general kernel with one wavefront or (more than 64 keys) two, or the
// LDS-tile kernel (kv <= 80 keys, c <= 8 new rows, head size 64 / 128).
enum StreamAttentionForm { STREAM_ATT_GENERAL_1W, STREAM_ATT_GENERAL_2W, STREAM_ATT_TILES_HD64, STREAM_ATT_TILES_HD128 };
StreamAttentionForm stream_attention_form(int kv, int c, int hd);
// CausalConformerConvModule::forward_cached middle (:51-73): depthwise conv over [cache(K-1 rows, zeros when !has_cache) ; g(c rows)],
// BatchNorm, SiLU -> out[S*c][d]; cache_out = last K-1 rows of the concatenation.
void launch_stream_dwconv(const float *g, const float *cache_in, int has_cache, int S, int c, int d, int kc, const float *w, const float *bias,
                          const float *bn_mean, const float *bn_rstd, const float *bn_g, const float *bn_b, float *out, float *cache_out,
                          hipStream_t s, int out_sigma = 0 /* out channels in the sigma layout */);
enum StreamDwconvInst { STREAM_DW_K9_C4, STREAM_DW_K31_C2, STREAM_DW_N };                      // stream_dwconv_kernel<KC, CMAX>; STREAM_DW_N: no kernel for that size
StreamDwconvInst stream_dwconv_inst(int kc);
bool stream_dwconv_tail_fusable(int c, int kc);   // the chunk sizes / conv size for which the conv may run as a product's epilogue instead (DwTail)

// Every instantiation the four launchers above can take: {launcher (0 conv1 + dw1, 1 dw2, 2 conv module, 3 streaming conv), instantiation, p0, p1, p2}.
//   conv1 + dw1: p0 = 1 for the packed two-channel kernel, p1 = XC, p2 = YS;  dw2: p1 = XO;  conv module: p0 = KC, p1 = TT, p2 = 1 sliding window /
//   0 loads first;  streaming conv: p0 = KC, p1 = CMAX (p2 there is the body a chunk takes: 0 registers when c <= CMAX, 1 the frame loop)
struct ConvInst { int launcher, inst, p0, p1, p2; };
constexpr ConvInst kConvInsts[] = {
    {0, C1D1_X20_Y2, 0, 20, 2}, {0, C1D1_X16_Y2, 0, 16, 2}, {0, C1D1_C2_X4_Y8, 1, 4, 8}, {0, C1D1_X10_Y8, 0, 10, 8}, {0, C1D1_X8_Y8, 0, 8, 8},
    {1, SUBDW_X5, 0, 5, 0}, {1, SUBDW_X4, 0, 4, 0},
    {2, DWCONV_K9_T2, 9, 2, !dwconv_loads_first(9, 2)}, {2, DWCONV_K9_T8, 9, 8, !dwconv_loads_first(9, 8)},
    {2, DWCONV_K31_T2, 31, 2, !dwconv_loads_first(31, 2)}, {2, DWCONV_K31_T8, 31, 8, !dwconv_loads_first(31, 8)},
    {3, STREAM_DW_K9_C4, 9, 4, 0}, {3, STREAM_DW_K31_C2, 31, 2, 0},
};
static_assert(sizeof(kConvInsts) / sizeof(kConvInsts[0]) == C1D1_N + SUBDW_N + DWCONV_N + STREAM_DW_N, "kConvInsts must list every instantiation");
inline const ConvInst *conv_inst(int launcher, int inst) {
    for (const ConvInst &c : kConvInsts) if (c.launcher == launcher && c.inst == inst) return &c;
    return nullptr;
}

// ---- decoders -------------------------------------------------------------------------------------------
void launch_logsoftmax_argmax(const float *logits, int64_t rows, int ld, int n, float *lp_out, int *best_idx, float *best_lp, hipStream_t s);
// outputs [B][pitch] (pitch 0 = T).  rag set: best_idx / best_lp are packed [sum T], utterance b has rag.T[b] frames from row rag.T_off[b].
void launch_ctc_collapse(const int *best_idx, const float *best_lp, int B, int T, int blank, int *ids, int *lens, int *start, int *end,
                         float *conf, hipStream_t s, int pitch = 0, const SeqRag &rag = SeqRag());
// ContextTrie of the phrase boosting (reference src/phrase_boost.cpp:9-66) in CSR form: the children of node i are the entries
// [off[i], off[i+1]) of (tok, node).  Every utterance carries its active-state set (the root plus at most one node per trie
// depth, so <= kTrieMaxActive for phrases of < kTrieMaxActive tokens).  off == nullptr: boosting is off.
constexpr int kTrieMaxActive = 64;
struct TrieDev {
    const int *off, *tok, *node;
    int n_nodes;
    float boost;
    int *act, *n_act;               // [B][kTrieMaxActive], [B]
};
void launch_ctc_boosted(const float *logp, int B, int T, int V, int blank, const TrieDev &trie, int *ids, int *lens, int *start, int *end,
                        float *conf, hipStream_t s, int pitch = 0, const SeqRag &rag = SeqRag());
// CTC prefix beam search (kernels/ctc_beam.hip) over log-softmax rows lp[rows][V] (uniform: B x T rows; rag set: packed).
constexpr int kBeamMaxWidth = 32, kBeamMaxPrune = 32;
constexpr int kBeamMaxVocab = 1 << 24;          // the token id's field of a candidate key
// top-K: tk_val / tk_id [rows][K] sorted (value down, id up), blank left out (K <= V - 1); lpb[rows] = lp[row][blank]
void launch_ctc_beam_topk(const float *lp, int64_t rows, int V, int blank, int K, float *tk_val, int *tk_id, float *lpb, hipStream_t s);
struct BeamWalkArgs {
    const float *tk_val; const int *tk_id; const float *lpb;
    int B, T, W, K, N;
    int2 *nodes;                                // [B][node_pitch] (parent node, token); node 0 = the empty prefix, node 1 + t W + r = born in frame t at rank r
    int64_t node_pitch;                         // >= (longest utterance) * W + 1
    int *hyp_node, *hyp_len; float *hyp_score;  // [B][N]: the N best prefixes of the last frame (a slot the beam does not fill: 0, 0, -inf)
    SeqRag rg;
};
void launch_ctc_beam_walk(const BeamWalkArgs &a, hipStream_t s);
// The walk with n-gram LM shallow fusion.  LmDev: the back-off automaton of ngram_lm.hpp in device memory -- state
// records (arc_lo, arc_n, back-off weight bits, back-off state), the arcs' tokens (sorted per state) and (log-prob bits, next state) records,
// and the dense table of the empty context over ids 0 .. U - 1 (U <= V; an id past it scores unk_lp and goes to state 0).
struct LmDev {
    const int4 *state; const int *arc_tok; const int2 *arc; const int2 *uni;
    int U; float unk_lp; int start;
    float alpha, beta;                          // a prefix's LM score grows by alpha * lookup + beta per token
};
struct BeamLmWalkArgs {
    BeamWalkArgs w;
    LmDev lm;
    float *hyp_lm;                              // [B][N]: the LM score of hyp_node's prefix (a slot the beam does not fill: 0)
};
void launch_ctc_beam_lm_walk(const BeamLmWalkArgs &a, hipStream_t s);
struct BeamAlignArgs {
    const float *lp; int V, blank;
    const int2 *nodes; int64_t node_pitch;
    const int *hyp_node, *hyp_len;
    int B, T, N, pitch;                         // token arrays [B][N][pitch], pitch >= the longest utterance
    int timestamps;                             // 0: ids / lens only
    int *ids, *lens, *start, *end; float *conf;
    unsigned char *bp; int64_t bp_pitch;        // back-pointers: bp_pitch >= T (2 T + 1) bytes per hypothesis (timestamps only)
    SeqRag rg;
};
void launch_ctc_beam_align(const BeamAlignArgs &a, hipStream_t s);
// CTC forced alignment of GIVEN token strings (kernels/ctc_align.hip) over the same rows.  One workgroup per utterance;
// every thread keeps a strip of lattice states in registers.  The three shapes (threads x states per thread): 64 x 4, 256 x 8, 1024 x 32.
constexpr int kAlignThreads[3] = {64, 256, 1024}, kAlignStrip[3] = {4, 8, 32};
constexpr int kAlignMaxStates = 1024 * 32;      // 2 L + 1 <= this (L <= 16383)
constexpr int kAlignBpCells = 16;               // lattice cells per back-pointer dword (2 bits each)
constexpr int kAlignTraceFrames = 64;           // frames of back-pointer rows staged in LDS per step of the back-trace
struct CtcAlignArgs {
    const float *lp; int V, blank;
    int B, T;                                   // uniform extents (rg.T == nullptr), else T = the longest utterance
    const int *ids, *id_off;                    // packed token strings, id_off[B + 1]
    unsigned *bp; const int64_t *bp_off;        // back-pointers: utterance b owns T_b rows of ceil((2 L_b + 1) / 16) dwords from dword bp_off[b]
    int *start, *end; float *conf;              // packed as ids (zero-filled by the caller: an utterance with ok = 0 writes none)
    float *score, *total; int *ok;              // [B]; total == nullptr: the forward pass is not run
    SeqRag rg;
};
// shape: index into kAlignThreads / kAlignStrip; every utterance of the batch needs 2 L + 1 <= kAlignThreads[shape] * kAlignStrip[shape]
void launch_ctc_align(const CtcAlignArgs &a, int shape, hipStream_t s);
// CTC keyword spotting (kernels/ctc_kws.hip) over the same rows: every keyword in every utterance, one wave per pair.
constexpr int kKwsMaxLen = 64;                  // tokens of a keyword: one lane each
constexpr int kKwsMaxHits = 16;
constexpr int kKwsAhead = 8;                    // frames whose log-probs are requested ahead of the walk
struct CtcKwsArgs {
    const float *lp; int V, blank;
    int B, T, n_kw;                             // uniform extents (rg.T == nullptr), else T = the longest utterance
    const int *ids, *kw_off;                    // packed keywords, kw_off[n_kw + 1]
    const float *g;                             // row maxima of lp (launch_ctc_rowmax), one per row
    int2 *eb;                                   // scratch: (score bits, start frame) per end frame, [B][n_kw][T_b]: entry n_kw * T_off[b] + k * T_b + t
    int max_hits; float min_score;
    int *n_hits;                                // [B][n_kw]
    int *start, *end; float *score;             // [B][n_kw][max_hits], written whole (unused slots 0 / 0 / -inf)
    SeqRag rg;
};
void launch_ctc_rowmax(const float *lp, float *g, int64_t rows, int V, hipStream_t s);
// every keyword needs 1 <= L <= kKwsMaxLen, max_hits 1 .. kKwsMaxHits, B <= 65535 (grid.y); g filled first
void launch_ctc_kws(const CtcKwsArgs &a, hipStream_t s);

// TDT forced alignment of GIVEN token strings (kernels/tdt_align.hip).  The lattice of utterance b is T_b x (U_b + 1)
// cells, cell (t, u) = the joint at frame t with the prediction net having consumed ids[:u]; cell c = t (U_b + 1) + u of the utterance sits at
// element cell_off[b] + c of blk, (cell_off[b] + c) * D of dl and -- for u < U_b -- lab_off[b] + t U_b + u of lab.
constexpr int kTdtAlignThreads[2] = {64, 256};  // workgroup width of the walk: one wave while the longest diagonal (U + 1 cells) fits it
constexpr int kTdtAlignMaxDur = 8;              // largest duration value: the ring of diagonals holds kTdtAlignMaxDur + 2 of them at most
constexpr int kTdtAlignMaxTokens = 1535;        // U <= this: (kTdtAlignMaxDur + 2) diagonals x (U + 1) cells x 4 bytes <= 61440 bytes of LDS
struct TdtLattice {
    int B, D;
    int durations[8];
    const int *T;                               // [B] frames
    const int *id_off;                          // [B + 1] packed token strings
    const int64_t *cell_off, *lab_off;          // [B + 1]
    float *lab, *blk, *dl;
};
struct TdtAlignArgs {
    TdtLattice lt;
    unsigned char *bp;                          // one byte per cell, utterance b from byte cell_off[b]: i = blank arc i, D + i = label arc i, 255 none
    int *start, *end, *dur_idx; float *conf;    // packed as ids (zero-filled by the caller: an utterance with ok = 0 writes none)
    float *score; int *ok;                      // [B]
    int u_max, dur_max;                         // over the batch: the dynamic LDS is (dur_max + 2) * (u_max + 1) floats
};
void launch_tdt_align(const TdtAlignArgs &a, hipStream_t s);
// Lattice rows [row0, row0 + n) of the batch (row = cell_off[b] + t (U_b + 1) + u): z[i][J] = relu(ep[ep_row0[b] + t][J] + pp[u B + b][J]), the
// joint's hidden activation (natural columns: the A operand of the heads product)
void launch_tdt_lattice_act(const TdtLattice &lt, const int *ep_row0, const float *ep, const float *pp, int J, int64_t row0, int n, float *z, hipStream_t s);
// ... and the same rows of the heads product's output, logits[i][V + D], taken to their 2 + D kept values: canonical log-softmax over the V label
// columns and over the D duration columns, gathered at ids[u] (u < U_b) and blank
void launch_tdt_lattice_keep(const TdtLattice &lt, const int *ids, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s);

// The forward-algorithm total of GIVEN token strings on the same lattice (kernels/tdt_total.hip): the log-sum over every
// path to END.  One workgroup per hypothesis, widths kTdtAlignThreads, the alignment's limits.
struct TdtTotalArgs {
    TdtLattice lt;
    float *total; int *ok;                      // [B]: ok = total > -inf
    int u_max, dur_max;                         // over the batch: the dynamic LDS is (dur_max + 2) * (u_max + 1) floats
};
void launch_tdt_total(const TdtTotalArgs &a, hipStream_t s);

// TDT keyword spotting (kernels/tdt_kws.hip): "utterance" b of the lattice is one (clip, keyword) pair, packed as for the
// alignment (column U_b = L is packed and never read), plus top[cell]: the largest token log-prob of the row.  One wave per pair, lane u owns column u.
struct TdtKwsArgs {
    TdtLattice lt;                              // lab / blk / dl NORMALISED in place by launch_tdt_kws_norm
    int4 *eb;                                   // scratch: (score bits, start frame, end frame, 0) per emission frame of the last token; pair b from entry
                                                // cell_off[b] - lab_off[b] (= the frames of the pairs before it)
    int max_hits; float min_score;
    int *n_hits;                                // [B]
    int *start, *end; float *score;             // [B][max_hits], written whole (unused slots 0 / 0 / -inf)
    int dur_max;                                // over the durations: the dynamic LDS is (dur_max + 2) * (2 D + 1) * 64 dwords
};
// z of lattice rows [row0, row0 + n) as launch_tdt_lattice_act forms it, the prediction net's rows taken through an indirection: pair b reads
// pp[(u n_net + net_of[b])][J] (the net is run once per distinct keyword, not once per pair)
void launch_tdt_kws_act(const TdtLattice &lt, const int *ep_row0, const float *ep, const float *pp, const int *net_of, int n_net, int J, int64_t row0, int n,
                        float *z, hipStream_t s);
// launch_tdt_lattice_keep that also stores top[row]
void launch_tdt_kws_keep(const TdtLattice &lt, float *top, const int *ids, const float *logits, int V, int blank, int64_t row0, int n, hipStream_t s);
// lab -= top, blk -= top, dl[i] -= max_i dl[i], per cell, in place (the arc costs relative to the greedy decision)
void launch_tdt_kws_norm(const TdtLattice &lt, const float *top, int64_t cells, hipStream_t s);
// every pair needs 1 <= U_b <= kKwsMaxLen, max_hits 1 .. kKwsMaxHits, durations in [0, kTdtAlignMaxDur]
void launch_tdt_kws(const TdtKwsArgs &a, hipStream_t s);

// Streaming TDT keyword spotting (kernels/tdt_kws_stream.hip): the same walk over the next c frames of every (stream, keyword)
// pair, picked up from the pair's CARRIED ring, and the online hit rule on the chunk's exit rows.  Every pair of the lattice has T = c frames.
constexpr int kKwsChunkMaxFrames = 62;          // frames of one push (the streaming decode workspace's limit)
struct TdtKwsChunkArgs {
    TdtLattice lt;                              // lab / blk / dl NORMALISED in place by launch_tdt_kws_norm
    float *ring;                                // carried: pair b from dword (dur_max + 2) (2 D + 1) id_off[b], [frame % (dur_max + 2)][2 D + 1][L_b]
    int4 *pend;                                 // carried, [B]: the pending hit (score bits, start, end, 1) or (.., .., .., 0)
    int *last_end;                              // carried, [B]: the end of the last hit that left (-1: none yet)
    int4 *ev; int *n_ev;                        // this push: [B][c] events (score bits, start, end, 0) in the order emitted, and their number [B]
    int4 *rows;                                 // optional, [B][c]: (E bits, Bs, Ee, 0) per frame
    int t0, c;                                  // the chunk is frames [t0, t0 + c) since the session began
    int dur_max, patience; float min_score;
};
void launch_tdt_kws_chunk(const TdtKwsChunkArgs &a, hipStream_t s);

// Endpointing on live audio (kernels/endpoint.hip): the level of the next n log-mel rows of every stream, the exact sliding
// minimum of the last W levels as the noise floor, the raw decision and the online START / END rule, one workgroup per stream.
constexpr int kEndpointMaxFrames = 512;         // rows of one call (a push of the streaming decode workspace's limit feeds about 500)
constexpr int kEndpointMaxWindow = 1024;        // floor_window in frames
constexpr int kEndpointMaxBins = 512;
constexpr int kEndpointStateWords = 8;          // carried per stream: in_utt, run_speech, run_sil, utt_start, last_speech, 3 spare
struct EndpointChunkArgs {
    const float *rows;                          // [S][n][F]: ln(mel + 2^-24), not normalised
    unsigned *ring;                             // carried, [S][W]: the key of frame f in slot f % W
    int *state;                                 // carried, [S][kEndpointStateWords]
    int4 *ev; int *n_ev;                        // this call: [S][n] events (kind | reason << 8, start, end, at) in the order emitted, and their number [S]
    float *level, *floor; int *speech0;         // optional, [S][n]
    int S, t0, n, F, W;                         // the rows are frames [t0, t0 + n) since the reset
    int min_speech, min_silence, max_utterance;
    float abs_thr, margin;
};
void launch_endpoint_chunk(const EndpointChunkArgs &a, hipStream_t s);
// The close of the streams s with mask[s] != 0 (a DEVICE array [S]).  Bit 0: the prediction net's rows of h / c [Ln][S][Hp] become 0 and token[s] the blank
// (h == nullptr: there is no decoder); bit 1: the acoustic state becomes "outside an utterance, run_speech = 0" (state == nullptr: there is no endpointer).
void launch_endpoint_close(const unsigned char *mask, int S, float *h, float *c, int Ln, int Hp, int *token, int blank, int *state, hipStream_t s);

// TDT beam search with n-best output (kernels/tdt_beam.hip).  R = B W rows, beam slot w of clip b is row b W + w.  The
// beam exists in two copies (step s reads copy s & 1 and writes the other): every per-row array below is [2][R].
constexpr int kTdtBeamMaxWidth = 16, kTdtBeamMaxLabels = 16, kTdtBeamMaxDurs = 8;
struct TdtBeamDev {
    int B, W, K, Kd, N, V, D, blank, max_tokens, J, L, Hp;
    int durations[8];
    const int *T, *row0;                        // [B]: frames, first enc_proj row
    int *valid, *t, *len, *par, *born, *tok;    // the beam: slot filled, frame pointer, tokens, parent row, born from a label arc (its token: tok, else the blank)
    float *score;
    unsigned long long *hash;                   // of the token string (a filter in front of the exact comparison)
    int *prefix;                                // [2][R][max_tokens] token strings
    int *lab_id; float *lab_lp;                 // [R][K + 1] the row's K best labels and the blank, sorted (id -1: no such label)
    int *dur_i; float *dur_lp;                  // [R][Kd] the row's best durations, sorted
    float *cand;                                // [R][(K + 1) Kd] candidate scores, label rank then duration rank
    int4 *bp;                                   // [steps][R] per step and new slot: parent slot, token or -1, emission frame * 8 + duration index, label log-prob bits
    int *live, *steps_done;                     // [B] live hypotheses of the clip's beam, steps the clip has taken
    int *live_total;                            // [step cap + 1] live hypotheses of the batch after s steps (zeroed by the host)
    float *hG[2], *cG[2], *ppG[2];              // gathered state of step s in copy s & 1: h, c [L][R][Hp] (h in the sigma layout), pred_proj [R][J]
    float *hN, *cN, *ppN;                       // the prediction-net step's outputs on the gathered state
    // n-gram LM shallow fusion: lmstate == nullptr is the unfused search, and none of the fields below is looked at
    int *lmstate; float *lm;                    // [2][R] the beam: the automaton's state after the slot's prefix, the prefix's LM score
    int *lab_ls; float *lab_lm;                 // [R][K + 1] beside lab_id: the state and LM score after the label (the blank: the row's own)
    LmDev ngram;
};
struct TdtBeamOut {
    int *ids, *start, *end, *dur_idx; float *conf;      // [B][N][max_tokens], zero-filled by the caller
    int *lens; float *score;                            // [B][N]
    int *ok;                                            // [B]
    float *lm_score;                                    // [B][N], the fused search only (a slot the beam does not fill: 0)
};
void launch_tdt_beam_init(const TdtBeamDev &a, hipStream_t s);
void launch_tdt_beam_gather(const TdtBeamDev &a, int step, hipStream_t s);
void launch_tdt_beam_act(const TdtBeamDev &a, int step, const float *ep, float *z, hipStream_t s);
void launch_tdt_beam_expand(const TdtBeamDev &a, int step, const float *logits, hipStream_t s);
void launch_tdt_beam_prune(const TdtBeamDev &a, int step, hipStream_t s);
void launch_tdt_beam_trace(const TdtBeamDev &a, const TdtBeamOut &o, hipStream_t s);

struct TdtState {
    int B, T, V, D, L, Hp, blank, max_symbols, max_tokens, max_steps;
    TrieDev trie;
    int keep_state;                 // streaming chunks (src/eou.cpp:17-98): the last token and h / c are carried in, end frames are not clamped
    int durations[8];
    const float *logits;            // [B][V+D]
    float *h, *c;                   // committed LSTM state [L][B][Hp]
    const float *hn, *cn;           // candidates of this step
    int *token, *t, *nsym, *n_out, *steps, *done, *lens, *done_count;
    int *ids, *start, *end;         // [B][max_tokens]
    float *conf;
    int h_bf16;                     // tolerance-class mode: h / hn are bf16 arrays (decode_gemv_bf16.hip); c / cn stay fp32
    float *margin;                  // [B] or null: running min over the utterance's decisions of (top-1 - top-2) label log-prob
    // Prediction-net caching (null = off).  After a BLANK the reference reverts the LSTM state and keeps the token (src/tdt.cpp:69-93), so the next
    // step's prediction.step and pred_proj are functions of unchanged inputs: bit for bit the values of the step before.  need[b] = 1 says
    // utterance b's next step must run them (set at the start and after every emitted token); the cell / pred_proj launches compact the set
    // rows and skip the rest, whose candidates hn / cn and pp = pred_proj(h') [+ bias] stay where the last computation left them.  After a blank
    // tdt_decide itself forms the next step's joint activation z = relu(enc_proj[t'] + pp) for the new frame t' (the one line of SK_ACT's
    // epilogue that depends on t).
    int *need = nullptr;            // [B]
    const float *pp = nullptr;      // [B][J] fp32, natural columns
    const float *ep = nullptr;      // enc_proj [B][T][J]
    float *z = nullptr;             // joint activation [B][J]: fp32 sigma layout, or bf16 natural when h_bf16
    int J = 0;
    // Frame window (small lock-step batches, plain greedy step, prediction-net caching on; 1 = off): the joint is evaluated for the frames t .. t + F - 1 of every
    // utterance in ONE heads product (rows b * F + f of z and logits; the 16-row MFMA tile is mostly empty at B <= 8), and tdt_decide walks through the blank
    // decisions whose successor frame lies inside the window -- the same evaluations in the same order, a run of blanks in one launch instead of one each.
    int F = 1;
    // ragged batches: utterance b has Tb[b] frames, its enc_proj rows start at row0[b] (null: T frames from row b * T); the safety cap on joint
    // evaluations is then per utterance, Tb[b] * (max_symbols + 1) + 16 -- what a single-clip run of that utterance would use
    const int *Tb = nullptr, *row0 = nullptr;
    // Teacher-forced scoring (pk_tdt_score: ONE utterance; pk_stream_score: every stream of a lock-step chunk): the decision of step k is
    // GIVEN -- label force_label[k], duration durations[force_dur[k]] -- instead of taken from the argmax, and the step's joint outputs are
    // recorded: score_lab[k][V] label log-probs, score_dur[k][D] duration log-probs.  The utterance is finished after n_force steps (or when
    // the frame pointer leaves it).  Batched form: utterance b's arrays start at element b * force_stride (rows b * force_stride + k of the
    // score arrays) and it walks n_force_b[b] steps (0: nothing to walk, finished at once).
    const int *force_label = nullptr, *force_dur = nullptr;
    int n_force = 0;
    float *score_lab = nullptr, *score_dur = nullptr;
    const int *n_force_b = nullptr;
    int force_stride = 0;
};
constexpr int kDecWindowMax = 8;    // TdtState::F <= this
constexpr int kMaxListRows = 2048;  // largest lock-step batch the compacted launches handle (larger batches run every row)
void launch_tdt_init(const TdtState &st, hipStream_t s);
// Tb_out[i] / row0_out[i], i < n: frames and first enc_proj row (row_base + its offset) of the utterances of one run; T == nullptr: a uniform
// run of T_uniform frames each
void launch_rag_decode_tables(const int *T, const int *T_off, int T_uniform, int n, int row_base, int *Tb_out, int *row0_out, hipStream_t s);
void launch_tdt_decide(const TdtState &st, hipStream_t s);
// The form of a decision launch, by the function the launcher switches on: value = kernel * 16 + slots * 4 + row.
//   kernel: tdt_decide_kernel's instantiation -- the exact greedy step, the register-resident step of the tolerance-class mode (h_bf16), phrase boosting, forced scoring
//   slots:  NC, the 256-element slots of candidate LSTM state a thread carries: 3 / 6 / 12 by L * Hp (boost and score: always 12)
//   row:    how the logits row reaches the workgroup: 5 or 33 register slots per thread by V + D (fast: its NQ), batches of 8 above 33 x 256, or the frame window (F > 1)
enum TdtDecideKernel { TDT_K_EXACT = 0, TDT_K_FAST = 1, TDT_K_BOOST = 2, TDT_K_SCORE = 3 };
enum TdtDecideSlots { TDT_NC3 = 0, TDT_NC6 = 1, TDT_NC12 = 2 };
enum TdtDecideRow { TDT_ROW_5 = 0, TDT_ROW_33 = 1, TDT_ROW_BATCH8 = 2, TDT_ROW_WINDOW = 3 };
enum TdtDecideForm : int {};
constexpr TdtDecideForm tdt_decide_form_of(int kernel, int slots, int row) { return (TdtDecideForm)(kernel * 16 + slots * 4 + row); }
constexpr int kTdtMaxState = 12 * 256;       // L * Hp the decision kernel can carry
constexpr int kTdtWindowMaxJ = 4 * 256;      // J up to which the decision kernel forms every z row of the next window
TdtDecideForm tdt_decide_form(const TdtState &st);
size_t tdt_decide_lds_bytes(const TdtState &st);
bool tdt_decide_launchable(const TdtState &st);   // false: launch_tdt_decide would abort (a window outside its conditions, L * Hp > kTdtMaxState)

// skinny products of the decode loop (kernels/decode_gemv.hip).  X and W are in the "sigma" K layout
// (4x4 index transpose inside every block of 16 k); K % 16 == 0.
enum SkinnyEpi { SK_BIAS = 0, SK_ACT = 1, SK_CELL = 2 };
struct SkinnyArgs {
    const float *X, *W;            // [B][K], [N][K]
    int B, N, K;
    const float *bias;             // SK_BIAS: [N] or null ; SK_ACT: pred_proj bias (switch A5) or null
    float *out; int ldo;           // SK_BIAS: [B][ldo] natural ; SK_ACT: z [B][N] sigma ; SK_CELL: h' [B][Hp] sigma
    // SK_ACT
    const float *ep; const int *t; int T;
    int F = 1;                     // SK_ACT frame window (TdtState::F): z rows b * F + f, f < F <= kDecWindowMax
    // SK_CELL (N = 4*Hp)
    const float *gi; int gi_ld; const int *gi_row; const float *c; float *cn; int Hp;
    // SK_CELL of an upper LSTM layer with the input projection fused in: gi = X2 W2^T + bias2 (X2 [B][K] sigma, W2 [4Hp][K] sigma); W2 null: gi is read
    const float *X2 = nullptr, *W2 = nullptr, *bias2 = nullptr;
    // prediction-net caching (TdtState::need): the launch covers only the rows b with need[b] != 0, compacted in ascending order
    // (B <= kMaxListRows); SK_ACT also stores pred_proj(h') [+ bias] to pp_out [B][N]
    const int *need = nullptr;
    float *pp_out = nullptr;
    const int *Tb = nullptr, *row0 = nullptr;   // SK_ACT on a ragged batch (TdtState::Tb / row0)
};
void launch_skinny_gemm(const SkinnyArgs &a, int epi, hipStream_t s);
// the same products in the tolerance-class mode: X / W / X2 / W2 point to bf16 data in NATURAL k order, the SK_ACT / SK_CELL outputs (z, h') are
// bf16; K % 32 == 0 (kernels/decode_gemv_bf16.hip)
void launch_skinny_gemm_bf16(const SkinnyArgs &a, int epi, hipStream_t s);

// the whole greedy loop of a batch in one launch (kernels/decode_persist.hip): the step-invariant arguments of every phase
struct TdtPersist {
    TdtState st;
    int L;
    SkinnyArgs cell[4], ih[4];      // per LSTM layer: W_hh product + cell ; (l > 0) W_ih product of the layer below's h'
    SkinnyArgs act, heads;          // joint activation ; label (+ duration) heads
    unsigned *bar;                  // grid-barrier words, kTdtBarrierWords of them, zeroed before the launch (decode_persist.hip)
    int *abort;                     // set by a workgroup whose barrier wait timed out
    long long timeout_ticks;        // wall_clock64 ticks (100 MHz)
};
constexpr int kTdtBarrierWords = 64 + 8 * 96;
size_t tdt_persistent_lds_bytes(const TdtState &st);
void launch_tdt_persistent(const TdtPersist &p, hipStream_t s);

// ---- LayerNorm, canonical reductions, math diagnostics ------------------------------------------
// A row lives in the registers of one wavefront, PER_LANE values per lane: kLnMaxCols columns is the widest row the family holds (every caller checks it:
// Model::validate_config, TransformerEncoder, the diagnostics).  The form of a launch, by the functions the four launchers switch on: which launcher,
// PER_LANE (2 / 8 / 16: d <= 128 / <= 512 / <= 1024), RPW (rows per wavefront; layernorm_kernel only), THEN (layernorm_stats_kernel) and, for
// launch_layernorm, which of its two branches took it (batch: rows >= kLnBatchRows -- PK_LN_RPW is 1, so both branches pick the same template today; the
// form still names the branch).  kLnForms lists every one; pk_diag_layernorm_form reports the form it launched (tests/test_gpu_layernorm.py).
#ifndef PK_LN_RPW
#define PK_LN_RPW 1                      // rows per wavefront of launch_layernorm's batch branch (kernels/norm.hip says why it stays 1)
#endif
constexpr int kLnMaxCols = 1024;
constexpr int64_t kLnBatchRows = 4096;
enum LnLauncher { LN_NORM, LN_NORM2, LN_STATS, LN_THEN_STATS, LN_LAUNCHERS };
constexpr int ln_form_of(int launcher, int per_lane, int rpw, bool then, bool batch) {
    return launcher << 12 | (batch ? 1 : 0) << 11 | (then ? 1 : 0) << 10 | rpw << 5 | per_lane;
}
constexpr int ln_form_per_lane(int form) { return form & 31; }
constexpr bool ln_form_batch(int form) { return (form >> 11) & 1; }
constexpr int ln_per_lane(int d) { return d <= 128 ? 2 : d <= 512 ? 8 : 16; }
constexpr bool ln_shape_ok(int64_t rows, int d) { return rows > 0 && d > 0 && d <= kLnMaxCols; }
// -> the form the launcher takes for this shape, -1 for a shape the family does not hold (the launchers refuse it)
constexpr int layernorm_form(int64_t rows, int d) {
    return !ln_shape_ok(rows, d) ? -1 : rows >= kLnBatchRows ? ln_form_of(LN_NORM, ln_per_lane(d), PK_LN_RPW, false, true) : ln_form_of(LN_NORM, ln_per_lane(d), 1, false, false);
}
constexpr int layernorm2_form(int64_t rows, int d) { return ln_shape_ok(rows, d) ? ln_form_of(LN_NORM2, ln_per_lane(d), 1, false, false) : -1; }
constexpr int layernorm_stats_form(int64_t rows, int d) { return ln_shape_ok(rows, d) ? ln_form_of(LN_STATS, ln_per_lane(d), 1, false, false) : -1; }
constexpr int layernorm_then_stats_form(int64_t rows, int d) { return ln_shape_ok(rows, d) ? ln_form_of(LN_THEN_STATS, ln_per_lane(d), 1, true, false) : -1; }
constexpr int kLnForms[] = {
    ln_form_of(LN_NORM, 2, 1, false, false), ln_form_of(LN_NORM, 8, 1, false, false), ln_form_of(LN_NORM, 16, 1, false, false),
    ln_form_of(LN_NORM, 2, PK_LN_RPW, false, true), ln_form_of(LN_NORM, 8, PK_LN_RPW, false, true), ln_form_of(LN_NORM, 16, PK_LN_RPW, false, true),
    ln_form_of(LN_NORM2, 2, 1, false, false), ln_form_of(LN_NORM2, 8, 1, false, false), ln_form_of(LN_NORM2, 16, 1, false, false),
    ln_form_of(LN_STATS, 2, 1, false, false), ln_form_of(LN_STATS, 8, 1, false, false), ln_form_of(LN_STATS, 16, 1, false, false),
    ln_form_of(LN_THEN_STATS, 2, 1, true, false), ln_form_of(LN_THEN_STATS, 8, 1, true, false), ln_form_of(LN_THEN_STATS, 16, 1, true, false),
};
constexpr int kLnFormCount = 3 * (LN_LAUNCHERS + 1);      // three PER_LANE x (four launchers + launch_layernorm's batch branch)
static_assert(sizeof(kLnForms) / sizeof(kLnForms[0]) == kLnFormCount, "kLnForms must list every instantiation");
// Every launcher returns the form it launched (the value its form function gives for the shape).
int launch_layernorm(const float *x, int64_t rows, int d, const float *g, const float *b, float eps, float *y, hipStream_t s, int y_bf16 = 0);   // y_bf16 = 1: y is a bf16 buffer (RNE); 2: fp32, columns in the sigma layout (GemmArgs::a_sigma); y may alias x (mode 0)
// y1 = LN(x; g1, b1), y2 = LN(y1; g2, b2) in one pass (y1 may alias x)
int launch_layernorm2(const float *x, int64_t rows, int d, const float *g1, const float *b1, const float *g2, const float *b2, float eps,
                      float *y1, float *y2, hipStream_t s, int y2_bf16 = 0);
// Statistics only (round 6): stats[row] = {mean, rstd} of x's rows -- layernorm_kernel's reductions (same sum64 butterflies, same divisions), no output tensor:
// the consumer normalises while it stages the rows (GemmArgs::ln_stats).
int launch_layernorm_stats(const float *x, int64_t rows, int d, float eps, float *stats, hipStream_t s);
// y1 = LN(x; g1, b1) written out (may alias x) + the statistics of y1's rows (what launch_layernorm2's second pass would start from)
int launch_layernorm_then_stats(const float *x, int64_t rows, int d, const float *g1, const float *b1, float eps, float *y1, float *stats, hipStream_t s);
void launch_sum64_rows(const float *x, int rows, int n, float *out, hipStream_t s);
void launch_math(int fn, const float *in, float *out, int64_t n, hipStream_t s);   // 0 exp 1 log 2 tanh 3 sigmoid 4 silu 5 sqrt 6 recip 7 relu 8 sigmoid4 9 silu4 20 fast_sigmoid 21 fast_silu
void launch_math_exhaustive(int fn, unsigned long long *out3, hipStream_t s);   // out3 must hold {0, 0, 1 << 32} on entry
void launch_scale(float *x, int64_t n, float a, hipStream_t s);

// ---- polyphase sinc resampler of input-rate PCM (kernels/resample.hip) --------------------------------------
// One launch over a packed ragged batch.  A workgroup of kResampleThreads lanes owns `run` consecutive outputs of one clip and stages the input
// span they read (at most span_cap floats) into LDS; output i = q * up + r of a clip reads the 32 taps around c = q * down + coff[r] with the
// fp64 weights of table row r.  Tables of at most kResampleLdsRows rows are staged into LDS too, larger ones are read from global memory.
constexpr int kResampleThreads = 256;
constexpr int kResampleTaps = 32;
constexpr int kResampleMaxRun = 1024;           // outputs per workgroup, lowered (in steps of 32) until the span fits kResampleSpanCap
constexpr int kResampleSpanCap = 5632;          // floats of input staged per workgroup (22 KB)
constexpr int kResampleLdsRows = 160;           // 160 rows x 33 doubles (padded) = 41.25 KB: with the span 63.9 KB, two workgroups per CU
struct ResampleClip { int64_t in_off, in_len, out_off, out_len, wg0; };   // extents in samples; wg0: the clip's first workgroup
struct ResampleArgs {
    const float *x; float *y;
    const ResampleClip *clip; int n_clips;      // clips with out_len == 0 own no workgroup
    const double *tab; const int *coff;         // [up][32] weights, [up] centre offsets (r * down) / up
    int up, down, run, span_cap;
    int64_t n_wg;                               // workgroups of the launch: sum of ceil(out_len / run)
};
void launch_resample(const ResampleArgs &a, hipStream_t s);

// ---- voice-activity segmentation of 16 kHz PCM (kernels/vad.hip) ------------------------------------------------
// One set of launches over a packed ragged batch.  A clip of n samples has F = ceil(n / 160) frames, cut into chunks of kVadRun frames; chunk
// k of the launch belongs to the last clip whose chunk0 <= k (clips without frames own none).  Every per-frame array (energy, flags) is packed
// clip after clip at frame_off, every per-chunk array at chunk0; the staged PCM of a clip starts at in_off, a multiple of 32 floats (128 bytes).
constexpr int kVadThreads = 256;
constexpr int kVadFrame = 160;                  // samples per frame (10 ms)
constexpr int kVadRun = 256;                    // frames of one chunk: what one workgroup handles per pass (pk_vad_run)
constexpr int kVadGrid = 8;                     // run starts are multiples of the encoder's 8-frame grid
struct VadClip { int64_t in_off, n; int32_t F, rank; int64_t frame_off, chunk0, run_off; };   // rank: of the floor among the clip's keys; run_off: its first run slot
struct VadSelect { uint32_t prefix, rank; };    // the radix select's state of one clip: key bits found so far, rank among the keys sharing them
struct VadArgs {
    const float *x;                             // staged PCM
    const VadClip *clip; int n_clips;
    int64_t n_chunks;                           // chunks of the launch: sum of ceil(F / kVadRun)
    float *energy;                              // [sum F]
    uint32_t *hist;                             // [n_clips][4][256], zero before the launches
    VadSelect *sel;                             // [n_clips]
    uint8_t *flag[2];                           // [sum F] each, ping-pong between the smoothing passes
    int32_t *first[2], *last[2];                // [n_chunks] each: first / last flagged frame of a chunk (clip-relative; F / -1 when none)
    int32_t *n_start, *n_end;                   // [n_chunks]: run starts / run ends inside a chunk
    int32_t *run_start, *run_end, *n_runs;      // [sum (F + 1) / 2] x 2, [n_clips] (zero before the launches)
    float abs_thr, ratio;
    int min_speech, min_silence, pad;           // frames
};
void launch_vad(const VadArgs &a, hipStream_t s);

}  // namespace pk
