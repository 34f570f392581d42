// parakeet.cpp_amd/csrc/conformer_block.hpp -- the steps of ConformerBlock::forward (src/encoder.cpp:196-204) that the offline encoder
// (Model::run_layers, engine.cpp) and the streaming encoder (StreamBatch::encode_device, stream.cpp) share: LayerNorm + product, the two
// FFNs, the qkv / out / pw1 / pw2 products and the end-of-block norm.  Attention and the depthwise conv stay with their callers.
#pragma once
#include "engine.hpp"

namespace pk {

// Where the two callers differ, as data: one instance per encoder call, filled once before the layer loop.  "offline" = Model::run_layers,
// "streaming" = StreamBatch::encode_device.  (Profile records are no field: the steps always go through Model::klaunch_begin / _end, and
// Model::prof is only ever set by the offline batch path.  Partial runs are an argument: ConformerBlock::end_block's next_runs.)
struct BlockMode {
    // both: cfg.gemm_bf16 -- the rows that exist only as GEMM operands (LayerNorm outputs, fc1 activations) are rounded to bf16 by their producers
    // (RNE, the rounding the GEMM's staging path would apply: same operand values) and stored in HALF the bytes of the same buffers
    int bf16 = 0;
    // both: fp32, rows <= kSmallMRows and the tiled copies exist -- every product is a latency-bound chain of dependent MFMAs (gemm_smallm.hip) on
    // W_sig with sigma-K activations, written that way by their producers (LayerNorm mode 2, sigma_cols of fc1, attention, conv); x stays natural
    int sigma = 0;
    // The tiled weight copies (Model::sigma_weights) attached to every product, or null.  offline: W_sig when `sigma`, none in bf16 mode (reason
    // not recorded); streaming: W_sig when `sigma`, W_t16 (copies_t16: the small-M bf16 kernel's operand tiles) in bf16 mode at rows <= kSmallMRowsBf16.
    const std::vector<Model::SigW> *copies = nullptr;
    bool copies_t16 = false;
    // The LayerNorm folds into its product (ln_folds) -- fp32: up to fold_max_rows rows.  offline: kLnFoldRows (engine.cpp; kept as found, not
    // re-measured); streaming: no cap of its own.  bf16: only with fold_bf16.  streaming: true; offline: false (reason not recorded).
    int fold_max_rows = kSmallMRows;
    bool fold_bf16 = false;
    // A second residual-stream buffer: with it a block's final norm rides on the next block's folding fc1 (GemmArgs::pre_g), which writes the
    // normalised rows there.  streaming: set when that fc1 folds and there is a next block; offline: null, never rides (reason not recorded).
    float *x_other = nullptr;
    // fc1 -> fc2 activations in bf16 mode.  offline: BLOCKED (out_blocked / a_blocked when gemm_bf16_blocked_handoff holds for both and h is
    // large enough); streaming: TILES8 (out_t8 / a_t8 when both products pass gemm_smallm_bf16_applies).  Each is the layout of the caller's kernels.
    enum Handoff { BLOCKED, TILES8 } handoff = BLOCKED;
    // GemmArgs::fast_act of fc1 and pw1.  offline: = bf16; streaming: 0, though its small-M bf16 kernel reads it (reason not recorded; kept as
    // found, not re-measured: it changes bits)
    int fast_act = 0;
    // qkv output.  offline: q and k in sigma columns for the fp32 attention kernels (2 d), or all bf16 for the bf16 one; streaming: natural fp32
    int qkv_sigma_cols = 0, qkv_out_bf16 = 0;
    // The A operands of out and pw2 (attention context, conv activations) are bf16.  offline: = bf16, its attention / conv kernels write in
    // act_mode(); streaming: 0, its cached kernels keep fp32 arithmetic on fp32 rows
    int ctx_bf16 = 0;
    int act_mode() const { return sigma ? 2 : bf16; }   // LayerNorm (offline: also attention / conv) output mode: 0 fp32, 1 bf16, 2 fp32 sigma
};

// The fold rule: the product `fg` (ConformerBlock::folded) takes the LayerNorm of its input rows in the same launch -- fp32: gemm_smallm_ln_kernel
// (needs W_sig), bit for bit norm + product; bf16: gemm_smallm_bf16.hip.  Four of a block's fifteen launches go.
inline bool ln_folds(const BlockMode &mode, const GemmArgs &fg, int epi) {
    if (mode.bf16) return mode.fold_bf16 && gemm_smallm_bf16_ln_applies(fg, epi);
    return fg.M <= mode.fold_max_rows && gemm_smallm_ln_applies(fg, epi);
}

// The shared steps of one encoder call on `rows` rows: x = the residual stream [rows][d] (x_home: where the last block's output must land),
// n = the normalised rows, h = the fc1 activations (h_cap bytes).
struct ConformerBlock {
    // the caller's part, brace-initialised: {model, mode, stream, rows, x, n, h, h_cap} and no more (a ninth value would overwrite x_home)
    Model &m;
    const BlockMode &mode;                                // the caller's instance, read at every step: streaming sets x_other after constructing this
    hipStream_t s;
    int64_t rows;
    float *x, *n, *h;
    size_t h_cap;
    // the steps' own state
    float *const x_home = x;
    const int d = m.cfg.hidden_size, f = m.cfg.ffn_intermediate;
    bool norm_done = false;                               // n holds the next ffn1's normalised rows (end_block wrote them)
    const float *pend_g = nullptr, *pend_b = nullptr;     // the previous block's final norm, riding on the next ffn1 fc1 (end_block)

    float *other() const { return x == x_home ? mode.x_other : x_home; }
    template <class F> void timed(double bytes, F launch) { m.klaunch_begin("layernorm", 0.0, bytes, s); launch(); m.klaunch_end(s); }
    void attach(GemmArgs &g, const float *Model::SigW::*w, int l) const {   // a_sigma and the tiled copy of W
        g.a_sigma = mode.sigma;
        if (mode.copies) (mode.copies_t16 ? g.W_t16 : g.W_sig) = (*mode.copies)[l].*w;
    }
    // what ln_gemm launches when the norm (ng, nb) folds into g: the product on the un-normalised natural rows
    GemmArgs folded(const GemmArgs &g, const float *ng, const float *nb) const {
        GemmArgs fg = g;
        fg.A = x; fg.lda = d; fg.a_sigma = 0; fg.a_bf16 = 0; fg.ln_g = ng; fg.ln_b = nb; fg.ln_eps = 1e-5f;
        return fg;
    }
    // y = LayerNorm(x) -> n, then the product g (A = n) -- or the product with the norm folded in (ln_folds), a pending final norm in front of it.
    // norm_done_: n holds the normalised rows already.  (The norm as a statistics pass applied by the fp32 tile kernel: measured slower)
    void ln_gemm(const char *name, const GemmArgs &g, int epi, const float *ng, const float *nb, bool norm_done_) {
        if (!norm_done_) {
            GemmArgs fg = folded(g, ng, nb);
            if (pend_g) {                                            // (checked when it was set: end_block)
                fg.pre_g = pend_g; fg.pre_b = pend_b; fg.pre_out = other(); fg.pre_ldo = d;
                m.run_gemm(name, fg, epi, s);
                x = fg.pre_out;                                      // the normalised rows are the residual stream from here on
                pend_g = pend_b = nullptr;
                return;
            }
            if (ln_folds(mode, fg, epi)) { m.run_gemm(name, fg, epi, s); return; }
            timed((mode.bf16 ? 1.5 : 2.0) * rows * d * 4, [&] { launch_layernorm(x, rows, d, ng, nb, 1e-5f, n, s, mode.act_mode()); });
        }
        m.run_gemm(name, g, epi, s);
    }
    GemmArgs fc1_args(int l, bool second) const {          // (sigma_cols: h is fc2's A operand)
        const LayerW &L = m.layers[l];
        GemmArgs g{n, d, second ? L.ffn2_w1 : L.ffn1_w1, d, second ? L.ffn2_b1 : L.ffn1_b1, h, f, nullptr, 0, 1.0f, (int)rows, f, d};
        g.a_bf16 = mode.bf16; g.out_bf16 = mode.bf16; g.fast_act = mode.fast_act; g.sigma_cols = mode.sigma ? f : 0;
        attach(g, second ? &Model::SigW::ffn2_w1 : &Model::SigW::ffn1_w1, l);
        return g;
    }
    // block l's ffn1 fc1 as it launches when it takes its own norm, and whether it does.  (The probes of end_block ask with these real arguments,
    // hand-off flags aside: the *_ln_applies / *_pre_applies predicates must stay blind to bias, fast_act, W_t16 and the out_t8 / out_blocked flags.)
    GemmArgs fc1_folded(int l) const { return folded(fc1_args(l, false), m.layers[l].ffn1_ng, m.layers[l].ffn1_nb); }
    bool fc1_folds(int l) const { return ln_folds(mode, fc1_folded(l), EPI_SILU); }
    // FeedForward::forward (src/encoder.cpp:39-46): x += 0.5 * fc2(silu(fc1(LN(x))))
    void ffn(int l, bool second) {
        const LayerW &L = m.layers[l];
        GemmArgs g1 = fc1_args(l, second), g2{h, f, second ? L.ffn2_w2 : L.ffn1_w2, f, second ? L.ffn2_b2 : L.ffn1_b2, x, d, x, d, 0.5f, (int)rows, d, f};
        g2.a_bf16 = mode.bf16;
        attach(g2, second ? &Model::SigW::ffn2_w2 : &Model::SigW::ffn1_w2, l);
        if (mode.bf16 && mode.handoff == BlockMode::BLOCKED) {
            // large batches: the fc1 activations live in 32 x 16 blocks between fc1's register epilogue and fc2's LDS-DMA (GemmArgs::out_blocked /
            // a_blocked: every store instruction of the epilogue writes one contiguous KB); h holds rows rounded up to 32
            g1.out_blocked = g2.a_blocked = gemm_bf16_blocked_handoff((int)rows, f, d, EPI_SILU, true) &&
                                            gemm_bf16_blocked_handoff((int)rows, d, f, EPI_RESID, false) && (size_t)((rows + 31) / 32 * 32) * f * 2 <= h_cap;
        } else if (mode.bf16) {   // both products on the small-M bf16 kernel: the activations in its 8-row operand tiles (GemmArgs::out_t8 / a_t8)
            GemmArgs p1 = g1, p2 = g2;
            p1.out_t8 = p2.a_t8 = 1;
            g1.out_t8 = g2.a_t8 = gemm_smallm_bf16_applies(p1, EPI_SILU) && gemm_smallm_bf16_applies(p2, EPI_RESID);
        }
        // (the first FFN's norm rides on the previous block's final_norm_ kernel, end_block -- unless the product folds it in)
        ln_gemm("ffn_fc1_silu", g1, EPI_SILU, second ? L.ffn2_ng : L.ffn1_ng, second ? L.ffn2_nb : L.ffn1_nb, !second && norm_done);
        if (!second) norm_done = false;
        g2.out = x; g2.resid = x;                                    // (a riding final norm has moved the residual stream)
        m.run_gemm("ffn_fc2_resid", g2, EPI_RESID, s);
    }
    void qkv(int l, float *out) {                          // LN + the [q k v] projection
        const LayerW &L = m.layers[l];
        GemmArgs g{n, d, L.wqkv, d, L.bqkv, out, 3 * d, nullptr, 0, 1.0f, (int)rows, 3 * d, d};
        g.sigma_cols = mode.qkv_sigma_cols; g.a_bf16 = mode.bf16; g.out_bf16 = mode.qkv_out_bf16;
        attach(g, &Model::SigW::wqkv, l);
        ln_gemm("attn_qkv", g, EPI_NONE, L.att_ng, L.att_nb, false);
    }
    GemmArgs pw1_args(int l, float *out) const {           // (streaming hangs its conv tail on them)
        GemmArgs g{n, d, m.layers[l].pw1_w, d, m.layers[l].pw1_b, out, d, nullptr, 0, 1.0f, (int)rows, d, d};
        g.a_bf16 = mode.bf16; g.fast_act = mode.fast_act;
        attach(g, &Model::SigW::pw1, l);
        return g;
    }
    void pw1(int l, const GemmArgs &g) { ln_gemm("conv_pw1_glu", g, EPI_GLU, m.layers[l].cv_ng, m.layers[l].cv_nb, false); }   // LN + pointwise conv 1 + GLU
    void resid(const char *name, const float *A, const float *W, const float *bias, const float *Model::SigW::*w, int l) {   // x += A W^T + bias
        GemmArgs g{A, d, W, d, bias, x, d, x, d, 1.0f, (int)rows, d, d};
        g.a_bf16 = mode.ctx_bf16;
        attach(g, w, l);
        m.run_gemm(name, g, EPI_RESID, s);
    }
    void att_out(int l, const float *ctx) { resid("attn_out_resid", ctx, m.layers[l].wo, m.layers[l].bo, &Model::SigW::wo, l); }
    void pw2(int l, const float *dwb) { resid("conv_pw2_resid", dwb, m.layers[l].pw2_w, m.layers[l].pw2_b, &Model::SigW::pw2, l); }
    // final_norm_ of block l (:202).  next_runs: block l + 1 follows, and the norm goes with its ffn1 norm (:40) in one pass over the rows -- or, when
    // that block's fc1 folds its own norm, rides in front of it (GemmArgs::pre_g: the product normalises twice and its first column tiles write the
    // normalised rows -- the next block's residual stream -- into the other of two buffers; fp32: bit for bit the separate launch).  Else alone, -> x_home.
    void end_block(int l, bool next_runs) {
        const LayerW &L = m.layers[l];
        bool next_folds = false, rides = false;
        if (next_runs) {
            GemmArgs fg = fc1_folded(l + 1);
            next_folds = ln_folds(mode, fg, EPI_SILU);
            fg.pre_g = L.fin_g; fg.pre_b = L.fin_b; fg.pre_out = other(); fg.pre_ldo = d;
            rides = next_folds && mode.x_other && (mode.bf16 ? gemm_smallm_bf16_pre_applies(fg, EPI_SILU) : gemm_smallm_pre_applies(fg, EPI_SILU));
        }
        if (next_runs && !next_folds) {
            timed(3.0 * rows * d * 4, [&] { launch_layernorm2(x, rows, d, L.fin_g, L.fin_b, m.layers[l + 1].ffn1_ng, m.layers[l + 1].ffn1_nb, 1e-5f, x, n, s, mode.act_mode()); });
            norm_done = true;
        } else if (rides) {
            pend_g = L.fin_g; pend_b = L.fin_b;           // (consumed by the next ffn1 fc1: ln_gemm)
        } else {
            timed(2.0 * rows * d * 4, [&] { launch_layernorm(x, rows, d, L.fin_g, L.fin_b, 1e-5f, x_home, s); });
            x = x_home;
        }
    }
};

}  // namespace pk
