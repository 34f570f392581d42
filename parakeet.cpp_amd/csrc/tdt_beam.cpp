// parakeet.cpp_amd/csrc/tdt_beam.cpp -- sizes and runs the TDT beam search: the host loop of per-step launches and its scratch.
#include "tdt_beam.hpp"

#include <algorithm>

#include "engine.hpp"

namespace pk {

pk_tdt_beam_options tdt_beam_options_of(const pk_tdt_beam_options *opt) {
    pk_tdt_beam_options o;
    pk_tdt_beam_options_default(&o);
    if (opt) o = *opt;
    return o;
}

void tdt_beam_model_checks(const Model &m, const pk_tdt_beam_options &o) {
    if (m.cfg.vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no prediction net / joint (encoder-only configuration): TDT beam search needs a TDT joint");
    if (m.cfg.rnnt_head || m.cfg.num_durations <= 0)
        fail(PK_ERR_UNSUPPORTED, "TDT beam search needs a TDT joint (label + duration heads): this model has an RNN-T head");
    if (m.cfg.gemm_bf16) fail(PK_ERR_UNSUPPORTED, "TDT beam search has no gemm_bf16 form: the decode weights of this model exist only rounded to bf16");
    if (m.boost_on) fail(PK_ERR_UNSUPPORTED, "TDT beam search has no phrase-boosted variant: clear the boost phrases of the model first");
    if (m.cfg.num_durations > 8) fail(PK_ERR_UNSUPPORTED, "TDT beam search: %d durations, the kernel is built for 1 to 8", m.cfg.num_durations);
    if (m.cfg.vocab_size < 2) fail(PK_ERR_UNSUPPORTED, "TDT beam search: a vocabulary of the blank alone");
    if (o.beam_width < 1 || o.beam_width > kTdtBeamMaxWidth) fail(PK_ERR_UNSUPPORTED, "TDT beam search: beam_width %d outside 1..%d", o.beam_width, kTdtBeamMaxWidth);
    if (o.label_prune < 1 || o.label_prune > kTdtBeamMaxLabels) fail(PK_ERR_UNSUPPORTED, "TDT beam search: label_prune %d outside 1..%d", o.label_prune, kTdtBeamMaxLabels);
    if (o.duration_prune < 1 || o.duration_prune > kTdtBeamMaxDurs)
        fail(PK_ERR_UNSUPPORTED, "TDT beam search: duration_prune %d outside 1..%d", o.duration_prune, kTdtBeamMaxDurs);
    if (o.n_best < 1 || o.n_best > o.beam_width) fail(PK_ERR_UNSUPPORTED, "TDT beam search: n_best %d outside 1..beam_width", o.n_best);
}

size_t tdt_beam_scratch(const Model &m, int B, int t_max, int W, int K, int Kd, int N, int max_tokens, bool fused) {
    const pk_config &c = m.cfg;
    const size_t R = (size_t)B * W, C = (size_t)(K + 1) * Kd, cap = (size_t)t_max + max_tokens, MT = (size_t)max_tokens;
    size_t n = 2 * R * (36 + 4 * MT);
    n += R * (8 * (size_t)(K + 1) + 8 * (size_t)Kd + 4 * C);
    n += cap * R * 16;
    n += (6 * (size_t)c.num_lstm_layers * R * c.pred_hidden + 3 * R * c.joint_hidden) * 4;
    n += R * ((size_t)c.joint_hidden + c.vocab_size + c.num_durations) * 4;
    n += (size_t)B * N * (5 * MT + 2) * 4 + (4 * (size_t)B + cap + 1) * 4;
    if (fused) n += 2 * R * 8 + R * 8 * (size_t)(K + 1) + (size_t)B * N * 4;
    return n;
}

void tdt_beam_plan(TdtBeamWs &ws, const Model &m, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options &o, int max_tokens, bool fused) {
    const int V = m.cfg.vocab_size, D = m.cfg.num_durations;
    const int K = std::min<int>(o.label_prune, V - 1), Kd = std::min<int>(o.duration_prune, D);
    int t_max = 0;
    int64_t rows = 0;
    std::vector<int32_t> tab(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        const int Tb = n_frames ? n_frames[b] : T;
        tab[b] = Tb; tab[B + b] = (int32_t)rows;
        rows += Tb; t_max = std::max(t_max, Tb);
        if (rows >= ((int64_t)1 << 31)) fail(PK_ERR_INVALID, "too many frames");
    }
    // (every factor is bounded first: the byte count below then stays far from overflow)
    if ((int64_t)max_tokens > ((int64_t)1 << 24) || (int64_t)B * o.beam_width > ((int64_t)1 << 24) ||
        tdt_beam_scratch(m, B, t_max, o.beam_width, K, Kd, o.n_best, max_tokens, fused) > kTdtBeamMaxScratch)
        fail(PK_ERR_UNSUPPORTED, "TDT beam search: the scratch of this call (beam, back-pointers, state, products) exceeds the cap of %zu bytes", kTdtBeamMaxScratch);
    ws.h_tab.swap(tab);
    ws.B = B; ws.W = o.beam_width; ws.K = K; ws.Kd = Kd; ws.N = o.n_best; ws.max_tokens = max_tokens; ws.t_max = t_max; ws.cap = t_max + max_tokens;
    ws.fused = fused;
}

TdtBeamDev TdtBeamWs::dev(const Model &m) const {
    const pk_config &c = m.cfg;
    TdtBeamDev a{};
    a.B = B; a.W = W; a.K = K; a.Kd = Kd; a.N = N; a.V = c.vocab_size; a.D = c.num_durations; a.blank = c.blank_id; a.max_tokens = max_tokens;
    a.J = c.joint_hidden; a.L = c.num_lstm_layers; a.Hp = c.pred_hidden;
    for (int i = 0; i < 8; ++i) a.durations[i] = i < a.D ? c.durations[i] : 0;
    const size_t R = (size_t)B * W;
    a.T = tab.as<int>(); a.row0 = a.T + B;
    int *iv = ints.as<int>();
    a.valid = iv; a.t = iv + 2 * R; a.len = iv + 4 * R; a.par = iv + 6 * R; a.born = iv + 8 * R; a.tok = iv + 10 * R;
    a.score = score.as<float>(); a.hash = hash.as<unsigned long long>(); a.prefix = prefix.as<int>();
    a.lab_id = lab_id.as<int>(); a.lab_lp = lab_lp.as<float>(); a.dur_i = dur_i.as<int>(); a.dur_lp = dur_lp.as<float>(); a.cand = cand.as<float>();
    a.bp = bp.as<int4>();
    a.live = ctl.as<int>(); a.steps_done = a.live + B; a.live_total = a.live + 2 * (size_t)B;
    const size_t hs = (size_t)a.L * R * a.Hp, ps = R * a.J;
    float *f = state.as<float>();
    a.hG[0] = f; a.hG[1] = f + hs; a.hN = f + 2 * hs; a.cG[0] = f + 3 * hs; a.cG[1] = f + 4 * hs; a.cN = f + 5 * hs;
    f += 6 * hs;
    a.ppG[0] = f; a.ppG[1] = f + ps; a.ppN = f + 2 * ps;
    if (fused) {
        a.lmstate = lmslot.as<int>(); a.lm = reinterpret_cast<float *>(a.lmstate + 2 * R);
        a.lab_ls = lmlab.as<int>(); a.lab_lm = reinterpret_cast<float *>(a.lab_ls + R * (K + 1));
    }
    return a;
}

TdtBeamOut TdtBeamWs::out_view() const {
    const size_t tok = (size_t)B * N * max_tokens, hy = (size_t)B * N;
    TdtBeamOut o{};
    int *p = out.as<int>();
    o.ids = p; o.start = p + tok; o.end = p + 2 * tok; o.dur_idx = p + 3 * tok; o.conf = reinterpret_cast<float *>(p + 4 * tok);
    o.lens = p + 5 * tok; o.score = reinterpret_cast<float *>(p + 5 * tok + hy); o.ok = p + 5 * tok + 2 * hy;
    if (fused) o.lm_score = reinterpret_cast<float *>(o.ok + B);
    return o;
}

void run_tdt_beam(Model &m, TdtBeamWs &ws, const float *d_ep, hipStream_t s, const LmDev *lm) {
    if ((lm != nullptr) != ws.fused) fail(PK_ERR_INVALID, "internal error: run_tdt_beam and tdt_beam_plan disagree about the language model");
    const pk_config &c = m.cfg;
    const int B = ws.B, W = ws.W, K = ws.K, Kd = ws.Kd, N = ws.N, MT = ws.max_tokens, cap = ws.cap;
    const int V = c.vocab_size, D = c.num_durations, J = c.joint_hidden, L = c.num_lstm_layers, Hp = c.pred_hidden;
    const size_t R = (size_t)B * W, C = (size_t)(K + 1) * Kd;
    ws.tab.reserve(ws.h_tab.size() * 4);
    ws.ints.reserve(12 * R * 4); ws.score.reserve(2 * R * 4); ws.hash.reserve(2 * R * 8); ws.prefix.reserve(2 * R * MT * 4);
    ws.lab_id.reserve(R * (K + 1) * 4); ws.lab_lp.reserve(R * (K + 1) * 4); ws.dur_i.reserve(R * Kd * 4); ws.dur_lp.reserve(R * Kd * 4);
    ws.cand.reserve(R * C * 4);
    ws.bp.reserve((size_t)cap * R * 16);
    ws.ctl.reserve((2 * (size_t)B + cap + 1) * 4);
    const size_t hs = (size_t)L * R * Hp, ps = R * J;
    ws.state.reserve((6 * hs + 3 * ps) * 4);
    ws.z.reserve(R * J * 4); ws.logits.reserve(R * (size_t)(V + D) * 4);
    const size_t tok = (size_t)B * N * MT, hy = (size_t)B * N;
    ws.out.reserve((5 * tok + 2 * hy + B + (lm ? hy : 0)) * 4);
    if (lm) { ws.lmslot.reserve(4 * R * 4); ws.lmlab.reserve(2 * R * (K + 1) * 4); }
    TdtBeamDev a = ws.dev(m);
    if (lm) a.ngram = *lm;
    const TdtBeamOut o = ws.out_view();
    PK_HIP(hipMemcpyAsync(ws.tab.p, ws.h_tab.data(), ws.h_tab.size() * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemsetAsync(ws.ctl.p, 0, (2 * (size_t)B + cap + 1) * 4, s));
    PK_HIP(hipMemsetAsync(ws.state.p, 0, (6 * hs + 3 * ps) * 4, s));     // (step 0 gathers the zero state from copy 1)
    PK_HIP(hipMemsetAsync(ws.z.p, 0, R * J * 4, s));                      // (rows that are not live take part in the products: keep them finite)
    PK_HIP(hipMemsetAsync(ws.out.p, 0, 5 * tok * 4, s));
    launch_tdt_beam_init(a, s);
    int step = 0, live = B;
    while (step < cap && live > 0) {
        const int g = std::min(kTdtBeamGroupSteps, cap - step);
        for (int k = 0; k < g; ++k, ++step) {
            const int p = step & 1;
            launch_tdt_beam_gather(a, step, s);
            // one prediction-net step of every row on its gathered state (run_tdt_align_pred's launches): a row born from a label arc consumes its token,
            // the others the blank, and nobody reads their output
            for (int l = 0; l < L; ++l) {
                SkinnyArgs k1{};
                const size_t off = (size_t)l * R * Hp;
                k1.X = a.hG[p] + off; k1.W = m.dec_whh_s[l]; k1.B = (int)R; k1.N = 4 * Hp; k1.K = Hp; k1.out = a.hN + off; k1.c = a.cG[p] + off; k1.cn = a.cN + off;
                k1.Hp = Hp; k1.gi_ld = 4 * Hp;
                if (l == 0) { k1.gi = m.dec.g1; k1.gi_row = a.tok + (size_t)p * R; }
                else { k1.X2 = a.hN + off - R * Hp; k1.W2 = m.dec_wih_s[l]; k1.bias2 = m.dec.bih[l]; }
                launch_skinny_gemm(k1, SK_CELL, s);
            }
            SkinnyArgs k2{};
            k2.X = a.hN + (size_t)(L - 1) * R * Hp; k2.W = m.dec_wp_s; k2.B = (int)R; k2.N = J; k2.K = Hp; k2.bias = m.dec.bp; k2.out = a.ppN; k2.ldo = J;
            launch_skinny_gemm(k2, SK_BIAS, s);
            launch_tdt_beam_act(a, step, d_ep, ws.z.as<float>(), s);
            GemmArgs gm{ws.z.as<float>(), J, m.wld, J, m.bld, ws.logits.as<float>(), V + D, nullptr, 0, 1.0f, (int)R, V + D, J};
            m.run_gemm("tdt_beam_heads", gm, EPI_NONE, s, /*fp32_weight=*/true);
            launch_tdt_beam_expand(a, step, ws.logits.as<float>(), s);
            launch_tdt_beam_prune(a, step, s);
        }
        PK_HIP(hipMemcpyAsync(&live, a.live_total + step, sizeof(int), hipMemcpyDeviceToHost, s));
        PK_HIP(hipStreamSynchronize(s));
    }
    ws.steps_run = step;
    launch_tdt_beam_trace(a, o, s);
}

void tdt_beam_copy_out(const TdtBeamWs &ws, int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                       int32_t *ok, hipStream_t s, float *lm_score) {
    const size_t tok = (size_t)ws.B * ws.N * ws.max_tokens, hy = (size_t)ws.B * ws.N;
    const TdtBeamOut o = ws.out_view();
    if (ids) PK_HIP(hipMemcpyAsync(ids, o.ids, tok * 4, hipMemcpyDeviceToHost, s));
    if (start) PK_HIP(hipMemcpyAsync(start, o.start, tok * 4, hipMemcpyDeviceToHost, s));
    if (end) PK_HIP(hipMemcpyAsync(end, o.end, tok * 4, hipMemcpyDeviceToHost, s));
    if (dur_idx) PK_HIP(hipMemcpyAsync(dur_idx, o.dur_idx, tok * 4, hipMemcpyDeviceToHost, s));
    if (conf) PK_HIP(hipMemcpyAsync(conf, o.conf, tok * 4, hipMemcpyDeviceToHost, s));
    if (lens) PK_HIP(hipMemcpyAsync(lens, o.lens, hy * 4, hipMemcpyDeviceToHost, s));
    if (score) PK_HIP(hipMemcpyAsync(score, o.score, hy * 4, hipMemcpyDeviceToHost, s));
    if (ok) PK_HIP(hipMemcpyAsync(ok, o.ok, (size_t)ws.B * 4, hipMemcpyDeviceToHost, s));
    if (lm_score && o.lm_score) PK_HIP(hipMemcpyAsync(lm_score, o.lm_score, hy * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

size_t tdt_beam_bytes(const TdtBeamWs &ws) {
    size_t n = 0;
    for (const DevBuf *b : {&ws.tab, &ws.ints, &ws.score, &ws.hash, &ws.prefix, &ws.lab_id, &ws.lab_lp, &ws.dur_i, &ws.dur_lp, &ws.cand, &ws.bp, &ws.ctl, &ws.state,
                            &ws.z, &ws.logits, &ws.out, &ws.lmslot, &ws.lmlab})
        n += b->cap;
    return n;
}

}  // namespace pk
