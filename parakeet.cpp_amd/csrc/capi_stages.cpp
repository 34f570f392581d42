// parakeet.cpp_amd/csrc/capi_stages.cpp -- the stage entry points of the C boundary on caller buffers: mel, subsample, encode, conformer blocks,
// CTC / TDT decode and scoring (uniform and ragged forms), the CTC prefix and TDT beam searches, the CTC and TDT forced alignments and the CTC and TDT keyword spotting.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_util.hpp"

using namespace pk;

static void size_ws_for_T(Model &m, int B, int T) {
    // a mel length that subsamples to exactly T frames: Tm = 8(T-1)+1
    m.ws.size_for(m.cfg, B, 0, 8 * (T - 1) + 1);
    if (m.ws.T != T) fail(PK_ERR_INVALID, "internal: workspace T %d != %d", m.ws.T, T);
}

// workspace of the host-buffer decode entry points for B utterances of n_frames[b] encoder frames (packed); returns the longest
static int size_ws_for_frames(Model &m, const int32_t *n_frames, int B) {
    int t_max = 0;
    for (int i = 0; i < B; ++i) t_max = std::max(t_max, (int)n_frames[i]);
    RagBatch r;
    r.build_from_frames(n_frames, B, att_block_rows_of(m, t_max));
    m.ws.size_ragged(m.cfg, B, r.sum_T, t_max, false, /*level=*/2);
    m.ws.set_ragged(r, m.stream);
    return t_max;
}

// The uniform and the ragged form of a stage share one body: n_frames == nullptr is B utterances of T frames each, otherwise utterance b has
// n_frames[b] frames, packed.  Sizes the workspace; -> the longest utterance, and the frames of the batch in `rows`.
static int size_ws(Model &m, const int32_t *n_frames, int B, int T, size_t &rows) {
    if (n_frames) T = size_ws_for_frames(m, n_frames, B);
    else size_ws_for_T(m, B, T);
    rows = n_frames ? (size_t)m.ws.rag.sum_T : (size_t)B * T;
    return T;
}

namespace {

// The events of a _timed entry point: destroyed on every exit path.
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    void create() { for (auto &x : e) PK_HIP(hipEventCreate(&x)); }
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
float median_of(std::vector<float> &v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}
// Times S stages that follow each other on the model's stream.  queue(ev) queues them once and records ev[k] before stage k, ev[S] after the
// last.  reps + 1 passes, each waited for and checked; the first warms the buffers up and is not counted.  -> ms[k]: the median of stage k.
template <int S, class Queue>
void time_stages(Model &m, int reps, float *ms, Queue &&queue) {
    Events<S + 1> ev;
    ev.create();
    std::vector<float> t[S];
    for (int r = 0; r <= reps; ++r) {
        queue(ev.e);
        PK_HIP(hipStreamSynchronize(m.stream));
        PK_CHECK_LAUNCH();
        for (int k = 0; k < S; ++k) {
            float v = 0;
            PK_HIP(hipEventElapsedTime(&v, ev.e[k], ev.e[k + 1]));
            if (r > 0) t[k].push_back(v);
        }
    }
    for (int k = 0; k < S; ++k) ms[k] = median_of(t[k]);
}

// The log-prob rows of the entry points that take them from the host (pk_ctc_beam_search, pk_ctc_align, pk_ctc_kws): [B][T], or packed with
// n_frames[b] rows of utterance b.  Two halves, so that a caller can refuse (no device, a plan that does not fit) between them.
struct HostRows {
    int64_t rows = 0;                                              // frames of the batch
    int T = 0;                                                     // the longest utterance
    std::vector<int32_t> tab;                                      // ragged: T[B] then T_off[B + 1]
    DevBuf d_lp, d_tab;                                            // alive for the call

    // host only: checks n_frames, counts the rows and builds the table
    void plan(const int32_t *n_frames, int B, int T_uniform) {
        rows = (int64_t)B * T_uniform; T = T_uniform;
        if (!n_frames) return;
        tab.resize(2 * (size_t)B + 1);
        rows = 0; T = 0;
        for (int b = 0; b < B; ++b) {
            need(n_frames[b] > 0, "n_frames[b] must be positive");
            tab[b] = n_frames[b]; tab[B + b] = (int32_t)rows;
            rows += n_frames[b]; T = std::max(T, (int)n_frames[b]);
            need(rows < ((int64_t)1 << 31), "too many frames");
        }
        tab[2 * (size_t)B] = (int32_t)rows;
    }
    // uploads logp [rows][V] (-> d_lp) and the table; -> the ragged extents on the device (uniform: none)
    SeqRag upload(const float *logp, int B, int V) {
        d_lp.reserve((size_t)rows * V * 4);
        PK_HIP(hipMemcpy(d_lp.p, logp, (size_t)rows * V * 4, hipMemcpyHostToDevice));
        SeqRag rag;
        if (!tab.empty()) {
            d_tab.reserve(tab.size() * 4);
            PK_HIP(hipMemcpy(d_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            rag.T = d_tab.as<int>(); rag.T_off = rag.T + B; rag.T_max = T;
        }
        return rag;
    }
};

}  // namespace

static void conformer_blocks(Model &m, const float *x_in, const int32_t *n_frames, int B, int T, int first_layer, int n_layers, float *x_out) {
    m.require_gpu();
    need(first_layer >= 0 && n_layers >= 0 && first_layer + n_layers <= m.cfg.num_layers, "layer range");
    size_t rows;
    size_ws(m, n_frames, B, T, rows);
    const size_t n = rows * m.cfg.hidden_size;
    PK_HIP(hipMemcpyAsync(m.ws.x.p, x_in, n * 4, hipMemcpyHostToDevice, m.stream));
    if (n_layers > 0) m.run_layers(m.ws, B, first_layer, first_layer + n_layers, 0, m.stream);
    PK_CHECK_LAUNCH();
    PK_HIP(hipMemcpyAsync(x_out, m.ws.x.p, n * 4, hipMemcpyDeviceToHost, m.stream));
    PK_HIP(hipStreamSynchronize(m.stream));
}

// The token arrays of the decode that was just queued, [B][pitch] each (start / end / conf optional), then one more array the decoder has
// (CTC: the log-probs, TDT: the step counts; optional); waits for the stream and zeroes the entries past lens[b].
static void copy_out_tokens(Model &m, int B, int pitch, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf, void *extra,
                            const void *d_extra, size_t extra_bytes) {
    const size_t tok = (size_t)B * pitch;
    PK_HIP(hipMemcpyAsync(ids, m.ws.ids.p, tok * 4, hipMemcpyDeviceToHost, m.stream));
    PK_HIP(hipMemcpyAsync(lens, m.ws.lens.p, (size_t)B * 4, hipMemcpyDeviceToHost, m.stream));
    if (start) PK_HIP(hipMemcpyAsync(start, m.ws.start.p, tok * 4, hipMemcpyDeviceToHost, m.stream));
    if (end) PK_HIP(hipMemcpyAsync(end, m.ws.end.p, tok * 4, hipMemcpyDeviceToHost, m.stream));
    if (conf) PK_HIP(hipMemcpyAsync(conf, m.ws.conf.p, tok * 4, hipMemcpyDeviceToHost, m.stream));
    if (extra) PK_HIP(hipMemcpyAsync(extra, d_extra, extra_bytes, hipMemcpyDeviceToHost, m.stream));
    PK_HIP(hipStreamSynchronize(m.stream));
    zero_tail(ids, lens, B, pitch); zero_tail(start, lens, B, pitch); zero_tail(end, lens, B, pitch); zero_tail(conf, lens, B, pitch);
}

static void ctc_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end,
                       float *conf, float *logp) {
    m.require_gpu();
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);                          // the token arrays are [B][T], T = the longest utterance
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, logp != nullptr, m.stream);
    PK_CHECK_LAUNCH();
    copy_out_tokens(m, B, T, ids, lens, start, end, conf, logp, m.ws.ctc_lp.p, rows * m.cfg.ctc_vocab_size * 4);
}

// -> true when at least one utterance hit the safety cap on joint evaluations (lens[b] = -1)
static bool tdt_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                       int32_t *end, float *conf, int32_t *steps) {
    m.require_gpu();
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);
    need(max_tokens <= m.ws.max_tokens,
         n_frames ? "max_tokens exceeds (longest utterance) * max_symbols_per_step" : "max_tokens exceeds T * max_symbols_per_step");
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_tdt(m.ws, m.ws.x.as<float>(), B, T, max_tokens, m.stream);
    PK_CHECK_LAUNCH();
    copy_out_tokens(m, B, max_tokens, ids, lens, start, end, conf, steps, m.ws.ints.as<int>() + 4 * B, (size_t)B * 4);
    bool cap_hit = false;
    for (int b = 0; b < B; ++b) cap_hit = cap_hit || lens[b] < 0;
    return cap_hit;
}
// the status of a TDT decode entry point: a decode that ran but hit the cap is PK_ERR_DECODE_CAP (the arrays are filled all the same)
static pk_status tdt_status(pk_status st, bool cap_hit) {
    if (st != PK_OK || !cap_hit) return st;
    set_last_error("TDT decode hit the safety cap on joint evaluations for at least one utterance (lens = -1)");
    return PK_ERR_DECODE_CAP;
}

pk_beam_options pk::beam_options_of(const pk_beam_options *opt) {
    pk_beam_options o;
    pk_beam_options_default(&o);
    if (opt) o = *opt;
    return o;
}
// The model check of everything that walks the CTC head's rows (include/parakeet_amd.h: beam search, alignment, keyword spotting); -> the CTC vocabulary and
// its blank.  A boost trie does not matter to the alignment and the spotting: run_ctc writes the unboosted log-softmax rows, and those are what is walked.
static void ctc_head_of(const Model &m, const char *what, int &V, int &blank) {
    if (m.cfg.ctc_vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no ctc_decoder_ head: %s needs one", what);
    V = m.cfg.ctc_vocab_size;
    blank = m.cfg.blank_id < V ? m.cfg.blank_id : V - 1;           // (as Model::run_ctc)
}
// what the beam search's model entry points refuse (include/parakeet_amd.h)
void pk::beam_model_checks(Model &m, const pk_beam_options &o, int &V, int &blank) {
    m.require_gpu();
    ctc_head_of(m, "CTC beam search", V, blank);
    if (m.boost_on) fail(PK_ERR_UNSUPPORTED, "CTC beam search has no phrase-boosted variant: clear the boost phrases of the model first");
    beam_check_options(o, V, blank);
}

// fused: the _lm entry points (lm must be given), else lm / lm_opt / lm_score are not looked at
static void ctc_beam_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int32_t *ids, int32_t *lens,
                            float *score, int32_t *start, int32_t *end, float *conf, bool fused = false, const pk_lm *lm = nullptr,
                            const pk_lm_options *lm_opt = nullptr, float *lm_score = nullptr) {
    const pk_beam_options o = beam_options_of(opt);
    int V = 0, blank = 0;
    beam_model_checks(m, o, V, blank);
    LmDev lmd{};
    if (fused) {
        lm_fusion_checks(lm, lm_opt, V, blank);
        lmd = lm_device_view(lm, lm_opt);
    }
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);                          // the token arrays are [B][N][T], T = the longest utterance
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
    run_ctc_beam(m.beam, m.ws.ctc_lp.as<float>(), B, T, (int64_t)rows, n_frames ? m.ws.rv.seq : SeqRag(), V, blank, o, m.stream, fused ? &lmd : nullptr);
    PK_CHECK_LAUNCH();
    const bool ts = o.timestamps != 0;
    beam_copy_out(m.beam, ids, lens, score, ts ? start : nullptr, ts ? end : nullptr, ts ? conf : nullptr, m.stream, fused ? lm_score : nullptr);
}

static void ctc_align_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids, const int32_t *id_offsets,
                             int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok) {
    int V = 0, blank = 0;
    ctc_head_of(m, "CTC alignment", V, blank);
    align_check_args(ids, id_offsets, B, V, blank);
    if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    m.require_gpu();
    align_plan(m.align, n_frames, B, T, id_offsets);
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
    run_ctc_align(m.align, m.ws.ctc_lp.as<float>(), B, T, n_frames ? m.ws.rv.seq : SeqRag(), V, blank, ids, total != nullptr, m.stream);
    PK_CHECK_LAUNCH();
    align_copy_out(m.align, start, end, conf, score, total, ok, m.stream);
}

// Sizes the workspace for and queues one planned (tdt_align_checks) TDT alignment of enc (host rows, uniform or packed) on the model's stream; results stay in m.talign.
// ev (optional, 4 events): recorded before the prediction net, the lattice, the walk and after it.
static void tdt_align_queue(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids, bool walk,
                            hipEvent_t *ev = nullptr, bool upload_enc = true) {
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);
    if (upload_enc) PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    if (ev) PK_HIP(hipEventRecord(ev[0], m.stream));
    tdt_lattice_upload(m.talign, ids, m.stream, /*token_results=*/true);
    run_tdt_align_pred(m, m.talign, ids, m.stream);
    if (ev) PK_HIP(hipEventRecord(ev[1], m.stream));
    m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
    run_tdt_align_lattice(m, m.talign, m.ws.ep.as<float>(), m.stream);
    if (ev) PK_HIP(hipEventRecord(ev[2], m.stream));
    if (walk) run_tdt_align_dp(m.talign, m.stream);
    if (ev) PK_HIP(hipEventRecord(ev[3], m.stream));
}

static void tdt_align_checks(Model &m, const int32_t *n_frames, int B, int T, const int32_t *ids, const int32_t *id_offsets, int chunk_rows) {
    tdt_align_model_checks(m);
    align_check_args(ids, id_offsets, B, m.cfg.vocab_size, m.cfg.blank_id);
    if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    need(chunk_rows >= 0, "chunk_rows");
    m.require_gpu();
    tdt_align_plan(m.talign, n_frames, B, T, id_offsets, m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden, chunk_rows);
}

static void tdt_align_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids, const int32_t *id_offsets,
                             int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok) {
    tdt_align_checks(m, n_frames, B, T, ids, id_offsets, 0);
    tdt_align_queue(m, enc, n_frames, B, T, ids, true);
    PK_CHECK_LAUNCH();
    tdt_align_copy_out(m.talign, start, end, dur_idx, conf, score, ok, m.stream);
}

static void ctc_kws_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                           const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    const pk_kws_options o = kws_options_of(opt);
    int V = 0, blank = 0;
    ctc_head_of(m, "CTC keyword spotting", V, blank);
    kws_check_args(kw_ids, kw_offsets, n_kw, B, V, blank, o);
    if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    m.require_gpu();
    kws_plan(m.kws, n_frames, B, T, kw_offsets, n_kw, o);
    size_t rows;
    T = size_ws(m, n_frames, B, T, rows);
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
    run_ctc_kws(m.kws, m.ws.ctc_lp.as<float>(), B, T, n_frames ? m.ws.rv.seq : SeqRag(), V, blank, kw_ids, m.stream);
    PK_CHECK_LAUNCH();
    kws_copy_out(m.kws, n_hits, start, end, score, m.stream);
}

extern "C" {

pk_status pk_mel(pk_model *h, const float *pcm, int n_clips, int64_t n_samples, float *feats, float *logmel) {
    return guard([&] {
        need(h && pcm && feats && n_clips > 0, "model/pcm/feats/n_clips");
        need(n_samples > 256, "n_samples must exceed n_fft/2 (reflect padding)");
        Model &m = *h->m;
        m.require_gpu();
        const int nf = pk_mel_num_frames(n_samples), F = m.cfg.mel_bins;
        const size_t n_in = (size_t)n_clips * n_samples, n_lm = (size_t)n_clips * F * nf;
        const int pitch = mel_logmel_pitch(nf);                      // the device's log-mel rows are padded to 16 frames (kernels.hpp)
        m.io_in.reserve(n_in * 4);
        m.io_tmp.reserve((size_t)n_clips * F * pitch * 4);
        m.io_out.reserve(n_lm * 4);
        PK_HIP(hipMemcpyAsync(m.io_in.p, pcm, n_in * 4, hipMemcpyHostToDevice, m.stream));
        m.run_mel(m.io_in.as<float>(), n_clips, n_samples, m.io_tmp.as<float>(), m.io_out.as<float>(), m.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(feats, m.io_out.p, n_lm * 4, hipMemcpyDeviceToHost, m.stream));
        if (logmel) PK_HIP(hipMemcpy2DAsync(logmel, (size_t)nf * 4, m.io_tmp.p, (size_t)pitch * 4, (size_t)nf * 4, (size_t)n_clips * F, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}


pk_status pk_subsample(pk_model *h, const float *feats, int B, int Tm, float *out) {
    return guard([&] {
        need(h && feats && out && B > 0 && Tm > 0, "model/feats/out/B/Tm");
        Model &m = *h->m;
        m.require_gpu();
        m.ws.size_for(m.cfg, B, 0, Tm);
        const size_t nin = (size_t)B * Tm * m.cfg.mel_bins, nout = (size_t)B * m.ws.T * m.cfg.hidden_size;
        PK_HIP(hipMemcpyAsync(m.ws.feats.p, feats, nin * 4, hipMemcpyHostToDevice, m.stream));
        m.run_subsample(m.ws, m.ws.feats.as<float>(), B, Tm, m.ws.x.as<float>(), m.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(out, m.ws.x.p, nout * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

pk_status pk_encode(pk_model *h, const float *feats, int B, int Tm, int stop_layer, int stop_stage, float *enc) {
    return guard([&] {
        need(h && feats && enc && B > 0 && Tm > 0, "model/feats/enc/B/Tm");
        need(stop_stage >= 0 && stop_stage <= 4, "stop_stage");
        Model &m = *h->m;
        m.require_gpu();
        m.ws.size_for(m.cfg, B, 0, Tm);
        const size_t nin = (size_t)B * Tm * m.cfg.mel_bins, nout = (size_t)B * m.ws.T * m.cfg.hidden_size;
        PK_HIP(hipMemcpyAsync(m.ws.feats.p, feats, nin * 4, hipMemcpyHostToDevice, m.stream));
        m.run_encoder(m.ws, m.ws.feats.as<float>(), B, Tm, stop_layer, stop_stage, m.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(enc, m.ws.x.p, nout * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

pk_status pk_conformer_blocks(pk_model *h, const float *x_in, int B, int T, int first_layer, int n_layers, float *x_out) {
    return guard([&] {
        need(h && x_in && x_out && B > 0 && T > 0, "model/x_in/x_out/B/T");
        conformer_blocks(*h->m, x_in, nullptr, B, T, first_layer, n_layers, x_out);
    });
}

pk_status pk_ctc_decode(pk_model *h, const float *enc, int B, int T, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end,
                        float *conf, float *logp) {
    return guard([&] {
        need(h && enc && ids && lens && B > 0 && T > 0, "model/enc/ids/lens/B/T");
        ctc_decode(*h->m, enc, nullptr, B, T, ids, lens, start, end, conf, logp);
    });
}

pk_status pk_tdt_decode(pk_model *h, const float *enc, int B, int T, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                        int32_t *end, float *conf, int32_t *steps) {
    bool cap_hit = false;
    const pk_status st = guard([&] {
        need(h && enc && ids && lens && B > 0 && T > 0 && max_tokens > 0, "model/enc/ids/lens/B/T/max_tokens");
        cap_hit = tdt_decode(*h->m, enc, nullptr, B, T, max_tokens, ids, lens, start, end, conf, steps);
    });
    return tdt_status(st, cap_hit);
}

/* ---- ragged (mixed-length) forms of the stage entry points: every tensor PACKED along the time axis ---------------------------------- */
pk_status pk_mel_ragged(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, float *feats, float *logmel) {
    return guard([&] {
        need(h && pcm && offsets && feats && n_clips > 0, "model/pcm/offsets/feats/n_clips");
        Model &m = *h->m;
        m.require_gpu();
        std::vector<int64_t> lens(n_clips);
        int64_t longest = 0;
        for (int i = 0; i < n_clips; ++i) { lens[i] = offsets[i + 1] - offsets[i]; longest = std::max(longest, lens[i]); }
        RagBatch r;
        r.build_from_samples(lens.data(), n_clips, 32);
        m.ws.size_ragged(m.cfg, n_clips, r.n_samples, longest, /*own_pcm=*/true);
        m.ws.set_ragged(r, m.stream);
        const size_t n_lm = (size_t)r.sum_Tm * m.cfg.mel_bins;
        for (int i = 0; i < n_clips; ++i)        // (the clips need not be contiguous in the caller's buffer)
            PK_HIP(hipMemcpyAsync(m.ws.pcm.as<float>() + r.pcm_off[i], pcm + offsets[i], (size_t)lens[i] * 4, hipMemcpyHostToDevice, m.stream));
        m.run_mel_ws(m.ws, m.ws.pcm.as<float>(), n_clips, m.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(feats, m.ws.feats.p, n_lm * 4, hipMemcpyDeviceToHost, m.stream));
        if (logmel) {                                               // per clip: [mel_bins][pitch] on the device -> [mel_bins][Tm] for the caller
            const int F = m.cfg.mel_bins;
            size_t dev_off = 0, host_off = 0;
            for (int i = 0; i < n_clips; ++i) {
                const int tm = r.Tm[i], pitch = mel_logmel_pitch(tm);
                PK_HIP(hipMemcpy2DAsync(logmel + host_off, (size_t)tm * 4, m.ws.logmel.as<float>() + dev_off, (size_t)pitch * 4, (size_t)tm * 4, (size_t)F,
                                        hipMemcpyDeviceToHost, m.stream));
                dev_off += (size_t)F * pitch; host_off += (size_t)F * tm;
            }
        }
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

pk_status pk_encode_ragged(pk_model *h, const float *feats, const int32_t *n_mel_frames, int B, int stop_layer, int stop_stage, float *enc) {
    return guard([&] {
        need(h && feats && n_mel_frames && enc && B > 0, "model/feats/n_mel_frames/enc/B");
        need(stop_stage >= 0 && stop_stage <= 4, "stop_stage");
        Model &m = *h->m;
        m.require_gpu();
        int tm_max = 0;
        for (int i = 0; i < B; ++i) tm_max = std::max(tm_max, (int)n_mel_frames[i]);
        RagBatch r;
        r.build_from_mel(n_mel_frames, B, att_block_rows_of(m, pk_encoder_num_frames(tm_max)));
        m.ws.size_ragged(m.cfg, B, r.sum_Tm, tm_max, false, /*level=*/1);
        m.ws.set_ragged(r, m.stream);
        PK_HIP(hipMemcpyAsync(m.ws.feats.p, feats, (size_t)r.sum_Tm * m.cfg.mel_bins * 4, hipMemcpyHostToDevice, m.stream));
        m.run_encoder(m.ws, m.ws.feats.as<float>(), B, 0, stop_layer, stop_stage, m.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(enc, m.ws.x.p, (size_t)r.sum_T * m.cfg.hidden_size * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

pk_status pk_conformer_blocks_ragged(pk_model *h, const float *x_in, const int32_t *n_frames, int B, int first_layer, int n_layers, float *x_out) {
    return guard([&] {
        need(h && x_in && x_out && n_frames && B > 0, "model/x_in/x_out/n_frames/B");
        conformer_blocks(*h->m, x_in, n_frames, B, 0, first_layer, n_layers, x_out);
    });
}

pk_status pk_ctc_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, int32_t *ids, int32_t *lens, int32_t *start,
                               int32_t *end, float *conf, float *logp) {
    return guard([&] {
        need(h && enc && n_frames && ids && lens && B > 0, "model/enc/n_frames/ids/lens/B");
        ctc_decode(*h->m, enc, n_frames, B, 0, ids, lens, start, end, conf, logp);
    });
}

pk_status pk_tdt_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, int max_tokens, int32_t *ids, int32_t *lens,
                               int32_t *start, int32_t *end, float *conf, int32_t *steps) {
    bool cap_hit = false;
    const pk_status st = guard([&] {
        need(h && enc && n_frames && ids && lens && B > 0 && max_tokens > 0, "model/enc/n_frames/ids/lens/B/max_tokens");
        cap_hit = tdt_decode(*h->m, enc, n_frames, B, 0, max_tokens, ids, lens, start, end, conf, steps);
    });
    return tdt_status(st, cap_hit);
}

/* tdt_greedy_decode's loop (src/tdt.cpp:62-106) along a GIVEN decision path, recording the joint's outputs (TDTJoint::forward, :15-24) */
pk_status pk_tdt_score(pk_model *h, const float *enc, int T, const int32_t *labels, const int32_t *dur_idx, int n_steps, float *label_logp,
                       float *dur_logp, int *n_done) {
    return guard([&] {
        need(h && enc && labels && dur_idx && T > 0 && n_steps > 0 && (label_logp || dur_logp), "model/enc/labels/dur_idx/T/n_steps/outputs");
        Model &m = *h->m;
        m.require_gpu();
        need(m.cfg.vocab_size > 0 && !m.cfg.rnnt_head && m.cfg.num_durations > 0, "pk_tdt_score needs a TDT joint (label + duration heads)");
        const int V = m.cfg.vocab_size, D = m.cfg.num_durations;
        for (int k = 0; k < n_steps; ++k)
            need(labels[k] >= 0 && labels[k] < V && dur_idx[k] >= 0 && dur_idx[k] < D, "labels[k] / dur_idx[k] out of range");
        size_ws_for_T(m, 1, T);
        Workspace &w = m.ws;
        const size_t nl = (size_t)n_steps * V, nd = (size_t)n_steps * D;
        m.io_in.reserve((size_t)2 * n_steps * sizeof(int));
        m.io_out.reserve((nl + nd) * 4);
        int *d_lab = m.io_in.as<int>(), *d_dur = d_lab + n_steps;
        float *d_sl = m.io_out.as<float>(), *d_sd = d_sl + nl;
        PK_HIP(hipMemcpyAsync(d_lab, labels, (size_t)n_steps * 4, hipMemcpyHostToDevice, m.stream));
        PK_HIP(hipMemcpyAsync(d_dur, dur_idx, (size_t)n_steps * 4, hipMemcpyHostToDevice, m.stream));
        PK_HIP(hipMemsetAsync(d_sl, 0, (nl + nd) * 4, m.stream));
        PK_HIP(hipMemcpyAsync(w.x.p, enc, (size_t)T * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        struct Scope { Workspace &w; ~Scope() { w.force_label = w.force_dur = nullptr; w.score_lab = w.score_dur = nullptr; w.n_force = 0; } } scope{w};
        w.force_label = d_lab; w.force_dur = d_dur; w.n_force = n_steps; w.score_lab = d_sl; w.score_dur = d_sd;
        m.run_tdt(w, w.x.as<float>(), 1, T, w.max_tokens, m.stream);
        PK_CHECK_LAUNCH();
        int steps = 0;
        PK_HIP(hipMemcpyAsync(&steps, w.ints.as<int>() + 4, sizeof(int), hipMemcpyDeviceToHost, m.stream));      // st.steps[0] (B = 1)
        if (label_logp) PK_HIP(hipMemcpyAsync(label_logp, d_sl, nl * 4, hipMemcpyDeviceToHost, m.stream));
        if (dur_logp) PK_HIP(hipMemcpyAsync(dur_logp, d_sd, nd * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
        if (n_done) *n_done = steps;
    });
}

pk_status pk_decode_margins(pk_model *h, float *min_margin, int B) {
    return guard([&] {
        need(h && min_margin && B > 0, "model/min_margin/B");
        Model &m = *h->m;
        m.require_gpu();
        need(B <= m.ws.B && m.ws.margin.p, "B exceeds the last pk_tdt_decode call");
        need(!m.boost_on, "margins are reported for unboosted decodes");
        PK_HIP(hipMemcpy(min_margin, m.ws.margin.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    });
}

/* ---- CTC prefix beam search (kernels/ctc_beam.hip; reference roadmap README.md:494) ------------------------------------------------ */
void pk_beam_options_default(pk_beam_options *out) {
    if (!out) return;
    out->beam_width = 8; out->token_prune = 16; out->n_best = 1; out->timestamps = 0;
}

// the body of pk_ctc_beam_search and pk_ctc_beam_search_lm (fused: as ctc_beam_decode)
static pk_status ctc_beam_search(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const pk_beam_options *opt,
                                 int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, bool fused,
                                 const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(logp && ids && lens && B > 0, "logp/ids/lens/B");
        need(n_frames || T > 0, "T");
        const pk_beam_options o = beam_options_of(opt);
        beam_check_options(o, V, blank);
        if (fused) lm_fusion_checks(lm, lm_opt, V, blank);
        need_device();
        LmDev lmd{};
        if (fused) lmd = lm_device_view(lm, lm_opt);
        HostRows in;
        in.plan(n_frames, B, T);
        BeamWs ws;
        const SeqRag rag = in.upload(logp, B, V);
        run_ctc_beam(ws, in.d_lp.as<float>(), B, in.T, in.rows, rag, V, blank, o, nullptr, fused ? &lmd : nullptr);
        PK_CHECK_LAUNCH();
        const bool ts = o.timestamps != 0;
        beam_copy_out(ws, ids, lens, score, ts ? start : nullptr, ts ? end : nullptr, ts ? conf : nullptr, nullptr, fused ? lm_score : nullptr);
    });
}

pk_status pk_ctc_beam_search(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const pk_beam_options *opt,
                             int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf) {
    return ctc_beam_search(logp, n_frames, B, T, V, blank, opt, ids, lens, score, start, end, conf, false, nullptr, nullptr, nullptr);
}

pk_status pk_ctc_beam_search_lm(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const pk_beam_options *opt,
                                int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm,
                                const pk_lm_options *lm_opt, float *lm_score) {
    return ctc_beam_search(logp, n_frames, B, T, V, blank, opt, ids, lens, score, start, end, conf, true, lm, lm_opt, lm_score);
}

pk_status pk_ctc_beam_decode(pk_model *h, const float *enc, int B, int T, const pk_beam_options *opt, int32_t *ids, int32_t *lens,
                             float *score, int32_t *start, int32_t *end, float *conf) {
    return guard([&] {
        need(h && enc && ids && lens && B > 0 && T > 0, "model/enc/ids/lens/B/T");
        ctc_beam_decode(*h->m, enc, nullptr, B, T, opt, ids, lens, score, start, end, conf);
    });
}

pk_status pk_ctc_beam_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const pk_beam_options *opt, int32_t *ids,
                                    int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf) {
    return guard([&] {
        need(h && enc && n_frames && ids && lens && B > 0, "model/enc/n_frames/ids/lens/B");
        ctc_beam_decode(*h->m, enc, n_frames, B, 0, opt, ids, lens, score, start, end, conf);
    });
}

pk_status pk_ctc_beam_decode_lm(pk_model *h, const float *enc, int B, int T, const pk_beam_options *opt, int32_t *ids, int32_t *lens,
                                float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm, const pk_lm_options *lm_opt,
                                float *lm_score) {
    return guard([&] {
        need(h && enc && ids && lens && B > 0 && T > 0, "model/enc/ids/lens/B/T");
        ctc_beam_decode(*h->m, enc, nullptr, B, T, opt, ids, lens, score, start, end, conf, true, lm, lm_opt, lm_score);
    });
}

pk_status pk_ctc_beam_decode_lm_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const pk_beam_options *opt, int32_t *ids,
                                       int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm,
                                       const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(h && enc && n_frames && ids && lens && B > 0, "model/enc/n_frames/ids/lens/B");
        ctc_beam_decode(*h->m, enc, n_frames, B, 0, opt, ids, lens, score, start, end, conf, true, lm, lm_opt, lm_score);
    });
}

// the body of pk_ctc_beam_decode_timed and pk_ctc_beam_decode_lm_timed (fused: as ctc_beam_decode)
static pk_status ctc_beam_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int reps,
                                       float ms[2], bool fused, const pk_lm *lm, const pk_lm_options *lm_opt) {
    return guard([&] {
        need(h && enc && ms && B > 0 && reps > 0 && (n_frames || T > 0), "model/enc/ms/B/T/reps");
        Model &m = *h->m;
        const pk_beam_options o = beam_options_of(opt);
        int V = 0, blank = 0;
        beam_model_checks(m, o, V, blank);
        LmDev lmd{};
        if (fused) {
            lm_fusion_checks(lm, lm_opt, V, blank);
            lmd = lm_device_view(lm, lm_opt);
        }
        size_t rows;
        T = size_ws(m, n_frames, B, T, rows);
        const SeqRag rag = n_frames ? m.ws.rv.seq : SeqRag();
        PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        time_stages<2>(m, reps, ms, [&](hipEvent_t *ev) {          // the greedy head, the search
            PK_HIP(hipEventRecord(ev[0], m.stream));
            m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
            PK_HIP(hipEventRecord(ev[1], m.stream));
            run_ctc_beam(m.beam, m.ws.ctc_lp.as<float>(), B, T, (int64_t)rows, rag, V, blank, o, m.stream, fused ? &lmd : nullptr);
            PK_HIP(hipEventRecord(ev[2], m.stream));
        });
    });
}

pk_status pk_ctc_beam_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int reps,
                                   float ms[2]) {
    return ctc_beam_decode_timed(h, enc, n_frames, B, T, opt, reps, ms, false, nullptr, nullptr);
}

pk_status pk_ctc_beam_decode_lm_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int reps,
                                      float ms[2], const pk_lm *lm, const pk_lm_options *lm_opt) {
    return ctc_beam_decode_timed(h, enc, n_frames, B, T, opt, reps, ms, true, lm, lm_opt);
}

/* ---- TDT beam search (kernels/tdt_beam.hip; reference roadmap README.md:494) ----------------------------------------------------- */
void pk_tdt_beam_options_default(pk_tdt_beam_options *out) {
    if (!out) return;
    out->beam_width = 8; out->label_prune = 8; out->duration_prune = 2; out->n_best = 1;
}

// checks and sizes one search (host only: every refusal comes before anything is allocated).  fused: the _lm entry points (lm must be given;
// DESIGN.md section 5.5.7): what the unfused search refuses, then what lm_fusion_checks refuses; else lm / lm_opt are not looked at
static void tdt_beam_checks(Model &m, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options &o, int max_tokens, bool fused = false,
                            const pk_lm *lm = nullptr, const pk_lm_options *lm_opt = nullptr) {
    tdt_beam_model_checks(m, o);
    if (fused) lm_fusion_checks(lm, lm_opt, m.cfg.vocab_size, m.cfg.blank_id);
    if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    m.require_gpu();
    tdt_beam_plan(m.tbeam, m, n_frames, B, T, o, max_tokens, fused);
}

static void tdt_beam_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt, int max_tokens, int32_t *ids,
                            int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, int32_t *ok, bool fused = false,
                            const pk_lm *lm = nullptr, const pk_lm_options *lm_opt = nullptr, float *lm_score = nullptr) {
    const pk_tdt_beam_options o = tdt_beam_options_of(opt);
    tdt_beam_checks(m, n_frames, B, T, o, max_tokens, fused, lm, lm_opt);
    LmDev lmd{};
    if (fused) lmd = lm_device_view(lm, lm_opt);
    size_t rows;
    size_ws(m, n_frames, B, T, rows);
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
    run_tdt_beam(m, m.tbeam, m.ws.ep.as<float>(), m.stream, fused ? &lmd : nullptr);
    PK_CHECK_LAUNCH();
    tdt_beam_copy_out(m.tbeam, ids, lens, score, start, end, dur_idx, conf, ok, m.stream, fused ? lm_score : nullptr);
}

pk_status pk_tdt_beam_decode(pk_model *h, const float *enc, int B, int T, const pk_tdt_beam_options *opt, int max_tokens, int32_t *ids,
                             int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, int32_t *ok) {
    return guard([&] {
        need(h && enc && ids && lens && score && B > 0 && T > 0 && max_tokens > 0, "model/enc/ids/lens/score/B/T/max_tokens");
        tdt_beam_decode(*h->m, enc, nullptr, B, T, opt, max_tokens, ids, lens, score, start, end, dur_idx, conf, ok);
    });
}

pk_status pk_tdt_beam_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const pk_tdt_beam_options *opt, int max_tokens,
                                    int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                                    int32_t *ok) {
    return guard([&] {
        need(h && enc && n_frames && ids && lens && score && B > 0 && max_tokens > 0, "model/enc/n_frames/ids/lens/score/B/max_tokens");
        tdt_beam_decode(*h->m, enc, n_frames, B, 0, opt, max_tokens, ids, lens, score, start, end, dur_idx, conf, ok);
    });
}

pk_status pk_tdt_beam_decode_lm(pk_model *h, const float *enc, int B, int T, const pk_tdt_beam_options *opt, int max_tokens, int32_t *ids,
                                int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, int32_t *ok,
                                const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(h && enc && ids && lens && score && B > 0 && T > 0 && max_tokens > 0, "model/enc/ids/lens/score/B/T/max_tokens");
        tdt_beam_decode(*h->m, enc, nullptr, B, T, opt, max_tokens, ids, lens, score, start, end, dur_idx, conf, ok, true, lm, lm_opt, lm_score);
    });
}

pk_status pk_tdt_beam_decode_lm_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const pk_tdt_beam_options *opt, int max_tokens,
                                       int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                                       int32_t *ok, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(h && enc && n_frames && ids && lens && score && B > 0 && max_tokens > 0, "model/enc/n_frames/ids/lens/score/B/max_tokens");
        tdt_beam_decode(*h->m, enc, n_frames, B, 0, opt, max_tokens, ids, lens, score, start, end, dur_idx, conf, ok, true, lm, lm_opt, lm_score);
    });
}

static pk_status tdt_beam_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt,
                                       int max_tokens, int reps, float ms[2], bool fused, const pk_lm *lm, const pk_lm_options *lm_opt) {
    return guard([&] {
        need(h && enc && ms && B > 0 && reps > 0 && max_tokens > 0 && (n_frames || T > 0), "model/enc/ms/B/T/max_tokens/reps");
        Model &m = *h->m;
        const pk_tdt_beam_options o = tdt_beam_options_of(opt);
        tdt_beam_checks(m, n_frames, B, T, o, max_tokens, fused, lm, lm_opt);
        LmDev lmd{};
        if (fused) lmd = lm_device_view(lm, lm_opt);
        size_t rows;
        T = size_ws(m, n_frames, B, T, rows);
        PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        time_stages<2>(m, reps, ms, [&](hipEvent_t *ev) {          // the greedy decode, the search
            PK_HIP(hipEventRecord(ev[0], m.stream));
            m.run_tdt(m.ws, m.ws.x.as<float>(), B, T, m.ws.max_tokens, m.stream);
            PK_HIP(hipEventRecord(ev[1], m.stream));
            m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
            run_tdt_beam(m, m.tbeam, m.ws.ep.as<float>(), m.stream, fused ? &lmd : nullptr);
            PK_HIP(hipEventRecord(ev[2], m.stream));
        });
    });
}

pk_status pk_tdt_beam_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt,
                                   int max_tokens, int reps, float ms[2]) {
    return tdt_beam_decode_timed(h, enc, n_frames, B, T, opt, max_tokens, reps, ms, false, nullptr, nullptr);
}

pk_status pk_tdt_beam_decode_lm_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt,
                                      int max_tokens, int reps, float ms[2], const pk_lm *lm, const pk_lm_options *lm_opt) {
    return tdt_beam_decode_timed(h, enc, n_frames, B, T, opt, max_tokens, reps, ms, true, lm, lm_opt);
}

int pk_tdt_beam_last_steps(const pk_model *h) { return h && h->m ? h->m->tbeam.steps_run : 0; }

/* ---- CTC forced alignment of given token strings (kernels/ctc_align.hip) ------------------------------------------------------------ */
pk_status pk_ctc_align(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const int32_t *ids, const int32_t *id_offsets,
                       int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok) {
    return guard([&] {
        align_check_args(ids, id_offsets, B, V, blank);
        need(logp && score && ok, "logp/score/ok");
        need(id_offsets[B] == 0 || (start && end && conf), "start/end/conf");
        need(n_frames || T > 0, "T");
        HostRows in;
        in.plan(n_frames, B, T);
        need_device();
        AlignWs ws;
        align_plan(ws, n_frames, B, in.T, id_offsets);             // (refuses before anything is allocated)
        const SeqRag rag = in.upload(logp, B, V);
        run_ctc_align(ws, in.d_lp.as<float>(), B, in.T, rag, V, blank, ids, total != nullptr, nullptr);
        PK_CHECK_LAUNCH();
        align_copy_out(ws, start, end, conf, score, total, ok, nullptr);
    });
}

pk_status pk_ctc_align_decode(pk_model *h, const float *enc, int B, int T, const int32_t *ids, const int32_t *id_offsets, int32_t *start,
                              int32_t *end, float *conf, float *score, float *total, int32_t *ok) {
    return guard([&] {
        need(h && enc && score && ok && T > 0, "model/enc/score/ok/T");
        ctc_align_decode(*h->m, enc, nullptr, B, T, ids, id_offsets, start, end, conf, score, total, ok);
    });
}

pk_status pk_ctc_align_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                                     int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok) {
    return guard([&] {
        need(h && enc && n_frames && score && ok, "model/enc/n_frames/score/ok");
        ctc_align_decode(*h->m, enc, n_frames, B, 0, ids, id_offsets, start, end, conf, score, total, ok);
    });
}

pk_status pk_ctc_align_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids,
                                    const int32_t *id_offsets, int want_total, int reps, float ms[2]) {
    return guard([&] {
        need(h && enc && ms && reps > 0 && (n_frames || T > 0), "model/enc/ms/T/reps");
        Model &m = *h->m;
        int V = 0, blank = 0;
        ctc_head_of(m, "CTC alignment", V, blank);
        align_check_args(ids, id_offsets, B, V, blank);
        if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
        m.require_gpu();
        align_plan(m.align, n_frames, B, T, id_offsets);
        size_t rows;
        T = size_ws(m, n_frames, B, T, rows);
        const SeqRag rag = n_frames ? m.ws.rv.seq : SeqRag();
        PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        time_stages<2>(m, reps, ms, [&](hipEvent_t *ev) {          // the head, the alignment
            PK_HIP(hipEventRecord(ev[0], m.stream));
            m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
            PK_HIP(hipEventRecord(ev[1], m.stream));
            run_ctc_align(m.align, m.ws.ctc_lp.as<float>(), B, T, rag, V, blank, ids, want_total != 0, m.stream);
            PK_HIP(hipEventRecord(ev[2], m.stream));
        });
    });
}

/* ---- TDT forced alignment of given token strings (kernels/tdt_align.hip) ------------------------------------------------------------ */
// The walks alone on a HOST lattice (pk_tdt_align here, pk_tdt_total below) share two halves; the entry point's own output checks run between them, where they
// always ran.  The first: the argument checks on the tables.
static void tdt_host_lattice_checks(const int32_t *durations, const int32_t *n_frames, int B, const int32_t *id_offsets) {
    need(B >= 1 && id_offsets && n_frames && durations, "B/id_offsets/n_frames/durations");
    need(id_offsets[0] == 0, "id_offsets[0] must be 0");
    for (int b = 0; b < B; ++b) {
        need(id_offsets[b + 1] >= id_offsets[b], "id_offsets decrease");
        need(n_frames[b] > 0, "n_frames[b] must be positive");
    }
}
// The second: the plan -- host only: it refuses before a device is looked for or anything is allocated --, then the upload of the tables and of the three
// lattice arrays on the null stream.
static void tdt_host_lattice_stage(TdtAlignWs &ws, const float *lab, const float *blk, const float *dl, const int32_t *durations, int D,
                                   const int32_t *n_frames, int B, const int32_t *id_offsets, bool back_pointers, const char *what) {
    tdt_lattice_plan(ws, n_frames, nullptr, B, 0, id_offsets, durations, D, 0, 0, 0, back_pointers, what);
    need_device();
    tdt_lattice_upload(ws, nullptr, nullptr, /*token_results=*/back_pointers);
    if (ws.labs) PK_HIP(hipMemcpyAsync(ws.lab.p, lab, (size_t)ws.labs * 4, hipMemcpyHostToDevice, nullptr));
    PK_HIP(hipMemcpyAsync(ws.blk.p, blk, (size_t)ws.cells * 4, hipMemcpyHostToDevice, nullptr));
    PK_HIP(hipMemcpyAsync(ws.dl.p, dl, (size_t)ws.cells * D * 4, hipMemcpyHostToDevice, nullptr));
}

pk_status pk_tdt_align(const float *lab, const float *blk, const float *dl, const int32_t *durations, int D, const int32_t *n_frames, int B,
                       const int32_t *id_offsets, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok) {
    return guard([&] {
        tdt_host_lattice_checks(durations, n_frames, B, id_offsets);
        need(blk && dl && score && ok, "blk/dl/score/ok");
        need(id_offsets[B] == 0 || (lab && start && end && dur_idx && conf), "lab/start/end/dur_idx/conf");
        TdtAlignWs ws;
        tdt_host_lattice_stage(ws, lab, blk, dl, durations, D, n_frames, B, id_offsets, /*back_pointers=*/true, "TDT alignment");
        run_tdt_align_dp(ws, nullptr);
        PK_CHECK_LAUNCH();
        tdt_align_copy_out(ws, start, end, dur_idx, conf, score, ok, nullptr);
    });
}

pk_status pk_tdt_align_decode(pk_model *h, const float *enc, int B, int T, const int32_t *ids, const int32_t *id_offsets, int32_t *start,
                              int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok) {
    return guard([&] {
        need(h && enc && score && ok && T > 0, "model/enc/score/ok/T");
        tdt_align_decode(*h->m, enc, nullptr, B, T, ids, id_offsets, start, end, dur_idx, conf, score, ok);
    });
}

pk_status pk_tdt_align_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *ids,
                                     const int32_t *id_offsets, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score,
                                     int32_t *ok) {
    return guard([&] {
        need(h && enc && n_frames && score && ok, "model/enc/n_frames/score/ok");
        tdt_align_decode(*h->m, enc, n_frames, B, 0, ids, id_offsets, start, end, dur_idx, conf, score, ok);
    });
}

pk_status pk_tdt_align_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids,
                                    const int32_t *id_offsets, int reps, float ms[4]) {
    return guard([&] {
        need(h && enc && ms && reps > 0 && (n_frames || T > 0), "model/enc/ms/T/reps");
        Model &m = *h->m;
        tdt_align_checks(m, n_frames, B, T, ids, id_offsets, 0);
        bool first = true;                                         // enc is uploaded by the first pass alone
        time_stages<3>(m, reps, ms, [&](hipEvent_t *ev) {          // the prediction net, the lattice, the walk
            tdt_align_queue(m, enc, n_frames, B, T, ids, true, ev, first);
            first = false;
        });
        // the heads product of ONE chunk alone (the rows the last pass left in the activation buffer), for the lattice stage's overhead over it
        const int n = (int)std::min<int64_t>(m.talign.chunk_rows, m.talign.cells);
        time_stages<1>(m, reps, ms + 3, [&](hipEvent_t *ev) {
            PK_HIP(hipEventRecord(ev[0], m.stream));
            run_tdt_align_heads(m, m.talign, n, m.stream);
            PK_HIP(hipEventRecord(ev[1], m.stream));
        });
    });
}

pk_status pk_diag_tdt_lattice(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                              int chunk_rows, float *lab, float *blk, float *dl) {
    return guard([&] {
        need(h && enc && n_frames && lab && blk && dl, "model/enc/n_frames/lab/blk/dl");
        Model &m = *h->m;
        tdt_align_checks(m, n_frames, B, 0, ids, id_offsets, chunk_rows);
        TdtAlignWs &ws = m.talign;
        const size_t G = PK_DIAG_TDT_LATTICE_GUARD, nl = (size_t)ws.labs + G, nb = (size_t)ws.cells + G, nd = (size_t)ws.cells * ws.D + G;
        ws.lab.reserve(nl * 4); ws.blk.reserve(nb * 4); ws.dl.reserve(nd * 4);
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.lab.p, 0x7FC5A5A5, nl, m.stream));
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.blk.p, 0x7FC5A5A5, nb, m.stream));
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.dl.p, 0x7FC5A5A5, nd, m.stream));
        tdt_align_queue(m, enc, n_frames, B, 0, ids, /*walk=*/false);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(lab, ws.lab.p, nl * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipMemcpyAsync(blk, ws.blk.p, nb * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipMemcpyAsync(dl, ws.dl.p, nd * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

}  // extern "C"

/* ---- the forward-algorithm total of given token strings under the TDT head (kernels/tdt_total.hip) ------------------------------------ */
// the argument checks of the model entry points; -> after them the call is planned (host only) in m.ttotal
static void tdt_total_checks(Model &m, const int32_t *n_frames, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets, const int32_t *clip_of,
                             int n_hyp) {
    tdt_align_model_checks(m);
    need(n_clips >= 1 && n_hyp >= 1, "n_clips/n_hyp");
    if (clip_of) for (int h = 0; h < n_hyp; ++h) need(clip_of[h] >= 0 && clip_of[h] < n_clips, "clip_of[h] outside [0, n_clips)");
    else need(n_hyp == n_clips, "clip_of == NULL needs n_hyp == n_clips");
    align_check_args(ids, id_offsets, n_hyp, m.cfg.vocab_size, m.cfg.blank_id);
    if (n_frames) for (int b = 0; b < n_clips; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    m.require_gpu();
    tdt_total_plan_call(m, m.ttotal, n_frames, n_clips, T, id_offsets, clip_of, n_hyp);
}

// uploads enc, runs enc_proj ONCE over the clips' rows, then the planned groups
static void tdt_total_run(Model &m, const float *enc, const int32_t *n_frames, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets,
                          hipEvent_t *ev = nullptr, float *ms = nullptr) {
    size_t rows;
    size_ws(m, n_frames, n_clips, T, rows);
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
    run_tdt_total_call(m, m.ttotal, m.ws.ep.as<float>(), ids, id_offsets, ev, ms);
    PK_CHECK_LAUNCH();
}

static void tdt_total_decode(Model &m, const float *enc, const int32_t *n_frames, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets,
                             const int32_t *clip_of, int n_hyp, float *total, int32_t *ok) {
    tdt_total_checks(m, n_frames, n_clips, T, ids, id_offsets, clip_of, n_hyp);
    tdt_total_run(m, enc, n_frames, n_clips, T, ids, id_offsets);
    std::copy(m.ttotal.total.begin(), m.ttotal.total.end(), total);
    std::copy(m.ttotal.ok.begin(), m.ttotal.ok.end(), ok);
}

extern "C" {

pk_status pk_tdt_total(const float *lab, const float *blk, const float *dl, const int32_t *durations, int D, const int32_t *n_frames, int B,
                       const int32_t *id_offsets, float *total, int32_t *ok) {
    return guard([&] {
        tdt_host_lattice_checks(durations, n_frames, B, id_offsets);
        need(blk && dl && total && ok, "blk/dl/total/ok");
        need(id_offsets[B] == 0 || lab, "lab");
        TdtAlignWs ws;
        tdt_host_lattice_stage(ws, lab, blk, dl, durations, D, n_frames, B, id_offsets, /*back_pointers=*/false, "TDT total");
        run_tdt_total_dp(ws, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(total, ws.out.p, (size_t)B * 4, hipMemcpyDeviceToHost, nullptr));
        PK_HIP(hipMemcpyAsync(ok, ws.out.as<int>() + B, (size_t)B * 4, hipMemcpyDeviceToHost, nullptr));
        PK_HIP(hipStreamSynchronize(nullptr));
    });
}

pk_status pk_tdt_total_decode(pk_model *h, const float *enc, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets, const int32_t *clip_of,
                              int n_hyp, float *total, int32_t *ok) {
    return guard([&] {
        need(h && enc && total && ok && T > 0, "model/enc/total/ok/T");
        tdt_total_decode(*h->m, enc, nullptr, n_clips, T, ids, id_offsets, clip_of, n_hyp, total, ok);
    });
}

pk_status pk_tdt_total_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int n_clips, const int32_t *ids, const int32_t *id_offsets,
                                     const int32_t *clip_of, int n_hyp, float *total, int32_t *ok) {
    return guard([&] {
        need(h && enc && n_frames && total && ok, "model/enc/n_frames/total/ok");
        tdt_total_decode(*h->m, enc, n_frames, n_clips, 0, ids, id_offsets, clip_of, n_hyp, total, ok);
    });
}

pk_status pk_tdt_total_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int n_clips, int T, const int32_t *ids,
                                    const int32_t *id_offsets, const int32_t *clip_of, int n_hyp, int reps, float ms[3]) {
    return guard([&] {
        need(h && enc && ms && reps > 0 && (n_frames || T > 0), "model/enc/ms/T/reps");
        Model &m = *h->m;
        tdt_total_checks(m, n_frames, n_clips, T, ids, id_offsets, clip_of, n_hyp);
        Events<4> ev;
        ev.create();
        std::vector<float> t[3];
        for (int r = 0; r <= reps; ++r) {                          // (the first pass warms the buffers up and is not counted)
            float v[3] = {0, 0, 0};                                // per stage, summed over the groups of the call: not time_stages' one pass of events
            tdt_total_run(m, enc, n_frames, n_clips, T, ids, id_offsets, ev.e, v);
            if (r > 0) for (int k = 0; k < 3; ++k) t[k].push_back(v[k]);
        }
        for (int k = 0; k < 3; ++k) ms[k] = median_of(t[k]);
    });
}

pk_status pk_diag_tdt_total_groups(const int32_t *n_frames_of_hyp, const int32_t *id_offsets, int n_hyp, const int32_t *durations, int D, int V, int J,
                                   int max_hyps, int32_t *group_of, int *n_groups) {
    return guard([&] {
        need(n_frames_of_hyp && id_offsets && durations && group_of && n_hyp >= 1, "n_frames_of_hyp/id_offsets/durations/group_of/n_hyp");
        need(id_offsets[0] == 0 && V >= 0 && J >= 0, "id_offsets[0]/V/J");
        for (int b = 0; b < n_hyp; ++b) {
            need(id_offsets[b + 1] >= id_offsets[b], "id_offsets decrease");
            need(n_frames_of_hyp[b] > 0, "n_frames_of_hyp[b] must be positive");
        }
        std::vector<int32_t> gs;
        tdt_total_groups(gs, n_frames_of_hyp, id_offsets, n_hyp, durations, D, V, J, max_hyps);
        for (size_t g = 0; g + 1 < gs.size(); ++g)
            for (int i = gs[g]; i < gs[g + 1]; ++i) group_of[i] = (int32_t)g;
        if (n_groups) *n_groups = (int)gs.size() - 1;
    });
}

pk_status pk_diag_rescore_order(const int32_t *lens, const float *ctc_score, const float *tdt_total, const int32_t *ok, int N, float tdt_weight,
                                int32_t *order, float *combined) {
    return guard([&] {
        need(lens && ctc_score && tdt_total && ok && order && combined && N >= 1, "lens/ctc_score/tdt_total/ok/order/combined/N");
        need(tdt_weight == tdt_weight && tdt_weight > -__builtin_huge_valf() && tdt_weight < __builtin_huge_valf(), "tdt_weight must be finite");
        rescore_order(lens, ctc_score, tdt_total, ok, N, tdt_weight, order, combined);
    });
}

/* ---- CTC keyword spotting (kernels/ctc_kws.hip) --------------------------------------------------------------------------------------- */
void pk_kws_options_default(pk_kws_options *out) {
    if (!out) return;
    *out = kws_options_of(nullptr);
}

pk_status pk_ctc_kws(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const int32_t *kw_ids, const int32_t *kw_offsets,
                     int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        const pk_kws_options o = kws_options_of(opt);
        kws_check_args(kw_ids, kw_offsets, n_kw, B, V, blank, o);
        need(logp && n_hits && start && end && score, "logp/n_hits/start/end/score");
        need(n_frames || T > 0, "T");
        HostRows in;
        in.plan(n_frames, B, T);
        need_device();
        KwsWs ws;
        kws_plan(ws, n_frames, B, in.T, kw_offsets, n_kw, o);      // (refuses before anything is allocated)
        const SeqRag rag = in.upload(logp, B, V);
        run_ctc_kws(ws, in.d_lp.as<float>(), B, in.T, rag, V, blank, kw_ids, nullptr);
        PK_CHECK_LAUNCH();
        kws_copy_out(ws, n_hits, start, end, score, nullptr);
    });
}

pk_status pk_ctc_kws_decode(pk_model *h, const float *enc, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                            const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        need(h && enc && n_hits && start && end && score && T > 0, "model/enc/n_hits/start/end/score/T");
        ctc_kws_decode(*h->m, enc, nullptr, B, T, kw_ids, kw_offsets, n_kw, opt, n_hits, start, end, score);
    });
}

pk_status pk_ctc_kws_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *kw_ids, const int32_t *kw_offsets,
                                   int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        need(h && enc && n_frames && n_hits && start && end && score, "model/enc/n_frames/n_hits/start/end/score");
        ctc_kws_decode(*h->m, enc, n_frames, B, 0, kw_ids, kw_offsets, n_kw, opt, n_hits, start, end, score);
    });
}

pk_status pk_ctc_kws_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids,
                                  const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int reps, float ms[2]) {
    return guard([&] {
        need(h && enc && ms && reps > 0 && (n_frames || T > 0), "model/enc/ms/T/reps");
        Model &m = *h->m;
        const pk_kws_options o = kws_options_of(opt);
        int V = 0, blank = 0;
        ctc_head_of(m, "CTC keyword spotting", V, blank);
        kws_check_args(kw_ids, kw_offsets, n_kw, B, V, blank, o);
        if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
        m.require_gpu();
        kws_plan(m.kws, n_frames, B, T, kw_offsets, n_kw, o);
        size_t rows;
        T = size_ws(m, n_frames, B, T, rows);
        const SeqRag rag = n_frames ? m.ws.rv.seq : SeqRag();
        PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        time_stages<2>(m, reps, ms, [&](hipEvent_t *ev) {          // the head, the spotting
            PK_HIP(hipEventRecord(ev[0], m.stream));
            m.run_ctc(m.ws, m.ws.x.as<float>(), B, T, true, m.stream);
            PK_HIP(hipEventRecord(ev[1], m.stream));
            run_ctc_kws(m.kws, m.ws.ctc_lp.as<float>(), B, T, rag, V, blank, kw_ids, m.stream);
            PK_HIP(hipEventRecord(ev[2], m.stream));
        });
    });
}

}  // extern "C"

/* ---- TDT keyword spotting (kernels/tdt_kws.hip) ---------------------------------------------------------------------------------------- */
// the checks of the model entry points; -> after them the call is planned (host only) in m.tkws
static void tdt_kws_checks(Model &m, const int32_t *n_frames, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                           const pk_kws_options &o) {
    tdt_align_model_checks(m);
    kws_check_args(kw_ids, kw_offsets, n_kw, B, m.cfg.vocab_size, m.cfg.blank_id, o, "TDT keyword spotting");
    if (n_frames) for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
    m.require_gpu();
    tdt_kws_plan_call(m.tkws, m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden, n_frames, B, T, kw_ids, kw_offsets, n_kw, nullptr,
                      nullptr, B * n_kw, o);
}

// uploads enc, runs enc_proj ONCE over the clips' rows, then the planned groups
static void tdt_kws_run(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets,
                        hipEvent_t *ev = nullptr, float *ms = nullptr) {
    size_t rows;
    size_ws(m, n_frames, B, T, rows);
    PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
    m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
    run_tdt_kws_call(m, m.tkws, m.ws.ep.as<float>(), kw_ids, kw_offsets, 0, true, ev, ms);
    PK_CHECK_LAUNCH();
}

static void tdt_kws_decode(Model &m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                           const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    tdt_kws_checks(m, n_frames, B, T, kw_ids, kw_offsets, n_kw, kws_options_of(opt));
    tdt_kws_run(m, enc, n_frames, B, T, kw_ids, kw_offsets);
    const TdtKwsWs &ws = m.tkws;
    std::copy(ws.n_hits.begin(), ws.n_hits.end(), n_hits);
    std::copy(ws.start.begin(), ws.start.end(), start);
    std::copy(ws.end.begin(), ws.end.end(), end);
    std::copy(ws.score.begin(), ws.score.end(), score);
}

extern "C" {

pk_status pk_tdt_kws(const float *lab, const float *blk, const float *dl, const float *top, const int32_t *durations, int D, const int32_t *n_frames,
                     int B, const int32_t *id_offsets, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        const pk_kws_options o = kws_options_of(opt);
        tdt_host_lattice_checks(durations, n_frames, B, id_offsets);
        need(lab && blk && dl && top && n_hits && start && end && score, "lab/blk/dl/top/n_hits/start/end/score");
        if (std::isnan(o.min_score) || o.min_score > 0.0f)
            fail(PK_ERR_INVALID, "invalid argument: min_score %g: a score is a log-ratio <= 0, so min_score must be <= 0", (double)o.min_score);
        for (int b = 0; b < B; ++b) {
            if (id_offsets[b + 1] == id_offsets[b]) fail(PK_ERR_INVALID, "invalid argument: keyword %d is empty", b);
            if (id_offsets[b + 1] - id_offsets[b] > kKwsMaxLen)
                fail(PK_ERR_UNSUPPORTED, "TDT keyword spotting: %d tokens in keyword %d, at most %d can be spotted", id_offsets[b + 1] - id_offsets[b], b,
                     kKwsMaxLen);
        }
        if (o.max_hits < 1 || o.max_hits > kKwsMaxHits)
            fail(PK_ERR_UNSUPPORTED, "TDT keyword spotting: max_hits = %d, supported 1 .. %d", o.max_hits, kKwsMaxHits);
        TdtKwsWs ws;
        ws.max_hits = o.max_hits; ws.min_score = o.min_score;
        // (the plan and the cap are host only: they refuse before a device is looked for or anything is allocated)
        tdt_lattice_plan(ws.a, n_frames, nullptr, B, 0, id_offsets, durations, D, 0, 0, 0, /*back_pointers=*/false, "TDT keyword spotting");
        if (tdt_kws_scratch(ws.a.cells, ws.a.labs, B, ws.a.u_max, D, 0, 0) > kTdtAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "TDT keyword spotting: the scratch of this call (lattice values, exit rows) exceeds the cap of %zu bytes",
                 kTdtAlignMaxScratch);
        need_device();
        tdt_lattice_upload(ws.a, nullptr, nullptr, /*token_results=*/false);
        ws.top.reserve((size_t)ws.a.cells * 4);
        PK_HIP(hipMemcpyAsync(ws.a.lab.p, lab, (size_t)ws.a.labs * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(ws.a.blk.p, blk, (size_t)ws.a.cells * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(ws.a.dl.p, dl, (size_t)ws.a.cells * D * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(ws.top.p, top, (size_t)ws.a.cells * 4, hipMemcpyHostToDevice, nullptr));
        run_tdt_kws_dp(ws, nullptr);
        PK_CHECK_LAUNCH();
        const size_t H = (size_t)o.max_hits;
        ws.n_hits.assign(B, 0); ws.start.assign(B * H, 0); ws.end.assign(B * H, 0); ws.score.assign(B * H, 0.0f);
        tdt_kws_gather(ws, 0, nullptr);
        std::copy(ws.n_hits.begin(), ws.n_hits.end(), n_hits);
        std::copy(ws.start.begin(), ws.start.end(), start);
        std::copy(ws.end.begin(), ws.end.end(), end);
        std::copy(ws.score.begin(), ws.score.end(), score);
    });
}

pk_status pk_tdt_kws_decode(pk_model *h, const float *enc, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                            const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        need(h && enc && n_hits && start && end && score && T > 0, "model/enc/n_hits/start/end/score/T");
        tdt_kws_decode(*h->m, enc, nullptr, B, T, kw_ids, kw_offsets, n_kw, opt, n_hits, start, end, score);
    });
}

pk_status pk_tdt_kws_decode_ragged(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *kw_ids, const int32_t *kw_offsets,
                                   int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score) {
    return guard([&] {
        need(h && enc && n_frames && n_hits && start && end && score, "model/enc/n_frames/n_hits/start/end/score");
        tdt_kws_decode(*h->m, enc, n_frames, B, 0, kw_ids, kw_offsets, n_kw, opt, n_hits, start, end, score);
    });
}

pk_status pk_tdt_kws_decode_timed(pk_model *h, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids,
                                  const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int reps, float ms[3]) {
    return guard([&] {
        need(h && enc && ms && reps > 0 && (n_frames || T > 0), "model/enc/ms/T/reps");
        Model &m = *h->m;
        tdt_kws_checks(m, n_frames, B, T, kw_ids, kw_offsets, n_kw, kws_options_of(opt));
        Events<4> ev;
        ev.create();
        std::vector<float> t[3];
        for (int r = 0; r <= reps; ++r) {                          // (the first pass warms the buffers up and is not counted)
            float v[3] = {0, 0, 0};                                // per stage, summed over the groups of the call
            tdt_kws_run(m, enc, n_frames, B, T, kw_ids, kw_offsets, ev.e, v);
            if (r > 0) for (int k = 0; k < 3; ++k) t[k].push_back(v[k]);
        }
        for (int k = 0; k < 3; ++k) ms[k] = median_of(t[k]);
    });
}

pk_status pk_diag_tdt_kws_lattice(pk_model *h, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                                  int chunk_rows, float *lab, float *blk, float *dl, float *top) {
    return guard([&] {
        need(h && enc && n_frames && lab && blk && dl && top && chunk_rows >= 0, "model/enc/n_frames/lab/blk/dl/top/chunk_rows");
        Model &m = *h->m;
        tdt_align_model_checks(m);
        const pk_kws_options o = kws_options_of(nullptr);
        kws_check_args(ids, id_offsets, B, B, m.cfg.vocab_size, m.cfg.blank_id, o, "TDT keyword spotting");
        for (int b = 0; b < B; ++b) need(n_frames[b] > 0, "n_frames[b] must be positive");
        m.require_gpu();
        std::vector<int32_t> self(B);
        for (int b = 0; b < B; ++b) self[b] = b;
        TdtKwsWs &ws = m.tkws;
        tdt_kws_plan_call(ws, m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden, n_frames, B, 0, ids, id_offsets, B, self.data(),
                          self.data(), B, o);
        need(ws.gstart.size() == 2, "the call must fit one group");
        int64_t cells = 0, labs = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t U = id_offsets[b + 1] - id_offsets[b];
            cells += (int64_t)n_frames[b] * (U + 1); labs += (int64_t)n_frames[b] * U;
        }
        const int D = m.cfg.num_durations;
        const size_t G = PK_DIAG_TDT_LATTICE_GUARD, nl = (size_t)labs + G, nb = (size_t)cells + G, nd = (size_t)cells * D + G;
        ws.a.lab.reserve(nl * 4); ws.a.blk.reserve(nb * 4); ws.a.dl.reserve(nd * 4); ws.top.reserve(nb * 4);
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.a.lab.p, 0x7FC5A5A5, nl, m.stream));
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.a.blk.p, 0x7FC5A5A5, nb, m.stream));
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.a.dl.p, 0x7FC5A5A5, nd, m.stream));
        PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ws.top.p, 0x7FC5A5A5, nb, m.stream));
        size_t rows;
        size_ws(m, n_frames, B, 0, rows);
        PK_HIP(hipMemcpyAsync(m.ws.x.p, enc, rows * m.cfg.hidden_size * 4, hipMemcpyHostToDevice, m.stream));
        m.run_enc_proj(m.ws.x.as<float>(), (int64_t)rows, m.ws.ep.as<float>(), m.stream);
        run_tdt_kws_call(m, ws, m.ws.ep.as<float>(), ids, id_offsets, chunk_rows, /*walk=*/false);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpyAsync(lab, ws.a.lab.p, nl * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipMemcpyAsync(blk, ws.a.blk.p, nb * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipMemcpyAsync(dl, ws.a.dl.p, nd * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipMemcpyAsync(top, ws.top.p, nb * 4, hipMemcpyDeviceToHost, m.stream));
        PK_HIP(hipStreamSynchronize(m.stream));
    });
}

}  // extern "C"
