// parakeet/transcribe.hpp -- the drop-in high-level API: parakeet::Transcriber / TDTTranscriber / transcribe() /
// to_gpu(), source-compatible with the reference's include/parakeet/transcribe.hpp:23-299, implemented on the
// MI355X engine's C ABI (include/parakeet_amd.h) instead of axiom tensors.
//
// Differences a caller can observe:
//  * the `const axiom::Tensor &samples` overloads become (const float *pcm, size_t n) / std::vector<float> -- the
//    reference itself uses (const float*, size_t) for raw PCM in read_audio() and transcribe_chunk();
//  * there is no CPU execution path: transcribe() places the model on GPU 0 on first use if to_gpu() was not called;
//  * audio files: RIFF/WAVE only (any sample rate: resampled to 16 kHz with the reference's sinc resampler; no FLAC/MP3/OGG);
//  * weights are loaded strictly (a missing / mis-shaped tensor throws instead of being ignored);
//  * boost_phrases / boost_score work as in the reference (the ContextTrie and the boosted argmax run on the GPU); the
//    Tensor-level free functions of phrase_boost.hpp (ctc_greedy_decode_boosted(Tensor, ...)) have C-ABI counterparts instead:
//    pk_set_boost_tokens / pk_set_boost_phrases + pk_ctc_decode / pk_tdt_decode;
//  * TDTTranscriber decodes with blank id = vocab_size - 1 (what the reference's CLI passes, src/main.cpp:252).  The reference CLASS
//    itself calls tdt_greedy_decode with its default blank_id = 1024 whatever the vocabulary (transcribe.hpp:274-279, tdt.hpp:78-80),
//    which differs for the 8193-token 600M vocabulary: construct TDTTranscriber(weights, vocab, config, /*blank_id=*/1024) to
//    reproduce the class literally;
//  * new: transcribe_batch() -- clips of ANY lengths are packed into ragged batches and decoded together, each clip bit-identical to
//    its single-clip result (the reference is batch-1 only; "batch inference" is a roadmap item, README.md:513).
// Errors surface as std::runtime_error with the reference's trigger conditions (unreadable vocab / audio, ...).
#pragma once

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <type_traits>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/parakeet_amd.h"
#include "config.hpp"
#include "timestamp.hpp"
#include "vocab.hpp"

namespace parakeet {

struct TranscribeResult {
    std::string text;
    std::vector<int> token_ids;
    std::vector<TimestampedToken> timestamped_tokens;   // filled when timestamps = true
    std::vector<WordTimestamp> word_timestamps;
};

enum class Decoder { CTC, TDT };

/// New (the reference's roadmap "Beam search decoding", README.md:494): one hypothesis of the CTC prefix beam search and its log-probability.
struct ScoredResult {
    TranscribeResult result;
    float score = 0.0f;
};
/// New: what Transcriber::align returns (pk_align_pcm): the given transcript with token and word timestamps from the CTC forced alignment,
/// the alignment path's log-probability and the CTC log-likelihood of the transcript.  aligned == false: the transcript does not fit the
/// audio (more tokens + adjacent repeats than frames); text and token_ids are filled, the timestamps are empty, score is -inf.
struct AlignResult : TranscribeResult {
    float score = 0.0f;
    float total = 0.0f;
    bool aligned = false;
};
/// New: one occurrence of a phrase found by Transcriber::spot (pk_spot_pcm): seconds from the start of the clip (end = the end of the last
/// frame) and the score, the log-ratio of the phrase's best path over the span to the unconstrained best path over it (<= 0; 0: the greedy
/// CTC path over the span is the phrase).
struct SpotHit {
    float start = 0.0f;
    float end = 0.0f;
    float score = 0.0f;
};
/// Parameters of Transcriber::spot (pk_kws_options).
struct SpotOptions {
    int max_hits = 1;                                               // hits per phrase, 1..16, best first, non-overlapping
    float min_score = -std::numeric_limits<float>::infinity();      // report only hits with score >= min_score (<= 0); -inf: no threshold
};
/// Parameters of Transcriber::transcribe_nbest (pk_beam_options); TranscribeOptions is untouched.
struct BeamOptions {
    int beam_width = 8;     // prefixes kept per frame, 1..32
    int token_prune = 16;   // most probable non-blank tokens considered per frame, 1..32
    int n_best = 1;         // hypotheses returned, 1..beam_width
    bool timestamps = false;
};

/// New: parameters of TDTTranscriber::transcribe_nbest (pk_tdt_beam_options).
struct TdtBeamOptions {
    int beam_width = 8;      // hypotheses kept per step, 1..16
    int label_prune = 8;     // most probable non-blank labels expanded per hypothesis, 1..16
    int duration_prune = 2;  // most probable durations expanded per label, 1..8
    int n_best = 1;          // hypotheses returned, 1..beam_width
    bool timestamps = false;
};

/// New: parameters of the TDT rescoring of an n-best list (pk_rescore_options).
struct RescoreOptions {
    float tdt_weight = 0.5f;   // w: hypotheses are ordered by (1 - w) * CTC score + w * TDT log-likelihood
};
/// New: one hypothesis of transcribe_nbest(audio, beam, rescore): score is the combined value, ctc_score / tdt_total its parts.
struct RescoredResult : ScoredResult {
    float ctc_score = 0.0f;
    float tdt_total = 0.0f;
};
/// New: an n-gram language model over the acoustic model's token ids (pk_lm: ARPA text whose words are decimal ids).
class LanguageModel {
  public:
    explicit LanguageModel(const std::string &arpa_path) {
        if (pk_lm_load(arpa_path.c_str(), &lm_) != PK_OK) {
            char msg[1024];
            pk_last_error(msg, sizeof msg);
            throw std::runtime_error(msg);
        }
    }
    ~LanguageModel() { pk_lm_free(lm_); }
    LanguageModel(const LanguageModel &) = delete;
    LanguageModel &operator=(const LanguageModel &) = delete;
    int order() const { return pk_lm_order(lm_); }
    int64_t num_ngrams() const { return pk_lm_num_ngrams(lm_); }
    /// pk_lm_score of one token string: its fp32 natural-log probability (host only); what an n-best list is rescored with
    float score(const std::vector<int> &token_ids, bool bos = true, bool eos = false) const {
        std::vector<int32_t> ids(token_ids.begin(), token_ids.end());
        const int32_t off[2] = {0, (int32_t)ids.size()};
        float out = 0.0f;
        if (pk_lm_score(lm_, ids.data(), off, 1, bos ? 1 : 0, eos ? 1 : 0, &out) != PK_OK) {
            char msg[1024];
            pk_last_error(msg, sizeof msg);
            throw std::runtime_error(msg);
        }
        return out;
    }
    const pk_lm *handle() const { return lm_; }

  private:
    pk_lm *lm_ = nullptr;
};
/// New: weights of the shallow fusion (pk_lm_options): hypotheses rank by score + lm_score, lm_score = sum per token of alpha * log p + beta.
struct LmOptions {
    float alpha = 0.5f;
    float beta = 0.0f;
};
/// New: one hypothesis of transcribe_nbest(audio, beam, lm): score stays the acoustic log-probability, lm_score is the model's part.
struct LmScoredResult : ScoredResult {
    float lm_score = 0.0f;
};
/// New: a causal Transformer LM over the acoustic model's token ids plus BOS / EOS (pk_nlm) that re-ranks n-best lists.
/// The file's tensor shapes give the rest of the configuration (pk_nlm_config_infer); eos_id < 0: no end-of-string term.
class NeuralLanguageModel {
  public:
    NeuralLanguageModel(const std::string &safetensors_path, int num_heads, int bos_id, int eos_id = -1, bool pre_ln = true, const std::string &prefix = "",
                        int device = 0) {
        cfg_ = pk_nlm_config{};
        cfg_.transformer.num_heads = num_heads;
        cfg_.transformer.pre_ln = pre_ln ? 1 : 0;
        cfg_.transformer.layer_norm_eps = 1e-5f;
        cfg_.bos_id = bos_id;
        cfg_.eos_id = eos_id;
        if (pk_nlm_config_infer(safetensors_path.c_str(), prefix.c_str(), &cfg_) != PK_OK ||
            pk_nlm_load(safetensors_path.c_str(), prefix.c_str(), &cfg_, device, &nlm_) != PK_OK) {
            char msg[1024];
            pk_last_error(msg, sizeof msg);
            throw std::runtime_error(msg);
        }
    }
    ~NeuralLanguageModel() { pk_nlm_free(nlm_); }
    NeuralLanguageModel(const NeuralLanguageModel &) = delete;
    NeuralLanguageModel &operator=(const NeuralLanguageModel &) = delete;
    const pk_nlm_config &config() const { return cfg_; }
    pk_nlm *handle() const { return nlm_; }

  private:
    pk_nlm_config cfg_;
    pk_nlm *nlm_ = nullptr;
};
/// New: weights of the re-ranking (pk_nlm_rescore_options): combined = am + alpha * nlm + beta * tokens.
struct NlmOptions {
    float alpha = 0.5f;
    float beta = 0.0f;
};
/// New: one hypothesis of transcribe_nbest(audio, beam, nlm): score is the combined value, am_score / nlm_score its parts.
struct NlmScoredResult : ScoredResult {
    float am_score = 0.0f;
    float nlm_score = 0.0f;
};
/// New: what Transcriber::score returns: the log-likelihood of the given transcript under the TDT head (pk_tdt_score_pcm: the forward algorithm
/// on the alignment's lattice).  scored == false: no path emits the transcript on this audio, log_likelihood is -inf.
struct ScoreResult {
    std::string text;
    std::vector<int> token_ids;
    float log_likelihood = 0.0f;
    bool scored = false;
};

struct TranscribeOptions {
    Decoder decoder = Decoder::TDT;
    bool timestamps = false;
    std::vector<std::string> boost_phrases;   // ContextTrie::build of these phrases biases the greedy argmax (phrase_boost.hpp)
    float boost_score = 5.0f;
    // New: cut the audio at its pauses on the device and transcribe only the speech, in pieces of at most vad_max_piece_s seconds that share
    // batches (pk_transcribe_pcm_vad); for long or sparse recordings.  Single device, 16 kHz.
    bool vad = false;
    float vad_max_piece_s = 30.0f;
};

namespace detail {

inline void check(pk_status st) {
    if (st == PK_OK) return;
    char msg[1024];
    pk_last_error(msg, sizeof msg);
    throw std::runtime_error(msg);
}

class Engine {   // owns one pk_model; shared by Transcriber and TDTTranscriber
  public:
    Engine(const std::string &weights_path, const std::string &vocab_path, const pk_config &cfg)
        : weights_path_(weights_path), vocab_path_(vocab_path), cfg_(cfg) {
        check(pk_model_load(weights_path.c_str(), vocab_path.empty() ? nullptr : vocab_path.c_str(), &cfg, &m_));
        tok_ = Tokenizer(m_);
    }
    ~Engine() {
        pk_group_free(g_);
        pk_model_free(m_);
    }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    void to_gpu(int device = 0) {
        check(pk_model_to_gpu(m_, device));
        on_gpu_ = true;
    }

    // New (the reference is single-device, README.md:513): one replica per GPU of this node, clips dealt to the devices in batches
    // (pk_group: one replica and one host thread + two-stream pipeline per device, no collective).  Empty list = every visible device.
    void to_all_gpus(const std::vector<int> &devices = {}) {
        pk_group_free(g_);
        g_ = nullptr;
        check(pk_group_create(weights_path_.c_str(), vocab_path_.empty() ? nullptr : vocab_path_.c_str(), &cfg_,
                              devices.empty() ? nullptr : devices.data(), (int)devices.size(), &g_));
        check(pk_group_set_attention_context(g_, att_left_, att_right_));
    }
    // New: limited-context encoder attention over frames [i - left, i + right] (pk_model_set_attention_context; NeMo's local attention
    // [L, L] is (L, L)); (-1, -1) = full attention.  Applies to this engine's model and its replicas.
    void set_attention_context(int left, int right) {
        check(pk_model_set_attention_context(m_, left, right));
        if (g_) check(pk_group_set_attention_context(g_, left, right));
        att_left_ = left;
        att_right_ = right;
    }
    // New: files at another rate than 16 kHz are read at their own rate and resampled on the device on their way into the call
    // (pk_model_set_input_rate for the duration of the call) instead of by pk_read_audio's host resampler.  Off by default: for rates that
    // neither divide nor are divided by 16 kHz the device's samples differ from the host's by one fp32 rounding now and then.
    void set_device_resampling(bool on) { device_resample_ = on; }
    int num_gpus() const { return g_ ? pk_group_size(g_) : (on_gpu_ ? 1 : 0); }

    std::vector<TranscribeResult> run(const std::vector<std::pair<const float *, size_t>> &clips, const TranscribeOptions &opts) {
        if (!g_ && !on_gpu_) to_gpu(0);
        std::vector<float> pcm;
        std::vector<int64_t> offsets{0};
        for (auto &c : clips) {
            pcm.insert(pcm.end(), c.first, c.first + c.second);
            offsets.push_back((int64_t)pcm.size());
        }
        pk_options o{};
        o.decoder = opts.decoder == Decoder::CTC ? PK_DECODER_CTC : PK_DECODER_TDT;
        o.timestamps = opts.timestamps ? 1 : 0;
        std::vector<const char *> phrases;
        for (auto &p : opts.boost_phrases) phrases.push_back(p.c_str());
        o.boost_phrases = phrases.data();
        o.n_boost_phrases = (int32_t)phrases.size();
        o.boost_score = opts.boost_score;
        pk_result *res = nullptr;
        if (opts.vad) {
            if (g_) throw std::runtime_error("TranscribeOptions::vad has no multi-GPU variant");
            pk_vad_options vo;
            pk_vad_options_default(&vo);
            vo.max_piece_s = opts.vad_max_piece_s;
            check(pk_transcribe_pcm_vad(m_, pcm.data(), offsets.data(), (int)clips.size(), &o, &vo, &res, nullptr, nullptr));
        } else if (g_) check(pk_group_transcribe_pcm(g_, pcm.data(), offsets.data(), (int)clips.size(), &o, &res));
        else check(pk_transcribe_pcm(m_, pcm.data(), offsets.data(), (int)clips.size(), &o, &res));
        std::vector<TranscribeResult> out(clips.size());
        for (size_t i = 0; i < clips.size(); ++i) convert(res[i], opts.timestamps, out[i]);
        pk_results_free(res, (int)clips.size());
        return out;
    }
    TranscribeResult run_file(const std::string &audio_path, const TranscribeOptions &opts) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run({{pcm, n}}, opts)[0]; });
    }

    // pk_transcribe_pcm_nbest on one clip: the CTC prefix beam search's hypotheses, best first (single device; replicas are not used)
    std::vector<ScoredResult> run_nbest(const float *pcm, size_t n, const BeamOptions &opts) {
        if (!on_gpu_) to_gpu(0);
        const pk_beam_options o = beam_options(opts);
        const int64_t offsets[2] = {0, (int64_t)n};
        pk_nbest *res = nullptr;
        check(pk_transcribe_pcm_nbest(m_, pcm, offsets, 1, &o, &res));
        return take_nbest<ScoredResult>(res, opts.timestamps, [](ScoredResult &, int) {});
    }
    std::vector<ScoredResult> run_nbest_file(const std::string &audio_path, const BeamOptions &opts) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest(pcm, n, opts); });
    }

    // pk_transcribe_pcm_nbest_lm on one clip: the search with n-gram LM shallow fusion, hypotheses in fused order
    std::vector<LmScoredResult> run_nbest_lm(const float *pcm, size_t n, const BeamOptions &opts, const LanguageModel &lm, const LmOptions &lmo) {
        if (!on_gpu_) to_gpu(0);
        const pk_beam_options o = beam_options(opts);
        const pk_lm_options lo = lm_options(lmo);
        const int64_t offsets[2] = {0, (int64_t)n};
        std::vector<float> lms((size_t)std::max(1, opts.n_best), 0.0f);
        pk_nbest *res = nullptr;
        check(pk_transcribe_pcm_nbest_lm(m_, pcm, offsets, 1, &o, &res, lm.handle(), &lo, lms.data()));
        return take_nbest<LmScoredResult>(res, opts.timestamps, [&](LmScoredResult &r, int j) { r.lm_score = lms[j]; });
    }
    std::vector<LmScoredResult> run_nbest_lm_file(const std::string &audio_path, const BeamOptions &opts, const LanguageModel &lm, const LmOptions &lmo) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest_lm(pcm, n, opts, lm, lmo); });
    }

    // pk_transcribe_pcm_nbest_tdt on one clip: the TDT beam search's hypotheses, best first; score is the path's log-probability
    std::vector<ScoredResult> run_nbest_tdt(const float *pcm, size_t n, const TdtBeamOptions &opts) {
        if (!on_gpu_) to_gpu(0);
        const pk_tdt_beam_options o = tdt_beam_options(opts);
        const int64_t offsets[2] = {0, (int64_t)n};
        pk_nbest *res = nullptr;
        check(pk_transcribe_pcm_nbest_tdt(m_, pcm, offsets, 1, &o, opts.timestamps ? 1 : 0, &res));
        return take_nbest<ScoredResult>(res, opts.timestamps, [](ScoredResult &, int) {});
    }
    std::vector<ScoredResult> run_nbest_tdt_file(const std::string &audio_path, const TdtBeamOptions &opts) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest_tdt(pcm, n, opts); });
    }

    // pk_transcribe_pcm_nbest_tdt_lm on one clip: the TDT beam search with n-gram LM shallow fusion, hypotheses in fused order
    std::vector<LmScoredResult> run_nbest_tdt_lm(const float *pcm, size_t n, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lmo) {
        if (!on_gpu_) to_gpu(0);
        const pk_tdt_beam_options o = tdt_beam_options(opts);
        const pk_lm_options lo = lm_options(lmo);
        const int64_t offsets[2] = {0, (int64_t)n};
        std::vector<float> lms((size_t)std::max(1, opts.n_best), 0.0f);
        pk_nbest *res = nullptr;
        check(pk_transcribe_pcm_nbest_tdt_lm(m_, pcm, offsets, 1, &o, opts.timestamps ? 1 : 0, &res, lm.handle(), &lo, lms.data()));
        return take_nbest<LmScoredResult>(res, opts.timestamps, [&](LmScoredResult &r, int j) { r.lm_score = lms[j]; });
    }
    std::vector<LmScoredResult> run_nbest_tdt_lm_file(const std::string &audio_path, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lmo) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest_tdt_lm(pcm, n, opts, lm, lmo); });
    }

    // the list of run_nbest (tdt false) or run_nbest_tdt (tdt true) re-ranked by a Transformer LM: pk_nbest_rescore_nlm on the list before it is taken
    template <class Options>
    std::vector<NlmScoredResult> run_nbest_nlm(const float *pcm, size_t n, const Options &opts, const NeuralLanguageModel &nlm, const NlmOptions &no) {
        if (!on_gpu_) to_gpu(0);
        const int64_t offsets[2] = {0, (int64_t)n};
        pk_nbest *res = nullptr;
        if constexpr (std::is_same<Options, TdtBeamOptions>::value) {
            const pk_tdt_beam_options o = tdt_beam_options(opts);
            check(pk_transcribe_pcm_nbest_tdt(m_, pcm, offsets, 1, &o, opts.timestamps ? 1 : 0, &res));
        } else {
            const pk_beam_options o = beam_options(opts);
            check(pk_transcribe_pcm_nbest(m_, pcm, offsets, 1, &o, &res));
        }
        const pk_nlm_rescore_options ro{no.alpha, no.beta};
        std::vector<float> am((size_t)std::max(1, opts.n_best)), ns(am.size());
        const pk_status st = pk_nbest_rescore_nlm(res, 1, nlm.handle(), &ro, am.data(), ns.data());
        if (st != PK_OK) pk_nbest_free(res, 1);
        check(st);
        return take_nbest<NlmScoredResult>(res, opts.timestamps, [&](NlmScoredResult &r, int j) { r.am_score = am[j]; r.nlm_score = ns[j]; });
    }
    template <class Options>
    std::vector<NlmScoredResult> run_nbest_nlm_file(const std::string &audio_path, const Options &opts, const NeuralLanguageModel &nlm, const NlmOptions &no) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest_nlm(pcm, n, opts, nlm, no); });
    }

    // pk_transcribe_pcm_nbest_rescored on one clip: run_nbest's list re-ranked by the TDT head's log-likelihood of every hypothesis
    std::vector<RescoredResult> run_nbest_rescored(const float *pcm, size_t n, const BeamOptions &opts, const RescoreOptions &rescore) {
        if (!on_gpu_) to_gpu(0);
        const pk_beam_options o = beam_options(opts);
        pk_rescore_options ro{rescore.tdt_weight};
        const int64_t offsets[2] = {0, (int64_t)n};
        pk_nbest *res = nullptr;
        std::vector<float> ctc((size_t)std::max(1, opts.n_best)), tdt(ctc.size());
        check(pk_transcribe_pcm_nbest_rescored(m_, pcm, offsets, 1, &o, &ro, &res, ctc.data(), tdt.data()));
        return take_nbest<RescoredResult>(res, opts.timestamps, [&](RescoredResult &r, int j) { r.ctc_score = ctc[j]; r.tdt_total = tdt[j]; });
    }
    std::vector<RescoredResult> run_nbest_rescored_file(const std::string &audio_path, const BeamOptions &opts, const RescoreOptions &rescore) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_nbest_rescored(pcm, n, opts, rescore); });
    }

    // the log-likelihood of `text` (tokenised by the model's vocabulary) on one clip under the TDT head: pk_tdt_score_pcm
    ScoreResult run_score(const float *pcm, size_t n, const std::string &text, bool tdt_head) {
        if (!tdt_head) throw std::invalid_argument("score: only the TDT head is scored here; the CTC head's log-likelihood is AlignResult::total of align()");
        if (!on_gpu_) to_gpu(0);
        const int64_t offsets[2] = {0, (int64_t)n};
        const char *texts[1] = {text.c_str()};
        ScoreResult out;
        out.text = text;
        for (int v : tok_.encode(text)) out.token_ids.push_back(v);
        int32_t ok = 0;
        check(pk_tdt_score_pcm(m_, pcm, offsets, 1, texts, nullptr, nullptr, nullptr, 1, &out.log_likelihood, &ok));
        out.scored = ok != 0;
        return out;
    }
    ScoreResult run_score_file(const std::string &audio_path, const std::string &text, bool tdt_head) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_score(pcm, n, text, tdt_head); });
    }

    // pk_align_pcm on one clip: the CTC forced alignment of `text` (tokenised by the model's vocabulary); single device
    // tdt_head: pk_tdt_align_pcm, the TDT forced alignment (no CTC head needed; AlignResult::total stays 0: that head has no forward pass)
    AlignResult run_align(const float *pcm, size_t n, const std::string &text, bool tdt_head = false) {
        if (!on_gpu_) to_gpu(0);
        const int64_t offsets[2] = {0, (int64_t)n};
        const char *texts[1] = {text.c_str()};
        pk_result *res = nullptr;
        float score = 0.0f, total = 0.0f;
        int32_t ok = 0;
        if (tdt_head) check(pk_tdt_align_pcm(m_, pcm, offsets, 1, texts, nullptr, nullptr, &res, &score, &ok));
        else check(pk_align_pcm(m_, pcm, offsets, 1, texts, nullptr, nullptr, &res, &score, &total, &ok));
        AlignResult out;
        out.score = score; out.total = total; out.aligned = ok != 0;
        convert(res[0], out.aligned, out);
        pk_results_free(res, 1);
        return out;
    }
    AlignResult run_align_file(const std::string &audio_path, const std::string &text, bool tdt_head = false) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_align(pcm, n, text, tdt_head); });
    }

    // pk_spot_pcm (tdt: pk_tdt_spot_pcm) on one clip: every phrase (tokenised by the model's vocabulary) -> its hits, best first; single device
    std::vector<std::vector<SpotHit>> run_spot(const float *pcm, size_t n, const std::vector<std::string> &phrases, const SpotOptions &opts, bool tdt = false) {
        if (!on_gpu_) to_gpu(0);
        std::vector<std::vector<SpotHit>> out(phrases.size());
        if (phrases.empty()) return out;
        const int64_t offsets[2] = {0, (int64_t)n};
        std::vector<const char *> texts;
        for (const auto &p : phrases) texts.push_back(p.c_str());
        pk_kws_options o;
        pk_kws_options_default(&o);
        o.max_hits = opts.max_hits; o.min_score = opts.min_score;
        const size_t K = phrases.size(), H = (size_t)(opts.max_hits > 0 ? opts.max_hits : 1);
        std::vector<int32_t> n_hits(K);
        std::vector<float> st(K * H), en(K * H), sc(K * H);
        check((tdt ? pk_tdt_spot_pcm : pk_spot_pcm)(m_, pcm, offsets, 1, texts.data(), nullptr, nullptr, (int)K, &o, n_hits.data(), st.data(), en.data(), sc.data()));
        for (size_t k = 0; k < K; ++k)
            for (int j = 0; j < n_hits[k]; ++j) out[k].push_back({st[k * H + j], en[k * H + j], sc[k * H + j]});
        return out;
    }
    std::vector<std::vector<SpotHit>> run_spot_file(const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &opts, bool tdt = false) {
        return with_audio(audio_path, [&](const float *pcm, size_t n) { return run_spot(pcm, n, phrases, opts, tdt); });
    }

    const Tokenizer &tokenizer() const { return tok_; }
    pk_model *handle() { return m_; }

  private:
    // read_audio(path): decode, downmix, resample to 16 kHz; the samples go to fn(pcm, n) and are freed when it returns or throws.
    // With set_device_resampling(true) the file keeps its own rate and the model takes that rate while fn runs.
    template <class Fn>
    auto with_audio(const std::string &audio_path, Fn fn) -> decltype(fn((const float *)nullptr, size_t())) {
        float *pcm = nullptr;
        int64_t n = 0, frames = 0;
        int sr = 0, rate = 16000, channels = 0;
        if (device_resample_) check(pk_audio_info(audio_path.c_str(), &rate, &channels, &frames));
        check(pk_read_audio(audio_path.c_str(), rate, &pcm, &n, &sr));
        struct Free { float *p; ~Free() { pk_free(p); } } guard{pcm};
        struct Rate {
            Engine *e; bool set;
            ~Rate() { if (set) { (void)pk_model_set_input_rate(e->m_, 16000); if (e->g_) (void)pk_group_set_input_rate(e->g_, 16000); } }
        } restore{this, rate != 16000};
        if (rate != 16000) {
            if (!g_ && !on_gpu_) to_gpu(0);
            check(pk_model_set_input_rate(m_, rate));
            if (g_) check(pk_group_set_input_rate(g_, rate));
        }
        return fn(pcm, (size_t)n);
    }
    // text and token ids of a pk_result and, with timestamps, its timestamped tokens and words
    static void convert(const pk_result &r, bool timestamps, TranscribeResult &out) {
        out.text = r.text ? r.text : "";
        out.token_ids.assign(r.token_ids, r.token_ids + r.n_tokens);
        if (!timestamps) return;
        for (int k = 0; k < r.n_tokens; ++k) out.timestamped_tokens.push_back({r.token_ids[k], r.start_frame[k], r.end_frame[k], r.confidence[k]});
        for (int k = 0; k < r.n_words; ++k) out.word_timestamps.push_back({r.words[k].word, r.words[k].start, r.words[k].end, r.words[k].confidence});
    }
    // the hypotheses of a one-clip pk_nbest array (freed here) as Result, a ScoredResult; extra(result, j) adds what the call returned beside them
    template <class Result, class Extra>
    static std::vector<Result> take_nbest(pk_nbest *res, bool timestamps, Extra extra) {
        std::vector<Result> out(res[0].n_hyp);
        for (int j = 0; j < res[0].n_hyp; ++j) {
            out[j].score = res[0].score[j];
            convert(res[0].hyp[j], timestamps, out[j].result);
            extra(out[j], j);
        }
        pk_nbest_free(res, 1);
        return out;
    }
    static pk_beam_options beam_options(const BeamOptions &opts) {
        pk_beam_options o;
        pk_beam_options_default(&o);
        o.beam_width = opts.beam_width; o.token_prune = opts.token_prune; o.n_best = opts.n_best; o.timestamps = opts.timestamps ? 1 : 0;
        return o;
    }
    static pk_tdt_beam_options tdt_beam_options(const TdtBeamOptions &opts) {
        pk_tdt_beam_options o;
        pk_tdt_beam_options_default(&o);
        o.beam_width = opts.beam_width; o.label_prune = opts.label_prune; o.duration_prune = opts.duration_prune; o.n_best = opts.n_best;
        return o;
    }
    static pk_lm_options lm_options(const LmOptions &opts) { return pk_lm_options{opts.alpha, opts.beta}; }

    std::string weights_path_, vocab_path_;
    pk_config cfg_;
    pk_model *m_ = nullptr;
    int att_left_ = -1, att_right_ = -1;
    bool device_resample_ = false;
    pk_group *g_ = nullptr;
    Tokenizer tok_;
    bool on_gpu_ = false;
};

}  // namespace detail

/// parakeet::Transcriber t("model.safetensors", "vocab.txt");  t.to_gpu();  auto r = t.transcribe("audio.wav");
class Transcriber {
  public:
    Transcriber(const std::string &weights_path, const std::string &vocab_path, const TDTCTCConfig &config = make_110m_config())
        : config_(config),
          eng_(weights_path, vocab_path,
               detail::flatten(config.encoder, config.prediction, config.joint, config.durations, config.ctc_vocab_size, "tdt_joint_.",
                               false, 1024)) {}   // blank_id: the decoders' default 1024 (tdt.hpp / ctc.hpp), as Transcriber uses it

    void to_gpu() { eng_.to_gpu(0); }
    void to_gpu(int device) { eng_.to_gpu(device); }
    /// New: a replica on every GPU of the node (or on `devices`); transcribe_batch() then shards its clips over them.
    void to_all_gpus(const std::vector<int> &devices = {}) { eng_.to_all_gpus(devices); }
    int num_gpus() const { return eng_.num_gpus(); }
    /// New: limited-context attention for long audio (Engine::set_attention_context); (-1, -1) restores full attention.
    void set_attention_context(int left, int right) { eng_.set_attention_context(left, right); }
    /// New: resample files on the device instead of on the host (Engine::set_device_resampling); off by default.
    void set_device_resampling(bool on) { eng_.set_device_resampling(on); }

    TranscribeResult transcribe(const std::string &audio_path, Decoder decoder = Decoder::TDT, bool timestamps = false) {
        return eng_.run_file(audio_path, options(decoder, timestamps));
    }
    TranscribeResult transcribe(const std::string &audio_path, const TranscribeOptions &opts) { return eng_.run_file(audio_path, opts); }
    TranscribeResult transcribe(const float *pcm, size_t n, Decoder decoder = Decoder::TDT, bool timestamps = false) {
        return eng_.run({{pcm, n}}, options(decoder, timestamps))[0];
    }
    TranscribeResult transcribe(const float *pcm, size_t n, const TranscribeOptions &opts) { return eng_.run({{pcm, n}}, opts)[0]; }
    TranscribeResult transcribe(const std::vector<float> &samples, Decoder decoder = Decoder::TDT, bool timestamps = false) {
        return transcribe(samples.data(), samples.size(), decoder, timestamps);
    }
    TranscribeResult transcribe(const std::vector<float> &samples, const TranscribeOptions &opts) {
        return transcribe(samples.data(), samples.size(), opts);
    }
    /// New: many clips at once; clips of equal length share a GPU batch.
    std::vector<TranscribeResult> transcribe_batch(const std::vector<std::vector<float>> &clips, const TranscribeOptions &opts = {}) {
        std::vector<std::pair<const float *, size_t>> v;
        for (auto &c : clips) v.emplace_back(c.data(), c.size());
        return eng_.run(v, opts);
    }
    /// New (roadmap "Beam search decoding", README.md:494): CTC prefix beam search on the device, the n best hypotheses with scores, best first.
    std::vector<ScoredResult> transcribe_nbest(const std::string &audio_path, const BeamOptions &opts = {}) { return eng_.run_nbest_file(audio_path, opts); }
    std::vector<ScoredResult> transcribe_nbest(const float *pcm, size_t n, const BeamOptions &opts = {}) { return eng_.run_nbest(pcm, n, opts); }
    std::vector<ScoredResult> transcribe_nbest(const std::vector<float> &samples, const BeamOptions &opts = {}) {
        return eng_.run_nbest(samples.data(), samples.size(), opts);
    }

    const Tokenizer &tokenizer() const { return eng_.tokenizer(); }
    const TDTCTCConfig &config() const { return config_; }
    /// New: CTC forced alignment of a known transcript (pk_align_pcm): when was each token / word of `text` said.  Needs the vocabulary.
    AlignResult align(const std::string &audio_path, const std::string &text) { return eng_.run_align_file(audio_path, text); }
    AlignResult align(const float *pcm, size_t n, const std::string &text) { return eng_.run_align(pcm, n, text); }
    AlignResult align(const std::vector<float> &samples, const std::string &text) { return eng_.run_align(samples.data(), samples.size(), text); }
    /// New: CTC keyword spotting (pk_spot_pcm): where in the audio was each phrase said; result[k] = the hits of phrases[k], best first.
    /// Needs the vocabulary.
    std::vector<std::vector<SpotHit>> spot(const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot_file(audio_path, phrases, opts);
    }
    std::vector<std::vector<SpotHit>> spot(const float *pcm, size_t n, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(pcm, n, phrases, opts);
    }
    std::vector<std::vector<SpotHit>> spot(const std::vector<float> &samples, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(samples.data(), samples.size(), phrases, opts);
    }
    /// New: keyword spotting through the TDT head (pk_tdt_spot_pcm): works without a CTC head.  A phrase is scored as if it
    /// began the utterance; score 0: greedy TDT decoding with that context emits the phrase there.
    std::vector<std::vector<SpotHit>> spot_tdt(const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot_file(audio_path, phrases, opts, true);
    }
    std::vector<std::vector<SpotHit>> spot_tdt(const float *pcm, size_t n, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(pcm, n, phrases, opts, true);
    }
    std::vector<std::vector<SpotHit>> spot_tdt(const std::vector<float> &samples, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(samples.data(), samples.size(), phrases, opts, true);
    }
    /// New: the same through the TDT head (pk_tdt_align_pcm): works without a CTC head.  AlignResult::total is 0.
    AlignResult align_tdt(const std::string &audio_path, const std::string &text) { return eng_.run_align_file(audio_path, text, true); }
    AlignResult align_tdt(const float *pcm, size_t n, const std::string &text) { return eng_.run_align(pcm, n, text, true); }
    AlignResult align_tdt(const std::vector<float> &samples, const std::string &text) { return eng_.run_align(samples.data(), samples.size(), text, true); }
    /// New: the search with n-gram LM shallow fusion (pk_transcribe_pcm_nbest_lm): hypotheses in fused order, score + lm_score per hypothesis
    std::vector<LmScoredResult> transcribe_nbest(const std::string &audio_path, const BeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_lm_file(audio_path, opts, lm, lm_opts);
    }
    std::vector<LmScoredResult> transcribe_nbest(const float *pcm, size_t n, const BeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_lm(pcm, n, opts, lm, lm_opts);
    }
    /// New: the list of either search re-ranked by a Transformer LM (pk_nbest_rescore_nlm): score + am_score + nlm_score
    std::vector<NlmScoredResult> transcribe_nbest(const std::string &audio_path, const BeamOptions &opts, const NeuralLanguageModel &nlm, const NlmOptions &no = {}) {
        return eng_.run_nbest_nlm_file(audio_path, opts, nlm, no);
    }
    std::vector<NlmScoredResult> transcribe_nbest_tdt(const std::string &audio_path, const TdtBeamOptions &opts, const NeuralLanguageModel &nlm, const NlmOptions &no = {}) {
        return eng_.run_nbest_nlm_file(audio_path, opts, nlm, no);
    }
    /// New: the same search through this model's TDT head (TDTTranscriber::transcribe_nbest)
    std::vector<ScoredResult> transcribe_nbest_tdt(const std::string &audio_path, const TdtBeamOptions &opts = {}) { return eng_.run_nbest_tdt_file(audio_path, opts); }
    std::vector<ScoredResult> transcribe_nbest_tdt(const float *pcm, size_t n, const TdtBeamOptions &opts = {}) { return eng_.run_nbest_tdt(pcm, n, opts); }
    /// New: the TDT beam search with n-gram LM shallow fusion (pk_transcribe_pcm_nbest_tdt_lm): fused order, score + lm_score
    std::vector<LmScoredResult> transcribe_nbest_tdt(const std::string &audio_path, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_tdt_lm_file(audio_path, opts, lm, lm_opts);
    }
    std::vector<LmScoredResult> transcribe_nbest_tdt(const float *pcm, size_t n, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_tdt_lm(pcm, n, opts, lm, lm_opts);
    }
    /// New: the log-likelihood of a given transcript: tdt_head = true through the TDT head's forward algorithm
    /// (pk_tdt_score_pcm; no CTC head needed).  false throws std::invalid_argument: the CTC head's log-likelihood is align()'s AlignResult::total.
    ScoreResult score(const std::string &audio_path, const std::string &text, bool tdt_head = true) { return eng_.run_score_file(audio_path, text, tdt_head); }
    ScoreResult score(const float *pcm, size_t n, const std::string &text, bool tdt_head = true) { return eng_.run_score(pcm, n, text, tdt_head); }
    ScoreResult score(const std::vector<float> &samples, const std::string &text, bool tdt_head = true) {
        return eng_.run_score(samples.data(), samples.size(), text, tdt_head);
    }
    /// New: the n-best list re-ranked by the TDT head (pk_transcribe_pcm_nbest_rescored): needs both heads.
    std::vector<RescoredResult> transcribe_nbest(const std::string &audio_path, const BeamOptions &opts, const RescoreOptions &rescore) {
        return eng_.run_nbest_rescored_file(audio_path, opts, rescore);
    }
    std::vector<RescoredResult> transcribe_nbest(const float *pcm, size_t n, const BeamOptions &opts, const RescoreOptions &rescore) {
        return eng_.run_nbest_rescored(pcm, n, opts, rescore);
    }

    pk_model *model() { return eng_.handle(); }   // the engine handle (the reference returns its ParakeetTDTCTC module tree)

  private:
    static TranscribeOptions options(Decoder d, bool ts) {
        TranscribeOptions o;
        o.decoder = d;
        o.timestamps = ts;
        return o;
    }
    TDTCTCConfig config_;
    detail::Engine eng_;
};

/// TDT-only models (no CTC head), e.g. the 600M multilingual checkpoint.
class TDTTranscriber {
  public:
    // blank_id < 0 (default): vocab_size - 1, what the reference CLI passes (main.cpp:252).  blank_id = 1024 reproduces the reference
    // class literally: its transcribe() calls tdt_greedy_decode with the decoder's default blank (transcribe.hpp:274-279, tdt.hpp:78-80).
    TDTTranscriber(const std::string &weights_path, const std::string &vocab_path, const TDTConfig &config = make_tdt_600m_config(),
                   int blank_id = -1)
        : config_(config),
          eng_(weights_path, vocab_path,
               detail::flatten(config.encoder, config.prediction, config.joint, config.durations, 0, "joint_.", false,
                               blank_id >= 0 ? blank_id : config.joint.vocab_size - 1)) {}

    void to_gpu() { eng_.to_gpu(0); }
    void to_gpu(int device) { eng_.to_gpu(device); }
    void to_all_gpus(const std::vector<int> &devices = {}) { eng_.to_all_gpus(devices); }
    int num_gpus() const { return eng_.num_gpus(); }
    /// New: limited-context attention for long audio (Engine::set_attention_context); (-1, -1) restores full attention.
    void set_attention_context(int left, int right) { eng_.set_attention_context(left, right); }
    /// New: resample files on the device instead of on the host (Engine::set_device_resampling); off by default.
    void set_device_resampling(bool on) { eng_.set_device_resampling(on); }

    TranscribeResult transcribe(const std::string &audio_path, bool timestamps = false) { return eng_.run_file(audio_path, options(timestamps)); }
    TranscribeResult transcribe(const std::string &audio_path, const TranscribeOptions &opts) { return eng_.run_file(audio_path, tdt(opts)); }
    TranscribeResult transcribe(const float *pcm, size_t n, bool timestamps = false) { return eng_.run({{pcm, n}}, options(timestamps))[0]; }
    TranscribeResult transcribe(const float *pcm, size_t n, const TranscribeOptions &opts) { return eng_.run({{pcm, n}}, tdt(opts))[0]; }
    TranscribeResult transcribe(const std::vector<float> &samples, bool timestamps = false) {
        return transcribe(samples.data(), samples.size(), timestamps);
    }
    std::vector<TranscribeResult> transcribe_batch(const std::vector<std::vector<float>> &clips, const TranscribeOptions &opts = {}) {
        std::vector<std::pair<const float *, size_t>> v;
        for (auto &c : clips) v.emplace_back(c.data(), c.size());
        return eng_.run(v, tdt(opts));
    }

    const Tokenizer &tokenizer() const { return eng_.tokenizer(); }
    const TDTConfig &config() const { return config_; }
    /// New: CTC forced alignment of a known transcript (pk_align_pcm): when was each token / word of `text` said.  Needs the vocabulary and a model
    /// with a CTC head (the tdt-600m preset has none: the call throws).
    AlignResult align(const std::string &audio_path, const std::string &text) { return eng_.run_align_file(audio_path, text); }
    AlignResult align(const float *pcm, size_t n, const std::string &text) { return eng_.run_align(pcm, n, text); }
    AlignResult align(const std::vector<float> &samples, const std::string &text) { return eng_.run_align(samples.data(), samples.size(), text); }
    /// New: CTC keyword spotting (pk_spot_pcm): where in the audio was each phrase said; result[k] = the hits of phrases[k], best first.
    /// Needs the vocabulary and a model with a CTC head (the tdt-600m preset has none: the call throws).
    std::vector<std::vector<SpotHit>> spot(const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot_file(audio_path, phrases, opts);
    }
    std::vector<std::vector<SpotHit>> spot(const float *pcm, size_t n, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(pcm, n, phrases, opts);
    }
    std::vector<std::vector<SpotHit>> spot(const std::vector<float> &samples, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(samples.data(), samples.size(), phrases, opts);
    }
    /// New: keyword spotting through the TDT head (pk_tdt_spot_pcm): works without a CTC head.  A phrase is scored as if it
    /// began the utterance; score 0: greedy TDT decoding with that context emits the phrase there.
    std::vector<std::vector<SpotHit>> spot_tdt(const std::string &audio_path, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot_file(audio_path, phrases, opts, true);
    }
    std::vector<std::vector<SpotHit>> spot_tdt(const float *pcm, size_t n, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(pcm, n, phrases, opts, true);
    }
    std::vector<std::vector<SpotHit>> spot_tdt(const std::vector<float> &samples, const std::vector<std::string> &phrases, const SpotOptions &opts = {}) {
        return eng_.run_spot(samples.data(), samples.size(), phrases, opts, true);
    }
    /// New: the same through the TDT head (pk_tdt_align_pcm): works without a CTC head.  AlignResult::total is 0.
    AlignResult align_tdt(const std::string &audio_path, const std::string &text) { return eng_.run_align_file(audio_path, text, true); }
    AlignResult align_tdt(const float *pcm, size_t n, const std::string &text) { return eng_.run_align(pcm, n, text, true); }
    AlignResult align_tdt(const std::vector<float> &samples, const std::string &text) { return eng_.run_align(samples.data(), samples.size(), text, true); }
    /// New: TDT beam search with n-best output: hypotheses best first, score = the path's log-probability.
    std::vector<ScoredResult> transcribe_nbest(const std::string &audio_path, const TdtBeamOptions &opts = {}) { return eng_.run_nbest_tdt_file(audio_path, opts); }
    std::vector<ScoredResult> transcribe_nbest(const float *pcm, size_t n, const TdtBeamOptions &opts = {}) { return eng_.run_nbest_tdt(pcm, n, opts); }
    std::vector<ScoredResult> transcribe_nbest(const std::vector<float> &samples, const TdtBeamOptions &opts = {}) {
        return eng_.run_nbest_tdt(samples.data(), samples.size(), opts);
    }
    /// New: the list re-ranked by a Transformer LM (pk_nbest_rescore_nlm): score + am_score + nlm_score
    std::vector<NlmScoredResult> transcribe_nbest(const std::string &audio_path, const TdtBeamOptions &opts, const NeuralLanguageModel &nlm, const NlmOptions &no = {}) {
        return eng_.run_nbest_nlm_file(audio_path, opts, nlm, no);
    }
    /// New: the search with n-gram LM shallow fusion (pk_transcribe_pcm_nbest_tdt_lm): fused order, score + lm_score
    std::vector<LmScoredResult> transcribe_nbest(const std::string &audio_path, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_tdt_lm_file(audio_path, opts, lm, lm_opts);
    }
    std::vector<LmScoredResult> transcribe_nbest(const float *pcm, size_t n, const TdtBeamOptions &opts, const LanguageModel &lm, const LmOptions &lm_opts = {}) {
        return eng_.run_nbest_tdt_lm(pcm, n, opts, lm, lm_opts);
    }
    /// New: the log-likelihood of a given transcript: tdt_head = true through the TDT head's forward algorithm
    /// (pk_tdt_score_pcm; no CTC head needed).  false throws std::invalid_argument: the CTC head's log-likelihood is align()'s AlignResult::total.
    ScoreResult score(const std::string &audio_path, const std::string &text, bool tdt_head = true) { return eng_.run_score_file(audio_path, text, tdt_head); }
    ScoreResult score(const float *pcm, size_t n, const std::string &text, bool tdt_head = true) { return eng_.run_score(pcm, n, text, tdt_head); }
    ScoreResult score(const std::vector<float> &samples, const std::string &text, bool tdt_head = true) {
        return eng_.run_score(samples.data(), samples.size(), text, tdt_head);
    }

    pk_model *model() { return eng_.handle(); }

  private:
    static TranscribeOptions options(bool ts) {
        TranscribeOptions o;
        o.timestamps = ts;
        return o;
    }
    static TranscribeOptions tdt(TranscribeOptions o) {
        o.decoder = Decoder::TDT;
        return o;
    }
    TDTConfig config_;
    detail::Engine eng_;
};

}  // namespace parakeet
