// parakeet/nemotron.hpp -- streaming drop-in: parakeet::NemotronTranscriber (reference include/parakeet/nemotron.hpp:54-133,
// src/nemotron.cpp:14-66) on the MI355X engine's streaming C ABI (pk_stream_*, include/parakeet_amd.h).
//
//   parakeet::NemotronTranscriber t("nemotron.safetensors", "vocab.txt", parakeet::make_nemotron_600m_config(/*latency_frames=*/1));
//   t.to_gpu();
//   while (have_audio) text += t.transcribe_chunk(pcm, n);      // new text of this chunk ("" while audio is being buffered)
//
// One object = one stream (the C ABI advances n lock-step streams per pk_stream for throughput: pk_stream_create(model, 16, ...)).
// Differences a caller can observe: the axiom::Tensor overload of transcribe_chunk becomes (const float*, size_t), which the
// reference also has (nemotron.hpp:93-96); there is no CPU path (the first chunk places the model on GPU 0 if to_gpu() was not
// called); weights load strictly.  The decode quirk of the reference is kept: transcribe_chunk decodes with the DEFAULT blank id
// of rnnt_streaming_decode_chunk, 1024 (nemotron.cpp:40-42, eou.hpp:91-94), whatever the vocabulary size.
#pragma once
#include <limits>

#include <functional>
#include <string>
#include <vector>

#include "transcribe.hpp"

namespace parakeet {

struct StreamingEncoderConfig : EncoderConfig {   // include/parakeet/streaming_encoder.hpp:17-23
    int att_context_left = 70;
    int att_context_right = 0;
    int chunk_size = 20;
};

struct NemotronConfig {                            // include/parakeet/nemotron.hpp:20-29
    StreamingEncoderConfig encoder;
    PredictionConfig prediction;
    JointConfig joint;
    std::vector<int> durations = {0, 1, 2, 3, 4};
    int latency_frames = 0;
};

inline NemotronConfig make_nemotron_600m_config(int latency_frames = 0) {   // nemotron.hpp:31-52
    NemotronConfig cfg;
    detail::set_encoder(cfg.encoder, 80, 1024, 24, 4096);
    detail::set_decoder(cfg.prediction, cfg.joint, 1024, 8193, 2);
    cfg.encoder.att_context_left = 70;
    cfg.encoder.att_context_right = latency_frames;
    cfg.encoder.chunk_size = 20;
    cfg.latency_frames = latency_frames;
    return cfg;
}

using PartialResultCallback = std::function<void(const std::string &partial)>;

struct EOUConfig {                                 // include/parakeet/eou.hpp:25-32
    StreamingEncoderConfig encoder;
    PredictionConfig prediction;
    JointConfig joint;
    std::vector<int> durations = {0, 1, 2, 3, 4};
    int eou_token_id = -1;
    int ctc_vocab_size = 1025;
};

inline EOUConfig make_eou_120m_config() {          // eou.hpp:34-56
    EOUConfig cfg;
    detail::set_encoder(cfg.encoder, 80, 512, 17, 2048);
    detail::set_decoder(cfg.prediction, cfg.joint, 512, 1025, 1);
    cfg.encoder.att_context_left = 70;
    cfg.encoder.att_context_right = 1;
    cfg.encoder.chunk_size = 20;
    cfg.eou_token_id = 1024;
    return cfg;
}

/// Options of the streaming keyword spotting (pk_stream_kws_options) and one hit as it leaves: seconds by the rule of the word timestamps,
/// start_frame * 0.08 and (end_frame + 1) * 0.08, frames counted from the start of the session.
struct StreamSpotOptions {
    float min_score = -std::numeric_limits<float>::infinity();
    int patience = 0;
};
struct SpotEvent {
    int keyword = 0;
    float start = 0.0f, end = 0.0f, score = 0.0f;
    int start_frame = 0, end_frame = 0;
};

/// Options of the endpointing on live audio (pk_endpoint_options; the defaults are the library's, choices and not measurements) and one finished
/// utterance: the tokens returned since the previous one ended, seconds at frame * 0.01 (10 ms mel frames counted from the start of the session).
struct EndpointOptions {
    float threshold_db = -50.0f, margin_db = 9.0f;
    int floor_window_ms = 3000, min_speech_ms = 100, min_silence_ms = 500;
    float max_utterance_s = 30.0f;
    int eou_token_id = -1;
    bool reset_decoder = true;
};
struct Utterance {
    std::string text;
    std::vector<int> ids;
    float start = 0.0f, end = 0.0f;
    int reason = 0;             ///< PK_ENDPOINT_SILENCE / _MAX_LENGTH / _TOKEN
};

namespace detail {

/// One streaming session on pk_stream_* : the body shared by NemotronTranscriber and StreamingTranscriber (both are
/// process_chunk -> forward_chunk -> rnnt_streaming_decode_chunk with the DEFAULT blank id 1024: nemotron.cpp:24-52, eou.cpp:113-146).
class StreamSession {
  public:
    StreamSession(const std::string &weights_path, const std::string &vocab_path, const StreamingEncoderConfig &enc, const PredictionConfig &pred,
                  const JointConfig &joint, const std::vector<int> &durations)
        : left_(enc.att_context_left), right_(enc.att_context_right),
          eng_(weights_path, vocab_path, flatten(enc, pred, joint, durations, 0, "joint_.", false, /*blank_id=*/1024)) {}
    ~StreamSession() { pk_stream_free(stream_); }
    StreamSession(const StreamSession &) = delete;
    StreamSession &operator=(const StreamSession &) = delete;

    void to_gpu() { eng_.to_gpu(0); on_gpu_ = true; }

    /// Process a chunk of raw float32 PCM (16 kHz mono) -> the new text of this chunk.
    std::string transcribe_chunk(const float *data, size_t num_samples) {
        if (num_samples == 0) return "";
        ensure_stream();
        const int mt = 256;
        std::vector<int32_t> ids(mt), start(mt), end(mt);
        std::vector<float> conf(mt);
        int32_t len = 0;
        detail::check(pk_stream_push(stream_, data, (int)num_samples, mt, ids.data(), &len, start.data(), end.data(), conf.data()));
        return take_tokens(ids, start, end, conf, len);
    }

  private:
    std::string take_tokens(const std::vector<int32_t> &ids, const std::vector<int32_t> &start, const std::vector<int32_t> &end,
                            const std::vector<float> &conf, int32_t len) {
        if (len <= 0) return "";
        std::vector<int> fresh(ids.begin(), ids.begin() + len);
        tokens_.insert(tokens_.end(), fresh.begin(), fresh.end());
        for (int i = 0; i < len; ++i) timestamped_.push_back({ids[i], start[i], end[i], conf[i]});
        if (!eng_.tokenizer().loaded()) return "";
        const std::string text = eng_.tokenizer().decode(fresh);
        if (partial_callback_) partial_callback_(text);
        return text;
    }
    static void append_events(const std::vector<pk_kws_event> &ev, int n, std::vector<SpotEvent> &out) {
        for (int i = 0; i < n && i < (int)ev.size(); ++i) {
            SpotEvent e;
            e.keyword = ev[i].keyword; e.score = ev[i].score; e.start_frame = ev[i].start; e.end_frame = ev[i].end;
            e.start = (float)ev[i].start * 0.08f; e.end = (float)(ev[i].end + 1) * 0.08f;
            out.push_back(e);
        }
    }

  public:
    /// Wake words on live audio (pk_stream_set_keywords): the phrases are watched by every transcribe_chunk_spot from here on; an empty list clears them.
    void set_keywords(const std::vector<std::string> &phrases, const StreamSpotOptions &opts = StreamSpotOptions()) {
        ensure_stream();
        std::vector<const char *> p;
        for (const std::string &s : phrases) p.push_back(s.c_str());
        pk_stream_kws_options o;
        o.min_score = opts.min_score; o.patience = opts.patience;
        detail::check(pk_stream_set_keywords(stream_, p.data(), nullptr, nullptr, (int)p.size(), &o));
        n_kw_ = (int)p.size();
    }
    /// transcribe_chunk that also spots the keywords in the chunk's frames: the hits that leave with this chunk are appended to `events`.
    std::string transcribe_chunk_spot(const float *data, size_t num_samples, std::vector<SpotEvent> &events) {
        if (num_samples == 0) return "";
        ensure_stream();
        const int mt = 256, cap = n_kw_ * 62;
        std::vector<int32_t> ids(mt), start(mt), end(mt);
        std::vector<float> conf(mt);
        std::vector<pk_kws_event> ev(cap > 0 ? cap : 1);
        int32_t len = 0;
        int n_ev = 0;
        detail::check(pk_stream_push_spot(stream_, data, (int)num_samples, mt, ids.data(), &len, start.data(), end.data(), conf.data(), ev.data(), cap,
                                          &n_ev));
        append_events(ev, n_ev, events);
        return take_tokens(ids, start, end, conf, len);
    }
    /// The hits still held back (pk_stream_spot_flush): call at the end of the audio.
    void flush_spots(std::vector<SpotEvent> &events) {
        if (!stream_ || n_kw_ == 0) return;
        std::vector<pk_kws_event> ev(n_kw_);
        int n_ev = 0;
        detail::check(pk_stream_spot_flush(stream_, ev.data(), n_kw_, &n_ev));
        append_events(ev, n_ev, events);
    }

    /// End of turn on live audio (pk_stream_set_endpointing): every transcribe_chunk_endpoint from here on feeds the endpointer.
    void set_endpointing(const EndpointOptions &opts = EndpointOptions()) {
        ensure_stream();
        pk_endpoint_options o;
        o.threshold_db = opts.threshold_db; o.margin_db = opts.margin_db; o.floor_window_ms = opts.floor_window_ms;
        o.min_speech_ms = opts.min_speech_ms; o.min_silence_ms = opts.min_silence_ms; o.max_utterance_s = opts.max_utterance_s;
        o.eou_token_id = opts.eou_token_id; o.reset_decoder = opts.reset_decoder ? 1 : 0;
        detail::check(pk_stream_set_endpointing(stream_, &o));
        utt_ids_.clear();
    }
    /// transcribe_chunk that also watches for the end of the utterance: an utterance that ended in this chunk is appended to `finished` with the tokens
    /// returned since the previous one ended (this chunk's included).
    std::string transcribe_chunk_endpoint(const float *data, size_t num_samples, std::vector<Utterance> &finished) {
        if (num_samples == 0) return "";
        ensure_stream();
        const int mt = 256, cap = 513;
        std::vector<int32_t> ids(mt), start(mt), end(mt);
        std::vector<float> conf(mt);
        std::vector<pk_endpoint_event> ev(cap);
        int32_t len = 0;
        int n_ev = 0;
        detail::check(pk_stream_push_endpoint(stream_, data, (int)num_samples, mt, ids.data(), &len, start.data(), end.data(), conf.data(), ev.data(), cap,
                                              &n_ev, nullptr, 0, nullptr));
        utt_ids_.insert(utt_ids_.end(), ids.begin(), ids.begin() + (len > 0 ? len : 0));
        for (int i = 0; i < n_ev && i < cap; ++i) {
            if (ev[i].kind != PK_ENDPOINT_END) continue;
            Utterance u;
            u.ids.swap(utt_ids_);
            u.start = (float)ev[i].start * 0.01f; u.end = (float)ev[i].end * 0.01f; u.reason = ev[i].reason;
            if (eng_.tokenizer().loaded() && !u.ids.empty()) u.text = eng_.tokenizer().decode(u.ids);
            finished.push_back(std::move(u));
        }
        return take_tokens(ids, start, end, conf, len);
    }

    /// int16 PCM convenience overload (nemotron.hpp:99-105)
    std::string transcribe_chunk(const int16_t *data, size_t num_samples) {
        std::vector<float> f(num_samples);
        for (size_t i = 0; i < num_samples; ++i) f[i] = static_cast<float>(data[i]) / 32768.0f;
        return transcribe_chunk(f.data(), num_samples);
    }

    /// Reset for a new utterance (nemotron.cpp:54-58)
    void reset() {
        if (stream_) detail::check(pk_stream_reset(stream_));
        tokens_.clear();
        timestamped_.clear();
        utt_ids_.clear();
    }
    /// Full transcription so far (nemotron.cpp:60-65)
    std::string get_text() const { return (eng_.tokenizer().loaded() && !tokens_.empty()) ? eng_.tokenizer().decode(tokens_) : ""; }
    void set_partial_callback(PartialResultCallback cb) { partial_callback_ = std::move(cb); }
    const std::vector<TimestampedToken> &get_timestamped_tokens() const { return timestamped_; }
    const Tokenizer &tokenizer() const { return eng_.tokenizer(); }

  private:
    void ensure_stream() {
        if (!on_gpu_) to_gpu();
        if (!stream_) detail::check(pk_stream_create(eng_.handle(), 1, left_, right_, &stream_));
    }
    int left_, right_;
    detail::Engine eng_;
    pk_stream *stream_ = nullptr;
    bool on_gpu_ = false;
    int n_kw_ = 0;
    std::vector<int> tokens_, utt_ids_;
    std::vector<TimestampedToken> timestamped_;
    PartialResultCallback partial_callback_;
};

}  // namespace detail

/// parakeet::NemotronTranscriber (reference include/parakeet/nemotron.hpp:73-133)
class NemotronTranscriber : public detail::StreamSession {
  public:
    NemotronTranscriber(const std::string &weights_path, const std::string &vocab_path, const NemotronConfig &config = make_nemotron_600m_config())
        : detail::StreamSession(weights_path, vocab_path, config.encoder, config.prediction, config.joint, config.durations), config_(config) {}

  private:
    NemotronConfig config_;
};

/// parakeet::StreamingTranscriber (reference include/parakeet/eou.hpp:101-160): the EOU model's streaming session.  As in the
/// reference's transcribe_chunk (src/eou.cpp:113-146) the end-of-utterance token id of the config takes no part in decoding.
class StreamingTranscriber : public detail::StreamSession {
  public:
    StreamingTranscriber(const std::string &weights_path, const std::string &vocab_path, const EOUConfig &config = make_eou_120m_config())
        : detail::StreamSession(weights_path, vocab_path, config.encoder, config.prediction, config.joint, config.durations), config_(config) {}

  private:
    EOUConfig config_;
};

}  // namespace parakeet
