// parakeet.cpp_amd/csrc/capi.cpp -- the model-level part of the extern "C" boundary declared in include/parakeet_amd.h: version, last error,
// device count, presets, model load / free / setters, frame counts, tokenizer, boost phrases, word grouping, audio I/O.
// Every entry point translates pk::Error / std::exception into a status code + thread-local message (guard, capi_util.hpp).
#include <cstring>

#include "capi_util.hpp"

using namespace pk;

// ContextTrie::build (src/phrase_boost.cpp:29-37): Tokenizer::encode of every phrase
std::vector<std::vector<int>> pk::encode_phrases(Model &m, const char *const *phrases, int n) {
    if (!m.tok.loaded()) fail(PK_ERR_INVALID, "boost phrases need a vocabulary (the model was loaded without one)");
    std::vector<std::vector<int>> ph;
    for (int i = 0; i < n; ++i) {
        need(phrases[i] != nullptr, "phrases[i]");
        auto v = m.tok.encode(phrases[i]);
        if (!v.empty()) ph.push_back(std::move(v));               // ContextTrie::build skips phrases that encode to nothing
    }
    if (ph.empty() && n > 0) ph.emplace_back();                   // a root-only trie: boosting on, nothing boosted
    return ph;
}

extern "C" {

const char *pk_version(void) { return "parakeet.cpp_amd 0.1 (gfx950)"; }

size_t pk_last_error(char *buf, size_t cap) {
    const std::string &e = last_error();
    if (buf && cap) {
        const size_t n = e.size() < cap - 1 ? e.size() : cap - 1;
        memcpy(buf, e.data(), n);
        buf[n] = 0;
    }
    return e.size();
}

int pk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

pk_status pk_config_preset(const char *name, pk_config *out) {
    return guard([&] {
        need(name && out, "name/out");
        pk_config c;
        memset(&c, 0, sizeof c);
        c.mel_bins = 80; c.subsampling_channels = 256; c.num_heads = 8; c.conv_kernel_size = 9;
        c.pred_hidden = 640; c.joint_hidden = 640; c.max_symbols_per_step = 10;
        const std::string n = name;
        if (n == "tdt-ctc-110m") {              // make_110m_config, config.hpp:77-95
            c.hidden_size = 512; c.num_layers = 17; c.ffn_intermediate = 2048; c.vocab_size = 1025; c.num_lstm_layers = 1;
            c.num_durations = 5; c.ctc_vocab_size = 1025; c.blank_id = 1024;
            snprintf(c.joint_prefix, sizeof c.joint_prefix, "tdt_joint_.");
        } else if (n == "tdt-600m") {           // make_tdt_600m_config, config.hpp:98-116
            c.mel_bins = 128; c.hidden_size = 1024; c.num_layers = 24; c.ffn_intermediate = 4096; c.vocab_size = 8193;
            c.num_lstm_layers = 2; c.num_durations = 5; c.ctc_vocab_size = 0; c.blank_id = 8192;
            snprintf(c.joint_prefix, sizeof c.joint_prefix, "joint_.");
        } else if (n == "rnnt-600m") {          // make_rnnt_600m_config, config.hpp:119-135
            c.hidden_size = 1024; c.num_layers = 24; c.ffn_intermediate = 4096; c.vocab_size = 1025; c.num_lstm_layers = 2;
            c.num_durations = 0; c.ctc_vocab_size = 0; c.blank_id = 1024; c.rnnt_head = 1;
            snprintf(c.joint_prefix, sizeof c.joint_prefix, "joint_.");
        } else if (n == "eou-120m") {           // make_eou_120m_config, eou.hpp:34-56 (streaming: use with pk_stream_*, context 70 / 1)
            c.hidden_size = 512; c.num_layers = 17; c.ffn_intermediate = 2048; c.vocab_size = 1025; c.num_lstm_layers = 1;
            c.num_durations = 5; c.ctc_vocab_size = 0; c.blank_id = 1024;
            snprintf(c.joint_prefix, sizeof c.joint_prefix, "joint_.");
        } else if (n == "nemotron-600m") {      // make_nemotron_600m_config, nemotron.hpp:31-52 (streaming: use with pk_stream_*)
            c.hidden_size = 1024; c.num_layers = 24; c.ffn_intermediate = 4096; c.vocab_size = 8193; c.num_lstm_layers = 2;
            c.num_durations = 5; c.ctc_vocab_size = 0;
            c.blank_id = 1024;                  // transcribe_chunk decodes with the DEFAULT blank_id of eou.hpp:91-94 (nemotron.cpp:40-42): kept literally
            snprintf(c.joint_prefix, sizeof c.joint_prefix, "joint_.");
        } else {
            fail(PK_ERR_INVALID, "unknown preset '%s'", name);
        }
        for (int i = 0; i < c.num_durations; ++i) c.durations[i] = i;
        *out = c;
    });
}

pk_status pk_model_load(const char *safetensors_path, const char *vocab_path, const pk_config *cfg, pk_model **out) {
    return guard([&] {
        need(safetensors_path && cfg && out, "path/cfg/out");
        auto h = std::make_unique<pk_model>();
        h->m = std::make_unique<Model>(safetensors_path, vocab_path ? vocab_path : "", *cfg);
        *out = h.release();
    });
}

pk_status pk_model_load_buffer(const void *safetensors_image, size_t n_bytes, const char *vocab_path, const pk_config *cfg, pk_model **out) {
    return guard([&] {
        need(safetensors_image && n_bytes > 0 && cfg && out, "image/n_bytes/cfg/out");
        auto h = std::make_unique<pk_model>();
        h->m = std::make_unique<Model>(safetensors_image, n_bytes, vocab_path ? vocab_path : "", *cfg);
        *out = h.release();
    });
}

pk_status pk_model_to_gpu(pk_model *m, int device) {
    return guard([&] { need(m, "model"); m->m->to_gpu(device); });
}

void pk_model_free(pk_model *m) { delete m; }

pk_status pk_model_set_decode_loop(pk_model *m, int mode) {
    return guard([&] {
        need(m, "model");
        need(mode == PK_DECODE_LOOP_PHASES || mode == PK_DECODE_LOOP_PERSISTENT || mode == PK_DECODE_LOOP_GRAPH, "mode");
        m->m->decode_loop = mode;
    });
}

pk_status pk_model_set_attention_context(pk_model *m, int left, int right) {
    return guard([&] { need(m, "model"); m->m->set_attention_context(left, right); });
}

pk_status pk_model_get_attention_context(const pk_model *m, int *left, int *right) {
    return guard([&] {
        need(m && left && right, "model/left/right");
        *left = m->m->att_left;
        *right = m->m->att_right;
    });
}

pk_status pk_model_config(const pk_model *m, pk_config *out) {
    return guard([&] { need(m && out, "model/out"); *out = m->m->cfg; });
}

int pk_mel_num_frames(int64_t n_samples) { return (int)(1 + n_samples / 160); }
int pk_encoder_num_frames(int n) {
    for (int i = 0; i < 3; ++i) n = (n - 1) / 2 + 1;
    return n;
}

// a malloc'ed copy for the caller (pk_free)
static void hand_over(const std::vector<float> &v, float **pcm, int64_t *n) {
    float *p = static_cast<float *>(malloc((v.size() ? v.size() : 1) * sizeof(float)));
    if (!p) fail(PK_ERR_IO, "out of memory");
    memcpy(p, v.data(), v.size() * sizeof(float));
    *pcm = p;
    *n = (int64_t)v.size();
}

pk_status pk_read_wav(const char *path, float **pcm, int64_t *n_samples, int *sample_rate) {
    return guard([&] {
        need(path && pcm && n_samples && sample_rate, "path/pcm/n_samples/sample_rate");
        std::vector<float> mono;
        int sr = 0;
        read_wav(path, mono, sr);
        hand_over(mono, pcm, n_samples);
        *sample_rate = sr;
    });
}
/* read_audio(path, target_sample_rate) (audio_io.cpp:453-483) restricted to RIFF/WAVE: decode, mono downmix, resample to
 * target_rate with the reference's Kaiser-windowed sinc (sinc_resample, :123-195). */
pk_status pk_read_audio(const char *path, int target_rate, float **pcm, int64_t *n_samples, int *original_rate) {
    return guard([&] {
        need(path && pcm && n_samples && target_rate > 0, "path/pcm/n_samples/target_rate");
        std::vector<float> mono, out;
        int sr = 0;
        read_wav(path, mono, sr);
        if (original_rate) *original_rate = sr;
        sinc_resample(mono.data(), mono.size(), sr, target_rate, out);
        hand_over(out, pcm, n_samples);
    });
}
/* resample() / read_audio(const float *pcm, n, sample_rate, target) (audio_io.cpp:250-262,506-514). */
/* read_audio(const uint8_t *data, size_t len, target) (audio_io.cpp:485-493), RIFF/WAVE images */
pk_status pk_read_audio_memory(const void *data, size_t len, int target_rate, float **pcm, int64_t *n_samples, int *original_rate, int *n_channels) {
    return guard([&] {
        need(data && len > 0 && pcm && n_samples && target_rate > 0, "data/len/pcm/n_samples/target_rate");
        std::vector<float> mono, out;
        int sr = 0;
        parse_wav(static_cast<const uint8_t *>(data), len, nullptr, mono, sr, n_channels, false);
        if (original_rate) *original_rate = sr;
        sinc_resample(mono.data(), mono.size(), sr, target_rate, out);
        hand_over(out, pcm, n_samples);
    });
}
/* get_audio_duration (audio_io.cpp:527-586): header walk only */
pk_status pk_audio_info(const char *path, int *sample_rate, int *n_channels, int64_t *n_frames) {
    return guard([&] {
        need(path != nullptr, "path");
        FILE *f = fopen(path, "rb");
        if (!f) fail(PK_ERR_IO, "Failed to open audio file: %s", path);
        std::vector<uint8_t> head(1 << 16);
        fseek(f, 0, SEEK_END);
        const long total = ftell(f);
        fseek(f, 0, SEEK_SET);
        const size_t got = fread(head.data(), 1, head.size(), f);
        fclose(f);
        head.resize(got);
        // only the head of the file is read; the data chunk's declared size (clamped to the file length) gives the frame count
        std::vector<float> mono;
        int sr = 0, ch = 0;
        parse_wav(head.data(), head.size(), path, mono, sr, &ch, true, total > 0 ? (size_t)total : 0);
        if (sample_rate) *sample_rate = sr;
        if (n_channels) *n_channels = ch;
        if (n_frames) *n_frames = (int64_t)wav_info_frames();
    });
}

pk_status pk_resample(const float *pcm, int64_t n, int src_rate, int dst_rate, float **out, int64_t *n_out) {
    return guard([&] {
        need(pcm && out && n_out && n >= 0 && src_rate > 0 && dst_rate > 0, "pcm/out/n/rates");
        std::vector<float> r;
        sinc_resample(pcm, (size_t)n, src_rate, dst_rate, r);
        hand_over(r, out, n_out);
    });
}
void pk_free(void *p) { free(p); }

/* ---- host-side text ---------------------------------------------------------------------------------------- */
int pk_vocab_size(const pk_model *m) { return m ? (int)m->m->tok.vocab_size() : 0; }

// The text entry points return a count (>= 0) or -1; like every other entry point no C++ exception may cross the ABI, so the
// bodies run under guard() and a failure (bad argument, std::bad_alloc) becomes -1 with pk_last_error() set.
int pk_detokenize(const pk_model *m, const int32_t *ids, int n, char *out, int cap) {
    int ret = -1;
    guard([&] {
        need(m && n >= 0 && (ids || n == 0), "model/ids/n");
        std::vector<int> v(ids, ids + n);
        const std::string s = m->m->tok.decode(v);
        if (out && cap > 0) {
            const int c = (int)s.size() < cap - 1 ? (int)s.size() : cap - 1;
            memcpy(out, s.data(), c);
            out[c] = 0;
        }
        ret = (int)s.size();
    });
    return ret;
}

int pk_tokenize(const pk_model *m, const char *text, int32_t *ids, int cap) {
    int ret = -1;
    guard([&] {
        need(m && text && (ids || cap <= 0), "model/text/ids");
        const auto v = m->m->tok.encode(text);
        for (int i = 0; i < (int)v.size() && i < cap; ++i) ids[i] = v[i];
        ret = (int)v.size();
    });
    return ret;
}

pk_status pk_set_boost_tokens(pk_model *h, const int32_t *ids, const int32_t *offsets, int n_phrases, float boost_score) {
    return guard([&] {
        need(h && n_phrases >= 0 && (n_phrases == 0 || (ids && offsets)), "model/ids/offsets/n_phrases");
        std::vector<std::vector<int>> ph;
        for (int i = 0; i < n_phrases; ++i) {
            need(offsets[i + 1] >= offsets[i], "offsets must be non-decreasing");
            ph.emplace_back(ids + offsets[i], ids + offsets[i + 1]);
        }
        h->m->set_boost(ph, boost_score);
    });
}

pk_status pk_set_boost_phrases(pk_model *h, const char *const *phrases, int n_phrases, float boost_score) {
    return guard([&] {
        need(h && n_phrases >= 0 && (n_phrases == 0 || phrases), "model/phrases/n_phrases");
        h->m->set_boost(encode_phrases(*h->m, phrases, n_phrases), boost_score);
    });
}

int pk_boost_trie_size(const pk_model *m) { return m && m->m->boost_on ? m->m->trie_nodes : 0; }

int pk_group_timestamps(const pk_model *m, const int32_t *ids, const int32_t *start, const int32_t *end, const float *conf, int n,
                        int sentences, char *words, int cap, float *wstart, float *wend, float *wconf, int wcap) {
    int ret = -1;
    guard([&] {
        need(m && n >= 0 && (n == 0 || (ids && start && end)), "model/ids/start/end/n");
        std::vector<TimestampedToken> tt(n);
        for (int i = 0; i < n; ++i) tt[i] = {ids[i], start[i], end[i], conf ? conf[i] : 1.0f};
        const auto w = group_timestamps(tt, m->m->tok.pieces(), sentences != 0);
        std::string joined;
        for (size_t i = 0; i < w.size(); ++i) {
            if (i) joined += '\n';
            joined += w[i].word;
            if ((int)i < wcap) {
                if (wstart) wstart[i] = w[i].start;
                if (wend) wend[i] = w[i].end;
                if (wconf) wconf[i] = w[i].confidence;
            }
        }
        if (words && cap > 0) {
            const int c = (int)joined.size() < cap - 1 ? (int)joined.size() : cap - 1;
            memcpy(words, joined.data(), c);
            words[c] = 0;
        }
        ret = (int)w.size();
    });
    return ret;
}

}  // extern "C"
