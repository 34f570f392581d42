// parakeet.cpp_amd/csrc/stream_endpoint.cpp -- sizes and launches the endpointing on live audio and owns its carried state.
#include "stream_endpoint.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pk {

static const char *const kWhat = "endpointing";

pk_endpoint_options endpoint_options_of(const pk_endpoint_options *opt) {
    pk_endpoint_options o;
    o.threshold_db = -50.0f; o.margin_db = 9.0f; o.floor_window_ms = 3000; o.min_speech_ms = 100; o.min_silence_ms = 500; o.max_utterance_s = 30.0f;
    o.eou_token_id = -1; o.reset_decoder = 1;
    return opt ? *opt : o;
}

EndpointParams endpoint_params(const pk_endpoint_options &o, int F, int V, int blank) {
    EndpointParams p;
    p.W = o.floor_window_ms / 10; p.min_speech = o.min_speech_ms / 10; p.min_silence = o.min_silence_ms / 10;
    const double mu = (double)o.max_utterance_s * 100.0;
    p.max_utterance = std::isnan(mu) ? 0 : (int)std::min(std::max(mu, -1.0), 2.0e9);
    p.eou_token_id = o.eou_token_id; p.reset_decoder = o.reset_decoder ? 1 : 0;
    if (p.min_speech < 1 || p.min_silence < 1 || p.W < 1)
        fail(PK_ERR_INVALID, "invalid argument: min_speech_ms %d, min_silence_ms %d, floor_window_ms %d: each at least one 10 ms frame", o.min_speech_ms,
             o.min_silence_ms, o.floor_window_ms);
    if (p.max_utterance < p.min_speech + 1)
        fail(PK_ERR_INVALID, "invalid argument: max_utterance_s %g: %d frames, at least min_speech + 1 = %d", (double)o.max_utterance_s, p.max_utterance,
             p.min_speech + 1);
    if (std::isnan(o.threshold_db) || std::isnan(o.margin_db)) fail(PK_ERR_INVALID, "invalid argument: threshold_db / margin_db is NaN");
    if (o.eou_token_id < -1 || (V > 0 && (o.eou_token_id >= V || o.eou_token_id == blank)))
        fail(PK_ERR_INVALID, "invalid argument: eou_token_id %d: -1 or a token of the vocabulary other than the blank", o.eou_token_id);
    if (F < 1) fail(PK_ERR_INVALID, "invalid argument: n_mels %d", F);
    if (p.W > kEndpointMaxWindow) fail(PK_ERR_UNSUPPORTED, "%s: a floor window of %d frames, at most %d", kWhat, p.W, kEndpointMaxWindow);
    if (F > kEndpointMaxBins) fail(PK_ERR_UNSUPPORTED, "%s: %d mel bins, at most %d", kWhat, F, kEndpointMaxBins);
    const double k = std::log(10.0) / 10.0;
    p.abs_thr = (float)(F * (double)o.threshold_db * k);
    p.margin = (float)(F * (double)o.margin_db * k);
    return p;
}

EndpointChunk::~EndpointChunk() {
    if (pin_) (void)hipHostFree(pin_);
}

void EndpointChunk::setup(int S_, int F_, const EndpointParams &p_) {
    if (S_ < 1) fail(PK_ERR_INVALID, "invalid argument: n_streams %d", S_);
    S = S_; F = F_; p = p_; t0 = 0; n = 0;
    nev_words_ = ((size_t)S + 3) / 4 * 4;
}

void EndpointChunk::alloc(hipStream_t s) {
    ring_.reserve((size_t)S * p.W * 4);
    // (sized for the largest call at once: the state in front of the events must not move)
    out_.reserve(((size_t)S * kEndpointStateWords + nev_words_ + (size_t)S * kEndpointMaxFrames * 4) * 4);
    mask_.reserve((size_t)S);
    clear(s);
}

void EndpointChunk::clear(hipStream_t s) {
    PK_HIP(hipMemsetAsync(ring_.p, 0xFF, (size_t)S * p.W * 4, s));
    PK_HIP(hipMemsetAsync(out_.p, 0, (size_t)S * kEndpointStateWords * 4, s));
    t0 = 0;
}

void EndpointChunk::check_frames(int n_) const {
    if (n_ < 1) fail(PK_ERR_INVALID, "invalid argument: %s: a call with no rows", kWhat);
    if (n_ > kEndpointMaxFrames) fail(PK_ERR_UNSUPPORTED, "%s: %d frames in one call, at most %d", kWhat, n_, kEndpointMaxFrames);
}

void EndpointChunk::run(const float *d_rows, int n_, bool rows, hipStream_t s, hipEvent_t *ev) {
    check_frames(n_);
    n = n_;
    const size_t head_bytes = ((size_t)S * kEndpointStateWords + nev_words_ + (size_t)S * n * 4) * 4, row_bytes = (size_t)S * n * 12;
    if (head_bytes + row_bytes > pin_bytes_) {                       // (no copy of an earlier call is in flight: every entry point ends synchronised)
        if (pin_) { PK_HIP(hipHostFree(pin_)); pin_ = nullptr; pin_bytes_ = 0; }
        PK_HIP(hipHostMalloc(&pin_, head_bytes + row_bytes, hipHostMallocDefault));
        pin_bytes_ = head_bytes + row_bytes;
    }
    if (rows) rows_.reserve(row_bytes);
    EndpointChunkArgs k{};
    k.rows = d_rows; k.ring = ring_.as<unsigned>(); k.state = out_.as<int>();
    k.n_ev = out_.as<int>() + (size_t)S * kEndpointStateWords;
    k.ev = reinterpret_cast<int4 *>(k.n_ev + nev_words_);
    if (rows) { k.level = rows_.as<float>(); k.floor = k.level + (size_t)S * n; k.speech0 = reinterpret_cast<int *>(k.floor + (size_t)S * n); }
    k.S = S; k.t0 = t0; k.n = n; k.F = F; k.W = p.W;
    k.min_speech = p.min_speech; k.min_silence = p.min_silence; k.max_utterance = p.max_utterance;
    k.abs_thr = p.abs_thr; k.margin = p.margin;
    if (ev) PK_HIP(hipEventRecord(ev[0], s));
    launch_endpoint_chunk(k, s);
    if (ev) PK_HIP(hipEventRecord(ev[1], s));
    PK_HIP(hipMemcpyAsync(pin_, out_.p, head_bytes, hipMemcpyDeviceToHost, s));
    if (rows) PK_HIP(hipMemcpyAsync(static_cast<char *>(pin_) + head_bytes, rows_.p, row_bytes, hipMemcpyDeviceToHost, s));
    rows_copied_ = rows;
    t0 += n;
}

void EndpointChunk::take(std::vector<std::vector<pk_endpoint_event>> &per_stream) const {
    const int32_t *nev = static_cast<const int32_t *>(pin_) + (size_t)S * kEndpointStateWords, *ev = nev + nev_words_;
    per_stream.assign(S, {});
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < nev[s] && k < n; ++k) {
            const int32_t *v = ev + ((size_t)s * n + k) * 4;
            pk_endpoint_event e;
            e.stream = s; e.kind = v[0] & 0xFF; e.reason = v[0] >> 8; e.start = v[1]; e.end = v[2]; e.at = v[3];
            per_stream[s].push_back(e);
        }
}

void EndpointChunk::take_rows(float *level, float *floor, int32_t *speech0) const {
    if (!rows_copied_) return;
    const size_t head_bytes = ((size_t)S * kEndpointStateWords + nev_words_ + (size_t)S * n * 4) * 4, nb = (size_t)S * n * 4;
    const char *r = static_cast<const char *>(pin_) + head_bytes;
    if (level) memcpy(level, r, nb);
    if (floor) memcpy(floor, r + nb, nb);
    if (speech0) memcpy(speech0, r + 2 * nb, nb);
}

void EndpointChunk::close(const std::vector<unsigned char> &bits, float *h, float *c, int Ln, int Hp, int *token, int blank, hipStream_t s) {
    PK_HIP(hipMemcpyAsync(mask_.p, bits.data(), (size_t)S, hipMemcpyHostToDevice, s));
    launch_endpoint_close(mask_.as<unsigned char>(), S, h, c, Ln, Hp, token, blank, out_.as<int>(), s);
}

void put_endpoint_events(const std::vector<std::vector<pk_endpoint_event>> &per_stream, pk_endpoint_event *events, int cap, int *n_events) {
    int n = 0;
    for (const auto &v : per_stream)
        for (const pk_endpoint_event &e : v) {
            if (n < cap) events[n] = e;
            ++n;
        }
    if (n_events) *n_events = n;
}

void reset_decoder_rows(const uint8_t *mask, int S, float *h, float *c, int Ln, int Hp, int *token, int blank, DevBuf &d_mask, hipStream_t s) {
    std::vector<unsigned char> bits(S);
    for (int i = 0; i < S; ++i) bits[i] = mask[i] ? 1 : 0;
    d_mask.reserve((size_t)S);
    PK_HIP(hipMemcpyAsync(d_mask.p, bits.data(), (size_t)S, hipMemcpyHostToDevice, s));
    launch_endpoint_close(d_mask.as<unsigned char>(), S, h, c, Ln, Hp, token, blank, nullptr, s);
    PK_CHECK_LAUNCH();
    PK_HIP(hipStreamSynchronize(s));
}

}  // namespace pk
