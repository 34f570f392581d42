// parakeet.cpp_amd/csrc/capi_stream_endpoint.cpp -- the extern "C" boundary of the endpointing on live audio (stream_endpoint.hpp, DESIGN.md
// 5.5.10): the kernel and the rule alone on host rows, and the endpointer of a streaming session.
#include <algorithm>
#include <vector>

#include "capi_util.hpp"
#include "stream.hpp"

using namespace pk;

struct pk_endpoint_chunk { EndpointChunk w; DevBuf rows; };

static void need_events(const pk_endpoint_event *events, int cap, const int *n_events) {
    need(n_events != nullptr && cap >= 0 && (events || cap == 0), "events/cap/n_events");
}

extern "C" {

void pk_endpoint_options_default(pk_endpoint_options *out) {
    if (out) *out = endpoint_options_of(nullptr);
}

pk_status pk_endpoint_chunk_create(int n_streams, int n_mels, const pk_endpoint_options *opt, pk_endpoint_chunk **out) {
    return guard([&] {
        need(out && n_streams >= 1, "out/n_streams");
        const EndpointParams p = endpoint_params(endpoint_options_of(opt), n_mels, 0, 0);      // (host only: refuses before a device is looked for)
        auto h = std::make_unique<pk_endpoint_chunk>();
        h->w.setup(n_streams, n_mels, p);
        need_device();
        h->w.alloc(nullptr);
        PK_HIP(hipStreamSynchronize(nullptr));
        *out = h.release();
    });
}

pk_status pk_endpoint_chunk_push(pk_endpoint_chunk *h, const float *rows, int n, float *level, float *floor, int32_t *speech0,
                                 pk_endpoint_event *events, int cap, int *n_events) {
    return guard([&] {
        need(h && rows, "endpointer/rows");
        need_events(events, cap, n_events);
        EndpointChunk &w = h->w;
        w.check_frames(n);
        const size_t bytes = (size_t)w.S * n * w.F * 4;
        h->rows.reserve(bytes);
        PK_HIP(hipMemcpyAsync(h->rows.p, rows, bytes, hipMemcpyHostToDevice, nullptr));
        w.run(h->rows.as<float>(), n, level || floor || speech0, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(nullptr));
        std::vector<std::vector<pk_endpoint_event>> per;
        w.take(per);
        put_endpoint_events(per, events, cap, n_events);
        w.take_rows(level, floor, speech0);
    });
}

pk_status pk_endpoint_chunk_close(pk_endpoint_chunk *h, const uint8_t *mask) {
    return guard([&] {
        need(h && mask, "endpointer/mask");
        std::vector<unsigned char> bits(h->w.S);
        for (int s = 0; s < h->w.S; ++s) bits[s] = mask[s] ? 2 : 0;
        h->w.close(bits, nullptr, nullptr, 0, 0, nullptr, 0, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(nullptr));
    });
}

pk_status pk_endpoint_chunk_reset(pk_endpoint_chunk *h) {
    return guard([&] {
        need(h != nullptr, "endpointer");
        h->w.clear(nullptr);
        PK_HIP(hipStreamSynchronize(nullptr));
    });
}

void pk_endpoint_chunk_free(pk_endpoint_chunk *h) { delete h; }

pk_status pk_stream_set_endpointing(pk_stream *s, const pk_endpoint_options *opt) {
    return guard([&] {
        need(s != nullptr, "stream");
        s->s->set_endpointing(opt);
    });
}

pk_status pk_stream_endpoint(pk_stream *s, const float *mel_rows, int n_frames, float *level, float *floor, int32_t *speech0,
                             pk_endpoint_event *events, int cap, int *n_events) {
    return guard([&] {
        need(s && mel_rows, "stream/mel_rows");
        need_events(events, cap, n_events);
        s->s->endpoint(mel_rows, n_frames, level, floor, speech0, events, cap, n_events);
    });
}

pk_status pk_stream_push_endpoint(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                                  int32_t *end, float *conf, pk_endpoint_event *events, int cap, int *n_events, pk_kws_event *kws_events,
                                  int kws_cap, int *kws_n_events) {
    return guard([&] {
        if (!s || !pcm || !ids || !lens || n_samples <= 0 || max_tokens <= 0) fail(PK_ERR_INVALID, "invalid argument: stream/pcm/ids/lens/sizes");
        need_events(events, cap, n_events);
        if (kws_events || kws_n_events) need(kws_n_events != nullptr && kws_cap >= 0 && (kws_events || kws_cap == 0), "kws_events/kws_cap/kws_n_events");
        s->s->push_endpoint(pcm, n_samples, max_tokens, ids, lens, start, end, conf, events, cap, n_events, kws_events, kws_cap, kws_n_events);
    });
}

pk_status pk_stream_reset_decoder(pk_stream *s, const uint8_t *mask) {
    return guard([&] {
        need(s && mask, "stream/mask");
        s->s->reset_decoder(mask);
    });
}

pk_status pk_stream_endpoint_timed(pk_stream *s, const float *mel_rows, int n_frames, int reps, float ms[1]) {
    return guard([&] {
        need(s && mel_rows && ms && reps > 0, "stream/mel_rows/ms/reps");
        std::vector<float> t;
        for (int r = 0; r <= reps; ++r) {                          // (the first pass warms the buffers up and is not counted)
            float v = 0.0f;
            int n = 0;
            s->s->endpoint(mel_rows, n_frames, nullptr, nullptr, nullptr, nullptr, 0, &n, &v);
            if (r > 0) t.push_back(v);
        }
        std::sort(t.begin(), t.end());
        ms[0] = t[t.size() / 2];
    });
}

}  // extern "C"
