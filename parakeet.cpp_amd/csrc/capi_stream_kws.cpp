// parakeet.cpp_amd/csrc/capi_stream_kws.cpp -- the extern "C" boundary of the streaming TDT keyword spotting (stream_kws.hpp): the
// chunked walk on host lattices, and the keyword set of a streaming session.
#include <algorithm>
#include <vector>

#include "capi_util.hpp"
#include "stream.hpp"

using namespace pk;

struct pk_tdt_kws_chunk { KwsChunk w; int D = 0; };

static void need_events(const pk_kws_event *events, int cap, const int *n_events) {
    need(n_events != nullptr && cap >= 0 && (events || cap == 0), "events/cap/n_events");
}

extern "C" {

void pk_stream_kws_options_default(pk_stream_kws_options *out) {
    if (out) *out = stream_kws_options_of(nullptr);
}

pk_status pk_tdt_kws_chunk_create(const int32_t *durations, int D, int n_pairs, const int32_t *kw_len, const pk_stream_kws_options *opt,
                                  pk_tdt_kws_chunk **out) {
    return guard([&] {
        need(durations && kw_len && out && n_pairs >= 1, "durations/kw_len/out/n_pairs");
        const pk_stream_kws_options o = stream_kws_options_of(opt);
        stream_kws_check_options(o);
        std::vector<int32_t> off(1, 0);
        for (int p = 0; p < n_pairs && p <= kStreamKwsMaxPairs; ++p) {
            if (kw_len[p] < 1) fail(PK_ERR_INVALID, "invalid argument: keyword %d is empty", p);
            off.push_back(off.back() + std::min<int32_t>(kw_len[p], kKwsMaxLen + 1));      // (a longer one is refused by the setup; the sum stays small)
        }
        auto h = std::make_unique<pk_tdt_kws_chunk>();
        h->D = D;
        h->w.setup(durations, D, std::move(off), n_pairs > kStreamKwsMaxPairs ? 1 : n_pairs, 0, 0, o, 0);   // (host only: refuses before a device is looked for)
        need_device();
        h->w.alloc(nullptr);
        PK_HIP(hipStreamSynchronize(nullptr));
        *out = h.release();
    });
}

pk_status pk_tdt_kws_chunk_push(pk_tdt_kws_chunk *h, const float *lab, const float *blk, const float *dl, const float *top, int c, float *E,
                                int32_t *Bs, int32_t *Ee, pk_kws_event *events, int cap, int *n_events) {
    return guard([&] {
        need(h && lab && blk && dl && top, "walker/lab/blk/dl/top");
        need_events(events, cap, n_events);
        need(c >= 1, "c must be at least 1");
        if (c > kKwsChunkMaxFrames) fail(PK_ERR_UNSUPPORTED, "streaming TDT keyword spotting: %d frames in one push, at most %d", c, kKwsChunkMaxFrames);
        KwsChunk &w = h->w;
        w.plan(c, nullptr, nullptr);
        PK_HIP(hipMemcpyAsync(w.a.lab.p, lab, (size_t)w.a.labs * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(w.a.blk.p, blk, (size_t)w.a.cells * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(w.a.dl.p, dl, (size_t)w.a.cells * h->D * 4, hipMemcpyHostToDevice, nullptr));
        PK_HIP(hipMemcpyAsync(w.top.p, top, (size_t)w.a.cells * 4, hipMemcpyHostToDevice, nullptr));
        w.walk(E || Bs || Ee, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(nullptr));
        w.collect(events, cap, n_events, E, Bs, Ee);
    });
}

pk_status pk_tdt_kws_chunk_flush(pk_tdt_kws_chunk *h, pk_kws_event *events, int cap, int *n_events) {
    return guard([&] {
        need(h != nullptr, "walker");
        need_events(events, cap, n_events);
        h->w.flush(events, cap, n_events, nullptr);
    });
}

pk_status pk_tdt_kws_chunk_reset(pk_tdt_kws_chunk *h) {
    return guard([&] {
        need(h != nullptr, "walker");
        h->w.clear(nullptr);
        PK_HIP(hipStreamSynchronize(nullptr));
    });
}

void pk_tdt_kws_chunk_free(pk_tdt_kws_chunk *h) { delete h; }

pk_status pk_stream_set_keywords(pk_stream *s, const char *const *phrases, const int32_t *ids_in, const int32_t *kw_offsets_in, int n_kw,
                                 const pk_stream_kws_options *opt) {
    return guard([&] {
        need(s && n_kw >= 0, "stream/n_kw");
        if (n_kw == 0) { s->s->set_keywords(nullptr, nullptr, 0, opt); return; }
        need(phrases || (ids_in && kw_offsets_in), "phrases or ids/kw_offsets");
        std::vector<int32_t> ids, off(1, 0);
        if (phrases) {
            Model &m = s->s->model();
            need(m.tok.loaded(), "spotting phrases needs the model's vocabulary");
            for (int k = 0; k < n_kw; ++k) {
                need(phrases[k] != nullptr, "phrases[k]");
                for (int v : m.tok.encode(phrases[k])) ids.push_back(v);
                off.push_back((int32_t)ids.size());
            }
            ids.push_back(0);                                      // (never read: keeps data() non-null for a list of empty phrases)
            ids_in = ids.data(); kw_offsets_in = off.data();
        }
        s->s->set_keywords(ids_in, kw_offsets_in, n_kw, opt);
    });
}

pk_status pk_stream_spot(pk_stream *s, const float *enc, int n_frames, float *E, int32_t *Bs, int32_t *Ee, pk_kws_event *events, int cap,
                         int *n_events) {
    return guard([&] {
        need(s && enc, "stream/enc");
        need_events(events, cap, n_events);
        s->s->spot(enc, n_frames, E, Bs, Ee, events, cap, n_events);
    });
}

pk_status pk_stream_push_spot(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                              int32_t *end, float *conf, pk_kws_event *events, int cap, int *n_events) {
    return guard([&] {
        if (!s || !pcm || !ids || !lens || n_samples <= 0 || max_tokens <= 0) fail(PK_ERR_INVALID, "invalid argument: stream/pcm/ids/lens/sizes");
        need_events(events, cap, n_events);
        s->s->push_spot(pcm, n_samples, max_tokens, ids, lens, start, end, conf, events, cap, n_events);
    });
}

pk_status pk_stream_spot_flush(pk_stream *s, pk_kws_event *events, int cap, int *n_events) {
    return guard([&] {
        need(s != nullptr, "stream");
        need_events(events, cap, n_events);
        s->s->spot_flush(events, cap, n_events);
    });
}

pk_status pk_stream_spot_timed(pk_stream *s, const float *enc, int n_frames, int reps, float ms[2]) {
    return guard([&] {
        need(s && enc && ms && reps > 0, "stream/enc/ms/reps");
        std::vector<float> t[2];
        for (int r = 0; r <= reps; ++r) {                          // (the first pass warms the buffers up and is not counted)
            float v[2] = {0, 0};
            int n = 0;
            s->s->spot(enc, n_frames, nullptr, nullptr, nullptr, nullptr, 0, &n, v);
            if (r > 0) for (int k = 0; k < 2; ++k) t[k].push_back(v[k]);
        }
        for (int k = 0; k < 2; ++k) {
            std::sort(t[k].begin(), t[k].end());
            ms[k] = t[k][t[k].size() / 2];
        }
    });
}

}  // extern "C"
