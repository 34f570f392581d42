// parakeet.cpp_amd/csrc/stream_kws.cpp -- sizes and launches the streaming TDT keyword spotting and owns its carried state.
#include "stream_kws.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>

#include "engine.hpp"
#include "tdt_kws.hpp"

namespace pk {

static const char *const kWhat = "streaming TDT keyword spotting";

pk_stream_kws_options stream_kws_options_of(const pk_stream_kws_options *opt) {
    pk_stream_kws_options o;
    o.min_score = -std::numeric_limits<float>::infinity();
    o.patience = 0;
    return opt ? *opt : o;
}

void stream_kws_check_options(const pk_stream_kws_options &o) {
    if (std::isnan(o.min_score) || o.min_score > 0.0f)
        fail(PK_ERR_INVALID, "invalid argument: min_score %g: a score is a log-ratio <= 0, so min_score must be <= 0", (double)o.min_score);
    if (o.patience < 0) fail(PK_ERR_INVALID, "invalid argument: patience %d: frames to wait after a hit's end, >= 0", o.patience);
}

KwsChunk::~KwsChunk() {
    if (pin_) (void)hipHostFree(pin_);
}

void KwsChunk::setup(const int32_t *durations, int D, std::vector<int32_t> id_off, int n_kw_, int V, int J, const pk_stream_kws_options &o,
                     size_t extra_bytes) {
    const int n = (int)id_off.size() - 1;
    if (n > kStreamKwsMaxPairs) fail(PK_ERR_UNSUPPORTED, "%s: %d (stream, keyword) pairs, at most %d can be walked", kWhat, n, kStreamKwsMaxPairs);
    for (int p = 0; p < n; ++p)
        if (id_off[p + 1] - id_off[p] > kKwsMaxLen)
            fail(PK_ERR_UNSUPPORTED, "%s: %d tokens in the keyword of pair %d, at most %d can be spotted", kWhat, id_off[p + 1] - id_off[p], p, kKwsMaxLen);
    // the lattice at the push limit (refuses D and the durations too), then the carried state on top of it: host arithmetic alone
    std::vector<int32_t> T(n, kKwsChunkMaxFrames), row0(n, 0);
    tdt_lattice_plan(a, T.data(), V > 0 ? row0.data() : nullptr, n, 0, id_off.data(), durations, D, V, J, 0, /*back_pointers=*/false, kWhat);
    const size_t ring_words = (size_t)(a.dur_max + 2) * (2 * D + 1) * (size_t)id_off[n];
    const size_t total = tdt_kws_scratch(a.cells, a.labs, n, a.u_max, D, V, J) + ring_words * 4 + (size_t)n * 20 +
                         (size_t)n * (4 + 32 * (size_t)kKwsChunkMaxFrames) + extra_bytes;
    if (total > kTdtAlignMaxScratch)
        fail(PK_ERR_UNSUPPORTED, "%s: the carried state and the lattice of a %d-frame push (%zu bytes) exceed the cap of %zu bytes", kWhat,
             kKwsChunkMaxFrames, total, kTdtAlignMaxScratch);
    n_pairs = n; n_kw = n_kw_; D_ = D; V_ = V; J_ = J; dur_max_ = a.dur_max; opt_ = o;
    for (int i = 0; i < 8; ++i) durations_[i] = i < D ? durations[i] : 0;
    id_off_ = std::move(id_off);
    ring_words_ = ring_words;
    nev_words_ = ((size_t)n + 3) / 4 * 4;
    c = 0; t0 = 0;
}

void KwsChunk::alloc(hipStream_t s) {
    ring_.reserve(std::max<size_t>(ring_words_, 1) * 4);
    pend_.reserve((size_t)n_pairs * 20);                            // the pending hits [pairs] (16 bytes each), then the ends of the last hits that left [pairs]
    clear(s);
}

void KwsChunk::clear(hipStream_t s) {
    PK_HIP(hipMemsetD32Async((hipDeviceptr_t)ring_.p, (int)0xFF800000u, std::max<size_t>(ring_words_, 1), s));      // every candidate -inf: nothing before frame 0
    PK_HIP(hipMemsetAsync(pend_.p, 0, (size_t)n_pairs * 16, s));
    PK_HIP(hipMemsetD32Async((hipDeviceptr_t)(pend_.as<int>() + (size_t)n_pairs * 4), -1, n_pairs, s));
    t0 = 0;
}

void KwsChunk::plan(int c_, const int32_t *ids, hipStream_t s) {
    if (c_ == c) return;
    T_.assign(n_pairs, c_);
    row0_.resize(n_pairs);
    for (int p = 0; p < n_pairs; ++p) row0_[p] = (p / n_kw) * c_;
    tdt_lattice_plan(a, T_.data(), V_ > 0 ? row0_.data() : nullptr, n_pairs, 0, id_off_.data(), durations_, D_, V_, J_, 0, /*back_pointers=*/false, kWhat);
    tdt_lattice_upload(a, ids, s, /*token_results=*/false);
    top.reserve((size_t)a.cells * 4);
    out_.reserve((nev_words_ + (size_t)n_pairs * c_ * 4) * 4);
    c = c_;
}

void KwsChunk::walk(bool rows, hipStream_t s) {
    const size_t ev_bytes = (nev_words_ + (size_t)n_pairs * c * 4) * 4, row_bytes = (size_t)n_pairs * c * 16;
    if (ev_bytes + row_bytes > pin_bytes_) {                         // (no copy of an earlier push is in flight: every entry point ends synchronised)
        if (pin_) { PK_HIP(hipHostFree(pin_)); pin_ = nullptr; pin_bytes_ = 0; }
        PK_HIP(hipHostMalloc(&pin_, ev_bytes + row_bytes, hipHostMallocDefault));
        pin_bytes_ = ev_bytes + row_bytes;
    }
    if (rows) rows_.reserve(row_bytes);
    TdtKwsChunkArgs k{};
    k.lt = a.lattice();
    launch_tdt_kws_norm(k.lt, top.as<float>(), a.cells, s);
    k.ring = ring_.as<float>(); k.pend = pend_.as<int4>(); k.last_end = pend_.as<int>() + (size_t)n_pairs * 4;
    k.n_ev = out_.as<int>(); k.ev = reinterpret_cast<int4 *>(out_.as<int>() + nev_words_);
    k.rows = rows ? rows_.as<int4>() : nullptr;
    k.t0 = t0; k.c = c; k.dur_max = dur_max_; k.patience = opt_.patience; k.min_score = opt_.min_score;
    launch_tdt_kws_chunk(k, s);
    PK_HIP(hipMemcpyAsync(pin_, out_.p, ev_bytes, hipMemcpyDeviceToHost, s));
    if (rows) PK_HIP(hipMemcpyAsync(static_cast<char *>(pin_) + ev_bytes, rows_.p, row_bytes, hipMemcpyDeviceToHost, s));
    rows_copied_ = rows;
    t0 += c;
}

static void put_event(pk_kws_event *events, int cap, int &n, int pair, int n_kw, const int32_t *v) {
    if (n < cap) {
        pk_kws_event &e = events[n];
        e.stream = pair / n_kw; e.keyword = pair % n_kw; e.start = v[1]; e.end = v[2];
        memcpy(&e.score, &v[0], 4);
    }
    ++n;
}

void KwsChunk::collect(pk_kws_event *events, int cap, int *n_events, float *E, int32_t *Bs, int32_t *Ee) {
    const int32_t *nev = static_cast<const int32_t *>(pin_), *ev = nev + nev_words_;
    int n = 0;
    for (int p = 0; p < n_pairs; ++p)
        for (int k = 0; k < nev[p]; ++k) put_event(events, cap, n, p, n_kw, ev + ((size_t)p * c + k) * 4);
    if (n_events) *n_events = n;
    if (rows_copied_ && (E || Bs || Ee)) {
        const int32_t *r = ev + (size_t)n_pairs * c * 4;
        for (size_t i = 0; i < (size_t)n_pairs * c; ++i) {
            if (E) memcpy(&E[i], &r[4 * i], 4);
            if (Bs) Bs[i] = r[4 * i + 1];
            if (Ee) Ee[i] = r[4 * i + 2];
        }
    }
}

void KwsChunk::flush(pk_kws_event *events, int cap, int *n_events, hipStream_t s) {
    std::vector<int32_t> pend((size_t)n_pairs * 5);
    int32_t *last = pend.data() + (size_t)n_pairs * 4;
    PK_HIP(hipMemcpyAsync(pend.data(), pend_.p, pend.size() * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
    int n = 0;
    for (int p = 0; p < n_pairs; ++p)
        if (pend[(size_t)p * 4 + 3]) {
            put_event(events, cap, n, p, n_kw, pend.data() + (size_t)p * 4);
            last[p] = pend[(size_t)p * 4 + 2];                       // the hit has left: what starts inside it no longer qualifies
        }
    PK_HIP(hipMemsetAsync(pend_.p, 0, (size_t)n_pairs * 16, s));
    PK_HIP(hipMemcpyAsync(pend_.as<int>() + (size_t)n_pairs * 4, last, (size_t)n_pairs * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipStreamSynchronize(s));
    if (n_events) *n_events = n;
}

size_t KwsChunk::bytes() const {
    size_t n = tdt_align_bytes(a);
    for (const DevBuf *b : {&top, &ring_, &pend_, &out_, &rows_}) n += b->cap;
    return n;
}

StreamKws::StreamKws(Model &m, int S, const int32_t *ids, const int32_t *kw_offsets, int n_kw, const pk_stream_kws_options &o) : m_(m), S_(S) {
    const pk_config &c = m.cfg;
    if (n_kw > kStreamKwsMaxKeywords) fail(PK_ERR_UNSUPPORTED, "%s: %d keywords, at most %d can be set", kWhat, n_kw, kStreamKwsMaxKeywords);
    if ((int64_t)S * n_kw > kStreamKwsMaxPairs)
        fail(PK_ERR_UNSUPPORTED, "%s: %d streams x %d keywords, at most %d pairs can be walked", kWhat, S, n_kw, kStreamKwsMaxPairs);
    const int J = c.joint_hidden;
    std::vector<int32_t> off(1, 0);
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < n_kw; ++k) {
            pid_.insert(pid_.end(), ids + kw_offsets[k], ids + kw_offsets[k + 1]);
            off.push_back((int32_t)pid_.size());
        }
    pid_.push_back(0);                                              // (never read: keeps data() non-null)
    // the distinct keywords, in the order of their first occurrence: the prediction net runs on those, once
    std::map<std::vector<int32_t>, int> seen;
    std::vector<int32_t> kids, koff(1, 0), net_of(n_kw);
    int u_max = 0;
    for (int k = 0; k < n_kw; ++k) {
        std::vector<int32_t> key(ids + kw_offsets[k], ids + kw_offsets[k + 1]);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int)koff.size() - 1).first;
            kids.insert(kids.end(), key.begin(), key.end());
            koff.push_back((int32_t)kids.size());
            u_max = std::max(u_max, (int)key.size());
        }
        net_of[k] = it->second;
    }
    n_net_ = (int)koff.size() - 1;
    const size_t net_bytes = (size_t)(u_max + 1) * n_net_ * ((size_t)J + 1) * 4 + (size_t)S * kKwsChunkMaxFrames * J * 4;
    w.setup(c.durations, c.num_durations, std::move(off), n_kw, c.vocab_size, J, o, net_bytes);
    // nothing was allocated so far
    hipStream_t s = m.stream;
    tdt_lattice_plan(net_, nullptr, nullptr, n_net_, 1, koff.data(), c.durations, c.num_durations, 0, 0, 0, /*back_pointers=*/false, kWhat);
    {
        const size_t st = (size_t)c.num_lstm_layers * n_net_ * c.pred_hidden * 4;
        DevBuf h, hn, cc, cn;                                       // the net's lock-step LSTM state: needed while it runs alone
        h.reserve(st); hn.reserve(st); cc.reserve(st); cn.reserve(st);
        float *state[4] = {h.as<float>(), hn.as<float>(), cc.as<float>(), cn.as<float>()};
        run_tdt_align_pred(m, net_, kids.data(), s, state);
        PK_HIP(hipStreamSynchronize(s));
    }
    std::vector<int32_t> pair_net((size_t)S * n_kw);
    for (size_t p = 0; p < pair_net.size(); ++p) pair_net[p] = net_of[p % n_kw];
    net_of_.reserve(pair_net.size() * 4);
    PK_HIP(hipMemcpyAsync(net_of_.p, pair_net.data(), pair_net.size() * 4, hipMemcpyHostToDevice, s));
    w.alloc(s);
    PK_HIP(hipStreamSynchronize(s));
    PK_CHECK_LAUNCH();
}

void StreamKws::enqueue(const float *d_enc, int c, bool rows, hipEvent_t *ev) {
    const int J = m_.cfg.joint_hidden;
    hipStream_t s = m_.stream;
    if (ev) PK_HIP(hipEventRecord(ev[0], s));
    ep_.reserve((size_t)S_ * c * J * 4);
    m_.run_enc_proj(d_enc, (int64_t)S_ * c, ep_.as<float>(), s);
    w.plan(c, pid_.data(), s);
    tdt_kws_build_lattice(m_, w.a, w.top.as<float>(), ep_.as<float>(), net_, net_of_.as<int>(), n_net_, s);
    if (ev) PK_HIP(hipEventRecord(ev[1], s));
    w.walk(rows, s);
    if (ev) PK_HIP(hipEventRecord(ev[2], s));
}

}  // namespace pk
