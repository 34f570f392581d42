// parakeet.cpp_amd/csrc/ctc_kws.cpp -- checks, sizes and launches the CTC keyword spotting and owns its scratch.
#include "ctc_kws.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace pk {

pk_kws_options kws_options_of(const pk_kws_options *opt) {
    pk_kws_options o;
    o.max_hits = 1;
    o.min_score = -std::numeric_limits<float>::infinity();
    if (opt) o = *opt;
    return o;
}

void kws_check_args(const int32_t *ids, const int32_t *kw_offsets, int n_kw, int B, int V, int blank, const pk_kws_options &opt, const char *what) {
    if (B < 1) fail(PK_ERR_INVALID, "invalid argument: B = %d", B);
    if (n_kw < 1) fail(PK_ERR_INVALID, "invalid argument: n_kw = %d", n_kw);
    if (!kw_offsets || !ids) fail(PK_ERR_INVALID, "invalid argument: kw_ids/kw_offsets");
    if (V < 2 || blank < 0 || blank >= V) fail(PK_ERR_INVALID, "invalid argument: blank id %d outside the vocabulary of %d", blank, V);
    if (std::isnan(opt.min_score) || opt.min_score > 0.0f)
        fail(PK_ERR_INVALID, "invalid argument: min_score %g: a score is a log-ratio <= 0, so min_score must be <= 0", (double)opt.min_score);
    if (kw_offsets[0] != 0) fail(PK_ERR_INVALID, "invalid argument: kw_offsets[0] must be 0");
    for (int k = 0; k < n_kw; ++k) {
        if (kw_offsets[k + 1] < kw_offsets[k]) fail(PK_ERR_INVALID, "invalid argument: kw_offsets decrease at keyword %d", k);
        if (kw_offsets[k + 1] == kw_offsets[k]) fail(PK_ERR_INVALID, "invalid argument: keyword %d is empty", k);
    }
    const int n = kw_offsets[n_kw];
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= V) fail(PK_ERR_INVALID, "invalid argument: token id %d at %d outside [0, %d)", ids[i], i, V);
        if (ids[i] == blank) fail(PK_ERR_INVALID, "invalid argument: token id at %d is the blank (%d)", i, blank);
    }
    if (opt.max_hits < 1 || opt.max_hits > kKwsMaxHits)
        fail(PK_ERR_UNSUPPORTED, "%s: max_hits = %d, supported 1 .. %d", what, opt.max_hits, kKwsMaxHits);
    for (int k = 0; k < n_kw; ++k)
        if (kw_offsets[k + 1] - kw_offsets[k] > kKwsMaxLen)
            fail(PK_ERR_UNSUPPORTED, "%s: %d tokens in keyword %d, at most %d can be spotted", what, kw_offsets[k + 1] - kw_offsets[k], k, kKwsMaxLen);
    if (B > 65535) fail(PK_ERR_UNSUPPORTED, "%s: %d utterances in one call, at most 65535", what, B);
}

void kws_plan(KwsWs &ws, const int32_t *n_frames, int B, int T, const int32_t *kw_offsets, int n_kw, const pk_kws_options &opt) {
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) rows += n_frames ? n_frames[b] : T;
    // 8 * n_kw * rows against the cap, without overflow: rows < 2^31 * 65535, n_kw < 2^31
    if (rows > 0 && (uint64_t)n_kw > (uint64_t)(kKwsMaxScratch / 8) / (uint64_t)rows)
        fail(PK_ERR_UNSUPPORTED, "CTC keyword spotting: the scratch (8 * n_kw * sum of T = 8 * %d * %lld bytes) exceeds the cap of %zu bytes", n_kw,
             (long long)rows, kKwsMaxScratch);
    ws.h_tab.assign(kw_offsets, kw_offsets + n_kw + 1);
    ws.B = B; ws.n_kw = n_kw; ws.max_hits = opt.max_hits; ws.min_score = opt.min_score;
    ws.n_ids = (size_t)kw_offsets[n_kw]; ws.rows = rows;
}

void run_ctc_kws(KwsWs &ws, const float *d_lp, int B, int T, const SeqRag &rag, int V, int blank, const int32_t *ids, hipStream_t s) {
    const size_t pairs = (size_t)B * ws.n_kw, slots = pairs * ws.max_hits;
    ws.ids.reserve(ws.n_ids * 4);
    ws.tab.reserve(ws.h_tab.size() * 4);
    ws.g.reserve((size_t)ws.rows * 4);
    ws.eb.reserve((size_t)ws.rows * ws.n_kw * 8);
    ws.out.reserve((pairs + 3 * slots) * 4);
    PK_HIP(hipMemcpyAsync(ws.ids.p, ids, ws.n_ids * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.tab.p, ws.h_tab.data(), ws.h_tab.size() * 4, hipMemcpyHostToDevice, s));
    launch_ctc_rowmax(d_lp, ws.g.as<float>(), ws.rows, V, s);
    CtcKwsArgs a{};
    a.lp = d_lp; a.V = V; a.blank = blank; a.B = B; a.T = T; a.n_kw = ws.n_kw;
    a.ids = ws.ids.as<int>(); a.kw_off = ws.tab.as<int>();
    a.g = ws.g.as<float>(); a.eb = ws.eb.as<int2>();
    a.max_hits = ws.max_hits; a.min_score = ws.min_score;
    a.n_hits = ws.out.as<int>();
    a.start = a.n_hits + pairs; a.end = a.start + slots; a.score = ws.out.as<float>() + pairs + 2 * slots;
    a.rg = rag;
    launch_ctc_kws(a, s);
}

void kws_copy_out(const KwsWs &ws, int32_t *n_hits, int32_t *start, int32_t *end, float *score, hipStream_t s) {
    const size_t pairs = (size_t)ws.B * ws.n_kw, slots = pairs * ws.max_hits;
    const int *o = ws.out.as<int>();
    if (n_hits) PK_HIP(hipMemcpyAsync(n_hits, o, pairs * 4, hipMemcpyDeviceToHost, s));
    if (start) PK_HIP(hipMemcpyAsync(start, o + pairs, slots * 4, hipMemcpyDeviceToHost, s));
    if (end) PK_HIP(hipMemcpyAsync(end, o + pairs + slots, slots * 4, hipMemcpyDeviceToHost, s));
    if (score) PK_HIP(hipMemcpyAsync(score, o + pairs + 2 * slots, slots * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

size_t kws_bytes(const KwsWs &ws) { return ws.ids.cap + ws.tab.cap + ws.g.cap + ws.eb.cap + ws.out.cap; }

}  // namespace pk
