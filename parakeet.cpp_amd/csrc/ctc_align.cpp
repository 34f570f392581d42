// parakeet.cpp_amd/csrc/ctc_align.cpp -- sizes and launches the CTC forced alignment of given token strings and owns its scratch.
#include "ctc_align.hpp"

#include <algorithm>

namespace pk {

void align_check_args(const int32_t *ids, const int32_t *id_offsets, int B, int V, int blank) {
    if (B < 1) fail(PK_ERR_INVALID, "invalid argument: B = %d", B);
    if (!id_offsets) fail(PK_ERR_INVALID, "invalid argument: id_offsets");
    if (V < 2 || blank < 0 || blank >= V) fail(PK_ERR_INVALID, "invalid argument: blank id %d outside the vocabulary of %d", blank, V);
    if (id_offsets[0] != 0) fail(PK_ERR_INVALID, "invalid argument: id_offsets[0] must be 0");
    for (int b = 0; b < B; ++b)
        if (id_offsets[b + 1] < id_offsets[b]) fail(PK_ERR_INVALID, "invalid argument: id_offsets decrease at utterance %d", b);
    const int n = id_offsets[B];
    if (n > 0 && !ids) fail(PK_ERR_INVALID, "invalid argument: ids");
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= V) fail(PK_ERR_INVALID, "invalid argument: token id %d at %d outside [0, %d)", ids[i], i, V);
        if (ids[i] == blank) fail(PK_ERR_INVALID, "invalid argument: token id at %d is the blank (%d)", i, blank);
    }
}

void align_plan(AlignWs &ws, const int32_t *n_frames, int B, int T, const int32_t *id_offsets) {
    ws.h_tab.assign(id_offsets, id_offsets + B + 1);
    ws.h_off.resize(B);
    int s_max = 1;
    size_t dwords = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = id_offsets[b + 1] - id_offsets[b], S = 2 * L + 1;
        if (S > kAlignMaxStates)
            fail(PK_ERR_UNSUPPORTED, "CTC alignment: %lld tokens in utterance %d, at most %d can be aligned", (long long)L, b, (kAlignMaxStates - 1) / 2);
        s_max = std::max(s_max, (int)S);
        ws.h_off[b] = (int64_t)dwords;
        dwords += (size_t)(n_frames ? n_frames[b] : T) * (size_t)((S + kAlignBpCells - 1) / kAlignBpCells);
        if (dwords * 4 > kAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "CTC alignment: the back-pointers (sum of T * ceil((2 L + 1) / 16) * 4 bytes) exceed the cap of %zu bytes",
                 kAlignMaxScratch);
    }
    ws.shape = 0;
    while (s_max > kAlignThreads[ws.shape] * kAlignStrip[ws.shape]) ++ws.shape;
    ws.B = B; ws.n_ids = (size_t)id_offsets[B]; ws.bp_dwords = dwords;
}

void run_ctc_align(AlignWs &ws, const float *d_lp, int B, int T, const SeqRag &rag, int V, int blank, const int32_t *ids, bool want_total,
                   hipStream_t s) {
    const size_t n = std::max<size_t>(ws.n_ids, 1);
    ws.ids.reserve(n * 4); ws.start.reserve(n * 4); ws.end.reserve(n * 4); ws.conf.reserve(n * 4);
    ws.tab.reserve(ws.h_tab.size() * 4); ws.off.reserve(ws.h_off.size() * 8);
    ws.bp.reserve(std::max<size_t>(ws.bp_dwords, 1) * 4);
    ws.out.reserve((size_t)B * 3 * 4);
    if (ws.n_ids) PK_HIP(hipMemcpyAsync(ws.ids.p, ids, ws.n_ids * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.tab.p, ws.h_tab.data(), ws.h_tab.size() * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.off.p, ws.h_off.data(), ws.h_off.size() * 8, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemsetAsync(ws.start.p, 0, n * 4, s));
    PK_HIP(hipMemsetAsync(ws.end.p, 0, n * 4, s));
    PK_HIP(hipMemsetAsync(ws.conf.p, 0, n * 4, s));
    CtcAlignArgs a{};
    a.lp = d_lp; a.V = V; a.blank = blank; a.B = B; a.T = T;
    a.ids = ws.ids.as<int>(); a.id_off = ws.tab.as<int>();
    a.bp = ws.bp.as<unsigned>(); a.bp_off = ws.off.as<int64_t>();
    a.start = ws.start.as<int>(); a.end = ws.end.as<int>(); a.conf = ws.conf.as<float>();
    a.score = ws.out.as<float>(); a.total = want_total ? a.score + B : nullptr; a.ok = ws.out.as<int>() + 2 * (size_t)B;
    a.rg = rag;
    launch_ctc_align(a, ws.shape, s);
}

void align_copy_out(const AlignWs &ws, int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok, hipStream_t s) {
    const size_t n = ws.n_ids, B = (size_t)ws.B;
    if (start && n) PK_HIP(hipMemcpyAsync(start, ws.start.p, n * 4, hipMemcpyDeviceToHost, s));
    if (end && n) PK_HIP(hipMemcpyAsync(end, ws.end.p, n * 4, hipMemcpyDeviceToHost, s));
    if (conf && n) PK_HIP(hipMemcpyAsync(conf, ws.conf.p, n * 4, hipMemcpyDeviceToHost, s));
    if (score) PK_HIP(hipMemcpyAsync(score, ws.out.p, B * 4, hipMemcpyDeviceToHost, s));
    if (total) PK_HIP(hipMemcpyAsync(total, ws.out.as<float>() + B, B * 4, hipMemcpyDeviceToHost, s));
    if (ok) PK_HIP(hipMemcpyAsync(ok, ws.out.as<int>() + 2 * B, B * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

}  // namespace pk
