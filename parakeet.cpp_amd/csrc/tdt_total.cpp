// parakeet.cpp_amd/csrc/tdt_total.cpp -- sizes, groups and launches the forward-algorithm total of given token strings under the TDT head, and
// holds the ordering rule of the rescored n-best list.
#include "tdt_total.hpp"

#include <algorithm>
#include <numeric>

#include "engine.hpp"

namespace pk {

size_t tdt_total_scratch(int64_t cells, int64_t labs, int n, int u_max, int D, int V, int J) {
    size_t bytes = 4 * ((size_t)labs + (size_t)cells * (1 + (size_t)D));
    if (V > 0) {
        const int64_t ch = std::min<int64_t>(tdt_align_chunk_rows(V + D), std::max<int64_t>(cells, 1));
        bytes += (size_t)ch * (size_t)(V + D + J) * 4 + (size_t)(u_max + 1) * (size_t)n * ((size_t)J + 1) * 4;
    }
    return bytes;
}

void tdt_total_groups(std::vector<int32_t> &gstart, const int32_t *T_of, const int32_t *id_offsets, int n_hyp, const int32_t *durations, int D, int V,
                      int J, int max_hyps) {
    if (D < 1 || D > 8) fail(PK_ERR_UNSUPPORTED, "TDT total: %d durations, the kernel is built for 1 to 8", D);
    for (int i = 0; i < D; ++i)
        if (durations[i] < 0 || durations[i] > kTdtAlignMaxDur)
            fail(PK_ERR_UNSUPPORTED, "TDT total: duration %d, the kernel is built for 0 to %d", durations[i], kTdtAlignMaxDur);
    if (max_hyps <= 0) max_hyps = kTdtTotalGroupHyps;
    gstart.assign(1, 0);
    int64_t cells = 0, labs = 0;
    int n = 0, u_max = 0;
    for (int h = 0; h < n_hyp; ++h) {
        const int64_t U = id_offsets[h + 1] - id_offsets[h], T = T_of[h];
        if (U > kTdtAlignMaxTokens)
            fail(PK_ERR_UNSUPPORTED, "TDT total: %lld tokens in hypothesis %d, at most %d can be scored", (long long)U, h, kTdtAlignMaxTokens);
        const int64_t hc = T * (U + 1), hl = T * U;
        if (hc > (int64_t)kTdtAlignMaxScratch || tdt_total_scratch(hc, hl, 1, (int)U, D, V, J) > kTdtAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "TDT total: the scratch of hypothesis %d alone (lattice values%s) exceeds the cap of %zu bytes", h,
                 V > 0 ? ", rows chunk, prediction net" : "", kTdtAlignMaxScratch);
        if (n > 0 && (n + 1 > max_hyps || tdt_total_scratch(cells + hc, labs + hl, n + 1, std::max(u_max, (int)U), D, V, J) > kTdtAlignMaxScratch)) {
            gstart.push_back(h);
            cells = labs = 0; n = 0; u_max = 0;
        }
        cells += hc; labs += hl; ++n; u_max = std::max(u_max, (int)U);
    }
    if (n_hyp > 0) gstart.push_back(n_hyp);
}

void run_tdt_total_dp(TdtAlignWs &ws, hipStream_t s) {
    TdtTotalArgs a{};
    a.lt = ws.lattice();
    a.total = ws.out.as<float>(); a.ok = ws.out.as<int>() + ws.B;
    a.u_max = ws.u_max; a.dur_max = ws.dur_max;
    launch_tdt_total(a, s);
}

void tdt_total_plan_call(Model &m, TdtTotalWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *id_offsets,
                         const int32_t *clip_of, int n_hyp) {
    std::vector<int32_t> row0(n_clips);
    int64_t rows = 0;
    for (int c = 0; c < n_clips; ++c) { row0[c] = (int32_t)rows; rows += n_frames ? n_frames[c] : T; }
    ws.T_of.resize(n_hyp); ws.row0_of.resize(n_hyp);
    for (int h = 0; h < n_hyp; ++h) {
        const int c = clip_of ? clip_of[h] : h;
        ws.T_of[h] = n_frames ? n_frames[c] : T;
        ws.row0_of[h] = row0[c];
    }
    tdt_total_groups(ws.gstart, ws.T_of.data(), id_offsets, n_hyp, m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden);
}

void run_tdt_total_call(Model &m, TdtTotalWs &ws, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev, float *ms) {
    const pk_config &c = m.cfg;
    const int n_hyp = (int)ws.T_of.size();
    ws.total.assign(n_hyp, 0.0f); ws.ok.assign(n_hyp, 0);
    hipStream_t s = m.stream;
    for (size_t g = 0; g + 1 < ws.gstart.size(); ++g) {
        const int g0 = ws.gstart[g], n = ws.gstart[g + 1] - g0;
        ws.off.resize(n + 1);
        for (int i = 0; i <= n; ++i) ws.off[i] = id_offsets[g0 + i] - id_offsets[g0];
        const int32_t *gids = ids + id_offsets[g0];
        tdt_lattice_plan(ws.a, ws.T_of.data() + g0, ws.row0_of.data() + g0, n, 0, ws.off.data(), c.durations, c.num_durations, c.vocab_size, c.joint_hidden,
                         0, /*back_pointers=*/false, "TDT total");
        const size_t st = (size_t)c.num_lstm_layers * n * c.pred_hidden * 4;
        ws.h.reserve(st); ws.hn.reserve(st); ws.c.reserve(st); ws.cn.reserve(st);
        float *state[4] = {ws.h.as<float>(), ws.hn.as<float>(), ws.c.as<float>(), ws.cn.as<float>()};
        if (ev) PK_HIP(hipEventRecord(ev[0], s));
        tdt_lattice_upload(ws.a, gids, s, /*token_results=*/false);
        run_tdt_align_pred(m, ws.a, gids, s, state);
        if (ev) PK_HIP(hipEventRecord(ev[1], s));
        run_tdt_align_lattice(m, ws.a, d_ep, s);
        if (ev) PK_HIP(hipEventRecord(ev[2], s));
        run_tdt_total_dp(ws.a, s);
        if (ev) PK_HIP(hipEventRecord(ev[3], s));
        PK_HIP(hipMemcpyAsync(ws.total.data() + g0, ws.a.out.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        PK_HIP(hipMemcpyAsync(ws.ok.data() + g0, ws.a.out.as<int>() + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        PK_HIP(hipStreamSynchronize(s));
        if (ev && ms)
            for (int k = 0; k < 3; ++k) {
                float v = 0;
                PK_HIP(hipEventElapsedTime(&v, ev[k], ev[k + 1]));
                ms[k] += v;
            }
    }
}

size_t tdt_total_bytes(const TdtTotalWs &ws) {
    size_t n = tdt_align_bytes(ws.a);
    for (const DevBuf *b : {&ws.h, &ws.hn, &ws.c, &ws.cn}) n += b->cap;
    return n;
}

void rescore_order(const int32_t *lens, const float *ctc, const float *tdt, const int32_t *ok, int N, float w, int32_t *order, float *combined) {
    const float NEG = -__builtin_huge_valf();
    std::vector<int> cls(N);
    const float w1 = 1.0f - w;
    for (int j = 0; j < N; ++j) {
        const bool unfilled = lens[j] == 0 && !(ctc[j] > NEG);
        cls[j] = unfilled ? 2 : ok[j] ? 0 : 1;                     // scored, filled but not scored, unfilled
        const float a = w1 * ctc[j], b = w * tdt[j];
        combined[j] = cls[j] == 0 ? a + b : NEG;                   // (a slot that is not scored: the formula would give 0 * -inf)
        if (combined[j] != combined[j]) { cls[j] = 1; combined[j] = NEG; }      // (NaN, from an infinite part: not scored; keeps the order strict weak)
        order[j] = j;
    }
    std::stable_sort(order, order + N, [&](int32_t x, int32_t y) {
        if (cls[x] != cls[y]) return cls[x] < cls[y];
        return cls[x] == 0 && combined[x] > combined[y];
    });
}

}  // namespace pk
