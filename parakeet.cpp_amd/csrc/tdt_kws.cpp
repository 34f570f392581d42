// parakeet.cpp_amd/csrc/tdt_kws.cpp -- sizes, groups and launches the TDT keyword spotting and owns its scratch.
#include "tdt_kws.hpp"

#include <algorithm>

#include "engine.hpp"
#include "tdt_total.hpp"

namespace pk {

static const char *const kWhat = "TDT keyword spotting";

size_t tdt_kws_scratch(int64_t cells, int64_t labs, int n, int u_max, int D, int V, int J) {
    return tdt_total_scratch(cells, labs, n, u_max, D, V, J) + 4 * (size_t)cells + 16 * (size_t)(cells - labs);
}

void tdt_kws_plan_call(TdtKwsWs &ws, const int32_t *durations, int D, int V, int J, const int32_t *n_frames, int n_clips, int T, const int32_t *kw_ids,
                       const int32_t *kw_offsets, int n_kw, const int32_t *clip_of, const int32_t *kw_of, int n_pairs, const pk_kws_options &opt) {
    if (D < 1 || D > 8) fail(PK_ERR_UNSUPPORTED, "%s: %d durations, the kernel is built for 1 to 8", kWhat, D);
    for (int i = 0; i < D; ++i)
        if (durations[i] < 0 || durations[i] > kTdtAlignMaxDur)
            fail(PK_ERR_UNSUPPORTED, "%s: duration %d, the kernel is built for 0 to %d", kWhat, durations[i], kTdtAlignMaxDur);
    std::vector<int32_t> row0(n_clips);
    int64_t rows = 0;
    for (int c = 0; c < n_clips; ++c) { row0[c] = (int32_t)rows; rows += n_frames ? n_frames[c] : T; }
    ws.T_of.resize(n_pairs); ws.row0_of.resize(n_pairs); ws.kw_of.resize(n_pairs);
    ws.poff.assign(1, 0); ws.pid.clear();
    const int max_pairs = n_kw > kTdtKwsGroupKeywords ? kTdtKwsGroupKeywords : kTdtKwsGroupPairs;
    ws.gstart.assign(1, 0);
    int64_t cells = 0, labs = 0;
    int n = 0, u_max = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int c = clip_of ? clip_of[p] : p / n_kw, k = kw_of ? kw_of[p] : p % n_kw;
        const int64_t L = kw_offsets[k + 1] - kw_offsets[k], Tp = n_frames ? n_frames[c] : T;
        ws.T_of[p] = (int32_t)Tp; ws.row0_of[p] = row0[c]; ws.kw_of[p] = k;
        ws.pid.insert(ws.pid.end(), kw_ids + kw_offsets[k], kw_ids + kw_offsets[k + 1]);
        ws.poff.push_back((int32_t)ws.pid.size());
        const int64_t pc = Tp * (L + 1), pl = Tp * L;
        if (pc > (int64_t)kTdtAlignMaxScratch || tdt_kws_scratch(pc, pl, 1, (int)L, D, V, J) > kTdtAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "%s: the scratch of keyword %d on clip %d alone (lattice values, exit rows%s) exceeds the cap of %zu bytes", kWhat, k, c,
                 V > 0 ? ", rows chunk, prediction net" : "", kTdtAlignMaxScratch);
        if (n > 0 && (n + 1 > max_pairs || tdt_kws_scratch(cells + pc, labs + pl, n + 1, std::max(u_max, (int)L), D, V, J) > kTdtAlignMaxScratch)) {
            ws.gstart.push_back(p);
            cells = labs = 0; n = 0; u_max = 0;
        }
        cells += pc; labs += pl; ++n; u_max = std::max(u_max, (int)L);
    }
    ws.gstart.push_back(n_pairs);
    ws.pid.push_back(0);                                           // (never read: keeps data() non-null)
    ws.max_hits = opt.max_hits; ws.min_score = opt.min_score;
}

void run_tdt_kws_dp(TdtKwsWs &ws, hipStream_t s) {
    const size_t n = (size_t)ws.a.B, slots = n * ws.max_hits;
    ws.eb.reserve((size_t)std::max<int64_t>(ws.a.cells - ws.a.labs, 1) * 16);
    ws.out.reserve((n + 3 * slots) * 4);
    TdtKwsArgs a{};
    a.lt = ws.a.lattice();
    launch_tdt_kws_norm(a.lt, ws.top.as<float>(), ws.a.cells, s);
    a.eb = ws.eb.as<int4>();
    a.max_hits = ws.max_hits; a.min_score = ws.min_score;
    a.n_hits = ws.out.as<int>();
    a.start = a.n_hits + n; a.end = a.start + slots; a.score = ws.out.as<float>() + n + 2 * slots;
    a.dur_max = ws.a.dur_max;
    launch_tdt_kws(a, s);
}

void tdt_kws_gather(TdtKwsWs &ws, int g0, hipStream_t s) {
    const size_t n = (size_t)ws.a.B, H = (size_t)ws.max_hits, slots = n * H;
    const int *o = ws.out.as<int>();
    PK_HIP(hipMemcpyAsync(ws.n_hits.data() + g0, o, n * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipMemcpyAsync(ws.start.data() + g0 * H, o + n, slots * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipMemcpyAsync(ws.end.data() + g0 * H, o + n + slots, slots * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipMemcpyAsync(ws.score.data() + g0 * H, o + n + 2 * slots, slots * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

void tdt_kws_build_lattice(Model &m, TdtAlignWs &a, float *top, const float *ep, const TdtAlignWs &net, const int *net_of, int n_net, hipStream_t s) {
    const pk_config &c = m.cfg;
    const int V = c.vocab_size, J = c.joint_hidden, CH = a.chunk_rows;
    a.z.reserve((size_t)CH * J * 4);
    a.logits.reserve((size_t)CH * (V + a.D) * 4);
    const TdtLattice lt = a.lattice();
    for (int64_t r0 = 0; r0 < a.cells; r0 += CH) {
        const int nr = (int)std::min<int64_t>(CH, a.cells - r0);
        launch_tdt_kws_act(lt, a.ep_row0(), ep, net.pp.as<float>(), net_of, n_net, J, r0, nr, a.z.as<float>(), s);
        run_tdt_align_heads(m, a, nr, s);
        launch_tdt_kws_keep(lt, top, a.ids.as<int>(), a.logits.as<float>(), V, c.blank_id, r0, nr, s);
    }
}

void run_tdt_kws_call(Model &m, TdtKwsWs &ws, const float *d_ep, const int32_t *kw_ids, const int32_t *kw_offsets, int chunk_rows, bool walk,
                      hipEvent_t *ev, float *ms) {
    const pk_config &c = m.cfg;
    const int n_pairs = (int)ws.T_of.size(), V = c.vocab_size, J = c.joint_hidden;
    const size_t H = (size_t)ws.max_hits;
    ws.n_hits.assign(n_pairs, 0); ws.start.assign(n_pairs * H, 0); ws.end.assign(n_pairs * H, 0); ws.score.assign(n_pairs * H, 0.0f);
    hipStream_t s = m.stream;
    int n_kw = 0;
    for (int k : ws.kw_of) n_kw = std::max(n_kw, k + 1);
    for (size_t g = 0; g + 1 < ws.gstart.size(); ++g) {
        const int g0 = ws.gstart[g], n = ws.gstart[g + 1] - g0;
        ws.off.resize(n + 1);
        for (int i = 0; i <= n; ++i) ws.off[i] = ws.poff[g0 + i] - ws.poff[g0];
        const int32_t *gids = ws.pid.data() + ws.poff[g0];
        tdt_lattice_plan(ws.a, ws.T_of.data() + g0, ws.row0_of.data() + g0, n, 0, ws.off.data(), c.durations, c.num_durations, V, J, chunk_rows,
                         /*back_pointers=*/false, kWhat);
        // the distinct keywords of the group, in the order of their first pair: the prediction net runs on those
        ws.slot.assign(n_kw, -1); ws.h_net_of.resize(n); ws.kids.clear(); ws.koff.assign(1, 0);
        for (int i = 0; i < n; ++i) {
            const int k = ws.kw_of[g0 + i];
            if (ws.slot[k] < 0) {
                ws.slot[k] = (int)ws.koff.size() - 1;
                ws.kids.insert(ws.kids.end(), kw_ids + kw_offsets[k], kw_ids + kw_offsets[k + 1]);
                ws.koff.push_back((int32_t)ws.kids.size());
            }
            ws.h_net_of[i] = ws.slot[k];
        }
        const int nk = (int)ws.koff.size() - 1;
        tdt_lattice_plan(ws.net, nullptr, nullptr, nk, 1, ws.koff.data(), c.durations, c.num_durations, 0, 0, 0, /*back_pointers=*/false, kWhat);
        const size_t st = (size_t)c.num_lstm_layers * nk * c.pred_hidden * 4;
        ws.h.reserve(st); ws.hn.reserve(st); ws.c.reserve(st); ws.cn.reserve(st);
        float *state[4] = {ws.h.as<float>(), ws.hn.as<float>(), ws.c.as<float>(), ws.cn.as<float>()};
        ws.net_of.reserve((size_t)n * 4);
        ws.top.reserve((size_t)std::max<int64_t>(ws.a.cells, 1) * 4);
        if (ev) PK_HIP(hipEventRecord(ev[0], s));
        tdt_lattice_upload(ws.a, gids, s, /*token_results=*/false);
        PK_HIP(hipMemcpyAsync(ws.net_of.p, ws.h_net_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        run_tdt_align_pred(m, ws.net, ws.kids.data(), s, state);
        if (ev) PK_HIP(hipEventRecord(ev[1], s));
        tdt_kws_build_lattice(m, ws.a, ws.top.as<float>(), d_ep, ws.net, ws.net_of.as<int>(), nk, s);
        if (ev) PK_HIP(hipEventRecord(ev[2], s));
        if (walk) run_tdt_kws_dp(ws, s);
        if (ev) PK_HIP(hipEventRecord(ev[3], s));
        if (walk) tdt_kws_gather(ws, g0, s);
        else PK_HIP(hipStreamSynchronize(s));
        if (ev && ms)
            for (int k = 0; k < 3; ++k) {
                float v = 0;
                PK_HIP(hipEventElapsedTime(&v, ev[k], ev[k + 1]));
                ms[k] += v;
            }
    }
}

size_t tdt_kws_bytes(const TdtKwsWs &ws) {
    size_t n = tdt_align_bytes(ws.a) + tdt_align_bytes(ws.net);
    for (const DevBuf *b : {&ws.top, &ws.eb, &ws.out, &ws.net_of, &ws.h, &ws.hn, &ws.c, &ws.cn}) n += b->cap;
    return n;
}

}  // namespace pk
