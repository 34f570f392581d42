// parakeet.cpp_amd/csrc/rnnt_lattice.cpp -- sizes, groups and launches the forced alignment and the forward-algorithm total of given token strings
// under the plain RNN-T head, and owns their scratch.
#include "rnnt_lattice.hpp"

#include <algorithm>

#include "engine.hpp"
#include "tdt_total.hpp"

namespace pk {

// rows of one chunk of a lattice of `cells` rows (what the scratch formula counts and the plan allocates); chunk_rows > 0 overrides the engine's size
static int rnnt_chunk_rows(int V, int64_t cells, int chunk_rows) {
    return (int)std::min<int64_t>(chunk_rows > 0 ? chunk_rows : tdt_align_chunk_rows(V), std::max<int64_t>(cells, 1));
}

static void rnnt_check_tokens(int64_t U, int b) {
    if (U > kRnntMaxTokens)
        fail(PK_ERR_UNSUPPORTED, "RNN-T lattice: %lld tokens in utterance %d, at most %d can be walked", (long long)U, b, kRnntMaxTokens);
}

size_t rnnt_lattice_scratch(int64_t cells, int64_t labs, int64_t words, int n, int u_max, int V, int J, int chunk_rows) {
    size_t bytes = 4 * ((size_t)labs + (size_t)cells + (size_t)words);
    if (V > 0) bytes += (size_t)rnnt_chunk_rows(V, cells, chunk_rows) * (size_t)(V + J) * 4 + (size_t)(u_max + 1) * (size_t)n * ((size_t)J + 1) * 4;
    return bytes;
}

RnntWalkArgs RnntLatticeWs::args() const {
    RnntWalkArgs r{};
    r.lt = a.lattice();
    r.bits_off = r.lt.lab_off + a.B + 1;
    r.bits = bits.as<unsigned>();
    r.value = a.out.as<float>(); r.ok = a.out.as<int>() + a.B;
    r.start = start.as<int>(); r.end = end.as<int>(); r.conf = conf.as<float>();
    r.u_max = a.u_max;
    return r;
}

// the sums of one utterance: cells, labs and (the alignment) dwords of back-pointer bits
static void rnnt_sums(int64_t T, int64_t U, bool align, int64_t &cells, int64_t &labs, int64_t &words) {
    cells = T * (U + 1); labs = T * U; words = align ? (U + 1) * ((T + 31) / 32) : 0;
}

void rnnt_lattice_plan(RnntLatticeWs &ws, const int32_t *T_of, const int32_t *row0, int n, const int32_t *off, int V, int J, bool align) {
    TdtAlignWs &a = ws.a;
    a.dur_max = 0;
    for (int i = 0; i < 8; ++i) a.durations[i] = 0;
    a.h_tab.assign(3 * (size_t)n + 1, 0);
    a.h_tab64.assign(3 * (size_t)n + 3, 0);
    int32_t *hT = a.h_tab.data(), *hoff = hT + n, *hrow = hoff + n + 1;
    int64_t *hcell = a.h_tab64.data(), *hlab = hcell + n + 1, *hbits = hlab + n + 1;
    int64_t cells = 0, labs = 0, words = 0, rows = 0;
    a.u_max = 0;
    for (int b = 0; b < n; ++b) {
        const int64_t U = off[b + 1] - off[b], Tb = T_of[b];
        rnnt_check_tokens(U, b);
        a.u_max = std::max(a.u_max, (int)U);
        hT[b] = (int32_t)Tb; hoff[b] = off[b]; hrow[b] = row0 ? row0[b] : (int32_t)rows;
        hcell[b] = cells; hlab[b] = labs; hbits[b] = words;
        int64_t c, l, w;
        rnnt_sums(Tb, U, align, c, l, w);
        cells += c; labs += l; words += w; rows += Tb;
        if ((size_t)cells * 4 > kTdtAlignMaxScratch) break;        // (refused below; keeps the sums far from overflow)
    }
    hoff[n] = off[n]; hcell[n] = cells; hlab[n] = labs; hbits[n] = words;
    if (rnnt_lattice_scratch(cells, labs, words, n, a.u_max, V, J, ws.chunk_rows) > kTdtAlignMaxScratch)
        fail(PK_ERR_UNSUPPORTED, "RNN-T lattice: the scratch of this call (lattice values%s%s) exceeds the cap of %zu bytes", align ? ", back-pointer bits" : "",
             V > 0 ? ", rows chunk, prediction net" : "", kTdtAlignMaxScratch);
    a.chunk_rows = V > 0 ? rnnt_chunk_rows(V, cells, ws.chunk_rows) : 0;
    a.B = n; a.D = 0; a.n_ids = (size_t)off[n]; a.cells = cells; a.labs = labs;
    ws.words = words; ws.align = align;
}

void rnnt_lattice_upload(RnntLatticeWs &ws, const int32_t *ids, hipStream_t s) {
    tdt_lattice_upload(ws.a, ids, s, /*token_results=*/false);      // (D = 0: no dl; the TDT byte back-pointers and token arrays stay empty)
    if (!ws.align) return;
    const size_t n = std::max<size_t>(ws.a.n_ids, 1);
    ws.bits.reserve((size_t)std::max<int64_t>(ws.words, 1) * 4);
    for (DevBuf *b : {&ws.start, &ws.end, &ws.conf}) {
        b->reserve(n * 4);
        PK_HIP(hipMemsetAsync(b->p, 0, n * 4, s));
    }
}

void run_rnnt_walk(RnntLatticeWs &ws, hipStream_t s, hipEvent_t *ev) {
    const RnntWalkArgs r = ws.args();
    launch_rnnt_walk(r, ws.align ? RNNT_FOLD_MAX : RNNT_FOLD_SUM, s);
    if (ev) PK_HIP(hipEventRecord(ev[0], s));
    if (ws.align) launch_rnnt_trace(r, s);
    if (ev) PK_HIP(hipEventRecord(ev[1], s));
}

void rnnt_copy_out(const RnntLatticeWs &ws, int32_t *start, int32_t *end, float *conf, float *value, int32_t *ok, hipStream_t s) {
    const size_t n = ws.a.n_ids, B = (size_t)ws.a.B;
    if (ws.align && n) {
        if (start) PK_HIP(hipMemcpyAsync(start, ws.start.p, n * 4, hipMemcpyDeviceToHost, s));
        if (end) PK_HIP(hipMemcpyAsync(end, ws.end.p, n * 4, hipMemcpyDeviceToHost, s));
        if (conf) PK_HIP(hipMemcpyAsync(conf, ws.conf.p, n * 4, hipMemcpyDeviceToHost, s));
    }
    PK_HIP(hipMemcpyAsync(value, ws.a.out.p, B * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipMemcpyAsync(ok, ws.a.out.as<int>() + B, B * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

void rnnt_model_checks(const Model &m) {
    if (m.cfg.vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no prediction net / joint (encoder-only configuration): the RNN-T lattice needs an RNN-T joint");
    if (!m.cfg.rnnt_head)
        fail(PK_ERR_UNSUPPORTED, "the RNN-T lattice needs the plain RNN-T joint (one [V] head): this model has a TDT joint, whose entry points are pk_tdt_align* / pk_tdt_total*");
    if (m.cfg.gemm_bf16) fail(PK_ERR_UNSUPPORTED, "the RNN-T lattice has no gemm_bf16 form: the decode weights of this model exist only rounded to bf16");
}

void rnnt_plan_call(Model &m, RnntLatticeWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *id_offsets, const int32_t *clip_of, int n_hyp,
                    bool align, int chunk_rows) {
    const int V = m.cfg.vocab_size, J = m.cfg.joint_hidden;
    std::vector<int32_t> row0(n_clips);
    int64_t rows = 0;
    for (int c = 0; c < n_clips; ++c) { row0[c] = (int32_t)rows; rows += n_frames ? n_frames[c] : T; }
    ws.T_of.resize(n_hyp); ws.row0_of.resize(n_hyp);
    ws.align = align; ws.chunk_rows = chunk_rows;
    // the limits of every utterance, and the groups: consecutive utterances, at most kTdtTotalGroupHyps, as many as stay under the cap
    ws.gstart.assign(1, 0);
    int64_t cells = 0, labs = 0, words = 0;
    int n = 0, u_max = 0;
    for (int h = 0; h < n_hyp; ++h) {
        const int c = clip_of ? clip_of[h] : h;
        ws.T_of[h] = n_frames ? n_frames[c] : T;
        ws.row0_of[h] = row0[c];
        const int64_t U = id_offsets[h + 1] - id_offsets[h];
        rnnt_check_tokens(U, h);
        int64_t hc, hl, hw;
        rnnt_sums(ws.T_of[h], U, align, hc, hl, hw);
        if (hc > (int64_t)kTdtAlignMaxScratch || rnnt_lattice_scratch(hc, hl, hw, 1, (int)U, V, J, chunk_rows) > kTdtAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "RNN-T lattice: the scratch of utterance %d alone (lattice values%s, rows chunk, prediction net) exceeds the cap of %zu bytes", h,
                 align ? ", back-pointer bits" : "", kTdtAlignMaxScratch);
        if (n > 0 && (n + 1 > kTdtTotalGroupHyps ||
                      rnnt_lattice_scratch(cells + hc, labs + hl, words + hw, n + 1, std::max(u_max, (int)U), V, J, chunk_rows) > kTdtAlignMaxScratch)) {
            ws.gstart.push_back(h);
            cells = labs = words = 0; n = 0; u_max = 0;
        }
        cells += hc; labs += hl; words += hw; ++n; u_max = std::max(u_max, (int)U);
    }
    ws.gstart.push_back(n_hyp);
}

// the heads product of the first n rows of the activation chunk against the RNN-T joint's resident [V][J] weights (Model::wld), on the fp32 GEMM
static void run_rnnt_heads(Model &m, TdtAlignWs &a, int n, hipStream_t s) {
    const int V = m.cfg.vocab_size, J = m.cfg.joint_hidden;
    GemmArgs g{a.z.as<float>(), J, m.wld, J, m.bld, a.logits.as<float>(), V, nullptr, 0, 1.0f, n, V, J};
    m.run_gemm("rnnt_lattice_heads", g, EPI_NONE, s, /*fp32_weight=*/true);
}

void run_rnnt_group_lattice(Model &m, RnntLatticeWs &ws, size_t g, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev) {
    const pk_config &c = m.cfg;
    const int V = c.vocab_size, J = c.joint_hidden;
    hipStream_t s = m.stream;
    const int g0 = ws.gstart[g], n = ws.gstart[g + 1] - g0;
    ws.off.resize(n + 1);
    for (int i = 0; i <= n; ++i) ws.off[i] = id_offsets[g0 + i] - id_offsets[g0];
    const int32_t *gids = ids + id_offsets[g0];
    rnnt_lattice_plan(ws, ws.T_of.data() + g0, ws.row0_of.data() + g0, n, ws.off.data(), V, J, ws.align);
    TdtAlignWs &a = ws.a;
    const size_t st = (size_t)c.num_lstm_layers * n * c.pred_hidden * 4;
    ws.h.reserve(st); ws.hn.reserve(st); ws.c.reserve(st); ws.cn.reserve(st);
    float *state[4] = {ws.h.as<float>(), ws.hn.as<float>(), ws.c.as<float>(), ws.cn.as<float>()};
    if (ev) PK_HIP(hipEventRecord(ev[0], s));
    rnnt_lattice_upload(ws, gids, s);
    run_tdt_align_pred(m, a, gids, s, state);                       // (takes any prediction net: pp[u][b] = pred_proj after [blank, ids[:u]])
    if (ev) PK_HIP(hipEventRecord(ev[1], s));
    const int CH = a.chunk_rows;
    a.z.reserve((size_t)CH * J * 4);
    a.logits.reserve((size_t)CH * V * 4);
    const TdtLattice lt = a.lattice();
    for (int64_t r0 = 0; r0 < a.cells; r0 += CH) {
        const int rows = (int)std::min<int64_t>(CH, a.cells - r0);
        launch_tdt_lattice_act(lt, a.ep_row0(), d_ep, a.pp.as<float>(), J, r0, rows, a.z.as<float>(), s);
        run_rnnt_heads(m, a, rows, s);
        launch_rnnt_lattice_keep(lt, a.ids.as<int>(), a.logits.as<float>(), V, c.blank_id, r0, rows, s);
    }
    if (ev) PK_HIP(hipEventRecord(ev[2], s));
}

void run_rnnt_call(Model &m, RnntLatticeWs &ws, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev, float *ms) {
    const int n_hyp = (int)ws.T_of.size();
    const size_t n_ids = (size_t)id_offsets[n_hyp];
    ws.value.assign(n_hyp, 0.0f); ws.ok.assign(n_hyp, 0);
    ws.h_start.assign(n_ids + 1, 0); ws.h_end.assign(n_ids + 1, 0); ws.h_conf.assign(n_ids + 1, 0.0f);
    hipStream_t s = m.stream;
    for (size_t g = 0; g + 1 < ws.gstart.size(); ++g) {
        const int g0 = ws.gstart[g], i0 = id_offsets[g0];
        run_rnnt_group_lattice(m, ws, g, d_ep, ids, id_offsets, ev);
        run_rnnt_walk(ws, s, ev ? ev + 3 : nullptr);
        rnnt_copy_out(ws, ws.h_start.data() + i0, ws.h_end.data() + i0, ws.h_conf.data() + i0, ws.value.data() + g0, ws.ok.data() + g0, s);
        if (ev && ms)
            for (int k = 0; k < 4; ++k) {
                float v = 0;
                PK_HIP(hipEventElapsedTime(&v, ev[k], ev[k + 1]));
                ms[k] += v;
            }
    }
}

size_t rnnt_lattice_bytes(const RnntLatticeWs &ws) {
    size_t n = tdt_align_bytes(ws.a);
    for (const DevBuf *b : {&ws.bits, &ws.start, &ws.end, &ws.conf, &ws.h, &ws.hn, &ws.c, &ws.cn}) n += b->cap;
    return n;
}

}  // namespace pk
