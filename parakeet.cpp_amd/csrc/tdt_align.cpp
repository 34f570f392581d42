// parakeet.cpp_amd/csrc/tdt_align.cpp -- sizes and launches the TDT forced alignment of given token strings and owns its scratch.
#include "tdt_align.hpp"

#include <algorithm>

#include "engine.hpp"

namespace pk {

TdtLattice TdtAlignWs::lattice() const {
    TdtLattice lt{};
    lt.B = B; lt.D = D;
    for (int i = 0; i < 8; ++i) lt.durations[i] = durations[i];
    lt.T = tab.as<int>(); lt.id_off = lt.T + B;
    lt.cell_off = tab64.as<int64_t>(); lt.lab_off = lt.cell_off + B + 1;
    lt.lab = lab.as<float>(); lt.blk = blk.as<float>(); lt.dl = dl.as<float>();
    return lt;
}

void tdt_align_plan(TdtAlignWs &ws, const int32_t *n_frames, int B, int T, const int32_t *id_offsets, const int32_t *durations, int D, int V, int J,
                    int chunk_rows) {
    tdt_lattice_plan(ws, n_frames, nullptr, B, T, id_offsets, durations, D, V, J, chunk_rows, /*back_pointers=*/true, "TDT alignment");
}

void tdt_lattice_plan(TdtAlignWs &ws, const int32_t *n_frames, const int32_t *row0, int B, int T, const int32_t *id_offsets, const int32_t *durations,
                      int D, int V, int J, int chunk_rows, bool back_pointers, const char *what) {
    const size_t bpb = back_pointers ? 1 : 0;
    if (D < 1 || D > 8) fail(PK_ERR_UNSUPPORTED, "%s: %d durations, the kernel is built for 1 to 8", what, D);
    ws.dur_max = 0;
    for (int i = 0; i < 8; ++i) ws.durations[i] = 0;
    for (int i = 0; i < D; ++i) {
        if (durations[i] < 0 || durations[i] > kTdtAlignMaxDur)
            fail(PK_ERR_UNSUPPORTED, "%s: duration %d, the kernel is built for 0 to %d", what, durations[i], kTdtAlignMaxDur);
        ws.durations[i] = durations[i];
        ws.dur_max = std::max(ws.dur_max, (int)durations[i]);
    }
    ws.h_tab.assign(3 * (size_t)B + 1, 0);
    ws.h_tab64.assign(2 * (size_t)B + 2, 0);
    int32_t *hT = ws.h_tab.data(), *hoff = hT + B, *hrow = hoff + B + 1;
    int64_t *hcell = ws.h_tab64.data(), *hlab = hcell + B + 1;
    int64_t cells = 0, labs = 0, rows = 0;
    ws.u_max = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t U = id_offsets[b + 1] - id_offsets[b], Tb = n_frames ? n_frames[b] : T;
        if (U > kTdtAlignMaxTokens)
            fail(PK_ERR_UNSUPPORTED, "%s: %lld tokens in utterance %d, at most %d can be aligned", what, (long long)U, b, kTdtAlignMaxTokens);
        ws.u_max = std::max(ws.u_max, (int)U);
        hT[b] = (int32_t)Tb; hoff[b] = id_offsets[b]; hrow[b] = row0 ? row0[b] : (int32_t)rows;
        hcell[b] = cells; hlab[b] = labs;
        cells += Tb * (U + 1); labs += Tb * U; rows += Tb;
        if ((size_t)cells * (4 + bpb + 4 * (size_t)D) > kTdtAlignMaxScratch) break;        // (refused below; keeps the sums far from overflow)
    }
    hoff[B] = id_offsets[B]; hcell[B] = cells; hlab[B] = labs;
    ws.chunk_rows = 0;
    size_t bytes = 4 * ((size_t)labs + (size_t)cells * (1 + D)) + (size_t)cells * bpb;
    if (V > 0) {
        ws.chunk_rows = chunk_rows > 0 ? chunk_rows : tdt_align_chunk_rows(V + D);
        if ((int64_t)ws.chunk_rows > cells) ws.chunk_rows = (int)std::max<int64_t>(cells, 1);
        bytes += (size_t)ws.chunk_rows * (size_t)(V + D + J) * 4 + (size_t)(ws.u_max + 1) * B * ((size_t)J + 1) * 4;
    }
    if (bytes > kTdtAlignMaxScratch)
        fail(PK_ERR_UNSUPPORTED, "%s: the scratch of this call (lattice values%s%s) exceeds the cap of %zu bytes", what,
             back_pointers ? ", back-pointers" : "", V > 0 ? ", rows chunk, prediction net" : "", kTdtAlignMaxScratch);
    ws.B = B; ws.D = D; ws.n_ids = (size_t)id_offsets[B]; ws.cells = cells; ws.labs = labs;
}

void tdt_lattice_upload(TdtAlignWs &ws, const int32_t *ids, hipStream_t s, bool token_results) {
    const size_t n = std::max<size_t>(ws.n_ids, 1), cells = (size_t)std::max<int64_t>(ws.cells, 1);
    ws.ids.reserve(n * 4);
    ws.tab.reserve(ws.h_tab.size() * 4); ws.tab64.reserve(ws.h_tab64.size() * 8);
    ws.lab.reserve(std::max<size_t>((size_t)ws.labs, 1) * 4); ws.blk.reserve(cells * 4); ws.dl.reserve(cells * ws.D * 4);
    ws.out.reserve((size_t)ws.B * 2 * 4);
    if (ws.n_ids && ids) PK_HIP(hipMemcpyAsync(ws.ids.p, ids, ws.n_ids * 4, hipMemcpyHostToDevice, s));      // (the walk alone reads no ids)
    PK_HIP(hipMemcpyAsync(ws.tab.p, ws.h_tab.data(), ws.h_tab.size() * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.tab64.p, ws.h_tab64.data(), ws.h_tab64.size() * 8, hipMemcpyHostToDevice, s));
    if (!token_results) return;
    ws.bp.reserve(cells);
    for (DevBuf *b : {&ws.start, &ws.end, &ws.didx, &ws.conf}) {
        b->reserve(n * 4);
        PK_HIP(hipMemsetAsync(b->p, 0, n * 4, s));
    }
}

void run_tdt_align_pred(Model &m, TdtAlignWs &ws, const int32_t *ids, hipStream_t s, float *const *state) {
    const pk_config &c = m.cfg;
    const int B = ws.B, Hp = c.pred_hidden, J = c.joint_hidden, L = c.num_lstm_layers, steps = ws.u_max + 1;
    Workspace &w = m.ws;
    ws.pp.reserve((size_t)steps * B * J * 4);
    ws.tok.reserve((size_t)steps * B * 4);
    // token of step u: the blank at u = 0, ids[u - 1] after it; an utterance past its last prefix keeps stepping on the blank (its rows are
    // independent chains nobody reads)
    ws.h_tok.assign((size_t)steps * B, c.blank_id);
    const int32_t *off = ws.h_tab.data() + B;
    for (int b = 0; b < B; ++b)
        for (int u = 1; u <= off[b + 1] - off[b]; ++u) ws.h_tok[(size_t)u * B + b] = ids[off[b] + u - 1];
    PK_HIP(hipMemcpyAsync(ws.tok.p, ws.h_tok.data(), ws.h_tok.size() * 4, hipMemcpyHostToDevice, s));
    const size_t st = (size_t)L * B * Hp;
    float *hb[2] = {state ? state[0] : w.h.as<float>(), state ? state[1] : w.hn.as<float>()};
    float *cb[2] = {state ? state[2] : w.c.as<float>(), state ? state[3] : w.cn.as<float>()};
    PK_HIP(hipMemsetAsync(hb[0], 0, st * 4, s));
    PK_HIP(hipMemsetAsync(cb[0], 0, st * 4, s));
    for (int u = 0; u < steps; ++u) {
        const float *hs = hb[u & 1], *cs = cb[u & 1];
        float *hd = hb[(u + 1) & 1], *cd = cb[(u + 1) & 1];          // every step commits: the candidates of step u are the state of step u + 1
        for (int l = 0; l < L; ++l) {
            SkinnyArgs a{};
            const size_t o = (size_t)l * B * Hp;
            a.X = hs + o; a.W = m.dec_whh_s[l]; a.B = B; a.N = 4 * Hp; a.K = Hp; a.out = hd + o; a.c = cs + o; a.cn = cd + o; a.Hp = Hp;
            a.gi_ld = 4 * Hp;
            if (l == 0) { a.gi = m.dec.g1; a.gi_row = ws.tok.as<int>() + (size_t)u * B; }
            else { a.X2 = hd + o - (size_t)B * Hp; a.W2 = m.dec_wih_s[l]; a.bias2 = m.dec.bih[l]; }
            launch_skinny_gemm(a, SK_CELL, s);
        }
        SkinnyArgs a{};
        a.X = hd + (size_t)(L - 1) * B * Hp; a.W = m.dec_wp_s; a.B = B; a.N = J; a.K = Hp; a.bias = m.dec.bp;
        a.out = ws.pp.as<float>() + (size_t)u * B * J; a.ldo = J;
        launch_skinny_gemm(a, SK_BIAS, s);
    }
}

void tdt_align_model_checks(const Model &m) {
    if (m.cfg.vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no prediction net / joint (encoder-only configuration): TDT alignment needs a TDT joint");
    if (m.cfg.rnnt_head || m.cfg.num_durations <= 0)
        fail(PK_ERR_UNSUPPORTED, "TDT alignment needs a TDT joint (label + duration heads): this model has an RNN-T head");
    if (m.cfg.gemm_bf16) fail(PK_ERR_UNSUPPORTED, "TDT alignment has no gemm_bf16 form: the decode weights of this model exist only rounded to bf16");
}

size_t tdt_align_bytes(const TdtAlignWs &ws) {
    size_t n = 0;
    for (const DevBuf *b : {&ws.lab, &ws.blk, &ws.dl, &ws.bp, &ws.tab, &ws.tab64, &ws.ids, &ws.start, &ws.end, &ws.didx, &ws.conf, &ws.out, &ws.pp, &ws.tok, &ws.z, &ws.logits})
        n += b->cap;
    return n;
}

// (the natural [V + D][J] copy of the heads weights is resident since the upload: Model::wld)
void run_tdt_align_heads(Model &m, TdtAlignWs &ws, int n, hipStream_t s) {
    const int VD = m.cfg.vocab_size + ws.D, J = m.cfg.joint_hidden;
    GemmArgs g{ws.z.as<float>(), J, m.wld, J, m.bld, ws.logits.as<float>(), VD, nullptr, 0, 1.0f, n, VD, J};
    m.run_gemm("tdt_align_heads", g, EPI_NONE, s, /*fp32_weight=*/true);
}

void run_tdt_align_lattice(Model &m, TdtAlignWs &ws, const float *d_ep, hipStream_t s) {
    const pk_config &c = m.cfg;
    const int V = c.vocab_size, D = ws.D, J = c.joint_hidden, CH = ws.chunk_rows;
    ws.z.reserve((size_t)CH * J * 4);
    ws.logits.reserve((size_t)CH * (V + D) * 4);
    const TdtLattice lt = ws.lattice();
    for (int64_t r0 = 0; r0 < ws.cells; r0 += CH) {
        const int n = (int)std::min<int64_t>(CH, ws.cells - r0);
        launch_tdt_lattice_act(lt, ws.ep_row0(), d_ep, ws.pp.as<float>(), J, r0, n, ws.z.as<float>(), s);
        run_tdt_align_heads(m, ws, n, s);
        launch_tdt_lattice_keep(lt, ws.ids.as<int>(), ws.logits.as<float>(), V, c.blank_id, r0, n, s);
    }
}

void run_tdt_align_dp(TdtAlignWs &ws, hipStream_t s) {
    TdtAlignArgs a{};
    a.lt = ws.lattice();
    a.bp = ws.bp.as<unsigned char>();
    a.start = ws.start.as<int>(); a.end = ws.end.as<int>(); a.dur_idx = ws.didx.as<int>(); a.conf = ws.conf.as<float>();
    a.score = ws.out.as<float>(); a.ok = ws.out.as<int>() + ws.B;
    a.u_max = ws.u_max; a.dur_max = ws.dur_max;
    launch_tdt_align(a, s);
}

void tdt_align_copy_out(const TdtAlignWs &ws, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok, hipStream_t s) {
    const size_t n = ws.n_ids, B = (size_t)ws.B;
    if (start && n) PK_HIP(hipMemcpyAsync(start, ws.start.p, n * 4, hipMemcpyDeviceToHost, s));
    if (end && n) PK_HIP(hipMemcpyAsync(end, ws.end.p, n * 4, hipMemcpyDeviceToHost, s));
    if (dur_idx && n) PK_HIP(hipMemcpyAsync(dur_idx, ws.didx.p, n * 4, hipMemcpyDeviceToHost, s));
    if (conf && n) PK_HIP(hipMemcpyAsync(conf, ws.conf.p, n * 4, hipMemcpyDeviceToHost, s));
    if (score) PK_HIP(hipMemcpyAsync(score, ws.out.p, B * 4, hipMemcpyDeviceToHost, s));
    if (ok) PK_HIP(hipMemcpyAsync(ok, ws.out.as<int>() + B, B * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

}  // namespace pk
