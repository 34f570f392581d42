// parakeet.cpp_amd/csrc/tdt_tree.cpp -- builds the prefix trees of a call, plans its groups of whole clips, lays out a group's tables and launches the
// prediction net by depth, the tree lattice and the walk (tdt_tree.hpp).
#include "tdt_tree.hpp"

#include <algorithm>
#include <unordered_map>

#include "engine.hpp"
#include "tdt_total.hpp"

namespace pk {

void tdt_prefix_tree_build(TdtPrefixTree &t, const int32_t *ids, const int32_t *id_offsets, const int32_t *clip_of, int n_clips, int n_hyp) {
    std::vector<int32_t> first(n_clips + 1, 0), by_clip(n_hyp);
    for (int h = 0; h < n_hyp; ++h) ++first[(clip_of ? clip_of[h] : h) + 1];
    for (int c = 0; c < n_clips; ++c) first[c + 1] += first[c];
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int h = 0; h < n_hyp; ++h) by_clip[fill[clip_of ? clip_of[h] : h]++] = h;
    t.node_off.assign(1, 0); t.parent.clear(); t.token.clear(); t.end_node.assign(n_hyp, 0);
    std::unordered_map<uint64_t, int32_t> edge;                     // (parent, token) -> child, of the clip being built
    for (int c = 0; c < n_clips; ++c) {
        const int32_t base = t.node_off[c];
        t.parent.push_back(-1); t.token.push_back(-1);
        edge.clear();
        for (int q = first[c]; q < first[c + 1]; ++q) {
            const int h = by_clip[q];
            int32_t k = 0;
            for (int i = id_offsets[h]; i < id_offsets[h + 1]; ++i) {
                const uint64_t key = (uint64_t)(uint32_t)k << 32 | (uint32_t)ids[i];
                const auto it = edge.find(key);
                if (it != edge.end()) { k = it->second; continue; }
                const int32_t nk = (int32_t)t.parent.size() - base;
                t.parent.push_back(k); t.token.push_back(ids[i]);
                edge.emplace(key, nk);
                k = nk;
            }
            t.end_node[h] = k;
        }
        t.node_off.push_back((int32_t)t.parent.size());
    }
}

size_t tdt_tree_scratch(int64_t cells, int64_t labs, int64_t nodes, int D, int V, int J, bool rows_chunk) {
    size_t bytes = 4 * ((size_t)labs + (size_t)cells * (1 + (size_t)D));
    if (V > 0) {
        const int64_t ch = rows_chunk ? std::min<int64_t>(tdt_align_chunk_rows(V + D), std::max<int64_t>(cells, 1)) : 0;
        bytes += (size_t)ch * (size_t)(V + D + J) * 4 + (size_t)nodes * ((size_t)J + 1) * 4;
    }
    return bytes;
}

int tdt_tree_check_durations(const int32_t *durations, int D) {
    if (D < 1 || D > 8) fail(PK_ERR_UNSUPPORTED, "TDT total (shared): %d durations, the kernel is built for 1 to 8", D);
    int dur_max = 0;
    for (int i = 0; i < D; ++i) {
        if (durations[i] < 0 || durations[i] > kTdtAlignMaxDur)
            fail(PK_ERR_UNSUPPORTED, "TDT total (shared): duration %d, the kernel is built for 0 to %d", durations[i], kTdtAlignMaxDur);
        dur_max = std::max(dur_max, (int)durations[i]);
    }
    return dur_max;
}

TdtTree TdtTreeWs::tree() const {
    TdtTree tr{};
    tr.C = C; tr.D = D;
    for (int i = 0; i < 8; ++i) tr.durations[i] = durations[i];
    const int *t = tab.as<int>();
    tr.T = t + o_T; tr.node_off = t + o_node_off; tr.row0 = t + o_row0; tr.parent = t + o_parent; tr.token = t + o_token; tr.ppos = t + o_ppos;
    tr.child_off = t + o_child_off; tr.child = t + o_child; tr.s_node = t + o_s_node; tr.s_parent = t + o_s_parent; tr.s_depth = t + o_s_depth;
    tr.dstart = t + o_dstart;
    tr.cell_off = tab64.as<int64_t>(); tr.lab_off = tr.cell_off + C + 1;
    tr.lab = lab.as<float>(); tr.blk = blk.as<float>(); tr.dl = dl.as<float>();
    return tr;
}

TdtTreeLatticeBf16Args TdtTreeWs::lattice_bf16_args(const float *ep, const float *pp, int V, int J, int blank) const {
    const int *t = tab.as<int>();
    return TdtTreeLatticeBf16Args{tree(), t + o_child_s, t + o_child_tok, ep, pp, nullptr, nullptr, V, J, blank, cells};
}

void tdt_tree_stage(TdtTreeWs &ws, const int32_t *cl, int C, const int32_t *T_of, const int32_t *row0_of, const TdtPrefixTree &pt, const int32_t *hc_off,
                    const int32_t *hc_list, const int32_t *durations, int D, int V, int J, int blank, bool rows_chunk) {
    ws.dur_max = tdt_tree_check_durations(durations, D);
    for (int i = 0; i < 8; ++i) ws.durations[i] = i < D ? durations[i] : 0;
    int64_t nodes = 0, cells = 0, labs = 0, hyps = 0;
    int n_max = 1;
    for (int g = 0; g < C; ++g) {
        const int q = cl[g];
        const int64_t n = pt.node_off[q + 1] - pt.node_off[q];
        if (n > kTdtTreeMaxNodes)
            fail(PK_ERR_UNSUPPORTED, "TDT total (shared): the prefix tree of clip %d has %lld nodes, at most %d can be walked", q, (long long)n, kTdtTreeMaxNodes);
        nodes += n; cells += T_of[q] * n; labs += T_of[q] * (n - 1); hyps += hc_off[q + 1] - hc_off[q];
        n_max = std::max(n_max, (int)n);
        if ((size_t)cells * 4 * (1 + (size_t)D) > kTdtAlignMaxScratch) break;      // (refused below; keeps the sums far from overflow)
    }
    if (tdt_tree_scratch(cells, labs, nodes, D, V, J, rows_chunk) > kTdtAlignMaxScratch)
        fail(PK_ERR_UNSUPPORTED, "TDT total (shared): the scratch of %s (lattice values%s) exceeds the cap of %zu bytes", C == 1 ? "one clip's tree" : "this call",
             V <= 0 ? "" : rows_chunk ? ", rows chunk, prediction net" : ", prediction net", kTdtAlignMaxScratch);
    ws.C = C; ws.D = D; ws.nodes = (int)nodes; ws.n_max = n_max; ws.n_hyp = (int)hyps; ws.cells = cells; ws.labs = labs;
    ws.chunk_rows = V > 0 && rows_chunk ? (int)std::min<int64_t>(tdt_align_chunk_rows(V + D), std::max<int64_t>(cells, 1)) : 0;
    const size_t N = (size_t)nodes, Cz = (size_t)C, H = (size_t)hyps;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += n; return at; };
    ws.o_T = take(Cz); ws.o_node_off = take(Cz + 1); ws.o_row0 = take(Cz); ws.o_parent = take(N); ws.o_token = take(N); ws.o_ppos = take(N);
    ws.o_child_off = take(N + 1); ws.o_child = take(N); ws.o_s_node = take(N); ws.o_s_parent = take(N); ws.o_s_depth = take(N);
    ws.o_dstart = take(N + Cz); ws.o_hyp_off = take(Cz + 1); ws.o_hyp_end = take(H + 1); ws.o_tok_d = take(N); ws.o_pslot = take(N);
    ws.o_child_s = take(N); ws.o_child_tok = take(N);
    ws.h_tab.assign(o, 0);
    ws.h_tab64.assign(2 * Cz + 2, 0);
    int32_t *tb = ws.h_tab.data();
    int64_t *cell_off = ws.h_tab64.data(), *lab_off = cell_off + C + 1;
    std::vector<int32_t> depth(N), cursor;
    ws.slot_hyp.clear();
    int levels = 1;
    int32_t nb_ = 0;
    cells = labs = 0;
    for (int g = 0; g < C; ++g) {
        const int q = cl[g], n = pt.node_off[q + 1] - pt.node_off[q], pb = pt.node_off[q], gb = nb_;
        tb[ws.o_T + g] = T_of[q]; tb[ws.o_node_off + g] = gb; tb[ws.o_row0 + g] = row0_of ? row0_of[q] : 0;
        cell_off[g] = cells; lab_off[g] = labs;
        cells += (int64_t)T_of[q] * n; labs += (int64_t)T_of[q] * (n - 1);
        int32_t *par = tb + ws.o_parent + gb, *coff = tb + ws.o_child_off + gb, *dep = depth.data() + gb;
        int dmax = 0;
        for (int k = 0; k < n; ++k) {
            par[k] = pt.parent[pb + k];
            tb[ws.o_token + gb + k] = pt.token.empty() ? 0 : pt.token[pb + k];
            dep[k] = k == 0 ? 0 : dep[par[k]] + 1;
            dmax = std::max(dmax, (int)dep[k]);
        }
        levels = std::max(levels, dmax + 1);
        // children (CSR over the group's nodes; values clip-local): count, prefix, fill in node order
        for (int k = 0; k <= n; ++k) coff[k] = 0;
        for (int k = 1; k < n; ++k) ++coff[par[k] + 1];
        coff[0] = gb - g;                                           // (nodes - clips so far: every node but a root is one child)
        for (int k = 0; k < n; ++k) coff[k + 1] += coff[k];
        cursor.assign(coff, coff + n);
        for (int k = 1; k < n; ++k) tb[ws.o_child + cursor[par[k]]++] = k;
        // ... and every node's children once more, sorted by the token on their edge (siblings' tokens are distinct), with those tokens beside them
        std::copy(tb + ws.o_child + coff[0], tb + ws.o_child + coff[n], tb + ws.o_child_s + coff[0]);
        const int32_t *tok = tb + ws.o_token + gb;
        for (int k = 0; k < n; ++k)
            std::sort(tb + ws.o_child_s + coff[k], tb + ws.o_child_s + coff[k + 1], [tok](int32_t x, int32_t y) { return tok[x] < tok[y]; });
        for (int j = coff[0]; j < coff[n]; ++j) tb[ws.o_child_tok + j] = tok[tb[ws.o_child_s + j]];
        // the clip's nodes in depth order (stable) and the first entry of every depth
        int32_t *ds = tb + ws.o_dstart + gb + g;
        for (int d = 0; d <= dmax + 1; ++d) ds[d] = 0;
        for (int k = 0; k < n; ++k) ++ds[dep[k] + 1];
        for (int d = 0; d <= dmax; ++d) ds[d + 1] += ds[d];
        cursor.assign(ds, ds + dmax + 1);
        for (int k = 0; k < n; ++k) {
            const int e = cursor[dep[k]]++;
            tb[ws.o_s_node + gb + e] = k; tb[ws.o_s_parent + gb + e] = par[k]; tb[ws.o_s_depth + gb + e] = dep[k];
        }
        tb[ws.o_hyp_off + g] = (int32_t)ws.slot_hyp.size();
        for (int i = hc_off[q]; i < hc_off[q + 1]; ++i) {
            tb[ws.o_hyp_end + ws.slot_hyp.size()] = pt.end_node[hc_list[i]];
            ws.slot_hyp.push_back(hc_list[i]);
        }
        nb_ += n;
    }
    tb[ws.o_node_off + C] = nb_; tb[ws.o_hyp_off + C] = (int32_t)ws.slot_hyp.size();
    cell_off[C] = cells; lab_off[C] = labs;
    // the group's nodes in depth order (depth, then clip, then node): the rows of the prediction net's steps and of its output
    ws.lvl.assign(levels + 1, 0);
    for (size_t i = 0; i < N; ++i) ++ws.lvl[depth[i] + 1];
    ws.width = 0;
    for (int d = 0; d < levels; ++d) { ws.width = std::max(ws.width, (int)ws.lvl[d + 1]); ws.lvl[d + 1] += ws.lvl[d]; }
    cursor.assign(ws.lvl.begin(), ws.lvl.end() - 1);
    for (int g = 0; g < C; ++g) {
        const int gb = tb[ws.o_node_off + g], n = tb[ws.o_node_off + g + 1] - gb;
        for (int k = 0; k < n; ++k) {                               // (parent < node: the parent's row is known)
            const int d = depth[gb + k], row = cursor[d]++;
            tb[ws.o_ppos + gb + k] = row;
            tb[ws.o_tok_d + row] = k == 0 ? blank : tb[ws.o_token + gb + k];
            tb[ws.o_pslot + row] = k == 0 ? -1 : tb[ws.o_ppos + gb + tb[ws.o_parent + gb + k]] - ws.lvl[d - 1];
        }
    }
}

void tdt_tree_upload(TdtTreeWs &ws, hipStream_t s) {
    const size_t cells = (size_t)std::max<int64_t>(ws.cells, 1);
    ws.tab.reserve(ws.h_tab.size() * 4); ws.tab64.reserve(ws.h_tab64.size() * 8);
    ws.lab.reserve(std::max<size_t>((size_t)ws.labs, 1) * 4); ws.blk.reserve(cells * 4); ws.dl.reserve(cells * ws.D * 4);
    ws.out.reserve(std::max<size_t>((size_t)ws.n_hyp, 1) * 2 * 4);
    PK_HIP(hipMemcpyAsync(ws.tab.p, ws.h_tab.data(), ws.h_tab.size() * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.tab64.p, ws.h_tab64.data(), ws.h_tab64.size() * 8, hipMemcpyHostToDevice, s));
}

void run_tdt_tree_pred(Model &m, TdtTreeWs &ws, hipStream_t s) {
    const pk_config &c = m.cfg;
    const int Hp = c.pred_hidden, J = c.joint_hidden, L = c.num_lstm_layers, G = ws.width;
    const size_t st = (size_t)L * G * Hp * 4, lay = (size_t)G * Hp;
    ws.h.reserve(st); ws.hn.reserve(st); ws.c.reserve(st); ws.cn.reserve(st);
    ws.pp.reserve((size_t)ws.nodes * J * 4);
    float *hg = ws.h.as<float>(), *hn = ws.hn.as<float>(), *cg = ws.c.as<float>(), *cn = ws.cn.as<float>();
    const int *tok_d = ws.tab.as<int>() + ws.o_tok_d, *pslot = ws.tab.as<int>() + ws.o_pslot;
    for (size_t u = 0; u + 1 < ws.lvl.size(); ++u) {
        const int r0 = ws.lvl[u], n = ws.lvl[u + 1] - r0;
        // the state every row of this depth starts from: its parent's candidates of the step before (zeros at a root, where nothing is read)
        launch_tdt_tree_gather(pslot + r0, n, L, Hp, (int64_t)lay, hn, cn, hg, cg, s);
        for (int l = 0; l < L; ++l) {
            SkinnyArgs a{};
            const size_t o = (size_t)l * lay;
            a.X = hg + o; a.W = m.dec_whh_s[l]; a.B = n; a.N = 4 * Hp; a.K = Hp; a.out = hn + o; a.c = cg + o; a.cn = cn + o; a.Hp = Hp;
            a.gi_ld = 4 * Hp;
            if (l == 0) { a.gi = m.dec.g1; a.gi_row = tok_d + r0; }
            else { a.X2 = hn + o - lay; a.W2 = m.dec_wih_s[l]; a.bias2 = m.dec.bih[l]; }
            launch_skinny_gemm(a, SK_CELL, s);
        }
        SkinnyArgs a{};
        a.X = hn + (size_t)(L - 1) * lay; a.W = m.dec_wp_s; a.B = n; a.N = J; a.K = Hp; a.bias = m.dec.bp;
        a.out = ws.pp.as<float>() + (size_t)r0 * J; a.ldo = J;
        launch_skinny_gemm(a, SK_BIAS, s);
    }
}

void run_tdt_tree_lattice(Model &m, TdtTreeWs &ws, const float *d_ep, hipStream_t s) {
    const pk_config &c = m.cfg;
    const int V = c.vocab_size, D = ws.D, J = c.joint_hidden, CH = ws.chunk_rows;
    if (m.tdt_lattice_bf16) {          // (a gemm_bf16 model: Model::set_tdt_total_shared admits no other state) one launch, no z, no logits
        TdtTreeLatticeBf16Args a = ws.lattice_bf16_args(d_ep, ws.pp.as<float>(), V, J, c.blank_id);
        a.w16 = m.wld_tl16_.p; a.bld = m.bld;
        launch_tdt_tree_lattice_bf16(a, s);
        return;
    }
    ws.z.reserve((size_t)CH * J * 4);
    ws.logits.reserve((size_t)CH * (V + D) * 4);
    const TdtTree tr = ws.tree();
    for (int64_t r0 = 0; r0 < ws.cells; r0 += CH) {
        const int n = (int)std::min<int64_t>(CH, ws.cells - r0);
        launch_tdt_tree_act(tr, d_ep, ws.pp.as<float>(), J, r0, n, ws.z.as<float>(), s);
        GemmArgs g{ws.z.as<float>(), J, m.wld, J, m.bld, ws.logits.as<float>(), V + D, nullptr, 0, 1.0f, n, V + D, J};      // (run_tdt_align_heads' product)
        m.run_gemm("tdt_align_heads", g, EPI_NONE, s, /*fp32_weight=*/true);
        launch_tdt_tree_keep(tr, ws.logits.as<float>(), V, c.blank_id, r0, n, s);
    }
}

void run_tdt_tree_dp(TdtTreeWs &ws, hipStream_t s) {
    TdtTreeTotalArgs a{};
    a.tr = ws.tree();
    a.hyp_off = ws.tab.as<int>() + ws.o_hyp_off; a.hyp_end = ws.tab.as<int>() + ws.o_hyp_end;
    a.total = ws.out.as<float>(); a.ok = ws.out.as<int>() + ws.n_hyp;
    a.n_max = ws.n_max; a.dur_max = ws.dur_max;
    launch_tdt_tree_total(a, s);
}

void tdt_tree_plan_call(Model &m, TdtTreeWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets,
                        const int32_t *clip_of, int n_hyp) {
    const pk_config &c = m.cfg;
    const int D = c.num_durations, V = c.vocab_size, J = c.joint_hidden;
    const bool rc = !m.tdt_lattice_bf16;                             // (the bf16 lattice kernel has no rows chunk)
    tdt_tree_check_durations(c.durations, D);
    tdt_prefix_tree_build(ws.pt, ids, id_offsets, clip_of, n_clips, n_hyp);
    ws.T_of.resize(n_clips); ws.row0_of.resize(n_clips);
    int64_t rows = 0;
    for (int q = 0; q < n_clips; ++q) { ws.T_of[q] = n_frames ? n_frames[q] : T; ws.row0_of[q] = (int32_t)rows; rows += ws.T_of[q]; }
    ws.hc_off.assign(n_clips + 1, 0); ws.hc_list.resize(n_hyp);
    for (int h = 0; h < n_hyp; ++h) ++ws.hc_off[(clip_of ? clip_of[h] : h) + 1];
    for (int q = 0; q < n_clips; ++q) ws.hc_off[q + 1] += ws.hc_off[q];
    std::vector<int32_t> fill(ws.hc_off.begin(), ws.hc_off.end() - 1);
    for (int h = 0; h < n_hyp; ++h) ws.hc_list[fill[clip_of ? clip_of[h] : h]++] = h;
    ws.walked.clear(); ws.gstart.assign(1, 0);
    int64_t cells = 0, labs = 0, nodes = 0;
    int hyps = 0, in_group = 0;
    for (int q = 0; q < n_clips; ++q) {
        const int nh = ws.hc_off[q + 1] - ws.hc_off[q];
        if (nh == 0) continue;
        const int64_t n = ws.pt.node_off[q + 1] - ws.pt.node_off[q], Tq = ws.T_of[q], qc = Tq * n, ql = Tq * (n - 1);
        if (n > kTdtTreeMaxNodes)
            fail(PK_ERR_UNSUPPORTED, "TDT total (shared): the prefix tree of clip %d has %lld nodes, at most %d can be walked", q, (long long)n, kTdtTreeMaxNodes);
        if (qc > (int64_t)kTdtAlignMaxScratch || tdt_tree_scratch(qc, ql, n, D, V, J, rc) > kTdtAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "TDT total (shared): the scratch of clip %d's tree alone (lattice values%s, prediction net) exceeds the cap of %zu bytes",
                 q, rc ? ", rows chunk" : "", kTdtAlignMaxScratch);
        if (in_group > 0 && (hyps + nh > kTdtTotalGroupHyps || tdt_tree_scratch(cells + qc, labs + ql, nodes + n, D, V, J, rc) > kTdtAlignMaxScratch)) {
            ws.gstart.push_back((int32_t)ws.walked.size());
            cells = labs = nodes = 0; hyps = in_group = 0;
        }
        ws.walked.push_back(q);
        cells += qc; labs += ql; nodes += n; hyps += nh; ++in_group;
    }
    ws.gstart.push_back((int32_t)ws.walked.size());
}

void run_tdt_tree_call(Model &m, TdtTreeWs &ws, const float *d_ep, std::vector<float> &total, std::vector<int32_t> &ok, hipEvent_t *ev, float *ms) {
    const pk_config &c = m.cfg;
    const size_t n_hyp = ws.hc_list.size();
    total.assign(n_hyp, 0.0f); ok.assign(n_hyp, 0);
    std::vector<float> gt;
    std::vector<int32_t> gk;
    hipStream_t s = m.stream;
    for (size_t g = 0; g + 1 < ws.gstart.size(); ++g) {
        const int g0 = ws.gstart[g], C = ws.gstart[g + 1] - g0;
        if (C <= 0) continue;
        tdt_tree_stage(ws, ws.walked.data() + g0, C, ws.T_of.data(), ws.row0_of.data(), ws.pt, ws.hc_off.data(), ws.hc_list.data(), c.durations,
                       c.num_durations, c.vocab_size, c.joint_hidden, c.blank_id, /*rows_chunk=*/!m.tdt_lattice_bf16);
        if (ev) PK_HIP(hipEventRecord(ev[0], s));
        tdt_tree_upload(ws, s);
        run_tdt_tree_pred(m, ws, s);
        if (ev) PK_HIP(hipEventRecord(ev[1], s));
        run_tdt_tree_lattice(m, ws, d_ep, s);
        if (ev) PK_HIP(hipEventRecord(ev[2], s));
        run_tdt_tree_dp(ws, s);
        if (ev) PK_HIP(hipEventRecord(ev[3], s));
        const size_t n = (size_t)ws.n_hyp;
        gt.resize(n); gk.resize(n);
        PK_HIP(hipMemcpyAsync(gt.data(), ws.out.p, n * 4, hipMemcpyDeviceToHost, s));
        PK_HIP(hipMemcpyAsync(gk.data(), ws.out.as<int>() + n, n * 4, hipMemcpyDeviceToHost, s));
        PK_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) { total[ws.slot_hyp[i]] = gt[i]; ok[ws.slot_hyp[i]] = gk[i]; }
        if (ev && ms)
            for (int k = 0; k < 3; ++k) {
                float v = 0;
                PK_HIP(hipEventElapsedTime(&v, ev[k], ev[k + 1]));
                ms[k] += v;
            }
    }
}

size_t tdt_tree_bytes(const TdtTreeWs &ws) {
    size_t n = 0;
    for (const DevBuf *b : {&ws.lab, &ws.blk, &ws.dl, &ws.tab, &ws.tab64, &ws.out, &ws.pp, &ws.z, &ws.logits, &ws.h, &ws.hn, &ws.c, &ws.cn}) n += b->cap;
    return n;
}

}  // namespace pk
