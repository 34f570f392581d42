// parakeet.cpp_amd/csrc/capi_diag.cpp -- the pk_diag_* entry points of the C boundary: single kernels and launcher decisions, run alone on
// operands the caller hands over, for the kernel-level tests: math, LayerNorm, attention, mel, conv, decode and memory (the products are in
// capi_diag_gemm.cpp).  Nothing here is kept between calls: every call stages its operands afresh, through the helpers of capi_diag_util.hpp.
#include "capi_diag_util.hpp"

using namespace pk;
using namespace pk::diag;

extern "C" {

pk_status pk_diag_math(int fn, const float *in, float *out, int64_t n) {
    return guard([&] {
        need(in && out && n > 0, "in/out/n");
        need_device();
        DevBuf x, y;
        up(x, in, n * 4);
        y.reserve(n * 4);
        launch_math(fn, x.as<float>(), y.as<float>(), n, nullptr);
        PK_CHECK_LAUNCH();
        down(out, y, n * 4);
    });
}

pk_status pk_diag_math_exhaustive(int fn, uint64_t *checked, uint64_t *mismatches, uint64_t *first_bad) {
    return guard([&] {
        need(fn == 3 || fn == 4 || fn == 13 || fn == 14, "fn must be 3, 4, 13 or 14");
        need(checked && mismatches && first_bad, "checked/mismatches/first_bad");
        need_device();
        DevBuf acc;
        const uint64_t init[3] = {0, 0, 1ull << 32};
        up(acc, init, sizeof init);
        launch_math_exhaustive(fn, acc.as<unsigned long long>(), nullptr);
        PK_CHECK_LAUNCH();
        uint64_t res[3];
        down(res, acc, sizeof res);
        *checked = res[0]; *mismatches = res[1]; *first_bad = res[2];
    });
}

pk_status pk_diag_pred_cache(int on) { g_diag_pred_cache.store(on ? 1 : 0); return PK_OK; }

pk_status pk_diag_skinny_gemm(const pk_skinny_diag *d) {
    return guard([&] {
        need(d, "args");
        const int B = d->B, N = d->N, K = d->K, epi = d->epi;
        const bool b16 = d->bf16 != 0, cell = epi == SK_CELL, act = epi == SK_ACT;
        need(epi == SK_BIAS || act || cell, "epi");
        need(d->X && d->W && d->out && B > 0 && N > 0 && K > 0, "X/W/out/B/N/K");
        const int F = act && d->F > 1 ? d->F : 1;
        const int wrows = cell ? 4 * N : N;
        if (b16) {
            need(K % 32 == 0, "bf16: K must be a multiple of 32");
            need(!cell || N % 4 == 0, "bf16 cell: Hp must be a multiple of 4");
            need(F == 1, "the frame window is an fp32 form");
        } else {
            need(K % 16 == 0, "fp32: K must be a multiple of 16");
            need(epi == SK_BIAS || N % 16 == 0, "fp32 activation / cell: N must be a multiple of 16 (sigma layout of the output)");
            need(F <= kDecWindowMax, "F");
            need(F == 1 || (d->need && B <= 16), "the frame window comes with need flags and B <= 16");
        }
        need(!d->need || B <= kMaxListRows, "need flags: B <= 2048");
        need(d->out_rows >= B * F, "out_rows >= B * F");
        const int ld = epi == SK_BIAS ? d->ldo : N;
        need(ld >= N, "ldo >= N");
        if (cell) {
            need(d->c && d->cn, "cell: c/cn");
            if (d->W2) need(d->X2 && d->bias2, "cell: X2/bias2 with W2");
            else {
                need(d->gi && d->gi_ld >= 4 * N && d->gi_rows > 0, "cell: gi/gi_ld/gi_rows");
                for (int b = 0; b < B; ++b) {
                    const int r = d->gi_row ? d->gi_row[b] : b;
                    need(r >= 0 && r < d->gi_rows, "cell: gi_row out of range");
                }
            }
        }
        if (act) {
            need(d->ep && d->t && d->ep_rows > 0, "activation: ep/t/ep_rows");
            for (int b = 0; b < B; ++b) {
                const int Tb = d->Tb ? d->Tb[b] : d->T;
                const int64_t r0 = d->row0 ? (int64_t)d->row0[b] : (int64_t)b * d->T;
                need(Tb >= 1 && r0 >= 0 && r0 + Tb <= d->ep_rows && d->t[b] >= 0, "activation: frames out of range");
            }
        }
        need_device();
        const size_t out_el = epi != SK_BIAS && b16 ? 2 : 4;
        DevBuf dX, dW, dX2, dW2, dbias, dbias2, dgi, dgr, dc, dep, dt, dTb, dr0, dneed, dout, dcn, dpp;
        auto up_x = [&](DevBuf &buf, const float *x) {
            if (b16) up16(buf, x, (size_t)B * K);
            else { const std::vector<float> p = pack_sigma(x, B, K); up(buf, p.data(), p.size() * 4); }
        };
        auto up_w = [&](DevBuf &buf, const float *w) {
            if (b16) { const std::vector<float> p = pack_dec16(w, wrows, K, cell); up16(buf, p.data(), p.size()); }
            else { const std::vector<float> p = pack_sigma(w, wrows, K); up(buf, p.data(), p.size() * 4); }
        };
        SkinnyArgs a{};
        up_x(dX, d->X); up_w(dW, d->W);
        a.X = dX.as<float>(); a.W = dW.as<float>(); a.B = B; a.N = wrows; a.K = K;
        if (d->bias && !cell) { up(dbias, d->bias, (size_t)N * 4); a.bias = dbias.as<float>(); }
        up(dout, d->out, (size_t)d->out_rows * ld * out_el);
        a.out = dout.as<float>(); a.ldo = ld;
        a.F = F;
        if (cell) {
            a.Hp = N;
            up(dc, d->c, (size_t)B * N * 4); a.c = dc.as<float>();
            up(dcn, d->cn, (size_t)d->out_rows * N * 4); a.cn = dcn.as<float>();
            if (d->W2) {
                up_x(dX2, d->X2); up_w(dW2, d->W2); up(dbias2, d->bias2, (size_t)4 * N * 4);
                a.X2 = dX2.as<float>(); a.W2 = dW2.as<float>(); a.bias2 = dbias2.as<float>();
                a.gi_ld = 4 * N;
            } else {
                up(dgi, d->gi, (size_t)d->gi_rows * d->gi_ld * 4); a.gi = dgi.as<float>(); a.gi_ld = d->gi_ld;
                if (d->gi_row) { up(dgr, d->gi_row, (size_t)B * 4); a.gi_row = dgr.as<int>(); }
            }
        }
        if (act) {
            up(dep, d->ep, (size_t)d->ep_rows * N * 4); a.ep = dep.as<float>();
            up(dt, d->t, (size_t)B * 4); a.t = dt.as<int>(); a.T = d->T;
            if (d->Tb) { up(dTb, d->Tb, (size_t)B * 4); a.Tb = dTb.as<int>(); }
            if (d->row0) { up(dr0, d->row0, (size_t)B * 4); a.row0 = dr0.as<int>(); }
            if (d->pp_out) { up(dpp, d->pp_out, (size_t)d->out_rows * N * 4); a.pp_out = dpp.as<float>(); }
        }
        if (d->need) { up(dneed, d->need, (size_t)B * 4); a.need = dneed.as<int>(); }
        if (b16) launch_skinny_gemm_bf16(a, epi, nullptr);
        else launch_skinny_gemm(a, epi, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->out, dout, (size_t)d->out_rows * ld * out_el);
        if (cell) down(d->cn, dcn, (size_t)d->out_rows * N * 4);
        if (act && d->pp_out) down(d->pp_out, dpp, (size_t)d->out_rows * N * 4);
    });
}

pk_status pk_diag_tdt_decide(const pk_tdt_decide_diag *d, int *form) {
    return guard([&] {
        need(d, "args");
        const int B = d->B, V = d->V, D = d->D, L = d->L, Hp = d->Hp, F = d->F > 1 ? d->F : 1, J = d->J, rows = d->rows, mt = d->max_tokens, VD = V + D;
        need(B > 0 && rows >= B && d->n_steps >= 1 && d->T >= 1, "B/rows/n_steps/T");
        need(V >= 1 && D >= 0 && D <= 16 && d->blank >= 0 && d->blank < V && mt >= 1 && d->max_symbols >= 1 && d->max_steps >= 0, "V/D/blank/max_tokens/max_symbols/max_steps");
        need(L >= 1 && L <= 4 && Hp >= 1 && (!d->h_bf16 || Hp % 2 == 0), "L/Hp");
        need(d->logits && d->hn && d->cn && d->h && d->c, "logits/hn/cn/h/c");
        need(d->t && d->steps && d->n_out && d->nsym && d->done && d->token && d->lens && d->done_count && d->ids && d->start && d->end && d->conf, "state words / token arrays");
        const size_t hp_h = d->h_bf16 ? Hp / 2 : Hp, n_h = (size_t)L * B * hp_h, n_c = (size_t)L * B * Hp;
        need((size_t)d->h_words >= n_h && (size_t)d->c_words >= n_c, "h_words/c_words");
        TdtState st{};
        st.B = B; st.T = d->T; st.V = V; st.D = D; st.L = L; st.Hp = Hp; st.blank = d->blank; st.max_symbols = d->max_symbols; st.max_tokens = mt;
        st.max_steps = d->max_steps; st.keep_state = d->keep_state; st.h_bf16 = d->h_bf16 ? 1 : 0; st.F = F; st.J = J;
        for (int i = 0; i < 8; ++i) st.durations[i] = d->durations[i];
        const bool pred = d->need != nullptr, boost = d->trie_off != nullptr, score = d->force_label != nullptr;
        // what the engine itself never launches (launch_tdt_decide would abort, or the kernel would leave its buffers)
        // (the form depends on WHETHER these three are set, nothing reads through them here: the caller's own arrays stand in until the device copies exist)
        st.need = d->need; st.trie.off = d->trie_off; st.force_label = d->force_label;
        need(tdt_decide_launchable(st), "L * Hp <= 3072; F > 1 only for the plain exact step with V + D <= 1280, F <= 8, J <= 1024");
        need(tdt_decide_lds_bytes(st) <= 160 * 1024, "LDS above 160 KB");
        need(!(boost && score), "trie and forced path together");
        const int64_t n_rows = (int64_t)d->n_steps * B * F;
        for (int64_t r = 0; D > 8 && r < n_rows; ++r) {            // TdtState holds 8 durations: a longer head must never choose past them
            const float *dl = d->logits + r * VD + V;
            float m8 = dl[0];
            for (int i = 1; i < 8; ++i) m8 = dl[i] > m8 ? dl[i] : m8;
            for (int i = 8; i < D; ++i) need(dl[i] < m8, "D > 8: the duration argmax must stay below index 8");
        }
        for (int b = 0; b < B; ++b) {
            need(d->t[b] >= 0 && d->steps[b] >= 0 && d->n_out[b] >= 0 && d->nsym[b] >= 0, "state words must not be negative");
            need(!d->Tb || d->Tb[b] >= 1, "Tb");
        }
        if (pred) {
            need(d->pp && d->ep && d->z && J >= 1 && d->ep_rows > 0, "need: pp/ep/z/J/ep_rows");
            need((size_t)d->z_words >= (d->h_bf16 ? ((size_t)B * J + 1) / 2 : (size_t)B * F * J), "z_words");
            need(d->h_bf16 || J % 16 == 0, "fp32 z: J must be a multiple of 16 (sigma layout)");
            for (int b = 0; b < B; ++b) {
                const int64_t r0 = d->row0 ? (int64_t)d->row0[b] : (int64_t)b * d->T;
                need(r0 >= 0 && r0 + (d->Tb ? d->Tb[b] : d->T) <= d->ep_rows, "need: enc_proj rows out of range");
            }
        }
        int n_edges = 0;
        if (boost) {
            need(d->trie_tok && d->trie_node && d->act && d->n_act && d->trie_nodes >= 1 && d->trie_off[0] == 0, "trie");
            for (int i = 0; i < d->trie_nodes; ++i) need(d->trie_off[i + 1] >= d->trie_off[i], "trie: offsets must not decrease");
            n_edges = d->trie_off[d->trie_nodes];
            for (int e = 0; e < n_edges; ++e) need(d->trie_node[e] >= 0 && d->trie_node[e] < d->trie_nodes, "trie: child node out of range");
            for (int b = 0; b < B; ++b) {
                need(d->n_act[b] >= 0 && d->n_act[b] <= kTrieMaxActive, "trie: n_act");
                for (int a = 0; a < d->n_act[b]; ++a) {
                    const int sn = d->act[(size_t)b * kTrieMaxActive + a];
                    need(sn >= 0 && sn < d->trie_nodes, "trie: active state out of range");
                }
            }
        }
        int64_t n_force_el = 0;
        if (score) {
            need(D >= 1 && D <= 8 && d->force_dur && d->force_stride >= 0, "forced path: 1 <= D <= 8, force_dur, force_stride");
            for (int b = 0; b < B; ++b) {
                const int nf = d->n_force_b ? d->n_force_b[b] : d->n_force;
                if (nf <= 0) continue;
                n_force_el = std::max(n_force_el, (int64_t)b * d->force_stride + nf);
                need(d->done[b] || d->steps[b] < nf, "forced path: steps past the path");
            }
            need(n_force_el <= d->force_len, "force_len");
            for (int64_t k = 0; k < d->force_len; ++k)
                need(d->force_label[k] >= 0 && d->force_label[k] < V && d->force_dur[k] >= 0 && d->force_dur[k] < D, "forced label / duration out of range");
            need((!d->score_lab && !d->score_dur) || d->score_rows >= n_force_el, "score_rows");
        }
        need_device();
        const size_t nb = (size_t)rows * 4, ntok = (size_t)rows * mt * 4;
        DevBuf lg, hn, cn, h, c, t, steps, n_out, nsym, done, token, lens, dc, ids, start, end, conf, margin, nd, pp, ep, z, Tb, row0, toff, ttok, tnode, act, nact, fl, fd,
            nfb, sl, sd;
        const size_t hn_step = n_h * 4, cn_step = n_c * 4, lg_step = (size_t)B * F * VD * 4;
        up(lg, d->logits, lg_step * d->n_steps); up(hn, d->hn, hn_step * d->n_steps); up(cn, d->cn, cn_step * d->n_steps);
        up(h, d->h, (size_t)d->h_words * 4); up(c, d->c, (size_t)d->c_words * 4);
        up(t, d->t, nb); up(steps, d->steps, nb); up(n_out, d->n_out, nb); up(nsym, d->nsym, nb); up(done, d->done, nb); up(token, d->token, nb); up(lens, d->lens, nb);
        up(dc, d->done_count, 4);
        up(ids, d->ids, ntok); up(start, d->start, ntok); up(end, d->end, ntok); up(conf, d->conf, ntok);
        st.h = h.as<float>(); st.c = c.as<float>();
        st.token = token.as<int>(); st.t = t.as<int>(); st.nsym = nsym.as<int>(); st.n_out = n_out.as<int>(); st.steps = steps.as<int>(); st.done = done.as<int>();
        st.lens = lens.as<int>(); st.done_count = dc.as<int>(); st.ids = ids.as<int>(); st.start = start.as<int>(); st.end = end.as<int>(); st.conf = conf.as<float>();
        if (d->margin) { up(margin, d->margin, nb); st.margin = margin.as<float>(); }
        st.need = nullptr; st.trie = TrieDev{}; st.force_label = nullptr;
        if (pred) {
            up(nd, d->need, nb); up(pp, d->pp, (size_t)B * J * 4); up(ep, d->ep, (size_t)d->ep_rows * J * 4); up(z, d->z, (size_t)d->z_words * 4);
            st.need = nd.as<int>(); st.pp = pp.as<float>(); st.ep = ep.as<float>(); st.z = z.as<float>();
        }
        if (d->Tb) { up(Tb, d->Tb, (size_t)B * 4); st.Tb = Tb.as<int>(); }
        if (d->row0) { up(row0, d->row0, (size_t)B * 4); st.row0 = row0.as<int>(); }
        if (boost) {
            up(toff, d->trie_off, (size_t)(d->trie_nodes + 1) * 4); up(ttok, d->trie_tok, (size_t)std::max(n_edges, 1) * 4); up(tnode, d->trie_node, (size_t)std::max(n_edges, 1) * 4);
            up(act, d->act, (size_t)rows * kTrieMaxActive * 4); up(nact, d->n_act, nb);
            st.trie = TrieDev{toff.as<int>(), ttok.as<int>(), tnode.as<int>(), d->trie_nodes, d->boost, act.as<int>(), nact.as<int>()};
        }
        if (score) {
            up(fl, d->force_label, (size_t)std::max<int64_t>(d->force_len, 1) * 4); up(fd, d->force_dur, (size_t)std::max<int64_t>(d->force_len, 1) * 4);
            st.force_label = fl.as<int>(); st.force_dur = fd.as<int>(); st.n_force = d->n_force; st.force_stride = d->force_stride;
            if (d->n_force_b) { up(nfb, d->n_force_b, (size_t)B * 4); st.n_force_b = nfb.as<int>(); }
            if (d->score_lab) { up(sl, d->score_lab, (size_t)d->score_rows * V * 4); st.score_lab = sl.as<float>(); }
            if (d->score_dur) { up(sd, d->score_dur, (size_t)d->score_rows * D * 4); st.score_dur = sd.as<float>(); }
        }
        for (int k = 0; k < d->n_steps; ++k) {
            st.logits = reinterpret_cast<const float *>(static_cast<const char *>(lg.p) + lg_step * k);
            st.hn = reinterpret_cast<const float *>(static_cast<const char *>(hn.p) + hn_step * k);
            st.cn = reinterpret_cast<const float *>(static_cast<const char *>(cn.p) + cn_step * k);
            launch_tdt_decide(st, nullptr);
        }
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->h, h, (size_t)d->h_words * 4); down(d->c, c, (size_t)d->c_words * 4);
        down(d->t, t, nb); down(d->steps, steps, nb); down(d->n_out, n_out, nb); down(d->nsym, nsym, nb); down(d->done, done, nb); down(d->token, token, nb);
        down(d->lens, lens, nb); down(d->done_count, dc, 4);
        down(d->ids, ids, ntok); down(d->start, start, ntok); down(d->end, end, ntok); down(d->conf, conf, ntok);
        if (d->margin) down(d->margin, margin, nb);
        if (pred) { down(d->need, nd, nb); down(d->z, z, (size_t)d->z_words * 4); }
        if (boost) { down(d->act, act, (size_t)rows * kTrieMaxActive * 4); down(d->n_act, nact, nb); }
        if (score && d->score_lab) down(d->score_lab, sl, (size_t)d->score_rows * V * 4);
        if (score && d->score_dur) down(d->score_dur, sd, (size_t)d->score_rows * D * 4);
        constexpr int kForm = (int)tdt_decide_form_of(TDT_K_SCORE, TDT_NC6, TDT_ROW_BATCH8);
        static_assert(PK_DIAG_TDT_KERNEL(kForm) == TDT_K_SCORE && PK_DIAG_TDT_SLOTS(kForm) == 6 && PK_DIAG_TDT_ROW(kForm) == TDT_ROW_BATCH8, "form fields");
        if (form) *form = (int)tdt_decide_form(st);
    });
}

pk_status pk_diag_tdt_beam_step(const pk_tdt_beam_step_diag *d) {
    return guard([&] {
        need(d, "args");
        const int B = d->B, W = d->W, K = d->K, Kd = d->Kd, N = d->N, V = d->V, D = d->D, MT = d->max_tokens, s = d->step, cap = d->cap;
        const bool fused = d->lm != nullptr, init = d->init != 0, trace = d->trace != 0;
        // what the search's entry points refuse (tdt_beam.cpp), then what launch_tdt_beam_prune would abort on
        if (W < 1 || W > kTdtBeamMaxWidth) fail(PK_ERR_UNSUPPORTED, "TDT beam step: beam_width %d outside 1..%d", W, kTdtBeamMaxWidth);
        if (K < 1 || K > kTdtBeamMaxLabels) fail(PK_ERR_UNSUPPORTED, "TDT beam step: label_prune %d outside 1..%d", K, kTdtBeamMaxLabels);
        if (Kd < 1 || Kd > kTdtBeamMaxDurs) fail(PK_ERR_UNSUPPORTED, "TDT beam step: duration_prune %d outside 1..%d", Kd, kTdtBeamMaxDurs);
        if (D < 1 || D > 8) fail(PK_ERR_UNSUPPORTED, "TDT beam step: %d durations, the kernel is built for 1 to 8", D);
        if (N < 1 || N > W) fail(PK_ERR_UNSUPPORTED, "TDT beam step: n_best %d outside 1..beam_width", N);
        need(Kd <= D, "duration_prune <= D");
        need(V >= 2 && V <= (1 << 20) && K <= V - 1, "label_prune <= V - 1 (V <= 2^20)");
        need(d->blank >= 0 && d->blank < V, "blank outside 0..V - 1");
        need(MT >= 1 && MT <= (1 << 20), "max_tokens (1..2^20)");
        need(B >= 1 && (int64_t)B * W <= (1 << 16), "B (B W <= 2^16)");
        const int R = B * W;
        need(cap >= 1 && cap <= (1 << 20) && s >= 0 && s < cap && d->rows >= R && d->rows <= R + 64, "cap / step (0..cap - 1) / rows (R..R + 64)");
        need((int64_t)R * MT <= (1 << 24) && (int64_t)cap * R <= (1 << 24) && (int64_t)R * (V + D) <= (1 << 26), "R max_tokens, cap R <= 2^24; R (V + D) <= 2^26");
        need(!init || s == 0, "init: the search begins at step 0");
        need(d->T && d->logits, "T/logits");
        need(d->valid && d->t && d->len && d->par && d->born && d->tok && d->score && d->hash && d->prefix, "beam arrays");
        need(d->live && d->steps_done && d->live_total && d->bp, "live/steps_done/live_total/bp");
        need(d->lab_id && d->lab_lp && d->dur_i && d->dur_lp && d->cand, "lab_id/lab_lp/dur_i/dur_lp/cand");
        need(!fused || (d->lmstate && d->lmv && d->lab_ls && d->lab_lm), "lm: lmstate/lmv/lab_ls/lab_lm");
        need(!trace || (d->ids && d->start && d->end && d->dur_idx && d->conf && d->lens && d->out_score && d->ok && (!fused || d->out_lm)), "trace: output arrays");
        for (int b = 0; b < B; ++b) need(d->T[b] >= 1, "T[b] must be positive");
        pk_lm_options lo{d->alpha, d->beta};
        if (fused) lm_fusion_checks(d->lm, &lo, V, d->blank);
        if (!init) {                                                // carried state the kernels index with
            for (int i = 0; i < 2 * R; ++i) {
                need(d->len[i] >= 0 && d->len[i] <= MT && d->t[i] >= 0, "carried beam: len outside 0..max_tokens or t < 0");
                need(!fused || (d->lmstate[i] >= 0 && d->lmstate[i] < lm_num_states(d->lm)), "carried beam: lmstate is no state of the model");
            }
            for (int b = 0; b < B; ++b) {
                const int sd = d->steps_done[b];
                need(sd >= 0 && sd <= cap && (!d->live[b] || sd == s), "steps_done outside 0..cap, or a live clip whose steps_done is not step");
                for (int st = 0; st < sd; ++st)
                    for (int w = 0; w < W; ++w) {
                        const int x = d->bp[((size_t)st * R + (size_t)b * W + w) * 4];
                        need(x >= 0 && x < W, "bp: the parent slot of a step taken is outside 0..W - 1");
                    }
            }
        }
        need_device();
        const size_t nR = (size_t)R, rows = (size_t)d->rows, C_ = (size_t)(K + 1) * Kd, hy = (size_t)B * N, tok = hy * MT;
        DevBuf Tb, lg, ints, score, hash, prefix, ctl, bp, lab_id, lab_lp, dur_i, dur_lp, cand, lmslot, lmlab, out;
        up(Tb, d->T, (size_t)B * 4);
        up(lg, d->logits, nR * (size_t)(V + D) * 4);
        ints.reserve(12 * nR * 4);
        int32_t *const beam_ints[6] = {d->valid, d->t, d->len, d->par, d->born, d->tok};
        for (int k = 0; k < 6; ++k) PK_HIP(hipMemcpy(ints.as<int>() + 2 * nR * k, beam_ints[k], 2 * nR * 4, hipMemcpyHostToDevice));
        up(score, d->score, 2 * nR * 4); up(hash, d->hash, 2 * nR * 8); up(prefix, d->prefix, 2 * nR * MT * 4);
        ctl.reserve((2 * (size_t)B + cap + 1) * 4);
        PK_HIP(hipMemcpy(ctl.as<int>(), d->live, (size_t)B * 4, hipMemcpyHostToDevice));
        PK_HIP(hipMemcpy(ctl.as<int>() + B, d->steps_done, (size_t)B * 4, hipMemcpyHostToDevice));
        PK_HIP(hipMemcpy(ctl.as<int>() + 2 * B, d->live_total, ((size_t)cap + 1) * 4, hipMemcpyHostToDevice));
        up(bp, d->bp, (size_t)cap * nR * 16);
        up(lab_id, d->lab_id, rows * (K + 1) * 4); up(lab_lp, d->lab_lp, rows * (K + 1) * 4);
        up(dur_i, d->dur_i, rows * Kd * 4); up(dur_lp, d->dur_lp, rows * Kd * 4); up(cand, d->cand, rows * C_ * 4);
        TdtBeamDev a{};
        a.B = B; a.W = W; a.K = K; a.Kd = Kd; a.N = N; a.V = V; a.D = D; a.blank = d->blank; a.max_tokens = MT;
        for (int i = 0; i < 8; ++i) a.durations[i] = i < D ? d->durations[i] : 0;
        a.T = Tb.as<int>(); a.row0 = nullptr;
        int *iv = ints.as<int>();
        a.valid = iv; a.t = iv + 2 * nR; a.len = iv + 4 * nR; a.par = iv + 6 * nR; a.born = iv + 8 * nR; a.tok = iv + 10 * nR;
        a.score = score.as<float>(); a.hash = hash.as<unsigned long long>(); a.prefix = prefix.as<int>();
        a.lab_id = lab_id.as<int>(); a.lab_lp = lab_lp.as<float>(); a.dur_i = dur_i.as<int>(); a.dur_lp = dur_lp.as<float>(); a.cand = cand.as<float>();
        a.bp = bp.as<int4>();
        a.live = ctl.as<int>(); a.steps_done = a.live + B; a.live_total = a.live + 2 * (size_t)B;
        if (fused) {
            lmslot.reserve(4 * nR * 4); lmlab.reserve(2 * rows * (K + 1) * 4);
            a.lmstate = lmslot.as<int>(); a.lm = reinterpret_cast<float *>(a.lmstate + 2 * nR);
            a.lab_ls = lmlab.as<int>(); a.lab_lm = reinterpret_cast<float *>(a.lab_ls + rows * (K + 1));
            PK_HIP(hipMemcpy(a.lmstate, d->lmstate, 2 * nR * 4, hipMemcpyHostToDevice)); PK_HIP(hipMemcpy(a.lm, d->lmv, 2 * nR * 4, hipMemcpyHostToDevice));
            PK_HIP(hipMemcpy(a.lab_ls, d->lab_ls, rows * (K + 1) * 4, hipMemcpyHostToDevice));
            PK_HIP(hipMemcpy(a.lab_lm, d->lab_lm, rows * (K + 1) * 4, hipMemcpyHostToDevice));
            a.ngram = lm_device_view(d->lm, &lo);
        }
        TdtBeamOut o{};
        if (trace) {
            out.reserve((5 * tok + 3 * hy + B) * 4);
            int *p = out.as<int>();
            o.ids = p; o.start = p + tok; o.end = p + 2 * tok; o.dur_idx = p + 3 * tok; o.conf = reinterpret_cast<float *>(p + 4 * tok);
            o.lens = p + 5 * tok; o.score = reinterpret_cast<float *>(p + 5 * tok + hy); o.ok = p + 5 * tok + 2 * hy;
            if (fused) o.lm_score = reinterpret_cast<float *>(o.ok + B);
            const void *const src[9] = {d->ids, d->start, d->end, d->dur_idx, d->conf, d->lens, d->out_score, d->ok, d->out_lm};
            void *const dst[9] = {o.ids, o.start, o.end, o.dur_idx, o.conf, o.lens, o.score, o.ok, o.lm_score};
            const size_t n[9] = {tok, tok, tok, tok, tok, hy, hy, (size_t)B, hy};
            for (int k = 0; k < (fused ? 9 : 8); ++k) PK_HIP(hipMemcpy(dst[k], src[k], n[k] * 4, hipMemcpyHostToDevice));
        }
        if (init) launch_tdt_beam_init(a, nullptr);
        launch_tdt_beam_expand(a, s, lg.as<float>(), nullptr);
        launch_tdt_beam_prune(a, s, nullptr);
        if (trace) launch_tdt_beam_trace(a, o, nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        for (int k = 0; k < 6; ++k) PK_HIP(hipMemcpy(beam_ints[k], ints.as<int>() + 2 * nR * k, 2 * nR * 4, hipMemcpyDeviceToHost));
        down(d->score, score, 2 * nR * 4); down(d->hash, hash, 2 * nR * 8); down(d->prefix, prefix, 2 * nR * MT * 4);
        PK_HIP(hipMemcpy(d->live, ctl.as<int>(), (size_t)B * 4, hipMemcpyDeviceToHost));
        PK_HIP(hipMemcpy(d->steps_done, ctl.as<int>() + B, (size_t)B * 4, hipMemcpyDeviceToHost));
        PK_HIP(hipMemcpy(d->live_total, ctl.as<int>() + 2 * B, ((size_t)cap + 1) * 4, hipMemcpyDeviceToHost));
        down(d->bp, bp, (size_t)cap * nR * 16);
        down(d->lab_id, lab_id, rows * (K + 1) * 4); down(d->lab_lp, lab_lp, rows * (K + 1) * 4);
        down(d->dur_i, dur_i, rows * Kd * 4); down(d->dur_lp, dur_lp, rows * Kd * 4); down(d->cand, cand, rows * C_ * 4);
        if (fused) {
            PK_HIP(hipMemcpy(d->lmstate, a.lmstate, 2 * nR * 4, hipMemcpyDeviceToHost)); PK_HIP(hipMemcpy(d->lmv, a.lm, 2 * nR * 4, hipMemcpyDeviceToHost));
            PK_HIP(hipMemcpy(d->lab_ls, a.lab_ls, rows * (K + 1) * 4, hipMemcpyDeviceToHost));
            PK_HIP(hipMemcpy(d->lab_lm, a.lab_lm, rows * (K + 1) * 4, hipMemcpyDeviceToHost));
        }
        if (trace) {
            void *const dst[9] = {d->ids, d->start, d->end, d->dur_idx, d->conf, d->lens, d->out_score, d->ok, d->out_lm};
            const void *const src[9] = {o.ids, o.start, o.end, o.dur_idx, o.conf, o.lens, o.score, o.ok, o.lm_score};
            const size_t n[9] = {tok, tok, tok, tok, tok, hy, hy, (size_t)B, hy};
            for (int k = 0; k < (fused ? 9 : 8); ++k) PK_HIP(hipMemcpy(dst[k], src[k], n[k] * 4, hipMemcpyDeviceToHost));
        }
    });
}

pk_status pk_diag_ctc_greedy(const pk_ctc_greedy_diag *d) {
    return guard([&] {
        need(d, "args");
        const int B = d->B, T = d->T, n = d->n, ld = d->ld, rows_out = d->out_rows, pitch = d->pitch;
        need(d->logits && d->lp && d->best_idx && d->best_lp && d->best_idx2 && d->best_lp2, "logits/lp/best_idx/best_lp/best_idx2/best_lp2");
        need(d->ids && d->lens && d->start && d->end && d->conf, "token arrays");
        need(B > 0 && n >= 1 && ld >= n && d->blank >= 0 && d->blank < n && rows_out >= B, "B/n/ld/blank/out_rows");
        int64_t rows = 0;
        int tmax = 0;
        std::vector<int32_t> img;                                      // SeqRag::T [B] then T_off [B + 1]
        if (d->n_frames) {
            img.assign(d->n_frames, d->n_frames + B);
            img.push_back(0);
            for (int b = 0; b < B; ++b) { need(d->n_frames[b] >= 1, "n_frames"); tmax = std::max(tmax, (int)d->n_frames[b]); rows += d->n_frames[b]; img.push_back((int32_t)rows); }
        } else {
            need(T >= 1, "T");
            rows = (int64_t)B * T; tmax = T;
        }
        need(pitch >= tmax, "pitch >= the longest utterance");
        need(d->lp_rows >= rows, "lp_rows >= the frames of the batch");
        const bool boost = d->trie_off != nullptr;
        int n_edges = 0;
        if (boost) {
            need(d->trie_tok && d->trie_node && d->trie_nodes >= 1 && d->trie_off[0] == 0, "trie");
            for (int i = 0; i < d->trie_nodes; ++i) need(d->trie_off[i + 1] >= d->trie_off[i], "trie: offsets must not decrease");
            n_edges = d->trie_off[d->trie_nodes];
            for (int e = 0; e < n_edges; ++e) need(d->trie_node[e] >= 0 && d->trie_node[e] < d->trie_nodes, "trie: child node out of range");
        }
        need_device();
        DevBuf lg, lp, bi, bl, bi2, bl2, ids, lens, start, end, conf, rimg, toff, ttok, tnode;
        const size_t nl = (size_t)d->lp_rows, ntok = (size_t)rows_out * pitch * 4;
        up(lg, d->logits, (size_t)rows * ld * 4);
        up(lp, d->lp, nl * n * 4); up(bi, d->best_idx, nl * 4); up(bl, d->best_lp, nl * 4); up(bi2, d->best_idx2, nl * 4); up(bl2, d->best_lp2, nl * 4);
        up(ids, d->ids, ntok); up(start, d->start, ntok); up(end, d->end, ntok); up(conf, d->conf, ntok); up(lens, d->lens, (size_t)rows_out * 4);
        SeqRag rag;
        if (d->n_frames) {
            up(rimg, img.data(), img.size() * 4);
            rag.T = rimg.as<int>(); rag.T_off = rimg.as<int>() + B; rag.T_max = tmax;
        }
        launch_logsoftmax_argmax(lg.as<float>(), rows, ld, n, nullptr, bi2.as<int>(), bl2.as<float>(), nullptr);      // without the log-prob rows ...
        launch_logsoftmax_argmax(lg.as<float>(), rows, ld, n, lp.as<float>(), bi.as<int>(), bl.as<float>(), nullptr);  // ... and with them
        if (boost) {
            up(toff, d->trie_off, (size_t)(d->trie_nodes + 1) * 4); up(ttok, d->trie_tok, (size_t)std::max(n_edges, 1) * 4); up(tnode, d->trie_node, (size_t)std::max(n_edges, 1) * 4);
            const TrieDev trie{toff.as<int>(), ttok.as<int>(), tnode.as<int>(), d->trie_nodes, d->boost, nullptr, nullptr};
            launch_ctc_boosted(lp.as<float>(), B, T, n, d->blank, trie, ids.as<int>(), lens.as<int>(), start.as<int>(), end.as<int>(), conf.as<float>(), nullptr, pitch, rag);
        } else {
            launch_ctc_collapse(bi.as<int>(), bl.as<float>(), B, T, d->blank, ids.as<int>(), lens.as<int>(), start.as<int>(), end.as<int>(), conf.as<float>(), nullptr, pitch, rag);
        }
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->lp, lp, nl * n * 4); down(d->best_idx, bi, nl * 4); down(d->best_lp, bl, nl * 4); down(d->best_idx2, bi2, nl * 4); down(d->best_lp2, bl2, nl * 4);
        down(d->ids, ids, ntok); down(d->start, start, ntok); down(d->end, end, ntok); down(d->conf, conf, ntok); down(d->lens, lens, (size_t)rows_out * 4);
    });
}

pk_status pk_diag_layernorm(const float *x, int64_t rows, int d, const float *gamma, const float *beta, float eps, float *y) {
    return guard([&] {
        need(x && gamma && beta && y && rows > 0 && d > 0 && d <= 1024, "x/gamma/beta/y/rows/d (d <= 1024)");
        need_device();
        DevBuf xb, g, b, yb;
        up(xb, x, (size_t)rows * d * 4);
        up(g, gamma, (size_t)d * 4);
        up(b, beta, (size_t)d * 4);
        yb.reserve((size_t)rows * d * 4);
        launch_layernorm(xb.as<float>(), rows, d, g.as<float>(), b.as<float>(), eps, yb.as<float>(), nullptr);
        PK_CHECK_LAUNCH();
        down(y, yb, (size_t)rows * d * 4);
    });
}

static void diag_layernorm(const float *x, int64_t rows, int d, const float *gamma, const float *beta, float eps, float *y, int mode) {
    need(x && gamma && beta && y && rows > 0 && d > 0 && d <= 1024, "x/gamma/beta/y/rows/d (d <= 1024)");
    need(mode == 0 || d % 16 == 0, "sigma columns: d must be a multiple of 16");
    need_device();
    DevBuf xb, gb, yb;
    up(xb, x, (size_t)rows * d * 4);
    const NormVecs v = up_norms(gb, d, gamma, beta);
    yb.reserve((size_t)rows * d * 4);
    launch_layernorm(xb.as<float>(), rows, d, v.g, v.b, eps, yb.as<float>(), nullptr, mode);
    PK_CHECK_LAUNCH();
    down(y, yb, (size_t)rows * d * 4);
}

pk_status pk_diag_layernorm_sigma(const float *x, int64_t rows, int d, const float *gamma, const float *beta, float eps, float *y) {
    return guard([&] { diag_layernorm(x, rows, d, gamma, beta, eps, y, 2); });
}

pk_status pk_diag_layernorm2(const float *x, int64_t rows, int d, const float *g1, const float *b1, const float *g2, const float *b2, float eps,
                             int y2_sigma, float *y1, float *y2) {
    return guard([&] {
        need(x && g1 && b1 && g2 && b2 && y1 && y2 && rows > 0 && d > 0 && d <= 1024, "x/g1/b1/g2/b2/y1/y2/rows/d (d <= 1024)");
        need(!y2_sigma || d % 16 == 0, "sigma columns: d must be a multiple of 16");
        need_device();
        DevBuf xb, gb, o1, o2;
        up(xb, x, (size_t)rows * d * 4);
        const NormVecs v = up_norms(gb, d, g1, b1, g2, b2);
        o1.reserve((size_t)rows * d * 4);
        o2.reserve((size_t)rows * d * 4);
        launch_layernorm2(xb.as<float>(), rows, d, v.g, v.b, v.g2, v.b2, eps, o1.as<float>(), o2.as<float>(), nullptr, y2_sigma ? 2 : 0);
        PK_CHECK_LAUNCH();
        down(y1, o1, (size_t)rows * d * 4);
        down(y2, o2, (size_t)rows * d * 4);
    });
}

// the PK_DIAG_LN_* macros of include/parakeet_amd.h decode what ln_form_of (kernels.hpp) encodes
constexpr int kLnFormProbe = ln_form_of(LN_THEN_STATS, 16, 3, true, true);
static_assert(PK_DIAG_LN_LAUNCHER(kLnFormProbe) == LN_THEN_STATS && PK_DIAG_LN_BATCH(kLnFormProbe) == 1 && PK_DIAG_LN_THEN(kLnFormProbe) == 1 &&
              PK_DIAG_LN_RPW(kLnFormProbe) == 3 && PK_DIAG_LN_PER_LANE(kLnFormProbe) == 16 && PK_DIAG_LN_THEN(ln_form_of(LN_NORM2, 8, 1, false, false)) == 0 &&
              PK_DIAG_LN_NORM == LN_NORM && PK_DIAG_LN_NORM2 == LN_NORM2 && PK_DIAG_LN_STATS == LN_STATS && PK_DIAG_LN_THEN_STATS == LN_THEN_STATS,
              "PK_DIAG_LN_* must decode ln_form_of");

int pk_diag_layernorm_forms(int32_t *out, int cap) { return copy_forms(kLnForms, kLnFormCount, out, cap); }

// the form the launcher would take: the launcher's own function (host arithmetic)
static int ln_diag_form(int launcher, int64_t rows, int d) {
    need(launcher >= 0 && launcher < LN_LAUNCHERS, "launcher (PK_DIAG_LN_NORM .. PK_DIAG_LN_THEN_STATS)");
    need(rows > 0 && d > 0, "rows/d");
    const int form = launcher == LN_NORM ? layernorm_form(rows, d) : launcher == LN_NORM2 ? layernorm2_form(rows, d)
                   : launcher == LN_STATS ? layernorm_stats_form(rows, d) : layernorm_then_stats_form(rows, d);
    if (form < 0) fail(PK_ERR_UNSUPPORTED, "pk_diag_layernorm_form: a row of %d columns (the LayerNorm kernels hold at most %d)", d, kLnMaxCols);
    return form;
}

pk_status pk_diag_layernorm_form_of(int launcher, int64_t rows, int d, int32_t *form) {
    return guard([&] {
        need(form, "form");
        *form = (int32_t)ln_diag_form(launcher, rows, d);
    });
}

pk_status pk_diag_layernorm_form(pk_layernorm_diag *a) {
    return guard([&] {
        need(a, "args");
        const int launcher = a->launcher, d = a->d, mode = a->mode;
        const int64_t rows = a->rows;
        (void)ln_diag_form(launcher, rows, d);                         // refuses what the launcher would refuse, before a device is looked for
        const bool norm = launcher == LN_NORM, norm2 = launcher == LN_NORM2, stats = launcher == LN_STATS || launcher == LN_THEN_STATS;
        const bool has_y = launcher != LN_STATS;                       // y: launch_layernorm's y, y1 of the other two
        need(a->x, "x");
        need(!(norm || norm2 || launcher == LN_THEN_STATS) || (a->g1 && a->b1), "g1/b1");
        need(!norm2 || (a->g2 && a->b2), "g2/b2");
        need(mode >= 0 && mode <= 2 && (mode == 0 || norm || norm2), "mode: 0, or 1 / 2 with launch_layernorm / launch_layernorm2");
        need(mode != 2 || d % 16 == 0, "sigma columns: d must be a multiple of 16");
        need(!a->in_place || (has_y && !(norm && mode != 0)), "in_place: launch_layernorm in mode 0, y1 of launch_layernorm2 / launch_layernorm_then_stats");
        // every buffer the launch writes is longer than what it may write: the words past the end come back as the fill pattern
        const int64_t n = rows * d;
        const int64_t y_need = (norm && mode == 1) ? n / 2 + 1 : n + 1, y2_need = mode == 1 ? n / 2 + 1 : n + 1;
        need(!has_y || (a->y && a->y_words >= y_need), "y / y_words: longer than rows * d elements");
        need(!norm2 || (a->y2 && a->y2_words >= y2_need), "y2 / y2_words: longer than rows * d elements");
        need(!stats || (a->stats && a->stats_words > 2 * rows), "stats / stats_words: longer than 2 * rows");
        need_device();
        DevBuf xb, gb, yb, y2b, sb;
        if (has_y) filled(yb, a->y_words);
        if (norm2) filled(y2b, a->y2_words);
        if (stats) filled(sb, a->stats_words);
        const float *x;
        if (a->in_place) {                                             // x lives at the start of the y / y1 buffer
            PK_HIP(hipMemcpy(yb.p, a->x, (size_t)n * 4, hipMemcpyHostToDevice));
            x = yb.as<float>();
        } else {
            up(xb, a->x, (size_t)n * 4);
            x = xb.as<float>();
        }
        const NormVecs v = up_norms(gb, d, a->g1, a->b1, a->g2, a->b2);
        int form = -1;
        switch (launcher) {
        case LN_NORM: form = launch_layernorm(x, rows, d, v.g, v.b, a->eps, yb.as<float>(), nullptr, mode); break;
        case LN_NORM2: form = launch_layernorm2(x, rows, d, v.g, v.b, v.g2, v.b2, a->eps, yb.as<float>(), y2b.as<float>(), nullptr, mode); break;
        case LN_STATS: form = launch_layernorm_stats(x, rows, d, a->eps, sb.as<float>(), nullptr); break;
        default: form = launch_layernorm_then_stats(x, rows, d, v.g, v.b, a->eps, yb.as<float>(), sb.as<float>(), nullptr); break;
        }
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        a->form = (int32_t)form;                                       // what the launcher switched on, not a second evaluation here
        if (has_y) down(a->y, yb, (size_t)a->y_words * 4);
        if (norm2) down(a->y2, y2b, (size_t)a->y2_words * 4);
        if (stats) down(a->stats, sb, (size_t)a->stats_words * 4);
    });
}

pk_status pk_diag_sum64(const float *x, int rows, int n, float *out) {
    return guard([&] {
        need(x && out && rows > 0 && n > 0, "x/out/rows/n");
        need_device();
        DevBuf xb, sums;
        up(xb, x, (size_t)rows * n * 4);
        sums.reserve((size_t)rows * 4);
        launch_sum64_rows(xb.as<float>(), rows, n, sums.as<float>(), nullptr);
        PK_CHECK_LAUNCH();
        down(out, sums, (size_t)rows * 4);
    });
}

// The launchers' own selection functions (kernels/kernels.hpp) for a model and a batch: what tests/test_gpu_conv_variants.py asks before it compares bits.
pk_status pk_diag_conv_variants(const pk_model *h, int B, int Tm, const int32_t *n_mel_frames, int stream_c, int32_t *out) {
    return guard([&] {
        need(h && out && B > 0 && (n_mel_frames || Tm > 0), "model/out/B/Tm");
        const pk_config &cfg = h->m->cfg;
        auto sl = [](int n) { return (n - 1) / 2 + 1; };
        int64_t rows_h2 = 0, rows_t = 0;
        for (int b = 0; b < B; ++b) {
            const int tm = n_mel_frames ? n_mel_frames[b] : Tm;
            need(tm > 0, "every utterance needs at least one mel frame");
            const int h2 = sl(sl(tm));
            rows_h2 += h2; rows_t += sl(h2);
        }
        const int W2 = sl(sl(cfg.mel_bins)), W3 = sl(W2);
        const int c1 = sub_conv1_dw1_inst(sub_conv1_dw1_strip_rows(rows_h2), cfg.subsampling_channels, W2), d2 = sub_dw_inst(W3);
        const int dw = dwconv_inst(rows_t, cfg.conv_kernel_size), sd = stream_dwconv_inst(cfg.conv_kernel_size);
        const ConvInst *i0 = conv_inst(0, c1), *i1 = conv_inst(1, d2), *i2 = conv_inst(2, dw), *i3 = conv_inst(3, sd);
        if (!i0 || !i1 || !i2 || !i3) fail(PK_ERR_UNSUPPORTED, "no kernel instantiation for this configuration");
        const int32_t v[PK_DIAG_CONV_VARIANT_WORDS] = {
            c1, i0->p0, i0->p1, i0->p2, (int32_t)rows_h2, d2, i1->p1, dw, i2->p0, i2->p1, i2->p2, (int32_t)rows_t,
            stream_c > 0 ? sd : -1, stream_c > 0 ? i3->p0 : -1, stream_c > 0 ? i3->p1 : -1, stream_c > 0 ? (stream_c <= i3->p1 ? 0 : 1) : -1,
            stream_c > 0 ? (int32_t)stream_dwconv_tail_fusable(stream_c, cfg.conv_kernel_size) : -1};
        memcpy(out, v, sizeof v);
    });
}
int pk_diag_conv_instantiations(int32_t *out, int cap_rows) {
    const int n = (int)(sizeof(kConvInsts) / sizeof(kConvInsts[0]));
    for (int i = 0; out && i < n && i < cap_rows; ++i) {
        const ConvInst &c = kConvInsts[i];
        const int32_t row[5] = {c.launcher, c.inst, c.p0, c.p1, c.p2};
        memcpy(out + 5 * i, row, sizeof row);
    }
    return n;
}
pk_status pk_diag_pos_table_frames(const pk_model *h, int32_t out[2]) {
    return guard([&] {
        need(h && out, "model/out");
        out[0] = h->m->pos32.T;
        out[1] = h->m->pos16.T;
    });
}

/* ---- one attention layer alone ------------------------------------------------------------------------------------------------------ */
// The batch of an attention diagnostic: B utterances of T frames, or (lens) of lens[b] frames each, packed.  -> the frames of the batch; T
// becomes the longest utterance (the launchers size the launch by it, as run_layers passes it).
static int64_t att_extents(const int32_t *lens, int B, int &T) {
    if (!lens) return (int64_t)B * T;
    int64_t rows = 0;
    T = 0;
    for (int b = 0; b < B; ++b) { need(lens[b] > 0, "lens"); T = std::max(T, (int)lens[b]); rows += lens[b]; }
    return rows;
}
// The encoder-frame batch of pk_conformer_blocks_ragged as the attention launchers take it: the engine's RagBatch of lens in attention blocks
// of block_rows rows, its image on the device, the views Workspace::set_ragged forms.  Uniform batch (no lens): the empty view.
static SeqRag att_rag(RagBatch &r, DevBuf &img, const int32_t *lens, int B, int block_rows, int pos_T) {
    SeqRag rag;
    if (!lens) return rag;
    r.build_from_frames(lens, B, block_rows);
    up(img, r.image.data(), r.image.size() * 4);
    const int32_t *dv = img.as<int32_t>();
    rag.units = {reinterpret_cast<const RagUnit *>(dv + r.o_u_att), r.n_u_att};
    rag.T = dv + r.o_T; rag.T_off = dv + r.o_T_off; rag.T_max = r.T_max; rag.pos_T = pos_T;
    return rag;
}
// [rows][cols] with the columns below n_sigma in the sigma layout, the way the producing GEMM writes them (GemmArgs::sigma_cols: 2 d of the
// 3 d columns of the qkv GEMM, every column of pos_proj)
static std::vector<float> att_sigma(const float *x, int64_t rows, int cols, int n_sigma) {
    std::vector<float> y((size_t)rows * cols);
    for (int64_t i = 0; i < rows; ++i)
        for (int c = 0; c < cols; ++c) y[(size_t)i * cols + (c < n_sigma ? dec_sigma(c) : c)] = x[(size_t)i * cols + c];
    return y;
}

// One relative-position attention layer alone, launched as run_layers launches it: the operands laid out the way their producing GEMMs
// write them (fp32: q / k thirds and the table in the sigma columns; bf16: everything rounded to bf16, natural columns, c vector on the device),
// a ragged batch described by the engine's RagBatch, the long-sequence scratch where the score block does not fit LDS.
pk_status pk_diag_relpos_attention(int kernel, int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv, const float *pos, int pos_T,
                                   const float *bias_u, const float *bias_v, float *ctx, int *variant) {
    return guard([&] {
        need(kernel == 0 || kernel == 1, "kernel must be 0 (fp32) or 1 (bf16)");
        need(qkv && pos && bias_u && bias_v && ctx && B > 0 && d > 0 && n_heads > 0 && d % n_heads == 0, "qkv/pos/bias_u/bias_v/ctx/B/d/n_heads");
        const int hd = d / n_heads;
        const int64_t rows = att_extents(lens, B, T);
        need(T > 0 && pos_T >= T, "T > 0 and pos_T >= T (ragged: >= max(lens))");
        if (kernel == 1) need(relpos_attention_bf16_lds_bytes(T, hd) > 0 && relpos_attention_bf16_lds_bytes(T, hd) <= 160 * 1024, "bf16 kernel: hd 64 or 128");
        else need(relpos_attention_lds_bytes(T, hd) > 0, "fp32 kernel: hd 32, 64, 96 or 128");
        need_device();
        const int64_t Ptab = 2 * (int64_t)pos_T - 1, n_ctx = (rows + PK_DIAG_ATTENTION_GUARD_ROWS) * d;
        RagBatch r;
        DevBuf rag_img, q, p, bu, bv, out;
        const SeqRag rag = att_rag(r, rag_img, lens, B, kernel == 1 ? relpos_attention_bf16_block_rows(hd) : 32, pos_T);
        up(bu, bias_u, (size_t)d * 4);
        up(bv, bias_v, (size_t)d * 4);
        int var = lens ? 2 : 0;
        if (kernel == 1) {
            DevBuf cvec;
            up16(q, qkv, (size_t)rows * 3 * d);
            up16(p, pos, (size_t)Ptab * d);
            cvec.reserve((size_t)n_heads * Ptab * 4);
            filled16(out, n_ctx);
            launch_pos_cvec(p.p, bu.as<float>(), bv.as<float>(), (int)Ptab, d, n_heads, cvec.as<float>(), nullptr);
            launch_relpos_attention_bf16(q.p, B, T, d, n_heads, p.p, cvec.as<float>(), bu.as<float>(), out.p, nullptr, pos_T, rag);
            PK_CHECK_LAUNCH();
            down16(ctx, out, (size_t)n_ctx);
            if (variant) *variant = var | 4;
            return;
        }
        const std::vector<float> qs = att_sigma(qkv, rows, 3 * d, 2 * d), ps = att_sigma(pos, Ptab, d, d);
        up(q, qs.data(), qs.size() * 4);
        up(p, ps.data(), ps.size() * 4);
        filled(out, n_ctx);
        DevBuf scratch;                                              // run_layers: a [32][T] score block past the LDS goes to global scratch
        if (relpos_attention_lds_bytes(T, hd) > 160 * 1024) {
            scratch.reserve(lens ? relpos_attention_scratch_bytes_units(r.n_u_att, T, n_heads, hd) : relpos_attention_scratch_bytes(B, T, n_heads, hd));
            var |= 1;
        }
        launch_relpos_attention(q.as<float>(), B, T, d, n_heads, p.as<float>(), bu.as<float>(), bv.as<float>(), out.as<float>(), nullptr, 0.0f,
                                scratch.as<float>(), 0, pos_T - T, rag);
        PK_CHECK_LAUNCH();
        down(ctx, out, (size_t)n_ctx * 4);
        if (variant) *variant = var;
    });
}

// The fp32 attention layer with the kernel form chosen by the caller (kernels.hpp ATT_FORM_*), any of the three ctx layouts, with or without
// the position term: what the strip form is held against the block form with.
pk_status pk_diag_relpos_attention_form(int form, int out_mode, int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv, const float *pos,
                                        int pos_T, const float *bias_u, const float *bias_v, float *ctx, int *form_ran) {
    return guard([&] {
        need(form == ATT_FORM_AUTO || form == ATT_FORM_BLOCK || form == ATT_FORM_STRIP, "form must be 0 (default), 1 (block) or 2 (strip)");
        need(out_mode >= 0 && out_mode <= 2, "out_mode must be 0 (fp32), 1 (bf16) or 2 (fp32, sigma columns)");
        need(qkv && ctx && B > 0 && d > 0 && n_heads > 0 && d % n_heads == 0, "qkv/ctx/B/d/n_heads");
        need(!pos || (bias_u && bias_v), "pos needs bias_u and bias_v");
        const int hd = d / n_heads;
        const int64_t rows = att_extents(lens, B, T);
        need(T > 0 && (!pos || pos_T >= T), "T > 0 and pos_T >= T (ragged: >= max(lens))");
        need(relpos_attention_lds_bytes(T, hd) > 0, "fp32 kernel: hd 32, 64, 96 or 128");
        need(out_mode != 2 || d % 16 == 0, "sigma columns: d must be a multiple of 16");
        const bool long_seq = relpos_attention_lds_bytes(T, hd) > 160 * 1024;
        const int ran = relpos_attention_form(T, hd, long_seq, form);
        if (ran < 0) fail(PK_ERR_UNSUPPORTED, "the strip form covers head sizes 32 and 64 up to 128 frames (got hd %d, T %d)", hd, T);
        need_device();
        const int64_t Ptab = 2 * (int64_t)pos_T - 1, n_ctx = (rows + PK_DIAG_ATTENTION_GUARD_ROWS) * d;
        RagBatch r;
        DevBuf rag_img, q, p, bu, bv, out, scratch;
        const SeqRag rag = att_rag(r, rag_img, lens, B, 32, pos ? pos_T : T);
        const std::vector<float> qs = att_sigma(qkv, rows, 3 * d, 2 * d);
        up(q, qs.data(), qs.size() * 4);
        if (pos) {
            const std::vector<float> ps = att_sigma(pos, Ptab, d, d);
            up(p, ps.data(), ps.size() * 4);
            up(bu, bias_u, (size_t)d * 4);
            up(bv, bias_v, (size_t)d * 4);
        }
        if (out_mode == 1) filled16(out, n_ctx);
        else filled(out, n_ctx);
        if (long_seq) scratch.reserve(lens ? relpos_attention_scratch_bytes_units(r.n_u_att, T, n_heads, hd) : relpos_attention_scratch_bytes(B, T, n_heads, hd));
        launch_relpos_attention(q.as<float>(), B, T, d, n_heads, pos ? p.as<float>() : nullptr, pos ? bu.as<float>() : nullptr,
                                pos ? bv.as<float>() : nullptr, out.as<float>(), nullptr, 0.0f, long_seq ? scratch.as<float>() : nullptr, out_mode,
                                pos ? pos_T - T : 0, rag, form);
        PK_CHECK_LAUNCH();
        if (out_mode == 1) down16(ctx, out, (size_t)n_ctx);
        else down(ctx, out, (size_t)n_ctx * 4);
        if (form_ran) *form_ran = ran;
    });
}

// One limited-context attention layer alone on the band kernel (kernels/attention.hip, BAND instantiation), launched as run_layers launches it in local mode.
pk_status pk_diag_relpos_local_attention(int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv, const float *pos, int left, int right,
                                         const float *bias_u, const float *bias_v, int out_mode, float *ctx, int *variant) {
    return guard([&] {
        need(qkv && pos && bias_u && bias_v && ctx && B > 0 && d > 0 && n_heads > 0 && d % n_heads == 0, "qkv/pos/bias_u/bias_v/ctx/B/d/n_heads");
        need(out_mode == 0 || out_mode == 1, "out_mode must be 0 (fp32) or 1 (bf16)");
        need((left == -1 && right == -1) || (left >= 0 && right >= 0), "left / right: both >= 0");
        need(left >= 0, "pk_diag_relpos_local_attention runs the band kernel: left, right >= 0");
        const int hd = d / n_heads, span = relpos_local_attention_max_span(hd);
        if (span < 0) fail(PK_ERR_UNSUPPORTED, "band kernel: hd 32, 64, 96 or 128 (got %d)", hd);
        if ((int64_t)left + right > span)
            fail(PK_ERR_UNSUPPORTED, "attention context (%d, %d): left + right is at most %d at head size %d", left, right, span, hd);
        const int64_t rows = att_extents(lens, B, T);
        need(T > 0, "T > 0 (ragged: lens > 0)");
        need_device();
        const int64_t Ptab = (int64_t)left + right + 1, n_ctx = (rows + PK_DIAG_ATTENTION_GUARD_ROWS) * d;
        RagBatch r;
        DevBuf rag_img, q, p, bu, bv, out;
        const SeqRag rag = att_rag(r, rag_img, lens, B, 32, /*pos_T=*/0);
        const std::vector<float> qs = att_sigma(qkv, rows, 3 * d, 2 * d), ps = att_sigma(pos, Ptab, d, d);
        up(q, qs.data(), qs.size() * 4);
        up(p, ps.data(), ps.size() * 4);
        up(bu, bias_u, (size_t)d * 4);
        up(bv, bias_v, (size_t)d * 4);
        if (out_mode == 1) filled16(out, n_ctx);
        else filled(out, n_ctx);
        launch_relpos_local_attention(q.as<float>(), B, T, d, n_heads, p.as<float>(), bu.as<float>(), bv.as<float>(), out.as<float>(), nullptr,
                                      out_mode, left, right, rag);
        PK_CHECK_LAUNCH();
        if (out_mode == 1) down16(ctx, out, (size_t)n_ctx);
        else down(ctx, out, (size_t)n_ctx * 4);
        if (variant) *variant = 8 | (lens ? 2 : 0) | (out_mode == 1 ? 16 : 0);
    });
}

// The cached attention of a streaming chunk alone, launched as StreamBatch::encode launches it (stream.cpp): natural columns, the rotation of
// the caches into a second buffer pair riding on the same launch.
pk_status pk_diag_stream_attention(int S, int c, int nc, int cache_rows, int d, int n_heads, const float *qkv_new, const float *kcache,
                                   const float *vcache, const float *pos, int P, const float *bias_u, const float *bias_v, int att_left,
                                   int att_right, int keep_max, int ctx_sigma, int rotate, float *ctx, float *cache_k_out, float *cache_v_out,
                                   int *form) {
    return guard([&] {
        need(qkv_new && kcache && vcache && pos && bias_u && bias_v && ctx, "qkv_new/kcache/vcache/pos/bias_u/bias_v/ctx");
        need(S > 0 && d > 0 && n_heads > 0 && d % n_heads == 0 && (d / n_heads) % 4 == 0, "S/d/n_heads (head size a multiple of 4)");
        need(c > 0, "c > 0");
        need(cache_rows > 0 && nc >= 0 && nc <= cache_rows, "0 <= nc <= cache_rows, cache_rows > 0");
        need(P >= nc + c, "P >= nc + c");
        need(!ctx_sigma || d % 16 == 0, "ctx_sigma: d must be a multiple of 16");
        need(!rotate || (cache_k_out && cache_v_out && keep_max <= cache_rows), "rotate: cache_k_out/cache_v_out, keep_max <= cache_rows");
        need_device();
        const size_t n_ctx = ((size_t)S * c + PK_DIAG_ATTENTION_GUARD_ROWS) * d, n_cache = ((size_t)S * cache_rows + PK_DIAG_ATTENTION_GUARD_ROWS) * d;
        DevBuf q, kc, vc, p, bu, bv, out, ko, vo;
        up(q, qkv_new, (size_t)S * c * 3 * d * 4);
        up(kc, kcache, (size_t)S * cache_rows * d * 4);
        up(vc, vcache, (size_t)S * cache_rows * d * 4);
        up(p, pos, (size_t)P * d * 4);
        up(bu, bias_u, (size_t)d * 4);
        up(bv, bias_v, (size_t)d * 4);
        filled(out, (int64_t)n_ctx);
        filled(ko, (int64_t)n_cache);
        filled(vo, (int64_t)n_cache);
        launch_stream_attention(q.as<float>(), kc.as<float>(), vc.as<float>(), cache_rows, S, c, nc, d, n_heads, p.as<float>(), P, bu.as<float>(),
                                bv.as<float>(), att_left, att_right, out.as<float>(), nullptr, rotate ? ko.as<float>() : nullptr,
                                rotate ? vo.as<float>() : nullptr, keep_max, ctx_sigma ? 1 : 0);
        PK_CHECK_LAUNCH();
        down(ctx, out, n_ctx * 4);
        if (cache_k_out) down(cache_k_out, ko, n_cache * 4);
        if (cache_v_out) down(cache_v_out, vo, n_cache * 4);
        static_assert(STREAM_ATT_GENERAL_1W == PK_DIAG_STREAM_ATT_GENERAL_1W && STREAM_ATT_GENERAL_2W == PK_DIAG_STREAM_ATT_GENERAL_2W &&
                      STREAM_ATT_TILES_HD64 == PK_DIAG_STREAM_ATT_TILES_HD64 && STREAM_ATT_TILES_HD128 == PK_DIAG_STREAM_ATT_TILES_HD128, "form values");
        if (form) *form = (int)stream_attention_form(nc + c, c, d / n_heads);
    });
}

// The mel front end alone (kernels/mel.hip), launched as Model::run_mel / run_mel_ws, MelFrontend::features and StreamBatch::mel launch it: the tables
// from the builder they share, a ragged batch described by the engine's RagBatch.  Both device buffers are filled before the launch and come back whole.
pk_status pk_diag_mel(int n_mels, int normalize, int stft_window_centered, int power_via_abs, int form, const float *pcm, int n_clips, int64_t n_samples,
                      const int64_t *offsets, float *logmel, int64_t logmel_words, float *feats, int64_t feats_words, int32_t *n_frames, int32_t *grid) {
    return guard([&] {
        need(form >= PK_DIAG_MEL_UNIFORM && form <= PK_DIAG_MEL_STREAM, "form");
        need(pcm && logmel && feats && n_frames && grid && n_clips > 0, "pcm/logmel/feats/n_frames/grid/n_clips");
        // (n_mels <= 512 is this entry's own limit: the offline kernel parks a frame's n_mels values in the head of its 576-word LDS array.  The engine's
        //  entry points take 80 / 128 bins, pk_frontend up to 128.)
        need(n_mels >= 1 && n_mels <= 512, "n_mels (1 .. 512)");
        const bool ragged = form == PK_DIAG_MEL_RAGGED, stream = form == PK_DIAG_MEL_STREAM;
        need(ragged == (offsets != nullptr), "offsets: with the ragged form, and only there");
        std::vector<int64_t> lens(n_clips);
        std::vector<int32_t> nf(n_clips);
        int64_t total = 0, sum_nf = 0, sum_pitch = 0;
        for (int b = 0; b < n_clips; ++b) {
            lens[b] = ragged ? offsets[b + 1] - offsets[b] : n_samples;
            if (stream) need(lens[b] >= 400, "streaming: at least 400 samples (one window)");
            else need(lens[b] > 256, "every clip needs more than 256 samples (n_fft / 2: reflect padding)");
            need(lens[b] <= ((int64_t)1 << 24), "at most 2^24 samples per clip");
            nf[b] = stream ? (int32_t)((lens[b] - 400) / 160 + 1) : (int32_t)(1 + lens[b] / 160);
            total += lens[b]; sum_nf += nf[b]; sum_pitch += mel_logmel_pitch(nf[b]);
        }
        // refuses a filterbank over kMelMaxTaps here, where nothing is allocated yet.  (No n_mels reaches that today: every FFT bin lies under at most two
        //  triangles, 514 packed taps at the most against 768.  The check guards the builder against a change of the filterbank, not an input.)
        const MelTablesHost th = make_mel_tables_host(n_mels, stft_window_centered != 0);
        // what the launches write: offline [clip][n_mels][pitch] then [frames of the batch][n_mels]; streaming [clip][frames][n_mels] and no features
        const int64_t n_lm = stream ? sum_nf * n_mels : sum_pitch * n_mels, n_ft = stream ? 0 : sum_nf * n_mels;
        need(logmel_words >= n_lm + PK_DIAG_MEL_SPARE_WORDS && feats_words >= n_ft + PK_DIAG_MEL_SPARE_WORDS, "logmel_words / feats_words: the device buffer and 64 spare words");
        need_device();
        std::vector<std::unique_ptr<DevBuf>> owned;
        MelTables tb = upload_mel_tables(th, [&](const float *h, size_t cnt) {
            owned.push_back(std::make_unique<DevBuf>());
            up(*owned.back(), h, (cnt ? cnt : 1) * 4);
            return owned.back()->as<float>();
        });
        tb.power_via_abs = power_via_abs ? 1 : 0;
        DevBuf x, lm, ft, img;
        x.reserve((size_t)total * 4);
        int64_t at = 0;
        for (int b = 0; b < n_clips; at += lens[b], ++b)            // (the clips of a ragged batch need not be contiguous in the caller's buffer)
            PK_HIP(hipMemcpy(x.as<float>() + at, pcm + (ragged ? offsets[b] : (int64_t)b * n_samples), (size_t)lens[b] * 4, hipMemcpyHostToDevice));
        filled(lm, logmel_words);
        filled(ft, feats_words);
        MelRag rag;
        RagBatch r;
        if (ragged) {                                               // the views Workspace::set_ragged forms
            r.build_from_samples(lens.data(), n_clips, 32);
            up(img, r.image.data(), r.image.size() * 4);
            const int32_t *dv = img.as<int32_t>();
            rag.pcm_off = reinterpret_cast<const int64_t *>(dv + r.o_pcm_off); rag.Tm = dv + r.o_Tm; rag.Tm_off = dv + r.o_Tm_off; rag.max_frames = r.Tm_max;
            rag.Tm_pad_off = dv + r.o_Tm_pad_off;
        }
        MelGrid g1{0, 0, 0}, g2{0, 0, 0};
        if (stream) {
            g1 = launch_mel_stream(x.as<float>(), n_clips, n_samples, nf[0], tb, lm.as<float>(), nullptr);
        } else {
            g1 = launch_mel_logmel(x.as<float>(), n_clips, ragged ? 0 : n_samples, ragged ? 0 : nf[0], tb, lm.as<float>(), nullptr, rag);
            g2 = launch_mel_normalize(lm.as<float>(), n_clips, n_mels, ragged ? 0 : nf[0], normalize ? 1 : 0, ft.as<float>(), nullptr, rag);
        }
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(logmel, lm, (size_t)logmel_words * 4);
        down(feats, ft, (size_t)feats_words * 4);
        memcpy(n_frames, nf.data(), (size_t)n_clips * 4);
        const int32_t gw[6] = {g1.x, g1.y, g1.threads, g2.x, g2.y, g2.threads};
        memcpy(grid, gw, sizeof gw);
    });
}

pk_status pk_diag_mem_info(pk_model *h, uint64_t out[3]) {
    return guard([&] {
        need(out != nullptr, "out");
        need_device();
        size_t fr = 0, tot = 0;
        PK_HIP(hipMemGetInfo(&fr, &tot));
        out[0] = fr; out[1] = tot; out[2] = 0;
        if (h) {
            const Model &m = *h->m;
            const Workspace &w = m.ws;
            size_t n = tdt_align_bytes(m.talign) + tdt_total_bytes(m.ttotal) + tdt_beam_bytes(m.tbeam) + kws_bytes(m.kws) + tdt_kws_bytes(m.tkws) + vad_bytes(m.vad);
            for (const DevBuf *b : {&w.pcm, &w.logmel, &w.feats, &w.a2, &w.a3, &w.a4, &w.a5, &w.flat, &w.x, &w.n, &w.hbuf, &w.qkv, &w.ctx, &w.g, &w.dwb, &w.ctc_logits,
                                    &w.ctc_lp, &w.best_idx, &w.best_lp, &w.ep, &w.gh, &w.gi, &w.pp, &w.z, &w.logits, &w.h, &w.c, &w.hn, &w.cn, &w.ints, &w.ids, &w.start,
                                    &w.end, &w.conf, &w.lens, &w.margin, &w.persist_bar, &w.trie_act, &w.ragdev, &m.io_in, &m.io_out, &m.io_tmp})
                n += b->cap;
            out[2] = n;
        }
    });
}

}  // extern "C"
