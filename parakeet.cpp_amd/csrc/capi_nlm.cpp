// parakeet.cpp_amd/csrc/capi_nlm.cpp -- the C boundary of the Transformer LM (neural_lm.cpp): pk_nlm_config_infer / load / free / score / score_timed,
// the host-only ordering diagnostic, and the two kernel diagnostics (causal attention, head).  pk_nbest_rescore_nlm lives in capi_batch.cpp, next to
// the store it re-orders.
#include <algorithm>
#include <cstring>

#include "capi_util.hpp"
#include "dec_pack.hpp"
#include "neural_lm.hpp"

using namespace pk;

extern "C" {

pk_status pk_nlm_config_infer(const char *safetensors_path, const char *prefix, pk_nlm_config *io) {
    return guard([&] {
        need(safetensors_path && io, "path/io");
        nlm_config_infer(safetensors_path, prefix ? prefix : "", *io);
    });
}

pk_status pk_nlm_load(const char *safetensors_path, const char *prefix, const pk_nlm_config *cfg, int device, pk_nlm **out) {
    return guard([&] {
        need(safetensors_path && cfg && out, "path/cfg/out");
        auto h = std::make_unique<pk_nlm>();
        h->lm = std::make_unique<NeuralLm>(safetensors_path, prefix ? prefix : "", *cfg, device);
        *out = h.release();
    });
}

void pk_nlm_free(pk_nlm *nlm) { delete nlm; }

pk_status pk_nlm_score(pk_nlm *nlm, const int32_t *ids, const int32_t *id_offsets, int n_strings, float *total, int32_t *ok, float *token_logp) {
    return guard([&] {
        need(nlm && id_offsets && total && ok && n_strings >= 0, "nlm/id_offsets/total/ok/n_strings");
        need(ids || id_offsets[n_strings] == 0, "ids");
        nlm->lm->score(ids, id_offsets, n_strings, total, ok, token_logp);
    });
}

pk_status pk_nlm_score_timed(pk_nlm *nlm, const int32_t *ids, const int32_t *id_offsets, int n_strings, int reps, float ms[3]) {
    return guard([&] {
        need(nlm && ids && id_offsets && ms && n_strings > 0 && reps > 0, "nlm/ids/id_offsets/ms/n_strings/reps");
        std::vector<float> total(n_strings), t[3];
        std::vector<int32_t> ok(n_strings);
        for (int r = 0; r <= reps; ++r) {
            float one[3];
            nlm->lm->score(ids, id_offsets, n_strings, total.data(), ok.data(), nullptr, one);
            if (r > 0) for (int k = 0; k < 3; ++k) t[k].push_back(one[k]);
        }
        for (int k = 0; k < 3; ++k) {
            std::sort(t[k].begin(), t[k].end());
            ms[k] = t[k][t[k].size() / 2];
        }
    });
}

pk_status pk_diag_nlm_order(const float *am, const float *nlm, const int32_t *lens, const int32_t *ok, int N, float alpha, float beta, int32_t *order,
                            float *combined) {
    return guard([&] {
        need(am && nlm && lens && ok && order && combined && N >= 0, "am/nlm/lens/ok/order/combined/N");
        nlm_order(am, nlm, lens, ok, N, alpha, beta, order, combined);
    });
}

pk_status pk_diag_nlm_set_scratch_cap(pk_nlm *nlm, uint64_t bytes) {
    return guard([&] {
        need(nlm != nullptr, "nlm");
        nlm->lm->scratch_cap = bytes ? (size_t)bytes : kNlmScratchCap;
    });
}

int pk_diag_nlm_groups(const pk_nlm *nlm) { return nlm ? nlm->lm->last_groups : 0; }

static void nlm_up(DevBuf &b, const void *h, size_t bytes) {
    b.reserve(bytes ? bytes : 4);
    PK_HIP(hipMemcpy(b.p, h, bytes, hipMemcpyHostToDevice));
}

pk_status pk_diag_causal_attention(int B, const int32_t *lens, int d, int n_heads, float scale, const float *qkv, float *ctx) {
    return guard([&] {
        need(lens && qkv && ctx && B > 0 && d > 0 && n_heads > 0 && d % n_heads == 0, "lens/qkv/ctx/B/d/n_heads");
        const int hd = d / n_heads;
        int T_max = 0, nu = 0;
        int64_t rows = 0;
        for (int b = 0; b < B; ++b) {
            need(lens[b] > 0 && lens[b] <= kNlmMaxPositions, "lens: 1 .. 512 positions");
            T_max = std::max(T_max, (int)lens[b]);
            rows += lens[b];
            nu += (lens[b] + 31) / 32;
        }
        if (causal_attention_lds_bytes(T_max, hd) == 0) fail(PK_ERR_UNSUPPORTED, "causal attention: hd 32, 64, 96 or 128 (got %d)", hd);
        need_device();
        std::vector<int32_t> img;                                    // [T B][T_off B+1][units 2 nu]
        img.insert(img.end(), lens, lens + B);
        int32_t off = 0;
        for (int b = 0; b <= B; ++b) { img.push_back(off); if (b < B) off += lens[b]; }
        const size_t o_u = img.size();
        for (int b = 0; b < B; ++b)
            for (int r0 = 0; r0 < lens[b]; r0 += 32) { img.push_back(b); img.push_back(r0); }
        std::vector<float> qs((size_t)rows * 3 * d);                 // q / k thirds in the sigma columns, as the qkv GEMM writes them
        for (int64_t i = 0; i < rows; ++i)
            for (int c = 0; c < 3 * d; ++c) qs[(size_t)i * 3 * d + (c < 2 * d ? dec_sigma(c) : c)] = qkv[(size_t)i * 3 * d + c];
        DevBuf dimg, q, out;
        nlm_up(dimg, img.data(), img.size() * 4);
        nlm_up(q, qs.data(), qs.size() * 4);
        const int64_t n_ctx = (rows + PK_DIAG_ATTENTION_GUARD_ROWS) * d;
        out.reserve((size_t)n_ctx * 4);
        PK_HIP(hipMemsetD32(out.p, 0x7fc5a5a5, (size_t)n_ctx));
        SeqRag rag;
        const int32_t *dv = dimg.as<int32_t>();
        rag.units = {reinterpret_cast<const RagUnit *>(dv + o_u), nu};
        rag.T = dv; rag.T_off = dv + B; rag.T_max = T_max;
        launch_causal_attention(q.as<float>(), d, n_heads, scale, out.as<float>(), nullptr, rag);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpy(ctx, out.p, (size_t)n_ctx * 4, hipMemcpyDeviceToHost));
    });
}

pk_status pk_diag_nlm_head_logp(const float *h, const float *W, const float *bias, const int32_t *targets, int64_t rows, int V, int d, float *lp) {
    return guard([&] {
        need(h && W && targets && lp && rows > 0 && V >= 1 && d > 0 && d % 32 == 0, "h/W/targets/lp/rows/V/d (d a multiple of 32)");
        for (int64_t r = 0; r < rows; ++r) need(targets[r] >= 0 && targets[r] < V, "targets in [0, V)");
        need_device();
        DevBuf dh, dw, db, dt, out;
        nlm_up(dh, h, (size_t)rows * d * 4);
        nlm_up(dw, W, (size_t)V * d * 4);
        if (bias) nlm_up(db, bias, (size_t)V * 4);
        nlm_up(dt, targets, (size_t)rows * 4);
        const size_t n = (size_t)rows + PK_DIAG_ATTENTION_GUARD_ROWS;
        out.reserve(n * 4);
        PK_HIP(hipMemsetD32(out.p, 0x7fc5a5a5, n));
        launch_nlm_head_logp(dh.as<float>(), d, dw.as<float>(), d, bias ? db.as<float>() : nullptr, dt.as<int32_t>(), rows, V, d, out.as<float>(), nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipMemcpy(lp, out.p, n * 4, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
