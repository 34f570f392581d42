// parakeet.cpp_amd/csrc/capi_diag_gemm.cpp -- the product diagnostics of the C boundary: the GEMM launchers (fp32 and bf16, tile and small-M
// families, with the LayerNorm and depthwise-conv folds) and the operand copies they read, run alone on operands the caller hands over.  Every
// call stages its operands afresh, through the helpers of capi_diag_util.hpp.
#include <atomic>

#include "capi_diag_util.hpp"

using namespace pk;
using namespace pk::diag;

extern "C" {

// The bf16 diag products run as a streaming session runs them: weights also as operand tiles of the small-M kernel (GemmArgs::W_t16) where the
// shape allows (rows % 16 == 0, K % 32 == 0).  pk_diag_smallm_bf16_tiles(0) keeps the natural layout only (both are tested, bit for bit).
static std::atomic<int> g_diag_tiles{1};
pk_status pk_diag_smallm_bf16_tiles(int on) { g_diag_tiles.store(on ? 1 : 0); return PK_OK; }
static const float *diag_operand_tiles(DevBuf &buf, const float *w16, int64_t rows, int K) {
    if (!g_diag_tiles.load() || rows % 16 != 0 || K % 32 != 0) return nullptr;
    buf.reserve((size_t)rows * K * 2);
    launch_tile_copy_bf16(w16, buf.as<float>(), rows, K, K, nullptr);
    return buf.as<float>();
}

// out = epi(alpha * A W^T + bias [, resid]) on one launcher -- the body of the four product diagnostics below.  bf16: W rounded to bf16, the
// bf16 launcher (a16: A handed over as bf16 too, GemmArgs::a_bf16; gamma / beta: the LayerNorm of the rows of A folded into the product).
static void diag_product(int M, int N, int K, const float *A, const float *W, const float *bias, int epi, const float *resid, float alpha, float *out,
                         bool bf16, bool a16 = false, const float *gamma = nullptr, const float *beta = nullptr, float eps = 0.0f) {
    need(epi >= 0 && epi <= 4, "epi");
    need(epi != EPI_RESID || resid, "resid");
    need_device();
    const int wrows = epi == EPI_GLU ? 2 * N : N;
    DevBuf a, w, b, r, o, gb, wt;
    if (a16) up16(a, A, (size_t)M * K);
    else up(a, A, (size_t)M * K * 4);
    if (bf16) up16(w, W, (size_t)wrows * K);
    else up(w, W, (size_t)wrows * K * 4);
    up(b, bias, (size_t)wrows * 4);
    up(r, resid, (size_t)M * N * 4);
    o.reserve((size_t)M * N * 4);
    GemmArgs g{a.as<float>(), K, w.as<float>(), K, bias ? b.as<float>() : nullptr, o.as<float>(), N,
               resid ? r.as<float>() : nullptr, N, alpha, M, N, K};
    if (a16) g.a_bf16 = 1;
    if (gamma) {
        const NormVecs v = up_norms(gb, K, gamma, beta);
        g.ln_g = v.g; g.ln_b = v.b; g.ln_eps = eps;
    }
    if (bf16) g.W_t16 = diag_operand_tiles(wt, w.as<float>(), wrows, K);
    if (gamma && !gemm_smallm_bf16_ln_applies(g, epi)) fail(PK_ERR_UNSUPPORTED, "pk_diag_ln_gemm_bf16: M <= %d, K = 256 * (1 .. 8; glu: .. 4)", kSmallMRowsBf16);
    if (bf16) launch_gemm_bf16(g, epi, nullptr);
    else launch_gemm(g, epi, nullptr);
    PK_CHECK_LAUNCH();
    down(out, o, (size_t)M * N * 4);
}

pk_status pk_diag_gemm(int M, int N, int K, const float *A, const float *W, const float *bias, int epi, const float *resid,
                       float alpha, float *out) {
    return guard([&] {
        need(A && W && out && M > 0 && N > 0 && K > 0, "A/W/out/M/N/K");
        need(K % 32 == 0, "K must be a multiple of 32");
        diag_product(M, N, K, A, W, bias, epi, resid, alpha, out, /*bf16=*/false);
    });
}

pk_status pk_diag_gemm_bf16(int M, int N, int K, const float *A, const float *W, const float *bias, int epi, const float *resid,
                            float alpha, float *out) {
    return guard([&] {
        need(A && W && out && M > 0 && N > 0 && K > 0, "A/W/out/M/N/K");
        need(K % 64 == 0, "K must be a multiple of 64");
        diag_product(M, N, K, A, W, bias, epi, resid, alpha, out, /*bf16=*/true);
    });
}

/* the same product with the activations handed over as bf16 (GemmArgs::a_bf16: what the producing kernels of the bf16 mode store) */
pk_status pk_diag_gemm_bf16_a16(int M, int N, int K, const float *A, const float *W, const float *bias, int epi, const float *resid,
                                float alpha, float *out) {
    return guard([&] {
        need(A && W && out && M > 0 && N > 0 && K > 0, "A/W/out/M/N/K");
        need(K % 64 == 0, "K must be a multiple of 64");
        diag_product(M, N, K, A, W, bias, epi, resid, alpha, out, /*bf16=*/true, /*a16=*/true);
    });
}

/* ... and with the LayerNorm of the input rows folded into the product (the streaming chunks of the tolerance-class mode) */
pk_status pk_diag_ln_gemm_bf16(int M, int N, int K, const float *A, const float *gamma, const float *beta, float eps, const float *W,
                               const float *bias, int epi, const float *resid, float alpha, float *out) {
    return guard([&] {
        need(A && gamma && beta && W && out && M > 0 && N > 0 && K > 0, "A/gamma/beta/W/out/M/N/K");
        diag_product(M, N, K, A, W, bias, epi, resid, alpha, out, /*bf16=*/true, /*a16=*/false, gamma, beta, eps);
    });
}

pk_status pk_diag_ln2_gemm_bf16(int M, int N, int K, const float *A, const float *pre_gamma, const float *pre_beta, const float *gamma, const float *beta,
                                float eps, const float *W, const float *bias, float *out, float *pre_out) {
    return guard([&] {
        need(M > 0 && N > 0 && K > 0 && A && pre_gamma && pre_beta && gamma && beta && W && out && pre_out, "arguments");
        need_device();
        DevBuf a, w, b, gb, o, po, wt_buf;
        up(a, A, (size_t)M * K * 4);
        up16(w, W, (size_t)N * K);
        if (bias) up(b, bias, (size_t)N * 4);
        const NormVecs v = up_norms(gb, K, pre_gamma, pre_beta, gamma, beta);
        o.reserve((size_t)M * N * 4);
        po.reserve((size_t)M * K * 4);
        GemmArgs g{a.as<float>(), K, w.as<float>(), K, bias ? b.as<float>() : nullptr, o.as<float>(), N, nullptr, 0, 1.0f, M, N, K};
        g.fast_act = 1;
        g.pre_g = v.g; g.pre_b = v.b; g.ln_g = v.g2; g.ln_b = v.b2; g.ln_eps = eps;
        g.pre_out = po.as<float>(); g.pre_ldo = K;
        g.W_t16 = diag_operand_tiles(wt_buf, w.as<float>(), N, K);
        if (!gemm_smallm_bf16_pre_applies(g, EPI_SILU)) fail(PK_ERR_UNSUPPORTED, "pk_diag_ln2_gemm_bf16: M <= %d, K = 256 * (1 .. 8)", kSmallMRowsBf16);
        launch_gemm_bf16(g, EPI_SILU, nullptr);
        PK_CHECK_LAUNCH();
        down(out, o, (size_t)M * N * 4);
        down(pre_out, po, (size_t)M * K * 4);
    });
}

pk_status pk_diag_glu_dwconv_bf16(int n_streams, int c, int d, const float *A, const float *gamma, const float *beta, float eps, const float *W,
                                  const float *bias, const float *cache_in, int has_cache, const float *dw_w, const float *dw_bias,
                                  const float *bn_mean, const float *bn_rstd, const float *bn_g, const float *bn_b, int fused, float *out,
                                  float *cache_out) {
    return guard([&] {
        need(n_streams > 0 && c > 0 && d > 0 && A && W && cache_in && dw_w && dw_bias && bn_mean && bn_rstd && bn_g && bn_b && out && cache_out, "arguments");
        need((gamma != nullptr) == (beta != nullptr), "gamma and beta: both or neither");
        need_device();
        const int M = n_streams * c, K = d, N = d;
        DevBuf a, w, b, gb, ci, co, par, glu, o;
        up(a, A, (size_t)M * K * 4);
        up16(w, W, (size_t)2 * N * K);
        if (bias) up(b, bias, (size_t)2 * N * 4);
        up(ci, cache_in, (size_t)n_streams * 8 * d * 4);
        co.reserve((size_t)n_streams * 8 * d * 4);
        glu.reserve((size_t)M * N * 4);
        o.reserve((size_t)M * N * 4);
        GemmArgs g{a.as<float>(), K, w.as<float>(), K, bias ? b.as<float>() : nullptr, glu.as<float>(), N, nullptr, 0, 1.0f, M, N, K};
        g.fast_act = 1;
        if (gamma) {
            const NormVecs v = up_norms(gb, K, gamma, beta);
            g.ln_g = v.g; g.ln_b = v.b; g.ln_eps = eps;
        }
        if (!(gamma ? gemm_smallm_bf16_ln_applies(g, EPI_GLU) : gemm_smallm_bf16_applies(g, EPI_GLU)))
            fail(PK_ERR_UNSUPPORTED, "pk_diag_glu_dwconv_bf16: M <= %d, d = 256 * (1 .. 4)", kSmallMRowsBf16);
        DevBuf wt_buf;
        g.W_t16 = diag_operand_tiles(wt_buf, w.as<float>(), 2 * N, K);
        DwTail tail = stage_dw_tail(par, d, dw_w, dw_bias, bn_mean, bn_rstd, bn_g, bn_b, ci.as<float>(), co.as<float>(), has_cache, c);
        if (fused) {
            if (!gemm_smallm_bf16_dw_applies(g, EPI_GLU, c, 9)) fail(PK_ERR_UNSUPPORTED, "pk_diag_glu_dwconv_bf16: the fused tail takes c = 1, 2 or 4 frames per stream");
            g.dw_tail = &tail; g.out = o.as<float>();
            launch_gemm_bf16(g, EPI_GLU, nullptr);
        } else {
            launch_gemm_bf16(g, EPI_GLU, nullptr);
            launch_stream_dwconv(glu.as<float>(), tail.cache_in, has_cache, n_streams, c, d, 9, tail.w, tail.bias, tail.bn_mean, tail.bn_rstd, tail.bn_g, tail.bn_b,
                                 o.as<float>(), tail.cache_out, nullptr, 0);
        }
        PK_CHECK_LAUNCH();
        down(out, o, (size_t)M * N * 4);
        down(cache_out, co, (size_t)n_streams * 8 * d * 4);
    });
}

pk_status pk_diag_ffn_bf16_smallm(int M, int d, int f, const float *x, const float *gamma, const float *beta, float eps, const float *W1, const float *b1,
                                  const float *W2, const float *b2, int act_tiles, float *out) {
    return guard([&] {
        need(M > 0 && d > 0 && f > 0 && x && gamma && beta && W1 && b1 && W2 && b2 && out, "arguments");
        need_device();
        DevBuf xb, gb, w1b, w2b, b1b, b2b, hb, ob;
        up(xb, x, (size_t)M * d * 4); up16(w1b, W1, (size_t)f * d); up16(w2b, W2, (size_t)d * f); up(b1b, b1, (size_t)f * 4); up(b2b, b2, (size_t)d * 4);
        const NormVecs v = up_norms(gb, d, gamma, beta);
        hb.reserve((size_t)((M + 7) / 8 * 8) * f * 2);
        up(ob, x, (size_t)M * d * 4);                                   // the residual stream: out = x + 0.5 * ffn(LN(x))
        GemmArgs g1{xb.as<float>(), d, w1b.as<float>(), d, b1b.as<float>(), hb.as<float>(), f, nullptr, 0, 1.0f, M, f, d};
        g1.ln_g = v.g; g1.ln_b = v.b; g1.ln_eps = eps; g1.out_bf16 = 1; g1.fast_act = 1; g1.out_t8 = act_tiles ? 1 : 0;
        GemmArgs g2{hb.as<float>(), f, w2b.as<float>(), f, b2b.as<float>(), ob.as<float>(), d, ob.as<float>(), d, 0.5f, M, d, f};
        g2.a_bf16 = 1; g2.a_t8 = act_tiles ? 1 : 0;
        DevBuf wt1, wt2;
        g1.W_t16 = diag_operand_tiles(wt1, w1b.as<float>(), f, d);
        g2.W_t16 = diag_operand_tiles(wt2, w2b.as<float>(), d, f);
        if (!gemm_smallm_bf16_ln_applies(g1, EPI_SILU) || !gemm_smallm_bf16_applies(g2, EPI_RESID))
            fail(PK_ERR_UNSUPPORTED, "pk_diag_ffn_bf16_smallm: M <= %d (act_tiles: M %% 8 == 0), d = 256 * (1 .. 8), f %% 256 == 0", kSmallMRowsBf16);
        launch_gemm_bf16(g1, EPI_SILU, nullptr);
        launch_gemm_bf16(g2, EPI_RESID, nullptr);
        PK_CHECK_LAUNCH();
        down(out, ob, (size_t)M * d * 4);
    });
}

pk_status pk_diag_sigma_copy(const float *src, int64_t rows, int K, int64_t ld, float *dst) {
    return guard([&] {
        need(src && dst && rows > 0 && rows % 16 == 0 && K > 0 && K % 64 == 0 && ld >= K, "src/dst, rows % 16 == 0, K % 64 == 0, ld >= K");
        need_device();
        DevBuf a, b;
        up(a, src, (size_t)rows * ld * 4);
        b.reserve((size_t)rows * K * 4);
        launch_sigma_copy(a.as<float>(), b.as<float>(), rows, K, ld, nullptr);
        PK_CHECK_LAUNCH();
        down(dst, b, (size_t)rows * K * 4);
    });
}

int pk_diag_gemm_smallm_forms(int32_t *out, int cap) { return copy_forms(kGemmSmallmForms.v, kGemmSmallmForms.n, out, cap); }

// One product of the small-M family, staged the way a streaming session / the single-clip encoder stages it (conformer_block.hpp ln_gemm, engine.cpp run_gemm).
pk_status pk_diag_gemm_smallm(pk_smallm_gemm_diag *d) {
    return guard([&] {
        need(d, "args");
        const int M = d->M, N = d->N, K = d->K, epi = d->epi;
        need(d->A && d->W && d->out && M > 0 && N > 0 && K > 0, "A/W/out/M/N/K");
        need(M <= kSmallMRows && K % 64 == 0, "the small-M family: M <= 1536, K % 64 == 0");
        need(epi >= EPI_NONE && epi <= EPI_GLU, "epi");
        need(epi != EPI_RESID || d->resid, "resid");
        need(d->lda >= K, "lda >= K");
        need(!d->w_sig || N % 16 == 0, "w_sig: N must be a multiple of 16 (launch_sigma_copy)");
        need_sigma_cols(d->sigma_cols, N);
        need((d->ln_g != nullptr) == (d->ln_b != nullptr) && (d->pre_g != nullptr) == (d->pre_b != nullptr), "gamma and beta: both or neither");
        need(!d->pre_g || (d->ln_g && d->pre_out), "pre_g comes with ln_g and pre_out");
        need(!d->ln_g || K <= 1024, "LayerNorm: K <= 1024");
        const bool dw = d->dw != 0;
        const int c = d->dw_c, S = dw && c > 0 ? M / c : 0;
        if (dw) {
            need(d->ln_g && epi == EPI_GLU && N == K && c > 0 && M % c == 0, "dw: ln_g, epi glu, N == K, M a multiple of dw_c");
            need(d->cache_in && d->cache_out && d->cache_streams >= S && d->dw_w && d->dw_bias && d->bn_mean && d->bn_rstd && d->bn_g && d->bn_b, "dw: caches / conv vectors");
            need(!d->dw_out_sigma || N % 16 == 0, "dw_out_sigma: d must be a multiple of 16");
            need(d->remap_rows == 0 && d->sigma_cols == 0, "dw: row-major activations");
        }
        need_output_fits(M, N, d->remap_rows, d->remap_gs, d->remap_rs, d->remap_cs, d->ldo, d->out_words);
        need_device();
        const int wrows = epi == EPI_GLU ? 2 * N : N;
        const bool sigA = d->a_sigma != 0, ln = d->ln_g != nullptr, fold = ln && d->fused;
        DevBuf a, w, ws, b, r, o, gb, nrm, po, ci, co, par, glu;
        // A: the rows the first launch reads.  A separate LayerNorm reads dense rows; the product reads them at the caller's pitch, in the sigma order
        // when nothing in front of it writes them so.  (The words past K of a row are the caller's, not the pattern: this entry does not pad.)
        const int64_t lda = (ln && !fold) ? K : d->lda;
        {
            std::vector<float> h((size_t)M * lda);
            for (int i = 0; i < M; ++i)
                for (int64_t k = 0; k < lda; ++k) h[(size_t)i * lda + ((sigA && !ln && k < K) ? dec_sigma((int)k) : k)] = d->A[(size_t)i * d->lda + k];
            up(a, h.data(), h.size() * 4);
        }
        up(w, d->W, (size_t)wrows * K * 4);
        if (d->w_sig) {
            ws.reserve((size_t)wrows * K * 4);
            launch_sigma_copy(w.as<float>(), ws.as<float>(), wrows, K, K, nullptr);
        }
        if (d->bias) up(b, d->bias, (size_t)wrows * 4);
        if (d->resid) up(r, d->resid, (size_t)M * N * 4);
        const NormVecs nv = ln ? up_norms(gb, K, d->ln_g, d->ln_b, d->pre_g, d->pre_b) : NormVecs{};
        filled(o, d->out_words);
        if (d->pre_g) filled(po, (int64_t)M * K);
        GemmArgs g{a.as<float>(), lda, w.as<float>(), K, d->bias ? b.as<float>() : nullptr, o.as<float>(), d->ldo,
                   d->resid ? r.as<float>() : nullptr, N, d->alpha, M, N, K};
        set_remap(g, *d);
        g.W_sig = d->w_sig ? ws.as<float>() : nullptr;
        g.a_sigma = sigA ? 1 : 0;
        DwTail tail{};
        if (dw) {
            up(ci, d->cache_in, (size_t)S * 8 * N * 4);
            filled(co, (int64_t)d->cache_streams * 8 * N);
            tail = stage_dw_tail(par, N, d->dw_w, d->dw_bias, d->bn_mean, d->bn_rstd, d->bn_g, d->bn_b, ci.as<float>(), co.as<float>(), d->dw_has_cache ? 1 : 0, c,
                                 d->dw_out_sigma ? 1 : 0);
        }
        if (fold) {                                                    // what ln_gemm launches when the norm folds: the un-normalised natural rows
            g.a_sigma = 0; g.ln_g = nv.g; g.ln_b = nv.b; g.ln_eps = d->eps;
            if (!gemm_smallm_ln_applies(g, epi))
                fail(PK_ERR_UNSUPPORTED, "pk_diag_gemm_smallm: the folded LayerNorm takes natural rows, w_sig, K = 512 / 1024, N %% 16 == 0, epi none / relu / silu / glu");
            if (d->pre_g) {
                g.pre_g = nv.g2; g.pre_b = nv.b2; g.pre_out = po.as<float>(); g.pre_ldo = K;
                if (!gemm_smallm_pre_applies(g, epi)) fail(PK_ERR_UNSUPPORTED, "pk_diag_gemm_smallm: the norm in front takes epi silu, N >= 512 and a single round of workgroups");
            }
            if (dw) {
                if (!gemm_smallm_dw_applies(g, epi, c, 9)) fail(PK_ERR_UNSUPPORTED, "pk_diag_gemm_smallm: the conv tail takes dw_c = 1, 2 or 4 and a single round of workgroups");
                g.dw_tail = &tail;
            }
        } else {
            if (g.a_sigma && !(g.W_sig && N % 16 == 0)) fail(PK_ERR_UNSUPPORTED, "pk_diag_gemm_smallm: sigma-K activations need the sigma-K weight copy (w_sig)");
            if (dw && stream_dwconv_inst(9) == STREAM_DW_N) fail(PK_ERR_UNSUPPORTED, "pk_diag_gemm_smallm: no streaming conv kernel of 9 taps");
            if (ln) {
                nrm.reserve((size_t)M * K * 4);
                const int mode = sigA ? 2 : 0;
                if (d->pre_g) launch_layernorm2(a.as<float>(), M, K, nv.g2, nv.b2, nv.g, nv.b, d->eps, po.as<float>(), nrm.as<float>(), nullptr, mode);
                else launch_layernorm(a.as<float>(), M, K, nv.g, nv.b, d->eps, nrm.as<float>(), nullptr, mode);
                g.A = nrm.as<float>();
            }
            if (dw) {
                glu.reserve((size_t)M * N * 4);
                g.out = glu.as<float>(); g.ldo = N;
            }
        }
        d->form = (int32_t)gemm_smallm_form(g, epi);
        launch_gemm(g, epi, nullptr);
        if (dw && !fold)
            launch_stream_dwconv(glu.as<float>(), tail.cache_in, tail.has_cache, S, c, N, 9, tail.w, tail.bias, tail.bn_mean, tail.bn_rstd, tail.bn_g, tail.bn_b,
                                 o.as<float>(), tail.cache_out, nullptr, tail.out_sigma);
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->out, o, (size_t)d->out_words * 4);
        if (d->pre_g) down(d->pre_out, po, (size_t)M * K * 4);
        if (dw) down(d->cache_out, co, (size_t)d->cache_streams * 8 * N * 4);
        static_assert(PK_DIAG_SMALLM_KERNEL(gemm_smallm_form_of(SMALLM_LN, EPI_GLU, 16, true, true, false)) == SMALLM_LN &&
                      PK_DIAG_SMALLM_EPI(gemm_smallm_form_of(SMALLM_LN, EPI_GLU, 16, true, true, false)) == EPI_GLU &&
                      PK_DIAG_SMALLM_RING(gemm_smallm_form_of(SMALLM_LN, EPI_GLU, 16, true, true, false)) == 16 &&
                      PK_DIAG_SMALLM_SIG(gemm_smallm_form_of(SMALLM_LN, EPI_GLU, 16, true, true, false)) == 1 &&
                      PK_DIAG_SMALLM_DW(gemm_smallm_form_of(SMALLM_LN, EPI_GLU, 16, true, true, false)) == 1 &&
                      PK_DIAG_SMALLM_PRE(gemm_smallm_form_of(SMALLM_RT2, EPI_RESID, 4, true, false, true)) == 1, "form fields");
    });
}

// the PK_DIAG_TILE_* macros of include/parakeet_amd.h decode what gemm_tile_form_of (kernels.hpp) encodes
constexpr int kTileFormProbe = gemm_tile_form_of(TILE_PIPE, 4, 2, 1, 2, 1, true, 2, EPI_GLU);
static_assert(PK_DIAG_TILE_KERNEL(kTileFormProbe) == TILE_PIPE && PK_DIAG_TILE_WGM(kTileFormProbe) == 4 && PK_DIAG_TILE_WGN(kTileFormProbe) == 2 &&
              PK_DIAG_TILE_TM(kTileFormProbe) == 1 && PK_DIAG_TILE_TN(kTileFormProbe) == 2 && PK_DIAG_TILE_NBUF(kTileFormProbe) == 1 &&
              PK_DIAG_TILE_LNA(kTileFormProbe) == 1 && PK_DIAG_TILE_SCHED(kTileFormProbe) == 2 && PK_DIAG_TILE_EPI(kTileFormProbe) == EPI_GLU &&
              PK_DIAG_TILE_KERNEL(gemm_tile_nt_form(128, 128, EPI_RESID)) == TILE_NT && PK_DIAG_TILE_TM(gemm_tile_nt_form(128, 128, EPI_RESID)) == 2,
              "PK_DIAG_TILE_* must decode gemm_tile_form_of");

int pk_diag_gemm_tile_forms(int32_t *out, int cap) { return copy_forms(kGemmTileForms.v, kGemmTileForms.n, out, cap); }

// What both tile diagnostics refuse for a product, before either looks for a device: a shape of the small-M family, what no tile kernel can do
// (gemm_tile_refusal: launch_gemm aborts on those), a LayerNorm fold outside gemm_ln_stats_applies.  ln: g comes back with placeholder norm pointers.
static void tile_product_checks(GemmArgs &g, int epi, bool ln, const char *who) {
    need(g.M > 0 && g.N > 0 && g.K > 0, "M/N/K");
    need(epi >= EPI_NONE && epi <= EPI_GLU, "epi");
    need(g.lda >= g.K && g.ldw >= g.K, "lda >= K, ldw >= K");
    if (!gemm_tile_applies(g)) fail(PK_ERR_UNSUPPORTED, "%s: M <= %d with K %% 64 == 0 runs on the small-M kernels (pk_diag_gemm_smallm)", who, kSmallMRows);
    if (const char *why = gemm_tile_refusal(g, epi)) fail(PK_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (ln) {
        static const float none[2] = {0.0f, 0.0f};                     // (never read: the form function and gemm_ln_stats_applies look at the pointers only)
        g.ln_g = g.ln_b = g.ln_stats = none;
        if (!gemm_ln_stats_applies(g, epi))
            fail(PK_ERR_UNSUPPORTED, "%s: the LayerNorm fold needs epi none / relu / silu on a wide product (M >= 1024, N >= 1024, not the long-K tile) or glu, K >= 64", who);
    }
}

pk_status pk_diag_gemm_tile_form(int M, int N, int K, int64_t lda, int64_t ldw, int epi, int ln, int32_t *form) {
    return guard([&] {
        need(form, "form");
        GemmArgs g{nullptr, lda, nullptr, ldw, nullptr, nullptr, N, nullptr, N, 1.0f, M, N, K};
        tile_product_checks(g, epi, ln != 0, "pk_diag_gemm_tile_form");
        *form = (int32_t)gemm_tile_form(g, epi);
    });
}

pk_status pk_diag_gemm_tile(pk_gemm_tile_diag *d) {
    return guard([&] {
        need(d, "args");
        const int M = d->M, N = d->N, K = d->K, epi = d->epi;
        need(d->A && d->W && d->out, "A/W/out");
        const bool ln = d->ln_g != nullptr;
        need(ln == (d->ln_b != nullptr), "gamma and beta: both or neither");
        need(!ln || K <= 1024, "LayerNorm: K <= 1024");
        GemmArgs g{nullptr, d->lda, nullptr, d->ldw, nullptr, nullptr, d->ldo, nullptr, d->ldr, d->alpha, M, N, K};
        set_remap(g, *d);
        need_sigma_cols(d->sigma_cols, N);
        need(epi != EPI_RESID || (d->resid && d->ldr >= N), "resid, ldr >= N");
        tile_product_checks(g, epi, ln, "pk_diag_gemm_tile");
        need(d->remap_rows <= 0 || d->sigma_cols == 0, "remap: no sigma_cols");
        need_output_fits(M, N, d->remap_rows, d->remap_gs, d->remap_rs, d->remap_cs, d->ldo, d->out_words);
        need_device();
        const int wrows = epi == EPI_GLU ? 2 * N : N;
        DevBuf a, w, b, r, o, gb, st, dense;
        up_padded(a, d->A, M, K, d->lda);
        up_padded(w, d->W, wrows, K, d->ldw);
        if (d->bias) up(b, d->bias, (size_t)wrows * 4);
        if (epi == EPI_RESID) up_padded(r, d->resid, M, N, d->ldr);
        filled(o, d->out_words);
        g.A = a.as<float>(); g.W = w.as<float>(); g.bias = d->bias ? b.as<float>() : nullptr; g.out = o.as<float>();
        g.resid = epi == EPI_RESID ? r.as<float>() : nullptr;
        if (ln) {                                                      // the statistics pass reads dense rows
            const float *X = a.as<float>();
            if (d->lda != K) {
                dense.reserve((size_t)M * K * 4);
                PK_HIP(hipMemcpy2D(dense.p, (size_t)K * 4, a.p, (size_t)d->lda * 4, (size_t)K * 4, (size_t)M, hipMemcpyDeviceToDevice));
                X = dense.as<float>();
            }
            const NormVecs v = up_norms(gb, K, d->ln_g, d->ln_b);
            st.reserve((size_t)M * 2 * 4);
            launch_layernorm_stats(X, M, K, d->eps, st.as<float>(), nullptr);
            g.ln_g = v.g; g.ln_b = v.b; g.ln_eps = d->eps; g.ln_stats = st.as<float>();
        }
        d->form = (int32_t)launch_gemm_tile(g, epi, nullptr);           // launch_gemm's own tile branch: the form it hands back is the one it switched on
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->out, o, (size_t)d->out_words * 4);
    });
}

// the PK_DIAG_BF16_* macros of include/parakeet_amd.h decode what gemm_bf16_form_of (kernels.hpp) encodes
constexpr int kBf16FormProbe = gemm_bf16_form_of(BF16_GLDS, 2, 4, 3, 2, true, BF16_EPI_PERSIST, EPI_GLU);
static_assert(PK_DIAG_BF16_KERNEL(kBf16FormProbe) == BF16_GLDS && PK_DIAG_BF16_WGM(kBf16FormProbe) == 2 && PK_DIAG_BF16_WGN(kBf16FormProbe) == 4 &&
              PK_DIAG_BF16_TM(kBf16FormProbe) == 3 && PK_DIAG_BF16_TN(kBf16FormProbe) == 2 && PK_DIAG_BF16_A16(kBf16FormProbe) == 1 &&
              PK_DIAG_BF16_EFO(kBf16FormProbe) == BF16_EPI_PERSIST && PK_DIAG_BF16_EPI(kBf16FormProbe) == EPI_GLU &&
              PK_DIAG_BF16_KERNEL(gemm_bf16_form_of(BF16_REG, 4, 2, 1, 2, false, BF16_EPI_LDS, EPI_RESID)) == BF16_REG,
              "PK_DIAG_BF16_* must decode gemm_bf16_form_of");

int pk_diag_gemm_bf16_tile_forms(int32_t *out, int cap) { return copy_forms(kGemmBf16Forms.v, kGemmBf16Forms.n, out, cap); }

// What both bf16 tile diagnostics check for a product before either looks for a device, and the GemmArgs (null operands replaced by a placeholder: the form
// function and the refusals look at the pointers for null only) they hand to gemm_bf16_form.
static GemmArgs bf16_tile_product(const pk_gemm_bf16_tile_diag *d, const char *who) {
    static const float some[1] = {0.0f};
    const int M = d->M, N = d->N, K = d->K, epi = d->epi;
    need(M > 0 && N > 0 && K > 0 && K % 64 == 0, "M/N/K (K a multiple of 64)");
    need(epi >= EPI_NONE && epi <= EPI_GLU, "epi");
    need(d->lda >= K && d->ldw >= K && d->ldw % 8 == 0 && d->lda % (d->a_bf16 ? 8 : 4) == 0, "lda >= K, ldw >= K; ldw % 8 == 0, lda % 8 == 0 (fp32 A: % 4)");
    need(epi != EPI_RESID || (d->resid && d->ldr >= N), "resid, ldr >= N");
    need_sigma_cols(d->sigma_cols, N);
    need(!d->a_blocked || (d->a_bf16 && d->lda % 16 == 0), "a_blocked: bf16 A, lda % 16 == 0");
    need(!d->out_blocked || (d->out_bf16 && d->ldo % 16 == 0 && d->ldo >= N), "out_blocked: bf16 rows out, ldo % 16 == 0");
    GemmArgs g{some, d->lda, some, d->ldw, d->bias ? some : nullptr, nullptr, d->ldo, epi == EPI_RESID ? some : nullptr, d->ldr, d->alpha, M, N, K};
    set_remap(g, *d);
    g.a_bf16 = d->a_bf16 ? 1 : 0; g.out_bf16 = d->out_bf16 ? 1 : 0; g.out_blocked = d->out_blocked ? 1 : 0; g.a_blocked = d->a_blocked ? 1 : 0;
    g.fast_act = d->fast_act ? 1 : 0; g.one_form = d->one_form ? 1 : 0;
    if (g.one_form && epi == EPI_GLU) fail(PK_ERR_UNSUPPORTED, "%s: one_form with glu (the 64 x 64 tile has no GLU instantiation; Model::run_gemm refuses it too)", who);
    if (gemm_smallm_bf16_applies(g, epi)) fail(PK_ERR_UNSUPPORTED, "%s: M <= %d with K %% 256 == 0 runs on the small-M bf16 kernel (pk_diag_gemm_smallm_bf16)", who, kSmallMRowsBf16);
    if (const char *why = gemm_bf16_refusal(g, epi)) fail(PK_ERR_UNSUPPORTED, "%s: %s", who, why);
    if (g.out_bf16 && (g.remap_rows != 0 || (g.ldo & 3) != 0 || (g.N & 3) != 0 || g.sigma_cols != 0 || epi == EPI_RESID || epi == EPI_GLU))
        fail(PK_ERR_UNSUPPORTED, "%s: a bf16 output needs the row-major wide epilogue (no remap, no sigma_cols, no glu, no resid, ldo and N multiples of 4)", who);
    if ((epi == EPI_GLU || epi == EPI_RESID) && g.sigma_cols != 0)
        fail(PK_ERR_UNSUPPORTED, "%s: glu or resid with sigma_cols (the wide epilogue reads the sigma columns without the GLU mapping and adds the residual by output position)", who);
    // (bf16 rows: two elements to a word)
    need(d->remap_rows <= 0 || d->sigma_cols == 0, "remap: no sigma_cols");
    need_output_fits(M, N, d->remap_rows, d->remap_gs, d->remap_rs, d->remap_cs, d->ldo, d->out_words * (g.out_bf16 ? 2 : 1), g.out_blocked != 0);
    return g;
}

pk_status pk_diag_gemm_bf16_tile_form(pk_gemm_bf16_tile_diag *d) {
    return guard([&] {
        need(d, "args");
        const GemmArgs g = bf16_tile_product(d, "pk_diag_gemm_bf16_tile_form");
        d->form = (int32_t)gemm_bf16_form(g, d->epi);
    });
}

pk_status pk_diag_gemm_bf16_tile(pk_gemm_bf16_tile_diag *d) {
    return guard([&] {
        need(d, "args");
        need(d->A && d->W && d->out, "A/W/out");
        GemmArgs g = bf16_tile_product(d, "pk_diag_gemm_bf16_tile");
        const int M = d->M, N = d->N, K = d->K, epi = d->epi;
        need_device();
        const int wrows = epi == EPI_GLU ? 2 * N : N;
        DevBuf a, w, b, r, o;
        if (g.a_bf16) up16_padded(a, d->A, M, K, d->lda, g.a_blocked ? ROWS16_BLOCKED : ROWS16_ROW_MAJOR);
        else up_padded(a, d->A, M, K, d->lda);
        up16_padded(w, d->W, wrows, K, d->ldw);
        if (d->bias) up(b, d->bias, (size_t)wrows * 4);
        if (epi == EPI_RESID) up_padded(r, d->resid, M, N, d->ldr);
        filled(o, d->out_words);
        g.A = a.as<float>(); g.W = w.as<float>(); g.bias = d->bias ? b.as<float>() : nullptr; g.out = o.as<float>();
        g.resid = epi == EPI_RESID ? r.as<float>() : nullptr;
        d->form = (int32_t)launch_gemm_bf16_tile(g, epi, nullptr);      // launch_gemm_bf16's own tile branch: the form it hands back is the one it switched on
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->out, o, (size_t)d->out_words * 4);
    });
}

// the PK_DIAG_SMALLM_BF16_* macros of include/parakeet_amd.h decode what gemm_smallm_bf16_form_of (kernels.hpp) encodes
constexpr int kSmallmBf16ProbeA = gemm_smallm_bf16_form_of(EPI_RESID, 16, 2, 16, true, false, 1, true, false, true, false, false);
constexpr int kSmallmBf16ProbeB = gemm_smallm_bf16_form_of(EPI_SILU, 8, 1, 8, false, true, 2, false, false, false, true, true);
constexpr int kSmallmBf16ProbeC = gemm_smallm_bf16_form_of(EPI_GLU, 8, 1, 16, false, false, 1, false, true, false, false, false);
static_assert(PK_DIAG_SMALLM_BF16_EPI(kSmallmBf16ProbeA) == EPI_RESID && PK_DIAG_SMALLM_BF16_STEPS(kSmallmBf16ProbeA) == 16 && PK_DIAG_SMALLM_BF16_RT(kSmallmBf16ProbeA) == 2 &&
              PK_DIAG_SMALLM_BF16_RVALID(kSmallmBf16ProbeA) == 16 && PK_DIAG_SMALLM_BF16_A16(kSmallmBf16ProbeA) == 1 && PK_DIAG_SMALLM_BF16_LN(kSmallmBf16ProbeA) == 0 &&
              PK_DIAG_SMALLM_BF16_CT(kSmallmBf16ProbeA) == 1 && PK_DIAG_SMALLM_BF16_WT(kSmallmBf16ProbeA) == 1 && PK_DIAG_SMALLM_BF16_DW(kSmallmBf16ProbeA) == 0 &&
              PK_DIAG_SMALLM_BF16_AT(kSmallmBf16ProbeA) == 1 && PK_DIAG_SMALLM_BF16_AL(kSmallmBf16ProbeA) == 0 && PK_DIAG_SMALLM_BF16_PRE(kSmallmBf16ProbeA) == 0 &&
              PK_DIAG_SMALLM_BF16_EPI(kSmallmBf16ProbeB) == EPI_SILU && PK_DIAG_SMALLM_BF16_STEPS(kSmallmBf16ProbeB) == 8 && PK_DIAG_SMALLM_BF16_RT(kSmallmBf16ProbeB) == 1 &&
              PK_DIAG_SMALLM_BF16_RVALID(kSmallmBf16ProbeB) == 8 && PK_DIAG_SMALLM_BF16_A16(kSmallmBf16ProbeB) == 0 && PK_DIAG_SMALLM_BF16_LN(kSmallmBf16ProbeB) == 1 &&
              PK_DIAG_SMALLM_BF16_CT(kSmallmBf16ProbeB) == 2 && PK_DIAG_SMALLM_BF16_WT(kSmallmBf16ProbeB) == 0 && PK_DIAG_SMALLM_BF16_AL(kSmallmBf16ProbeB) == 1 &&
              PK_DIAG_SMALLM_BF16_PRE(kSmallmBf16ProbeB) == 1 && PK_DIAG_SMALLM_BF16_DW(kSmallmBf16ProbeC) == 1 && PK_DIAG_SMALLM_BF16_EPI(kSmallmBf16ProbeC) == EPI_GLU &&
              PK_DIAG_SMALLM_BF16_AT(kSmallmBf16ProbeC) == 0,
              "PK_DIAG_SMALLM_BF16_* must decode gemm_smallm_bf16_form_of");

int pk_diag_gemm_smallm_bf16_forms(int32_t *out, int cap) { return copy_forms(kGemmSmallmBf16Forms.v, kGemmSmallmBf16Forms.n, out, cap); }

// What both small-M bf16 diagnostics check for a product before either looks for a device, and the GemmArgs (operands replaced by placeholders: the form
// function and the predicates look at the pointers for null / for each other only) they hand to gemm_smallm_bf16_form.  tail: where g.dw_tail points.
static GemmArgs smallm_bf16_product(const pk_gemm_smallm_bf16_diag *d, DwTail &tail, const char *who) {
    static const float some[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    static float sink[2];
    const int M = d->M, N = d->N, K = d->K, epi = d->epi;
    need(M > 0 && N > 0 && K > 0, "M/N/K");
    need(epi >= EPI_NONE && epi <= EPI_GLU, "epi");
    need(d->lda >= K && d->ldw >= K, "lda >= K, ldw >= K");
    need((d->ln_g != nullptr) == (d->ln_b != nullptr) && (d->pre_g != nullptr) == (d->pre_b != nullptr), "gamma and beta: both or neither");
    need(!d->pre_g || d->ln_g, "pre_g comes with ln_g");
    need(epi != EPI_RESID || d->resid_in_place || d->ldr >= N, "ldr >= N");
    need(!d->resid_in_place || (epi == EPI_RESID && d->ldr == d->ldo && !d->out_bf16), "resid_in_place: epi resid, ldr == ldo, fp32 rows");
    const bool dw = d->dw != 0;
    const int c = d->dw_c;
    if (dw) need(c > 0 && d->cache_streams >= (M + c - 1) / c, "dw: dw_c > 0, cache_streams >= ceil(M / dw_c)");
    GemmArgs g{some, d->lda, some + 1, d->ldw, d->bias ? some : nullptr, sink, d->ldo, epi == EPI_RESID ? (d->resid_in_place ? sink : some) : nullptr,
               d->resid_in_place ? d->ldo : d->ldr, d->alpha, M, N, K};
    g.a_bf16 = d->a_bf16 ? 1 : 0; g.out_bf16 = d->out_bf16 ? 1 : 0; g.out_t8 = d->out_t8 ? 1 : 0; g.a_t8 = d->a_t8 ? 1 : 0; g.fast_act = d->fast_act ? 1 : 0;
    g.one_form = d->one_form ? 1 : 0;
    const int wrows = epi == EPI_GLU ? 2 * N : N;
    if (d->w_tiles && wrows % 16 == 0) g.W_t16 = some + 2;          // (the launcher takes it for N % 16 == 0)
    if (d->ln_g) { g.ln_g = some; g.ln_b = some; g.ln_eps = d->eps; }
    if (d->pre_g) { g.pre_g = some; g.pre_b = some; g.pre_out = d->pre_out ? sink + 1 : nullptr; g.pre_ldo = d->pre_ldo; }
    if (!gemm_smallm_bf16_applies(g, epi))
        fail(PK_ERR_UNSUPPORTED, "%s: gemm_smallm_bf16_applies refuses: M <= %d, K %% 256 == 0, no one_form, ldw %% 8 == 0, lda %% 8 == 0 (fp32 A: %% 4); bf16 rows out not for resid / glu; "
             "out_t8: bf16 rows out, M %% 8 == 0, N %% 32 == 0, ldo == N; a_t8: bf16 A, M %% 8 == 0, lda == K, epi resid", who, kSmallMRowsBf16);
    if (d->ln_g && !gemm_smallm_bf16_ln_applies(g, epi))
        fail(PK_ERR_UNSUPPORTED, "%s: gemm_smallm_bf16_ln_applies refuses: the folded LayerNorm takes fp32 rows, K = 256 * (1 .. 8; glu: .. 4)", who);
    if (d->pre_g && !gemm_smallm_bf16_pre_applies(g, epi))
        fail(PK_ERR_UNSUPPORTED, "%s: gemm_smallm_bf16_pre_applies refuses: the norm in front takes epi silu, N >= 256, pre_ldo >= K and a multiple of 4", who);
    if (dw) {
        if (!gemm_smallm_bf16_dw_applies(g, epi, c, 9))
            fail(PK_ERR_UNSUPPORTED, "%s: gemm_smallm_bf16_dw_applies refuses: the conv tail takes epi glu, dw_c = 1, 2 or 4, M %% dw_c == 0, N %% 16 == 0, fp32 rows out", who);
        tail = DwTail{some, sink, d->dw_has_cache ? 1 : 0, c, some, some, some, some, some, some};
        g.dw_tail = &tail;
    }
    // (bf16 rows: two elements to a word; out_t8: whole tiles, ldo == N and M % 8 == 0)
    need_output_fits(M, N, 0, 0, 0, 0, d->ldo, d->out_words * (g.out_bf16 ? 2 : 1));
    if (d->pre_g && d->pre_out) need((int64_t)(M - 1) * d->pre_ldo + K <= d->pre_out_words, "pre_out_words >= (M - 1) pre_ldo + K");
    return g;
}

pk_status pk_diag_gemm_smallm_bf16_form(pk_gemm_smallm_bf16_diag *d) {
    return guard([&] {
        need(d, "args");
        DwTail tail{};
        const GemmArgs g = smallm_bf16_product(d, tail, "pk_diag_gemm_smallm_bf16_form");
        d->form = (int32_t)gemm_smallm_bf16_form(g, d->epi);
    });
}

// One product of the small-M bf16 family, launched as launch_gemm_bf16 launches it
pk_status pk_diag_gemm_smallm_bf16(pk_gemm_smallm_bf16_diag *d) {
    return guard([&] {
        need(d, "args");
        need(d->A && d->W && d->out, "A/W/out");
        need(d->epi != EPI_RESID || d->resid, "resid");
        need(!d->pre_g || d->pre_out, "pre_g comes with pre_out");
        need(!d->dw || (d->cache_in && d->cache_out && d->dw_w && d->dw_bias && d->bn_mean && d->bn_rstd && d->bn_g && d->bn_b), "dw: caches / conv vectors");
        DwTail tail{};
        GemmArgs g = smallm_bf16_product(d, tail, "pk_diag_gemm_smallm_bf16");
        const int M = d->M, N = d->N, K = d->K, epi = d->epi;
        need_device();
        const int wrows = epi == EPI_GLU ? 2 * N : N;
        DevBuf a, w, wt, b, r, o, gb, po, ci, co, par;
        if (g.a_bf16) up16_padded(a, d->A, M, K, d->lda, g.a_t8 ? ROWS16_TILES8 : ROWS16_ROW_MAJOR);
        else up_padded(a, d->A, M, K, d->lda);
        up16_padded(w, d->W, wrows, K, d->ldw);
        if (g.W_t16) {
            wt.reserve((size_t)wrows * K * 2);
            launch_tile_copy_bf16(w.as<float>(), wt.as<float>(), wrows, K, d->ldw, nullptr);
            g.W_t16 = wt.as<float>();
        }
        if (d->bias) up(b, d->bias, (size_t)wrows * 4);
        filled(o, d->out_words);
        g.A = a.as<float>(); g.W = w.as<float>(); g.bias = d->bias ? b.as<float>() : nullptr; g.out = o.as<float>();
        g.resid = nullptr;
        if (epi == EPI_RESID) {
            if (d->resid_in_place) {                                   // resid == out, as fc2 of a block runs: the rows of the residual stream inside the fill
                PK_HIP(hipMemcpy2D(o.p, (size_t)d->ldo * 4, d->resid, (size_t)d->ldr * 4, (size_t)N * 4, (size_t)M, hipMemcpyHostToDevice));
                g.resid = o.as<float>();
            } else {
                up_padded(r, d->resid, M, N, d->ldr);
                g.resid = r.as<float>();
            }
        }
        if (d->ln_g) {
            const NormVecs v = up_norms(gb, K, d->ln_g, d->ln_b, d->pre_g, d->pre_b);
            g.ln_g = v.g; g.ln_b = v.b;
            if (d->pre_g) {
                filled(po, d->pre_out_words);
                g.pre_g = v.g2; g.pre_b = v.b2; g.pre_out = po.as<float>();
            }
        }
        if (d->dw) {
            up(ci, d->cache_in, (size_t)(M / d->dw_c) * 8 * N * 4);
            filled(co, (int64_t)d->cache_streams * 8 * N);
            tail = stage_dw_tail(par, N, d->dw_w, d->dw_bias, d->bn_mean, d->bn_rstd, d->bn_g, d->bn_b, ci.as<float>(), co.as<float>(), d->dw_has_cache ? 1 : 0, d->dw_c);
        }
        d->form = (int32_t)launch_gemm_smallm_bf16(g, epi, nullptr);    // the form it hands back is the one it switched on
        PK_CHECK_LAUNCH();
        PK_HIP(hipDeviceSynchronize());
        down(d->out, o, (size_t)d->out_words * 4);
        if (d->pre_g) down(d->pre_out, po, (size_t)d->pre_out_words * 4);
        if (d->dw) down(d->cache_out, co, (size_t)d->cache_streams * 8 * N * 4);
    });
}

pk_status pk_diag_tile_copy_bf16(const float *src, int64_t rows, int K, int64_t ld, uint16_t *dst) {
    return guard([&] {
        need(src && dst && rows > 0 && rows % 16 == 0 && K > 0 && K % 32 == 0 && ld >= K && ld % 8 == 0, "src/dst, rows % 16 == 0, K % 32 == 0, ld >= K, ld % 8 == 0");
        need_device();
        DevBuf a, b;
        up16_padded(a, src, rows, K, ld);
        b.reserve((size_t)rows * K * 2);
        launch_tile_copy_bf16(a.as<float>(), b.as<float>(), rows, K, ld, nullptr);
        PK_CHECK_LAUNCH();
        down(dst, b, (size_t)rows * K * 2);
    });
}

pk_status pk_diag_ln_gemm(int M, int N, int K, const float *A, const float *pre_gamma, const float *pre_beta, const float *gamma, const float *beta, float eps,
                          const float *W, const float *bias, int epi, int fold, float *out, float *y1) {
    return guard([&] {
        need(A && gamma && beta && W && out && M > 0 && N > 0 && K > 0 && K <= 1024, "A/gamma/beta/W/out/M/N/K (K <= 1024)");
        need((pre_gamma == nullptr) == (pre_beta == nullptr), "pre_gamma and pre_beta: both or neither");
        need(epi == EPI_NONE || epi == EPI_RELU || epi == EPI_SILU || epi == EPI_GLU, "epi: none / relu / silu / glu");
        need_device();
        const int wrows = epi == EPI_GLU ? 2 * N : N;
        DevBuf a, w, b, gb, o, n, x1;
        up(a, A, (size_t)M * K * 4);
        up(w, W, (size_t)wrows * K * 4);
        if (bias) up(b, bias, (size_t)wrows * 4);
        const NormVecs v = up_norms(gb, K, gamma, beta, pre_gamma, pre_beta);
        o.reserve((size_t)M * N * 4);
        n.reserve((size_t)M * K * 4);
        x1.reserve((size_t)M * K * 4);
        const float *X = a.as<float>();
        GemmArgs g{n.as<float>(), K, w.as<float>(), K, bias ? b.as<float>() : nullptr, o.as<float>(), N, nullptr, 0, 1.0f, M, N, K};
        if (fold) {
            if (pre_gamma) { launch_layernorm_then_stats(X, M, K, v.g2, v.b2, eps, x1.as<float>(), n.as<float>(), nullptr); X = x1.as<float>(); }
            else launch_layernorm_stats(X, M, K, eps, n.as<float>(), nullptr);
            g.A = X; g.ln_g = v.g; g.ln_b = v.b; g.ln_eps = eps; g.ln_stats = n.as<float>();
            if (!gemm_ln_stats_applies(g, epi)) fail(PK_ERR_UNSUPPORTED, "pk_diag_ln_gemm: fold = 1 needs M > %d, K %% 32 == 0 and a wide (N >= 1024) or glu product", kSmallMRows);
        } else {
            if (pre_gamma) launch_layernorm2(X, M, K, v.g2, v.b2, v.g, v.b, eps, x1.as<float>(), n.as<float>(), nullptr);
            else launch_layernorm(X, M, K, v.g, v.b, eps, n.as<float>(), nullptr);
        }
        launch_gemm(g, epi, nullptr);
        PK_CHECK_LAUNCH();
        down(out, o, (size_t)M * N * 4);
        if (y1 && pre_gamma) down(y1, x1, (size_t)M * K * 4);
    });
}

}  // extern "C"
