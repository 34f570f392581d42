// parakeet.cpp_amd/csrc/stream.cpp -- the streaming path (BASELINE configs[4]: N concurrent streams per GPU with cached
// encoder state): StreamingAudioPreprocessor::process_chunk (src/audio.cpp:195-259), StreamingFastConformerEncoder::
// forward_chunk (src/streaming_encoder.cpp:430-472) and rnnt_streaming_decode_chunk (src/eou.cpp:17-98), the three calls of
// NemotronTranscriber::transcribe_chunk / StreamingTranscriber::transcribe_chunk (src/nemotron.cpp:24-52, src/eou.cpp:113-146).
//
// One pk_stream = S streams advanced in LOCK-STEP (every push hands each stream the same number of samples, so all S share
// the chunk geometry: frames produced, leftovers, cache lengths) -- the batch dimension of every kernel.  All state lives in
// HBM (K/V caches [S][left][d] and conv caches [S][K-1][d] per layer, leftover mel frames, LSTM state, last token); the host
// keeps only the pre-emphasis carry and the < 560 overlap samples per stream.  The per-chunk work is tiny (1-3 encoder frames
// per stream): FFN / projection products run on the MFMA GEMM with M = S*c rows, the cached attention and causal conv are
// exact-chain VALU kernels (kernels/stream.hip).  Bit-identical to the oracle's Stream (tests/test_gpu_stream.py).
// The Conformer block's products, FFNs and norms are conformer_block.hpp's, shared with the offline encoder; encode_device keeps the cached
// attention and the cached depthwise conv (or its fused tail).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

#include "capi_util.hpp"
#include "conformer_block.hpp"
#include "ctc_kws.hpp"
#include "stream.hpp"

namespace pk {

StreamBatch::StreamBatch(Model &m, int n_streams, int att_left, int att_right) : S(n_streams), m_(m), left_(att_left), right_(att_right) {
    m_.require_gpu();
    if (S <= 0 || att_left < 0 || att_right < 0) fail(PK_ERR_INVALID, "n_streams / attention context");
    if (m_.cfg.rnnt_head) fail(PK_ERR_UNSUPPORTED, "streaming decode is the TDT-joint loop of src/eou.cpp (label + duration heads)");
    const int d = m_.cfg.hidden_size, F = m_.cfg.mel_bins, K = m_.cfg.conv_kernel_size;
    mel_cache_.reserve((size_t)S * 8 * F * 4);
    for (int l = 0; l < m_.cfg.num_layers; ++l) {
        layers_.push_back(std::make_unique<LayerState>());
        LayerState &L = *layers_.back();
        for (int i = 0; i < 2; ++i) {
            L.k[i].reserve((size_t)S * (left_ > 0 ? left_ : 1) * d * 4);
            L.v[i].reserve((size_t)S * (left_ > 0 ? left_ : 1) * d * 4);
            L.conv[i].reserve((size_t)S * (K - 1) * d * 4);
        }
    }
    // (the tiled weight copies are built by the first chunk whose row count takes the small-M kernels, encode_device: a session set that never
    //  qualifies, e.g. 128 streams x 2 frames in the bf16 mode, never pays for them -- round-5 advisor finding)
    dec_cap_frames_ = 64;                                           // encoder frames per chunk the decode workspace is sized for
    wd_.size_for(m_.cfg, S, 0, 8 * (dec_cap_frames_ - 1) + 1);
    reset();
}

void StreamBatch::reset() {
    m_.require_gpu();
    preemph_last_.assign(S, 0.0f);
    overlap_.assign(S, {});
    n_mel_cache_ = 0;
    frame_offset_ = 0;
    for (auto &L : layers_) { L->cur = L->ccur = 0; L->n_kv = 0; L->has_conv = 0; }
    const int Hp = m_.cfg.pred_hidden, Ln = m_.cfg.num_lstm_layers;
    PK_HIP(hipMemset(wd_.h.p, 0, (size_t)Ln * S * Hp * 4));
    PK_HIP(hipMemset(wd_.c.p, 0, (size_t)Ln * S * Hp * 4));
    std::vector<int> tok(S, m_.cfg.blank_id);                       // last_token = blank (src/eou.cpp:33-35)
    PK_HIP(hipMemcpy(wd_.ints.p, tok.data(), (size_t)S * 4, hipMemcpyHostToDevice));
    if (kws_) {                                                     // the keywords stay; the walk and the pending hits start over at frame 0
        kws_->w.clear(m_.stream);
        PK_HIP(hipStreamSynchronize(m_.stream));
    }
    if (ep_) {                                                      // the options stay; the window, the rule's state and the frame numbering start over
        ep_->clear(m_.stream);
        PK_HIP(hipStreamSynchronize(m_.stream));
    }
}

// ---- StreamingAudioPreprocessor::process_chunk --------------------------------------------------------------------------------
int StreamBatch::mel(const float *pcm, int n, float *out, int cap_frames) { return mel_impl(pcm, n, out, cap_frames, true); }

int StreamBatch::mel_impl(const float *pcm, int n, float *out, int cap_frames, bool sync) {
    m_.require_gpu();
    if (n <= 0) fail(PK_ERR_INVALID, "n_samples");
    const int F = m_.cfg.mel_bins;
    const int total = (int)overlap_[0].size() + n;
    if ((size_t)S * total > pin_pcm_floats_) {                      // (no upload of an earlier call is in flight: every entry point ends synchronised)
        if (pin_pcm_) { PK_HIP(hipHostFree(pin_pcm_)); pin_pcm_ = nullptr; pin_pcm_floats_ = 0; }
        const size_t want = (size_t)S * total + (size_t)S * 1024;
        PK_HIP(hipHostMalloc(reinterpret_cast<void **>(&pin_pcm_), want * 4, hipHostMallocDefault));
        pin_pcm_floats_ = want;
    }
    float *const buf = pin_pcm_;
    for (int s = 0; s < S; ++s) {                                   // 1. pre-emphasis with the carried sample, 2. prepend the overlap (:204-214)
        float *b = buf + (size_t)s * total;
        memcpy(b, overlap_[s].data(), overlap_[s].size() * 4);
        float last = preemph_last_[s];
        const float *src = pcm + (size_t)s * n;
        for (int i = 0; i < n; ++i) {
            const float cur = src[i];
            const float t = 0.97f * last;
            b[overlap_[s].size() + i] = cur - t;
            last = cur;
        }
        preemph_last_[s] = last;
    }
    const int n_frames = total < 400 ? 0 : (total - 400) / 160 + 1;
    if (n_frames <= 0) {                                            // :216-228 buffer everything
        for (int s = 0; s < S; ++s) overlap_[s].assign(buf + (size_t)s * total, buf + (size_t)(s + 1) * total);
        return 0;
    }
    if (out && n_frames > cap_frames) fail(PK_ERR_INVALID, "mel output holds %d frames, chunk produces %d", cap_frames, n_frames);
    const int consumed = (n_frames - 1) * 160 + 400;               // :230-231
    for (int s = 0; s < S; ++s) overlap_[s].assign(buf + (size_t)s * total + consumed, buf + (size_t)(s + 1) * total);
    pre_.reserve((size_t)S * consumed * 4);
    mel_dev_.reserve((size_t)S * n_frames * F * 4);
    hipStream_t st = m_.stream;
    PK_HIP(hipMemcpy2DAsync(pre_.p, (size_t)consumed * 4, buf, (size_t)total * 4, (size_t)consumed * 4, S, hipMemcpyHostToDevice, st));
    launch_mel_stream(pre_.as<float>(), S, consumed, n_frames, m_.mel, mel_dev_.as<float>(), st);
    PK_CHECK_LAUNCH();
    if (out) PK_HIP(hipMemcpyAsync(out, mel_dev_.p, (size_t)S * n_frames * F * 4, hipMemcpyDeviceToHost, st));
    if (sync || out) PK_HIP(hipStreamSynchronize(st));              // (a push synchronises once, when it fetches the chunk's tokens)
    return n_frames;
}

// pos_proj_ of every layer for the position table of length Tp = att_left + c (src/streaming_encoder.cpp:452-454, :214), natural columns
const float *StreamBatch::pos_table(int Tp) {
    auto it = pos_tables_.find(Tp);
    if (it != pos_tables_.end()) return it->second->as<float>();
    const int d = m_.cfg.hidden_size, P = 2 * Tp - 1;
    std::vector<float> pe((size_t)P * d);
    for (int p = 0; p < P; ++p) {                                   // sinusoidal_position_embedding (src/encoder.cpp:9-30), float math
        const float position = (float)(Tp - 1 - p);
        for (int i = 0; i < d; i += 2) {
            const float div_term = std::exp((float)i * (-std::log(10000.0f) / (float)d));
            pe[(size_t)p * d + i] = std::sin(position * div_term);
            if (i + 1 < d) pe[(size_t)p * d + i + 1] = std::cos(position * div_term);
        }
    }
    DevBuf tmp;
    tmp.reserve(pe.size() * 4);
    auto tab = std::make_unique<DevBuf>();
    tab->reserve((size_t)m_.cfg.num_layers * P * d * 4);
    hipStream_t st = m_.stream;
    PK_HIP(hipMemcpyAsync(tmp.p, pe.data(), pe.size() * 4, hipMemcpyHostToDevice, st));
    for (int l = 0; l < m_.cfg.num_layers; ++l) {
        GemmArgs g{tmp.as<float>(), d, m_.layers[l].wpos, d, nullptr, tab->as<float>() + (size_t)l * P * d, d, nullptr, 0, 1.0f, P, d, d};
        m_.run_gemm("pos_proj", g, EPI_NONE, st);
    }
    PK_HIP(hipStreamSynchronize(st));
    const float *r = tab->as<float>();
    pos_tables_[Tp] = std::move(tab);
    return r;
}

// ---- StreamingFastConformerEncoder::forward_chunk ---------------------------------------------------------------------------------
int StreamBatch::encode_device(const float *d_mel, int n_frames) {
    const pk_config &cfg = m_.cfg;
    const int F = cfg.mel_bins, d = cfg.hidden_size, K = cfg.conv_kernel_size;
    hipStream_t st = m_.stream;
    // CausalConvSubsampling::forward_cached (:348-385): prepend the leftover frames, consume a multiple of 8, keep the rest
    const int total = n_mel_cache_ + n_frames, consumable = (total / 8) * 8, leftover = total - consumable;
    // The tiled weight copies (Model::sigma_weights: +1.2 / 2.4 GB for the 600M models) are built by the first chunk whose row count takes the small-M kernels
    // -- HERE, before any carried state (mel leftovers, caches) is touched: an allocation failure leaves the streams exactly where they were.
    // (rows of this chunk = S * consumable / 8: the three stride-2 stages of a multiple of 8 frames)
    if (!sig_ && consumable > 0 && (int64_t)S * (consumable / 8) <= (cfg.gemm_bf16 ? kSmallMRowsBf16 : kSmallMRows)) sig_ = &m_.sigma_weights();
    mel_all_.reserve((size_t)S * (total > 0 ? total : 1) * F * 4);
    const size_t rowb = (size_t)F * 4;
    if (n_mel_cache_ > 0)
        PK_HIP(hipMemcpy2DAsync(mel_all_.p, (size_t)total * rowb, mel_cache_.p, 8 * rowb, (size_t)n_mel_cache_ * rowb, S, hipMemcpyDeviceToDevice, st));
    PK_HIP(hipMemcpy2DAsync((char *)mel_all_.p + (size_t)n_mel_cache_ * rowb, (size_t)total * rowb, d_mel, (size_t)n_frames * rowb,
                            (size_t)n_frames * rowb, S, hipMemcpyDeviceToDevice, st));
    if (leftover > 0)
        PK_HIP(hipMemcpy2DAsync(mel_cache_.p, 8 * rowb, (char *)mel_all_.p + (size_t)consumable * rowb, (size_t)total * rowb, (size_t)leftover * rowb, S,
                                hipMemcpyDeviceToDevice, st));
    n_mel_cache_ = leftover;
    if (consumable == 0) return 0;
    // forward() on the consumable frames: the offline conv stack on a contiguous [S][consumable][F] tensor
    enc_in_.reserve((size_t)S * consumable * F * 4);
    PK_HIP(hipMemcpy2DAsync(enc_in_.p, (size_t)consumable * rowb, mel_all_.p, (size_t)total * rowb, (size_t)consumable * rowb, S, hipMemcpyDeviceToDevice, st));
    ws_.size_for(cfg, S, 0, consumable);
    const int c = ws_.T;
    m_.run_subsample(ws_, enc_in_.as<float>(), S, consumable, ws_.x.as<float>(), st);
    const int Tp = left_ + c, P = 2 * Tp - 1;
    const float *ptab = pos_table(Tp);
    const int64_t rows = (int64_t)S * c;
    const int cache_rows = left_ > 0 ? left_ : 1;
    // How this chunk runs the block (conformer_block.hpp: BlockMode says what each field means and which encoder sets what)
    const bool have_sig = sig_ && !sig_->empty();                  // (built at the top of this function by the first chunk that qualifies)
    const int sg = (!cfg.gemm_bf16 && rows <= kSmallMRows && have_sig) ? 1 : 0;
    // (tolerance-class mode: the copies are the bf16 operand tiles of the small-M bf16 kernel, GemmArgs::W_t16 -- a weight load reads one contiguous KB)
    const bool wt = cfg.gemm_bf16 && rows <= kSmallMRowsBf16 && have_sig;
    // Tolerance-class mode (pk_config.gemm_bf16; specification: the oracle's Stream in its gemm_bf16 mode): every product of the chunk takes bf16
    // operands; attention, depthwise conv and the caches stay fp32 arithmetic on the products' fp32 outputs.
    const int a16 = cfg.gemm_bf16 ? 1 : 0;
    BlockMode mode;
    mode.bf16 = a16; mode.sigma = sg; mode.copies = (sg || wt) ? sig_ : nullptr; mode.copies_t16 = wt;
    mode.fold_bf16 = true; mode.handoff = BlockMode::TILES8;
    ConformerBlock blk{m_, mode, st, rows, ws_.x.as<float>(), ws_.n.as<float>(), ws_.hbuf.as<float>(), ws_.hbuf.cap};
    if (cfg.num_layers > 1 && blk.fc1_folds(1)) {   // the blocks' ffn1 fc1 fold their norm: the final norms in front can ride on them (BlockMode::x_other)
        x_alt_.reserve((size_t)rows * d * 4);
        mode.x_other = x_alt_.as<float>();
    }
    for (int l = 0; l < cfg.num_layers; ++l) {
        const LayerW &L = m_.layers[l];
        LayerState &Ls = *layers_[l];
        blk.ffn(l, false);                                                                             // ffn1_ (:294)
        // StreamingConformerAttention::forward_cached (:162-272): natural columns (no sigma layout here)
        blk.qkv(l, ws_.qkv.as<float>());
        const float *kc = Ls.k[Ls.cur].as<float>(), *vc = Ls.v[Ls.cur].as<float>();
        // attention of the chunk's rows + (same launch, extra blocks) the rotation of the K / V caches into the other buffer pair
        launch_stream_attention(ws_.qkv.as<float>(), kc, vc, cache_rows, S, c, Ls.n_kv, d, cfg.num_heads, ptab + (size_t)l * P * d, P, L.pos_u, L.pos_v,
                                left_, right_, ws_.ctx.as<float>(), st, Ls.k[Ls.cur ^ 1].as<float>(), Ls.v[Ls.cur ^ 1].as<float>(), left_, sg);
        Ls.cur ^= 1;
        Ls.n_kv = (Ls.n_kv + c > left_) ? left_ : Ls.n_kv + c;
        blk.att_out(l, ws_.ctx.as<float>());
        // CausalConformerConvModule::forward_cached (:41-78)
        {
            GemmArgs g = blk.pw1_args(l, ws_.g.as<float>());
            DwTail tail{Ls.conv[Ls.ccur].as<float>(), Ls.conv[Ls.ccur ^ 1].as<float>(), Ls.has_conv, c, L.dw_w, L.dw_b, L.bn_mean, L.bn_rstd, L.bn_g, L.bn_b, sg};
            // The depthwise conv + BatchNorm + SiLU of the conv module in the GLU epilogue of pw1 (kernels.hpp: DwTail) -- one launch less per block,
            // bit-identical to the separate kernel (both modes) -- where the small-M kernels can (rows stream-major, c = 1 / 2 / 4 frames per stream)
            const GemmArgs probe = blk.folded(g, L.cv_ng, L.cv_nb);                                      // what ln_gemm will launch when the norm folds
            // (tolerance-class mode: with or without the folded norm; exact mode: the tail lives in the kernel with the norm folded in)
            const bool fused_dw = a16 ? gemm_smallm_bf16_dw_applies(probe, EPI_GLU, c, K) && gemm_smallm_bf16_dw_applies(g, EPI_GLU, c, K)
                                      : sg && gemm_smallm_dw_applies(probe, EPI_GLU, c, K);
            if (fused_dw) { g.dw_tail = &tail; g.out = ws_.dwb.as<float>(); }
            blk.pw1(l, g);
            if (!fused_dw)
                launch_stream_dwconv(ws_.g.as<float>(), Ls.conv[Ls.ccur].as<float>(), Ls.has_conv, S, c, d, K, L.dw_w, L.dw_b, L.bn_mean, L.bn_rstd, L.bn_g, L.bn_b,
                                     ws_.dwb.as<float>(), Ls.conv[Ls.ccur ^ 1].as<float>(), st, sg);
        }
        Ls.ccur ^= 1;
        Ls.has_conv = 1;
        blk.pw2(l, ws_.dwb.as<float>());
        blk.ffn(l, true);                                                                              // ffn2_
        blk.end_block(l, l + 1 < cfg.num_layers);                                                      // final_norm_ (the last block's lands in ws_.x)
    }
    PK_CHECK_LAUNCH();
    return c;
}

int StreamBatch::encode(const float *mel_in, int n_frames, float *enc, int cap_frames) {
    m_.require_gpu();
    if (n_frames <= 0) fail(PK_ERR_INVALID, "n_frames");
    const int F = m_.cfg.mel_bins, d = m_.cfg.hidden_size;
    mel_dev_.reserve((size_t)S * n_frames * F * 4);
    PK_HIP(hipMemcpyAsync(mel_dev_.p, mel_in, (size_t)S * n_frames * F * 4, hipMemcpyHostToDevice, m_.stream));
    const int c = encode_device(mel_dev_.as<float>(), n_frames);
    if (c > 0) {
        if (c > cap_frames) fail(PK_ERR_INVALID, "encoder output holds %d frames, chunk produces %d", cap_frames, c);
        PK_HIP(hipMemcpyAsync(enc, ws_.x.p, (size_t)S * c * d * 4, hipMemcpyDeviceToHost, m_.stream));
    }
    PK_HIP(hipStreamSynchronize(m_.stream));
    return c;
}

int StreamBatch::encode_keep(const float *mel_in, int n_frames, const float **d_enc) {
    m_.require_gpu();
    if (n_frames <= 0) fail(PK_ERR_INVALID, "n_frames");
    const int F = m_.cfg.mel_bins;
    mel_dev_.reserve((size_t)S * n_frames * F * 4);
    PK_HIP(hipMemcpyAsync(mel_dev_.p, mel_in, (size_t)S * n_frames * F * 4, hipMemcpyHostToDevice, m_.stream));
    const int c = encode_device(mel_dev_.as<float>(), n_frames);
    *d_enc = ws_.x.as<float>();
    return c;
}

// ---- rnnt_streaming_decode_chunk -------------------------------------------------------------------------------------------------------
void StreamBatch::decode_device(const float *d_enc, int c, int max_tokens) {
    if (c > dec_cap_frames_) fail(PK_ERR_UNSUPPORTED, "chunk of %d encoder frames exceeds the stream's decode workspace (%d)", c, dec_cap_frames_);
    if (max_tokens > wd_.max_tokens) fail(PK_ERR_INVALID, "max_tokens %d > %d", max_tokens, wd_.max_tokens);
    wd_.T = c;
    m_.run_tdt(wd_, d_enc, S, c, max_tokens, m_.stream, /*keep_state=*/true);
}

StreamBatch::~StreamBatch() {
    if (pin_tok_) (void)hipHostFree(pin_tok_);
    if (pin_pcm_) (void)hipHostFree(pin_pcm_);
}
void *StreamBatch::pinned_tokens(size_t bytes) {
    if (bytes > pin_tok_bytes_) {
        if (pin_tok_) { PK_HIP(hipHostFree(pin_tok_)); pin_tok_ = nullptr; pin_tok_bytes_ = 0; }
        PK_HIP(hipHostMalloc(&pin_tok_, bytes, hipHostMallocDefault));
        pin_tok_bytes_ = bytes;
    }
    return pin_tok_;
}

// `pin`: pinned staging of S * (1 + 4 * max_tokens) words (StreamBatch::pinned_tokens).  The copies are enqueued by the decode loop's poll hook
// (Workspace::before_poll: they ride on the poll's synchronisation -- one host round trip per chunk) or, when the loop did not end on a poll, here.
static void enqueue_token_copies(Workspace &wd, int S, int max_tokens, bool start, bool end, bool conf, void *pin, hipStream_t st) {
    const size_t nt = (size_t)S * max_tokens, nb = nt * 4;
    int32_t *p_lens = static_cast<int32_t *>(pin), *p_ids = p_lens + S, *p_start = p_ids + nt, *p_end = p_start + nt;
    float *p_conf = reinterpret_cast<float *>(p_end + nt);
    PK_HIP(hipMemcpyAsync(p_lens, wd.lens.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    PK_HIP(hipMemcpyAsync(p_ids, wd.ids.p, nb, hipMemcpyDeviceToHost, st));
    if (start) PK_HIP(hipMemcpyAsync(p_start, wd.start.p, nb, hipMemcpyDeviceToHost, st));
    if (end) PK_HIP(hipMemcpyAsync(p_end, wd.end.p, nb, hipMemcpyDeviceToHost, st));
    if (conf) PK_HIP(hipMemcpyAsync(p_conf, wd.conf.p, nb, hipMemcpyDeviceToHost, st));
}
static void fetch_tokens(Model &m, Workspace &wd, int S, int max_tokens, int frame_offset, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end,
                         float *conf, void *pin) {
    hipStream_t st = m.stream;
    const size_t nt = (size_t)S * max_tokens, nb = nt * 4;
    int32_t *p_lens = static_cast<int32_t *>(pin), *p_ids = p_lens + S, *p_start = p_ids + nt, *p_end = p_start + nt;
    float *p_conf = reinterpret_cast<float *>(p_end + nt);
    if (!wd.poll_hit) {                                             // (the results are not on the host yet)
        enqueue_token_copies(wd, S, max_tokens, start != nullptr, end != nullptr, conf != nullptr, pin, st);
        PK_HIP(hipStreamSynchronize(st));
    }
    memcpy(lens, p_lens, (size_t)S * 4);
    memcpy(ids, p_ids, nb);
    if (start) memcpy(start, p_start, nb);
    if (end) memcpy(end, p_end, nb);
    if (conf) memcpy(conf, p_conf, nb);
    for (int s = 0; s < S; ++s) {
        if (lens[s] < 0) fail(PK_ERR_DECODE_CAP, "stream %d: TDT loop hit the safety cap", s);
        for (int i = 0; i < max_tokens; ++i) {
            const size_t o = (size_t)s * max_tokens + i;
            if (i < lens[s]) {                                      // frames relative to the stream (src/eou.cpp:77-79)
                if (start) start[o] += frame_offset;
                if (end) end[o] += frame_offset;
            } else {                                                // never hand stale device memory to the caller
                ids[o] = 0;
                if (start) start[o] = 0;
                if (end) end[o] = 0;
                if (conf) conf[o] = 0.0f;
            }
        }
    }
}

void StreamBatch::decode(const float *enc, int c, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    m_.require_gpu();
    if (c <= 0 || max_tokens <= 0) fail(PK_ERR_INVALID, "c / max_tokens");
    const int d = m_.cfg.hidden_size;
    enc_in_.reserve((size_t)S * c * d * 4);
    PK_HIP(hipMemcpyAsync(enc_in_.p, enc, (size_t)S * c * d * 4, hipMemcpyHostToDevice, m_.stream));
    void *pin = pinned_tokens((size_t)S * (1 + 4 * (size_t)max_tokens) * 4);
    {
        struct Hook { Workspace &w; ~Hook() { w.before_poll = nullptr; } } hook{wd_};
        wd_.poll_hit = false;
        wd_.before_poll = [&](hipStream_t st) { enqueue_token_copies(wd_, S, max_tokens, start != nullptr, end != nullptr, conf != nullptr, pin, st); };
        decode_device(enc_in_.as<float>(), c, max_tokens);
    }
    fetch_tokens(m_, wd_, S, max_tokens, frame_offset_, ids, lens, start, end, conf, pin);
    frame_offset_ += c;
}

void StreamBatch::score(const float *enc, int c, const int32_t *labels, const int32_t *dur_idx, const int32_t *n_steps, int cap, float *label_logp,
                        float *dur_logp, int32_t *n_done) {
    m_.require_gpu();
    if (c <= 0 || cap <= 0 || !enc || !labels || !dur_idx || !n_steps) fail(PK_ERR_INVALID, "enc / c / labels / dur_idx / n_steps / cap");
    if (c > dec_cap_frames_) fail(PK_ERR_UNSUPPORTED, "chunk of %d encoder frames exceeds the stream's decode workspace (%d)", c, dec_cap_frames_);
    const int d = m_.cfg.hidden_size, V = m_.cfg.vocab_size, D = m_.cfg.rnnt_head ? 0 : m_.cfg.num_durations;
    if (V <= 0 || D <= 0) fail(PK_ERR_UNSUPPORTED, "pk_stream_score needs a TDT joint (label + duration heads)");
    for (int s = 0; s < S; ++s) {
        if (n_steps[s] < 0 || n_steps[s] > cap) fail(PK_ERR_INVALID, "n_steps[%d] = %d: 0 .. cap", s, n_steps[s]);
        for (int k = 0; k < n_steps[s]; ++k) {
            const int32_t l = labels[(size_t)s * cap + k], di = dur_idx[(size_t)s * cap + k];
            if (l < 0 || l >= V || di < 0 || di >= D) fail(PK_ERR_INVALID, "stream %d step %d: label / duration index out of range", s, k);
        }
    }
    hipStream_t st = m_.stream;
    const size_t nk = (size_t)S * cap;
    enc_in_.reserve((size_t)S * c * d * 4);
    force_.reserve((2 * nk + S) * sizeof(int));
    score_.reserve(nk * (size_t)(V + D) * 4);
    int *d_lab = force_.as<int>(), *d_dur = d_lab + nk, *d_n = d_dur + nk;
    float *d_sl = score_.as<float>(), *d_sd = d_sl + nk * V;
    PK_HIP(hipMemcpyAsync(enc_in_.p, enc, (size_t)S * c * d * 4, hipMemcpyHostToDevice, st));
    PK_HIP(hipMemcpyAsync(d_lab, labels, nk * 4, hipMemcpyHostToDevice, st));
    PK_HIP(hipMemcpyAsync(d_dur, dur_idx, nk * 4, hipMemcpyHostToDevice, st));
    PK_HIP(hipMemcpyAsync(d_n, n_steps, (size_t)S * 4, hipMemcpyHostToDevice, st));
    PK_HIP(hipMemsetAsync(d_sl, 0, nk * (size_t)(V + D) * 4, st));
    struct Scope {
        Workspace &w;
        ~Scope() { w.force_label = w.force_dur = w.n_force_b = nullptr; w.score_lab = w.score_dur = nullptr; w.n_force = w.force_stride = 0; }
    } scope{wd_};
    wd_.force_label = d_lab; wd_.force_dur = d_dur; wd_.n_force_b = d_n; wd_.force_stride = cap; wd_.n_force = cap;
    wd_.score_lab = d_sl; wd_.score_dur = d_sd;
    wd_.T = c;
    m_.run_tdt(wd_, enc_in_.as<float>(), S, c, wd_.max_tokens, st, /*keep_state=*/true);
    PK_CHECK_LAUNCH();
    if (n_done) PK_HIP(hipMemcpyAsync(n_done, wd_.ints.as<int>() + 4 * S, (size_t)S * 4, hipMemcpyDeviceToHost, st));      // TdtState::steps
    if (label_logp) PK_HIP(hipMemcpyAsync(label_logp, d_sl, nk * (size_t)V * 4, hipMemcpyDeviceToHost, st));
    if (dur_logp) PK_HIP(hipMemcpyAsync(dur_logp, d_sd, nk * (size_t)D * 4, hipMemcpyDeviceToHost, st));
    PK_HIP(hipStreamSynchronize(st));
    frame_offset_ += c;
}

void StreamBatch::push(const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    push_impl(pcm, n_samples, max_tokens, ids, lens, start, end, conf, /*spot=*/false);
}

void StreamBatch::push_impl(const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf,
                            bool spot, bool endpoint) {
    // Validate BEFORE any carried state (pre-emphasis carry, overlap samples, caches) is touched: a rejected push must leave the streams
    // exactly where they were.  Bound on the encoder frames this push can produce: < 8 leftover mel frames + (559 overlap + n_samples) / 160 + 1
    // new ones, / 8, + 1 -- at most dec_cap_frames_ when n_samples <= (dec_cap_frames_ - 2) * 8 hops.
    if (max_tokens <= 0 || max_tokens > wd_.max_tokens) fail(PK_ERR_INVALID, "max_tokens %d: 1 .. %d", max_tokens, wd_.max_tokens);
    if ((int64_t)n_samples > (int64_t)(dec_cap_frames_ - 2) * 8 * 160)
        fail(PK_ERR_UNSUPPORTED, "a push of %d samples exceeds the stream's decode workspace (%d encoder frames per chunk: at most %d samples)",
             n_samples, dec_cap_frames_, (dec_cap_frames_ - 2) * 8 * 160);
    for (int s = 0; s < S; ++s) lens[s] = 0;
    const int n_frames = mel_impl(pcm, n_samples, nullptr, 0, /*sync=*/false);
    if (n_frames == 0) return;
    // (the endpointer takes the push's mel rows, whether or not the encoder has eight of them to consume: queued here, in front of the encoder and the
    //  decode loop on the same stream, so that the push's one synchronisation brings its events; a valid push feeds at most 497 frames)
    if (endpoint) ep_->run(mel_dev_.as<float>(), n_frames, /*rows=*/false, m_.stream);
    const int c = encode_device(mel_dev_.as<float>(), n_frames);
    if (c == 0) { PK_HIP(hipStreamSynchronize(m_.stream)); return; }
    void *pin = pinned_tokens((size_t)S * (1 + 4 * (size_t)max_tokens) * 4);
    // (the walk of the chunk's frames and the copy of its events are queued in front of the decode loop, on the same stream: the loop's poll waits for both)
    if (spot) kws_->enqueue(ws_.x.as<float>(), c, /*rows=*/false);
    {
        struct Hook { Workspace &w; ~Hook() { w.before_poll = nullptr; } } hook{wd_};
        wd_.poll_hit = false;
        wd_.before_poll = [&](hipStream_t st) { enqueue_token_copies(wd_, S, max_tokens, start != nullptr, end != nullptr, conf != nullptr, pin, st); };
        decode_device(ws_.x.as<float>(), c, max_tokens);
    }
    fetch_tokens(m_, wd_, S, max_tokens, frame_offset_, ids, lens, start, end, conf, pin);
    frame_offset_ += c;
}

// ---- streaming keyword spotting (stream_kws.hpp) ---------------------------------------------------------------------------------------
void StreamBatch::set_keywords(const int32_t *ids, const int32_t *kw_offsets, int n_kw, const pk_stream_kws_options *opt) {
    if (n_kw == 0) { kws_.reset(); return; }
    tdt_align_model_checks(m_);
    const pk_stream_kws_options o = stream_kws_options_of(opt);
    pk_kws_options ko;
    ko.max_hits = 1; ko.min_score = o.min_score;
    kws_check_args(ids, kw_offsets, n_kw, S, m_.cfg.vocab_size, m_.cfg.blank_id, ko, "streaming TDT keyword spotting");
    stream_kws_check_options(o);
    m_.require_gpu();
    auto next = std::make_unique<StreamKws>(m_, S, ids, kw_offsets, n_kw, o);      // (a refused set leaves the one in place as it was)
    kws_ = std::move(next);
}

void StreamBatch::spot(const float *enc, int c, float *E, int32_t *Bs, int32_t *Ee, pk_kws_event *events, int cap, int *n_events, float *ms) {
    m_.require_gpu();
    if (!kws_) fail(PK_ERR_INVALID, "invalid argument: no keywords are set on this session (pk_stream_set_keywords)");
    if (c <= 0) fail(PK_ERR_INVALID, "invalid argument: n_frames");
    if (c > kKwsChunkMaxFrames) fail(PK_ERR_UNSUPPORTED, "a chunk of %d encoder frames: at most %d can be spotted in one call", c, kKwsChunkMaxFrames);
    const int d = m_.cfg.hidden_size;
    hipStream_t st = m_.stream;
    enc_in_.reserve((size_t)S * c * d * 4);
    PK_HIP(hipMemcpyAsync(enc_in_.p, enc, (size_t)S * c * d * 4, hipMemcpyHostToDevice, st));
    hipEvent_t ev[3] = {};
    if (ms) for (auto &e : ev) PK_HIP(hipEventCreate(&e));
    kws_->enqueue(enc_in_.as<float>(), c, E || Bs || Ee, ms ? ev : nullptr);
    PK_CHECK_LAUNCH();
    PK_HIP(hipStreamSynchronize(st));
    if (ms) {
        for (int k = 0; k < 2; ++k) PK_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        for (auto &e : ev) (void)hipEventDestroy(e);
    }
    kws_->w.collect(events, cap, n_events, E, Bs, Ee);
}

void StreamBatch::push_spot(const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf,
                            pk_kws_event *events, int cap, int *n_events) {
    if (!kws_) fail(PK_ERR_INVALID, "invalid argument: no keywords are set on this session (pk_stream_set_keywords)");
    *n_events = 0;
    const int before = kws_->w.t0;
    push_impl(pcm, n_samples, max_tokens, ids, lens, start, end, conf, /*spot=*/true);
    if (kws_->w.t0 != before) kws_->w.collect(events, cap, n_events, nullptr, nullptr, nullptr);     // (a push that buffered everything walked no frame)
}

void StreamBatch::spot_flush(pk_kws_event *events, int cap, int *n_events) {
    m_.require_gpu();
    if (!kws_) fail(PK_ERR_INVALID, "invalid argument: no keywords are set on this session (pk_stream_set_keywords)");
    kws_->w.flush(events, cap, n_events, m_.stream);
}

// ---- endpointing (stream_endpoint.hpp) ----------------------------------------------------------------------------------------------------
void StreamBatch::set_endpointing(const pk_endpoint_options *opt) {
    if (!opt) { ep_.reset(); return; }
    const EndpointParams p = endpoint_params(*opt, m_.cfg.mel_bins, m_.cfg.vocab_size, m_.cfg.blank_id);
    if (m_.cfg.gemm_bf16) fail(PK_ERR_UNSUPPORTED, "endpointing is not built for the gemm_bf16 streaming mode");
    m_.require_gpu();
    auto next = std::make_unique<EndpointChunk>();                  // (a refused set leaves the options in place as they were)
    next->setup(S, m_.cfg.mel_bins, p);
    next->alloc(m_.stream);
    PK_HIP(hipStreamSynchronize(m_.stream));
    ep_ = std::move(next);
}

void StreamBatch::endpoint(const float *mel_rows, int n, float *level, float *floor, int32_t *speech0, pk_endpoint_event *events, int cap,
                           int *n_events, float *ms) {
    m_.require_gpu();
    if (!ep_) fail(PK_ERR_INVALID, "invalid argument: no endpointing options are set on this session (pk_stream_set_endpointing)");
    ep_->check_frames(n);
    hipStream_t st = m_.stream;
    const size_t bytes = (size_t)S * n * m_.cfg.mel_bins * 4;
    ep_in_.reserve(bytes);
    PK_HIP(hipMemcpyAsync(ep_in_.p, mel_rows, bytes, hipMemcpyHostToDevice, st));
    hipEvent_t ev[2] = {};
    if (ms) for (auto &e : ev) PK_HIP(hipEventCreate(&e));
    ep_->run(ep_in_.as<float>(), n, level || floor || speech0, st, ms ? ev : nullptr);
    PK_CHECK_LAUNCH();
    PK_HIP(hipStreamSynchronize(st));
    if (ms) {
        PK_HIP(hipEventElapsedTime(ms, ev[0], ev[1]));
        for (auto &e : ev) (void)hipEventDestroy(e);
    }
    std::vector<std::vector<pk_endpoint_event>> per;
    ep_->take(per);
    put_endpoint_events(per, events, cap, n_events);
    ep_->take_rows(level, floor, speech0);
}

void StreamBatch::push_endpoint(const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end,
                                float *conf, pk_endpoint_event *events, int cap, int *n_events, pk_kws_event *kws_events, int kws_cap,
                                int *kws_n_events) {
    if (!ep_) fail(PK_ERR_INVALID, "invalid argument: no endpointing options are set on this session (pk_stream_set_endpointing)");
    const bool spot = kws_n_events != nullptr;
    if (spot && !kws_) fail(PK_ERR_INVALID, "invalid argument: no keywords are set on this session (pk_stream_set_keywords)");
    *n_events = 0;
    if (spot) *kws_n_events = 0;
    const int before = ep_->t0, kws_before = spot ? kws_->w.t0 : 0;
    push_impl(pcm, n_samples, max_tokens, ids, lens, start, end, conf, spot, /*endpoint=*/true);
    if (spot && kws_->w.t0 != kws_before) kws_->w.collect(kws_events, kws_cap, kws_n_events, nullptr, nullptr, nullptr);
    if (ep_->t0 == before) return;                                  // (a push that buffered everything fed no frame)
    std::vector<std::vector<pk_endpoint_event>> per;
    ep_->take(per);
    // the token rule and the decision to close, on the host: bit 0 restarts the stream's prediction net, bit 1 closes its acoustic state
    std::vector<unsigned char> bits(S, 0);
    bool any = false;
    const EndpointParams &p = ep_->p;
    for (int s = 0; s < S; ++s) {
        bool ended = false;
        for (const pk_endpoint_event &e : per[s]) ended = ended || e.kind == PK_ENDPOINT_END;
        if (p.eou_token_id >= 0)
            for (int i = 0; i < lens[s]; ++i)
                if (ids[(size_t)s * max_tokens + i] == p.eou_token_id) {
                    const int at = ep_->t0 - 1;
                    pk_endpoint_event e;
                    e.stream = s; e.kind = PK_ENDPOINT_END; e.reason = PK_ENDPOINT_TOKEN; e.start = ep_->in_utt(s) ? ep_->utt_start(s) : at; e.end = at; e.at = at;
                    per[s].push_back(e);
                    bits[s] |= 2;
                    ended = true;
                    break;
                }
        if (ended && p.reset_decoder) bits[s] |= 1;
        any = any || bits[s];
    }
    if (any) {                                                      // (about once per utterance: the wait is not on the steady path)
        ep_->close(bits, wd_.h.as<float>(), wd_.c.as<float>(), m_.cfg.num_lstm_layers, m_.cfg.pred_hidden, wd_.ints.as<int>(), m_.cfg.blank_id, m_.stream);
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(m_.stream));
    }
    put_endpoint_events(per, events, cap, n_events);
}

void StreamBatch::reset_decoder(const uint8_t *mask) {
    m_.require_gpu();
    reset_decoder_rows(mask, S, wd_.h.as<float>(), wd_.c.as<float>(), m_.cfg.num_lstm_layers, m_.cfg.pred_hidden, wd_.ints.as<int>(), m_.cfg.blank_id,
                       dec_mask_, m_.stream);
}

}  // namespace pk

using namespace pk;

extern "C" {

pk_status pk_stream_create(pk_model *m, int n_streams, int att_context_left, int att_context_right, pk_stream **out) {
    return guard([&] {
        if (!m || !out) fail(PK_ERR_INVALID, "invalid argument: model/out");
        auto h = std::make_unique<pk_stream>();
        h->s = std::make_unique<StreamBatch>(*m->m, n_streams, att_context_left, att_context_right);
        *out = h.release();
    });
}
void pk_stream_free(pk_stream *s) { delete s; }
pk_status pk_stream_reset(pk_stream *s) {
    return guard([&] { if (!s) fail(PK_ERR_INVALID, "stream"); s->s->reset(); });
}
pk_status pk_stream_push(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                         int32_t *end, float *conf) {
    return guard([&] {
        if (!s || !pcm || !ids || !lens || n_samples <= 0 || max_tokens <= 0) fail(PK_ERR_INVALID, "invalid argument: stream/pcm/ids/lens/sizes");
        s->s->push(pcm, n_samples, max_tokens, ids, lens, start, end, conf);
    });
}
pk_status pk_stream_mel(pk_stream *s, const float *pcm, int n_samples, float *out, int cap_frames, int *n_frames) {
    return guard([&] {
        if (!s || !pcm || !out || !n_frames) fail(PK_ERR_INVALID, "invalid argument: stream/pcm/out/n_frames");
        *n_frames = s->s->mel(pcm, n_samples, out, cap_frames);
    });
}
pk_status pk_stream_encode(pk_stream *s, const float *mel, int n_frames, float *enc, int cap_frames, int *n_out) {
    return guard([&] {
        if (!s || !mel || !enc || !n_out) fail(PK_ERR_INVALID, "invalid argument: stream/mel/enc/n_out");
        *n_out = s->s->encode(mel, n_frames, enc, cap_frames);
    });
}
pk_status pk_stream_decode(pk_stream *s, const float *enc, int n_frames, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                           int32_t *end, float *conf) {
    return guard([&] {
        if (!s || !enc || !ids || !lens) fail(PK_ERR_INVALID, "invalid argument: stream/enc/ids/lens");
        s->s->decode(enc, n_frames, max_tokens, ids, lens, start, end, conf);
    });
}
pk_status pk_stream_score(pk_stream *s, const float *enc, int n_frames, const int32_t *labels, const int32_t *dur_idx, const int32_t *n_steps,
                          int cap, float *label_logp, float *dur_logp, int32_t *n_done) {
    return guard([&] {
        if (!s) fail(PK_ERR_INVALID, "stream");
        s->s->score(enc, n_frames, labels, dur_idx, n_steps, cap, label_logp, dur_logp, n_done);
    });
}

}  // extern "C"
