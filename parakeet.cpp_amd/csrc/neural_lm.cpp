// parakeet.cpp_amd/csrc/neural_lm.cpp -- the Transformer LM behind pk_nlm_* (n-best rescoring, the reference's roadmap item "Neural LM rescoring:
// N-best reranking with a Transformer LM after beam search").  The model is NeMo's TransformerLMModel shape: token +
// position embeddings, Transformer encoder blocks under a causal mask with ReLU feed-forwards, an output projection, over the acoustic model's own
// token ids plus BOS / EOS.  The strings of a call are PACKED along the row axis (no padded position is computed), like the clips of a ragged
// encoder batch: the GEMMs and LayerNorms are row-wise, the causal attention takes the per-string extents (SeqRag), the head is row-wise.
//   nlm_embed_kernel -> [emb_norm_] -> TransformerEncoder::forward_dev(causal) -> nlm_head_logp_kernel -> lp[rows] -> host sums
// The logits [rows][Vlm] are never written.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_util.hpp"
#include "neural_lm.hpp"
#include "safetensors.hpp"

namespace pk {

namespace {
const float NEG = -__builtin_huge_valf();

struct StageEvents {            // the four events around the three stages of a timed group
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    explicit StageEvents(bool on) { if (on) for (auto &e : ev) PK_HIP(hipEventCreate(&e)); }
    ~StageEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    StageEvents(const StageEvents &) = delete;
    StageEvents &operator=(const StageEvents &) = delete;
};

const HostTensor *want(const SafeTensors &st, const std::string &prefix, const std::string &name, std::initializer_list<int64_t> shape) {
    const HostTensor *t = st.find(prefix + name);
    if (!t) fail(PK_ERR_WEIGHTS, "missing tensor '%s%s'", prefix.c_str(), name.c_str());
    int64_t n = 1;
    for (int64_t s : shape) n *= s;
    bool same = t->dtype == "F32" && t->numel() == n;
    if (same && shape.size() == 2) same = t->shape.size() == 2 && t->shape[0] == *shape.begin();      // (a [a][b] tensor must not pass as [b][a])
    if (!same) fail(PK_ERR_WEIGHTS, "tensor '%s%s': expected %lld F32 elements%s", prefix.c_str(), name.c_str(), (long long)n, shape.size() == 2 ? " as a matrix of the configured shape" : "");
    return t;
}
}  // namespace

void nlm_config_infer(const std::string &path, const std::string &prefix, pk_nlm_config &io) {
    SafeTensors st(path);
    auto mat = [&](const std::string &name) {
        const HostTensor *t = st.find(prefix + name);
        if (!t) fail(PK_ERR_WEIGHTS, "missing tensor '%s%s'", prefix.c_str(), name.c_str());
        if (t->dtype != "F32" || t->shape.size() != 2) fail(PK_ERR_WEIGHTS, "tensor '%s%s': expected an F32 matrix", prefix.c_str(), name.c_str());
        return t;
    };
    const HostTensor *tok = mat("tok_emb_.weight"), *pos = mat("pos_emb_.weight");
    if (pos->shape[1] != tok->shape[1]) fail(PK_ERR_WEIGHTS, "tok_emb_.weight and pos_emb_.weight differ in width");
    int L = 0;
    while (st.find(prefix + "layers_." + std::to_string(L) + ".norm1_.weight")) ++L;
    if (L == 0) fail(PK_ERR_WEIGHTS, "missing tensor '%slayers_.0.norm1_.weight'", prefix.c_str());
    const HostTensor *fc1 = mat("layers_.0.fc1_.weight");
    io.vocab_size = (int32_t)tok->shape[0];
    io.max_positions = (int32_t)pos->shape[0];
    io.transformer.hidden_size = (int32_t)tok->shape[1];
    io.transformer.num_layers = L;
    io.transformer.ffn_intermediate = (int32_t)fc1->shape[0];
    io.transformer.has_final_norm = st.find(prefix + "final_norm_.weight") ? 1 : 0;
    io.has_emb_norm = st.find(prefix + "emb_norm_.weight") ? 1 : 0;
    io.tied_head = st.find(prefix + "lm_head_.weight") ? 0 : 1;
}

void nlm_order(const float *am, const float *nlm, const int32_t *lens, const int32_t *ok, int N, float alpha, float beta, int32_t *order, float *combined) {
    for (int j = 0; j < N; ++j) order[j] = j;
    if (alpha == 0.0f && beta == 0.0f) {                             // the identity: nothing is read but am
        for (int j = 0; j < N; ++j) combined[j] = am[j];
        return;
    }
    std::vector<int> cls(N);
    for (int j = 0; j < N; ++j) {
        const float a = alpha * nlm[j], b = beta * (float)lens[j];
        const float ab = a + b;
        const float c = am[j] + ab;
        cls[j] = (ok[j] && c == c) ? 0 : 1;                          // (NaN, from infinite parts: not scored; keeps the order strict weak)
        combined[j] = cls[j] == 0 ? c : NEG;
    }
    std::stable_sort(order, order + N, [&](int32_t x, int32_t y) {
        if (cls[x] != cls[y]) return cls[x] < cls[y];
        return cls[x] == 0 && combined[x] > combined[y];
    });
}

const float *NeuralLm::upload(const float *h, size_t n) {
    weights_.push_back(std::make_unique<DevBuf>());
    DevBuf &b = *weights_.back();
    b.reserve((n ? n : 1) * sizeof(float));
    PK_HIP(hipMemcpy(b.p, h, n * sizeof(float), hipMemcpyHostToDevice));
    return b.as<float>();
}

NeuralLm::NeuralLm(const std::string &weights_path, const std::string &prefix, const pk_nlm_config &c, int device) : cfg(c) {
    // ---- every refusal first: configuration, then the file's tensors (all of them, the encoder's too), then the device ----
    TransformerEncoder::check_config(c.transformer);
    const int d = c.transformer.hidden_size, f = c.transformer.ffn_intermediate, V = c.vocab_size, L = c.transformer.num_layers;
    if (V < 2) fail(PK_ERR_INVALID, "vocab_size must be at least 2");
    if (c.max_positions < 1) fail(PK_ERR_INVALID, "max_positions must be at least 1");
    if (c.max_positions > kNlmMaxPositions)
        fail(PK_ERR_UNSUPPORTED, "max_positions %d > %d (the causal attention keeps a string's score block in LDS)", c.max_positions, kNlmMaxPositions);
    if (c.bos_id < 0 || c.bos_id >= V) fail(PK_ERR_INVALID, "bos_id %d outside the vocabulary of %d", c.bos_id, V);
    if (c.eos_id >= V || (c.eos_id >= 0 && c.eos_id == c.bos_id)) fail(PK_ERR_INVALID, "eos_id %d: must be below %d and differ from bos_id (negative: no end term)", c.eos_id, V);
    {
        SafeTensors st(weights_path);
        want(st, prefix, "tok_emb_.weight", {V, d});
        want(st, prefix, "pos_emb_.weight", {c.max_positions, d});
        if (c.has_emb_norm) { want(st, prefix, "emb_norm_.weight", {d}); want(st, prefix, "emb_norm_.bias", {d}); }
        if (!c.tied_head) {
            want(st, prefix, "lm_head_.weight", {V, d});
            if (st.find(prefix + "lm_head_.bias")) want(st, prefix, "lm_head_.bias", {V});
        }
        for (int l = 0; l < L; ++l) {
            const std::string q = "layers_." + std::to_string(l) + ".";
            for (const char *nm : {"norm1_", "norm2_"}) { want(st, prefix, q + nm + ".weight", {d}); want(st, prefix, q + nm + ".bias", {d}); }
            for (const char *nm : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
                want(st, prefix, q + "mha_." + nm + ".weight", {(int64_t)d * d});
                want(st, prefix, q + "mha_." + nm + ".bias", {d});
            }
            want(st, prefix, q + "fc1_.weight", {(int64_t)f * d}); want(st, prefix, q + "fc1_.bias", {f});
            want(st, prefix, q + "fc2_.weight", {(int64_t)d * f}); want(st, prefix, q + "fc2_.bias", {d});
        }
        if (c.transformer.has_final_norm) { want(st, prefix, "final_norm_.weight", {d}); want(st, prefix, "final_norm_.bias", {d}); }
    }
    enc_ = std::make_unique<TransformerEncoder>(weights_path, prefix, c.transformer, device);     // (device checks, stream, the blocks' weights)
    SafeTensors st(weights_path);
    tok_ = upload(st.find(prefix + "tok_emb_.weight")->f32(), (size_t)V * d);
    pos_ = upload(st.find(prefix + "pos_emb_.weight")->f32(), (size_t)c.max_positions * d);
    if (c.has_emb_norm) { eg_ = upload(st.find(prefix + "emb_norm_.weight")->f32(), d); eb_ = upload(st.find(prefix + "emb_norm_.bias")->f32(), d); }
    hw_ = tok_;
    if (!c.tied_head) {
        hw_ = upload(st.find(prefix + "lm_head_.weight")->f32(), (size_t)V * d);
        if (const HostTensor *b = st.find(prefix + "lm_head_.bias")) hb_ = upload(b->f32(), V);
    }
}

NeuralLm::~NeuralLm() {
    if (enc_) (void)hipSetDevice(enc_->device());               // the buffers free themselves, on this device
}

void NeuralLm::check_ids(const int32_t *ids, const int32_t *id_off, int n) const {
    if (id_off[0] != 0) fail(PK_ERR_INVALID, "invalid argument: id_offsets[0] must be 0");
    for (int b = 0; b < n; ++b)
        if (id_off[b + 1] < id_off[b]) fail(PK_ERR_INVALID, "invalid argument: id_offsets must not decrease (string %d)", b);
    for (int b = 0; b < n; ++b)
        for (int q = id_off[b]; q < id_off[b + 1]; ++q) {
            const int32_t t = ids[q];
            if (t < 0 || t >= cfg.vocab_size) fail(PK_ERR_INVALID, "string %d: token id %d outside the LM vocabulary of %d", b, (int)t, cfg.vocab_size);
            if (t == cfg.bos_id) fail(PK_ERR_INVALID, "string %d: token id %d is the LM's bos_id (it is fed at position 0 only)", b, (int)t);
        }
}

size_t NeuralLm::bytes_per_row() const {
    return (size_t)cfg.transformer.hidden_size * sizeof(float) + enc_->scratch_bytes_per_row() + 3 * sizeof(int32_t) + sizeof(float);
}

// One group: the strings strs[0..ng) of the call (each with 1 <= P <= max_positions positions, `rows` in all) -> hlp_[rows], packed in that order.
void NeuralLm::run_group(const int32_t *ids, const int32_t *id_off, const int *strs, int ng, int64_t rows, float *ms) {
    const int d = cfg.transformer.hidden_size, end = cfg.eos_id >= 0 ? 1 : 0;
    hipStream_t s = enc_->stream();
    // the int32 image of the group's tables: [ids][id_off ng+1][row_off ng+1][T ng][row_str rows][units 2 nu]; the targets follow on the device
    img_.clear();
    std::vector<int32_t> goff(1, 0), roff(1, 0), T(ng);
    for (int g = 0; g < ng; ++g) {
        const int b = strs[g], nb = id_off[b + 1] - id_off[b];
        img_.insert(img_.end(), ids + id_off[b], ids + id_off[b + 1]);
        goff.push_back(goff.back() + nb);
        T[g] = nb + end;
        roff.push_back(roff.back() + T[g]);
    }
    const size_t o_ids = 0, o_goff = img_.size();
    img_.insert(img_.end(), goff.begin(), goff.end());
    const size_t o_roff = img_.size();
    img_.insert(img_.end(), roff.begin(), roff.end());
    const size_t o_T = img_.size();
    img_.insert(img_.end(), T.begin(), T.end());
    const size_t o_rs = img_.size();
    int T_max = 0, nu = 0;
    for (int g = 0; g < ng; ++g) {
        img_.insert(img_.end(), (size_t)T[g], g);
        T_max = std::max(T_max, (int)T[g]);
        nu += (T[g] + 31) / 32;
    }
    const size_t o_u = img_.size();
    for (int g = 0; g < ng; ++g)
        for (int r0 = 0; r0 < T[g]; r0 += 32) { img_.push_back(g); img_.push_back(r0); }
    const size_t o_tgt = img_.size();
    meta_.reserve((o_tgt + (size_t)rows) * 4);
    x_.reserve((size_t)rows * d * 4);
    lp_.reserve((size_t)rows * 4);
    hlp_.resize((size_t)rows);
    const int32_t *dv = meta_.as<int32_t>();
    PK_HIP(hipMemcpyAsync(meta_.p, img_.data(), o_tgt * 4, hipMemcpyHostToDevice, s));
    SeqRag rag;
    rag.units = {reinterpret_cast<const RagUnit *>(dv + o_u), nu};
    rag.T = dv + o_T; rag.T_off = dv + o_roff; rag.T_max = T_max;
    StageEvents events(ms != nullptr);
    hipEvent_t (&ev)[4] = events.ev;
    const float eps = cfg.transformer.layer_norm_eps > 0.0f ? cfg.transformer.layer_norm_eps : 1e-5f;
    float *x = x_.as<float>();
    if (ms) PK_HIP(hipEventRecord(ev[0], s));
    launch_nlm_embed(tok_, pos_, dv + o_ids, dv + o_goff, dv + o_roff, dv + o_rs, cfg.bos_id, cfg.eos_id, d, rows, x, meta_.as<int32_t>() + o_tgt, s);
    if (cfg.has_emb_norm) launch_layernorm(x, rows, d, eg_, eb_, eps, x, s);
    if (ms) PK_HIP(hipEventRecord(ev[1], s));
    enc_->forward_dev(x, ng, T_max, s, &rag, rows);
    if (ms) PK_HIP(hipEventRecord(ev[2], s));
    launch_nlm_head_logp(x, d, hw_, d, hb_, dv + o_tgt, rows, cfg.vocab_size, d, lp_.as<float>(), s);
    if (ms) PK_HIP(hipEventRecord(ev[3], s));
    PK_CHECK_LAUNCH();
    PK_HIP(hipMemcpyAsync(hlp_.data(), lp_.p, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
    if (ms)
        for (int k = 0; k < 3; ++k) {
            float t = 0.0f;
            PK_HIP(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
            ms[k] += t;
        }
}

void NeuralLm::score(const int32_t *ids, const int32_t *id_off, int n, float *total, int32_t *ok, float *token_logp, float *ms) {
    check_ids(ids, id_off, n);
    PK_HIP(hipSetDevice(enc_->device()));
    const int end = cfg.eos_id >= 0 ? 1 : 0;
    if (ms) ms[0] = ms[1] = ms[2] = 0.0f;
    if (token_logp)
        for (int64_t q = 0; q < (int64_t)id_off[n] + n; ++q) token_logp[q] = 0.0f;
    last_groups = 0;
    const size_t bpr = bytes_per_row();
    std::vector<int> grp;
    int64_t rows = 0;
    auto flush = [&] {
        if (grp.empty()) return;
        run_group(ids, id_off, grp.data(), (int)grp.size(), rows, ms);
        ++last_groups;
        int64_t r = 0;
        for (int b : grp) {
            const int P = id_off[b + 1] - id_off[b] + end;
            float t = 0.0f;
            for (int i = 0; i < P; ++i) t = t + hlp_[(size_t)(r + i)];        // left to right, fp32
            total[b] = t;
            if (token_logp) memcpy(token_logp + id_off[b] + b, hlp_.data() + r, (size_t)P * 4);
            r += P;
        }
        grp.clear();
        rows = 0;
    };
    for (int b = 0; b < n; ++b) {
        const int P = id_off[b + 1] - id_off[b] + end;
        if (P > cfg.max_positions) { ok[b] = 0; total[b] = NEG; continue; }
        ok[b] = 1;
        if (P == 0) { total[b] = 0.0f; continue; }                   // the empty string without an end term
        if (!grp.empty() && (size_t)(rows + P) * bpr > scratch_cap) flush();
        grp.push_back(b);
        rows += P;
    }
    flush();
}

}  // namespace pk
