// parakeet.cpp_amd/csrc/capi_lm.cpp -- the n-gram language model at the C boundary: pk_lm_load(_buffer), pk_lm_free, pk_lm_score, and the device
// copies the fused CTC and TDT beam searches read (one per device, made on first use).
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>

#include "capi_util.hpp"
#include "ngram_lm.hpp"

using namespace pk;

namespace {
struct LmDevCopy { DevBuf state, arc_tok, arc, uni; };
}  // namespace

struct pk_lm {
    NgramLm lm;
    mutable std::mutex mu;
    mutable std::map<int, std::unique_ptr<LmDevCopy>> dev;      // by device id
};

static_assert(sizeof(LmState) == 16 && sizeof(LmArc) == 8, "the device reads LmState as int4 and LmArc as int2");

void pk::lm_fusion_checks(const pk_lm *lm, const pk_lm_options *opt, int V, int blank) {
    need(lm != nullptr, "lm");
    if (opt && !(std::isfinite(opt->alpha) && std::isfinite(opt->beta))) fail(PK_ERR_INVALID, "lm alpha and beta must be finite");
    lm_check_vocab(lm->lm, V, blank);
}

LmDev pk::lm_device_view(const pk_lm *lm, const pk_lm_options *opt) {
    int device = 0;
    PK_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(lm->mu);
    auto &slot = lm->dev[device];
    const NgramLm &m = lm->lm;
    if (!slot) {
        auto c = std::make_unique<LmDevCopy>();
        auto up = [](DevBuf &d, const void *src, size_t bytes) {
            d.reserve(bytes ? bytes : 16);                              // (an order-1 model has no arcs: the pointers stay valid all the same)
            if (bytes) PK_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        };
        up(c->state, m.state.data(), m.state.size() * sizeof(LmState));
        up(c->arc_tok, m.arc_tok.data(), m.arc_tok.size() * sizeof(int32_t));
        up(c->arc, m.arc.data(), m.arc.size() * sizeof(LmArc));
        up(c->uni, m.uni.data(), m.uni.size() * sizeof(LmArc));
        slot = std::move(c);
    }
    pk_lm_options o;
    pk_lm_options_default(&o);
    if (opt) o = *opt;
    LmDev d{};
    d.state = slot->state.as<int4>(); d.arc_tok = slot->arc_tok.as<int>(); d.arc = slot->arc.as<int2>(); d.uni = slot->uni.as<int2>();
    d.U = m.U(); d.unk_lp = m.unk_lp; d.start = m.start;
    d.alpha = o.alpha; d.beta = o.beta;
    return d;
}

int pk::lm_num_states(const pk_lm *lm) { return (int)lm->lm.state.size(); }

void pk_lm_options_default(pk_lm_options *out) {
    if (!out) return;
    out->alpha = 0.5f; out->beta = 0.0f;
}

pk_status pk_lm_load_buffer(const char *text, size_t n_bytes, pk_lm **out) {
    return guard([&] {
        need(text && out, "text/out");
        auto h = std::make_unique<pk_lm>();
        lm_parse_arpa(text, n_bytes, h->lm);
        *out = h.release();
    });
}

pk_status pk_lm_load(const char *path, pk_lm **out) {
    return guard([&] {
        need(path && out, "path/out");
        struct File { FILE *f; ~File() { if (f) std::fclose(f); } } file{std::fopen(path, "rb")};
        if (!file.f) fail(PK_ERR_IO, "Cannot open language model file: %s", path);
        std::vector<char> text;
        char buf[1 << 16];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, file.f)) > 0;) text.insert(text.end(), buf, buf + n);
        if (std::ferror(file.f)) fail(PK_ERR_IO, "Cannot read language model file: %s", path);
        text.push_back(0);                                              // (keeps data() valid for an empty file; not part of the text)
        auto h = std::make_unique<pk_lm>();
        lm_parse_arpa(text.data(), text.size() - 1, h->lm);
        *out = h.release();
    });
}

void pk_lm_free(pk_lm *lm) {
    if (!lm) return;
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto &kv : lm->dev) {                                          // every copy is freed on the device it lives on
        if (have) (void)hipSetDevice(kv.first);
        kv.second.reset();
    }
    if (have && !lm->dev.empty()) (void)hipSetDevice(cur);
    delete lm;
}

int pk_lm_order(const pk_lm *lm) { return lm ? lm->lm.order : 0; }
int64_t pk_lm_num_ngrams(const pk_lm *lm) { return lm ? lm->lm.num_ngrams() : 0; }

pk_status pk_lm_score(const pk_lm *lm, const int32_t *ids, const int32_t *id_offsets, int n_strings, int bos, int eos, float *logp) {
    return guard([&] {
        need(lm && id_offsets && logp && n_strings >= 0, "lm/id_offsets/logp/n_strings");
        for (int i = 0; i < n_strings; ++i) {
            need(id_offsets[i] >= 0 && id_offsets[i + 1] >= id_offsets[i], "id_offsets must not decrease");
            need(ids || id_offsets[i + 1] == id_offsets[i], "ids");
        }
        for (int i = 0; i < n_strings; ++i)
            logp[i] = lm_score_string(lm->lm, ids ? ids + id_offsets[i] : nullptr, id_offsets[i + 1] - id_offsets[i], bos != 0, eos != 0);
    });
}
