// parakeet.cpp_amd/csrc/neural_lm.hpp -- a causal Transformer LM over token ids for n-best rescoring (the rule is
// restated in include/parakeet_amd.h): embeddings -> TransformerEncoder under the causal attention form -> the fused head.  See neural_lm.cpp.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "transformer.hpp"

namespace pk {

constexpr int kNlmMaxPositions = 512;                     // the causal attention keeps a [32][positions] score block in LDS
constexpr size_t kNlmScratchCap = (size_t)1 << 30;        // a call past it is cut into groups of whole strings

// what pk_nlm_config_infer reads off the tensor shapes (host only)
void nlm_config_infer(const std::string &path, const std::string &prefix, pk_nlm_config &io);
// The ordering rule of pk_nbest_rescore_nlm for one list (tests/nlm_ref.py nlm_order): slots 0 .. N-1 in the incoming order -> order[N], combined[N] by slot
void nlm_order(const float *am, const float *nlm, const int32_t *lens, const int32_t *ok, int N, float alpha, float beta, int32_t *order, float *combined);

class NeuralLm {
  public:
    NeuralLm(const std::string &weights_path, const std::string &prefix, const pk_nlm_config &c, int device);
    ~NeuralLm();
    // PK_ERR_INVALID for malformed offsets or an id the model refuses; nothing is allocated before that
    void check_ids(const int32_t *ids, const int32_t *id_off, int n) const;
    // total / ok [n]; token_logp optional (layout: the header's); ms optional [3]: stage times of this pass summed over its groups
    void score(const int32_t *ids, const int32_t *id_off, int n, float *total, int32_t *ok, float *token_logp, float *ms = nullptr);
    pk_nlm_config cfg;
    size_t scratch_cap = kNlmScratchCap;
    int last_groups = 0;

  private:
    std::unique_ptr<TransformerEncoder> enc_;
    std::vector<std::unique_ptr<DevBuf>> weights_;          // owned from the moment they exist: a constructor that throws frees them
    const float *tok_ = nullptr, *pos_ = nullptr, *eg_ = nullptr, *eb_ = nullptr, *hw_ = nullptr, *hb_ = nullptr;
    DevBuf x_, meta_, lp_;
    std::vector<int32_t> img_;
    std::vector<float> hlp_;
    const float *upload(const float *h, size_t n);
    size_t bytes_per_row() const;
    void run_group(const int32_t *ids, const int32_t *id_off, const int *strs, int ng, int64_t rows, float *ms);
};

}  // namespace pk

struct pk_nlm {
    std::unique_ptr<pk::NeuralLm> lm;
};
