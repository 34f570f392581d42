// parakeet.cpp_amd/csrc/ngram_lm.hpp -- back-off n-gram language model over token ids: ARPA text in, a back-off automaton of flat arrays out
// (DESIGN.md section 5.5.6).  Host only; kernels/ctc_beam.hip reads the same arrays from device memory (LmDev of kernels/kernels.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pk {

constexpr int kLmMaxOrder = 5;
constexpr int kLmMaxId = 1 << 24;                       // token ids are 0 .. kLmMaxId - 1 (the token field of a beam candidate's key)
constexpr int kLmBos = kLmMaxId, kLmEos = kLmMaxId + 1, kLmUnk = kLmMaxId + 2;     // <s>, </s>, <unk> as symbols of the automaton

struct LmState { int32_t arc_lo, arc_n; float bo; int32_t bo_state; };             // 16 bytes: one load on the device
struct LmArc { float lp; int32_t next; };                                          // 8 bytes

// One state per context: state 0 = the empty context, then every n-gram of order < n in file order.  The arcs of a non-empty state are
// arc_tok / arc [arc_lo, arc_lo + arc_n), sorted by symbol; state 0 has the dense table uni[0 .. U) instead (an id without a unigram holds
// <unk>'s value and goes to state 0), so every lookup ends in O(1).  Every value is natural-log fp32: strtod -> * 2.302585092994046 in double
// -> rounded once.
struct NgramLm {
    int order = 0;
    std::vector<int64_t> counts;                        // n-grams per order
    std::vector<LmState> state;
    std::vector<int32_t> arc_tok;
    std::vector<LmArc> arc;
    std::vector<LmArc> uni;
    std::vector<uint8_t> has_uni, named;                // [U]: the id has a unigram / occurs anywhere in the file
    bool has_unk = false, has_bos = false, has_eos = false;
    float unk_lp = 0.0f;
    LmArc eos_uni{0.0f, 0};                             // </s> in the empty context
    int start = 0;                                      // the context <s> when the file has <s> (and order > 1), else 0

    int64_t num_ngrams() const { int64_t n = 0; for (auto c : counts) n += c; return n; }
    int U() const { return (int)uni.size(); }

    // acc = 0; while (s, c) has no arc and s != 0: acc = acc + bo[s], s = backoff[s]; -> acc + p(arc), the arc's next state.  One fp32 add per
    // level.  c: a token id >= 0 or kLmEos.  false: a miss in the empty context of a model without <unk> (lp / next untouched).
    bool lookup(int s, int c, float &lp, int &next) const;
};

// Parses ARPA text (words: decimal token ids, <s>, </s>, <unk>; orders 1..5) and compiles it.  Throws pk::Error(PK_ERR_INVALID) naming the line
// for everything DESIGN.md section 5.5.6 lists; reads with bounds and sizes nothing by the declared counts.
void lm_parse_arpa(const char *text, size_t n_bytes, NgramLm &out);

// The fp32 left-to-right sum of lookup over ids[0 .. n): from the start state with bos, else from the empty context; with eos the </s> term is
// added last.  Throws PK_ERR_INVALID for a negative id, an id >= 2^24 or a miss without <unk>.
float lm_score_string(const NgramLm &lm, const int32_t *ids, int n, bool bos, bool eos);

// What the fused search needs of a model for a vocabulary of V entries: no id >= V, the blank not named, and <unk> or a unigram for every
// non-blank id.  Throws PK_ERR_INVALID.
void lm_check_vocab(const NgramLm &lm, int V, int blank);

}  // namespace pk
