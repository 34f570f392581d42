// parakeet.cpp_amd/csrc/tdt_beam.hpp -- host side of the TDT beam search with n-best output (kernels/tdt_beam.hip) and of its
// form with n-gram LM shallow fusion.
#pragma once
#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

class Model;

// Scratch of one call, with R = B W rows, C = (K + 1) Kd candidates per row, cap = Tmax + max_tokens steps, L / Hp / J / V / D the model's:
//   beam             2 R (36 + 4 max_tokens) bytes       (two copies: eight words per slot and its token string)
//   expansion        R (8 (K + 1) + 8 Kd + 4 C) bytes
//   back-pointers    cap R 16 bytes
//   state            (6 L R Hp + 3 R J) 4 bytes           (h, c, pred_proj: two gathered copies and the prediction-net step's output)
//   products         R (J + V + D) 4 bytes                (the heads product's input and output)
//   outputs, tables  B N (5 max_tokens + 2) 4 + (4 B + cap + 1) 4 bytes
//   fused only       2 R 8 + R 8 (K + 1) + B N 4 bytes   (per slot the LM state and score, per sorted label the same, lm_score)
// Above the cap, or with options out of range: PK_ERR_UNSUPPORTED before anything is allocated.
constexpr size_t kTdtBeamMaxScratch = (size_t)1 << 30;
constexpr int kTdtBeamGroupSteps = 8;           // steps enqueued between two reads of the "live hypotheses" word

struct TdtBeamWs {
    DevBuf tab, ints, score, hash, prefix, lab_id, lab_lp, dur_i, dur_lp, cand, bp, ctl, state, z, logits, out;
    DevBuf lmslot, lmlab;                       // the fused search only: lmstate, lm [2][R] and lab_ls, lab_lm [R][K + 1]
    bool fused = false;                         // the planned call is a fused one (sizes the scratch; run_tdt_beam is then given the model)
    std::vector<int32_t> h_tab;                 // T[B], row0[B]
    int B = 0, W = 0, K = 0, Kd = 0, N = 0, max_tokens = 0, t_max = 0, cap = 0;
    int steps_run = 0;                          // steps the last call enqueued
    TdtBeamDev dev(const Model &m) const;       // device view (after the buffers are reserved)
    TdtBeamOut out_view() const;
};

pk_tdt_beam_options tdt_beam_options_of(const pk_tdt_beam_options *opt);
// what the model entry points refuse (include/parakeet_amd.h): no TDT joint, gemm_bf16, a boost trie, options out of range
void tdt_beam_model_checks(const Model &m, const pk_tdt_beam_options &o);
size_t tdt_beam_scratch(const Model &m, int B, int t_max, int W, int K, int Kd, int N, int max_tokens, bool fused = false);
// Sizes the call (host only) and refuses past the scratch cap.  n_frames == nullptr: B clips of T frames, rows b T; else packed.
void tdt_beam_plan(TdtBeamWs &ws, const Model &m, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options &o, int max_tokens, bool fused = false);
// the search over ep = enc_proj of the batch's frames, and the back-trace; waits for the stream between groups of steps.
// lm: the fused search (the call was planned as one), null: the unfused search
void run_tdt_beam(Model &m, TdtBeamWs &ws, const float *d_ep, hipStream_t s, const LmDev *lm = nullptr);
// copies the results of the last search out ([B][N][max_tokens] / [B][N] / [B]; optional ones may be null) and waits for the stream
// (lm_score: after a fused search only)
void tdt_beam_copy_out(const TdtBeamWs &ws, int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                       int32_t *ok, hipStream_t s, float *lm_score = nullptr);
size_t tdt_beam_bytes(const TdtBeamWs &ws);

}  // namespace pk
