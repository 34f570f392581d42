// parakeet.cpp_amd/csrc/rnnt_lattice.hpp -- host side of the forced alignment and the forward-algorithm total of given token strings under the plain
// RNN-T head (kernels/rnnt_lattice.hip).
#pragma once
#include "tdt_align.hpp"

namespace pk {

class Model;

// Scratch of one walk, with cells = sum_b T_b (U_b + 1), labs = sum_b T_b U_b and words = sum_b (U_b + 1) ceil(T_b / 32) over its utterances:
//   lattice values   4 (labs + cells) bytes
//   back-pointers    4 words bytes                       (the alignment only: one bit per cell)
// and, when the lattice is computed from a model (V, J its vocabulary and joint width, U_max the longest string of the walk's n utterances):
//   rows chunk       chunk_rows (V + J) 4 bytes          (the heads product's output and its input, chunk_rows = tdt_align_chunk_rows(V))
//   prediction net   (U_max + 1) n (J + 1) 4 bytes       (pred_proj of every prefix, lock-step over the utterances, and the token table)
// capped at kTdtAlignMaxScratch (1 GiB, tdt_align.hpp).  The model entry points walk the utterances of a call in GROUPS of consecutive ones, at most
// kTdtTotalGroupHyps and as many as stay under the cap; every value of an utterance comes from its own rows alone, so the grouping changes no bit.
// An utterance of more than kRnntMaxTokens tokens, or whose own scratch exceeds the cap: PK_ERR_UNSUPPORTED before anything is allocated.
size_t rnnt_lattice_scratch(int64_t cells, int64_t labs, int64_t words, int n, int u_max, int V, int J, int chunk_rows = 0);

struct RnntLatticeWs {
    TdtAlignWs a;                                   // the lattice of one group packed as the TDT one with D = 0 (dl stays empty): its tables (tab64 carries
                                                    // bits_off[n + 1] behind cell_off and lab_off), ids, the prediction net's rows, the rows chunk, out = value[n], ok[n]
    DevBuf bits, start, end, conf;                  // the alignment only
    DevBuf h, hn, c, cn;                            // LSTM state of the lock-step prediction net, [L][group][Hp] each
    int64_t words = 0;                              // dwords of back-pointer bits of the planned group
    bool align = false;
    int chunk_rows = 0;                             // > 0: overrides the chunk size (the diagnostic)
    std::vector<int32_t> T_of, row0_of, off, gstart;   // of the call: frames and first enc_proj row of every utterance, group-local offsets, group starts
    std::vector<float> value, h_conf;               // results of the call, gathered group by group: score or total [n], conf packed as the ids
    std::vector<int32_t> ok, h_start, h_end;
    RnntWalkArgs args() const;                      // device view (after rnnt_lattice_upload)
};

// Sizes one walk over n utterances (host only) and refuses past the limits.  off[n + 1]: token offsets from 0; row0 != nullptr: utterance b reads the
// encoder rows from row0[b] on instead of its own packed rows.  V > 0: the lattice comes from a model.
void rnnt_lattice_plan(RnntLatticeWs &ws, const int32_t *T_of, const int32_t *row0, int n, const int32_t *off, int V, int J, bool align);
// reserves the buffers of the planned walk, uploads its tables and token strings on s, zero-fills the alignment's token arrays
void rnnt_lattice_upload(RnntLatticeWs &ws, const int32_t *ids, hipStream_t s);
// the walk (and, for the alignment, the back-trace) over ws.a.lab / blk; results stay on the device.  ev (optional, 2 events): around the back-trace.
void run_rnnt_walk(RnntLatticeWs &ws, hipStream_t s, hipEvent_t *ev = nullptr);
// copies the results of the planned walk to host arrays (token arrays may be null) and waits for the stream
void rnnt_copy_out(const RnntLatticeWs &ws, int32_t *start, int32_t *end, float *conf, float *value, int32_t *ok, hipStream_t s);

// what the model entry points refuse (include/parakeet_amd.h): no RNN-T head (encoder-only, TDT joint), gemm_bf16
void rnnt_model_checks(const Model &m);
// Plans a call of the model entry points (host only, refuses before anything is allocated): n_hyp token strings, string h on the frames of clip
// clip_of[h] (nullptr: h); n_frames[n_clips] (nullptr: T each) -> ws.gstart and the per-utterance tables.
void rnnt_plan_call(Model &m, RnntLatticeWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *id_offsets, const int32_t *clip_of, int n_hyp,
                    bool align, int chunk_rows = 0);
// group g of the planned call up to its lattice values: tables and ids up, prediction net, activation + heads product + keep in row chunks.
// d_ep = enc_proj of the call's packed frames.  ev (optional): ev[0] / ev[1] / ev[2] recorded before the prediction net, the lattice, and after it.
void run_rnnt_group_lattice(Model &m, RnntLatticeWs &ws, size_t g, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev = nullptr);
// Queues the planned call on the model's stream group by group: lattice, walk, results to ws.value / ok / h_start / h_end / h_conf (synchronises once
// per group).  ev (optional, 5 events), ms[4] accumulates the prediction net, the lattice, the walk, the back-trace.
void run_rnnt_call(Model &m, RnntLatticeWs &ws, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev = nullptr, float *ms = nullptr);
size_t rnnt_lattice_bytes(const RnntLatticeWs &ws);

}  // namespace pk
