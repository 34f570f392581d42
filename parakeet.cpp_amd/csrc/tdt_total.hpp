// parakeet.cpp_amd/csrc/tdt_total.hpp -- host side of the forward-algorithm total of given token strings under the TDT head and of the n-best
// rescoring on top of it (kernels/tdt_total.hip).
#pragma once
#include "tdt_align.hpp"

namespace pk {

class Model;

// Scratch of one walk, with cells = sum_h T_h (U_h + 1) and labs = sum_h T_h U_h over its hypotheses: the alignment's (tdt_align.hpp) without the
// back-pointer bytes,
//   lattice values   4 (labs + cells + cells D) bytes
// and, when the lattice is computed from a model,
//   rows chunk       chunk_rows (V + D + J) 4 bytes
//   prediction net   (U_max + 1) n (J + 1) 4 bytes
// capped at kTdtAlignMaxScratch.  The model entry points walk the hypotheses of a call in GROUPS (tdt_total_groups): consecutive hypotheses, at
// most kTdtTotalGroupHyps of them (the width the lock-step prediction net's state is kept for), as many as stay under the cap.  A hypothesis whose
// own scratch exceeds the cap is refused with PK_ERR_UNSUPPORTED before anything is allocated.  Every value of a hypothesis is computed from its
// own rows alone, so the grouping changes no bit of any result.
constexpr int kTdtTotalGroupHyps = 256;

struct TdtTotalWs {
    TdtAlignWs a;                                   // the lattice, its tables and the prediction-net rows of one group (bp / start / end / didx / conf stay empty)
    DevBuf h, hn, c, cn;                            // LSTM state of the lock-step prediction net, [L][group][Hp] each
    std::vector<int32_t> T_of, row0_of, off, gstart;   // of the call: frames and first enc_proj row of every hypothesis, group-local offsets, group starts
    std::vector<float> total;                       // results of the call, gathered group by group
    std::vector<int32_t> ok;
};

// scratch bytes of n hypotheses with these sums (V = 0: a host lattice)
size_t tdt_total_scratch(int64_t cells, int64_t labs, int n, int u_max, int D, int V, int J);
// Checks the limits of every hypothesis (D, durations, U, own scratch) and cuts [0, n_hyp) into groups -> gstart (gstart.back() == n_hyp).
// Host only; refuses with PK_ERR_UNSUPPORTED.  max_hyps <= 0: kTdtTotalGroupHyps.
void tdt_total_groups(std::vector<int32_t> &gstart, const int32_t *T_of, const int32_t *id_offsets, int n_hyp, const int32_t *durations, int D, int V,
                      int J, int max_hyps = 0);
// the walk alone on a planned and uploaded lattice: results on the device in ws.out (total[B], ok[B])
// (upload first: tdt_lattice_upload of tdt_align.hpp with token_results = false -- no back-pointers, no token arrays)
void run_tdt_total_dp(TdtAlignWs &ws, hipStream_t s);
// Plans a call of the model entry points (host only, refuses before anything is allocated): n_hyp hypotheses, hypothesis h on the frames of clip
// clip_of[h] (nullptr: h, and n_hyp must equal n_clips); n_frames[n_clips] (nullptr: T each).
void tdt_total_plan_call(Model &m, TdtTotalWs &ws, const int32_t *n_frames, int n_clips, int T, const int32_t *id_offsets,
                         const int32_t *clip_of, int n_hyp);
// Queues the planned call on the model's stream: d_ep = enc_proj of the call's packed frames.  Group by group: prediction net, lattice, walk, results
// to ws.total / ws.ok (synchronises once per group).  ev (optional, 4 events per group, recorded around the three stages), ms[3] accumulates them.
void run_tdt_total_call(Model &m, TdtTotalWs &ws, const float *d_ep, const int32_t *ids, const int32_t *id_offsets, hipEvent_t *ev = nullptr,
                        float *ms = nullptr);
size_t tdt_total_bytes(const TdtTotalWs &ws);

// The ordering rule of pk_transcribe_pcm_nbest_rescored for one clip (tests/tdt_total_ref.py rescore_order): slots 0 .. N-1 in beam order ->
// order[N] and combined[N] (by slot).  Host only.
void rescore_order(const int32_t *lens, const float *ctc, const float *tdt, const int32_t *ok, int N, float w, int32_t *order, float *combined);

}  // namespace pk
