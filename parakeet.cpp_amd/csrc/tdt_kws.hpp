// parakeet.cpp_amd/csrc/tdt_kws.hpp -- host side of the TDT keyword spotting (kernels/tdt_kws.hip).
#pragma once
#include "ctc_kws.hpp"
#include "tdt_align.hpp"

namespace pk {

class Model;

// A call spots n_kw keywords in n_clips clips: n_clips x n_kw PAIRS, pair p = clip p / n_kw, keyword p % n_kw (the order of the results).  Every pair
// has a lattice of its own, packed as the alignment's (tdt_align.hpp), so with cells = sum_p T_p (L_p + 1), labs = sum_p T_p L_p, frames = sum_p T_p the
// scratch of n pairs is the total's (tdt_total.hpp: lattice values, rows chunk, prediction net) plus
//   top              4 cells bytes
//   exit rows        16 frames bytes                      (score, start, end per emission frame of the last token)
// capped at kTdtAlignMaxScratch.  The model entry points walk the pairs in GROUPS of consecutive pairs, as many as stay under the cap; the prediction net
// runs once per DISTINCT keyword of a group (at most kTdtKwsGroupKeywords of them, the width its lock-step state is kept for).  A pair whose own scratch
// exceeds the cap, a keyword of more than kKwsMaxLen tokens, max_hits outside 1 .. kKwsMaxHits, D outside 1 .. 8 or a duration outside
// [0, kTdtAlignMaxDur]: PK_ERR_UNSUPPORTED before anything is allocated.  Every value of a pair is computed from its own rows alone, so the grouping
// changes no bit of any result.
constexpr int kTdtKwsGroupKeywords = 256;
constexpr int kTdtKwsGroupPairs = 65536;

struct TdtKwsWs {
    TdtAlignWs a;                                   // the lattice of one group, its tables, the rows chunk
    TdtAlignWs net;                                 // the prediction net over the group's distinct keywords: its host tables, pp and tok alone
    DevBuf top, eb, out, net_of;                    // out: n_hits [n], then start, end, score [n][max_hits] each; net_of[n]: the net's slot of every pair
    DevBuf h, hn, c, cn;                            // LSTM state of the lock-step prediction net, [L][keywords][Hp] each
    std::vector<int32_t> T_of, row0_of, kw_of, pid, poff, off, gstart, h_net_of, kids, koff, slot;
    int max_hits = 1;
    float min_score = 0.0f;
    std::vector<int32_t> n_hits, start, end;        // results of the call, gathered group by group: [pairs], [pairs][max_hits]
    std::vector<float> score;
};

// scratch bytes of n pairs with these sums (V = 0: a host lattice)
size_t tdt_kws_scratch(int64_t cells, int64_t labs, int n, int u_max, int D, int V, int J);
// Plans a call (host only; refuses before anything is allocated).  n_frames[n_clips] (nullptr: T each).  clip_of / kw_of == nullptr: every keyword in every
// clip, n_pairs = n_clips * n_kw; otherwise pair p is keyword kw_of[p] on clip clip_of[p].  kws_check_args comes first.
void tdt_kws_plan_call(TdtKwsWs &ws, const int32_t *durations, int D, int V, int J, const int32_t *n_frames, int n_clips, int T, const int32_t *kw_ids,
                       const int32_t *kw_offsets, int n_kw, const int32_t *clip_of, const int32_t *kw_of, int n_pairs, const pk_kws_options &opt);
// The normalisation, the walk and the picking over the uploaded lattice of ws.a and ws.top; results stay on the device in ws.out.
void run_tdt_kws_dp(TdtKwsWs &ws, hipStream_t s);
// copies the n results of the walk just queued to ws.n_hits / start / end / score from pair g0 on and waits for the stream
void tdt_kws_gather(TdtKwsWs &ws, int g0, hipStream_t s);
// Queues the lattice of the pairs planned and uploaded in `a` (its values, and top[cells]) in chunks of a.chunk_rows rows: activation, heads product, kept
// values.  ep = enc_proj of the frames a.ep_row0() points into; pair b reads the rows of slot net_of[b] (device, [pairs]) of net.pp, which holds n_net slots.
void tdt_kws_build_lattice(Model &m, TdtAlignWs &a, float *top, const float *ep, const TdtAlignWs &net, const int *net_of, int n_net, hipStream_t s);
// Queues the planned call on the model's stream: d_ep = enc_proj of the call's packed frames.  Group by group: prediction net, lattice, walk (walk == false:
// the lattice of the LAST group is left in ws.a / ws.top, not normalised).  ev (optional, 4 events), ms[3] accumulates the three stages over the groups.
void run_tdt_kws_call(Model &m, TdtKwsWs &ws, const float *d_ep, const int32_t *kw_ids, const int32_t *kw_offsets, int chunk_rows = 0, bool walk = true,
                      hipEvent_t *ev = nullptr, float *ms = nullptr);
size_t tdt_kws_bytes(const TdtKwsWs &ws);

}  // namespace pk
