// parakeet.cpp_amd/csrc/ctc_beam.hpp -- host side of the CTC prefix beam search (kernels/ctc_beam.hip).
#pragma once
#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

// Caps of the forced alignment (timestamps): its alpha rows live in LDS (5 T + 2 words <= 64 KB) and its back-pointers take
// T (2 T + 1) bytes per hypothesis in global scratch, bounded in total.  Past either: PK_ERR_UNSUPPORTED (the search itself has no such cap).
constexpr int kBeamAlignMaxFrames = 3200;
constexpr size_t kBeamAlignMaxScratch = (size_t)1 << 30;

// grow-only device buffers of one search: top-K tables, node pool, hypothesis heads, back-pointers and the output arrays
struct BeamWs {
    DevBuf tk_val, tk_id, lpb, nodes, hyp, bp;
    DevBuf ids, lens, start, end, conf;         // [B][N][pitch], lens [B][N]; score = hyp_score
    DevBuf hyp_lm;                              // [B][N]: the LM score of every hypothesis (fused search only)
    int B = 0, N = 0, pitch = 0;                // extents of the last search
    const float *score() const { return hyp.as<float>() + 2 * (size_t)B * N; }
};

// throws PK_ERR_INVALID for parameters out of range (width 1..32, prune 1..32, n_best 1..width, 2 <= V <= 2^24, blank inside V)
void beam_check_options(const pk_beam_options &opt, int V, int blank);

// The whole search on stream s over device log-probs d_lp: uniform (rag.T == nullptr: B x T rows) or packed (rag set, T = the longest
// utterance).  rows = total frames.  Results stay on the device in ws (token arrays zero-filled first: unused slots read 0).
// lm != nullptr: the fused walk (ctc_beam_walk_kernel<true>) over that model takes the place of the unfused one and fills ws.hyp_lm.
void run_ctc_beam(BeamWs &ws, const float *d_lp, int B, int T, int64_t rows, const SeqRag &rag, int V, int blank, const pk_beam_options &opt,
                  hipStream_t s, const LmDev *lm = nullptr);

// copies the results of the last search out (any pointer may be null; lm_score only after a fused search) and waits for the stream
void beam_copy_out(const BeamWs &ws, int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, hipStream_t s,
                   float *lm_score = nullptr);

}  // namespace pk
