// parakeet.cpp_amd/csrc/ctc_align.hpp -- host side of the CTC forced alignment of given token strings (kernels/ctc_align.hip).
#pragma once
#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

// Scratch of one call: the back-pointers, sum_b T_b * ceil((2 L_b + 1) / 16) * 4 bytes (2 bits per lattice cell).  Above the cap, or a string
// of more than kAlignMaxStates states (L > 16383): PK_ERR_UNSUPPORTED before anything is allocated.
constexpr size_t kAlignMaxScratch = (size_t)1 << 30;

// grow-only device buffers of one alignment and the host tables that are uploaded for it
struct AlignWs {
    DevBuf ids, tab, off, bp, start, end, conf, out;   // out: score[B], total[B], ok[B]
    std::vector<int32_t> h_tab;                         // id_off[B + 1]
    std::vector<int64_t> h_off;                         // bp_off[B]
    int B = 0, shape = 0;
    size_t n_ids = 0, bp_dwords = 0;
};

// PK_ERR_INVALID: B < 1, non-monotone offsets (id_offsets[0] must be 0), an id outside [0, V) or equal to blank, blank outside [0, V)
void align_check_args(const int32_t *ids, const int32_t *id_offsets, int B, int V, int blank);

// Sizes the call (host only): shape and back-pointer offsets into ws; PK_ERR_UNSUPPORTED past the caps.  n_frames == nullptr: every utterance T frames.
void align_plan(AlignWs &ws, const int32_t *n_frames, int B, int T, const int32_t *id_offsets);

// The alignment on stream s over device log-probs d_lp (uniform: rag.T == nullptr, B x T rows; packed: rag set).  align_plan comes first.
// Results stay on the device in ws (start / end / conf zero-filled first).
void run_ctc_align(AlignWs &ws, const float *d_lp, int B, int T, const SeqRag &rag, int V, int blank, const int32_t *ids, bool want_total,
                   hipStream_t s);

// copies the results of the last alignment out (start / end / conf / total may be null) and waits for the stream
void align_copy_out(const AlignWs &ws, int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok, hipStream_t s);

}  // namespace pk
