// parakeet.cpp_amd/csrc/ctc_kws.hpp -- host side of the CTC keyword spotting (kernels/ctc_kws.hip).
#pragma once
#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

// Scratch of one call: (score, start frame) per end frame, keyword and utterance: 8 * n_kw * sum_b T_b bytes.  Above the cap, a keyword of more
// than kKwsMaxLen tokens or max_hits outside 1 .. kKwsMaxHits: PK_ERR_UNSUPPORTED before anything is allocated.
constexpr size_t kKwsMaxScratch = (size_t)1 << 30;

// grow-only device buffers of one spotting call and the host table that is uploaded for it
struct KwsWs {
    DevBuf ids, tab, g, eb, out;                        // out: n_hits [B][n_kw], then start, end, score [B][n_kw][max_hits] each
    std::vector<int32_t> h_tab;                         // kw_off[n_kw + 1]
    int B = 0, n_kw = 0, max_hits = 1;
    float min_score = 0.0f;
    size_t n_ids = 0;
    int64_t rows = 0;
};

// the options of a call: the library's defaults where opt == nullptr
pk_kws_options kws_options_of(const pk_kws_options *opt);

// PK_ERR_INVALID: B < 1, n_kw < 1, kw_offsets that decrease (kw_offsets[0] must be 0), an empty keyword, an id outside [0, V) or equal to blank,
// blank outside [0, V), min_score > 0 or NaN.  PK_ERR_UNSUPPORTED: a keyword of more than kKwsMaxLen tokens, max_hits outside 1 .. kKwsMaxHits.
// `what`: the name the refusals carry (the TDT spotting of tdt_kws.hpp runs the same checks).
void kws_check_args(const int32_t *ids, const int32_t *kw_offsets, int n_kw, int B, int V, int blank, const pk_kws_options &opt,
                    const char *what = "CTC keyword spotting");

// Sizes the call (host only); PK_ERR_UNSUPPORTED past the scratch cap.  n_frames == nullptr: every utterance T frames.  kws_check_args comes first.
void kws_plan(KwsWs &ws, const int32_t *n_frames, int B, int T, const int32_t *kw_offsets, int n_kw, const pk_kws_options &opt);

// The row maxima, the walk and the picking on stream s over device log-probs d_lp (uniform: rag.T == nullptr, B x T rows; packed: rag set).
// kws_plan comes first.  Results stay on the device in ws.
void run_ctc_kws(KwsWs &ws, const float *d_lp, int B, int T, const SeqRag &rag, int V, int blank, const int32_t *ids, hipStream_t s);

// copies the results of the last call out ([B][n_kw] and [B][n_kw][max_hits]) and waits for the stream
void kws_copy_out(const KwsWs &ws, int32_t *n_hits, int32_t *start, int32_t *end, float *score, hipStream_t s);

// bytes of device memory the spotting's buffers hold (pk_diag_mem_info)
size_t kws_bytes(const KwsWs &ws);

}  // namespace pk
