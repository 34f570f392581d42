// parakeet.cpp_amd/csrc/tdt_align.hpp -- host side of the TDT forced alignment of given token strings (kernels/tdt_align.hip).
#pragma once
#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

class Model;

// Scratch of one call, with cells = sum_b T_b (U_b + 1) and labs = sum_b T_b U_b:
//   lattice values   4 (labs + cells + cells D) bytes
//   back-pointers    cells bytes
// and, when the lattice is computed from a model (V, J its vocabulary and joint width, U_max the longest string of the batch):
//   rows chunk       chunk_rows (V + D + J) 4 bytes      (the heads product's output and its input, chunk_rows = tdt_align_chunk_rows(V + D))
//   prediction net   (U_max + 1) B (J + 1) 4 bytes       (pred_proj of every prefix, lock-step over the batch, and the token table)
// Above the cap, for a string of more than kTdtAlignMaxTokens tokens, a duration outside [0, kTdtAlignMaxDur] or D outside [1, 8]:
// PK_ERR_UNSUPPORTED before anything is allocated.
constexpr size_t kTdtAlignMaxScratch = (size_t)1 << 30;
// rows of one chunk of the lattice: at most 256 MiB of logits, a multiple of 128 (the GEMM's tile height), at least 128
inline int tdt_align_chunk_rows(int VD) {
    const int64_t r = ((int64_t)256 << 20) / ((int64_t)VD * 4) / 128 * 128;
    return (int)(r < 128 ? 128 : r > 65536 ? 65536 : r);
}

// grow-only device buffers of one alignment and the host tables that are uploaded for it
struct TdtAlignWs {
    DevBuf lab, blk, dl, bp, tab, tab64, ids, start, end, didx, conf, out;   // tab: T[B], id_off[B + 1], ep_row0[B]; tab64: cell_off[B + 1], lab_off[B + 1]; out: score[B], ok[B]
    DevBuf pp, tok, z, logits;
    std::vector<int32_t> h_tab, h_tok;
    std::vector<int64_t> h_tab64;
    int B = 0, D = 0, u_max = 0, dur_max = 0, chunk_rows = 0;
    int durations[8] = {};
    size_t n_ids = 0;
    int64_t cells = 0, labs = 0;
    TdtLattice lattice() const;                     // device view (after tdt_lattice_upload)
    const int *ep_row0() const { return tab.as<int>() + 2 * (size_t)B + 1; }
};

// Sizes the call (host only) and refuses past the limits.  n_frames == nullptr: every utterance T frames.  V > 0: the lattice comes from a model
// (V, J: vocabulary and joint width; chunk_rows > 0 overrides the chunk size).
void tdt_align_plan(TdtAlignWs &ws, const int32_t *n_frames, int B, int T, const int32_t *id_offsets, const int32_t *durations, int D, int V = 0,
                    int J = 0, int chunk_rows = 0);
// The same plan for any walk over the lattice (the alignment, the forward-algorithm total of tdt_total.hpp).  row0 != nullptr: utterance b reads the
// encoder rows from row0[b] on (several token strings may share one clip's frames) instead of its own packed rows; back_pointers: the walk keeps one
// byte per cell; what: the name the refusals carry.
void tdt_lattice_plan(TdtAlignWs &ws, const int32_t *n_frames, const int32_t *row0, int B, int T, const int32_t *id_offsets, const int32_t *durations,
                      int D, int V, int J, int chunk_rows, bool back_pointers, const char *what);
// Reserves the lattice buffers of a planned walk and uploads its tables and token strings on s.  token_results (the alignment; the total keeps none):
// also reserves the back-pointers and the per-token result arrays, and zero-fills the latter.
void tdt_lattice_upload(TdtAlignWs &ws, const int32_t *ids, hipStream_t s, bool token_results);
// pred_proj of every prefix: U_max + 1 lock-step steps of the prediction net over [blank, ids...] on the decode loop's skinny products -> ws.pp.
// Uses m.ws's LSTM state buffers (sized for B utterances by the caller), or state = {h, hn, c, cn}, each [L][B][Hp] floats.
void run_tdt_align_pred(Model &m, TdtAlignWs &ws, const int32_t *ids, hipStream_t s, float *const *state = nullptr);
// the lattice values from ep = enc_proj of the packed frames (ws.tab's ep_row0), in chunks of ws.chunk_rows rows -> ws.lab / blk / dl
void run_tdt_align_lattice(Model &m, TdtAlignWs &ws, const float *d_ep, hipStream_t s);
// the heads product of the first n rows of ws.z alone -> ws.logits (what run_tdt_align_lattice runs per chunk; the timed entry point measures it on its own)
void run_tdt_align_heads(Model &m, TdtAlignWs &ws, int n, hipStream_t s);
// what the model entry points refuse (include/parakeet_amd.h): no TDT joint (encoder-only, RNN-T head), gemm_bf16
void tdt_align_model_checks(const Model &m);
// bytes of device memory the alignment's buffers hold (pk_diag_mem_info)
size_t tdt_align_bytes(const TdtAlignWs &ws);
// the walk and the back-trace over ws.lab / blk / dl; results stay on the device in ws
void run_tdt_align_dp(TdtAlignWs &ws, hipStream_t s);
// copies the results of the last alignment out (token arrays may be null) and waits for the stream
void tdt_align_copy_out(const TdtAlignWs &ws, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok, hipStream_t s);

}  // namespace pk
