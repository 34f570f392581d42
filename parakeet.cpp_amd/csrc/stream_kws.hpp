// parakeet.cpp_amd/csrc/stream_kws.hpp -- host side of the streaming TDT keyword spotting (kernels/tdt_kws_stream.hip).
#pragma once
#include <vector>

#include "tdt_align.hpp"

namespace pk {

class Model;

// n PAIRS are walked chunk by chunk; pair p is (stream p / n_kw, keyword p % n_kw).  What a pair carries from push to push lives on the device:
//   ring       (dur_max + 2) (2 D + 1) L_p 4 bytes        (the candidates and start frames its columns offered over the last dur_max + 2 frames)
//   pending    20 bytes                                    (the hit the online rule holds back, and the end of the last hit that left)
// and a push of c frames needs the lattice of n pairs x c frames (tdt_kws.hpp's formula: values, top, rows chunk) plus 16 c + 4 bytes of events per pair.
// The sum at c = kKwsChunkMaxFrames is capped at kTdtAlignMaxScratch; past it, more than kStreamKwsMaxKeywords keywords or kStreamKwsMaxPairs pairs, a
// keyword of more than kKwsMaxLen tokens, D outside 1 .. 8 or a duration outside [0, kTdtAlignMaxDur]: PK_ERR_UNSUPPORTED before anything is allocated.
constexpr int kStreamKwsMaxKeywords = 256;
constexpr int kStreamKwsMaxPairs = 65536;

// the options of a set: the library's defaults (-inf, 0) where opt == nullptr; PK_ERR_INVALID for min_score > 0 or NaN, patience < 0
pk_stream_kws_options stream_kws_options_of(const pk_stream_kws_options *opt);
void stream_kws_check_options(const pk_stream_kws_options &o);

// The carried state of n pairs, the lattice of the current chunk and the launches over it.
class KwsChunk {
  public:
    ~KwsChunk();
    // Host only: keeps the tables and refuses past the limits.  id_off[n_pairs + 1]: the pairs' packed keyword lengths; n_kw: keywords per stream (events
    // name pair p as stream p / n_kw, keyword p % n_kw).  V > 0: the lattice comes from a model (pairs of stream s read enc_proj rows s c + t).
    void setup(const int32_t *durations, int D, std::vector<int32_t> id_off, int n_kw, int V, int J, const pk_stream_kws_options &o, size_t extra_bytes);
    // allocates the carried state and clears it
    void alloc(hipStream_t s);
    // -inf candidates, no pending hit, frame 0 next
    void clear(hipStream_t s);
    // sizes the lattice for chunks of c frames (tables re-uploaded when c changes); ids: the pairs' packed tokens (the model route's keep launch reads them)
    void plan(int c, const int32_t *ids, hipStream_t s);
    // the normalisation, the walk and the rule over the lattice in a / top; results are copied to pinned memory on s (not waited for)
    void walk(bool rows, hipStream_t s);
    // after s was waited for: this push's events ordered by pair then by emission (the first cap are written, *n_events is the total) and, where
    // asked for, the rows [n_pairs][c]
    void collect(pk_kws_event *events, int cap, int *n_events, float *E, int32_t *Bs, int32_t *Ee);
    // emits every pending hit (waits for s)
    void flush(pk_kws_event *events, int cap, int *n_events, hipStream_t s);
    size_t bytes() const;

    TdtAlignWs a;
    DevBuf top;
    int n_pairs = 0, n_kw = 1, c = 0, t0 = 0;

  private:
    DevBuf ring_, pend_, out_, rows_;               // out_: n_ev [pairs] (padded to 16 bytes), then ev [pairs][c]
    std::vector<int32_t> id_off_, T_, row0_;
    int durations_[8] = {}, D_ = 0, V_ = 0, J_ = 0, dur_max_ = 0;
    pk_stream_kws_options opt_{};
    size_t ring_words_ = 0, nev_words_ = 0;
    void *pin_ = nullptr;
    size_t pin_bytes_ = 0;
    bool rows_copied_ = false;
};

// The keyword set of a streaming session: the prediction net's rows of every distinct keyword, kept for the life of the set, and the pairs' walk.
class StreamKws {
  public:
    // kws_check_args and the model checks come first (the caller's); refuses before anything is allocated
    StreamKws(Model &m, int S, const int32_t *ids, const int32_t *kw_offsets, int n_kw, const pk_stream_kws_options &o);
    // queues enc_proj of the chunk's rows d_enc [S c][hidden], the lattice and the walk on the model's stream
    void enqueue(const float *d_enc, int c, bool rows, hipEvent_t *ev = nullptr);
    KwsChunk w;

  private:
    Model &m_;
    int S_;
    TdtAlignWs net_;                                // its pp: [u][distinct keyword][J]
    DevBuf ep_, net_of_;
    std::vector<int32_t> pid_;
    int n_net_ = 0;
};

}  // namespace pk
