// parakeet.cpp_amd/csrc/stream_endpoint.hpp -- host side of the endpointing on live audio (kernels/endpoint.hip).
#pragma once
#include <vector>

#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

// pk_endpoint_options in frames, with the two thresholds of the raw decision
struct EndpointParams {
    int W = 0, min_speech = 0, min_silence = 0, max_utterance = 0, eou_token_id = -1, reset_decoder = 1;
    float abs_thr = 0.0f, margin = 0.0f;
};
// the library's defaults where opt == nullptr
pk_endpoint_options endpoint_options_of(const pk_endpoint_options *opt);
// Host arithmetic alone.  PK_ERR_INVALID / PK_ERR_UNSUPPORTED as the header lists them; V > 0: eou_token_id is checked against the vocabulary and the blank.
EndpointParams endpoint_params(const pk_endpoint_options &o, int F, int V, int blank);

// What S streams carry from call to call lives on the device: the ring of W keys per stream and kEndpointStateWords words of rule state; a call of n
// frames adds 16 n + 4 bytes of events per stream (and 12 n of rows where the caller asks for them).
class EndpointChunk {
  public:
    ~EndpointChunk();
    EndpointChunk() = default;
    EndpointChunk(const EndpointChunk &) = delete;
    EndpointChunk &operator=(const EndpointChunk &) = delete;
    // host only
    void setup(int S, int F, const EndpointParams &p);
    // allocates the carried state and clears it
    void alloc(hipStream_t s);
    // every key 0xFFFFFFFF, outside an utterance, frame 0 next
    void clear(hipStream_t s);
    // refuses n outside 1 .. kEndpointMaxFrames (before anything is queued)
    void check_frames(int n) const;
    // the kernel over d_rows [S][n][F] (device) and the copy of its events, counts and state into pinned memory, on s (not waited for); ev: two events
    // recorded around the kernel's launch
    void run(const float *d_rows, int n, bool rows, hipStream_t s, hipEvent_t *ev = nullptr);
    // after s was waited for: this call's events per stream in the order emitted ...
    void take(std::vector<std::vector<pk_endpoint_event>> &per_stream) const;
    // ... the rows [S][n] where asked for, and the rule's state after the call
    void take_rows(float *level, float *floor, int32_t *speech0) const;
    bool in_utt(int s) const { return state_after(s)[0] != 0; }
    int utt_start(int s) const { return state_after(s)[3]; }
    // the close of the streams with bits[s] != 0 (bit 0: the prediction net h / c [Ln][S][Hp] and token, skipped where h == nullptr; bit 1: the acoustic
    // state), queued on s
    void close(const std::vector<unsigned char> &bits, float *h, float *c, int Ln, int Hp, int *token, int blank, hipStream_t s);
    int S = 0, F = 0, t0 = 0, n = 0;
    EndpointParams p;

  private:
    const int32_t *state_after(int s) const { return static_cast<const int32_t *>(pin_) + (size_t)s * kEndpointStateWords; }
    DevBuf ring_, out_, rows_, mask_;                   // out_: state [S][8], n_ev [S] (padded to 16 bytes), ev [S][n]
    size_t nev_words_ = 0;
    void *pin_ = nullptr;
    size_t pin_bytes_ = 0;
    bool rows_copied_ = false;
};

// events ordered by stream, then by emission: the first cap are written, *n_events is the total
void put_endpoint_events(const std::vector<std::vector<pk_endpoint_event>> &per_stream, pk_endpoint_event *events, int cap, int *n_events);

// The close on a session's decode workspace without an endpointer (pk_stream_reset_decoder): mask [S] on the host; waits for s.
void reset_decoder_rows(const uint8_t *mask, int S, float *h, float *c, int Ln, int Hp, int *token, int blank, DevBuf &d_mask, hipStream_t s);

}  // namespace pk
