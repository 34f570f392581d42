// parakeet.cpp_amd/csrc/vad.hpp -- host side of the voice-activity segmentation (kernels/vad.hip): the options as the
// kernels take them, the extents and the scratch of a packed batch, the launches, and the host logic that turns a clip's runs into pieces.
#pragma once
#include <cstring>
#include <functional>

#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

constexpr size_t kVadMaxScratch = (size_t)1 << 30;

// pk_vad_options checked and converted: thresholds rounded once from double, durations in frames
struct VadParams {
    float abs_thr = 0, ratio = 0;
    int floor_percent = 0, min_speech = 0, min_silence = 0, pad = 0, max_gap = 0, max_piece = 0;
};
pk_vad_options vad_default_options();
VadParams vad_params(const pk_vad_options *opt);               // NULL: the defaults; PK_ERR_INVALID for what the header lists

inline uint32_t vad_key(float e) { uint32_t k; memcpy(&k, &e, 4); return e != e ? 0xffffffffu : k; }
// frames of a clip of n samples; PK_ERR_INVALID for n < 0, PK_ERR_UNSUPPORTED for n >= 2^31
int32_t vad_frames(int64_t n);

// Grow-only device state of the stage on one device.  tabs: first[2], last[2], n_start, n_end per chunk; runs: run_start then run_end.
struct VadWs {
    DevBuf raw, clips, energy, hist, sel, flag, tabs, runs, n_runs;
    std::vector<VadClip> h_clips;
    int64_t S = 0, F = 0, C = 0, R = 0;                          // of the batch last sized (the header's formula)
};
size_t vad_bytes(const VadWs &ws);                               // bytes of device memory the buffers hold (pk_diag_mem_info)

// Sizes the batch (host only): fills ws.h_clips and ws.S / F / C / R; PK_ERR_UNSUPPORTED when the scratch would pass kVadMaxScratch.
void vad_plan(VadWs &ws, const VadParams &p, const int64_t *len, int n_clips);
// Reserves the scratch of what vad_plan sized, uploads the clips (clip(i) = host pointer of clip i's len[i] samples) and the extents on s.
// Waits for s first (the previous call's extents are uploaded out of ws.h_clips).
void vad_upload(VadWs &ws, int n_clips, const std::function<const float *(int)> &clip, hipStream_t s);
// The launches alone over what vad_upload left on the device; the runs stay there (vad_results).
void vad_launch(VadWs &ws, const VadParams &p, int n_clips, hipStream_t s);
// Host copies after the launches (synchronous on s): n_runs [n_clips]; run_start / run_end [R] and energy [F] where given.
void vad_results(VadWs &ws, int n_clips, int32_t *n_runs, int32_t *run_start, int32_t *run_end, float *energy, hipStream_t s);

// The pieces of one clip (host only; pk_vad_plan): frame ranges [first, last] in order.
struct VadPiece { int32_t first, last; };
void vad_pieces(int64_t n_samples, const int32_t *run_start, const int32_t *run_end, int n_runs, const float *energy, const VadParams &p,
                std::vector<VadPiece> &out);

}  // namespace pk
