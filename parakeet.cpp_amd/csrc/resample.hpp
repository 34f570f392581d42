// parakeet.cpp_amd/csrc/resample.hpp -- host side of the device resampler (kernels/resample.hip): the phase table of a
// (src, dst) pair, the extents of a packed batch and the launch.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <utility>

#include "common.hpp"
#include "kernels/kernels.hpp"

namespace pk {

constexpr int kModelRate = 16000;               // what the mel frontend takes
constexpr int kResampleMinRate = 4000, kResampleMaxRate = 384000;

// wav.cpp: the filter of sinc_resample and the weight of one of its taps (false: outside the window, the tap is skipped)
struct SincFilter { double cutoff, filter_scale, sample_ratio, width_factor; };
SincFilter sinc_filter(int src_rate, int dst_rate);
bool sinc_tap_weight(const SincFilter &f, double dist, double *weight);

// PK_ERR_UNSUPPORTED outside [kResampleMinRate, kResampleMaxRate]
void resample_check_rates(int src_rate, int dst_rate);
// ceil(n * up / down), the host resampler's output length; PK_ERR_UNSUPPORTED for n >= 2^31, PK_ERR_INVALID for n < 0
int64_t resample_length(int64_t n, int src_rate, int dst_rate);

// Outputs per workgroup at this pair of rates: the largest multiple of 32 up to kResampleMaxRun whose input span run * down / up + 34 fits
// kResampleSpanCap (at least 32 inside the rate range: down / up <= 96).
int resample_run(int src_rate, int dst_rate);

// The table of one (src, dst) pair (host only): w[r][k] is the weight of the tap at distance ((r * down) % up) / up + (15 - k) from the output's
// position, coff[r] = (r * down) / up the whole input samples phase r lies past q * down.  run = resample_run, span_cap = run * down / up + 34.
struct ResampleTable {
    int src = 0, dst = 0, up = 0, down = 0, run = 0, span_cap = 0;
    std::vector<double> w;
    std::vector<int32_t> coff;
};
void resample_build_table(int src_rate, int dst_rate, ResampleTable &t);

// Grow-only device state of the resampler on one device: the tables it has uploaded, the staged input-rate PCM and the batch's extents.
struct ResampleWs {
    struct DevTable { ResampleTable t; DevBuf w, coff; };
    std::map<std::pair<int, int>, std::unique_ptr<DevTable>> tabs;
    DevBuf raw, clips;
    std::vector<ResampleClip> h_clips;
    const DevTable &table(int src_rate, int dst_rate);      // built and uploaded (synchronously) on first use
};

// Sizes the launch of n_clips clips of in_len[i] input samples (host only): fills ws.h_clips with the packed input offsets, out_off[i] (where
// clip i's output starts, in samples of y) and the workgroups; -> the total of input samples.  PK_ERR_UNSUPPORTED for a clip of 2^31 samples or more.
int64_t resample_plan(ResampleWs &ws, const ResampleTable &t, const int64_t *in_len, const int64_t *out_off, int n_clips);

// The stage on stream s: clip(i) = host pointer of clip i's in_len[i] input-rate samples.  They are uploaded back to back into ws.raw and
// resampled into d_out at out_off[i].  Waits for s first (the extents of the previous call are uploaded out of ws.h_clips); src != dst.
void resample_stage(ResampleWs &ws, int src_rate, int dst_rate, int n_clips, const std::function<const float *(int)> &clip, const int64_t *in_len,
                    const int64_t *out_off, float *d_out, hipStream_t s);

// the kernel alone over what resample_plan sized and ws.raw / ws.clips hold
void resample_launch(ResampleWs &ws, const ResampleWs::DevTable &dt, int n_clips, const float *d_in, float *d_out, hipStream_t s);

}  // namespace pk
