// parakeet.cpp_amd/csrc/resample.cpp -- builds the phase tables of the device resampler, sizes its launches and owns its staging buffers.
#include "resample.hpp"

#include <algorithm>

namespace pk {

static int gcd_of(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

void resample_check_rates(int src_rate, int dst_rate) {
    if (src_rate < kResampleMinRate || src_rate > kResampleMaxRate || dst_rate < kResampleMinRate || dst_rate > kResampleMaxRate)
        fail(PK_ERR_UNSUPPORTED, "resampling %d Hz -> %d Hz: rates from %d to %d Hz are taken", src_rate, dst_rate, kResampleMinRate, kResampleMaxRate);
}

int64_t resample_length(int64_t n, int src_rate, int dst_rate) {
    resample_check_rates(src_rate, dst_rate);
    if (n < 0) fail(PK_ERR_INVALID, "invalid argument: %lld samples", (long long)n);
    if (n >= ((int64_t)1 << 31)) fail(PK_ERR_UNSUPPORTED, "resampling: a clip of %lld samples (fewer than 2^31 are taken)", (long long)n);
    const int g = gcd_of(src_rate, dst_rate);
    const int64_t up = dst_rate / g, down = src_rate / g;
    return (n * up + down - 1) / down;          // n < 2^31, up <= 384 000: below 2^50
}

int resample_run(int src_rate, int dst_rate) {
    resample_check_rates(src_rate, dst_rate);
    const int g = gcd_of(src_rate, dst_rate);
    const int64_t up = dst_rate / g, down = src_rate / g;
    const int64_t fit = ((int64_t)(kResampleSpanCap - 34) * up / down) / 32 * 32;
    if (fit < 32) fail(PK_ERR_UNSUPPORTED, "resampling %d Hz -> %d Hz: 32 outputs read more than %d input samples", src_rate, dst_rate, kResampleSpanCap);
    return (int)std::min<int64_t>(kResampleMaxRun, fit);
}

void resample_build_table(int src_rate, int dst_rate, ResampleTable &t) {
    resample_check_rates(src_rate, dst_rate);
    const int g = gcd_of(src_rate, dst_rate);
    t.src = src_rate; t.dst = dst_rate; t.up = dst_rate / g; t.down = src_rate / g;
    const SincFilter f = sinc_filter(src_rate, dst_rate);
    t.w.assign((size_t)t.up * kResampleTaps, 0.0);
    t.coff.resize(t.up);
    for (int r = 0; r < t.up; ++r) {
        const int64_t p = (int64_t)r * t.down;
        t.coff[r] = (int32_t)(p / t.up);
        const double frac = (double)(p % t.up) / t.up;
        // |dist| <= 16 and width_factor >= 1: the window test of sinc_resample (|dist / width_factor| > 16) never skips one of these taps
        for (int k = 0; k < kResampleTaps; ++k)
            if (!sinc_tap_weight(f, frac + (double)(kResampleTaps / 2 - 1 - k), &t.w[(size_t)r * kResampleTaps + k]))
                fail(PK_ERR_INVALID, "internal: tap %d of phase %d lies outside the window", k, r);
    }
    t.run = resample_run(src_rate, dst_rate);
    t.span_cap = (int)((int64_t)t.run * t.down / t.up) + 34;
}

const ResampleWs::DevTable &ResampleWs::table(int src_rate, int dst_rate) {
    auto &slot = tabs[{src_rate, dst_rate}];
    if (!slot) {
        auto dt = std::make_unique<DevTable>();
        resample_build_table(src_rate, dst_rate, dt->t);
        dt->w.reserve(dt->t.w.size() * 8);
        dt->coff.reserve(dt->t.coff.size() * 4);
        PK_HIP(hipMemcpy(dt->w.p, dt->t.w.data(), dt->t.w.size() * 8, hipMemcpyHostToDevice));
        PK_HIP(hipMemcpy(dt->coff.p, dt->t.coff.data(), dt->t.coff.size() * 4, hipMemcpyHostToDevice));
        slot = std::move(dt);
    }
    return *slot;
}

int64_t resample_plan(ResampleWs &ws, const ResampleTable &t, const int64_t *in_len, const int64_t *out_off, int n_clips) {
    ws.h_clips.resize(n_clips);
    int64_t in_total = 0, wg = 0;
    for (int i = 0; i < n_clips; ++i) {
        ResampleClip &c = ws.h_clips[i];
        c.in_off = in_total; c.in_len = in_len[i]; c.out_off = out_off[i];
        c.out_len = resample_length(in_len[i], t.src, t.dst);
        c.wg0 = wg;
        in_total += in_len[i];
        wg += (c.out_len + t.run - 1) / t.run;
    }
    if (wg > 0x7fffffff) fail(PK_ERR_UNSUPPORTED, "resampling: the batch needs %lld workgroups", (long long)wg);
    return in_total;
}

void resample_launch(ResampleWs &ws, const ResampleWs::DevTable &dt, int n_clips, const float *d_in, float *d_out, hipStream_t s) {
    if (n_clips <= 0) return;
    const ResampleClip &last = ws.h_clips[n_clips - 1];
    ResampleArgs a{};
    a.x = d_in; a.y = d_out;
    a.clip = ws.clips.as<ResampleClip>(); a.n_clips = n_clips;
    a.tab = dt.w.as<double>(); a.coff = dt.coff.as<int>();
    a.up = dt.t.up; a.down = dt.t.down; a.run = dt.t.run; a.span_cap = dt.t.span_cap;
    a.n_wg = last.wg0 + (last.out_len + dt.t.run - 1) / dt.t.run;
    launch_resample(a, s);
}

void resample_stage(ResampleWs &ws, int src_rate, int dst_rate, int n_clips, const std::function<const float *(int)> &clip, const int64_t *in_len,
                    const int64_t *out_off, float *d_out, hipStream_t s) {
    const ResampleWs::DevTable &dt = ws.table(src_rate, dst_rate);
    PK_HIP(hipStreamSynchronize(s));
    const int64_t in_total = resample_plan(ws, dt.t, in_len, out_off, n_clips);
    ws.raw.reserve((size_t)std::max<int64_t>(in_total, 1) * 4);
    ws.clips.reserve((size_t)n_clips * sizeof(ResampleClip));
    for (int i = 0; i < n_clips;) {             // clips that follow each other in host memory go as one copy
        int j = i + 1;
        int64_t run = in_len[i];
        while (j < n_clips && clip(j) == clip(j - 1) + in_len[j - 1]) { run += in_len[j]; ++j; }
        if (run > 0) PK_HIP(hipMemcpyAsync(ws.raw.as<float>() + ws.h_clips[i].in_off, clip(i), (size_t)run * 4, hipMemcpyHostToDevice, s));
        i = j;
    }
    PK_HIP(hipMemcpyAsync(ws.clips.p, ws.h_clips.data(), (size_t)n_clips * sizeof(ResampleClip), hipMemcpyHostToDevice, s));
    resample_launch(ws, dt, n_clips, ws.raw.as<float>(), d_out, s);
}

}  // namespace pk
