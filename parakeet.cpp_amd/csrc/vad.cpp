// parakeet.cpp_amd/csrc/vad.cpp -- checks the options of the voice-activity segmentation, sizes its launches, owns its scratch, and cuts runs into pieces.
#include "vad.hpp"

#include <algorithm>
#include <cmath>

namespace pk {

pk_vad_options vad_default_options() {
    pk_vad_options o{};
    o.threshold_db = -50.0f; o.margin_db = 9.0f; o.floor_percent = 10;
    o.min_speech_ms = 100; o.min_silence_ms = 300; o.pad_ms = 200; o.max_gap_ms = 1000; o.max_piece_s = 30.0f;
    return o;
}

VadParams vad_params(const pk_vad_options *opt) {
    const pk_vad_options o = opt ? *opt : vad_default_options();
    if (!std::isfinite(o.threshold_db) || !std::isfinite(o.margin_db) || !std::isfinite(o.max_piece_s)) fail(PK_ERR_INVALID, "VAD options: a value is not finite");
    if (o.threshold_db < -200.0f || o.threshold_db > 60.0f) fail(PK_ERR_INVALID, "VAD options: threshold_db %g outside [-200, 60]", (double)o.threshold_db);
    if (o.margin_db < 0.0f || o.margin_db > 100.0f) fail(PK_ERR_INVALID, "VAD options: margin_db %g outside [0, 100]", (double)o.margin_db);
    if (o.floor_percent < 0 || o.floor_percent > 100) fail(PK_ERR_INVALID, "VAD options: floor_percent %d outside 0 .. 100", o.floor_percent);
    for (int32_t ms : {o.min_speech_ms, o.min_silence_ms, o.pad_ms, o.max_gap_ms})
        if (ms < 0 || ms > 3600000) fail(PK_ERR_INVALID, "VAD options: %d ms outside 0 .. 3600000", ms);
    const double mp = std::floor((double)o.max_piece_s * 100.0 + 0.5);
    if (mp < 16.0 || mp > 360000.0) fail(PK_ERR_INVALID, "VAD options: max_piece_s %g is %.0f frames (16 .. 360000 are taken)", (double)o.max_piece_s, mp);
    VadParams p;
    p.abs_thr = (float)(160.0 * std::pow(10.0, (double)o.threshold_db / 10.0));
    p.ratio = (float)std::pow(10.0, (double)o.margin_db / 10.0);
    p.floor_percent = o.floor_percent;
    p.min_speech = o.min_speech_ms / 10; p.min_silence = o.min_silence_ms / 10; p.pad = o.pad_ms / 10; p.max_gap = o.max_gap_ms / 10;
    p.max_piece = (int)mp;
    return p;
}

int32_t vad_frames(int64_t n) {
    if (n < 0) fail(PK_ERR_INVALID, "invalid argument: %lld samples", (long long)n);
    if (n >= ((int64_t)1 << 31)) fail(PK_ERR_UNSUPPORTED, "VAD: a clip of %lld samples (fewer than 2^31 are taken)", (long long)n);
    return (int32_t)((n + kVadFrame - 1) / kVadFrame);
}

size_t vad_bytes(const VadWs &ws) {
    size_t n = 0;
    for (const DevBuf *b : {&ws.raw, &ws.clips, &ws.energy, &ws.hist, &ws.sel, &ws.flag, &ws.tabs, &ws.runs, &ws.n_runs}) n += b->cap;
    return n;
}

void vad_plan(VadWs &ws, const VadParams &p, const int64_t *len, int n_clips) {
    ws.h_clips.resize(n_clips);
    int64_t S = 0, F = 0, C = 0, R = 0;
    for (int i = 0; i < n_clips; ++i) {
        VadClip &c = ws.h_clips[i];
        c.F = vad_frames(len[i]);
        c.in_off = S; c.n = len[i]; c.frame_off = F; c.chunk0 = C; c.run_off = R;
        c.rank = c.F > 0 ? (int32_t)(((int64_t)(c.F - 1) * p.floor_percent) / 100) : 0;
        S += (len[i] + 31) / 32 * 32;
        F += c.F;
        C += (c.F + kVadRun - 1) / kVadRun;
        R += (c.F + 1) / 2;
    }
    const double bytes = 4.0 * S + 6.0 * F + 24.0 * C + 8.0 * R + (double)(4 * 256 * 4 + sizeof(VadSelect) + 4 + sizeof(VadClip)) * n_clips;
    if (bytes > (double)kVadMaxScratch) fail(PK_ERR_UNSUPPORTED, "VAD: the batch needs %.0f bytes of scratch (at most 1 GiB is taken)", bytes);
    ws.S = S; ws.F = F; ws.C = C; ws.R = R;
}

void vad_upload(VadWs &ws, int n_clips, const std::function<const float *(int)> &clip, hipStream_t s) {
    PK_HIP(hipStreamSynchronize(s));
    ws.raw.reserve((size_t)std::max<int64_t>(ws.S, 1) * 4);
    ws.clips.reserve((size_t)n_clips * sizeof(VadClip));
    ws.energy.reserve((size_t)std::max<int64_t>(ws.F, 1) * 4);
    ws.hist.reserve((size_t)n_clips * 4 * 256 * 4);
    ws.sel.reserve((size_t)n_clips * sizeof(VadSelect));
    ws.flag.reserve((size_t)std::max<int64_t>(ws.F, 1) * 2);
    ws.tabs.reserve((size_t)std::max<int64_t>(ws.C, 1) * 6 * 4);
    ws.runs.reserve((size_t)std::max<int64_t>(ws.R, 1) * 2 * 4);
    ws.n_runs.reserve((size_t)n_clips * 4);
    for (int i = 0; i < n_clips; ++i)
        if (ws.h_clips[i].n > 0) PK_HIP(hipMemcpyAsync(ws.raw.as<float>() + ws.h_clips[i].in_off, clip(i), (size_t)ws.h_clips[i].n * 4, hipMemcpyHostToDevice, s));
    PK_HIP(hipMemcpyAsync(ws.clips.p, ws.h_clips.data(), (size_t)n_clips * sizeof(VadClip), hipMemcpyHostToDevice, s));
}

void vad_launch(VadWs &ws, const VadParams &p, int n_clips, hipStream_t s) {
    if (n_clips <= 0) return;
    PK_HIP(hipMemsetAsync(ws.hist.p, 0, (size_t)n_clips * 4 * 256 * 4, s));
    PK_HIP(hipMemsetAsync(ws.n_runs.p, 0, (size_t)n_clips * 4, s));
    VadArgs a{};
    a.x = ws.raw.as<float>();
    a.clip = ws.clips.as<VadClip>(); a.n_clips = n_clips; a.n_chunks = ws.C;
    a.energy = ws.energy.as<float>();
    a.hist = ws.hist.as<uint32_t>(); a.sel = ws.sel.as<VadSelect>();
    a.flag[0] = ws.flag.as<uint8_t>(); a.flag[1] = a.flag[0] + std::max<int64_t>(ws.F, 1);
    int32_t *t = ws.tabs.as<int32_t>();
    const int64_t C = std::max<int64_t>(ws.C, 1);
    a.first[0] = t; a.first[1] = t + C; a.last[0] = t + 2 * C; a.last[1] = t + 3 * C; a.n_start = t + 4 * C; a.n_end = t + 5 * C;
    a.run_start = ws.runs.as<int32_t>(); a.run_end = a.run_start + std::max<int64_t>(ws.R, 1);
    a.n_runs = ws.n_runs.as<int32_t>();
    a.abs_thr = p.abs_thr; a.ratio = p.ratio;
    a.min_speech = p.min_speech; a.min_silence = p.min_silence; a.pad = p.pad;
    launch_vad(a, s);
}

void vad_results(VadWs &ws, int n_clips, int32_t *n_runs, int32_t *run_start, int32_t *run_end, float *energy, hipStream_t s) {
    PK_HIP(hipMemcpyAsync(n_runs, ws.n_runs.p, (size_t)n_clips * 4, hipMemcpyDeviceToHost, s));
    const int32_t *rs = ws.runs.as<int32_t>(), *re = rs + std::max<int64_t>(ws.R, 1);
    if (run_start && ws.R) PK_HIP(hipMemcpyAsync(run_start, rs, (size_t)ws.R * 4, hipMemcpyDeviceToHost, s));
    if (run_end && ws.R) PK_HIP(hipMemcpyAsync(run_end, re, (size_t)ws.R * 4, hipMemcpyDeviceToHost, s));
    if (energy && ws.F) PK_HIP(hipMemcpyAsync(energy, ws.energy.p, (size_t)ws.F * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

void vad_pieces(int64_t n_samples, const int32_t *run_start, const int32_t *run_end, int n_runs, const float *energy, const VadParams &p,
                std::vector<VadPiece> &out) {
    const int32_t F = vad_frames(n_samples);
    const int mp = p.max_piece;
    bool open = false;
    VadPiece cur{0, 0};
    auto take = [&](int32_t s, int32_t e) {                        // a run of at most max_piece frames
        if (open && s - cur.last - 1 <= p.max_gap && e - cur.first + 1 <= mp) { cur.last = e; return; }
        if (open) out.push_back(cur);
        cur = {s, e};
        open = true;
    };
    int32_t prev_end = -1;
    for (int r = 0; r < n_runs; ++r) {
        int32_t s = run_start[r];
        const int32_t e = run_end[r];
        if (s < 0 || e < s || e >= F || s <= prev_end) fail(PK_ERR_INVALID, "invalid argument: run %d [%d, %d] of a clip of %d frames", r, s, e, F);
        prev_end = e;
        while (e - s + 1 > mp) {
            if (!energy) fail(PK_ERR_INVALID, "invalid argument: energy (a run longer than max_piece is cut at its quietest frame)");
            int32_t best = -1;
            uint32_t best_key = 0;
            for (int32_t f = s + mp / 2; f <= s + mp - 1; ++f) {
                if ((f + 1) % kVadGrid != 0) continue;
                const uint32_t k = vad_key(energy[f]);
                if (best < 0 || k < best_key) { best = f; best_key = k; }
            }
            if (best < 0) fail(PK_ERR_INVALID, "invalid argument: run %d starts at frame %d, not on the 8-frame grid", r, s);
            take(s, best);
            s = best + 1;
        }
        take(s, e);
    }
    if (open) out.push_back(cur);
}

}  // namespace pk
