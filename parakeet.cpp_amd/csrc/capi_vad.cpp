// parakeet.cpp_amd/csrc/capi_vad.cpp -- the voice-activity entry points of the C boundary: the options and the piece plan (host arithmetic), the
// device stage on caller buffers (pk_vad_pcm, _timed) and the one-call transcription of the pieces (pk_transcribe_pcm_vad).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "capi_util.hpp"

using namespace pk;

namespace {

// what pk_vad_pcm, its timed form and pk_transcribe_pcm_vad check before they look for a device; -> the options and the clips' lengths
VadParams stage_args(const float *pcm, const int64_t *offsets, int n_clips, const pk_vad_options *opt, std::vector<int64_t> &len) {
    need(offsets && n_clips > 0, "offsets/n_clips");
    const VadParams p = vad_params(opt);
    len.resize(n_clips);
    for (int i = 0; i < n_clips; ++i) {
        len[i] = offsets[i + 1] - offsets[i];
        need(len[i] >= 0, "offsets decrease");
        (void)vad_frames(len[i]);                                  // (refuses a clip of 2^31 samples or more)
    }
    need(pcm || offsets[n_clips] == offsets[0], "pcm");
    return p;
}

pk_vad_piece *pieces_out(const std::vector<pk_vad_piece> &v) {
    if (v.empty()) return nullptr;
    auto *out = static_cast<pk_vad_piece *>(malloc(v.size() * sizeof(pk_vad_piece)));
    if (!out) fail(PK_ERR_INVALID, "out of memory");
    memcpy(out, v.data(), v.size() * sizeof(pk_vad_piece));
    return out;
}

// the pieces of one clip as sample ranges, appended to out
void plan_clip(int clip, int64_t n, const int32_t *rs, const int32_t *re, int nr, const float *energy, const VadParams &p, std::vector<pk_vad_piece> &out) {
    std::vector<VadPiece> fr;
    vad_pieces(n, rs, re, nr, energy, p, fr);
    for (const VadPiece &q : fr) {
        pk_vad_piece o;
        memset(&o, 0, sizeof o);
        o.clip = clip;
        o.begin = (int64_t)q.first * kVadFrame;
        o.end = std::min<int64_t>(n, ((int64_t)q.last + 1) * kVadFrame);
        out.push_back(o);
    }
}

}  // namespace

extern "C" {

void pk_vad_options_default(pk_vad_options *out) {
    if (out) *out = vad_default_options();
}

int pk_vad_run(void) { return kVadRun; }

pk_status pk_vad_pcm(int device, const float *pcm, const int64_t *offsets, int n_clips, const pk_vad_options *opt, int32_t *n_runs,
                     int32_t *run_start, int32_t *run_end, float *energy) {
    return guard([&] {
        need(n_runs && run_start && run_end, "n_runs/run_start/run_end");
        std::vector<int64_t> len;
        const VadParams p = stage_args(pcm, offsets, n_clips, opt, len);
        VadWs ws;
        vad_plan(ws, p, len.data(), n_clips);
        need_device();
        PK_HIP(hipSetDevice(device));
        vad_upload(ws, n_clips, [&](int i) { return pcm + offsets[i]; }, nullptr);
        // the caller's arrays go up first: what the kernels leave alone comes back as it was
        int32_t *rs = ws.runs.as<int32_t>(), *re = rs + std::max<int64_t>(ws.R, 1);
        if (ws.R) {
            PK_HIP(hipMemcpyAsync(rs, run_start, (size_t)ws.R * 4, hipMemcpyHostToDevice, nullptr));
            PK_HIP(hipMemcpyAsync(re, run_end, (size_t)ws.R * 4, hipMemcpyHostToDevice, nullptr));
        }
        if (energy && ws.F) PK_HIP(hipMemcpyAsync(ws.energy.p, energy, (size_t)ws.F * 4, hipMemcpyHostToDevice, nullptr));
        vad_launch(ws, p, n_clips, nullptr);
        PK_CHECK_LAUNCH();
        vad_results(ws, n_clips, n_runs, run_start, run_end, energy, nullptr);
    });
}

pk_status pk_vad_plan(int64_t n_samples, const int32_t *run_start, const int32_t *run_end, int n_runs, const float *energy,
                      const pk_vad_options *opt, pk_vad_piece **pieces, int *n_pieces) {
    return guard([&] {
        need(pieces && n_pieces && n_runs >= 0 && (n_runs == 0 || (run_start && run_end)), "pieces/n_pieces/runs");
        const VadParams p = vad_params(opt);
        std::vector<pk_vad_piece> out;
        plan_clip(0, n_samples, run_start, run_end, n_runs, energy, p, out);
        *pieces = pieces_out(out);
        *n_pieces = (int)out.size();
    });
}

pk_status pk_vad_pcm_timed(int device, const float *pcm, const int64_t *offsets, int n_clips, const pk_vad_options *opt, int reps, float *ms) {
    return guard([&] {
        need(ms && reps > 0, "ms/reps");
        std::vector<int64_t> len;
        const VadParams p = stage_args(pcm, offsets, n_clips, opt, len);
        VadWs ws;
        vad_plan(ws, p, len.data(), n_clips);
        need_device();
        PK_HIP(hipSetDevice(device));
        vad_upload(ws, n_clips, [&](int i) { return pcm + offsets[i]; }, nullptr);
        struct Ev { hipEvent_t e[2] = {}; ~Ev() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } ev;
        for (auto &x : ev.e) PK_HIP(hipEventCreate(&x));
        std::vector<float> t;
        for (int r = 0; r <= reps; ++r) {                          // (the first pass warms the buffers up and is not counted)
            PK_HIP(hipEventRecord(ev.e[0], nullptr));
            vad_launch(ws, p, n_clips, nullptr);
            PK_HIP(hipEventRecord(ev.e[1], nullptr));
            PK_HIP(hipStreamSynchronize(nullptr));
            PK_CHECK_LAUNCH();
            float v = 0;
            PK_HIP(hipEventElapsedTime(&v, ev.e[0], ev.e[1]));
            if (r) t.push_back(v);
        }
        std::sort(t.begin(), t.end());
        *ms = t[t.size() / 2];
    });
}

pk_status pk_transcribe_pcm_vad(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt,
                                const pk_vad_options *vad_opt, pk_result **results, pk_vad_piece **pieces, int *n_pieces) {
    return guard([&] {
        need(h && pcm && results && (!pieces == !n_pieces), "model/pcm/results/pieces_out");
        Model &m = *h->m;
        if (m.input_rate != kModelRate)
            fail(PK_ERR_UNSUPPORTED, "pk_transcribe_pcm_vad takes 16 kHz PCM; this model's input rate is %d Hz (the VAD has no variant on resampled audio)", m.input_rate);
        std::vector<int64_t> len;
        const VadParams p = stage_args(pcm, offsets, n_clips, vad_opt, len);
        vad_plan(m.vad, p, len.data(), n_clips);
        m.require_gpu();
        vad_upload(m.vad, n_clips, [&](int i) { return pcm + offsets[i]; }, m.stream);
        vad_launch(m.vad, p, n_clips, m.stream);
        PK_CHECK_LAUNCH();
        std::vector<int32_t> nr(n_clips), rs(std::max<int64_t>(m.vad.R, 1)), re(rs.size());
        std::vector<float> en(std::max<int64_t>(m.vad.F, 1));
        vad_results(m.vad, n_clips, nr.data(), rs.data(), re.data(), en.data(), m.stream);
        std::vector<pk_vad_piece> all;
        for (int i = 0; i < n_clips; ++i) {
            const VadClip &c = m.vad.h_clips[i];
            plan_clip(i, len[i], rs.data() + c.run_off, re.data() + c.run_off, nr[i], en.data() + c.frame_off, p, all);
        }
        std::vector<ClipSpan> span(all.size());
        std::vector<int> clip_of(all.size()), off(all.size());
        for (size_t k = 0; k < all.size(); ++k) {
            span[k] = {pcm + offsets[all[k].clip] + all[k].begin, all[k].end - all[k].begin};
            clip_of[k] = all[k].clip;
            off[k] = (int)(all[k].begin / (kVadFrame * kVadGrid));
        }
        pk_vad_piece *out = pieces ? pieces_out(all) : nullptr;
        try {
            *results = transcribe_pieces(m, span, clip_of, off, n_clips, opt);
        } catch (...) {
            free(out);
            throw;
        }
        if (pieces) { *pieces = out; *n_pieces = (int)all.size(); }
    });
}

}  // extern "C"
