// parakeet.cpp_amd/csrc/capi_resample.cpp -- the resampling entry points of the C boundary: the host arithmetic (pk_resample_length / _run / _table),
// the device stage on caller buffers (pk_resample_device, _timed) and the input rate of a model's one-call API.
#include <algorithm>
#include <cstring>

#include "capi_util.hpp"

using namespace pk;

namespace {

// what pk_resample_device and its timed form check before they look for a device; -> the clips' input lengths
void device_args(const float *pcm, const int64_t *offsets, int n_clips, int src_rate, int dst_rate, std::vector<int64_t> &in_len) {
    need(offsets && n_clips > 0, "offsets/n_clips");
    resample_check_rates(src_rate, dst_rate);
    in_len.resize(n_clips);
    for (int i = 0; i < n_clips; ++i) {
        in_len[i] = offsets[i + 1] - offsets[i];
        need(in_len[i] >= 0, "offsets decrease");
        (void)resample_length(in_len[i], src_rate, dst_rate);      // (refuses a clip of 2^31 samples or more)
    }
    need(pcm || offsets[n_clips] == offsets[0], "pcm");
}

}  // namespace

extern "C" {

int64_t pk_resample_length(int64_t n, int src_rate, int dst_rate) {
    int64_t out = -1;
    (void)guard([&] { out = resample_length(n, src_rate, dst_rate); });
    return out;
}

int pk_resample_run(int src_rate, int dst_rate) {
    int run = 0;
    (void)guard([&] { run = resample_run(src_rate, dst_rate); });
    return run;
}

pk_status pk_resample_table(int src_rate, int dst_rate, double *table, int cap_rows, int *up, int *down) {
    return guard([&] {
        need(up && down, "up/down");
        ResampleTable t;
        resample_build_table(src_rate, dst_rate, t);
        *up = t.up; *down = t.down;
        if (!table) return;
        need(cap_rows >= t.up, "cap_rows < up");
        memcpy(table, t.w.data(), t.w.size() * sizeof(double));
    });
}

pk_status pk_resample_device(int device, const float *pcm, const int64_t *offsets, int n_clips, int src_rate, int dst_rate, float *out,
                             const int64_t *out_offsets) {
    return guard([&] {
        need(out && out_offsets, "out/out_offsets");
        std::vector<int64_t> in_len;
        device_args(pcm, offsets, n_clips, src_rate, dst_rate, in_len);
        need(out_offsets[0] >= 0, "out_offsets[0] < 0");
        for (int i = 0; i < n_clips; ++i)
            need(out_offsets[i + 1] - out_offsets[i] >= resample_length(in_len[i], src_rate, dst_rate), "out_offsets leave a clip too little room");
        if (src_rate == dst_rate) {
            for (int i = 0; i < n_clips; ++i)
                if (in_len[i]) memcpy(out + out_offsets[i], pcm + offsets[i], (size_t)in_len[i] * 4);
            return;
        }
        need_device();
        PK_HIP(hipSetDevice(device));
        ResampleWs ws;
        DevBuf d_out;
        const size_t out_total = (size_t)out_offsets[n_clips];
        d_out.reserve(std::max<size_t>(out_total, 1) * 4);
        if (out_total) PK_HIP(hipMemcpy(d_out.p, out, out_total * 4, hipMemcpyHostToDevice));
        resample_stage(ws, src_rate, dst_rate, n_clips, [&](int i) { return pcm + offsets[i]; }, in_len.data(), out_offsets, d_out.as<float>(), nullptr);
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(nullptr));
        if (out_total) PK_HIP(hipMemcpy(out, d_out.p, out_total * 4, hipMemcpyDeviceToHost));
    });
}

pk_status pk_resample_device_timed(int device, const float *pcm, const int64_t *offsets, int n_clips, int src_rate, int dst_rate, int reps, float *ms) {
    return guard([&] {
        need(ms && reps > 0, "ms/reps");
        std::vector<int64_t> in_len;
        device_args(pcm, offsets, n_clips, src_rate, dst_rate, in_len);
        need(src_rate != dst_rate, "equal rates are a copy: nothing to time");
        need_device();
        PK_HIP(hipSetDevice(device));
        std::vector<int64_t> out_off(n_clips + 1, 0);
        for (int i = 0; i < n_clips; ++i) out_off[i + 1] = out_off[i] + resample_length(in_len[i], src_rate, dst_rate);
        ResampleWs ws;
        DevBuf d_out;
        d_out.reserve(std::max<int64_t>(out_off[n_clips], 1) * 4);
        resample_stage(ws, src_rate, dst_rate, n_clips, [&](int i) { return pcm + offsets[i]; }, in_len.data(), out_off.data(), d_out.as<float>(), nullptr);
        PK_HIP(hipStreamSynchronize(nullptr));
        PK_CHECK_LAUNCH();
        struct Ev { hipEvent_t e[2] = {}; ~Ev() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } ev;
        for (auto &x : ev.e) PK_HIP(hipEventCreate(&x));
        const ResampleWs::DevTable &dt = ws.table(src_rate, dst_rate);
        std::vector<float> t;
        for (int r = 0; r < reps; ++r) {
            PK_HIP(hipEventRecord(ev.e[0], nullptr));
            resample_launch(ws, dt, n_clips, ws.raw.as<float>(), d_out.as<float>(), nullptr);
            PK_HIP(hipEventRecord(ev.e[1], nullptr));
            PK_HIP(hipStreamSynchronize(nullptr));
            PK_CHECK_LAUNCH();
            float v = 0;
            PK_HIP(hipEventElapsedTime(&v, ev.e[0], ev.e[1]));
            t.push_back(v);
        }
        std::sort(t.begin(), t.end());
        *ms = t[t.size() / 2];
    });
}

pk_status pk_model_set_input_rate(pk_model *m, int rate) {
    return guard([&] { need(m, "model"); m->m->set_input_rate(rate); });
}

pk_status pk_model_get_input_rate(const pk_model *m, int *rate) {
    return guard([&] { need(m && rate, "model/rate"); *rate = m->m->input_rate; });
}

}  // extern "C"
