// parakeet.cpp_amd/csrc/capi_group.cpp -- pk_group_*: one node, several GPUs (a replica and a host thread per device), and the RCCL
// exchange check.  The only file of the boundary that includes rccl_dyn.hpp.
#include <algorithm>
#include <chrono>
#include <exception>
#include <thread>

#include "capi_util.hpp"
#include "rccl_dyn.hpp"

using namespace pk;

extern "C" {

struct pk_group {
    std::vector<int> devices;
    std::vector<std::unique_ptr<Model>> models;
    double wall_ms_max = 0.0, audio_s = 0.0;
    std::vector<int32_t> clips_per_rank;
    std::vector<double> wall_ms;
    std::vector<std::vector<int>> last_shard;  // clip indices each rank handled in the last call (pk_group_verify_exchange)
    // RCCL is only touched by pk_group_verify_exchange: communicators and streams are created on its first call
    const RcclApi *rccl = nullptr;
    std::vector<ncclComm_t> comms;
    std::vector<hipStream_t> streams;
    ~pk_group() {
        for (size_t r = 0; r < streams.size(); ++r) {
            (void)hipSetDevice(devices[r]);
            if (streams[r]) (void)hipStreamDestroy(streams[r]);
        }
        models.clear();
        if (rccl) for (auto c : comms) if (c) (void)rccl->CommDestroy(c);
    }
};
#define PK_NCCL(api, call) do { ncclResult_t r_ = (api)->call; if (r_ != ncclSuccess) fail(PK_ERR_HIP, "RCCL: %s (%s)", (api)->GetErrorString(r_), #call); } while (0)

// runs fn(rank) on one host thread per device; the first exception of any rank is rethrown on the calling thread
static void for_each_rank(int n, const std::function<void(int)> &fn) {
    if (n == 1) { fn(0); return; }
    std::vector<std::exception_ptr> err(n);
    std::vector<std::thread> th;
    for (int r = 0; r < n; ++r)
        th.emplace_back([&, r] {
            try { fn(r); } catch (...) { err[r] = std::current_exception(); }
        });
    for (auto &t : th) t.join();
    for (auto &e : err) if (e) std::rethrow_exception(e);
}

pk_status pk_group_create(const char *weights, const char *vocab, const pk_config *cfg, const int *devices, int n_devices, pk_group **out) {
    return guard([&] {
        need(weights && cfg && out, "weights/cfg/out");
        int visible = 0;
        if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) fail(PK_ERR_NO_DEVICE, "no HIP device available (this engine has no CPU path)");
        auto g = std::make_unique<pk_group>();
        if (!devices || n_devices <= 0) {
            for (int d = 0; d < visible; ++d) g->devices.push_back(d);
        } else {
            for (int i = 0; i < n_devices; ++i) {
                need(devices[i] >= 0 && devices[i] < visible, "devices[i] out of range");
                g->devices.push_back(devices[i]);
            }
        }
        const int G = (int)g->devices.size();
        // ONE disk read (mmap) shared by every rank: each replica is built from the same host image by its own host thread -- the per-tensor
        // layout transforms and uploads of the G devices run concurrently, each device over its own PCIe link; no copy of the image is made.
        SafeTensors image(weights);
        const void *base = image.image_base();
        const size_t len = image.image_bytes();
        g->models.resize(G);
        const std::string vp = vocab ? vocab : "";
        for_each_rank(G, [&](int r) {
            g->models[r] = std::make_unique<Model>(base, len, vp, *cfg, /*borrow=*/true);
            g->models[r]->to_gpu(g->devices[r]);
        });
        g->clips_per_rank.assign(G, 0);
        g->wall_ms.assign(G, 0.0);
        g->last_shard.assign(G, {});
        *out = g.release();
    });
}

void pk_group_free(pk_group *g) { delete g; }
pk_status pk_group_set_attention_context(pk_group *g, int left, int right) {
    return guard([&] {
        need(g && !g->models.empty(), "group");
        g->models[0]->set_attention_context(left, right);           // (validated once: every replica has the same configuration)
        for (auto &m : g->models) m->set_attention_context(left, right);
    });
}
pk_status pk_group_set_input_rate(pk_group *g, int rate) {
    return guard([&] {
        need(g && !g->models.empty(), "group");
        g->models[0]->set_input_rate(rate);                             // (validated once)
        for (auto &m : g->models) m->set_input_rate(rate);
    });
}
int pk_group_size(const pk_group *g) { return g ? (int)g->devices.size() : 0; }

pk_status pk_group_transcribe_pcm(pk_group *g, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt, pk_result **results) {
    return guard([&] {
        need(g && pcm && offsets && results && n_clips > 0, "group/pcm/offsets/results/n_clips");
        const int G = (int)g->devices.size();
        // partition by AUDIO: clips sorted by length, longest first, each dealt to the rank with the least audio so far (equal lengths: rank
        // r takes clips r, r+G, ...); every rank then packs its own clips into ragged batches (transcribe_clips)
        std::vector<int> order(n_clips);
        for (int i = 0; i < n_clips; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });
        std::vector<std::vector<int>> shard(G);
        std::vector<int64_t> load(G, 0);
        double audio = 0.0;
        for (int i = 0; i < n_clips; ++i) {
            const int64_t len = offsets[order[i] + 1] - offsets[order[i]];
            const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            shard[r].push_back(order[i]);
            load[r] += len;
            audio += (double)len / (double)g->models[0]->input_rate;
        }
        auto store = new_store(n_clips);
        ResultStore &R = *store;
        std::vector<double> wall_ms(G, 0.0);
        // No collective anywhere: utterances share nothing, every rank writes the result slots of its own clips, and the ranks never wait
        // for each other.  Each rank runs its batches through its replica's two-stream pipeline (transcribe_clips).
        for_each_rank(G, [&](int r) {
            if (shard[r].empty()) return;
            const auto t0 = std::chrono::steady_clock::now();
            transcribe_clips(*g->models[r], pcm, offsets, shard[r], opt, R);
            wall_ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
        g->wall_ms = wall_ms;
        g->wall_ms_max = *std::max_element(wall_ms.begin(), wall_ms.end());
        g->audio_s = audio;
        for (int r = 0; r < G; ++r) g->clips_per_rank[r] = (int32_t)shard[r].size();
        g->last_shard = shard;
        *results = publish_store(std::move(store), n_clips, opt && opt->timestamps);
    });
}

pk_status pk_group_last_stats(const pk_group *g, double *wall_ms_max, double *audio_seconds, int32_t *clips_per_rank) {
    return guard([&] {
        need(g, "group");
        if (wall_ms_max) *wall_ms_max = g->wall_ms_max;
        if (audio_seconds) *audio_seconds = g->audio_s;
        if (clips_per_rank) std::copy(g->clips_per_rank.begin(), g->clips_per_rank.end(), clips_per_rank);
    });
}

// Debug check, never part of a transcription: the token ids of the last pk_group_transcribe_pcm go rank by rank through device memory and
// ONE fixed-stride ncclAllGather ([clips_per_rank][2 + max_tokens] int32 -- the exchange a multi-PROCESS deployment ends with,
// parakeet.cpp_amd/shard.py) plus an ncclAllReduce(max) of the per-rank token maxima and wall times; every rank's copy of the gathered
// matrix must reproduce `results`.  RCCL is loaded here, on first use (rccl_dyn.hpp); without it: PK_ERR_UNSUPPORTED.
pk_status pk_group_verify_exchange(pk_group *g, const pk_result *results, int n_clips, int *rccl_ranks) {
    return guard([&] {
        need(g && results && n_clips > 0, "group/results/n_clips");
        const int G = (int)g->devices.size();
        size_t total = 0;
        for (auto &sh : g->last_shard) total += sh.size();
        need((int)total == n_clips, "results are not those of the last pk_group_transcribe_pcm");
        if (!g->rccl) {
            std::string why;
            g->rccl = rccl_api(&why);
            if (!g->rccl) fail(PK_ERR_UNSUPPORTED, "RCCL is not available on this host (%s)", why.c_str());
            g->comms.assign(G, nullptr);
            for (int r = 0; r < G; ++r) {                  // RCCL's init turns ANY pending HIP error into a failure: start from a clean slate on every device
                PK_HIP(hipSetDevice(g->devices[r]));
                PK_HIP(hipDeviceSynchronize());
                (void)hipGetLastError();
            }
            PK_NCCL(g->rccl, CommInitAll(g->comms.data(), G, g->devices.data()));
            g->streams.assign(G, nullptr);
            for (int r = 0; r < G; ++r) {
                PK_HIP(hipSetDevice(g->devices[r]));
                PK_HIP(hipStreamCreateWithFlags(&g->streams[r], hipStreamNonBlocking));
            }
        }
        const RcclApi *N = g->rccl;
        if (rccl_ranks) PK_NCCL(N, CommCount(g->comms[0], rccl_ranks));
        const auto &shard = g->last_shard;
        size_t cap = 1;
        int local_max = 0;
        std::vector<std::vector<int>> rank_max(G, std::vector<int>(2, 0));
        for (int r = 0; r < G; ++r) {
            cap = std::max(cap, shard[r].size());
            for (int c : shard[r]) rank_max[r][0] = std::max(rank_max[r][0], (int)results[c].n_tokens);
            rank_max[r][1] = (int)std::min(g->wall_ms[r] * 1000.0, 2.0e9);                    // microseconds
            local_max = std::max(local_max, rank_max[r][0]);
        }
        std::vector<int *> dmax(G, nullptr);
        std::vector<int32_t *> dmat(G, nullptr), dall(G, nullptr);
        struct Guard {
            std::vector<int *> &a; std::vector<int32_t *> &b, &c; std::vector<int> &dev;
            ~Guard() { for (size_t r = 0; r < dev.size(); ++r) { (void)hipSetDevice(dev[r]); if (a[r]) (void)hipFree(a[r]); if (b[r]) (void)hipFree(b[r]); if (c[r]) (void)hipFree(c[r]); } }
        } free_all{dmax, dmat, dall, g->devices};
        for (int r = 0; r < G; ++r) {
            PK_HIP(hipSetDevice(g->devices[r]));
            PK_HIP(hipMalloc(reinterpret_cast<void **>(&dmax[r]), 2 * sizeof(int)));
            PK_HIP(hipMemcpyAsync(dmax[r], rank_max[r].data(), 2 * sizeof(int), hipMemcpyHostToDevice, g->streams[r]));
        }
        PK_NCCL(N, GroupStart());
        for (int r = 0; r < G; ++r) {
            PK_HIP(hipSetDevice(g->devices[r]));
            PK_NCCL(N, AllReduce(dmax[r], dmax[r], 2, ncclInt32, ncclMax, g->comms[r], g->streams[r]));
        }
        PK_NCCL(N, GroupEnd());
        int reduced[2] = {0, 0};
        PK_HIP(hipSetDevice(g->devices[0]));
        PK_HIP(hipMemcpyAsync(reduced, dmax[0], sizeof(reduced), hipMemcpyDeviceToHost, g->streams[0]));
        PK_HIP(hipStreamSynchronize(g->streams[0]));
        const int max_tok = reduced[0];
        if (max_tok != local_max) fail(PK_ERR_HIP, "RCCL all-reduce(max) returned %d tokens, the ranks hold %d", max_tok, local_max);
        if (std::abs(reduced[1] / 1000.0 - g->wall_ms_max) > 1.0) fail(PK_ERR_HIP, "RCCL all-reduce(max) of the wall times returned %d us", reduced[1]);
        const size_t stride = 2 + (size_t)max_tok, per_rank = cap * stride;
        std::vector<std::vector<int32_t>> hmat(G);
        for (int r = 0; r < G; ++r) {                      // row = [global clip index, n_tokens, ids...] ; unused rows: index -1
            hmat[r].assign(per_rank, 0);
            for (size_t i = 0; i < cap; ++i) hmat[r][i * stride] = -1;
            for (size_t i = 0; i < shard[r].size(); ++i) {
                const int c = shard[r][i];
                int32_t *row = hmat[r].data() + i * stride;
                row[0] = c;
                row[1] = results[c].n_tokens;
                std::copy(results[c].token_ids, results[c].token_ids + results[c].n_tokens, row + 2);
            }
            PK_HIP(hipSetDevice(g->devices[r]));
            PK_HIP(hipMalloc(reinterpret_cast<void **>(&dmat[r]), per_rank * 4));
            PK_HIP(hipMalloc(reinterpret_cast<void **>(&dall[r]), per_rank * 4 * G));
            PK_HIP(hipMemcpyAsync(dmat[r], hmat[r].data(), per_rank * 4, hipMemcpyHostToDevice, g->streams[r]));
        }
        PK_NCCL(N, GroupStart());
        for (int r = 0; r < G; ++r) {
            PK_HIP(hipSetDevice(g->devices[r]));
            PK_NCCL(N, AllGather(dmat[r], dall[r], per_rank, ncclInt32, g->comms[r], g->streams[r]));
        }
        PK_NCCL(N, GroupEnd());
        std::vector<int32_t> all(per_rank * G);
        for (int r = 0; r < G; ++r) {                      // EVERY rank's copy of the gathered matrix is checked
            PK_HIP(hipSetDevice(g->devices[r]));
            PK_HIP(hipMemcpyAsync(all.data(), dall[r], all.size() * 4, hipMemcpyDeviceToHost, g->streams[r]));
            PK_HIP(hipStreamSynchronize(g->streams[r]));
            int seen = 0;
            for (size_t row = 0; row < (size_t)G * cap; ++row) {
                const int32_t *p = all.data() + row * stride;
                if (p[0] < 0) continue;
                need(p[0] < n_clips && p[1] >= 0 && p[1] <= max_tok, "gathered token matrix row");
                if (results[p[0]].n_tokens != p[1] || !std::equal(p + 2, p + 2 + p[1], results[p[0]].token_ids))
                    fail(PK_ERR_HIP, "RCCL all-gather: rank %d holds different token ids for clip %d", r, p[0]);
                ++seen;
            }
            if (seen != n_clips) fail(PK_ERR_HIP, "RCCL all-gather: rank %d holds %d of %d clips", r, seen, n_clips);
        }
    });
}

}  // extern "C"
