// parakeet.cpp_amd/csrc/capi_batch.cpp -- the resident two-stream batch pipeline (pk_batch_*) and the one-call API on top of it:
// the packing policy (pk_plan_batches), pk_transcribe_pcm, pk_transcribe_pcm_nbest(_rescored, _tdt), pk_align_pcm, pk_tdt_align_pcm, pk_tdt_score_pcm, pk_spot_pcm and the result stores they hand out.
#include <algorithm>
#include <cstring>

#include "capi_util.hpp"
#include "neural_lm.hpp"

using namespace pk;

extern "C" {

/* ---- resident batch pipeline ---------------------------------------------------------------------------- */
// Two workspaces + two streams: the latency-bound decode loop of batch k (high-priority stream, a few small kernels
// per step) runs concurrently with the MFMA-bound mel + encoder of batch k+1 (main stream).  pk_batch_run(k) enqueues
// encoder(k) and then drives decode(k-1); pk_batch_sync / pk_batch_results flush the decode still pending.
// A stream of DISTINCT batches keeps the overlap with pk_batch_upload_async (PCM double-buffered, copied on its own stream
// under the running encoder) + pk_batch_results_done (the batch whose decode finished inside the last pk_batch_run; no flush).
struct pk_batch {
    Model *m;
    DevBuf pcm2[2];             // [max_clips][n_samples] x 2: the buffer being read by mel(k) and the one upload(k+1) fills
    int cur = 0;                // buffer the next pk_batch_run reads
    int staged = -1;            // buffer filled by pk_batch_upload_async and not yet consumed by a run
    int staged_clips = 0;
    // What each PCM buffer holds: a uniform batch (clips x n_samples) or a RAGGED one (clips of different lengths packed back to back,
    // pk_batch_upload_ragged).  A pipeline created with pk_batch_create_ragged takes both, run by run, inside its capacity.
    struct Held { bool ragged = false; int64_t n_samples = 0; RagBatch rag; } held[2];
    bool rag_capacity = false;  // created with pk_batch_create_ragged (capacity in ws[].rag_cap_*)
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done[2], mel_done[2];
    bool mel_used[2] = {false, false};
    int slot_clips[2] = {0, 0}; // clips of the run that owns each workspace
    int last_clips = 0;         // clips of the newest finished results
    Workspace ws[2];
    int n_clips = 0;
    int runs = 0;               // pk_batch_run calls so far
    int pending_slot = -1, pending_decoder = -1;   // decode not yet driven
    int last_slot = -1, last_decoder = -1;         // where the newest finished results live
    hipEvent_t ev[4];
    hipEvent_t enc_done[2], dec_done[2];
    bool used[2] = {false, false};
    bool ev_ok = false;
    // Decode groups (pk_batch_set_decode_group): the TDT loops of `group` consecutive runs are driven as ONE lock-step batch.  The loop is
    // launch-bound (4 launches per symbol step whatever the batch), and every launch on the decode stream costs the encoder of the
    // following run ~2 us (profiles/r02_decode_persistent.md): a group of G cuts that by G.  enc_proj of run k goes into its rows of
    // grp[fill].ep on the ENCODER stream right after encoder(k) (the encoder workspaces are then free again); a full group is decoded
    // under the encoder of the run after it.  Results of run k are available once its group is decoded (pk_batch_results_back).
    int group = 1;
    bool overlap = true;        // pk_batch_set_decode_overlap: false = the decode loop runs on the encoder's stream, after it
    hipStream_t dec_stream() const { return overlap ? m->stream_dec : m->stream; }
    struct Member { int clips, row0; int64_t seq; };
    struct Group {
        Workspace w;                    // decode state of group * max_clips utterances
        std::vector<Member> mem;        // runs in this group, oldest first
        int rows = 0;                   // utterances so far
        int64_t ep_rows = 0;            // enc_proj rows so far (ragged-capacity pipelines: runs of different row counts)
        int T_max = 0;                  // longest utterance among the members (bounds the lock-step loop)
        DevBuf tabs;                    // ragged-capacity pipelines: Tb[cap] then row0[cap] of the group's utterances (TdtState::Tb / row0)
        hipEvent_t ep_done = nullptr, dec_done = nullptr;
        bool decoded = false, used = false;
    } grp[2];
    struct Loc { Workspace *w; int row0, clips, decoder; hipEvent_t ev; int64_t seq; };
    // Finished (decode driven) runs, oldest first.  An entry stays readable until the buffers it points into are recycled: a pipeline
    // slot when run k+2 is encoded into it, a group buffer when the group after next starts to fill it.  Nothing else removes entries, so a
    // flush that drives a full group AND the partial group behind it keeps the runs of both (round-2 advisor finding).
    std::vector<Loc> done;
    int64_t slot_seq[2] = {-1, -1};     // run index that owns each pipeline slot
    void forget(const Workspace *w) {   // the buffers of `w` are about to be overwritten
        done.erase(std::remove_if(done.begin(), done.end(), [w](const Loc &l) { return l.w == w; }), done.end());
    }
    int fill = 0;                       // group collecting runs
    int ready = -1;                     // full group whose decode has not been driven yet
};

// makes the batch held by the current PCM buffer the run of workspace w
static void batch_set_run(pk_batch *b, Workspace &w, hipStream_t s) {
    const pk_batch::Held &H = b->held[b->cur];
    if (H.ragged) w.set_ragged(H.rag, s);
    else if (b->rag_capacity) w.set_uniform(b->n_clips, H.n_samples);
}

static void batch_encode(pk_batch *b, int slot) {
    Model &m = *b->m;
    Workspace &w = b->ws[slot];
    hipStream_t s = m.stream;
    b->forget(&w);                                           // the results of run k-2 live in this slot: no longer readable
    b->slot_seq[slot] = b->runs;
    if (b->used[slot]) PK_HIP(hipStreamWaitEvent(s, b->dec_done[slot], 0));   // decode(k-2) must be done with this slot
    if (b->staged >= 0) {                                    // a batch uploaded under the previous run: switch buffers
        b->cur = b->staged;
        b->n_clips = b->staged_clips;
        b->staged = -1;
        PK_HIP(hipStreamWaitEvent(s, b->copy_done[b->cur], 0));
    }
    batch_set_run(b, w, s);                                  // uniform or ragged: what the PCM buffer holds (tables uploaded on s)
    m.run_mel_ws(w, b->pcm2[b->cur].as<float>(), b->n_clips, s);
    PK_HIP(hipEventRecord(b->mel_done[b->cur], s));         // the PCM buffer is free again once the mel kernels have read it
    b->mel_used[b->cur] = true;
    m.run_encoder(w, w.feats.as<float>(), b->n_clips, w.Tm, -1, 0, s);
    PK_HIP(hipEventRecord(b->enc_done[slot], s));
    b->used[slot] = true;
    b->slot_clips[slot] = b->n_clips;
}

static void batch_decode(pk_batch *b, int slot, int decoder, hipStream_t s) {
    Model &m = *b->m;
    Workspace &w = b->ws[slot];
    if (s != m.stream) PK_HIP(hipStreamWaitEvent(s, b->enc_done[slot], 0));
    const int nc = b->slot_clips[slot] > 0 ? b->slot_clips[slot] : b->n_clips;
    if (decoder == PK_DECODER_CTC) m.run_ctc(w, w.x.as<float>(), nc, w.T_run, false, s);
    else m.run_tdt(w, w.x.as<float>(), nc, w.T_run, w.max_tokens, s);
    PK_HIP(hipEventRecord(b->dec_done[slot], s));
    b->last_slot = slot;
    b->last_decoder = decoder;
    b->last_clips = nc;
    b->forget(&w);                                            // (the timed / profiled single-slot paths decode into a slot they did not encode)
    b->done.push_back({&w, 0, nc, decoder, b->dec_done[slot], b->slot_seq[slot]});
}

// host-driven TDT loop of a whole decode group on the decode stream
static void group_drive(pk_batch *b, int gi) {
    Model &m = *b->m;
    auto &G = b->grp[gi];
    hipStream_t s = b->dec_stream();
    if (s != m.stream) PK_HIP(hipStreamWaitEvent(s, G.ep_done, 0));
    m.run_tdt_loop(G.w, G.rows, b->rag_capacity ? G.T_max : G.w.T, G.w.max_tokens, s);
    PK_HIP(hipEventRecord(G.dec_done, s));
    G.decoded = true;
    for (auto &mm : G.mem) b->done.push_back({&G.w, mm.row0, mm.clips, PK_DECODER_TDT, G.dec_done, mm.seq});
    b->last_slot = 0;                                         // (a result exists)
    b->last_decoder = PK_DECODER_TDT;
    b->last_clips = G.mem.back().clips;
}

// closes the group being filled (full, or partial at a flush) and makes the other buffer the one to fill
static void group_close(pk_batch *b) {
    auto &G = b->grp[b->fill];
    PK_HIP(hipEventRecord(G.ep_done, b->m->stream));
    b->ready = b->fill;
    b->fill ^= 1;
    b->grp[b->fill].mem.clear();
}

static void batch_flush(pk_batch *b) {
    if (b->pending_slot >= 0) {
        const int slot = b->pending_slot, dec = b->pending_decoder;
        b->pending_slot = -1;
        batch_decode(b, slot, dec, b->dec_stream());
    }
    if (b->ready >= 0) { const int r = b->ready; b->ready = -1; group_drive(b, r); }
    if (b->group > 1 && !b->grp[b->fill].mem.empty()) {      // a partial group: decode what there is
        group_close(b);
        const int r = b->ready;
        b->ready = -1;
        group_drive(b, r);
    }
    PK_HIP(hipStreamSynchronize(b->m->stream_dec));
    PK_HIP(hipStreamSynchronize(b->m->stream));
}

static void batch_run(pk_batch *b, int decoder) {
    Model &m = *b->m;
    m.require_gpu();
    need(b->n_clips > 0 || b->staged >= 0, "pk_batch_upload() first");
    need(decoder == PK_DECODER_CTC || decoder == PK_DECODER_TDT, "decoder");
    const int slot = b->runs & 1;
    const bool grouped = b->group > 1 && decoder == PK_DECODER_TDT;
    if (!grouped && b->group > 1 && (b->ready >= 0 || !b->grp[b->fill].mem.empty())) batch_flush(b);   // decoder switch inside a group
    batch_encode(b, slot);                                   // encoder(k) is queued first ...
    if (b->pending_slot >= 0) {                              // ... then the host drives decode(k-1) while it runs
        const int ps = b->pending_slot, pd = b->pending_decoder;
        b->pending_slot = -1;
        batch_decode(b, ps, pd, b->dec_stream());
    }
    if (grouped) {
        auto &G = b->grp[b->fill];
        Workspace &w = b->ws[slot];
        if (G.mem.empty()) {                                 // first run of a group: the buffer's previous decode must be done with it
            if (G.used) PK_HIP(hipStreamWaitEvent(m.stream, G.dec_done, 0));
            b->forget(&G.w);                                 // the runs of the group decoded two groups ago are overwritten from here on
            G.rows = 0;
            G.ep_rows = 0;
            G.T_max = 0;
            G.decoded = false;
        }
        const int nc = b->slot_clips[slot];
        const int64_t run_rows = w.rows(nc);
        m.run_enc_proj(w.x.as<float>(), run_rows, G.w.ep.as<float>() + (size_t)G.ep_rows * m.cfg.joint_hidden, m.stream);
        if (b->rag_capacity) {
            // the group's utterances have their own frame counts / first enc_proj rows: gathered behind the earlier members' (TdtState::Tb / row0)
            int *Tb = G.tabs.as<int>(), *row0 = Tb + G.w.B;
            launch_rag_decode_tables(w.ragged ? w.rv.seq.T : nullptr, w.ragged ? w.rv.seq.T_off : nullptr, w.T_run, nc, (int)G.ep_rows, Tb + G.rows, row0 + G.rows,
                                     m.stream);
            G.w.dec_Tb = Tb; G.w.dec_row0 = row0;
            G.T_max = std::max(G.T_max, w.t_max());
        }
        G.mem.push_back({nc, G.rows, b->slot_seq[slot]});
        G.rows += nc;
        G.ep_rows += run_rows;
        G.used = true;
        const bool full = (int)G.mem.size() == b->group;
        if (b->ready >= 0) {                                 // the group completed by an earlier run: decode it under this encoder
            const int r = b->ready;
            b->ready = -1;
            group_drive(b, r);
        }
        if (full) group_close(b);
    } else {
        b->pending_slot = slot;
        b->pending_decoder = decoder;
    }
    b->runs += 1;
    PK_CHECK_LAUNCH();
}

// (re)sizes the two pipeline slots for batches of up to max_clips clips of n_samples samples; buffers only ever grow
static void batch_size(pk_batch *b, int max_clips, int64_t n_samples) {
    Model &m = *b->m;
    for (auto &p : b->pcm2) p.reserve((size_t)max_clips * n_samples * 4);
    for (auto &w : b->ws) w.size_for(m.cfg, max_clips, -n_samples, pk_mel_num_frames(n_samples));
    for (auto &h : b->held) { h.ragged = false; h.n_samples = n_samples; }
    b->rag_capacity = false;
}
// capacity for ragged AND uniform batches of <= max_clips clips, <= max_total samples in all, <= max_clip per clip (buffers only ever grow)
static void batch_size_ragged(pk_batch *b, int max_clips, int64_t max_total, int64_t max_clip) {
    Model &m = *b->m;
    for (auto &p : b->pcm2) p.reserve((size_t)max_total * 4);
    for (auto &w : b->ws) w.size_ragged(m.cfg, max_clips, max_total, max_clip, /*own_pcm=*/false);
    for (auto &h : b->held) { h.ragged = false; h.n_samples = 0; }
    b->rag_capacity = true;
}

static std::unique_ptr<pk_batch> batch_new(Model &m, int max_clips, int64_t n_samples, int64_t rag_total = 0) {
    m.require_gpu();
    auto b = std::make_unique<pk_batch>();
    b->m = &m;
    if (rag_total > 0) batch_size_ragged(b.get(), max_clips, rag_total, n_samples);
    else batch_size(b.get(), max_clips, n_samples);
    for (auto &e : b->ev) PK_HIP(hipEventCreate(&e));
    PK_HIP(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        PK_HIP(hipEventCreateWithFlags(&b->enc_done[i], hipEventDisableTiming));
        PK_HIP(hipEventCreateWithFlags(&b->dec_done[i], hipEventDisableTiming));
        PK_HIP(hipEventCreateWithFlags(&b->copy_done[i], hipEventDisableTiming));
        PK_HIP(hipEventCreateWithFlags(&b->mel_done[i], hipEventDisableTiming));
    }
    b->ev_ok = true;
    return b;
}

pk_status pk_batch_create(pk_model *h, int max_clips, int64_t n_samples, pk_batch **out) {
    return guard([&] {
        need(h && out && max_clips > 0 && n_samples > 256, "model/out/max_clips/n_samples");
        *out = batch_new(*h->m, max_clips, n_samples).release();
    });
}

pk_status pk_batch_create_ragged(pk_model *h, int max_clips, int64_t max_total_samples, int64_t max_clip_samples, pk_batch **out) {
    return guard([&] {
        need(h && out && max_clips > 0 && max_clip_samples > 256 && max_total_samples >= max_clip_samples, "model/out/max_clips/max_total_samples/max_clip_samples");
        *out = batch_new(*h->m, max_clips, max_clip_samples, max_total_samples).release();
    });
}

void pk_batch_free(pk_batch *b) {
    if (!b) return;
    if (b->ev_ok) {
        (void)hipStreamSynchronize(b->m->stream_dec);
        (void)hipStreamSynchronize(b->m->stream);
        (void)hipStreamSynchronize(b->copy_stream);
        for (auto &e : b->ev) (void)hipEventDestroy(e);
        for (int i = 0; i < 2; ++i) {
            (void)hipEventDestroy(b->enc_done[i]); (void)hipEventDestroy(b->dec_done[i]);
            (void)hipEventDestroy(b->copy_done[i]); (void)hipEventDestroy(b->mel_done[i]);
        }
        (void)hipStreamDestroy(b->copy_stream);
        for (auto &G : b->grp) {
            if (G.ep_done) (void)hipEventDestroy(G.ep_done);
            if (G.dec_done) (void)hipEventDestroy(G.dec_done);
        }
    }
    delete b;
}

pk_status pk_batch_upload(pk_batch *b, const float *pcm, int n_clips) {
    return guard([&] {
        need(b && pcm && n_clips > 0 && n_clips <= b->ws[0].B, "batch/pcm/n_clips");
        need(!b->rag_capacity, "a pipeline created with pk_batch_create_ragged takes pk_batch_upload_ragged (equal lengths are a special case of it)");
        b->m->require_gpu();
        batch_flush(b);
        PK_HIP(hipStreamSynchronize(b->copy_stream));
        b->staged = -1;
        PK_HIP(hipMemcpyAsync(b->pcm2[b->cur].p, pcm, (size_t)n_clips * b->ws[0].n_samples * 4, hipMemcpyHostToDevice, b->m->stream));
        PK_HIP(hipStreamSynchronize(b->m->stream));
        b->n_clips = n_clips;
    });
}

// what a PCM buffer holds after staging clips of the given lengths: a uniform batch when all lengths agree (the plain kernels: no tables),
// otherwise a ragged one
static void batch_hold(pk_batch *b, int buf, const int64_t *lens, int n_clips) {
    Model &m = *b->m;
    pk_batch::Held &H = b->held[buf];
    bool same = true;
    int64_t total = 0, longest = 0;
    for (int i = 0; i < n_clips; ++i) { same = same && lens[i] == lens[0]; total += lens[i]; longest = std::max(longest, lens[i]); }
    const Workspace &w = b->ws[0];
    if (n_clips > w.rag_cap_clips || total > w.rag_cap_samples || longest > w.rag_cap_clip)
        fail(PK_ERR_INVALID, "batch of %d clips / %lld samples (longest %lld) exceeds the pipeline's capacity (%d clips, %lld samples, %lld per clip)", n_clips,
             (long long)total, (long long)longest, w.rag_cap_clips, (long long)w.rag_cap_samples, (long long)w.rag_cap_clip);
    for (int i = 0; i < n_clips; ++i) need(lens[i] > 256, "every clip needs more than 256 samples");
    H.ragged = !same;
    H.n_samples = same ? lens[0] : 0;
    if (!same) {
        const int t_max = pk_encoder_num_frames(pk_mel_num_frames(longest));
        H.rag.build_from_samples(lens, n_clips, att_block_rows_of(m, t_max));
    }
}

pk_status pk_batch_upload_ragged(pk_batch *b, const float *pcm, const int64_t *offsets, int n_clips) {
    return guard([&] {
        need(b && pcm && offsets && n_clips > 0, "batch/pcm/offsets/n_clips");
        need(b->rag_capacity, "pk_batch_upload_ragged needs a pipeline created with pk_batch_create_ragged");
        b->m->require_gpu();
        batch_flush(b);
        PK_HIP(hipStreamSynchronize(b->copy_stream));
        b->staged = -1;
        std::vector<int64_t> lens(n_clips);
        for (int i = 0; i < n_clips; ++i) lens[i] = offsets[i + 1] - offsets[i];
        batch_hold(b, b->cur, lens.data(), n_clips);
        int64_t o = 0;
        for (int i = 0; i < n_clips; ++i) {        // packed back to back in the device buffer, whatever the gaps in the caller's
            PK_HIP(hipMemcpyAsync(b->pcm2[b->cur].as<float>() + o, pcm + offsets[i], (size_t)lens[i] * 4, hipMemcpyHostToDevice, b->m->stream));
            o += lens[i];
        }
        PK_HIP(hipStreamSynchronize(b->m->stream));
        b->n_clips = n_clips;
    });
}

// stages the NEXT batch into the PCM buffer the running encoder does not read, on the copy stream.  clip(i) = host pointer of clip i;
// clips that follow each other in host memory go as one copy.  raw_lens: the clips are at the model's input rate, raw_lens[i] samples each; they are
// uploaded to the resampler's staging buffer and the kernel writes their lens[i] 16 kHz samples where the copy would have (resample.hpp).
static void batch_stage(pk_batch *b, int n_clips, const std::function<const float *(int)> &clip, const int64_t *lens = nullptr,
                        const int64_t *raw_lens = nullptr) {
    b->m->require_gpu();
    const int nb = b->staged >= 0 ? b->staged : (b->cur ^ 1);      // re-staging before a run overwrites the staged batch
    std::vector<int64_t> uni;
    if (!lens) { uni.assign(n_clips, b->held[nb].n_samples > 0 ? b->held[nb].n_samples : b->ws[0].n_samples); lens = uni.data(); }
    if (b->rag_capacity) batch_hold(b, nb, lens, n_clips);         // (validates the batch against the capacity before anything is copied)
    PK_HIP(hipStreamSynchronize(b->copy_stream));                  // at most one copy in flight; the previous host buffer is released here
    if (b->mel_used[nb]) PK_HIP(hipStreamWaitEvent(b->copy_stream, b->mel_done[nb], 0));   // the last mel that read this buffer
    int64_t o = 0;
    if (raw_lens) {
        std::vector<int64_t> out_off(n_clips);
        for (int i = 0; i < n_clips; ++i) { out_off[i] = o; o += lens[i]; }
        resample_stage(b->m->rs, b->m->input_rate, kModelRate, n_clips, clip, raw_lens, out_off.data(), b->pcm2[nb].as<float>(), b->copy_stream);
    } else for (int i = 0; i < n_clips;) {
        int j = i + 1;
        int64_t run = lens[i];
        while (j < n_clips && clip(j) == clip(j - 1) + lens[j - 1]) { run += lens[j]; ++j; }
        PK_HIP(hipMemcpyAsync(b->pcm2[nb].as<float>() + o, clip(i), (size_t)run * 4, hipMemcpyHostToDevice, b->copy_stream));
        o += run;
        i = j;
    }
    PK_HIP(hipEventRecord(b->copy_done[nb], b->copy_stream));
    b->staged = nb;
    b->staged_clips = n_clips;
}

pk_status pk_batch_upload_async(pk_batch *b, const float *pcm, int n_clips) {
    return guard([&] {
        need(b && pcm && n_clips > 0 && n_clips <= b->ws[0].B, "batch/pcm/n_clips");
        need(!b->rag_capacity, "a pipeline created with pk_batch_create_ragged takes pk_batch_upload_ragged_async");
        const int64_t n = b->ws[0].n_samples;
        batch_stage(b, n_clips, [&](int i) { return pcm + (size_t)i * n; });
    });
}

pk_status pk_batch_upload_ragged_async(pk_batch *b, const float *pcm, const int64_t *offsets, int n_clips) {
    return guard([&] {
        need(b && pcm && offsets && n_clips > 0, "batch/pcm/offsets/n_clips");
        need(b->rag_capacity, "pk_batch_upload_ragged_async needs a pipeline created with pk_batch_create_ragged");
        std::vector<int64_t> lens(n_clips);
        for (int i = 0; i < n_clips; ++i) lens[i] = offsets[i + 1] - offsets[i];
        batch_stage(b, n_clips, [&](int i) { return pcm + offsets[i]; }, lens.data());
    });
}

pk_status pk_batch_run(pk_batch *b, int decoder) {
    return guard([&] { need(b, "batch"); batch_run(b, decoder); });
}

pk_status pk_batch_sync(pk_batch *b) {
    return guard([&] { need(b, "batch"); b->m->require_gpu(); batch_flush(b); });
}

int pk_batch_max_tokens(const pk_batch *b) { return b ? b->ws[0].max_tokens : 0; }

// copies the results of one finished run: rows [row0, row0 + clips) of its workspace, presented as [clips][max_tokens]
static void copy_results(const pk_batch::Loc &L, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    Workspace &w = *L.w;
    const int B = L.clips, mt = w.max_tokens;
    const size_t src_w = (size_t)(L.decoder == PK_DECODER_TDT ? mt : w.T);        // CTC arrays are [B][T] on the device
    auto pitch = [&](void *dst, const void *src) {
        if (dst) PK_HIP(hipMemcpy2D(dst, (size_t)mt * 4, static_cast<const char *>(src) + (size_t)L.row0 * src_w * 4, src_w * 4, src_w * 4, B, hipMemcpyDeviceToHost));
    };
    PK_HIP(hipMemcpy(lens, w.lens.as<int>() + L.row0, (size_t)B * 4, hipMemcpyDeviceToHost));
    pitch(ids, w.ids.p); pitch(start, w.start.p); pitch(end, w.end.p); pitch(conf, w.conf.p);
    zero_tail(ids, lens, B, mt); zero_tail(start, lens, B, mt); zero_tail(end, lens, B, mt); zero_tail(conf, lens, B, mt);
}

pk_status pk_batch_results(pk_batch *b, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    return guard([&] {
        need(b && ids && lens, "batch/ids/lens");
        b->m->require_gpu();
        batch_flush(b);
        need(!b->done.empty(), "pk_batch_run() first");
        copy_results(b->done.back(), ids, lens, start, end, conf);
    });
}

pk_status pk_batch_results_back(pk_batch *b, int back, int *n_clips, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    return guard([&] {
        need(b && ids && lens, "batch/ids/lens");
        b->m->require_gpu();
        need(!b->done.empty(), "no decoded batch yet: the decode of run k finishes inside a later pk_batch_run (or pk_batch_sync)");
        need(back >= 0 && back < (int)b->done.size(), "back: only the runs of the newest decoded group are kept");
        const pk_batch::Loc &L = b->done[b->done.size() - 1 - (size_t)back];
        PK_HIP(hipEventSynchronize(L.ev));
        if (n_clips) *n_clips = L.clips;
        copy_results(L, ids, lens, start, end, conf);
    });
}

pk_status pk_batch_margins(pk_batch *b, int back, float *min_margin) {
    return guard([&] {
        need(b && min_margin, "batch/min_margin");
        b->m->require_gpu();
        need(back >= 0 && back < (int)b->done.size(), "back: 0 <= back < pk_batch_results_available()");
        const pk_batch::Loc &L = b->done[b->done.size() - 1 - (size_t)back];
        need(L.decoder == PK_DECODER_TDT && !b->m->boost_on, "margins are reported for unboosted TDT / RNNT decodes");
        PK_HIP(hipEventSynchronize(L.ev));
        PK_HIP(hipMemcpy(min_margin, L.w->margin.as<float>() + L.row0, (size_t)L.clips * 4, hipMemcpyDeviceToHost));
    });
}

pk_status pk_batch_results_done(pk_batch *b, int *n_clips, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf) {
    return pk_batch_results_back(b, 0, n_clips, ids, lens, start, end, conf);
}

int pk_batch_results_available(const pk_batch *b) { return b ? (int)b->done.size() : 0; }

static void batch_set_group(pk_batch *b, int group) {
    need(group >= 1 && group <= 16, "decode group: 1 .. 16 runs");
    Model &m = *b->m;
    m.require_gpu();
    batch_flush(b);
    for (auto &G : b->grp) b->forget(&G.w);              // their buffers may be reallocated below: read results BEFORE changing the group size
    if (group > 1) {
        need(m.cfg.vocab_size > 0, "decode groups apply to the TDT / RNNT decoder; this model has none");
        for (auto &G : b->grp) {
            G.w.size_decode(m.cfg, group * b->ws[0].B, b->ws[0].T, (size_t)group * b->ws[0].rag_cap_rows);
            if (b->rag_capacity) G.tabs.reserve((size_t)2 * group * b->ws[0].B * sizeof(int));
            if (!G.ep_done) PK_HIP(hipEventCreateWithFlags(&G.ep_done, hipEventDisableTiming));
            if (!G.dec_done) PK_HIP(hipEventCreateWithFlags(&G.dec_done, hipEventDisableTiming));
            G.mem.clear();
            G.rows = 0;
            G.ep_rows = 0;
            G.T_max = 0;
            G.used = G.decoded = false;
        }
    }
    b->fill = 0;
    b->ready = -1;
    b->group = group;
}

pk_status pk_batch_set_decode_overlap(pk_batch *b, int on) {
    return guard([&] {
        need(b, "batch");
        b->m->require_gpu();
        batch_flush(b);
        b->overlap = on != 0;
    });
}

pk_status pk_batch_set_decode_group(pk_batch *b, int group) {
    return guard([&] { need(b, "batch"); batch_set_group(b, group); });
}

// One un-pipelined run on the main stream with hipEvents between the stages (mel / encoder / decode / total, ms).
pk_status pk_batch_run_timed(pk_batch *b, int decoder, float ms[4]) {
    return guard([&] {
        need(b && ms, "batch/ms");
        need(decoder == PK_DECODER_CTC || decoder == PK_DECODER_TDT, "decoder");
        Model &m = *b->m;
        m.require_gpu();
        need(b->n_clips > 0, "pk_batch_upload() first");
        batch_flush(b);
        Workspace &w = b->ws[0];
        hipStream_t s = m.stream;
        batch_set_run(b, w, s);
        PK_HIP(hipEventRecord(b->ev[0], s));
        m.run_mel_ws(w, b->pcm2[b->cur].as<float>(), b->n_clips, s);
        PK_HIP(hipEventRecord(b->ev[1], s));
        m.run_encoder(w, w.feats.as<float>(), b->n_clips, w.Tm, -1, 0, s);
        PK_HIP(hipEventRecord(b->ev[2], s));
        b->slot_clips[0] = b->n_clips;
        batch_decode(b, 0, decoder, s);
        PK_HIP(hipEventRecord(b->ev[3], s));
        PK_CHECK_LAUNCH();
        PK_HIP(hipStreamSynchronize(s));
        b->used[0] = true;
        PK_HIP(hipEventElapsedTime(&ms[0], b->ev[0], b->ev[1]));
        PK_HIP(hipEventElapsedTime(&ms[1], b->ev[1], b->ev[2]));
        PK_HIP(hipEventElapsedTime(&ms[2], b->ev[2], b->ev[3]));
        PK_HIP(hipEventElapsedTime(&ms[3], b->ev[0], b->ev[3]));
    });
}

void *pk_batch_dev_pcm(pk_batch *b) { return b ? b->pcm2[b->cur].p : nullptr; }
void *pk_batch_stream(pk_batch *b) { return b ? (void *)b->m->stream : nullptr; }

int pk_batch_profile(pk_batch *b, int decoder, pk_kernel_stat *out, int cap) {
    int n_out = -1;
    pk_status st = guard([&] {
        need(b && out && cap > 0, "batch/out/cap");
        need(decoder == 0 || decoder == 1, "decoder must be 0 (CTC) or 1 (TDT)");
        need(b->n_clips > 0, "no clips uploaded");
        Model &m = *b->m;
        m.require_gpu();
        ProfileSink sink;
        m.prof = &sink;
        batch_flush(b);
        try {
            Workspace &w = b->ws[0];
            batch_set_run(b, w, m.stream);
            m.run_mel_ws(w, b->pcm2[b->cur].as<float>(), b->n_clips, m.stream);
            m.run_encoder(w, w.feats.as<float>(), b->n_clips, w.Tm, -1, 0, m.stream);
            b->slot_clips[0] = b->n_clips;
            batch_decode(b, 0, decoder, m.stream);
            PK_HIP(hipStreamSynchronize(m.stream));
            b->used[0] = true;
        } catch (...) {
            m.prof = nullptr;
            throw;
        }
        m.prof = nullptr;
        std::vector<pk_kernel_stat> agg;
        for (auto &r : sink.recs) {
            float ms = 0.0f;
            PK_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
            size_t i = 0;
            for (; i < agg.size(); ++i)
                if (r.name == agg[i].name) break;
            if (i == agg.size()) {
                pk_kernel_stat k;
                memset(&k, 0, sizeof k);
                snprintf(k.name, sizeof k.name, "%s", r.name.c_str());
                agg.push_back(k);
            }
            agg[i].launches += 1;
            agg[i].total_ms += ms;
            agg[i].flops += r.flops;
            agg[i].bytes += r.bytes;
        }
        n_out = (int)agg.size();
        for (int i = 0; i < n_out && i < cap; ++i) out[i] = agg[i];
    });
    return st == PK_OK ? n_out : (int)st;
}

// Brings a pipeline back to a defined idle state after an error inside a run (nothing pending, nothing readable).
static void batch_reset(pk_batch *b) {
    (void)hipStreamSynchronize(b->m->stream_dec);
    (void)hipStreamSynchronize(b->m->stream);
    (void)hipStreamSynchronize(b->copy_stream);
    (void)hipGetLastError();
    b->pending_slot = b->pending_decoder = -1;
    b->ready = -1;
    b->staged = -1;
    b->n_clips = 0;
    for (auto &G : b->grp) { G.mem.clear(); G.rows = 0; G.ep_rows = 0; G.T_max = 0; }
    b->done.clear();
}

static const size_t kTokenShrinkBytes = (size_t)512 << 20;   // token arrays of a pipeline (2 slots + 2 decode groups) above which a shorter call re-sizes them
// The pipeline a Model keeps for the one-call API (pk_transcribe_pcm, every rank of a pk_group): created on first use with ragged capacity
// (batches of mixed lengths AND uniform ones), re-sized when a call needs more (buffers only grow; the token arrays may shrink, see below), freed with the model.
static pk_batch *model_pipeline(Model &m, int max_clips, int64_t max_total, int64_t max_clip) {
    m.require_gpu();
    if (!m.pipe) {
        m.pipe = batch_new(m, max_clips, max_clip, max_total).release();
        m.pipe_free = [](void *p) { pk_batch_free(static_cast<pk_batch *>(p)); };
        return static_cast<pk_batch *>(m.pipe);
    }
    pk_batch *b = static_cast<pk_batch *>(m.pipe);
    batch_flush(b);
    PK_HIP(hipStreamSynchronize(b->copy_stream));
    b->done.clear();
    b->staged = -1;
    b->n_clips = 0;
    const Workspace &w = b->ws[0];
    // Buffers only grow -- except the token arrays, the one allocation pitched (clips x longest clip x max_symbols): when the pipeline was
    // sized for a clip at least twice as long as anything in this call and those arrays are large, they are released and re-reserved for this
    // call's longest clip, so that one long file does not make every later batch carry (and copy, and zero) its pitch (round-4 advisor finding).
    int64_t clip_cap = std::max(max_clip, w.rag_cap_clip);
    size_t tok = 0;
    for (auto &x : b->ws) tok += x.token_bytes();
    for (auto &G : b->grp) tok += G.w.token_bytes();
    // ... and whenever transcribe_clips' segment rule would have cut here (clips four times shorter than what the arrays are pitched for AND
    // one slot's arrays above kTokenShrinkBytes / 8): a segment cut is always followed by a re-pitch (round-5 advisor finding: between the two
    // thresholds a cut used to happen with no shrink behind it, and every batch of the new segment still carried the long file's pitch).
    const bool seg_rule = max_clip * 4 <= w.rag_cap_clip && w.token_bytes() > kTokenShrinkBytes / 8;
    if ((tok > kTokenShrinkBytes && max_clip * 2 <= w.rag_cap_clip) || seg_rule) {
        for (auto &x : b->ws) x.release_tokens();
        for (auto &G : b->grp) { b->forget(&G.w); G.w.release_tokens(); }
        clip_cap = max_clip;
    }
    batch_size_ragged(b, std::max(max_clips, w.rag_cap_clips), std::max(max_total, w.rag_cap_samples), clip_cap);
    return b;
}

}  // extern "C"

/* ---- one-call API ------------------------------------------------------------------------------------------ */

struct pk::ResultStore {      // owns everything a pk_result array points into
    std::vector<pk_result> res;
    std::vector<std::string> text;
    std::vector<std::vector<int32_t>> ids, start, end;
    std::vector<std::vector<float>> conf;
    std::vector<std::vector<std::string>> word_text;
    std::vector<std::vector<pk_word>> words;
};
void pk::ResultStoreDelete::operator()(ResultStore *s) const { delete s; }

// The packing policy of the one-call API (pure host logic; pk_plan_batches exposes it): clips sorted by length, longest first (stable), then
// cut greedily into batches of at most kMaxBatchClips clips and kBatchRows ENCODER ROWS (a single longer clip gets a batch of its own).
// Rows, not seconds, are what the batch costs: every product of the encoder is an M x N x K GEMM with M = the batch's packed rows, tiled 128
// (64) rows high, and 8192 rows are exactly the tile grids the kernels were tuned on -- fc2 / out_proj / pw2: 256 (512) tiles = ONE round of the
// 256 CUs, fc1: 1024 tiles = two rounds.  One tile row more starts another round of workgroups on every product: measured round 4
// (profiles/r04_mixed_bench_distributions.txt) 8272 rows cost fc2 +52 %, out_proj / pw2 +59 %, the encoder 27.3 instead of ~21 ms.
static const int kMaxBatchClips = 256;
static const int64_t kBatchRows = 8192;                          // 64 tile rows of 128; 64 x 10 s = 8064 rows, 65 x 10 s = 8190
static void plan_batches(const int64_t *len, int n, std::vector<int> &order, std::vector<int> &bstart) {
    order.resize(n);
    std::vector<int64_t> rows(n);
    for (int i = 0; i < n; ++i) {
        need(len[i] > 256, "every clip needs more than 256 samples");
        need(len[i] <= ((int64_t)1 << 30), "clip too long");
        order[i] = i;
        rows[i] = pk_encoder_num_frames(pk_mel_num_frames(len[i]));
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
    bstart.clear();
    for (int i = 0; i < n;) {
        bstart.push_back(i);
        int64_t tot = 0;
        int j = i;
        while (j < n && j - i < kMaxBatchClips && (j == i || tot + rows[order[j]] <= kBatchRows)) tot += rows[order[j++]];
        i = j;
    }
    bstart.push_back(n);
}

// The n tokens of one hypothesis into slot c of R: ids and text (transcribe.hpp:149,172) and, where the timestamp arrays are given, frames,
// confidences and the word grouping (group_timestamps, transcribe.hpp:150-152).
static void store_tokens(Model &m, ResultStore &R, int c, int n, const int32_t *ids, const int32_t *start, const int32_t *end, const float *conf) {
    R.ids[c].assign(ids, ids + n);
    std::vector<int> iv(R.ids[c].begin(), R.ids[c].end());
    if (m.tok.loaded()) R.text[c] = m.tok.decode(iv);
    if (!start) return;
    R.start[c].assign(start, start + n);
    R.end[c].assign(end, end + n);
    R.conf[c].assign(conf, conf + n);
    if (!m.tok.loaded()) return;
    std::vector<TimestampedToken> tt(n);
    for (int q = 0; q < n; ++q) tt[q] = {R.ids[c][q], R.start[c][q], R.end[c][q], R.conf[c][q]};
    auto words = group_timestamps(tt, m.tok.pieces(), false);
    for (auto &wd : words) R.word_text[c].push_back(wd.word);
    for (size_t q = 0; q < words.size(); ++q)
        R.words[c].push_back({R.word_text[c][q].c_str(), words[q].start, words[q].end, words[q].confidence});
}

// Transcriber::transcribe (transcribe.hpp:99-179) of the clips listed in `clips` (global indices into offsets), results into the slots
// of the same indices of R.  One model, one device; called by pk_transcribe_pcm (all clips) and by every rank of a pk_group.
void pk::transcribe_clips(Model &m, const float *pcm, const int64_t *offsets, const std::vector<int> &clips, const pk_options *opt, ResultStore &R) {
    int n = 0;
    for (int c : clips) n = std::max(n, c + 1);
    std::vector<ClipSpan> span(n);
    for (int c : clips) span[c] = {pcm + offsets[c], offsets[c + 1] - offsets[c]};
    transcribe_spans(m, span.data(), clips, opt, R);
}

// ... of clips that need not follow each other in memory: clip c is the span[c].n samples at span[c].p
void pk::transcribe_spans(Model &m, const ClipSpan *span, const std::vector<int> &clips, const pk_options *opt, ResultStore &R) {
    m.require_gpu();
    const int decoder = opt ? opt->decoder : PK_DECODER_TDT;
    const bool ts = opt && opt->timestamps;
    need(decoder == PK_DECODER_CTC || decoder == PK_DECODER_TDT, "options.decoder");
    // per-call boost phrases (transcribe.hpp:110-115): the model-level setting comes back when the call ends
    struct BoostScope {
        Model &m; bool active = false; std::vector<std::vector<int>> saved; float saved_score = 0.0f;
        ~BoostScope() { if (active) { try { m.set_boost(saved, saved_score); } catch (...) {} } }
    } scope{m};
    if (opt && opt->n_boost_phrases > 0) {
        need(opt->boost_phrases != nullptr, "options.boost_phrases");
        auto ph = encode_phrases(m, opt->boost_phrases, opt->n_boost_phrases);
        scope.saved = m.boost_phrases; scope.saved_score = m.boost_score; scope.active = true;
        m.set_boost(ph, opt->boost_score);
    }
    // Mixed-length batching (the reference's roadmap item "batch inference: pad + length-mask", README.md:513 -- done by PACKING, no padding
    // and no masks: every clip keeps its own extents in every kernel and comes out bit-identical to a single-clip call).  The clips are
    // sorted by length, longest first (the position tables and the workspace are then sized once, by the first batch), and packed greedily
    // into batches of at most kMaxBatchClips clips and kBatchRows encoder rows -- neighbours in length share a batch, so the lock-step decode
    // loop of a batch ends for all of them at about the same step.  The batches go through the model's two-stream pipeline (struct
    // pk_batch): PCM of batch k+1 is staged on the copy stream and decode(k) -- or, from four batches on, the decode loops of four batches as
    // one lock-step group -- runs under encoder(k+1).  A batch whose clips all have the same length runs the plain uniform kernels.
    const int n_clips = (int)clips.size();
    if (n_clips == 0) return;
    // At another input rate than 16 kHz (Model::input_rate) pcm / offsets count input-rate samples: the batches are planned by the RESAMPLED
    // lengths and every batch is resampled on the device while it is staged (batch_stage); everything behind that sees 16 kHz samples.
    const bool resampled = m.input_rate != kModelRate;
    std::vector<int64_t> clip_len(n_clips);
    for (int i = 0; i < n_clips; ++i) {
        const int64_t raw = span[clips[i]].n;
        clip_len[i] = resampled ? resample_length(raw, m.input_rate, kModelRate) : raw;
    }
    std::vector<int> order, bstart;                                // order: positions in `clips`, longest first; bstart: first position of every batch, + the end
    plan_batches(clip_len.data(), n_clips, order, bstart);
    std::vector<int64_t> len16(n_clips);                           // 16 kHz samples of the clip at position i of `order`
    for (int i = 0; i < n_clips; ++i) len16[i] = clip_len[order[i]];
    for (auto &o : order) o = clips[o];                            // ... as global clip indices from here on
    auto len_of = [&](int i) { return len16[i]; };
    const int nb_all = (int)bstart.size() - 1;
    // The output arrays of a pipeline are pitched (clips x longest clip x max_symbols).  With the clips sorted longest first, one very long
    // file in front of many short ones would make every batch of the call carry its pitch (a 1 h file and 256 short clips: ~0.5 GB per array,
    // per slot and decode group, copied and zeroed per batch -- round-4 advisor finding).  So the batch list is cut into SEGMENTS, each run
    // through the pipeline sized for its own longest clip: a new segment starts where the clips have become four times shorter than the
    // segment's first AND the segment's token arrays would be large.  Ordinary calls (10 s .. a few minutes per clip) are one segment.
    const int sym = m.cfg.max_symbols_per_step > 0 ? m.cfg.max_symbols_per_step : 10;
    auto frames_of = [&](int64_t n) { return (int64_t)pk_encoder_num_frames(pk_mel_num_frames(n)); };
    std::vector<int32_t> ids, st, en, lens;
    std::vector<float> cf;
    for (int kseg = 0; kseg < nb_all;) {
    const int seg0 = kseg;
    int64_t cap_total = 0;
    int cap_clips = 0;
    const int64_t seg_T = frames_of(len_of(bstart[seg0]));
    for (; kseg < nb_all; ++kseg) {
        const int nc = bstart[kseg + 1] - bstart[kseg];
        if (kseg > seg0 && len_of(bstart[kseg]) * 4 <= len_of(bstart[seg0]) &&
            (size_t)std::max(cap_clips, nc) * seg_T * sym * 4 * 4 > kTokenShrinkBytes / 8) break;
        int64_t tot = 0;
        for (int i = bstart[kseg]; i < bstart[kseg + 1]; ++i) tot += len_of(i);
        cap_total = std::max(cap_total, tot);
        cap_clips = std::max(cap_clips, nc);
    }
    const int nb = kseg - seg0;                                    // batches seg0 .. kseg-1 run as one pipeline pass
    pk_batch *b = model_pipeline(m, cap_clips, cap_total, len_of(bstart[seg0]));
    try {
        batch_set_group(b, (decoder == PK_DECODER_TDT && nb >= 4) ? 4 : 1);
        const int64_t first_seq = b->runs;
        const int mt = b->ws[0].max_tokens;
        std::vector<char> taken(nb, 0);
        std::vector<int64_t> blens, braw;
        const int *bs = bstart.data() + seg0;                      // (the lambdas below index the segment's batches 0 .. nb-1)
        auto stage = [&](int k) {
            const int c0 = bs[k], nc = bs[k + 1] - c0;
            blens.resize(nc);
            for (int i = 0; i < nc; ++i) blens[i] = len_of(c0 + i);
            if (resampled) {
                braw.resize(nc);
                for (int i = 0; i < nc; ++i) braw[i] = span[order[c0 + i]].n;
            }
            batch_stage(b, nc, [&](int i) { return span[order[c0 + i]].p; }, blens.data(), resampled ? braw.data() : nullptr);
        };
        auto drain = [&]() {                                  // every finished run of this call that has not been handed out yet
            for (const auto &L : b->done) {
                const int64_t k = L.seq - first_seq;
                if (k < 0 || k >= nb || taken[k]) continue;
                taken[k] = 1;
                const int B = L.clips;
                const size_t tok = (size_t)B * mt;
                ids.resize(tok); lens.resize(B);
                if (ts) { st.resize(tok); en.resize(tok); cf.resize(tok); }
                PK_HIP(hipEventSynchronize(L.ev));
                copy_results(L, ids.data(), lens.data(), ts ? st.data() : nullptr, ts ? en.data() : nullptr, ts ? cf.data() : nullptr);
                for (int i = 0; i < B; ++i) {
                    const int c = order[bs[k] + i];
                    if (lens[i] < 0) fail(PK_ERR_DECODE_CAP, "TDT decode hit the safety cap on clip %d", c);
                    const size_t o0 = (size_t)i * mt;
                    store_tokens(m, R, c, lens[i], ids.data() + o0, ts ? st.data() + o0 : nullptr, ts ? en.data() + o0 : nullptr, ts ? cf.data() + o0 : nullptr);
                }
            }
        };
        stage(0);
        for (int k = 0; k < nb; ++k) {
            batch_run(b, decoder);                               // encoder(k) queued, then decode(k-1) / the finished group driven under it
            if (k + 1 < nb) stage(k + 1);
            drain();
        }
        batch_flush(b);
        drain();
        for (int k = 0; k < nb; ++k)
            if (!taken[k]) fail(PK_ERR_HIP, "internal: batch %d of the pipeline produced no result", seg0 + k);
    } catch (...) {
        batch_reset(b);
        throw;
    }
    }   // segments
}

ResultStorePtr pk::new_store(int n_clips) {
    ResultStorePtr store(new ResultStore);
    ResultStore &R = *store;
    R.res.resize(n_clips + 1);            // one hidden trailing slot keeps the store pointer
    R.text.resize(n_clips); R.ids.resize(n_clips); R.start.resize(n_clips); R.end.resize(n_clips); R.conf.resize(n_clips);
    R.word_text.resize(n_clips); R.words.resize(n_clips);
    return store;
}
// points the pk_result array of the store at its contents
static void point_results(ResultStore &R, int n_clips, bool ts) {
    for (int c = 0; c < n_clips; ++c) {
        pk_result &r = R.res[c];
        r.text = R.text[c].c_str();
        r.n_tokens = (int32_t)R.ids[c].size();
        r.token_ids = R.ids[c].data();
        r.start_frame = ts ? R.start[c].data() : nullptr;
        r.end_frame = ts ? R.end[c].data() : nullptr;
        r.confidence = ts ? R.conf[c].data() : nullptr;
        r.n_words = (int32_t)R.words[c].size();
        r.words = R.words[c].data();
    }
}
// hands the store over to the caller as a pk_result array (freed by pk_results_free)
pk_result *pk::publish_store(ResultStorePtr store, int n_clips, bool ts) {
    ResultStore &R = *store;
    point_results(R, n_clips, ts);
    memset(&R.res[n_clips], 0, sizeof(pk_result));
    R.res[n_clips].text = reinterpret_cast<const char *>(store.get());   // back-pointer for pk_results_free
    pk_result *out = R.res.data();
    store.release();
    return out;
}

// pk_transcribe_pcm_vad behind its segmentation: the pieces (piece_clip ascending, time order inside a clip; piece_off = the piece's first
// encoder frame in its clip) go through transcribe_spans as ordinary clips, and every clip's result is its pieces' results merged in that
// order (the rule is the header's).  A piece of 256 samples or fewer is not transcribed.
pk_result *pk::transcribe_pieces(Model &m, const std::vector<ClipSpan> &piece, const std::vector<int> &piece_clip, const std::vector<int> &piece_off,
                                 int n_clips, const pk_options *opt) {
    const bool ts = opt && opt->timestamps;
    const int np = (int)piece.size();
    auto parts = new_store(np);
    std::vector<int> run;
    for (int i = 0; i < np; ++i)
        if (piece[i].n > 256) run.push_back(i);
    transcribe_spans(m, piece.data(), run, opt, *parts);
    ResultStore &P = *parts;
    auto store = new_store(n_clips);
    ResultStore &R = *store;
    for (int i = 0; i < np; ++i) {
        const int c = piece_clip[i], off = piece_off[i];
        if (!P.text[i].empty()) { if (!R.text[c].empty()) R.text[c] += ' '; R.text[c] += P.text[i]; }
        R.ids[c].insert(R.ids[c].end(), P.ids[i].begin(), P.ids[i].end());
        for (int32_t v : P.start[i]) R.start[c].push_back(v + off);
        for (int32_t v : P.end[i]) R.end[c].push_back(v + off);
        R.conf[c].insert(R.conf[c].end(), P.conf[i].begin(), P.conf[i].end());
        for (const auto &w : P.word_text[i]) R.word_text[c].push_back(w);
    }
    std::vector<size_t> nw(n_clips, 0);                            // (the words point at their strings: those are all in place first)
    for (int i = 0; i < np; ++i) {
        const int c = piece_clip[i];
        const double shift = piece_off[i] * 0.08;
        for (const pk_word &w : P.words[i]) {
            R.words[c].push_back({R.word_text[c][nw[c]].c_str(), (float)((double)w.start + shift), (float)((double)w.end + shift), w.confidence});
            ++nw[c];
        }
    }
    return publish_store(std::move(store), n_clips, ts);
}

extern "C" {

pk_status pk_plan_batches(const int64_t *n_samples, int n_clips, int32_t *batch_of_clip, int32_t *pos_in_batch, int *n_batches) {
    return guard([&] {
        need(n_samples && n_clips > 0 && batch_of_clip, "n_samples/n_clips/batch_of_clip");
        std::vector<int> order, bstart;
        plan_batches(n_samples, n_clips, order, bstart);
        for (size_t k = 0; k + 1 < bstart.size(); ++k)
            for (int i = bstart[k]; i < bstart[k + 1]; ++i) {
                batch_of_clip[order[i]] = (int32_t)k;
                if (pos_in_batch) pos_in_batch[order[i]] = i - bstart[k];
            }
        if (n_batches) *n_batches = (int)bstart.size() - 1;
    });
}

pk_status pk_ragged_extents(const int64_t *n_samples, int n_clips, int32_t *n_mel_frames, int32_t *n_enc_frames, int64_t *totals) {
    return guard([&] {
        need(n_samples && n_clips > 0, "n_samples/n_clips");
        RagBatch r;
        r.build_from_samples(n_samples, n_clips, 32);
        for (int i = 0; i < n_clips; ++i) {
            if (n_mel_frames) n_mel_frames[i] = r.Tm[i];
            if (n_enc_frames) n_enc_frames[i] = r.T[i];
        }
        if (totals) { totals[0] = r.n_samples; totals[1] = r.sum_Tm; totals[2] = r.sum_H2; totals[3] = r.sum_T; totals[4] = r.n_u_att; totals[5] = r.n_u_dw; totals[6] = r.n_u_c1; }
    });
}

pk_status pk_transcribe_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt,
                            pk_result **results) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        auto store = new_store(n_clips);
        std::vector<int> all(n_clips);
        for (int i = 0; i < n_clips; ++i) all[i] = i;
        transcribe_clips(*h->m, pcm, offsets, all, opt, *store);
        *results = publish_store(std::move(store), n_clips, opt && opt->timestamps);
    });
}

}  // extern "C"

namespace {

// The batch loop of every one-call entry point that works on the encoder's rows: the call's clips in the packing of
// pk_transcribe_pcm (plan_batches: longest first, <= 256 clips / 8192 rows per batch), every batch from PCM to the encoder output m.ws.x and,
// with ctc, the log-softmax rows of the CTC head, left on the device in m.ws.ctc_lp (packed; extents in r and m.ws.rv.seq).  Per batch of nc
// clips, clip[i] being the caller's index of the batch's clip i:
//   prepare(clip, nc)   false: the batch is skipped before it is encoded;
//   sized(r, nc)        runs once the extents are known and before anything is allocated or queued: the head's plan refuses here;
//   body(clip, nc, r)   the head on the encoded rows; results go to the caller's slots clip[i].
template <class Prepare, class Sized, class Body>
void for_each_batch(Model &m, const float *pcm, const int64_t *offsets, int n_clips, bool ctc, Prepare prepare, Sized sized, Body body) {
    const bool resampled = m.input_rate != kModelRate;            // input-rate PCM: planned by the resampled lengths, as in transcribe_clips
    std::vector<int64_t> clip_len(n_clips), blens, braw;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t raw = offsets[i + 1] - offsets[i];
        clip_len[i] = resampled ? resample_length(raw, m.input_rate, kModelRate) : raw;
    }
    std::vector<int> order, bstart;
    plan_batches(clip_len.data(), n_clips, order, bstart);
    for (size_t k = 0; k + 1 < bstart.size(); ++k) {
        const int *clip = order.data() + bstart[k];
        const int nc = bstart[k + 1] - bstart[k];
        if (!prepare(clip, nc)) continue;
        blens.resize(nc);
        for (int i = 0; i < nc; ++i) blens[i] = clip_len[clip[i]];
        const int64_t longest = blens[0];
        RagBatch r;
        r.build_from_samples(blens.data(), nc, att_block_rows_of(m, pk_encoder_num_frames(pk_mel_num_frames(longest))));
        sized(r, nc);
        m.ws.size_ragged(m.cfg, nc, r.n_samples, longest, /*own_pcm=*/true);
        m.ws.set_ragged(r, m.stream);
        if (resampled) {
            braw.resize(nc);
            for (int i = 0; i < nc; ++i) braw[i] = offsets[clip[i] + 1] - offsets[clip[i]];
            resample_stage(m.rs, m.input_rate, kModelRate, nc, [&](int i) { return pcm + offsets[clip[i]]; }, braw.data(), r.pcm_off.data(), m.ws.pcm.as<float>(),
                           m.stream);
        } else for (int i = 0; i < nc; ++i)
            PK_HIP(hipMemcpyAsync(m.ws.pcm.as<float>() + r.pcm_off[i], pcm + offsets[clip[i]], (size_t)blens[i] * 4, hipMemcpyHostToDevice, m.stream));
        m.run_mel_ws(m.ws, m.ws.pcm.as<float>(), nc, m.stream);
        m.run_encoder(m.ws, m.ws.feats.as<float>(), nc, 0, -1, 0, m.stream);
        if (ctc) m.run_ctc(m.ws, m.ws.x.as<float>(), nc, r.T_max, true, m.stream);
        body(clip, nc, r);
    }
}
const auto every_batch = [](const int *, int) { return true; };
const float NEGF = -__builtin_huge_valf();

struct BeamHost {             // a batch's search output on the host: nc * N slots of `pitch` tokens; an unfilled slot has score -inf
    std::vector<int32_t> ids, lens, st, en;
    std::vector<float> sc, cf, lms;
    size_t pitch = 0;
    bool ts = false;
    void size(size_t slots, size_t pitch_, bool ts_) {
        pitch = pitch_; ts = ts_;
        ids.resize(slots * pitch); lens.resize(slots); sc.resize(slots); lms.assign(slots, 0.0f);
        if (ts) { st.resize(slots * pitch); en.resize(slots * pitch); cf.resize(slots * pitch); }
    }
    int32_t *start() { return ts ? st.data() : nullptr; }
    int32_t *end() { return ts ? en.data() : nullptr; }
    float *conf() { return ts ? cf.data() : nullptr; }
};

struct NbestStore {           // owns everything a pk_nbest array points into
    std::vector<pk_nbest> out;                              // one hidden trailing slot keeps the store pointer
    std::vector<ResultStorePtr> clip;                       // the hypotheses of one clip: a ResultStore of n_hyp results
    std::vector<std::vector<float>> score;
    int N = 0;                                              // the n_best of the search that filled it (pk_nbest_rescore_nlm pitches its outputs by it)
    explicit NbestStore(int n_clips) : out((size_t)n_clips + 1), clip(n_clips), score(n_clips) {}
    // Clip c of the call gets the filled ones of the N slots of the batch's clip i (they come first): position j of its list is slot ord[j],
    // scored ranked[ord[j]].  Returns their number.
    int fill(Model &m, int c, int i, int N, BeamHost &h, const int32_t *ord, const float *ranked) {
        const size_t hy0 = (size_t)i * N;
        this->N = N;
        int nh = 0;
        while (nh < N && h.sc[hy0 + nh] > NEGF) ++nh;
        clip[c] = new_store(nh);
        ResultStore &R = *clip[c];
        score[c].resize(nh);
        for (int j = 0; j < nh; ++j) {
            const size_t hy = hy0 + ord[j], o0 = hy * h.pitch;
            score[c][j] = ranked[ord[j]];
            store_tokens(m, R, j, h.lens[hy], h.ids.data() + o0, h.ts ? h.st.data() + o0 : nullptr, h.ts ? h.en.data() + o0 : nullptr,
                         h.ts ? h.cf.data() + o0 : nullptr);
        }
        point_results(R, nh, h.ts);
        out[c].n_hyp = nh;
        out[c].hyp = R.res.data();
        out[c].score = score[c].data();
        return nh;
    }
    // hands the store over to the caller as a pk_nbest array (freed by pk_nbest_free)
    static pk_nbest *publish(std::unique_ptr<NbestStore> store) {
        pk_nbest &tail = store->out.back();
        tail.n_hyp = 0; tail.score = nullptr;
        tail.hyp = reinterpret_cast<const pk_result *>(store.get());     // back-pointer for pk_nbest_free
        return store.release()->out.data();
    }
};
}  // namespace

extern "C" {

// The body of pk_transcribe_pcm_nbest and pk_transcribe_pcm_nbest_rescored.  tdt_weight != nullptr: every returned hypothesis of a batch is scored
// under the TDT head on the batch's encoder rows (tdt_total.hpp; enc_proj once per batch, hypotheses of a clip share its rows) and each clip's list
// is re-ordered by rescore_order; ctc_out / tdt_out (optional, [n_clips][N]) take the parts in the returned order.
// fused: the body of pk_transcribe_pcm_nbest_lm too: the search runs with the language model lm (lists stay in the
// search's fused order) and lm_out (optional, [n_clips][N]) takes every returned hypothesis's LM score, 0 past n_hyp.
static void nbest_pcm(Model &m, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *opt, const float *tdt_weight,
                      pk_nbest **results, float *ctc_out, float *tdt_out, bool fused = false, const pk_lm *lm = nullptr,
                      const pk_lm_options *lm_opt = nullptr, float *lm_out = nullptr) {
    const pk_beam_options o = beam_options_of(opt);
    int V = 0, blank = 0;
    beam_model_checks(m, o, V, blank);
    LmDev lmd{};
    if (fused) {
        lm_fusion_checks(lm, lm_opt, V, blank);
        lmd = lm_device_view(lm, lm_opt);
    }
    const bool ts = o.timestamps != 0;
    const int N = o.n_best;
    auto store = std::make_unique<NbestStore>(n_clips);
    BeamHost h;
    std::vector<int32_t> hids, hoff, hclip, hslot, okv, ord;
    std::vector<float> tt, comb;
    for_each_batch(m, pcm, offsets, n_clips, /*ctc=*/true, every_batch, [](const RagBatch &, int) {}, [&](const int *clip, int nc, const RagBatch &r) {
        const int T = r.T_max;
        run_ctc_beam(m.beam, m.ws.ctc_lp.as<float>(), nc, T, r.sum_T, m.ws.rv.seq, V, blank, o, m.stream, fused ? &lmd : nullptr);
        PK_CHECK_LAUNCH();
        const size_t hyps = (size_t)nc * N;
        h.size(hyps, T, ts);
        beam_copy_out(m.beam, h.ids.data(), h.lens.data(), h.sc.data(), h.start(), h.end(), h.conf(), m.stream, fused ? h.lms.data() : nullptr);
        if (tdt_weight) {
            // the filled slots of the batch as one packed call of the total: hypothesis (i, j) on the rows of the batch's clip i
            hids.clear(); hoff.assign(1, 0); hclip.clear(); hslot.clear();
            for (int i = 0; i < nc; ++i)
                for (int j = 0; j < N && h.sc[(size_t)i * N + j] > NEGF; ++j) {
                    const size_t hy = (size_t)i * N + j;
                    hids.insert(hids.end(), h.ids.begin() + hy * T, h.ids.begin() + hy * T + h.lens[hy]);
                    hoff.push_back((int32_t)hids.size()); hclip.push_back(i); hslot.push_back((int32_t)hy);
                }
            tt.assign(hyps, NEGF); okv.assign(hyps, 0);
            const int nh_all = (int)hclip.size();
            if (nh_all > 0) {
                hids.push_back(0);                              // (never read: keeps data() valid when every hypothesis is empty)
                // the total's limits (1535 tokens, the scratch cap) depend on the search's output: this is the earliest they can be checked (header)
                align_check_args(hids.data(), hoff.data(), nh_all, m.cfg.vocab_size, m.cfg.blank_id);
                tdt_total_plan_call(m, m.ttotal, r.T.data(), nc, 0, hoff.data(), hclip.data(), nh_all);
                m.run_enc_proj(m.ws.x.as<float>(), r.sum_T, m.ws.ep.as<float>(), m.stream);
                run_tdt_total_call(m, m.ttotal, m.ws.ep.as<float>(), hids.data(), hoff.data());
                PK_CHECK_LAUNCH();
                for (int q = 0; q < nh_all; ++q) { tt[hslot[q]] = m.ttotal.total[q]; okv[hslot[q]] = m.ttotal.ok[q]; }
            }
        }
        for (int i = 0; i < nc; ++i) {
            const int c = clip[i];
            const size_t hy0 = (size_t)i * N;
            ord.resize(N); comb.resize(N);
            for (int j = 0; j < N; ++j) { ord[j] = j; comb[j] = h.sc[hy0 + j]; }
            if (tdt_weight) rescore_order(h.lens.data() + hy0, h.sc.data() + hy0, tt.data() + hy0, okv.data() + hy0, N, *tdt_weight, ord.data(), comb.data());
            const int nh = store->fill(m, c, i, N, h, ord.data(), comb.data());
            for (int j = 0; j < N; ++j) {                       // position j of the returned list holds the beam's slot ord[j]; the nh filled slots come first
                const size_t hy = hy0 + ord[j];
                if (ctc_out) ctc_out[(size_t)c * N + j] = j < nh ? h.sc[hy] : NEGF;
                if (tdt_out) tdt_out[(size_t)c * N + j] = j < nh ? tt[hy] : NEGF;
                if (lm_out) lm_out[(size_t)c * N + j] = j < nh ? h.lms[hy] : 0.0f;
            }
        }
    });
    *results = NbestStore::publish(std::move(store));
}

pk_status pk_transcribe_pcm_nbest(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *opt,
                                  pk_nbest **results) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        nbest_pcm(*h->m, pcm, offsets, n_clips, opt, nullptr, results, nullptr, nullptr);
    });
}

pk_status pk_transcribe_pcm_nbest_lm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *opt,
                                     pk_nbest **results, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        nbest_pcm(*h->m, pcm, offsets, n_clips, opt, nullptr, results, nullptr, nullptr, true, lm, lm_opt, lm_score);
    });
}

pk_status pk_transcribe_pcm_nbest_rescored(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *beam_opt,
                                           const pk_rescore_options *rescore_opt, pk_nbest **results, float *ctc_score, float *tdt_total) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        Model &m = *h->m;
        const float w = rescore_opt ? rescore_opt->tdt_weight : 0.5f;
        need(w == w && w > -__builtin_huge_valf() && w < __builtin_huge_valf(), "tdt_weight must be finite");
        if (m.cfg.ctc_vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no ctc_decoder_ head: the rescored n-best needs the CTC head for the search");
        tdt_align_model_checks(m);
        if (m.cfg.ctc_vocab_size != m.cfg.vocab_size)
            fail(PK_ERR_UNSUPPORTED, "the CTC head (%d) and the TDT head (%d) of this model do not share a vocabulary", m.cfg.ctc_vocab_size, m.cfg.vocab_size);
        nbest_pcm(m, pcm, offsets, n_clips, beam_opt, &w, results, ctc_score, tdt_total);
    });
}

// The body of pk_transcribe_pcm_nbest_tdt: the batches of pk_transcribe_pcm_nbest; every batch is searched through the TDT head (tdt_beam.hpp) on
// its encoder rows, enc_proj once per batch.  fused: pk_transcribe_pcm_nbest_tdt_lm (lm must be given), lists in fused
// order and lm_out [n_clips][N] beside them; else lm / lm_opt / lm_out are not looked at.
static void nbest_tdt_pcm(Model &m, const float *pcm, const int64_t *offsets, int n_clips, const pk_tdt_beam_options *opt, bool ts, pk_nbest **results,
                          bool fused = false, const pk_lm *lm = nullptr, const pk_lm_options *lm_opt = nullptr, float *lm_out = nullptr) {
    const pk_tdt_beam_options o = tdt_beam_options_of(opt);
    tdt_beam_model_checks(m, o);
    if (fused) lm_fusion_checks(lm, lm_opt, m.cfg.vocab_size, m.cfg.blank_id);
    m.require_gpu();
    LmDev lmd{};
    bool have_lmd = false;                                     // the device copy is made after the first batch's plan: a refusal allocates nothing
    const int N = o.n_best;
    auto store = std::make_unique<NbestStore>(n_clips);
    BeamHost h;
    std::vector<int32_t> identity(N);
    for (int j = 0; j < N; ++j) identity[j] = j;
    const int sym = m.cfg.max_symbols_per_step > 0 ? m.cfg.max_symbols_per_step : 10;
    int MT = 0;
    for_each_batch(m, pcm, offsets, n_clips, /*ctc=*/false, every_batch, [&](const RagBatch &rb, int nc) {
        MT = rb.T_max * sym;
        tdt_beam_plan(m.tbeam, m, rb.T.data(), nc, 0, o, MT, fused);            // (refuses before the batch is allocated or queued)
        if (fused && !have_lmd) { lmd = lm_device_view(lm, lm_opt); have_lmd = true; }
    }, [&](const int *clip, int nc, const RagBatch &r) {
        m.run_enc_proj(m.ws.x.as<float>(), r.sum_T, m.ws.ep.as<float>(), m.stream);
        run_tdt_beam(m, m.tbeam, m.ws.ep.as<float>(), m.stream, fused ? &lmd : nullptr);
        PK_CHECK_LAUNCH();
        h.size((size_t)nc * N, MT, ts);
        tdt_beam_copy_out(m.tbeam, h.ids.data(), h.lens.data(), h.sc.data(), h.start(), h.end(), nullptr, h.conf(), nullptr, m.stream,
                          fused ? h.lms.data() : nullptr);
        for (int i = 0; i < nc; ++i) {
            const int c = clip[i];
            const int nh = store->fill(m, c, i, N, h, identity.data(), h.sc.data() + (size_t)i * N);
            if (lm_out) for (int j = 0; j < N; ++j) lm_out[(size_t)c * N + j] = j < nh ? h.lms[(size_t)i * N + j] : 0.0f;
        }
    });
    *results = NbestStore::publish(std::move(store));
}

pk_status pk_transcribe_pcm_nbest_tdt(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_tdt_beam_options *opt,
                                      int timestamps, pk_nbest **results) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        nbest_tdt_pcm(*h->m, pcm, offsets, n_clips, opt, timestamps != 0, results);
    });
}

pk_status pk_transcribe_pcm_nbest_tdt_lm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const pk_tdt_beam_options *opt,
                                         int timestamps, pk_nbest **results, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score) {
    return guard([&] {
        need(h && pcm && offsets && results && n_clips > 0, "model/pcm/offsets/results/n_clips");
        nbest_tdt_pcm(*h->m, pcm, offsets, n_clips, opt, timestamps != 0, results, true, lm, lm_opt, lm_score);
    });
}

// pk_align_pcm / pk_tdt_align_pcm / pk_tdt_score_pcm: the transcripts of the call (texts tokenised, or the given ids checked) packed in the caller's clip order
static void align_transcripts(Model &m, int n_clips, const char *const *texts, const int32_t *ids_in, const int32_t *id_offsets_in, int V, int blank,
                              std::vector<int32_t> &all_ids, std::vector<int32_t> &all_off) {
    all_ids.clear(); all_off.assign(n_clips + 1, 0);
    if (texts) {
        need(m.tok.loaded(), "aligning text needs the model's vocabulary");
        for (int c = 0; c < n_clips; ++c) {
            need(texts[c] != nullptr, "texts[c]");
            for (int v : m.tok.encode(texts[c])) all_ids.push_back(v);
            all_off[c + 1] = (int32_t)all_ids.size();
        }
        align_check_args(all_ids.data(), all_off.data(), n_clips, V, blank);
    } else {
        align_check_args(ids_in, id_offsets_in, n_clips, V, blank);
        all_off.assign(id_offsets_in, id_offsets_in + n_clips + 1);
        all_ids.assign(ids_in, ids_in + all_off[n_clips]);
    }
}

// The body of pk_tdt_score_pcm: the batches of pk_transcribe_pcm; the transcripts of a batch's clips are scored on its encoder rows.
static void score_pcm(Model &m, const float *pcm, const int64_t *offsets, int n_clips, const std::vector<int32_t> &all_ids, const std::vector<int32_t> &all_off,
                      const int32_t *clip_of, int n_hyp, float *total, int32_t *ok) {
    std::vector<std::vector<int>> hyps_of(n_clips);
    for (int q = 0; q < n_hyp; ++q) hyps_of[clip_of ? clip_of[q] : q].push_back(q);
    std::vector<int32_t> bids, boff, bclip, bhyp, nfr;
    for_each_batch(m, pcm, offsets, n_clips, /*ctc=*/false, [&](const int *clip, int nc) {
        bids.clear(); boff.assign(1, 0); bclip.clear(); bhyp.clear();
        for (int i = 0; i < nc; ++i)
            for (int q : hyps_of[clip[i]]) {
                bids.insert(bids.end(), all_ids.begin() + all_off[q], all_ids.begin() + all_off[q + 1]);
                boff.push_back((int32_t)bids.size()); bclip.push_back(i); bhyp.push_back(q);
            }
        bids.push_back(0);
        return !bhyp.empty();                                       // (no transcript for any clip of this batch: nothing to encode)
    }, [&](const RagBatch &rb, int nc) {
        nfr.assign(rb.T.begin(), rb.T.begin() + nc);                   // (the plan refuses before the batch is encoded)
        tdt_total_plan_call(m, m.ttotal, nfr.data(), nc, 0, boff.data(), bclip.data(), (int)bhyp.size());
    }, [&](const int *, int, const RagBatch &r) {
        m.run_enc_proj(m.ws.x.as<float>(), r.sum_T, m.ws.ep.as<float>(), m.stream);
        run_tdt_total_call(m, m.ttotal, m.ws.ep.as<float>(), bids.data(), boff.data());
        PK_CHECK_LAUNCH();
        for (size_t q = 0; q < bhyp.size(); ++q) { total[bhyp[q]] = m.ttotal.total[q]; ok[bhyp[q]] = m.ttotal.ok[q]; }
    });
}

pk_status pk_tdt_score_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts, const int32_t *ids_in,
                           const int32_t *id_offsets_in, const int32_t *clip_of, int n_hyp, float *total, int32_t *ok) {
    return guard([&] {
        need(h && pcm && offsets && total && ok && n_clips > 0 && n_hyp > 0, "model/pcm/offsets/total/ok/n_clips/n_hyp");
        need(texts || id_offsets_in, "texts or ids/id_offsets");
        Model &m = *h->m;
        tdt_align_model_checks(m);
        if (clip_of) for (int q = 0; q < n_hyp; ++q) need(clip_of[q] >= 0 && clip_of[q] < n_clips, "clip_of[h] outside [0, n_clips)");
        else need(n_hyp == n_clips, "clip_of == NULL needs n_hyp == n_clips");
        std::vector<int32_t> all_ids, all_off;
        align_transcripts(m, n_hyp, texts, ids_in, id_offsets_in, m.cfg.vocab_size, m.cfg.blank_id, all_ids, all_off);
        m.require_gpu();
        score_pcm(m, pcm, offsets, n_clips, all_ids, all_off, clip_of, n_hyp, total, ok);
    });
}

// The body of pk_align_pcm and pk_tdt_align_pcm: every batch aligned through the chosen head, tokens and words stored.
static void align_pcm(Model &m, bool tdt, const float *pcm, const int64_t *offsets, int n_clips, const std::vector<int32_t> &all_ids,
                      const std::vector<int32_t> &all_off, pk_result **results, float *score, float *total, int32_t *ok) {
    const int V = m.cfg.ctc_vocab_size, blank = m.cfg.blank_id < V ? m.cfg.blank_id : V - 1;      // (CTC head only)
    auto store = new_store(n_clips);
    std::vector<int32_t> bids, boff, nfr, st, en, di, okv;
    std::vector<float> cf, sc, tt;
    for_each_batch(m, pcm, offsets, n_clips, /*ctc=*/!tdt, [&](const int *clip, int nc) {
        boff.assign(nc + 1, 0); bids.clear();
        for (int i = 0; i < nc; ++i) {
            bids.insert(bids.end(), all_ids.begin() + all_off[clip[i]], all_ids.begin() + all_off[clip[i] + 1]);
            boff[i + 1] = (int32_t)bids.size();
        }
        return true;
    }, [&](const RagBatch &rb, int nc) {
        nfr.assign(rb.T.begin(), rb.T.begin() + nc);                   // (the plans refuse before the batch is encoded)
        if (tdt) tdt_align_plan(m.talign, nfr.data(), nc, rb.T_max, boff.data(), m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden);
        else align_plan(m.align, nfr.data(), nc, rb.T_max, boff.data());
    }, [&](const int *clip, int nc, const RagBatch &r) {
        const size_t n = bids.size();
        st.assign(n + 1, 0); en.assign(n + 1, 0); di.assign(n + 1, 0); cf.assign(n + 1, 0.0f); sc.resize(nc); tt.resize(nc); okv.resize(nc);
        if (tdt) {
            tdt_lattice_upload(m.talign, bids.data(), m.stream, /*token_results=*/true);
            run_tdt_align_pred(m, m.talign, bids.data(), m.stream);
            m.run_enc_proj(m.ws.x.as<float>(), r.sum_T, m.ws.ep.as<float>(), m.stream);
            run_tdt_align_lattice(m, m.talign, m.ws.ep.as<float>(), m.stream);
            run_tdt_align_dp(m.talign, m.stream);
            PK_CHECK_LAUNCH();
            tdt_align_copy_out(m.talign, st.data(), en.data(), di.data(), cf.data(), sc.data(), okv.data(), m.stream);
        } else {
            run_ctc_align(m.align, m.ws.ctc_lp.as<float>(), nc, r.T_max, m.ws.rv.seq, V, blank, bids.data(), total != nullptr, m.stream);
            PK_CHECK_LAUNCH();
            align_copy_out(m.align, st.data(), en.data(), cf.data(), sc.data(), total ? tt.data() : nullptr, okv.data(), m.stream);
        }
        for (int i = 0; i < nc; ++i) {
            const int c = clip[i], o0 = boff[i], L = boff[i + 1] - o0;
            const bool good = okv[i] != 0;
            store_tokens(m, *store, c, L, bids.data() + o0, good ? st.data() + o0 : nullptr, good ? en.data() + o0 : nullptr, good ? cf.data() + o0 : nullptr);
            ok[c] = okv[i];
            if (score) score[c] = sc[i];
            if (total) total[c] = tt[i];
        }
    });
    pk_result *out = publish_store(std::move(store), n_clips, true);
    for (int c = 0; c < n_clips; ++c)
        if (!ok[c]) out[c].start_frame = out[c].end_frame = nullptr, out[c].confidence = nullptr;
    *results = out;
}

pk_status pk_align_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts, const int32_t *ids_in,
                       const int32_t *id_offsets_in, pk_result **results, float *score, float *total, int32_t *ok) {
    return guard([&] {
        need(h && pcm && offsets && results && ok && n_clips > 0, "model/pcm/offsets/results/ok/n_clips");
        need(texts || id_offsets_in, "texts or ids/id_offsets");
        Model &m = *h->m;
        if (m.cfg.ctc_vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no ctc_decoder_ head: CTC alignment needs one");
        const int V = m.cfg.ctc_vocab_size, blank = m.cfg.blank_id < V ? m.cfg.blank_id : V - 1;
        std::vector<int32_t> all_ids, all_off;
        align_transcripts(m, n_clips, texts, ids_in, id_offsets_in, V, blank, all_ids, all_off);
        m.require_gpu();
        align_pcm(m, false, pcm, offsets, n_clips, all_ids, all_off, results, score, total, ok);
    });
}

pk_status pk_tdt_align_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts, const int32_t *ids_in,
                           const int32_t *id_offsets_in, pk_result **results, float *score, int32_t *ok) {
    return guard([&] {
        need(h && pcm && offsets && results && ok && n_clips > 0, "model/pcm/offsets/results/ok/n_clips");
        need(texts || id_offsets_in, "texts or ids/id_offsets");
        Model &m = *h->m;
        tdt_align_model_checks(m);
        std::vector<int32_t> all_ids, all_off;
        align_transcripts(m, n_clips, texts, ids_in, id_offsets_in, m.cfg.vocab_size, m.cfg.blank_id, all_ids, all_off);
        m.require_gpu();
        align_pcm(m, true, pcm, offsets, n_clips, all_ids, all_off, results, score, nullptr, ok);
    });
}

}  // extern "C"

// The body of pk_spot_pcm and pk_tdt_spot_pcm: the keywords (phrases or ids), the batches of pk_transcribe_pcm, the head's spotting on every batch's
// rows, frames to seconds.  tdt: through the TDT head (tdt_kws.hpp) instead of the CTC head's log-probs.
static void spot_pcm(Model &m, bool tdt, const float *pcm, const int64_t *offsets, int n_clips, const char *const *phrases, const int32_t *ids_in,
                     const int32_t *kw_offsets_in, int n_kw, const pk_kws_options *opt, int32_t *n_hits, float *start_s, float *end_s, float *score) {
    const char *what = tdt ? "TDT keyword spotting" : "CTC keyword spotting";
    const int V = tdt ? m.cfg.vocab_size : m.cfg.ctc_vocab_size, blank = m.cfg.blank_id < V ? m.cfg.blank_id : V - 1;
    const pk_kws_options o = kws_options_of(opt);
    std::vector<int32_t> ids, off;                             // the keywords, packed; the same for every batch
    if (phrases) {
        need(n_kw >= 1, "n_kw");
        need(m.tok.loaded(), "spotting phrases needs the model's vocabulary");
        off.assign(1, 0);
        for (int k = 0; k < n_kw; ++k) {
            need(phrases[k] != nullptr, "phrases[k]");
            for (int v : m.tok.encode(phrases[k])) ids.push_back(v);
            off.push_back((int32_t)ids.size());
        }
        ids.push_back(0);                                      // (never read: keeps data() non-null for a list of empty phrases)
        kws_check_args(ids.data(), off.data(), n_kw, n_clips, V, blank, o, what);
    } else {
        kws_check_args(ids_in, kw_offsets_in, n_kw, n_clips, V, blank, o, what);
        off.assign(kw_offsets_in, kw_offsets_in + n_kw + 1);
        ids.assign(ids_in, ids_in + off[n_kw]);
    }
    m.require_gpu();
    const size_t H = (size_t)o.max_hits, per_clip = (size_t)n_kw * H;
    std::vector<int32_t> nfr, nh, st, en;
    std::vector<float> sc;
    for_each_batch(m, pcm, offsets, n_clips, /*ctc=*/!tdt, every_batch, [&](const RagBatch &rb, int nc) {
        nfr.assign(rb.T.begin(), rb.T.begin() + nc);                                // (the plan refuses before the batch is encoded)
        if (tdt) tdt_kws_plan_call(m.tkws, m.cfg.durations, m.cfg.num_durations, m.cfg.vocab_size, m.cfg.joint_hidden, nfr.data(), nc, 0, ids.data(), off.data(),
                                   n_kw, nullptr, nullptr, nc * n_kw, o);
        else kws_plan(m.kws, nfr.data(), nc, rb.T_max, off.data(), n_kw, o);
    }, [&](const int *clip, int nc, const RagBatch &r) {
        const int32_t *bnh, *bst, *ben;
        const float *bsc;
        if (tdt) {
            m.run_enc_proj(m.ws.x.as<float>(), r.sum_T, m.ws.ep.as<float>(), m.stream);
            run_tdt_kws_call(m, m.tkws, m.ws.ep.as<float>(), ids.data(), off.data());
            PK_CHECK_LAUNCH();
            bnh = m.tkws.n_hits.data(); bst = m.tkws.start.data(); ben = m.tkws.end.data(); bsc = m.tkws.score.data();
        } else {
            run_ctc_kws(m.kws, m.ws.ctc_lp.as<float>(), nc, r.T_max, m.ws.rv.seq, V, blank, ids.data(), m.stream);
            PK_CHECK_LAUNCH();
            nh.resize((size_t)nc * n_kw); st.resize(nc * per_clip); en.resize(nc * per_clip); sc.resize(nc * per_clip);
            kws_copy_out(m.kws, nh.data(), st.data(), en.data(), sc.data(), m.stream);
            bnh = nh.data(); bst = st.data(); ben = en.data(); bsc = sc.data();
        }
        for (int i = 0; i < nc; ++i) {
            const size_t c = (size_t)clip[i];
            for (int q = 0; q < n_kw; ++q) {
                const int n = bnh[(size_t)i * n_kw + q];
                n_hits[c * n_kw + q] = n;
                for (size_t j = 0; j < H; ++j) {
                    const size_t src = i * per_clip + q * H + j, dst = c * per_clip + q * H + j;
                    const bool hit = (int)j < n;
                    start_s[dst] = hit ? frame_to_seconds(bst[src]) : 0.0f;
                    end_s[dst] = hit ? frame_to_seconds(ben[src] + 1) : 0.0f;       // the END of the last frame
                    score[dst] = bsc[src];
                }
            }
        }
    });
}

extern "C" {

pk_status pk_spot_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const char *const *phrases, const int32_t *ids_in,
                      const int32_t *kw_offsets_in, int n_kw, const pk_kws_options *opt, int32_t *n_hits, float *start_s, float *end_s, float *score) {
    return guard([&] {
        need(h && pcm && offsets && n_hits && start_s && end_s && score && n_clips > 0, "model/pcm/offsets/n_hits/start_s/end_s/score/n_clips");
        need(phrases || (ids_in && kw_offsets_in), "phrases or ids/kw_offsets");
        Model &m = *h->m;
        if (m.cfg.ctc_vocab_size <= 0) fail(PK_ERR_UNSUPPORTED, "this model has no ctc_decoder_ head: CTC keyword spotting needs one");
        spot_pcm(m, false, pcm, offsets, n_clips, phrases, ids_in, kw_offsets_in, n_kw, opt, n_hits, start_s, end_s, score);
    });
}

pk_status pk_tdt_spot_pcm(pk_model *h, const float *pcm, const int64_t *offsets, int n_clips, const char *const *phrases, const int32_t *ids_in,
                          const int32_t *kw_offsets_in, int n_kw, const pk_kws_options *opt, int32_t *n_hits, float *start_s, float *end_s, float *score) {
    return guard([&] {
        need(h && pcm && offsets && n_hits && start_s && end_s && score && n_clips > 0, "model/pcm/offsets/n_hits/start_s/end_s/score/n_clips");
        need(phrases || (ids_in && kw_offsets_in), "phrases or ids/kw_offsets");
        Model &m = *h->m;
        tdt_align_model_checks(m);
        spot_pcm(m, true, pcm, offsets, n_clips, phrases, ids_in, kw_offsets_in, n_kw, opt, n_hits, start_s, end_s, score);
    });
}

// Re-ranking of n-best lists with the Transformer LM (neural_lm.hpp; the rule is the header's): every hypothesis of the call scored in ONE packed
// pk_nlm_score, then each clip's slots permuted in the store -- the pk_result structs (pointers into per-slot vectors that stay where they are) and
// the scores.
pk_status pk_nbest_rescore_nlm(pk_nbest *results, int n_clips, pk_nlm *nlm, const pk_nlm_rescore_options *opt, float *am_score, float *nlm_score) {
    return guard([&] {
        need(results && nlm && n_clips > 0, "results/nlm/n_clips");
        const float alpha = opt ? opt->alpha : 0.5f, beta = opt ? opt->beta : 0.0f;
        need(alpha == alpha && beta == beta, "options: alpha / beta must not be NaN");
        NbestStore &S = *reinterpret_cast<NbestStore *>(const_cast<pk_result *>(results[n_clips].hyp));
        need(S.out.data() == results && (int)S.clip.size() == n_clips, "results / n_clips: not a list of the n-best entry points");
        const int N = S.N;
        std::vector<int32_t> ids, off(1, 0);
        for (int c = 0; c < n_clips; ++c)
            for (int j = 0; j < results[c].n_hyp; ++j) {
                const pk_result &r = results[c].hyp[j];
                ids.insert(ids.end(), r.token_ids, r.token_ids + r.n_tokens);
                off.push_back((int32_t)ids.size());
            }
        const int nh_all = (int)off.size() - 1;
        ids.push_back(0);                                        // (never read: keeps data() valid when every hypothesis is empty)
        std::vector<float> tot(nh_all + 1);
        std::vector<int32_t> okv(nh_all + 1);
        nlm->lm->score(ids.data(), off.data(), nh_all, tot.data(), okv.data(), nullptr);   // (refuses bad ids before any list is touched)
        const bool identity = alpha == 0.0f && beta == 0.0f;
        std::vector<int32_t> ord, lens;
        std::vector<float> comb, am;
        std::vector<pk_result> tmp;
        int q0 = 0;
        for (int c = 0; c < n_clips; ++c) {
            const int nh = results[c].n_hyp;
            ord.resize(nh); lens.resize(nh); comb.resize(nh); am.assign(S.score[c].begin(), S.score[c].end());
            for (int j = 0; j < nh; ++j) lens[j] = results[c].hyp[j].n_tokens;
            nlm_order(am.data(), tot.data() + q0, lens.data(), okv.data() + q0, nh, alpha, beta, ord.data(), comb.data());
            if (!identity) {
                ResultStore &R = *S.clip[c];
                tmp.assign(R.res.begin(), R.res.begin() + nh);
                for (int j = 0; j < nh; ++j) { R.res[j] = tmp[ord[j]]; S.score[c][j] = comb[ord[j]]; }
            }
            for (int j = 0; j < N; ++j) {
                if (am_score) am_score[(size_t)c * N + j] = j < nh ? am[ord[j]] : NEGF;
                if (nlm_score) nlm_score[(size_t)c * N + j] = j < nh ? tot[q0 + ord[j]] : NEGF;
            }
            q0 += nh;
        }
    });
}

void pk_nbest_free(pk_nbest *results, int n_clips) {
    if (!results || n_clips < 0) return;
    delete reinterpret_cast<NbestStore *>(const_cast<pk_result *>(results[n_clips].hyp));
}

void pk_results_free(pk_result *results, int n_clips) {
    if (!results || n_clips < 0) return;
    delete reinterpret_cast<ResultStore *>(const_cast<char *>(results[n_clips].text));
}

}  // extern "C"
