// parakeet.cpp_amd/csrc/ctc_beam.cpp -- launches the three kernels of the CTC prefix beam search and owns their scratch.
#include "ctc_beam.hpp"

#include <algorithm>

namespace pk {

void beam_check_options(const pk_beam_options &opt, int V, int blank) {
    if (opt.beam_width < 1 || opt.beam_width > kBeamMaxWidth) fail(PK_ERR_INVALID, "beam_width %d outside 1..%d", opt.beam_width, kBeamMaxWidth);
    if (opt.token_prune < 1 || opt.token_prune > kBeamMaxPrune) fail(PK_ERR_INVALID, "token_prune %d outside 1..%d", opt.token_prune, kBeamMaxPrune);
    if (opt.n_best < 1 || opt.n_best > opt.beam_width) fail(PK_ERR_INVALID, "n_best %d outside 1..beam_width (%d)", opt.n_best, opt.beam_width);
    if (V < 2 || V > kBeamMaxVocab) fail(PK_ERR_INVALID, "vocabulary of %d entries outside 2..%d", V, kBeamMaxVocab);
    if (blank < 0 || blank >= V) fail(PK_ERR_INVALID, "blank id %d outside the vocabulary of %d", blank, V);
}

void run_ctc_beam(BeamWs &ws, const float *d_lp, int B, int T, int64_t rows, const SeqRag &rag, int V, int blank, const pk_beam_options &opt,
                  hipStream_t s, const LmDev *lm) {
    beam_check_options(opt, V, blank);
    const int W = opt.beam_width, K = std::min(opt.token_prune, V - 1), N = opt.n_best;
    const bool ts = opt.timestamps != 0;
    const size_t hyps = (size_t)B * N, tok = hyps * T;
    const size_t bp_pitch = (size_t)T * (2 * (size_t)T + 1);
    if (ts) {
        if (T > kBeamAlignMaxFrames)
            fail(PK_ERR_UNSUPPORTED, "beam search timestamps: %d frames exceed the alignment's cap of %d (search without timestamps has none)", T,
                 kBeamAlignMaxFrames);
        if (hyps * bp_pitch > kBeamAlignMaxScratch)
            fail(PK_ERR_UNSUPPORTED, "beam search timestamps: %zu hypotheses of %d frames need %zu bytes of back-pointers, the cap is %zu", hyps, T,
                 hyps * bp_pitch, kBeamAlignMaxScratch);
    }
    const int64_t node_pitch = (int64_t)T * W + 1;
    ws.tk_val.reserve((size_t)rows * K * 4); ws.tk_id.reserve((size_t)rows * K * 4); ws.lpb.reserve((size_t)rows * 4);
    ws.nodes.reserve((size_t)B * node_pitch * sizeof(int2));
    ws.hyp.reserve(hyps * 3 * 4);
    ws.ids.reserve(tok * 4); ws.lens.reserve(hyps * 4);
    PK_HIP(hipMemsetAsync(ws.ids.p, 0, tok * 4, s));
    if (ts) {
        ws.bp.reserve(hyps * bp_pitch);
        ws.start.reserve(tok * 4); ws.end.reserve(tok * 4); ws.conf.reserve(tok * 4);
        PK_HIP(hipMemsetAsync(ws.start.p, 0, tok * 4, s));
        PK_HIP(hipMemsetAsync(ws.end.p, 0, tok * 4, s));
        PK_HIP(hipMemsetAsync(ws.conf.p, 0, tok * 4, s));
    }
    ws.B = B; ws.N = N; ws.pitch = T;
    launch_ctc_beam_topk(d_lp, rows, V, blank, K, ws.tk_val.as<float>(), ws.tk_id.as<int>(), ws.lpb.as<float>(), s);
    BeamWalkArgs wa{};
    wa.tk_val = ws.tk_val.as<float>(); wa.tk_id = ws.tk_id.as<int>(); wa.lpb = ws.lpb.as<float>();
    wa.B = B; wa.T = T; wa.W = W; wa.K = K; wa.N = N;
    wa.nodes = ws.nodes.as<int2>(); wa.node_pitch = node_pitch;
    wa.hyp_node = ws.hyp.as<int>(); wa.hyp_len = wa.hyp_node + hyps; wa.hyp_score = reinterpret_cast<float *>(wa.hyp_len + hyps);
    wa.rg = rag;
    if (lm) {
        ws.hyp_lm.reserve(hyps * 4);
        BeamLmWalkArgs la{};
        la.w = wa; la.lm = *lm; la.hyp_lm = ws.hyp_lm.as<float>();
        launch_ctc_beam_lm_walk(la, s);
    } else {
        launch_ctc_beam_walk(wa, s);
    }
    BeamAlignArgs aa{};
    aa.lp = d_lp; aa.V = V; aa.blank = blank;
    aa.nodes = wa.nodes; aa.node_pitch = node_pitch;
    aa.hyp_node = wa.hyp_node; aa.hyp_len = wa.hyp_len;
    aa.B = B; aa.T = T; aa.N = N; aa.pitch = T;
    aa.timestamps = ts ? 1 : 0;
    aa.ids = ws.ids.as<int>(); aa.lens = ws.lens.as<int>();
    aa.start = ts ? ws.start.as<int>() : nullptr; aa.end = ts ? ws.end.as<int>() : nullptr; aa.conf = ts ? ws.conf.as<float>() : nullptr;
    aa.bp = ts ? ws.bp.as<unsigned char>() : nullptr; aa.bp_pitch = (int64_t)bp_pitch;
    aa.rg = rag;
    launch_ctc_beam_align(aa, s);
}

void beam_copy_out(const BeamWs &ws, int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, hipStream_t s,
                   float *lm_score) {
    const size_t hyps = (size_t)ws.B * ws.N, tok = hyps * ws.pitch;
    if (ids) PK_HIP(hipMemcpyAsync(ids, ws.ids.p, tok * 4, hipMemcpyDeviceToHost, s));
    if (lens) PK_HIP(hipMemcpyAsync(lens, ws.lens.p, hyps * 4, hipMemcpyDeviceToHost, s));
    if (score) PK_HIP(hipMemcpyAsync(score, ws.score(), hyps * 4, hipMemcpyDeviceToHost, s));
    if (lm_score) PK_HIP(hipMemcpyAsync(lm_score, ws.hyp_lm.p, hyps * 4, hipMemcpyDeviceToHost, s));
    if (start) PK_HIP(hipMemcpyAsync(start, ws.start.p, tok * 4, hipMemcpyDeviceToHost, s));
    if (end) PK_HIP(hipMemcpyAsync(end, ws.end.p, tok * 4, hipMemcpyDeviceToHost, s));
    if (conf) PK_HIP(hipMemcpyAsync(conf, ws.conf.p, tok * 4, hipMemcpyDeviceToHost, s));
    PK_HIP(hipStreamSynchronize(s));
}

}  // namespace pk
