// parakeet.cpp_amd/csrc/capi_util.hpp -- what the translation units of the extern "C" boundary share (capi*.cpp, stream.cpp, sortformer.cpp,
// frontend.cpp, transformer.cpp): the exception -> status translation, the argument check, and the few helpers that cross the capi*.cpp files.
#pragma once
#include <functional>
#include <memory>

#include "engine.hpp"

namespace pk {

const std::string &last_error();
void read_wav(const std::string &path, std::vector<float> &mono, int &sample_rate, int *n_channels = nullptr);
void parse_wav(const uint8_t *bytes, size_t n_bytes, const char *what, std::vector<float> &mono, int &sample_rate, int *n_channels, bool info_only, size_t file_len = 0);
size_t wav_info_frames();
void sinc_resample(const float *input, size_t input_len, int src_rate, int dst_rate, std::vector<float> &output);

// Every entry point runs under guard: pk::Error / std::exception become a status code + the thread-local message.
inline pk_status guard(const std::function<void()> &fn) {
    try {
        fn();
        return PK_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return PK_ERR_INVALID;
    }
}

inline void need(bool ok, const char *what) {
    if (!ok) fail(PK_ERR_INVALID, "invalid argument: %s", what);
}

inline void need_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) fail(PK_ERR_NO_DEVICE, "no HIP device available (this engine has no CPU path)");
}

// Token arrays come back as whole [B][pitch] blocks; the device only writes the first lens[b] entries of a row.  Zero the rest
// on the host so that a caller comparing / hashing whole arrays sees deterministic contents (never stale device memory).
template <class T>
void zero_tail(T *a, const int32_t *lens, int B, int pitch) {
    if (!a) return;
    for (int b = 0; b < B; ++b) {
        const int n = lens[b] < 0 ? 0 : (lens[b] < pitch ? lens[b] : pitch);
        for (int i = n; i < pitch; ++i) a[(size_t)b * pitch + i] = T(0);
    }
}

// rows of one attention block in a ragged batch whose longest utterance has T_max encoder frames
inline int att_block_rows_of(Model &m, int T_max) {
    return m.attn_bf16(T_max) ? relpos_attention_bf16_block_rows(m.cfg.hidden_size / m.cfg.num_heads) : 32;
}

// capi.cpp
std::vector<std::vector<int>> encode_phrases(Model &m, const char *const *phrases, int n);

// capi_stages.cpp: the options of the CTC beam entry points, and what they refuse for a model (-> its CTC vocabulary and blank)
pk_beam_options beam_options_of(const pk_beam_options *opt);
void beam_model_checks(Model &m, const pk_beam_options &o, int &V, int &blank);

// capi_lm.cpp: what the fused CTC beam entry points refuse about a language model for a vocabulary of V entries (host only: lm NULL, non-finite
// weights, ids outside the vocabulary, the blank, missing coverage; PK_ERR_INVALID), and the model's arrays on the current device (uploaded on
// first use there) with the weights of opt (NULL: the defaults).
void lm_fusion_checks(const pk_lm *lm, const pk_lm_options *opt, int V, int blank);
LmDev lm_device_view(const pk_lm *lm, const pk_lm_options *opt);
int lm_num_states(const pk_lm *lm);         // the states of the automaton: what a carried LM state may index (capi_diag.cpp)

// capi_batch.cpp: the one-call transcription of some clips of a call through the model's pipeline, used by every rank of a pk_group too.
// ResultStore owns everything a pk_result array points into; only capi_batch.cpp sees inside it.
struct ResultStore;
struct ResultStoreDelete { void operator()(ResultStore *s) const; };
using ResultStorePtr = std::unique_ptr<ResultStore, ResultStoreDelete>;
ResultStorePtr new_store(int n_clips);
void transcribe_clips(Model &m, const float *pcm, const int64_t *offsets, const std::vector<int> &clips, const pk_options *opt, ResultStore &R);
pk_result *publish_store(ResultStorePtr store, int n_clips, bool ts);   // hands the store to the caller (pk_results_free)
// ... of clips anywhere in host memory (span[c] for every c in `clips`), and of the pieces a segmentation cut n_clips clips into, merged per clip
struct ClipSpan { const float *p = nullptr; int64_t n = 0; };
void transcribe_spans(Model &m, const ClipSpan *span, const std::vector<int> &clips, const pk_options *opt, ResultStore &R);
pk_result *transcribe_pieces(Model &m, const std::vector<ClipSpan> &piece, const std::vector<int> &piece_clip, const std::vector<int> &piece_off,
                             int n_clips, const pk_options *opt);

}  // namespace pk
