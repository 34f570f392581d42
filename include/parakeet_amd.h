/*
 * include/parakeet_amd.h -- C ABI of the MI355X-native Parakeet hot path
 * (libparakeet_amd.so, built from parakeet.cpp_amd/csrc by hipcc for gfx950).
 *
 * The reference (Frikallo/parakeet.cpp) has NO plugin / FFI interface: its
 * boundary is the header-only C++ class API in include/parakeet/transcribe.hpp,
 * which calls axiom::Tensor methods directly; a flat C API is an unchecked
 * roadmap item (README.md:518).  This header is therefore the C ABI that the
 * reference's classes would bind if they delegated their arithmetic: each entry
 * point cites the reference interface it replaces.  The source-compatible C++
 * facade (parakeet::Transcriber, TDTTranscriber, TranscribeResult, ...) that sits
 * on top of it lives in parakeet.cpp_amd/include/parakeet/ ; INTEGRATION.md shows
 * the binding a reference maintainer would add.
 *
 * Conventions: plain C types only; the caller owns every input buffer; outputs
 * are caller-allocated unless the function returns an opaque handle, which the
 * library owns until the matching *_free.  Every function returns PK_OK (0) or
 * a negative pk_status; pk_last_error() holds the message (thread-local).
 * Host pointers unless a parameter is named dev_*.  One pk_model may be used
 * from one thread at a time (the reference's objects are not thread-safe
 * either: vocab.hpp:33-35).  There is no CPU fallback: every compute entry point
 * fails with PK_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef PARAKEET_AMD_H
#define PARAKEET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pk_status;
enum {
    PK_OK = 0,
    PK_ERR_INVALID = -1,     /* bad argument / shape */
    PK_ERR_IO = -2,          /* unreadable weights / vocab / audio (reference: std::runtime_error, vocab.cpp:12-14, audio_io.cpp:271-286) */
    PK_ERR_WEIGHTS = -3,     /* missing tensor or wrong shape (the reference loads non-strict, transcribe.hpp:63; we are strict) */
    PK_ERR_NO_DEVICE = -4,   /* no usable gfx950 device / model not on the GPU */
    PK_ERR_HIP = -5,         /* HIP runtime failure */
    PK_ERR_DECODE_CAP = -6,  /* TDT loop hit the safety cap on joint evaluations (the reference has none, tdt.cpp:62-106) */
    PK_ERR_UNSUPPORTED = -7
};

/* include/parakeet/config.hpp:9-95 (EncoderConfig, PredictionConfig, JointConfig, TDTCTCConfig) flattened. */
typedef struct pk_config {
    int32_t mel_bins;              /* EncoderConfig::mel_bins            80 / 128 */
    int32_t subsampling_channels;  /* EncoderConfig::subsampling_channels 256 */
    int32_t hidden_size;           /* EncoderConfig::hidden_size          512 / 1024 */
    int32_t num_layers;            /* 17 / 24 */
    int32_t num_heads;             /* 8 */
    int32_t ffn_intermediate;      /* 2048 / 4096 */
    int32_t conv_kernel_size;      /* 9 */
    int32_t vocab_size;            /* joint label vocab incl. blank: 1025 / 8193 */
    int32_t pred_hidden;           /* 640 */
    int32_t num_lstm_layers;       /* 1 / 2 */
    int32_t joint_hidden;          /* 640 */
    int32_t num_durations;         /* TDT: 5 ; RNNT head: 0 */
    int32_t durations[8];          /* {0,1,2,3,4} */
    int32_t ctc_vocab_size;        /* 1025, or 0 when the model has no ctc_decoder_ */
    int32_t blank_id;              /* tdt.hpp:71-74 default 1024 ; 600M: vocab_size-1 (main.cpp:252) */
    int32_t max_symbols_per_step;  /* 10 */
    int32_t joint_pred_bias;       /* switch A5: 0 = drop pred_proj_.bias like the reference's Linear(bias=false) (tdt.cpp:10-11) */
    int32_t rnnt_head;             /* 1: joint has a single out_proj_ (rnnt.cpp:37-44) instead of label_/duration_proj_ */
    int32_t stft_window_centered;  /* switch A1: placement of the 400-tap Hann window in the 512-point STFT frame (audio.cpp:117-120;
                                      axiom's stft is not available).  0 (default) = left-aligned, zero-padded on the right: what the
                                      reference author's own check of the C++ features does (scripts/compare_features.py:33-37; pinned by
                                      tests/golden/ref_compare_features_seed7.npz).  1 = centred like torch.stft / NeMo. */
    int32_t gemm_bf16;             /* 0: every product is an fp32 fma chain (bit-identical to the CPU oracle).  1: the encoder-side Linear /
                                      1x1-conv products (and the CTC / enc_proj heads) take bf16 operands with fp32 accumulation on
                                      v_mfma_f32_32x32x16_bf16 -- the precision BASELINE configs[2] names for tdt-600m; the decode loop,
                                      attention scores, norms and depthwise convs stay fp32.  Needs every such K % 64 == 0.  This mode is
                                      compared with the oracle within a tolerance, never bit for bit; since round 2 it also stores the
                                      activations that exist only as GEMM operands as bf16 (the same rounded values) and evaluates SiLU /
                                      sigmoid / the attention softmax on the hardware exp2 / rcp (1 ulp fp32).  Since round 3 the offline
                                      attention (head sizes 64 / 128) and the decode loop's GEMVs also take bf16 operands
                                      (kernels/attention_bf16.hip, decode_gemv_bf16.hip); the specification of the mode is the oracle's
                                      gemm_bf16 mode.  The streaming path (pk_stream_*) and pk_transformer_* keep fp32
                                      attention and exact activations in this mode: only their Linear products and decode GEMVs change.
                                      Round 4: on a streaming model this IS the tolerance-class streaming mode -- every Linear / 1x1-conv
                                      product of a chunk on bf16 operands (kernels/gemm_smallm_bf16.hip: K split over the waves of a workgroup,
                                      the LayerNorm of a product's input folded in), specification = the oracle's Stream with gemm_bf16 = 1,
                                      compared within the bounds of tests/test_gpu_stream.py; 16 lock-step streams of
                                      nemotron-600m cost 2.4-2.5 ms per 160 ms chunk instead of 3.1-3.2. */
    char joint_prefix[32];         /* "tdt_joint_." (tdt_ctc.cpp:5-9) or "joint_." (tdt.cpp:28-32) */
    /* encoder-only uses (Sortformer's NEST encoder, src/sortformer.cpp:41-47): vocab_size = 0 loads no prediction net / joint */
    int32_t xscaling;              /* StreamingEncoderConfig::xscaling (streaming_encoder.cpp:402-406, :444-447): x *= sqrt(hidden) after subsampling */
    int32_t mel_normalize_off;     /* AudioConfig::normalize = false (audio.cpp:140): features are the raw log-mel (Sortformer, main.cpp:516) */
    char encoder_prefix[32];       /* module name of the encoder in the state dict; "" = "encoder_." ; Sortformer: "nest_encoder_." */
} pk_config;

/* make_110m_config / make_tdt_600m_config / make_rnnt_600m_config (config.hpp:77-135). name: "tdt-ctc-110m" | "tdt-600m" | "rnnt-600m" |
 * "nemotron-600m" (nemotron.hpp:31-52) | "eou-120m" (eou.hpp:34-56) -- streaming models, see pk_stream_*. */
pk_status pk_config_preset(const char *name, pk_config *out);

typedef struct pk_model pk_model;

const char *pk_version(void);
/* Copies the calling thread's last error message; returns its length. */
size_t pk_last_error(char *buf, size_t cap);
int pk_device_count(void);

/* ---- model lifetime: Transcriber::Transcriber (transcribe.hpp:59-65), to_gpu() (:68-71) ------------------ */
/* safetensors with the reference's tensor names (scripts/convert_nemo.py:98-310); vocab_path may be NULL. */
pk_status pk_model_load(const char *safetensors_path, const char *vocab_path, const pk_config *cfg, pk_model **out);
/* The same from a safetensors image in memory (copied): what a rank receives when rank 0 reads the file once and broadcasts it
 * (RCCL) instead of every rank going to storage. */
pk_status pk_model_load_buffer(const void *safetensors_image, size_t n_bytes, const char *vocab_path, const pk_config *cfg, pk_model **out);
/* Upload (packed) weights to HBM on `device` and build the execution plan.  Idempotent per device.
 * HBM use: the weights once, plus -- fp32 mode, on the first call that runs fewer than 1537 encoder rows at a time (one or a few clips,
 * every streaming session) -- a second copy of the encoder's Linear weights tiled for the small-batch kernels (0.4 GB for tdt-ctc-110m,
 * 2.4 GB for the 600M models), shared by all later calls and streams of the model. */
pk_status pk_model_to_gpu(pk_model *m, int device);
void pk_model_free(pk_model *m);
pk_status pk_model_config(const pk_model *m, pk_config *out);
/* How the TDT / RNNT greedy loop (src/tdt.cpp:62-106) is issued.  Every mode runs the SAME device functions and gives identical results
 * (tests/test_gpu_decode.py); they differ in launch structure only.  PHASES (default): one launch per phase of a symbol step (LSTM cells,
 * joint activation, heads, decision), the host polls a done-counter every 16 steps.  PERSISTENT: the whole loop in one launch, phases
 * separated by a grid barrier (needs <= 2 LSTM layers, no phrase boosting, no carried streaming state; otherwise PHASES is used).
 * GRAPH: the 16-step chunk of PHASES captured once as a hipGraph and replayed. */
enum { PK_DECODE_LOOP_PHASES = 0, PK_DECODE_LOOP_PERSISTENT = 1, PK_DECODE_LOOP_GRAPH = 2 };
pk_status pk_model_set_decode_loop(pk_model *m, int mode);
/* Limited-context ("local") self-attention of the offline encoder: each query frame i attends only to the encoder frames
 * [i - left, i + right] of its utterance (left, right >= 0; (-1, -1) = full attention, the default; anything else PK_ERR_INVALID).
 * NeMo's rel_pos_local_attn with att_context_size [L, L] is (L, L).  Attention cost and memory become linear in the clip length: no
 * length limit from the attention, no global score scratch, and a projected position table of left + right + 1 rows per layer
 * instead of 2 T - 1.  left + right must fit the band kernel's LDS score block ([32][left + right + 32]): at most 1136 / 1072 / 1008 / 1072
 * at head size 32 / 64 / 96 / 128, otherwise PK_ERR_UNSUPPORTED.  Applies to pk_encode*, pk_conformer_blocks*, pk_transcribe_* and
 * the batch API of this model; not to the streaming path, pk_transformer_* or Sortformer.  fp32 mode: bit-identical to full attention when
 * the band covers the utterance (left, right >= T - 1).  gemm_bf16 mode: the attention runs on the fp32 band kernel with a bf16 context.
 * Switching back to (-1, -1) gives exactly the results of a model that never set it.  Not to be changed while a batch is in flight. */
pk_status pk_model_set_attention_context(pk_model *m, int left, int right);
pk_status pk_model_get_attention_context(const pk_model *m, int *left, int *right);

/* ---- stage entry points (host buffers; used by the parity tests and the C++ facade) ----------------------- */
/* preprocess_audio (src/audio.cpp:100-158): n_clips clips of n_samples each -> feats[n_clips][n_frames][mel_bins],
 * n_frames = 1 + n_samples/160.  logmel (optional, may be NULL): [n_clips][mel_bins][n_frames] before normalisation. */
pk_status pk_mel(pk_model *m, const float *pcm, int n_clips, int64_t n_samples, float *feats, float *logmel);
int pk_mel_num_frames(int64_t n_samples);
int pk_encoder_num_frames(int n_mel_frames); /* floor((n-1)/2)+1 three times (encoder.cpp:208-217) */

/* FastConformerEncoder::forward (src/encoder.cpp:253-271): feats[B][Tm][mel] -> enc[B][T][hidden].
 * stop_layer / stop_stage cut the pipeline for stage-wise parity checks: run `stop_layer` full blocks, then the
 * next block up to stop_stage (0 none, 1 ffn1, 2 +attn, 3 +conv, 4 +ffn2); pass (num_layers, 0) -- or (-1, 0) -- for all. */
pk_status pk_encode(pk_model *m, const float *feats, int B, int Tm, int stop_layer, int stop_stage, float *enc);
/* ConformerBlock::forward x n_layers starting at first_layer (src/encoder.cpp:196-204, the loop at :267-269), on an encoder
 * stream x[B][T][hidden] given by the caller.  This is the boundary the reference author's own PyTorch check
 * (scripts/compare_encoder.py) cuts at: tests/golden/ holds its outputs. */
pk_status pk_conformer_blocks(pk_model *m, const float *x_in, int B, int T, int first_layer, int n_layers, float *x_out);
/* ConvSubsampling::forward only (src/encoder.cpp:219-241). */
pk_status pk_subsample(pk_model *m, const float *feats, int B, int Tm, float *out);

/* CTCDecoder::forward + ctc_greedy_decode(_with_timestamps) (src/ctc.cpp:12-25, :40-127).
 * ids/start/end/conf: [B][T] (NULL to skip the optional ones); lens[B]; logp (optional) [B][T][ctc_vocab]. */
pk_status pk_ctc_decode(pk_model *m, const float *enc, int B, int T, int32_t *ids, int32_t *lens, int32_t *start,
                        int32_t *end, float *conf, float *logp);
/* tdt_greedy_decode(_with_timestamps) (src/tdt.cpp:36-201; RNNT head: src/rnnt.cpp:56-177).
 * ids/start/end/conf: [B][max_tokens]; lens[B] (-1 if the safety cap hit); steps[B] joint evaluations (optional). */
pk_status pk_tdt_decode(pk_model *m, const float *enc, int B, int T, int max_tokens, int32_t *ids, int32_t *lens,
                        int32_t *start, int32_t *end, float *conf, int32_t *steps);

/* ---- ragged (mixed-length) forms of the stage entry points -------------------------------------------------------------------
 * The reference's roadmap item "Batch inference: pad + length-mask multiple audio files, batch through encoder and decoder" (README.md:513;
 * mask seam src/encoder.cpp:163-165) -- done by PACKING instead of padding: the B clips of a batch lie back to back along the time axis of
 * every tensor, GEMMs / LayerNorm / activations are row-wise and see one tall matrix, and the kernels that look across rows (STFT framing,
 * the stride-2 convolutions, the depthwise conv, attention with its relative-position table, the greedy decoders) take per-clip extents.
 * No padded frame is ever computed and no mask is needed; every clip's result is BIT-IDENTICAL to the same clip run alone (same fma
 * chains, same softmax extent, same zero padding at its own edges) -- tests/test_gpu_ragged.py.
 * pk_mel_ragged: clip i = pcm[offsets[i] .. offsets[i+1]) -> feats packed [sum_i Tm_i][mel_bins], Tm_i = pk_mel_num_frames(len_i); logmel
 *   (optional) per clip one [mel_bins][Tm_i] block, blocks back to back.
 * pk_encode_ragged: feats packed as above, n_mel_frames[B] -> enc packed [sum_i T_i][hidden], T_i = pk_encoder_num_frames(Tm_i).
 * pk_conformer_blocks_ragged: x packed [sum_i n_frames[i]][hidden] in and out.
 * pk_ctc_decode_ragged / pk_tdt_decode_ragged: enc packed, n_frames[B]; token arrays [B][max_i n_frames[i]] resp. [B][max_tokens] as in the
 *   uniform calls; logp (optional) packed [sum_i T_i][ctc_vocab]. */
pk_status pk_mel_ragged(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, float *feats, float *logmel);
pk_status pk_encode_ragged(pk_model *m, const float *feats, const int32_t *n_mel_frames, int B, int stop_layer, int stop_stage, float *enc);
pk_status pk_conformer_blocks_ragged(pk_model *m, const float *x_in, const int32_t *n_frames, int B, int first_layer, int n_layers, float *x_out);
pk_status pk_ctc_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, int32_t *ids, int32_t *lens, int32_t *start,
                               int32_t *end, float *conf, float *logp);
pk_status pk_tdt_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, int max_tokens, int32_t *ids, int32_t *lens,
                               int32_t *start, int32_t *end, float *conf, int32_t *steps);

/* Teacher-forced joint scores -- "TDT logits within stated fp tolerance" made checkable for a greedy decoder: the loop of
 * tdt_greedy_decode (src/tdt.cpp:62-106) on ONE utterance enc[T][hidden] with the decision of every step GIVEN (labels[k], and
 * dur_idx[k] = an index into pk_config.durations) instead of taken from the argmax, so that the state every step is scored in -- frame
 * pointer, last token, LSTM state -- is the one another implementation (the CPU oracle, the reference) was in at the same step.  A blank
 * reverts the LSTM state and advances by max(duration, 1) (:88-93); a token commits it and advances by its duration (0: same frame,
 * :95-105).  Outputs per step k < *n_done: label_logp[k][vocab_size], dur_logp[k][num_durations] = the joint's log-softmax outputs
 * (TDTJoint::forward, :15-24); either may be NULL.  *n_done = steps evaluated (< n_steps when the frame pointer left the utterance). */
pk_status pk_tdt_score(pk_model *m, const float *enc, int T, const int32_t *labels, const int32_t *dur_idx, int n_steps, float *label_logp,
                       float *dur_logp, int *n_done);

/* Early warning of the tolerance-class (bf16) mode, SURVEY.md 8(c): per utterance of the LAST pk_tdt_decode on this model, the smallest
 * (top-1 minus top-2) log-prob over all of its greedy decisions -- the label argmax (tdt.cpp:78-82) and, for TDT heads, the duration argmax
 * (:84-86: a flip there moves the frame pointer and every later token with it): how close the decode came to a different path.  A margin below the mode's numerical error marks a token that may differ from the reference.  Not produced for
 * boosted or streaming decodes. */
pk_status pk_decode_margins(pk_model *m, float *min_margin, int B);

/* ---- resident batch pipeline (device buffers; what bench.py times) ---------------------------------------- */
typedef struct pk_batch pk_batch;
enum { PK_DECODER_CTC = 0, PK_DECODER_TDT = 1 }; /* enum class Decoder (transcribe.hpp:34) */
/* A batch slot of up to max_clips clips of exactly n_samples samples, all buffers resident in HBM. */
pk_status pk_batch_create(pk_model *m, int max_clips, int64_t n_samples, pk_batch **out);
void pk_batch_free(pk_batch *b);
/* The same pipeline with RAGGED capacity: every run takes up to max_clips clips of ANY lengths (<= max_clip_samples each, <=
 * max_total_samples in all), packed -- see the ragged stage entry points above.  pk_batch_upload_ragged: clip i = pcm[offsets[i] ..
 * offsets[i+1]); a batch whose clips all have one length runs the uniform kernels.  pk_batch_run / _sync / _results* / decode groups work
 * as for uniform pipelines; the token arrays are [n_clips][pk_batch_max_tokens], pitched for the longest clip the pipeline can hold. */
pk_status pk_batch_create_ragged(pk_model *m, int max_clips, int64_t max_total_samples, int64_t max_clip_samples, pk_batch **out);
pk_status pk_batch_upload_ragged(pk_batch *b, const float *pcm, const int64_t *offsets, int n_clips);
pk_status pk_batch_upload_ragged_async(pk_batch *b, const float *pcm, const int64_t *offsets, int n_clips);
/* Host -> HBM copy of the PCM (outside bench's timed region). */
pk_status pk_batch_upload(pk_batch *b, const float *pcm, int n_clips);
/* mel -> encoder -> decode, enqueued on the batch's stream; returns without synchronising. */
/* Streams of distinct batches: copy the NEXT batch into the second PCM buffer on a copy stream while the current encoder runs
 * (no flush; the host buffer may be reused after the call returns for pageable memory, after the next call into the batch for
 * pinned memory).  The next pk_batch_run consumes it. */
pk_status pk_batch_upload_async(pk_batch *b, const float *pcm, int n_clips);
pk_status pk_batch_run(pk_batch *b, int decoder);
pk_status pk_batch_sync(pk_batch *b);
/* Token ids etc. of the last run (synchronises).  Arrays [n_clips][max_tokens]; max_tokens = pk_batch_max_tokens. */
int pk_batch_max_tokens(const pk_batch *b);
pk_status pk_batch_results(pk_batch *b, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf);
/* Results of the newest batch whose decode has FINISHED -- run k's decode is driven inside pk_batch_run(k+1) -- without flushing the
 * decode still pending: the consumer side of the pipeline (run(k+1); results_done -> batch k).  *n_clips = its clip count. */
pk_status pk_batch_results_done(pk_batch *b, int *n_clips, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf);
/* Decode groups (throughput mode of the pipeline; default 1 = decode(k) under encoder(k+1)).  With group = G the TDT / RNNT greedy loops of
 * G consecutive pk_batch_run calls are driven as ONE lock-step batch of G * n_clips utterances under the encoder of the run after them:
 * the loop of tdt_greedy_decode (src/tdt.cpp:62-106) is launch-bound -- four launches per symbol step whatever the batch -- so G runs
 * share them.  Token ids, frames and confidences of every run are unchanged (the utterances are independent); what changes is WHEN they
 * are available: after the G-th run of the group (+1), or at pk_batch_sync / pk_batch_results.  1 <= G <= 16; flushes the pipeline. */
pk_status pk_batch_set_decode_group(pk_batch *b, int group);
/* on (default): the decode loop of run k / of a finished group runs on a second, high-priority stream UNDER the encoder of the following run.
 * off: it runs on the encoder's stream, after the encoder -- no concurrency on the device.  The decode GEMVs stream the prediction-net and
 * joint weights through L2 once per symbol step (13 MB for tdt-ctc-110m, 42 MB for tdt-600m); for the large heads that traffic costs the
 * concurrently running encoder GEMMs more than the loop's own duration, so serial issue can be the faster schedule.
 * Results are identical either way.  Flushes the pipeline. */
pk_status pk_batch_set_decode_overlap(pk_batch *b, int on);
/* Results of the (back+1)-th newest run whose decode has finished (back = 0: the newest, = pk_batch_results_done), 0 <= back <
 * pk_batch_results_available().  A finished run stays readable until its buffers are recycled: without groups until the run after next is
 * issued, with groups of G until the first run of the group after next -- so the G runs of the newest decoded group are always there, and a
 * pk_batch_sync that decodes a full group and the partial group behind it keeps the runs of both.  pk_batch_set_decode_group drops the
 * runs held in group buffers: read them first. */
pk_status pk_batch_results_back(pk_batch *b, int back, int *n_clips, int32_t *ids, int32_t *lens, int32_t *start, int32_t *end, float *conf);
int pk_batch_results_available(const pk_batch *b);
/* pk_decode_margins for the (back+1)-th newest finished run of the pipeline: min_margin[n_clips of that run]. */
pk_status pk_batch_margins(pk_batch *b, int back, float *min_margin);
/* Stage timers of the last pk_batch_run_timed (ms): mel, encoder, decode, total (hipEvents on the batch stream). */
pk_status pk_batch_run_timed(pk_batch *b, int decoder, float ms[4]);
/* Raw device pointers for zero-copy producers (e.g. torch tensors): PCM [max_clips][n_samples] f32. */
void *pk_batch_dev_pcm(pk_batch *b);
void *pk_batch_stream(pk_batch *b);

/* Per-kernel timing of ONE pk_batch_run with hipEvents around every launch (slow; for the roofline object only).
 * Fills up to cap records; returns the number of distinct kernels. */
typedef struct pk_kernel_stat {
    char name[64];
    int32_t launches;
    float total_ms;
    double flops;  /* algorithmic flops of those launches (0 for memory-bound kernels) */
    double bytes;  /* algorithmic HBM bytes of those launches */
} pk_kernel_stat;
int pk_batch_profile(pk_batch *b, int decoder, pk_kernel_stat *out, int cap);

/* ---- one-call API: Transcriber::transcribe (transcribe.hpp:74-179) ---------------------------------------- */
typedef struct pk_options {     /* TranscribeOptions (transcribe.hpp:38-43) */
    int32_t decoder;            /* PK_DECODER_* */
    int32_t timestamps;
    /* boost_phrases / boost_score (transcribe.hpp:41-42): when n_boost_phrases > 0 the phrases are tokenised with the model's
     * vocabulary (ContextTrie::build, src/phrase_boost.cpp:29-37) and this call decodes boosted; 0 phrases = the model-level
     * setting of pk_set_boost_* (off by default).  boost_score is used as given (the reference's default is 5.0). */
    const char *const *boost_phrases;
    int32_t n_boost_phrases;
    float boost_score;
} pk_options;
typedef struct pk_word {        /* WordTimestamp (timestamp.hpp:18-23) */
    const char *word;
    float start, end, confidence;
} pk_word;
typedef struct pk_result {      /* TranscribeResult (transcribe.hpp:23-30) + TimestampedToken (timestamp.hpp:11-16) */
    const char *text;
    int32_t n_tokens;
    const int32_t *token_ids;
    const int32_t *start_frame; /* NULL unless options.timestamps */
    const int32_t *end_frame;
    const float *confidence;
    int32_t n_words;
    const pk_word *words;
} pk_result;
/* Clips are pcm[offsets[i] .. offsets[i+1]), of ANY lengths: they are sorted by length and packed into ragged batches (<= 256 clips, <= 8192
 * encoder rows = 655 s of audio per batch: the row count at which every GEMM of the encoder fills whole rounds of the 256 CUs) that go through
 * the two-stream pipeline; every clip's result is bit-identical to transcribing it alone.
 * results: array of n_clips pk_result, owned by the library until pk_results_free. */
pk_status pk_transcribe_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt,
                            pk_result **results);
/* The packing policy of pk_transcribe_pcm / pk_group_transcribe_pcm on its own (host logic, no GPU needed): clips of n_samples[i] samples
 * are sorted by length (longest first, stable) and cut into batches of <= 256 clips and <= 8192 encoder rows (pk_encoder_num_frames of
 * pk_mel_num_frames of the length; 65 clips of 10 s); batch_of_clip[i] = the
 * batch clip i lands in (batch 0 holds the longest clips), pos_in_batch[i] (optional) = its row in that batch. */
pk_status pk_plan_batches(const int64_t *n_samples, int n_clips, int32_t *batch_of_clip, int32_t *pos_in_batch, int *n_batches);
/* Per-clip extents of a ragged batch (host logic): mel frames pk_mel_num_frames(n), encoder frames pk_encoder_num_frames(...) of every
 * clip; totals (optional, 7 values): samples, mel frames, rows after the second stride-2 stage, encoder rows, attention row blocks,
 * depthwise-conv strips, subsampling strips of the packed batch -- what the ragged kernels' grids are sized by. */
pk_status pk_ragged_extents(const int64_t *n_samples, int n_clips, int32_t *n_mel_frames, int32_t *n_enc_frames, int64_t *totals);
void pk_results_free(pk_result *results, int n_clips);

/* ---- CTC prefix beam search with n-best output and alignment -------------------------------------------------------------
 * The reference's roadmap line "Beam search decoding -- CTC prefix beam search ... with configurable width" (README.md:494, tier 1; the gate of
 * its "N-gram LM shallow fusion" :495 and "Neural LM rescoring -- N-best reranking" :514 lines, which need an n-best list with scores).  The search, its per-frame token pruning, every tie rule and the
 * forced alignment that gives a hypothesis its timestamps are specified operation by operation in DESIGN.md section 5.5
 * (tests/ctc_beam_ref.py is that specification in Python; the device result equals it bit for bit).  All of it runs on the device
 * (kernels/ctc_beam.hip).  No phrase boost inside the beam (a language model: the _lm entry points below); pk_group and streaming sessions have no beam variant. */
typedef struct pk_beam_options {
    int32_t beam_width;         /* W: prefixes kept per frame, 1..32 */
    int32_t token_prune;        /* K: non-blank tokens considered per frame (the K most probable), 1..32, clamped to V - 1 */
    int32_t n_best;             /* N: hypotheses returned per utterance, 1..beam_width */
    int32_t timestamps;         /* != 0: forced (Viterbi) alignment of every returned hypothesis -> start / end / conf */
} pk_beam_options;
/* README.md:494 "with configurable width": the defaults W = 8, K = 16, N = 1, no timestamps */
void pk_beam_options_default(pk_beam_options *out);
/* README.md:494 "CTC prefix beam search", the search alone: HOST log-probs in, n-best out.  Needs a device, no model.
 * logp: n_frames == NULL: [B][T][V]; else packed [sum_b n_frames[b]][V] and T is ignored (the arrays are pitched for the longest utterance,
 * Tmax).  Outputs: ids / start / end / conf [B][N][Tmax] (start / end / conf optional, written only with opt->timestamps), lens / score
 * [B][N]; hypotheses best first, score = log(p_blank + p_non_blank) of the prefix after the last frame.  A slot the beam cannot fill (fewer
 * than N prefixes exist, e.g. T = 1) has lens 0 and score -inf; unused token slots are 0.  opt == NULL: the defaults.
 * Timestamps past 3200 frames, or more than 1 GiB of alignment back-pointers (B N T (2 T + 1) bytes): PK_ERR_UNSUPPORTED. */
pk_status pk_ctc_beam_search(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const pk_beam_options *opt,
                             int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf);
/* CTC head + log-softmax (the kernels of pk_ctc_decode) + the search on the model's stream (README.md:494 on the encoder's
 * output); the log-probs never leave the device.  enc [B][T][hidden] resp. packed with n_frames[B]; outputs as above with
 * Tmax = T resp. max n_frames.  PK_ERR_UNSUPPORTED for a model without a CTC head or with a boost trie set. */
pk_status pk_ctc_beam_decode(pk_model *m, const float *enc, int B, int T, const pk_beam_options *opt, int32_t *ids, int32_t *lens,
                             float *score, int32_t *start, int32_t *end, float *conf);
pk_status pk_ctc_beam_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const pk_beam_options *opt, int32_t *ids,
                                    int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf);
/* Stage timers of the search (tools/bench_ctc_beam.py): the CTC head + log-softmax + greedy collapse (what pk_ctc_decode runs), then top-K +
 * walk + back-trace / alignment, each between hipEvents on the model's stream; medians of `reps` passes after one warm-up.  n_frames NULL:
 * uniform [B][T].  ms[0] = greedy CTC stage, ms[1] = beam search stage. */
pk_status pk_ctc_beam_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int reps,
                                   float ms[2]);
/* One call from PCM to n-best (what README.md:514 "N-best reranking" consumes): clips packed into ragged batches by the policy of pk_transcribe_pcm
 * (pk_plan_batches), encoded, searched.  results[i]: the n_hyp <= N hypotheses of clip i, best first: hyp[j] a pk_result as pk_transcribe_pcm
 * fills it (text through the model's vocabulary, words through the grouping of pk_group_timestamps when opt->timestamps), score[j] its
 * log-probability.  Owned by the library until pk_nbest_free. */
typedef struct pk_nbest {
    int32_t n_hyp;
    const pk_result *hyp;
    const float *score;
} pk_nbest;
pk_status pk_transcribe_pcm_nbest(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *opt,
                                  pk_nbest **results);
void pk_nbest_free(pk_nbest *results, int n_clips);

/* ---- N-gram language-model shallow fusion of the CTC prefix beam search ---------------------------------------------------
 * The reference's roadmap line "N-gram LM shallow fusion: load ARPA language models, score partial hypotheses during beam search"
 * (README.md:495).  A back-off n-gram model over the acoustic model's TOKEN IDS (the words of the ARPA text are decimal ids, "17", plus <s>,
 * </s> and <unk>: what an n-gram trainer makes of tools/make_token_corpus.py's output), orders 1..5, log10 values, a missing back-off
 * column is 0; probabilities are not checked for normalisation.  Every value is converted once (strtod -> * 2.302585092994046 in double ->
 * fp32): natural-log fp32 is what everything below sees.  The model compiles to a back-off automaton, and
 *   lookup(s, c): acc = 0; while (s, c) has no arc and s is not the empty context: acc = acc + backoff_weight[s], s = backoff[s];
 *                 -> acc + p(arc) and the arc's next state; a miss in the empty context scores <unk>'s unigram and goes to the empty context
 * is the one scoring rule of pk_lm_score and of the fused search (tests/ngram_lm_ref.py and tests/ctc_beam_lm_ref.py
 * are the specification in Python; host and device results equal them bit for bit).  Word-level models, binary KenLM files, neural models,
 * the </s> term inside the search, pk_group / streaming variants and boosting together with a model: no variant.  Fusion inside the TDT beam
 * search: the _lm entry points of its section below. */
typedef struct pk_lm pk_lm;
/* Parses and compiles ARPA text from a file resp. from n_bytes of memory (no terminator needed).  Host only.  PK_ERR_INVALID with the line
 * named in pk_last_error for: a word that is neither a decimal id nor <s> / </s> / <unk>; an id >= 2^24; "ngram k=" counts that disagree with
 * the sections (or an order past 5); an n-gram whose first k - 1 words are not an entry themselves; a duplicate n-gram; a value that is not a
 * finite number; an id without a unigram in a model without <unk>; text that ends before \end\.  PK_ERR_IO when the file cannot be read. */
pk_status pk_lm_load(const char *path, pk_lm **out);
pk_status pk_lm_load_buffer(const char *text, size_t n_bytes, pk_lm **out);
/* Frees the model and its device copies (one per device, made on the first fused search there). */
void pk_lm_free(pk_lm *lm);
int pk_lm_order(const pk_lm *lm);                       /* 1..5; 0 for NULL */
int64_t pk_lm_num_ngrams(const pk_lm *lm);              /* entries of all orders */
/* Host only, no device: logp[i] = the fp32 left-to-right sum of lookup over string i = ids[id_offsets[i] .. id_offsets[i + 1]), from the
 * context <s> with bos != 0 (when the file has <s>; else, and with bos == 0, from the empty context), plus the </s> term with eos != 0.  An
 * empty string scores 0 (resp. its </s> term).  What a caller rescores an n-best list with.  PK_ERR_INVALID for a
 * negative id, an id >= 2^24, or an id without a unigram under a model without <unk>. */
pk_status pk_lm_score(const pk_lm *lm, const int32_t *ids, const int32_t *id_offsets, int n_strings, int bos, int eos, float *logp);
typedef struct pk_lm_options {
    float alpha;                /* weight of the model's log-probability */
    float beta;                 /* added per token (a length reward when positive) */
} pk_lm_options;
/* alpha = 0.5, beta = 0.0: a choice, not a measurement of accuracy on any data */
void pk_lm_options_default(pk_lm_options *out);
/* The entry points of the unfused search with a model: the arguments of pk_ctc_beam_search / _decode / _decode_ragged / _decode_timed resp.
 * pk_transcribe_pcm_nbest, then the model, its weights (NULL: the defaults) and one more output, lm_score [B][N] (optional).  A beam entry
 * carries the automaton's state after its prefix and the prefix's LM score lm (start: the start state, 0); extending by token c:
 * (lp, s2) = lookup(state, c), lm2 = lm + ((alpha * lp) + beta), three separately rounded fp32 operations.  A candidate is selectable exactly
 * when the unfused search selects it, and ranks by score + lm (one fp32 add) where the unfused search ranks by score; token pruning stays
 * acoustic, merges are the unfused search's (lm is a function of the token string alone), </s> is never proposed.  Hypotheses come back in fused
 * order; score keeps its meaning (the prefix's acoustic log-probability), lm_score is lm; a slot the beam cannot fill has lm_score 0.
 * Refusals beyond the unfused entry point's: PK_ERR_INVALID for lm == NULL, a non-finite alpha or beta, a model that names the blank id or an
 * id >= V, or one with neither <unk> nor a unigram for every non-blank id of the vocabulary. */
pk_status pk_ctc_beam_search_lm(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const pk_beam_options *opt,
                                int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm,
                                const pk_lm_options *lm_opt, float *lm_score);
/* PK_ERR_UNSUPPORTED for a model without a CTC head or with a boost trie set, as pk_ctc_beam_decode. */
pk_status pk_ctc_beam_decode_lm(pk_model *m, const float *enc, int B, int T, const pk_beam_options *opt, int32_t *ids, int32_t *lens,
                                float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm, const pk_lm_options *lm_opt,
                                float *lm_score);
pk_status pk_ctc_beam_decode_lm_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const pk_beam_options *opt, int32_t *ids,
                                       int32_t *lens, float *score, int32_t *start, int32_t *end, float *conf, const pk_lm *lm,
                                       const pk_lm_options *lm_opt, float *lm_score);
/* Stage timers as pk_ctc_beam_decode_timed (tools/bench_ctc_beam_lm.py): ms[1] = top-K + fused walk + back-trace / alignment. */
pk_status pk_ctc_beam_decode_lm_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const pk_beam_options *opt, int reps,
                                      float ms[2], const pk_lm *lm, const pk_lm_options *lm_opt);
/* pk_transcribe_pcm_nbest through the fused search: results[i].score[j] stays the acoustic score, lm_score (optional, [n_clips][N], N =
 * opt->n_best) takes the LM scores beside it: lm_score[i * N + j] belongs to results[i].hyp[j], slots past n_hyp read 0.  pk_nbest is unchanged. */
pk_status pk_transcribe_pcm_nbest_lm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *opt,
                                     pk_nbest **results, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score);

/* ---- TDT beam search with n-best output ----------------------------------------------------------------------------------
 * The other half of the reference's roadmap line "Beam search decoding -- CTC prefix beam search and TDT/RNNT beam search with configurable
 * width" (README.md:494), for models whose only decoder is the TDT head (tdt-600m).  A max-path search over the lattice of DESIGN.md section
 * 5.5.2: a hypothesis is one concrete path (token prefix, frame pointer, fp32 score = the path's left-to-right sum, each arc
 * score + (label log-prob + duration log-prob)); two paths reaching the same (prefix, frame) are one state and the better one stays.  Every
 * step, tie rule and the duplicate rule are specified in DESIGN.md section 5.5.5 (tests/tdt_beam_ref.py is that specification in Python; the
 * device result equals it bit for bit).  max_symbols_per_step is not part of the search.  The score of a hypothesis is ONE alignment's
 * log-probability, at most pk_tdt_align_decode's score for the same ids; pk_tdt_total_decode on the returned ids gives the log-likelihood
 * summed over every alignment.  RNN-T heads, gemm_bf16, boosting inside the beam, pk_group and streaming sessions: no variant.  An n-gram
 * language model inside the search: the _lm entry points at the end of this section. */
typedef struct pk_tdt_beam_options {
    int32_t beam_width;         /* W: hypotheses kept per step, 1..16 */
    int32_t label_prune;        /* K: non-blank labels expanded per hypothesis (the K most probable) next to the blank, 1..16, clamped to V - 1 */
    int32_t duration_prune;     /* Kd: durations expanded per label (the Kd most probable), 1..8, clamped to D */
    int32_t n_best;             /* N: hypotheses returned per utterance, 1..beam_width */
} pk_tdt_beam_options;
/* The defaults W = 8, K = 8, Kd = 2, N = 1: choices, not measurements of accuracy or speed */
void pk_tdt_beam_options_default(pk_tdt_beam_options *out);
/* enc_proj once per clip, then the search on the model's stream (a host loop of ordinary launches with a hard cap of Tmax + max_tokens
 * steps).  enc [B][T][hidden] resp. packed with n_frames[B].  Outputs: ids / start / end / dur_idx / conf [B][N][max_tokens] (start / end /
 * dur_idx / conf optional) as pk_tdt_align defines them, lens / score [B][N], ok [B] (optional) = 0 when no hypothesis of the clip reached the
 * last frame; hypotheses in beam order (scores descend), distinct token strings.  A slot the beam cannot fill has lens 0 and score -inf;
 * unused token slots are 0.  A hypothesis holds at most max_tokens tokens.  opt == NULL: the defaults.  With W = K = Kd = 1 this is the greedy
 * loop of pk_tdt_decode without its max_symbols_per_step.
 * PK_ERR_UNSUPPORTED (before anything is allocated): a model without a TDT joint (RNN-T head, encoder only), gemm_bf16, a boost trie set,
 * options out of range, or more than 1 GiB of scratch (formula: csrc/tdt_beam.hpp). */
pk_status pk_tdt_beam_decode(pk_model *m, const float *enc, int B, int T, const pk_tdt_beam_options *opt, int max_tokens, int32_t *ids,
                             int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, int32_t *ok);
pk_status pk_tdt_beam_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const pk_tdt_beam_options *opt, int max_tokens,
                                    int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                                    int32_t *ok);
/* Stage timers (tools/bench_tdt_beam.py): the greedy TDT stage (enc_proj + the greedy loop, what pk_tdt_decode runs), then the search stage
 * (enc_proj + the search + back-trace), each between hipEvents on the model's stream; medians of `reps` passes after one warm-up.  n_frames
 * NULL: uniform [B][T].  ms[0] = greedy TDT stage, ms[1] = beam search stage. */
pk_status pk_tdt_beam_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt,
                                   int max_tokens, int reps, float ms[2]);
/* One call from PCM to n-best through the TDT head: clips packed as pk_transcribe_pcm_nbest packs them, encoded, searched with
 * max_tokens = (frames of the batch's longest clip) * max_symbols_per_step.  results as pk_transcribe_pcm_nbest fills them (timestamps != 0:
 * start / end / confidence and words), score[j] the hypothesis's path log-probability; freed with pk_nbest_free. */
pk_status pk_transcribe_pcm_nbest_tdt(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_tdt_beam_options *opt,
                                      int timestamps, pk_nbest **results);
/* The search with n-gram LM shallow fusion (tests/tdt_beam_lm_ref.py is the specification in Python, the device
 * result equals it bit for bit): the arguments of the unfused entry point, then the model, its weights (NULL: the defaults) and one more
 * output, lm_score [B][N] (optional).  A hypothesis carries the automaton's state after its prefix and the prefix's LM score lm (start: the
 * start state, 0).  A blank arc inherits both; a label arc with token c has (lp, s2) = lookup(state, c), lm2 = lm + ((alpha * lp) + beta), three
 * separately rounded fp32 operations, one lookup for all durations of the label.  Label and duration pruning stay acoustic and a candidate's
 * score stays the acoustic one; the duplicate rule and the choice of the W best decide by score + lm (one fp32 add) where the unfused search
 * decides by score.  </s> is never proposed.  Hypotheses come back in fused order; score keeps its meaning (the path's acoustic
 * log-probability), lm_score is lm; a slot the beam cannot fill has score -inf and lm_score 0.  With alpha = beta = 0 every output equals the
 * unfused search's bit for bit.
 * Refusals, before anything is allocated (the model's device copy included): PK_ERR_UNSUPPORTED as the unfused entry point (the scratch formula grows by the fused terms);
 * PK_ERR_INVALID for lm == NULL, a non-finite alpha or beta, a model that names the blank id or an id >= V, or one with neither <unk> nor a
 * unigram for every non-blank id of the vocabulary.  Still no variant: the </s> term, word-level models, RNN-T heads, gemm_bf16, boosting
 * together with a model, pk_group and streaming sessions. */
pk_status pk_tdt_beam_decode_lm(pk_model *m, const float *enc, int B, int T, const pk_tdt_beam_options *opt, int max_tokens, int32_t *ids,
                                int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, int32_t *ok,
                                const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score);
pk_status pk_tdt_beam_decode_lm_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const pk_tdt_beam_options *opt, int max_tokens,
                                       int32_t *ids, int32_t *lens, float *score, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf,
                                       int32_t *ok, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score);
/* Stage timers as pk_tdt_beam_decode_timed (tools/bench_tdt_beam_lm.py): ms[1] = enc_proj + the fused search + back-trace. */
pk_status pk_tdt_beam_decode_lm_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const pk_tdt_beam_options *opt,
                                      int max_tokens, int reps, float ms[2], const pk_lm *lm, const pk_lm_options *lm_opt);
/* Steps (expand + prune rounds of the host loop) that the model's last TDT beam search enqueued, fused or not, _timed calls included: the
 * search stops between groups of 8 steps once no hypothesis of the batch is live, so the count is a multiple of 8 or the cap Tmax + max_tokens.
 * What tools/bench_tdt_beam_lm.py divides the fused stage's extra time by.  0 before the first search and for NULL. */
int pk_tdt_beam_last_steps(const pk_model *m);
/* pk_transcribe_pcm_nbest_tdt through the fused search: results[i].score[j] stays the acoustic score, lm_score (optional, [n_clips][N], N =
 * opt->n_best) takes the LM scores beside it: lm_score[i * N + j] belongs to results[i].hyp[j], slots past n_hyp read 0.  pk_nbest is unchanged. */
pk_status pk_transcribe_pcm_nbest_tdt_lm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_tdt_beam_options *opt,
                                         int timestamps, pk_nbest **results, const pk_lm *lm, const pk_lm_options *lm_opt, float *lm_score);

/* ---- CTC forced alignment of a GIVEN transcript ---------------------------------------------------------------------------
 * Given the log-probs and the token string that was said: when was each token said.  The alignment is the max-plus (Viterbi) path on the
 * 2 L + 1 state CTC lattice, specified operation by operation in DESIGN.md section 5.5.1 (tests/ctc_align_ref.py is that specification in
 * Python; the device result equals it bit for bit): fp32, one add per cell, predecessor ties stay / previous state / skip, a skip only onto
 * a token that differs from the token before it, end state the last blank unless the last token's state is strictly better.
 * All of it runs on the device (kernels/ctc_align.hip).  pk_group and streaming sessions have no alignment variant; the TDT head: pk_tdt_align* below.
 *
 * pk_ctc_align: HOST log-probs in.  Needs a device, no model.  logp / n_frames / B / T / V / blank as pk_ctc_beam_search.  ids: the token
 * strings of the B utterances packed, utterance b = ids[id_offsets[b] .. id_offsets[b+1]) (id_offsets[0] = 0; an empty string is valid).
 * Outputs: start / end / conf packed as ids (first and last frame of every token, conf = exp(logp[start][id])); score[B] the path's
 * log-probability; total[B] (optional, NULL: not computed) the CTC log-likelihood of the string, the forward algorithm on the same lattice
 * (>= score); ok[B] = 1, or 0 where the string cannot be aligned (more tokens + adjacent repeats than frames, or every path -inf): then
 * score = -inf and the utterance's start / end / conf are 0.
 * PK_ERR_INVALID (before any device work): B < 1, offsets that decrease, an id outside [0, V) or equal to blank.
 * PK_ERR_UNSUPPORTED (before anything is allocated): a string of more than 16383 tokens, or more than 1 GiB of back-pointers
 * (sum over the utterances of T_b * ceil((2 L_b + 1) / 16) * 4 bytes; one hour of audio, T = 45000, with L = 15000 takes 338 MB). */
pk_status pk_ctc_align(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const int32_t *ids, const int32_t *id_offsets,
                       int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok);
/* CTC head + log-softmax (the kernels of pk_ctc_decode) + the alignment on the model's stream; the log-probs never leave the device.
 * enc [B][T][hidden] resp. packed with n_frames[B].  PK_ERR_UNSUPPORTED for a model without a CTC head.  A boost trie set on the model does
 * not matter: the alignment reads the unboosted log-softmax rows. */
pk_status pk_ctc_align_decode(pk_model *m, const float *enc, int B, int T, const int32_t *ids, const int32_t *id_offsets, int32_t *start,
                              int32_t *end, float *conf, float *score, float *total, int32_t *ok);
pk_status pk_ctc_align_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                                     int32_t *start, int32_t *end, float *conf, float *score, float *total, int32_t *ok);
/* Stage timers of the alignment (tools/bench_ctc_align.py): the CTC head + log-softmax + greedy collapse, then the alignment (uploads of the
 * token strings, zero-fills and the kernel), each between hipEvents on the model's stream; medians of `reps` passes after one warm-up.
 * n_frames NULL: uniform [B][T].  ms[0] = CTC stage, ms[1] = alignment stage. */
pk_status pk_ctc_align_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids,
                                    const int32_t *id_offsets, int want_total, int reps, float ms[2]);
/* One call from PCM and transcripts to timestamps: clips of any length packed into ragged batches by the policy of pk_transcribe_pcm
 * (pk_plan_batches), encoded (the attention context set on the model applies: that is how an hour-long clip gets through), aligned.
 * The transcripts: texts[n_clips] UTF-8 (tokenised as pk_tokenize does; needs the model's vocabulary), or, with texts == NULL, ids packed with
 * id_offsets[n_clips + 1].  results[i]: a pk_result as pk_transcribe_pcm fills it with timestamps on (words through the grouping of
 * pk_group_timestamps), owned by the library until pk_results_free; a clip with ok = 0 gets its text and ids but NULL timestamp arrays and no
 * words.  score / total (either optional) / ok: [n_clips], as pk_ctc_align. */
pk_status pk_align_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts_or_null,
                       const int32_t *ids_or_null, const int32_t *id_offsets, pk_result **results, float *score, float *total, int32_t *ok);

/* ---- TDT forced alignment of a GIVEN transcript ---------------------------------------------------------------------------
 * The same question through the TDT head (label + duration joint), for the models without a CTC head.  The lattice of an utterance of T frames
 * and U tokens is T x (U + 1) joint evaluations -- cell (t, u): frame t, the prediction net having consumed ids[:u] -- with the arcs of the
 * greedy loop (src/tdt.cpp:62-106): blank with duration i to (t + max(dur[i], 1), u), label ids[u] with duration i to (t + dur[i], u + 1), an
 * arc past the last frame ends the utterance when all U tokens are out.  The alignment is the max-plus path, specified operation by operation in
 * DESIGN.md section 5.5.2 (tests/tdt_align_ref.py is that specification; the device result equals it bit for bit).  max_symbols_per_step is
 * not part of the lattice (as in pk_tdt_score).  The forward-algorithm total of the same lattice: pk_tdt_total* below.  All of it runs on the device
 * (kernels/tdt_align.hip).
 *
 * pk_tdt_align: the walk alone on a HOST lattice.  Needs a device, no model.  Utterance b has n_frames[b] >= 1 frames and the tokens
 * id_offsets[b] .. id_offsets[b+1] (id_offsets[0] = 0; U = 0 is valid); its values are packed utterance after utterance:
 * lab [T_b][U_b], blk [T_b][U_b + 1], dl [T_b][U_b + 1][D].  durations[D], 1 <= D <= 8.
 * Outputs: start / end / dur_idx / conf packed as the tokens (token k emitted at frame start[k] with duration index dur_idx[k],
 * end[k] = min(start[k] + max(dur, 1) - 1, T - 1), conf[k] = exp(lab[start[k]][k])), score[B] the path's log-probability, ok[B] = 1, or 0
 * where no path reaches the end: then score = -inf and the utterance's arrays are 0.
 * PK_ERR_INVALID (before any device work): B < 1, n_frames[b] < 1, offsets that decrease.
 * PK_ERR_UNSUPPORTED (before anything is allocated): D outside [1, 8], a duration outside [0, 8], more than 1535 tokens in an utterance, or
 * more than 1 GiB of scratch: with cells = sum_b T_b (U_b + 1) and labs = sum_b T_b U_b, 4 (labs + cells (1 + D)) + cells bytes. */
pk_status pk_tdt_align(const float *lab, const float *blk, const float *dl, const int32_t *durations, int D, const int32_t *n_frames, int B,
                       const int32_t *id_offsets, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok);
/* Prediction net over every prefix + enc_proj + the lattice (joint of every cell in row chunks: the [cells][V + D] logits never exist at once)
 * + the walk, on the model's stream.  enc [B][T][hidden] resp. packed with n_frames[B]; ids packed with id_offsets[B + 1].
 * PK_ERR_INVALID: an id outside [0, V) or equal to blank, decreasing offsets.  PK_ERR_UNSUPPORTED: a model without a TDT joint (RNN-T head,
 * encoder-only), a gemm_bf16 model (its decode weights exist only rounded), or past the limits above; the scratch then also counts
 * chunk_rows (V + D + J) 4 bytes of the rows chunk and (U_max + 1) B (J + 1) 4 bytes of the prediction net's outputs.  A boost trie set on
 * the model does not matter. */
pk_status pk_tdt_align_decode(pk_model *m, const float *enc, int B, int T, const int32_t *ids, const int32_t *id_offsets, int32_t *start,
                              int32_t *end, int32_t *dur_idx, float *conf, float *score, int32_t *ok);
pk_status pk_tdt_align_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *ids,
                                     const int32_t *id_offsets, int32_t *start, int32_t *end, int32_t *dur_idx, float *conf, float *score,
                                     int32_t *ok);
/* Stage timers (tools/bench_tdt_align.py), each between hipEvents on the model's stream, medians of `reps` passes after one warm-up:
 * ms[0] = prediction net (uploads, U_max + 1 lock-step steps), ms[1] = lattice (enc_proj + activation + heads product + reduction, all
 * chunks), ms[2] = the walk and back-trace, ms[3] = the heads product of ONE chunk alone (min(chunk_rows, cells) x (V + D) x J, timed on its
 * own after the passes: what the lattice stage's activation and reduction kernels cost on top of it).  n_frames NULL: uniform [B][T]. */
pk_status pk_tdt_align_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *ids,
                                    const int32_t *id_offsets, int reps, float ms[4]);
/* One call from PCM and transcripts to timestamps, as pk_align_pcm (same packing, same result layout; the attention context set on the model
 * applies), through the TDT head: works for models without a CTC head.  score (optional) / ok: [n_clips]. */
pk_status pk_tdt_align_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts_or_null,
                           const int32_t *ids_or_null, const int32_t *id_offsets, pk_result **results, float *score, int32_t *ok);
/* Diagnostic: the lattice values of a ragged batch as pk_tdt_align takes them, brought back to the host.  chunk_rows > 0 overrides the
 * engine's chunk size (lattice rows per heads product), 0 keeps it.  lab / blk / dl receive labs / cells / cells D floats FOLLOWED BY
 * PK_DIAG_TDT_LATTICE_GUARD more each: the device buffers are filled with the pattern 0x7FC5A5A5 before the first launch and copied back
 * whole, so a word the launches did not write comes back as that pattern. */
#define PK_DIAG_TDT_LATTICE_GUARD 64
pk_status pk_diag_tdt_lattice(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                              int chunk_rows, float *lab, float *blk, float *dl);
/* ---- TDT log-likelihood of a GIVEN transcript, and CTC n-best rescored with it ------------------------------------------------
 * How probable is this token string under the TDT head: the forward algorithm on the lattice of pk_tdt_align (same cells, same arcs; a blank of
 * duration 0 and a blank of duration 1 are two arcs to the next frame and both are summed), specified operation by operation in DESIGN.md
 * section 5.5.3 (tests/tdt_total_ref.py is that specification; the device result equals it bit for bit).  No length normalisation, no language
 * model, no bf16 form, no RNN-T head; pk_group and streaming sessions have no variant.  All of it runs on the device (kernels/tdt_total.hip).
 *
 * pk_tdt_total: the walk alone on a HOST lattice, packed as for pk_tdt_align.  Needs a device, no model.  total[B] = the log-sum over every path
 * to the end (>= the alignment's score), ok[B] = 1, or 0 where no path reaches the end (total = -inf).  Refusals as pk_tdt_align; the scratch
 * formula is the alignment's without its back-pointer bytes: 4 (labs + cells (1 + D)) <= 1 GiB. */
pk_status pk_tdt_total(const float *lab, const float *blk, const float *dl, const int32_t *durations, int D, const int32_t *n_frames, int B,
                       const int32_t *id_offsets, float *total, int32_t *ok);
/* Prediction net over every prefix + enc_proj + lattice + walk on the model's stream, for n_hyp token strings over n_clips clips:
 * hypothesis h reads the frames of clip clip_of[h], so several transcripts of one clip share its rows and enc_proj runs once per clip.
 * enc [n_clips][T][hidden] resp. packed with n_frames[n_clips]; ids packed with id_offsets[n_hyp + 1]; total / ok [n_hyp].
 * clip_of == NULL: hypothesis h on clip h, and n_hyp must equal n_clips.
 * The hypotheses are walked in groups of consecutive ones: at most 256, and as many as keep the group's scratch (the formula above plus the rows
 * chunk and the prediction net's outputs, as pk_tdt_align_decode counts them) under 1 GiB.  Grouping changes no bit of any result.
 * PK_ERR_INVALID: a clip_of entry outside [0, n_clips), n_hyp != n_clips without clip_of, an id outside [0, V) or equal to blank, decreasing
 * offsets.  PK_ERR_UNSUPPORTED exactly where pk_tdt_align_decode refuses: no TDT joint, gemm_bf16, D / durations / 1535 tokens, or one
 * hypothesis whose own scratch exceeds the cap.  A boost trie set on the model does not matter. */
pk_status pk_tdt_total_decode(pk_model *m, const float *enc, int n_clips, int T, const int32_t *ids, const int32_t *id_offsets,
                              const int32_t *clip_of_or_null, int n_hyp, float *total, int32_t *ok);
pk_status pk_tdt_total_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int n_clips, const int32_t *ids,
                                     const int32_t *id_offsets, const int32_t *clip_of_or_null, int n_hyp, float *total, int32_t *ok);
/* Stage timers (tools/bench_tdt_rescore.py), between hipEvents on the model's stream, summed over the groups of the call, medians of `reps`
 * passes after one warm-up: ms[0] = prediction net (with the host-to-device copies of every group's token strings and tables, as the
 * alignment's timer counts them; U_max + 1 lock-step steps per group), ms[1] = lattice (activation + heads product + reduction, all chunks), ms[2] = the forward
 * pass.  n_frames NULL: uniform [n_clips][T]. */
pk_status pk_tdt_total_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int n_clips, int T, const int32_t *ids,
                                    const int32_t *id_offsets, const int32_t *clip_of_or_null, int n_hyp, int reps, float ms[3]);
/* One call from PCM and one or more transcripts per clip to log-likelihoods: clips packed and encoded as pk_tdt_align_pcm does it (the
 * attention context set on the model applies); texts[n_hyp] UTF-8, or ids packed with id_offsets[n_hyp + 1]; clip_of as above (a clip without a
 * transcript is allowed); total / ok [n_hyp]. */
pk_status pk_tdt_score_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const char *const *texts_or_null,
                           const int32_t *ids_or_null, const int32_t *id_offsets, const int32_t *clip_of_or_null, int n_hyp, float *total,
                           int32_t *ok);
/* The reference's roadmap line "N-best reranking" (README.md:514) with the model's own stronger head as the second opinion:
 * pk_transcribe_pcm_nbest, then every returned hypothesis scored under the TDT head (an empty hypothesis is U = 0, which is valid), then each
 * clip's list re-ordered by combined = fl(fl((1 - w) ctc) + fl(w tdt)), w = tdt_weight, all in fp32: stable, descending, ties keep the beam's
 * order; a hypothesis the TDT head cannot score (ok = 0) sorts after every scored one and carries combined = -inf.  score[j] of the pk_nbest is
 * combined; ctc_score / tdt_total (optional, [n_clips][N], N = n_best) carry the parts in the returned order, -inf in the slots past n_hyp.
 * rescore_opt == NULL: tdt_weight 0.5.  tdt_weight 0 returns the beam's own list.
 * PK_ERR_UNSUPPORTED for a model without both heads (or whose heads do not share a vocabulary), and wherever the two stages refuse.  The model
 * refusals come before any work.  The limits of the total (a hypothesis over 1535 tokens, one whose own scratch exceeds 1 GiB) depend on what
 * the search returns, so they are checked LATE: after a batch has been encoded and searched, and after earlier batches of the call were fully
 * processed.  The call then fails as a whole and returns no list; only clips of more than 1535 encoder frames (about two minutes) can reach
 * them.  pk_tdt_score_pcm and pk_tdt_align_pcm, whose strings are given, refuse before encoding. */
typedef struct pk_rescore_options {
    float tdt_weight;           /* w: weight of the TDT log-likelihood, 1 - w that of the CTC score; finite */
} pk_rescore_options;
pk_status pk_transcribe_pcm_nbest_rescored(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_beam_options *beam_opt,
                                           const pk_rescore_options *rescore_opt, pk_nbest **results, float *ctc_score, float *tdt_total);
/* Diagnostics, host arithmetic (no device, no model): the groups pk_tdt_total_decode would walk n_hyp hypotheses of n_frames_of_hyp[h] frames in
 * (group_of[n_hyp]; V / J the vocabulary and joint width, max_hyps <= 0: the engine's 256), and the ordering rule above on the N slots of one
 * clip in beam order (order[j] = the slot at position j, combined[] by slot). */
pk_status pk_diag_tdt_total_groups(const int32_t *n_frames_of_hyp, const int32_t *id_offsets, int n_hyp, const int32_t *durations, int D, int V, int J,
                                   int max_hyps, int32_t *group_of, int *n_groups);
pk_status pk_diag_rescore_order(const int32_t *lens, const float *ctc_score, const float *tdt_total, const int32_t *ok, int N, float tdt_weight,
                                int32_t *order, float *combined);
/* Diagnostic: out[0] / out[1] = free / total bytes of the current device (hipMemGetInfo), out[2] = the bytes of device memory the grow-only
 * buffers of m's stage entry points hold (workspace, io scratch, TDT alignment, TDT total and keyword-spotting scratch; 0 with m == NULL): what a call that promises to
 * allocate nothing must leave unchanged. */
pk_status pk_diag_mem_info(pk_model *m, uint64_t out[3]);

/* ---- CTC keyword spotting: is a phrase said anywhere in this audio, and when ---------------------------------------------------
 * Given the log-probs and a list of keywords (token strings): the best non-overlapping spans in which each keyword was said.  A keyword's
 * lattice is the CTC lattice of its L tokens without the leading and the trailing blank (2 L - 1 states; arcs stay / previous state / skip,
 * a skip only onto a token that differs from the token before it), walked max-plus with a FREE start (the first state may be entered at any
 * frame with value +0.0) and a FREE end (the last state is read at every frame).  The cost of a symbol at a frame is its log-prob minus the
 * frame's largest log-prob, so a score is the log-ratio of the keyword's best path over a span to the unconstrained best path over the same
 * span: <= 0, without a bias towards short spans, and exactly +0.0 where the greedy path over the span IS the keyword.  The hits of a
 * (utterance, keyword) pair are picked greedily: the best end frame (ties: the earliest), its span [start, end], then every end frame whose
 * span meets that one is out; up to max_hits times, in the order picked.  Specified operation by operation in DESIGN.md section 5.5.4
 * (tests/ctc_kws_ref.py is that specification in Python; the device result equals it bit for bit).  All of it runs on the device
 * (kernels/ctc_kws.hip).  Matching is on token strings: "cat" matches inside "category" unless the tokenisation differs.  No threshold is
 * applied unless the caller sets one.  pk_group has no spotting variant; streaming sessions spot through the TDT head (pk_stream_set_keywords below).
 * PRECONDITION: every row of the log-probs has a finite maximum (a true log-softmax row always has one).
 *
 * pk_ctc_kws: HOST log-probs in.  Needs a device, no model.  logp / n_frames / B / T / V / blank as pk_ctc_beam_search.  kw_ids: the n_kw keywords
 * packed, keyword k = kw_ids[kw_offsets[k] .. kw_offsets[k+1]) (kw_offsets[0] = 0).  Every keyword is searched in every utterance.
 * Outputs: n_hits [B][n_kw]; start / end (encoder frames, inclusive) and score [B][n_kw][max_hits]; unused slots are start = end = 0,
 * score = -inf.
 * PK_ERR_INVALID (before any device work): B < 1, n_kw < 1, an empty keyword, offsets that decrease, an id outside [0, V) or equal to blank,
 * min_score > 0 or NaN.
 * PK_ERR_UNSUPPORTED (before anything is allocated): a keyword of more than 64 tokens, max_hits outside 1 .. 16, more than 65535 utterances, or
 * more than 1 GiB of scratch (8 * n_kw * sum of T_b bytes: 128 keywords over one hour, T = 45000, take 46 MB). */
typedef struct pk_kws_options {
    int32_t max_hits;           /* hits reported per (utterance, keyword), 1 .. 16 */
    float min_score;            /* only end frames with score >= min_score are picked; <= 0, -inf: no threshold */
} pk_kws_options;
/* the defaults: max_hits = 1, min_score = -inf (the best span is reported and the caller applies a threshold).  opt == NULL means the defaults. */
void pk_kws_options_default(pk_kws_options *out);
pk_status pk_ctc_kws(const float *logp, const int32_t *n_frames, int B, int T, int V, int blank, const int32_t *kw_ids, const int32_t *kw_offsets,
                     int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
/* CTC head + log-softmax (the kernels of pk_ctc_decode) + the spotting on the model's stream; the log-probs never leave the device.
 * enc [B][T][hidden] resp. packed with n_frames[B].  PK_ERR_UNSUPPORTED for a model without a CTC head.  A boost trie set on the model does
 * not matter: the spotting reads the unboosted log-softmax rows. */
pk_status pk_ctc_kws_decode(pk_model *m, const float *enc, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                            const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
pk_status pk_ctc_kws_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *kw_ids, const int32_t *kw_offsets,
                                   int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
/* Stage timers of the spotting (tools/bench_ctc_kws.py): the CTC head + log-softmax + greedy collapse, then the spotting (uploads of the
 * keywords, the row maxima, the walk and the picking), each between hipEvents on the model's stream; medians of `reps` passes after one
 * warm-up.  n_frames NULL: uniform [B][T].  ms[0] = CTC stage, ms[1] = spotting stage. */
pk_status pk_ctc_kws_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids,
                                  const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int reps, float ms[2]);
/* One call from PCM and phrases to hits: clips of any length packed into ragged batches by the policy of pk_transcribe_pcm (pk_plan_batches)
 * exactly as pk_align_pcm packs them, encoded (the attention context set on the model applies), spotted.  The keywords: phrases[n_kw] UTF-8
 * (tokenised as pk_tokenize does; needs the model's vocabulary), or, with phrases == NULL, ids packed with kw_offsets[n_kw + 1].  Every keyword
 * is searched in every clip.  n_hits [n_clips][n_kw]; start_s / end_s / score [n_clips][n_kw][max_hits] in the caller's clip order.  Times are
 * seconds by the rule of the timestamps (frame * 0.08 s): start_s is the start of the first frame, end_s the END of the last frame
 * ((end + 1) * 0.08 s); unused slots 0 / 0 / -inf. */
pk_status pk_spot_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const char *const *phrases_or_null,
                      const int32_t *ids_or_null, const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int32_t *n_hits, float *start_s,
                      float *end_s, float *score);
/* ---- Keyword spotting through the TDT head (kernels/tdt_kws.hip; specification: tests/tdt_kws_ref.py) ----------
 * The same question for a model without a CTC head.  Every (clip, keyword) pair has the lattice of pk_tdt_align, the prediction net teacher-forced
 * over [blank, keyword...] FROM ITS INITIAL STATE: the keyword is scored as if it began the utterance (a known approximation).  An arc costs its
 * log-prob relative to the greedy decision of its cell (token head: minus the row's largest log-prob `top`; duration head: minus its largest), the
 * match may begin at any frame and ends on the last token's label arc at any frame.  A score is <= 0 and exactly +0.0 where greedy decoding with
 * this context emits the keyword there.  start = the frame at which the first token is emitted (pk_tdt_align's start[0]), end = the last frame of
 * the last token (its end[L - 1]).  pk_kws_options and the picking are those of the CTC form.
 * Refusals: PK_ERR_INVALID as pk_ctc_kws; PK_ERR_UNSUPPORTED, before anything is allocated: a keyword of more than 64 tokens, max_hits outside
 * 1 .. 16, D outside 1 .. 8 or a duration outside [0, 8], a pair whose own scratch exceeds 1 GiB, an RNN-T head, a gemm_bf16 model.
 *
 * pk_tdt_kws: the walk and the picking alone on HOST lattices, one per pair, packed as for pk_tdt_align (pair b: n_frames[b] frames, a keyword of
 * id_offsets[b + 1] - id_offsets[b] >= 1 tokens; column L is packed and never read) plus top, packed like blk.  Every read row needs a finite top
 * >= its lab and blk and one finite duration log-prob.  n_hits [B]; start / end / score [B][max_hits].  Needs a device, no model. */
pk_status pk_tdt_kws(const float *lab, const float *blk, const float *dl, const float *top, const int32_t *durations, int D, const int32_t *n_frames,
                     int B, const int32_t *id_offsets, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
/* enc_proj, the prediction net (once per distinct keyword), the lattice in chunks, the walk and the picking on the model's stream.  Arguments and
 * results as pk_ctc_kws_decode(_ragged): every keyword in every clip, n_hits [B][n_kw], start / end / score [B][n_kw][max_hits]. */
pk_status pk_tdt_kws_decode(pk_model *m, const float *enc, int B, int T, const int32_t *kw_ids, const int32_t *kw_offsets, int n_kw,
                            const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
pk_status pk_tdt_kws_decode_ragged(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *kw_ids, const int32_t *kw_offsets,
                                   int n_kw, const pk_kws_options *opt, int32_t *n_hits, int32_t *start, int32_t *end, float *score);
/* Stage timers (tools/bench_tdt_kws.py), as pk_tdt_total_decode_timed: ms[0] = prediction net (with the uploads of the tables), ms[1] = lattice,
 * ms[2] = normalisation + walk + picking, each summed over the groups of the call; medians of `reps` passes after one warm-up. */
pk_status pk_tdt_kws_decode_timed(pk_model *m, const float *enc, const int32_t *n_frames, int B, int T, const int32_t *kw_ids,
                                  const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int reps, float ms[3]);
/* pk_spot_pcm through the TDT head: same batch loop, same seconds rule, same input-rate handling, same result layout. */
pk_status pk_tdt_spot_pcm(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const char *const *phrases_or_null,
                          const int32_t *ids_or_null, const int32_t *kw_offsets, int n_kw, const pk_kws_options *opt, int32_t *n_hits, float *start_s,
                          float *end_s, float *score);
/* Diagnostic: the spotting's lattice BEFORE the normalisation, as pk_diag_tdt_lattice returns the alignment's (utterance b with its own token string
 * of >= 1 tokens; the guard words and chunk_rows as there), plus top: cells + PK_DIAG_TDT_LATTICE_GUARD floats.  The call must fit one group. */
pk_status pk_diag_tdt_kws_lattice(pk_model *m, const float *enc, const int32_t *n_frames, int B, const int32_t *ids, const int32_t *id_offsets,
                                  int chunk_rows, float *lab, float *blk, float *dl, float *top);

/* ---- one node, several GPUs: utterance shards (the reference has no multi-device path, README.md:513) ----------
 * A pk_group is one model REPLICA per device of this process: the safetensors file is mapped once and every replica is built from that
 * one host image by its own host thread (each device uploads over its own PCIe link).  pk_group_transcribe_pcm deals the clips, longest
 * first, each to the device with the least audio so far (equal lengths: rank r takes clips r, r+G, ...); every device packs its clips into
 * ragged batches; one host thread drives each device through the SAME two-stream pipeline pk_transcribe_pcm uses (PCM of batch k+1 staged and decode(k) driven
 * under encoder(k+1); from four batches per rank on, decode groups of four).  Utterances share nothing, so there is NO collective: not on
 * the data path and -- one process, one address space -- not for the results either; the ranks never wait for each other.  The library has
 * no link-time dependency on RCCL.  (The multi-PROCESS deployment -- one process per GPU under torch.distributed, bench.py --gpus N,
 * tools/transcribe_sharded.py -- ends with one RCCL all-gather of the token matrix; pk_group_verify_exchange below runs that exchange
 * in-process as a check.)  devices = NULL / n_devices <= 0: every visible device.
 * Same result contract as pk_transcribe_pcm (which is what a group of one device computes, clip for clip). */
typedef struct pk_group pk_group;
pk_status pk_group_create(const char *safetensors_path, const char *vocab_path_or_null, const pk_config *cfg, const int *devices,
                          int n_devices, pk_group **out);
void pk_group_free(pk_group *g);
/* pk_model_set_attention_context on every replica of the group. */
pk_status pk_group_set_attention_context(pk_group *g, int left, int right);
int pk_group_size(const pk_group *g);
pk_status pk_group_transcribe_pcm(pk_group *g, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt,
                                  pk_result **results);
/* figures of the last pk_group_transcribe_pcm: max-over-ranks wall time of the compute phase, total audio seconds, clips handled by
 * each rank (clips_per_rank[pk_group_size]); any pointer may be NULL */
pk_status pk_group_last_stats(const pk_group *g, double *wall_ms_max, double *audio_seconds, int32_t *clips_per_rank);
/* Debug check of the result exchange a multi-process deployment performs, run in-process over RCCL (loaded with dlopen on first use;
 * PK_ERR_UNSUPPORTED with the loader's message when librccl is not installed): the token ids of `results` (those of the LAST
 * pk_group_transcribe_pcm) go rank by rank through device memory, one ncclAllReduce(max) of (token maximum, wall time) and one fixed-stride
 * ncclAllGather of the [clips_per_rank][2 + max_tokens] int32 matrix; every rank's gathered copy must reproduce `results`.
 * *rccl_ranks (optional) = ncclCommCount of the communicator. */
pk_status pk_group_verify_exchange(pk_group *g, const pk_result *results, int n_clips, int *rccl_ranks);

/* read_audio (audio_io.cpp:453-483) restricted to RIFF/WAVE PCM16 / float32; mono-downmix; must be 16 kHz.
 * Returns a malloc'd buffer the caller frees with pk_free. */
pk_status pk_read_wav(const char *path, float **pcm, int64_t *n_samples, int *sample_rate);
/* read_audio(path, target_sample_rate) (audio_io.cpp:453-483) for RIFF/WAVE files: decode, mono downmix (sum * 1/channels,
 * :198-214) and resampling to target_rate with the reference's Kaiser-windowed sinc interpolator (sinc_resample, :123-195; fp64,
 * beta 7.857, 16-tap half width).  FLAC / MP3 / OGG are not decoded.  pk_resample: the resampler alone (resample(), :250-262). */
pk_status pk_read_audio(const char *path, int target_rate, float **pcm, int64_t *n_samples, int *original_rate);
pk_status pk_resample(const float *pcm, int64_t n, int src_rate, int dst_rate, float **out, int64_t *n_out);
/* ---- resampling on the device (kernels/resample.hip) ---------------------------------------------------------------
 * pk_resample's filter in polyphase form: with g = gcd(src, dst), up = dst / g and down = src / g the 32 weights of output i depend on
 * i mod up only.  They are tabulated once per (src, dst) on the host in fp64 from pk_resample's own expressions, and one launch turns a
 * packed ragged batch of input-rate clips into dst-rate samples, 32 fp64 multiply-adds per output.  The specification is
 * tests/resample_ref.py, which the device reproduces bit for bit.  Against pk_resample the result is bit-identical when src / dst or
 * dst / src is an integer; otherwise a few samples in 10 000 differ by one fp32 rounding (pk_resample rounds i * src / dst to a double
 * before it takes the tap distances, the table takes them from the exact fraction; tests/test_resample_ref.py holds the bounds).
 * Rates from 4000 to 384000 Hz, clips of fewer than 2^31 samples; anything else is PK_ERR_UNSUPPORTED before anything is allocated.
 * Out of scope: resampling inside streaming sessions (it needs history and lookahead carried across chunks), int16 or multi-channel input
 * on the device, pk_batch_* at other rates, and any change to pk_resample or to a default.
 * pk_resample_length: samples pk_resample returns for n input samples, ceil(n * up / down) (host arithmetic; -1 for a refused argument).
 * pk_resample_run: outputs one workgroup of the kernel owns at this pair of rates (they read run * down / up + 32 input samples); 0 if refused.
 * pk_resample_table: the table, host only.  table (may be NULL) takes up x 32 doubles, row r = phase r, column k = the tap at input sample
 *   c - 15 + k around the centre c; cap_rows < up: PK_ERR_INVALID, with *up / *down still set.
 * pk_resample_device: the stage alone on `device`, host buffers in and out.  Clip i = pcm[offsets[i] .. offsets[i+1]) at src_rate; its
 *   pk_resample_length samples go to out[out_offsets[i] ..), which must end at or before out_offsets[i+1].  out[0 .. out_offsets[n_clips]) is
 *   uploaded before and read back after the launch, so what lies between the clips' outputs comes back as it was unless the kernel wrote
 *   there.  Empty clips are allowed and give empty outputs.  src_rate == dst_rate copies.
 * pk_resample_device_timed: the same launch reps times between hipEvents; *ms = the median (input already on the device, nothing read back). */
int64_t pk_resample_length(int64_t n, int src_rate, int dst_rate);
int pk_resample_run(int src_rate, int dst_rate);
pk_status pk_resample_table(int src_rate, int dst_rate, double *table, int cap_rows, int *up, int *down);
pk_status pk_resample_device(int device, const float *pcm, const int64_t *offsets, int n_clips, int src_rate, int dst_rate, float *out,
                             const int64_t *out_offsets);
pk_status pk_resample_device_timed(int device, const float *pcm, const int64_t *offsets, int n_clips, int src_rate, int dst_rate, int reps, float *ms);
/* Sample rate of the PCM that the one-call entry points of this model take: pk_transcribe_pcm, pk_transcribe_pcm_nbest (and _nbest_lm,
 * _nbest_tdt, _nbest_tdt_lm, _nbest_rescored), pk_align_pcm, pk_tdt_align_pcm, pk_tdt_score_pcm and pk_spot_pcm.  Default 16000: the path
 * as it always was.  At another rate (4000 .. 384000, else PK_ERR_UNSUPPORTED and the previous rate stays in force) pcm and offsets of those
 * calls count input-rate samples; batches are planned by the resampled lengths, every batch is uploaded raw and resampled on the device
 * into the buffer the 16 kHz copy went to, and frames, timestamps and every result are those of the 16 kHz signal
 * pk_resample_device(rate -> 16000) gives.  UNCHANGED, always 16 kHz: pk_mel*, pk_batch_* (what bench.py times), pk_stream_*,
 * pk_sortformer_forward_pcm, pk_frontend_* and pk_resample itself.  Not to be changed while a call is in flight. */
pk_status pk_model_set_input_rate(pk_model *m, int rate);
pk_status pk_model_get_input_rate(const pk_model *m, int *rate);
/* pk_model_set_input_rate on every replica of the group (pk_group_transcribe_pcm then takes input-rate PCM). */
pk_status pk_group_set_input_rate(pk_group *g, int rate);
/* ---- voice-activity segmentation on the device (kernels/vad.hip) ---------------------------------------------------
 * The reference's roadmap lines "VAD: skip silent regions, reduce compute" (README.md:512) and "Long-form audio chunking" (README.md:511): an
 * energy detector in front of the mel front end cuts long or sparse 16 kHz audio at its pauses into pieces of at most max_piece_s seconds,
 * and the pieces go through the ragged packer of pk_transcribe_pcm as ordinary clips, so silence is never encoded and the encoder keeps full
 * attention.  Every rule is specified in DESIGN.md section 5.8 (tests/vad_ref.py is that specification in Python; the device result equals
 * it bit for bit).  In short, for a clip of n samples: F = ceil(n / 160) frames of 10 ms; e[f] = the fp32 sum of squares of a frame (zeros
 * past n, in the fixed order of section 5.8); key(e) = the bit pattern of e, 0xFFFFFFFF for a NaN; floor = the energy of rank
 * ((F - 1) * floor_percent) / 100 in ascending key order, found exactly (a radix select on the device); speech0[f] = e[f] >
 * fmaxf(abs_thr, floor * ratio) with abs_thr = (float)(160 * 10^(threshold_db / 10)) and ratio = (float)(10^(margin_db / 10)), both rounded
 * once from double; then non-speech gaps shorter than min_silence between speech become speech, speech runs shorter than min_speech are
 * dropped, and every remaining run [s, e] is padded and snapped to the encoder's 8-frame grid, s' = 8 * floor(max(0, s - pad) / 8),
 * e' = min(F - 1, 8 * ceil((min(F - 1, e + pad) + 1) / 8) - 1), overlapping and touching runs merged.  Runs are disjoint, ascending, and
 * start on multiples of 8 frames (1280 samples = one encoder frame).
 * Millisecond options become frames by integer division by 10; max_piece is the integer nearest to 100 * max_piece_s.  Refused with
 * PK_ERR_INVALID before any device work: a non-finite option, threshold_db outside [-200, 60], margin_db outside [0, 100], floor_percent
 * outside 0 .. 100, a millisecond option outside 0 .. 3 600 000, max_piece below 16 frames (the cut window then always holds a candidate) or
 * above 360 000.  A clip of 2^31 samples or more is PK_ERR_UNSUPPORTED.
 * Device scratch (grow-only; counted in pk_diag_mem_info for a model's): with S = the clips' samples, each clip rounded up to 32, F = the
 * frames and C = the chunks of pk_vad_run() frames of all clips, R = the sum of (F_i + 1) / 2,
 *     4 S + 6 F + 24 C + 8 R + 4156 n_clips bytes;
 * more than 1 GiB is PK_ERR_UNSUPPORTED before anything is allocated.
 * No variant for pk_group, streaming sessions, the n-best, alignment or spotting entry points, and none on resampled audio. */
typedef struct pk_vad_options {
    float threshold_db;         /* absolute threshold: mean square of a frame, dB re full scale */
    float margin_db;            /* ... or this far above the noise floor, whichever is higher */
    int32_t floor_percent;      /* the noise floor is this percentile of the clip's frame energies */
    int32_t min_speech_ms;
    int32_t min_silence_ms;
    int32_t pad_ms;
    int32_t max_gap_ms;         /* pieces: runs at most this far apart share a piece */
    float max_piece_s;          /* pieces: longest piece */
} pk_vad_options;
/* The defaults -50 dB, 9 dB, 10 %, 100 ms, 300 ms, 200 ms, 1000 ms, 30 s: choices, not measurements of accuracy or speed */
void pk_vad_options_default(pk_vad_options *out);
typedef struct pk_vad_piece {
    int32_t clip;               /* index of the clip the piece was cut from */
    int64_t begin, end;         /* samples [begin, end) of that clip; begin is a multiple of 1280 */
} pk_vad_piece;
/* pk_vad_run: frames one workgroup handles per pass (a chunk); clips longer than that carry the select's and the smoothing's state across chunks.
 * pk_vad_pcm: the stage alone on `device`, host buffers in and out, no model.  Clip i = pcm[offsets[i] .. offsets[i+1]) at 16 kHz with F_i
 *   frames.  n_runs[i] = its runs; they are frame indices run_start / run_end[r_i .. r_i + n_runs[i]) with r_i = the sum of (F_j + 1) / 2 over
 *   the clips before i -- (F + 1) / 2 runs per clip always suffice, so both arrays hold the sum of (F_i + 1) / 2 entries.  energy (optional)
 *   takes the sum of F_i frame energies, clip after clip.  run_start, run_end and energy are uploaded before and read back after the
 *   launches, so every entry the kernels do not write comes back as it was.  opt == NULL: the defaults.  Empty clips are allowed.
 * pk_vad_plan: the pieces of ONE clip from its runs and energies (host logic, no device): walking the runs in order, a run joins the open
 *   piece when it starts at most max_gap frames after the piece's end and the joined piece spans at most max_piece frames, otherwise it
 *   opens a new piece; a run longer than max_piece is first cut after the frame f in [s + max_piece / 2, s + max_piece - 1] with
 *   (f + 1) % 8 == 0 whose key(e[f]) is smallest (the earliest of equals), [s, f] being a run of its own and [f + 1, e] treated again.  Piece
 *   [s, e] is the samples [160 s, min(n_samples, 160 (e + 1))); its frame offset in encoder frames is s / 8.  energy holds F values (read
 *   only where a run is cut).  *pieces is malloc'd (pk_free; NULL when there are none), every clip field 0.
 * pk_vad_pcm_timed: the launches of pk_vad_pcm alone between hipEvents, reps + 1 passes, the first not counted; *ms = the median (input
 *   already on the device, nothing read back). */
int pk_vad_run(void);
pk_status pk_vad_pcm(int device, const float *pcm, const int64_t *offsets, int n_clips, const pk_vad_options *opt, int32_t *n_runs,
                     int32_t *run_start, int32_t *run_end, float *energy);
pk_status pk_vad_plan(int64_t n_samples, const int32_t *run_start, const int32_t *run_end, int n_runs, const float *energy,
                      const pk_vad_options *opt, pk_vad_piece **pieces, int *n_pieces);
pk_status pk_vad_pcm_timed(int device, const float *pcm, const int64_t *offsets, int n_clips, const pk_vad_options *opt, int reps, float *ms);
/* pk_transcribe_pcm on the speech of long or sparse clips: the VAD runs on all clips on the model's stream, pk_vad_plan cuts every clip into
 * pieces, and all pieces of all clips are transcribed as ordinary clips of one pk_transcribe_pcm call (packed together by its policy; the
 * pieces' samples are uploaded a second time from the host).  Clip i's pk_result is its pieces' results merged in time order: token ids
 * concatenated; start_frame / end_frame with the piece's frame offset (begin / 1280) added; confidences unchanged; the words concatenated,
 * start and end becoming (float)((double)t + offset * 0.08); text = the pieces' non-empty texts joined by one space.  A clip without speech
 * has empty text, 0 tokens and 0 words.  A piece of 256 samples or fewer (only the tail of a clip can be one) is listed but not transcribed.
 * pieces_out / n_pieces_out (optional, together): every piece in clip order, then time order (malloc'd, pk_free; NULL when there are none).
 * A model whose input rate is not 16 kHz: PK_ERR_UNSUPPORTED before any work. */
pk_status pk_transcribe_pcm_vad(pk_model *m, const float *pcm, const int64_t *offsets, int n_clips, const pk_options *opt,
                                const pk_vad_options *vad_opt, pk_result **results, pk_vad_piece **pieces_out, int *n_pieces_out);
/* read_audio(const uint8_t *data, size_t len, target) (audio_io.hpp:27-28): an encoded RIFF/WAVE image in memory -> mono PCM at
 * target_rate (malloc'd, pk_free). */
pk_status pk_read_audio_memory(const void *data, size_t len, int target_rate, float **pcm, int64_t *n_samples, int *original_rate, int *n_channels);
/* get_audio_duration (audio_io.hpp:39, audio_io.cpp:527-586): header walk, no decode.  duration = n_frames / sample_rate. */
pk_status pk_audio_info(const char *path, int *sample_rate, int *n_channels, int64_t *n_frames);
void pk_free(void *p);

/* ---- streaming: NemotronTranscriber / StreamingTranscriber::transcribe_chunk (src/nemotron.cpp:24-52, src/eou.cpp:113-146) -------- */
/* A pk_stream is n_streams independent streaming sessions advanced in LOCK-STEP on one GPU (BASELINE configs[4]: 16 concurrent
 * streams per GPU): every push hands EACH stream the same number of samples.  The model is a TDT-joint model loaded with
 * pk_model_load / pk_model_to_gpu (the streaming encoder uses the offline encoder's tensor names, streaming_encoder.cpp:276-428).
 * State kept per stream: pre-emphasis carry + overlap samples (StreamingAudioPreprocessor, audio.cpp:171-259), leftover mel
 * frames, per-layer K/V and conv caches (EncoderCache, streaming_encoder.hpp:25-41), LSTM state + last token + frame offset
 * (StreamingDecodeState, eou.hpp:80-87).  att_context_left / right: StreamingEncoderConfig (streaming_encoder.hpp:17-23;
 * Nemotron 70 / latency_frames, EOU 70 / 1).  pk_config.xscaling is honoured (the Sortformer NEST preset sets it:
 * streaming_encoder.cpp:444-447); the SiLU subsampling variant of that config is not implemented (no shipped preset enables it). */
typedef struct pk_stream pk_stream;
pk_status pk_stream_create(pk_model *m, int n_streams, int att_context_left, int att_context_right, pk_stream **out);
void pk_stream_free(pk_stream *s);
pk_status pk_stream_reset(pk_stream *s);    /* NemotronTranscriber::reset (nemotron.cpp:54-58) */
/* pcm[n_streams][n_samples] -> the tokens each stream emitted for this chunk: ids/start/end/conf [n_streams][max_tokens]
 * (start / end: encoder frames since the stream began, eou.cpp:77-79), lens[n_streams] (0 while audio is still being buffered).
 * Limit: one push carries at most 79 360 samples (4.96 s = 62 encoder frames: the per-chunk decode workspace); a longer push is rejected
 * with PK_ERR_UNSUPPORTED BEFORE any carried state changes -- split it into several pushes (the reference's chunks are 1-14 frames). */
pk_status pk_stream_push(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                         int32_t *end, float *conf);
/* the three stages of a push, on host buffers, for parity tests (each consumes / updates the same carried state):
 * process_chunk -> out[n_streams][*n_frames][mel_bins] (un-normalised log-mel); forward_chunk -> enc[n_streams][*n_out][hidden];
 * rnnt_streaming_decode_chunk.  *n_frames / *n_out = 0: everything was buffered. */
pk_status pk_stream_mel(pk_stream *s, const float *pcm, int n_samples, float *out, int cap_frames, int *n_frames);
pk_status pk_stream_encode(pk_stream *s, const float *mel, int n_frames, float *enc, int cap_frames, int *n_out);
pk_status pk_stream_decode(pk_stream *s, const float *enc, int n_frames, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                           int32_t *end, float *conf);
/* rnnt_streaming_decode_chunk (src/eou.cpp:17-98) of every stream along a GIVEN decision path -- the streaming counterpart of pk_tdt_score
 * (parity tests of the tolerance-class mode: "TDT logits within stated fp tolerance").  enc[n_streams][n_frames][hidden]; stream s walks
 * n_steps[s] decisions labels[s][k] / dur_idx[s][k] (both [n_streams][cap]; a duration as an index into pk_config.durations) instead of its
 * argmax, and the joint's outputs of every step (TDTJoint::forward, src/tdt.cpp:15-24) are recorded: label_logp[n_streams][cap][vocab]
 * (may be NULL), dur_logp[n_streams][cap][num_durations] (may be NULL); rows beyond a stream's steps are zero.  The LSTM state, last token
 * and frame offset each stream carries into its next chunk are the ones that path leaves (StreamingDecodeState, eou.hpp:80-87).
 * n_done[n_streams] (may be NULL) = steps walked (= n_steps[s] for a path the reference's loop can take on this chunk). */
pk_status pk_stream_score(pk_stream *s, const float *enc, int n_frames, const int32_t *labels, const int32_t *dur_idx, const int32_t *n_steps,
                          int cap, float *label_logp, float *dur_logp, int32_t *n_done);

/* ---- streaming TDT keyword spotting: wake words on live audio (kernels/tdt_kws_stream.hip) ------------------
 * The walk of pk_tdt_kws, stopped at every chunk boundary and picked up again from a state carried on the device, and a hit rule that needs no
 * future frame.  Specification: tests/tdt_kws_stream_ref.py (ChunkWalk + OnlinePick), matched bit for bit.  The rule keeps one pending hit per
 * (stream, keyword) pair, fed frame by frame: (1) a pending hit leaves when t > its end + patience; (2) frame t qualifies when E[t] > -inf,
 * E[t] >= min_score and Bs[t] lies after the end of the last hit that left; (3) with nothing pending it becomes the pending hit; (4) where its span [Bs[t], Ee[t]] meets the pending span it replaces the
 * pending hit only when E[t] is strictly larger; (5) where it does not, the pending hit leaves and the frame becomes pending.  This is an online
 * approximation of pk_tdt_kws's greedy picking: a pending hit that was replaced is never reported.  Frames count from the start of the session
 * (the last reset), spans are inclusive, and a span's end is t + max(duration, 1) - 1 without a clamp: it may lie past the frames seen so far.
 * PK_ERR_INVALID: whatever pk_tdt_kws refuses that way (an empty keyword, an id outside [0, V) or equal to blank, min_score > 0 or NaN), patience < 0,
 * n_frames < 1.  PK_ERR_UNSUPPORTED, before anything is allocated: a keyword of more than 64 tokens, D outside 1 .. 8, a duration outside [0, 8], more
 * than 256 keywords or 65536 pairs, more than 62 frames in one call, more than 1 GiB of carried state plus lattice at the 62-frame limit, and for
 * a session: a model without a TDT joint, gemm_bf16. */
typedef struct pk_stream_kws_options {
    float min_score;           /* -inf: every frame with a path qualifies */
    int32_t patience;          /* 0: frames to wait after a pending hit's end before it leaves */
} pk_stream_kws_options;
typedef struct pk_kws_event {
    int32_t stream, keyword, start, end;   /* frames since the stream began, inclusive */
    float score;
} pk_kws_event;
void pk_stream_kws_options_default(pk_stream_kws_options *out);
/* The chunked walk and the online rule alone, on host lattices (no model): the counterpart of pk_tdt_kws.  n_pairs walks, pair p with a keyword
 * of kw_len[p] tokens.  A push hands every pair the lattice rows of the next c frames (1 <= c <= 62), packed as for pk_tdt_kws with n_frames = c
 * for every pair.  E / Bs / Ee [n_pairs][c] (each may be NULL): the exit rows of the push.  events: ordered by pair, then by emission; the first
 * `cap` are written and *n_events is the total (cap = n_pairs * c never truncates); an event names its pair in `keyword` (stream = 0). */
typedef struct pk_tdt_kws_chunk pk_tdt_kws_chunk;
pk_status pk_tdt_kws_chunk_create(const int32_t *durations, int D, int n_pairs, const int32_t *kw_len, const pk_stream_kws_options *opt,
                                  pk_tdt_kws_chunk **out);
pk_status pk_tdt_kws_chunk_push(pk_tdt_kws_chunk *w, const float *lab, const float *blk, const float *dl, const float *top, int c, float *E,
                                int32_t *Bs, int32_t *Ee, pk_kws_event *events, int cap, int *n_events);
/* emits every pending hit (ordered by pair) */
pk_status pk_tdt_kws_chunk_flush(pk_tdt_kws_chunk *w, pk_kws_event *events, int cap, int *n_events);
/* back to frame 0: the carried state and the pending hits are cleared */
pk_status pk_tdt_kws_chunk_reset(pk_tdt_kws_chunk *w);
void pk_tdt_kws_chunk_free(pk_tdt_kws_chunk *w);
/* On a streaming session: every keyword is watched in every stream, pair = stream * n_kw + keyword.  Keywords as phrases (needs the model's
 * vocabulary) or as ids + kw_offsets[n_kw + 1]; n_kw = 0 clears the set.  The prediction net runs here, once per distinct keyword.  A refused call
 * leaves the set in place as it was.  pk_stream_reset keeps the keywords, clears the walk and the pending hits and restarts the frame numbering.
 * pk_stream_push, pk_stream_decode and pk_stream_reset return what they return without keywords; they do not feed the walk: a session that spots
 * hands every chunk to pk_stream_spot or pk_stream_push_spot, and an event's frames count the frames those calls have seen. */
pk_status pk_stream_set_keywords(pk_stream *s, const char *const *phrases_or_null, const int32_t *ids_or_null, const int32_t *kw_offsets, int n_kw,
                                 const pk_stream_kws_options *opt);
/* Stage form: enc [n_streams][n_frames][hidden] on the host, as pk_stream_decode takes it (1 <= n_frames <= 62).  E / Bs / Ee
 * [n_streams * n_kw][n_frames], each may be NULL. */
pk_status pk_stream_spot(pk_stream *s, const float *enc, int n_frames, float *E, int32_t *Bs, int32_t *Ee, pk_kws_event *events, int cap,
                         int *n_events);
/* pk_stream_push that also walks the chunk's frames: the same tokens, and the events of this push in the same host round trip. */
pk_status pk_stream_push_spot(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                              int32_t *end, float *conf, pk_kws_event *events, int cap, int *n_events);
pk_status pk_stream_spot_flush(pk_stream *s, pk_kws_event *events, int cap, int *n_events);
/* Stage timers (tools/bench_stream_kws.py): pk_stream_spot `reps` times after one warm-up on the same rows, HIP events, medians: ms[0] = enc_proj +
 * lattice, ms[1] = normalisation + walk + rule.  The walk's state advances by reps + 1 chunks. */
pk_status pk_stream_spot_timed(pk_stream *s, const float *enc, int n_frames, int reps, float ms[2]);

/* ---- endpointing on live audio: utterance boundaries in streaming pushes (kernels/endpoint.hip) -------------
 * When did the speaker start, and when have they finished: START / END events on the log-mel rows a streaming push already leaves on the device
 * ([n_frames][n_mels] raw ln(mel + 2^-24) per stream, as pk_stream_mel returns them; 10 ms per frame).  Specification: tests/endpoint_ref.py, matched
 * bit for bit.  Per frame: the level (the fp32 sum of the frame's bins in a fixed order), the noise floor (the exact minimum of the last floor_window
 * levels: causal, where pk_vad's percentile needs the whole clip), speech0 = level > fmaxf(n_mels threshold_db ln10/10, floor + n_mels margin_db ln10/10).
 * The rule, frame by frame: min_speech speech frames in a row open an utterance (START; start = the first of them); inside one, min_silence frames
 * without speech in a row end it (END / SILENCE; end = the last speech frame), else its max_utterance-th frame ends it (END / MAX_LENGTH; end = that
 * frame).  At most one event per frame and stream; they do not depend on how the audio was cut into pushes.  Token rule (eou_token_id >= 0, sessions
 * only): a push that returns that token id for a stream emits END / TOKEN for it (start = the open utterance's, or the event's own frame where none is
 * open; end = at = the last mel frame the push fed) and closes the stream's acoustic state (outside an utterance, no speech run).  Close: with
 * reset_decoder set, a stream for which any END fired in a push has its prediction-net state put back to what pk_stream_reset gives it (h = c = 0, last
 * token = blank) after that push's decode and before the next push's: the tokens the push returned belong to the utterance that ended, and because the
 * close takes effect at a push boundary the transcript after it depends on the chunking (the acoustic events do not).  The noise-floor window, the
 * encoder caches, the mel leftovers, the frame numbering and a keyword walk are not touched.
 * Frames count the mel frames the endpoint calls have seen since the last reset; the encoder frame of a mel frame is frame / 8.
 * The defaults are choices, not measurements (as pk_vad_options' are): threshold_db and margin_db are section 5.8's figures read as the mean
 * log-mel power per bin.
 * PK_ERR_INVALID: min_speech_ms < 10, min_silence_ms < 10, floor_window_ms < 10, max_utterance_s * 100 < min_speech frames + 1, a NaN threshold_db or
 * margin_db, eou_token_id outside [-1, vocabulary) or equal to the blank, a call with no rows, endpointing with no options set, kws outputs with no
 * keywords set.  PK_ERR_UNSUPPORTED, before anything is allocated: floor_window above 1024 frames, more than 512 frames in one call, n_mels > 512, a
 * gemm_bf16 model.  A refused set leaves the previous options in place. */
typedef struct pk_endpoint_options {
    float threshold_db;        /* -50: absolute level below which a frame is never speech (mean log-mel power per bin, dB) */
    float margin_db;           /* 9: ... and it must exceed the noise floor by this much */
    int32_t floor_window_ms;   /* 3000 */
    int32_t min_speech_ms;     /* 100 */
    int32_t min_silence_ms;    /* 500 */
    float max_utterance_s;     /* 30 */
    int32_t eou_token_id;      /* -1: no token rule */
    int32_t reset_decoder;     /* 1 */
} pk_endpoint_options;
enum { PK_ENDPOINT_START = 1, PK_ENDPOINT_END = 2 };
enum { PK_ENDPOINT_NONE = 0, PK_ENDPOINT_SILENCE = 1, PK_ENDPOINT_MAX_LENGTH = 2, PK_ENDPOINT_TOKEN = 3 };
typedef struct pk_endpoint_event {
    int32_t stream, kind, reason;
    int32_t start, end, at;    /* mel frames since the reset, inclusive; at: the frame at which the event was emitted */
} pk_endpoint_event;
void pk_endpoint_options_default(pk_endpoint_options *out);
/* The kernel and the rule alone, on host rows (needs a device, no model).  A push hands every stream its next n rows: rows [n_streams][n][n_mels],
 * 1 <= n <= 512.  level / floor / speech0 [n_streams][n] (each may be NULL).  events: ordered by stream, then by emission; the first `cap` are
 * written and *n_events is the total (cap = n_streams * n never truncates).  _close: the acoustic close of the streams with mask[s] != 0. */
typedef struct pk_endpoint_chunk pk_endpoint_chunk;
pk_status pk_endpoint_chunk_create(int n_streams, int n_mels, const pk_endpoint_options *opt, pk_endpoint_chunk **out);
pk_status pk_endpoint_chunk_push(pk_endpoint_chunk *w, const float *rows, int n, float *level, float *floor, int32_t *speech0,
                                 pk_endpoint_event *events, int cap, int *n_events);
pk_status pk_endpoint_chunk_close(pk_endpoint_chunk *w, const uint8_t *mask);
/* back to frame 0: the window and the rule's state are cleared, the options stay */
pk_status pk_endpoint_chunk_reset(pk_endpoint_chunk *w);
void pk_endpoint_chunk_free(pk_endpoint_chunk *w);
/* On a streaming session.  opt NULL clears the endpointer; a set starts it at frame 0 of the endpoint calls that follow.  pk_stream_reset keeps the
 * options and clears the state.  pk_stream_push, pk_stream_push_spot and pk_stream_decode return what they return without it and do not feed it. */
pk_status pk_stream_set_endpointing(pk_stream *s, const pk_endpoint_options *opt_or_null);
/* Stage form: mel_rows [n_streams][n_frames][n_mels] on the host, as pk_stream_mel returns them.  No token rule (no tokens). */
pk_status pk_stream_endpoint(pk_stream *s, const float *mel_rows, int n_frames, float *level, float *floor, int32_t *speech0,
                             pk_endpoint_event *events, int cap, int *n_events);
/* pk_stream_push that also feeds the endpointer the push's mel frames: the same tokens, and the events in the same host round trip.  With
 * kws_events / kws_n_events non-NULL the call is pk_stream_push_spot too (keywords must be set): wake word, transcript and end of turn from one push. */
pk_status pk_stream_push_endpoint(pk_stream *s, const float *pcm, int n_samples, int max_tokens, int32_t *ids, int32_t *lens, int32_t *start,
                                  int32_t *end, float *conf, pk_endpoint_event *events, int cap, int *n_events, pk_kws_event *kws_events,
                                  int kws_cap, int *kws_n_events);
/* The close without the endpointer: the prediction-net state of the streams with mask[s] != 0 becomes what pk_stream_reset gives it; nothing else
 * is touched.  For a caller with an end-of-turn policy of its own. */
pk_status pk_stream_reset_decoder(pk_stream *s, const uint8_t *mask);
/* Stage timer (tools/bench_stream_endpoint.py): the chunk kernel alone on the given rows `reps` times after one warm-up, HIP events, the median in
 * ms[0].  The endpointer's state advances by reps + 1 chunks. */
pk_status pk_stream_endpoint_timed(pk_stream *s, const float *mel_rows, int n_frames, int reps, float ms[1]);

/* ---- plain Transformer encoder: TransformerEncoder::forward / TransformerBlock::forward (src/transformer.cpp:15-88) ------------ */
/* include/parakeet/transformer.hpp:12-21 (TransformerConfig), dropout omitted (inference). */
typedef struct pk_transformer_config {
    int32_t hidden_size;       /* 192 */
    int32_t num_layers;        /* 18 */
    int32_t num_heads;         /* 8 (heads narrower than 32 are zero-padded internally: same bits) */
    int32_t ffn_intermediate;  /* 768 */
    int32_t pre_ln;            /* 1 = pre-norm (x + f(LN(x))), 0 = post-norm (LN(x + f(x))) */
    int32_t has_final_norm;
    float layer_norm_eps;      /* 1e-5 */
} pk_transformer_config;
typedef struct pk_transformer pk_transformer;
/* Tensors <prefix>layers_.<i>.{norm1_,norm2_,mha_.{q,k,v,out}_proj,fc1_,fc2_}.{weight,bias} [+ <prefix>final_norm_.*] of a
 * safetensors file (the module tree of transformer.cpp:12,69-73), uploaded to `device`. */
pk_status pk_transformer_load(const char *safetensors_path, const char *prefix, const pk_transformer_config *cfg, int device,
                              pk_transformer **out);
/* x[B][T][hidden] -> y[B][T][hidden] (host buffers).  The optional attention mask of the reference (transformer.cpp:40-42) is
 * not supported: no caller on the ASR path passes one. */
pk_status pk_transformer_forward(pk_transformer *t, const float *x, int B, int T, float *y);
void pk_transformer_free(pk_transformer *t);

/* ---- preprocess_audio on its own (include/parakeet/audio.hpp:7-30, src/audio.cpp:100-158): the mel front end without a model, for callers
 * that hand features to pk_sortformer_forward / pk_encode themselves.  feats: [pk_mel_num_frames(n_samples)][n_mels]; normalize = 0 is
 * AudioConfig::normalize = false (raw log-mel, what Sortformer takes); stft_window_centered: switch A1 of pk_config. */
typedef struct pk_frontend pk_frontend;
pk_status pk_frontend_create(int n_mels, int normalize, int stft_window_centered, int device, pk_frontend **out);
pk_status pk_frontend_features(pk_frontend *f, const float *pcm, int64_t n_samples, float *feats, int *n_frames);
void pk_frontend_free(pk_frontend *f);

/* ---- Sortformer speaker diarization (include/parakeet/sortformer.hpp:28-129, src/sortformer.cpp:41-121) ------------------------
 * NEST FastConformer (offline Conformer path, xscaling, weights under "nest_encoder_.") -> projection_ -> TransformerEncoder
 * ("transformer_.") -> relu -> first_hidden_ -> relu -> output_proj_ -> sigmoid.  One handle = weights on one device. */
typedef struct pk_sortformer_config {   /* SortformerConfig (sortformer.hpp:28-41) */
    pk_config nest;                     /* encoder fields only: vocab_size = ctc_vocab_size = 0, xscaling = 1, mel_normalize_off = 1 */
    pk_transformer_config transformer;
    int32_t max_speakers;               /* 4 */
    float activity_threshold;           /* 0.5 */
    int32_t att_context_left;           /* 70: StreamingEncoderConfig of the NEST encoder (sortformer.hpp:53-54), used by diarize_chunk */
    int32_t att_context_right;          /* 0 */
} pk_sortformer_config;
typedef struct pk_sortformer pk_sortformer;
void pk_sortformer_config_preset(pk_sortformer_config *out);              /* make_sortformer_117m_config (sortformer.hpp:43-76) */
pk_status pk_sortformer_load(const char *safetensors_path, const pk_sortformer_config *cfg, int device, pk_sortformer **out);
void pk_sortformer_free(pk_sortformer *s);
/* Sortformer::forward (:50-69): feats[B][Tm][mel_bins] -> probs[B][T][max_speakers], T = pk_encoder_num_frames(Tm) (also in *T_out). */
pk_status pk_sortformer_forward(pk_sortformer *s, const float *feats, int B, int Tm, float *probs, int *T_out);
/* preprocess_audio with normalize = false (src/main.cpp:513-517, src/diarize.cpp:81-88) + forward, for n_clips clips of n_samples. */
pk_status pk_sortformer_forward_pcm(pk_sortformer *s, const float *pcm, int n_clips, int64_t n_samples, float *probs, int *T_out);
/* Sortformer::diarize_chunk (:123-150), one streaming session per handle: forward_chunk of the NEST encoder on cached K / V / conv
 * state (the streaming path of pk_stream_*), then projection / transformer / head on THIS chunk's frames.  feats[n_frames][mel_bins]
 * (un-normalised log-mel, any chunking) -> probs[c][max_speakers]; *T_out = c (0: all frames were buffered: the subsampling consumes
 * multiples of 8).  AOSCCache::update and probs_to_segments on the chunk are host loops (pk_sortformer_segments). */
pk_status pk_sortformer_diarize_chunk(pk_sortformer *s, const float *feats, int n_frames, float *probs, int cap_frames, int *T_out);
pk_status pk_sortformer_stream_reset(pk_sortformer *s);
/* Sortformer::probs_to_segments (:71-113) on one utterance's probs[T][S]: runs of prob > threshold per speaker, seconds = frame * 0.08,
 * sorted by start.  Writes at most cap segments, returns the number found. */
int pk_sortformer_segments(const float *probs, int T, int S, float threshold, int32_t *speaker, float *start, float *end, int cap);

/* ---- host-side text (src/vocab.cpp:29-117, src/timestamp.cpp:24-111) -------------------------------------- */
int pk_vocab_size(const pk_model *m);
/* Tokenizer::decode -> returns needed length; writes at most cap-1 bytes + NUL. */
int pk_detokenize(const pk_model *m, const int32_t *ids, int n, char *out, int cap);
/* Tokenizer::encode (greedy longest match) -> number of ids (writes at most cap). */
int pk_tokenize(const pk_model *m, const char *text, int32_t *ids, int cap);
/* Phrase boosting (include/parakeet/phrase_boost.hpp:22-116, src/phrase_boost.cpp): a ContextTrie over token sequences biases
 * the CTC / TDT greedy argmax by +boost_score towards tokens that continue a phrase.  The trie lives on the device with the
 * model; once set, pk_ctc_decode, pk_tdt_decode, pk_batch_run and pk_transcribe_pcm decode boosted (confidences stay the
 * unboosted probabilities).  n_phrases = 0 switches boosting off.  Phrases are limited to 63 tokens.  RNNT decode and streaming
 * sessions have no boosted variant in the reference: PK_ERR_UNSUPPORTED while boosting is on.
 * pk_set_boost_tokens: phrase i = ids[offsets[i] .. offsets[i+1])  (ContextTrie::insert, :11-27; empty phrases are ignored).
 * pk_set_boost_phrases: ContextTrie::build (:29-37) -- Tokenizer::encode of each phrase; needs a vocabulary. */
pk_status pk_set_boost_tokens(pk_model *m, const int32_t *ids, const int32_t *offsets, int n_phrases, float boost_score);
pk_status pk_set_boost_phrases(pk_model *m, const char *const *phrases, int n_phrases, float boost_score);
/* number of trie nodes (ContextTrie::size, 1 = root only), 0 when boosting is off */
int pk_boost_trie_size(const pk_model *m);
/* group_timestamps: words '\n'-joined into `words`; returns the word count. sentences!=0 -> TimestampMode::Sentences. */
int pk_group_timestamps(const pk_model *m, const int32_t *ids, const int32_t *start, const int32_t *end, const float *conf,
                        int n, int sentences, char *words, int cap, float *wstart, float *wend, float *wconf, int wcap);

/* ---- diagnostics used by the GPU parity tests (single kernels behind the same ABI) ------------------------ */
/* Device math, elementwise: fn 0 exp, 1 log, 2 tanh, 3 sigmoid, 4 silu, 5 sqrt, 6 reciprocal, 7 relu, 8 / 9 sigmoid / silu as the GEMM
 * epilogues evaluate them (guarded short sequences, pk_devmath.h), 20 / 21 sigmoid / silu on the hardware exp2 and rcp (GemmArgs::fast_act: the
 * bf16 mode's epilogues; within a derived bound of the exact value, tests/test_gpu_bf16_tile_gemm.py). */
pk_status pk_diag_math(int fn, const float *in, float *out, int64_t n);
/* Every one of the 2^32 bit patterns of x through a device-side identity (kernels/norm.hip, math_exhaustive_kernel): fn 3 / 4 = wherever the
 * short sigmoid / SiLU instruction sequences of the GEMM epilogues claim validity they equal the specification's value; fn 13 / 14 = the guarded
 * four-at-a-time forms equal the specification on every pattern.  checked = patterns examined, mismatches must be 0, first_bad = lowest
 * mismatching pattern (2^32 when none).  About 0.1 s. */
pk_status pk_diag_math_exhaustive(int fn, uint64_t *checked, uint64_t *mismatches, uint64_t *first_bad);
/* out[M][N] = epi(A[M][K] * W[N][K]^T + bias) with the production fp32-MFMA GEMM.  epi: 0 none, 1 relu, 2 silu,
 * 3 residual: out = resid + alpha*(acc+bias), 4 glu (N even: out[M][N/2] = a * sigmoid(b)). */
pk_status pk_diag_gemm(int M, int N, int K, const float *A, const float *W, const float *bias, int epi,
                       const float *resid, float alpha, float *out);
/* The bf16-operand / fp32-accumulate GEMM of pk_config.gemm_bf16 (W is given in fp32 and rounded here like at upload); K % 64 == 0. */
pk_status pk_diag_gemm_bf16(int M, int N, int K, const float *A, const float *W, const float *bias, int epi,
                            const float *resid, float alpha, float *out);
/* The same with the activations stored as bf16 before the product (rounded here; in the engine the producing kernel's epilogue stores them so):
 * large shapes take the direct-to-LDS kernel (kernels/gemm_bf16_glds.hpp). */
pk_status pk_diag_gemm_bf16_a16(int M, int N, int K, const float *A, const float *W, const float *bias, int epi,
                                const float *resid, float alpha, float *out);
/* The small-M form of that product with the LayerNorm of its input rows folded in (kernels/gemm_smallm_bf16.hip; the streaming chunks of the
 * tolerance-class mode): out = epi(bf16(LayerNorm(A; gamma, beta, eps)) * bf16(W)^T + bias).  M <= 128, K = 256 * (1 .. 8; glu: .. 4).
 * PK_ERR_UNSUPPORTED for any other shape. */
/* The bf16 diag products (pk_diag_gemm_bf16*, pk_diag_ln_gemm_bf16, pk_diag_glu_dwconv_bf16, pk_diag_ffn_bf16_smallm) hand the small-M kernel
 * its weights ALSO as operand tiles (kernels.hpp GemmArgs::W_t16), as a streaming session does; on = 0 keeps the natural layout only.  Process-wide
 * test switch; both give the same bits. */
pk_status pk_diag_smallm_bf16_tiles(int on);
pk_status pk_diag_ln_gemm_bf16(int M, int N, int K, const float *A, const float *gamma, const float *beta, float eps, const float *W,
                               const float *bias, int epi, const float *resid, float alpha, float *out);
/* Two LayerNorms in front of a product (a block's final_norm_ folded, with the next block's first norm, into that block's fc1; streaming,
 * tolerance-class mode): out = silu(bf16(LN(LN(A; pre_gamma, pre_beta); gamma, beta)) bf16(W)^T + bias), pre_out [M][K] = LN(A; pre_gamma, pre_beta)
 * (the residual stream of the block that starts there).  M <= 128, K = 256 * (1 .. 8). */
pk_status pk_diag_ln2_gemm_bf16(int M, int N, int K, const float *A, const float *pre_gamma, const float *pre_beta, const float *gamma, const float *beta,
                                float eps, const float *W, const float *bias, float *out, float *pre_out);
/* The conv module's first half on a streaming chunk of the tolerance-class mode: GLU(bf16(LayerNorm(A)) bf16(W)^T + bias) -> causal depthwise
 * conv (kernel 9) over [cache_in ; the c new rows] of every stream -> BatchNorm -> SiLU (reference src/streaming_encoder.cpp:41-78).  A = [n_streams * c][d]
 * rows, stream-major; W [2 d][d]; cache_in / cache_out [n_streams][8][d]; gamma = beta = NULL: A is taken as it is.  fused = 1: the conv runs in
 * the product's epilogue (kernels.hpp DwTail; c = 1, 2 or 4), fused = 0: the separate kernel -- both bit for bit the same (tests/test_gpu_bf16.py). */
pk_status pk_diag_glu_dwconv_bf16(int n_streams, int c, int d, const float *A, const float *gamma, const float *beta, float eps, const float *W,
                                  const float *bias, const float *cache_in, int has_cache, const float *dw_w, const float *dw_bias,
                                  const float *bn_mean, const float *bn_rstd, const float *bn_g, const float *bn_b, int fused, float *out,
                                  float *cache_out);
/* One feed-forward module of a streaming chunk in the tolerance-class mode, on the small-M bf16 kernel: out = x + 0.5 * (W2 bf16(silu(W1 bf16(LN(x)) + b1)) + b2)
 * (reference src/encoder.cpp:36-46), x [M][d], W1 [f][d], W2 [d][f].  act_tiles = 1: the fc1 activations travel in the kernel's 8-row operand
 * tiles (kernels.hpp GemmArgs::out_t8 / a_t8; M % 8 == 0), 0: as rows -- bit for bit the same (tests/test_gpu_bf16.py). */
pk_status pk_diag_ffn_bf16_smallm(int M, int d, int f, const float *x, const float *gamma, const float *beta, float eps, const float *W1, const float *b1,
                                  const float *W2, const float *b2, int act_tiles, float *out);
pk_status pk_diag_layernorm(const float *x, int64_t rows, int d, const float *gamma, const float *beta, float eps, float *y);
/* LayerNorm + product on a LARGE fp32 batch (round 6; reference src/encoder.cpp:40-41, :60-61, :182-183: norm, then Linear / pointwise conv):
 * out = epi(LN(X; gamma, beta, eps) W^T + bias), X [M][K], W [N][K] (glu: [2N][K]), epi 0 none / 1 relu / 2 silu / 4 glu.
 * fold = 0: the separate LayerNorm launch, then the tile GEMM on the normalised rows.  fold = 1: a statistics pass ({mean, rstd} per row) and the tile
 * GEMM normalising while it stages its A tiles (kernels/gemm_pipe.hpp, LNA) -- what the encoder of a batch runs; bit for bit the same.
 * pre_gamma / pre_beta (both or neither): X = LN(A; pre_gamma, pre_beta) first -- a block's final_norm_ in front of the next block's ffn1 norm; y1 (optional,
 * [M][K]) receives X.  fold = 1 then writes X and takes the statistics of X's rows in one launch (launch_layernorm_then_stats).
 * PK_ERR_UNSUPPORTED where the engine would not fold (M <= 1536, N < 1024 for the non-glu epilogues, K % 32). */
pk_status pk_diag_ln_gemm(int M, int N, int K, const float *A, const float *pre_gamma, const float *pre_beta, const float *gamma, const float *beta, float eps,
                          const float *W, const float *bias, int epi, int fold, float *out, float *y1);
/* sum64 of each row of x[rows][n] (the canonical wavefront reduction). */
pk_status pk_diag_sum64(const float *x, int rows, int n, float *out);
/* One relative-position attention layer alone (reference src/encoder.cpp:135-171), on the production kernel the encoder runs:
 * kernel 0 = the fp32 kernel (kernels/attention.hip; hd 32 / 64 / 96 / 128; past its LDS limit the global-scratch variant),
 * kernel 1 = the bf16 kernel of the tolerance-class mode (kernels/attention_bf16.hip; hd 64 / 128; qkv and pos are rounded to bf16 here, RNE,
 * and c = (v - u) . P is formed on the device by the engine's kernel).  hd = d / n_heads.
 * qkv [rows][3 d] natural columns (q | k | v), pos [2 pos_T - 1][d] (the projected position table of pos_T >= T frames: the kernel reads its
 * window, rows pos_T - T ..), bias_u / bias_v [d].  lens = NULL: a uniform batch of B x T frames (rows = B T); otherwise a ragged (packed) batch of
 * B utterances of lens[b] frames (rows = sum lens; T is ignored, pos_T >= max lens).
 * ctx receives [rows + PK_DIAG_ATTENTION_GUARD_ROWS][d] floats (bf16 results widened): the device buffer is filled with a NaN pattern before the
 * launch -- fp32 0x7FC5A5A5, bf16 0x7FC5 (widened 0x7FC50000) -- so elements the kernel did not write come back as that pattern.
 * variant (may be NULL): bit 0 = the score block went to global scratch, bit 1 = ragged instantiation, bit 2 = the bf16 kernel. */
#define PK_DIAG_ATTENTION_GUARD_ROWS 128
pk_status pk_diag_relpos_attention(int kernel, int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv, const float *pos, int pos_T,
                                   const float *bias_u, const float *bias_v, float *ctx, int *variant);
/* The fp32 kernel of pk_diag_relpos_attention with the kernel form chosen by the caller: form 0 = the one the encoder would run, 1 = the block
 * form (32 query rows per workgroup, the score block in LDS), 2 = the strip form (one wave per 16 query rows, the scores in registers; head size
 * 32 / 64, longest sequence <= 128 frames).  A form that does not cover the shape is PK_ERR_UNSUPPORTED, never another kernel.  out_mode: 0 fp32
 * ctx, 1 ctx rounded to bf16 with the fast exp / reciprocal of the bf16 mode (widened here, unwritten 0x7FC50000), 2 fp32 ctx in the sigma column
 * layout.  pos may be NULL (bias_u / bias_v / pos_T ignored): scores are the scaled content term only.  Everything else as above.
 * form_ran (may be NULL): 1 or 2. */
pk_status pk_diag_relpos_attention_form(int form, int out_mode, int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv,
                                        const float *pos, int pos_T, const float *bias_u, const float *bias_v, float *ctx, int *form_ran);
/* One limited-context attention layer alone on the band kernel the encoder runs in local mode (kernels/attention.hip, BAND instantiation): query row i of an
 * utterance attends to keys [max(0, i - left), min(T - 1, i + right)] (left, right >= 0).  qkv, bias_u, bias_v, B, lens, T as for
 * pk_diag_relpos_attention; pos [left + right + 1][d] is the LOCAL table, row r the projected position i - j = left - r.  out_mode 0: fp32 ctx,
 * 1: ctx rounded to bf16 (the engine's gemm_bf16 mode; widened to fp32 here, unwritten pattern 0x7FC50000).  ctx: [rows +
 * PK_DIAG_ATTENTION_GUARD_ROWS][d], NaN-filled before the launch as above.  PK_ERR_UNSUPPORTED past the LDS limit of
 * pk_model_set_attention_context.  variant (may be NULL): bit 1 = ragged instantiation, bit 3 = the band kernel ran, bit 4 = bf16 output. */
pk_status pk_diag_relpos_local_attention(int B, const int32_t *lens, int T, int d, int n_heads, const float *qkv, const float *pos, int left, int right,
                                         const float *bias_u, const float *bias_v, int out_mode, float *ctx, int *variant);
/* The cached attention of the streaming encoder alone (kernels/stream.hip; reference src/streaming_encoder.cpp:162-272), launched as a session
 * launches it for S lock-step streams: qkv_new [S c][3 d] natural columns (q | k | v of the chunk's c rows per stream), kcache / vcache
 * [S][cache_rows][d] of which the first nc rows of every stream are valid, pos [P][d] the projected position table (the kernel reads its last
 * nc + c rows), bias_u / bias_v [d], the [att_left, att_right] context (-1, -1: no mask), hd = d / n_heads (a multiple of 4).  rotate != 0: the
 * same launch writes the new caches, the last min(keep_max, nc + c) rows of [cache ; chunk] per stream, to cache_k_out / cache_v_out.
 * ctx_sigma != 0: the columns of ctx in the sigma layout the out-projection reads (d a multiple of 16).
 * ctx receives [S c + PK_DIAG_ATTENTION_GUARD_ROWS][d] floats, cache_k_out / cache_v_out (may be NULL when rotate == 0) [S cache_rows +
 * PK_DIAG_ATTENTION_GUARD_ROWS][d]: all three device buffers are filled with the pattern 0x7FC5A5A5 before the launch, so a word the launch did
 * not write comes back as that pattern.  form (may be NULL): the launch taken, by the function the launcher switches on.
 * PK_ERR_INVALID, and nothing is launched, for c <= 0, nc > cache_rows, P < nc + c, keep_max > cache_rows with rotate. */
#define PK_DIAG_STREAM_ATT_GENERAL_1W 0   /* stream_attention_kernel, one wavefront */
#define PK_DIAG_STREAM_ATT_GENERAL_2W 1   /* ... two wavefronts (more than 64 keys) */
#define PK_DIAG_STREAM_ATT_TILES_HD64 2   /* stream_attention_tiles_kernel, head size 64 */
#define PK_DIAG_STREAM_ATT_TILES_HD128 3  /* ... head size 128 */
pk_status pk_diag_stream_attention(int S, int c, int nc, int cache_rows, int d, int n_heads, const float *qkv_new, const float *kcache,
                                   const float *vcache, const float *pos, int P, const float *bias_u, const float *bias_v, int att_left,
                                   int att_right, int keep_max, int ctx_sigma, int rotate, float *ctx, float *cache_k_out, float *cache_v_out,
                                   int *form);
/* The mel front end alone (kernels/mel.hip; reference src/audio.cpp:100-158 and :222-252), without a model: the tables come from the builder the
 * models and pk_frontend use, for n_mels bins (1 .. 512: this entry's own limit, what one frame's LDS array holds), the window placed per stft_window_centered (switch A1), the power per power_via_abs (A2).
 *   form PK_DIAG_MEL_UNIFORM  n_clips clips of n_samples each, pcm [n_clips][n_samples]; offsets NULL.  launch_mel_logmel, then launch_mel_normalize
 *                             with the normalize flag: logmel = [clip][n_mels][pitch], pitch = frames rounded up to 16; feats = [clip][frames][n_mels].
 *   form PK_DIAG_MEL_RAGGED   clip i = pcm[offsets[i] .. offsets[i + 1]) (n_samples ignored), the ragged launch of the same two: the clips' log-mel
 *                             blocks [n_mels][pitch of clip i] one behind the other, feats packed along the frames.
 *   form PK_DIAG_MEL_STREAM   launch_mel_stream on pcm [n_clips][n_samples] as given: an ALREADY pre-emphasised signal, frame t = samples
 *                             [160 t, 160 t + 400); logmel = [clip][frames][n_mels], no normalise step (feats stays untouched).
 * logmel / feats receive logmel_words / feats_words floats each: the device buffer of that many words is filled with PK_DIAG_MEL_FILL before the
 * launch and copied back whole, so a word no launch wrote (pad columns, spare words) comes back as the fill.  Each must hold what the launches write
 * plus at least PK_DIAG_MEL_SPARE_WORDS.  n_frames [n_clips]: the frame count of every clip; grid [6]: the log-mel launch's grid x, y and threads per
 * workgroup, then the normalise launch's (0 0 0 for the streaming form).
 * PK_ERR_INVALID, before anything is allocated or launched: a clip of 256 samples or fewer (offline), fewer than 400 samples (streaming), n_mels < 1;
 * PK_ERR_UNSUPPORTED: a filterbank of more packed taps than the kernel stages (no n_mels gives one today: at most 514 taps against 768). */
#define PK_DIAG_MEL_UNIFORM 0
#define PK_DIAG_MEL_RAGGED 1
#define PK_DIAG_MEL_STREAM 2
#define PK_DIAG_MEL_FILL 0x7FC5A5A5u
#define PK_DIAG_MEL_SPARE_WORDS 64
pk_status pk_diag_mel(int n_mels, int normalize, int stft_window_centered, int power_via_abs, int form, const float *pcm, int n_clips, int64_t n_samples,
                      const int64_t *offsets, float *logmel, int64_t logmel_words, float *feats, int64_t feats_words, int32_t *n_frames, int32_t *grid);
/* Which instantiation of the convolution kernels outside the GEMM the engine launches for this model and batch, computed by the functions the
 * launchers themselves switch on (kernels/kernels.hpp: sub_conv1_dw1_inst, sub_dw_inst, dwconv_inst, stream_dwconv_inst).  Host arithmetic only: no
 * device is needed.  The batch is B utterances of Tm mel frames each (n_mel_frames = NULL), or a ragged batch of B utterances of n_mel_frames[b]
 * frames (Tm ignored).  A batch of B x T encoder frames handed to pk_conformer_blocks is described by Tm = 8 T - 7.  stream_c > 0 adds the
 * streaming conv kernel for a chunk of stream_c encoder frames per session.  out receives PK_DIAG_CONV_VARIANT_WORDS words:
 *   [0..4]   conv1 + dw1:   instantiation id, 1 = the packed two-channel kernel / 0 = one channel per thread, XC (columns per chunk), YS (rows per
 *                           strip), the batch's total rows after dw1
 *   [5..6]   dw2:           instantiation id, XO (output columns per thread)
 *   [7..11]  conv module:   instantiation id, KC (taps), TT (frames per strip), body (0 = all rows loaded first, 1 = sliding window), total encoder frames
 *   [12..16] streaming conv (-1 each when stream_c <= 0): instantiation id, KC, CMAX, body (0 = the chunk in registers, 1 = the frame loop),
 *                           1 if that chunk size and conv size may instead run as the epilogue of the preceding product (kernels.hpp DwTail), else 0
 * pk_diag_conv_instantiations lists every instantiation those launchers can take as rows of five words {launcher (0 conv1 + dw1, 1 dw2, 2 conv
 * module, 3 streaming conv), instantiation id, and the three parameters reported above}; returns the number of rows (at most cap_rows are written). */
#define PK_DIAG_CONV_VARIANT_WORDS 17
pk_status pk_diag_conv_variants(const pk_model *m, int B, int Tm, const int32_t *n_mel_frames, int stream_c, int32_t *out);
int pk_diag_conv_instantiations(int32_t *out, int cap_rows);
/* The sequence lengths the model's two resident relative-position table sets were built for: out[0] the fp32 set's, out[1] the bf16 attention's
 * (0: not built yet).  A set holds 2 T - 1 rows per layer, is rebuilt when a call's longest utterance exceeds T, and serves every shorter one from a
 * window of its rows; limited-context attention (pk_model_set_attention_context) uses neither.  Reads two host integers: no device is needed.
 * (tests/test_gpu_call_history.py asserts with it that a call ran on a table built for a longer one.) */
pk_status pk_diag_pos_table_frames(const pk_model *m, int32_t out[2]);
/* ONE launch of a skinny product of the TDT / RNNT decode loop (kernels/decode_gemv.hip, kernels/decode_gemv_bf16.hip; kernels.hpp SkinnyArgs).
 * Every operand is given in its NATURAL layout as fp32 and packed here by the functions the loader packs with (csrc/dec_pack.hpp): fp32 mode = the
 * sigma K order of X / W / X2 / W2; bf16 mode = X / X2 rounded to bf16 (RNE), W / W2 in the kernel's per-lane tile order, rounded to bf16.
 *   epi 0 (bias):        out[b][n] = X[b] . W[n] (+ bias[n]);  out fp32 [out_rows][ldo], ldo >= N.
 *   epi 1 (activation):  p = X[b] . W[n] (+ bias[n]); pp_out[b][n] = p (pp_out may be NULL); z[b][n] = relu(ep[r0_b + min(t[b], Tb_b - 1)][n] + p) with
 *                        Tb_b = Tb ? Tb[b] : T and r0_b = row0 ? row0[b] : b * T;  ep [ep_rows][N].  z: [out_rows][N]; fp32 mode: sigma column order,
 *                        and with F > 1 (fp32 only; needs `need` and B <= 16) the rows b * F + f take the frames t[b] + f, f < F.
 *   epi 2 (LSTM cell):   N is the hidden size Hp; W [4 Hp][K]; gates = gi + X[b] . W[g Hp + j] with gi = gi_tab[gi_row ? gi_row[b] : b][g Hp + j] (row
 *                        stride gi_ld), or, when W2 is set, gi = X2[b] . W2[g Hp + j] + bias2[g Hp + j];  c' = sigmoid(f) c + sigmoid(i) tanh(g) -> cn [out_rows][Hp]
 *                        fp32; h' = sigmoid(o) tanh(c') -> out [out_rows][Hp] (fp32 mode: sigma column order).
 * bf16 mode stores z / h' as bf16: out then holds uint16 words.  need (may be NULL): [B] flags; only rows with a set flag are computed (B <= 16: the flags as
 * predicates; 16 < B <= 2048: the compacted row list; PK_ERR_INVALID above that).  out / cn / pp_out are BOTH input and output: the caller fills them with a
 * pattern, they are copied to the device, the kernel runs, they are copied back whole -- out_rows >= B * F, the rows past the batch and (epi 0) the columns
 * past N show stores that left the output.  Shapes: bf16 K % 32 == 0 and (cell) Hp % 4 == 0; fp32 K % 16 == 0 and (activation / cell) N % 16 == 0. */
typedef struct pk_skinny_diag {
    int32_t bf16, epi, B, N, K;
    const float *X, *W, *bias;
    const float *gi; int32_t gi_rows, gi_ld; const int32_t *gi_row; const float *c;
    const float *X2, *W2, *bias2;
    const float *ep; int64_t ep_rows; const int32_t *t; int32_t T; const int32_t *Tb, *row0; int32_t F;
    const int32_t *need;
    int32_t out_rows, ldo;
    void *out; float *cn, *pp_out;
} pk_skinny_diag;
pk_status pk_diag_skinny_gemm(const pk_skinny_diag *a);
/* Prediction-net caching of the per-phase decode loop (kernels.hpp TdtState::need) on / off; process-wide test switch, default on.  Off: every
 * phase launch covers every utterance at any batch size -- the same words, bit for bit (tests/test_gpu_bf16_decode_batch.py). */
pk_status pk_diag_pred_cache(int on);
/* n_steps >= 1 back-to-back launches of the greedy decision kernel of the TDT / RNNT decode loop (kernels/decode.hip launch_tdt_decide; kernels.hpp
 * TdtState) on state the CALLER sets -- no initialisation launch runs, so a call may start in the middle of an utterance.  Scalars as TdtState names them
 * (D = 0: the RNNT step).  Per step k: logits [n_steps][B F][V + D] and the candidate LSTM state hn / cn [n_steps][L][B][Hp] (h_bf16: h / hn hold bf16 words,
 * Hp even).  Every other array is BOTH input and output, as pk_diag_skinny_gemm's: copied up whole, copied back whole after the last launch.
 *   [rows] (rows >= B: the rows past the batch show stray stores): t, steps, n_out, nsym, done, token, lens, margin (may be NULL), need (may be NULL), n_act
 *   [rows][max_tokens]: ids, start, end, conf;  [1]: done_count;  h: h_words 32-bit words (>= L B Hp, h_bf16: L B Hp / 2), c: c_words (>= L B Hp)
 *   need set (prediction-net caching): pp [B][J], ep [ep_rows][J], z of z_words 32-bit words (>= B F J fp32 in the sigma column order; h_bf16: B J bf16 words,
 *   natural order), utterance b's enc_proj rows start at row0[b] (NULL: b T) and it has Tb[b] frames (NULL: T).  Tb set also makes the cap per utterance.
 *   trie_off set (phrase boosting): the trie in CSR form, trie_off [trie_nodes + 1], trie_tok / trie_node [trie_off[trie_nodes]], boost; act [rows][64], n_act.
 *   force_label set (forced scoring): force_label / force_dur [force_len], utterance b walks n_force_b[b] (NULL: n_force) steps from element b force_stride;
 *   score_lab [score_rows][V] / score_dur [score_rows][D] (either may be NULL) receive the rows b force_stride + step.
 * form (may be NULL): the launch taken, by the function the launcher switches on: PK_DIAG_TDT_KERNEL(form) exact / fast / boost / score, PK_DIAG_TDT_SLOTS(form)
 * the 256-element slots of LSTM state per thread (3 / 6 / 12), PK_DIAG_TDT_ROW(form) how the logits row is staged (5 or 33 register slots -- the fast kernel's NQ --,
 * batches of 8, the frame window).
 * PK_ERR_INVALID, and nothing is launched, for what the engine never launches: L Hp > 3072; F > 1 outside the plain exact step with V + D <= 1280, F <= 8 and
 * J <= 1024; more than 160 KB of LDS; D > 16, or D > 8 with a logits row whose duration maximum is not among the first 8 (TdtState holds 8 durations); state words,
 * frames, trie nodes or forced decisions out of range. */
#define PK_DIAG_TDT_KERNEL(form) ((form) >> 4)         /* 0 exact, 1 fast, 2 boost, 3 score */
#define PK_DIAG_TDT_SLOTS(form) (3 << (((form) >> 2) & 3))
#define PK_DIAG_TDT_ROW(form) ((form) & 3)             /* 0: 5 slots, 1: 33 slots, 2: batches of 8, 3: frame window */
typedef struct pk_tdt_decide_diag {
    int32_t B, T, V, D, L, Hp, blank, max_symbols, max_tokens, max_steps, keep_state, h_bf16, F, J;
    int32_t durations[8];
    int32_t n_steps, rows;
    const float *logits; const void *hn; const float *cn;
    int32_t *t, *steps, *n_out, *nsym, *done, *token, *lens, *done_count;
    void *h; float *c; int64_t h_words, c_words;
    int32_t *ids, *start, *end; float *conf;
    float *margin;
    int32_t *need; const float *pp, *ep; int64_t ep_rows; void *z; int64_t z_words;
    const int32_t *Tb, *row0;
    const int32_t *trie_off, *trie_tok, *trie_node; int32_t trie_nodes; float boost; int32_t *act, *n_act;
    const int32_t *force_label, *force_dur; int64_t force_len; int32_t n_force; const int32_t *n_force_b; int32_t force_stride;
    float *score_lab, *score_dur; int64_t score_rows;
} pk_tdt_decide_diag;
pk_status pk_diag_tdt_decide(const pk_tdt_decide_diag *a, int *form);
/* ONE step of the TDT beam search's own kernels (kernels/tdt_beam.hip; kernels.hpp TdtBeamDev) on rows the CALLER gives, without a model: launch_tdt_beam_init
 * when init != 0 (then step must be 0), one launch_tdt_beam_expand and one launch_tdt_beam_prune for `step`, then launch_tdt_beam_trace when trace != 0.  Nothing
 * else is launched.  logits [R][V + D] (R = B W) are the raw fp32 rows the heads product would have written: the kernels' own log-softmax runs on them.
 * Every array below is BOTH input and output, as pk_diag_tdt_decide's: copied up whole, copied back whole, so a caller carries a search from step to step.
 *   the beam, both copies: valid, t, len, par, born, tok, score, hash [2][R], prefix [2][R][max_tokens]; with lm set also lmstate, lmv (the prefix's LM score) [2][R].
 *       hash is opaque: carried, never made up -- a search begins with init = 1.
 *   live, steps_done [B]; live_total [cap + 1] (zeros before the first step); bp [cap][R][4] (step < cap).
 *   the step's intermediates, `rows` >= R rows each (the rows past R show stray stores): lab_id, lab_lp [rows][K + 1], dur_i, dur_lp [rows][Kd],
 *       cand [rows][(K + 1) Kd]; with lm set also lab_ls, lab_lm [rows][K + 1].
 *   the back-trace (trace != 0): ids, start, end, dur_idx, conf [B][N][max_tokens] (the search's host zero-fills them: the kernel writes filled slots only),
 *       lens, out_score [B][N], ok [B]; with lm set also out_lm [B][N].
 * lm (may be NULL) with alpha / beta selects the fused instantiations.
 * Refused before anything is allocated or launched.  PK_ERR_UNSUPPORTED: W, K outside 1..16, Kd or D outside 1..8, N outside 1..W (what the search's entry
 * points refuse).  PK_ERR_INVALID: Kd > D, K > V - 1, blank outside 0..V - 1, max_tokens < 1, T[b] < 1, step outside 0..cap - 1, rows < R, a missing array, what
 * lm_fusion refuses about the model, and -- init == 0 -- carried state the kernels would index with: len outside 0..max_tokens, t < 0, steps_done outside 0..cap
 * (a live clip: != step), an lmstate that is no state of the model, a back-pointer record of a step taken whose parent slot is outside 0..W - 1. */
typedef struct pk_tdt_beam_step_diag {
    int32_t B, W, K, Kd, N, V, D, blank, max_tokens;
    int32_t durations[8];
    int32_t step, init, trace, rows, cap;
    const int32_t *T;
    const float *logits;
    int32_t *valid, *t, *len, *par, *born, *tok; float *score; uint64_t *hash; int32_t *prefix;
    int32_t *live, *steps_done, *live_total, *bp;
    int32_t *lab_id; float *lab_lp; int32_t *dur_i; float *dur_lp, *cand;
    const pk_lm *lm; float alpha, beta;
    int32_t *lmstate; float *lmv; int32_t *lab_ls; float *lab_lm;
    int32_t *ids, *start, *end, *dur_idx; float *conf; int32_t *lens; float *out_score; int32_t *ok; float *out_lm;
} pk_tdt_beam_step_diag;
pk_status pk_diag_tdt_beam_step(const pk_tdt_beam_step_diag *a);
/* The CTC greedy kernels alone (kernels/decode.hip): the row log-softmax + first-max argmax over logits [frames][ld] (n <= ld values per row), once without and
 * once with the log-prob rows (best_idx2 / best_lp2, then lp / best_idx / best_lp), then the collapse -- or, trie_off set, the boosted walk over lp.  B utterances
 * of T frames, or n_frames[b] frames each, packed.  All outputs are in/out as above: lp [lp_rows][n], best_* [lp_rows] (lp_rows >= frames), ids / start / end /
 * conf [out_rows][pitch] (pitch >= the longest utterance), lens [out_rows] (out_rows >= B). */
typedef struct pk_ctc_greedy_diag {
    int32_t B, T, n, ld, blank, pitch, out_rows;
    const int32_t *n_frames;
    const float *logits;
    int64_t lp_rows;
    float *lp; int32_t *best_idx; float *best_lp; int32_t *best_idx2; float *best_lp2;
    int32_t *ids, *lens, *start, *end; float *conf;
    const int32_t *trie_off, *trie_tok, *trie_node; int32_t trie_nodes; float boost;
} pk_ctc_greedy_diag;
pk_status pk_diag_ctc_greedy(const pk_ctc_greedy_diag *a);
/* ONE product of the fp32 small-M GEMM family alone (kernels/gemm_smallm.hip; kernels.hpp GemmArgs), staged and launched as the engine launches it:
 * out = epi(X W^T + bias), M <= 1536, K % 64 == 0; epi 0 none / 1 relu / 2 silu / 3 out = resid + alpha * (..) / 4 glu (W [2N][K], bias [2N]).
 * Every operand is given in its NATURAL layout: A [M][lda] (lda >= K), W [N][K], bias, resid [M][N].
 *   w_sig:   a copy of W in the kernel's tiled load order is built on the device (launch_sigma_copy; N % 16 == 0) and handed over as GemmArgs::W_sig.
 *   a_sigma: the rows of A reach the product with their K axis in the sigma order (GemmArgs::a_sigma): written so by the LayerNorm in front (ln_g set,
 *            fused = 0: launch_layernorm mode 2, with pre_g launch_layernorm2), else permuted at upload.
 *   sigma_cols (a multiple of 16, <= N): the output columns below it are written in the sigma order.  remap_rows > 0: the output offset of (row, col) is
 *            (row / remap_rows) remap_gs + (row % remap_rows) remap_rs + col remap_cs instead of row ldo + col.
 *   ln_g / ln_b / eps: X = LayerNorm(A).  fused = 1: folded into the product (gemm_smallm_ln_kernel; needs w_sig, K = 512 / 1024; a_sigma is ignored);
 *            fused = 0: the separate LayerNorm launch, then the product on its rows.
 *   pre_g / pre_b (with ln_g; epi silu): X = LN(LN(A; pre); ln), pre_out [M][K] receives LN(A; pre).  fused = 0: launch_layernorm2, then the product.
 *   dw (with ln_g; epi glu; N = K = d; rows = [M / dw_c streams][dw_c frames]): the streaming conv module's depthwise conv (kernel 9) + BatchNorm + SiLU over
 *            [cache_in ; GLU rows] of every stream (kernels.hpp DwTail): out receives the activations (dw_out_sigma: columns in the sigma order), cache_out
 *            the streams' new caches.  cache_in [M / dw_c][8][d], cache_out [cache_streams >= M / dw_c][8][d], dw_w [9][d], the five vectors [d].
 *            fused = 0: LayerNorm, the GLU product, then launch_stream_dwconv.
 * out (out_words floats: every offset the product may write lies inside), cache_out and pre_out come back WHOLE and exactly as the launches left them --
 * permuted columns stay permuted --; their device buffers are filled with the pattern 0x7FC5A5A5 before the first launch.
 * form receives the form of the product launch, by the function the launcher switches on (kernels.hpp gemm_smallm_form): PK_DIAG_SMALLM_KERNEL 0 chain /
 * 1 two row tiles per wave / 2 LayerNorm folded in, PK_DIAG_SMALLM_EPI, PK_DIAG_SMALLM_RING the ring depth 8 / 2 / 1 (two row tiles: 4; folded: K / 64),
 * PK_DIAG_SMALLM_SIG / _DW / _PRE.  pk_diag_gemm_smallm_forms lists every form the launcher can take (host arithmetic; returns their number, writes at most cap).
 * PK_ERR_UNSUPPORTED, and nothing is launched, for what the engine refuses: a_sigma without w_sig (or N % 16 != 0), a folded norm / second norm / conv tail
 * outside gemm_smallm_ln_applies / gemm_smallm_pre_applies / gemm_smallm_dw_applies. */
#define PK_DIAG_SMALLM_KERNEL(form) ((form) >> 12)
#define PK_DIAG_SMALLM_EPI(form) (((form) >> 9) & 7)
#define PK_DIAG_SMALLM_RING(form) (((form) >> 3) & 63)
#define PK_DIAG_SMALLM_SIG(form) (((form) >> 2) & 1)
#define PK_DIAG_SMALLM_DW(form) (((form) >> 1) & 1)
#define PK_DIAG_SMALLM_PRE(form) ((form) & 1)
typedef struct pk_smallm_gemm_diag {
    int32_t M, N, K, epi, w_sig, a_sigma, sigma_cols, fused;
    const float *A; int64_t lda;
    const float *W, *bias, *resid; float alpha;
    int32_t remap_rows; int64_t remap_gs, remap_rs, remap_cs;
    const float *ln_g, *ln_b; float eps;
    const float *pre_g, *pre_b; float *pre_out;
    int32_t dw, dw_c, dw_has_cache, dw_out_sigma, cache_streams;
    const float *cache_in; float *cache_out;
    const float *dw_w, *dw_bias, *bn_mean, *bn_rstd, *bn_g, *bn_b;
    int64_t ldo, out_words; float *out;
    int32_t form;
} pk_smallm_gemm_diag;
pk_status pk_diag_gemm_smallm(pk_smallm_gemm_diag *a);
int pk_diag_gemm_smallm_forms(int32_t *out, int cap);
/* The layouts those products read, alone: the tiled weight copy dst [rows K] of src [rows][ld] (launch_sigma_copy; rows % 16 == 0, K % 64 == 0, ld >= K);
 * LayerNorm with the output columns in the sigma order (launch_layernorm mode 2); and y1 = LN(x; g1, b1), y2 = LN(y1; g2, b2) in one pass with y2_sigma != 0:
 * y2's columns in the sigma order (launch_layernorm2).  d <= 1024, a multiple of 16. */
pk_status pk_diag_sigma_copy(const float *src, int64_t rows, int K, int64_t ld, float *dst);
pk_status pk_diag_layernorm_sigma(const float *x, int64_t rows, int d, const float *gamma, const float *beta, float eps, float *y);
pk_status pk_diag_layernorm2(const float *x, int64_t rows, int d, const float *g1, const float *b1, const float *g2, const float *b2, float eps,
                             int y2_sigma, float *y1, float *y2);
/* ONE launch of the LayerNorm family alone (kernels/norm.hip), exactly one launcher per call:
 *   launcher PK_DIAG_LN_NORM        launch_layernorm:            y = LN(x; g1, b1)                            mode 0 fp32 / 1 bf16 (RNE) / 2 fp32, sigma columns
 *            PK_DIAG_LN_NORM2       launch_layernorm2:           y = LN(x; g1, b1) (fp32), y2 = LN(y; g2, b2)  mode: y2's, as above
 *            PK_DIAG_LN_STATS       launch_layernorm_stats:      stats[row] = {mean, rstd} of x's rows
 *            PK_DIAG_LN_THEN_STATS  launch_layernorm_then_stats: y = LN(x; g1, b1), stats of y's rows
 *   x [rows][d] fp32, 0 < d <= 1024 (mode 2: d % 16 == 0); g1 / b1 / g2 / b2 [d] where the launcher reads them.
 *   in_place: y aliases the device copy of x (launch_layernorm in mode 0; y1 of the other two), as the encoders call them.
 *   y / y2 / stats: caller-sized buffers of y_words / y2_words / stats_words 32-bit words, each LONGER than what the launch may write (rows * d elements --
 *            a bf16 buffer holds two to a word --; 2 * rows for stats).  Their device buffers are filled with 0x7FC5A5A5 before the launch and come back
 *            WHOLE, exactly as the launch left them.  Buffers the launcher does not write are ignored.
 * form receives the form of the launch, as the launcher itself reports it (kernels.hpp layernorm_form and its kin): PK_DIAG_LN_LAUNCHER, _PER_LANE (values
 * of the row per lane: 2 / 8 / 16), _RPW (rows per wavefront), _THEN, and PK_DIAG_LN_BATCH: launch_layernorm's branch for rows >= 4096.
 * pk_diag_layernorm_forms lists every form the launchers can take; pk_diag_layernorm_form_of answers for a shape -- both host arithmetic, no device.
 * PK_ERR_UNSUPPORTED: d > 1024 (a row lives in one wavefront's registers).  PK_ERR_INVALID: malformed arguments.  Both before a device is looked for. */
#define PK_DIAG_LN_NORM 0
#define PK_DIAG_LN_NORM2 1
#define PK_DIAG_LN_STATS 2
#define PK_DIAG_LN_THEN_STATS 3
#define PK_DIAG_LN_LAUNCHER(form) ((form) >> 12)
#define PK_DIAG_LN_BATCH(form) (((form) >> 11) & 1)
#define PK_DIAG_LN_THEN(form) (((form) >> 10) & 1)
#define PK_DIAG_LN_RPW(form) (((form) >> 5) & 31)
#define PK_DIAG_LN_PER_LANE(form) ((form) & 31)
typedef struct pk_layernorm_diag {
    int32_t launcher, d, mode, in_place;
    int64_t rows; float eps;
    const float *x, *g1, *b1, *g2, *b2;
    uint32_t *y; int64_t y_words;
    uint32_t *y2; int64_t y2_words;
    uint32_t *stats; int64_t stats_words;
    int32_t form;
} pk_layernorm_diag;
pk_status pk_diag_layernorm_form(pk_layernorm_diag *a);
int pk_diag_layernorm_forms(int32_t *out, int cap);
pk_status pk_diag_layernorm_form_of(int launcher, int64_t rows, int d, int32_t *form);
/* ONE product of the fp32 tile GEMM family alone (kernels/gemm.hip, gemm_pipe.hpp; kernels.hpp GemmArgs): out = epi(X W^T + bias) for a product
 * launch_gemm keeps on a tile kernel (M > 1536 or K % 64 != 0); epi as above (glu: W [2N][ldw], bias [2N]).
 *   A [M][lda] (lda >= K), W [N or 2N][ldw] (ldw >= K), resid [M][ldr] (ldr >= N): host arrays AT THOSE PITCHES; on the device every word of a row past
 *            K (resid: N) is replaced by the NaN pattern 0x7FC5A5A5 before the launch.
 *   sigma_cols / remap_*: as for pk_diag_gemm_smallm.  ldo >= N; out (out_words floats: every offset the product may write lies inside) comes back WHOLE,
 *            exactly as the launch left it; its device buffer is filled with 0x7FC5A5A5 first.
 *   ln_g / ln_b / eps: X = LayerNorm(A), run as the statistics pass (launch_layernorm_stats) + the fold into the A staging (GemmArgs::ln_stats).
 * form receives the form of the launch, by the function launch_gemm switches on (kernels.hpp gemm_tile_form): PK_DIAG_TILE_KERNEL 0 gemm_nt_kernel /
 * 1 gemm_pipe_kernel, PK_DIAG_TILE_WGM x _WGN waves of _TM x _TN 32 x 32 accumulators (the tile is 32 WGM TM x 32 WGN TN), PK_DIAG_TILE_NBUF, _LNA, _SCHED,
 * PK_DIAG_TILE_EPI.  pk_diag_gemm_tile_forms lists every form the launcher can take; pk_diag_gemm_tile_form answers for a shape (ln != 0: with the LayerNorm
 * fold) what pk_diag_gemm_tile would launch -- both host arithmetic, no device.
 * Refused before anything is launched, PK_ERR_UNSUPPORTED: a shape of the small-M family; what no tile kernel can do -- glu or resid with sigma_cols != 0,
 * K % 32 != 0, lda or ldw no multiple of 4 --; a LayerNorm outside gemm_ln_stats_applies.  PK_ERR_INVALID: malformed arguments. */
#define PK_DIAG_TILE_KERNEL(form) ((form) >> 20)
#define PK_DIAG_TILE_WGM(form) (((form) >> 17) & 7)
#define PK_DIAG_TILE_WGN(form) (((form) >> 14) & 7)
#define PK_DIAG_TILE_TM(form) (((form) >> 11) & 7)
#define PK_DIAG_TILE_TN(form) (((form) >> 8) & 7)
#define PK_DIAG_TILE_NBUF(form) (((form) >> 6) & 3)
#define PK_DIAG_TILE_LNA(form) (((form) >> 5) & 1)
#define PK_DIAG_TILE_SCHED(form) (((form) >> 3) & 3)
#define PK_DIAG_TILE_EPI(form) ((form) & 7)
typedef struct pk_gemm_tile_diag {
    int32_t M, N, K, epi, sigma_cols;
    const float *A; int64_t lda;
    const float *W; int64_t ldw;
    const float *bias;
    const float *resid; int64_t ldr; float alpha;
    int32_t remap_rows; int64_t remap_gs, remap_rs, remap_cs;
    const float *ln_g, *ln_b; float eps;
    int64_t ldo, out_words; float *out;
    int32_t form;
} pk_gemm_tile_diag;
pk_status pk_diag_gemm_tile(pk_gemm_tile_diag *a);
int pk_diag_gemm_tile_forms(int32_t *out, int cap);
pk_status pk_diag_gemm_tile_form(int M, int N, int K, int64_t lda, int64_t ldw, int epi, int ln, int32_t *form);
/* ONE product of the bf16 tile GEMM family alone (kernels/gemm.hip launch_gemm_bf16, gemm_bf16.hpp, gemm_bf16_glds.hpp; kernels.hpp GemmArgs):
 * out = epi(bf16(A) bf16(W)^T + bias), fp32 accumulation, for a product launch_gemm_bf16 keeps on a tile kernel (not gemm_smallm_bf16_applies).
 *   A [M][lda] fp32 (a_bf16 != 0: rounded to bf16 on the host, nearest even, and read as bf16; lda % 8 == 0, else % 4), W [N or 2N][ldw] (rounded to
 *            bf16; ldw % 8 == 0), resid [M][ldr] fp32: host arrays AT THOSE PITCHES; K % 64 == 0.  On the device every element of a row past K (resid: N)
 *            is a NaN (fp32 0x7FC5A5A5, bf16 0x7FC5).
 *   a_blocked: A (a_bf16) is staged in the blocked hand-off layout -- block (row / 32, k / 16) holds 32 x 16 bf16 row-major, blocks ordered
 *            [row / 32][lda / 16], rows rounded up to 32 (the rows past M are NaN); lda % 16 == 0.
 *   one_form: GemmArgs's -- the product takes the register-staged 64 x 64 tile at every M (M <= 128 with K % 256 == 0 included, which is then no shape of
 *            the small-M kernel); not with glu (PK_ERR_UNSUPPORTED).
 *   fast_act, out_bf16, out_blocked, sigma_cols, remap_*: GemmArgs's.  out_bf16: out holds bf16 rows [M][ldo] (out_blocked: blocks [ceil(M / 32)][ldo / 16],
 *            ldo % 16 == 0), two to a word.
 *   out (out_words 32-bit words: every offset the product may write lies inside) comes back WHOLE, exactly as the launch left it; its device buffer is
 *            filled with 0x7FC5A5A5 first.
 * form receives the form of the launch, by the function launch_gemm_bf16 switches on (kernels.hpp gemm_bf16_form): PK_DIAG_BF16_KERNEL 0 gemm_bf16_kernel
 * (register-staged) / 1 gemm_bf16_glds_kernel (direct-to-LDS), PK_DIAG_BF16_WGM x _WGN waves of _TM x _TN 32 x 32 accumulators, PK_DIAG_BF16_A16,
 * PK_DIAG_BF16_EFO 0 the LDS epilogue / 1 the register epilogue on one tile per workgroup / 2 the persistent walk with the register epilogue / 3 the
 * register residual epilogue, PK_DIAG_BF16_EPI.  pk_diag_gemm_bf16_tile_forms lists every form the launcher can take; pk_diag_gemm_bf16_tile_form
 * answers what pk_diag_gemm_bf16_tile would launch for a filled-in struct (pointers are looked at for null only) -- both host arithmetic, no device.
 * Refused before anything is launched, PK_ERR_UNSUPPORTED: a shape of the small-M bf16 kernel; what the launcher aborts on (out_blocked on a product the
 * register epilogue does not take, out_blocked / a_blocked on the register-staged kernel); out_bf16 with a remap, sigma_cols, glu, resid, or ldo / N no
 * multiple of 4 (Model::run_gemm's check); glu or resid with sigma_cols.  PK_ERR_INVALID: malformed arguments. */
#define PK_DIAG_BF16_KERNEL(form) ((form) >> 18)
#define PK_DIAG_BF16_WGM(form) (((form) >> 15) & 7)
#define PK_DIAG_BF16_WGN(form) (((form) >> 12) & 7)
#define PK_DIAG_BF16_TM(form) (((form) >> 9) & 7)
#define PK_DIAG_BF16_TN(form) (((form) >> 6) & 7)
#define PK_DIAG_BF16_A16(form) (((form) >> 5) & 1)
#define PK_DIAG_BF16_EFO(form) (((form) >> 3) & 3)
#define PK_DIAG_BF16_EPI(form) ((form) & 7)
typedef struct pk_gemm_bf16_tile_diag {
    int32_t M, N, K, epi, sigma_cols;
    int32_t a_bf16, a_blocked, out_bf16, out_blocked, fast_act;
    const float *A; int64_t lda;
    const float *W; int64_t ldw;
    const float *bias;
    const float *resid; int64_t ldr; float alpha;
    int32_t remap_rows; int64_t remap_gs, remap_rs, remap_cs;
    int64_t ldo, out_words; uint32_t *out;
    int32_t form;
    int32_t one_form;
} pk_gemm_bf16_tile_diag;
pk_status pk_diag_gemm_bf16_tile(pk_gemm_bf16_tile_diag *a);
int pk_diag_gemm_bf16_tile_forms(int32_t *out, int cap);
pk_status pk_diag_gemm_bf16_tile_form(pk_gemm_bf16_tile_diag *a);
/* ONE product of the small-M bf16 GEMM family alone (kernels/gemm_smallm_bf16.hip; kernels.hpp GemmArgs): out = epi(bf16(X) bf16(W)^T + bias), fp32
 * accumulation, for a product gemm_smallm_bf16_applies accepts (M <= 128, K % 256 == 0); epi as above (glu: W [2N][ldw], bias [2N]).
 *   A [M][lda] fp32 (a_bf16 != 0: rounded to bf16 on the host, nearest even, and read as bf16), W [N or 2N][ldw] (rounded to bf16), resid [M][ldr] fp32: host
 *            arrays AT THOSE PITCHES.  On the device every element of a row past K (resid: N) is a NaN (fp32 0x7FC5A5A5, bf16 0x7FC5).
 *   a_t8:    A (a_bf16, lda == K, M % 8 == 0, epi resid) is staged in 8-row operand tiles: element (row, k) at
 *            ((row / 8) (lda / 32) + k / 32) 256 + ((row % 8) + 8 (k / 8 % 4)) 8 + k % 8.
 *   w_tiles: a copy of the bf16 weights in the kernel's operand tiles is built on the device (launch_tile_copy_bf16, from W at its pitch) and handed over as
 *            GemmArgs::W_t16 when the weight rows are a multiple of 16; the launcher takes it for N % 16 == 0.
 *   one_form: GemmArgs's -- gemm_smallm_bf16_applies refuses every product that sets it (PK_ERR_UNSUPPORTED).
 *   out_bf16 / out_t8 / fast_act: GemmArgs's.  out_bf16: out holds bf16 rows [M][ldo], two to a word (out_t8: 8-row tiles as above, ldo == N, N % 32 == 0).
 *   resid_in_place: the residual is staged INSIDE out (resid == out, ldr == ldo, as fc2 of a block runs); the rest of out holds the fill.
 *   ln_g / ln_b / eps: X = LayerNorm(A) folded into the product (fp32 rows, K = 256 * (1 .. 8; glu: .. 4)).
 *   pre_g / pre_b (with ln_g; epi silu, N >= 256): X = LN(LN(A; pre); ln); pre_out [M][pre_ldo] (pre_out_words words) receives LN(A; pre).
 *   dw (epi glu; rows = [M / dw_c streams][dw_c frames], dw_c = 1 / 2 / 4; N % 16 == 0): the streaming conv module's depthwise conv (kernel 9) + BatchNorm + SiLU
 *            over [cache_in ; GLU rows] of every stream in the epilogue (kernels.hpp DwTail): out receives the activations, cache_out the streams' new caches.
 *            cache_in [M / dw_c][8][N], cache_out [cache_streams >= M / dw_c][8][N], dw_w [9][N], the five vectors [N].
 * out (out_words 32-bit words), pre_out and cache_out come back WHOLE, exactly as the launch left them; their device buffers are filled with 0x7FC5A5A5
 * first.  Every offset the product may write is checked to lie inside them.
 * form receives the form of the launch, by the function launch_gemm_smallm_bf16 switches on (kernels.hpp gemm_smallm_bf16_form): PK_DIAG_SMALLM_BF16_EPI,
 * _STEPS (MFMA steps of 32 k per K slice: 8 / 16), _RT (row tiles per wave: 1 / 2), _RVALID (the rows of a tile that exist: 8 / 16), _A16, _LN, _CT (column
 * tiles per wave: 1 / 2), _WT (operand-tiled weights), _DW, _AT (a_t8), _AL (rows by LDS-DMA), _PRE.  pk_diag_gemm_smallm_bf16_forms lists every form the
 * launcher can take; pk_diag_gemm_smallm_bf16_form answers what pk_diag_gemm_smallm_bf16 would launch for a filled-in struct (pointers are looked at for
 * null only) -- both host arithmetic, no device.
 * Refused before anything is launched or a device is looked for, PK_ERR_UNSUPPORTED: what gemm_smallm_bf16_applies / _ln_applies / _pre_applies / _dw_applies
 * refuse (the message names the predicate).  PK_ERR_INVALID: malformed arguments, a buffer too small.
 * pk_diag_tile_copy_bf16: launch_tile_copy_bf16 alone -- src [rows][ld] (rounded to bf16; NaN past K) -> dst rows x K bf16 in the operand tiles. */
#define PK_DIAG_SMALLM_BF16_EPI(form) ((form) & 7)
#define PK_DIAG_SMALLM_BF16_STEPS(form) ((((form) >> 3) & 1) ? 16 : 8)
#define PK_DIAG_SMALLM_BF16_RT(form) ((((form) >> 4) & 1) + 1)
#define PK_DIAG_SMALLM_BF16_RVALID(form) ((((form) >> 5) & 1) ? 16 : 8)
#define PK_DIAG_SMALLM_BF16_A16(form) (((form) >> 6) & 1)
#define PK_DIAG_SMALLM_BF16_LN(form) (((form) >> 7) & 1)
#define PK_DIAG_SMALLM_BF16_CT(form) ((((form) >> 8) & 1) + 1)
#define PK_DIAG_SMALLM_BF16_WT(form) (((form) >> 9) & 1)
#define PK_DIAG_SMALLM_BF16_DW(form) (((form) >> 10) & 1)
#define PK_DIAG_SMALLM_BF16_AT(form) (((form) >> 11) & 1)
#define PK_DIAG_SMALLM_BF16_AL(form) (((form) >> 12) & 1)
#define PK_DIAG_SMALLM_BF16_PRE(form) (((form) >> 13) & 1)
typedef struct pk_gemm_smallm_bf16_diag {
    int32_t M, N, K, epi;
    int32_t a_bf16, out_bf16, out_t8, a_t8, fast_act, w_tiles, resid_in_place;
    const float *A; int64_t lda;
    const float *W; int64_t ldw;
    const float *bias;
    const float *resid; int64_t ldr; float alpha;
    const float *ln_g, *ln_b; float eps;
    const float *pre_g, *pre_b; uint32_t *pre_out; int64_t pre_ldo, pre_out_words;
    int32_t dw, dw_c, dw_has_cache, cache_streams;
    const float *cache_in; uint32_t *cache_out;
    const float *dw_w, *dw_bias, *bn_mean, *bn_rstd, *bn_g, *bn_b;
    int64_t ldo, out_words; uint32_t *out;
    int32_t form;
    int32_t one_form;
} pk_gemm_smallm_bf16_diag;
pk_status pk_diag_gemm_smallm_bf16(pk_gemm_smallm_bf16_diag *a);
int pk_diag_gemm_smallm_bf16_forms(int32_t *out, int cap);
pk_status pk_diag_gemm_smallm_bf16_form(pk_gemm_smallm_bf16_diag *a);
pk_status pk_diag_tile_copy_bf16(const float *src, int64_t rows, int K, int64_t ld, uint16_t *dst);

/* ---- neural LM rescoring: n-best reranking with a Transformer LM after beam search (the reference's roadmap, README.md "Neural LM rescoring") ------
 * A causal Transformer LM over the acoustic model's own token ids plus BOS and EOS: token and position embeddings, the blocks of
 * pk_transformer_* under a causal mask (ReLU feed-forwards, pre- or post-norm), an output projection.  fp32 throughout.  DESIGN.md section 5.5.11.
 * Tensors under <prefix>: tok_emb_.weight [Vlm][d], pos_emb_.weight [max_positions][d] (a sinusoidal table is stored as a tensor by whoever
 * converts the model), emb_norm_.{weight,bias} [d] (optional), the layers_.<i>.* / final_norm_.* tree of pk_transformer_load,
 * lm_head_.weight [Vlm][d] and lm_head_.bias [Vlm] (untied head; the bias is optional).
 *
 * The scoring rule for a token string ids[0..n):
 *   inputs     x_0 = bos_id, x_i = ids[i-1].  With an end term (eos_id >= 0) there are P = n + 1 positions, otherwise P = n.
 *   embedding  h_i = tok_emb[x_i] + pos_emb[i] (one fp32 add), then emb_norm_ if present.
 *   blocks     TransformerEncoder's, with attention softmax(scale q_i . k_j over j <= i) V, scale = 1 / sqrt(real head dim); then final_norm_ if present.
 *   head       logit_i[c] = h_i . W[c] (+ b[c]), a k-ordered fp32 fma chain from zero; lp_i = logit_i[target_i] - logsumexp_c logit_i[c], target_i = ids[i]
 *              for i < n and eos_id for i = n.
 *   total      the left-to-right fp32 sum of lp_i.  The empty string scores 0 without an end term and lp(eos | bos) with one.
 *   too long   a string with P > max_positions is not scored: ok = 0, total = -inf.
 *   bad ids    an id < 0, >= Vlm, or equal to bos_id: PK_ERR_INVALID for the call.
 * No padded position is computed: the strings of a call are packed like the clips of a ragged encoder batch, and a string's bits do not depend
 * on what it is packed with.  A call whose scratch would pass 1 GiB is cut into groups of whole strings on the host. */
typedef struct pk_nlm_config {
    int32_t vocab_size;        /* Vlm: rows of the embedding and of the head */
    int32_t max_positions;     /* rows of the position table; <= 512 */
    pk_transformer_config transformer;   /* hidden, layers, heads, ffn, pre_ln, has_final_norm, eps */
    int32_t has_emb_norm;      /* LayerNorm after token + position embedding */
    int32_t tied_head;         /* 1: the head is tok_emb_.weight; 0: lm_head_.weight (+ optional lm_head_.bias) */
    int32_t bos_id;            /* fed at position 0 */
    int32_t eos_id;            /* < 0: no end-of-string term */
} pk_nlm_config;
typedef struct pk_nlm pk_nlm;
/* Fills what the tensor shapes determine: vocab_size, hidden_size, num_layers, ffn_intermediate, max_positions, has_emb_norm, has_final_norm,
 * tied_head.  The caller's num_heads, pre_ln, bos_id, eos_id and layer_norm_eps stay as given.  Host only. */
pk_status pk_nlm_config_infer(const char *safetensors_path, const char *prefix, pk_nlm_config *io);
/* Refused before anything is allocated: what pk_transformer_load refuses about the configuration, max_positions > 512 (PK_ERR_UNSUPPORTED), bos_id
 * outside [0, Vlm) or eos_id >= Vlm or eos_id == bos_id (PK_ERR_INVALID), a missing or mis-shaped tensor (PK_ERR_WEIGHTS). */
pk_status pk_nlm_load(const char *safetensors_path, const char *prefix, const pk_nlm_config *cfg, int device, pk_nlm **out);
void pk_nlm_free(pk_nlm *nlm);
/* ids packed, id_offsets[n_strings + 1].  total / ok [n_strings].  token_logp (optional): string b's lp_i at token_logp[id_offsets[b] + b + i],
 * i.e. packed by id_offsets plus one slot per string for the end term (0 where the model has none); the slots of a string that is not scored read 0. */
pk_status pk_nlm_score(pk_nlm *nlm, const int32_t *ids, const int32_t *id_offsets, int n_strings, float *total, int32_t *ok, float *token_logp);
/* Stage timers (tools/bench_nlm_rescore.py): pk_nlm_score run reps + 1 times, hipEvents on the handle's stream around the stages of every group,
 * summed over the groups, medians of the last reps passes: ms[0] = embedding (+ emb_norm_), ms[1] = blocks (+ final_norm_), ms[2] = head. */
pk_status pk_nlm_score_timed(pk_nlm *nlm, const int32_t *ids, const int32_t *id_offsets, int n_strings, int reps, float ms[3]);
/* Re-ranking of the lists of pk_transcribe_pcm_nbest, _nbest_lm, _nbest_tdt or _nbest_tdt_lm, in place: every hypothesis is scored by pk_nlm_score,
 * combined = am + ((alpha * nlm) + (beta * len)) in four separately rounded fp32 operations (am = the list's score[j], len = n_tokens), and each
 * clip's list is re-ordered stably, descending, ties keeping the incoming order; a hypothesis that is not scored (ok = 0), or whose combined is
 * NaN, goes after every scored one with combined = -inf.  score[j] becomes combined; hyp[j] (text, ids, words, timestamps) moves with its slot,
 * unchanged.  alpha == 0 and beta == 0 leaves every list bit for bit as it was.  am_score / nlm_score (optional): [n_clips][N], N = the n_best
 * of the search that made the lists, in the returned order, -inf in the slots past n_hyp.  opt == NULL: alpha 0.5, beta 0 (a choice, not a
 * measurement).  An id the LM refuses fails the call before any list is touched. */
typedef struct pk_nlm_rescore_options { float alpha, beta; } pk_nlm_rescore_options;
pk_status pk_nbest_rescore_nlm(pk_nbest *results, int n_clips, pk_nlm *nlm, const pk_nlm_rescore_options *opt, float *am_score, float *nlm_score);
/* Diagnostics.  pk_diag_nlm_order: the ordering rule above on the N slots of one list, host arithmetic only (order[j] = the slot at position j,
 * combined[] by slot).  pk_diag_nlm_set_scratch_cap: the scratch cap of pk_nlm_score's grouping in bytes (0: back to 1 GiB); a group always holds
 * at least one string.  pk_diag_nlm_groups (may be called after a pk_nlm_score): the number of groups the last call ran. */
pk_status pk_diag_nlm_order(const float *am, const float *nlm, const int32_t *lens, const int32_t *ok, int N, float alpha, float beta,
                            int32_t *order, float *combined);
pk_status pk_diag_nlm_set_scratch_cap(pk_nlm *nlm, uint64_t bytes);
int pk_diag_nlm_groups(const pk_nlm *nlm);
/* The causal attention kernel alone (kernels/attention.hip, CAUSAL instantiation) on B packed sequences of lens[b] <= 512 positions:
 * ctx_i = softmax_j<=i(scale q_i . k_j) V, no position term.  qkv [rows][3 d] natural columns (q | k | v), hd = d / n_heads in {32, 64, 96, 128}
 * (a narrower head is zero-padded by the caller, as TransformerEncoder does; scale is the caller's).  ctx receives
 * [rows + PK_DIAG_ATTENTION_GUARD_ROWS][d] floats; the device buffer is filled with 0x7FC5A5A5 before the launch. */
pk_status pk_diag_causal_attention(int B, const int32_t *lens, int d, int n_heads, float scale, const float *qkv, float *ctx);
/* The head kernel alone: lp[r] = logit_r[targets[r]] - logsumexp_c logit_r[c], logit_r[c] = h_r . W_c (+ bias[c]).  h [rows][d], W [V][d], bias [V]
 * or NULL, targets [rows] in [0, V); d a multiple of 32, V >= 1.  lp receives rows + PK_DIAG_ATTENTION_GUARD_ROWS floats, 0x7FC5A5A5-filled before the launch. */
pk_status pk_diag_nlm_head_logp(const float *h, const float *W, const float *bias, const int32_t *targets, int64_t rows, int V, int d, float *lp);

#ifdef __cplusplus
}
#endif
#endif /* PARAKEET_AMD_H */
