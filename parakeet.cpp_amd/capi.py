"""ctypes binding of include/parakeet_amd.h (libparakeet_amd.so).  Plumbing for tests and bench.py.
Fails loudly if the HIP library is missing -- there is no Python / CPU fallback."""
import ctypes as C
import os

import numpy as np

from .config import ModelConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PK_LIB") or os.path.join(_HERE, "libparakeet_amd.so")   # PK_LIB: experiment builds of the same library
_LIB = None

f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class PkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pk_status {code}: {msg}")
        self.code = code


class PkConfig(C.Structure):
    _fields_ = [("mel_bins", C.c_int32), ("subsampling_channels", C.c_int32), ("hidden_size", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("ffn_intermediate", C.c_int32),
                ("conv_kernel_size", C.c_int32), ("vocab_size", C.c_int32), ("pred_hidden", C.c_int32),
                ("num_lstm_layers", C.c_int32), ("joint_hidden", C.c_int32), ("num_durations", C.c_int32),
                ("durations", C.c_int32 * 8), ("ctc_vocab_size", C.c_int32), ("blank_id", C.c_int32),
                ("max_symbols_per_step", C.c_int32), ("joint_pred_bias", C.c_int32), ("rnnt_head", C.c_int32), ("stft_window_centered", C.c_int32), ("gemm_bf16", C.c_int32),
                ("joint_prefix", C.c_char * 32), ("xscaling", C.c_int32), ("mel_normalize_off", C.c_int32),
                ("encoder_prefix", C.c_char * 32)]


class PkTransformerConfig(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("ffn_intermediate", C.c_int32),
                ("pre_ln", C.c_int32), ("has_final_norm", C.c_int32), ("layer_norm_eps", C.c_float)]


class PkSortformerConfig(C.Structure):
    _fields_ = [("nest", PkConfig), ("transformer", PkTransformerConfig), ("max_speakers", C.c_int32), ("activity_threshold", C.c_float),
                ("att_context_left", C.c_int32), ("att_context_right", C.c_int32)]


class PkKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int32), ("total_ms", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


class PkOptions(C.Structure):
    _fields_ = [("decoder", C.c_int32), ("timestamps", C.c_int32), ("boost_phrases", C.POINTER(C.c_char_p)),
                ("n_boost_phrases", C.c_int32), ("boost_score", C.c_float)]


class PkWord(C.Structure):
    _fields_ = [("word", C.c_char_p), ("start", C.c_float), ("end", C.c_float), ("confidence", C.c_float)]


class PkResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("n_tokens", C.c_int32), ("token_ids", i32p), ("start_frame", i32p),
                ("end_frame", i32p), ("confidence", f32p), ("n_words", C.c_int32), ("words", C.POINTER(PkWord))]


class PkBeamOptions(C.Structure):
    _fields_ = [("beam_width", C.c_int32), ("token_prune", C.c_int32), ("n_best", C.c_int32), ("timestamps", C.c_int32)]


class PkTdtBeamOptions(C.Structure):
    _fields_ = [("beam_width", C.c_int32), ("label_prune", C.c_int32), ("duration_prune", C.c_int32), ("n_best", C.c_int32)]


class PkRescoreOptions(C.Structure):
    _fields_ = [("tdt_weight", C.c_float)]


class PkKwsOptions(C.Structure):
    _fields_ = [("max_hits", C.c_int32), ("min_score", C.c_float)]


class PkStreamKwsOptions(C.Structure):
    _fields_ = [("min_score", C.c_float), ("patience", C.c_int32)]


class PkKwsEvent(C.Structure):
    _fields_ = [("stream", C.c_int32), ("keyword", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("score", C.c_float)]


class PkEndpointOptions(C.Structure):
    _fields_ = [("threshold_db", C.c_float), ("margin_db", C.c_float), ("floor_window_ms", C.c_int32), ("min_speech_ms", C.c_int32),
                ("min_silence_ms", C.c_int32), ("max_utterance_s", C.c_float), ("eou_token_id", C.c_int32), ("reset_decoder", C.c_int32)]


class PkEndpointEvent(C.Structure):
    _fields_ = [("stream", C.c_int32), ("kind", C.c_int32), ("reason", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("at", C.c_int32)]


class PkVadOptions(C.Structure):
    _fields_ = [("threshold_db", C.c_float), ("margin_db", C.c_float), ("floor_percent", C.c_int32), ("min_speech_ms", C.c_int32),
                ("min_silence_ms", C.c_int32), ("pad_ms", C.c_int32), ("max_gap_ms", C.c_int32), ("max_piece_s", C.c_float)]


class PkVadPiece(C.Structure):
    _fields_ = [("clip", C.c_int32), ("begin", C.c_int64), ("end", C.c_int64)]


class PkNbest(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("hyp", C.POINTER(PkResult)), ("score", f32p)]


class PkLmOptions(C.Structure):
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float)]


class PkNlmConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("max_positions", C.c_int32), ("transformer", PkTransformerConfig), ("has_emb_norm", C.c_int32),
                ("tied_head", C.c_int32), ("bos_id", C.c_int32), ("eos_id", C.c_int32)]


class PkNlmRescoreOptions(C.Structure):
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float)]


def to_pk_config(cfg: ModelConfig) -> PkConfig:
    c = PkConfig()
    c.mel_bins, c.subsampling_channels, c.hidden_size = cfg.mel_bins, cfg.subsampling_channels, cfg.hidden_size
    c.num_layers, c.num_heads, c.ffn_intermediate = cfg.num_layers, cfg.num_heads, cfg.ffn_intermediate
    c.conv_kernel_size, c.vocab_size, c.pred_hidden = cfg.conv_kernel_size, cfg.vocab_size, cfg.pred_hidden
    c.num_lstm_layers, c.joint_hidden, c.num_durations = cfg.num_lstm_layers, cfg.joint_hidden, len(cfg.durations)
    for i, d in enumerate(cfg.durations):
        c.durations[i] = d
    c.ctc_vocab_size, c.blank_id, c.max_symbols_per_step = cfg.ctc_vocab_size, cfg.blank_id, cfg.max_symbols_per_step
    c.joint_pred_bias, c.rnnt_head = 0, int(cfg.head == "rnnt")
    c.stft_window_centered = int(getattr(cfg, "stft_window_centered", False))
    c.gemm_bf16 = int(getattr(cfg, "gemm_bf16", False))
    c.joint_prefix = cfg.joint_prefix.encode()
    c.xscaling = int(getattr(cfg, "xscaling", False))
    c.mel_normalize_off = int(not getattr(cfg, "mel_normalize", True))
    ep = getattr(cfg, "encoder_prefix", "encoder_.")
    c.encoder_prefix = b"" if ep == "encoder_." else ep.encode()
    return c


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.pk_version.restype = C.c_char_p
    L.pk_last_error.restype = C.c_size_t
    L.pk_last_error.argtypes = [C.c_char_p, C.c_size_t]
    L.pk_config_preset.argtypes = [C.c_char_p, C.POINTER(PkConfig)]
    L.pk_model_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PkConfig), C.POINTER(C.c_void_p)]
    L.pk_model_to_gpu.argtypes = [C.c_void_p, C.c_int]
    L.pk_model_free.argtypes = [C.c_void_p]
    L.pk_model_config.argtypes = [C.c_void_p, C.POINTER(PkConfig)]
    L.pk_mel.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64, f32p, f32p]
    L.pk_mel_num_frames.argtypes = [C.c_int64]
    L.pk_encoder_num_frames.argtypes = [C.c_int]
    L.pk_diag_math.argtypes = [C.c_int, f32p, f32p, C.c_int64]
    L.pk_diag_math_exhaustive.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pk_diag_gemm.argtypes = [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_int, f32p, C.c_float, f32p]
    L.pk_diag_gemm_bf16.argtypes = L.pk_diag_gemm.argtypes
    L.pk_diag_gemm_bf16_a16.argtypes = L.pk_diag_gemm.argtypes
    L.pk_diag_layernorm.argtypes = [f32p, C.c_int64, C.c_int, f32p, f32p, C.c_float, f32p]
    L.pk_diag_ln_gemm.argtypes = [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_float, f32p, f32p, C.c_int, C.c_int, f32p, f32p]
    L.pk_diag_sum64.argtypes = [f32p, C.c_int, C.c_int, f32p]
    L.pk_diag_relpos_attention.argtypes = [C.c_int, C.c_int, i32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, f32p,
                                           C.POINTER(C.c_int)]
    for name, at in _LATE_SIGNATURES.items():
        if hasattr(L, name):
            getattr(L, name).argtypes = at
    _LIB = L
    return L


_LATE_SIGNATURES = {
    "pk_encode": [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p],
    "pk_conformer_blocks": [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int, C.c_int, f32p],
    "pk_subsample": [C.c_void_p, f32p, C.c_int, C.c_int, f32p],
    "pk_ctc_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p],
    "pk_tdt_decode": [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, i32p],
    "pk_model_set_decode_loop": [C.c_void_p, C.c_int],
    "pk_plan_batches": [i64p, C.c_int, i32p, i32p, C.POINTER(C.c_int)],
    "pk_ragged_extents": [i64p, C.c_int, i32p, i32p, i64p],
    "pk_tdt_score": [C.c_void_p, f32p, C.c_int, i32p, i32p, C.c_int, f32p, f32p, C.POINTER(C.c_int)],
    "pk_mel_ragged": [C.c_void_p, f32p, i64p, C.c_int, f32p, f32p],
    "pk_encode_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.c_int, f32p],
    "pk_conformer_blocks_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.c_int, f32p],
    "pk_ctc_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p],
    "pk_tdt_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, i32p],
    "pk_batch_create_ragged": [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)],
    "pk_batch_upload_ragged": [C.c_void_p, f32p, i64p, C.c_int],
    "pk_batch_upload_ragged_async": [C.c_void_p, f32p, i64p, C.c_int],
    "pk_batch_create": [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_void_p)],
    "pk_batch_free": [C.c_void_p],
    "pk_batch_upload": [C.c_void_p, f32p, C.c_int],
    "pk_batch_run": [C.c_void_p, C.c_int],
    "pk_batch_upload_async": [C.c_void_p, f32p, C.c_int],
    "pk_batch_results_done": [C.c_void_p, C.POINTER(C.c_int), i32p, i32p, i32p, i32p, f32p],
    "pk_batch_results_back": [C.c_void_p, C.c_int, C.POINTER(C.c_int), i32p, i32p, i32p, i32p, f32p],
    "pk_batch_results_available": [C.c_void_p],
    "pk_batch_set_decode_group": [C.c_void_p, C.c_int],
    "pk_batch_sync": [C.c_void_p],
    "pk_batch_set_decode_overlap": [C.c_void_p, C.c_int],
    "pk_batch_margins": [C.c_void_p, C.c_int, f32p],
    "pk_decode_margins": [C.c_void_p, f32p, C.c_int],
    "pk_batch_max_tokens": [C.c_void_p],
    "pk_batch_results": [C.c_void_p, i32p, i32p, i32p, i32p, f32p],
    "pk_batch_run_timed": [C.c_void_p, C.c_int, f32p],
    "pk_batch_profile": [C.c_void_p, C.c_int, C.POINTER(PkKernelStat), C.c_int],
    "pk_transcribe_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkOptions), C.POINTER(C.POINTER(PkResult))],
    "pk_results_free": [C.POINTER(PkResult), C.c_int],
    "pk_read_wav": [C.c_char_p, C.POINTER(f32p), i64p, C.POINTER(C.c_int)],
    "pk_free": [C.c_void_p],
    "pk_vocab_size": [C.c_void_p],
    "pk_detokenize": [C.c_void_p, i32p, C.c_int, C.c_char_p, C.c_int],
    "pk_tokenize": [C.c_void_p, C.c_char_p, i32p, C.c_int],
    "pk_set_boost_tokens": [C.c_void_p, i32p, i32p, C.c_int, C.c_float],
    "pk_set_boost_phrases": [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_float],
    "pk_boost_trie_size": [C.c_void_p],
    "pk_group_timestamps": [C.c_void_p, i32p, i32p, i32p, f32p, C.c_int, C.c_int, C.c_char_p, C.c_int, f32p, f32p, f32p, C.c_int],
    "pk_group_create": [C.c_char_p, C.c_char_p, C.POINTER(PkConfig), i32p, C.c_int, C.POINTER(C.c_void_p)],
    "pk_group_free": [C.c_void_p],
    "pk_group_size": [C.c_void_p],
    "pk_group_transcribe_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkOptions), C.POINTER(C.POINTER(PkResult))],
    "pk_group_last_stats": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), i32p],
    "pk_group_verify_exchange": [C.c_void_p, C.POINTER(PkResult), C.c_int, C.POINTER(C.c_int)],
    "pk_beam_options_default": [C.POINTER(PkBeamOptions)],
    "pk_tdt_beam_options_default": [C.POINTER(PkTdtBeamOptions)],
    "pk_ctc_beam_search": [f32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p],
    "pk_ctc_beam_decode": [C.c_void_p, f32p, C.c_int, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p],
    "pk_ctc_beam_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p],
    "pk_ctc_beam_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.POINTER(PkBeamOptions), C.c_int, f32p],
    "pk_transcribe_pcm_nbest": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkBeamOptions), C.POINTER(C.POINTER(PkNbest))],
    "pk_nbest_free": [C.POINTER(PkNbest), C.c_int],
    "pk_nlm_config_infer": [C.c_char_p, C.c_char_p, C.POINTER(PkNlmConfig)],
    "pk_nlm_load": [C.c_char_p, C.c_char_p, C.POINTER(PkNlmConfig), C.c_int, C.POINTER(C.c_void_p)],
    "pk_nlm_free": [C.c_void_p],
    "pk_nlm_score": [C.c_void_p, i32p, i32p, C.c_int, f32p, i32p, f32p],
    "pk_nlm_score_timed": [C.c_void_p, i32p, i32p, C.c_int, C.c_int, f32p],
    "pk_nbest_rescore_nlm": [C.POINTER(PkNbest), C.c_int, C.c_void_p, C.POINTER(PkNlmRescoreOptions), f32p, f32p],
    "pk_diag_nlm_order": [f32p, f32p, i32p, i32p, C.c_int, C.c_float, C.c_float, i32p, f32p],
    "pk_diag_nlm_set_scratch_cap": [C.c_void_p, C.c_uint64],
    "pk_diag_nlm_groups": [C.c_void_p],
    "pk_diag_causal_attention": [C.c_int, i32p, C.c_int, C.c_int, C.c_float, f32p, f32p],
    "pk_diag_nlm_head_logp": [f32p, f32p, f32p, i32p, C.c_int64, C.c_int, C.c_int, f32p],
    "pk_lm_load": [C.c_char_p, C.POINTER(C.c_void_p)],
    "pk_lm_load_buffer": [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)],
    "pk_lm_free": [C.c_void_p],
    "pk_lm_order": [C.c_void_p],
    "pk_lm_num_ngrams": [C.c_void_p],
    "pk_lm_score": [C.c_void_p, i32p, i32p, C.c_int, C.c_int, C.c_int, f32p],
    "pk_lm_options_default": [C.POINTER(PkLmOptions)],
    "pk_ctc_beam_search_lm": [f32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p,
                              C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_ctc_beam_decode_lm": [C.c_void_p, f32p, C.c_int, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p,
                              C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_ctc_beam_decode_lm_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.POINTER(PkBeamOptions), i32p, i32p, f32p, i32p, i32p, f32p,
                                     C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_ctc_beam_decode_lm_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.POINTER(PkBeamOptions), C.c_int, f32p, C.c_void_p, C.POINTER(PkLmOptions)],
    "pk_transcribe_pcm_nbest_lm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkBeamOptions), C.POINTER(C.POINTER(PkNbest)),
                                   C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_tdt_beam_decode": [C.c_void_p, f32p, C.c_int, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, i32p, i32p, f32p, i32p, i32p, i32p, f32p, i32p],
    "pk_tdt_beam_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, i32p, i32p, f32p, i32p, i32p, i32p, f32p, i32p],
    "pk_tdt_beam_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, C.c_int, f32p],
    "pk_transcribe_pcm_nbest_tdt": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, C.POINTER(C.POINTER(PkNbest))],
    "pk_tdt_beam_decode_lm": [C.c_void_p, f32p, C.c_int, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, i32p, i32p, f32p, i32p, i32p, i32p, f32p, i32p,
                              C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_tdt_beam_decode_lm_ragged": [C.c_void_p, f32p, i32p, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, i32p, i32p, f32p, i32p, i32p, i32p, f32p, i32p,
                                     C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_tdt_beam_decode_lm_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, C.c_int, f32p, C.c_void_p,
                                    C.POINTER(PkLmOptions)],
    "pk_tdt_beam_last_steps": [C.c_void_p],
    "pk_transcribe_pcm_nbest_tdt_lm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkTdtBeamOptions), C.c_int, C.POINTER(C.POINTER(PkNbest)),
                                       C.c_void_p, C.POINTER(PkLmOptions), f32p],
    "pk_ctc_align": [f32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p, f32p, i32p],
    "pk_ctc_align_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p, f32p, i32p],
    "pk_ctc_align_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p, f32p, i32p],
    "pk_ctc_align_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.c_int, f32p],
    "pk_align_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(C.c_char_p), i32p, i32p, C.POINTER(C.POINTER(PkResult)), f32p, f32p, i32p],
    "pk_tdt_align": [f32p, f32p, f32p, i32p, C.c_int, i32p, C.c_int, i32p, i32p, i32p, i32p, f32p, f32p, i32p],
    "pk_tdt_align_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, i32p, f32p, f32p, i32p],
    "pk_tdt_align_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, i32p, i32p, i32p, f32p, f32p, i32p],
    "pk_tdt_align_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, f32p],
    "pk_diag_mem_info": [C.c_void_p, C.POINTER(C.c_uint64)],
    "pk_tdt_total": [f32p, f32p, f32p, i32p, C.c_int, i32p, C.c_int, i32p, f32p, i32p],
    "pk_tdt_total_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, C.c_int, f32p, i32p],
    "pk_tdt_total_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, i32p, C.c_int, f32p, i32p],
    "pk_tdt_total_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, i32p, C.c_int, C.c_int, f32p],
    "pk_tdt_score_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(C.c_char_p), i32p, i32p, i32p, C.c_int, f32p, i32p],
    "pk_transcribe_pcm_nbest_rescored": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkBeamOptions), C.POINTER(PkRescoreOptions),
                                         C.POINTER(C.POINTER(PkNbest)), f32p, f32p],
    "pk_diag_tdt_total_groups": [i32p, i32p, C.c_int, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.POINTER(C.c_int)],
    "pk_diag_rescore_order": [i32p, f32p, f32p, i32p, C.c_int, C.c_float, i32p, f32p],
    "pk_tdt_align_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(C.c_char_p), i32p, i32p, C.POINTER(C.POINTER(PkResult)), f32p, i32p],
    "pk_diag_tdt_lattice": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, C.c_int, f32p, f32p, f32p],
    "pk_kws_options_default": [C.POINTER(PkKwsOptions)],
    "pk_ctc_kws": [f32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_ctc_kws_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_ctc_kws_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_ctc_kws_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), C.c_int, f32p],
    "pk_spot_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(C.c_char_p), i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, f32p, f32p, f32p],
    "pk_tdt_kws": [f32p, f32p, f32p, f32p, i32p, C.c_int, i32p, C.c_int, i32p, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_tdt_kws_decode": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_tdt_kws_decode_ragged": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, i32p, i32p, f32p],
    "pk_tdt_kws_decode_timed": [C.c_void_p, f32p, i32p, C.c_int, C.c_int, i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), C.c_int, f32p],
    "pk_tdt_spot_pcm": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(C.c_char_p), i32p, i32p, C.c_int, C.POINTER(PkKwsOptions), i32p, f32p, f32p, f32p],
    "pk_diag_tdt_kws_lattice": [C.c_void_p, f32p, i32p, C.c_int, i32p, i32p, C.c_int, f32p, f32p, f32p, f32p],
    "pk_stream_kws_options_default": [C.POINTER(PkStreamKwsOptions)],
    "pk_tdt_kws_chunk_create": [i32p, C.c_int, C.c_int, i32p, C.POINTER(PkStreamKwsOptions), C.POINTER(C.c_void_p)],
    "pk_tdt_kws_chunk_push": [C.c_void_p, f32p, f32p, f32p, f32p, C.c_int, f32p, i32p, i32p, C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_tdt_kws_chunk_flush": [C.c_void_p, C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_tdt_kws_chunk_reset": [C.c_void_p],
    "pk_tdt_kws_chunk_free": [C.c_void_p],
    "pk_stream_set_keywords": [C.c_void_p, C.POINTER(C.c_char_p), i32p, i32p, C.c_int, C.POINTER(PkStreamKwsOptions)],
    "pk_stream_spot": [C.c_void_p, f32p, C.c_int, f32p, i32p, i32p, C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_stream_push_spot": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_stream_spot_flush": [C.c_void_p, C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_stream_spot_timed": [C.c_void_p, f32p, C.c_int, C.c_int, f32p],
    "pk_endpoint_options_default": [C.POINTER(PkEndpointOptions)],
    "pk_endpoint_chunk_create": [C.c_int, C.c_int, C.POINTER(PkEndpointOptions), C.POINTER(C.c_void_p)],
    "pk_endpoint_chunk_push": [C.c_void_p, f32p, C.c_int, f32p, f32p, i32p, C.POINTER(PkEndpointEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_endpoint_chunk_close": [C.c_void_p, C.POINTER(C.c_uint8)],
    "pk_endpoint_chunk_reset": [C.c_void_p],
    "pk_endpoint_chunk_free": [C.c_void_p],
    "pk_stream_set_endpointing": [C.c_void_p, C.POINTER(PkEndpointOptions)],
    "pk_stream_endpoint": [C.c_void_p, f32p, C.c_int, f32p, f32p, i32p, C.POINTER(PkEndpointEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_stream_push_endpoint": [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p, C.POINTER(PkEndpointEvent), C.c_int,
                                C.POINTER(C.c_int), C.POINTER(PkKwsEvent), C.c_int, C.POINTER(C.c_int)],
    "pk_stream_reset_decoder": [C.c_void_p, C.POINTER(C.c_uint8)],
    "pk_stream_endpoint_timed": [C.c_void_p, f32p, C.c_int, C.c_int, f32p],
    "pk_model_set_attention_context": [C.c_void_p, C.c_int, C.c_int],
    "pk_model_get_attention_context": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "pk_group_set_attention_context": [C.c_void_p, C.c_int, C.c_int],
    "pk_resample_length": [C.c_int64, C.c_int, C.c_int],
    "pk_resample_run": [C.c_int, C.c_int],
    "pk_resample_table": [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "pk_resample_device": [C.c_int, f32p, i64p, C.c_int, C.c_int, C.c_int, f32p, i64p],
    "pk_resample_device_timed": [C.c_int, f32p, i64p, C.c_int, C.c_int, C.c_int, C.c_int, f32p],
    "pk_vad_options_default": [C.POINTER(PkVadOptions)],
    "pk_vad_run": [],
    "pk_vad_pcm": [C.c_int, f32p, i64p, C.c_int, C.POINTER(PkVadOptions), i32p, i32p, i32p, f32p],
    "pk_vad_plan": [C.c_int64, i32p, i32p, C.c_int, f32p, C.POINTER(PkVadOptions), C.POINTER(C.POINTER(PkVadPiece)), C.POINTER(C.c_int)],
    "pk_vad_pcm_timed": [C.c_int, f32p, i64p, C.c_int, C.POINTER(PkVadOptions), C.c_int, f32p],
    "pk_transcribe_pcm_vad": [C.c_void_p, f32p, i64p, C.c_int, C.POINTER(PkOptions), C.POINTER(PkVadOptions), C.POINTER(C.POINTER(PkResult)),
                              C.POINTER(C.POINTER(PkVadPiece)), C.POINTER(C.c_int)],
    "pk_model_set_input_rate": [C.c_void_p, C.c_int],
    "pk_model_get_input_rate": [C.c_void_p, C.POINTER(C.c_int)],
    "pk_group_set_input_rate": [C.c_void_p, C.c_int],
    "pk_diag_conv_variants": [C.c_void_p, C.c_int, C.c_int, i32p, C.c_int, i32p],
    "pk_diag_conv_instantiations": [i32p, C.c_int],
    "pk_diag_pos_table_frames": [C.c_void_p, i32p],
    "pk_diag_relpos_local_attention": [C.c_int, i32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p,
                                       C.POINTER(C.c_int)],
    "pk_diag_relpos_attention_form": [C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, f32p, f32p,
                                      C.POINTER(C.c_int)],
    "pk_diag_stream_attention": [C.c_int] * 6 + [f32p] * 4 + [C.c_int, f32p, f32p] + [C.c_int] * 5 + [f32p] * 3 + [C.POINTER(C.c_int)],
    "pk_diag_mel": [C.c_int] * 5 + [f32p, C.c_int, C.c_int64, i64p, f32p, C.c_int64, f32p, C.c_int64, i32p, i32p],
    "pk_diag_ln_gemm_bf16": [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_float, f32p, f32p, C.c_int, f32p, C.c_float, f32p],
    "pk_diag_ln2_gemm_bf16": [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, C.c_float, f32p, f32p, f32p, f32p],
    "pk_diag_smallm_bf16_tiles": [C.c_int],
    "pk_diag_pred_cache": [C.c_int],
    "pk_diag_ffn_bf16_smallm": [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_float, f32p, f32p, f32p, f32p, C.c_int, f32p],
    "pk_diag_glu_dwconv_bf16": [C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, C.c_float, f32p, f32p, f32p, C.c_int] + [f32p] * 6 + [C.c_int, f32p, f32p],
    "pk_diag_sigma_copy": [f32p, C.c_int64, C.c_int, C.c_int64, f32p],
    "pk_diag_tile_copy_bf16": [f32p, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_uint16)],
    "pk_diag_layernorm_sigma": [f32p, C.c_int64, C.c_int, f32p, f32p, C.c_float, f32p],
    "pk_diag_layernorm2": [f32p, C.c_int64, C.c_int] + [f32p] * 4 + [C.c_float, C.c_int, f32p, f32p],
    "pk_diag_layernorm_form_of": [C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int32)],
    "pk_diag_gemm_tile_form": [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int32)],
}   # (the entries that take a struct are added where the struct is defined; lib() runs after the module has loaded)


def _f(a):
    return a.ctypes.data_as(f32p)


def _i(a):
    return a.ctypes.data_as(i32p)


def _c(a, dt=np.float32):
    return np.ascontiguousarray(a, dtype=dt)


def _pitched(a, ld):
    """a [rows][cols] at a row pitch of ld floats (zeros behind every row); a itself when ld is None or its width"""
    if ld is None or ld == a.shape[1]:
        return a
    p = np.zeros((a.shape[0], int(ld)), np.float32)
    n = min(a.shape[1], int(ld))
    p[:, :n] = a[:, :n]
    return p


class _Keep:
    """The arrays an argument struct points into, held until the wrapper returns.  opt(a): an optional array converted, retained -> its pointer (None: None)."""

    def __init__(self, *arrays):
        self.arrays = list(arrays)

    def opt(self, a, dt=np.float32):
        if a is None:
            return None
        a = _c(a, dt)
        self.arrays.append(a)
        return a.ctypes.data_as(f32p if dt == np.float32 else i32p)


def _forms(fn_name, decode):
    """a pk_diag_*_forms(out, cap) listing, every entry through `decode`"""
    fn = getattr(lib(), fn_name)
    out = np.zeros(fn(None, 0), np.int32)
    fn(_i(out), out.size)
    return [decode(int(v)) for v in out]


def _set_remap(d, remap):
    """remap = (rows, gs, rs, cs) or None into the remap_* fields of a product's argument struct"""
    if remap is not None:
        d.remap_rows, d.remap_gs, d.remap_rs, d.remap_cs = (int(v) for v in remap)


def _out_words_default(d, M, N, ldo, out_words, half=False, blocked=False):
    """d.ldo (default N) and d.out_words (default: the words of M rows at that pitch; half: two bf16 to a word; blocked: the rows rounded up to 32)"""
    d.ldo = int(ldo) if ldo is not None else N
    if out_words is None:
        rows = (M + 31) // 32 * 32 if blocked else M
        out_words = (rows * d.ldo + 1) // 2 if half else rows * d.ldo
    d.out_words = int(out_words)


def check(st):
    if st != 0:
        buf = C.create_string_buffer(2048)
        lib().pk_last_error(buf, 2048)
        raise PkError(st, buf.value.decode(errors="replace"))


def plan_batches(n_samples):
    """pk_plan_batches: how the one-call API packs clips of these lengths -> (batch_of_clip, pos_in_batch, n_batches).  Host logic."""
    n = np.ascontiguousarray(n_samples, np.int64)
    b = np.zeros(len(n), np.int32); p = np.zeros(len(n), np.int32); nb = C.c_int(0)
    check(lib().pk_plan_batches(n.ctypes.data_as(i64p), len(n), _i(b), _i(p), C.byref(nb)))
    return b, p, nb.value


def ragged_extents(n_samples):
    n = np.ascontiguousarray(n_samples, np.int64)
    tm = np.zeros(len(n), np.int32); t = np.zeros(len(n), np.int32); tot = np.zeros(7, np.int64)
    check(lib().pk_ragged_extents(n.ctypes.data_as(i64p), len(n), _i(tm), _i(t), tot.ctypes.data_as(i64p)))
    return tm, t, tot


def device_count():
    return lib().pk_device_count()


# ---- CTC prefix beam search (include/parakeet_amd.h) ------------------------------
def beam_options(beam_width=None, token_prune=None, n_best=None, timestamps=False):
    """pk_beam_options: the library's defaults (W = 8, K = 16, N = 1) with the given fields replaced."""
    o = PkBeamOptions()
    lib().pk_beam_options_default(C.byref(o))
    if beam_width is not None:
        o.beam_width = beam_width
    if token_prune is not None:
        o.token_prune = token_prune
    if n_best is not None:
        o.n_best = n_best
    o.timestamps = 1 if timestamps else 0
    return o


def tdt_beam_options(beam_width=None, label_prune=None, duration_prune=None, n_best=None):
    """pk_tdt_beam_options: the library's defaults (W = 8, K = 8, Kd = 2, N = 1) with the given fields replaced."""
    o = PkTdtBeamOptions()
    lib().pk_tdt_beam_options_default(C.byref(o))
    for k, v in (("beam_width", beam_width), ("label_prune", label_prune), ("duration_prune", duration_prune), ("n_best", n_best)):
        if v is not None:
            setattr(o, k, v)
    return o


def lm_options(alpha=None, beta=None):
    """pk_lm_options: the library's defaults (alpha = 0.5, beta = 0.0) with the given fields replaced."""
    o = PkLmOptions()
    lib().pk_lm_options_default(C.byref(o))
    if alpha is not None:
        o.alpha = alpha
    if beta is not None:
        o.beta = beta
    return o


class Lm:
    """pk_lm: a back-off n-gram language model over token ids (ARPA text; include/parakeet_amd.h)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        check(lib().pk_lm_load(os.fspath(path).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_text(cls, text):
        raw = text if isinstance(text, (bytes, bytearray)) else text.encode()
        h = C.c_void_p()
        check(lib().pk_lm_load_buffer(bytes(raw), len(raw), C.byref(h)))
        return cls(h)

    @property
    def order(self):
        return int(lib().pk_lm_order(self._h))

    @property
    def num_ngrams(self):
        fn = lib().pk_lm_num_ngrams
        fn.restype = C.c_int64
        return int(fn(self._h))

    def score(self, id_lists, bos=True, eos=False):
        """pk_lm_score: the fp32 log-probability (natural log) of every id list -> float32 array."""
        ids, off = _pack_ids(id_lists)
        out = np.zeros(len(id_lists), np.float32)
        check(lib().pk_lm_score(self._h, _i(ids), _i(off), len(id_lists), int(bool(bos)), int(bool(eos)), _f(out)))
        return out

    def close(self):
        if self._h:
            lib().pk_lm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _enc_head(enc):
    """(ragged?, packed rows, T[B]) of rows [B][T][d] or a list of [T_b][d] matrices: encoder output, or log-probabilities"""
    if isinstance(enc, (list, tuple)):
        T = np.asarray([e.shape[0] for e in enc], np.int32)
        return True, _c(np.concatenate([_c(e) for e in enc], axis=0)), T
    x = _c(enc)
    return False, x, np.full(x.shape[0], x.shape[1], np.int32)


def _tmax(rag, x, T):
    return int(T.max()) if rag else x.shape[1]


def _beam_call(fn, head, B, tmax, o, lm=None, lm_alpha=None, lm_beta=None):
    """lm given: fn is the _lm form of the entry point; the result gains "lm_score" [B][N]."""
    N = max(1, o.n_best)
    ids = np.zeros((B, N, tmax), np.int32); st = np.zeros((B, N, tmax), np.int32); en = np.zeros((B, N, tmax), np.int32)
    cf = np.zeros((B, N, tmax), np.float32); lens = np.zeros((B, N), np.int32); score = np.zeros((B, N), np.float32)
    if lm is None:
        check(fn(*head, C.byref(o), _i(ids), _i(lens), _f(score), _i(st), _i(en), _f(cf)))
        return dict(ids=ids, lens=lens, score=score, start=st, end=en, conf=cf)
    lo = lm_options(lm_alpha, lm_beta)
    lms = np.zeros((B, N), np.float32)
    check(fn(*head, C.byref(o), _i(ids), _i(lens), _f(score), _i(st), _i(en), _f(cf), lm._h, C.byref(lo), _f(lms)))
    return dict(ids=ids, lens=lens, score=score, start=st, end=en, conf=cf, lm_score=lms)


def ctc_beam_search(logp, blank, beam_width=None, token_prune=None, n_best=None, timestamps=False, lm=None, lm_alpha=None, lm_beta=None):
    """pk_ctc_beam_search: logp [B][T][V] (uniform) or a list of [T_b][V] matrices (ragged) -> dict of ids / start / end / conf
    [B][N][Tmax], lens / score [B][N]; hypotheses best first, an unfilled slot has lens 0 and score -inf.  Needs a device, no model.
    lm (an Lm): pk_ctc_beam_search_lm, shallow fusion with weights lm_alpha / lm_beta (None: the defaults); adds lm_score [B][N]."""
    o = beam_options(beam_width, token_prune, n_best, timestamps)
    fn = lib().pk_ctc_beam_search if lm is None else lib().pk_ctc_beam_search_lm
    rag, lp, T = _enc_head(logp)
    head = (_f(lp), _i(T) if rag else None, len(T), 0 if rag else lp.shape[1], lp.shape[-1], blank)
    return _beam_call(fn, head, len(T), _tmax(rag, lp, T), o, lm, lm_alpha, lm_beta)


# ---- CTC forced alignment of given token strings (include/parakeet_amd.h) ------
def _pack_ids(ids_list):
    off = np.zeros(len(ids_list) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in ids_list])
    ids = np.zeros(max(1, int(off[-1])), np.int32)
    if off[-1]:
        ids[: off[-1]] = np.concatenate([np.asarray(x, np.int32).ravel() for x in ids_list])
    return ids, off


def _align_call(fn, head, ids_list, total):
    """-> list (one dict per utterance) of start / end / conf arrays [L_b], score, ok and, when asked for, total."""
    B = len(ids_list)
    ids, off = _pack_ids(ids_list)
    st = np.zeros(len(ids), np.int32); en = np.zeros(len(ids), np.int32); cf = np.zeros(len(ids), np.float32)
    sc = np.zeros(B, np.float32); tt = np.zeros(B, np.float32); ok = np.zeros(B, np.int32)
    check(fn(*head, _i(ids), _i(off), _i(st), _i(en), _f(cf), _f(sc), _f(tt) if total else None, _i(ok)))
    out = []
    for b in range(B):
        d = dict(start=st[off[b]:off[b + 1]].copy(), end=en[off[b]:off[b + 1]].copy(), conf=cf[off[b]:off[b + 1]].copy(), score=sc[b], ok=int(ok[b]))
        if total:
            d["total"] = tt[b]
        out.append(d)
    return out


def ctc_align(logp, ids, blank, total=True):
    """pk_ctc_align: logp [B][T][V] (uniform) or a list of [T_b][V] matrices (ragged); ids: one token sequence per utterance.
    Needs a device, no model."""
    rag, lp, T = _enc_head(logp)
    return _align_call(lib().pk_ctc_align, (_f(lp), _i(T) if rag else None, len(T), 0 if rag else lp.shape[1], lp.shape[-1], blank), ids, total)


# ---- TDT forced alignment of given token strings (include/parakeet_amd.h) ------
TDT_LATTICE_GUARD = 64                                              # PK_DIAG_TDT_LATTICE_GUARD


def _tdt_align_call(fn, head, off):
    """-> list (one dict per utterance) of start / end / dur_idx / conf arrays [U_b], score, ok.  head: the arguments in front of id_offsets."""
    B = len(off) - 1
    n = max(1, int(off[-1]))
    st = np.zeros(n, np.int32); en = np.zeros(n, np.int32); di = np.zeros(n, np.int32); cf = np.zeros(n, np.float32)
    sc = np.zeros(B, np.float32); ok = np.zeros(B, np.int32)
    check(fn(*head, _i(off), _i(st), _i(en), _i(di), _f(cf), _f(sc), _i(ok)))
    return [dict(start=st[off[b]:off[b + 1]].copy(), end=en[off[b]:off[b + 1]].copy(), dur_idx=di[off[b]:off[b + 1]].copy(),
                 conf=cf[off[b]:off[b + 1]].copy(), score=sc[b], ok=int(ok[b])) for b in range(B)]


def mem_info(model=None):
    """pk_diag_mem_info -> (free bytes, total bytes of the device, bytes the model's grow-only stage buffers hold)"""
    out = (C.c_uint64 * 3)()
    check(lib().pk_diag_mem_info(model._h if model is not None else None, out))
    return int(out[0]), int(out[1]), int(out[2])


def tdt_align(lattices, durations):
    """pk_tdt_align: lattices = one (lab [T][U], blk [T][U+1], dl [T][U+1][D]) per utterance.  Needs a device, no model."""
    T = np.asarray([x[1].shape[0] for x in lattices], np.int32)
    off = np.zeros(len(lattices) + 1, np.int32)
    off[1:] = np.cumsum([x[1].shape[1] - 1 for x in lattices])
    cat = lambda k: _c(np.concatenate([_c(x[k]).ravel() for x in lattices] + [np.zeros(1, np.float32)]))
    lab, blk, dl = cat(0), cat(1), cat(2)
    dur = np.ascontiguousarray(durations, np.int32)
    return _tdt_align_call(lib().pk_tdt_align, (_f(lab), _f(blk), _f(dl), _i(dur), len(dur), _i(T), len(T)), off)


# ---- TDT log-likelihood of given token strings, n-best rescoring (include/parakeet_amd.h) ------
def tdt_total(lattices, durations):
    """pk_tdt_total: lattices as capi.tdt_align takes them -> list (one dict per utterance) of total, ok.  Needs a device, no model."""
    T = np.asarray([x[1].shape[0] for x in lattices], np.int32)
    off = np.zeros(len(lattices) + 1, np.int32)
    off[1:] = np.cumsum([x[1].shape[1] - 1 for x in lattices])
    cat = lambda k: _c(np.concatenate([_c(x[k]).ravel() for x in lattices] + [np.zeros(1, np.float32)]))
    lab, blk, dl = cat(0), cat(1), cat(2)
    dur = np.ascontiguousarray(durations, np.int32)
    tt = np.zeros(len(T), np.float32); ok = np.zeros(len(T), np.int32)
    check(lib().pk_tdt_total(_f(lab), _f(blk), _f(dl), _i(dur), len(dur), _i(T), len(T), _i(off), _f(tt), _i(ok)))
    return [dict(total=tt[b], ok=int(ok[b])) for b in range(len(T))]


def tdt_total_groups(n_frames_of_hyp, lengths, durations, V, J, max_hyps=0):
    """pk_diag_tdt_total_groups: the group every hypothesis (n_frames_of_hyp[h] frames, lengths[h] tokens) is walked in.  Host arithmetic."""
    T = np.ascontiguousarray(n_frames_of_hyp, np.int32)
    off = np.zeros(len(T) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    dur = np.ascontiguousarray(durations, np.int32)
    g = np.zeros(len(T), np.int32); n = C.c_int(0)
    check(lib().pk_diag_tdt_total_groups(_i(T), _i(off), len(T), _i(dur), len(dur), int(V), int(J), int(max_hyps), _i(g), C.byref(n)))
    return g, n.value


def rescore_order(lens, ctc, tdt, ok, tdt_weight):
    """pk_diag_rescore_order: the ordering rule of pk_transcribe_pcm_nbest_rescored on the N slots of one clip -> (order, combined by slot).
    Host arithmetic."""
    lens, ok = np.ascontiguousarray(lens, np.int32), np.ascontiguousarray(ok, np.int32)
    ctc, tdt = np.ascontiguousarray(ctc, np.float32), np.ascontiguousarray(tdt, np.float32)
    order = np.zeros(len(ctc), np.int32); comb = np.zeros(len(ctc), np.float32)
    check(lib().pk_diag_rescore_order(_i(lens), _f(ctc), _f(tdt), _i(ok), len(ctc), float(tdt_weight), _i(order), _f(comb)))
    return order.tolist(), comb


# ---- CTC keyword spotting (include/parakeet_amd.h) -----------------------------
def kws_options(max_hits=None, min_score=None):
    """pk_kws_options: the library's defaults (max_hits = 1, min_score = -inf) with the given fields replaced."""
    o = PkKwsOptions()
    lib().pk_kws_options_default(C.byref(o))
    if max_hits is not None:
        o.max_hits = max_hits
    if min_score is not None:
        o.min_score = min_score
    return o


def _kws_call(fn, head, B, keywords, o):
    """-> dict of n_hits [B][n_kw], start / end / score [B][n_kw][max_hits] (unused slots 0 / 0 / -inf)."""
    ids, off = _pack_ids(keywords)
    K, H = len(keywords), max(1, o.max_hits)
    nh = np.zeros((B, K), np.int32); st = np.zeros((B, K, H), np.int32); en = np.zeros((B, K, H), np.int32); sc = np.zeros((B, K, H), np.float32)
    check(fn(*head, _i(ids), _i(off), K, C.byref(o), _i(nh), _i(st), _i(en), _f(sc)))
    return dict(n_hits=nh, start=st, end=en, score=sc)


def ctc_kws(logp, keywords, blank, max_hits=None, min_score=None):
    """pk_ctc_kws: logp [B][T][V] (uniform) or a list of [T_b][V] matrices (ragged); keywords: a list of token sequences, every one searched
    in every utterance.  Needs a device, no model."""
    o = kws_options(max_hits, min_score)
    rag, lp, T = _enc_head(logp)
    return _kws_call(lib().pk_ctc_kws, (_f(lp), _i(T) if rag else None, len(T), 0 if rag else lp.shape[1], lp.shape[-1], blank), len(T), keywords, o)


# ---- TDT keyword spotting (include/parakeet_amd.h) -----------------------------
def tdt_kws(lattices, durations, max_hits=None, min_score=None):
    """pk_tdt_kws: lattices = one (lab [T][L], blk [T][L+1], dl [T][L+1][D], top [T][L+1]) per (clip, keyword) pair -> dict of n_hits [B],
    start / end / score [B][max_hits] (unused slots 0 / 0 / -inf).  Needs a device, no model."""
    o = kws_options(max_hits, min_score)
    T = np.asarray([x[1].shape[0] for x in lattices], np.int32)
    off = np.zeros(len(lattices) + 1, np.int32)
    off[1:] = np.cumsum([x[1].shape[1] - 1 for x in lattices])
    cat = lambda k: _c(np.concatenate([_c(x[k]).ravel() for x in lattices] + [np.zeros(1, np.float32)]))
    lab, blk, dl, top = cat(0), cat(1), cat(2), cat(3)
    dur = np.ascontiguousarray(durations, np.int32)
    B, H = len(T), max(1, o.max_hits)
    nh = np.zeros(B, np.int32); st = np.zeros((B, H), np.int32); en = np.zeros((B, H), np.int32); sc = np.zeros((B, H), np.float32)
    check(lib().pk_tdt_kws(_f(lab), _f(blk), _f(dl), _f(top), _i(dur), len(dur), _i(T), B, _i(off), C.byref(o), _i(nh), _i(st), _i(en), _f(sc)))
    return dict(n_hits=nh, start=st, end=en, score=sc)


# ---- streaming TDT keyword spotting (include/parakeet_amd.h) --------------------
KWS_CHUNK_MAX = 62


def stream_kws_options(min_score=None, patience=None):
    """pk_stream_kws_options: the library's defaults (min_score = -inf, patience = 0) with the given fields replaced."""
    o = PkStreamKwsOptions()
    lib().pk_stream_kws_options_default(C.byref(o))
    if min_score is not None:
        o.min_score = min_score
    if patience is not None:
        o.patience = patience
    return o


def _events(buf, n):
    """-> [(stream, keyword, start, end, score as np.float32)...]"""
    return [(e.stream, e.keyword, e.start, e.end, np.float32(e.score)) for e in buf[:n]]


class TdtKwsChunkWalk:
    """pk_tdt_kws_chunk_*: the chunked walk and the online rule alone on host lattices, n pairs with keywords of kw_len[p] tokens.  Needs a
    device, no model."""

    def __init__(self, kw_len, durations, min_score=None, patience=None):
        self.kw_len = np.ascontiguousarray(kw_len, np.int32)
        self.dur = np.ascontiguousarray(durations, np.int32)
        self.n = len(self.kw_len)
        o = stream_kws_options(min_score, patience)
        self._h = C.c_void_p()
        check(lib().pk_tdt_kws_chunk_create(_i(self.dur), len(self.dur), self.n, _i(self.kw_len), C.byref(o), C.byref(self._h)))

    def push(self, lattices, rows=True, cap=None, c=None):
        """lattices: one (lab [c][L], blk [c][L+1], dl [c][L+1][D], top [c][L+1]) per pair, the next c frames -> dict(E, Bs, Ee [n][c] (rows),
        events (the first cap), n_events (the total))."""
        assert len(lattices) == self.n
        c = lattices[0][1].shape[0] if c is None else c
        cat = lambda k: _c(np.concatenate([_c(x[k]).ravel() for x in lattices] + [np.zeros(1, np.float32)]))
        lab, blk, dl, top = cat(0), cat(1), cat(2), cat(3)
        cap = self.n * max(c, 1) if cap is None else cap
        ev = (PkKwsEvent * max(cap, 1))()
        n = C.c_int(0)
        cc = max(c, 1)
        E = np.zeros((self.n, cc), np.float32); Bs = np.zeros((self.n, cc), np.int32); Ee = np.zeros((self.n, cc), np.int32)
        check(lib().pk_tdt_kws_chunk_push(self._h, _f(lab), _f(blk), _f(dl), _f(top), c, _f(E) if rows else None, _i(Bs) if rows else None,
                                          _i(Ee) if rows else None, ev, cap, C.byref(n)))
        return dict(E=E, Bs=Bs, Ee=Ee, events=_events(ev, min(n.value, cap)), n_events=n.value)

    def flush(self):
        ev = (PkKwsEvent * self.n)()
        n = C.c_int(0)
        check(lib().pk_tdt_kws_chunk_flush(self._h, ev, self.n, C.byref(n)))
        return _events(ev, n.value)

    def reset(self):
        check(lib().pk_tdt_kws_chunk_reset(self._h))

    def close(self):
        if self._h:
            lib().pk_tdt_kws_chunk_free(self._h)
            self._h = None


# ---- endpointing on live audio (include/parakeet_amd.h) ------------------------
ENDPOINT_START, ENDPOINT_END = 1, 2
ENDPOINT_NONE, ENDPOINT_SILENCE, ENDPOINT_MAX_LENGTH, ENDPOINT_TOKEN = 0, 1, 2, 3
ENDPOINT_MAX_FRAMES = 512


def endpoint_options(**kw):
    """pk_endpoint_options: the library's defaults with the given fields replaced."""
    o = PkEndpointOptions()
    lib().pk_endpoint_options_default(C.byref(o))
    for k, v in kw.items():
        if v is not None:
            assert hasattr(o, k), k
            setattr(o, k, v)
    return o


def _ep_events(buf, n):
    """-> [(stream, kind, reason, start, end, at)...]"""
    return [(e.stream, e.kind, e.reason, e.start, e.end, e.at) for e in buf[:n]]


def _mask(mask, S):
    m = np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8)
    assert m.shape == (S,)
    return m, m.ctypes.data_as(C.POINTER(C.c_uint8))


class EndpointChunk:
    """pk_endpoint_chunk_*: the endpointing kernel and its rule alone on host rows, n_streams independent streams of n_mels bins.  Needs a device,
    no model."""

    def __init__(self, n_streams, n_mels, **options):
        self.S, self.F = n_streams, n_mels
        o = endpoint_options(**options)
        self._h = C.c_void_p()
        check(lib().pk_endpoint_chunk_create(n_streams, n_mels, C.byref(o), C.byref(self._h)))

    def push(self, rows, want_rows=True, cap=None):
        """rows [S][n][F], the next n frames of every stream -> dict(level, floor, speech0 [S][n] (want_rows), events (the first cap), n_events (the
        total))."""
        rows = _c(rows)
        assert rows.ndim == 3 and rows.shape[0] == self.S and rows.shape[2] == self.F
        n = rows.shape[1]
        cap = self.S * max(n, 1) if cap is None else cap
        ev = (PkEndpointEvent * max(cap, 1))()
        ne = C.c_int(0)
        lv = np.zeros((self.S, max(n, 1)), np.float32); fl = np.zeros((self.S, max(n, 1)), np.float32); sp = np.zeros((self.S, max(n, 1)), np.int32)
        padded = _c(np.concatenate([rows.ravel(), np.zeros(1, np.float32)]))
        check(lib().pk_endpoint_chunk_push(self._h, _f(padded), n, _f(lv) if want_rows else None, _f(fl) if want_rows else None,
                                           _i(sp) if want_rows else None, ev, cap, C.byref(ne)))
        return dict(level=lv, floor=fl, speech0=sp, events=_ep_events(ev, min(ne.value, cap)), n_events=ne.value)

    def close_streams(self, mask):
        """pk_endpoint_chunk_close: the acoustic close of the streams with mask[s] set."""
        m, p = _mask(mask, self.S)
        check(lib().pk_endpoint_chunk_close(self._h, p))

    def reset(self):
        check(lib().pk_endpoint_chunk_reset(self._h))

    def close(self):
        if self._h:
            lib().pk_endpoint_chunk_free(self._h)
            self._h = None


class Utterances:
    """Collects the tokens of every stream of a session that pushes through Stream.push_endpoint and yields the utterances that finished: feed(r) with
    push_endpoint's dict -> [dict(stream, ids, text (None without a vocabulary), start, end (seconds: frame * 0.01), reason)...].  The tokens a push
    returns belong to the utterance that ended in it."""

    def __init__(self, stream):
        self.stream = stream
        self.ids = [[] for _ in range(stream.S)]

    def feed(self, r):
        out = []
        for s in range(self.stream.S):
            self.ids[s] += r["ids"][s, :r["lens"][s]].tolist()
        for (s, kind, reason, start, end, at) in r["events"]:
            if kind != ENDPOINT_END:
                continue
            ids, self.ids[s] = self.ids[s], []
            text = None
            if lib().pk_vocab_size(self.stream.model._h) > 0:
                arr = np.ascontiguousarray(ids + [0], np.int32)
                buf = C.create_string_buffer(lib().pk_detokenize(self.stream.model._h, _i(arr), len(ids), None, 0) + 1)
                lib().pk_detokenize(self.stream.model._h, _i(arr), len(ids), buf, len(buf))
                text = buf.value.decode("utf-8", "replace")
            out.append(dict(stream=s, ids=ids, text=text, start=start * 0.01, end=end * 0.01, reason=reason))
        return out


# ---- diagnostics ---------------------------------------------------------------------------------
MATH_FN = {"exp": 0, "log": 1, "tanh": 2, "sigmoid": 3, "silu": 4, "sqrt": 5, "rcp": 6, "sigmoid4": 8, "silu4": 9, "fast_sigmoid": 20, "fast_silu": 21}
EPI = {"none": 0, "relu": 1, "silu": 2, "resid": 3, "glu": 4}


def diag_math(fn, x):
    x = _c(x)
    y = np.empty_like(x)
    check(lib().pk_diag_math(MATH_FN[fn], _f(x), _f(y), x.size))
    return y


def diag_math_exhaustive(fn, guarded=False):
    """all 2^32 bit patterns through the device-side identity of pk_diag_math_exhaustive -> (checked, mismatches, first_bad)"""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().pk_diag_math_exhaustive(MATH_FN[fn] + (10 if guarded else 0), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def resample(pcm, src_rate, dst_rate):
    """pk_resample: the reference's Kaiser-windowed sinc resampler (src/audio_io.cpp:123-195)."""
    pcm = _c(pcm)
    L = lib()
    L.pk_resample.argtypes = [f32p, C.c_int64, C.c_int, C.c_int, C.POINTER(f32p), C.POINTER(C.c_int64)]
    L.pk_free.argtypes = [C.c_void_p]
    out, n = f32p(), C.c_int64(0)
    check(L.pk_resample(_f(pcm), pcm.size, src_rate, dst_rate, C.byref(out), C.byref(n)))
    r = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[: n.value].copy()
    L.pk_free(out)
    return r


def resample_length(n, src_rate, dst_rate):
    """pk_resample_length: samples pk_resample returns for n input samples (host arithmetic)."""
    L = lib()
    L.pk_resample_length.restype = C.c_int64
    r = L.pk_resample_length(int(n), int(src_rate), int(dst_rate))
    if r < 0:                      # refused: negative n is PK_ERR_INVALID, a rate or a length out of range PK_ERR_UNSUPPORTED
        check(-1 if int(n) < 0 and all(4000 <= int(x) <= 384000 for x in (src_rate, dst_rate)) else -7)
    return r


def resample_run(src_rate, dst_rate):
    """pk_resample_run: outputs one workgroup of the resampling kernel owns at this pair of rates."""
    return lib().pk_resample_run(int(src_rate), int(dst_rate))


def resample_table(src_rate, dst_rate):
    """pk_resample_table: the phase table of the device resampler -> (table [up][32] float64, up, down).  Host only."""
    up, down = C.c_int(0), C.c_int(0)
    check(lib().pk_resample_table(int(src_rate), int(dst_rate), None, 0, C.byref(up), C.byref(down)))
    t = np.zeros((up.value, 32), np.float64)
    check(lib().pk_resample_table(int(src_rate), int(dst_rate), t.ctypes.data_as(C.POINTER(C.c_double)), up.value, C.byref(up), C.byref(down)))
    return t, up.value, down.value


def resample_device(clips, src_rate, dst_rate, device=0, out=None, out_offsets=None):
    """pk_resample_device: a list of input-rate clips (empty ones allowed) through the device resampler -> list of dst-rate clips.
    out / out_offsets (n + 1 entries): write into the caller's buffer instead (everything of out[: out_offsets[-1]] outside the clips'
    outputs comes back untouched) and return it."""
    clips = [_c(c).reshape(-1) for c in clips]
    off = np.zeros(len(clips) + 1, np.int64)
    off[1:] = np.cumsum([c.size for c in clips])
    pcm = np.concatenate(clips) if off[-1] else np.zeros(1, np.float32)
    lens = [resample_length(c.size, src_rate, dst_rate) for c in clips]
    own = out is None
    if own:
        out_offsets = np.zeros(len(clips) + 1, np.int64)
        out_offsets[1:] = np.cumsum(lens)
        out = np.zeros(max(int(out_offsets[-1]), 1), np.float32)
    out_offsets = np.ascontiguousarray(out_offsets, np.int64)
    check(lib().pk_resample_device(int(device), _f(pcm), off.ctypes.data_as(i64p), len(clips), int(src_rate), int(dst_rate), _f(out),
                                   out_offsets.ctypes.data_as(i64p)))
    if not own:
        return out
    return [out[out_offsets[i]: out_offsets[i] + lens[i]].copy() for i in range(len(clips))]


def resample_device_timed(clips, src_rate, dst_rate, reps=20, device=0):
    """pk_resample_device_timed: median milliseconds of the resampling launch alone (hipEvents; the input is on the device)."""
    clips = [_c(c).reshape(-1) for c in clips]
    off = np.zeros(len(clips) + 1, np.int64)
    off[1:] = np.cumsum([c.size for c in clips])
    pcm = np.concatenate(clips)
    ms = np.zeros(1, np.float32)
    check(lib().pk_resample_device_timed(int(device), _f(pcm), off.ctypes.data_as(i64p), len(clips), int(src_rate), int(dst_rate), int(reps), _f(ms)))
    return float(ms[0])


def vad_options(**options):
    """pk_vad_options: the defaults of pk_vad_options_default with the given fields replaced"""
    o = PkVadOptions()
    lib().pk_vad_options_default.restype = None
    lib().pk_vad_options_default(C.byref(o))
    for k, v in options.items():
        if k not in dict(PkVadOptions._fields_):
            raise TypeError(f"no VAD option {k!r}")
        setattr(o, k, v)
    return o


def vad_run():
    """pk_vad_run: frames one workgroup of the VAD kernels handles per pass"""
    return lib().pk_vad_run()


def _vad_pieces(ptr, n):
    """a pk_vad_piece array (freed here) as a list of (clip, begin, end)"""
    try:
        return [(ptr[i].clip, ptr[i].begin, ptr[i].end) for i in range(n)]
    finally:
        lib().pk_free.argtypes = [C.c_void_p]
        lib().pk_free(C.cast(ptr, C.c_void_p))


def vad(clips, device=0, run_start=None, run_end=None, energy=None, **options):
    """pk_vad_pcm: a list of 16 kHz clips (empty ones allowed) through the device VAD -> list of dicts with runs ([n][2] int32 frame ranges,
    ends inclusive) and energy ([F] float32).  run_start / run_end / energy: the arrays the call works in (with their contents), for tests that
    look at what the kernels leave alone; clip i's runs start at the sum of (F_j + 1) // 2 over the clips before it."""
    pcm, off, n = _clips(clips)
    F = [(int(off[i + 1] - off[i]) + 159) // 160 for i in range(n)]
    cap = [(f + 1) // 2 for f in F]
    rs = np.zeros(max(1, sum(cap)), np.int32) if run_start is None else run_start
    re = np.zeros(max(1, sum(cap)), np.int32) if run_end is None else run_end
    en = np.zeros(max(1, sum(F)), np.float32) if energy is None else energy
    nr = np.zeros(n, np.int32)
    o = vad_options(**options)
    check(lib().pk_vad_pcm(int(device), _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), _i(nr), _i(rs), _i(re), _f(en)))
    out, r0, f0 = [], 0, 0
    for i in range(n):
        out.append(dict(runs=np.stack([rs[r0:r0 + nr[i]], re[r0:r0 + nr[i]]], axis=1), energy=en[f0:f0 + F[i]].copy()))
        r0 += cap[i]
        f0 += F[i]
    return out


def vad_timed(clips, reps=20, device=0, **options):
    """pk_vad_pcm_timed: median milliseconds of the VAD launches alone (hipEvents; the input is on the device)."""
    pcm, off, n = _clips(clips)
    ms = np.zeros(1, np.float32)
    o = vad_options(**options)
    check(lib().pk_vad_pcm_timed(int(device), _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), int(reps), _f(ms)))
    return float(ms[0])


def vad_plan(n_samples, runs, energy, **options):
    """pk_vad_plan: the pieces of one clip from its runs ([n][2] frame ranges) and frame energies -> list of (begin, end) samples.  Host only."""
    runs = np.ascontiguousarray(runs, np.int32).reshape(-1, 2)
    rs, re = np.ascontiguousarray(runs[:, 0]), np.ascontiguousarray(runs[:, 1])
    en = None if energy is None else np.ascontiguousarray(energy, np.float32)
    o = vad_options(**options)
    ptr, n = C.POINTER(PkVadPiece)(), C.c_int(0)
    check(lib().pk_vad_plan(int(n_samples), _i(rs), _i(re), len(runs), None if en is None else _f(en), C.byref(o), C.byref(ptr), C.byref(n)))
    return [(b, e) for _, b, e in _vad_pieces(ptr, n.value)]


def read_audio(path, target_rate=16000):
    """pk_read_audio: WAV -> mono -> resampled to target_rate; returns (pcm, original_rate)."""
    L = lib()
    L.pk_read_audio.argtypes = [C.c_char_p, C.c_int, C.POINTER(f32p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.pk_free.argtypes = [C.c_void_p]
    out, n, sr = f32p(), C.c_int64(0), C.c_int(0)
    check(L.pk_read_audio(path.encode(), target_rate, C.byref(out), C.byref(n), C.byref(sr)))
    r = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[: n.value].copy()
    L.pk_free(out)
    return r, sr.value


def diag_gemm(A, W, bias=None, epi="none", resid=None, alpha=1.0, bf16=False, a16=False):
    A, W = _c(A), _c(W)
    M, K = A.shape
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    b = _c(bias) if bias is not None else None
    r = _c(resid) if resid is not None else None
    out = np.empty((M, N), np.float32)
    fn = (lib().pk_diag_gemm_bf16_a16 if a16 else lib().pk_diag_gemm_bf16) if bf16 else lib().pk_diag_gemm
    check(fn(M, N, K, _f(A), _f(W), _f(b) if b is not None else None, EPI[epi], _f(r) if r is not None else None, alpha, _f(out)))
    return out


def diag_ln_gemm_bf16(A, gamma, beta, W, bias=None, epi="none", resid=None, alpha=1.0, eps=1e-5):
    """pk_diag_ln_gemm_bf16: epi(bf16(LayerNorm(A)) bf16(W)^T + bias) on the small-M bf16 kernel with the LayerNorm folded in."""
    A, W, gamma, beta = _c(A), _c(W), _c(gamma), _c(beta)
    M, K = A.shape
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    b = _c(bias) if bias is not None else None
    r = _c(resid) if resid is not None else None
    out = np.empty((M, N), np.float32)
    check(lib().pk_diag_ln_gemm_bf16(M, N, K, _f(A), _f(gamma), _f(beta), eps, _f(W), _f(b) if b is not None else None, EPI[epi],
                                     _f(r) if r is not None else None, alpha, _f(out)))
    return out


def diag_ln2_gemm_bf16(A, pre_gamma, pre_beta, gamma, beta, W, bias, eps=1e-5):
    """pk_diag_ln2_gemm_bf16: silu(bf16(LN(LN(A; pre); gamma, beta)) bf16(W)^T + bias) and LN(A; pre) on the small-M bf16 kernel."""
    A, W, pg, pb, g, b, bias = (_c(v) for v in (A, W, pre_gamma, pre_beta, gamma, beta, bias))
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), np.float32); pre = np.empty((M, K), np.float32)
    check(lib().pk_diag_ln2_gemm_bf16(M, N, K, _f(A), _f(pg), _f(pb), _f(g), _f(b), eps, _f(W), _f(bias), _f(out), _f(pre)))
    return out, pre


def diag_smallm_bf16_tiles(on):
    """pk_diag_smallm_bf16_tiles: the bf16 diag products with / without the operand-tiled weight copy (test switch, process-wide)."""
    check(lib().pk_diag_smallm_bf16_tiles(int(on)))


class PkSkinnyDiag(C.Structure):
    _fields_ = [("bf16", C.c_int32), ("epi", C.c_int32), ("B", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("X", f32p), ("W", f32p), ("bias", f32p),
                ("gi", f32p), ("gi_rows", C.c_int32), ("gi_ld", C.c_int32), ("gi_row", i32p), ("c", f32p),
                ("X2", f32p), ("W2", f32p), ("bias2", f32p),
                ("ep", f32p), ("ep_rows", C.c_int64), ("t", i32p), ("T", C.c_int32), ("Tb", i32p), ("row0", i32p), ("F", C.c_int32),
                ("need", i32p), ("out_rows", C.c_int32), ("ldo", C.c_int32), ("out", C.c_void_p), ("cn", f32p), ("pp_out", f32p)]


_LATE_SIGNATURES["pk_diag_skinny_gemm"] = [C.POINTER(PkSkinnyDiag)]


SKINNY_EPI = {"bias": 0, "act": 1, "cell": 2}
SKINNY_FILL32, SKINNY_FILL16 = 0x7FC5A5A5, 0x7FC5          # what an element no store reached comes back as (fp32 / bf16 outputs)


def sigma16(n):
    """the fp32 decode kernels' column order (pk_devmath.h sigma_col; its own inverse): the 4x4 index transpose inside every block of 16"""
    k = np.arange(n)
    return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3)


def diag_skinny_gemm(epi, X, W, bias=None, bf16=False, gi=None, gi_row=None, c=None, X2=None, W2=None, bias2=None, ep=None, t=None, T=0,
                     Tb=None, row0=None, F=1, want_pp=False, need=None, pad_rows=3, pad_cols=5):
    """pk_diag_skinny_gemm: one launch of a decode-loop product on operands in natural layout (include/parakeet_amd.h).  Returns a dict of the WHOLE
    output buffers, pattern-filled before the launch (SKINNY_FILL32 / SKINNY_FILL16) and pad_rows rows longer than the batch: `out` ([B F + pad][N + pad_cols]
    fp32 for "bias"; [B F + pad][N] for "act" / "cell": uint16 bf16 words in the bf16 mode, else fp32 words with the sigma column order undone), `cn`
    (cell) and `pp` (act with want_pp) as uint32 words."""
    e = SKINNY_EPI[epi]
    X, W = _c(X), _c(W)
    B, K = X.shape
    N = W.shape[0] // 4 if epi == "cell" else W.shape[0]
    F = int(F) if epi == "act" else 1
    rows = B * F + pad_rows
    opt = _Keep(X, W).opt

    d = PkSkinnyDiag()
    d.bf16, d.epi, d.B, d.N, d.K = int(bool(bf16)), e, B, N, K
    d.X, d.W, d.bias = _f(X), _f(W), opt(bias)
    if gi is not None:
        gi = _c(gi)
        d.gi_rows, d.gi_ld = gi.shape
    d.gi, d.gi_row, d.c = opt(gi), opt(gi_row, np.int32), opt(c)
    d.X2, d.W2, d.bias2 = opt(X2), opt(W2), opt(bias2)
    if ep is not None:
        ep = _c(ep).reshape(-1, N)
        d.ep_rows = ep.shape[0]
    d.ep, d.t, d.T, d.Tb, d.row0, d.F = opt(ep), opt(t, np.int32), int(T), opt(Tb, np.int32), opt(row0, np.int32), F
    d.need = opt(need, np.int32)
    ld = N + pad_cols if epi == "bias" else N
    half = bool(bf16) and epi != "bias"
    out = np.full((rows, ld), SKINNY_FILL16 if half else SKINNY_FILL32, np.uint16 if half else np.uint32)
    cn = np.full((rows, N), SKINNY_FILL32, np.uint32) if epi == "cell" else None
    pp = np.full((rows, N), SKINNY_FILL32, np.uint32) if (epi == "act" and want_pp) else None
    d.out_rows, d.ldo, d.out = rows, ld, out.ctypes.data_as(C.c_void_p)
    d.cn = cn.ctypes.data_as(f32p) if cn is not None else None
    d.pp_out = pp.ctypes.data_as(f32p) if pp is not None else None
    check(lib().pk_diag_skinny_gemm(C.byref(d)))
    if not half and epi != "bias":
        out = np.ascontiguousarray(out[:, sigma16(N)])
    return dict(out=out, cn=cn, pp=pp)


class PkTdtDecideDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("B", "T", "V", "D", "L", "Hp", "blank", "max_symbols", "max_tokens", "max_steps", "keep_state", "h_bf16", "F", "J")]
                + [("durations", C.c_int32 * 8), ("n_steps", C.c_int32), ("rows", C.c_int32),
                   ("logits", f32p), ("hn", C.c_void_p), ("cn", f32p)]
                + [(k, i32p) for k in ("t", "steps", "n_out", "nsym", "done", "token", "lens", "done_count")]
                + [("h", C.c_void_p), ("c", f32p), ("h_words", C.c_int64), ("c_words", C.c_int64),
                   ("ids", i32p), ("start", i32p), ("end", i32p), ("conf", f32p), ("margin", f32p),
                   ("need", i32p), ("pp", f32p), ("ep", f32p), ("ep_rows", C.c_int64), ("z", C.c_void_p), ("z_words", C.c_int64),
                   ("Tb", i32p), ("row0", i32p),
                   ("trie_off", i32p), ("trie_tok", i32p), ("trie_node", i32p), ("trie_nodes", C.c_int32), ("boost", C.c_float), ("act", i32p), ("n_act", i32p),
                   ("force_label", i32p), ("force_dur", i32p), ("force_len", C.c_int64), ("n_force", C.c_int32), ("n_force_b", i32p), ("force_stride", C.c_int32),
                   ("score_lab", f32p), ("score_dur", f32p), ("score_rows", C.c_int64)])


_LATE_SIGNATURES["pk_diag_tdt_decide"] = [C.POINTER(PkTdtDecideDiag), C.POINTER(C.c_int)]


class PkCtcGreedyDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("B", "T", "n", "ld", "blank", "pitch", "out_rows")]
                + [("n_frames", i32p), ("logits", f32p), ("lp_rows", C.c_int64), ("lp", f32p), ("best_idx", i32p), ("best_lp", f32p), ("best_idx2", i32p), ("best_lp2", f32p),
                   ("ids", i32p), ("lens", i32p), ("start", i32p), ("end", i32p), ("conf", f32p),
                   ("trie_off", i32p), ("trie_tok", i32p), ("trie_node", i32p), ("trie_nodes", C.c_int32), ("boost", C.c_float)])


_LATE_SIGNATURES["pk_diag_ctc_greedy"] = [C.POINTER(PkCtcGreedyDiag)]


TDT_KERNELS = ("exact", "fast", "boost", "score")                  # PK_DIAG_TDT_KERNEL
TDT_ROWS = ("row5", "row33", "batch8", "window")                   # PK_DIAG_TDT_ROW


def tdt_form(form):
    """PK_DIAG_TDT_KERNEL / _SLOTS / _ROW of a form word -> (kernel, NC, row staging)"""
    return TDT_KERNELS[form >> 4], 3 << ((form >> 2) & 3), TDT_ROWS[form & 3]


def _padded(a, lead, dt, pad):
    """`a` (its first axis = lead rows) as dt words with `pad` pattern-filled rows behind it"""
    a = np.ascontiguousarray(a)
    assert a.shape[0] == lead and a.dtype.itemsize == np.dtype(dt).itemsize, (a.shape, a.dtype, lead)
    out = np.full((lead + pad,) + a.shape[1:], SKINNY_FILL32, np.uint32).view(dt)
    out[:lead] = a.view(dt)
    return out


def _flat_guard(a, guard):
    """a's bytes as 32-bit words with `guard` pattern words behind them"""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    assert w.size % 4 == 0
    out = np.full(w.size // 4 + guard, SKINNY_FILL32, np.uint32)
    out[: w.size // 4] = w.view(np.uint32)
    return out


def diag_tdt_decide(sc, logits, hn, cn, st, pad_rows=3, guard=32):
    """pk_diag_tdt_decide (include/parakeet_amd.h): logits [n_steps][B F][V + D], hn / cn [n_steps][L][B][Hp] (hn uint16 bf16 words when sc["h_bf16"]).
    sc: the scalars of the struct (durations a list).  st: the batch's state, arrays with B leading rows -- t, steps, n_out, nsym, done, token, lens, ids, start,
    end, conf, h, c and done_count; optional margin; need + pp + ep + z (z natural columns, [B F][J] fp32 or [B][J] uint16); Tb, row0; trie = (off, tok, node,
    boost) + act + n_act; force = (label, dur, n_force, n_force_b, stride) + score_lab / score_dur.  Returns the WHOLE buffers after the last launch: the per-row
    arrays pad_rows pattern-filled rows longer than the batch, h / c / z as flat uint32 words with `guard` pattern words behind them (z: fp32 words back in
    natural order), and "form"."""
    B, F, J = sc["B"], max(1, sc.get("F", 1)), sc.get("J", 0)
    logits, cn = _c(logits), _c(cn)
    hn = np.ascontiguousarray(hn, np.uint16 if sc.get("h_bf16") else np.float32)
    d = PkTdtDecideDiag()
    for k in ("B", "T", "V", "D", "L", "Hp", "blank", "max_symbols", "max_tokens", "max_steps", "keep_state", "h_bf16", "F", "J"):
        setattr(d, k, int(sc.get(k, 0)))
    d.F = F
    for i, v in enumerate(sc.get("durations", [])):
        if i < 8:
            d.durations[i] = int(v)
    d.n_steps, d.rows = logits.shape[0], B + pad_rows
    keep = [logits, hn, cn]
    out = {}

    def io(name, dt, lead=B):
        a = _padded(np.asarray(st[name]), lead, dt, pad_rows)
        out[name] = a
        return a.ctypes.data_as(f32p if dt == np.float32 else i32p)

    def ro(a, dt=np.int32):
        a = _c(a, dt)
        keep.append(a)
        return a.ctypes.data_as(f32p if dt == np.float32 else i32p)

    d.logits, d.hn, d.cn = _f(logits), hn.ctypes.data_as(C.c_void_p), _f(cn)
    for k in ("t", "steps", "n_out", "nsym", "done", "token", "lens", "ids", "start", "end"):
        setattr(d, k, io(k, np.int32))
    d.conf = io("conf", np.float32)
    out["done_count"] = np.asarray([st["done_count"]], np.int32)
    d.done_count = _i(out["done_count"])
    out["h"], out["c"] = _flat_guard(st["h"], guard), _flat_guard(st["c"], guard)
    d.h, d.c, d.h_words, d.c_words = out["h"].ctypes.data_as(C.c_void_p), out["c"].ctypes.data_as(f32p), out["h"].size, out["c"].size
    if st.get("margin") is not None:
        d.margin = io("margin", np.float32)
    if st.get("need") is not None:
        d.need = io("need", np.int32)
        ep = _c(st["ep"]).reshape(-1, J)
        d.pp, d.ep, d.ep_rows = ro(st["pp"], np.float32), ro(ep, np.float32), ep.shape[0]
        z = np.ascontiguousarray(st["z"])
        if not sc.get("h_bf16"):
            z = np.ascontiguousarray(z.reshape(B * F, J)[:, sigma16(J)])
        out["z"] = _flat_guard(z, guard)
        d.z, d.z_words = out["z"].ctypes.data_as(C.c_void_p), out["z"].size
    if st.get("Tb") is not None:
        d.Tb = ro(st["Tb"])
    if st.get("row0") is not None:
        d.row0 = ro(st["row0"])
    if st.get("trie") is not None:
        off, tok, node, boost = st["trie"]
        d.trie_off, d.trie_tok, d.trie_node = ro(off), ro(tok if len(tok) else [0]), ro(node if len(node) else [0])
        d.trie_nodes, d.boost = len(off) - 1, float(boost)
        d.act, d.n_act = io("act", np.int32), io("n_act", np.int32)
    if st.get("force") is not None:
        lab, dur, n_force, n_force_b, stride = st["force"]
        d.force_label, d.force_dur, d.force_len, d.n_force, d.force_stride = ro(lab), ro(dur), len(lab), int(n_force), int(stride)
        if n_force_b is not None:
            d.n_force_b = ro(n_force_b)
        for k in ("score_lab", "score_dur"):
            if st.get(k) is not None:
                out[k] = np.ascontiguousarray(st[k], np.float32).copy()
                setattr(d, k, _f(out[k]))
                d.score_rows = out[k].shape[0]
    form = C.c_int(-1)
    check(lib().pk_diag_tdt_decide(C.byref(d), C.byref(form)))
    if "z" in out and not sc.get("h_bf16"):
        body = out["z"][: B * F * J].reshape(B * F, J)[:, sigma16(J)]
        out["z"] = np.concatenate([body.reshape(-1), out["z"][B * F * J:]])
    out["form"] = form.value
    return out


class PkTdtBeamStepDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("B", "W", "K", "Kd", "N", "V", "D", "blank", "max_tokens")]
                + [("durations", C.c_int32 * 8)] + [(k, C.c_int32) for k in ("step", "init", "trace", "rows", "cap")]
                + [("T", i32p), ("logits", f32p)]
                + [(k, i32p) for k in ("valid", "t", "len", "par", "born", "tok")] + [("score", f32p), ("hash", C.POINTER(C.c_uint64)), ("prefix", i32p)]
                + [(k, i32p) for k in ("live", "steps_done", "live_total", "bp")]
                + [("lab_id", i32p), ("lab_lp", f32p), ("dur_i", i32p), ("dur_lp", f32p), ("cand", f32p)]
                + [("lm", C.c_void_p), ("alpha", C.c_float), ("beta", C.c_float), ("lmstate", i32p), ("lmv", f32p), ("lab_ls", i32p), ("lab_lm", f32p)]
                + [("ids", i32p), ("start", i32p), ("end", i32p), ("dur_idx", i32p), ("conf", f32p), ("lens", i32p), ("out_score", f32p), ("ok", i32p),
                   ("out_lm", f32p)])


_LATE_SIGNATURES["pk_diag_tdt_beam_step"] = [C.POINTER(PkTdtBeamStepDiag)]


TDT_BEAM_STEP_SCALARS = ("B", "W", "K", "Kd", "N", "V", "D", "blank", "max_tokens")


def tdt_beam_step_state(sc, T, cap, fused=False, pad_rows=3):
    """The arrays of pk_diag_tdt_beam_step for a search that has not begun, every one filled with the pattern SKINNY_FILL32 except live_total (zeros: the
    search's host zeroes it) and the back-trace's token arrays (zeros, likewise).  sc: the scalars B, W, K, Kd, N, V, D, blank, max_tokens and durations; T [B]
    frames per clip; cap: the steps bp / live_total hold.  The intermediates have pad_rows rows more than the beam."""
    B, W, K, Kd, N, MT = (int(sc[k]) for k in ("B", "W", "K", "Kd", "N", "max_tokens"))
    R, rows = B * W, B * W + pad_rows
    fill = lambda shape, dt: np.full(shape, SKINNY_FILL32, np.uint32).view(dt)
    st = dict(T=_c(T, np.int32), cap=int(cap), rows=rows, fused=bool(fused))
    for k in ("valid", "t", "len", "par", "born", "tok"):
        st[k] = fill((2, R), np.int32)
    st["score"], st["prefix"] = fill((2, R), np.float32), fill((2, R, MT), np.int32)
    st["hash"] = np.full((2, R), (SKINNY_FILL32 << 32) | SKINNY_FILL32, np.uint64)
    st["live"], st["steps_done"], st["live_total"], st["bp"] = fill(B, np.int32), fill(B, np.int32), np.zeros(cap + 1, np.int32), fill((cap, R, 4), np.int32)
    st["lab_id"], st["lab_lp"] = fill((rows, K + 1), np.int32), fill((rows, K + 1), np.float32)
    st["dur_i"], st["dur_lp"], st["cand"] = fill((rows, Kd), np.int32), fill((rows, Kd), np.float32), fill((rows, (K + 1) * Kd), np.float32)
    if fused:
        st["lmstate"], st["lmv"] = fill((2, R), np.int32), fill((2, R), np.float32)
        st["lab_ls"], st["lab_lm"] = fill((rows, K + 1), np.int32), fill((rows, K + 1), np.float32)
    for k in ("ids", "start", "end", "dur_idx"):
        st[k] = np.zeros((B, N, MT), np.int32)
    st["conf"] = np.zeros((B, N, MT), np.float32)
    st["lens"], st["out_score"], st["ok"], st["out_lm"] = fill((B, N), np.int32), fill((B, N), np.float32), fill(B, np.int32), fill((B, N), np.float32)
    return st


TDT_BEAM_STEP_SCRATCH = ("lab_id", "lab_lp", "dur_i", "dur_lp", "cand", "lab_ls", "lab_lm")


def diag_tdt_beam_step(sc, st, logits, step, init=False, trace=False, lm=None, alpha=0.0, beta=0.0):
    """pk_diag_tdt_beam_step (include/parakeet_amd.h) on the arrays of tdt_beam_step_state, CHANGED IN PLACE: (init,) expand + prune of `step` on the rows
    logits [B W][V + D], (the back-trace).  The step's intermediates are refilled with the pattern before the call, so what comes back is this step's."""
    logits = _c(logits)
    d = PkTdtBeamStepDiag()
    for k in TDT_BEAM_STEP_SCALARS:
        setattr(d, k, int(sc[k]))
    for i, v in enumerate(list(sc["durations"])[:8]):
        d.durations[i] = int(v)
    R = d.B * d.W
    assert logits.shape == (R, d.V + d.D), (logits.shape, R, d.V + d.D)
    d.step, d.init, d.trace, d.rows, d.cap = int(step), int(bool(init)), int(bool(trace)), int(st["rows"]), int(st["cap"])
    for k in TDT_BEAM_STEP_SCRATCH:
        if k in st:
            st[k].view(np.uint32)[...] = SKINNY_FILL32
    d.T, d.logits = _i(st["T"]), _f(logits)
    for k, ty in PkTdtBeamStepDiag._fields_:                       # every in / out array the state holds
        a = st.get(k)
        if k in ("T", "logits", "lm") or not isinstance(a, np.ndarray) or (lm is None and k == "out_lm"):
            continue
        assert a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"], k
        setattr(d, k, a.ctypes.data_as(ty))
    if lm is not None:
        d.lm, d.alpha, d.beta = lm._h, float(alpha), float(beta)
    check(lib().pk_diag_tdt_beam_step(C.byref(d)))
    return st


def diag_ctc_greedy(logits, n, blank, B=None, T=0, n_frames=None, pitch=None, trie=None, pad_rows=3):
    """pk_diag_ctc_greedy: logits [frames][ld] (the first n columns of a row are its values).  Uniform batch: B x T frames; ragged: n_frames [B], packed.
    trie = (off, tok, node, boost): the boosted kernel instead of the collapse.  Returns the whole pattern-filled buffers: lp [frames + pad][n], best_idx /
    best_lp (the launch with log-prob rows) and best_idx2 / best_lp2 (without) [frames + pad], ids / start / end / conf [B + pad][pitch], lens [B + pad]."""
    logits = _c(logits)
    frames, ld = logits.shape
    nf = _c(n_frames, np.int32) if n_frames is not None else None
    B = len(nf) if nf is not None else B
    tmax = int(nf.max()) if nf is not None else T
    pitch = pitch or tmax
    fill = lambda shape, dt: np.full(shape, SKINNY_FILL32, np.uint32).view(dt)
    o = dict(lp=fill((frames + pad_rows, n), np.float32), best_idx=fill(frames + pad_rows, np.int32), best_lp=fill(frames + pad_rows, np.float32),
             best_idx2=fill(frames + pad_rows, np.int32), best_lp2=fill(frames + pad_rows, np.float32), lens=fill(B + pad_rows, np.int32),
             ids=fill((B + pad_rows, pitch), np.int32), start=fill((B + pad_rows, pitch), np.int32), end=fill((B + pad_rows, pitch), np.int32),
             conf=fill((B + pad_rows, pitch), np.float32))
    d = PkCtcGreedyDiag()
    d.B, d.T, d.n, d.ld, d.blank, d.pitch, d.out_rows, d.lp_rows = B, int(T), n, ld, blank, pitch, B + pad_rows, frames + pad_rows
    d.n_frames = _i(nf) if nf is not None else None
    d.logits = _f(logits)
    for k, a in o.items():
        setattr(d, k, a.ctypes.data_as(f32p if a.dtype == np.float32 else i32p))
    keep = []
    if trie is not None:
        off, tok, node, boost = trie
        keep = [_c(off, np.int32), _c(tok if len(tok) else [0], np.int32), _c(node if len(node) else [0], np.int32)]
        d.trie_off, d.trie_tok, d.trie_node, d.trie_nodes, d.boost = _i(keep[0]), _i(keep[1]), _i(keep[2]), len(off) - 1, float(boost)
    check(lib().pk_diag_ctc_greedy(C.byref(d)))
    return o


def diag_pred_cache(on):
    """pk_diag_pred_cache: prediction-net caching of the per-phase decode loop on / off (test switch, process-wide, default on)."""
    check(lib().pk_diag_pred_cache(int(on)))


def diag_ffn_bf16_smallm(x, gamma, beta, W1, b1, W2, b2, act_tiles, eps=1e-5):
    """pk_diag_ffn_bf16_smallm: x + 0.5 * ffn(LN(x)) of a streaming chunk on the small-M bf16 kernel; act_tiles = fc1 activations in 8-row operand tiles."""
    x, gamma, beta, W1, b1, W2, b2 = (_c(v) for v in (x, gamma, beta, W1, b1, W2, b2))
    M, d = x.shape
    f = W1.shape[0]
    out = np.empty((M, d), np.float32)
    check(lib().pk_diag_ffn_bf16_smallm(M, d, f, _f(x), _f(gamma), _f(beta), eps, _f(W1), _f(b1), _f(W2), _f(b2), int(act_tiles), _f(out)))
    return out


def diag_glu_dwconv_bf16(A, W, bias, cache_in, has_cache, dw_w, dw_bias, bn_mean, bn_rstd, bn_g, bn_b, c, fused, gamma=None, beta=None, eps=1e-5):
    """pk_diag_glu_dwconv_bf16: pw1 (GLU) + causal depthwise conv + BatchNorm + SiLU of a streaming chunk; fused = the conv in the product's epilogue."""
    A, W, bias, cache_in = _c(A), _c(W), _c(bias), _c(cache_in)
    M, d = A.shape
    S = M // c
    ps = [_c(v) for v in (dw_w, dw_bias, bn_mean, bn_rstd, bn_g, bn_b)]
    g, b = (_c(gamma), _c(beta)) if gamma is not None else (None, None)
    out = np.empty((M, d), np.float32); cache_out = np.empty((S, 8, d), np.float32)
    check(lib().pk_diag_glu_dwconv_bf16(S, c, d, _f(A), _f(g) if g is not None else None, _f(b) if b is not None else None, eps, _f(W), _f(bias), _f(cache_in),
                                        int(has_cache), *[_f(v) for v in ps], int(fused), _f(out), _f(cache_out)))
    return out, cache_out


class Stream:
    """pk_stream_*: n lock-step streaming sessions on the GPU (reference NemotronTranscriber::transcribe_chunk)."""

    def __init__(self, model, n_streams, att_context_left=70, att_context_right=0):
        L = lib()
        L.pk_stream_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.pk_stream_free.argtypes = [C.c_void_p]
        L.pk_stream_free.restype = None
        L.pk_stream_reset.argtypes = [C.c_void_p]
        L.pk_stream_push.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p]
        L.pk_stream_mel.argtypes = [C.c_void_p, f32p, C.c_int, f32p, C.c_int, C.POINTER(C.c_int)]
        L.pk_stream_encode.argtypes = [C.c_void_p, f32p, C.c_int, f32p, C.c_int, C.POINTER(C.c_int)]
        L.pk_stream_decode.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, i32p, i32p, i32p, i32p, f32p]
        self.model, self.S = model, n_streams
        self.n_kw = 0
        self._h = C.c_void_p()
        check(L.pk_stream_create(model._h, n_streams, att_context_left, att_context_right, C.byref(self._h)))

    def _tok(self, fn, x, n, mt):
        ids = np.zeros((self.S, mt), np.int32); st = np.zeros((self.S, mt), np.int32); en = np.zeros((self.S, mt), np.int32)
        cf = np.zeros((self.S, mt), np.float32); lens = np.zeros(self.S, np.int32)
        check(fn(self._h, _f(x), n, mt, _i(ids), _i(lens), _i(st), _i(en), _f(cf)))
        return dict(ids=ids, lens=lens, start=st, end=en, conf=cf)

    def push(self, pcm, max_tokens=64):
        pcm = _c(pcm)
        assert pcm.shape[0] == self.S
        return self._tok(lib().pk_stream_push, pcm, pcm.shape[1], max_tokens)

    def mel(self, pcm):
        pcm = _c(pcm)
        cap = pcm.shape[1] // 160 + 8
        out = np.zeros((self.S, cap, self.model.cfg.mel_bins), np.float32)
        n = C.c_int(0)
        check(lib().pk_stream_mel(self._h, _f(pcm), pcm.shape[1], _f(out), cap, C.byref(n)))
        return np.ascontiguousarray(out.reshape(-1)[: self.S * n.value * self.model.cfg.mel_bins].reshape(self.S, n.value, -1))

    def encode(self, mel):
        mel = _c(mel)
        cap = mel.shape[1] // 8 + 2
        out = np.zeros((self.S, cap, self.model.cfg.hidden_size), np.float32)
        n = C.c_int(0)
        check(lib().pk_stream_encode(self._h, _f(mel), mel.shape[1], _f(out), cap, C.byref(n)))
        d = self.model.cfg.hidden_size
        return np.ascontiguousarray(out.reshape(-1)[: self.S * n.value * d].reshape(self.S, n.value, d))

    def decode(self, enc, max_tokens=64):
        enc = _c(enc)
        return self._tok(lib().pk_stream_decode, enc, enc.shape[1], max_tokens)

    def score(self, enc, labels, dur_idx, n_steps, rows=True):
        """pk_stream_score: every stream walks its GIVEN decisions labels[s][:n_steps[s]] / dur_idx[s][...] on this chunk's enc[S][c][d];
        -> label_lp [S][cap][V] (rows=True), dur_lp [S][cap][D], n [S] steps walked."""
        enc = _c(enc)
        labels = _c(labels, np.int32); dur_idx = _c(dur_idx, np.int32); n_steps = _c(n_steps, np.int32)
        assert enc.shape[0] == self.S and labels.shape == dur_idx.shape and labels.shape[0] == self.S and n_steps.shape == (self.S,)
        cap = labels.shape[1]
        cfg = self.model.cfg
        V, D = cfg.vocab_size, len(cfg.durations)
        L = lib()
        L.pk_stream_score.argtypes = [C.c_void_p, f32p, C.c_int, i32p, i32p, i32p, C.c_int, f32p, f32p, i32p]
        llp = np.zeros((self.S, cap, V), np.float32) if rows else None
        dlp = np.zeros((self.S, cap, D), np.float32)
        nd = np.zeros(self.S, np.int32)
        check(L.pk_stream_score(self._h, _f(enc), enc.shape[1], _i(labels), _i(dur_idx), _i(n_steps), cap, _f(llp) if rows else None, _f(dlp), _i(nd)))
        return dict(label_lp=llp, dur_lp=dlp, n=nd)

    def set_keywords(self, phrases=None, ids=None, min_score=None, patience=None):
        """pk_stream_set_keywords: phrases (needs the model's vocabulary) or ids (a list of token sequences); neither, or an empty list, clears
        the set.  Every keyword is watched in every stream: pair = stream * n_kw + keyword."""
        o = stream_kws_options(min_score, patience)
        if phrases:
            arr = (C.c_char_p * len(phrases))(*[p.encode() for p in phrases])
            check(lib().pk_stream_set_keywords(self._h, arr, None, None, len(phrases), C.byref(o)))
            self.n_kw = len(phrases)
        elif ids:
            pid, off = _pack_ids(ids)
            check(lib().pk_stream_set_keywords(self._h, None, _i(pid), _i(off), len(ids), C.byref(o)))
            self.n_kw = len(ids)
        else:
            check(lib().pk_stream_set_keywords(self._h, None, None, None, 0, C.byref(o)))
            self.n_kw = 0

    def spot(self, enc, rows=False):
        """pk_stream_spot: the stage form on this chunk's enc [S][c][d] -> dict(events [(stream, keyword, start, end, score)...], n_events and,
        with rows, E / Bs / Ee [S * n_kw][c])."""
        enc = _c(enc)
        c, P = enc.shape[1], self.S * self.n_kw
        cap = P * max(c, 1)
        ev = (PkKwsEvent * max(cap, 1))()
        n = C.c_int(0)
        E = np.zeros((P, max(c, 1)), np.float32); Bs = np.zeros((P, max(c, 1)), np.int32); Ee = np.zeros((P, max(c, 1)), np.int32)
        check(lib().pk_stream_spot(self._h, _f(enc), c, _f(E) if rows else None, _i(Bs) if rows else None, _i(Ee) if rows else None, ev, cap, C.byref(n)))
        out = dict(events=_events(ev, n.value), n_events=n.value)
        if rows:
            out.update(E=E, Bs=Bs, Ee=Ee)
        return out

    def push_spot(self, pcm, max_tokens=64):
        """pk_stream_push_spot: push() that also walks the chunk's frames -> push()'s dict with events / n_events."""
        pcm = _c(pcm)
        assert pcm.shape[0] == self.S
        mt = max_tokens
        ids = np.zeros((self.S, mt), np.int32); st = np.zeros((self.S, mt), np.int32); en = np.zeros((self.S, mt), np.int32)
        cf = np.zeros((self.S, mt), np.float32); lens = np.zeros(self.S, np.int32)
        cap = self.S * self.n_kw * KWS_CHUNK_MAX
        ev = (PkKwsEvent * max(cap, 1))()
        n = C.c_int(0)
        check(lib().pk_stream_push_spot(self._h, _f(pcm), pcm.shape[1], mt, _i(ids), _i(lens), _i(st), _i(en), _f(cf), ev, cap, C.byref(n)))
        return dict(ids=ids, lens=lens, start=st, end=en, conf=cf, events=_events(ev, n.value), n_events=n.value)

    def spot_flush(self):
        cap = self.S * self.n_kw
        ev = (PkKwsEvent * max(cap, 1))()
        n = C.c_int(0)
        check(lib().pk_stream_spot_flush(self._h, ev, cap, C.byref(n)))
        return _events(ev, n.value)

    def spot_timed(self, enc, reps=3):
        """pk_stream_spot_timed -> (enc_proj + lattice ms, walk + rule ms), HIP events, medians of reps passes."""
        enc = _c(enc)
        ms = np.zeros(2, np.float32)
        check(lib().pk_stream_spot_timed(self._h, _f(enc), enc.shape[1], reps, _f(ms)))
        return float(ms[0]), float(ms[1])

    def set_endpointing(self, enable=True, **options):
        """pk_stream_set_endpointing: the library's defaults with the given pk_endpoint_options fields replaced; enable=False clears it."""
        if not enable:
            check(lib().pk_stream_set_endpointing(self._h, None))
            return
        o = endpoint_options(**options)
        check(lib().pk_stream_set_endpointing(self._h, C.byref(o)))

    def endpoint(self, mel, want_rows=False):
        """pk_stream_endpoint: the stage form on this chunk's mel rows [S][n][F] -> dict(events [(stream, kind, reason, start, end, at)...], n_events
        and, with want_rows, level / floor / speech0 [S][n])."""
        mel = _c(mel)
        n = mel.shape[1]
        cap = self.S * max(n, 1)
        ev = (PkEndpointEvent * cap)()
        ne = C.c_int(0)
        lv = np.zeros((self.S, max(n, 1)), np.float32); fl = np.zeros((self.S, max(n, 1)), np.float32); sp = np.zeros((self.S, max(n, 1)), np.int32)
        check(lib().pk_stream_endpoint(self._h, _f(mel), n, _f(lv) if want_rows else None, _f(fl) if want_rows else None,
                                       _i(sp) if want_rows else None, ev, cap, C.byref(ne)))
        out = dict(events=_ep_events(ev, ne.value), n_events=ne.value)
        if want_rows:
            out.update(level=lv, floor=fl, speech0=sp)
        return out

    def push_endpoint(self, pcm, max_tokens=64, spot=False):
        """pk_stream_push_endpoint: push() that also feeds the endpointer -> push()'s dict with events / n_events (the endpoint events) and, with
        spot, kws_events / kws_n_events (what push_spot returns as events)."""
        pcm = _c(pcm)
        assert pcm.shape[0] == self.S
        mt = max_tokens
        ids = np.zeros((self.S, mt), np.int32); st = np.zeros((self.S, mt), np.int32); en = np.zeros((self.S, mt), np.int32)
        cf = np.zeros((self.S, mt), np.float32); lens = np.zeros(self.S, np.int32)
        cap = self.S * (ENDPOINT_MAX_FRAMES + 1)
        ev = (PkEndpointEvent * cap)()
        ne = C.c_int(0)
        kcap = self.S * self.n_kw * KWS_CHUNK_MAX
        kev = (PkKwsEvent * max(kcap, 1))()
        kn = C.c_int(0)
        check(lib().pk_stream_push_endpoint(self._h, _f(pcm), pcm.shape[1], mt, _i(ids), _i(lens), _i(st), _i(en), _f(cf), ev, cap, C.byref(ne),
                                            kev if spot else None, kcap if spot else 0, C.byref(kn) if spot else None))
        out = dict(ids=ids, lens=lens, start=st, end=en, conf=cf, events=_ep_events(ev, ne.value), n_events=ne.value)
        if spot:
            out.update(kws_events=_events(kev, kn.value), kws_n_events=kn.value)
        return out

    def reset_decoder(self, mask):
        """pk_stream_reset_decoder: the prediction-net state of the streams with mask[s] set becomes what reset() gives it; nothing else is touched."""
        m, p = _mask(mask, self.S)
        check(lib().pk_stream_reset_decoder(self._h, p))

    def endpoint_timed(self, mel, reps=3):
        """pk_stream_endpoint_timed -> the chunk kernel's ms, HIP events, median of reps passes."""
        mel = _c(mel)
        ms = np.zeros(1, np.float32)
        check(lib().pk_stream_endpoint_timed(self._h, _f(mel), mel.shape[1], reps, _f(ms)))
        return float(ms[0])

    def reset(self):
        check(lib().pk_stream_reset(self._h))

    def close(self):
        if self._h:
            lib().pk_stream_free(self._h)
            self._h = None


class Transformer:
    """pk_transformer_*: TransformerEncoder of the reference (src/transformer.cpp) on the GPU."""

    def __init__(self, weights_path, prefix, hidden_size, num_layers, num_heads, ffn_intermediate, pre_ln=True, has_final_norm=False,
                 layer_norm_eps=1e-5, device=0):
        L = lib()
        L.pk_transformer_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PkTransformerConfig), C.c_int, C.POINTER(C.c_void_p)]
        L.pk_transformer_forward.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, f32p]
        L.pk_transformer_free.argtypes = [C.c_void_p]
        L.pk_transformer_free.restype = None
        c = PkTransformerConfig(hidden_size, num_layers, num_heads, ffn_intermediate, int(pre_ln), int(has_final_norm), layer_norm_eps)
        self._h = C.c_void_p()
        check(L.pk_transformer_load(weights_path.encode(), prefix.encode(), C.byref(c), device, C.byref(self._h)))

    def forward(self, x):
        x = _c(x)
        B, T, _ = x.shape
        y = np.empty_like(x)
        check(lib().pk_transformer_forward(self._h, _f(x), B, T, _f(y)))
        return y

    def close(self):
        if self._h:
            lib().pk_transformer_free(self._h)
            self._h = None


class Sortformer:
    """pk_sortformer_*: Sortformer diarization (reference include/parakeet/sortformer.hpp:99-129) on the GPU."""

    def __init__(self, weights_path, sf, device=0):
        L = lib()
        L.pk_sortformer_load.argtypes = [C.c_char_p, C.POINTER(PkSortformerConfig), C.c_int, C.POINTER(C.c_void_p)]
        L.pk_sortformer_free.argtypes = [C.c_void_p]
        L.pk_sortformer_free.restype = None
        L.pk_sortformer_forward.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, f32p, C.POINTER(C.c_int)]
        L.pk_sortformer_forward_pcm.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64, f32p, C.POINTER(C.c_int)]
        L.pk_sortformer_segments.argtypes = [f32p, C.c_int, C.c_int, C.c_float, i32p, f32p, f32p, C.c_int]
        self.sf = sf
        c = PkSortformerConfig()
        c.nest = to_pk_config(sf.nest_encoder)
        c.transformer = PkTransformerConfig(sf.transformer_hidden, sf.transformer_layers, sf.transformer_heads, sf.transformer_ffn,
                                            int(sf.pre_ln), int(sf.has_final_norm), 1e-5)
        c.max_speakers, c.activity_threshold = sf.max_speakers, sf.activity_threshold
        c.att_context_left, c.att_context_right = sf.att_context_left, sf.att_context_right
        L.pk_sortformer_diarize_chunk.argtypes = [C.c_void_p, f32p, C.c_int, f32p, C.c_int, C.POINTER(C.c_int)]
        L.pk_sortformer_stream_reset.argtypes = [C.c_void_p]
        self._h = C.c_void_p()
        check(L.pk_sortformer_load(weights_path.encode(), C.byref(c), device, C.byref(self._h)))

    def forward(self, feats):
        """Sortformer::forward: feats [B][Tm][mel] -> probs [B][T][S]."""
        feats = _c(feats)
        B, Tm, _ = feats.shape
        T = lib().pk_encoder_num_frames(Tm)
        probs = np.zeros((B, T, self.sf.max_speakers), np.float32)
        check(lib().pk_sortformer_forward(self._h, _f(feats), B, Tm, _f(probs), None))
        return probs

    def diarize_chunk(self, feats):
        """Sortformer::diarize_chunk on feats [n_frames][mel]: -> probs [c][S] of this chunk (c may be 0)."""
        feats = _c(feats)
        cap = feats.shape[0] // 8 + 4
        probs = np.zeros((cap, self.sf.max_speakers), np.float32)
        n = C.c_int(0)
        check(lib().pk_sortformer_diarize_chunk(self._h, _f(feats), feats.shape[0], _f(probs), cap, C.byref(n)))
        return probs[:n.value]

    def reset_stream(self):
        check(lib().pk_sortformer_stream_reset(self._h))

    def forward_pcm(self, pcm):
        pcm = _c(pcm)
        if pcm.ndim == 1:
            pcm = pcm[None]
        B, n = pcm.shape
        T = lib().pk_encoder_num_frames(lib().pk_mel_num_frames(n))
        probs = np.zeros((B, T, self.sf.max_speakers), np.float32)
        check(lib().pk_sortformer_forward_pcm(self._h, _f(pcm), B, n, _f(probs), None))
        return probs

    def close(self):
        if self._h:
            lib().pk_sortformer_free(self._h)
            self._h = None


def sortformer_segments(probs, threshold=0.5):
    """Sortformer::probs_to_segments on probs [T][S] -> list of (speaker, start_s, end_s)."""
    L = lib()
    L.pk_sortformer_segments.argtypes = [f32p, C.c_int, C.c_int, C.c_float, i32p, f32p, f32p, C.c_int]
    probs = _c(probs)
    T, S = probs.shape
    cap = S * (T // 2 + 2)
    spk = np.zeros(cap, np.int32); a = np.zeros(cap, np.float32); b = np.zeros(cap, np.float32)
    n = L.pk_sortformer_segments(_f(probs), T, S, threshold, _i(spk), _f(a), _f(b), cap)
    return [(int(spk[i]), float(a[i]), float(b[i])) for i in range(n)]


class Frontend:
    """pk_frontend_*: preprocess_audio without a model (reference src/audio.cpp:100-158)."""

    def __init__(self, n_mels=80, normalize=True, window_centered=False, device=0):
        L = lib()
        L.pk_frontend_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.pk_frontend_features.argtypes = [C.c_void_p, f32p, C.c_int64, f32p, C.POINTER(C.c_int)]
        L.pk_frontend_free.argtypes = [C.c_void_p]
        L.pk_frontend_free.restype = None
        self.n_mels = n_mels
        self._h = C.c_void_p()
        check(L.pk_frontend_create(n_mels, int(normalize), int(window_centered), device, C.byref(self._h)))

    def features(self, pcm):
        pcm = _c(pcm).ravel()
        nf = lib().pk_mel_num_frames(pcm.size)
        out = np.zeros((nf, self.n_mels), np.float32)
        check(lib().pk_frontend_features(self._h, _f(pcm), pcm.size, _f(out), None))
        return out

    def close(self):
        if self._h:
            lib().pk_frontend_free(self._h)
            self._h = None


def read_audio_memory(data: bytes, target_rate=16000):
    """read_audio(const uint8_t*, size_t, target) -> (mono pcm at target_rate, original rate, channels)."""
    L = lib()
    L.pk_read_audio_memory.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(f32p), i64p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    p = f32p(); n = C.c_int64(0); sr = C.c_int(0); ch = C.c_int(0)
    check(L.pk_read_audio_memory(data, len(data), target_rate, C.byref(p), C.byref(n), C.byref(sr), C.byref(ch)))
    out = np.ctypeslib.as_array(p, shape=(max(1, n.value),))[:n.value].copy()
    L.pk_free(p)
    return out, sr.value, ch.value


def audio_info(path):
    """get_audio_duration's header walk -> (sample_rate, channels, frames)."""
    L = lib()
    L.pk_audio_info.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), i64p]
    sr = C.c_int(0); ch = C.c_int(0); n = C.c_int64(0)
    check(L.pk_audio_info(path.encode(), C.byref(sr), C.byref(ch), C.byref(n)))
    return sr.value, ch.value, n.value


def diag_layernorm(x, g, b, eps=1e-5):
    x, g, b = _c(x), _c(g), _c(b)
    y = np.empty_like(x)
    check(lib().pk_diag_layernorm(_f(x), x.size // x.shape[-1], x.shape[-1], _f(g), _f(b), eps, _f(y)))
    return y


def diag_ln_gemm(A, gamma, beta, W, bias=None, epi="none", fold=True, pre_gamma=None, pre_beta=None, eps=1e-5):
    """out = epi(LN(X) W^T + bias) on a large fp32 batch, X = A or LN(A; pre_gamma, pre_beta); fold: the statistics pass + the tile GEMM that normalises
    while staging A (what the engine runs), else LayerNorm launch + GEMM.  Returns (out, X or None)."""
    A, W, gamma, beta = _c(A), _c(W), _c(gamma), _c(beta)
    M, K = A.shape
    e = EPI[epi]
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    out = np.empty((M, N), np.float32)
    y1 = np.empty((M, K), np.float32) if pre_gamma is not None else None
    pg = _c(pre_gamma) if pre_gamma is not None else None
    pb = _c(pre_beta) if pre_beta is not None else None
    bb = _c(bias) if bias is not None else None
    check(lib().pk_diag_ln_gemm(M, N, K, _f(A), _f(pg) if pg is not None else None, _f(pb) if pb is not None else None, _f(gamma), _f(beta), eps, _f(W),
                                _f(bb) if bb is not None else None, e, 1 if fold else 0, _f(out), _f(y1) if y1 is not None else None))
    return out, y1


def diag_sum64(x):
    x = _c(x)
    out = np.empty(x.shape[0], np.float32)
    check(lib().pk_diag_sum64(_f(x), x.shape[0], x.shape[1], _f(out)))
    return out


def diag_relpos_local_attention(qkv, pos, bias_u, bias_v, n_heads, left, right, B=1, lens=None, out_mode=0):
    """pk_diag_relpos_local_attention: one limited-context attention layer on the band kernel.  qkv [rows][3 d] as for
    diag_relpos_attention, pos the LOCAL table [left + right + 1][d] (row r: position i - j = left - r), out_mode 0 fp32 / 1 bf16 ctx ->
    (ctx [rows + ATT_GUARD_ROWS][d] fp32 with the guard rows, variant bits: 2 ragged, 8 band kernel, 16 bf16 output)."""
    qkv, pos, bu, bv = _c(qkv), _c(pos), _c(bias_u), _c(bias_v)
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    assert qkv.shape[1] == 3 * d and pos.shape[1] == d and bu.shape == (d,) and bv.shape == (d,)
    if lens is not None:
        ln = np.ascontiguousarray(lens, np.int32)
        assert int(ln.sum()) == rows
        B, T, lp = len(ln), int(ln.max()), _i(ln)
    else:
        assert rows % B == 0
        T, lp = rows // B, None
    out = np.empty((rows + ATT_GUARD_ROWS, d), np.float32)
    var = C.c_int(-1)
    check(lib().pk_diag_relpos_local_attention(B, lp, T, d, n_heads, _f(qkv), _f(pos), int(left), int(right), _f(bu), _f(bv), int(out_mode),
                                               _f(out), C.byref(var)))
    return out, var.value


CONV_VARIANT_WORDS = 17                  # PK_DIAG_CONV_VARIANT_WORDS


def diag_conv_instantiations():
    """pk_diag_conv_instantiations: every instantiation of the conv1 + dw1, dw2, conv-module and streaming-conv launchers, as the tuples
    Model.conv_variants reports."""
    n = lib().pk_diag_conv_instantiations(None, 0)
    out = np.zeros((n, 5), np.int32)
    lib().pk_diag_conv_instantiations(_i(out), n)
    return [tuple(int(x) for x in row) for row in out]


ATT_GUARD_ROWS = 128                     # PK_DIAG_ATTENTION_GUARD_ROWS
ATT_UNWRITTEN = {"fp32": 0x7FC5A5A5, "bf16": 0x7FC50000}   # bit pattern of an element the kernel did not write


def diag_relpos_attention(kernel, qkv, pos, bias_u, bias_v, n_heads, B=1, lens=None):
    """pk_diag_relpos_attention: one relative-position attention layer on the production kernel ("fp32" or "bf16").
    qkv [rows][3 d] (rows = B T, or sum(lens) for a packed ragged batch), pos [2 pos_T - 1][d] -> (ctx [rows + ATT_GUARD_ROWS][d] fp32 with the
    guard rows, variant bits: 1 global scratch, 2 ragged, 4 bf16)."""
    qkv, pos, bu, bv = _c(qkv), _c(pos), _c(bias_u), _c(bias_v)
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    pos_T = (pos.shape[0] + 1) // 2
    assert qkv.shape[1] == 3 * d and pos.shape == (2 * pos_T - 1, d) and bu.shape == (d,) and bv.shape == (d,)
    if lens is not None:
        ln = np.ascontiguousarray(lens, np.int32)
        assert int(ln.sum()) == rows
        B, T, lp = len(ln), int(ln.max()), _i(ln)
    else:
        assert rows % B == 0
        T, lp = rows // B, None
    out = np.empty((rows + ATT_GUARD_ROWS, d), np.float32)
    var = C.c_int(-1)
    check(lib().pk_diag_relpos_attention({"fp32": 0, "bf16": 1}[kernel], B, lp, T, d, n_heads, _f(qkv), _f(pos), pos_T, _f(bu), _f(bv), _f(out),
                                         C.byref(var)))
    return out, var.value


ATT_FORMS = {"default": 0, "block": 1, "strip": 2}          # kernels.hpp ATT_FORM_*
ATT_OUT_MODES = {"fp32": 0, "bf16": 1, "sigma": 2}


def diag_relpos_attention_form(form, qkv, pos, bias_u, bias_v, n_heads, B=1, lens=None, out_mode="fp32"):
    """pk_diag_relpos_attention_form: the fp32 attention layer on the kernel form asked for ("default", "block", "strip"; PkError if the form
    does not cover the shape).  Arguments as diag_relpos_attention; pos None: no position term; out_mode "fp32", "bf16" (widened) or "sigma"
    (fp32, sigma columns) -> (ctx [rows + ATT_GUARD_ROWS][d] fp32 with the guard rows, the form that ran: "block" or "strip")."""
    qkv = _c(qkv)
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    assert qkv.shape[1] == 3 * d
    if pos is not None:
        pos, bu, bv = _c(pos), _c(bias_u), _c(bias_v)
        pos_T = (pos.shape[0] + 1) // 2
        assert pos.shape == (2 * pos_T - 1, d) and bu.shape == (d,) and bv.shape == (d,)
    if lens is not None:
        ln = np.ascontiguousarray(lens, np.int32)
        assert int(ln.sum()) == rows
        B, T, lp = len(ln), int(ln.max()), _i(ln)
    else:
        assert rows % B == 0
        T, lp = rows // B, None
    out = np.empty((rows + ATT_GUARD_ROWS, d), np.float32)
    ran = C.c_int(-1)
    none = C.cast(None, f32p)
    check(lib().pk_diag_relpos_attention_form(ATT_FORMS[form], ATT_OUT_MODES[out_mode], B, lp, T, d, n_heads, _f(qkv),
                                              none if pos is None else _f(pos), 0 if pos is None else pos_T,
                                              none if pos is None else _f(bu), none if pos is None else _f(bv), _f(out), C.byref(ran)))
    return out, {1: "block", 2: "strip"}[ran.value]


STREAM_ATT_FORMS = ("general-1w", "general-2w", "tiles-hd64", "tiles-hd128")   # PK_DIAG_STREAM_ATT_*


def diag_stream_attention(qkv_new, kcache, vcache, nc, pos, bias_u, bias_v, n_heads, left, right, keep_max, ctx_sigma=False, rotate=True):
    """pk_diag_stream_attention: the cached attention of one streaming chunk alone, launched as a session launches it.  qkv_new [S][c][3 d]
    (natural columns), kcache / vcache [S][cache_rows][d] with nc valid rows per stream, pos [P][d] -> (ctx [S c + ATT_GUARD_ROWS][d],
    cache_k_out, cache_v_out [S cache_rows + ATT_GUARD_ROWS][d], form: one of STREAM_ATT_FORMS).  Every output word the launch did not write
    holds ATT_UNWRITTEN["fp32"]; ctx_sigma: the columns of ctx in the sigma layout; rotate: the launch also writes the new caches."""
    qkv, kc, vc, pos, bu, bv = _c(qkv_new), _c(kcache), _c(vcache), _c(pos), _c(bias_u), _c(bias_v)
    S, c, d = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    cache_rows = kc.shape[1]
    assert qkv.shape == (S, c, 3 * d) and kc.shape == vc.shape == (S, cache_rows, d) and pos.shape[1] == d and bu.shape == bv.shape == (d,)
    ctx = np.empty((S * c + ATT_GUARD_ROWS, d), np.float32)
    ko, vo = (np.empty((S * cache_rows + ATT_GUARD_ROWS, d), np.float32) for _ in range(2))
    form = C.c_int(-1)
    check(lib().pk_diag_stream_attention(S, c, int(nc), cache_rows, d, n_heads, _f(qkv), _f(kc), _f(vc), _f(pos), pos.shape[0], _f(bu), _f(bv),
                                         int(left), int(right), int(keep_max), int(bool(ctx_sigma)), int(bool(rotate)), _f(ctx), _f(ko), _f(vo),
                                         C.byref(form)))
    return ctx, ko, vo, STREAM_ATT_FORMS[form.value]


MEL_FORMS = ("uniform", "ragged", "stream")     # PK_DIAG_MEL_UNIFORM / _RAGGED / _STREAM
MEL_FILL = 0x7FC5A5A5                           # PK_DIAG_MEL_FILL: what a word no launch wrote comes back as
MEL_SPARE_WORDS = 64                            # PK_DIAG_MEL_SPARE_WORDS


def mel_logmel_pitch(n_frames):
    """frames per row of a clip's log-mel block on the device (kernels.hpp mel_logmel_pitch)"""
    return (n_frames + 15) & ~15


def diag_mel(pcm, form="uniform", n_mels=80, normalize=True, window_centered=False, power_via_abs=True, spare=MEL_SPARE_WORDS, logmel=None, feats=None):
    """pk_diag_mel: the mel front end alone, no model.  form "uniform": pcm [B][n] -> log-mel blocks [B][n_mels][pitch], features [B][frames][n_mels];
    "ragged": pcm a list of clips -> blocks [n_mels][pitch of the clip] one behind the other, features packed along the frames; "stream": pcm [B][n]
    ALREADY pre-emphasised -> log-mel [B][frames][n_mels], no features.  -> (logmel, feats, n_frames [B], grid): both buffers WHOLE and flat, what the
    launches write plus `spare` words, every word no launch wrote holding MEL_FILL; grid = ((x, y, threads) of the log-mel launch, of the normalise
    launch).  logmel / feats: buffers of the caller's to receive them (a refused call leaves them as they were)."""
    f = MEL_FORMS.index(form)
    if form == "ragged":
        clips = [_c(c).reshape(-1) for c in pcm]
        B, n = len(clips), 0
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([c.size for c in clips])
        x = np.concatenate(clips) if B else np.zeros(0, np.float32)
        lens = [c.size for c in clips]
    else:
        x = _c(pcm)
        x = x[None] if x.ndim == 1 else x
        B, n = x.shape
        off, lens = None, [n] * B
    nf = [max(0, (m - 400) // 160 + 1) if form == "stream" else 1 + m // 160 for m in lens]
    n_lm = sum(nf) * n_mels if form == "stream" else sum(mel_logmel_pitch(t) for t in nf) * n_mels
    n_ft = 0 if form == "stream" else sum(nf) * n_mels
    logmel = np.empty(n_lm + spare, np.float32) if logmel is None else logmel
    feats = np.empty(n_ft + spare, np.float32) if feats is None else feats
    assert logmel.dtype == feats.dtype == np.float32 and logmel.flags.c_contiguous and feats.flags.c_contiguous
    frames, grid = np.zeros(max(B, 1), np.int32), np.zeros(6, np.int32)
    check(lib().pk_diag_mel(int(n_mels), int(bool(normalize)), int(bool(window_centered)), int(bool(power_via_abs)), f, _f(x), B, n,
                            off.ctypes.data_as(i64p) if off is not None else None, _f(logmel), logmel.size, _f(feats), feats.size, _i(frames), _i(grid)))
    return logmel, feats, frames[:B], (tuple(int(v) for v in grid[:3]), tuple(int(v) for v in grid[3:]))


class PkSmallmGemmDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("M", "N", "K", "epi", "w_sig", "a_sigma", "sigma_cols", "fused")]
                + [("A", f32p), ("lda", C.c_int64), ("W", f32p), ("bias", f32p), ("resid", f32p), ("alpha", C.c_float),
                   ("remap_rows", C.c_int32), ("remap_gs", C.c_int64), ("remap_rs", C.c_int64), ("remap_cs", C.c_int64),
                   ("ln_g", f32p), ("ln_b", f32p), ("eps", C.c_float), ("pre_g", f32p), ("pre_b", f32p), ("pre_out", f32p)]
                + [(k, C.c_int32) for k in ("dw", "dw_c", "dw_has_cache", "dw_out_sigma", "cache_streams")]
                + [("cache_in", f32p), ("cache_out", f32p)]
                + [(k, f32p) for k in ("dw_w", "dw_bias", "bn_mean", "bn_rstd", "bn_g", "bn_b")]
                + [("ldo", C.c_int64), ("out_words", C.c_int64), ("out", f32p), ("form", C.c_int32)])


_LATE_SIGNATURES["pk_diag_gemm_smallm"] = [C.POINTER(PkSmallmGemmDiag)]


SMALLM_KERNELS = ("chain", "rt2", "ln")


def smallm_form(v):
    """A GemmSmallmForm value (kernels.hpp; PK_DIAG_SMALLM_*) -> (kernel, epi, ring depth or K / 64, sig, dw, pre)"""
    epi = {n: k for k, n in EPI.items()}[(v >> 9) & 7]
    return SMALLM_KERNELS[v >> 12], epi, (v >> 3) & 63, bool(v & 4), bool(v & 2), bool(v & 1)


def diag_gemm_smallm_forms():
    """pk_diag_gemm_smallm_forms: every form launch_gemm_smallm can take, as smallm_form tuples.  Host arithmetic."""
    return _forms("pk_diag_gemm_smallm_forms", smallm_form)


def diag_gemm_smallm(A, W, bias=None, epi="none", resid=None, alpha=1.0, w_sig=False, a_sigma=False, sigma_cols=0, remap=None, ldo=None, out_words=None,
                     ln=None, pre=None, eps=1e-5, dw=None, fused=True, lda_cols=None):
    """pk_diag_gemm_smallm: one product of the fp32 small-M family alone (include/parakeet_amd.h).  A [M][lda >= K] (K = lda_cols or A's width), W natural;
    remap = (rows, gs, rs, cs); ln = (gamma, beta); pre = (gamma, beta); dw = dict(c, has_cache, out_sigma, cache_in [S][8][d], cache_streams, w [9][d], bias,
    bn_mean, bn_rstd, bn_g, bn_b).  Returns dict(out = the WHOLE output buffer as uint32 words [out_words] exactly as the launches left it (SKINNY_FILL32
    where nothing was stored), form = smallm_form tuple, pre_out [M][K] words, cache_out [cache_streams][8][d] words)."""
    A, W = _c(A), _c(W)
    M, lda = A.shape
    K = int(lda_cols) if lda_cols is not None else lda
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    assert W.shape[1] == K
    opt = _Keep(A, W).opt
    d = PkSmallmGemmDiag()
    d.M, d.N, d.K, d.epi, d.w_sig, d.a_sigma, d.sigma_cols, d.fused = M, N, K, EPI[epi], int(bool(w_sig)), int(bool(a_sigma)), int(sigma_cols), int(bool(fused))
    d.A, d.lda, d.W, d.bias, d.resid, d.alpha = _f(A), lda, _f(W), opt(bias), opt(resid), alpha
    _set_remap(d, remap)
    d.eps = eps
    if ln is not None:
        d.ln_g, d.ln_b = opt(ln[0]), opt(ln[1])
    pre_out = None
    if pre is not None:
        pre_out = np.zeros((M, K), np.uint32)
        d.pre_g, d.pre_b, d.pre_out = opt(pre[0]), opt(pre[1]), pre_out.ctypes.data_as(f32p)
    cache_out = None
    if dw is not None:
        ns = int(dw.get("cache_streams", M // dw["c"]))
        cache_out = np.zeros((ns, 8, N), np.uint32)
        d.dw, d.dw_c, d.dw_has_cache, d.dw_out_sigma, d.cache_streams = 1, int(dw["c"]), int(bool(dw["has_cache"])), int(bool(dw.get("out_sigma"))), ns
        d.cache_in, d.cache_out = opt(dw["cache_in"]), cache_out.ctypes.data_as(f32p)
        d.dw_w, d.dw_bias, d.bn_mean, d.bn_rstd, d.bn_g, d.bn_b = (opt(dw[k]) for k in ("w", "bias", "bn_mean", "bn_rstd", "bn_g", "bn_b"))
    _out_words_default(d, M, N, ldo, out_words)
    out = np.zeros(d.out_words, np.uint32)
    d.out = out.ctypes.data_as(f32p)
    d.form = -1
    check(lib().pk_diag_gemm_smallm(C.byref(d)))
    return dict(out=out, form=smallm_form(d.form), pre_out=pre_out, cache_out=cache_out)


def diag_sigma_copy(src, K=None):
    """pk_diag_sigma_copy: src [rows][ld >= K] -> the rows x K floats of the W_sig tiling (launch_sigma_copy)."""
    src = _c(src)
    rows, ld = src.shape
    K = ld if K is None else int(K)
    dst = np.empty(rows * K, np.float32)
    check(lib().pk_diag_sigma_copy(_f(src), rows, K, ld, _f(dst)))
    return dst


def diag_layernorm_sigma(x, g, b, eps=1e-5):
    """pk_diag_layernorm_sigma: launch_layernorm mode 2 -- LayerNorm with the output columns in the sigma order."""
    x, g, b = _c(x), _c(g), _c(b)
    y = np.empty_like(x)
    check(lib().pk_diag_layernorm_sigma(_f(x), x.shape[0], x.shape[1], _f(g), _f(b), eps, _f(y)))
    return y


def diag_layernorm2(x, g1, b1, g2, b2, y2_sigma=False, eps=1e-5):
    """pk_diag_layernorm2: (y1 = LN(x; g1, b1), y2 = LN(y1; g2, b2)) in one launch; y2_sigma: y2's columns in the sigma order."""
    x, g1, b1, g2, b2 = (_c(v) for v in (x, g1, b1, g2, b2))
    y1, y2 = np.empty_like(x), np.empty_like(x)
    check(lib().pk_diag_layernorm2(_f(x), x.shape[0], x.shape[1], _f(g1), _f(b1), _f(g2), _f(b2), eps, int(bool(y2_sigma)), _f(y1), _f(y2)))
    return y1, y2


class PkLayernormDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("launcher", "d", "mode", "in_place")] + [("rows", C.c_int64), ("eps", C.c_float)]
                + [(k, f32p) for k in ("x", "g1", "b1", "g2", "b2")]
                + [("y", C.POINTER(C.c_uint32)), ("y_words", C.c_int64), ("y2", C.POINTER(C.c_uint32)), ("y2_words", C.c_int64),
                   ("stats", C.POINTER(C.c_uint32)), ("stats_words", C.c_int64), ("form", C.c_int32)])


_LATE_SIGNATURES["pk_diag_layernorm_form"] = [C.POINTER(PkLayernormDiag)]


LN_LAUNCHERS = ("norm", "norm2", "stats", "then_stats")       # PK_DIAG_LN_NORM .. PK_DIAG_LN_THEN_STATS
LN_PAD_WORDS = 67                                               # spare words behind every output buffer of diag_layernorm_form (any positive count will do)


def ln_form(v):
    """A LayerNorm form value (kernels.hpp ln_form_of; PK_DIAG_LN_*) -> (launcher, PER_LANE, RPW, THEN, batch branch)"""
    return LN_LAUNCHERS[v >> 12], v & 31, (v >> 5) & 31, bool((v >> 10) & 1), bool((v >> 11) & 1)


def diag_layernorm_forms():
    """pk_diag_layernorm_forms: every form the four LayerNorm launchers can take, as ln_form tuples.  Host arithmetic."""
    return _forms("pk_diag_layernorm_forms", ln_form)


def diag_layernorm_form_of(launcher, rows, d):
    """pk_diag_layernorm_form_of: the form `launcher` (one of LN_LAUNCHERS) takes for rows x d.  Host arithmetic."""
    form = C.c_int32(-1)
    check(lib().pk_diag_layernorm_form_of(LN_LAUNCHERS.index(launcher), int(rows), int(d), C.byref(form)))
    return ln_form(form.value)


def diag_layernorm_form(launcher, x, g1=None, b1=None, g2=None, b2=None, eps=1e-5, mode=0, in_place=False, pad_words=LN_PAD_WORDS):
    """pk_diag_layernorm_form: one launch of one LayerNorm launcher (one of LN_LAUNCHERS) alone (include/parakeet_amd.h).  x [rows][d]; mode 0 fp32 /
    1 bf16 / 2 fp32 sigma columns (of y for "norm", of y2 for "norm2"); in_place: y / y1 aliases the device copy of x.  Returns dict(form = ln_form tuple,
    and for every buffer the launcher writes -- y (y1 of "norm2" / "then_stats"), y2, stats -- the WHOLE buffer as uint32 words exactly as the launch left
    it: the payload followed by pad_words words, SKINNY_FILL32 wherever nothing was stored; a bf16 buffer holds two elements to a word)."""
    x = _c(x)
    rows, d = x.shape
    opt = _Keep(x).opt
    a = PkLayernormDiag()
    a.launcher, a.d, a.mode, a.in_place, a.rows, a.eps = LN_LAUNCHERS.index(launcher), d, int(mode), int(bool(in_place)), rows, eps
    a.x, a.g1, a.b1, a.g2, a.b2 = _f(x), opt(g1), opt(b1), opt(g2), opt(b2)
    n = rows * d
    out = {}

    def buf(name, words):
        b = np.zeros(words + pad_words, np.uint32)
        out[name] = b
        setattr(a, name, b.ctypes.data_as(C.POINTER(C.c_uint32)))
        setattr(a, name + "_words", b.size)

    if launcher != "stats":
        buf("y", (n + 1) // 2 if (launcher == "norm" and mode == 1) else n)
    if launcher == "norm2":
        buf("y2", (n + 1) // 2 if mode == 1 else n)
    if launcher in ("stats", "then_stats"):
        buf("stats", 2 * rows)
    a.form = -1
    check(lib().pk_diag_layernorm_form(C.byref(a)))
    out["form"] = ln_form(a.form)
    return out


class PkGemmTileDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("M", "N", "K", "epi", "sigma_cols")]
                + [("A", f32p), ("lda", C.c_int64), ("W", f32p), ("ldw", C.c_int64), ("bias", f32p), ("resid", f32p), ("ldr", C.c_int64), ("alpha", C.c_float),
                   ("remap_rows", C.c_int32), ("remap_gs", C.c_int64), ("remap_rs", C.c_int64), ("remap_cs", C.c_int64),
                   ("ln_g", f32p), ("ln_b", f32p), ("eps", C.c_float), ("ldo", C.c_int64), ("out_words", C.c_int64), ("out", f32p), ("form", C.c_int32)])


_LATE_SIGNATURES["pk_diag_gemm_tile"] = [C.POINTER(PkGemmTileDiag)]


def tile_form(v):
    """A GemmTileForm value (kernels.hpp; PK_DIAG_TILE_*) -> (kernel, tile, NBUF, LNA, SCHED, epi): kernel "nt" (gemm_nt_kernel, tile = (BM, BN)) or "pipe"
    (gemm_pipe_kernel, tile = (WGM, WGN, TM, TN): WGM x WGN waves of TM x TN 32 x 32 accumulators)"""
    epi = {n: k for k, n in EPI.items()}[v & 7]
    wgm, wgn, tm, tn = (v >> 17) & 7, (v >> 14) & 7, (v >> 11) & 7, (v >> 8) & 7
    kernel = ("nt", "pipe")[v >> 20]
    tile = (32 * wgm * tm, 32 * wgn * tn) if kernel == "nt" else (wgm, wgn, tm, tn)
    return kernel, tile, (v >> 6) & 3, bool(v & 32), (v >> 3) & 3, epi


def diag_gemm_tile_forms():
    """pk_diag_gemm_tile_forms: every form launch_gemm can take on the tile kernels, as tile_form tuples.  Host arithmetic."""
    return _forms("pk_diag_gemm_tile_forms", tile_form)


def diag_gemm_tile_form(M, N, K, lda=None, ldw=None, epi="none", ln=False):
    """pk_diag_gemm_tile_form: the form pk_diag_gemm_tile would launch for this product (ln: with the LayerNorm fold).  Host arithmetic; the refusals
    of pk_diag_gemm_tile that depend on the shape alone raise here too."""
    form = C.c_int32(-1)
    check(lib().pk_diag_gemm_tile_form(M, N, K, K if lda is None else lda, K if ldw is None else ldw, EPI[epi], int(bool(ln)), C.byref(form)))
    return tile_form(form.value)


def diag_gemm_tile(A, W, bias=None, epi="none", resid=None, alpha=1.0, sigma_cols=0, remap=None, ldo=None, out_words=None, ln=None, eps=1e-5,
                   lda=None, ldw=None, ldr=None):
    """pk_diag_gemm_tile: one product of the fp32 tile GEMM family alone (include/parakeet_amd.h).  A [M][K], W [N or 2N][K], resid [M][N] dense; lda / ldw /
    ldr: the pitches they are staged at (the padding holds a NaN pattern on the device); remap = (rows, gs, rs, cs); ln = (gamma, beta).
    Returns dict(out = the WHOLE output buffer as uint32 words [out_words] exactly as the launch left it (SKINNY_FILL32 where nothing was stored),
    form = tile_form tuple)."""
    A, W = _c(A), _c(W)
    M, K = A.shape
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    assert W.shape[1] == K
    d = PkGemmTileDiag()
    A, W = _pitched(A, lda), _pitched(W, ldw)
    opt = _Keep(A, W).opt
    d.M, d.N, d.K, d.epi, d.sigma_cols = M, N, K, EPI[epi], int(sigma_cols)
    d.A, d.lda, d.W, d.ldw, d.bias, d.alpha = _f(A), A.shape[1], _f(W), W.shape[1], opt(bias), alpha
    if resid is not None:
        resid = _pitched(_c(resid), ldr)
        d.resid, d.ldr = opt(resid), resid.shape[1]
    _set_remap(d, remap)
    d.eps = eps
    if ln is not None:
        d.ln_g, d.ln_b = opt(ln[0]), opt(ln[1])
    _out_words_default(d, M, N, ldo, out_words)
    out = np.zeros(max(d.out_words, 1), np.uint32)
    d.out = out.ctypes.data_as(f32p)
    d.form = -1
    check(lib().pk_diag_gemm_tile(C.byref(d)))
    return dict(out=out[:d.out_words], form=tile_form(d.form))


class PkGemmBf16TileDiag(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("M", "N", "K", "epi", "sigma_cols", "a_bf16", "a_blocked", "out_bf16", "out_blocked", "fast_act")]
                + [("A", f32p), ("lda", C.c_int64), ("W", f32p), ("ldw", C.c_int64), ("bias", f32p), ("resid", f32p), ("ldr", C.c_int64), ("alpha", C.c_float),
                   ("remap_rows", C.c_int32), ("remap_gs", C.c_int64), ("remap_rs", C.c_int64), ("remap_cs", C.c_int64),
                   ("ldo", C.c_int64), ("out_words", C.c_int64), ("out", C.POINTER(C.c_uint32)), ("form", C.c_int32), ("one_form", C.c_int32)])


_LATE_SIGNATURES["pk_diag_gemm_bf16_tile_form"] = [C.POINTER(PkGemmBf16TileDiag)]
_LATE_SIGNATURES["pk_diag_gemm_bf16_tile"] = [C.POINTER(PkGemmBf16TileDiag)]


BF16_EPILOGUES = ("lds", "direct", "persist", "resid_reg")


def bf16_form(v):
    """A GemmBf16Form value (kernels.hpp; PK_DIAG_BF16_*) -> (kernel, (WGM, WGN, TM, TN), a16, epilogue form, epi): kernel "reg" (gemm_bf16_kernel,
    register-staged) or "glds" (gemm_bf16_glds_kernel, direct-to-LDS); WGM x WGN waves of TM x TN 32 x 32 accumulators; epilogue form one of BF16_EPILOGUES"""
    epi = {n: k for k, n in EPI.items()}[v & 7]
    return ("reg", "glds")[v >> 18], ((v >> 15) & 7, (v >> 12) & 7, (v >> 9) & 7, (v >> 6) & 7), bool(v & 32), BF16_EPILOGUES[(v >> 3) & 3], epi


def diag_gemm_bf16_tile_forms():
    """pk_diag_gemm_bf16_tile_forms: every form launch_gemm_bf16 can take on the tile kernels, as bf16_form tuples.  Host arithmetic."""
    return _forms("pk_diag_gemm_bf16_tile_forms", bf16_form)


def _bf16_tile_args(M, N, K, epi, a16, bias, resid, alpha, lda, ldw, ldo, ldr, sigma_cols, remap, fast_act, out_bf16, out_blocked, a_blocked, out_words):
    d = PkGemmBf16TileDiag()
    d.M, d.N, d.K, d.epi, d.sigma_cols = M, N, K, EPI[epi], int(sigma_cols)
    d.a_bf16, d.a_blocked, d.out_bf16, d.out_blocked, d.fast_act = (int(bool(v)) for v in (a16, a_blocked, out_bf16, out_blocked, fast_act))
    d.lda, d.ldw, d.ldr, d.alpha = int(lda or K), int(ldw or K), int(ldr or N), alpha
    _set_remap(d, remap)
    _out_words_default(d, M, N, ldo, out_words, half=out_bf16, blocked=out_blocked)
    d.form = -1
    return d


def diag_gemm_bf16_tile_form(M, N, K, epi="none", a16=False, bias=True, alpha=1.0, lda=None, ldw=None, ldo=None, ldr=None, sigma_cols=0, remap=None,
                             fast_act=False, out_bf16=False, out_blocked=False, a_blocked=False, out_words=None, one_form=False):
    """pk_diag_gemm_bf16_tile_form: the form pk_diag_gemm_bf16_tile would launch for this product.  Host arithmetic, no device; every refusal of
    pk_diag_gemm_bf16_tile raises here too."""
    d = _bf16_tile_args(M, N, K, epi, a16, bias, None, alpha, lda, ldw, ldo, ldr, sigma_cols, remap, fast_act, out_bf16, out_blocked, a_blocked, out_words)
    one = np.zeros(1, np.float32)                                   # (looked at for null only)
    d.bias = _f(one) if bias else None
    d.resid = _f(one) if epi == "resid" else None
    d.one_form = int(bool(one_form))
    check(lib().pk_diag_gemm_bf16_tile_form(C.byref(d)))
    return bf16_form(d.form)


def diag_gemm_bf16_tile(A, W, bias=None, epi="none", resid=None, alpha=1.0, a16=False, lda=None, ldw=None, ldo=None, ldr=None, sigma_cols=0, remap=None,
                        fast_act=False, out_bf16=False, out_blocked=False, a_blocked=False, out_words=None, one_form=False):
    """pk_diag_gemm_bf16_tile: one product of the bf16 tile GEMM family alone (include/parakeet_amd.h).  A [M][K], W [N or 2N][K], resid [M][N] dense fp32
    (the entry rounds W, and A with a16, to bf16); lda / ldw / ldr: the pitches they are staged at (NaN behind every row on the device); a_blocked: A staged
    in 32 x 16 blocks; remap = (rows, gs, rs, cs).  Returns dict(out = the WHOLE output buffer as uint32 words [out_words] exactly as the launch left it
    (SKINNY_FILL32 where nothing was stored; out_bf16: two bf16 to a word), form = bf16_form tuple)."""
    A, W = _c(A), _c(W)
    M, K = A.shape
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    assert W.shape[1] == K
    A, W = _pitched(A, lda), _pitched(W, ldw)
    d = _bf16_tile_args(M, N, K, epi, a16, bias is not None, resid, alpha, A.shape[1], W.shape[1], ldo, ldr, sigma_cols, remap, fast_act, out_bf16,
                        out_blocked, a_blocked, out_words)
    opt = _Keep(A, W).opt
    d.A, d.W, d.bias = _f(A), _f(W), opt(bias)
    if resid is not None:
        resid = _pitched(_c(resid), ldr)
        d.resid, d.ldr = opt(resid), resid.shape[1]
    out = np.zeros(max(d.out_words, 1), np.uint32)
    d.out = out.ctypes.data_as(C.POINTER(C.c_uint32))
    d.one_form = int(bool(one_form))
    check(lib().pk_diag_gemm_bf16_tile(C.byref(d)))
    return dict(out=out[:d.out_words], form=bf16_form(d.form))


class PkGemmSmallmBf16Diag(C.Structure):
    _u32p = C.POINTER(C.c_uint32)
    _fields_ = ([(k, C.c_int32) for k in ("M", "N", "K", "epi", "a_bf16", "out_bf16", "out_t8", "a_t8", "fast_act", "w_tiles", "resid_in_place")]
                + [("A", f32p), ("lda", C.c_int64), ("W", f32p), ("ldw", C.c_int64), ("bias", f32p), ("resid", f32p), ("ldr", C.c_int64), ("alpha", C.c_float),
                   ("ln_g", f32p), ("ln_b", f32p), ("eps", C.c_float), ("pre_g", f32p), ("pre_b", f32p), ("pre_out", _u32p), ("pre_ldo", C.c_int64),
                   ("pre_out_words", C.c_int64)]
                + [(k, C.c_int32) for k in ("dw", "dw_c", "dw_has_cache", "cache_streams")]
                + [("cache_in", f32p), ("cache_out", _u32p)]
                + [(k, f32p) for k in ("dw_w", "dw_bias", "bn_mean", "bn_rstd", "bn_g", "bn_b")]
                + [("ldo", C.c_int64), ("out_words", C.c_int64), ("out", _u32p), ("form", C.c_int32), ("one_form", C.c_int32)])


_LATE_SIGNATURES["pk_diag_gemm_smallm_bf16_form"] = [C.POINTER(PkGemmSmallmBf16Diag)]
_LATE_SIGNATURES["pk_diag_gemm_smallm_bf16"] = [C.POINTER(PkGemmSmallmBf16Diag)]


SMALLM_BF16_FIELDS = ("epi", "steps", "rt", "rvalid", "a16", "ln", "ct", "wt", "dw", "at", "al", "pre")


def smallm_bf16_form(v):
    """A GemmSmallmBf16Form value (kernels.hpp; PK_DIAG_SMALLM_BF16_*) -> (epi, STEPS 8 / 16, RT 1 / 2, rvalid 8 / 16, A16, LN, CT 1 / 2, WT, DW, AT, AL, PRE):
    SMALLM_BF16_FIELDS names the positions"""
    epi = {n: k for k, n in EPI.items()}[v & 7]
    bit = lambda i: bool((v >> i) & 1)  # noqa: E731
    return (epi, 16 if bit(3) else 8, 2 if bit(4) else 1, 16 if bit(5) else 8, bit(6), bit(7), 2 if bit(8) else 1, bit(9), bit(10), bit(11), bit(12), bit(13))


def diag_gemm_smallm_bf16_forms():
    """pk_diag_gemm_smallm_bf16_forms: every form launch_gemm_smallm_bf16 can take, as smallm_bf16_form tuples.  Host arithmetic."""
    return _forms("pk_diag_gemm_smallm_bf16_forms", smallm_bf16_form)


def _smallm_bf16_args(M, N, K, epi, a16, alpha, lda, ldw, ldo, ldr, out_bf16, out_t8, a_t8, fast_act, w_tiles, resid_in_place, eps, pre_ldo, pre_out_words,
                      dw_c, has_cache, cache_streams, out_words):
    d = PkGemmSmallmBf16Diag()
    d.M, d.N, d.K, d.epi = M, N, K, EPI[epi]
    d.a_bf16, d.out_bf16, d.out_t8, d.a_t8, d.fast_act, d.w_tiles, d.resid_in_place = (int(bool(v)) for v in (a16, out_bf16, out_t8, a_t8, fast_act, w_tiles, resid_in_place))
    _out_words_default(d, M, N, ldo, out_words, half=out_bf16)
    d.lda, d.ldw, d.ldr, d.alpha, d.eps = int(lda or K), int(ldw or K), int(ldr or (d.ldo if resid_in_place else N)), alpha, eps
    d.pre_ldo = int(pre_ldo or K)
    d.pre_out_words = int(pre_out_words) if pre_out_words is not None else M * d.pre_ldo
    if dw_c:
        d.dw, d.dw_c, d.dw_has_cache = 1, int(dw_c), int(bool(has_cache))
        d.cache_streams = int(cache_streams) if cache_streams is not None else -(-M // int(dw_c))
    d.form = -1
    return d


def diag_gemm_smallm_bf16_form(M, N, K, epi="none", a16=False, bias=True, alpha=1.0, lda=None, ldw=None, ldo=None, ldr=None, out_bf16=False, out_t8=False,
                               a_t8=False, fast_act=False, w_tiles=True, resid_in_place=False, ln=False, pre=False, eps=1e-5, pre_ldo=None, pre_out_words=None,
                               dw_c=0, has_cache=True, cache_streams=None, out_words=None, one_form=False):
    """pk_diag_gemm_smallm_bf16_form: the form pk_diag_gemm_smallm_bf16 would launch for this product (ln / pre / dw_c: with the folded norm, the norm in front,
    the conv tail).  Host arithmetic, no device; every refusal of pk_diag_gemm_smallm_bf16 that depends on the shape and the switches raises here too."""
    d = _smallm_bf16_args(M, N, K, epi, a16, alpha, lda, ldw, ldo, ldr, out_bf16, out_t8, a_t8, fast_act, w_tiles, resid_in_place, eps, pre_ldo, pre_out_words,
                          dw_c, has_cache, cache_streams, out_words)
    one = np.zeros(1, np.float32)                                   # (looked at for null only)
    one32 = np.zeros(1, np.uint32)
    d.bias = _f(one) if bias else None
    d.resid = _f(one) if epi == "resid" else None
    if ln or pre:
        d.ln_g = d.ln_b = _f(one)
    if pre:
        d.pre_g = d.pre_b = _f(one)
        d.pre_out = one32.ctypes.data_as(C.POINTER(C.c_uint32))
    d.one_form = int(bool(one_form))
    check(lib().pk_diag_gemm_smallm_bf16_form(C.byref(d)))
    return smallm_bf16_form(d.form)


def diag_gemm_smallm_bf16(A, W, bias=None, epi="none", resid=None, alpha=1.0, a16=False, lda=None, ldw=None, ldo=None, ldr=None, out_bf16=False, out_t8=False,
                          a_t8=False, fast_act=False, w_tiles=True, resid_in_place=False, ln=None, pre=None, eps=1e-5, pre_ldo=None, pre_out_words=None,
                          dw=None, out_words=None, into=None):
    """pk_diag_gemm_smallm_bf16: one product of the small-M bf16 family alone (include/parakeet_amd.h).  A [M][K], W [N or 2N][K], resid [M][N] dense fp32 (the
    entry rounds W, and A with a16, to bf16); lda / ldw / ldr: the pitches they are staged at (NaN behind every row on the device); ln = (gamma, beta);
    pre = (gamma, beta); dw = dict(c, has_cache, cache_in [S][8][N], cache_streams, w [9][N], bias, bn_mean, bn_rstd, bn_g, bn_b).  Returns dict(out = the
    WHOLE output buffer as uint32 words [out_words] exactly as the launch left it (SKINNY_FILL32 where nothing was stored; out_bf16: two bf16 to a word),
    form = smallm_bf16_form tuple, pre_out [pre_out_words] words, cache_out [cache_streams 8 N] words).  into: a dict that receives the host buffers (out,
    pre_out, cache_out; pre-filled with the word into["fill"]) and the argument struct ("args") BEFORE the call -- what a refused call left of them."""
    A, W = _c(A), _c(W)
    M, K = A.shape
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]
    assert W.shape[1] == K
    A, W = _pitched(A, lda), _pitched(W, ldw)
    d = _smallm_bf16_args(M, N, K, epi, a16, alpha, A.shape[1], W.shape[1], ldo, ldr, out_bf16, out_t8, a_t8, fast_act, w_tiles, resid_in_place, eps, pre_ldo,
                          pre_out_words, dw["c"] if dw else 0, dw["has_cache"] if dw else False, dw.get("cache_streams") if dw else None, out_words)
    opt = _Keep(A, W).opt
    u32p = C.POINTER(C.c_uint32)
    d.A, d.W, d.bias = _f(A), _f(W), opt(bias)
    if resid is not None:
        d.resid = opt(_pitched(_c(resid), d.ldr))
    if ln is not None:
        d.ln_g, d.ln_b = opt(ln[0]), opt(ln[1])
    pre_out = None
    if pre is not None:
        pre_out = np.zeros(max(d.pre_out_words, 1), np.uint32)
        d.pre_g, d.pre_b, d.pre_out = opt(pre[0]), opt(pre[1]), pre_out.ctypes.data_as(u32p)
    cache_out = None
    if dw is not None:
        cache_out = np.zeros(max(d.cache_streams, 1) * 8 * N, np.uint32)
        d.cache_in, d.cache_out = opt(dw["cache_in"]), cache_out.ctypes.data_as(u32p)
        d.dw_w, d.dw_bias, d.bn_mean, d.bn_rstd, d.bn_g, d.bn_b = (opt(dw[k]) for k in ("w", "bias", "bn_mean", "bn_rstd", "bn_g", "bn_b"))
    out = np.zeros(max(d.out_words, 1), np.uint32)
    d.out = out.ctypes.data_as(u32p)
    if into is not None:
        for buf in (out, pre_out, cache_out):
            if buf is not None:
                buf.fill(into.get("fill", 0))
        into.update(out=out, pre_out=pre_out, cache_out=cache_out, args=d)
    check(lib().pk_diag_gemm_smallm_bf16(C.byref(d)))
    return dict(out=out[:d.out_words], form=smallm_bf16_form(d.form), pre_out=pre_out, cache_out=cache_out)


def diag_tile_copy_bf16(src, K=None):
    """pk_diag_tile_copy_bf16: src [rows][ld >= K] (rounded to bf16) -> the rows x K bf16 bit patterns of the W_t16 operand tiles (launch_tile_copy_bf16)."""
    src = _c(src)
    rows, ld = src.shape
    K = ld if K is None else int(K)
    dst = np.empty(rows * K, np.uint16)
    check(lib().pk_diag_tile_copy_bf16(_f(src), rows, K, ld, dst.ctypes.data_as(C.POINTER(C.c_uint16))))
    return dst


class Batch:
    """pk_batch: the resident pipeline (clips of one length stay in HBM; decode(k) overlaps encoder(k+1))."""

    def __init__(self, model, max_clips, n_samples):
        self._h = C.c_void_p()
        self.n_clips = 0
        self._cap = max_clips
        check(lib().pk_batch_create(model._h, max_clips, n_samples, C.byref(self._h)))

    @classmethod
    def ragged(cls, model, max_clips, max_total_samples, max_clip_samples):
        """pk_batch_create_ragged: a pipeline whose runs take clips of ANY lengths (packed, no padding)."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.n_clips = 0
        self._cap = max_clips
        check(lib().pk_batch_create_ragged(model._h, max_clips, int(max_total_samples), int(max_clip_samples), C.byref(self._h)))
        return self

    @staticmethod
    def _pack(clips):
        clips = [_c(c).ravel() for c in clips]
        off = np.zeros(len(clips) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clips])
        return np.concatenate(clips), off

    def upload_ragged(self, clips):
        pcm, off = self._pack(clips)
        self.n_clips = len(off) - 1
        check(lib().pk_batch_upload_ragged(self._h, _f(pcm), off.ctypes.data_as(i64p), self.n_clips))

    def upload_ragged_async(self, clips):
        pcm, off = self._pack(clips)
        self._staged = pcm
        self._staged_clips = len(off) - 1
        check(lib().pk_batch_upload_ragged_async(self._h, _f(pcm), off.ctypes.data_as(i64p), len(off) - 1))

    def upload(self, pcm):
        pcm = _c(pcm)
        self.n_clips = pcm.shape[0]
        check(lib().pk_batch_upload(self._h, _f(pcm), self.n_clips))

    def upload_async(self, pcm):
        """Stage the NEXT batch under the running encoder (double-buffered PCM, no flush)."""
        pcm = _c(pcm)
        self._staged = pcm                                   # keep the host array alive until the copy has been consumed
        self._staged_clips = pcm.shape[0]
        check(lib().pk_batch_upload_async(self._h, _f(pcm), pcm.shape[0]))

    def run(self, decoder="tdt"):
        if getattr(self, "_staged_clips", 0):
            self.n_clips, self._staged_clips = self._staged_clips, 0
        check(lib().pk_batch_run(self._h, {"ctc": 0, "tdt": 1}[decoder]))

    def set_decode_group(self, group):
        """Throughput mode: the TDT loops of `group` consecutive runs are decoded as one lock-step batch (results unchanged, later)."""
        check(lib().pk_batch_set_decode_group(self._h, int(group)))

    def set_decode_overlap(self, on):
        """on: decode on a second stream under the next encoder (default); off: on the encoder's stream, after it.  Same results."""
        check(lib().pk_batch_set_decode_overlap(self._h, int(bool(on))))

    def sync(self):
        check(lib().pk_batch_sync(self._h))

    def results_available(self):
        return int(lib().pk_batch_results_available(self._h))

    def results_back(self, back=0):
        """Results of the (back+1)-th newest run whose decode has finished; no flush."""
        mt = lib().pk_batch_max_tokens(self._h)
        cap = self._cap
        ids = np.zeros((cap, mt), np.int32); st = np.zeros((cap, mt), np.int32); en = np.zeros((cap, mt), np.int32)
        cf = np.zeros((cap, mt), np.float32); lens = np.zeros(cap, np.int32)
        n = C.c_int(0)
        check(lib().pk_batch_results_back(self._h, int(back), C.byref(n), _i(ids), _i(lens), _i(st), _i(en), _f(cf)))
        B = n.value
        return dict(ids=ids[:B], lens=lens[:B], start=st[:B], end=en[:B], conf=cf[:B])

    def margins(self, back=0, n_clips=None):
        """pk_batch_margins: smallest top-1 / top-2 label log-prob margin of every clip of the (back+1)-th newest finished run."""
        mg = np.zeros(self._cap, np.float32)
        check(lib().pk_batch_margins(self._h, int(back), _f(mg)))
        return mg[: (n_clips if n_clips is not None else self._cap)]

    def results_done(self):
        """Results of the newest batch whose decode has finished (run k's decode completes inside run k+1); no flush."""
        mt = lib().pk_batch_max_tokens(self._h)
        cap = self._cap
        ids = np.zeros((cap, mt), np.int32); st = np.zeros((cap, mt), np.int32); en = np.zeros((cap, mt), np.int32)
        cf = np.zeros((cap, mt), np.float32); lens = np.zeros(cap, np.int32)
        n = C.c_int(0)
        check(lib().pk_batch_results_done(self._h, C.byref(n), _i(ids), _i(lens), _i(st), _i(en), _f(cf)))
        B = n.value
        return dict(ids=ids[:B], lens=lens[:B], start=st[:B], end=en[:B], conf=cf[:B])

    def results(self):
        B, mt = self.n_clips, lib().pk_batch_max_tokens(self._h)
        ids = np.zeros((B, mt), np.int32); st = np.zeros((B, mt), np.int32); en = np.zeros((B, mt), np.int32)
        cf = np.zeros((B, mt), np.float32); lens = np.zeros(B, np.int32)
        check(lib().pk_batch_results(self._h, _i(ids), _i(lens), _i(st), _i(en), _f(cf)))
        return dict(ids=ids, lens=lens, start=st, end=en, conf=cf)

    def close(self):
        if self._h:
            lib().pk_batch_free(self._h)
            self._h = None


# ---- model -------------------------------------------------------------------------------------------
def pack_clips(clips):
    """(pcm, offsets) of a list of clips: what pk_transcribe_pcm takes (one copy of the audio; do it outside a timed region)."""
    clips = [_c(c).ravel() for c in clips]
    off = np.zeros(len(clips) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clips])
    return np.concatenate(clips), off


def _clips(clips):
    """(pcm, offsets, n) of a list of clips, or of clips already packed as the tuple (pcm, offsets)"""
    if isinstance(clips, tuple):
        pcm, off = _c(clips[0]), np.ascontiguousarray(clips[1], np.int64)
    else:
        pcm, off = pack_clips(clips)
    return pcm, off, len(off) - 1


def _result_dict(r, timestamps):
    """a pk_result as a dict: text, token_ids and, with timestamps, start / end / conf per token and the words"""
    d = dict(text=(r.text or b"").decode(), token_ids=[r.token_ids[k] for k in range(r.n_tokens)])
    if timestamps:
        d["start"] = [r.start_frame[k] for k in range(r.n_tokens)]
        d["end"] = [r.end_frame[k] for k in range(r.n_tokens)]
        d["conf"] = [r.confidence[k] for k in range(r.n_tokens)]
        d["words"] = [(r.words[k].word.decode(), r.words[k].start, r.words[k].end, r.words[k].confidence) for k in range(r.n_words)]
    return d


def _result_list(res, n, timestamps, with_raw=None):
    """a pk_result array (freed here) as a list of dicts; timestamps[i]: clip i has the timestamp entries"""
    try:
        out = [_result_dict(res[i], timestamps[i]) for i in range(n)]
        if with_raw is not None:
            with_raw(res, n)                                     # e.g. pk_group_verify_exchange on the pk_result array itself
        return out
    finally:
        lib().pk_results_free(res, n)


def _nbest_list(res, n, timestamps, extra=None):
    """a pk_nbest array (freed here) as, per clip, a list of dicts with "score"; extra: name -> [n][N] array of a further per-hypothesis entry"""
    try:
        out = []
        for i in range(n):
            hyps = []
            for j in range(res[i].n_hyp):
                d = _result_dict(res[i].hyp[j], timestamps)
                d["score"] = float(res[i].score[j])
                for k, v in (extra or {}).items():
                    d[k] = float(v[i, j])
                hyps.append(d)
            out.append(hyps)
        return out
    finally:
        lib().pk_nbest_free(res, n)


def _nlm_rerank(res, n, N, nlm, alpha, beta):
    """pk_nbest_rescore_nlm on a pk_nbest array in place (nlm None: nothing) -> the extra per-hypothesis entries for _nbest_list.  The array is freed
    here when the call fails."""
    if nlm is None:
        return None
    am, ns = np.zeros((n, max(1, N)), np.float32), np.zeros((n, max(1, N)), np.float32)
    o = nlm_rescore_options(alpha, beta)
    st = lib().pk_nbest_rescore_nlm(res, n, nlm._h, C.byref(o), _f(am), _f(ns))
    if st != 0:
        try:
            check(st)
        finally:
            lib().pk_nbest_free(res, n)
    return dict(am_score=am, nlm_score=ns)


def _transcript_args(texts, ids, n):
    """the (texts, ids, id_offsets) arguments of an entry point that takes n transcripts as texts or as token id sequences"""
    assert (texts is None) != (ids is None), "texts or ids"
    if texts is not None:
        return (C.c_char_p * n)(*[t.encode() for t in texts]), None, None
    pid, poff = _pack_ids(ids)
    return None, _i(pid), _i(poff)


def _transcribe(fn, handle, clips, decoder, timestamps, boost_phrases, boost_score, with_raw=None):
    pcm, off, n = _clips(clips)
    opt = PkOptions()
    opt.decoder = {"ctc": 0, "tdt": 1}[decoder]
    opt.timestamps = 1 if timestamps else 0
    keep = (C.c_char_p * max(1, len(boost_phrases)))(*[p.encode() for p in boost_phrases])
    opt.boost_phrases = keep
    opt.n_boost_phrases = len(boost_phrases)
    opt.boost_score = boost_score
    res = C.POINTER(PkResult)()
    check(fn(handle, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(opt), C.byref(res)))
    return _result_list(res, n, [timestamps] * n, with_raw=with_raw)


class Group:
    """pk_group: one model replica per GPU of this process, utterance batches dealt round-robin, one host thread and one two-stream
    pipeline per device, no collective (include/parakeet_amd.h, "one node, several GPUs")."""

    def __init__(self, weights_path, cfg: ModelConfig, vocab_path: str = None, devices=None):
        self.cfg = cfg
        self._h = C.c_void_p()
        pc = to_pk_config(cfg)
        dev = np.ascontiguousarray(devices, np.int32) if devices is not None else None
        check(lib().pk_group_create(weights_path.encode(), vocab_path.encode() if vocab_path else None, C.byref(pc),
                                    _i(dev) if dev is not None else None, len(dev) if dev is not None else 0, C.byref(self._h)))

    def size(self):
        return lib().pk_group_size(self._h)

    def transcribe_pcm(self, clips, decoder="tdt", timestamps=False, boost_phrases=(), boost_score=5.0, verify_exchange=False):
        """verify_exchange: also run pk_group_verify_exchange (the RCCL all-reduce + all-gather of the token matrix) on the results;
        self.rccl_ranks then holds the communicator's rank count."""
        raw = None
        if verify_exchange:
            def raw(res, n):
                ranks = C.c_int(0)
                check(lib().pk_group_verify_exchange(self._h, res, n, C.byref(ranks)))
                self.rccl_ranks = ranks.value
        return _transcribe(lib().pk_group_transcribe_pcm, self._h, clips, decoder, timestamps, boost_phrases, boost_score, with_raw=raw)

    def set_attention_context(self, left, right):
        """pk_group_set_attention_context: Model.set_attention_context on every replica."""
        check(lib().pk_group_set_attention_context(self._h, int(left), int(right)))

    def set_input_rate(self, rate):
        """pk_group_set_input_rate: Model.set_input_rate on every replica."""
        check(lib().pk_group_set_input_rate(self._h, int(rate)))

    def last_stats(self):
        wall, audio = C.c_double(0), C.c_double(0)
        per = np.zeros(self.size(), np.int32)
        check(lib().pk_group_last_stats(self._h, C.byref(wall), C.byref(audio), _i(per)))
        return dict(wall_ms_max=wall.value, audio_seconds=audio.value, clips_per_rank=per.tolist())

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_group_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Thin handle over pk_model (mirrors parakeet::Transcriber's ctor + to_gpu(), transcribe.hpp:59-71)."""

    def __init__(self, weights_path, cfg: ModelConfig, vocab_path: str = None, device: int = None):
        """weights_path: a safetensors file, or its bytes (bytes / uint8 ndarray), e.g. as received from a broadcast."""
        self.cfg = cfg
        self._h = C.c_void_p()
        pc = to_pk_config(cfg)
        vp = vocab_path.encode() if vocab_path else None
        if isinstance(weights_path, str):
            check(lib().pk_model_load(weights_path.encode(), vp, C.byref(pc), C.byref(self._h)))
        else:
            img = np.frombuffer(weights_path, np.uint8) if isinstance(weights_path, (bytes, bytearray)) else np.ascontiguousarray(weights_path, np.uint8)
            L = lib()
            L.pk_model_load_buffer.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(PkConfig), C.POINTER(C.c_void_p)]
            check(L.pk_model_load_buffer(img.ctypes.data_as(C.c_void_p), img.size, vp, C.byref(pc), C.byref(self._h)))
        if device is not None:
            self.to_gpu(device)

    def to_gpu(self, device: int = 0):
        check(lib().pk_model_to_gpu(self._h, device))
        return self

    def set_attention_context(self, left, right):
        """pk_model_set_attention_context: limited-context attention over encoder frames [i - left, i + right] (NeMo's local attention
        [L, L] is (L, L)); (-1, -1) restores full attention."""
        check(lib().pk_model_set_attention_context(self._h, int(left), int(right)))

    def attention_context(self):
        l, r = C.c_int(0), C.c_int(0)
        check(lib().pk_model_get_attention_context(self._h, C.byref(l), C.byref(r)))
        return l.value, r.value

    def set_input_rate(self, rate):
        """pk_model_set_input_rate: the one-call entry points (transcribe_pcm, the n-best forms, align_pcm, tdt_align_pcm, tdt_score_pcm,
        spot_pcm) take PCM at this rate and resample it to 16 kHz on the device; 16000 (default) is the plain path."""
        check(lib().pk_model_set_input_rate(self._h, int(rate)))

    def input_rate(self):
        r = C.c_int(0)
        check(lib().pk_model_get_input_rate(self._h, C.byref(r)))
        return r.value

    def set_decode_loop(self, mode):
        """pk_model_set_decode_loop: "phases" (default) | "persistent" | "graph" -- same results, different launch structure."""
        check(lib().pk_model_set_decode_loop(self._h, {"phases": 0, "persistent": 1, "graph": 2}[mode]))

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # stage entry points ---------------------------------------------------------------------------------
    def mel(self, pcm, return_logmel=False):
        pcm = _c(pcm)
        if pcm.ndim == 1:
            pcm = pcm[None]
        B, n = pcm.shape
        nf = lib().pk_mel_num_frames(n)
        feats = np.empty((B, nf, self.cfg.mel_bins), np.float32)
        lm = np.empty((B, self.cfg.mel_bins, nf), np.float32) if return_logmel else None
        check(lib().pk_mel(self._h, _f(pcm), B, n, _f(feats), _f(lm) if return_logmel else None))
        return (feats, lm) if return_logmel else feats

    # ragged (mixed-length) forms: lists of per-clip arrays in, lists of per-clip arrays out (packed along time inside) -----------------
    def mel_ragged(self, clips, return_logmel=False):
        clips = [_c(c).ravel() for c in clips]
        off = np.zeros(len(clips) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in clips])
        pcm = np.concatenate(clips)
        nf = [lib().pk_mel_num_frames(len(c)) for c in clips]
        F = self.cfg.mel_bins
        feats = np.empty((sum(nf), F), np.float32)
        lm = np.empty(sum(nf) * F, np.float32) if return_logmel else None
        check(lib().pk_mel_ragged(self._h, _f(pcm), off.ctypes.data_as(i64p), len(clips), _f(feats), _f(lm) if return_logmel else None))
        o = np.concatenate([[0], np.cumsum(nf)])
        fl = [feats[o[i]:o[i + 1]] for i in range(len(clips))]
        if not return_logmel:
            return fl
        return fl, [lm[o[i] * F:o[i + 1] * F].reshape(F, nf[i]) for i in range(len(clips))]

    def encode_ragged(self, feats_list, stop_layer=-1, stop_stage=0):
        tm = np.asarray([f.shape[0] for f in feats_list], np.int32)
        T = [lib().pk_encoder_num_frames(int(t)) for t in tm]
        feats = _c(np.concatenate([_c(f) for f in feats_list], axis=0))
        out = np.empty((sum(T), self.cfg.hidden_size), np.float32)
        check(lib().pk_encode_ragged(self._h, _f(feats), _i(tm), len(tm), stop_layer, stop_stage, _f(out)))
        o = np.concatenate([[0], np.cumsum(T)])
        return [out[o[i]:o[i + 1]] for i in range(len(tm))]

    def conformer_blocks_ragged(self, x_list, first_layer=0, n_layers=None):
        T = np.asarray([x.shape[0] for x in x_list], np.int32)
        x = _c(np.concatenate([_c(v) for v in x_list], axis=0))
        out = np.empty_like(x)
        n = self.cfg.num_layers - first_layer if n_layers is None else n_layers
        check(lib().pk_conformer_blocks_ragged(self._h, _f(x), _i(T), len(T), first_layer, n, _f(out)))
        o = np.concatenate([[0], np.cumsum(T)])
        return [out[o[i]:o[i + 1]] for i in range(len(T))]

    def ctc_decode_ragged(self, enc_list, return_logp=False):
        T = np.asarray([e.shape[0] for e in enc_list], np.int32)
        enc = _c(np.concatenate([_c(e) for e in enc_list], axis=0))
        B, tm = len(T), int(T.max())
        ids = np.zeros((B, tm), np.int32); st = np.zeros((B, tm), np.int32); en = np.zeros((B, tm), np.int32)
        cf = np.zeros((B, tm), np.float32); lens = np.zeros(B, np.int32)
        lp = np.empty((int(T.sum()), self.cfg.ctc_vocab_size), np.float32) if return_logp else None
        check(lib().pk_ctc_decode_ragged(self._h, _f(enc), _i(T), B, _i(ids), _i(lens), _i(st), _i(en), _f(cf), _f(lp) if return_logp else None))
        r = dict(ids=ids, lens=lens, start=st, end=en, conf=cf)
        if return_logp:
            o = np.concatenate([[0], np.cumsum(T)])
            r["logp"] = [lp[o[i]:o[i + 1]] for i in range(B)]
        return r

    def tdt_decode_ragged(self, enc_list, max_tokens=None):
        T = np.asarray([e.shape[0] for e in enc_list], np.int32)
        enc = _c(np.concatenate([_c(e) for e in enc_list], axis=0))
        B = len(T)
        mt = max_tokens or int(T.max()) * self.cfg.max_symbols_per_step
        ids = np.zeros((B, mt), np.int32); st = np.zeros((B, mt), np.int32); en = np.zeros((B, mt), np.int32)
        cf = np.zeros((B, mt), np.float32); lens = np.zeros(B, np.int32); steps = np.zeros(B, np.int32)
        check(lib().pk_tdt_decode_ragged(self._h, _f(enc), _i(T), B, mt, _i(ids), _i(lens), _i(st), _i(en), _f(cf), _i(steps)))
        r = dict(ids=ids, lens=lens, start=st, end=en, conf=cf, steps=steps)
        if not getattr(self, "_boosted", False):
            mg = np.zeros(B, np.float32)
            if lib().pk_decode_margins(self._h, _f(mg), B) == 0:
                r["min_margin"] = mg
        return r

    def conv_variants(self, B=1, Tm=1, T=None, n_mel_frames=None, stream_c=0):
        """pk_diag_conv_variants: the instantiations the engine launches for this model and batch (B utterances of Tm mel frames, or of T encoder
        frames as conformer_blocks takes them, or a ragged batch of n_mel_frames[b] mel frames; stream_c: frames per streaming chunk) ->
        dict of tuples, each the row pk_diag_conv_instantiations lists for it: c1d1 (0, id, packed, XC, YS), dw2 (1, id, 0, XO, 0),
        dwconv (2, id, KC, TT, body), stream (3, id, KC, CMAX, 0) or None; rows_h2 / rows_t; stream_body (0 registers, 1 frame loop) and
        stream_fusable (the chunk may run as the preceding product's epilogue instead)."""
        out = np.zeros(CONV_VARIANT_WORDS, np.int32)
        if n_mel_frames is not None:
            tm = np.ascontiguousarray(n_mel_frames, np.int32)
            check(lib().pk_diag_conv_variants(self._h, len(tm), 0, _i(tm), int(stream_c), _i(out)))
        else:
            check(lib().pk_diag_conv_variants(self._h, int(B), int(Tm) if T is None else 8 * int(T) - 7, None, int(stream_c), _i(out)))
        v = [int(x) for x in out]
        r = dict(c1d1=(0, v[0], v[1], v[2], v[3]), rows_h2=v[4], dw2=(1, v[5], 0, v[6], 0), dwconv=(2, v[7], v[8], v[9], v[10]), rows_t=v[11],
                 stream=None, stream_body=None, stream_fusable=None)
        if stream_c > 0:
            r.update(stream=(3, v[12], v[13], v[14], 0), stream_body=v[15], stream_fusable=bool(v[16]))
        return r

    def pos_table_frames(self):
        """pk_diag_pos_table_frames: (T the fp32 relative-position tables were built for, T of the bf16 attention's set); 0 = not built yet."""
        out = np.zeros(2, np.int32)
        check(lib().pk_diag_pos_table_frames(self._h, _i(out)))
        return int(out[0]), int(out[1])

    def subsample(self, feats):
        feats = _c(feats)
        B, Tm, _ = feats.shape
        out = np.empty((B, lib().pk_encoder_num_frames(Tm), self.cfg.hidden_size), np.float32)
        check(lib().pk_subsample(self._h, _f(feats), B, Tm, _f(out)))
        return out

    def encode(self, feats, stop_layer=-1, stop_stage=0):
        feats = _c(feats)
        B, Tm, _ = feats.shape
        out = np.empty((B, lib().pk_encoder_num_frames(Tm), self.cfg.hidden_size), np.float32)
        check(lib().pk_encode(self._h, _f(feats), B, Tm, stop_layer, stop_stage, _f(out)))
        return out

    def conformer_blocks(self, x, first_layer=0, n_layers=None):
        x = _c(x)
        B, T, _ = x.shape
        out = np.empty_like(x)
        n = self.cfg.num_layers - first_layer if n_layers is None else n_layers
        check(lib().pk_conformer_blocks(self._h, _f(x), B, T, first_layer, n, _f(out)))
        return out

    # phrase boosting (reference include/parakeet/phrase_boost.hpp) ------------------------------------------
    def set_boost_tokens(self, phrases, boost_score=5.0):
        """ContextTrie::insert of each token-id sequence; an empty list switches boosting off."""
        flat = np.asarray([t for p in phrases for t in p], np.int32)
        off = np.zeros(len(phrases) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in phrases])
        check(lib().pk_set_boost_tokens(self._h, _i(flat) if len(flat) else _i(np.zeros(1, np.int32)), _i(off), len(phrases), boost_score))

    def set_boost_phrases(self, phrases, boost_score=5.0):
        """ContextTrie::build: Tokenizer::encode of each phrase (needs a vocabulary)."""
        arr = (C.c_char_p * max(1, len(phrases)))(*[p.encode() for p in phrases])
        check(lib().pk_set_boost_phrases(self._h, arr, len(phrases), boost_score))

    def boost_trie_size(self):
        return lib().pk_boost_trie_size(self._h)

    def tokenize(self, text):
        ids = np.zeros(4 * len(text.encode()) + 8, np.int32)
        n = lib().pk_tokenize(self._h, text.encode(), _i(ids), len(ids))
        return ids[:n].tolist()

    def _rows_head(self, rag, x, T):
        """the leading arguments of a stage entry point and of its _ragged form"""
        return (self._h, _f(x), _i(T), len(T)) if rag else (self._h, _f(x), x.shape[0], x.shape[1])

    def _timed_head(self, enc):
        """the leading arguments of a _timed entry point, which takes both forms (a pointer made by data_as keeps its array alive)"""
        rag, x, T = _enc_head(enc)
        return self._h, _f(x), _i(T) if rag else None, len(T), 0 if rag else x.shape[1]

    def transcribe_pcm(self, clips, decoder="tdt", timestamps=False, boost_phrases=(), boost_score=5.0, vad=None):
        """pk_transcribe_pcm: Transcriber::transcribe (transcribe.hpp:91-180) on in-memory clips -> list of dicts.
        vad (True, or a dict of pk_vad_options fields): pk_transcribe_pcm_vad, the clips cut at their pauses and only the speech transcribed
        -> (list of dicts, pieces as a list of (clip, begin, end) samples)."""
        if vad is None or vad is False:
            return _transcribe(lib().pk_transcribe_pcm, self._h, clips, decoder, timestamps, boost_phrases, boost_score)
        vo = vad_options(**(vad if isinstance(vad, dict) else {}))
        ptr, n = C.POINTER(PkVadPiece)(), C.c_int(0)

        def fn(handle, pcm, off, n_clips, opt, res):
            return lib().pk_transcribe_pcm_vad(handle, pcm, off, n_clips, opt, C.byref(vo), res, C.byref(ptr), C.byref(n))
        res = _transcribe(fn, self._h, clips, decoder, timestamps, boost_phrases, boost_score)
        return res, _vad_pieces(ptr, n.value)

    def ctc_beam_decode(self, enc, beam_width=None, token_prune=None, n_best=None, timestamps=False, lm=None, lm_alpha=None, lm_beta=None):
        """pk_ctc_beam_decode(_ragged): enc [B][T][d], or a list of [T_b][d] matrices (one packed batch) -> as ctc_beam_search.
        lm (an Lm): pk_ctc_beam_decode_lm(_ragged)."""
        o = beam_options(beam_width, token_prune, n_best, timestamps)
        L = lib()
        rag, x, T = _enc_head(enc)
        if rag:
            fn = L.pk_ctc_beam_decode_ragged if lm is None else L.pk_ctc_beam_decode_lm_ragged
        else:
            fn = L.pk_ctc_beam_decode if lm is None else L.pk_ctc_beam_decode_lm
        return _beam_call(fn, self._rows_head(rag, x, T), len(T), _tmax(rag, x, T), o, lm, lm_alpha, lm_beta)

    def tdt_beam_decode(self, enc, beam_width=None, label_prune=None, duration_prune=None, n_best=None, max_tokens=None, lm=None, lm_alpha=None,
                        lm_beta=None):
        """pk_tdt_beam_decode(_ragged): enc [B][T][d], or a list of [T_b][d] matrices (one packed batch) -> dict of ids / start / end /
        dur_idx / conf [B][N][max_tokens], lens / score [B][N], ok [B].  max_tokens None: (longest clip) * max_symbols_per_step.
        lm (an Lm): pk_tdt_beam_decode_lm(_ragged), shallow fusion with weights lm_alpha / lm_beta (None: the defaults); adds lm_score [B][N]."""
        o = tdt_beam_options(beam_width, label_prune, duration_prune, n_best)
        rag, x, T = _enc_head(enc)
        B, N = len(T), max(1, o.n_best)
        mt = int(max_tokens or int(T.max()) * self.cfg.max_symbols_per_step)
        ids = np.zeros((B, N, mt), np.int32); st = np.zeros((B, N, mt), np.int32); en = np.zeros((B, N, mt), np.int32)
        di = np.zeros((B, N, mt), np.int32); cf = np.zeros((B, N, mt), np.float32)
        lens = np.zeros((B, N), np.int32); score = np.zeros((B, N), np.float32); ok = np.zeros(B, np.int32)
        tail = (C.byref(o), mt, _i(ids), _i(lens), _f(score), _i(st), _i(en), _i(di), _f(cf), _i(ok))
        out = dict(ids=ids, lens=lens, score=score, start=st, end=en, dur_idx=di, conf=cf, ok=ok)
        L = lib()
        if lm is not None:
            lo = lm_options(lm_alpha, lm_beta)
            out["lm_score"] = np.zeros((B, N), np.float32)
            tail += (lm._h, C.byref(lo), _f(out["lm_score"]))
        if rag:
            check((L.pk_tdt_beam_decode_ragged if lm is None else L.pk_tdt_beam_decode_lm_ragged)(self._h, _f(x), _i(T), B, *tail))
        else:
            check((L.pk_tdt_beam_decode if lm is None else L.pk_tdt_beam_decode_lm)(self._h, _f(x), x.shape[0], x.shape[1], *tail))
        return out

    def tdt_beam_decode_timed(self, enc, beam_width=None, label_prune=None, duration_prune=None, n_best=None, max_tokens=None, reps=5, lm=None,
                              lm_alpha=None, lm_beta=None):
        """pk_tdt_beam_decode_timed -> (greedy TDT stage ms, beam search stage ms), HIP events, medians of reps passes.
        lm (an Lm): pk_tdt_beam_decode_lm_timed, the second stage is the fused search."""
        o = tdt_beam_options(beam_width, label_prune, duration_prune, n_best)
        rag, x, T = _enc_head(enc)
        mt = int(max_tokens or int(T.max()) * self.cfg.max_symbols_per_step)
        ms = np.zeros(2, np.float32)
        head = (self._h, _f(x), _i(T) if rag else None, len(T), 0 if rag else x.shape[1], C.byref(o), mt, reps, _f(ms))
        if lm is None:
            check(lib().pk_tdt_beam_decode_timed(*head))
        else:
            lo = lm_options(lm_alpha, lm_beta)
            check(lib().pk_tdt_beam_decode_lm_timed(*head, lm._h, C.byref(lo)))
        return float(ms[0]), float(ms[1])

    def tdt_beam_last_steps(self):
        """pk_tdt_beam_last_steps: steps the last TDT beam search of this model enqueued (fused or not, timed calls included)."""
        return int(lib().pk_tdt_beam_last_steps(self._h))

    def transcribe_nbest_tdt(self, clips, beam_width=None, label_prune=None, duration_prune=None, n_best=None, timestamps=False, lm=None, lm_alpha=None,
                             lm_beta=None, nlm=None, nlm_alpha=None, nlm_beta=None):
        """pk_transcribe_pcm_nbest_tdt: per clip a list of hypotheses through the TDT head, best first: dicts as transcribe_nbest returns them.
        lm (an Lm): pk_transcribe_pcm_nbest_tdt_lm; lists in fused order, every dict gains "lm_score".
        nlm (a NeuralLm): the lists re-ranked by pk_nbest_rescore_nlm before they are returned; every dict gains "am_score" and "nlm_score"."""
        if lm is not None and nlm is not None:
            raise ValueError("lm= and nlm= together: run the fused search, then NeuralLm.rescore on the returned lists (lm_score is in search order)")
        pcm, off, n = _clips(clips)
        o = tdt_beam_options(beam_width, label_prune, duration_prune, n_best)
        res = C.POINTER(PkNbest)()
        if lm is None:
            check(lib().pk_transcribe_pcm_nbest_tdt(self._h, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), int(timestamps), C.byref(res)))
            return _nbest_list(res, n, timestamps, _nlm_rerank(res, n, o.n_best, nlm, nlm_alpha, nlm_beta))
        lo = lm_options(lm_alpha, lm_beta)
        lms = np.zeros((n, max(1, o.n_best)), np.float32)
        check(lib().pk_transcribe_pcm_nbest_tdt_lm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), int(timestamps), C.byref(res), lm._h,
                                                   C.byref(lo), _f(lms)))
        return _nbest_list(res, n, timestamps, dict(lm_score=lms))

    def ctc_align_decode(self, enc, ids, total=True):
        """pk_ctc_align_decode(_ragged): enc [B][T][d], or a list of [T_b][d] matrices (one packed batch) -> as ctc_align."""
        rag, x, T = _enc_head(enc)
        return _align_call(lib().pk_ctc_align_decode_ragged if rag else lib().pk_ctc_align_decode, self._rows_head(rag, x, T), ids, total)

    def ctc_align_decode_timed(self, enc, ids, total=False, reps=5):
        """pk_ctc_align_decode_timed -> (CTC stage ms, alignment stage ms), HIP events, medians of reps passes."""
        pid, poff = _pack_ids(ids)
        ms = np.zeros(2, np.float32)
        check(lib().pk_ctc_align_decode_timed(*self._timed_head(enc), _i(pid), _i(poff), int(total), reps, _f(ms)))
        return float(ms[0]), float(ms[1])

    def align(self, clips, texts=None, ids=None, total=True):
        """pk_align_pcm: the clips (list, or packed (pcm, offsets)) against their transcripts, given as texts (needs the vocabulary) or as
        token id sequences -> list of dicts as transcribe_pcm(timestamps=True) returns them + "score", "ok" (and "total"); a clip that
        cannot be aligned has ok = 0 and no timestamp entries."""
        pcm, off, n = _clips(clips)
        sc = np.zeros(n, np.float32); tt = np.zeros(n, np.float32); ok = np.zeros(n, np.int32)
        res = C.POINTER(PkResult)()
        check(lib().pk_align_pcm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, *_transcript_args(texts, ids, n), C.byref(res), _f(sc),
                                 _f(tt) if total else None, _i(ok)))
        out = _result_list(res, n, ok)
        for i, d in enumerate(out):
            d.update(score=float(sc[i]), ok=int(ok[i]))
            if total:
                d["total"] = float(tt[i])
        return out

    def tdt_align_decode(self, enc, ids):
        """pk_tdt_align_decode(_ragged): enc [B][T][d], or a list of [T_b][d] matrices (one packed batch); ids: one token sequence per
        utterance -> as capi.tdt_align."""
        rag, x, T = _enc_head(enc)
        pid, off = _pack_ids(ids)
        if rag:
            return _tdt_align_call(lib().pk_tdt_align_decode_ragged, (self._h, _f(x), _i(T), len(T), _i(pid)), off)
        return _tdt_align_call(lib().pk_tdt_align_decode, (self._h, _f(x), x.shape[0], x.shape[1], _i(pid)), off)

    def tdt_align_decode_timed(self, enc, ids, reps=5):
        """pk_tdt_align_decode_timed -> (prediction net ms, lattice ms, walk ms, heads product of one chunk alone ms), HIP events, medians of
        reps passes."""
        rag, x, T = _enc_head(enc)
        pid, off = _pack_ids(ids)
        ms = np.zeros(4, np.float32)
        check(lib().pk_tdt_align_decode_timed(self._h, _f(x), _i(T) if rag else None, len(T), 0 if rag else x.shape[1], _i(pid), _i(off), reps, _f(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2]), float(ms[3])

    def tdt_lattice(self, enc, ids, chunk_rows=0):
        """pk_diag_tdt_lattice: enc a list of [T_b][d] matrices (or [B][T][d]) -> list of dicts lab [T][U], blk [T][U+1], dl [T][U+1][D], and
        "guard": the three buffers' words past the written extent as uint32 (the fill pattern 0x7FC5A5A5 when nothing wrote there)."""
        _, x, T = _enc_head(enc)
        pid, off = _pack_ids(ids)
        U = np.diff(off).astype(np.int64)
        D = len(self.cfg.durations)
        cells, labs = int((T * (U + 1)).sum()), int((T * U).sum())
        G = TDT_LATTICE_GUARD
        lab = np.zeros(labs + G, np.float32); blk = np.zeros(cells + G, np.float32); dl = np.zeros(cells * D + G, np.float32)
        check(lib().pk_diag_tdt_lattice(self._h, _f(x), _i(T), len(T), _i(pid), _i(off), int(chunk_rows), _f(lab), _f(blk), _f(dl)))
        out, c0, l0 = [], 0, 0
        for b in range(len(T)):
            t, u = int(T[b]), int(U[b])
            out.append(dict(lab=lab[l0:l0 + t * u].reshape(t, u).copy(), blk=blk[c0:c0 + t * (u + 1)].reshape(t, u + 1).copy(),
                            dl=dl[c0 * D:(c0 + t * (u + 1)) * D].reshape(t, u + 1, D).copy()))
            c0 += t * (u + 1); l0 += t * u
        guard = np.concatenate([lab[labs:], blk[cells:], dl[cells * D:]]).view(np.uint32)
        return out, guard

    def align_tdt(self, clips, texts=None, ids=None):
        """pk_tdt_align_pcm: Model.align through the TDT head (no CTC head needed) -> list of dicts as align() returns them, without "total"."""
        pcm, off, n = _clips(clips)
        sc = np.zeros(n, np.float32); ok = np.zeros(n, np.int32)
        res = C.POINTER(PkResult)()
        check(lib().pk_tdt_align_pcm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, *_transcript_args(texts, ids, n), C.byref(res), _f(sc), _i(ok)))
        out = _result_list(res, n, ok)
        for i, d in enumerate(out):
            d.update(score=float(sc[i]), ok=int(ok[i]))
        return out

    def _total_args(self, enc, ids, clip_of):
        rag, x, T = _enc_head(enc)
        pid, off = _pack_ids(ids)
        co = None if clip_of is None else np.ascontiguousarray(clip_of, np.int32)
        return rag, x, T, pid, off, co

    def tdt_total_decode(self, enc, ids, clip_of=None):
        """pk_tdt_total_decode(_ragged): enc [n_clips][T][d] or a list of [T_c][d] matrices; ids: one token sequence per hypothesis;
        clip_of[h]: the clip hypothesis h is scored on (None: hypothesis h on clip h) -> list of dicts total, ok."""
        rag, x, T, pid, off, co = self._total_args(enc, ids, clip_of)
        n = len(off) - 1
        tt = np.zeros(n, np.float32); ok = np.zeros(n, np.int32)
        tail = (_i(pid), _i(off), _i(co) if co is not None else None, n, _f(tt), _i(ok))
        if rag:
            check(lib().pk_tdt_total_decode_ragged(self._h, _f(x), _i(T), len(T), *tail))
        else:
            check(lib().pk_tdt_total_decode(self._h, _f(x), x.shape[0], x.shape[1], *tail))
        return [dict(total=tt[b], ok=int(ok[b])) for b in range(n)]

    def tdt_total_decode_timed(self, enc, ids, clip_of=None, reps=5):
        """pk_tdt_total_decode_timed -> (prediction net ms, lattice ms, forward pass ms), HIP events, medians of reps passes."""
        rag, x, T, pid, off, co = self._total_args(enc, ids, clip_of)
        ms = np.zeros(3, np.float32)
        check(lib().pk_tdt_total_decode_timed(self._h, _f(x), _i(T) if rag else None, len(T), 0 if rag else x.shape[1], _i(pid), _i(off),
                                              _i(co) if co is not None else None, len(off) - 1, reps, _f(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def score_tdt(self, clips, texts=None, ids=None, clip_of=None):
        """pk_tdt_score_pcm: the TDT log-likelihood of one or more transcripts per clip (texts need the vocabulary) -> list of dicts total, ok."""
        pcm, off, n_clips = _clips(clips)
        n = len(texts) if texts is not None else len(ids)
        co = None if clip_of is None else np.ascontiguousarray(clip_of, np.int32)
        tt = np.zeros(n, np.float32); ok = np.zeros(n, np.int32)
        check(lib().pk_tdt_score_pcm(self._h, _f(pcm), off.ctypes.data_as(i64p), n_clips, *_transcript_args(texts, ids, n),
                                     _i(co) if co is not None else None, n, _f(tt), _i(ok)))
        return [dict(total=tt[b], ok=int(ok[b])) for b in range(n)]

    def transcribe_nbest_rescored(self, clips, beam_width=None, token_prune=None, n_best=None, timestamps=False, tdt_weight=0.5):
        """pk_transcribe_pcm_nbest_rescored: transcribe_nbest re-ranked by the TDT head: per clip a list of dicts as transcribe_nbest returns
        them, "score" the combined value, + "ctc_score" and "tdt_total"."""
        pcm, off, n = _clips(clips)
        o = beam_options(beam_width, token_prune, n_best, timestamps)
        ro = PkRescoreOptions(float(tdt_weight))
        N = max(1, o.n_best)
        cs = np.zeros((n, N), np.float32); tt = np.zeros((n, N), np.float32)
        res = C.POINTER(PkNbest)()
        check(lib().pk_transcribe_pcm_nbest_rescored(self._h, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), C.byref(ro), C.byref(res), _f(cs), _f(tt)))
        return _nbest_list(res, n, timestamps, dict(ctc_score=cs, tdt_total=tt))

    def ctc_kws_decode(self, enc, keywords, max_hits=None, min_score=None):
        """pk_ctc_kws_decode(_ragged): enc [B][T][d], or a list of [T_b][d] matrices (one packed batch) -> as ctc_kws."""
        o = kws_options(max_hits, min_score)
        rag, x, T = _enc_head(enc)
        return _kws_call(lib().pk_ctc_kws_decode_ragged if rag else lib().pk_ctc_kws_decode, self._rows_head(rag, x, T), len(T), keywords, o)

    def ctc_kws_decode_timed(self, enc, keywords, max_hits=None, min_score=None, reps=5):
        """pk_ctc_kws_decode_timed -> (CTC stage ms, spotting stage ms), HIP events, medians of reps passes."""
        o = kws_options(max_hits, min_score)
        pid, poff = _pack_ids(keywords)
        ms = np.zeros(2, np.float32)
        check(lib().pk_ctc_kws_decode_timed(*self._timed_head(enc), _i(pid), _i(poff), len(keywords), C.byref(o), reps, _f(ms)))
        return float(ms[0]), float(ms[1])

    def spot(self, clips, phrases=None, ids=None, max_hits=None, min_score=None):
        """pk_spot_pcm: every phrase (texts: needs the vocabulary; or token id sequences) searched in every clip (list, or packed
        (pcm, offsets)) -> per clip, per phrase, a list of (start_s, end_s, score), best first."""
        assert (phrases is None) != (ids is None), "phrases or ids"
        pcm, off, n = _clips(clips)
        o = kws_options(max_hits, min_score)
        K, H = len(phrases if phrases is not None else ids), max(1, o.max_hits)
        tail = _transcript_args(phrases, ids, K)
        nh = np.zeros((n, K), np.int32); st = np.zeros((n, K, H), np.float32); en = np.zeros((n, K, H), np.float32); sc = np.zeros((n, K, H), np.float32)
        check(lib().pk_spot_pcm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, *tail, K, C.byref(o), _i(nh), _f(st), _f(en), _f(sc)))
        return [[[(float(st[c, k, j]), float(en[c, k, j]), float(sc[c, k, j])) for j in range(nh[c, k])] for k in range(K)] for c in range(n)]

    def tdt_kws_decode(self, enc, keywords, max_hits=None, min_score=None):
        """pk_tdt_kws_decode(_ragged): ctc_kws_decode through the TDT head (no CTC head needed) -> as ctc_kws."""
        o = kws_options(max_hits, min_score)
        rag, x, T = _enc_head(enc)
        return _kws_call(lib().pk_tdt_kws_decode_ragged if rag else lib().pk_tdt_kws_decode, self._rows_head(rag, x, T), len(T), keywords, o)

    def tdt_kws_decode_timed(self, enc, keywords, max_hits=None, min_score=None, reps=5):
        """pk_tdt_kws_decode_timed -> (prediction net ms, lattice ms, walk + picking ms), HIP events, medians of reps passes."""
        o = kws_options(max_hits, min_score)
        pid, poff = _pack_ids(keywords)
        ms = np.zeros(3, np.float32)
        check(lib().pk_tdt_kws_decode_timed(*self._timed_head(enc), _i(pid), _i(poff), len(keywords), C.byref(o), reps, _f(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def tdt_kws_lattice(self, enc, ids, chunk_rows=0):
        """pk_diag_tdt_kws_lattice: as tdt_lattice, every dict with "top" [T][U+1] too, before the spotting's normalisation."""
        _, x, T = _enc_head(enc)
        pid, off = _pack_ids(ids)
        U = np.diff(off).astype(np.int64)
        D = len(self.cfg.durations)
        cells, labs = int((T * (U + 1)).sum()), int((T * U).sum())
        G = TDT_LATTICE_GUARD
        lab = np.zeros(labs + G, np.float32); blk = np.zeros(cells + G, np.float32); dl = np.zeros(cells * D + G, np.float32)
        top = np.zeros(cells + G, np.float32)
        check(lib().pk_diag_tdt_kws_lattice(self._h, _f(x), _i(T), len(T), _i(pid), _i(off), int(chunk_rows), _f(lab), _f(blk), _f(dl), _f(top)))
        out, c0, l0 = [], 0, 0
        for b in range(len(T)):
            t, u = int(T[b]), int(U[b])
            out.append(dict(lab=lab[l0:l0 + t * u].reshape(t, u).copy(), blk=blk[c0:c0 + t * (u + 1)].reshape(t, u + 1).copy(),
                            dl=dl[c0 * D:(c0 + t * (u + 1)) * D].reshape(t, u + 1, D).copy(), top=top[c0:c0 + t * (u + 1)].reshape(t, u + 1).copy()))
            c0 += t * (u + 1); l0 += t * u
        guard = np.concatenate([lab[labs:], blk[cells:], dl[cells * D:], top[cells:]]).view(np.uint32)
        return out, guard

    def spot_tdt(self, clips, phrases=None, ids=None, max_hits=None, min_score=None):
        """pk_tdt_spot_pcm: Model.spot through the TDT head (no CTC head needed) -> as spot()."""
        assert (phrases is None) != (ids is None), "phrases or ids"
        pcm, off, n = _clips(clips)
        o = kws_options(max_hits, min_score)
        K, H = len(phrases if phrases is not None else ids), max(1, o.max_hits)
        tail = _transcript_args(phrases, ids, K)
        nh = np.zeros((n, K), np.int32); st = np.zeros((n, K, H), np.float32); en = np.zeros((n, K, H), np.float32); sc = np.zeros((n, K, H), np.float32)
        check(lib().pk_tdt_spot_pcm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, *tail, K, C.byref(o), _i(nh), _f(st), _f(en), _f(sc)))
        return [[[(float(st[c, k, j]), float(en[c, k, j]), float(sc[c, k, j])) for j in range(nh[c, k])] for k in range(K)] for c in range(n)]

    def ctc_beam_decode_timed(self, enc, beam_width=None, token_prune=None, n_best=None, timestamps=False, reps=5, lm=None, lm_alpha=None, lm_beta=None):
        """pk_ctc_beam_decode_timed -> (greedy CTC stage ms, beam search stage ms), HIP events, medians of reps passes.
        lm (an Lm): pk_ctc_beam_decode_lm_timed, the beam stage with the fused walk."""
        o = beam_options(beam_width, token_prune, n_best, timestamps)
        ms = np.zeros(2, np.float32)
        head = (*self._timed_head(enc), C.byref(o), reps, _f(ms))
        if lm is None:
            check(lib().pk_ctc_beam_decode_timed(*head))
        else:
            lo = lm_options(lm_alpha, lm_beta)
            check(lib().pk_ctc_beam_decode_lm_timed(*head, lm._h, C.byref(lo)))
        return float(ms[0]), float(ms[1])

    def transcribe_nbest(self, clips, beam_width=None, token_prune=None, n_best=None, timestamps=False, lm=None, lm_alpha=None, lm_beta=None, nlm=None,
                         nlm_alpha=None, nlm_beta=None):
        """pk_transcribe_pcm_nbest: per clip a list of hypotheses, best first: dicts as transcribe_pcm returns them + "score".
        lm (an Lm): pk_transcribe_pcm_nbest_lm; lists in fused order, every dict gains "lm_score".
        nlm (a NeuralLm): the lists re-ranked by pk_nbest_rescore_nlm before they are returned; every dict gains "am_score" and "nlm_score"."""
        if lm is not None and nlm is not None:
            raise ValueError("lm= and nlm= together: run the fused search, then NeuralLm.rescore on the returned lists (lm_score is in search order)")
        pcm, off, n = _clips(clips)
        o = beam_options(beam_width, token_prune, n_best, timestamps)
        res = C.POINTER(PkNbest)()
        if lm is None:
            check(lib().pk_transcribe_pcm_nbest(self._h, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), C.byref(res)))
            return _nbest_list(res, n, timestamps, _nlm_rerank(res, n, o.n_best, nlm, nlm_alpha, nlm_beta))
        lo = lm_options(lm_alpha, lm_beta)
        lms = np.zeros((n, max(1, o.n_best)), np.float32)
        check(lib().pk_transcribe_pcm_nbest_lm(self._h, _f(pcm), off.ctypes.data_as(i64p), n, C.byref(o), C.byref(res), lm._h, C.byref(lo), _f(lms)))
        return _nbest_list(res, n, timestamps, dict(lm_score=lms))

    def ctc_decode(self, enc, return_logp=False):
        enc = _c(enc)
        B, T, _ = enc.shape
        ids = np.zeros((B, T), np.int32); st = np.zeros((B, T), np.int32); en = np.zeros((B, T), np.int32)
        cf = np.zeros((B, T), np.float32); lens = np.zeros(B, np.int32)
        lp = np.empty((B, T, self.cfg.ctc_vocab_size), np.float32) if return_logp else None
        check(lib().pk_ctc_decode(self._h, _f(enc), B, T, _i(ids), _i(lens), _i(st), _i(en), _f(cf), _f(lp) if return_logp else None))
        r = dict(ids=ids, lens=lens, start=st, end=en, conf=cf)
        if return_logp:
            r["logp"] = lp
        return r

    def tdt_score(self, enc, labels, dur_idx):
        """pk_tdt_score: the TDT loop on ONE utterance enc[T][d] along the given decisions -> per-step label / duration log-probs."""
        enc = _c(enc)
        lab, dur = _c(labels, np.int32), _c(dur_idx, np.int32)
        n = len(lab)
        llp = np.zeros((n, self.cfg.vocab_size), np.float32); dlp = np.zeros((n, len(self.cfg.durations)), np.float32)
        done = C.c_int(0)
        check(lib().pk_tdt_score(self._h, _f(enc), enc.shape[0], _i(lab), _i(dur), n, _f(llp), _f(dlp), C.byref(done)))
        return dict(n=done.value, label_lp=llp[:done.value], dur_lp=dlp[:done.value])

    def tdt_decode(self, enc, max_tokens=None):
        enc = _c(enc)
        B, T, _ = enc.shape
        mt = max_tokens or T * self.cfg.max_symbols_per_step
        ids = np.zeros((B, mt), np.int32); st = np.zeros((B, mt), np.int32); en = np.zeros((B, mt), np.int32)
        cf = np.zeros((B, mt), np.float32); lens = np.zeros(B, np.int32); steps = np.zeros(B, np.int32)
        check(lib().pk_tdt_decode(self._h, _f(enc), B, T, mt, _i(ids), _i(lens), _i(st), _i(en), _f(cf), _i(steps)))
        r = dict(ids=ids, lens=lens, start=st, end=en, conf=cf, steps=steps)
        if not getattr(self, "_boosted", False):
            mg = np.zeros(B, np.float32)
            if lib().pk_decode_margins(self._h, _f(mg), B) == 0:
                r["min_margin"] = mg                         # smallest top-1 / top-2 label log-prob margin per utterance
        return r


# ---- neural LM rescoring (include/parakeet_amd.h "neural LM rescoring") -------------------------------------------------
def nlm_rescore_options(alpha=None, beta=None):
    """pk_nlm_rescore_options with the header's defaults (alpha 0.5, beta 0)"""
    return PkNlmRescoreOptions(0.5 if alpha is None else alpha, 0.0 if beta is None else beta)


def nlm_config(vocab_size=0, max_positions=0, hidden_size=0, num_layers=0, num_heads=1, ffn_intermediate=0, pre_ln=True, has_final_norm=False,
               layer_norm_eps=1e-5, has_emb_norm=False, tied_head=True, bos_id=0, eos_id=-1):
    return PkNlmConfig(vocab_size, max_positions, PkTransformerConfig(hidden_size, num_layers, num_heads, ffn_intermediate, int(pre_ln),
                                                                      int(has_final_norm), layer_norm_eps), int(has_emb_norm), int(tied_head), bos_id, eos_id)


def nlm_config_infer(weights_path, prefix="", num_heads=1, pre_ln=True, bos_id=0, eos_id=-1, layer_norm_eps=1e-5):
    """pk_nlm_config_infer: what the tensor shapes determine, the rest as given.  Host only."""
    c = nlm_config(num_heads=num_heads, pre_ln=pre_ln, bos_id=bos_id, eos_id=eos_id, layer_norm_eps=layer_norm_eps)
    check(lib().pk_nlm_config_infer(weights_path.encode(), prefix.encode(), C.byref(c)))
    return c


def diag_nlm_order(am, nlm, lens, ok, alpha, beta):
    """pk_diag_nlm_order: the re-ranking rule on one list -> (order, combined by slot).  Host arithmetic only."""
    am, nlm, lens, ok = _c(am), _c(nlm), _c(lens, np.int32), _c(ok, np.int32)
    N = len(am)
    order, comb = np.zeros(max(1, N), np.int32), np.zeros(max(1, N), np.float32)
    check(lib().pk_diag_nlm_order(_f(am), _f(nlm), _i(lens), _i(ok), N, alpha, beta, _i(order), _f(comb)))
    return order[:N], comb[:N]


def diag_causal_attention(qkv, lens, n_heads, scale):
    """pk_diag_causal_attention: qkv [rows][3 d] of packed sequences -> ctx [rows + guard][d] as uint32-viewable floats (unwritten: 0x7FC5A5A5)."""
    qkv, lens = _c(qkv), _c(lens, np.int32)
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    assert rows == int(lens.sum())
    ctx = np.zeros((rows + ATT_GUARD_ROWS, d), np.float32)
    check(lib().pk_diag_causal_attention(len(lens), _i(lens), d, n_heads, scale, _f(qkv), _f(ctx)))
    return ctx


def diag_nlm_head_logp(h, W, bias, targets):
    """pk_diag_nlm_head_logp: h [rows][d], W [V][d], bias [V] or None, targets [rows] -> lp [rows + guard] (unwritten: 0x7FC5A5A5)."""
    h, W, targets = _c(h), _c(W), _c(targets, np.int32)
    bias = None if bias is None else _c(bias)
    rows, d = h.shape
    lp = np.zeros(rows + ATT_GUARD_ROWS, np.float32)
    check(lib().pk_diag_nlm_head_logp(_f(h), _f(W), _f(bias) if bias is not None else None, _i(targets), rows, W.shape[0], d, _f(lp)))
    return lp


class NeuralLm:
    """pk_nlm: a causal Transformer LM over token ids for n-best rescoring."""

    def __init__(self, weights_path, cfg, prefix="", device=0):
        lib().pk_nlm_free.restype = None
        self.cfg = cfg
        self._h = C.c_void_p()
        check(lib().pk_nlm_load(weights_path.encode(), prefix.encode(), C.byref(cfg), device, C.byref(self._h)))

    def score(self, strings, token_logp=False):
        """pk_nlm_score -> (total [n], ok [n]) and, with token_logp, per string the array of its P log-probabilities (None where ok = 0)"""
        ids, off = _pack_ids(strings)
        n = len(strings)
        total, ok = np.zeros(max(1, n), np.float32), np.zeros(max(1, n), np.int32)
        tl = np.zeros(int(off[-1]) + n + 1, np.float32)
        check(lib().pk_nlm_score(self._h, _i(ids), _i(off), n, _f(total), _i(ok), _f(tl) if token_logp else None))
        if not token_logp:
            return total[:n], ok[:n]
        end = 1 if self.cfg.eos_id >= 0 else 0
        per = [tl[off[b] + b: off[b + 1] + b + end].copy() if ok[b] else None for b in range(n)]
        return total[:n], ok[:n], per

    def score_timed(self, strings, reps=5):
        """pk_nlm_score_timed -> (embedding ms, blocks ms, head ms), HIP events, medians of reps passes"""
        ids, off = _pack_ids(strings)
        ms = np.zeros(3, np.float32)
        check(lib().pk_nlm_score_timed(self._h, _i(ids), _i(off), len(strings), reps, _f(ms)))
        return tuple(float(x) for x in ms)

    def rescore(self, nbest, alpha=None, beta=None):
        """The two-call route on lists already in Python (what transcribe_nbest* returned): pk_nlm_score on every hypothesis's ids, then the rule of
        pk_diag_nlm_order per clip -> new lists of the same dicts with "score" = combined and "am_score" / "nlm_score" added."""
        o = nlm_rescore_options(alpha, beta)
        flat = [h["token_ids"] for hyps in nbest for h in hyps]
        total, ok = self.score(flat) if flat else (np.zeros(0, np.float32), np.zeros(0, np.int32))
        out, q = [], 0
        for hyps in nbest:
            k = len(hyps)
            am = np.asarray([h["score"] for h in hyps], np.float32)
            order, comb = diag_nlm_order(am, total[q:q + k], [len(h["token_ids"]) for h in hyps], ok[q:q + k], o.alpha, o.beta)
            out.append([dict(hyps[j], score=float(comb[j]), am_score=float(am[j]), nlm_score=float(total[q + j])) for j in order])
            q += k
        return out

    def set_scratch_cap(self, nbytes):
        check(lib().pk_diag_nlm_set_scratch_cap(self._h, nbytes))

    def last_groups(self):
        return int(lib().pk_diag_nlm_groups(self._h))

    def close(self):
        if self._h:
            lib().pk_nlm_free(self._h)
            self._h = None
