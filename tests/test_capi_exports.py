"""CPU-side checks of the drop-in boundary: libparakeet_amd.so loads without a GPU, exports every symbol
include/parakeet_amd.h declares, and every compute entry point FAILS LOUDLY (no CPU fallback) when no device
is present.  No compute calls are made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

HEADER = os.path.join(ROOT, "include", "parakeet_amd.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = capi.lib()
    syms = declared_symbols()
    assert len(syms) >= 35
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, f"declared in include/parakeet_amd.h but not exported: {missing}"


def test_presets_match_reference_config_values():
    """include/parakeet/config.hpp:77-135 (the reference's ConfigPresets tests, tests/test_all.cpp:135-194)."""
    L = capi.lib()
    c = capi.PkConfig()
    capi.check(L.pk_config_preset(b"tdt-ctc-110m", C.byref(c)))
    assert (c.hidden_size, c.num_layers, c.num_heads, c.ffn_intermediate, c.mel_bins) == (512, 17, 8, 2048, 80)
    assert (c.vocab_size, c.num_lstm_layers, c.ctc_vocab_size, c.num_durations, c.blank_id) == (1025, 1, 1025, 5, 1024)
    assert list(c.durations)[:5] == [0, 1, 2, 3, 4] and c.joint_prefix == b"tdt_joint_."
    capi.check(L.pk_config_preset(b"tdt-600m", C.byref(c)))
    assert (c.hidden_size, c.num_layers, c.mel_bins, c.vocab_size, c.num_lstm_layers, c.ctc_vocab_size) == (1024, 24, 128, 8193, 2, 0)
    capi.check(L.pk_config_preset(b"rnnt-600m", C.byref(c)))
    assert (c.hidden_size, c.vocab_size, c.rnnt_head, c.num_durations) == (1024, 1025, 1, 0)
    assert L.pk_config_preset(b"nope", C.byref(c)) != 0
    for name, f in pk.PRESETS.items():
        if name == "tiny":
            continue
        capi.check(L.pk_config_preset(name.encode(), C.byref(c)))
        py = capi.to_pk_config(f())
        for fld, _ in capi.PkConfig._fields_:
            a, b = getattr(c, fld), getattr(py, fld)
            assert (list(a) == list(b)) if fld == "durations" else (a == b), (name, fld)


def test_frame_count_helpers():
    L = capi.lib()
    assert L.pk_mel_num_frames(160000) == 1001 and L.pk_mel_num_frames(480000) == 3001 and L.pk_mel_num_frames(16000) == 101
    assert L.pk_encoder_num_frames(1001) == 126 and L.pk_encoder_num_frames(3001) == 376


@pytest.mark.skipif(capi.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_is_a_loud_error(tmp_path):
    cfg = pk.make_tiny_config()
    wp = tmp_path / "t.safetensors"
    synth.save_weights(str(wp), synth.synth_weights(cfg))
    m = capi.Model(str(wp), cfg)                       # host-side load works without a GPU
    with pytest.raises(capi.PkError) as e:
        m.to_gpu(0)
    assert e.value.code == -4 and "no CPU path" in str(e.value)
    with pytest.raises(capi.PkError) as e:
        m.mel(np.zeros(16000, np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError):
        capi.diag_math("exp", [0.0])
    import tdt_decide_ref as R                        # the decision-kernel diagnostics: valid arguments, no device
    o = R.make_case(R.CASES[0])
    with pytest.raises(capi.PkError) as e:
        capi.diag_tdt_decide(o["sc"], o["logits"], o["hn"], o["cn"], o["st"])
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        capi.diag_ctc_greedy(np.zeros((4, 9), np.float32), 9, 8, B=1, T=4)
    assert e.value.code == -4
    sc = dict(B=1, W=2, K=2, Kd=1, N=1, V=5, D=2, blank=4, max_tokens=3, durations=[0, 1])       # the beam step diagnostics: valid arguments, no device
    with pytest.raises(capi.PkError) as e:
        capi.diag_tdt_beam_step(sc, capi.tdt_beam_step_state(sc, [2], 5), np.zeros((2, 7), np.float32), 0, init=True, trace=True)
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:             # the small-M GEMM diagnostics: valid arguments, no device
        capi.diag_gemm_smallm(np.zeros((4, 64), np.float32), np.zeros((16, 64), np.float32), w_sig=True, a_sigma=True)
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        capi.diag_sigma_copy(np.zeros((16, 64), np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        capi.diag_layernorm_sigma(np.zeros((2, 128), np.float32), np.ones(128, np.float32), np.zeros(128, np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:             # the tile GEMM diagnostic: valid arguments, no device
        capi.diag_gemm_tile(np.zeros((4, 96), np.float32), np.zeros((16, 96), np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:             # the small-M bf16 GEMM diagnostics: valid arguments, no device
        capi.diag_gemm_smallm_bf16(np.zeros((4, 256), np.float32), np.zeros((16, 256), np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        capi.diag_tile_copy_bf16(np.zeros((16, 32), np.float32))
    assert e.value.code == -4
    for form, pcm in (("uniform", np.zeros((2, 700), np.float32)), ("ragged", [np.zeros(700, np.float32), np.zeros(257, np.float32)]),
                      ("stream", np.zeros((2, 400), np.float32))):   # the mel front end diagnostic: valid arguments, no device
        with pytest.raises(capi.PkError) as e:
            capi.diag_mel(pcm, form, n_mels=65)
        assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:             # the LayerNorm family's diagnostic: valid arguments, no device
        capi.diag_layernorm_form("norm2", np.zeros((5, 160), np.float32), *[np.ones(160, np.float32)] * 4, mode=1, in_place=True)
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        capi.diag_layernorm_form("stats", np.zeros((5, 63), np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:             # the multi-GPU entry point as well
        capi.Group(str(wp), cfg)
    assert e.value.code == -4


def test_strict_weight_loading_errors(tmp_path):
    cfg = pk.make_tiny_config()
    with pytest.raises(capi.PkError) as e:
        capi.Model(str(tmp_path / "missing.safetensors"), cfg)
    assert e.value.code == -2 and "Cannot open weights file" in str(e.value)
    bad = tmp_path / "bad.safetensors"
    bad.write_bytes(b"\xff" * 64)
    with pytest.raises(capi.PkError):
        capi.Model(str(bad), cfg)
    wp = tmp_path / "t.safetensors"
    synth.save_weights(str(wp), synth.synth_weights(cfg))
    with pytest.raises(capi.PkError) as e:             # reference: std::runtime_error("Cannot open vocab file: ...") vocab.cpp:12-14
        capi.Model(str(wp), cfg, vocab_path=str(tmp_path / "no_vocab.txt"))
    assert "Cannot open vocab file" in str(e.value)


def test_smallm_gemm_form_table_and_argument_checks_need_no_device():
    """pk_diag_gemm_smallm_forms (what tests/test_gpu_smallm_gemm.py::test_every_form_has_a_case compares its cases with) is host arithmetic: one form
    per instantiation of the three kernels; and pk_diag_gemm_smallm refuses malformed arguments before it looks for a device."""
    every = capi.diag_gemm_smallm_forms()
    assert len(every) == 46 and len(set(every)) == 46
    chain = [f for f in every if f[0] == "chain"]
    assert {(e, r, s) for _, e, r, s, _, _ in chain} == {(e, r, s) for e in capi.EPI for r in (8, 2, 1) for s in (False, True)}
    assert all(not dw and not pre for *_, dw, pre in chain)
    assert sorted(f[1:] for f in every if f[0] == "rt2") == sorted((e, 4, True, False, False) for e in ("none", "relu", "silu", "resid"))
    ln = [f for f in every if f[0] == "ln"]
    assert {f[2] for f in ln} == {8, 16} and all(f[3] for f in ln) and "resid" not in {f[1] for f in ln}
    assert {f[1] for f in ln if f[4]} == {"glu"} and {f[1] for f in ln if f[5]} == {"silu"} and not any(f[4] and f[5] for f in ln)
    A, W = np.zeros((4, 64), np.float32), np.zeros((40, 64), np.float32)
    for bad in (dict(w_sig=True), dict(sigma_cols=8), dict(sigma_cols=48), dict(epi="resid"), dict(ldo=39), dict(out_words=4 * 40 - 1),
                dict(remap=(2, 80, 1, 2), out_words=159), dict(pre=(np.ones(64, np.float32), np.zeros(64, np.float32)))):
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm(A, W, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_smallm(np.zeros((4, 96), np.float32), np.zeros((16, 96), np.float32))
    assert e.value.code == -1


def test_tile_gemm_form_table_queries_and_argument_checks_need_no_device():
    """pk_diag_gemm_tile_forms (what tests/test_gpu_tile_gemm.py::test_every_form_has_a_case compares its cases with) and pk_diag_gemm_tile_form are host
    arithmetic: one form per instantiation launch_gemm can take, the tiles the comments of tests/test_gpu_gemm_schedule.py name for its shapes; and
    pk_diag_gemm_tile refuses what no tile kernel can do, and malformed arguments, before it looks for a device."""
    NT64, NT128, LONGK, WIDE, T128X64, T64X64 = (64, 64), (128, 128), (2, 4, 2, 1), (4, 2, 1, 2), (2, 2, 2, 1), (2, 2, 1, 1)
    four = ("none", "relu", "silu", "resid")
    want = {("nt", NT64, 2, False, 0, e) for e in four} | {("nt", NT128, 2, False, 0, "glu")}
    want |= {("pipe", LONGK, 1, False, 0 if e == "none" else 2, e) for e in four}
    want |= {("pipe", WIDE, 1, False, 2, e) for e in capi.EPI} | {("pipe", WIDE, 1, True, 2, e) for e in ("none", "relu", "silu", "glu")}
    want |= {("pipe", T128X64, 2, False, 0, e) for e in four} | {("pipe", T64X64, 2, False, 0, e) for e in four}
    every = capi.diag_gemm_tile_forms()
    assert len(every) == 26 and set(every) == want              # (no duplicates; every entry decodes to an instantiation that exists)
    q = capi.diag_gemm_tile_form
    assert q(8064, 512, 2048, epi="resid") == ("pipe", LONGK, 1, False, 2, "resid")      # fc2: the long-K single-round tile
    assert q(8064, 512, 2048) == ("pipe", LONGK, 1, False, 0, "none")                    # ... without an epilogue function: the compiler-placed loop
    assert q(8064, 2048, 512, epi="silu") == ("pipe", WIDE, 1, False, 2, "silu")         # fc1: the wide tile
    assert q(8064, 2048, 512, epi="silu", ln=True) == ("pipe", WIDE, 1, True, 2, "silu")
    assert q(8064, 512, 512, epi="resid") == ("pipe", WIDE, 1, False, 2, "resid")        # out_proj / pw2
    assert q(8064, 512, 512, epi="glu", ln=True) == ("pipe", WIDE, 1, True, 2, "glu")
    assert q(1601, 2048, 512, epi="silu") == ("pipe", WIDE, 1, False, 2, "silu")         # the smallest M past the small-M kernels
    assert q(16128, 512, 2048, epi="resid") == ("pipe", T128X64, 2, False, 0, "resid")   # fc2 at twice the rows: 504 tiles of 128 x 128 are no single round
    assert q(65536, 256, 1024) == ("pipe", WIDE, 1, False, 2, "none")
    assert q(1537, 512, 512, epi="relu")[0] == "pipe" and q(1, 5, 32) == ("nt", NT64, 2, False, 0, "none")
    for bad in (dict(M=1536, N=512, K=512), dict(M=126, N=512, K=512),                   # the small-M family
                dict(M=2000, N=64, K=48), dict(M=2000, N=64, K=80), dict(M=2000, N=64, K=16),   # K % 32 != 0
                dict(M=2000, N=64, K=96, lda=98), dict(M=2000, N=64, K=96, ldw=97), dict(M=2000, N=64, K=96, lda=101),
                dict(M=8064, N=512, K=2048, ln=True), dict(M=8064, N=512, K=512, epi="resid", ln=True), dict(M=8064, N=512, K=512, ln=True),
                dict(M=8064, N=2048, K=32, ln=True)):
        with pytest.raises(capi.PkError) as e:
            q(**bad)
        assert e.value.code == -7, bad
    for bad in (dict(M=0, N=5, K=32), dict(M=2000, N=64, K=96, lda=92), dict(M=2000, N=64, K=96, ldw=64)):
        with pytest.raises(capi.PkError) as e:
            q(**bad)
        assert e.value.code == -1, bad
    A, W = np.zeros((4, 96), np.float32), np.zeros((40, 96), np.float32)
    for bad in (dict(epi="glu", sigma_cols=16), dict(epi="resid", resid=np.zeros((4, 40), np.float32), sigma_cols=16), dict(lda=98), dict(ldw=99), dict(ln=(np.ones(96, np.float32), np.zeros(96, np.float32)))):
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_tile(A, W, **bad)
        assert e.value.code == -7, bad
    for bad in (np.zeros((4, 40), np.float32), np.zeros((4, 64), np.float32)):           # K % 32 != 0; a small-M shape
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_tile(bad, np.zeros((40, bad.shape[1]), np.float32))
        assert e.value.code == -7
    for bad in (dict(sigma_cols=8), dict(sigma_cols=48), dict(epi="resid"), dict(ldo=39), dict(out_words=4 * 40 - 1), dict(remap=(2, 80, 1, 2), out_words=159),
                dict(epi="resid", resid=np.zeros((4, 40), np.float32), ldr=36)):
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_tile(A, W, **bad)
        assert e.value.code == -1, bad


def test_bf16_tile_gemm_form_table_queries_and_refusals_need_no_device():
    """pk_diag_gemm_bf16_tile_forms (what tests/test_gpu_bf16_tile_gemm.py::test_every_form_has_a_case compares its cases with) and
    pk_diag_gemm_bf16_tile_form are host arithmetic: one form per instantiation launch_gemm_bf16 can take, the production products of tdt-600m on the forms
    gemm.hip's comments name; and both entries refuse what the launcher aborts on, and what Model::run_gemm refuses, before they look for a device."""
    R64, R128X64, R128, G192, G256 = (2, 2, 1, 1), (2, 2, 2, 1), (4, 2, 1, 2), (2, 4, 3, 2), (4, 2, 2, 4)
    four = ("none", "relu", "silu", "resid")
    want = {("reg", t, a, "lds", e) for t in (R64, R128X64, R128) for a in (False, True) for e in four} | {("reg", R128, a, "lds", "glu") for a in (False, True)}
    want |= {("glds", g, True, f, e) for g in (G192, G256) for f in ("lds", "direct", "persist") for e in ("none", "relu", "silu", "glu")}
    want |= {("glds", g, True, f, "resid") for g in (G192, G256) for f in ("lds", "resid_reg")}
    every = capi.diag_gemm_bf16_tile_forms()
    assert len(every) == 54 and set(every) == want
    q = capi.diag_gemm_bf16_tile_form
    M = 12032                                                        # tdt-600m, 32 clips of 30 s
    assert q(M, 4096, 1024, epi="silu", a16=True, fast_act=True, out_bf16=True, out_blocked=True) == ("glds", G256, True, "persist", "silu")   # fc1
    assert q(M, 1024, 4096, epi="resid", a16=True, alpha=0.5, a_blocked=True, lda=4096) == ("glds", G192, True, "resid_reg", "resid")        # fc2: one round
    assert q(M, 3072, 1024, a16=True) == ("glds", G192, True, "persist", "none")                                                            # qkv
    assert q(M, 4096, 1024, epi="silu", a16=True) == ("glds", G256, True, "lds", "silu")              # polynomial activations: the LDS epilogue
    assert q(M, 1024, 1024, epi="resid", a16=True, ldr=1025) == ("glds", G192, True, "lds", "resid")
    assert q(M, 1024, 1024, epi="silu") == ("reg", R128, False, "lds", "silu")                        # fp32 rows of A: the register-staged kernel
    assert q(2000, 512, 512, a16=True) == ("reg", R128X64, True, "lds", "none") and q(2000, 128, 512) == ("reg", R64, False, "lds", "none")
    for bad in (dict(M=M, N=4096, K=1024, epi="silu", a16=True, out_bf16=True, out_blocked=True),    # blocked rows need the register epilogue (fast_act)
                dict(M=2000, N=512, K=512, a16=True, out_bf16=True, out_blocked=True), dict(M=2000, N=512, K=512, a16=True, a_blocked=True),
                dict(M=M, N=1024, K=1024, epi="glu", a16=True, fast_act=True, out_bf16=True), dict(M=M, N=1024, K=1024, epi="resid", a16=True, out_bf16=True),
                dict(M=M, N=1024, K=1024, a16=True, out_bf16=True, sigma_cols=16), dict(M=2000, N=510, K=512, out_bf16=True, ldo=510),
                dict(M=2000, N=512, K=512, epi="glu", sigma_cols=16), dict(M=2000, N=512, K=512, epi="resid", sigma_cols=16), dict(M=128, N=512, K=512)):
        with pytest.raises(capi.PkError) as e:
            q(**bad)
        assert e.value.code == -7, bad
    for bad in (dict(M=2000, N=512, K=96), dict(M=2000, N=512, K=512, a16=True, lda=516), dict(M=2000, N=512, K=512, ldw=516), dict(M=2000, N=512, K=512, sigma_cols=8),
                dict(M=2000, N=512, K=512, ldo=500), dict(M=2000, N=512, K=512, out_words=100), dict(M=M, N=1024, K=1024, a_blocked=True),
                dict(M=M + 8, N=1024, K=1024, a16=True, fast_act=True, epi="silu", out_bf16=True, out_blocked=True, out_words=(M + 8) * 512)):   # rows rounded up to 32
        with pytest.raises(capi.PkError) as e:
            q(**bad)
        assert e.value.code == -1, bad
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_bf16_tile(np.zeros((2000, 512), np.float32), np.zeros((512, 512), np.float32), a16=True, a_blocked=True)
    assert e.value.code == -7


def test_smallm_bf16_gemm_form_table_queries_and_refusals_need_no_device():
    """pk_diag_gemm_smallm_bf16_forms (what tests/test_gpu_smallm_bf16_gemm.py::test_every_form_has_a_case compares its cases with) and
    pk_diag_gemm_smallm_bf16_form are host arithmetic: the streaming products of the 600M models (16 streams x 2 frames) on the forms gemm_smallm_bf16.hip's
    comments name; and pk_diag_gemm_smallm_bf16 refuses what the family's predicates refuse before it looks for a device."""
    for name in ("pk_diag_gemm_smallm_bf16", "pk_diag_gemm_smallm_bf16_form", "pk_diag_gemm_smallm_bf16_forms"):
        assert name in declared_symbols() and hasattr(capi.lib(), name)
    every = capi.diag_gemm_smallm_bf16_forms()
    assert len(every) == 154 and len(set(every)) == 154
    i = {n: k for k, n in enumerate(capi.SMALLM_BF16_FIELDS)}
    for f in every:
        assert f[i["steps"]] == 8 or (f[i["a16"]] and f[i["epi"]] != "glu")
        assert not (f[i["ln"]] and f[i["a16"]])
        assert f[i["rt"]] == 1 or (f[i["epi"]] != "glu" and f[i["ct"]] == 1 and f[i["rvalid"]] == 16 and not (f[i["dw"]] or f[i["al"]] or f[i["pre"]]))
        assert f[i["ct"]] == 1 or (not f[i["a16"]] and f[i["epi"]] != "glu" and f[i["rvalid"]] == 16)
        assert f[i["al"]] == (f[i["rt"]] == 1 and not f[i["a16"]] and f[i["wt"]])
        assert (not f[i["at"]] or (f[i["epi"]] == "resid" and f[i["a16"]])) and (not f[i["dw"]] or f[i["epi"]] == "glu")
        assert not f[i["pre"]] or (f[i["ln"]] and f[i["epi"]] == "silu")
    q = capi.diag_gemm_smallm_bf16_form
    assert q(32, 4096, 1024, epi="silu", ln=True, pre=True, out_bf16=True, out_t8=True, fast_act=True) == ("silu", 8, 1, 16, False, True, 2, True, False, False, True, True)   # fc1
    assert q(32, 1024, 4096, epi="resid", a16=True, a_t8=True, alpha=0.5, resid_in_place=True) == ("resid", 16, 1, 8, True, False, 1, True, False, True, False, False)        # fc2
    assert q(32, 3072, 1024, ln=True) == ("none", 8, 1, 16, False, True, 2, True, False, False, True, False)                                                                  # qkv
    assert q(32, 1024, 1024, epi="glu", ln=True, dw_c=2) == ("glu", 8, 1, 8, False, True, 1, True, True, False, True, False)                                                  # pw1 + conv tail
    assert q(128, 768, 512, a16=True) == ("none", 8, 2, 16, True, False, 1, True, False, False, False, False)
    assert q(128, 1030, 512) == ("none", 8, 2, 16, False, False, 1, False, False, False, False, False)                       # ragged N: natural weights
    for bad in (dict(M=129, N=256, K=256), dict(M=8, N=256, K=320), dict(M=8, N=256, K=256, epi="glu", out_bf16=True), dict(M=8, N=256, K=2304, ln=True),
                dict(M=8, N=240, K=512, epi="silu", ln=True, pre=True), dict(M=9, N=256, K=256, epi="glu", dw_c=3)):
        with pytest.raises(capi.PkError) as e:
            q(**bad)
        assert e.value.code == -7, bad
    with pytest.raises(capi.PkError) as e:                           # refused before a device is looked for
        capi.diag_gemm_smallm_bf16(np.zeros((8, 320), np.float32), np.zeros((16, 320), np.float32))
    assert e.value.code == -7
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_smallm_bf16(np.zeros((8, 256), np.float32), np.zeros((16, 256), np.float32), ldo=8)
    assert e.value.code == -1


def test_layernorm_form_table_queries_and_refusals_need_no_device():
    """pk_diag_layernorm_forms (what tests/test_gpu_layernorm.py::test_every_form_has_a_case compares its cases with) and pk_diag_layernorm_form_of are
    host arithmetic: three PER_LANE instantiations of every launcher, launch_layernorm's two branches listed apart; and pk_diag_layernorm_form refuses a
    row wider than the family holds, and malformed arguments, before it looks for a device."""
    for name in ("pk_diag_layernorm_form", "pk_diag_layernorm_forms", "pk_diag_layernorm_form_of"):
        assert name in declared_symbols() and hasattr(capi.lib(), name)
    every = capi.diag_layernorm_forms()
    want = {("norm", p, 1, False, batch) for p in (2, 8, 16) for batch in (False, True)}
    want |= {(l, p, 1, l == "then_stats", False) for l in ("norm2", "stats", "then_stats") for p in (2, 8, 16)}
    assert len(every) == 15 and set(every) == want
    q = capi.diag_layernorm_form_of
    assert q("norm", 4095, 128) == ("norm", 2, 1, False, False) and q("norm", 4096, 128) == ("norm", 2, 1, False, True)
    assert q("norm", 1, 129) == ("norm", 8, 1, False, False) and q("norm2", 70000, 512) == ("norm2", 8, 1, False, False)
    assert q("stats", 1, 513) == ("stats", 16, 1, False, False) and q("then_stats", 8064, 1024) == ("then_stats", 16, 1, True, False)
    x, one = np.zeros((3, 64), np.float32), np.ones(64, np.float32)
    for launcher in capi.LN_LAUNCHERS:
        with pytest.raises(capi.PkError) as e:
            q(launcher, 4, 1025)
        assert e.value.code == -7, launcher
        with pytest.raises(capi.PkError) as e:
            capi.diag_layernorm_form(launcher, np.zeros((2, 1056), np.float32), *[np.ones(1056, np.float32)] * 4)
        assert e.value.code == -7, launcher
    for bad in (dict(rows=0, d=64), dict(rows=4, d=0)):
        with pytest.raises(capi.PkError) as e:
            q("norm", **bad)
        assert e.value.code == -1, bad
    for launcher, args, kw in (("norm", (one,), {}), ("norm2", (one, one), {}), ("then_stats", (), {}),          # gamma / beta missing
                               ("stats", (), dict(mode=1)), ("then_stats", (one, one), dict(mode=2)),            # a mode the launcher does not have
                               ("norm", (one, one), dict(mode=3)), ("norm", (one, one), dict(mode=1, in_place=True)), ("stats", (), dict(in_place=True)),
                               ("norm", (one, one), dict(pad_words=0)), ("stats", (), dict(pad_words=0))):          # a buffer no longer than the rows
        with pytest.raises(capi.PkError) as e:
            capi.diag_layernorm_form(launcher, x, *args, **kw)
        assert e.value.code == -1, (launcher, kw)
    with pytest.raises(capi.PkError) as e:                           # sigma columns come in blocks of 16
        capi.diag_layernorm_form("norm", np.zeros((3, 40), np.float32), np.ones(40, np.float32), np.ones(40, np.float32), mode=2)
    assert e.value.code == -1


def test_transformer_refuses_a_hidden_size_past_the_layernorm_row_width(tmp_path):
    """hidden_size 1536 with 12 heads passes every other configuration check (a multiple of 32, head size 128): the LayerNorm kernels hold rows of at
    most 1024 columns, so it is PK_ERR_UNSUPPORTED like Model::validate_config's -- decided before a device is looked for, with or without one."""
    with pytest.raises(capi.PkError) as e:
        capi.Transformer(str(tmp_path / "none.safetensors"), "t.", 1536, 1, 12, 3072)
    assert e.value.code == -7 and "1024" in str(e.value)
    with pytest.raises(capi.PkError) as e:                           # the widest row is still a configuration the checks let through
        capi.Transformer(str(tmp_path / "none.safetensors"), "t.", 1024, 1, 8, 2048)
    assert e.value.code in (-4, -2)                                  # no device; with one: the weights file does not exist


def test_conv_variant_diagnostics_are_host_arithmetic(tmp_path):
    """pk_diag_conv_variants / pk_diag_conv_instantiations (what tests/test_gpu_conv_variants.py asks before it compares bits) need no device:
    every reported variant is a row of the list, a ragged batch of equal lengths is the uniform batch, and T describes pk_conformer_blocks' input."""
    every = capi.diag_conv_instantiations()
    assert len(every) >= 13 and len(set(every)) == len(every) and {e[0] for e in every} == {0, 1, 2, 3}
    for kc in (9, 31):
        cfg = pk.make_tiny_config(conv_kernel_size=kc)
        wp = tmp_path / f"t{kc}.safetensors"
        synth.save_weights(str(wp), synth.synth_weights(cfg))
        m = capi.Model(str(wp), cfg)
        v = m.conv_variants(B=3, Tm=203, stream_c=2)
        assert (v["rows_h2"], v["rows_t"]) == (3 * 51, 3 * 26) and v["dwconv"][2] == kc and v["stream"][2] == kc
        assert all(v[k] in every for k in ("c1d1", "dw2", "dwconv", "stream"))
        assert v == m.conv_variants(n_mel_frames=[203, 203, 203], stream_c=2)
        assert m.conv_variants(B=5, T=37)["rows_t"] == 5 * 37 and m.conv_variants(B=1, Tm=9)["stream"] is None
        assert m.conv_variants(stream_c=1, Tm=9)["stream_fusable"] == (kc == 9) and not m.conv_variants(stream_c=3, Tm=9)["stream_fusable"]
        # more rows never go back to the small-batch strips
        ys = [m.conv_variants(B=B, Tm=1001)["c1d1"][4] for B in range(1, 40)]
        tt = [m.conv_variants(B=B, Tm=1001)["dwconv"][3] for B in range(1, 40)]
        assert ys == sorted(ys) and tt == sorted(tt) and {2, 8} == set(ys) == set(tt)
        with pytest.raises(capi.PkError):
            m.conv_variants(n_mel_frames=[5, 0])
        m.close()


def test_bf16_one_form_is_one_tile_at_every_m_and_no_small_m_shape():
    """GemmArgs::one_form (the relative-position tables of the bf16 mode: rows built under one M, read under another) through the two form queries: the
    register-staged 64 x 64 tile whatever M is -- where the dispatch would take the small-M bf16 kernel, the 128 x 64 or the 128 x 128 tile --, refused by
    gemm_smallm_bf16_applies, refused with GLU.  Host arithmetic."""
    R64 = ("reg", (2, 2, 1, 1), False, "lds", "none")
    q, qs = capi.diag_gemm_bf16_tile_form, capi.diag_gemm_smallm_bf16_form
    for d in (128, 256, 512, 1024):
        for M in (1, 64, 127, 128, 129, 1023, 1024, 1025, 20001):
            assert q(M, d, d, bias=False, out_bf16=True, one_form=True) == R64, (M, d)
            assert q(M, d, d, bias=False, sigma_cols=d, one_form=True) == R64, (M, d)       # the fp32-attention table of the bf16 mode
    assert q(1025, 512, 512, bias=False, out_bf16=True) == ("reg", (2, 2, 2, 1), False, "lds", "none")
    assert q(1025, 1024, 1024, bias=False, out_bf16=True) == ("reg", (4, 2, 1, 2), False, "lds", "none")
    assert qs(127, 512, 512, bias=False, out_bf16=True)[0] == "none"
    for bad in (lambda: qs(127, 512, 512, bias=False, out_bf16=True, one_form=True), lambda: q(127, 512, 512, bias=False, out_bf16=True),
                lambda: q(2000, 512, 512, epi="glu", one_form=True)):
        with pytest.raises(capi.PkError) as e:
            bad()
        assert e.value.code == -7


def test_pos_table_diagnostic_reads_a_model_without_a_device(tmp_path):
    """pk_diag_pos_table_frames (what tests/test_gpu_call_history.py asserts after every call) reads two host integers: a model that has run nothing
    reports (0, 0), with or without a device, and null arguments are PK_ERR_INVALID."""
    assert "pk_diag_pos_table_frames" in declared_symbols() and hasattr(capi.lib(), "pk_diag_pos_table_frames")
    cfg = pk.make_tiny_config()
    wp = tmp_path / "t.safetensors"
    synth.save_weights(str(wp), synth.synth_weights(cfg))
    m = capi.Model(str(wp), cfg)
    assert m.pos_table_frames() == (0, 0)
    out = np.full(2, 7, np.int32)
    assert capi.lib().pk_diag_pos_table_frames(None, out.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert capi.lib().pk_diag_pos_table_frames(m._h, None) == -1 and out.tolist() == [7, 7]
    m.close()


def test_mel_diagnostic_refuses_before_it_looks_for_a_device():
    """pk_diag_mel (what tests/test_gpu_mel_forms.py launches the front end through) checks its arguments on the host: a clip the reflect padding
    cannot frame, a chunk shorter than one window, a bin count or buffers it cannot take are PK_ERR_INVALID with or without a device, and the
    caller's buffers stay as they were."""
    assert "pk_diag_mel" in declared_symbols()
    ok = np.zeros(700, np.float32)
    bad = [("uniform", np.zeros((1, 256), np.float32), {}), ("ragged", [ok, np.zeros(256, np.float32), ok], {}),
           ("stream", np.zeros((2, 399), np.float32), {}), ("uniform", ok, dict(n_mels=0)), ("uniform", ok, dict(n_mels=513)),
           ("uniform", ok, dict(short=(80 * 16 + 63, 5 * 80 + 64))), ("uniform", ok, dict(short=(80 * 16 + 64, 5 * 80 + 63))),
           ("stream", ok, dict(short=(2 * 80 + 63, 64))), ("stream", ok, dict(short=(2 * 80 + 64, 63)))]
    for form, pcm, kw in bad:
        lm, ft = np.full(4096, -77.25, np.float32), np.full(4096, -77.25, np.float32)
        if "short" in kw:                                           # one buffer a word short of what the launches write plus 64 spare words
            lm, ft = lm[:kw["short"][0]], ft[:kw["short"][1]]
            kw = {}
        with pytest.raises(capi.PkError) as e:
            capi.diag_mel(pcm, form, logmel=lm, feats=ft, **kw)
        assert e.value.code == -1, (form, kw)
        assert np.all(lm == np.float32(-77.25)) and np.all(ft == np.float32(-77.25))
    L = capi.lib()
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out, nf, grid = np.zeros(4096, np.float32), np.zeros(1, np.int32), np.zeros(6, np.int32)
    off = np.array([0, 700], np.int64)
    assert L.pk_diag_mel(80, 1, 0, 1, 3, f32(ok), 1, 700, None, f32(out), 4096, f32(out), 4096, i32(nf), i32(grid)) == -1       # no such form
    assert L.pk_diag_mel(80, 1, 0, 1, 1, f32(ok), 1, 700, None, f32(out), 4096, f32(out), 4096, i32(nf), i32(grid)) == -1       # ragged without offsets
    assert L.pk_diag_mel(80, 1, 0, 1, 0, f32(ok), 1, 700, off.ctypes.data_as(C.POINTER(C.c_int64)), f32(out), 4096, f32(out), 4096, i32(nf), i32(grid)) == -1
    assert L.pk_diag_mel(80, 1, 0, 1, 0, None, 1, 700, None, f32(out), 4096, f32(out), 4096, i32(nf), i32(grid)) == -1
    assert not out.any()
