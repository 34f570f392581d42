"""Limited-context attention through the engine (pk_model_set_attention_context / pk_group_set_attention_context / the C++ facade).

(a) a window covering every utterance is bit-identical to the default mode and to the oracle (uniform, ragged, single clip = small-M sigma path);
(b) banded windows against the float64 torch restatement tests/torch_ref_local.py; (c) ragged batches clip by clip bit-identical to single
runs; (d) switching back to (-1, -1) gives a fresh model's bits; (e) a 75-minute clip, refused by full attention, transcribes in local mode;
(f) the bf16 mode within its 2e-2 max|x| bound of fp32 local mode; (g) pk_group; (h) the facade."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import gpu_common as G
import torch_ref_local as TL
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu
PK_ERR_INVALID, PK_ERR_UNSUPPORTED = -1, -7
# torch band reference vs the fp32 engine, max |diff| <= TOL * max(1, max |reference|): the order of test_reference_golden's 1e-4 for one block
TOL = 1e-4


def _model(tmp, cfg, seed):
    """(weights, weights path, oracle model, GPU model) -- a model of its own (the shared gpu_common cache must not see a local setting)"""
    import oracle
    W = synth.synth_weights(cfg, seed=seed)
    wp = os.path.join(str(tmp), f"{cfg.name}_{seed}.safetensors")
    synth.save_weights(wp, W)
    return W, wp, oracle.Model(cfg, W), capi.Model(wp, cfg, device=0)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    cfg = G.tiny()
    W, wp, om, gm = _model(tmp_path_factory.mktemp("loc_tiny"), cfg, 4242)
    yield cfg, W, wp, om, gm
    gm.close()


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    cfg = G.one_layer_110m(1)
    W, wp, om, gm = _model(tmp_path_factory.mktemp("loc_wide"), cfg, 4243)
    yield cfg, W, wp, om, gm
    gm.close()


@pytest.fixture(scope="module")
def tiny_hd128(tmp_path_factory):
    cfg = G.tiny(num_heads=1, name="tiny-hd128")
    W, wp, om, gm = _model(tmp_path_factory.mktemp("loc_hd128"), cfg, 4244)
    yield cfg, W, wp, om, gm
    gm.close()


def _feats(B, Tm, F, seed):
    return np.random.default_rng(seed).standard_normal((B, Tm, F)).astype(np.float32)


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_covering_window_bit_identical_to_default_and_oracle(which, tiny, wide):
    cfg, W, wp, om, gm = {"tiny": tiny, "wide": wide}[which]
    cases = [("uniform", _feats(3, 301, cfg.mel_bins, 1)), ("single", _feats(1, 517, cfg.mel_bins, 2))]
    ragged = [_feats(1, n, cfg.mel_bins, 3 + i)[0] for i, n in enumerate((301, 97, 517, 9))]
    try:
        for what, f in cases:
            T = capi.lib().pk_encoder_num_frames(f.shape[1])
            gm.set_attention_context(-1, -1)
            full = gm.encode(f)
            gm.set_attention_context(T - 1, T + 6)
            assert gm.attention_context() == (T - 1, T + 6)
            loc = gm.encode(f)
            G.assert_bits_equal(loc, full, f"{which} {what}: covering window vs full attention")
            G.assert_bits_equal(loc, om.encoder(f), f"{which} {what}: covering window vs oracle")
        T = max(capi.lib().pk_encoder_num_frames(r.shape[0]) for r in ragged)
        gm.set_attention_context(T + 3, T - 1)
        got = gm.encode_ragged(ragged)
        for i, r in enumerate(ragged):
            G.assert_bits_equal(got[i], om.encoder(r[None])[0], f"{which} ragged clip {i}: covering window vs oracle")
    finally:
        gm.set_attention_context(-1, -1)


@pytest.mark.parametrize("which,T,left,right", [("tiny", 1000, 16, 16), ("tiny", 2100, 64, 64), ("tiny", 3000, 70, 13),
                                                ("hd128", 1500, 64, 64), ("hd128", 2600, 70, 13), ("hd128", 1200, 16, 16)])
def test_banded_blocks_vs_torch_float64(which, T, left, right, tiny, tiny_hd128):
    cfg, W, wp, om, gm = {"tiny": tiny, "hd128": tiny_hd128}[which]
    x = np.random.default_rng(T + left).standard_normal((1, T, cfg.hidden_size)).astype(np.float32)
    try:
        gm.set_attention_context(left, right)
        got = gm.conformer_blocks(x)
    finally:
        gm.set_attention_context(-1, -1)
    want = TL.conformer_blocks(W, cfg, x, left, right)
    err = np.abs(got - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), f"max |diff| {err:.3e} vs max |x| {np.abs(want).max():.3f}"
    print(f"\n{which} T{T} L{left} R{right}: max |diff| {err:.3e}", end="")


def test_banded_encode_vs_torch_float64(tiny):
    cfg, W, wp, om, gm = tiny
    f = _feats(2, 9001, cfg.mel_bins, 9)
    try:
        gm.set_attention_context(16, 16)
        got = gm.encode(f)
    finally:
        gm.set_attention_context(-1, -1)
    want = TL.conformer_blocks(W, cfg, om.subsampling(f), 16, 16)
    err = np.abs(got - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), f"max |diff| {err:.3e}"


def test_ragged_clips_bit_identical_to_single_runs(tiny, tiny_hd128):
    for cfg, W, wp, om, gm in (tiny, tiny_hd128):
        rng = np.random.default_rng(17)
        xs = [rng.standard_normal((n, cfg.hidden_size)).astype(np.float32) for n in (700, 5, 33, 1500, 64, 129)]
        try:
            for left, right in ((16, 16), (70, 13), (0, 0)):
                gm.set_attention_context(left, right)
                got = gm.conformer_blocks_ragged(xs)
                for i, x in enumerate(xs):
                    G.assert_bits_equal(got[i], gm.conformer_blocks(x[None])[0], f"{cfg.name} ({left},{right}) ragged clip {i} vs alone")
                feats = [_feats(1, n, cfg.mel_bins, 30 + i)[0] for i, n in enumerate((4001, 301, 12))]
                enc = gm.encode_ragged(feats)
                for i, f in enumerate(feats):
                    G.assert_bits_equal(enc[i], gm.encode(f[None])[0], f"{cfg.name} ({left},{right}) ragged encode clip {i} vs alone")
        finally:
            gm.set_attention_context(-1, -1)


def test_toggle_back_is_a_fresh_model(tiny, tmp_path):
    cfg, W, wp, om, gm = tiny
    f = _feats(2, 2001, cfg.mel_bins, 21)
    fresh = capi.Model(wp, cfg, device=0)
    want = fresh.encode(f)
    fresh.close()
    gm.set_attention_context(16, 16)
    loc = gm.encode(f)
    gm.set_attention_context(-1, -1)
    assert gm.attention_context() == (-1, -1)
    G.assert_bits_equal(gm.encode(f), want, "(-1, -1) after a local window vs a fresh model")
    assert not np.array_equal(loc, want), "degenerate test: the local window changed nothing"


def test_invalid_and_too_wide_contexts_refused(tiny, tiny_hd128):
    for cfg, W, wp, om, gm in (tiny, tiny_hd128):
        for l, r in ((-1, 0), (0, -1), (-2, -2), (5, -3)):
            with pytest.raises(capi.PkError) as e:
                gm.set_attention_context(l, r)
            assert e.value.code == PK_ERR_INVALID
        span = {64: 1072, 128: 1072}[cfg.hidden_size // cfg.num_heads]
        with pytest.raises(capi.PkError, match=str(span)) as e:
            gm.set_attention_context(span // 2 + 1, span - span // 2)
        assert e.value.code == PK_ERR_UNSUPPORTED
        gm.set_attention_context(span // 2, span - span // 2)
        gm.set_attention_context(-1, -1)
        assert gm.attention_context() == (-1, -1)


def test_long_clip_75_minutes(tiny):
    cfg, W, wp, om, gm = tiny
    n = 75 * 60 * 16000
    pcm = (0.1 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    T = capi.lib().pk_encoder_num_frames(1 + n // 160)
    assert T > 56000
    with pytest.raises(capi.PkError) as e:                       # full attention: the score scratch would exceed 64 GB (existing behaviour)
        gm.transcribe_pcm([pcm], decoder="ctc")
    assert e.value.code == PK_ERR_UNSUPPORTED
    try:
        gm.set_attention_context(64, 64)
        ctc = gm.transcribe_pcm([pcm], decoder="ctc")[0]["token_ids"]
        tdt = gm.transcribe_pcm([pcm], decoder="tdt")[0]["token_ids"]
        enc = gm.encode(gm.mel(pcm[None]))
        c = gm.ctc_decode(enc)
        assert ctc == c["ids"][0, : c["lens"][0]].tolist(), "transcribe_pcm (CTC) vs ctc_decode(encode(...))"
        t = gm.tdt_decode(enc)
        assert tdt == t["ids"][0, : t["lens"][0]].tolist(), "transcribe_pcm (TDT) vs tdt_decode(encode(...))"
        x = np.random.default_rng(6).standard_normal((1, T, cfg.hidden_size)).astype(np.float32)
        got = gm.conformer_blocks(x)
    finally:
        gm.set_attention_context(-1, -1)
    want = TL.conformer_blocks(W, cfg, x, 64, 64)
    err = np.abs(got - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), f"T {T}: max |diff| {err:.3e}"


def test_bf16_mode_local_within_bound_of_fp32_local(tmp_path):
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16")      # the config of tests/test_gpu_bf16.py
    W = synth.synth_weights(cfg, seed=42)
    wp = str(tmp_path / "bf16.safetensors")
    synth.save_weights(wp, W)
    g16 = capi.Model(wp, cfg, device=0)
    g32 = capi.Model(wp, dataclasses.replace(cfg, gemm_bf16=False), device=0)
    f = _feats(2, 4001, cfg.mel_bins, 8)
    for m in (g16, g32):
        m.set_attention_context(64, 64)
    a, b = g16.encode(f), g32.encode(f)
    feats = [_feats(1, n, cfg.mel_bins, 40 + i)[0] for i, n in enumerate((4001, 301))]
    ra, rb = g16.encode_ragged(feats), g32.encode_ragged(feats)
    g16.close(); g32.close()
    for got, want, what in [(a, b, "uniform")] + [(ra[i], rb[i], f"ragged clip {i}") for i in range(2)]:
        mx = np.abs(want).max()
        assert np.abs(got - want).max() <= 2e-2 * mx, what
        assert not np.array_equal(got, want), f"{what}: degenerate test, bf16 mode equals fp32"


def test_group_matches_model(tiny):
    cfg, W, wp, om, gm = tiny
    clips = [synth.synth_pcm(1, n, seed=60 + i)[0] for i, n in enumerate((160000, 48000, 320000))]
    grp = capi.Group(wp, cfg, devices=[0])
    try:
        grp.set_attention_context(16, 16)
        gm.set_attention_context(16, 16)
        for dec in ("ctc", "tdt"):
            a = [r["token_ids"] for r in grp.transcribe_pcm(clips, decoder=dec)]
            b = [r["token_ids"] for r in gm.transcribe_pcm(clips, decoder=dec)]
            assert a == b, dec
        with pytest.raises(capi.PkError):
            grp.set_attention_context(-1, 3)
    finally:
        gm.set_attention_context(-1, -1)
        grp.close()


def test_facade_set_attention_context(tmp_path):
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "transcribe_wav")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()
    W = synth.synth_weights(cfg, seed=42)
    wp, vp, ap = str(tmp_path / "model.safetensors"), str(tmp_path / "vocab.txt"), str(tmp_path / "clip.wav")
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 96000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    full = gm.transcribe_pcm([q], decoder="tdt")[0]["token_ids"]
    gm.set_attention_context(8, 8)
    want = gm.transcribe_pcm([q], decoder="tdt")[0]["token_ids"]
    gm.close()
    out = subprocess.run([exe, wp, vp, ap, "tdt", "--local-attention", "8,8"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["token_ids"] == want
    out = subprocess.run([exe, wp, vp, ap, "tdt"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["token_ids"] == full
