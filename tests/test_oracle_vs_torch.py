"""The C oracle against an independent torch-CPU restatement (the reference itself cannot be
built here: its arithmetic is the un-vendored axiom submodule).  fp32 round-off tolerances."""
import numpy as np
import pytest

import torch_ref
from parakeet_cpp_amd import synth


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("n_mels,n", [(80, 16000), (128, 24000), (80, 5433)])
def test_mel_matches_torch_stft(orc, n_mels, n, centered):
    pcm = synth.synth_pcm(1, n, seed=5)[0]
    feats, logmel = orc.mel(pcm, n_mels=n_mels, return_logmel=True, window_centered=centered)
    fb = orc.mel_filterbank(n_mels=n_mels)
    tf, tl = torch_ref.mel_features(pcm, fb, n_mels=n_mels, window_centered=centered)
    assert feats.shape == (1 + n // 160, n_mels)
    assert np.max(np.abs(logmel - tl)) < 2e-3          # log amplifies round-off in near-empty bins
    assert np.max(np.abs(feats - tf)) < 2e-3


def test_mel_window_switch_default_is_left_aligned(orc):
    """Switch A1: the reference author's check script left-aligns the window (compare_features.py:33-37); that is the default,
    torch.stft / NeMo centring is the alternative -- and the two are genuinely different features."""
    pcm = synth.synth_pcm(1, 16000, seed=6)[0]
    assert np.array_equal(orc.mel(pcm), orc.mel(pcm, window_centered=False))
    assert np.max(np.abs(orc.mel(pcm) - orc.mel(pcm, window_centered=True))) > 1e-2


def test_filterbank_matches_slaney_formula(orc):
    fb = orc.mel_filterbank(n_mels=80)
    assert fb.shape == (257, 80)
    assert np.all(fb >= 0) and np.all(fb.sum(0) > 0)
    # Slaney area normalisation: every triangle integrates to ~1 over Hz (bin width 31.25 Hz)
    area = fb.sum(0) * 31.25
    assert np.all(np.abs(area[5:] - 1.0) < 0.15)


def test_subsampling_matches_torch(orc, tiny_cfg, tiny_weights, tiny_oracle):
    feats = np.random.default_rng(0).standard_normal((2, 203, tiny_cfg.mel_bins)).astype(np.float32)
    out = tiny_oracle.subsampling(feats)
    ref = torch_ref.subsampling(tiny_weights, feats)
    assert out.shape == ref.shape == (2, 26, tiny_cfg.hidden_size)
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("stop", [1, 2, 3, 4, 0])
def test_conformer_block_matches_torch(orc, tiny_cfg, tiny_weights, tiny_oracle, stop):
    x = np.random.default_rng(1).standard_normal((2, 37, tiny_cfg.hidden_size)).astype(np.float32)
    pe = orc.pos_emb(37, tiny_cfg.hidden_size)
    out = tiny_oracle.conformer_block(1, x, pe, stop_after=stop)
    ref = torch_ref.conformer_block(tiny_weights, 1, x, pe, tiny_cfg.num_heads, stop_after=stop)
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("mel_bins", [72, 96])
def test_subsampling_matches_torch_other_widths(orc, mel_bins, C):
    """Mel widths whose subsampled widths (18 / 24 after two stride-2 stages, 9 / 12 after three) are not the 20 / 32 and 10 / 16 of the presets:
    the kernels split those rows into column chunks with a partial last chunk, so the oracle they are compared with is pinned here first."""
    from conftest import pk
    cfg = pk.make_tiny_config(mel_bins=mel_bins, subsampling_channels=C)
    W = synth.synth_weights(cfg, seed=42)
    feats = np.random.default_rng(mel_bins + C).standard_normal((2, 203, mel_bins)).astype(np.float32)
    out = orc.Model(cfg, W).subsampling(feats)
    ref = torch_ref.subsampling(W, feats)
    assert out.shape == ref.shape == (2, 26, cfg.hidden_size)
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("T", [1, 7, 16, 37])
@pytest.mark.parametrize("stop", [3, 0])
def test_conformer_block_31_taps_matches_torch(orc, stop, T):
    """conv_kernel_size = 31 (the other size the engine instantiates): after the conv module and after the whole block.  T <= 15: every window of
    31 taps hangs over both ends of the utterance."""
    from conftest import pk
    cfg = pk.make_tiny_config(conv_kernel_size=31)
    W = synth.synth_weights(cfg, seed=42)
    assert W["encoder_.layers_.1.conv_.depthwise_conv_.weight"].shape[-1] == 31
    x = np.random.default_rng(T).standard_normal((2, T, cfg.hidden_size)).astype(np.float32)
    pe = orc.pos_emb(T, cfg.hidden_size)
    out = orc.Model(cfg, W).conformer_block(1, x, pe, stop_after=stop)
    ref = torch_ref.conformer_block(W, 1, x, pe, cfg.num_heads, stop_after=stop)
    assert rel_err(out, ref) < 2e-5


def test_pos_emb_matches_numpy_float(orc):
    pe = orc.pos_emb(20, 64)
    ref = torch_ref.pos_emb(20, 64)
    assert np.max(np.abs(pe - ref)) < 1e-6


def test_encoder_ctc_tdt_match_torch(orc, tiny_cfg, tiny_weights, tiny_oracle):
    pcm = synth.synth_pcm(3, 32000, seed=9)
    feats = np.stack([orc.mel(p) for p in pcm])
    enc = tiny_oracle.encoder(feats)
    ref = torch_ref.encoder(tiny_weights, tiny_cfg, feats)
    assert rel_err(enc, ref) < 5e-5
    lp = tiny_oracle.ctc_logprobs(enc)
    assert np.max(np.abs(lp - torch_ref.ctc_logprobs(tiny_weights, enc))) < 1e-4
    r = tiny_oracle.tdt_greedy(enc, max_steps=4000)
    tids = torch_ref.tdt_greedy(tiny_weights, tiny_cfg, enc, max_steps=4000)
    assert not r["overflow"]
    for b in range(3):
        assert r["ids"][b, : r["lens"][b]].tolist() == tids[b]


def test_full_width_block_matches_torch(orc):
    """One real-size (d=512, 8 heads, ffn 2048) layer, T=126."""
    import dataclasses
    from conftest import pk
    cfg = dataclasses.replace(pk.make_110m_config(), num_layers=1)
    W = synth.synth_weights(cfg, seed=3)
    m = orc.Model(cfg, W)
    x = np.random.default_rng(2).standard_normal((1, 126, 512)).astype(np.float32)
    pe = orc.pos_emb(126, 512)
    assert rel_err(m.conformer_block(0, x, pe), torch_ref.conformer_block(W, 0, x, pe, 8)) < 2e-5


@pytest.mark.parametrize("preset,T", [("110m", 60), ("600m", 40), ("tiny", 37)])
def test_bf16_mode_block_matches_independent_torch_statement(orc, preset, T):
    """The oracle's tolerance-class mode (gemm_bf16) is the SPECIFICATION the bf16 kernels are compared with -- so it is pinned here against an
    independent statement of the same rules (tests/torch_ref.py conformer_block(bf16=True): tensor ops, torch's own bf16 rounding): which
    operands are rounded (every Linear / 1x1 conv), and for head sizes 64 (110m) / 128 (600m) the bf16 attention form (stored q / k / v / position
    table, one biased query copy + the c-vector, rounded probabilities, unrounded normaliser, stored context); head size 16 (tiny) keeps the fp32
    attention on the rounded products.  The two differ in accumulation order only: they must agree far inside the mode's own distance from
    fp32 (a last-bit difference may still flip a bf16 rounding here and there: not fp32 round-off)."""
    import dataclasses
    from conftest import pk
    base = {"110m": pk.make_110m_config, "600m": pk.make_tdt_600m_config, "tiny": pk.make_tiny_config}[preset]()
    cfg = dataclasses.replace(base, num_layers=1, gemm_bf16=True)
    W = synth.synth_weights(cfg, seed=3)
    m16, m32 = orc.Model(cfg, W), orc.Model(dataclasses.replace(cfg, gemm_bf16=False), W)
    d = cfg.hidden_size
    x = np.random.default_rng(2).standard_normal((1, T, d)).astype(np.float32)
    pe = orc.pos_emb(T, d)
    for stop in (2, 0):                                             # after the attention sub-block, and the whole block
        got = m16.conformer_block(0, x, pe, stop_after=stop)
        ref = torch_ref.conformer_block(W, 0, x, pe, cfg.num_heads, stop_after=stop, bf16=True)
        f32 = m32.conformer_block(0, x, pe, stop_after=stop)
        mx = np.abs(f32).max()
        dev, gap = np.abs(got - ref).mean() / mx, np.abs(got - f32).mean() / mx
        print(f"{preset} stop {stop}: oracle bf16 vs torch bf16 mean {dev:.2e}, max {np.abs(got - ref).max() / mx:.2e}; oracle bf16 vs fp32 mean {gap:.2e}")
        assert gap > 1e-4, "the mode must differ from fp32"
        # (measured: after the attention 2e-5 .. 6e-5 against a gap of 4e-4; after the whole block -- two more rounded products, the GLU and SiLU
        #  in between, each flip of a bf16 rounding carried on -- 1.4e-4 .. 1.8e-4 against 4.8e-4)
        assert dev < (0.25 if stop == 2 else 0.5) * gap and np.abs(got - ref).max() <= 2e-2 * mx


def test_bf16_mode_decode_matches_independent_torch_statement(orc):
    """The decode rules of the tolerance-class mode (bf16 weights of the recurrent / projection / head products, h' and z stored as bf16, the
    layer-0 input projection and the cell state fp32) against an independent torch statement, at the LOGITS: the oracle walks its own greedy
    path, the torch restatement is forced along the same decisions, and every step's label / duration log-probs must agree far inside the
    mode's own distance from fp32 (the fp32 oracle forced along the same path)."""
    import dataclasses
    from conftest import pk
    cfg = dataclasses.replace(pk.make_110m_config(), num_layers=2, gemm_bf16=True)    # (the 2-layer cut emits tokens on synthetic audio)
    W = synth.synth_weights(cfg, seed=42)
    m16, m32 = orc.Model(cfg, W), orc.Model(dataclasses.replace(cfg, gemm_bf16=False), W)
    enc = m16.encoder(orc.mel(synth.synth_pcm(1, 96000, seed=77)[0])[None])[0]
    r = m16.tdt_score(enc)                                          # its own greedy path + every step's log-probs
    assert r["n"] >= 20 and (r["labels"] != cfg.blank_id).sum() >= 5
    lab, dur = torch_ref.tdt_score(W, cfg, enc, r["labels"], r["dur_idx"], bf16=True)
    f = m32.tdt_score(enc, labels=r["labels"], dur_idx=r["dur_idx"])
    n = min(len(lab), r["n"], f["n"])
    assert n == r["n"]
    top = np.argsort(-r["label_lp"][:n], axis=1)[:, :8]              # the labels that matter: the oracle's top 8 of every step
    take = lambda a: np.take_along_axis(a[:n], top, axis=1)
    dev = max(np.abs(take(lab) - take(r["label_lp"])).max(), np.abs(dur[:n] - r["dur_lp"][:n]).max())
    gap = max(np.abs(take(f["label_lp"]) - take(r["label_lp"])).max(), np.abs(f["dur_lp"][:n] - r["dur_lp"][:n]).max())
    print(f"bf16 decode, {n} steps ({int((r['labels'] != cfg.blank_id).sum())} tokens): oracle vs torch max |dlogp| {dev:.2e}; oracle bf16 vs fp32 along the same path {gap:.2e}")
    assert gap > 1e-3 and dev < 0.4 * gap               # (measured 1.7e-3 against 7.9e-3: a flipped bf16 rounding of one h' / z element moves a logit by ~1e-3)
