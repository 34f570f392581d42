"""Batched greedy decode in the bf16 mode (kernels/decode_gemv_bf16.hip inside Model::run_tdt_loop) past one row tile: 13 encoder-like utterances
repeated with period 13 to B = 17 .. 130 (2100 on the tiny model), on three decoders -- tiny-bf16 (K = 64, heads with a padded grid), tiny-bf16 with
two LSTM layers (the fused upper-layer projection) and a one-encoder-layer 110m-bf16 (K = 640, 1030 head columns).
 * within a batch every copy of an utterance carries the same words (whatever wave, workgroup row or list position the compaction gave it);
 * with prediction-net caching switched off (pk_diag_pred_cache(0): every launch covers every row, MODE 0) the same call returns the same words --
   cached and uncached read the same enc_proj buffer and caching is specified as bit-exact;
 * the bf16 oracle's greedy decode of the 13 base utterances agrees with every row at the level of the mode's other tests (agreement >= 0.95).
Bit equality ACROSS batch sizes is deliberately not asserted: enc_proj has M = B T rows and may take a GEMM kernel with another accumulation order."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk

pytestmark = pytest.mark.gpu

P, T = 13, 40
WORDS = ("lens", "steps", "ids", "start", "end")


def enc_like(B, T, d, seed):
    x = np.random.default_rng(seed).standard_normal((B, T, d)).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def agreement(a, b):
    """1 - edit distance / length, as tests/test_gpu_bf16.py counts it"""
    n, m = len(a), len(b)
    prev = list(range(m + 1))
    for i in range(1, n + 1):
        cur = [i] + [0] * m
        for j in range(1, m + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return 1.0 - prev[m] / max(n, m, 1)


def valid(r):
    """the result words with everything behind an utterance's length cleared (the library leaves those slots as they were)"""
    keep = np.arange(r["ids"].shape[1])[None, :] < r["lens"][:, None]
    out = dict(r)
    for k in ("ids", "start", "end", "conf"):
        out[k] = np.where(keep, r[k], 0).astype(r[k].dtype)
    return out


def _models():
    return {"tiny": G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16"),
            "tiny2l": G.tiny(subsampling_channels=64, gemm_bf16=True, num_lstm_layers=2, name="tiny-bf16-2l"),
            "110m": dataclasses.replace(pk.make_110m_config(), num_layers=1, gemm_bf16=True, name="110m-1L-bf16")}


@pytest.fixture(scope="module")
def setups(tmp_path_factory):
    """model name -> (product model, base utterances, the oracle's decode of them), built on first use"""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = _models()[name]
            W, om, gm = G.make_pair(tmp_path_factory.mktemp("b16dec"), cfg, seed={"tiny": 5, "tiny2l": 6, "110m": 7}[name])
            base = enc_like(P, T, cfg.hidden_size, 31)
            o = om.tdt_greedy(base, max_steps=0)
            assert not o["overflow"]
            cache[name] = (gm, base, o)
        return cache[name]
    return get


def same_words(a, b, what):
    for k in WORDS:
        assert np.array_equal(a[k], b[k]), (what, k)
    G.assert_bits_equal(a["conf"], b["conf"], f"{what}: confidence")
    G.assert_bits_equal(a["min_margin"], b["min_margin"], f"{what}: min_margin")


@pytest.mark.parametrize("name,B", [(m, B) for m in ("tiny", "tiny2l", "110m") for B in (17, 32, 64, 65, 130)] + [("tiny", 2100)])
def test_batched_bf16_decode(setups, name, B):
    from parakeet_cpp_amd import capi
    gm, base, o = setups(name)
    idx = np.arange(B) % P
    enc = np.ascontiguousarray(base[idx])
    g = valid(gm.tdt_decode(enc))
    # within the batch: every copy equals the first copy of its utterance
    first = {k: v[idx] for k, v in g.items()}
    same_words(g, first, f"{name} B {B}: copies of an utterance")
    # against the launches that cover every row
    capi.diag_pred_cache(0)
    try:
        plain = valid(gm.tdt_decode(enc))
    finally:
        capi.diag_pred_cache(1)
    same_words(g, plain, f"{name} B {B}: cached vs every-row launches")
    # against the specification
    for b in range(B):
        u = idx[b]
        assert agreement(g["ids"][b, : g["lens"][b]].tolist(), o["ids"][u, : o["lens"][u]].tolist()) >= 0.95, (b, u)
    # degeneracy guards: tokens, blanks (rows the caching skipped), utterances that finish at different steps (partly flagged tiles)
    assert g["lens"][:P].sum() > 10, "nothing decoded"
    assert (g["steps"] - g["lens"]).sum() > 0, "no blank step: caching skipped nothing"
    n = min(B, 32)
    assert len(set(g["steps"][:n].tolist())) > 1 and len(set(g["start"][:n, 0].tolist())) > 1, "the rows of a tile would all be flagged (or all skipped) at every step"
