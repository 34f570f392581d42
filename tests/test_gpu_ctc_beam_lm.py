"""GPU: the CTC prefix beam search with n-gram LM shallow fusion (ctc_beam_walk_kernel<true> of kernels/ctc_beam.hip) against its written
specification, tests/ctc_beam_lm_ref.py, BIT FOR BIT: token ids, lengths, score bits, lm_score bits, start / end frames and confidence
bits of every returned hypothesis.  No case is skipped or filtered: the contract is equality."""
import dataclasses
import functools

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth

import ctc_beam_lm_ref as RL
import ctc_beam_ref as R
import ngram_lm_ref as NR

pytestmark = pytest.mark.gpu

FAMILIES = ["uniform", "peaky", "ties", "repeats"]
LMS = {
    "order1": dict(order=1, density=1.0, unk=False, bos=False),
    "order3_sparse_unk": dict(order=3, density=0.5, unk=True, bos=False),
    "order5_sparse_bos": dict(order=5, density=0.5, unk=False, bos=True),
}
WEIGHTS = [(0.5, 0.0), (1.5, -0.5), (0.0, 1.0)]


@functools.lru_cache(maxsize=None)
def lm_pair(name, V):
    """(reference model, device-side model) of one synthetic ARPA text over the ids 0 .. V - 2; shared by every test that needs it."""
    text = NR.make_arpa(V, seed=V + len(name), **LMS[name])
    return NR.RefLm(text), capi.Lm.from_text(text)


def make_lp(family, T, V, rng):
    """One [T][V] fp32 log-prob matrix of the family; blank = V - 1.  (make_lp of tests/test_gpu_ctc_beam.py, restated.)"""
    blank = V - 1
    if family == "uniform":                                          # what random weights give: nearly flat rows
        return R.log_softmax32(rng.normal(size=(T, V)) * 0.05)
    if family == "peaky":                                            # one dominant symbol per frame, short runs, blank often
        x = rng.normal(size=(T, V))
        t = 0
        while t < T:
            run = int(rng.integers(1, 4))
            c = blank if rng.random() < 0.5 else int(rng.integers(0, V - 1))
            x[t:t + run, c] += 9.0
            t += run
        return R.log_softmax32(x)
    if family == "ties":                                             # exact ties on purpose: few distinct levels, duplicated columns and rows
        x = np.round(rng.normal(size=(T, V)) * 1.5) / 2.0
        x[:, 1 % (V - 1)] = x[:, 0]
        if V > 4:
            x[:, 3] = x[:, 2]
        x[:, blank] = x[:, 0]
        if T > 1:
            x[1::2] = x[0::2][: len(x[1::2])]
        return R.log_softmax32(x)
    assert family == "repeats"                                       # long runs of one token, the same token again after a blank
    x = rng.normal(size=(T, V)) * 0.5
    c = int(rng.integers(0, V - 1))
    t = 0
    while t < T:
        run = int(rng.integers(3, 12))
        x[t:t + run, c] += 6.0
        t += run
        if rng.random() < 0.6 and t < T:
            x[t, blank] += 6.0
            t += 1
        if rng.random() < 0.2:
            c = int(rng.integers(0, V - 1))
    return R.log_softmax32(x)


def assert_same(got, want, what):
    assert np.array_equal(got["lens"], want["lens"]), f"{what}: lengths {got['lens'].tolist()} vs {want['lens'].tolist()}"
    assert np.array_equal(got["ids"], want["ids"]), f"{what}: token ids"
    assert np.array_equal(G.bits(got["score"]), G.bits(want["score"])), f"{what}: score bits {got['score']} vs {want['score']}"
    assert np.array_equal(G.bits(got["lm_score"]), G.bits(want["lm_score"])), f"{what}: lm_score bits {got['lm_score']} vs {want['lm_score']}"
    assert np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]), f"{what}: start / end frames"
    assert np.array_equal(G.bits(got["conf"]), G.bits(want["conf"])), f"{what}: confidence bits"


SHAPES = [(1, 5, 8, 4, 8), (2, 5, 32, 32, 32), (31, 33, 32, 32, 32), (31, 5, 8, 16, 1), (126, 1025, 8, 16, 8), (126, 33, 2, 1, 1),
          (31, 1025, 32, 32, 1), (2, 1025, 1, 32, 1)]


@pytest.mark.parametrize("alpha,beta", WEIGHTS)
@pytest.mark.parametrize("lm_name", sorted(LMS))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T,V,W,K,N", SHAPES)
def test_fused_search_equals_reference(T, V, W, K, N, family, lm_name, alpha, beta):
    rng = np.random.default_rng(T * 1000003 + V * 101 + W * 7 + K * 3 + N + 17 * FAMILIES.index(family))
    lp = make_lp(family, T, V, rng)
    ref, lm = lm_pair(lm_name, V)
    got = capi.ctc_beam_search(lp[None], V - 1, W, K, N, timestamps=True, lm=lm, lm_alpha=alpha, lm_beta=beta)
    want = RL.search_batch_lm([lp], V - 1, ref, alpha, beta, W, K, N)
    assert_same(got, want, f"{family} {lm_name} a={alpha} b={beta} T={T} V={V} W={W} K={K} N={N}")
    no_ts = capi.ctc_beam_search(lp[None], V - 1, W, K, N, timestamps=False, lm=lm, lm_alpha=alpha, lm_beta=beta)
    assert np.array_equal(no_ts["ids"], want["ids"]) and np.array_equal(G.bits(no_ts["lm_score"]), G.bits(want["lm_score"]))


RAGGED_T = [1, 2, 13, 40, 7, 31]                                     # a subset of tests/test_gpu_ctc_beam.py's, the length-1 clip included


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("V,W,K,N,lm_name,alpha,beta", [(33, 8, 16, 8, "order3_sparse_unk", 0.5, 0.0), (5, 32, 32, 32, "order5_sparse_bos", 1.5, -0.5),
                                                        (1025, 2, 4, 1, "order1", 0.0, 1.0)])
def test_fused_search_equals_reference_ragged_batch(V, W, K, N, lm_name, alpha, beta, family):
    rng = np.random.default_rng(1000 + V + FAMILIES.index(family))
    lps = [make_lp(family, t, V, rng) for t in RAGGED_T]
    ref, lm = lm_pair(lm_name, V)
    kw = dict(timestamps=True, lm=lm, lm_alpha=alpha, lm_beta=beta)
    got = capi.ctc_beam_search(lps, V - 1, W, K, N, **kw)
    assert_same(got, RL.search_batch_lm(lps, V - 1, ref, alpha, beta, W, K, N), f"ragged {family} {lm_name} V={V} W={W} K={K} N={N}")
    for b, lp in enumerate(lps):                                     # and every utterance equals the utterance searched alone
        alone = capi.ctc_beam_search(lp[None], V - 1, W, K, N, **kw)
        t = lp.shape[0]
        for key in ("ids", "start", "end", "conf"):
            assert np.array_equal(G.bits(got[key][b, :, :t]), G.bits(alone[key][0])), f"utterance {b} {key}: packed vs alone"
        for key in ("score", "lm_score", "lens"):
            assert np.array_equal(G.bits(got[key][b]), G.bits(alone[key][0])), f"utterance {b} {key}: packed vs alone"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lm_name", sorted(LMS))
@pytest.mark.parametrize("T,V,W,K,N", [(31, 33, 32, 32, 32), (126, 1025, 8, 16, 8), (31, 5, 8, 16, 1)])
def test_zero_weights_are_the_unfused_search(T, V, W, K, N, lm_name, family):
    rng = np.random.default_rng(T + V + 31 * FAMILIES.index(family))
    lps = np.stack([make_lp(family, T, V, rng) for _ in range(2)])
    _, lm = lm_pair(lm_name, V)
    plain = capi.ctc_beam_search(lps, V - 1, W, K, N, timestamps=True)
    fused = capi.ctc_beam_search(lps, V - 1, W, K, N, timestamps=True, lm=lm, lm_alpha=0.0, lm_beta=0.0)
    for key in ("ids", "lens", "score", "start", "end", "conf"):
        assert np.array_equal(G.bits(plain[key]), G.bits(fused[key])), key
    assert not G.bits(fused["lm_score"]).any(), "lm_score is +0.0 everywhere"


def test_flip_the_model_changes_the_one_best():
    lp, blank, text, alpha, beta = RL.flip_case()
    ref = NR.RefLm(text)
    assert R.beam_search(lp, blank, 4, 2, 4)[0][0] == (0,) and RL.beam_search_lm(lp, blank, ref, alpha, beta, 4, 2, 4)[0][0] == (1,)    # by the reference first
    lm = capi.Lm.from_text(text)
    plain = capi.ctc_beam_search(lp[None], blank, 4, 2, 4, timestamps=True)
    fused = capi.ctc_beam_search(lp[None], blank, 4, 2, 4, timestamps=True, lm=lm, lm_alpha=alpha, lm_beta=beta)
    assert plain["ids"][0, 0, 0] == 0 and fused["ids"][0, 0, 0] == 1 and plain["lens"][0, 0] == fused["lens"][0, 0] == 1
    assert_same(fused, RL.search_batch_lm([lp], blank, ref, alpha, beta, 4, 2, 4), "flip case")
    lm.close()


@pytest.fixture(scope="module")
def tiny_pair(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("beam_lm_tiny"), pk.make_tiny_config(), seed=42, with_vocab=True)


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def test_model_entry_points_equal_the_search_on_the_models_logp(tiny_pair):
    W_, om, gm = tiny_pair
    cfg = om.cfg
    V = cfg.ctc_vocab_size
    assert cfg.blank_id == V - 1
    ref, lm = lm_pair("order3_sparse_unk", V)
    kw = dict(timestamps=True, lm=lm, lm_alpha=1.5, lm_beta=-0.5)
    rng = np.random.default_rng(21)
    enc = normed(rng, (2, 40, cfg.hidden_size))
    logp = gm.ctc_decode(enc, return_logp=True)["logp"]
    got = gm.ctc_beam_decode(enc, 8, 16, 4, **kw)
    assert_same(got, capi.ctc_beam_search(logp, cfg.blank_id, 8, 16, 4, **kw), "pk_ctc_beam_decode_lm vs the fused search on logp")
    assert_same(got, RL.search_batch_lm([x for x in logp], cfg.blank_id, ref, 1.5, -0.5, 8, 16, 4), "pk_ctc_beam_decode_lm vs the reference")
    plain = gm.ctc_beam_decode(enc, 8, 16, 4, timestamps=True)
    assert "lm_score" not in plain
    xs = [normed(rng, (t, cfg.hidden_size)) for t in [1, 2, 13, 40, 7, 31]]
    rl = gm.ctc_decode_ragged(xs, return_logp=True)["logp"]
    rg = gm.ctc_beam_decode(xs, 4, 8, 4, **kw)
    assert_same(rg, capi.ctc_beam_search(rl, cfg.blank_id, 4, 8, 4, **kw), "ragged fused decode vs the fused search on logp")
    a, b = gm.ctc_beam_decode_timed(enc, 8, 16, 4, reps=1, lm=lm)
    assert a > 0 and b > 0


@pytest.fixture(scope="module")
def vocab_model(tmp_path_factory):
    td = tmp_path_factory.mktemp("beam_lm_vocab")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield cfg, gm
    gm.close()


def test_transcribe_nbest_with_a_model_agrees_with_the_fused_decode(vocab_model):
    cfg, gm = vocab_model
    _, lm = lm_pair("order5_sparse_bos", cfg.ctc_vocab_size)
    clips = [synth.synth_pcm(1, n, seed=50 + i)[0] for i, n in enumerate((32000, 12345, 700, 32000))]
    res = gm.transcribe_nbest(clips, 8, 16, 4, timestamps=True, lm=lm, lm_alpha=1.5, lm_beta=-0.5)
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    n_tok = 0
    for i, hyps in enumerate(res):
        dec = gm.ctc_beam_decode(enc[i][None], 8, 16, 4, timestamps=True, lm=lm, lm_alpha=1.5, lm_beta=-0.5)
        assert 1 <= len(hyps) <= 4 and len(hyps) == int(np.sum(dec["score"][0] > -np.inf))
        for j, h in enumerate(hyps):
            n = dec["lens"][0, j]
            assert h["token_ids"] == dec["ids"][0, j, :n].tolist(), f"clip {i} hypothesis {j}: ids vs pk_ctc_beam_decode_lm"
            assert np.float32(h["score"]).view(np.uint32) == dec["score"][0, j].view(np.uint32)
            assert np.float32(h["lm_score"]).view(np.uint32) == dec["lm_score"][0, j].view(np.uint32)
            assert h["start"] == dec["start"][0, j, :n].tolist() and h["end"] == dec["end"][0, j, :n].tolist()
            n_tok += int(n)
    assert n_tok > 0, "degenerate test: no hypothesis had a token"


def test_refusals(tiny_pair, tmp_path):
    W_, om, gm = tiny_pair
    V = om.cfg.ctc_vocab_size
    _, lm = lm_pair("order1", V)
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, om.cfg.hidden_size))
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie set: refused as the unfused search refuses it
    try:
        with pytest.raises(capi.PkError) as e:
            gm.ctc_beam_decode(enc, lm=lm)
        assert e.value.code == -7 and "boost" in str(e.value)
        with pytest.raises(capi.PkError) as e:
            gm.transcribe_nbest([synth.synth_pcm(1, 16000, seed=1)[0]], lm=lm)
        assert e.value.code == -7
    finally:
        gm.set_boost_tokens([], 5.0)
    assert "lm_score" in gm.ctc_beam_decode(enc, lm=lm)              # and works again
    _, wide = lm_pair("order1", V + 4)                               # names ids >= V and the blank
    with pytest.raises(capi.PkError) as e:
        gm.ctc_beam_decode(enc, lm=wide)
    assert e.value.code == -1
    with pytest.raises(capi.PkError) as e:
        gm.ctc_beam_decode(enc, lm=lm, lm_alpha=float("nan"))
    assert e.value.code == -1
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc")      # no CTC head: refused
    Wn = {k: v for k, v in synth.synth_weights(cfg, seed=1).items() if not k.startswith("ctc_decoder_")}
    wp = str(tmp_path / "noctc.safetensors")
    synth.save_weights(wp, Wn)
    m2 = capi.Model(wp, cfg, device=0)
    with pytest.raises(capi.PkError) as e:
        m2.ctc_beam_decode(enc, lm=lm)
    assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    m2.close()
