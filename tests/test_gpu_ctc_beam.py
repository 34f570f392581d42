"""GPU: the CTC prefix beam search (kernels/ctc_beam.hip) against its written specification, tests/ctc_beam_ref.py, BIT FOR BIT:
token ids, lengths, score bits, start / end frames and confidence bits of every returned hypothesis.  No case is skipped or filtered
by a margin rule: the contract is equality."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_common as G
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = ["uniform", "peaky", "ties", "repeats", "allblank"]


def make_lp(family, T, V, rng):
    """One [T][V] fp32 log-prob matrix of the family; blank = V - 1."""
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
        x[:, 1 % (V - 1)] = x[:, 0]                                  # tokens 0 and 1 always tie: p + 0 and p + 1 score the same
        if V > 4:
            x[:, 3] = x[:, 2]
        x[:, blank] = x[:, 0]                                        # stay (by blank) ties with extending by token 0
        if T > 1:
            x[1::2] = x[0::2][: len(x[1::2])]                        # pairs of identical frames
        return R.log_softmax32(x)
    if family == "repeats":                                          # long runs of one token, the same token again after a blank
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
    x = rng.normal(size=(T, V)) * 0.1                                # allblank
    x[:, blank] += 25.0
    return R.log_softmax32(x)


def assert_same(got, want, what):
    assert np.array_equal(got["lens"], want["lens"]), f"{what}: lengths {got['lens'].tolist()} vs {want['lens'].tolist()}"
    assert np.array_equal(got["ids"], want["ids"]), f"{what}: token ids"
    assert np.array_equal(G.bits(got["score"]), G.bits(want["score"])), f"{what}: score bits {got['score']} vs {want['score']}"
    assert np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]), f"{what}: start / end frames"
    assert np.array_equal(G.bits(got["conf"]), G.bits(want["conf"])), f"{what}: confidence bits"


# (T, V, W, K, N): every T, V, W, K of the contract appears; large T is paired with a small W x K to keep the Python reference in hand
SHAPES = [
    (1, 5, 8, 4, 8), (2, 5, 32, 32, 32), (31, 33, 32, 32, 32), (31, 5, 8, 16, 1), (126, 1025, 8, 16, 8), (126, 33, 2, 1, 1),
    (376, 1025, 2, 4, 2), (376, 33, 8, 4, 1), (1500, 33, 2, 4, 1), (1500, 5, 1, 1, 1), (126, 8193, 8, 4, 1), (31, 8193, 32, 16, 32),
    (2, 1025, 1, 32, 1), (1, 8193, 2, 16, 2), (31, 1025, 32, 32, 1), (126, 5, 32, 4, 32),
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T,V,W,K,N", SHAPES)
def test_search_equals_reference_uniform_batch(T, V, W, K, N, family):
    rng = np.random.default_rng(T * 1000003 + V * 101 + W * 7 + K * 3 + N + 17 * FAMILIES.index(family))
    B = 2 if T * V <= 126 * 8193 else 1
    lps = [make_lp(family, T, V, rng) for _ in range(B)]
    got = capi.ctc_beam_search(np.stack(lps), V - 1, W, K, N, timestamps=True)
    want = R.search_batch(lps, V - 1, W, K, N)
    assert_same(got, want, f"{family} T={T} V={V} W={W} K={K} N={N}")
    assert np.all(want["lens"] <= T), "a hypothesis longer than its utterance cannot come out of the search"
    no_ts = capi.ctc_beam_search(np.stack(lps), V - 1, W, K, N, timestamps=False)   # the search itself does not depend on the alignment
    assert np.array_equal(no_ts["ids"], want["ids"]) and np.array_equal(G.bits(no_ts["score"]), G.bits(want["score"]))


# lengths as tests/test_gpu_ragged.py walks its decoders on, a length-1 clip included
RAGGED_T = [1, 2, 13, 40, 126, 7, 64, 99, 3, 126, 55, 31]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("V,W,K,N", [(33, 8, 16, 8), (1025, 2, 4, 1), (5, 32, 32, 32), (8193, 1, 1, 1)])
def test_search_equals_reference_ragged_batch(V, W, K, N, family):
    rng = np.random.default_rng(1000 + V + FAMILIES.index(family))
    lps = [make_lp(family, t, V, rng) for t in RAGGED_T]
    got = capi.ctc_beam_search(lps, V - 1, W, K, N, timestamps=True)
    want = R.search_batch(lps, V - 1, W, K, N)
    assert_same(got, want, f"ragged {family} V={V} W={W} K={K} N={N}")
    for b, lp in enumerate(lps):                                     # and every utterance equals the utterance searched alone
        alone = capi.ctc_beam_search(lp[None], V - 1, W, K, N, timestamps=True)
        t = lp.shape[0]
        for key in ("ids", "start", "end", "conf"):
            assert np.array_equal(G.bits(got[key][b, :, :t]), G.bits(alone[key][0])), f"utterance {b} {key}: packed vs alone"
        assert np.array_equal(G.bits(got["score"][b]), G.bits(alone["score"][0]))


def test_prefix_that_leaves_and_reenters_merges_by_its_string():
    lp, ev = R.find_reentry_case()
    assert lp is not None and ev, "the reference must show the event on this input"      # asserted on the CPU, by the reference
    V = lp.shape[1]
    got = capi.ctc_beam_search(lp[None], V - 1, 3, 2, 3, timestamps=True)
    assert_same(got, R.search_batch([lp], V - 1, 3, 2, 3), "re-entry case")
    for t, _ in ev:                                                  # also right after each event frame
        g = capi.ctc_beam_search(lp[None, :t + 1], V - 1, 3, 2, 3, timestamps=True)
        assert_same(g, R.search_batch([lp[:t + 1]], V - 1, 3, 2, 3), f"re-entry case cut after frame {t}")


@pytest.fixture(scope="module")
def tiny_pair(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("beam_tiny"), pk.make_tiny_config(), seed=42, with_vocab=True)


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


PEAKY_SCALE = 200.0


def test_width_one_on_peaky_rows_is_the_greedy_collapse(tiny_pair):
    """W = 1, K = 1 keeps per frame the better of "stay" and "extend by the frame's best token"; on rows with one dominant symbol that is
    the greedy path, and the best alignment of its string is the argmax path.  Peaky rows from the model itself: its CTC head on encoder
    rows scaled up, so the SAME rows go through pk_ctc_decode's collapse and through the search."""
    W_, om, gm = tiny_pair
    rng = np.random.default_rng(11)
    enc = normed(rng, (3, 60, om.cfg.hidden_size)) * np.float32(PEAKY_SCALE)
    g = gm.ctc_decode(enc, return_logp=True)
    assert np.mean(np.exp(g["logp"].max(-1)) > 0.99) > 0.9, "the premise: rows with one dominant symbol"
    got = capi.ctc_beam_search(g["logp"], om.cfg.blank_id, 1, 1, 1, timestamps=True)
    assert np.array_equal(got["lens"][:, 0], g["lens"])
    assert np.array_equal(got["ids"][:, 0], g["ids"]) and g["lens"].sum() > 10
    assert np.array_equal(got["start"][:, 0], g["start"]) and np.array_equal(got["end"][:, 0], g["end"])
    assert np.array_equal(G.bits(got["conf"][:, 0]), G.bits(g["conf"]))
    one = gm.ctc_beam_decode(enc, 1, 1, 1, timestamps=True)          # and the model entry point on the same rows
    assert_same(one, got, "pk_ctc_beam_decode, W = K = 1")


@pytest.mark.parametrize("preset", ["tiny", "110m"])
def test_beam_decode_equals_search_on_the_models_logp(preset, tiny_pair, tmp_path_factory):
    if preset == "tiny":
        W_, om, gm = tiny_pair
        T_uniform, rag_T = 40, [1, 2, 13, 40, 7, 31]
    else:
        W_, om, gm = G.make_pair(tmp_path_factory.mktemp("beam_110m"), G.one_layer_110m(1), seed=42)
        T_uniform, rag_T = 126, [126, 1, 64, 99]
    cfg = om.cfg
    rng = np.random.default_rng(21)
    enc = normed(rng, (2, T_uniform, cfg.hidden_size))
    logp = gm.ctc_decode(enc, return_logp=True)["logp"]
    got = gm.ctc_beam_decode(enc, 8, 16, 4, timestamps=True)
    assert_same(got, capi.ctc_beam_search(logp, cfg.blank_id, 8, 16, 4, timestamps=True), f"{preset}: pk_ctc_beam_decode vs the search on logp")
    assert_same(got, R.search_batch([x for x in logp], cfg.blank_id, 8, 16, 4), f"{preset}: pk_ctc_beam_decode vs the reference")
    xs = [normed(rng, (t, cfg.hidden_size)) for t in rag_T]
    rl = gm.ctc_decode_ragged(xs, return_logp=True)["logp"]
    rg = gm.ctc_beam_decode(xs, 4, 8, 4, timestamps=True)
    assert_same(rg, capi.ctc_beam_search(rl, cfg.blank_id, 4, 8, 4, timestamps=True), f"{preset}: ragged decode vs the search on logp")
    for b, x in enumerate(xs):
        alone = gm.ctc_beam_decode(x[None], 4, 8, 4, timestamps=True)
        t = x.shape[0]
        for key in ("ids", "start", "end", "conf"):
            assert np.array_equal(G.bits(rg[key][b, :, :t]), G.bits(alone[key][0])), f"{preset} clip {b} {key}: packed vs alone"
        assert np.array_equal(G.bits(rg["score"][b]), G.bits(alone["score"][0])) and np.array_equal(rg["lens"][b], alone["lens"][0])


@pytest.fixture(scope="module")
def vocab_model(tmp_path_factory):
    """A tiny model loaded WITH a vocabulary (its own handle: the shared pair of gpu_common may have been made without one)."""
    td = tmp_path_factory.mktemp("beam_vocab")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield cfg, gm
    gm.close()


def test_transcribe_nbest(vocab_model):
    cfg, gm = vocab_model
    L = capi.lib()
    clips = [synth.synth_pcm(1, n, seed=50 + i)[0] for i, n in enumerate((32000, 12345, 700, 32000))]
    res = gm.transcribe_nbest(clips, 8, 16, 4, timestamps=True)
    assert len(res) == len(clips)
    feats = gm.mel_ragged(clips)
    enc = gm.encode_ragged(feats)
    n_tok = 0
    for i, hyps in enumerate(res):
        dec = gm.ctc_beam_decode(enc[i][None], 8, 16, 4, timestamps=True)
        assert 1 <= len(hyps) <= 4
        assert len(hyps) == int(np.sum(dec["score"][0] > -np.inf))
        sc = [h["score"] for h in hyps]
        assert sc == sorted(sc, reverse=True), "scores non-increasing"
        for j, h in enumerate(hyps):
            n = dec["lens"][0, j]
            assert h["token_ids"] == dec["ids"][0, j, :n].tolist(), f"clip {i} hypothesis {j}: ids vs pk_ctc_beam_decode"
            assert np.float32(h["score"]).view(np.uint32) == dec["score"][0, j].view(np.uint32)
            assert h["start"] == dec["start"][0, j, :n].tolist() and h["end"] == dec["end"][0, j, :n].tolist()
            ids = np.asarray(h["token_ids"], np.int32)
            buf = C_buf(4096)
            assert L.pk_detokenize(gm._h, capi._i(ids) if n else None, int(n), buf, 4096) >= 0
            assert h["text"] == buf.value.decode()
            st, en = np.asarray(h["start"], np.int32), np.asarray(h["end"], np.int32)
            cf = np.asarray(h["conf"], np.float32)
            wbuf = C_buf(1 << 16)
            ws, we, wc = np.zeros(256, np.float32), np.zeros(256, np.float32), np.zeros(256, np.float32)
            nw = L.pk_group_timestamps(gm._h, capi._i(ids) if n else None, capi._i(st) if n else None, capi._i(en) if n else None,
                                       capi._f(cf) if n else None, int(n), 0, wbuf, 1 << 16, capi._f(ws), capi._f(we), capi._f(wc), 256)
            assert nw == len(h["words"])
            words = wbuf.value.decode().split("\n") if nw else []
            for k, (wd, a, b, c) in enumerate(h["words"]):
                assert wd == words[k] and np.float32(a) == ws[k] and np.float32(b) == we[k] and np.float32(c) == wc[k]
            n_tok += int(n)
    assert n_tok > 0, "degenerate test: no hypothesis had a token"


def C_buf(n):
    import ctypes
    return ctypes.create_string_buffer(n)


def test_refusals(tiny_pair, tmp_path):
    W_, om, gm = tiny_pair
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, om.cfg.hidden_size))
    for kw in (dict(beam_width=0), dict(beam_width=33), dict(token_prune=0), dict(token_prune=33), dict(beam_width=4, n_best=5)):
        with pytest.raises(capi.PkError) as e:
            gm.ctc_beam_decode(enc, **kw)
        assert e.value.code == -1 and str(e.value), kw
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie set: refused
    try:
        with pytest.raises(capi.PkError) as e:
            gm.ctc_beam_decode(enc)
        assert e.value.code == -7 and "boost" in str(e.value)
        with pytest.raises(capi.PkError) as e:
            gm.transcribe_nbest([synth.synth_pcm(1, 16000, seed=1)[0]])
        assert e.value.code == -7
    finally:
        gm.set_boost_tokens([], 5.0)
    gm.ctc_beam_decode(enc)                                          # and works again
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc")      # no CTC head: refused
    Wn = {k: v for k, v in synth.synth_weights(cfg, seed=1).items() if not k.startswith("ctc_decoder_")}
    wp = str(tmp_path / "noctc.safetensors")
    synth.save_weights(wp, Wn)
    m2 = capi.Model(wp, cfg, device=0)
    with pytest.raises(capi.PkError) as e:
        m2.ctc_beam_decode(enc)
    assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    m2.close()
    with pytest.raises(capi.PkError) as e:                            # the alignment's stated cap
        capi.ctc_beam_search(np.zeros((1, 3201, 3), np.float32), 2, 1, 1, 1, timestamps=True)
    assert e.value.code == -7
    capi.ctc_beam_search(R.log_softmax32(np.zeros((1, 3201, 3))), 2, 1, 1, 1, timestamps=False)


def test_facade_transcribe_nbest_through_the_cli(tmp_path):
    """Transcriber::transcribe_nbest compiled into examples/parakeet_cli (--beam W --nbest N --decoder ctc): the hypotheses it prints are
    those of Model.transcribe_nbest on the samples the WAV holds."""
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "parakeet_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()                                      # the CLI's Transcriber is the 17-layer preset
    wp, vp, ap = str(tmp_path / "model.safetensors"), str(tmp_path / "vocab.txt"), str(tmp_path / "clip.wav")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 48000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    want = gm.transcribe_nbest([q], 8, 16, 3)[0]
    gm.close()
    out = subprocess.run([exe, wp, ap, "--vocab", vp, "--decoder", "ctc", "--beam", "8", "--nbest", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    toks = [[int(x) for x in m.split()] for m in re.findall(r"^Tokens \(\d+\):(.*)$", out.stdout, flags=re.M)]
    scores = [float(x) for x in re.findall(r"=== Hypothesis \d+ score (\S+) ===", out.stdout)]
    assert toks == [h["token_ids"] for h in want]
    assert [np.float32(s) for s in scores] == [np.float32(h["score"]) for h in want]
    assert len(want) == 3 and sum(len(t) for t in toks) > 3
    bad = subprocess.run([exe, wp, ap, "--vocab", vp, "--beam", "8"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--beam needs the CTC decoder" in bad.stderr
