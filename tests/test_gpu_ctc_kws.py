"""GPU: CTC keyword spotting (kernels/ctc_kws.hip) against its written specification, tests/ctc_kws_ref.py: scores BIT FOR BIT, spans and
counts exactly, unused slots 0 / 0 / -inf."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import gpu_common as G
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

import ctc_align_ref as A
import ctc_kws_ref as R

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)
FRAME_S = np.float32(0.08)                                          # seconds per encoder frame (the rule of the timestamps)


def same(got, want, what):
    """got: the dict of capi.ctc_kws; want: the dict of ctc_kws_ref.spot_batch"""
    assert np.array_equal(got["n_hits"], want["n_hits"]), f"{what}: n_hits\n{got['n_hits']}\nvs\n{want['n_hits']}"
    assert np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]), f"{what}: spans"
    assert np.array_equal(G.bits(got["score"]), G.bits(want["score"])), f"{what}: score bits"
    used = np.arange(got["score"].shape[2])[None, None, :] < got["n_hits"][:, :, None]
    assert np.all(got["score"][~used] == NEG) and not got["start"][~used].any() and not got["end"][~used].any(), f"{what}: unused slots"
    assert not np.any(np.signbit(got["score"][got["score"] == 0])), f"{what}: a zero score is +0.0"


def make_rows(family, T, V, rng):
    lp = A.make_lp(family, T, V, rng)
    assert np.all(np.isfinite(lp.max(axis=1))), "every row keeps a finite maximum"
    return lp


def rand_kw(rng, L, V):
    return rng.integers(0, V - 1, size=L).astype(np.int32)


@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("T", [1, 2, 7, 130])
def test_ties_and_holes_equal_the_reference(T, family):
    rng = np.random.default_rng(17 * T + (family == "holes"))
    V = 8
    lps = [make_rows(family, T, V, rng) for _ in range(2)]
    kws = [rand_kw(rng, L, V) for L in (1, 1, 2, 2, 3, 5, 8)] + [np.array([3, 3], np.int32), np.array([1, 1, 2], np.int32)]
    got = capi.ctc_kws(np.stack(lps), kws, V - 1, max_hits=4)
    want = R.spot_batch(lps, kws, V - 1, max_hits=4)
    same(got, want, f"{family} T={T}")
    if T == 130 and family == "ties":
        assert (want["score"] == 0).any() and want["n_hits"].max() == 4, "with 8 symbols exact matches and several hits do occur"
    if T == 1:
        assert np.all(want["n_hits"][:, 2:] == 0) and np.all(want["n_hits"][:, :2] <= 1)


LENGTHS = [1, 2, 3, 16, 17, 32, 33, 64]


@pytest.mark.parametrize("family,V", [("ties", 8), ("peaky", 33)])
def test_keyword_lengths_across_the_lane_boundaries(family, V):
    """One lane per token: L = 16 / 17 and 32 / 33 straddle the DPP row and the half-wave, L = 64 fills the wave."""
    rng = np.random.default_rng(64 + V)
    T = 140
    lp = make_rows(family, T, V, rng)
    kws = []
    for L in LENGTHS:
        kws.append(rand_kw(rng, L, V))                              # (V = 8: adjacent repeats are frequent)
        kws.append(np.full(L, 2, np.int32))                         # one repeated token: no skip anywhere, 2 L - 1 frames at least
        if L > 1:
            k = (np.cumsum(rng.integers(1, V - 1, size=L)) % (V - 1)).astype(np.int32)      # neighbours differ ...
            k[L // 2] = k[L // 2 - 1]                                                        # ... but for one repeat in the middle
            kws.append(k)
    got = capi.ctc_kws(lp[None], kws, V - 1, max_hits=2)
    want = R.spot_batch([lp], kws, V - 1, max_hits=2)
    same(got, want, f"{family} V={V}")
    assert want["n_hits"][0, -3] >= 1 and want["n_hits"][0, -2] >= 1, "L = 64 fits 140 frames, the repeated token (127 frames) too"
    short = capi.ctc_kws(lp[None, :63], [kws[-3], kws[-1], kws[0]], V - 1, max_hits=2)
    same(short, R.spot_batch([lp[:63]], [kws[-3], kws[-1], kws[0]], V - 1, max_hits=2), "T = 63")
    assert short["n_hits"][0, 0] == 0 and short["n_hits"][0, 1] == 0, "64 tokens cannot fit 63 frames"


RAG_T = [1, 9, 64, 65, 130]


@pytest.fixture(scope="module")
def ragged_case():
    rng = np.random.default_rng(537)
    V = 8
    lps = [make_rows("ties", t, V, rng) for t in RAG_T]
    kws = [rand_kw(rng, int(rng.integers(1, 9)), V) for _ in range(37)]
    walks = [[R.walk(lp, kw, V - 1) for kw in kws] for lp in lps]   # computed once; the options only change the picking
    return V, lps, kws, walks


@pytest.mark.parametrize("max_hits", [1, 4, 16])
@pytest.mark.parametrize("min_score", ["-inf", "zero", "mid"])
def test_ragged_batch_and_options(ragged_case, max_hits, min_score):
    V, lps, kws, walks = ragged_case
    best = np.asarray([E.max() for row in walks for E, _ in row], np.float32)
    assert (best > NEG).sum() > 50
    thr = {"-inf": NEG, "zero": np.float32(0.0), "mid": np.float32(np.median(best[best > NEG]))}[min_score]   # from the reference's own scores
    B, K = len(lps), len(kws)
    want = dict(n_hits=np.zeros((B, K), np.int32), start=np.zeros((B, K, max_hits), np.int32), end=np.zeros((B, K, max_hits), np.int32),
                score=np.full((B, K, max_hits), NEG, np.float32))
    for b in range(B):
        for k in range(K):
            want["n_hits"][b, k], want["start"][b, k], want["end"][b, k], want["score"][b, k] = R.pick(*walks[b][k], max_hits, thr)
    got = capi.ctc_kws(lps, kws, V - 1, max_hits=max_hits, min_score=float(thr))
    same(got, want, f"max_hits={max_hits} min_score={thr}")
    if min_score == "mid":
        assert 0 < (want["n_hits"] > 0).sum() < (best > NEG).sum(), "the threshold cuts some pairs and keeps some"
    if min_score == "-inf" and max_hits == 16:
        assert want["n_hits"].max() > 4 and (want["n_hits"][0] <= 1).all()
        for b, lp in enumerate(lps):                                 # packed equals alone
            alone = capi.ctc_kws(lp[None], kws, V - 1, max_hits=max_hits)
            for key in ("n_hits", "start", "end"):
                assert np.array_equal(alone[key][0], got[key][b]), f"utterance {b} alone: {key}"
            assert np.array_equal(G.bits(alone["score"][0]), G.bits(got["score"][b]))


def test_planted_keywords_score_zero_at_their_spans():
    V, blank, T = 1025, 1024, 80
    rng = np.random.default_rng(1025)
    lp = R.plant(A.make_lp("peaky", T, V, rng), [blank] * T, 0)     # the greedy path is all blank, then:
    R.plant(lp, [5, 5, 9, blank, 9, 2], 11)                         # frames 11 .. 16
    R.plant(lp, [5, 9, blank, 9, 9, 2], 50)                         # frames 50 .. 55
    kws = [np.array([5, 9, 9, 2], np.int32), np.array([5, 9], np.int32), np.array([9, 2], np.int32), np.array([700], np.int32)]
    got = capi.ctc_kws(lp[None], kws, blank, max_hits=2)
    same(got, R.spot_batch([lp], kws, blank, max_hits=2), "planted")
    hits = lambda k: [(int(got["start"][0, k, j]), int(got["end"][0, k, j]), float(got["score"][0, k, j])) for j in range(got["n_hits"][0, k])]
    assert hits(0) == [(11, 16, 0.0), (50, 55, 0.0)], "equal scores: the earlier frame first"
    assert hits(1) == [(11, 13, 0.0), (50, 51, 0.0)], "a prefix of the planted keyword"
    assert hits(2) == [(15, 16, 0.0), (53, 55, 0.0)]
    assert len(hits(3)) == 2 and all(s < 0 for _, _, s in hits(3)), "a token that was not said: the best spans, far from zero"
    assert capi.ctc_kws(lp[None], kws, blank, max_hits=2, min_score=-1.0)["n_hits"].tolist() == [[2, 2, 2, 0]]


@pytest.fixture(scope="module")
def tiny_pair(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("kws_tiny"), pk.make_tiny_config(), seed=42, with_vocab=True)


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def test_kws_decode_on_the_models_rows(tiny_pair):
    W_, om, gm = tiny_pair
    cfg = om.cfg
    rng = np.random.default_rng(31)
    enc = normed(rng, (2, 40, cfg.hidden_size)) * np.float32(200.0)  # peaky rows: the greedy output has tokens
    g = gm.ctc_decode(enc, return_logp=True)
    said = [g["ids"][b, :g["lens"][b]] for b in range(2)]
    assert min(len(x) for x in said) >= 4
    kws = [said[0][:3], said[0][2:4], said[1][:1], said[1][1:6], rand_kw(rng, 4, cfg.ctc_vocab_size)]
    got = gm.ctc_kws_decode(enc, kws, max_hits=3)
    same(got, capi.ctc_kws(g["logp"], kws, cfg.blank_id, max_hits=3), "pk_ctc_kws_decode vs pk_ctc_kws on the model's log-probs")
    same(got, R.spot_batch(list(g["logp"]), kws, cfg.blank_id, max_hits=3), "vs the reference")
    assert got["score"][0, 0, 0] == 0 and got["score"][1, 2, 0] == 0, "what greedy decoding emits is found with score 0"
    xs = [normed(rng, (t, cfg.hidden_size)) * np.float32(200.0) for t in (1, 2, 13, 40, 7, 31)]
    rg = gm.ctc_decode_ragged(xs, return_logp=True)
    ra = gm.ctc_kws_decode(xs, kws, max_hits=3)
    same(ra, capi.ctc_kws([rg["logp"][b] for b in range(len(xs))], kws, cfg.blank_id, max_hits=3), "ragged: vs pk_ctc_kws")
    for b, x in enumerate(xs):
        one = gm.ctc_kws_decode(x[None], kws, max_hits=3)
        for key in ("n_hits", "start", "end"):
            assert np.array_equal(one[key][0], ra[key][b]), f"clip {b}: packed vs alone, {key}"
        assert np.array_equal(G.bits(one["score"][0]), G.bits(ra["score"][b]))
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie does not matter: the unboosted rows are walked
    try:
        same(gm.ctc_kws_decode(enc, kws, max_hits=3), got, "with a boost trie set")
    finally:
        gm.set_boost_tokens([], 5.0)
    ms = gm.ctc_kws_decode_timed(enc, kws, max_hits=3, reps=2)
    assert ms[0] > 0 and ms[1] > 0


@pytest.fixture(scope="module")
def vocab_model(tmp_path_factory):
    td = tmp_path_factory.mktemp("kws_vocab")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield cfg, gm
    gm.close()


def phrases_of(gm, clips):
    """Some phrases the model itself finds plausible: words of its own hypotheses (1 .. 64 tokens each)."""
    words = []
    for h in gm.transcribe_nbest(clips, 8, 16, 1):
        w = h[0]["text"].split()
        words += [w[0], " ".join(w[1:3])] if len(w) >= 3 else w[:1]
    out = []
    for p in words:
        if p and p not in out and 1 <= len(gm.tokenize(p)) <= 64:
            out.append(p)
    assert len(out) >= 2
    return out


def test_model_spot_phrases_in_hits_out(vocab_model):
    cfg, gm = vocab_model
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 48000))]
    phrases = phrases_of(gm, clips)
    res = gm.spot(clips, phrases=phrases, max_hits=3)
    ids = [gm.tokenize(p) for p in phrases]
    assert gm.spot(clips, ids=ids, max_hits=3) == res, "phrases and their token ids give the same hits"
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    n = 0
    for c, clip in enumerate(clips):
        assert gm.spot([clip], phrases=phrases, max_hits=3)[0] == res[c], f"clip {c} alone"
        fr = gm.ctc_kws_decode(enc[c][None], [np.asarray(x, np.int32) for x in ids], max_hits=3)
        for k in range(len(phrases)):
            assert len(res[c][k]) == fr["n_hits"][0, k]
            for j, (s, e, sc) in enumerate(res[c][k]):
                assert np.float32(s) == np.float32(fr["start"][0, k, j]) * FRAME_S, "start of the first frame"
                assert np.float32(e) == np.float32(fr["end"][0, k, j] + 1) * FRAME_S, "end of the last frame"
                assert np.float32(sc).view(np.uint32) == fr["score"][0, k, j].view(np.uint32)
                n += 1
    assert n > 0


def test_refusals(tiny_pair, vocab_model, tmp_path):
    W_, om, gm = tiny_pair
    cfg = om.cfg
    rng = np.random.default_rng(4)
    V = 8
    lp = A.make_lp("ties", 9, V, rng)[None]
    enc = normed(rng, (1, 8, cfg.hidden_size))
    gm.ctc_kws_decode(enc, [np.asarray([1], np.int32)])              # (the model's buffers exist from here on)
    free0, _, held0 = capi.mem_info(gm)

    def refused(code, word, fn):
        with pytest.raises(capi.PkError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), f"{code} / {word!r}: got {e.value.code} / {e.value}"
        assert capi.mem_info(gm)[2] == held0, "a refused call changes no buffer of the model"

    kw = [np.asarray([1, 2], np.int32)]
    for where, call in (("host rows", lambda k, **o: capi.ctc_kws(lp, k, V - 1, **o)), ("model", lambda k, **o: gm.ctc_kws_decode(enc, k, **o))):
        blank = V - 1 if where == "host rows" else cfg.blank_id
        refused(-7, "64", lambda: call([np.ones(65, np.int32)]))
        refused(-7, "max_hits", lambda: call(kw, max_hits=0))
        refused(-7, "max_hits", lambda: call(kw, max_hits=17))
        refused(-1, "min_score", lambda: call(kw, min_score=0.5))
        refused(-1, "min_score", lambda: call(kw, min_score=float("nan")))
        refused(-1, "blank", lambda: call([np.asarray([1, blank], np.int32)]))
        refused(-1, "empty", lambda: call([np.asarray([1], np.int32), np.zeros(0, np.int32)]))
        refused(-1, "outside", lambda: call([np.asarray([-1], np.int32)]))
    refused(-1, "n_kw", lambda: capi.ctc_kws(lp, [], V - 1))
    clip = synth.synth_pcm(1, 16000, seed=1)[0]
    refused(-7, "64", lambda: gm.spot([clip], ids=[[1] * 65]))
    refused(-1, "min_score", lambda: gm.spot([clip], ids=[[1]], min_score=1.0))
    refused(-1, "empty", lambda: vocab_model[1].spot([clip], phrases=[""]))      # (a model that has its vocabulary)
    # the scratch cap, from the formula 8 * n_kw * sum T <= 2^30: T = 140000 and 1000 keywords need 1.12e9 bytes.  Refused before anything is
    # allocated or read, so the rows need not hold log-probs (V = 2: 1.1 MB of host memory).
    T, K = 140000, 1000
    assert 8 * K * T > 1 << 30
    refused(-7, "cap", lambda: capi.ctc_kws(np.zeros((1, T, 2), np.float32), [np.zeros(1, np.int32)] * K, 1))
    assert capi.mem_info(gm)[0] >= free0 - (256 << 20), "nothing is allocated for a refused call"
    nocfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc")      # no CTC head: refused
    Wn = {k: v for k, v in synth.synth_weights(nocfg, seed=1).items() if not k.startswith("ctc_decoder_")}
    wp = str(tmp_path / "noctc.safetensors")
    synth.save_weights(wp, Wn)
    m2 = capi.Model(wp, nocfg, device=0)
    try:
        for fn in (lambda: m2.ctc_kws_decode(enc, kw), lambda: m2.spot([clip], ids=[[1]]), lambda: m2.ctc_kws_decode_timed(enc, kw)):
            with pytest.raises(capi.PkError) as e:
                fn()
            assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    finally:
        m2.close()


def test_facade_spot_through_the_cli(tmp_path):
    """Transcriber::spot compiled into examples/parakeet_cli (--spot, --spot-file, --spot-hits, --spot-min-score): the lines it prints are
    the hits of Model.spot on the samples the WAV holds.  The CLI runs as a fresh child process."""
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "parakeet_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()                                      # the CLI's Transcriber is the 17-layer preset
    wp, vp, ap, fp = str(tmp_path / "model.safetensors"), str(tmp_path / "vocab.txt"), str(tmp_path / "clip.wav"), str(tmp_path / "phrases.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 48000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    phrases = phrases_of(gm, [q])[:2]
    want = gm.spot([q], phrases=phrases, max_hits=3)[0]
    want_thr = gm.spot([q], phrases=phrases, max_hits=3, min_score=-0.5)[0]
    gm.close()
    assert sum(len(h) for h in want) >= 2
    open(fp, "w").write("\n".join(phrases) + "\n")

    def run(*extra):
        return subprocess.run([exe, wp, ap, "--vocab", vp, *extra], capture_output=True, text=True, timeout=600)

    def hits_of(out):
        rows = [ln.split("\t") for ln in out.splitlines() if ln.count("\t") == 3]
        return [(r[0], np.float32(r[1]), np.float32(r[2]), np.float32(r[3])) for r in rows]

    def lines(hits):
        return [(p, np.float32(s), np.float32(e), np.float32(sc)) for p, hs in zip(phrases, hits) for s, e, sc in hs]
    by_flag = run("--spot", phrases[0], "--spot", phrases[1], "--spot-hits", "3")
    assert by_flag.returncode == 0, by_flag.stderr
    assert hits_of(by_flag.stdout) == lines(want)
    by_file = run("--spot-file", fp, "--spot-hits", "3", "--spot-min-score", "-0.5")
    assert by_file.returncode == 0, by_file.stderr
    assert hits_of(by_file.stdout) == lines(want_thr)
    one = run("--spot", phrases[0])
    assert one.returncode == 0 and hits_of(one.stdout) == lines(want)[:1], "the default is the best hit alone"
    bad = run("--spot", phrases[0], "--spot-hits", "17")
    assert bad.returncode == 1 and "max_hits" in bad.stderr
    assert run("--model", "tdt-600m", "--spot", phrases[0]).returncode == 1
