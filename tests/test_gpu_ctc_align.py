"""GPU: the CTC forced alignment of given token strings (kernels/ctc_align.hip) against its written specification, tests/ctc_align_ref.py,
BIT FOR BIT: start / end / ok equal, conf / score / total equal as bit patterns."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_common as G
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

import ctc_align_ref as R
import ctc_beam_ref as BR

pytestmark = pytest.mark.gpu

FAMILIES = ["ties", "holes", "peaky"]

# The kernel as built (csrc/kernels/kernels.hpp): three shapes of threads x states per thread, chosen by the longest string's S = 2 L + 1,
#   kAlignThreads = {64, 256, 1024}, kAlignStrip = {4, 8, 32}   ->   S <= 256, S <= 2048, S <= 32768 (= kAlignMaxStates; past it: refused)
# a wave is 64 lanes, so inside a shape the waves meet at S = 64 * strip * i: 256 (= the first shape), 512, 1024, ... for 256 x 8 and 2048 (= the
# second shape), 4096 for 1024 x 32; strips meet at every multiple of 4 / 8 / 32; back-pointers are packed kAlignBpCells = 16 cells per
# dword, so rows grow by a dword at S = 16 i.  S is odd, so "the boundary, one less, one more" are S = boundary - 1 and boundary + 1.
SHAPE_BOUNDS = [256, 2048]
WAVE_BOUNDS = [512, 4096]
STRIP_BOUNDS = [4, 8, 32, 64]
PACK_BOUNDS = [16, 48]
EDGE_L = sorted({(bnd + d) // 2 for bnd in SHAPE_BOUNDS + WAVE_BOUNDS + STRIP_BOUNDS + PACK_BOUNDS for d in (-2, 0)})   # S = bnd - 1, bnd + 1
MAX_L = (32768 - 1) // 2


def same(got, want, what):
    assert got["ok"] == want["ok"], f"{what}: ok {got['ok']} vs {want['ok']}"
    assert np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]), f"{what}: start / end frames"
    for k in ("conf", "score", "total"):
        if k in want and k in got:
            assert np.array_equal(G.bits(np.asarray(got[k], np.float32)), G.bits(np.asarray(want[k], np.float32))), f"{what}: {k} bits {got[k]} vs {want[k]}"
    if not want["ok"]:
        assert got["score"] == -np.inf and not got["start"].any() and not got["end"].any() and not got["conf"].any()


def rand_ids(rng, L, V):
    return rng.integers(0, V - 1, size=L).astype(np.int32)


def distinct_ids(rng, L, V):
    return rng.permutation(V - 1)[:L].astype(np.int32)


SMALL = [(1, 0, 5, "rand"), (1, 1, 5, "rand"), (2, 1, 5, "rand"), (7, 3, 5, "aab"), (4, 3, 5, "aab"), (3, 3, 5, "aab"), (130, 128, 5, "rand"),
         (130, 128, 129, "distinct"), (126, 30, 1025, "rand"), (376, 90, 8193, "rand")]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T,L,V,kind", SMALL)
def test_alignment_equals_reference_uniform_batch(T, L, V, kind, family):
    rng = np.random.default_rng(T * 1009 + L * 31 + V + 7 * FAMILIES.index(family))
    lps = [R.make_lp(family, T, V, rng) for _ in range(2)]
    ids = [np.array([1, 1, 2], np.int32) if kind == "aab" else distinct_ids(rng, L, V) if kind == "distinct" else rand_ids(rng, L, V) for _ in lps]
    got = capi.ctc_align(np.stack(lps), ids, V - 1)
    for b, lp in enumerate(lps):
        want = R.full(lp, ids[b], V - 1)
        same(got[b], want, f"{family} T={T} L={L} V={V} utterance {b}")
        if kind == "aab":
            assert T >= 4 or want["ok"] == 0, "[a, a, b] needs 4 frames"
            assert T < 4 or family == "holes" or want["ok"] == 1     # (at T = 4 the one path may run through a -inf entry of "holes")
        if (T, L, V) == (130, 128, 5):
            assert want["ok"] == 0, "128 random tokens of 4 repeat too often for 130 frames"
        if want["ok"]:
            assert want["total"] >= want["score"]
    no_total = capi.ctc_align(np.stack(lps), ids, V - 1, total=False)      # the max-plus pass alone (its own instantiation)
    for b in range(2):
        same(no_total[b], {k: v for k, v in got[b].items() if k != "total"}, "without total")


def test_alignment_past_the_old_frame_limit():
    rng = np.random.default_rng(4100)
    lp, ids = R.make_lp("ties", 4100, 33, rng), rand_ids(rng, 2000, 33)
    same(capi.ctc_align(lp[None], [ids], 32)[0], R.full(lp, ids, 32), "T=4100 L=2000 V=33")


def test_alignment_of_a_long_recording():
    """The one case that is allowed to take seconds in the reference (S = 6001: past the 4096-state wave boundary of the 1024 x 32 shape)."""
    rng = np.random.default_rng(12000)
    lp, ids = R.make_lp("ties", 12000, 9, rng), rand_ids(rng, 3000, 9)
    got = capi.ctc_align(lp[None], [ids], 8)[0]
    want = R.full(lp, ids, 8)
    assert want["ok"] == 1
    same(got, want, "T=12000 L=3000 V=9")


def edge_ids(rng, L, V):
    """L tokens that can be aligned in L + 40 frames: neighbours differ, except at up to 8 places where a token is repeated on purpose (a
    forbidden skip and a forced blank), which costs at most 16 of the 40 spare frames."""
    ids = (np.cumsum(rng.integers(1, V - 1, size=L)) % (V - 1)).astype(np.int32)
    if L > 16:
        for j in rng.integers(1, L, size=8):
            ids[j] = ids[j - 1]
    return ids


@pytest.mark.parametrize("family", FAMILIES)
def test_strip_and_packing_edges(family):
    rng = np.random.default_rng(5 + FAMILIES.index(family))
    for L in EDGE_L:
        T, V = L + 40, 33
        lp, ids = R.make_lp(family, T, V, rng), edge_ids(rng, L, V)
        want = R.full(lp, ids, V - 1)
        if family != "holes":                                        # (a -inf entry can close the few paths of a string this tight)
            assert want["ok"] == 1, f"{family} L={L}: the edge case must have a path to check"
        same(capi.ctc_align(lp[None], [ids], V - 1)[0], want, f"{family} L={L} S={2 * L + 1}")
        got = capi.ctc_align(lp[None], [ids], V - 1, total=False)[0]
        same(got, {k: v for k, v in want.items() if k != "total"}, f"{family} L={L} without total")


def test_longest_string_and_one_more():
    """L = 16383: the full lattice's back-pointers alone would take the reference 538 MB, so this one case is compared with the reference
    restricted to the band (81 states wide at T = L + 40), which tests/test_ctc_align_ref.py shows equal to the full lattice."""
    rng = np.random.default_rng(99)
    L, V = MAX_L, 33
    T = L + 40
    lp = R.make_lp("ties", T, V, rng)
    ids = edge_ids(rng, L, V)
    want = R.lattice_banded(lp, ids, V - 1)
    assert want["ok"] == 1
    same(capi.ctc_align(lp[None], [ids], V - 1)[0], want, f"L={L}")
    with pytest.raises(capi.PkError) as e:
        capi.ctc_align(lp[None], [np.append(ids, 0).astype(np.int32)], V - 1)
    assert e.value.code == -7 and "16383" in str(e.value)


RAG_T = [1, 2, 300, 13, 126, 7, 64, 257, 40]
RAG_L = [0, 1, 130, 0, 30, 5, 31, 128, 17]                           # utterance 5: 5 tokens + 4 repeats in 7 frames: cannot be aligned


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_batch_equals_single_utterance_runs(family):
    rng = np.random.default_rng(300 + FAMILIES.index(family))
    V = 33
    lps = [R.make_lp(family, t, V, rng) for t in RAG_T]
    ids = [rand_ids(rng, l, V) for l in RAG_L]
    ids[5][:] = 3
    got = capi.ctc_align(lps, ids, V - 1)
    assert got[5]["ok"] == 0
    for b, lp in enumerate(lps):
        same(got[b], capi.ctc_align(lp[None], [ids[b]], V - 1)[0], f"{family} utterance {b}: packed vs alone")
        same(got[b], R.full(lp, ids[b], V - 1), f"{family} utterance {b} vs the reference")


def test_alignment_of_beam_hypotheses_equals_the_beams_own():
    rng = np.random.default_rng(60)
    T, V, W, N = 60, 33, 8, 8
    lps = [R.make_lp(f, T, V, rng) for f in ("ties", "peaky")]
    beam = capi.ctc_beam_search(np.stack(lps), V - 1, W, 16, N, timestamps=True)
    n = 0
    for b, lp in enumerate(lps):
        for j in range(N):
            if not beam["score"][b, j] > -np.inf:
                continue
            L = beam["lens"][b, j]
            r = capi.ctc_align(lp[None], [beam["ids"][b, j, :L]], V - 1)[0]
            assert r["ok"] == 1 and r["total"] >= r["score"]
            assert np.array_equal(r["start"], beam["start"][b, j, :L]) and np.array_equal(r["end"], beam["end"][b, j, :L])
            assert np.array_equal(G.bits(r["conf"]), G.bits(beam["conf"][b, j, :L]))
            n += int(L)
    assert n > 20


@pytest.fixture(scope="module")
def tiny_pair(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("align_tiny"), pk.make_tiny_config(), seed=42, with_vocab=True)


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


@pytest.mark.parametrize("preset", ["tiny", "110m"])
def test_align_decode_on_the_models_rows(preset, tiny_pair, tmp_path_factory):
    if preset == "tiny":
        W_, om, gm = tiny_pair
        T_uniform, rag_T = 40, [1, 2, 13, 40, 7, 31]
    else:
        W_, om, gm = G.make_pair(tmp_path_factory.mktemp("align_110m"), G.one_layer_110m(1), seed=42)
        T_uniform, rag_T = 126, [126, 1, 64, 99]
    cfg = om.cfg
    rng = np.random.default_rng(31)
    enc = normed(rng, (2, T_uniform, cfg.hidden_size)) * np.float32(200.0)      # peaky rows: the greedy output has tokens
    g = gm.ctc_decode(enc, return_logp=True)
    ids = [g["ids"][b, :g["lens"][b]] for b in range(2)]
    assert sum(len(x) for x in ids) > 10
    got = gm.ctc_align_decode(enc, ids)
    on_logp = capi.ctc_align(g["logp"], ids, cfg.blank_id)
    for b in range(2):
        same(got[b], on_logp[b], f"{preset}: pk_ctc_align_decode vs pk_ctc_align on the model's log-probs")
        same(got[b], R.full(g["logp"][b], ids[b], cfg.blank_id), f"{preset}: vs the reference")
        assert got[b]["ok"] == 1, "the greedy output is a path, so it can be aligned"
        n = g["lens"][b]
        assert np.all(got[b]["start"] <= g["start"][b, :n]) and np.all(g["start"][b, :n] <= got[b]["end"]), "greedy's frame inside [start, end]"
    xs = [normed(rng, (t, cfg.hidden_size)) * np.float32(200.0) for t in rag_T]
    rg = gm.ctc_decode_ragged(xs, return_logp=True)
    rids = [rg["ids"][b, :rg["lens"][b]] for b in range(len(xs))]
    ra = gm.ctc_align_decode(xs, rids)
    for b, x in enumerate(xs):
        same(ra[b], gm.ctc_align_decode(x[None], [rids[b]])[0], f"{preset} clip {b}: packed vs alone")
        same(ra[b], capi.ctc_align(rg["logp"][b][None], [rids[b]], cfg.blank_id)[0], f"{preset} clip {b}: vs pk_ctc_align")
        assert ra[b]["ok"] == 1
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie does not matter: the unboosted rows are aligned
    try:
        for b in range(2):
            same(gm.ctc_align_decode(enc, ids)[b], got[b], "with a boost trie set")
    finally:
        gm.set_boost_tokens([], 5.0)


@pytest.fixture(scope="module")
def vocab_model(tmp_path_factory):
    td = tmp_path_factory.mktemp("align_vocab")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield cfg, gm
    gm.close()


def test_model_align_text_in_words_out(vocab_model):
    import ctypes
    cfg, gm = vocab_model
    L = capi.lib()
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 700, 48000))]
    hyp = gm.transcribe_nbest(clips, 8, 16, 1)                       # some text the model itself finds plausible
    texts = [h[0]["text"] for h in hyp]
    texts[2] = texts[0] + " " + texts[0] + " " + texts[0]            # far too long for a clip of 700 samples
    res = gm.align(clips, texts=texts)
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    n_words = 0
    for i, r in enumerate(res):
        ids = gm.tokenize(texts[i])
        assert r["token_ids"] == ids
        one = gm.ctc_align_decode(enc[i][None], [np.asarray(ids, np.int32)])[0]
        assert r["ok"] == one["ok"] and np.float32(r["score"]).view(np.uint32) == one["score"].view(np.uint32)
        assert np.float32(r["total"]).view(np.uint32) == one["total"].view(np.uint32)
        if not r["ok"]:
            assert "start" not in r
            continue
        assert r["start"] == one["start"].tolist() and r["end"] == one["end"].tolist()
        assert np.array_equal(G.bits(np.asarray(r["conf"], np.float32)), G.bits(one["conf"]))
        n = len(ids)
        ia, st, en, cf = np.asarray(ids, np.int32), one["start"], one["end"], one["conf"]
        wbuf = ctypes.create_string_buffer(1 << 16)
        ws, we, wc = np.zeros(256, np.float32), np.zeros(256, np.float32), np.zeros(256, np.float32)
        nw = L.pk_group_timestamps(gm._h, capi._i(ia) if n else None, capi._i(st) if n else None, capi._i(en) if n else None,
                                   capi._f(cf) if n else None, int(n), 0, wbuf, 1 << 16, capi._f(ws), capi._f(we), capi._f(wc), 256)
        assert nw == len(r["words"])
        words = wbuf.value.decode().split("\n") if nw else []
        for k, (wd, a, b, c) in enumerate(r["words"]):
            assert wd == words[k] and np.float32(a) == ws[k] and np.float32(b) == we[k] and np.float32(c) == wc[k]
        n_words += nw
    assert res[2]["ok"] == 0 and n_words > 0
    by_ids = gm.align(clips, ids=[gm.tokenize(t) for t in texts])    # the same transcripts given as ids
    assert by_ids == res


def test_facade_align_through_the_cli(tmp_path):
    """Transcriber::align compiled into examples/parakeet_cli (--align "text" and --align-file path): the word timestamps and the score it
    prints are those of Model.align on the samples the WAV holds.  The CLI runs as a fresh child process."""
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "parakeet_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()                                      # the CLI's Transcriber is the 17-layer preset
    wp, vp, ap, tp = str(tmp_path / "model.safetensors"), str(tmp_path / "vocab.txt"), str(tmp_path / "clip.wav"), str(tmp_path / "text.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 48000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    text = gm.transcribe_nbest([q], 8, 16, 1)[0][0]["text"]
    assert len(text.split()) >= 1
    want = gm.align([q], texts=[text])[0]
    too_long = " ".join([text] * 40)
    assert gm.align([q], texts=[too_long])[0]["ok"] == 0
    gm.close()
    assert want["ok"] == 1 and len(want["words"]) >= 1
    open(tp, "w").write(text + "\n")

    def run(*extra):
        return subprocess.run([exe, wp, ap, "--vocab", vp, *extra], capture_output=True, text=True, timeout=600)

    def words_of(out):
        return re.findall(r"^  \[(\S+)s - (\S+)s\] \((\S+)\) (.*)$", out, flags=re.M)
    lines = [(f"{a:.2f}", f"{b:.2f}", f"{c:.3f}", w) for w, a, b, c in want["words"]]
    for extra in (("--align", text), ("--align-file", tp)):
        out = run(*extra)
        assert out.returncode == 0, out.stderr
        assert words_of(out.stdout) == lines, extra[0]
        toks = [[int(x) for x in m.split()] for m in re.findall(r"^Tokens \(\d+\):(.*)$", out.stdout, flags=re.M)]
        assert toks == [want["token_ids"]]
        sc, tot = re.search(r"^Alignment: score (\S+) log-likelihood (\S+)$", out.stdout, flags=re.M).groups()
        assert np.float32(sc) == np.float32(want["score"]) and np.float32(tot) == np.float32(want["total"])
    ts = run("--decoder", "ctc", "--timestamps")                      # the format is the one --timestamps prints
    assert ts.returncode == 0 and words_of(ts.stdout), ts.stderr
    bad = run("--align", too_long)
    assert bad.returncode == 1 and "cannot be aligned" in bad.stderr
    assert run("--model", "sortformer", "--align", text).returncode == 1


def test_refusals(tiny_pair, tmp_path):
    W_, om, gm = tiny_pair
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, om.cfg.hidden_size))
    for bad in ([om.cfg.blank_id], [-1], [om.cfg.ctc_vocab_size]):
        with pytest.raises(capi.PkError) as e:
            gm.ctc_align_decode(enc, [np.asarray(bad, np.int32)])
        assert e.value.code == -1, bad
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc")      # no CTC head: refused
    Wn = {k: v for k, v in synth.synth_weights(cfg, seed=1).items() if not k.startswith("ctc_decoder_")}
    wp = str(tmp_path / "noctc.safetensors")
    synth.save_weights(wp, Wn)
    m2 = capi.Model(wp, cfg, device=0)
    with pytest.raises(capi.PkError) as e:
        m2.ctc_align_decode(enc, [np.asarray([1], np.int32)])
    assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    with pytest.raises(capi.PkError) as e:
        m2.align([synth.synth_pcm(1, 16000, seed=1)[0]], ids=[[1]])
    assert e.value.code == -7
    m2.close()
    # the scratch cap, from the formula T * ceil((2 L + 1) / 16) * 4 bytes <= 2^30: T = 140000, L = 16000 needs 140000 * 2001 * 4 = 1.12e9 bytes.
    # Refused before anything is allocated or read, so the rows need not hold log-probs (V = 2: 1.1 MB of host memory).
    T, L = 140000, 16000
    assert T * ((2 * L + 1 + 15) // 16) * 4 > 1 << 30
    with pytest.raises(capi.PkError) as e:
        capi.ctc_align(np.zeros((1, T, 2), np.float32), [np.zeros(L, np.int32)], 1)
    assert e.value.code == -7 and "cap" in str(e.value)
