"""GPU: the TDT forced alignment of given token strings (kernels/tdt_align.hip) against its written specification, tests/tdt_align_ref.py, and
the lattice it is computed on against the oracle's teacher-forced scoring, BIT FOR BIT."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_common as G
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

import tdt_align_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = ["ties", "holes", "peaky"]
DURS = {"d01234": [0, 1, 2, 3, 4], "d01": [0, 1], "d124": [1, 2, 4], "d8": [4, 0, 1, 1, 2, 8, 3, 5]}

# The kernel as built (csrc/kernels/kernels.hpp, kernels/tdt_align.hip):
#   workgroup width  kTdtAlignThreads = {64, 256}: one wave while the longest diagonal, U + 1 cells, fits it -> U + 1 = 63 / 64 / 65
#   cells per thread a thread of the 256-wide form takes cells lo + tid + 256 j -> a second cell at U + 1 = 257, a third at 513 (needs T >= U + 1)
#   ring size        dur_max + 2 diagonals, dur_max <= kTdtAlignMaxDur = 8 -> the duration sets below give rings of 3, 6 and 10; 9 is refused
#   tokens           U <= kTdtAlignMaxTokens = 1535 (the ring of 10 diagonals x 1536 cells is 61440 bytes of LDS); 1536 is refused.  The kernel's real
#                    limit is the joint one, ring x pitch: U = 1534 and 1535 run with dur_max = 8 (the largest LDS configuration, six cells per thread)
#   every boundary case is ALIGNABLE in the reference (asserted), so alpha, back-pointers, back-trace and conf are all compared there
#   back-pointers    one byte per cell, row pitch U + 1: nothing is packed, odd and even pitches are both among the shapes
SMALL = [(1, 0), (1, 1), (1, 3), (2, 1), (5, 3), (8, 8)]
EDGES = [(66, 62), (66, 63), (66, 64), (258, 254), (258, 256), (514, 510), (514, 512), (3, 1535)]
LARGE = [(130, 40), (376, 90)]


def same(got, want, what):
    assert got["ok"] == want["ok"], f"{what}: ok {got['ok']} vs {want['ok']}"
    for k in ("start", "end", "dur_idx"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    for k in ("conf", "score"):
        assert np.array_equal(G.bits(np.asarray(got[k], np.float32)), G.bits(np.asarray(want[k], np.float32))), f"{what}: {k} bits {got[k]} vs {want[k]}"
    if not want["ok"]:
        assert got["score"] == -np.inf and not got["start"].any() and not got["end"].any() and not got["dur_idx"].any() and not got["conf"].any()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dname", list(DURS))
@pytest.mark.parametrize("T,U", SMALL)
def test_walk_equals_reference_small_uniform_batches(T, U, dname, family):
    dur = DURS[dname]
    rng = np.random.default_rng(T * 1009 + U * 31 + len(dur) + 7 * FAMILIES.index(family))
    lats = [R.make_lattice(family, T, U, len(dur), rng) for _ in range(3)]
    got = capi.tdt_align(lats, dur)
    for b, lat in enumerate(lats):
        same(got[b], R.align(*lat, dur), f"{family} {dname} T={T} U={U} utterance {b}")


BOUNDARY = ([(T, U, ("d01", "d01234", "d8")[k % 3], ("ties", "peaky")[k % 2]) for k, (T, U) in enumerate(EDGES)]
            + [(3, 1535, "d8", "ties"), (3, 1534, "d8", "peaky")]
            + [(T, U, dn, "peaky") for (T, U) in LARGE for dn in ("d01234", "d124")] + [(130, 40, "d8", "ties"), (130, 40, "d01", "holes")])


@pytest.mark.parametrize("T,U,dname,family", BOUNDARY)
def test_walk_equals_reference_at_the_kernels_boundaries(T, U, dname, family):
    dur = DURS[dname]
    rng = np.random.default_rng(T * 1009 + U * 31 + len(dur))
    lat = R.make_lattice(family, T, U, len(dur), rng)
    want = R.align(*lat, dur)
    assert want["ok"] == 1 and want["score"] > -np.inf, "a boundary case must align: otherwise only zeros are compared"
    same(capi.tdt_align([lat], dur)[0], want, f"{family} {dname} T={T} U={U}")


def test_ragged_batch_with_empty_and_unalignable_neighbours():
    dur = DURS["d124"]
    rng = np.random.default_rng(77)
    shapes = [(9, 3), (7, 0), (4, 5), (70, 66), (12, 12), (1, 0)]    # (4, 5): more tokens than frames and no zero duration
    lats = [R.make_lattice("ties", T, U, 3, rng) for T, U in shapes]
    got = capi.tdt_align(lats, dur)
    want = [R.align(*lat, dur) for lat in lats]
    for b in range(len(shapes)):
        same(got[b], want[b], f"ragged utterance {b} {shapes[b]}")
        same(capi.tdt_align([lats[b]], dur)[0], got[b], f"utterance {b}: alone vs in the batch")
    assert want[2]["ok"] == 0 and [w["ok"] for w in want[:2] + want[3:]] == [1] * 5


# ---- the lattice against the oracle ---------------------------------------------------------------------------------------------------------
def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def model_of(tmp, which):
    if which == "tiny":
        cfg = G.tiny()
    elif which == "tiny2l":
        cfg = G.tiny(num_lstm_layers=2, vocab_size=78, blank_id=77, ctc_vocab_size=78, durations=[0, 1, 2, 4], name="tiny2l-v78")    # V + D = 82
    else:
        cfg = dataclasses.replace(pk.make_tdt_600m_config(), num_layers=1, name="600m-1L-align")      # vocabulary 8193, 2 LSTM layers, 640 / 640
    return (cfg,) + G.make_pair(tmp, cfg, seed=31)


CASES = {"tiny": ([(40, 12), (40, 12), (33, 1), (40, 12), (9, 0)], (0, 520, 7)),      # 1615 cells: one product above the small-M kernel's 1536 rows with chunk_rows = 0
         "tiny2l": ([(40, 1), (9, 12), (20, 0)], (0, 40, 50)),                         # cells 80 / 117 / 20: 40 puts an edge between utterances 0 and 1 and inside both
         "600m": ([(40, 1), (9, 12), (20, 0)], (40,))}


@pytest.mark.parametrize("which", list(CASES))
def test_lattice_equals_the_oracles_teacher_forced_rows(tmp_path_factory, which):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("lat_" + which), which)
    shapes, chunks = CASES[which]
    rng = np.random.default_rng(len(which))
    encs = [normed(rng, (T, cfg.hidden_size)) for T, _ in shapes]
    ids = [rng.integers(0, cfg.blank_id, size=U).astype(np.int32) for _, U in shapes]
    want = [R.oracle_lattice(om, e, i) for e, i in zip(encs, ids)]
    for ch in chunks:
        got, guard = gm.tdt_lattice(encs, ids, chunk_rows=ch)
        assert np.all(guard == 0x7FC5A5A5), f"chunk_rows {ch}: a word past the written extent was touched"
        for b, (lab, blk, dl) in enumerate(want):
            G.assert_bits_equal(got[b]["lab"], lab, f"{which} chunk_rows {ch} utterance {b}: label log-probs")
            G.assert_bits_equal(got[b]["blk"], blk, f"{which} chunk_rows {ch} utterance {b}: blank log-probs")
            G.assert_bits_equal(got[b]["dl"], dl, f"{which} chunk_rows {ch} utterance {b}: duration log-probs")
    if which == "tiny":                                             # end to end on the same batch: the walk on the device's lattice
        dur = list(cfg.durations)
        got = gm.tdt_align_decode(encs, ids)
        for b, lat in enumerate(want):
            same(got[b], R.align(*lat, dur), f"tdt_align_decode utterance {b}")
            same(gm.tdt_align_decode(encs[b][None], [ids[b]])[0], got[b], f"utterance {b}: uniform call alone vs packed")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_greedy_transcript_aligns_and_beats_the_greedy_path(tmp_path_factory):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("e2e"), "tiny")
    rng = np.random.default_rng(5)
    enc = normed(rng, (3, 30, cfg.hidden_size))
    g = om.tdt_greedy(enc)
    ids = [g["ids"][b, :g["lens"][b]] for b in range(3)]
    assert sum(len(i) for i in ids) > 3, "degenerate test: nothing decoded"
    got = gm.tdt_align_decode(enc, ids)
    for b in range(3):
        same(got[b], R.align(*R.oracle_lattice(om, enc[b], ids[b]), list(cfg.durations)), f"utterance {b}")
        assert got[b]["ok"] == 1, "the greedy output is a path, so it can be aligned"
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie does not matter
    try:
        for b in range(3):
            same(gm.tdt_align_decode(enc, ids)[b], got[b], "with a boost trie set")
    finally:
        gm.set_boost_tokens([], 5.0)


@pytest.fixture(scope="module")
def noctc_vocab_model(tmp_path_factory):
    """A model WITHOUT a CTC head (what tdt-600m is): Model.align refuses it, Model.align_tdt aligns through it."""
    td = tmp_path_factory.mktemp("tdt_align_vocab")
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, durations=[1, 2, 4], name="tiny-noctc-align")    # no zero duration: a token needs a frame
    W = {k: v for k, v in synth.synth_weights(cfg, seed=42).items() if not k.startswith("ctc_decoder_")}
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield cfg, gm
    gm.close()


def test_model_align_tdt_from_pcm_equals_its_stages(noctc_vocab_model):
    cfg, gm = noctc_vocab_model
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 700, 48000))]
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    assert [e.shape[0] for e in enc][2] < 5 and min(e.shape[0] for i, e in enumerate(enc) if i != 2) >= 9
    words = [p[1:] for p in synth.synth_vocab(cfg.vocab_size - 1) if p.startswith("\u2581")]      # whole-word pieces of the model's vocabulary
    texts = [" ".join(words[a:b]) for a, b in ((0, 3), (3, 5), (5, 11), (11, 15))]           # clip 2: more tokens than its frames, unalignable
    ids = [gm.tokenize(t) for t in texts]
    assert [len(i) for i in ids] == [3, 2, 6, 4]
    with pytest.raises(capi.PkError) as e:
        gm.align(clips, ids=ids)
    assert e.value.code == -7, "no CTC head: the CTC alignment still refuses"
    res = gm.align_tdt(clips, ids=ids)
    n_words = 0
    for i, r in enumerate(res):
        one = gm.tdt_align_decode(enc[i][None], [np.asarray(ids[i], np.int32)])[0]
        assert r["token_ids"] == ids[i]
        assert r["ok"] == one["ok"] and np.float32(r["score"]).view(np.uint32) == one["score"].view(np.uint32)
        if not r["ok"]:
            assert "start" not in r
            continue
        assert r["start"] == one["start"].tolist() and r["end"] == one["end"].tolist()
        assert np.array_equal(G.bits(np.asarray(r["conf"], np.float32)), G.bits(one["conf"]))
        n_words += len(r["words"])
    assert res[2]["ok"] == 0 and res[0]["ok"] == 1 and n_words > 0
    assert gm.align_tdt(clips, texts=texts) == res, "the same transcripts given as text"


def test_facade_align_tdt_through_the_cli(tmp_path):
    """Transcriber::align_tdt compiled into examples/parakeet_cli (--align "text" --align-head tdt): the word timestamps and the score it
    prints are those of Model.align_tdt on the samples the WAV holds.  The CLI runs as a fresh child process."""
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
    text = gm.transcribe_nbest([q], 8, 16, 1)[0][0]["text"]
    assert len(text.split()) >= 1
    want = gm.align_tdt([q], texts=[text])[0]
    gm.close()
    assert want["ok"] == 1 and len(want["words"]) >= 1

    def run(*extra):
        return subprocess.run([exe, wp, ap, "--vocab", vp, *extra], capture_output=True, text=True, timeout=600)
    out = run("--align", text, "--align-head", "tdt")
    assert out.returncode == 0, out.stderr
    words = re.findall(r"^  \[(\S+)s - (\S+)s\] \((\S+)\) (.*)$", out.stdout, flags=re.M)
    assert words == [(f"{a:.2f}", f"{b:.2f}", f"{c:.3f}", w) for w, a, b, c in want["words"]]
    toks = [[int(x) for x in m.split()] for m in re.findall(r"^Tokens \(\d+\):(.*)$", out.stdout, flags=re.M)]
    assert toks == [want["token_ids"]]
    sc = re.search(r"^Alignment \(tdt\): score (\S+)$", out.stdout, flags=re.M).group(1)
    assert np.float32(sc) == np.float32(want["score"])
    assert run("--align", text, "--align-head", "nope").returncode == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refuse")
    cfg, W, om, gm = model_of(tmp, "tiny")
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, cfg.hidden_size))
    for bad in ([cfg.blank_id], [-1], [cfg.vocab_size]):
        with pytest.raises(capi.PkError) as e:
            gm.tdt_align_decode(enc, [np.asarray(bad, np.int32)])
        assert e.value.code == -1, bad
    L = capi.lib()
    z, zi = np.zeros(4, np.float32), np.zeros(4, np.int32)
    enc2 = normed(rng, (2, 8, cfg.hidden_size))
    st = L.pk_tdt_align_decode(gm._h, capi._f(enc2), 2, 8, capi._i(np.asarray([1, 2], np.int32)), capi._i(np.asarray([0, 2, 1], np.int32)), capi._i(zi),
                               capi._i(zi), capi._i(zi), capi._f(z), capi._f(z), capi._i(zi))
    assert st == -1, "decreasing offsets"
    with pytest.raises(capi.PkError) as e:                           # more tokens than the kernel is built for
        gm.tdt_align_decode(enc, [np.ones(1536, np.int32)])
    assert e.value.code == -7 and "1535" in str(e.value)
    # the scratch cap of a model call: lattice values 4 (labs + cells (1 + D)) + cells back-pointers (+ chunk and prediction net) <= 2^30.  T = 30000, U = 1500,
    # D = 5: cells = 45 030 000 -> 4 (45 000 000 + 270 180 000) + 45 030 000 = 1.3e9.  Refused before anything is allocated or uploaded: the
    # encoder rows handed in are 30000 x 128 floats of host memory nobody reads.
    T, U = 30000, 1500
    assert 4 * (T * U + T * (U + 1) * 6) + T * (U + 1) > 1 << 30
    gm.tdt_align_decode(enc, [np.asarray([1, 2], np.int32)])         # (the buffers of a small call exist: a refused one must not grow or replace them)
    free0, _, held0 = capi.mem_info(gm)
    assert held0 > 0
    with pytest.raises(capi.PkError) as e:
        gm.tdt_align_decode(np.zeros((1, T, cfg.hidden_size), np.float32), [np.ones(U, np.int32)])
    assert e.value.code == -7 and "cap" in str(e.value)
    free1, _, held1 = capi.mem_info(gm)
    assert held1 == held0, "a refused call changes no buffer of the model's workspace or alignment scratch"
    # the device's free memory (shared with whatever else runs on it, hence the slack): the refused call would have taken more than 1 GiB
    assert free1 >= free0 - (256 << 20), "nothing is allocated for a refused call"
    for kw, msg in ((dict(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt-al"), "RNN-T"),
                    (dict(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-al"), "gemm_bf16")):
        c2 = G.tiny(**kw)
        wp = str(tmp / (c2.name + ".safetensors"))
        synth.save_weights(wp, synth.synth_weights(c2, seed=12))
        m2 = capi.Model(wp, c2, device=0)
        try:
            with pytest.raises(capi.PkError) as e:
                m2.tdt_align_decode(enc, [np.asarray([1], np.int32)])
            assert e.value.code == -7 and msg in str(e.value)
            with pytest.raises(capi.PkError) as e:
                m2.align_tdt([synth.synth_pcm(1, 16000, seed=1)[0]], ids=[[1]])
            assert e.value.code == -7
        finally:
            m2.close()
    with pytest.raises(capi.PkError) as e:                           # the walk alone: a duration the ring is not built for
        capi.tdt_align([R.make_lattice("ties", 3, 1, 2, rng)], [0, 9])
    assert e.value.code == -7
