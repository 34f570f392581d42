"""GPU: the forward-algorithm total of given token strings under the TDT head (kernels/tdt_total.hip) against its written specification,
tests/tdt_total_ref.py, hypotheses that share one clip's frames, and the CTC n-best list rescored with it, BIT FOR BIT."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_common as G
from conftest import ROOT, pk
from parakeet_cpp_amd import capi, synth

import tdt_align_ref as A
import tdt_total_ref as R

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)


def same(got, want, what):
    """got: a dict of the library; want: the specification's fp32 total."""
    want = np.float32(want)
    assert np.float32(got["total"]).view(np.uint32) == want.view(np.uint32), f"{what}: total bits {got['total']!r} vs {want!r}"
    assert got["ok"] == (1 if want > NEG else 0), f"{what}: ok"


def same_lists(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["ok"] == y["ok"] and np.float32(x["total"]).view(np.uint32) == np.float32(y["total"]).view(np.uint32), f"{what}: hypothesis {k}: {x} vs {y}"


# ---- the walk on host lattices ----------------------------------------------------------------------------------------------------------------
# The shapes of tests/test_gpu_tdt_align.py (listed in tests/tdt_total_ref.py): the kernel has the alignment's widths, ring and limits.
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dname", list(R.DURS))
@pytest.mark.parametrize("T,U", R.SMALL)
def test_walk_equals_reference_small_uniform_batches(T, U, dname, family):
    dur = R.DURS[dname]
    lats = R.small_lattices(T, U, dname, family)
    got = capi.tdt_total(lats, dur)
    for b, lat in enumerate(lats):
        same(got[b], R.forward_total(*lat, dur), f"{family} {dname} T={T} U={U} utterance {b}")


@pytest.mark.parametrize("T,U,dname,family", R.BOUNDARY)
def test_walk_equals_reference_at_the_kernels_boundaries(T, U, dname, family):
    dur = R.DURS[dname]
    lat = R.boundary_lattice(T, U, dname, family)
    want = R.forward_total(*lat, dur)
    assert np.isfinite(want), "a boundary case must have a finite total: otherwise only -inf is compared"
    same(capi.tdt_total([lat], dur)[0], want, f"{family} {dname} T={T} U={U}")


def test_ragged_batch_with_empty_and_unreachable_neighbours():
    dur = R.DURS["d124"]
    lats = R.ragged_lattices()
    got = capi.tdt_total(lats, dur)
    want = [R.forward_total(*lat, dur) for lat in lats]
    for b in range(len(lats)):
        same(got[b], want[b], f"ragged utterance {b} {R.RAGGED[b]}")
        same_lists(capi.tdt_total([lats[b]], dur), [got[b]], f"utterance {b}: alone vs in the batch")
    assert [g["ok"] for g in got] == [1, 1, 0, 1, 1, 1]


# ---- hypotheses that share a clip's frames ----------------------------------------------------------------------------------------------------
def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def model_of(tmp, which):
    """As tests/test_gpu_tdt_align.py builds its models."""
    if which == "tiny":
        cfg = G.tiny()
    else:
        cfg = G.tiny(num_lstm_layers=2, vocab_size=78, blank_id=77, ctc_vocab_size=78, durations=[0, 1, 2, 4], name="tiny2l-v78")    # V + D = 82
    return (cfg,) + G.make_pair(tmp, cfg, seed=31)


def shared_case(cfg, seed):
    """3 clips of T = 40, 9, 20 and 7 hypotheses; lengths include 0, 1 and 12; hypotheses 0 and 2 of clip 0 share a prefix of 5 tokens."""
    rng = np.random.default_rng(seed)
    encs = [normed(rng, (T, cfg.hidden_size)) for T in (40, 9, 20)]
    clip_of = [0, 0, 0, 1, 1, 2, 2]
    ids = [rng.integers(0, cfg.blank_id, size=U).astype(np.int32) for U in (12, 0, 8, 1, 5, 12, 3)]
    ids[2][:5] = ids[0][:5]
    return encs, ids, clip_of


@pytest.fixture(scope="module")
def tiny_shared(tmp_path_factory):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("total_tiny"), "tiny")
    encs, ids, clip_of = shared_case(cfg, 3)
    return cfg, om, gm, encs, ids, clip_of, gm.tdt_total_decode(encs, ids, clip_of)


def test_shared_frames_equal_replicated_frames_and_single_calls(tiny_shared):
    cfg, om, gm, encs, ids, clip_of, got = tiny_shared
    rep = [encs[c] for c in clip_of]
    lats, guard = gm.tdt_lattice(rep, ids)
    on_lattice = capi.tdt_total([(l["lab"], l["blk"], l["dl"]) for l in lats], list(cfg.durations))
    same_lists(got, on_lattice, "clip_of vs the walk on the lattice of the replicated batch")
    same_lists(got, gm.tdt_total_decode(rep, ids), "clip_of vs enc replicated, clip_of = None")
    for h in range(len(ids)):
        same_lists([got[h]], gm.tdt_total_decode(encs[clip_of[h]][None], [ids[h]]), f"hypothesis {h} alone (uniform call)")
    same_lists(got[3:5], gm.tdt_total_decode(encs, ids[3:5], [1, 1]), "a call whose hypotheses leave clips 0 and 2 without a transcript")
    assert all(g["ok"] == 1 for g in got)


def test_shared_frames_two_lstm_layers_with_chunk_edges_inside_a_hypothesis(tmp_path_factory):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("total_2l"), "tiny2l")
    encs, ids, clip_of = shared_case(cfg, 4)
    got = gm.tdt_total_decode(encs, ids, clip_of)
    rep = [encs[c] for c in clip_of]
    for ch in (0, 50):                                              # 50 rows per heads product: edges inside hypothesis 0 (520 cells) and the others
        lats, _ = gm.tdt_lattice(rep, ids, chunk_rows=ch)
        same_lists(got, capi.tdt_total([(l["lab"], l["blk"], l["dl"]) for l in lats], list(cfg.durations)), f"chunk_rows {ch}")
    for h in (0, 1, 4):
        same(got[h], R.forward_total(*A.oracle_lattice(om, encs[clip_of[h]], ids[h]), list(cfg.durations)), f"tiny2l hypothesis {h} vs the specification")


def test_model_path_equals_the_specification_on_the_oracles_lattice(tiny_shared):
    cfg, om, gm, encs, ids, clip_of, got = tiny_shared
    for h in range(len(ids)):
        same(got[h], R.forward_total(*A.oracle_lattice(om, encs[clip_of[h]], ids[h]), list(cfg.durations)), f"hypothesis {h}")


def test_greedy_transcript_has_a_finite_total_above_its_alignment(tmp_path_factory):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("total_e2e"), "tiny")
    rng = np.random.default_rng(5)
    enc = normed(rng, (3, 30, cfg.hidden_size))
    g = om.tdt_greedy(enc)
    ids = [g["ids"][b, :g["lens"][b]] for b in range(3)]
    assert sum(len(i) for i in ids) > 3, "degenerate test: nothing decoded"
    got = gm.tdt_total_decode(enc, ids)
    al = gm.tdt_align_decode(enc, ids)
    for b in range(3):
        assert got[b]["ok"] == 1 and np.isfinite(got[b]["total"]) and got[b]["total"] >= al[b]["score"], (b, got[b], al[b]["score"])
    gm.set_boost_tokens([[1, 2]], 5.0)                               # a boost trie does not matter
    try:
        same_lists(gm.tdt_total_decode(enc, ids), got, "with a boost trie set")
    finally:
        gm.set_boost_tokens([], 5.0)
    ms = gm.tdt_total_decode_timed(enc, ids, reps=2)
    assert len(ms) == 3 and all(v > 0 for v in ms)


# ---- from PCM -------------------------------------------------------------------------------------------------------------------------------
def vocab_model(td, cfg):
    W = synth.synth_weights(cfg, seed=42)
    if cfg.ctc_vocab_size == 0:
        W = {k: v for k, v in W.items() if not k.startswith("ctc_decoder_")}
    wp, vp = str(td / (cfg.name + ".safetensors")), str(td / (cfg.name + "_vocab.txt"))
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    return capi.Model(wp, cfg, vocab_path=vp, device=0)


def test_score_tdt_from_pcm_equals_its_stages(tmp_path):
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, durations=[1, 2, 4], name="tiny-noctc-total")
    gm = vocab_model(tmp_path, cfg)
    try:
        clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 700, 48000))]
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        words = [p[1:] for p in synth.synth_vocab(cfg.vocab_size - 1) if p.startswith("▁")]
        texts = [" ".join(words[a:b]) for a, b in ((0, 3), (3, 5), (5, 11), (11, 15), (2, 4), (0, 0))]
        clip_of = [0, 1, 2, 3, 0, 3]                                # clip 2 (4 frames): more tokens than frames and no zero duration, ok = 0
        ids = [gm.tokenize(t) for t in texts]
        got = gm.score_tdt(clips, ids=ids, clip_of=clip_of)
        for h in range(len(ids)):
            same_lists([got[h]], gm.tdt_total_decode(enc[clip_of[h]][None], [np.asarray(ids[h], np.int32)]), f"transcript {h}: from PCM vs its stages")
        assert [g["ok"] for g in got] == [1, 1, 0, 1, 1, 1]
        same_lists(gm.score_tdt(clips, texts=texts, clip_of=clip_of), got, "the same transcripts given as text")
        same_lists(gm.score_tdt(clips, ids=ids[:4]), got[:4], "one transcript per clip, clip_of = None")
        with pytest.raises(capi.PkError) as e:                      # no CTC head: nothing to search with
            gm.transcribe_nbest_rescored(clips)
        assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    finally:
        gm.close()


RESCORE_SEED = 0                                                    # (the test asserts that this seed shows the re-ranking)


def test_transcribe_nbest_rescored_equals_its_stages(tmp_path):
    cfg = dataclasses.replace(pk.make_tiny_config(), name="tiny-hybrid-rescore")
    gm = vocab_model(tmp_path, cfg)
    try:
        clips = [synth.synth_pcm(1, n, seed=90 + RESCORE_SEED + i)[0] for i, n in enumerate((32000, 20000))]
        beam = gm.transcribe_nbest(clips, 8, 16, 4)
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        flat = [(c, h) for c in range(2) for h in beam[c]]
        tot = gm.tdt_total_decode(enc, [np.asarray(h["token_ids"], np.int32) for _, h in flat], [c for c, _ in flat])
        differs = 0
        for w in (0.0, 0.5, 1.0):
            got = gm.transcribe_nbest_rescored(clips, 8, 16, 4, tdt_weight=w)
            k = 0
            for c in range(2):
                n = len(beam[c])
                ctc = np.asarray([h["score"] for h in beam[c]], np.float32)
                tdt = np.asarray([t["total"] for t in tot[k:k + n]], np.float32)
                ok = [t["ok"] for t in tot[k:k + n]]
                k += n
                order, comb = R.rescore_order([max(1, len(h["token_ids"])) for h in beam[c]], ctc, tdt, ok, w)
                assert len(got[c]) == n
                for p, j in enumerate(order):
                    g = got[c][p]
                    assert g["token_ids"] == beam[c][j]["token_ids"] and g["text"] == beam[c][j]["text"], (w, c, p)
                    for key, want in (("ctc_score", ctc[j]), ("tdt_total", tdt[j]), ("score", comb[j])):
                        assert np.float32(g[key]).view(np.uint32) == np.float32(want).view(np.uint32), (w, c, p, key, g[key], want)
                if w == 0.0:
                    assert [g["token_ids"] for g in got[c]] == [h["token_ids"] for h in beam[c]]
                    assert [np.float32(g["score"]) for g in got[c]] == [np.float32(h["score"]) for h in beam[c]], "weight 0: the beam's own list"
                if w == 1.0:
                    differs += order != list(range(n))
        assert sum(len(b) for b in beam) >= 6 and differs >= 1, "pick a seed for which the TDT head re-ranks at least one clip's list"
    finally:
        gm.close()


# ---- facade and CLI -------------------------------------------------------------------------------------------------------------------------
def test_facade_score_and_rescored_nbest_through_the_cli(tmp_path):
    """Transcriber::score and transcribe_nbest(path, beam, rescore) compiled into examples/parakeet_cli (--score "text"; --nbest N --rescore-tdt W):
    what it prints are Model.score_tdt and Model.transcribe_nbest_rescored on the samples the WAV holds.  The CLI runs as a fresh child process."""
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
    want_score = gm.score_tdt([q], texts=[text])[0]
    want_list = gm.transcribe_nbest_rescored([q], 8, 16, 4, tdt_weight=0.5)[0]
    gm.close()
    assert want_score["ok"] == 1 and len(want_list) >= 2

    def run(*extra):
        return subprocess.run([exe, wp, ap, "--vocab", vp, *extra], capture_output=True, text=True, timeout=600)
    out = run("--score", text)
    assert out.returncode == 0, out.stderr
    sc = re.search(r"^Score \(tdt\): log-likelihood (\S+)$", out.stdout, flags=re.M).group(1)
    assert np.float32(sc) == np.float32(f"{want_score['total']:.4f}")
    out = run("--beam", "8", "--nbest", "4", "--rescore-tdt", "0.5")
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^#(\d+) \[(\S+)\] ctc (\S+) tdt (\S+) (.*)$", out.stdout, flags=re.M)
    assert rows == [(str(j + 1), f"{h['score']:.4f}", f"{h['ctc_score']:.4f}", f"{h['tdt_total']:.4f}", h["text"]) for j, h in enumerate(want_list)]
    assert run("--rescore-tdt", "0.5").returncode == 1, "--rescore-tdt needs --nbest"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("total_refuse")
    cfg, W, om, gm = model_of(tmp, "tiny")
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, cfg.hidden_size))
    enc2 = normed(rng, (2, 8, cfg.hidden_size))
    one = [np.asarray([1, 2], np.int32)]
    gm.tdt_total_decode(enc, one)                                    # (the buffers of a small call exist: a refused one must not grow or replace them)
    free0, _, held0 = capi.mem_info(gm)
    assert held0 > 0

    def refused(code, fn, *a, msg=None, **kw):
        with pytest.raises(capi.PkError) as e:
            fn(*a, **kw)
        assert e.value.code == code and (msg is None or msg in str(e.value)), (code, e.value.code, str(e.value))
        assert capi.mem_info(gm)[2] == held0, "a refused call changes no buffer of the model's workspace or scratch"

    refused(-1, gm.tdt_total_decode, enc2, one * 3, [0, 2, 1])       # clip_of out of range
    refused(-1, gm.tdt_total_decode, enc2, one * 3, [0, -1, 1])
    refused(-1, gm.tdt_total_decode, enc2, one * 3)                  # clip_of == NULL with n_hyp != n_clips
    for bad in ([cfg.blank_id], [-1], [cfg.vocab_size]):             # an id equal to blank, outside the vocabulary
        refused(-1, gm.tdt_total_decode, enc, [np.asarray(bad, np.int32)])
    L = capi.lib()
    z, zi = np.zeros(4, np.float32), np.zeros(4, np.int32)
    st = L.pk_tdt_total_decode(gm._h, capi._f(enc2), 2, 8, capi._i(np.asarray([1, 2], np.int32)), capi._i(np.asarray([0, 2, 1], np.int32)), None, 2,
                               capi._f(z), capi._i(zi))
    assert st == -1 and capi.mem_info(gm)[2] == held0, "decreasing offsets"
    refused(-7, gm.tdt_total_decode, enc, [np.ones(1536, np.int32)], msg="1535")      # U = 1536
    # past the 1 GiB scratch formula, one hypothesis alone: T = 30000, U = 1500, D = 5 -> 4 (45 000 000 + 45 030 000 x 6) = 1.26e9.  Refused before
    # anything is allocated or uploaded: the encoder rows handed in are host memory nobody reads.
    T, U = 30000, 1500
    assert 4 * (T * U + T * (U + 1) * 6) > 1 << 30
    refused(-7, gm.tdt_total_decode, np.zeros((1, T, cfg.hidden_size), np.float32), [np.ones(U, np.int32)], msg="cap")
    assert capi.mem_info(gm)[0] >= free0 - (256 << 20), "nothing is allocated for a refused call"
    refused(-7, gm.score_tdt, [synth.synth_pcm(1, 16000, seed=1)[0]], ids=[np.ones(1536, np.int32)])
    lat = [A.make_lattice("ties", 3, 1, 2, rng)]
    refused(-7, capi.tdt_total, lat, [0, 9])                        # the walk alone: a duration of 9
    refused(-7, capi.tdt_total, [A.make_lattice("ties", 3, 1, 9, rng)], [0] * 9)       # D = 9
    for kw, msg in ((dict(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt-tot"), "RNN-T"),
                    (dict(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tot"), "gemm_bf16")):
        c2 = G.tiny(**kw)
        wp = str(tmp / (c2.name + ".safetensors"))
        synth.save_weights(wp, synth.synth_weights(c2, seed=12))
        m2 = capi.Model(wp, c2, device=0)
        try:
            held2 = capi.mem_info(m2)[2]
            for fn, a, k in ((m2.tdt_total_decode, (enc, [np.asarray([1], np.int32)]), {}),
                             (m2.score_tdt, ([synth.synth_pcm(1, 16000, seed=1)[0]],), dict(ids=[[1]])),
                             (m2.transcribe_nbest_rescored, ([synth.synth_pcm(1, 16000, seed=1)[0]],), {})):
                with pytest.raises(capi.PkError) as e:
                    fn(*a, **k)
                assert e.value.code == -7, (c2.name, fn.__name__)
                assert capi.mem_info(m2)[2] == held2
            with pytest.raises(capi.PkError) as e:
                m2.tdt_total_decode(enc, [np.asarray([1], np.int32)])
            assert msg in str(e.value)
        finally:
            m2.close()
    cn = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc-tot")     # no CTC head: the rescored call has nothing to search with
    Wn = {k: v for k, v in synth.synth_weights(cn, seed=1).items() if not k.startswith("ctc_decoder_")}
    wp = str(tmp / "noctc.safetensors")
    synth.save_weights(wp, Wn)
    m3 = capi.Model(wp, cn, device=0)
    try:
        held3 = capi.mem_info(m3)[2]
        with pytest.raises(capi.PkError) as e:
            m3.transcribe_nbest_rescored([synth.synth_pcm(1, 16000, seed=1)[0]])
        assert e.value.code == -7 and "ctc_decoder_" in str(e.value) and capi.mem_info(m3)[2] == held3
        assert m3.tdt_total_decode(enc, one)[0]["ok"] == 1, "the total itself needs no CTC head"
    finally:
        m3.close()


def test_new_symbols_are_exported_and_declared():
    L = capi.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "parakeet_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", txt))       # the rule of tests/test_capi_exports.py
    for name in ("pk_tdt_total", "pk_tdt_total_decode", "pk_tdt_total_decode_ragged", "pk_tdt_total_decode_timed", "pk_tdt_score_pcm",
                 "pk_transcribe_pcm_nbest_rescored", "pk_diag_tdt_total_groups", "pk_diag_rescore_order"):
        assert name in declared and hasattr(L, name), name
    assert not [s for s in declared if not hasattr(L, s)]
