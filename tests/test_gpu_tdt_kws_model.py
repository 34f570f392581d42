"""GPU: the TDT keyword spotting through a model (csrc/tdt_kws.cpp, kernels/tdt_kws.hip): its lattice against the oracle's rows, the entry points
against the specification tests/tdt_kws_ref.py run on that lattice, shared and ragged calls, the greedy output as a keyword, the refusals, and
the call from PCM -- BIT FOR BIT."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth

import tdt_kws_ref as R

pytestmark = pytest.mark.gpu

NEG = R.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def model_of(tmp, which):
    """The tiny TDT configurations of tests/test_gpu_tdt_total.py; "noctc": a model without a CTC head."""
    if which == "tiny2l":
        cfg = G.tiny(num_lstm_layers=2, vocab_size=78, blank_id=77, ctc_vocab_size=78, durations=[0, 1, 2, 4], name="tiny2l-v78")
        return (cfg,) + G.make_pair(tmp, cfg, seed=31)
    import oracle
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc-kws")
    W = {k: v for k, v in synth.synth_weights(cfg, seed=42).items() if not k.startswith("ctc_decoder_")}
    wp, vp = str(tmp / (cfg.name + ".safetensors")), str(tmp / (cfg.name + "_vocab.txt"))
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    return cfg, W, oracle.Model(cfg, W), capi.Model(wp, cfg, vocab_path=vp, device=0)


def oracle_lattice(om, enc, ids):
    """tdt_align_ref.oracle_lattice with top: the maximum of the oracle's token log-prob row."""
    cfg = om.cfg
    dur = list(cfg.durations)
    i0, i1 = dur.index(0), dur.index(1)
    T, U, D = enc.shape[0], len(ids), len(dur)
    lab = np.zeros((T, U), np.float32); blk = np.zeros((T, U + 1), np.float32); dl = np.zeros((T, U + 1, D), np.float32)
    top = np.zeros((T, U + 1), np.float32)
    for u in range(U + 1):
        labels = np.asarray(list(ids[:u]) + [cfg.blank_id] * T, np.int32)
        didx = np.asarray([i0] * u + [i1] * T, np.int32)
        r = om.tdt_score(enc, labels, didx)
        rows = r["label_lp"][u:u + T]
        blk[:, u] = rows[:, cfg.blank_id]
        if u < U:
            lab[:, u] = rows[:, int(ids[u])]
        dl[:, u] = r["dur_lp"][u:u + T]
        top[:, u] = rows.max(axis=1)
    return lab, blk, dl, top


def ref_arrays(lats, dur, n_clips, n_kw, H, ms=NEG):
    """tdt_kws_ref on the lattices of the pairs (clip-major) -> the arrays of Model.tdt_kws_decode"""
    nh = np.zeros((n_clips, n_kw), np.int32); st = np.zeros((n_clips, n_kw, H), np.int32); en = np.zeros((n_clips, n_kw, H), np.int32)
    sc = np.zeros((n_clips, n_kw, H), np.float32)
    for p, l in enumerate(lats):
        r = R.spot(l["lab"], l["blk"], l["dl"], l["top"], dur, H, ms)
        c, k = divmod(p, n_kw)
        nh[c, k], st[c, k], en[c, k], sc[c, k] = r["n_hits"], r["start"], r["end"], r["score"]
    return dict(n_hits=nh, start=st, end=en, score=sc)


def same_arrays(a, b, what):
    for k in ("n_hits", "start", "end"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k}\n{a[k]}\nvs\n{b[k]}"
    assert np.array_equal(bits(a["score"]), bits(b["score"])), f"{what}: score bits\n{a['score']}\nvs\n{b['score']}"


@pytest.fixture(scope="module", params=["tiny2l", "noctc"])
def case(request, tmp_path_factory):
    cfg, W, om, gm = model_of(tmp_path_factory.mktemp("kws_" + request.param), request.param)
    rng = np.random.default_rng(9)
    encs = [normed(rng, (T, cfg.hidden_size)) for T in (40, 9, 21)]
    kws = [rng.integers(0, cfg.blank_id, size=L).astype(np.int32) for L in (3, 1, 12, 2)]
    kws[3][:1] = kws[0][:1]
    yield request.param, cfg, om, gm, encs, kws
    if request.param == "noctc":
        gm.close()


def test_lattice_equals_the_oracle_under_three_chunk_sizes(case):
    which, cfg, om, gm, encs, kws = case
    ids = [kws[0], kws[2], kws[1]]                                  # cells 160 / 117 / 42
    want = [oracle_lattice(om, e, i) for e, i in zip(encs, ids)]
    first = None
    for ch in (0, 40, 150):
        got, guard = gm.tdt_kws_lattice(encs, ids, chunk_rows=ch)
        assert np.all(guard == 0x7FC5A5A5), f"chunk_rows {ch}: a word past the written extent was touched"
        for b, (lab, blk, dl, top) in enumerate(want):
            G.assert_bits_equal(got[b]["blk"], blk, f"{which} chunk_rows {ch} utterance {b}: blank log-probs")
            G.assert_bits_equal(got[b]["dl"], dl, f"{which} chunk_rows {ch} utterance {b}: duration log-probs")
            G.assert_bits_equal(got[b]["top"], top, f"{which} chunk_rows {ch} utterance {b}: top")
            G.assert_bits_equal(got[b]["lab"], lab, f"{which} chunk_rows {ch} utterance {b}: label log-probs")
            assert np.all(got[b]["top"] >= got[b]["blk"]) and np.all(got[b]["top"][:, :-1] >= got[b]["lab"])
        if first is None:
            first = got
        for b in range(len(ids)):
            for k in ("lab", "blk", "dl", "top"):
                G.assert_bits_equal(got[b][k], first[b][k], f"{which} chunk_rows {ch} vs 0, utterance {b}: {k}")
    al, _ = gm.tdt_lattice(encs, ids)                               # the alignment's lattice: the same rows through the other activation kernel
    for b in range(len(ids)):
        for k in ("lab", "blk", "dl"):
            G.assert_bits_equal(first[b][k], al[b][k], f"{which} utterance {b}: {k} vs pk_diag_tdt_lattice")


def test_decode_equals_the_reference_shared_single_and_ragged(case):
    which, cfg, om, gm, encs, kws = case
    dur = list(cfg.durations)
    K, H, ms = len(kws), 4, np.float32(-30.0)
    rep = [encs[c] for c in range(len(encs)) for _ in range(K)]
    lats, _ = gm.tdt_kws_lattice(rep, kws * len(encs))
    want = ref_arrays(lats, dur, len(encs), K, H, ms)
    got = gm.tdt_kws_decode(encs, kws, max_hits=H, min_score=float(ms))
    same_arrays(got, want, f"{which}: the shared call vs the reference on the device's lattice")
    assert want["n_hits"].sum() > 0, "degenerate test: no hit anywhere"
    on_lattice = capi.tdt_kws([(l["lab"], l["blk"], l["dl"], l["top"]) for l in lats], dur, max_hits=H, min_score=float(ms))
    for k in ("n_hits", "start", "end", "score"):
        assert np.array_equal(on_lattice[k].reshape(got[k].shape).view(np.uint32), got[k].view(np.uint32)), f"{which}: pk_tdt_kws on the lattice: {k}"
    for c in range(len(encs)):                                      # every pair alone, through the uniform form
        for k in range(K):
            one = gm.tdt_kws_decode(encs[c][None], [kws[k]], max_hits=H, min_score=float(ms))
            same_arrays(one, {q: got[q][c:c + 1, k:k + 1] for q in got}, f"{which}: clip {c} keyword {k} alone")
    T = 12
    uni = np.stack([e[:T] if len(e) >= T else np.concatenate([e, encs[0][: T - len(e)]]) for e in encs])
    same_arrays(gm.tdt_kws_decode(uni, kws, max_hits=H), gm.tdt_kws_decode(list(uni), kws, max_hits=H), f"{which}: uniform vs ragged form")
    ms3 = gm.tdt_kws_decode_timed(encs, kws, max_hits=H, reps=2)
    assert len(ms3) == 3 and all(v > 0 for v in ms3)


def test_greedy_output_as_keyword_scores_plus_zero_at_the_greedy_frames(case):
    which, cfg, om, gm, encs, kws = case
    rng = np.random.default_rng(21)
    enc = normed(rng, (6, 30, cfg.hidden_size))
    g = gm.tdt_decode(enc)
    tested = 0
    for b in range(len(enc)):
        n = int(g["lens"][b])
        if n < 2:
            continue
        k = min(n, 3)
        starts = g["start"][b, :k]
        if np.any(np.bincount(starts) >= cfg.max_symbols_per_step):
            continue                                                # (the greedy loop's forced advance is no decision of the joint)
        r = gm.tdt_kws_decode(enc[b][None], [g["ids"][b, :k]], max_hits=16, min_score=0.0)
        hits = [(int(r["start"][0, 0, j]), int(r["end"][0, 0, j])) for j in range(r["n_hits"][0, 0])]
        assert (int(starts[0]), int(g["end"][b, k - 1])) in hits, (which, b, hits, starts, g["end"][b, :k])
        assert np.all(bits(r["score"][0, 0, : len(hits)]) == 0), "+0.0, sign bit clear"
        tested += 1
    assert tested > 0, "degenerate test: no clip decoded two tokens"


def test_refusals_allocate_nothing(case, tmp_path_factory):
    which, cfg, om, gm, encs, kws = case
    enc = encs[1][None]
    held0 = capi.mem_info(gm)[2]

    def refused(code, fn, *a, msg=None, **kw):
        with pytest.raises(capi.PkError) as e:
            fn(*a, **kw)
        assert e.value.code == code and (msg is None or msg in str(e.value)), (code, e.value.code, str(e.value))
        assert capi.mem_info(gm)[2] == held0, "a refused call changes no buffer of the model's workspace or scratch"

    one = [np.asarray([1, 2], np.int32)]
    refused(-7, gm.tdt_kws_decode, enc, [np.ones(65, np.int32)], msg="64")
    refused(-7, gm.tdt_kws_decode, enc, one, max_hits=0)
    refused(-7, gm.tdt_kws_decode, enc, one, max_hits=17)
    refused(-1, gm.tdt_kws_decode, enc, one, min_score=1.0)
    refused(-1, gm.tdt_kws_decode, enc, [np.zeros(0, np.int32)])
    for bad in ([cfg.blank_id], [-1], [cfg.vocab_size]):
        refused(-1, gm.tdt_kws_decode, enc, [np.asarray(bad, np.int32)])
    # one pair past the 1 GiB cap alone: T = 600000, L = 64, D durations -> 4 T (64 + 65 (2 + D)) + 16 T > 2^30; refused before the rows are read
    T = 600000
    assert 4 * T * (64 + 65 * (2 + len(cfg.durations))) > 1 << 30
    free0 = capi.mem_info(gm)[0]
    refused(-7, gm.tdt_kws_decode, np.zeros((1, T, cfg.hidden_size), np.float32), [np.ones(64, np.int32)], msg="cap")
    assert capi.mem_info(gm)[0] >= free0 - (256 << 20), "nothing is allocated for a refused call"
    refused(-7, gm.spot_tdt, [synth.synth_pcm(1, 16000, seed=1)[0]], ids=[np.ones(65, np.int32)])
    if which != "noctc":
        return
    with pytest.raises(capi.PkError) as e:                          # pk_spot_pcm keeps refusing a model without a CTC head
        gm.spot([synth.synth_pcm(1, 16000, seed=1)[0]], ids=[[1]])
    assert e.value.code == -7 and "ctc_decoder_" in str(e.value)
    tmp = tmp_path_factory.mktemp("kws_refuse")
    for kw, msg in ((dict(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt-kws"), "RNN-T"),
                    (dict(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-kws"), "gemm_bf16")):
        c2 = G.tiny(**kw)
        wp = str(tmp / (c2.name + ".safetensors"))
        synth.save_weights(wp, synth.synth_weights(c2, seed=12))
        m2 = capi.Model(wp, c2, device=0)
        try:
            held2 = capi.mem_info(m2)[2]
            for fn, a, k in ((m2.tdt_kws_decode, (enc, [np.asarray([1], np.int32)]), {}),
                             (m2.spot_tdt, ([synth.synth_pcm(1, 16000, seed=1)[0]],), dict(ids=[[1]]))):
                with pytest.raises(capi.PkError) as e:
                    fn(*a, **k)
                assert e.value.code == -7 and msg in str(e.value), (c2.name, fn.__name__, str(e.value))
                assert capi.mem_info(m2)[2] == held2
        finally:
            m2.close()


def test_spot_tdt_from_pcm_equals_its_stages(case):
    which, cfg, om, gm, encs, kws = case
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 700, 48000))]
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    H = 3
    got = gm.spot_tdt(clips, ids=[k.tolist() for k in kws], max_hits=H)
    want = gm.tdt_kws_decode(list(enc), kws, max_hits=H)
    f32 = np.float32
    n_all = 0
    for c in range(len(clips)):
        for k in range(len(kws)):
            n = int(want["n_hits"][c, k])
            assert len(got[c][k]) == n, (c, k)
            n_all += n
            for j in range(n):
                s, e, v = got[c][k][j]
                assert f32(s) == f32(f32(want["start"][c, k, j]) * f32(0.08)) and f32(e) == f32(f32(want["end"][c, k, j] + 1) * f32(0.08)), (c, k, j)
                assert bits(v) == bits(want["score"][c, k, j])
    assert n_all > 0
    if which == "noctc":                                            # phrases through the vocabulary
        words = [p[1:] for p in synth.synth_vocab(cfg.vocab_size - 1) if p.startswith("▁")]
        texts = [" ".join(words[0:2]), words[3]]
        by_text = gm.spot_tdt(clips, phrases=texts, max_hits=H)
        by_ids = gm.spot_tdt(clips, ids=[gm.tokenize(t) for t in texts], max_hits=H)
        assert by_text == by_ids
