"""GPU: streaming TDT keyword spotting through the model (pk_stream_set_keywords / pk_stream_spot / pk_stream_push_spot) on a
tiny streaming model with 3 lock-step streams: the per-chunk lattice, walk and online rule against tests/tdt_kws_stream_ref.py run over the
un-normalised lattices of the existing offline diagnostic (Model.tdt_kws_lattice) on the session's concatenated encoder rows -- rows bit for bit,
events exactly --, the one-call form against the stage form, and the transcription with and without keywords."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

import tdt_kws_stream_ref as SR

pytestmark = pytest.mark.gpu

NEG = SR.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
S, LEFT, RIGHT, CHUNK, N_CHUNKS = 3, 70, 1, 2560, 19               # 19 chunks of 160 ms: about 3 s
PATIENCE = 2


def same_events(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} events vs {len(want)}: {got} vs {want}"
    for g, w in zip(got, want):
        assert g[:4] == w[:4] and bits(g[4]) == bits(w[4]), f"{what}: {g} vs {w}"


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    """The audio, the encoder rows and greedy tokens of every chunk (stage calls), the keywords cut from them, and the specification's rows and
    events over the same chunking -- computed once, shared by the tests."""
    cfg = G.tiny(num_layers=2, name="tiny-stream")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tspot"), cfg, seed=5)
    pcm = synth.synth_pcm(S, CHUNK * N_CHUNKS, seed=123)
    a = capi.Stream(gm, S, LEFT, RIGHT)
    encs, toks = [], [[] for _ in range(S)]                         # encs[i]: [S][c][d] or None where the chunk produced no frame
    for i in range(N_CHUNKS):
        m = a.mel(pcm[:, i * CHUNK:(i + 1) * CHUNK])
        e = a.encode(m) if m.shape[1] else m
        if e.shape[1] == 0:
            encs.append(None)
            continue
        encs.append(e)
        r = a.decode(e)
        for s in range(S):
            toks[s] += r["ids"][s, :r["lens"][s]].tolist()
    assert all(len(t) >= 4 for t in toks), [len(t) for t in toks]
    seen = set(sum(toks, []))
    never = next(v for v in range(cfg.vocab_size) if v != cfg.blank_id and v not in seen)
    kws = [toks[0][:1], toks[1][1:3], toks[2][:4], toks[0][1:4], [never, never, never]]
    n_kw = len(kws)
    whole = [np.concatenate([e[s] for e in encs if e is not None]) for s in range(S)]
    lat, guard = gm.tdt_kws_lattice([whole[p // n_kw] for p in range(S * n_kw)], [kws[p % n_kw] for p in range(S * n_kw)])
    lats = [(l["lab"], l["blk"], l["dl"], l["top"]) for l in lat]
    dur = list(cfg.durations)
    # the threshold: the median of the specification's finite scores (without a threshold), so that frames fall on both sides
    finite = np.concatenate([E[E > NEG] for E in (SR.ChunkWalk(len(kws[p % n_kw]), dur).push(*lats[p])[0] for p in range(S * n_kw))])
    min_score = np.float32(np.median(finite))
    spotters = [SR.Spotter(len(kws[p % n_kw]), dur, min_score, PATIENCE) for p in range(S * n_kw)]
    want, t0 = [], 0
    for e in encs:
        if e is None:
            want.append(None)
            continue
        c = e.shape[1]
        rows, ev = [], []
        for p, sp in enumerate(spotters):
            E, Bs, Ee, out = sp.push(*SR.cut(lats[p], t0, c))
            rows.append((E, Bs, Ee))
            ev += [(p // n_kw, p % n_kw, st, en, sc) for sc, st, en in out]
        want.append((rows, ev))
        t0 += c
    flush = []
    for p, sp in enumerate(spotters):
        flush += [(p // n_kw, p % n_kw, st, en, sc) for sc, st, en in sp.flush()]
    n_ev = sum(len(w[1]) for w in want if w) + len(flush)
    assert n_ev >= 3 and any(np.any((r[0] > NEG) & (r[0] < min_score)) for w in want if w for r in w[0])
    yield dict(cfg=cfg, gm=gm, pcm=pcm, a=a, encs=encs, kws=kws, min_score=float(min_score), want=want, flush=flush)
    a.close()


def test_stage_form_equals_the_specification(session):
    x = session
    a = x["a"]
    a.set_keywords(ids=x["kws"], min_score=x["min_score"], patience=PATIENCE)
    a.reset()
    for i, e in enumerate(x["encs"]):
        if e is None:
            continue
        got = a.spot(e, rows=True)
        rows, ev = x["want"][i]
        for p, (E, Bs, Ee) in enumerate(rows):
            assert np.array_equal(bits(got["E"][p]), bits(E)), f"chunk {i} pair {p}: E {got['E'][p]} vs {E}"
            assert np.array_equal(got["Bs"][p], Bs) and np.array_equal(got["Ee"][p], Ee), f"chunk {i} pair {p}: spans"
        assert got["n_events"] == len(ev)
        same_events(got["events"], ev, f"chunk {i}")
    same_events(a.spot_flush(), x["flush"], "flush")
    assert a.spot_flush() == []


def test_one_call_form_transcription_and_reset(session):
    x = session
    gm, pcm = x["gm"], x["pcm"]
    b, c = capi.Stream(gm, S, LEFT, RIGHT), capi.Stream(gm, S, LEFT, RIGHT)
    try:
        b.set_keywords(ids=x["kws"], min_score=x["min_score"], patience=PATIENCE)
        plain, n_tok = [], 0
        for i in range(N_CHUNKS):
            plain.append(c.push(pcm[:, i * CHUNK:(i + 1) * CHUNK]))
            n_tok += int(plain[-1]["lens"].sum())
        assert n_tok >= 12

        def same_tokens(r, i):
            for k in ("ids", "lens", "start", "end"):
                assert np.array_equal(r[k], plain[i][k]), (i, k)
            assert np.array_equal(bits(r["conf"]), bits(plain[i]["conf"])), i

        for round_ in range(2):                                     # the second round after reset(): the same audio repeats the same events
            for i in range(N_CHUNKS):
                r = b.push_spot(pcm[:, i * CHUNK:(i + 1) * CHUNK])
                same_tokens(r, i)
                want = x["want"][i][1] if x["want"][i] else []
                assert r["n_events"] == len(want)
                same_events(r["events"], want, f"round {round_} chunk {i}")
            same_events(b.spot_flush(), x["flush"], f"round {round_} flush")
            b.reset()
        for i in range(N_CHUNKS):                                   # push with keywords set returns what it returns without them
            same_tokens(b.push(pcm[:, i * CHUNK:(i + 1) * CHUNK]), i)
        b.set_keywords()                                            # cleared: spotting is refused, push goes on
        with pytest.raises(capi.PkError) as e:
            b.spot_flush()
        assert e.value.code == -1
    finally:
        b.close(); c.close()


def test_refusals(session, tmp_path_factory):
    x = session
    a, cfg = x["a"], x["cfg"]

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.PkError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (code, e.value.code, str(e.value))

    a.set_keywords(ids=x["kws"])
    refused(-1, a.set_keywords, ids=[[1]], patience=-1)
    refused(-1, a.set_keywords, ids=[[1]], min_score=0.25)
    refused(-1, a.set_keywords, ids=[[cfg.blank_id]])
    refused(-1, a.set_keywords, ids=[[1], []])
    refused(-7, a.set_keywords, ids=[[1] * 65])
    refused(-7, a.set_keywords, ids=[[1]] * 257)
    d = cfg.hidden_size
    refused(-7, a.spot, np.zeros((S, 63, d), np.float32))
    assert a.n_kw == len(x["kws"])                                  # a refused call leaves the set in place as it was
    a.reset()
    e0 = next(e for e in x["encs"] if e is not None)
    got = a.spot(e0, rows=True)
    assert got["E"].shape[0] == S * len(x["kws"])
    tmp = tmp_path_factory.mktemp("spot_refuse")
    for kw in (dict(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt-spot"),
               dict(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-spot")):
        c2 = G.tiny(**kw)
        wp = str(tmp / (c2.name + ".safetensors"))
        synth.save_weights(wp, synth.synth_weights(c2, seed=12))
        m2 = capi.Model(wp, c2, device=0)
        try:
            with pytest.raises(capi.PkError) as e:                  # (an RNN-T head is refused when the session is created)
                s2 = capi.Stream(m2, 2, LEFT, RIGHT)
                try:
                    s2.set_keywords(ids=[[1]])
                finally:
                    s2.close()
            assert e.value.code == -7, (c2.name, str(e.value))
        finally:
            m2.close()
