"""GPU: endpointing through the model (pk_stream_set_endpointing / pk_stream_endpoint / pk_stream_push_endpoint / pk_stream_reset_decoder, DESIGN.md
5.5.10) on a tiny streaming model with 3 lock-step streams and audio of noise bursts between stretches of zeros: the events against
tests/endpoint_ref.py fed the rows a twin session's pk_stream_mel returns, the transcript against twin sessions (plain pushes, and plain pushes with
pk_stream_reset_decoder where the specification says the prediction net restarts), the token rule, the combined call with keywords, and the calls
that must not change."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

import endpoint_ref as R

pytestmark = pytest.mark.gpu

bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
S, LEFT, RIGHT, CHUNK, N_CHUNKS = 3, 70, 1, 2560, 25               # 25 chunks of 160 ms: 4 s
OPT = dict(min_speech_ms=30, min_silence_ms=150, floor_window_ms=1000)


def make_pcm():
    """noise bursts of 0.25 .. 0.45 s between stretches of zeros of about 0.4 s, different in every stream"""
    rng = np.random.default_rng(77)
    pcm = np.zeros((S, CHUNK * N_CHUNKS), np.float32)
    for s in range(S):
        t = 1600 + 900 * s
        while t < pcm.shape[1] - 4000:
            n = int(rng.integers(4000, 7200))
            pcm[s, t:t + n] = (0.1 * rng.standard_normal(n)).astype(np.float32)
            t += n + int(rng.integers(5600, 7200))
    return pcm


def chunk(pcm, i):
    return pcm[:, i * CHUNK:(i + 1) * CHUNK]


def same_tokens(r, want, what):
    for k in ("ids", "lens", "start", "end"):
        assert np.array_equal(r[k], want[k]), (what, k, r[k], want[k])
    assert np.array_equal(bits(r["conf"]), bits(want["conf"])), what


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    """The audio; per chunk the mel rows and encoder rows of a twin session driven through the stage calls and the tokens of a twin driven through plain
    pushes; the specification's acoustic events per push -- computed once, shared by the tests."""
    cfg = G.tiny(num_layers=2, name="tiny-stream")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tend"), cfg, seed=5)
    pcm = make_pcm()
    a, c = capi.Stream(gm, S, LEFT, RIGHT), capi.Stream(gm, S, LEFT, RIGHT)
    mels, encs, plain = [], [], []
    for i in range(N_CHUNKS):
        m = a.mel(chunk(pcm, i))
        mels.append(m)
        e = a.encode(m) if m.shape[1] else None
        encs.append(e if e is not None and e.shape[1] else None)
        plain.append(c.push(chunk(pcm, i)))
    a.close(); c.close()
    opt = R.Options(cfg.mel_bins, V=cfg.vocab_size, blank=cfg.blank_id, **OPT)
    eps = [R.Endpointer(opt) for _ in range(S)]
    want = []                                                       # per push: (a, floor, speech0 [S][n], events ordered by stream then emission)
    for m in mels:
        if m.shape[1] == 0:
            want.append(None)
            continue
        per = [e.push(m[s]) for s, e in enumerate(eps)]
        want.append((np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]),
                     [(s,) + v for s, p in enumerate(per) for v in p[3]]))
    ends = [[v for w in want if w for v in w[3] if v[0] == s and v[1] == R.END] for s in range(S)]
    assert all(len(e) >= 2 for e in ends), ends                     # every stream ends at least two utterances
    toks = [sum((r["ids"][s, :r["lens"][s]].tolist() for r in plain), []) for s in range(S)]
    assert all(len(t) >= 4 for t in toks), [len(t) for t in toks]
    yield dict(cfg=cfg, gm=gm, pcm=pcm, mels=mels, encs=encs, plain=plain, want=want, toks=toks)


def run_against_twin(x, **opt):
    """A session that pushes through push_endpoint against (1) the specification fed the twin's mel rows and the ids the session itself returned,
    (2) a twin on which the test calls reset_decoder after the pushes in which the specification restarts a stream's prediction net.
    -> the events of every push"""
    gm, pcm, cfg = x["gm"], x["pcm"], x["cfg"]
    o = dict(OPT); o.update(opt)
    ropt = R.Options(cfg.mel_bins, V=cfg.vocab_size, blank=cfg.blank_id, **o)
    eps = [R.Endpointer(ropt) for _ in range(S)]
    b, t = capi.Stream(gm, S, LEFT, RIGHT), capi.Stream(gm, S, LEFT, RIGHT)
    out = []
    try:
        b.set_endpointing(**o)
        for i in range(N_CHUNKS):
            r = b.push_endpoint(chunk(pcm, i))
            same_tokens(r, t.push(chunk(pcm, i)), f"push {i}")
            m = x["mels"][i]
            ev, mask = [], [0] * S
            if m.shape[1]:
                for s, e in enumerate(eps):
                    v, reset = e.push_with_tokens(m[s], r["ids"][s, :r["lens"][s]])
                    ev += [(s,) + k for k in v]
                    mask[s] = int(reset)
            assert r["n_events"] == len(ev) and r["events"] == ev, f"push {i}: {r['events']} vs {ev}"
            if any(mask):
                t.reset_decoder(mask)
            out.append((ev, mask))
    finally:
        b.close(); t.close()
    return out


def test_events_equal_the_specification_and_the_transcript_is_unchanged_without_the_reset(session):
    x = session
    gm, pcm = x["gm"], x["pcm"]
    b, a = capi.Stream(gm, S, LEFT, RIGHT), capi.Stream(gm, S, LEFT, RIGHT)
    try:
        b.set_endpointing(reset_decoder=0, **OPT)
        a.set_endpointing(**OPT)
        for round_ in range(2):                                     # the second round after reset(): the options stay, the same audio repeats the events
            for i in range(N_CHUNKS):
                r = b.push_endpoint(chunk(pcm, i))
                same_tokens(r, x["plain"][i], f"round {round_} push {i}")
                want = x["want"][i]
                assert r["events"] == (want[3] if want else []), f"round {round_} push {i}: {r['events']} vs {want and want[3]}"
                if want and round_ == 0:                            # the stage form on the twin's rows: the same, and the rows bit for bit
                    g = a.endpoint(x["mels"][i], want_rows=True)
                    assert g["events"] == want[3], f"stage push {i}"
                    assert np.array_equal(bits(g["level"]), bits(want[0])) and np.array_equal(bits(g["floor"]), bits(want[1])), f"stage push {i}"
                    assert np.array_equal(g["speech0"], want[2])
            b.reset()
        for i in range(N_CHUNKS):                                   # push with endpointing set returns what it returns without it
            same_tokens(b.push(chunk(pcm, i)), x["plain"][i], f"plain push {i}")
        b.set_endpointing(False)                                    # cleared: endpoint calls are refused, push goes on
        with pytest.raises(capi.PkError) as e:
            b.push_endpoint(chunk(pcm, 0))
        assert e.value.code == -1
    finally:
        a.close(); b.close()


def test_transcript_with_the_reset_equals_a_twin_reset_by_hand(session):
    out = run_against_twin(session)
    n_reset = sum(sum(m) for _, m in out)
    assert n_reset >= 6, n_reset                                    # (every stream ends at least two utterances)
    assert [e for ev, _ in out for e in ev] == [e for w in session["want"] if w for e in w[3]]


def test_token_rule(session):
    x = session
    first = next(r for r in x["plain"] if r["lens"].sum())          # the first push that returns a token: nothing was closed before it
    s0 = int(np.argmax(first["lens"] > 0))
    eou = int(first["ids"][s0, 0])
    out = run_against_twin(x, eou_token_id=eou)
    tok = [(i, e) for i, (ev, _) in enumerate(out) for e in ev if e[2] == R.TOKEN]
    assert tok and tok[0][1][0] == s0, tok
    for i, e in tok:                                                # fired in the push that returned the token; end = at = the last frame fed
        assert e[1] == R.END and e[4] == e[5] and out[i][1][e[0]] == 1
    assert any(sum(m) == 1 for _, m in out)                         # a push that closes one stream alone (the twin comparison shows the others go on)


def test_reset_decoder_itself(session):
    x = session
    gm, pcm = x["gm"], x["pcm"]
    K = 9
    enc = np.concatenate([e for e in x["encs"][K:K + 8] if e is not None], axis=1)        # given encoder rows [S][c][d]
    offset = sum(e.shape[1] for e in x["encs"][:K] if e is not None)
    f, h, g = (capi.Stream(gm, S, LEFT, RIGHT) for _ in range(3))
    try:
        for i in range(K):
            f.push(chunk(pcm, i)); h.push(chunk(pcm, i))
        mask = [1, 0, 1]
        f.reset_decoder(mask)
        rf, rh, rg = f.decode(enc), h.decode(enc), g.decode(enc)
        assert rg["lens"].sum() > 0 and rh["lens"].sum() > 0
        for s in range(S):
            w = rg if mask[s] else rh
            n = w["lens"][s]
            assert rf["lens"][s] == n, s
            assert np.array_equal(rf["ids"][s, :n], w["ids"][s, :n]) and np.array_equal(bits(rf["conf"][s, :n]), bits(w["conf"][s, :n])), s
            off = offset if mask[s] else 0                          # a fresh session counts its frames from 0
            assert np.array_equal(rf["start"][s, :n], w["start"][s, :n] + off) and np.array_equal(rf["end"][s, :n], w["end"][s, :n] + off), s
    finally:
        f.close(); h.close(); g.close()


def test_combined_call_with_keywords(session):
    x = session
    gm, pcm, toks = x["gm"], x["pcm"], x["toks"]
    kws = [toks[0][:1], toks[1][1:3], toks[2][:2]]
    b, t = capi.Stream(gm, S, LEFT, RIGHT), capi.Stream(gm, S, LEFT, RIGHT)
    try:
        b.set_endpointing(reset_decoder=0, **OPT)
        with pytest.raises(capi.PkError) as e:                      # kws outputs with no keywords set
            b.push_endpoint(chunk(pcm, 0), spot=True)
        assert e.value.code == -1
        b.reset()
        b.set_keywords(ids=kws, patience=2)
        t.set_keywords(ids=kws, patience=2)
        n_kws = 0
        for i in range(N_CHUNKS):
            r, w = b.push_endpoint(chunk(pcm, i), spot=True), t.push_spot(chunk(pcm, i))
            same_tokens(r, w, f"push {i}")
            assert r["kws_n_events"] == w["n_events"] and len(r["kws_events"]) == len(w["events"])
            for p, q in zip(r["kws_events"], w["events"]):
                assert p[:4] == q[:4] and bits(p[4]) == bits(q[4]), (i, p, q)
            want = x["want"][i]
            assert r["events"] == (want[3] if want else []), f"push {i}"
            n_kws += w["n_events"]
        assert n_kws >= 1
    finally:
        b.close(); t.close()


def test_refusals(session, tmp_path_factory):
    x = session
    gm, cfg = x["gm"], x["cfg"]

    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.PkError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (code, e.value.code, str(e.value))

    a = capi.Stream(gm, S, LEFT, RIGHT)
    try:
        m = x["mels"][0]
        assert m.shape[1]
        refused(-1, a.endpoint, m)                                  # no options set
        a.set_endpointing(**OPT)
        refused(-1, a.set_endpointing, eou_token_id=cfg.blank_id)
        refused(-1, a.set_endpointing, eou_token_id=cfg.vocab_size)
        refused(-1, a.set_endpointing, min_silence_ms=5)
        refused(-7, a.set_endpointing, floor_window_ms=20000)
        refused(-7, a.endpoint, np.zeros((S, 513, cfg.mel_bins), np.float32))
        refused(-1, a.endpoint, np.zeros((S, 0, cfg.mel_bins), np.float32))
        got = a.endpoint(m, want_rows=True)                         # a refused set leaves the previous options in place, at frame 0
        assert got["events"] == x["want"][0][3] and np.array_equal(bits(got["floor"]), bits(x["want"][0][1]))
    finally:
        a.close()
    c2 = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-endpoint")
    wp = str(tmp_path_factory.mktemp("endpoint_refuse") / (c2.name + ".safetensors"))
    synth.save_weights(wp, synth.synth_weights(c2, seed=12))
    m2 = capi.Model(wp, c2, device=0)
    try:
        s2 = capi.Stream(m2, 2, LEFT, RIGHT)
        try:
            refused(-7, s2.set_endpointing)
        finally:
            s2.close()
    finally:
        m2.close()
