"""GPU: the TDT beam search with n-best output (kernels/tdt_beam.hip) against its written specification, tests/tdt_beam_ref.py driven by
the oracle's teacher-forced joint rows, BIT FOR BIT; its W = K = Kd = 1 form against the greedy loop; its scores against the alignment and
the forward total of the same ids; its refusals; and the one-call entry point against the staged call."""
import ctypes as C
import os

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth

import tdt_beam_ref as R

pytestmark = pytest.mark.gpu

_MODELS = {}


def model_of(tmp_path_factory, which):
    """(cfg, oracle model, device model) of the tiny configurations: vocabulary 33, one / two LSTM layers, D = 5 / 1."""
    if which in _MODELS:
        return _MODELS[which]
    import oracle
    kw = dict(vocab_size=33, blank_id=32, ctc_vocab_size=33, name="tiny-tbeam-" + which)
    if which == "d1-2l":
        kw.update(num_lstm_layers=2, durations=[1])
    cfg = G.tiny(**kw)
    W = {k: v.copy() for k, v in synth.synth_weights(cfg, seed=31).items()}
    pre = "tdt_joint_."
    if which == "zero":                                             # the zero duration wins: several symbols per frame
        W[pre + "duration_proj_.bias"][0] += 5.0
        W[pre + "label_proj_.bias"][-1] -= 2.0
    if which == "ties":                                             # two vocabulary rows with identical weights: exact score ties
        for a, b in ((3, 4), (10, 20)):
            W[pre + "label_proj_.weight"][b] = W[pre + "label_proj_.weight"][a]
            W[pre + "label_proj_.bias"][b] = W[pre + "label_proj_.bias"][a]
    wp = os.path.join(str(tmp_path_factory.mktemp("tbeam_" + which)), "w.safetensors")
    synth.save_weights(wp, W)
    _MODELS[which] = (cfg, oracle.Model(cfg, W), capi.Model(wp, cfg, device=0))
    return _MODELS[which]


def normed(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def same_as_reference(cfg, om, got, encs, W, K, Kd, N, mt, what):
    n_tok = 0
    for b, enc in enumerate(encs):
        want = R.search(R.oracle_joint(om, enc), enc.shape[0], cfg.blank_id, list(cfg.durations), W, K, Kd, N, mt)
        tag = f"{what} clip {b} (T = {enc.shape[0]})"
        assert got["ok"][b] == want["ok"], tag
        assert np.array_equal(got["lens"][b], want["lens"]), f"{tag}: lens {got['lens'][b]} vs {want['lens']}"
        for k in ("ids", "start", "end", "dur_idx"):
            assert np.array_equal(got[k][b], want[k]), f"{tag}: {k}"
        for k in ("score", "conf"):
            assert np.array_equal(G.bits(got[k][b]), G.bits(want[k])), f"{tag}: {k} bits {got[k][b]} vs {want[k]}"
        n_tok += int(want["lens"].sum())
    return n_tok


# (configuration, clips -- ("u", B, T): uniform call, ("r", T_0, T_1, ...): one packed ragged call --, W, K, Kd, N, max_tokens)
CASES = {
    "uniform-w3": ("d5", ("u", 3, 7), 3, 4, 2, 3, None),
    "uniform-w8-all-durations": ("d5", ("u", 2, 12), 8, 8, 5, 8, None),
    "w1": ("d5", ("u", 2, 12), 1, 1, 1, 1, None),
    "w16": ("d5", ("u", 1, 12), 16, 16, 2, 16, None),
    "ragged-21-rows": ("d5", ("r", 12, 1, 2, 7, 12, 1, 7), 3, 3, 1, 2, None),        # B W = 21: across the 16-row tile; clips of 1 frame finish at once
    "ragged-72-rows": ("d5", ("r", 12, 2, 7, 1, 12, 7, 2, 12, 1), 8, 4, 2, 8, None),  # B W = 72: across the 64-row tile
    "two-layers-d1-w16": ("d1-2l", ("u", 2, 7), 16, 16, 1, 16, None),
    "two-layers-d1-unfilled": ("d1-2l", ("u", 2, 1), 16, 1, 1, 16, None),             # T = 1, K = 1: two states exist, N = 16 slots
    "max-tokens": ("d5", ("u", 2, 7), 3, 3, 2, 3, 2),
    "zero-duration": ("zero", ("u", 2, 7), 3, 3, 1, 3, None),
    "zero-duration-max-tokens": ("zero", ("r", 7, 2, 1), 8, 3, 2, 4, 3),             # several symbols per frame against max_tokens = 3
    "ties": ("ties", ("u", 2, 7), 8, 8, 2, 8, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_bit_equals_the_specification(tmp_path_factory, name):
    which, shape, W, K, Kd, N, mt = CASES[name]
    cfg, om, gm = model_of(tmp_path_factory, which)
    rng = np.random.default_rng(len(name) * 7 + W)
    if shape[0] == "u":
        enc_arg = normed(rng, (shape[1], shape[2], cfg.hidden_size))
        encs = list(enc_arg)
    else:
        encs = [normed(rng, (T, cfg.hidden_size)) for T in shape[1:]]
        enc_arg = encs
    mt = mt or max(e.shape[0] for e in encs) * cfg.max_symbols_per_step
    got = gm.tdt_beam_decode(enc_arg, W, K, Kd, N, max_tokens=mt)
    n_tok = same_as_reference(cfg, om, got, encs, W, K, Kd, N, mt, name)
    assert n_tok > 0, "degenerate case: no hypothesis holds a token"
    if name == "two-layers-d1-unfilled":
        assert (got["score"][:, 2:] == -np.inf).all() and (got["lens"][:, 2:] == 0).all() and (got["score"][:, :2] > -np.inf).all()
    if name in ("max-tokens", "zero-duration", "zero-duration-max-tokens"):
        # (zero-duration: max_tokens = 70 labels of the first frames, then the blanks to the end: the search ends at its step cap T + max_tokens.
        #  Every arc adds at least one to t + len, so at the cap every hypothesis is finished: a clip cannot end there with ok = 0)
        assert got["lens"].max() == mt, "max_tokens was not reached"
    if which == "zero":
        same = [(got["start"][b, n, 1:L] == got["start"][b, n, :max(L - 1, 0)]).any() for b in range(len(encs)) for n in range(N) for L in [got["lens"][b, n]]]
        assert any(same), "no hypothesis holds two tokens of one frame"
    if name == "ties":
        assert (got["ids"] == 3).any() or (got["ids"] == 10).any(), "the tied rows never came up"


def test_width_one_is_the_greedy_loop(tmp_path_factory):
    n_tok = 0
    for which, B, T in (("d5", 3, 12), ("d5", 2, 7), ("d1-2l", 3, 12), ("d5", 2, 1), ("d1-2l", 1, 2)):
        cfg, om, gm = model_of(tmp_path_factory, which)
        enc = normed(np.random.default_rng(B * 100 + T), (B, T, cfg.hidden_size))
        g = gm.tdt_decode(enc)
        assert (g["steps"] < T * (cfg.max_symbols_per_step + 1) + 16).all() and (g["lens"] >= 0).all()
        mt = g["ids"].shape[1]
        r = gm.tdt_beam_decode(enc, 1, 1, 1, 1, max_tokens=mt)
        assert (r["ok"] == 1).all()
        assert np.array_equal(r["lens"][:, 0], g["lens"])
        for k in ("ids", "start", "end"):
            assert np.array_equal(r[k][:, 0], g[k]), (which, B, T, k)
        assert np.array_equal(G.bits(r["conf"][:, 0]), G.bits(g["conf"])), (which, B, T)
        n_tok += int(g["lens"].sum())
    assert n_tok > 3, "degenerate test: nothing decoded"


def test_scores_descend_hypotheses_differ_and_stay_below_the_alignment_and_the_total(tmp_path_factory):
    cfg, om, gm = model_of(tmp_path_factory, "d5")
    rng = np.random.default_rng(9)
    encs = [normed(rng, (T, cfg.hidden_size)) for T in (12, 7, 2)]
    N = 8
    r = gm.tdt_beam_decode(encs, 8, 8, 2, N)
    hyp_enc, hyp_ids, clip_of, scores = [], [], [], []
    for b in range(len(encs)):
        filled = int((r["score"][b] > -np.inf).sum())
        assert filled >= 2 and r["ok"][b] == 1
        sc = r["score"][b, :filled]
        assert (sc[:-1] >= sc[1:]).all(), "scores descend"
        strings = [tuple(r["ids"][b, n, :r["lens"][b, n]]) for n in range(filled)]
        assert len(set(strings)) == filled, "the hypotheses of a clip are distinct"
        for n in range(filled):
            hyp_enc.append(encs[b]); hyp_ids.append(np.asarray(strings[n], np.int32)); clip_of.append(b); scores.append(sc[n])
    al = gm.tdt_align_decode(hyp_enc, hyp_ids)
    tt = gm.tdt_total_decode(encs, hyp_ids, clip_of=clip_of)
    n_eq = 0
    for h, s in enumerate(scores):
        assert al[h]["ok"] == 1 and tt[h]["ok"] == 1
        assert s <= al[h]["score"], f"hypothesis {h}: a path's score {s} above the best path's {al[h]['score']}"
        assert s <= tt[h]["total"], f"hypothesis {h}: a path's score {s} above the sum over all paths {tt[h]['total']}"
        n_eq += int(np.float32(s).view(np.uint32) == np.float32(al[h]["score"]).view(np.uint32))
    assert n_eq >= 1, "for some hypothesis the search's path IS the best alignment"


def test_refusals(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tbeam_refuse")
    cfg, om, gm = model_of(tmp_path_factory, "d5")
    rng = np.random.default_rng(4)
    enc = normed(rng, (1, 8, cfg.hidden_size))
    for kw in (dict(beam_width=0), dict(beam_width=17), dict(label_prune=0), dict(label_prune=17), dict(duration_prune=0), dict(duration_prune=9),
               dict(n_best=0), dict(beam_width=4, n_best=5)):
        with pytest.raises(capi.PkError) as e:
            gm.tdt_beam_decode(enc, **kw)
        assert e.value.code == -7 and list(kw)[-1] in str(e.value), kw
    gm.set_boost_tokens([[1, 2]], 5.0)
    try:
        with pytest.raises(capi.PkError) as e:
            gm.tdt_beam_decode(enc)
        assert e.value.code == -7 and "boost" in str(e.value)
    finally:
        gm.set_boost_tokens([], 5.0)
    # the scratch cap: the two copies of the token strings alone are 2 B W max_tokens 4 bytes = 2 x 16 x 2^23 x 4 = 2^30.  Refused before anything
    # is allocated or written: the output arrays handed in are a few words nobody touches.
    gm.tdt_beam_decode(enc)                                          # (the buffers of a small call exist: a refused one must not grow or replace them)
    free0, _, held0 = capi.mem_info(gm)
    o = capi.tdt_beam_options(16, 16, 8, 1)
    z, zi = np.zeros(4, np.float32), np.zeros(4, np.int32)
    st = capi.lib().pk_tdt_beam_decode(gm._h, capi._f(enc), 1, 8, C.byref(o), 1 << 23, capi._i(zi), capi._i(zi), capi._f(z), None, None, None, None, None)
    buf = C.create_string_buffer(2048)
    capi.lib().pk_last_error(buf, 2048)
    assert st == -7 and b"cap" in buf.value
    free1, _, held1 = capi.mem_info(gm)
    assert held1 == held0 and free1 >= free0 - (256 << 20), "nothing is allocated for a refused call"
    assert not zi.any() and not z.any()
    for kw, msg in ((dict(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt-tbeam"), "RNN-T"),
                    (dict(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tbeam"), "gemm_bf16")):
        c2 = G.tiny(**kw)
        wp = str(tmp / (c2.name + ".safetensors"))
        synth.save_weights(wp, synth.synth_weights(c2, seed=12))
        m2 = capi.Model(wp, c2, device=0)
        try:
            with pytest.raises(capi.PkError) as e:
                m2.tdt_beam_decode(enc, max_tokens=8)
            assert e.value.code == -7 and msg in str(e.value)
            with pytest.raises(capi.PkError) as e:
                m2.transcribe_nbest_tdt([synth.synth_pcm(1, 16000, seed=1)[0]])
            assert e.value.code == -7
        finally:
            m2.close()
    nest = pk.make_nest_encoder_config(name="nest-tiny-tbeam", subsampling_channels=32, hidden_size=128, num_layers=2, num_heads=2, ffn_intermediate=256)
    wp = str(tmp / "nest.safetensors")
    synth.save_weights(wp, synth.synth_weights(nest, seed=12))
    m3 = capi.Model(wp, nest, device=0)                             # no prediction net, no joint
    try:
        with pytest.raises(capi.PkError) as e:
            m3.tdt_beam_decode(normed(rng, (1, 8, nest.hidden_size)), max_tokens=8)
        assert e.value.code == -7 and "joint" in str(e.value)
    finally:
        m3.close()


def test_one_call_from_pcm_equals_the_staged_call(tmp_path_factory):
    td = tmp_path_factory.mktemp("tbeam_pcm")
    import dataclasses
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc-tbeam")     # what tdt-600m is: no CTC head
    W = {k: v for k, v in synth.synth_weights(cfg, seed=42).items() if not k.startswith("ctc_decoder_")}
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    try:
        clips = [synth.synth_pcm(1, n, seed=80 + i)[0] for i, n in enumerate((24000, 9000, 16000))]
        with pytest.raises(capi.PkError) as e:
            gm.transcribe_nbest(clips, 4, 8, 2)
        assert e.value.code == -7, "no CTC head: the CTC n-best still refuses"
        res = gm.transcribe_nbest_tdt(clips, 4, 4, 2, 3, timestamps=True)
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        mt = max(e.shape[0] for e in enc) * cfg.max_symbols_per_step
        st = gm.tdt_beam_decode(enc, 4, 4, 2, 3, max_tokens=mt)
        n_tok = 0
        for i, hyps in enumerate(res):
            filled = int((st["score"][i] > -np.inf).sum())
            assert len(hyps) == filled >= 1
            for j, h in enumerate(hyps):
                L = int(st["lens"][i, j])
                assert h["token_ids"] == st["ids"][i, j, :L].tolist()
                assert np.float32(h["score"]).view(np.uint32) == st["score"][i, j].view(np.uint32)
                assert h["start"] == st["start"][i, j, :L].tolist() and h["end"] == st["end"][i, j, :L].tolist()
                assert np.array_equal(G.bits(np.asarray(h["conf"], np.float32)), G.bits(st["conf"][i, j, :L]))
                n_tok += L
        assert n_tok > 0
        plain = gm.transcribe_nbest_tdt(clips, 4, 4, 2, 3)
        assert [[h["token_ids"] for h in c] for c in plain] == [[h["token_ids"] for h in c] for c in res] and "start" not in plain[0][0]
    finally:
        gm.close()
