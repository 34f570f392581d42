"""GPU: the TDT beam search with n-gram LM shallow fusion (the kLm kernels of kernels/tdt_beam.hip) against its written specification,
tests/tdt_beam_lm_ref.py driven by the oracle's teacher-forced joint rows, BIT FOR BIT; its zero-weight form against the unfused search;
a model that changes the 1-best; the one-call entry point against the staged call; its refusals."""
import ctypes as C
import dataclasses
import functools
import os

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth

import ngram_lm_ref as NR
import tdt_beam_lm_ref as RL
import tdt_beam_ref as R
from test_gpu_tdt_beam import model_of, normed

pytestmark = pytest.mark.gpu

V = 33                                                              # the tiny configurations of test_gpu_tdt_beam.model_of
LMS = {                                                             # the three families of tests/test_gpu_ctc_beam_lm.py
    "order1": dict(order=1, density=1.0, unk=False, bos=False),
    "order3_sparse_unk": dict(order=3, density=0.5, unk=True, bos=False),
    "order5_sparse_bos": dict(order=5, density=0.5, unk=False, bos=True),
}


@functools.lru_cache(maxsize=None)
def lm_pair(name):
    """(reference model, device-side model) of one synthetic ARPA text over the ids 0 .. V - 2; shared by every test that needs it."""
    text = NR.make_arpa(V, seed=V + len(name), **LMS[name])
    return NR.RefLm(text), capi.Lm.from_text(text)


_CLIPS = {}


def clips_of(tmp_path_factory, which, shape, seed):
    """(enc argument of the call, [(enc of a clip, its memoised oracle joint)]): the joint rows of a clip are computed once, whatever the
    number of searches that walk it."""
    key = (which, shape, seed)
    if key not in _CLIPS:
        cfg, om, _ = model_of(tmp_path_factory, which)
        rng = np.random.default_rng(seed)
        if shape[0] == "u":
            arg = normed(rng, (shape[1], shape[2], cfg.hidden_size))
            encs = list(arg)
        else:
            encs = [normed(rng, (T, cfg.hidden_size)) for T in shape[1:]]
            arg = encs
        _CLIPS[key] = (arg, [(e, R.oracle_joint(om, e)) for e in encs])
    return _CLIPS[key]


def same_as_reference(cfg, got, clips, ref, alpha, beta, W, K, Kd, N, mt, what):
    n_tok = 0
    for b, (enc, joint) in enumerate(clips):
        want = RL.search(joint, enc.shape[0], cfg.blank_id, list(cfg.durations), ref, alpha, beta, W, K, Kd, N, mt)
        tag = f"{what} clip {b} (T = {enc.shape[0]})"
        assert got["ok"][b] == want["ok"], tag
        assert np.array_equal(got["lens"][b], want["lens"]), f"{tag}: lens {got['lens'][b]} vs {want['lens']}"
        for k in ("ids", "start", "end", "dur_idx"):
            assert np.array_equal(got[k][b], want[k]), f"{tag}: {k}"
        for k in ("score", "conf", "lm_score"):
            assert np.array_equal(G.bits(got[k][b]), G.bits(want[k])), f"{tag}: {k} bits {got[k][b]} vs {want[k]}"
        n_tok += int(want["lens"].sum())
    return n_tok


# (configuration, clips -- ("u", B, T): uniform call, ("r", T_0, T_1, ...): one packed ragged call --, W, K, Kd, N, max_tokens, [(model, alpha, beta)])
ALL = [(name, a, b) for name in sorted(LMS) for a, b in ((0.5, 0.75), (1.5, -0.5))]
CASES = {
    "uniform": ("d5", ("u", 3, 7), 3, 4, 2, 3, None, ALL),         # every family, a positive and a negative beta
    "w16": ("d5", ("u", 1, 12), 16, 16, 2, 16, None, [("order3_sparse_unk", 0.5, 0.75)]),          # the pool limit
    "ragged-21-rows": ("d5", ("r", 12, 1, 2, 7, 12, 1, 7), 3, 3, 1, 2, None, [("order5_sparse_bos", 1.5, -0.5)]),       # across the 16-row tile
    "ragged-72-rows": ("d5", ("r", 12, 2, 7, 1, 12, 7, 2, 12, 1), 8, 4, 2, 8, None, [("order3_sparse_unk", 1.5, -0.5)]),   # across the 64-row tile
    "two-layers-d1": ("d1-2l", ("u", 2, 7), 16, 16, 1, 16, None, [("order1", 0.5, 0.75), ("order5_sparse_bos", 0.5, 0.75)]),
    "max-tokens": ("d5", ("u", 2, 7), 3, 3, 2, 3, 2, [("order3_sparse_unk", 0.5, 0.75), ("order1", 1.5, -0.5)]),
    "zero-duration": ("zero", ("r", 7, 2, 1), 8, 3, 2, 4, 3, [("order5_sparse_bos", 0.5, 0.75), ("order3_sparse_unk", 1.5, -0.5)]),
    # exact acoustic ties: the unigrams of order1 tell the tied ids apart (the model breaks the tie); with alpha = 0 the tied ids keep equal f
    # and the position rule decides
    "ties": ("ties", ("u", 2, 7), 8, 8, 2, 8, None, [("order1", 0.5, 0.75), ("order3_sparse_unk", 0.0, -0.5)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_bit_equals_the_specification(tmp_path_factory, name):
    which, shape, W, K, Kd, N, mt, lms = CASES[name]
    cfg, om, gm = model_of(tmp_path_factory, which)
    assert cfg.vocab_size == V
    arg, clips = clips_of(tmp_path_factory, which, shape, len(name) * 7 + W)
    mt = mt or max(e.shape[0] for e, _ in clips) * cfg.max_symbols_per_step
    for lm_name, alpha, beta in lms:
        ref, lm = lm_pair(lm_name)
        got = gm.tdt_beam_decode(arg, W, K, Kd, N, max_tokens=mt, lm=lm, lm_alpha=alpha, lm_beta=beta)
        n_tok = same_as_reference(cfg, got, clips, ref, alpha, beta, W, K, Kd, N, mt, f"{name} {lm_name} a={alpha} b={beta}")
        assert n_tok > 0, "degenerate case: no hypothesis holds a token"
        if which == "zero":                                         # several tokens of one frame: the LM state advances more than once on a frame
            same = [(got["start"][b, n, 1:L] == got["start"][b, n, :max(L - 1, 0)]).any() for b in range(len(clips)) for n in range(N)
                    for L in [got["lens"][b, n]]]
            assert any(same), "no hypothesis holds two tokens of one frame"
        if which == "ties":
            assert np.isin(got["ids"], (3, 4, 10, 20)).any(), "the tied rows never came up"


@pytest.mark.parametrize("name", ["uniform", "ragged-21-rows", "zero-duration", "ties", "two-layers-d1"])
def test_zero_weights_are_the_unfused_search(tmp_path_factory, name):
    which, shape, W, K, Kd, N, mt, lms = CASES[name]
    cfg, om, gm = model_of(tmp_path_factory, which)
    arg, clips = clips_of(tmp_path_factory, which, shape, len(name) * 7 + W)
    mt = mt or max(e.shape[0] for e, _ in clips) * cfg.max_symbols_per_step
    plain = gm.tdt_beam_decode(arg, W, K, Kd, N, max_tokens=mt)
    assert "lm_score" not in plain and plain["lens"].sum() > 0
    for lm_name in sorted({x[0] for x in lms}):
        fused = gm.tdt_beam_decode(arg, W, K, Kd, N, max_tokens=mt, lm=lm_pair(lm_name)[1], lm_alpha=0.0, lm_beta=0.0)
        for key in ("ids", "lens", "score", "start", "end", "dur_idx", "conf", "ok"):
            assert np.array_equal(G.bits(plain[key]), G.bits(fused[key])), (lm_name, key)
        assert not G.bits(fused["lm_score"]).any(), "lm_score is +0.0 everywhere"


def test_a_model_that_favours_one_token_changes_the_one_best(tmp_path_factory):
    cfg, om, gm = model_of(tmp_path_factory, "d5")
    arg, clips = clips_of(tmp_path_factory, "d5", ("u", 3, 7), len("uniform") * 7 + 3)
    plain = gm.tdt_beam_decode(arg, 8, 8, 2, 8)
    b = int(np.argmax(plain["lens"][:, 0]))
    best = plain["ids"][b, 0, :plain["lens"][b, 0]].tolist()
    # a token some other hypothesis of the clip holds and the 1-best does not: the acoustic pruning proposes it
    others = [int(c) for n in range(1, 8) for c in plain["ids"][b, n, :plain["lens"][b, n]] if int(c) not in best]
    assert best and others, "degenerate test: the acoustic beam holds no alternative"
    text = RL.flip_arpa(V, others[0], lp_rest=-1.0)
    ref, lm = NR.RefLm(text), capi.Lm.from_text(text)
    fused = gm.tdt_beam_decode(arg, 8, 8, 2, 8, lm=lm, lm_alpha=1.0, lm_beta=1.0)
    got = fused["ids"][b, 0, :fused["lens"][b, 0]].tolist()
    assert got != best, "the model did not change the 1-best"
    assert got and all(c == others[0] for c in got), (best, got)
    mt = max(e.shape[0] for e, _ in clips) * cfg.max_symbols_per_step
    same_as_reference(cfg, fused, clips, ref, 1.0, 1.0, 8, 8, 2, 8, mt, "flip case")
    lm.close()


def test_one_call_from_pcm_equals_the_staged_call(tmp_path_factory):
    td = tmp_path_factory.mktemp("tbeam_lm_pcm")
    cfg = dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc-tbeam-lm")  # what tdt-600m is: no CTC head
    W = {k: v for k, v in synth.synth_weights(cfg, seed=42).items() if not k.startswith("ctc_decoder_")}
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, W)
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    text = NR.make_arpa(cfg.vocab_size, seed=3, **LMS["order3_sparse_unk"])
    lm = capi.Lm.from_text(text)
    try:
        clips = [synth.synth_pcm(1, n, seed=80 + i)[0] for i, n in enumerate((24000, 9000, 16000))]
        kw = dict(lm=lm, lm_alpha=1.5, lm_beta=-0.5)
        res = gm.transcribe_nbest_tdt(clips, 4, 4, 2, 3, timestamps=True, **kw)
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        mt = max(e.shape[0] for e in enc) * cfg.max_symbols_per_step
        st = gm.tdt_beam_decode(enc, 4, 4, 2, 3, max_tokens=mt, **kw)
        n_tok = 0
        for i, hyps in enumerate(res):
            filled = int((st["score"][i] > -np.inf).sum())
            assert len(hyps) == filled >= 1
            for j, h in enumerate(hyps):
                L = int(st["lens"][i, j])
                assert h["token_ids"] == st["ids"][i, j, :L].tolist()
                assert np.float32(h["score"]).view(np.uint32) == st["score"][i, j].view(np.uint32)
                assert np.float32(h["lm_score"]).view(np.uint32) == st["lm_score"][i, j].view(np.uint32)
                assert h["start"] == st["start"][i, j, :L].tolist() and h["end"] == st["end"][i, j, :L].tolist()
                n_tok += L
        assert n_tok > 0
        assert "lm_score" not in gm.transcribe_nbest_tdt(clips, 4, 4, 2, 3)[0][0]
        a, b = gm.tdt_beam_decode_timed(enc, 4, 4, 2, 3, max_tokens=mt, reps=1, lm=lm)
        assert a > 0 and b > 0
    finally:
        lm.close()
        gm.close()


def test_refusals(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tbeam_lm_refuse")
    cfg, om, gm = model_of(tmp_path_factory, "d5")
    _, lm = lm_pair("order1")
    enc = normed(np.random.default_rng(4), (1, 8, cfg.hidden_size))
    assert "lm_score" in gm.tdt_beam_decode(enc, lm=lm)              # (the buffers of a small fused call exist: a refused one must not grow or replace them)
    free0, _, held0 = capi.mem_info(gm)
    L = capi.lib()
    o, lo = capi.tdt_beam_options(4, 4, 2, 2), capi.lm_options()
    z, zi = np.zeros(2 * 64, np.float32), np.zeros(2 * 64, np.int32)

    def raw(model, lm_h, lm_opt, opt=o, mt=64):
        return L.pk_tdt_beam_decode_lm(model._h, capi._f(enc), 1, 8, C.byref(opt), mt, capi._i(zi), capi._i(zi), capi._f(z), None, None, None, None, None,
                                       lm_h, C.byref(lm_opt) if lm_opt is not None else None, None)
    assert raw(gm, None, lo) == -1, "lm == NULL"
    assert raw(gm, lm._h, capi.lm_options(alpha=float("nan"))) == -1 and raw(gm, lm._h, capi.lm_options(beta=float("inf"))) == -1
    wide = capi.Lm.from_text(NR.make_arpa(V + 4, seed=1, **LMS["order1"]))      # names the blank (32) and ids >= V
    blank_only = capi.Lm.from_text(NR.make_arpa(V + 1, seed=1, **LMS["order1"]))   # names the ids 0 .. 32: the blank, nothing >= V
    assert raw(gm, wide._h, lo) == -1 and raw(gm, blank_only._h, lo) == -1
    with pytest.raises(capi.PkError) as e:
        gm.tdt_beam_decode(enc, lm=wide)
    assert e.value.code == -1
    gm.set_boost_tokens([[1, 2]], 5.0)
    try:
        assert raw(gm, lm._h, lo) == -7
        with pytest.raises(capi.PkError) as e:
            gm.transcribe_nbest_tdt([synth.synth_pcm(1, 16000, seed=1)[0]], lm=lm)
        assert e.value.code == -7 and "boost" in str(e.value)
    finally:
        gm.set_boost_tokens([], 5.0)
    assert raw(gm, lm._h, lo, capi.tdt_beam_options(17, 4, 2, 2)) == -7, "options out of range"
    assert raw(gm, lm._h, lo, capi.tdt_beam_options(16, 16, 8, 1), 1 << 23) == -7, "the scratch cap"
    buf = C.create_string_buffer(2048)
    L.pk_last_error(buf, 2048)
    assert b"cap" in buf.value
    free1, _, held1 = capi.mem_info(gm)
    assert held1 == held0 and free1 >= free0 - (256 << 20), "nothing is allocated for a refused call"
    assert not zi.any() and not z.any()
    c2 = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tbeam-lm")
    wp = str(tmp / (c2.name + ".safetensors"))
    synth.save_weights(wp, synth.synth_weights(c2, seed=12))
    m2 = capi.Model(wp, c2, device=0)
    try:
        assert raw(m2, lm._h, lo, mt=8) == -7
        with pytest.raises(capi.PkError) as e:
            m2.tdt_beam_decode(enc, max_tokens=8, lm=lm)
        assert e.value.code == -7 and "gemm_bf16" in str(e.value)
    finally:
        m2.close()
    assert "lm_score" in gm.tdt_beam_decode(enc, lm=lm)              # and works again
    wide.close(); blank_only.close()


def test_facade_transcribe_nbest_tdt_with_a_model_through_the_cli(tmp_path):
    """Transcriber::transcribe_nbest_tdt(audio, opts, lm) compiled into examples/parakeet_cli (--beam W --beam-head tdt --lm file.arpa): the
    hypotheses it prints, with both scores, are those of Model.transcribe_nbest_tdt(..., lm=) on the samples the WAV holds."""
    import re
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "parakeet_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()                                      # the CLI's Transcriber is the 17-layer preset
    wp, vp, ap, lp = (str(tmp_path / n) for n in ("model.safetensors", "vocab.txt", "clip.wav", "m.arpa"))
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 32000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    text = NR.make_arpa(cfg.vocab_size, seed=9, **LMS["order3_sparse_unk"])
    with open(lp, "w") as f:
        f.write(text)
    gm, lm = capi.Model(wp, cfg, vocab_path=vp, device=0), capi.Lm.from_text(text)
    want = gm.transcribe_nbest_tdt([q], 4, 8, 2, 3, lm=lm, lm_alpha=1.5, lm_beta=-0.5)[0]
    lm.close(); gm.close()
    head = [exe, wp, ap, "--vocab", vp, "--beam", "4", "--nbest", "3", "--lm", lp, "--lm-alpha", "1.5", "--lm-beta", "-0.5"]
    out = subprocess.run(head + ["--beam-head", "tdt"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    toks = [[int(x) for x in m.split()] for m in re.findall(r"^Tokens \(\d+\):(.*)$", out.stdout, flags=re.M)]
    both = re.findall(r"=== Hypothesis \d+ score (\S+) lm (\S+) ===", out.stdout)
    assert len(want) >= 1 and len(both) == len(want) and "Beam search (tdt)" in out.stdout and "3-gram model" in out.stdout
    assert toks == [h["token_ids"] for h in want]
    assert [(np.float32(s), np.float32(l)) for s, l in both] == [(np.float32(h["score"]), np.float32(h["lm_score"])) for h in want]
    bad = subprocess.run(head + ["--beam-head", "tdt", "--rescore-tdt", "0.5"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--lm needs --beam W" in bad.stderr
