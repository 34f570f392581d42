"""GPU: the Transformer LM end to end (pk_nlm_load / pk_nlm_score) against the float64 reference of tests/nlm_ref.py, packing and grouping bit
for bit, its refusals, and the n-best re-ranking (pk_nbest_rescore_nlm) on the lists of the CTC and the TDT beam search."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import nlm_ref as R
from conftest import pk
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 33, 46, 47, 48)
BOS, EOS, VLM = 65, 66, 67                                           # the tiny acoustic model's ids are 0 .. 63 (blank 64)
VARIANTS = {
    "pre": dict(pre_ln=True, has_final_norm=True, tied_head=True),
    "post": dict(pre_ln=False, has_final_norm=False, has_emb_norm=True, tied_head=False),
}
_LMS = {}


def lm_cfg(variant, eos=True, max_positions=48):
    return capi.nlm_config(vocab_size=VLM, max_positions=max_positions, hidden_size=64, num_layers=2, num_heads=2, ffn_intermediate=128, bos_id=BOS,
                           eos_id=EOS if eos else -1, **VARIANTS[variant])


def lm_of(tmp_path_factory, variant, eos=True, max_positions=48):
    """(cfg, weights, device model): the same weights with and without the end term"""
    key = (variant, eos, max_positions)
    if key not in _LMS:
        cfg = lm_cfg(variant, eos, max_positions)
        W = synth.synth_nlm_weights(lm_cfg(variant, True, max_positions), seed=11)
        wp = str(tmp_path_factory.mktemp("nlm") / "lm.safetensors")
        synth.save_weights(wp, W)
        _LMS[key] = (cfg, W, capi.NeuralLm(wp, cfg))
    return _LMS[key]


def strings(seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 64, n).astype(np.int32) for n in LENGTHS]


@pytest.mark.parametrize("eos", [True, False])
@pytest.mark.parametrize("variant", ["pre", "post"])
def test_scores_against_the_float64_reference(tmp_path_factory, variant, eos):
    cfg, W, lm = lm_of(tmp_path_factory, variant, eos)
    S = strings()
    total, ok, per = lm.score(S, token_logp=True)
    y = g = 0.0
    for b, ids in enumerate(S):
        ref = R.token_logp(W, cfg, ids)
        if ref is None:
            assert eos and len(ids) == 48 and ok[b] == 0 and total[b] == -np.inf and per[b] is None
            continue
        assert ok[b] == 1 and per[b].shape == ref.shape
        if len(ref) == 0:
            assert total[b].view(np.uint32) == 0                     # the empty string without an end term: +0.0
            continue
        f32 = R.token_logp(W, cfg, ids, np.float32)
        y = max(y, float(np.abs(f32.astype(np.float64) - ref).max()), abs(float(R.total_of(f32)) - float(ref.sum())))
        g = max(g, float(np.abs(per[b].astype(np.float64) - ref).max()), abs(float(total[b]) - float(ref.sum())))
        assert total[b].view(np.uint32) == R.total_of(per[b]).view(np.uint32), "total is the left-to-right fp32 sum of token_logp"
    assert ok[LENGTHS.index(47)] == 1 and (ok[LENGTHS.index(48)] == 1) == (not eos)
    print(f"nlm {variant} eos={eos}: GPU max distance to float64 {g:.3g}, fp32 NumPy's {y:.3g}, ratio {g / y:.3g} (bound 4)")
    assert g <= 4 * y, f"GPU distance {g:.3g} > 4 x the fp32 NumPy evaluation's {y:.3g}"


@pytest.mark.parametrize("variant", ["pre", "post"])
def test_packing_and_grouping_do_not_change_bits(tmp_path_factory, variant):
    cfg, W, lm = lm_of(tmp_path_factory, variant, True)
    S = strings()[:-1]                                               # (48 is not scored with the end term)
    total, ok, per = lm.score(S, token_logp=True)
    for b, ids in enumerate(S):
        t1, ok1, p1 = lm.score([ids], token_logp=True)
        assert ok1[0] == 1 and t1[0].view(np.uint32) == total[b].view(np.uint32)
        assert np.array_equal(p1[0].view(np.uint32), per[b].view(np.uint32)), f"length {len(ids)} alone differs from the batch"
    rng = np.random.default_rng(5)
    pick = rng.permutation(np.arange(300) % len(S))
    lm.set_scratch_cap(2 << 20)                                      # about a thousand rows per group: the call crosses host group boundaries
    try:
        t3, ok3, p3 = lm.score([S[i] for i in pick], token_logp=True)
        assert lm.last_groups() > 1
    finally:
        lm.set_scratch_cap(0)
    for q, i in enumerate(pick):
        assert ok3[q] == 1 and t3[q].view(np.uint32) == total[i].view(np.uint32)
        assert np.array_equal(p3[q].view(np.uint32), per[i].view(np.uint32)), f"copy {q} of length {len(S[i])} differs"
    t4, _, p4 = lm.score([S[i] for i in pick], token_logp=True)      # one group
    assert lm.last_groups() == 1 and np.array_equal(t4.view(np.uint32), t3.view(np.uint32))


def test_no_leak_end_to_end(tmp_path_factory):
    cfg, W, lm = lm_of(tmp_path_factory, "pre", True)
    a = strings()[LENGTHS.index(33)]
    b = a.copy()
    b[-1] = (b[-1] + 1) % 64
    _, _, pa = lm.score([a], token_logp=True)
    _, _, pb = lm.score([b], token_logp=True)
    assert np.array_equal(pa[0][:32].view(np.uint32), pb[0][:32].view(np.uint32))
    assert pa[0][32] != pb[0][32] and pa[0][33] != pb[0][33]


def test_refusals_allocate_nothing(tmp_path_factory):
    """Free device memory before and after (other processes share the device: 1 MiB of slack).  So that the check can see an allocation, the refused
    loads are of a model whose weights are 6 MiB and the refused calls would need 16 MiB of scratch more than the handle holds."""
    cfg, W, lm = lm_of(tmp_path_factory, "pre", True)
    lm.score(strings())                                              # warm: small buffers only
    big = capi.nlm_config(vocab_size=VLM, max_positions=48, hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, bos_id=BOS, eos_id=EOS,
                          **VARIANTS["pre"])
    Wb = synth.synth_nlm_weights(big, seed=2)
    assert sum(v.nbytes for v in Wb.values()) > (6 << 20)
    tmp = tmp_path_factory.mktemp("nlm_bad")
    wp, nopos = str(tmp / "lm.safetensors"), str(tmp / "nopos.safetensors")
    synth.save_weights(wp, Wb)
    synth.save_weights(nopos, {k: v for k, v in Wb.items() if k != "pos_emb_.weight"})
    rng = np.random.default_rng(4)
    many = [rng.integers(0, 64, 40).astype(np.int32) for _ in range(200)]      # 8200 rows x 2 KB of scratch if it ran
    free0 = capi.mem_info()[0]
    for bad, msg in (([1, 2, BOS, 3], "bos_id"), ([1, VLM, 3], "vocabulary"), ([1, -1], "vocabulary")):
        with pytest.raises(capi.PkError) as e:
            lm.score(many + [np.asarray(bad, np.int32)])
        assert e.value.code == -1 and msg in str(e.value)
    with pytest.raises(capi.PkError) as e:
        capi.NeuralLm(wp, capi.nlm_config(vocab_size=VLM, max_positions=513, hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, bos_id=BOS,
                                          eos_id=EOS, **VARIANTS["pre"]))
    assert e.value.code == -7 and "512" in str(e.value)
    with pytest.raises(capi.PkError) as e:
        capi.NeuralLm(nopos, big)
    assert e.value.code == -3 and "pos_emb_.weight" in str(e.value)
    with pytest.raises(capi.PkError) as e:                           # the LAST tensor the encoder would upload is missing: refused before the first upload
        synth.save_weights(nopos, {k: v for k, v in Wb.items() if k != "final_norm_.bias"})
        capi.NeuralLm(nopos, big)
    assert e.value.code == -3 and "final_norm_.bias" in str(e.value)
    assert capi.mem_info()[0] >= free0 - (1 << 20), "a refused call allocated device memory"
    ok_lm = capi.NeuralLm(wp, big)                                   # the file itself loads, and the check above would have seen it
    try:
        assert capi.mem_info()[0] <= free0 - (5 << 20)
    finally:
        ok_lm.close()


def am_models(tmp_path_factory):
    td = tmp_path_factory.mktemp("nlm_am")
    out = {}
    for name in ("ctc", "tdt"):
        cfg = pk.make_tiny_config() if name == "ctc" else dataclasses.replace(pk.make_tiny_config(), ctc_vocab_size=0, name="tiny-noctc-nlm")
        W = {k: v for k, v in synth.synth_weights(cfg, seed=42).items() if name == "ctc" or not k.startswith("ctc_decoder_")}
        wp, vp = str(td / f"{name}.safetensors"), str(td / f"{name}_vocab.txt")
        synth.save_weights(wp, W)
        synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
        out[name] = capi.Model(wp, cfg, vocab_path=vp, device=0)
    return out


def nbest_of(gm, name, clips, **kw):
    if name == "ctc":
        return gm.transcribe_nbest(clips, 8, None, 4, timestamps=True, **kw)
    return gm.transcribe_nbest_tdt(clips, 8, None, None, 4, timestamps=True, **kw)


def same_hyp(a, b):
    return all(a[k] == b[k] for k in ("text", "token_ids", "start", "end", "words")) and np.array_equal(
        G.bits(np.asarray(a["conf"], np.float32)), G.bits(np.asarray(b["conf"], np.float32)))


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def test_reranking_of_ctc_and_tdt_lists(tmp_path_factory):
    cfg, W, lm = lm_of(tmp_path_factory, "pre", True)
    models = am_models(tmp_path_factory)
    clips = [synth.synth_pcm(1, n, seed=80 + i)[0] for i, n in enumerate((24000, 9000, 16000))]
    try:
        for name, gm in models.items():
            base = nbest_of(gm, name, clips)
            assert sum(len(c) for c in base) > len(clips), "the search must return lists worth re-ranking"
            alpha, beta = 0.7, 0.3
            res = nbest_of(gm, name, clips, nlm=lm, nlm_alpha=alpha, nlm_beta=beta)
            moved = 0
            for hyps0, hyps in zip(base, res):
                assert len(hyps) == len(hyps0)
                key0 = [tuple(h["token_ids"]) for h in hyps0]
                assert len(set(key0)) == len(key0)
                perm = [key0.index(tuple(h["token_ids"])) for h in hyps]
                assert sorted(perm) == list(range(len(hyps0))), "the slots are a permutation of the incoming ones"
                moved += perm != sorted(perm)
                for h, j in zip(hyps, perm):
                    assert same_hyp(h, hyps0[j]) and f32bits(h["am_score"]) == f32bits(hyps0[j]["score"])
                tot, ok = lm.score([np.asarray(h["token_ids"], np.int32) for h in hyps])
                assert all(ok) and [f32bits(h["nlm_score"]) for h in hyps] == [f32bits(t) for t in tot]
                lens = [len(h["token_ids"]) for h in hyps]
                # the rule on the incoming list gives the returned order; on the returned list it is the identity
                tot0, ok0 = lm.score([np.asarray(h["token_ids"], np.int32) for h in hyps0])
                o0, c0 = capi.diag_nlm_order([h["score"] for h in hyps0], tot0, [len(k) for k in key0], ok0, alpha, beta)
                assert list(o0) == perm and [f32bits(h["score"]) for h in hyps] == [f32bits(c0[j]) for j in perm]
                o1, c1 = capi.diag_nlm_order([h["am_score"] for h in hyps], [h["nlm_score"] for h in hyps], lens, [1] * len(hyps), alpha, beta)
                assert list(o1) == list(range(len(hyps))) and [f32bits(c) for c in c1] == [f32bits(h["score"]) for h in hyps]
            print(f"{name}: {moved} of {len(base)} lists changed order")
            # alpha = beta = 0: bit for bit the incoming lists
            ident = nbest_of(gm, name, clips, nlm=lm, nlm_alpha=0.0, nlm_beta=0.0)
            for hyps0, hyps in zip(base, ident):
                assert len(hyps) == len(hyps0)
                assert all(same_hyp(a, b) and f32bits(a["score"]) == f32bits(b["score"]) for a, b in zip(hyps, hyps0))
            # the Python two-call route: the same lists
            two = lm.rescore(base, alpha, beta)
            for hyps2, hyps in zip(two, res):
                assert [h["token_ids"] for h in hyps2] == [h["token_ids"] for h in hyps]
                for k in ("score", "am_score", "nlm_score"):
                    assert [f32bits(h[k]) for h in hyps2] == [f32bits(h[k]) for h in hyps], k
            # a hypothesis too long for max_positions sorts last with -inf
            # max_positions = the shortest hypothesis's positions (its tokens + the end term): it fits, every longer one does not
            all_lens = sorted(len(h["token_ids"]) for c in base for h in c)
            assert all_lens[0] < all_lens[-1], f"{name}: every hypothesis has {all_lens[0]} tokens: no max_positions separates them"
            cut = all_lens[0] + 1
            _, _, short = lm_of(tmp_path_factory, "pre", True, max_positions=cut)
            res2 = nbest_of(gm, name, clips, nlm=short, nlm_alpha=alpha, nlm_beta=beta)
            n_fit = n_long = 0
            for hyps0, hyps in zip(base, res2):
                assert sorted(tuple(h["token_ids"]) for h in hyps) == sorted(tuple(h["token_ids"]) for h in hyps0)
                fits = [len(h["token_ids"]) + 1 <= cut for h in hyps]
                assert fits == sorted(fits, reverse=True), "unscored hypotheses come after every scored one"
                for h, f in zip(hyps, fits):
                    assert (h["score"] == -np.inf and h["nlm_score"] == -np.inf) == (not f)
                    assert f32bits(h["am_score"]) == f32bits(next(g["score"] for g in hyps0 if g["token_ids"] == h["token_ids"]))
                long_ids = [h["token_ids"] for h, f in zip(hyps, fits) if not f]
                assert long_ids == [h["token_ids"] for h in hyps0 if len(h["token_ids"]) + 1 > cut], "unscored hypotheses keep the incoming order"
                n_fit += sum(fits)
                n_long += len(fits) - sum(fits)
            assert n_fit > 0 and n_long > 0
            print(f"{name}: max_positions {cut}: {n_fit} hypotheses scored, {n_long} too long")
            # lm= and nlm= together are refused before the search runs
            with pytest.raises(ValueError):
                nbest_of(gm, name, clips, lm=object(), nlm=lm)
    finally:
        for gm in models.values():
            gm.close()


def test_cli_reranks_both_searches_with_the_nlm_flags(tmp_path):
    """examples/parakeet_cli --beam W --nbest N --nlm file --nlm-heads H --nlm-bos ID --nlm-eos ID (the CTC search, and --beam-head tdt): the
    hypotheses it prints, with the combined score and both parts, are those of Model.transcribe_nbest*(..., nlm=) on the samples the WAV holds."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "parakeet.cpp_amd", "examples", "parakeet_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    cfg = pk.make_110m_config()                                      # the CLI's Transcriber is the 17-layer preset: ids 0 .. 1023, blank 1024
    wp, vp, ap, lp = (str(tmp_path / n) for n in ("model.safetensors", "vocab.txt", "clip.wav", "lm.safetensors"))
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(1024))
    pcm = synth.synth_pcm(1, 32000, seed=21)[0]
    synth.write_wav_pcm16(ap, pcm)
    q = (np.clip(pcm, -1, 1) * 32767.0).astype("<i2").astype(np.float32) / 32768.0    # what the WAV holds
    lc = capi.nlm_config(vocab_size=1027, max_positions=512, hidden_size=64, num_layers=2, num_heads=2, ffn_intermediate=128, bos_id=1025, eos_id=1026,
                         **VARIANTS["pre"])
    synth.save_weights(lp, synth.synth_nlm_weights(lc, seed=3))
    gm, lm = capi.Model(wp, cfg, vocab_path=vp, device=0), capi.NeuralLm(lp, lc)
    want = {"ctc": gm.transcribe_nbest([q], 4, 16, 3, nlm=lm, nlm_alpha=0.8, nlm_beta=0.25)[0],
            "tdt": gm.transcribe_nbest_tdt([q], 4, 8, 2, 3, nlm=lm, nlm_alpha=0.8, nlm_beta=0.25)[0]}
    lm.close(); gm.close()
    head = [exe, wp, ap, "--vocab", vp, "--beam", "4", "--nbest", "3", "--nlm", lp, "--nlm-heads", "2", "--nlm-bos", "1025", "--nlm-eos", "1026",
            "--nlm-alpha", "0.8", "--nlm-beta", "0.25"]
    for name, extra in (("ctc", ["--decoder", "ctc"]), ("tdt", ["--beam-head", "tdt"])):
        out = subprocess.run(head + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        toks = [[int(x) for x in m.split()] for m in re.findall(r"^Tokens \(\d+\):(.*)$", out.stdout, flags=re.M)]
        parts = re.findall(r"=== Hypothesis \d+ score (\S+) am (\S+) nlm (\S+) ===", out.stdout)
        assert len(want[name]) >= 1 and len(parts) == len(want[name]) and f"Beam search ({name})" in out.stdout and "Transformer LM (2 layers" in out.stdout
        assert toks == [h["token_ids"] for h in want[name]]
        assert [tuple(np.float32(x) for x in p) for p in parts] == [tuple(np.float32(h[k]) for k in ("score", "am_score", "nlm_score")) for h in want[name]]
    bad = subprocess.run(head + ["--decoder", "ctc", "--lm", "x.arpa"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--nlm needs" in bad.stderr
    bad = subprocess.run([a for a in head if a not in ("--nlm-bos", "1025")] + ["--decoder", "ctc"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--nlm needs" in bad.stderr
