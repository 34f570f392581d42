"""CPU checks of the neural LM rescoring reference (tests/nlm_ref.py) and of the host-only entry points of the C boundary: the re-ranking
rule (pk_diag_nlm_order) and pk_nlm_config_infer.  No device is needed."""
import numpy as np
import pytest

import nlm_ref as R
from parakeet_cpp_amd import capi, synth


def small_cfg(**kw):
    c = dict(vocab_size=23, max_positions=12, hidden_size=32, num_layers=2, num_heads=2, ffn_intermediate=64, pre_ln=True, has_final_norm=True,
             tied_head=True, bos_id=21, eos_id=22)
    c.update(kw)
    return capi.nlm_config(**c)


def test_causal_reference_is_full_attention_with_a_minus_inf_upper_triangle():
    rng = np.random.default_rng(3)
    for T, hd in ((1, 8), (2, 8), (33, 24), (70, 16)):
        q, k, v = (rng.standard_normal((T, hd)) for _ in range(3))
        ctx, bound, sigma = R.causal_head_reference(q, k, v, 0.25)
        assert np.abs(ctx - R.masked_full_attention(q, k, v, 0.25)).max() < 1e-13
        assert np.all(bound > 0) and np.all(sigma > 0) and np.all(sigma <= bound)
    # row 0 attends to key 0 alone: ctx_0 = v_0 whatever the scores are
    assert np.array_equal(R.causal_head_reference(q, k, v, 0.25)[0][0], v[0])


@pytest.mark.parametrize("kw", [dict(), dict(pre_ln=False, has_final_norm=False, has_emb_norm=True, tied_head=False), dict(eos_id=-1)])
def test_prefix_property_and_normalisation(kw):
    cfg = small_cfg(**kw)
    W = synth.synth_nlm_weights(cfg, seed=5)
    rng = np.random.default_rng(1)
    ids = rng.integers(0, 21, 9)
    full = R.token_logp(W, cfg, ids)
    end = 1 if cfg.eos_id >= 0 else 0
    assert full.shape == (9 + end,) and np.all(full < 0)
    for n in (0, 1, 4, 8):
        part = R.token_logp(W, cfg, ids[:n])
        assert part.shape == (n + end,)
        assert np.abs(part[:n] - full[:n]).max(initial=0.0) < 1e-12        # a prefix's log-probs are the first entries of the longer string's
    allp = R.token_logp(W, cfg, ids, all_targets=True)
    assert allp.shape == (9 + end, cfg.vocab_size)
    assert np.abs(np.exp(allp).sum(axis=1) - 1.0).max() < 1e-12
    assert np.array_equal(allp[np.arange(9), ids], full[:9])
    # the softmaxes of the synthetic weights spread: no position is one-hot, none is uniform
    top = np.exp(allp).max(axis=1)
    assert top.max() < 0.9 and top.min() > 1.5 / cfg.vocab_size
    # fp32 yardstick: the same function, close to the float64 one
    assert np.abs(R.token_logp(W, cfg, ids, np.float32) - full).max() < 1e-4
    # too long: not scored
    assert R.token_logp(W, cfg, rng.integers(0, 21, cfg.max_positions + 1 - end)) is None
    assert R.token_logp(W, cfg, rng.integers(0, 21, cfg.max_positions - end)) is not None


def test_head_reference_bound_is_positive_and_small():
    rng = np.random.default_rng(2)
    h, W, b = rng.standard_normal((5, 64)), rng.standard_normal((33, 64)) / 8, rng.standard_normal(33)
    lp, bound = R.head_logp_reference(h, W, b)
    assert np.abs(np.exp(lp).sum(axis=1) - 1).max() < 1e-12
    assert np.all(bound > 0) and bound.max() < 1e-3
    t = np.array([0, 32, 5, 7, 1])
    lp_t, bound_t = R.head_logp_reference(h, W, b, t)
    assert np.array_equal(lp_t, lp[np.arange(5), t]) and np.array_equal(bound_t, bound[np.arange(5), t])


ORDER_CASES = [
    # am, nlm, lens, ok
    ([-1.0, -2.0, -3.0, -2.0], [-5.0, -1.0, -1.0, -1.0], [3, 3, 3, 3], [1, 1, 1, 1]),                # a tie between slots 1 and 3: incoming order kept
    ([-1.0, -2.0, -3.0, -4.0], [-9.0, -1.0, -1.0, -0.5], [2, 4, 0, 7], [1, 0, 1, 0]),                # ok = 0 slots go last, in incoming order
    ([-1.0, -np.inf, -3.0], [-2.0, -1.0, -np.inf], [1, 2, 3], [1, 1, 1]),                            # -inf scores stay scored and sort last among them
    ([-1.5, -1.5, -1.5], [-2.0, -2.0, -2.0], [5, 5, 5], [1, 1, 1]),                                  # all equal
    ([-1.0, -2.0], [np.inf, -1.0], [1, 1], [1, 1]),                                                  # -inf + inf would be NaN only with am = -inf
    ([-np.inf, -2.0], [np.inf, -1.0], [1, 1], [1, 1]),                                               # NaN combined: not scored
    ([], [], [], []),
]


@pytest.mark.parametrize("case", range(len(ORDER_CASES)))
@pytest.mark.parametrize("alpha,beta", [(0.5, 0.0), (0.3, 0.7), (1.0, -0.25), (0.0, 0.5), (0.0, 0.0)])
def test_diag_nlm_order_is_the_python_rule(case, alpha, beta):
    am, nlm, lens, ok = ORDER_CASES[case]
    want_o, want_c = R.nlm_order(am, nlm, lens, ok, alpha, beta)
    got_o, got_c = capi.diag_nlm_order(np.asarray(am, np.float32), np.asarray(nlm, np.float32), lens, ok, alpha, beta)
    assert list(got_o) == list(want_o)
    assert np.array_equal(np.asarray(got_c, np.float32).view(np.uint32), np.asarray(want_c, np.float32).view(np.uint32))
    assert sorted(got_o) == list(range(len(am)))
    if alpha == 0.0 and beta == 0.0:                                 # the identity, whatever ok says
        assert list(got_o) == list(range(len(am)))
        assert np.array_equal(np.asarray(got_c, np.float32).view(np.uint32), np.asarray(am, np.float32).view(np.uint32))


def test_order_rule_places_ties_and_unscored_slots():
    o, c = R.nlm_order(*ORDER_CASES[0], 0.5, 0.0)
    assert o == [1, 3, 0, 2] and list(c) == [-3.5, -2.5, -3.5, -2.5]
    o, c = R.nlm_order(*ORDER_CASES[1], 0.5, 0.0)
    assert o == [2, 0, 1, 3] and c[1] == -np.inf and c[3] == -np.inf


@pytest.mark.parametrize("kw", [dict(), dict(pre_ln=False, has_final_norm=False, has_emb_norm=True, tied_head=False, num_layers=3, ffn_intermediate=96)])
def test_config_infer_returns_the_config_the_file_was_written_with(tmp_path, kw):
    cfg = small_cfg(**kw)
    wp = str(tmp_path / "nlm.safetensors")
    synth.save_weights(wp, synth.synth_nlm_weights(cfg, seed=1, prefix="lm."))
    t = cfg.transformer
    got = capi.nlm_config_infer(wp, "lm.", num_heads=t.num_heads, pre_ln=bool(t.pre_ln), bos_id=cfg.bos_id, eos_id=cfg.eos_id)
    for f in ("vocab_size", "max_positions", "has_emb_norm", "tied_head", "bos_id", "eos_id"):
        assert getattr(got, f) == getattr(cfg, f), f
    for f in ("hidden_size", "num_layers", "num_heads", "ffn_intermediate", "pre_ln", "has_final_norm"):
        assert getattr(got.transformer, f) == getattr(t, f), f
    with pytest.raises(capi.PkError) as e:                           # another prefix: the tensors are not there
        capi.nlm_config_infer(wp, "other.")
    assert e.value.code == -3 and "tok_emb_.weight" in str(e.value)


def test_load_refusals_that_need_no_device(tmp_path):
    """max_positions past 512 and a missing position table are refused before a device is looked for."""
    cfg = small_cfg()
    W = synth.synth_nlm_weights(cfg, seed=1)
    wp = str(tmp_path / "nlm.safetensors")
    synth.save_weights(wp, W)
    big = small_cfg(max_positions=513)
    with pytest.raises(capi.PkError) as e:
        capi.NeuralLm(wp, big)
    assert e.value.code == -7 and "512" in str(e.value)
    del W["pos_emb_.weight"]
    wq = str(tmp_path / "nopos.safetensors")
    synth.save_weights(wq, W)
    with pytest.raises(capi.PkError) as e:
        capi.NeuralLm(wq, cfg)
    assert e.value.code == -3 and "pos_emb_.weight" in str(e.value)
    with pytest.raises(capi.PkError) as e:
        capi.NeuralLm(wp, small_cfg(bos_id=23))
    assert e.value.code == -1
