"""CPU checks of the fused CTC prefix beam search specification (tests/ctc_beam_lm_ref.py): the fp32 reference
against a float64 brute force over all V^T paths plus the float64 LM score, the constructed input on which the model changes the 1-best,
and what alpha = beta = 0 reduces to.  The device side is compared with the same reference in tests/test_gpu_ctc_beam_lm.py."""
import numpy as np
import pytest

import ctc_beam_lm_ref as RL
import ctc_beam_ref as R
import ngram_lm_ref as NR
from test_ctc_beam_ref import CASES, score_bound

# Error bound of an fp32 LM score against exact arithmetic on the same fp32 table.  Token k of a string passes through
#   a lookup: at most order - 1 adds of back-off weights and the add of the arc's value, every intermediate bounded by a_k = the sum of
#             the |terms| of the chain                                                    -> order roundings, each <= u a_k, scaled by |alpha|
#   alpha * lp                                                                            -> one rounding  <= u |alpha| a_k
#   (.) + beta                                                                            -> one rounding  <= u (|alpha| a_k + |beta|)
#   lm + (.)                                                                              -> one rounding  <= u S_k
# with u = 2^-24 and S_k = sum_{j <= k} (|alpha| a_j + |beta|), which bounds |lm| after token k and each of the three magnitudes above.
# That is order + 3 roundings per token, each <= u S_k to first order: the LM term is (order + 3) u sum_k S_k.  Second-order terms are
# smaller by a factor (order + 3) L u < 1e-5 at these lengths; 1 % on top of the first-order bound covers them.
U24 = 2.0 ** -24


def lm_bound(lm, p, alpha, beta):
    hist = lm.start(True)
    S, total = 0.0, 0.0
    for c in p:
        S += abs(alpha) * lm.lookup(hist, c)[1] + abs(beta)
        total += S
        hist = hist + (c,)
    return 1.01 * (lm.order + 3) * U24 * total


LMS = {
    "order1": dict(order=1, density=1.0, unk=False, bos=False),
    "order3_sparse_unk": dict(order=3, density=0.5, unk=True, bos=False),
    "order5_sparse_bos": dict(order=5, density=0.7, unk=False, bos=True),
    "order2_dense": dict(order=2, density=3.0, unk=False, bos=True),
}


@pytest.mark.parametrize("T,V,seed", CASES)
@pytest.mark.parametrize("family", ["uniform", "peaky"])
@pytest.mark.parametrize("lm_name", sorted(LMS))
@pytest.mark.parametrize("alpha,beta", [(0.5, 0.0), (1.5, -0.5), (0.0, 1.0)])
def test_fused_reference_matches_float64_brute_force(T, V, seed, family, lm_name, alpha, beta):
    rng = np.random.default_rng(100 + seed)
    lp = R.log_softmax32(rng.normal(size=(T, V)) * (0.3 if family == "uniform" else 4.0))
    blank = V - 1
    lm = NR.RefLm(NR.make_arpa(V, seed=seed, **LMS[lm_name]))
    bf = R.brute_force(lp, blank)
    W = len(bf)                                                     # every prefix fits: nothing is pruned
    got = RL.beam_search_lm(lp, blank, lm, alpha, beta, beam_width=W, token_prune=V - 1, n_best=W)
    assert sorted(p for p, _, _ in got) == sorted(bf), "the final beam holds exactly the label strings of the brute force"
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
    fused = []
    for p, s, l in got:
        want = bf[p] + a32 * lm.score64(p) + b32 * len(p)
        bound = score_bound(T, bf[p]) + lm_bound(lm, p, a32, b32)
        assert abs(float(s) + float(l) - want) <= bound, (p, float(s), float(l), want, bound)
        assert abs(float(s) - bf[p]) <= score_bound(T, bf[p]), "score keeps its meaning: the acoustic log-probability"
        fused.append(float(np.float32(s + l)))
    assert fused == sorted(fused, reverse=True), "hypotheses come back in fused order"


def test_flip_the_model_changes_the_one_best():
    lp, blank, text, alpha, beta = RL.flip_case()
    lm = NR.RefLm(text)
    plain = R.beam_search(lp, blank, 4, 2, 4)
    fused = RL.beam_search_lm(lp, blank, lm, alpha, beta, 4, 2, 4)
    assert plain[0][0] == (0,) and fused[0][0] == (1,), (plain, fused)
    by = {p: s for p, s in plain}
    for p, s, l in fused:                                           # the same prefixes with the same acoustic scores, re-ranked
        assert by[p].view(np.uint32) == s.view(np.uint32)
        assert l.view(np.uint32) == np.float32(alpha * lm.score(p)).view(np.uint32) or len(p) != 1


@pytest.mark.parametrize("seed", range(4))
def test_zero_weights_are_the_unfused_search(seed):
    rng = np.random.default_rng(300 + seed)
    T, V = 24, 7
    lp = R.log_softmax32(rng.normal(size=(T, V)) * 2.0)
    lm = NR.RefLm(NR.make_arpa(V, 3, 1.0, True, True, seed=seed))
    plain = R.beam_search(lp, V - 1, 6, 4, 6)
    fused = RL.beam_search_lm(lp, V - 1, lm, 0.0, 0.0, 6, 4, 6)
    assert [p for p, _ in plain] == [p for p, _, _ in fused]
    assert [s.view(np.uint32) for _, s in plain] == [s.view(np.uint32) for _, s, _ in fused]
    assert all(l.view(np.uint32) == 0 for _, _, l in fused), "lm_score is +0.0"
