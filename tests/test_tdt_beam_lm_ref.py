"""CPU: the written specification of the TDT beam search with n-gram LM shallow fusion (tests/tdt_beam_lm_ref.py):
the unpruned search against a float64 enumeration of every path plus the float64 LM score, what alpha = beta = 0 reduces to, lm_score
against the left-to-right sum of lookups, the fused order, and a model that changes the 1-best.  The device side is compared with the
same specification in tests/test_gpu_tdt_beam_lm.py."""
import numpy as np
import pytest

import ngram_lm_ref as NR
import tdt_beam_lm_ref as RL
import tdt_beam_ref as R
from test_ctc_beam_lm_ref import U24
from test_tdt_beam_ref import random_joint

F = np.float32
LMS = {
    "order1": dict(order=1, density=1.0, unk=False, bos=False),
    "order3_sparse_unk": dict(order=3, density=0.5, unk=True, bos=False),
    "order5_sparse_bos": dict(order=5, density=0.7, unk=False, bos=True),
}
WEIGHTS = [(0.5, 0.0), (1.5, -0.5), (0.7, 0.8)]


def every_path64(joint, T, blank, V, dur, max_tokens, lm, alpha, beta):
    """Every complete path of the lattice in float64 -> (number of paths, the largest sum(arc) + alpha * lm64 + beta * len, the largest
    error bound of a path).

    The bound of one path of n arcs over a prefix of L tokens, u = 2^-24.  M = (sum over its arcs of |x| + |dl|) + S_L bounds every
    intermediate of the fp32 computation, S_k = sum_{j <= k} (|alpha| a_j + |beta|) as in tests/test_ctc_beam_lm_ref.py (a_j: the sum of
    the |terms| of token j's lookup chain).
      acoustic      per arc x + dl and score + (.)                                                   2 n roundings, each <= u M
      decisions     per step one f = score + lm of the entry that stays and one of the entry it is compared with: a decision between
                    two entries of a state, or a tie of f, can go against the exact order by those two roundings     2 n roundings <= u M
      LM            order + 3 roundings per token, each <= u S_k (test_ctc_beam_lm_ref.lm_bound)       (order + 3) u sum_k S_k
    1 % on top covers the second-order terms.  The search returns a real path (its value is within its bound of an exact path value <= the
    maximum) and never loses the best path by more than that path's bound, so the largest bound over all paths bounds the 1-best's error."""
    h0 = lm.start(True)
    best = [0, -np.inf, 0.0]

    def go(t, prefix, hist, acc, mag, n, lm64, S, sumS):
        if t >= T:
            best[0] += 1
            best[1] = max(best[1], acc + alpha * lm64 + beta * len(prefix))
            best[2] = max(best[2], 1.01 * U24 * (4 * n * (mag + S) + (lm.order + 3) * sumS))
            return
        logp, dl = joint(t, prefix)
        for i in range(V):
            if i != blank and len(prefix) >= max_tokens:
                continue
            if i != blank:
                S2 = S + abs(alpha) * lm.lookup(hist, i)[1] + abs(beta)
                l2 = lm64 + lm.lookup64(hist, i)
            for d in range(len(dur)):
                a2, m2 = acc + (float(logp[i]) + float(dl[d])), mag + abs(float(logp[i])) + abs(float(dl[d]))
                if i == blank:
                    go(t + max(dur[d], 1), prefix, hist, a2, m2, n + 1, lm64, S, sumS)
                else:
                    go(t + dur[d], prefix + (i,), hist + (i,), a2, m2, n + 1, l2, S2, sumS + S2)
    go(0, (), h0, 0.0, 0.0, 0, 0.0, 0.0, 0.0)
    return tuple(best)


# (T, durations, seeds).  The lattice of V = 4 with durations [1, 2] has 36 complete paths at T = 2 and 176 at T = 3 (every arc advances the
# frame), with [0, 1] and max_tokens = 3 it has 1039 and 5543.  "At least a few hundred paths per case" therefore cannot hold for one joint at
# the [1, 2] shapes: there a case is several seeds (several joints and models, each searched and enumerated on its own), as many as make its
# enumeration 300 paths, and the count is asserted over the case.  The [0, 1] cases meet it on one seed.
EXHAUSTIVE = [(2, [0, 1], (1,)), (3, [0, 1], (2,)), (2, [1, 2], tuple(range(10, 19))), (3, [1, 2], (3, 4))]


@pytest.mark.parametrize("T,dur,seeds", EXHAUSTIVE)
@pytest.mark.parametrize("lm_name", sorted(LMS))
def test_unpruned_fused_search_equals_the_float64_enumeration_of_every_path(T, dur, seeds, lm_name):
    V, blank, mt = 4, 3, 3
    n_paths = 0
    for seed in seeds:
        alpha, beta = WEIGHTS[(seed + len(lm_name)) % len(WEIGHTS)]
        a32, b32 = float(F(alpha)), float(F(beta))
        joint = random_joint(seed, V, len(dur))
        memo = {}
        cached = lambda t, p: memo[(t, p)] if (t, p) in memo else memo.setdefault((t, p), joint(t, p))
        lm = NR.RefLm(NR.make_arpa(V, seed=seed, **LMS[lm_name]))
        n, want, bound = every_path64(cached, T, blank, V, dur, mt, lm, a32, b32)
        n_paths += n
        trace = []
        BIG = 1 << 20                                               # wider than the lattice has states: nothing is pruned
        r = RL.search(cached, T, blank, dur, lm, alpha, beta, BIG, V - 1, len(dur), 8, mt, trace=trace)
        assert all(len(b) < BIG for b in trace) and r["ok"] == 1
        got = float(r["score"][0]) + float(r["lm_score"][0])
        assert abs(got - want) <= bound, (seed, got, want, bound)
        assert bound < 1e-3, "the bound is a rounding bound, not a tolerance"
    assert n_paths >= 300, f"the brute force enumerated only {n_paths} paths"


def fields_equal(a, b):
    for k in ("ids", "lens", "start", "end", "dur_idx", "score", "conf"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), k
    assert a["ok"] == b["ok"] and a["steps"] == b["steps"]


@pytest.mark.parametrize("seed", range(4))
def test_zero_weights_are_the_unfused_search(seed, orc):
    V, dur, T, mt = 6, [0, 1, 2], 5, 4
    joint = random_joint(40 + seed, V, len(dur))
    lm = NR.RefLm(NR.make_arpa(V, 3, 1.0, True, True, seed=seed))
    plain = R.search(joint, T, V - 1, dur, 4, 3, 2, 4, mt)
    fused = RL.search(joint, T, V - 1, dur, lm, 0.0, 0.0, 4, 3, 2, 4, mt)
    fields_equal(plain, fused)
    assert plain["lens"].sum() > 0, "degenerate test: no hypothesis holds a token"
    assert not fused["lm_score"].view(np.uint32).any(), "lm_score is +0.0"


@pytest.mark.parametrize("lm_name", sorted(LMS))
@pytest.mark.parametrize("alpha,beta", WEIGHTS)
def test_lm_score_is_the_sum_of_lookups_and_hypotheses_come_back_in_fused_order(lm_name, alpha, beta, orc):
    V, dur, T, mt, N = 6, [0, 1, 2], 5, 4, 6
    joint = random_joint(7, V, len(dur))
    lm = NR.RefLm(NR.make_arpa(V, seed=5, **LMS[lm_name]))
    r = RL.search(joint, T, V - 1, dur, lm, alpha, beta, 6, 4, 2, N, mt)
    filled = int((r["score"] > -np.inf).sum())
    assert filled >= 2 and r["lens"].sum() > 0
    for n in range(N):
        hist, want = lm.start(True), F(0.0)
        for c in r["ids"][n, :r["lens"][n]]:
            want = F(want + F(F(F(alpha) * lm.lookup(hist, int(c))[0]) + F(beta)))
            hist = hist + (int(c),)
        assert F(r["lm_score"][n]).view(np.uint32) == want.view(np.uint32), n
        if n >= filled:
            assert r["score"][n] == -np.inf and F(r["lm_score"][n]).view(np.uint32) == 0, "an unfilled slot: score -inf, lm_score +0.0"
    f = [F(r["score"][n] + r["lm_score"][n]) for n in range(filled)]
    assert all(f[n] >= f[n + 1] for n in range(filled - 1)), "score + lm_score (one fp32 add) does not increase"
    strings = [tuple(r["ids"][n, :r["lens"][n]]) for n in range(filled)]
    assert len(set(strings)) == filled


def test_a_model_that_favours_one_token_changes_the_one_best(orc):
    V, dur, T, mt = 6, [0, 1, 2], 5, 4
    joint = random_joint(3, V, len(dur))
    plain = R.search(joint, T, V - 1, dur, 8, 5, 3, 8, mt)
    best = tuple(plain["ids"][0, :plain["lens"][0]])
    token = next(c for c in range(V - 1) if c not in best)
    lm = NR.RefLm(RL.flip_arpa(V, token))
    fused = RL.search(joint, T, V - 1, dur, lm, 1.0, 0.0, 8, 5, 3, 8, mt)
    got = tuple(fused["ids"][0, :fused["lens"][0]])
    assert got != best, "the model did not change the 1-best"
    assert all(c == token for c in got), (best, got)
    by = {tuple(plain["ids"][n, :plain["lens"][n]]): plain["score"][n] for n in range(8)}
    if got in by:                                                   # the same path where the unfused search kept the string too
        assert fused["score"][0] <= by[got]


def test_a_tie_of_f_between_entries_of_one_state_keeps_the_earlier_pool_entry():
    """A finished hypothesis and a blank arc into the same state whose acoustic scores differ by less than score + lm can tell apart: the
    earlier pool entry (the finished one) stays, with its own lower acoustic score -- the one case in which deciding by f is not deciding
    by score.  (In a search the two carry equal lm because lm is a function of the string; step takes the values it is given.)"""
    lm = NR.RefLm(RL.flip_arpa(3, 0))
    rows = {(1, (0,)): ([-9.0, -9.0, -0.125], [-0.5, -0.75])}
    jt = lambda t, p: tuple(np.asarray(a, np.float32) for a in rows[(t, tuple(p))])
    tok, hist = ((0, 0, F(-1.0)),), lm.start(True) + (0,)

    def stays(lmv):
        beam = [((0,), 2, F(-2.0), tok, hist, F(lmv)), ((0,), 1, F(-1.0), tok, hist, F(lmv))]      # finished at T = 2; live, its blank arc reaches (t = 2, (0,))
        new = RL.step(beam, jt, lm, F(1.0), F(0.0), 2, 2, [1, 1], 4, 1, 2, 4)
        same = [h for h in new if h[0] == (0,) and h[1] == 2]
        assert len(same) == 1, "one state"
        return same[0][2]
    assert stays(0.0) == F(-1.625), "f tells the two apart: the better score stays"
    assert stays(-3.0e7) == F(-2.0), "at lm = -3e7 an fp32 ulp is 2: f ties, and the earlier pool entry stays"


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    from parakeet_cpp_amd import capi
    L = capi.lib()
    for name in ("pk_tdt_beam_decode_lm", "pk_tdt_beam_decode_lm_ragged", "pk_tdt_beam_decode_lm_timed", "pk_transcribe_pcm_nbest_tdt_lm"):
        assert hasattr(L, name), name
    z = np.zeros(4, np.float32); zi = np.zeros(4, np.int32)
    assert L.pk_tdt_beam_decode_lm(None, capi._f(z), 1, 1, None, 1, capi._i(zi), capi._i(zi), capi._f(z), None, None, None, None, None, None, None, None) == -1
