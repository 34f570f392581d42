"""CPU: pins tests/ctc_kws_ref.py, the written specification of the CTC keyword spotting, on cases whose answer is
known without it, and against a brute-force search over all (start, end) spans."""
import numpy as np
import pytest

import ctc_align_ref as A
import ctc_kws_ref as R

NEG = np.float32(-np.inf)


def peaky(T, V, seed):
    """A "peaky" input whose greedy path is all blank (V - 1) before anything is planted, so that nothing matches by accident."""
    rng = np.random.default_rng(seed)
    lp = A.make_lp("peaky", T, V, rng)
    return R.plant(lp, [V - 1] * T, 0)


def test_a_planted_keyword_scores_zero_at_its_span():
    V, blank = 33, 32
    lp = peaky(40, V, 1)
    kw = [5, 9, 9, 2]
    R.plant(lp, [5, 5, blank, 9, blank, 9, 9, 2], 11)               # frames 11 .. 18; the repeat has its blank
    r = R.spot(lp, kw, blank)
    assert r["n_hits"] == 1 and (r["start"][0], r["end"][0]) == (11, 18)
    assert r["score"][0] == 0.0 and not np.signbit(r["score"][0])
    E, Bs = R.walk(lp, kw, blank)
    assert np.all(E <= 0) and not np.any(np.signbit(E[E == 0])), "scores are <= 0 and a zero is +0.0"


def test_two_occurrences_two_hits_and_the_better_one_first():
    V, blank = 33, 32
    lp = peaky(60, V, 2)
    kw = [7, 3]
    R.plant(lp, [7, blank, 3], 10)                                  # frames 10 .. 12, exact
    R.plant(lp, [7, 7, 3], 40)                                      # frames 40 .. 42 ...
    lp[41, 7] -= np.float32(0.5)                                    # ... a little worse: the best symbol of frame 41 is still 7
    lp[41, 8] = lp[41, 7] + np.float32(1.0)                         # now it is not
    r = R.spot(lp, kw, blank, max_hits=4)
    assert r["n_hits"] >= 2
    assert (r["start"][0], r["end"][0], r["score"][0]) == (10, 12, 0.0)
    assert (r["start"][1], r["end"][1]) == (40, 42) and r["score"][1] == np.float32(-1.0)
    one = R.spot(lp, kw, blank, max_hits=1)
    assert one["n_hits"] == 1 and (one["start"][0], one["end"][0], one["score"][0]) == (10, 12, 0.0)
    thr = R.spot(lp, kw, blank, max_hits=4, min_score=np.float32(-0.5))
    assert thr["n_hits"] == 1 and thr["score"][1] == NEG and thr["start"][1] == 0 and thr["end"][1] == 0, "unused slots: 0 / 0 / -inf"
    both = R.spot(lp, kw, blank, max_hits=4, min_score=np.float32(-1.0))
    assert both["n_hits"] == 2, "min_score is inclusive"
    for h in range(r["n_hits"]):
        for j in range(h):
            assert r["end"][j] < r["start"][h] or r["end"][h] < r["start"][j], "hits do not overlap"


def test_an_adjacent_repeat_needs_its_blank():
    V, blank = 33, 32
    kw = [4, 4]
    with_blank = R.plant(peaky(20, V, 3), [4, blank, 4], 5)
    r = R.spot(with_blank, kw, blank)
    assert (r["start"][0], r["end"][0], r["score"][0]) == (5, 7, 0.0)
    without = R.plant(peaky(20, V, 3), [4, 4], 5)                   # "4 4" collapses to one token: no exact match anywhere
    r = R.spot(without, kw, blank)
    assert r["n_hits"] == 1 and r["score"][0] < 0
    assert r["end"][0] - r["start"][0] + 1 >= 3


def test_a_clip_shorter_than_the_keyword_has_no_hit():
    rng = np.random.default_rng(4)
    V, blank = 9, 8
    lp = A.make_lp("ties", 3, V, rng)
    assert R.spot(lp, [1, 2, 3, 4], blank, max_hits=3)["n_hits"] == 0
    assert R.spot(lp, [1, 1], blank)["n_hits"] == 1, "[a, a] fits three frames exactly"
    assert R.spot(lp[:2], [1, 1], blank)["n_hits"] == 0
    r = R.spot(lp[:1], [1], blank)
    assert r["n_hits"] == 1 and (r["start"][0], r["end"][0]) == (0, 0)
    E, _ = R.walk(lp, [1, 2, 3], blank)
    assert np.all(E[:2] == NEG) and E[2] > NEG


def test_a_row_without_a_finite_maximum_is_refused():
    lp = np.full((3, 4), NEG, np.float32)
    with pytest.raises(AssertionError):
        R.walk(lp, [1], 3)


KWS = [[0], [1, 2], [2, 2], [0, 1, 0], [1, 1, 1], [3, 3, 0], [2, 0, 0]]


@pytest.mark.parametrize("family", ["ties", "holes", "peaky"])
@pytest.mark.parametrize("T", [1, 2, 5, 12])
def test_equals_a_brute_force_search_over_all_spans(family, T):
    rng = np.random.default_rng(100 + T + 7 * ["ties", "holes", "peaky"].index(family))
    V, blank = 5, 4
    n_unique = 0
    for trial in range(6):
        lp = A.make_lp(family, T, V, rng)
        if family == "holes":
            lp[np.arange(T), rng.integers(0, V, size=T)] = np.float32(-1.0)      # every row keeps a finite maximum
        for kw in KWS:
            E, Bs = R.walk(lp, kw, blank)
            bE, bstarts = R.brute_force(lp, kw, blank)
            assert np.array_equal(E.view(np.uint32), bE.view(np.uint32)), f"{family} T={T} {kw}: scores per end frame"
            for t in range(T):
                if E[t] > NEG:
                    assert Bs[t] in bstarts[t], f"{family} T={T} {kw}: start of the match that ends at {t}"
                    n_unique += len(bstarts[t]) == 1
            # the hits: the brute-force maximum over every span, where it is unique
            r = R.spot(lp, kw, blank, max_hits=3)
            if (bE > NEG).any():
                top = bE.max()
                ends = np.nonzero(bE == top)[0]
                assert r["score"][0].view(np.uint32) == top.view(np.uint32)
                assert r["end"][0] == ends[0]
                if len(ends) == 1 and len(bstarts[ends[0]]) == 1:
                    assert r["start"][0] == bstarts[ends[0]][0]
            else:
                assert r["n_hits"] == 0
    assert T < 5 or n_unique > 0
