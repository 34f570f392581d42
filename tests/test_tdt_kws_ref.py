"""The specification of the TDT keyword spotting (tests/tdt_kws_ref.py) against a brute-force enumeration of every path, a
planted greedy path, and the peak picking on hand-made rows.  CPU only."""
import numpy as np
import pytest

import tdt_kws_ref as R

NEG = R.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)

DURS = ([0, 1, 2], [1, 2], [0, 1], [1], [2, 0, 1])


@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("dur", DURS, ids=lambda d: "d" + "".join(map(str, d)))
def test_walk_equals_brute_force(family, dur):
    rng = np.random.default_rng(len(dur) * 17 + sum(dur) + (family == "holes"))
    seen_tie = 0
    for T in (1, 2, 3, 5, 6):
        for L in (1, 2, 3):
            lat = R.make_lattice(family, T, L, len(dur), rng)
            E, Bs, Ee, ties = R.walk(*lat, dur)
            seen_tie += ties
            best = R.brute_force(*lat, dur)
            for e in range(T):
                assert bits(E[e]) == bits(best[:, e].max()), (T, L, e)
                if E[e] > NEG:
                    assert 0 <= Bs[e] <= e and bits(best[Bs[e], e]) == bits(E[e]), (T, L, e)      # the start the ref reports reaches the maximum
                    assert e <= Ee[e] <= T - 1
                    assert not (E[e] == 0 and np.signbit(E[e]))
    assert seen_tie > 0                                             # the families do exercise the tie rule


def test_planted_path_scores_plus_zero():
    rng = np.random.default_rng(5)
    dur = [0, 1, 2, 4]
    T, L = 20, 4
    lab, blk, dl, top = R.make_lattice("ties", T, L, len(dur), rng)
    # nothing else may be greedy: push every label strictly below the row's best first
    lab = np.minimum(lab, top[:, :L] - np.float32(0.5)).astype(np.float32)
    steps = [([], 2), ([1], 0), ([], 1), ([3, 1], 2)]              # token 0 (dur 2) | blank 1, token 1 (dur 0) | token 2 (dur 1) | blanks 4, 1, token 3 (dur 2)
    s, e = R.plant(lab, blk, dl, top, dur, 3, steps)
    assert (s, e) == (3, 3 + 2 + 1 + 0 + 1 + 4 + 1 + 2 - 1)
    r = R.spot(lab, blk, dl, top, dur, max_hits=4, min_score=0.0)  # min_score 0: only a greedy match counts
    assert r["n_hits"] == 1
    assert (r["start"][0], r["end"][0]) == (s, e)
    assert bits(r["score"][0]) == 0                                 # +0.0, sign bit clear
    assert np.all(r["start"][1:] == 0) and np.all(r["end"][1:] == 0) and np.all(r["score"][1:] == NEG)


def test_single_token_reads_column_zero():
    dur = [1, 2]
    T = 4
    top = np.full((T, 2), -0.25, np.float32)
    lab = np.asarray([[-1.0], [-0.25], [-3.0], [-0.5]], np.float32)
    blk = np.full((T, 2), -0.25, np.float32)
    dl = np.tile(np.asarray([-0.5, -1.0], np.float32), (T, 2, 1))
    E, Bs, Ee, _ = R.walk(lab, blk, dl, top, dur)
    assert bits(E).tolist() == bits(np.asarray([-0.75, 0.0, -2.75, -0.25], np.float32)).tolist()
    assert Bs.tolist() == [0, 1, 2, 3] and Ee.tolist() == [0, 1, 2, 3]


def test_pick_rules():
    E = np.asarray([-1.0, -0.5, -0.5, NEG, -2.0, -0.25, -3.0], np.float32)
    Bs = np.asarray([0, 0, 2, 0, 3, 5, 6], np.int32)
    Ee = np.asarray([0, 1, 3, 0, 4, 6, 6], np.int32)
    n, st, en, sc = R.pick(E, Bs, Ee, max_hits=4)
    # best: t = 5 [5, 6] masks t = 6 [6, 6]; then the tie -0.5 goes to the lower frame t = 1 [0, 1], which masks t = 0; then t = 2 [2, 3] masks
    # t = 4 [3, 4]; nothing is left for the fourth slot
    assert n == 3
    assert st.tolist() == [5, 0, 2, 0] and en.tolist() == [6, 1, 3, 0]
    assert bits(sc).tolist() == bits(np.asarray([-0.25, -0.5, -0.5, NEG], np.float32)).tolist()
    n, st, en, sc = R.pick(E, Bs, Ee, max_hits=4, min_score=-0.4)
    assert n == 1 and (st[0], en[0]) == (5, 6)
    n, st, en, sc = R.pick(E, Bs, Ee, max_hits=1)
    assert n == 1 and len(st) == 1
    n, *_ = R.pick(np.full(3, NEG, np.float32), np.zeros(3, np.int32), np.zeros(3, np.int32), max_hits=2)
    assert n == 0
    # a span that ends past its emission frame masks an entry that begins inside it
    n, st, en, _ = R.pick(np.asarray([-0.5, -1.0], np.float32), np.asarray([0, 1], np.int32), np.asarray([1, 1], np.int32), max_hits=2)
    assert n == 1 and (st[0], en[0]) == (0, 1)
