"""CPU: the specification of the RNN-T forced alignment and total (tests/rnnt_lattice_ref.py) against an enumeration of every path."""
import numpy as np
import pytest

import rnnt_lattice_ref as R

F = np.float32
NEG = F(-np.inf)


def lattice(T, U, rng, hole=0.0):
    x = rng.normal(size=(T, U + 1, 5)) * 2.0
    l = (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)
    lab, blk = np.ascontiguousarray(l[:, :U, 0]), np.ascontiguousarray(l[:, :, 4])
    for a in (lab, blk):
        a[rng.random(size=a.shape) < hole] = NEG
    return lab, blk


@pytest.mark.parametrize("hole", [0.0, 0.25], ids=["dense", "holes"])
def test_both_walks_equal_the_enumeration_of_every_path(hole):
    """fp32 addition is monotone, so the max-plus walk's score IS the largest left-to-right path sum, bit for bit, and the back-trace is a path
    with that sum.  The total is held to the float64 log-sum of the paths within 4 (T + U) ulp of the larger of 1 and |total|: a cell costs two
    adds and one log-add, each rounding at most twice at the size of alpha, along chains of at most T + U cells."""
    rng = np.random.default_rng(11)
    n_paths = 0
    for T in range(1, 6):
        for U in range(0, 5):
            lab, blk = lattice(T, U, rng, hole)
            sums = R.path_sums(lab, blk)
            a, tt = R.align(lab, blk), R.total(lab, blk)
            assert a["score"].dtype == np.float32 and a["score"] == sums.max(), (T, U)
            assert a["ok"] == (1 if sums.max() > NEG else 0) == tt["ok"]
            assert tt["total"] >= a["score"]
            n_paths += len(sums)
            if not a["ok"]:
                assert tt["total"] == NEG and not a["start"].any()
                continue
            want = np.logaddexp.reduce(sums.astype(np.float64))
            assert abs(np.float64(tt["total"]) - want) <= 4 * (T + U) * 2.0 ** -23 * max(1.0, abs(want)), (T, U, tt["total"], want)
            # the back-trace: frames never decrease, and walking it left to right through the lattice gives the score
            st = a["start"]
            assert (np.diff(st) >= 0).all() and (a["end"] == st).all()
            acc, t = F(0.0), 0
            for k in range(U + 1):
                stop = st[k] if k < U else T - 1
                while t < stop:
                    acc, t = F(acc + blk[t, k]), t + 1
                acc = F(acc + (lab[t, k] if k < U else blk[T - 1, U]))
            assert acc == a["score"], (T, U)
            assert np.allclose(a["conf"], np.exp(lab[st, np.arange(U)].astype(np.float64)), rtol=1e-6, atol=0)
    assert n_paths == 251                                           # sum of C(T - 1 + U, U) over the shapes


def test_ties_keep_the_blank_arc():
    """Every weight equal: all paths tie, the strict > keeps the blank candidate wherever one exists, so every token leaves at frame 0."""
    lab, blk = np.full((4, 3), -1.0, np.float32), np.full((4, 4), -1.0, np.float32)
    a = R.align(lab, blk)
    assert a["ok"] == 1 and a["score"] == F(-7.0) and (a["start"] == 0).all()
