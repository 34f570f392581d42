"""CPU: the specification of the CTC forced alignment (tests/ctc_align_ref.py) against an enumeration of every path, its tie rules, the band
rule, and the argument checks of pk_ctc_align, which need no device."""
import itertools
import math

import numpy as np
import pytest

from parakeet_cpp_amd import capi

import ctc_align_ref as R
import ctc_beam_ref as B


def enumerate_paths(lp, ids, blank):
    """float64 over all V^T paths that collapse to ids -> (best path sum, log of the summed path probabilities); (-inf, -inf) when none"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    sums = []
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], -1
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if out == list(ids):
            sums.append(sum(lp[t, c] for t, c in enumerate(path)))
    sums = [x for x in sums if x > -math.inf]
    if not sums:
        return -math.inf, -math.inf
    m = max(sums)
    return m, m + math.log(math.fsum(math.exp(x - m) for x in sums))


STRINGS = [(), (0,), (1,), (0, 1), (0, 0), (1, 0, 1), (0, 0, 1), (1, 1, 1)]


@pytest.mark.parametrize("family", ["ties", "holes", "peaky"])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 6])
def test_reference_equals_the_enumeration_of_all_paths(T, family):
    rng = np.random.default_rng(100 * T + len(family))
    lp = R.make_lp(family, T, 3, rng)
    for ids in STRINGS:
        best, tot = enumerate_paths(lp, ids, 2)
        r = R.full(lp, ids, 2)
        assert r["ok"] == (1 if best > -math.inf else 0), (T, ids)
        if r["ok"]:
            assert abs(float(r["score"]) - best) <= 1e-5, (T, ids, r["score"], best)
            assert abs(float(r["total"]) - tot) <= 1e-5, (T, ids, r["total"], tot)
            assert r["total"] >= r["score"] or abs(float(r["total"]) - float(r["score"])) <= 1e-5
            assert np.all(r["start"] <= r["end"]) and np.all(r["end"][:-1] < r["start"][1:])
        else:
            assert r["score"] == -np.inf and r["total"] == -np.inf and not r["start"].any() and not r["conf"].any()
        n_rep = sum(a == b for a, b in zip(ids, ids[1:]))
        if len(ids) + n_rep > T:
            assert r["ok"] == 0, "more tokens + adjacent repeats than frames cannot be aligned"


def test_tie_rules_on_quantised_rows():
    """All rows equal and every column the same value: every path ties.  Stay wins over previous state wins over skip, and the end state
    is the last blank: walking back from the last blank the path stays wherever the cell could be reached by staying, so every token is
    emitted as early as possible, one frame each (token k in frame k), and the last blank takes the rest."""
    T, V = 9, 4
    lp = B.log_softmax32(np.zeros((T, V)))
    r = R.align(lp, (0, 1, 0), 3)
    assert r["ok"] == 1
    assert r["start"].tolist() == [0, 1, 2] and r["end"].tolist() == [0, 1, 2]
    rb = R.lattice_banded(lp, (0, 1, 0), 3)
    assert rb["start"].tolist() == r["start"].tolist() and rb["end"].tolist() == r["end"].tolist()
    # a repeated token forces the blank between: [a, a] at T = 3 is exactly alignable, at T = 2 it is not
    assert R.align(lp[:3], (0, 0), 3)["ok"] == 1 and R.align(lp[:2], (0, 0), 3)["ok"] == 0
    # strictly better last token state wins the end, an equal one does not
    lp2 = lp.copy()
    lp2[-1, 0] += np.float32(0.25)
    assert R.align(lp2, (0,), 3)["end"].tolist() == [T - 1]
    assert R.align(lp, (0,), 3)["end"].tolist() == [0]
    # L = 0: the sum of the blank column as the lattice adds it (fp32, in frame order)
    s = lp[0, 3]
    for t in range(1, T):
        s = np.float32(s + lp[t, 3])
    r0 = R.full(lp, (), 3)
    assert r0["ok"] == 1 and r0["score"].view(np.uint32) == s.view(np.uint32) == r0["total"].view(np.uint32)


@pytest.mark.parametrize("family", ["ties", "holes", "peaky"])
def test_band_pruning_changes_nothing(family):
    rng = np.random.default_rng(7 + len(family))
    cases = [(1, 0), (1, 1), (2, 1), (4, 3), (3, 3), (7, 3), (12, 0), (20, 9), (20, 19), (33, 5), (40, 16), (60, 25), (25, 12)]
    for T, L in cases:
        for V in (3, 5):
            lp = R.make_lp(family, T, V, rng)
            ids = rng.integers(0, V - 1, size=L)
            a, b = R.full(lp, ids, V - 1), R.lattice_banded(lp, ids, V - 1)
            assert a["ok"] == b["ok"], (T, L, V)
            for k in ("start", "end"):
                assert np.array_equal(a[k], b[k]), (T, L, V, k)
            for k in ("conf", "score", "total"):
                assert np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)), (T, L, V, k)


def _call(lp, ids_list, blank, **kw):
    return capi.ctc_align(lp, ids_list, blank, **kw)


def test_argument_checks_need_no_device():
    import ctypes as C
    L = capi.lib()
    lp = B.log_softmax32(np.zeros((1, 4, 5)))
    for bad in ([[5]], [[-1]], [[4]], [[0, 4, 1]]):                  # an id outside [0, V), an id equal to blank (4)
        with pytest.raises(capi.PkError) as e:
            _call(lp, bad, 4)
        assert e.value.code == -1 and str(e.value), bad
    ids = np.array([0, 1, 2], np.int32); st = np.zeros(3, np.int32); en = np.zeros(3, np.int32); cf = np.zeros(3, np.float32)
    sc = np.zeros(2, np.float32); ok = np.zeros(2, np.int32)
    lp2 = B.log_softmax32(np.zeros((2, 4, 5)))

    def raw(off, B_=2):
        off = np.asarray(off, np.int32)
        return L.pk_ctc_align(capi._f(lp2), None, B_, 4, 5, 4, capi._i(ids), capi._i(off), capi._i(st), capi._i(en), capi._f(cf), capi._f(sc), None,
                              capi._i(ok))
    assert raw([0, 2, 1]) == -1                                      # non-monotone offsets
    assert raw([1, 2, 3]) == -1                                      # offsets that do not start at 0
    assert raw([0, 1, 3], B_=0) == -1 and raw([0, 1, 3], B_=-3) == -1    # B < 1


def test_compute_call_without_a_device_fails_loudly():
    """Valid arguments: -4 (PK_ERR_NO_DEVICE) where no device is present, as every other compute entry point; a result where one is."""
    lp = B.log_softmax32(np.zeros((1, 4, 5)))
    if capi.device_count() > 0:
        assert _call(lp, [[0, 1]], 4)[0]["ok"] == 1
        return
    with pytest.raises(capi.PkError) as e:
        _call(lp, [[0, 1]], 4)
    assert e.value.code == -4 and "no CPU path" in str(e.value)
