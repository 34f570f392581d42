"""CPU checks of the CTC prefix beam search specification (tests/ctc_beam_ref.py) and of its public surface:
the fp32 reference against a float64 brute force over all V^T paths, the forced alignment's invariants, and the new C ABI symbols
(declared, exported, loud without a device).  The device side is compared with the same reference in tests/test_gpu_ctc_beam.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from parakeet_cpp_amd import capi

import ctc_beam_ref as R

HEADER = os.path.join(ROOT, "include", "parakeet_amd.h")
BEAM_SYMBOLS = ["pk_beam_options_default", "pk_ctc_beam_search", "pk_ctc_beam_decode", "pk_ctc_beam_decode_ragged", "pk_ctc_beam_decode_timed",
                "pk_transcribe_pcm_nbest", "pk_nbest_free"]

# Error bound of an fp32 score against exact arithmetic.  Per frame a prefix's value passes through at most: one add of lp (rounding
# <= 2^-24 |x|), lae for p_nb and lae for the score, each: exp and log evaluated to ~1 ulp of values <= 1 and the sum 1 + e (<= 3 * 2^-23
# absolute together) and the final add (2^-24 |x|).  lae is a log of a sum of exponentials, so an input error passes through with a factor
# <= 1 (no amplification).  Together <= 6 * 2^-23 + 3 * 2^-24 |x| <= 8 * 2^-23 max(1, |x|) per frame, and |x| <= |score| up to the terms
# of the frames still to come (log-probs only decrease a prefix's total), so over T frames: 8 T 2^-23 max(1, |score|).
def score_bound(T, score):
    return 8.0 * T * 2.0 ** -23 * max(1.0, abs(score))


CASES = [(1, 2, 0), (2, 3, 1), (3, 4, 2), (4, 4, 3), (5, 3, 4), (6, 3, 5), (6, 4, 6), (5, 4, 7), (6, 2, 8)]


@pytest.mark.parametrize("T,V,seed", CASES)
@pytest.mark.parametrize("family", ["uniform", "peaky"])
def test_reference_matches_float64_brute_force(T, V, seed, family):
    rng = np.random.default_rng(100 + seed)
    lp = R.log_softmax32(rng.normal(size=(T, V)) * (0.3 if family == "uniform" else 4.0))
    blank = V - 1
    bf = R.brute_force(lp, blank)
    W = len(bf)                                                     # every prefix fits: nothing is pruned
    got = R.beam_search(lp, blank, beam_width=W, token_prune=V - 1, n_best=W)
    assert sorted(p for p, _ in got) == sorted(bf), "the final beam holds exactly the label strings of the brute force"
    worst = 0.0
    for p, s in got:
        err = abs(float(s) - bf[p])
        worst = max(worst, err / score_bound(T, bf[p]))
        assert err <= score_bound(T, bf[p]), (p, float(s), bf[p])
    print(f"T={T} V={V} {family}: {len(bf)} prefixes, worst |fp32 - float64| = {worst:.3f} of the bound")
    # same order wherever the float64 scores of neighbours (in the fp32 order) are further apart than both bounds
    for (p0, _), (p1, _) in zip(got, got[1:]):
        gap = bf[p0] - bf[p1]
        if abs(gap) > score_bound(T, bf[p0]) + score_bound(T, bf[p1]):
            assert gap > 0, (p0, p1, bf[p0], bf[p1])


def test_narrow_beam_returns_sorted_distinct_prefixes():
    rng = np.random.default_rng(5)
    lp = R.log_softmax32(rng.normal(size=(40, 33)) * 2.0)
    got = R.beam_search(lp, 32, beam_width=8, token_prune=4, n_best=8)
    assert len(got) == 8 and len({p for p, _ in got}) == 8
    sc = [float(s) for _, s in got]
    assert sc == sorted(sc, reverse=True)
    assert all(len(p) <= 40 for p, _ in got)


@pytest.mark.parametrize("seed", range(6))
def test_alignment_invariants(seed):
    rng = np.random.default_rng(200 + seed)
    T, V = int(rng.integers(1, 40)), int(rng.integers(3, 12))
    lp = R.log_softmax32(rng.normal(size=(T, V)) * 2.0)
    blank = V - 1
    for p, _ in R.beam_search(lp, blank, beam_width=6, token_prune=min(4, V - 1), n_best=6):
        al = R.viterbi_align(lp, p, blank)
        assert al is not None, "a hypothesis of the search can always be aligned"
        L = len(p)
        st, en = al["start"], al["end"]
        assert np.all(st <= en) and np.all(st >= 0) and np.all(en < T)
        assert np.all(st[1:] > en[:-1]), "runs are ordered and disjoint"
        path, sym = al["path"], al["sym"]
        for k in range(L):                                           # contiguous: exactly the frames start..end sit in the token's state
            assert np.array_equal(np.nonzero(path == 2 * k + 1)[0], np.arange(st[k], en[k] + 1))
            if k and p[k] == p[k - 1]:
                assert st[k] > en[k - 1] + 1, "a repeated token needs a blank between its runs"
        s = np.float32(lp[0, sym[path[0]]])                          # re-scoring the path: the same adds in the same order
        for t in range(1, T):
            s = np.float32(s + lp[t, sym[path[t]]])
        assert s.view(np.uint32) == np.float32(al["score"]).view(np.uint32)
        assert np.array_equal(al["conf"].view(np.uint32), R._math("exp", lp[st, list(p)]).view(np.uint32) if L else np.zeros(0, np.uint32))


def test_alignment_refuses_what_cannot_be_aligned():
    lp = R.log_softmax32(np.zeros((2, 4)))
    assert R.viterbi_align(lp, (0, 1, 2), 3) is None                 # L > T
    assert R.viterbi_align(lp, (1, 1), 3) is None                    # a repeat needs three frames
    assert R.viterbi_align(lp, (0, 1), 3) is not None


def test_reentry_case_exists_on_the_reference():
    lp, ev = R.find_reentry_case()
    assert lp is not None and ev, "no input found on which a prefix leaves the beam, re-enters and is merged by its string"


def test_beam_symbols_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", txt))
    L = capi.lib()
    for s in BEAM_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/parakeet_amd.h"
        assert hasattr(L, s), f"{s} is not exported by libparakeet_amd.so"
        assert s in capi._LATE_SIGNATURES, f"{s} has no ctypes signature in capi.py"
    assert "pk_beam_options" in txt and "pk_nbest" in txt
    o = capi.beam_options()
    assert (o.beam_width, o.token_prune, o.n_best, o.timestamps) == (8, 16, 1, 0)
    assert C.sizeof(capi.PkBeamOptions) == 16


def test_beam_parameters_out_of_range_are_refused():
    lp = np.zeros((1, 3, 5), np.float32)
    for kw in (dict(beam_width=0), dict(beam_width=33), dict(token_prune=0), dict(token_prune=33), dict(n_best=0),
               dict(beam_width=4, n_best=5)):
        with pytest.raises(capi.PkError) as e:
            capi.ctc_beam_search(lp, 4, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(capi.PkError) as e:
        capi.ctc_beam_search(lp, 5)                                  # blank outside the vocabulary
    assert e.value.code == -1


@pytest.mark.skipif(capi.device_count() > 0, reason="checks the no-GPU failure mode")
def test_beam_search_without_a_device_is_a_loud_error(tmp_path):
    from conftest import pk
    from parakeet_cpp_amd import synth
    with pytest.raises(capi.PkError) as e:
        capi.ctc_beam_search(np.zeros((1, 3, 5), np.float32), 4)
    assert e.value.code == -4 and "no CPU path" in str(e.value)
    cfg = pk.make_tiny_config()
    wp = tmp_path / "t.safetensors"
    synth.save_weights(str(wp), synth.synth_weights(cfg))
    m = capi.Model(str(wp), cfg)                                     # host-side load works without a GPU
    with pytest.raises(capi.PkError) as e:
        m.ctc_beam_decode(np.zeros((1, 4, cfg.hidden_size), np.float32))
    assert e.value.code == -4
    with pytest.raises(capi.PkError) as e:
        m.transcribe_nbest([np.zeros(16000, np.float32)])
    assert e.value.code == -4
