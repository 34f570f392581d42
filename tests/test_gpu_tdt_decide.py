"""The greedy decision kernel of the TDT / RNNT decode loop alone (kernels/decode_dev.hpp tdt_decide_one through pk_diag_tdt_decide: a handful of back-to-back
launches on caller-given state) against the plain restatement of tests/tdt_decide_ref.py (tests/test_tdt_decide_ref.py holds that restatement to the oracle's
decoders and to planted faults on the CPU).

Cases: tdt_decide_ref.CASES -- every value tdt_decide_form can return (kernel exact / fast / boost / score x NC 3 / 6 / 12 x row staging 5 slots / 33 slots /
batches of 8 / frame window), exact ties placed per thread, per wave, across waves, against the last index and against the blank, a single winner with its
runner-up at the same placements (the margin shows the runner-up reduction), ties of ROUNDED log-probs, window walks that meet the cap inside the window,
random decision scripts that run into max_tokens, the safety cap, the end of ragged utterances and finished utterances, the prediction-net caching words, the
frame window, tries and forced paths.  The form the launcher reports must be the one the case list expects.

Exact, boost and score kernels: every word bit for bit -- state words, token arrays, h / c, margin, need / z, active trie states, score rows -- and the
pattern-filled rows and guard words behind the batch untouched.  Fast kernel (h_bf16): integer words, h / c and z exact wherever the float64 margin of every
decision of the utterance exceeds the derived limit; each token's conf within the bound of its own decision's winner, the margin within the bound of the
decisions that can have set it; a decision under the limit ends that utterance's comparison and may only happen in the tie families.  The margin of a decision
is taken to the best DIFFERENT logit value: equal logits give equal computed log-probs, so the fast kernel too must decide an exact tie by the lowest index,
and the "ties" cases are compared in full.  In the "rounded" cases the candidates differ by an ulp of the logit, nearly every live utterance goes under the
limit at its first decision, and little more than the form, the guard rows and the finished utterances is checked there.

D = 9 runs with logits whose duration maximum stays below index 8: TdtState holds 8 durations, the engine refuses more, and pk_diag_tdt_decide refuses a row
that could choose past them.

Worst observed err / bound of the fast form on the MI355X (pytest -s prints every case): see the line FAST_WORST below.
"""
import numpy as np
import pytest

import tdt_decide_ref as R

pytestmark = pytest.mark.gpu

FAST_WORST = "conf err / bound 0.207 (fast-form-v7-d5-l1h768-b5; 0.06 at most from V = 64 up, 0.0005 at V = 8193), margin err / bound 0.0008 (fast-runnerup-v600)"
IDS = [R.case_id(c) for c in R.CASES]
FILL = np.uint32(R.FILL32)


@pytest.fixture(scope="module")
def fns(orc):
    return orc.log_softmax_rows, (lambda x: orc.math_v("exp", x))


def launch(o, n_steps=None):
    from parakeet_cpp_amd import capi
    k = o["logits"].shape[0] if n_steps is None else n_steps
    return capi.diag_tdt_decide(o["sc"], o["logits"][:k], o["hn"][:k], o["cn"][:k], o["st"])


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def exact_mismatches(o, c, S, got, rows=None):
    """names of the buffers that differ from the reference (rows: the utterances to compare; default all)"""
    B = o["sc"]["B"]
    sel = np.arange(B) if rows is None else np.asarray(rows, int)
    bad = []
    names = [k for k in R.STATE_WORDS + ("conf", "margin", "need", "n_act", "score_lab", "score_dur") if k in S and S[k] is not None and k in got]
    if c["h_bf16"]:
        names = [k for k in names if k not in ("conf", "margin")]
    for k in names:
        g, w = words(got[k]), words(np.asarray(S[k]))
        lead = w.shape[0]
        if k in ("score_lab", "score_dur"):
            if not np.array_equal(g, w):
                bad.append(k)
            continue
        if not np.array_equal(g[:lead][sel], w[sel]):
            bad.append(k)
        if not np.all(g[lead:] == FILL):
            bad.append(k + ": stores behind the batch")
    for k in ("h", "c"):
        w = words(np.asarray(S[k]))                                  # [L][B][width]
        n = w.size * w.dtype.itemsize // 4
        g = got[k][:n].view(w.dtype).reshape(w.shape)
        if not np.array_equal(g[:, sel], w[:, sel]):
            bad.append(k)
        if not np.all(got[k][n:] == FILL):
            bad.append(k + ": stores behind the state")
    if "z" in got:
        w = words(np.asarray(S["z"]))                                # (as words: a row no blank formed keeps the NaN pattern)
        n = w.size * w.dtype.itemsize // 4
        F = w.shape[0] // B
        zsel = (sel[:, None] * F + np.arange(F)).reshape(-1)
        if not np.array_equal(got["z"][:n].view(w.dtype).reshape(w.shape)[zsel], w[zsel]):
            bad.append("z")
        if not np.all(got["z"][n:] == FILL):
            bad.append("z: stores behind the rows")
    if "act" in got:
        for b in sel:
            na = int(S["n_act"][b])
            if c["compare_act"] and sorted(got["act"][b, :na].tolist()) != sorted(S["act"][b, :na].tolist()):
                bad.append(f"act[{b}]")
    if rows is None and int(got["done_count"][0]) != int(S["done_count"]):
        bad.append("done_count")
    return bad


def first_bad_step(o, c, fns):
    """replay with fewer launches: the first launch after which a word differs (bisection)"""
    lo, hi = 1, o["logits"].shape[0]
    while lo < hi:
        mid = (lo + hi) // 2
        if exact_mismatches(o, c, R.run(o, *fns, n_steps=mid), launch(o, mid)):
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("c", [c for c in R.CASES if not c["h_bf16"]], ids=[i for i, c in zip(IDS, R.CASES) if not c["h_bf16"]])
def test_exact_forms_word_for_word(c, fns):
    from parakeet_cpp_amd import capi
    o = R.make_case(c)
    S = R.run(o, *fns)
    got = launch(o)
    assert capi.tdt_form(got["form"]) == R.form_of(o["sc"], o["boost"], o["score"])
    bad = exact_mismatches(o, c, S, got)
    assert not bad, f"{bad}; first differing launch: {first_bad_step(o, c, fns)}"
    live = np.flatnonzero(o["st"]["done"] == 0)
    if not o["score"]:                                              # (a forced path of no steps finishes without a decision)
        assert live.size and (np.asarray(S["steps"])[live] > o["st"]["steps"][live]).all(), "degenerate: a live utterance took no decision"


@pytest.mark.parametrize("c", [c for c in R.CASES if c["h_bf16"]], ids=[i for i, c in zip(IDS, R.CASES) if c["h_bf16"]])
def test_fast_form_within_its_bound(c, fns):
    from parakeet_cpp_amd import capi
    o = R.make_case(c)
    log = []
    S = R.run(o, *fns, fast=True, log=log)
    got = launch(o)
    assert capi.tdt_form(got["form"]) == R.form_of(o["sc"])
    B, mt = o["sc"]["B"], o["sc"]["max_tokens"]
    unsafe = {}
    for e in log:
        if e["m64"] <= e["limit"] and e["b"] not in unsafe:
            unsafe[e["b"]] = e["n_out"]
    assert not unsafe or c["fam"] in R.TIE_FAMILIES, f"decisions under the limit outside the tie families: {unsafe}"
    safe = [b for b in range(B) if b not in unsafe]
    bad = exact_mismatches(o, c, S, got, rows=safe if unsafe else None)
    assert not bad, bad
    for b, n in unsafe.items():                                     # the tokens stored before the close decision still count
        n = min(n, mt)
        for k in ("ids", "start", "end"):
            assert np.array_equal(got[k][b, :n], S[k][b, :n]), (k, b)
    worst_c = worst_m = 0.0
    u = 2.0 ** -23                                                  # the fp32 rounding of the margin itself (one subtraction: half of this), with room
    uc = 2.0 ** -22                                                 # conf = the specification's fp32 exp of the computed log-prob, taken at 2 ulp
    for b in safe:
        decs = [e for e in log if e["b"] == b]
        for e in decs:                                              # each stored token against the bound of ITS decision's winner: |exp(lp + d) - exp(lp)|
            if not e["tok"] or e["n_out"] >= mt:
                continue
            w, g = float(S["conf"][b, e["n_out"]]), float(got["conf"][b, e["n_out"]])
            assert not np.isnan(g), f"conf[{b}, {e['n_out']}]: a token the kernel left out keeps the NaN pattern"
            worst_c = max(worst_c, abs(g - w) / (w * (np.expm1(e["bk"]) + uc)))
        wm, gm = float(S["margin"][b]), float(got["margin"][b])
        if np.isfinite(wm):                                         # the running minimum: only a decision that can be the smallest contributes its error
            top = min(e["mg"] + e["emg"] for e in decs)
            emg = max(e["emg"] for e in decs if e["mg"] - e["emg"] <= top)
            worst_m = max(worst_m, abs(gm - wm) / (emg + u * max(1.0, abs(wm))))
        else:
            assert gm == wm
    print(f"{R.case_id(c)} {capi.tdt_form(got['form'])}: compared {len(safe)} of {B}, conf err / bound {worst_c:.4f}, margin err / bound {worst_m:.4f}")
    assert worst_c <= 1.0 and worst_m <= 1.0
