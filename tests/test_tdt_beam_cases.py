"""CPU: the table joints of tests/tdt_beam_cases.py do what they were written for -- shown by the specification alone (tests/tdt_beam_ref.py,
tests/tdt_beam_lm_ref.py), before tests/test_gpu_tdt_beam_kernels.py holds the kernels against the same searches."""
import numpy as np
import pytest

import tdt_beam_cases as TC
import tdt_beam_lm_ref as RL
import tdt_beam_ref as R


def walks(name, **kw):
    return [TC.walk_of(name, b, **kw) for b in range(TC.CASES[name].B)]


def live_rows(case, ws):
    """(clip, hypothesis) of every row some step of the case expands"""
    return [(b, h) for b, (steps, _) in enumerate(ws) for s in steps for h in s["before"] if h[1] < case.Ts[b]]


@pytest.mark.parametrize("name", list(TC.CASES))
def test_every_case_finishes_hypotheses_with_tokens_and_merges_duplicates(name):
    case, ws = TC.CASES[name], walks(name)
    assert all(out["ok"] == 1 for _, out in ws), "a clip without a finished hypothesis"
    assert sum(int(out["lens"].sum()) for _, out in ws) > 0, "no finished hypothesis holds a token"
    assert all(len(steps) <= case.cap for steps, _ in ws)
    merged = [m for steps, _ in ws for s in steps for m in s["info"]["merged"]]
    assert merged, "no duplicate state was merged"
    rows = live_rows(case, ws)
    picks = [R.expand_row(*case.logprobs(b, h[1], h[0]), case.blank, case.K, case.Kd)[0] for b, h in rows]
    if case.family == "one-lane":
        # a lane owns ceil((V - lane) / 64) labels: 4 of the K picks from one lane where a lane owns that many
        most = max(max(np.bincount([i % 64 for i, _ in labs if i != case.blank], minlength=64)) for labs in picks)
        assert most >= min(4, case.K, (case.V - 1) // 64), most
    if case.family == "holes":
        assert any(x == -np.inf for labs in picks for i, x in labs if i != case.blank), "no -inf pick"
        assert any(np.isfinite(x) for labs in picks for i, x in labs if i != case.blank)
    if case.family in ("ties", "rising"):
        tied = sum(1 for labs in picks for (i, x), (j, y) in zip(labs, labs[1:]) if x == y)
        assert tied > 0, "no two neighbouring picks hold the same log-prob"
    if case.family == "rising":
        # within the winning lane's stride the value grows with the id: the first pick is never the lane's first element
        assert all(next(i for i, _ in labs if i != case.blank) >= 64 for labs in picks if case.V > 128)
    if name == "long-prefix":
        assert any(n > 256 and other for n, t, other in merged), "no duplicate of more than 256 tokens from another slot"
        assert ws[0][1]["lens"].max() == case.max_tokens == 300
    if name == "full-pool-v1025":
        assert case.W + case.W * (case.K + 1) * case.Kd == 2192
        assert any(sum(h[1] < case.Ts[0] for h in s["before"]) == 16 for s in ws[0][0]), "no step with 16 live slots: the pool never fills"


def test_the_table_covers_the_sizes_and_placements():
    cs = list(TC.CASES.values())
    assert {c.V for c in cs} >= {2, 64, 65, 128, 129, 1025, 8193}
    assert {c.K for c in cs} >= {1, 4, 16} and {c.W for c in cs} >= {1, 3, 16}
    assert {c.B * c.W for c in cs} >= {5, 16, 48} and all(c.B * c.W <= 32 for c in cs if c.V == 8193)
    assert any(c.Kd == 1 < c.D for c in cs) and any(c.Kd == c.D > 1 for c in cs)
    assert {tuple(c.durations) for c in cs} >= {(0, 1, 2, 3, 4), (1,), tuple(range(8))}
    assert any(sorted(c.durations) != c.durations and 0 in c.durations and 8 in c.durations for c in cs)
    assert any(sorted(c.Ts) == [1, 2, 6] for c in cs) and all(max(c.Ts) <= 8 for c in cs)
    assert {c.family for c in cs} == {"ties", "one-lane", "rising", "holes", "peaky", "long"}
    for name in TC.CASES:
        walks(name)                                                 # (draws every row a search meets)
    where = lambda c: "first" if c.blank == 0 else "last" if c.blank == c.V - 1 else "middle"
    seen = {(where(c), m) for c in cs for m in c.modes}
    want = {(w, m) for w in ("first", "middle", "last") for m in TC.BLANK_MODES} - {("first", "tie-low"), ("last", "tie-high")}
    assert seen >= want, want - seen


def test_info_changes_nothing_and_names_the_parent():
    case = TC.CASES["ties-v65"]
    for b in range(case.B):
        for s in TC.walk_of("ties-v65", b)[0]:
            plain = R.step(s["before"], case.joint(b), case.Ts[b], case.blank, case.durations, case.W, case.K, case.Kd, case.max_tokens)
            assert plain == s["after"]
            for h, w in zip(s["after"], s["info"]["parent"]):
                par = s["before"][w]
                assert h[0][: len(par[0])] == par[0] and len(h[0]) - len(par[0]) in (0, 1) and h[1] >= par[1]


@pytest.mark.parametrize("name,lm_name,alpha,beta", TC.FUSED)
def test_fused_cases_walk_the_model(name, lm_name, alpha, beta):
    case, ref = TC.CASES[name], TC.ref_lm(TC.CASES[name].V, lm_name)
    ws = walks(name, lm_name=lm_name, alpha=alpha, beta=beta)
    assert sum(int(out["lens"].sum()) for _, out in ws) > 0
    states = {TC.lm_state_of(ref, h[4]) for steps, _ in ws for s in steps for h in s["after"]}
    assert len(states) > 2, "the automaton never leaves its first states"
    if alpha != 0.0:
        plain = walks(name)
        assert any(not np.array_equal(a[1]["ids"], b[1]["ids"]) or not np.array_equal(a[1]["score"], b[1]["score"]) for a, b in zip(ws, plain)), \
            "the model changes nothing"
    for steps, out in ws:
        assert (out["lm_score"][out["score"] == -np.inf] == 0).all()
