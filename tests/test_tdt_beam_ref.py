"""CPU: the written specification of the TDT beam search (tests/tdt_beam_ref.py) against an enumeration of every
path, its tie and duplicate rules on constructed rows, and its W = K = Kd = 1 form against the oracle's greedy loop."""
import numpy as np
import pytest

from parakeet_cpp_amd import capi, synth

import tdt_beam_ref as R

F = np.float32
DUR = [0, 1, 2]


def random_joint(seed, V, D):
    """Random log-softmax tables, seeded per (t, prefix)."""
    def joint(t, prefix):
        rng = np.random.default_rng([seed, t, len(prefix), *prefix])
        def lsm(x):
            x = x - x.max()
            return (x - np.log(np.exp(x).sum())).astype(np.float32)
        return lsm(rng.normal(size=V) * 2), lsm(rng.normal(size=D) * 2)
    return joint


def every_path(joint, T, blank, V, dur, max_tokens):
    """Every path of the lattice to the end -> {prefix: best left-to-right fp32 sum}, states merged by (prefix, t) as the search merges them is
    NOT done here: plain enumeration."""
    best = {}

    def go(t, prefix, score):
        if t >= T:
            if prefix not in best or score > best[prefix]:
                best[prefix] = score
            return
        logp, dl = joint(t, prefix)
        for i in range(V):
            if i != blank and len(prefix) >= max_tokens:
                continue
            for d in range(len(dur)):
                s = F(score + F(logp[i] + dl[d]))
                if i == blank:
                    go(t + max(dur[d], 1), prefix, s)
                else:
                    go(t + dur[d], prefix + (i,), s)
    go(0, (), F(0.0))
    return best


@pytest.mark.parametrize("T,V,mt,seed", [(1, 3, 2, 1), (3, 3, 3, 2), (4, 4, 2, 3), (4, 3, 3, 4), (2, 4, 3, 5)])
def test_unpruned_search_equals_the_enumeration_of_every_path(T, V, mt, seed):
    blank = V - 1
    joint = random_joint(seed, V, len(DUR))
    want = every_path(joint, T, blank, V, DUR, mt)
    # a beam wider than the lattice has states: nothing is pruned (the device's limit of 16 is not the specification's)
    trace = []
    BIG, N = 1 << 20, 64
    r = R.search(joint, T, blank, DUR, BIG, 16, 8, N, mt, trace=trace)
    assert all(len(b) < BIG for b in trace)
    top = max(want.items(), key=lambda kv: float(kv[1]))
    assert r["ok"] == 1 and tuple(r["ids"][0, :r["lens"][0]]) == top[0]
    assert F(r["score"][0]).view(np.uint32) == F(top[1]).view(np.uint32)
    got = {tuple(r["ids"][n, :r["lens"][n]]): r["score"][n] for n in range(N) if r["score"][n] > -np.inf}
    assert len(got) == min(N, len(want)), "every prefix that reaches the end is returned once"
    for p, s in got.items():
        assert F(s).view(np.uint32) == F(want[p]).view(np.uint32), p
    assert all(r["score"][n] >= r["score"][n + 1] for n in range(N - 1))


def table_joint(rows):
    """joint from a dict (t, prefix) -> (logp, dl); any fp32 values are valid inputs of the search"""
    return lambda t, prefix: tuple(np.asarray(a, np.float32) for a in rows[(t, tuple(prefix))])


def test_row_order_ties_go_to_the_lower_id_and_the_blank_sorts_with_the_labels():
    labs, durs = R.expand_row([-1.0, -0.5, -0.5, -2.0, -0.5], [-1.0, -0.25, -0.25], blank=4, K=2, Kd=2)
    assert [i for i, _ in labs] == [1, 2, 4] and [i for i, _ in durs] == [1, 2]
    labs, _ = R.expand_row([-1.0, -0.5, -0.5, -2.0, -0.25], [-1.0], blank=4, K=3, Kd=1)
    assert [i for i, _ in labs] == [4, 1, 2, 0]
    labs, durs = R.expand_row([-1.0, -3.0], [-1.0, -2.0], blank=0, K=16, Kd=8)      # K, Kd clamp to V - 1, D
    assert [i for i, _ in labs] == [0, 1] and len(durs) == 2


def test_blank_arcs_of_durations_0_and_1_are_one_state_and_the_earlier_stays():
    # one step at T = 1.  Blank with durations 0, 1 and 2 all reach (t = 1, ()): one state, the best score stays; label 0 with durations 1 and 2
    # both reach (1, (0,)); with duration 0 it stays live at (0, (0,))
    rows = {(0, ()): ([-4.0, -0.5], [-0.25, -1.0, -3.0])}
    start = [((), 0, F(0.0), ())]
    beam = R.step(start, table_joint(rows), 1, 1, DUR, 4, 1, 3, 2)
    assert [(p, t) for p, t, _, _ in beam] == [((), 1), ((0,), 0), ((0,), 1)]
    assert [s for _, _, s, _ in beam] == [F(-0.75), F(-4.25), F(-5.0)]
    assert beam[2][3] == ((0, 1, F(-4.0)),), "of the equal states the better score stays (duration 1 over duration 2)"
    # equal scores: the earlier pool entry stays (duration rank 0 of the tie, index 1)
    rows = {(0, ()): ([-4.0, -0.5], [-3.0, -1.0, -1.0])}
    beam = R.step(start, table_joint(rows), 1, 1, [0, 1, 2], 4, 1, 3, 2)
    assert beam[1][:3] == ((0,), 1, F(-5.0)) and beam[1][3][0][1] == 1
    # W cuts after the duplicates are merged
    assert [(p, t) for p, t, _, _ in R.step(start, table_joint(rows), 1, 1, DUR, 2, 1, 3, 2)] == [((), 1), ((0,), 1)]


def test_a_tie_between_states_goes_to_the_earlier_pool_position_and_w1_is_the_greedy_argmax():
    # label 0 and the blank tie exactly: the label has the lower id, sorts first, and stays at W = 1 -- what the greedy argmax picks
    rows = {(0, ()): ([-0.5, -0.5], [-0.25]), (1, ()): ([-0.5, -0.5], [-0.25]), (1, (0,)): ([-3.0, -0.25], [-0.25])}
    r = R.search(table_joint(rows), 2, 1, [1], 1, 1, 1, 1, 4)
    assert r["lens"][0] == 1 and r["ids"][0, 0] == 0 and r["start"][0, 0] == 0 and r["end"][0, 0] == 0
    # max_tokens: a full hypothesis forms no label candidates
    r = R.search(table_joint({(0, ()): ([-0.1, -3.0], [-0.1, -3.0]), (0, (0,)): ([-0.1, -3.0], [-0.1, -3.0])}), 1, 1, [0, 1], 1, 1, 1, 1, 1)
    assert r["ok"] == 1 and r["lens"][0] == 1 and r["steps"] == 2


def test_nothing_is_live_at_the_step_cap():
    """Every arc adds at least one to t + len(prefix), so after T + max_tokens steps every hypothesis sits at t = T: the cap of the host
    loop cannot cut a search short, and ok = 0 needs a clip whose candidates are all absent."""
    for seed in range(6):
        T, mt = 3, 4
        joint = random_joint(seed, 4, 3)
        biased = lambda t, p: (joint(t, p)[0], np.asarray([-0.01, -5.0, -6.0], np.float32))       # the zero duration wins: several symbols per frame
        r = R.search(biased, T, 3, DUR, 3, 2, 1, 3, mt)
        assert r["ok"] == 1 and r["steps"] <= T + mt


@pytest.fixture(scope="module")
def tiny_oracles(orc):
    from conftest import pk
    cfgs = [pk.make_tiny_config(),
            pk.make_tiny_config(num_lstm_layers=2, vocab_size=78, blank_id=77, ctc_vocab_size=78, durations=[0, 1, 2, 4], name="tiny2l-v78")]
    return [(c, orc.Model(c, synth.synth_weights(c, seed=31))) for c in cfgs]


def test_width_one_is_the_oracles_greedy_loop(tiny_oracles):
    n_tokens = 0
    for cfg, om in tiny_oracles:
        for seed, T in ((11, 30), (12, 24), (13, 12), (14, 7), (15, 2), (16, 1)):
            x = np.random.default_rng(seed).standard_normal((T, cfg.hidden_size)).astype(np.float32)
            enc = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
            cap = T * (cfg.max_symbols_per_step + 1) + 16
            walk = om.tdt_score(enc)                                # the greedy path, decision by decision
            assert walk["n"] < cap, "choose a seed for which the oracle's greedy loop ends before its own evaluation cap"
            g = om.tdt_greedy(enc[None])
            L = int(g["lens"][0])
            mt = g["ids"].shape[1]
            r = R.search(R.oracle_joint(om, enc), T, cfg.blank_id, list(cfg.durations), 1, 1, 1, 1, mt)
            assert r["ok"] == 1 and r["lens"][0] == L
            for k in ("ids", "start", "end"):
                assert np.array_equal(r[k][0, :L], g[k][0, :L]), (cfg.name, seed, k)
            assert np.array_equal(r["conf"][0, :L].view(np.uint32), g["conf"][0, :L].view(np.uint32))
            n_tokens += L
    assert n_tokens > 3, "degenerate test: nothing decoded"


def test_entry_points_are_exported_and_refuse_bad_arguments_without_a_device():
    L = capi.lib()
    for name in ("pk_tdt_beam_options_default", "pk_tdt_beam_decode", "pk_tdt_beam_decode_ragged", "pk_tdt_beam_decode_timed", "pk_transcribe_pcm_nbest_tdt"):
        assert hasattr(L, name), name
    o = capi.tdt_beam_options()
    assert (o.beam_width, o.label_prune, o.duration_prune, o.n_best) == (8, 8, 2, 1)
    z = np.zeros(4, np.float32); zi = np.zeros(4, np.int32)
    assert L.pk_tdt_beam_decode(None, capi._f(z), 1, 1, None, 1, capi._i(zi), capi._i(zi), capi._f(z), None, None, None, None, None) == -1
