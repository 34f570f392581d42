"""CPU checks of tests/tdt_decide_ref.py, the reference tests/test_gpu_tdt_decide.py and tests/test_gpu_ctc_greedy.py hold the decision kernels to:
its log-softmax path is the oracle's own, its control flow reproduces the oracle's decoders when driven with the oracle's own decisions, every planted
fault is caught by a named case, the case list reaches every form of the launcher, and the fast form's exclusion rule excludes nothing on ordinary cases."""
import numpy as np
import pytest

import tdt_decide_ref as R
from conftest import pk
from parakeet_cpp_amd import synth


@pytest.fixture(scope="module")
def fns(orc):
    return orc.log_softmax_rows, (lambda x: orc.math_v("exp", x))


def fresh(sc, Tb=None):
    """the state the decode loop's initialisation leaves (kernels/decode.hip tdt_init_kernel)"""
    B, mt, L, Hp = sc["B"], sc["max_tokens"], sc["L"], sc["Hp"]
    z = lambda: np.zeros(B, np.int32)
    st = dict(t=z(), steps=z(), n_out=z(), nsym=z(), done=z(), token=np.full(B, sc["blank"], np.int32), lens=z(), done_count=0,
              h=np.zeros((L, B, Hp), np.float32), c=np.zeros((L, B, Hp), np.float32), ids=np.zeros((B, mt), np.int32), start=np.zeros((B, mt), np.int32),
              end=np.zeros((B, mt), np.int32), conf=np.zeros((B, mt), np.float32), margin=np.full(B, np.inf, np.float32))
    if Tb is not None:
        st["Tb"], st["row0"] = np.asarray(Tb, np.int32), np.zeros(B, np.int32)
    return st


def drive(sc, scripts, fns, Tb=None):
    """scripts: per utterance (labels, dur_idx) of every decision -> the reference's final state"""
    n = max(len(s[0]) for s in scripts) + 1
    V, D, B = sc["V"], sc["D"], sc["B"]
    logits = np.zeros((n, B, V + D), np.float32)
    for b, (lab, dur) in enumerate(scripts):
        logits[: len(lab), b] = R.script_logits(V, D, lab, dur)
    hn = np.zeros((n, sc["L"], B, sc["Hp"]), np.float32)
    return R.run(dict(sc=sc, logits=logits, hn=hn, cn=hn, st=fresh(sc, Tb)), *fns)


def model(orc, **kw):
    cfg = pk.make_tiny_config(**kw)
    return cfg, orc.Model(cfg, synth.synth_weights(cfg, seed=7))


def scalars(cfg, B, T, mt, max_steps=0):
    D = 0 if cfg.head == "rnnt" else len(cfg.durations)
    return dict(B=B, T=T, V=cfg.vocab_size, D=D, L=cfg.num_lstm_layers, Hp=cfg.pred_hidden, blank=cfg.blank_id, max_symbols=cfg.max_symbols_per_step,
                max_tokens=mt, max_steps=max_steps, keep_state=0, h_bf16=0, F=1, J=0, durations=list(cfg.durations)[:D])


def test_log_softmax_rows_is_the_oracles_ctc_row(orc, tiny_oracle, tiny_cfg, tiny_weights):
    enc = np.random.default_rng(3).standard_normal((2, 9, tiny_cfg.hidden_size)).astype(np.float32)
    lp = tiny_oracle.ctc_logprobs(enc)
    logits = orc.linear(enc.reshape(-1, enc.shape[-1]), tiny_weights["ctc_decoder_.proj_.weight"].reshape(tiny_cfg.ctc_vocab_size, -1), tiny_weights["ctc_decoder_.proj_.bias"])
    mine = orc.log_softmax_rows(logits).reshape(lp.shape)
    assert np.array_equal(mine.view(np.uint32), lp.view(np.uint32))


def test_log_softmax_rows_is_the_oracles_label_head(orc, tiny_oracle, tiny_cfg, tiny_weights):
    """the first joint evaluation of the decode (token = blank, zero LSTM state) composed from the oracle's own products and functions, its label row through
    log_softmax_rows: the bits tdt_greedy(first_logp=True) reports"""
    W, jp, Hp = tiny_weights, tiny_cfg.joint_prefix, tiny_cfg.pred_hidden
    enc = np.random.default_rng(4).standard_normal((1, 5, tiny_cfg.hidden_size)).astype(np.float32)
    want = tiny_oracle.tdt_greedy(enc, first_logp=True)["first_logp"]
    cell = "prediction_.lstm_.cells_.0."
    x = W["prediction_.embed_.weight"][tiny_cfg.blank_id][None]
    g = (orc.linear(x, W[cell + "input_proj_.weight"])[0] + W[cell + "input_proj_.bias"]) + orc.linear(np.zeros((1, Hp), np.float32), W[cell + "hidden_proj_.weight"])[0]
    i, f, gg, o = (orc.math_v(fn, g[k * Hp: (k + 1) * Hp]) for k, fn in enumerate(("sigmoid", "sigmoid", "tanh", "sigmoid")))
    cn = f * np.float32(0) + i * gg
    h = o * orc.math_v("tanh", cn)
    s = orc.linear(enc[0, :1], W[jp + "enc_proj_.weight"], W[jp + "enc_proj_.bias"])[0] + orc.linear(h[None], W[jp + "pred_proj_.weight"])[0]
    lab = orc.linear(np.maximum(s, np.float32(0))[None], W[jp + "label_proj_.weight"])[0] + W[jp + "label_proj_.bias"]
    assert np.array_equal(orc.log_softmax_rows(lab[None]).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("limits", ["plain", "cap", "few-tokens"])
def test_tdt_control_flow_against_the_oracle(orc, fns, layers, limits):
    cfg, om = model(orc, num_lstm_layers=layers)
    T, B = 40, 3
    enc = np.random.default_rng(5 + layers).standard_normal((B, T, cfg.hidden_size)).astype(np.float32)
    mt = 1 if limits == "few-tokens" else T * cfg.max_symbols_per_step
    cap = 6 if limits == "cap" else 0
    g = om.tdt_greedy(enc, max_tokens=mt, max_steps=cap, margin=True)
    scripts = []
    for b in range(B):
        s = om.tdt_score(enc[b], rows=False)
        assert np.array_equal(s["labels"], g["step_label"][b, : s["n"]]) or cap
        scripts.append((s["labels"], s["dur_idx"]))
    S = drive(scalars(cfg, B, T, mt, cap), scripts, fns)
    if limits == "few-tokens":
        assert (S["n_out"] > mt).any(), "the case must overflow max_tokens"
    if cap:
        assert (g["lens"] == -1).any(), "the case must trip the cap"
    assert np.array_equal(S["lens"], g["lens"]) and np.array_equal(S["steps"], g["steps"]) and S["done"].all()
    for b in range(B):
        n = max(int(g["lens"][b]), 0) if not cap else min(int(S["n_out"][b]), mt)
        for k in ("ids", "start", "end"):
            assert np.array_equal(S[k][b, :n], g[k][b, :n]), (k, b)


def test_rnnt_control_flow_against_the_oracle(orc, fns):
    cfg, om = model(orc, head="rnnt", durations=[], max_symbols_per_step=3)
    T, B = 10, 2
    enc = np.random.default_rng(9).standard_normal((B, T, cfg.hidden_size)).astype(np.float32)
    g = om.rnnt_greedy(enc)
    scripts = []
    for b in range(B):                                             # per frame: its tokens, then a blank unless max_symbols ran out (src/rnnt.cpp:82-107)
        lab = []
        for t in range(T):
            tk = [int(g["ids"][b, i]) for i in range(g["lens"][b]) if g["start"][b, i] == t]
            lab += tk + ([cfg.blank_id] if len(tk) < cfg.max_symbols_per_step else [])
        scripts.append((lab, None))
    S = drive(scalars(cfg, B, T, T * 3), scripts, fns)
    assert np.array_equal(S["lens"], g["lens"]) and S["done"].all()
    for b in range(B):
        n = g["lens"][b]
        assert np.array_equal(S["ids"][b, :n], g["ids"][b, :n]) and np.array_equal(S["start"][b, :n], g["start"][b, :n]) and np.array_equal(S["end"][b, :n], g["start"][b, :n])


def test_ragged_pair_against_the_oracle(orc, fns):
    cfg, om = model(orc)
    Ts = (11, 4)
    rng = np.random.default_rng(12)
    scripts, want = [], []
    for T in Ts:
        enc = rng.standard_normal((1, T, cfg.hidden_size)).astype(np.float32)
        want.append(om.tdt_greedy(enc, max_tokens=40))
        s = om.tdt_score(enc[0], rows=False)
        scripts.append((s["labels"], s["dur_idx"]))
    S = drive(scalars(cfg, 2, max(Ts), 40, max_steps=1000), scripts, fns, Tb=Ts)
    for b, g in enumerate(want):
        n = g["lens"][0]
        assert S["lens"][b] == n and S["steps"][b] == g["steps"][0]
        for k in ("ids", "start", "end"):
            assert np.array_equal(S[k][b, :n], g[k][0, :n]), (k, b)


@pytest.mark.parametrize("c", R.CTC_CASES, ids=[c["name"] for c in R.CTC_CASES])
def test_ctc_reference_against_the_oracle(orc, c):
    o = R.make_ctc_case(c)
    lp = orc.log_softmax_rows(o["logits"][:, : o["n"]])
    trie = R.Trie(*o["trie"]) if o["trie"] else None
    otrie = orc.Trie(o["phrases"]) if o["trie"] else None
    r0 = 0
    for T in o["n_frames"]:
        u = lp[r0: r0 + T]
        ids, st, en, cl = R.ctc_greedy(u, o["blank"], trie)
        g = orc.ctc_greedy_boosted(u[None], o["blank"], otrie, o["boost"]) if trie else orc.ctc_greedy(u[None], o["blank"])
        n = g["lens"][0]
        assert n == len(ids) and np.array_equal(g["ids"][0, :n], ids) and np.array_equal(g["start"][0, :n], st) and np.array_equal(g["end"][0, :n], en)
        assert np.array_equal(g["conf"][0, :n].view(np.uint32), orc.math_v("exp", cl).view(np.uint32))
        r0 += T


def compared(S):
    return {k: np.array(S[k], copy=True) for k in R.STATE_WORDS + ("h", "c", "conf", "margin", "done_count") if k in S}


def differs(a, b):
    return any(not np.array_equal(np.asarray(a[k]).view(np.uint32) if np.asarray(a[k]).dtype == np.float32 else a[k],
                                  np.asarray(b[k]).view(np.uint32) if np.asarray(b[k]).dtype == np.float32 else b[k]) for k in a)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_planted_fault_is_caught_by_its_named_case(mutant, fns):
    c = next(c for c in R.CASES if c["name"] == R.MUTANT_CAUGHT_BY[mutant])
    o = R.make_case(c)
    assert differs(compared(R.run(o, *fns)), compared(R.run(o, *fns, mut=(mutant,)))), f"{c['name']} does not notice {mutant}"


@pytest.mark.parametrize("F", [2, 4, 8])
def test_window_walk_meets_the_cap_inside_the_window(F, fns):
    """the event happens -- after ONE launch a live utterance is finished by the cap (lens == -1) at a window row f > 0, and one at row 0 -- and both cap faults
    (off by one; the walk not looking at the cap) change a word of every such case"""
    c = next(c for c in R.CASES if c["name"] == f"window-cap-f{F}")
    o = R.make_case(c)
    S = R.run(o, *fns, n_steps=1)
    live = o["st"]["done"] == 0
    assert (live & (S["lens"] == -1) & (S["last_f"] > 0)).any() and (live & (S["lens"] == -1) & (S["last_f"] == 0)).any()
    assert (S["steps"][live & (S["lens"] == -1)] == c["max_steps"]).all()
    for mutant in ("cap_off_by_one", "window_cap_ignored"):
        assert differs(compared(R.run(o, *fns)), compared(R.run(o, *fns, mut=(mutant,)))) or (F == 2 and mutant == "window_cap_ignored"), mutant
    if F == 2:                                                     # (two rows: past row 1 the window ends the walk whatever the cap says; row 0 still shows it)
        assert differs(compared(R.run(o, *fns, n_steps=1)), compared(R.run(o, *fns, mut=("window_cap_ignored",), n_steps=1)))


def test_runner_up_placements_show_in_the_margin(fns):
    """every live utterance of the runner-up family: one winner, margin = its log-prob minus the runner-up's (about 1.0, never the 6.0 to the noise), and the
    placements put winner and runner-up into one thread, one wave, and different waves"""
    for c in (c for c in R.CASES if c["fam"] == "runnerup" and not c["h_bf16"]):
        o = R.make_case(c)
        S = R.run(o, *fns)
        live = o["st"]["done"] == 0
        assert np.all(np.abs(S["margin"][live] - 1.0) < 1e-3), c["name"]
        kinds = set()
        for b in np.flatnonzero(live):
            row = o["logits"][0, b, : c["V"]]
            w, ru = int(np.argmax(row)), np.flatnonzero(row == 7.0)
            assert (row == 8.0).sum() == 1 and ru.size in (1, 2)
            for r in ru:
                kinds.add("thread" if r % 256 == w % 256 else "wave" if (r % 256) // 64 == (w % 256) // 64 else ("waves-up" if r > w else "waves-down"))
        assert kinds == {"thread", "wave", "waves-up", "waves-down"}, (c["name"], kinds)


def test_boost_flips_a_tie(fns):
    c = next(c for c in R.CASES if c["name"] == "boost-flips-tie")
    o = R.make_case(c)
    S = R.run(o, *fns)
    live = np.flatnonzero(o["st"]["done"] == 0)
    for b in live:
        n0, n1 = int(o["st"]["n_out"][b]), int(S["n_out"][b])
        assert n1 > n0 and (S["ids"][b, n0:n1] == 9).all()           # unboosted, the lower index 2 would win the tie
    o["st"]["trie"] = o["st"]["trie"][:3] + (0.0,)
    S0 = R.run(o, *fns)
    assert all((S0["ids"][b, int(o["st"]["n_out"][b]): int(S0["n_out"][b])] == 2).all() for b in live)


def test_case_list_reaches_every_decide_form():
    got = {R.form_of(R.make_case(c)["sc"], c["trie"] is not None, c["score"]) for c in R.CASES}
    assert got == R.ALL_FORMS and len(R.ALL_FORMS) == 24


def test_rounded_ties_merge_under_the_specifications_rounding(orc):
    """the rounded-tie family is what it claims: the two candidates differ as logits and are one rounded log-prob, the lower index carrying the smaller logit"""
    for c in (c for c in R.CASES if c["fam"] == "rounded" and not c["h_bf16"]):
        o = R.make_case(c)
        V = c["V"]
        for row in o["logits"].reshape(-1, V + c["D"]):
            lp = orc.log_softmax_rows(row[None, :V])[0]
            k, raw = R.first_max(lp), R.first_max(row[:V])
            assert k < raw and lp[k] == lp[raw] and row[k] < row[raw]


def test_fast_rule_excludes_nothing_on_ordinary_cases(fns):
    worst = np.inf
    for c in (c for c in R.CASES if c["h_bf16"] and c["fam"] not in R.TIE_FAMILIES):
        log = []
        R.run(R.make_case(c), *fns, fast=True, log=log)
        assert log
        for e in log:
            assert e["m64"] > e["limit"], (c["name"], e)
            worst = min(worst, e["m64"] / e["limit"])
    assert worst > 100          # scripted winners stand 6.0 above the noise; the limit is below 2e-3 at every vocabulary of the list


def test_what_the_engine_never_launches_is_refused():
    """PK_ERR_INVALID before anything is launched (the checks need no device), never the launcher's abort"""
    from parakeet_cpp_amd import capi

    def launch(o, k):
        return capi.diag_tdt_decide(o["sc"], o["logits"][:k], o["hn"][:k], o["cn"][:k], o["st"])

    base = next(c for c in R.CASES if c["name"] == "script-need-j16")
    for kw in (dict(L=4, Hp=772), dict(F=2, V=1276), dict(F=9), dict(F=2, J=1040), dict(F=2, h_bf16=1), dict(V=30000, D=5, need=False, J=0)):
        o = R.make_case(dict(base, **kw))
        with pytest.raises(capi.PkError) as e:
            launch(o, 1)
        assert e.value.code == -1, (kw, e.value)
    o = R.make_case(dict(base, D=9, need=False, J=0))
    o["logits"][0, 0, o["sc"]["V"] + 8] = 9.0                       # a duration maximum past the 8 durations the state holds
    with pytest.raises(capi.PkError) as e:
        launch(o, 1)
    assert e.value.code == -1
