"""GPU: the TDT beam search's own kernels (kernels/tdt_beam.hip: init, expand, prune, trace and their fused instantiations) ALONE, through
pk_diag_tdt_beam_step, on the table joints of tests/tdt_beam_cases.py at real vocabulary sizes -- whole searches driven step by step and held
against the written specification (tests/tdt_beam_ref.py, tests/tdt_beam_lm_ref.py) after EVERY step, bit for bit:
    expand   lab_id, lab_lp, dur_i, dur_lp, cand (and lab_ls, lab_lm) of every live row; rows of clips that are not live, slots that are not
             valid and finished hypotheses keep the fill pattern (their logits rows are NaN), and so do the guard rows past the beam;
    prune    the new beam copy (valid, t, len, score, prefix, par, born, tok, and lmstate, lm), the step's back-pointer records, live,
             steps_done, live_total; the copy the step read and the clips that are not live stay as they were;
    trace    ids, start, end, dur_idx, conf, lens, score, ok (and lm_score) after the last step.
No tolerance anywhere: the contract is equality with the specification."""
import functools

import numpy as np
import pytest

from parakeet_cpp_amd import capi

import tdt_beam_cases as TC
import tdt_beam_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
FILL = capi.SKINNY_FILL32
BEAM = ("valid", "t", "len", "par", "born", "tok", "score", "hash", "prefix")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def device_lm(V, lm_name):
    return capi.Lm.from_text(TC.arpa_of(V, lm_name))


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == FILL).all())


def want_row(case, b, h, ref, alpha, beta):
    """what the expansion stores for the live hypothesis h of clip b"""
    logp, dl = case.logprobs(b, h[1], h[0])
    labs, durs = R.expand_row(logp, dl, case.blank, case.K, case.Kd)
    with np.errstate(all="ignore"):
        cand = [F(h[2] + F(x + y)) for _, x in labs for _, y in durs]
    w = dict(lab_id=[i for i, _ in labs], lab_lp=[x for _, x in labs], dur_i=[i for i, _ in durs], dur_lp=[y for _, y in durs], cand=cand)
    if ref is not None:
        hist, lmv = h[4], h[5]
        w["lab_ls"], w["lab_lm"] = [], []
        for i, _ in labs:
            if i == case.blank:
                w["lab_ls"].append(TC.lm_state_of(ref, hist)); w["lab_lm"].append(lmv)
            else:
                with np.errstate(all="ignore"):
                    w["lab_lm"].append(F(lmv + F(F(F(alpha) * ref.lookup(hist, i)[0]) + F(beta))))
                w["lab_ls"].append(TC.lm_state_of(ref, hist + (i,)))
    return w


def check_expand(case, st, live, ref, alpha, beta, tag):
    R_ = case.B * case.W
    for r in range(st["rows"]):
        h = live.get(r)
        for k in capi.TDT_BEAM_STEP_SCRATCH:
            if k not in st:
                continue
            if h is None:
                assert untouched(st[k][r]), f"{tag} row {r}{' (guard)' if r >= R_ else ''}: {k} was written for a row the step does not expand"
    for r, (b, h) in live.items():
        want = want_row(case, b, h, ref, alpha, beta)
        for k, v in want.items():
            got = st[k][r]
            if got.dtype == np.float32:
                assert np.array_equal(bits(got), bits(v)), f"{tag} row {r} (clip {b}, t {h[1]}, {len(h[0])} tokens): {k} {got} vs {np.asarray(v)}"
            else:
                assert got.tolist() == list(v), f"{tag} row {r} (clip {b}, t {h[1]}, {len(h[0])} tokens): {k} {got.tolist()} vs {list(v)}"


def want_beam(case, b, step, ref):
    """slot -> the words the pruning stores for clip b's new beam, and the back-pointer record of the slot"""
    T, blank, out = case.Ts[b], case.blank, []
    for j in range(case.W):
        if j >= len(step["after"]):
            w = dict(valid=0, t=0, len=0, score=R.NEG, par=b * case.W + j, born=0, tok=blank, prefix=(), bp=(j, -1, 0, 0))
            if ref is not None:
                w.update(lmv=F(0.0), lmstate=0)
        else:
            h, src = step["after"][j], step["info"]["parent"][j]
            label = len(h[0]) == len(step["before"][src][0]) + 1
            bp = (src, -1, 0, 0)
            if label:
                t_em, d, x = h[3][-1]
                bp = (src, h[0][-1], t_em * 8 + d, int(np.asarray(x, np.float32).view(np.int32)))
            w = dict(valid=1, t=h[1], len=len(h[0]), score=h[2], par=b * case.W + src, born=int(label), tok=h[0][-1] if label else blank, prefix=h[0], bp=bp)
            if ref is not None:
                w.update(lmv=h[5], lmstate=TC.lm_state_of(ref, h[4]))
        out.append(w)
    return out


def check_prune(case, st, before, s, walks, ref, tag):
    W, q = case.W, (s & 1) ^ 1
    total = 0
    for b in range(case.B):
        rows = slice(b * W, (b + 1) * W)
        steps = walks[b][0]
        if s >= len(steps):                                         # the clip is not live: nothing of it moves
            for k in before:
                if k in ("live", "steps_done"):
                    assert st[k][b] == before[k][b], f"{tag} clip {b} (not live): {k}"
                elif k == "bp":
                    assert np.array_equal(st[k][:, rows], before[k][:, rows]), f"{tag} clip {b} (not live): bp"
                elif k != "live_total":
                    assert np.array_equal(st[k][:, rows], before[k][:, rows]), f"{tag} clip {b} (not live): {k}"
            continue
        want = want_beam(case, b, steps[s], ref)
        for j, w in enumerate(want):
            r, where = b * W + j, f"{tag} clip {b} slot {j}"
            for k in ("valid", "t", "len", "par", "born", "tok") + (("lmstate",) if ref is not None else ()):
                assert st[k][q, r] == w[k], f"{where}: {k} {st[k][q, r]} vs {w[k]}"
            for k in ("score",) + (("lmv",) if ref is not None else ()):
                assert bits(st[k][q, r]) == bits(w[k]), f"{where}: {k} {st[k][q, r]} vs {w[k]}"
            assert st["prefix"][q, r, : w["len"]].tolist() == list(w["prefix"]), f"{where}: prefix"
            assert tuple(st["bp"][s, r].tolist()) == w["bp"], f"{where}: bp {st['bp'][s, r].tolist()} vs {w['bp']}"
            if not w["valid"]:
                assert st["hash"][q, r] == 0, f"{where}: hash of an empty slot"
        same = {}
        for j, w in enumerate(want):                                # (the hash is a function of the token string)
            if w["valid"]:
                assert same.setdefault(w["prefix"], st["hash"][q, b * W + j]) == st["hash"][q, b * W + j], f"{tag} clip {b}: two hashes of one token string"
        n_live = sum(1 for w in want if w["valid"] and w["t"] < case.Ts[b])
        total += n_live
        assert st["live"][b] == n_live and st["steps_done"][b] == s + 1, f"{tag} clip {b}: live {st['live'][b]} vs {n_live}, steps_done {st['steps_done'][b]}"
    want_total = before["live_total"].copy()
    want_total[s + 1] += total
    assert np.array_equal(st["live_total"], want_total), f"{tag}: live_total {st['live_total']} vs {want_total}"
    if s > 0:                                                       # the copy the step read, and the records of the steps before
        for k in BEAM + (("lmstate", "lmv") if ref is not None else ()):
            assert np.array_equal(st[k][s & 1], before[k][s & 1]), f"{tag}: {k} of the copy the step reads was written"
        assert np.array_equal(st["bp"][:s], before["bp"][:s]) and untouched(st["bp"][s + 1:]), f"{tag}: bp outside the step's records"


def check_init(case, st, ref):
    """after init + step 0: copy 0 is the start state (the step wrote copy 1 only)"""
    W, R_ = case.W, case.B * case.W
    first = np.arange(R_) % W == 0
    assert np.array_equal(st["valid"][0], first.astype(np.int32)) and not st["t"][0].any() and not st["len"][0].any()
    assert np.array_equal(st["par"][0], np.arange(R_)) and (st["born"][0] == 1).all() and (st["tok"][0] == case.blank).all()
    assert np.array_equal(bits(st["score"][0]), bits(np.where(first, F(0.0), R.NEG))) and not st["hash"][0].any()
    if ref is not None:
        assert (st["lmstate"][0] == TC.lm_state_of(ref, ref.start(True))).all() and not bits(st["lmv"][0]).any()
    assert st["live_total"][0] == case.B


def check_trace(case, st, walks, ref, tag):
    for b, (_, out) in enumerate(walks):
        assert st["ok"][b] == out["ok"], f"{tag} clip {b}: ok"
        assert np.array_equal(st["lens"][b], out["lens"]), f"{tag} clip {b}: lens {st['lens'][b]} vs {out['lens']}"
        for k in ("ids", "start", "end", "dur_idx"):
            assert np.array_equal(st[k][b], out[k]), f"{tag} clip {b}: {k}"
        for k, o in (("out_score", "score"), ("conf", "conf")) + ((("out_lm", "lm_score"),) if ref is not None else ()):
            assert np.array_equal(bits(st[k][b]), bits(out[o])), f"{tag} clip {b}: {o} bits {st[k][b]} vs {out[o]}"
    if ref is None:
        assert untouched(st["out_lm"])


def drive(name, lm_name=None, alpha=0.0, beta=0.0):
    """one whole search of the case through pk_diag_tdt_beam_step, every step checked"""
    case = TC.CASES[name]
    ref = TC.ref_lm(case.V, lm_name) if lm_name else None
    lm = device_lm(case.V, lm_name) if lm_name else None
    walks = [TC.walk_of(name, b, lm_name, alpha, beta) for b in range(case.B)]
    n_steps = max(len(steps) for steps, _ in walks)
    assert 1 <= n_steps <= case.cap
    sc = case.scalars()
    st = capi.tdt_beam_step_state(sc, case.Ts, case.cap, fused=lm is not None)
    carried = BEAM + ("live", "steps_done", "live_total", "bp") + (("lmstate", "lmv") if lm is not None else ())
    for s in range(n_steps):
        tag = f"{name}{' + ' + lm_name if lm_name else ''} step {s}"
        logits = np.full((case.B * case.W, case.V + case.D), np.nan, np.float32)
        live = {}
        for b, (steps, _) in enumerate(walks):
            if s < len(steps):
                for w, h in enumerate(steps[s]["before"]):
                    if h[1] < case.Ts[b]:
                        live[b * case.W + w] = (b, h)
                        logits[b * case.W + w] = case.row(b, h[1], len(h[0]), h[0][-1] if h[0] else -1)
        before = {k: st[k].copy() for k in carried}
        if s == 0:
            before["live_total"][0] = case.B                        # (init's own word)
        capi.diag_tdt_beam_step(sc, st, logits, s, init=s == 0, trace=s == n_steps - 1, lm=lm, alpha=alpha, beta=beta)
        if s == 0:
            check_init(case, st, ref)
        check_expand(case, st, live, ref, alpha, beta, tag)
        check_prune(case, st, before, s, walks, ref, tag)
    check_trace(case, st, walks, ref, f"{name} trace")
    return st, walks


@pytest.mark.parametrize("name", list(TC.CASES))
def test_every_step_of_the_search_equals_the_specification(name):
    st, walks = drive(name)
    assert sum(int(out["lens"].sum()) for _, out in walks) > 0


@pytest.mark.parametrize("name,lm_name,alpha,beta", TC.FUSED)
def test_every_step_of_the_fused_search_equals_the_specification(name, lm_name, alpha, beta):
    st, walks = drive(name, lm_name, alpha, beta)
    assert sum(int(out["lens"].sum()) for _, out in walks) > 0


def test_the_back_trace_alone_after_the_search_ended():
    """trace = 1 on a step no clip is live in: expand and prune return at once, the trace reads the beams where the clips left them"""
    name = "ties-v65"
    st, walks = drive(name)
    case = TC.CASES[name]
    n = max(len(steps) for steps, _ in walks)
    for k in ("ids", "start", "end", "dur_idx", "conf"):
        st[k][...] = 0
    for k in ("lens", "out_score", "ok"):
        st[k].view(np.uint32)[...] = FILL
    before = {k: st[k].copy() for k in BEAM + ("live", "steps_done", "live_total", "bp")}
    capi.diag_tdt_beam_step(case.scalars(), st, np.full((case.B * case.W, case.V + case.D), np.nan, np.float32), n, trace=True)
    for k, v in before.items():
        assert np.array_equal(st[k], v), k
    assert all(untouched(st[k]) for k in capi.TDT_BEAM_STEP_SCRATCH if k in st)
    check_trace(case, st, walks, None, "trace alone")


def test_refusals():
    case = TC.CASES["ties-v65"]
    good = case.scalars()

    def refused(code, word, lm=None, edit=None, step=0, init=True, trace=False, T=None, **kw):
        sc = dict(good, **kw)
        st = capi.tdt_beam_step_state(sc, case.Ts if T is None else T, case.cap, fused=lm is not None)
        if edit:
            edit(st)
        keep = {k: v.copy() for k, v in st.items() if isinstance(v, np.ndarray)}
        with pytest.raises(capi.PkError) as e:
            capi.diag_tdt_beam_step(sc, st, np.zeros((sc["B"] * sc["W"], sc["V"] + sc["D"]), np.float32), step, init=init, trace=trace, lm=lm)
        assert e.value.code == code and word in str(e.value), (kw, str(e.value))
        assert all(st[k].tobytes() == v.tobytes() for k, v in keep.items()), "a refused call wrote"

    for kw, word in ((dict(W=0, N=0), "beam_width"), (dict(W=17), "beam_width"), (dict(K=0), "label_prune"), (dict(K=17), "label_prune"),
                     (dict(Kd=0), "duration_prune"), (dict(Kd=9, D=8, durations=list(range(8))), "duration_prune"), (dict(D=0, Kd=1), "durations"),
                     (dict(D=9, durations=list(range(9))), "durations"), (dict(N=0), "n_best"), (dict(N=case.W + 1), "n_best")):
        refused(-7, word, **kw)
    for kw, word in ((dict(Kd=5, D=1, durations=[1]), "duration_prune <= D"), (dict(V=16, K=16, blank=0), "label_prune <= V - 1"),
                     (dict(V=2, K=2, blank=0), "label_prune <= V - 1"), (dict(blank=-1), "blank"), (dict(blank=case.V), "blank"), (dict(max_tokens=0), "max_tokens")):
        refused(-1, word, **kw)
    refused(-1, "T[b]", T=[1, 0, 6])
    refused(-1, "T[b]", T=[1, -3, 6])
    refused(-1, "step", step=case.cap)
    refused(-1, "step", step=-1)
    refused(-1, "init", step=1)
    # carried state the kernels would index with (init = 0)
    def ok_state(st):
        for k in ("valid", "t", "len", "par", "born", "tok", "live", "steps_done", "bp"):
            st[k][...] = 0
    def then(f):
        return lambda st: (ok_state(st), f(st))
    refused(-1, "len", init=False, edit=then(lambda st: st["len"].__setitem__((1, 2), case.max_tokens + 1)))
    refused(-1, "len", init=False, edit=then(lambda st: st["len"].__setitem__((0, 0), -1)))
    refused(-1, "len", init=False, edit=then(lambda st: st["t"].__setitem__((0, 1), -1)))
    refused(-1, "steps_done", init=False, edit=then(lambda st: st["steps_done"].__setitem__(1, case.cap + 1)))
    refused(-1, "steps_done", init=False, step=2, edit=then(lambda st: (st["live"].__setitem__(0, 1), st["steps_done"].__setitem__(0, 1))))
    refused(-1, "bp", init=False, step=2, edit=then(lambda st: (st["steps_done"].__setitem__(slice(None), 2), st["bp"].__setitem__((1, 4, 0), case.W))))
    lm = device_lm(case.V, "order3_sparse_unk")                     # names the ids 0 .. V - 2: a blank among them is refused
    refused(-1, "blank", lm=lm)
    refused(-1, "lmstate", lm=lm, blank=case.V - 1, init=False, edit=then(lambda st: (st["lmstate"].__setitem__(slice(None), 0), st["lmstate"].__setitem__((1, 0), 1 << 20))))
    refused(-1, "lmstate", lm=lm, blank=case.V - 1, init=False, edit=then(lambda st: (st["lmstate"].__setitem__(slice(None), 0), st["lmstate"].__setitem__((0, 3), -1))))
