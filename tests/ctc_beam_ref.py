"""CTC prefix beam search, its forced alignment and a brute force, in plain Python: the written specification of
DESIGN.md section 5.5 that kernels/ctc_beam.hip is compared against bit for bit.

Prefixes are tuples of token ids (identity = the token string), every value is an fp32 scalar, every add is one fp32 add written
as (prev + lp), exp / log go through oracle.math_v (pinned to the device's dexpf / dlogf).  The candidates of a frame are evaluated as
numpy fp32 vectors -- element-wise, so each element sees exactly the scalar operations of the specification."""
import itertools
import math

import numpy as np

F = np.float32
NEG = F(-np.inf)


def _math(fn, x):
    import oracle
    return oracle.math_v(fn, np.ascontiguousarray(x, np.float32))


def lae(a, b):
    """log(exp a + exp b): m + log(1 + exp(n - m)), m = max, n = min; m where n == -inf.  Element-wise on fp32 arrays."""
    a = np.atleast_1d(np.asarray(a, np.float32))
    b = np.atleast_1d(np.asarray(b, np.float32))
    m, n = np.maximum(a, b), np.minimum(a, b)
    out = m.copy()
    sel = n > NEG
    if sel.any():
        d = (n[sel] - m[sel]).astype(np.float32)
        s = (F(1.0) + _math("exp", d)).astype(np.float32)
        out[sel] = (m[sel] + _math("log", s)).astype(np.float32)
    return out


def topk_tokens(row, blank, K):
    """The K non-blank tokens with the largest log-prob, ties: lower id first -> (ids, values)."""
    ids = np.array([i for i in range(len(row)) if i != blank], np.int64)
    vals = np.asarray(row, np.float32)[ids]
    order = np.lexsort((ids, -(vals + F(0.0))))[:K]                 # (+ 0: -0.0 and 0.0 are one value)
    return ids[order], vals[order]


def beam_search(lp, blank, beam_width=8, token_prune=16, n_best=1, trace=None):
    """lp [T][V] fp32 -> list of (ids tuple, score fp32), best first, at most n_best entries (fewer when the beam holds fewer).
    trace (optional list): receives the beam's prefix tuples after every frame."""
    lp = np.ascontiguousarray(lp, np.float32)
    T, V = lp.shape
    W, K = int(beam_width), max(1, min(int(token_prune), V - 1))
    beam = [dict(p=(), pb=F(0.0), pnb=NEG, tot=F(0.0))]
    with np.errstate(all="ignore"):
        for t in range(T):
            cid, cval = topk_tokens(lp[t], blank, K)
            kof = {int(c): k for k, c in enumerate(cid)}
            lpb = lp[t, blank]
            rank = {e["p"]: i for i, e in enumerate(beam)}
            nb = len(beam)
            npb = np.full(nb, NEG, np.float32); rep = np.full(nb, NEG, np.float32); mrg = np.full(nb, NEG, np.float32)
            for i, e in enumerate(beam):
                npb[i] = e["tot"] + lpb                             # blank keeps p
                if e["p"]:
                    last = e["p"][-1]
                    k = kof.get(last)
                    if k is not None:
                        rep[i] = e["pnb"] + cval[k]                 # c == l keeps p via p_nb
                        j = rank.get(e["p"][:-1])                   # an extension that IS this beam prefix: its term lands here
                        if j is not None:
                            par = beam[j]
                            src = par["pb"] if (par["p"] and par["p"][-1] == last) else par["tot"]
                            mrg[i] = src + cval[k]
            npnb = lae(rep, mrg)
            sc = lae(npb, npnb)
            cands = []
            for i, e in enumerate(beam):
                if sc[i] > NEG:
                    cands.append((-float(sc[i]), i, 0, 0, e["p"], npb[i], npnb[i], sc[i]))
                last = e["p"][-1] if e["p"] else -1
                for k in range(K):
                    c = int(cid[k])
                    q = e["p"] + (c,)
                    if q in rank:
                        continue                                    # merged into q's own entry above
                    v = F((e["pb"] if c == last else e["tot"]) + cval[k])
                    if v > NEG:
                        cands.append((-float(v), i, 1, c, q, NEG, v, v))
            cands.sort(key=lambda x: x[:4])                         # score, then parent rank, stay before extend, token id
            beam = [dict(p=c[4], pb=F(c[5]), pnb=F(c[6]), tot=F(c[7])) for c in cands[:W]]
            if trace is not None:
                trace.append([e["p"] for e in beam])
    return [(e["p"], e["tot"]) for e in beam[:n_best]]


def viterbi_align(lp, ids, blank):
    """Forced alignment of `ids` on the 2 L + 1 state lattice, max-plus in fp32 (one add per cell).  Predecessor ties: stay, previous
    state, skip; end state: the last blank unless the last token's state is strictly better.
    -> dict(start, end, conf, score, path) or None when the string cannot be aligned."""
    lp = np.ascontiguousarray(lp, np.float32)
    T = lp.shape[0]
    L = len(ids)
    S = 2 * L + 1
    sym = np.full(S, blank, np.int64)
    sym[1::2] = np.asarray(ids, np.int64)
    can_skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        can_skip[s] = sym[s] != sym[s - 2]
    a = np.full(S, NEG, np.float32)
    a[0] = lp[0, blank]
    if L:
        a[1] = lp[0, sym[1]]
    bp = np.zeros((T, S), np.uint8)
    with np.errstate(all="ignore"):
        for t in range(1, T):
            best = a.copy()
            ptr = np.zeros(S, np.uint8)
            prev = np.full(S, NEG, np.float32); prev[1:] = a[:-1]
            skip = np.full(S, NEG, np.float32); skip[2:] = a[:-2]; skip[~can_skip] = NEG
            m = prev > best
            best[m] = prev[m]; ptr[m] = 1
            m = skip > best
            best[m] = skip[m]; ptr[m] = 2
            a = (best + lp[t, sym]).astype(np.float32)
            bp[t] = ptr
    s = S - 1
    if L and a[S - 2] > a[S - 1]:
        s = S - 2
    if not a[s] > NEG:
        return None
    score = a[s]
    path = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(bp[t, s])
    start = np.zeros(L, np.int32); end = np.zeros(L, np.int32)
    for k in range(L):
        fr = np.nonzero(path == 2 * k + 1)[0]
        start[k], end[k] = fr[0], fr[-1]
    conf = _math("exp", lp[start, np.asarray(ids, np.int64)]) if L else np.zeros(0, np.float32)
    return dict(start=start, end=end, conf=conf, score=score, path=path, sym=sym)


def search_batch(lps, blank, beam_width, token_prune, n_best, timestamps=True):
    """The arrays pk_ctc_beam_search returns for a list of [T_b][V] log-prob matrices: ids / start / end / conf [B][N][Tmax],
    lens / score [B][N]; unused hypothesis slots: lens 0, score -inf; unused token slots 0."""
    B, N = len(lps), n_best
    Tmax = max(x.shape[0] for x in lps)
    ids = np.zeros((B, N, Tmax), np.int32); st = np.zeros((B, N, Tmax), np.int32); en = np.zeros((B, N, Tmax), np.int32)
    cf = np.zeros((B, N, Tmax), np.float32); lens = np.zeros((B, N), np.int32); score = np.full((B, N), NEG, np.float32)
    for b, lp in enumerate(lps):
        for j, (p, s) in enumerate(beam_search(lp, blank, beam_width, token_prune, n_best)):
            L = len(p)
            ids[b, j, :L] = p; lens[b, j] = L; score[b, j] = s
            if timestamps:
                al = viterbi_align(lp, p, blank)
                assert al is not None, "a hypothesis of the search cannot be aligned"
                st[b, j, :L] = al["start"]; en[b, j, :L] = al["end"]; cf[b, j, :L] = al["conf"]
    return dict(ids=ids, lens=lens, score=score, start=st, end=en, conf=cf)


def log_softmax32(x):
    """fp32 log-softmax rows (test inputs only: any fp32 matrix is a valid input of the search)."""
    x = np.asarray(x, np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def reentry_events(trace):
    """Frames t at which a beam prefix q receives the merged extension of its parent string (q[:-1] in the beam at t - 1, q too) although
    the parent string was OUT of the beam at some frame since q first appeared: the route a parent-pointer trie alone would miss."""
    first, events = {}, []
    for t, beam in enumerate(trace):
        for q in beam:
            first.setdefault(q, t)
    for t in range(1, len(trace)):
        prev = set(trace[t - 1])
        for q in trace[t]:
            if len(q) >= 1 and q in prev and q[:-1] in prev:
                if any(q[:-1] not in trace[u] for u in range(first[q], t - 1)):
                    events.append((t, q))
    return events


def find_reentry_case(V=4, T=12, W=3, K=2, tries=4000, seed=0):
    """A deterministic input on which a prefix leaves the beam and re-enters while its extension stayed, and the re-entered prefix is then
    extended into that extension at a frame where the token is among the candidates -> (lp, events)."""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        lp = log_softmax32(rng.normal(size=(T, V)) * 1.5)
        trace = []
        beam_search(lp, V - 1, W, K, W, trace=trace)
        ev = []
        for t, q in reentry_events(trace):
            cid, _ = topk_tokens(lp[t], V - 1, K)
            if q[-1] in cid:
                ev.append((t, q))
        if ev:
            return lp, ev
    return None, []


def brute_force(lp, blank):
    """float64: every one of the V^T paths, collapsed -> {ids tuple: log of the summed path probability}."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = 0.0
        out, prev = [], -1
        for t, c in enumerate(path):
            s += lp[t, c]
            if c != prev and c != blank:
                out.append(c)
            prev = c
        acc.setdefault(tuple(out), []).append(s)
    res = {}
    for k, v in acc.items():
        m = max(v)
        res[k] = m + math.log(math.fsum(math.exp(x - m) for x in v)) if m > -math.inf else -math.inf
    return res
