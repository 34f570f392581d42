"""CTC keyword spotting, in plain Python: the written specification of DESIGN.md section 5.5.4 that kernels/ctc_kws.hip is compared
against bit for bit.

walk() is max-plus on the 2 L - 1 state lattice of a keyword (no leading or trailing blank) with a FREE start and a FREE end: state 0 may
be entered at any frame with value +0.0, and the value of the last state is read at every frame.  The cost of a symbol at a frame is its
log-prob minus the frame's maximum, so a score is the log-ratio of the keyword's best path over a span to the greedy path over the same
span: <= 0, and exactly +0.0 where the greedy path over the span IS the keyword.  Every state carries the frame at which its path entered,
so one row of (a, b) is the whole state: no back-pointers.  pick() is greedy non-overlapping peak picking on the per-end-frame scores.
brute_force() is the same answer from a forced alignment (the arcs and tie order of ctc_align_ref / ctc_beam_ref.viterbi_align) per span."""
import numpy as np

import ctc_beam_ref as B

F = np.float32
NEG = F(-np.inf)
MAX_L = 64
MAX_HITS = 16


def _lattice_of(ids, blank):
    L = len(ids)
    assert 1 <= L <= MAX_L and all(int(v) != blank for v in ids), "1 <= L <= 64 and no blank inside a keyword"
    S = 2 * L - 1
    sym = np.full(S, blank, np.int64)
    sym[0::2] = np.asarray(ids, np.int64)
    can_skip = np.zeros(S, bool)
    can_skip[2::2] = sym[2::2] != sym[0:-2:2]
    return L, S, sym, can_skip


def costs(lp):
    """c[t][v] = fl(lp[t][v] - g[t]), g[t] = max_v lp[t][v] (exact).  Every row must have a finite maximum."""
    lp = np.ascontiguousarray(lp, np.float32)
    g = lp.max(axis=1)
    assert np.all(np.isfinite(g)), "every row of lp needs a finite maximum (true log-softmax rows have one)"
    with np.errstate(all="ignore"):
        return (lp - g[:, None]).astype(np.float32)


def walk(lp, ids, blank):
    """-> E[T] fp32, Bs[T] int32: the best score of a match that ends at frame t and the frame at which that match starts."""
    c = costs(lp)
    T = c.shape[0]
    L, S, sym, can_skip = _lattice_of(ids, blank)
    a = np.full(S, NEG, np.float32)
    b = np.zeros(S, np.int32)
    E = np.full(T, NEG, np.float32)
    Bs = np.zeros(T, np.int32)
    with np.errstate(all="ignore"):
        for t in range(T):
            best, org = a.copy(), b.copy()                         # stay
            prev = np.full(S, NEG, np.float32); prev[1:] = a[:-1]
            pb = np.zeros(S, np.int32); pb[1:] = b[:-1]
            m = prev > best
            best[m] = prev[m]; org[m] = pb[m]
            skip = np.full(S, NEG, np.float32); skip[2:] = a[:-2]; skip[~can_skip] = NEG
            sb = np.zeros(S, np.int32); sb[2:] = b[:-2]
            m = skip > best
            best[m] = skip[m]; org[m] = sb[m]
            if F(0.0) > best[0]:                                   # enter
                best[0] = F(0.0); org[0] = t
            a = (best + c[t, sym]).astype(np.float32)
            b = org
            E[t], Bs[t] = a[S - 1], b[S - 1]
    return E, Bs


def pick(E, Bs, max_hits=1, min_score=NEG):
    """Greedy non-overlapping peak picking -> (n_hits, start[max_hits], end[max_hits], score[max_hits]); unused slots 0 / 0 / -inf."""
    assert 1 <= max_hits <= MAX_HITS and not min_score > 0
    T = len(E)
    alive = np.ones(T, bool)
    st = np.zeros(max_hits, np.int32); en = np.zeros(max_hits, np.int32); sc = np.full(max_hits, NEG, np.float32)
    n = 0
    fr = np.arange(T)
    while n < max_hits:
        cand = alive & (E > NEG) & (E >= F(min_score))
        if not cand.any():
            break
        t = int(np.nonzero(cand & (E == E[cand].max()))[0][0])      # the largest score; on a tie the lowest frame
        st[n], en[n], sc[n] = Bs[t], t, E[t]
        n += 1
        alive &= ~((Bs <= t) & (Bs[t] <= fr))                       # [Bs[t'], t'] meets [Bs[t], t]
    return n, st, en, sc


def spot(lp, ids, blank, max_hits=1, min_score=NEG):
    """The hits of one keyword in one clip -> dict(n_hits, start, end, score)."""
    E, Bs = walk(lp, ids, blank)
    n, st, en, sc = pick(E, Bs, max_hits, min_score)
    return dict(n_hits=n, start=st, end=en, score=sc)


def spot_batch(lps, keywords, blank, max_hits=1, min_score=NEG):
    """The arrays pk_ctc_kws returns for a list of [T_b][V] matrices: n_hits [B][n_kw], start / end / score [B][n_kw][max_hits]."""
    Bn, K = len(lps), len(keywords)
    nh = np.zeros((Bn, K), np.int32); st = np.zeros((Bn, K, max_hits), np.int32); en = np.zeros((Bn, K, max_hits), np.int32)
    sc = np.full((Bn, K, max_hits), NEG, np.float32)
    for i, lp in enumerate(lps):
        for k, kw in enumerate(keywords):
            r = spot(lp, kw, blank, max_hits, min_score)
            nh[i, k], st[i, k], en[i, k], sc[i, k] = r["n_hits"], r["start"], r["end"], r["score"]
    return dict(n_hits=nh, start=st, end=en, score=sc)


def span_score(c, sym, can_skip, s0, e0):
    """Max-plus forced alignment of the 2 L - 1 state lattice on the frames [s0, e0] of the costs c: the path starts in state 0 at s0 and
    ends in state S - 1 at e0.  Arcs and tie order as ctc_beam_ref.viterbi_align; -inf when the span is too short."""
    S = len(sym)
    a = np.full(S, NEG, np.float32)
    with np.errstate(all="ignore"):
        a[0] = F(F(0.0) + c[s0, sym[0]])
        for t in range(s0 + 1, e0 + 1):
            best = a.copy()
            prev = np.full(S, NEG, np.float32); prev[1:] = a[:-1]
            skip = np.full(S, NEG, np.float32); skip[2:] = a[:-2]; skip[~can_skip] = NEG
            m = prev > best
            best[m] = prev[m]
            m = skip > best
            best[m] = skip[m]
            a = (best + c[t, sym]).astype(np.float32)
    return a[S - 1]


def brute_force(lp, ids, blank):
    """Per end frame e: the maximum over all start frames s <= e of span_score, and the start frames that reach it."""
    c = costs(lp)
    T = c.shape[0]
    L, S, sym, can_skip = _lattice_of(ids, blank)
    E = np.full(T, NEG, np.float32)
    starts = [[] for _ in range(T)]
    for e in range(T):
        sc = np.asarray([span_score(c, sym, can_skip, s, e) for s in range(e + 1)], np.float32)
        E[e] = sc.max()
        if E[e] > NEG:
            starts[e] = [s for s in range(e + 1) if sc[s] == E[e]]
    return E, starts


def plant(lp, path_syms, t0):
    """Makes path_syms the best symbols of the frames t0, t0 + 1, ... of lp (in place): the row's maximum moves onto the symbol."""
    for i, v in enumerate(path_syms):
        row = lp[t0 + i]
        j = int(np.argmax(row))
        row[j], row[v] = row[v], row[j]
    return lp
