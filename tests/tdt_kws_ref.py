"""TDT keyword spotting, in plain numpy fp32: the written specification of DESIGN.md section 5.5.8 that kernels/tdt_kws.hip is compared
against bit for bit.

One (clip, keyword) pair: T >= 1 frames, a keyword ids[L] (1 <= L <= 64, no blank), durations dur[D] (1 <= D <= 8, every one in [0, 8]) and
the lattice of section 5.5.2 (tests/tdt_align_ref.py) with the prediction net teacher-forced over [blank, ids...] from its initial state,
    lab[T][L]      lab[t][u] the label log-prob of ids[u]
    blk[T][L+1]    the blank log-prob
    dl[T][L+1][D]  the duration log-probs
    top[T][L+1]    the largest token-head log-prob of the row
of which only the columns u = 0 .. L-1 are read (the match ends on the last label arc; column L is packed, as pk_tdt_align packs it, and
ignored).  Every row needs a finite top and a finite largest duration log-prob, as true log-softmax rows have.

normalise(): every value relative to the greedy decision of its cell, nlab = fl(lab - top), nblk = fl(blk - top), ndl[i] = fl(dl[i] - dmax),
dmax = max_i dl[i] (exact).  Arc i out of (t, u) with head value x costs w = fl(nx + ndl[i]) <= 0, +0.0 exactly where the arc is the greedy
decision of the cell; no -0.0 arises (x - x = +0.0 in round-to-nearest, and +0.0 + +0.0 = +0.0): asserted.

walk(): max-plus in pull form, every state carries (a, b) = (score, frame at which the first token was emitted).  Column 0 is ENTER:
a[t][0] = +0.0, b[t][0] = t at every frame, no blank arcs.  For 1 <= u <= L-1 the candidates come in the order of 5.5.2: blank arcs
i = 0 .. D-1 from (t - max(dur[i], 1), u), then label arcs i = 0 .. D-1 from (t - dur[i], u - 1); a candidate is fl(a[src] + w); strict >
keeps the earlier one; b is copied from the chosen source; a negative source frame does not exist; a cell no candidate raises is -inf with
b = 0.  EXIT per emission frame t of the last token: v_i = fl(a[t][L-1] + w(lab[t][L-1], i)), i = 0 .. D-1 (the target frame may be >= T),
E[t] = max with strict > from -inf, Bs[t] = b[t][L-1], Ee[t] = token_end(t, dur[i*], T) (0 where E[t] is -inf).

pick(): the greedy non-overlapping peak picking of 5.5.4 on spans [Bs[t], Ee[t]]."""
import numpy as np

F = np.float32
NEG = F(-np.inf)
MAX_L = 64
MAX_HITS = 16
MAX_DUR = 8


def token_end(t, dur, T):
    return min(t + max(int(dur), 1) - 1, T - 1)


def normalise(lab, blk, dl, top):
    """-> (nlab [T][L], nblk [T][L+1], ndl [T][L+1][D]) fp32; asserts that no used value is > 0, NaN or -0.0."""
    blk = np.ascontiguousarray(blk, np.float32)
    T, L = blk.shape[0], blk.shape[1] - 1
    lab = np.ascontiguousarray(lab, np.float32).reshape(T, L)
    dl = np.ascontiguousarray(dl, np.float32).reshape(T, L + 1, -1)
    top = np.ascontiguousarray(top, np.float32).reshape(T, L + 1)
    dmax = dl.max(axis=2)
    assert np.all(np.isfinite(top[:, :L])) and np.all(np.isfinite(dmax[:, :L])), "every row needs a finite top and a finite duration maximum"
    with np.errstate(all="ignore"):
        nlab = (lab - top[:, :L]).astype(np.float32)
        nblk = (blk - top).astype(np.float32)
        ndl = (dl - dmax[:, :, None]).astype(np.float32)
    for x in (nlab, nblk[:, :L], ndl[:, :L]):
        assert not np.any(x > 0) and not np.any(np.isnan(x)), "top / dmax must bound the row"
        assert not np.any(np.signbit(x) & (x == 0)), "-0.0 cannot arise"
    return nlab, nblk, ndl


def _w(nx, ndl_i):
    w = F(nx + ndl_i)
    assert not (w == 0 and np.signbit(w))
    return w


def walk(lab, blk, dl, top, dur):
    """-> E[T] fp32, Bs[T] int32, Ee[T] int32, and the number of cells (EXIT folds included) in which two candidates tied at the maximum."""
    nlab, nblk, ndl = normalise(lab, blk, dl, top)
    T, L = nblk.shape[0], nblk.shape[1] - 1
    D = len(dur)
    assert T >= 1 and 1 <= L <= MAX_L and 1 <= D <= 8 and ndl.shape[2] == D and all(0 <= int(d) <= MAX_DUR for d in dur)
    a = np.full((T, L), NEG, np.float32)
    b = np.zeros((T, L), np.int32)
    E = np.full(T, NEG, np.float32); Bs = np.zeros(T, np.int32); Ee = np.zeros(T, np.int32)
    ties = 0
    with np.errstate(all="ignore"):
        for t in range(T):
            a[t, 0], b[t, 0] = F(0.0), t
            for u in range(1, L):
                best, org, cands = NEG, 0, []
                for i in range(D):
                    ts = t - max(int(dur[i]), 1)
                    if ts >= 0:
                        c = F(a[ts, u] + _w(nblk[ts, u], ndl[ts, u, i]))
                        cands.append(c)
                        if c > best:
                            best, org = c, b[ts, u]
                for i in range(D):
                    ts = t - int(dur[i])
                    if ts >= 0:
                        c = F(a[ts, u - 1] + _w(nlab[ts, u - 1], ndl[ts, u - 1, i]))
                        cands.append(c)
                        if c > best:
                            best, org = c, b[ts, u - 1]
                a[t, u], b[t, u] = best, org
                ties += best > NEG and sum(1 for c in cands if c == best) > 1
            best, arg, cands = NEG, -1, []
            for i in range(D):
                c = F(a[t, L - 1] + _w(nlab[t, L - 1], ndl[t, L - 1, i]))
                cands.append(c)
                if c > best:
                    best, arg = c, i
            E[t], Bs[t] = best, b[t, L - 1]
            Ee[t] = token_end(t, dur[arg], T) if arg >= 0 else 0
            ties += best > NEG and sum(1 for c in cands if c == best) > 1
    return E, Bs, Ee, int(ties)


def pick(E, Bs, Ee, max_hits=1, min_score=NEG):
    """Greedy non-overlapping peak picking on spans [Bs[t], Ee[t]] -> (n_hits, start[max_hits], end[max_hits], score[max_hits]); unused
    slots 0 / 0 / -inf.  The rule of ctc_kws_ref.pick, whose spans end at t itself."""
    assert 1 <= max_hits <= MAX_HITS and not min_score > 0
    E = np.asarray(E, np.float32); Bs = np.asarray(Bs, np.int32); Ee = np.asarray(Ee, np.int32)
    alive = np.ones(len(E), bool)
    st = np.zeros(max_hits, np.int32); en = np.zeros(max_hits, np.int32); sc = np.full(max_hits, NEG, np.float32)
    n = 0
    while n < max_hits:
        cand = alive & (E > NEG) & (E >= F(min_score))
        if not cand.any():
            break
        t = int(np.nonzero(cand & (E == E[cand].max()))[0][0])      # the largest score; on a tie the lowest frame
        st[n], en[n], sc[n] = Bs[t], Ee[t], E[t]
        n += 1
        alive &= ~((Bs <= Ee[t]) & (Bs[t] <= Ee))                   # [Bs[t'], Ee[t']] meets [Bs[t], Ee[t]]
    return n, st, en, sc


def spot(lab, blk, dl, top, dur, max_hits=1, min_score=NEG):
    """The hits of one keyword in one clip -> dict(n_hits, start, end, score)."""
    E, Bs, Ee, _ = walk(lab, blk, dl, top, dur)
    n, st, en, sc = pick(E, Bs, Ee, max_hits, min_score)
    return dict(n_hits=n, start=st, end=en, score=sc)


def brute_force(lab, blk, dl, top, dur):
    """Every path of every (entry frame s, emission frame e of the last token) by enumeration -> best[s][e], the maximum of the left-to-right
    fp32 sums of the paths' arc costs, from +0.0 (-inf: no path).  For small lattices only."""
    nlab, nblk, ndl = normalise(lab, blk, dl, top)
    T, L = nblk.shape[0], nblk.shape[1] - 1
    D = len(dur)
    best = np.full((T, T), NEG, np.float32)

    def go(s, t, u, acc):
        with np.errstate(all="ignore"):
            if u == L - 1:                                          # the last token may be emitted here, by any duration
                for i in range(D):
                    v = F(acc + _w(nlab[t, u], ndl[t, u, i]))
                    if v > best[s, t]:
                        best[s, t] = v
            if u >= 1:                                              # (column 0 has no blank arcs)
                for i in range(D):
                    tn = t + max(int(dur[i]), 1)
                    if tn < T:
                        go(s, tn, u, F(acc + _w(nblk[t, u], ndl[t, u, i])))
            if u < L - 1:
                for i in range(D):
                    tn = t + int(dur[i])
                    if tn < T:
                        go(s, tn, u + 1, F(acc + _w(nlab[t, u], ndl[t, u, i])))

    for s in range(T):
        go(s, s, 0, F(0.0))
    return best


def make_lattice(family, T, L, D, rng):
    """The input families of the spotting tests -> (lab, blk, dl, top).  "ties": every value one of a few exactly representable numbers, so
    sums are exact and paths tie; "holes": the same with about 10 % of lab / blk / dl at -inf (every cell keeps a finite duration).  top is
    the maximum of the cell's lab and blk, raised to -0.25 in about a third of the cells (some other token leads there)."""
    vals = np.asarray([-0.25, -0.5, -1.0, -1.5, -2.0, -3.0], np.float32)
    lab, blk, dl = (vals[rng.integers(0, len(vals), size=sh)] for sh in ((T, L), (T, L + 1), (T, L + 1, D)))
    top = blk.copy()
    top[:, :L] = np.maximum(top[:, :L], lab)
    top[rng.random(size=top.shape) < 0.33] = F(-0.25)
    if family == "holes":
        for x in (lab, blk, dl):
            x[rng.random(size=x.shape) < 0.1] = NEG
        dl[..., 0][np.all(dl == NEG, axis=-1)] = F(-0.5)
    else:
        assert family == "ties"
    return lab, blk, dl, top


def plant(lab, blk, dl, top, dur, t0, steps):
    """Makes the keyword's path the greedy decision of every cell it visits (in place): from (t0, 0), steps[u] = (blank duration indices
    taken in column u before the token -- none allowed in column 0 --, the token's duration index).  -> (start, end) of the planted hit."""
    T, L = blk.shape[0], blk.shape[1] - 1
    t, end = t0, t0
    for u, (blanks, li) in enumerate(steps):
        assert u > 0 or not blanks
        for bi in blanks:
            blk[t, u] = top[t, u]; dl[t, u, bi] = dl[t, u].max()
            t += max(int(dur[bi]), 1)
        lab[t, u] = top[t, u]; dl[t, u, li] = dl[t, u].max()
        if u == L - 1:
            # the exit takes the first duration at the maximum: make li the only one
            dl[t, u, :] = np.where(np.arange(len(dur)) == li, dl[t, u, li], np.minimum(dl[t, u], dl[t, u, li] - F(1.0)))
            end = token_end(t, dur[li], T)
        else:
            t += int(dur[li])
        assert t < T
    return t0, end
