"""CTC forced alignment of a given token string, in plain Python: the written specification of DESIGN.md section 5.5.1 that
kernels/ctc_align.hip is compared against bit for bit.

align() IS ctc_beam_ref.viterbi_align (the rule the beam search's timestamps already follow).  forward_total() is the forward algorithm on
the same lattice with ctc_beam_ref.lae: per cell lae(lae(stay, prev), skip) + lp, a forbidden skip contributing -inf.
lattice_banded() is both passes restricted to the band of cells that are reachable from the start AND can reach the end: the same
operations on fewer cells.  tests/test_ctc_align_ref.py shows that it changes nothing; the GPU tests use it for the longest string only
(L = 16383 at T = L + 40: the band is 81 states wide, the full lattice's back-pointers alone would take 538 MB)."""
import numpy as np

import ctc_beam_ref as B

F = np.float32
NEG = F(-np.inf)


def align(lp, ids, blank):
    """-> dict(start, end, conf, score, ok): ok = 0 (score -inf, empty-handed arrays of zeros) when the string cannot be aligned."""
    r = B.viterbi_align(lp, ids, blank)
    L = len(ids)
    if r is None:
        return dict(start=np.zeros(L, np.int32), end=np.zeros(L, np.int32), conf=np.zeros(L, np.float32), score=NEG, ok=0)
    return dict(start=r["start"], end=r["end"], conf=np.asarray(r["conf"], np.float32), score=F(r["score"]), ok=1)


def _lattice_of(ids, blank):
    L = len(ids)
    S = 2 * L + 1
    sym = np.full(S, blank, np.int64)
    sym[1::2] = np.asarray(ids, np.int64)
    can_skip = np.zeros(S, bool)
    can_skip[3::2] = sym[3::2] != sym[1:-2:2]
    return L, S, sym, can_skip


def forward_total(lp, ids, blank):
    """The CTC log-likelihood of `ids`: fp32, lae(lae(stay, prev), skip) + lp per cell; at the end lae(alpha[S-1], alpha[S-2]), alpha[0] for L = 0."""
    lp = np.ascontiguousarray(lp, np.float32)
    T = lp.shape[0]
    L, S, sym, can_skip = _lattice_of(ids, blank)
    a = np.full(S, NEG, np.float32)
    a[0] = lp[0, blank]
    if L:
        a[1] = lp[0, sym[1]]
    with np.errstate(all="ignore"):
        for t in range(1, T):
            prev = np.full(S, NEG, np.float32); prev[1:] = a[:-1]
            skip = np.full(S, NEG, np.float32); skip[2:] = a[:-2]; skip[~can_skip] = NEG
            a = (B.lae(B.lae(a, prev), skip) + lp[t, sym]).astype(np.float32)
    return F(B.lae(a[S - 1], a[S - 2])[0]) if L else F(a[0])


def band(t, T, S):
    """First and last state of frame t that is reachable from the start and can reach the end (may be empty: lo > hi)."""
    return max(0, S - 1 - (2 * (T - 1 - t) + 1)), min(S - 1, 2 * t + 1)


def lattice_banded(lp, ids, blank, want_total=True):
    """align() and forward_total() on the band only -> align()'s dict (+ total).  Cells outside the band are never computed or stored."""
    lp = np.ascontiguousarray(lp, np.float32)
    T = lp.shape[0]
    L, S, sym, can_skip = _lattice_of(ids, blank)
    a = np.full(S + 2, NEG, np.float32)                              # a[s + 2] = alpha[s]; two -inf cells in front serve s - 1, s - 2 < 0
    f = np.full(S + 2, NEG, np.float32)
    a[2] = f[2] = lp[0, blank]
    if L:
        a[3] = f[3] = lp[0, sym[1]]
    rows = [None] * T                                               # (lo, back-pointers of [lo, hi]) per frame
    with np.errstate(all="ignore"):
        for t in range(1, T):
            lo, hi = band(t, T, S)
            if lo > hi:
                continue
            sl = slice(lo + 2, hi + 3)
            stay, prev, skp = a[sl].copy(), a[lo + 1:hi + 2].copy(), a[lo:hi + 1].copy()
            ok_skip = can_skip[lo:hi + 1]
            skp[~ok_skip] = NEG
            best, ptr = stay.copy(), np.zeros(hi - lo + 1, np.uint8)
            m = prev > best
            best[m] = prev[m]; ptr[m] = 1
            m = skp > best
            best[m] = skp[m]; ptr[m] = 2
            e = lp[t, sym[lo:hi + 1]]
            if want_total:
                fs = f[lo:hi + 1].copy()
                fs[~ok_skip] = NEG
                f[sl] = (B.lae(B.lae(f[sl], f[lo + 1:hi + 2]), fs) + e).astype(np.float32)
            a[sl] = (best + e).astype(np.float32)
            rows[t] = (lo, ptr)
    al, fl = a[2:], f[2:]
    s = S - 1
    if L and al[S - 2] > al[S - 1]:
        s = S - 2
    out = dict(start=np.zeros(L, np.int32), end=np.zeros(L, np.int32), conf=np.zeros(L, np.float32), score=NEG, ok=0)
    if want_total:
        out["total"] = F(B.lae(fl[S - 1], fl[S - 2])[0]) if L else F(fl[0])
    if not al[s] > NEG:
        return out
    out["score"], out["ok"] = F(al[s]), 1
    lastk = -1
    for t in range(T - 1, -1, -1):
        if s & 1:
            k = s >> 1
            if k != lastk:
                out["end"][k] = t
                lastk = k
            out["start"][k] = t
        if t > 0:
            lo, ptr = rows[t]
            s -= int(ptr[s - lo])
    if L:
        out["conf"] = np.asarray(B._math("exp", lp[out["start"], np.asarray(ids, np.int64)]), np.float32)
    return out


def full(lp, ids, blank):
    """align() + total on the full lattice."""
    r = align(lp, ids, blank)
    r["total"] = forward_total(lp, ids, blank)
    return r


def make_lp(family, T, V, rng):
    """The input families of the alignment tests, blank = V - 1: "ties" log_softmax32(round(4 N(0,1)) / 4); "holes" the same with about
    10 % of the entries -inf; "peaky" one dominant column per frame."""
    x = np.round(4.0 * rng.normal(size=(T, V))) / 4.0
    if family == "peaky":
        x = rng.normal(size=(T, V))
        x[np.arange(T), rng.integers(0, V, size=T)] += 9.0
    lp = B.log_softmax32(x)
    if family == "holes":
        lp[rng.random(size=(T, V)) < 0.1] = NEG
    return lp
