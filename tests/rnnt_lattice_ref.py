"""Forced alignment and the forward-algorithm total of a given token string under the plain RNN-T head, in numpy fp32: the written
specification of DESIGN.md section 5.5.12 that kernels/rnnt_lattice.hip is compared against bit for bit.

One utterance: T >= 1 frames, U >= 0 tokens ids[U] (no blank among them) and the lattice scores -- the canonical log-softmax of the joint's
single [V] head at frame t with the prediction net teacher-forced over [blank, ids[:u]]:
    lab[T][U]      lab[t][u] the log-prob of ids[u]
    blk[T][U+1]    the blank's log-prob
Arcs out of cell (t, u), as the greedy loop moves (src/rnnt.cpp; max_symbols_per_step is not part of the lattice):
    blank: to (t + 1, u)             weight blk[t][u]
    label: to (t, u + 1), u < U      weight lab[t][u]
The one arc to the terminal END is the blank out of (T - 1, U).  Every cell has two predecessors, both on the anti-diagonal before its own.
Both walks are in pull form: alpha[0][0] = +0.0, every other cell starts at -inf and takes its candidates in the order blank from (t - 1, u),
then label from (t, u - 1); a candidate is fl(alpha[src] + x), one fp32 add; a candidate whose source lies outside the lattice does not exist
(a -inf in its place gives the same bits under either fold).
    alignment  max-plus: a strict > keeps the earlier candidate; the back-pointer of a cell is one bit, 1 = the label arc.
               score = fl(alpha[T-1][U] + blk[T-1][U]), ok = 0 where that is -inf.  Token k emitted at frame t: start[k] = end[k] = t,
               conf[k] = dexpf(lab[t][k]).
    total      log-sum: a left fold from -inf with ctc_beam_ref.lae (DESIGN.md 5.5.3's two-operand log-add); the same END arc; ok = total > -inf.
The cells of an anti-diagonal depend on the one before it only, so both walks fold a whole diagonal as numpy vectors: element-wise, every cell
sees exactly the scalar operations above."""
import numpy as np

from ctc_beam_ref import lae
from tdt_align_ref import _dexp

F = np.float32
NEG = F(-np.inf)


def _shapes(lab, blk):
    blk = np.ascontiguousarray(blk, np.float32)
    T, U = blk.shape[0], blk.shape[1] - 1
    assert T >= 1 and U >= 0
    return np.ascontiguousarray(lab, np.float32).reshape(T, U), blk, T, U


def _walk(lab, blk, log_sum):
    """-> (alpha [T][U+1], label bits [T][U+1], END value)."""
    lab, blk, T, U = _shapes(lab, blk)
    alpha = np.full((T, U + 1), NEG, np.float32)
    bit = np.zeros((T, U + 1), np.uint8)
    alpha[0, 0] = F(0.0)
    with np.errstate(all="ignore"):
        for d in range(1, T + U):
            u = np.arange(max(0, d - (T - 1)), min(d, U) + 1)
            t = d - u
            tp, up = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
            cb = np.where(t >= 1, alpha[tp, u] + blk[tp, u], NEG).astype(np.float32)
            cl = np.where(u >= 1, alpha[t, up] + lab[t, up], NEG).astype(np.float32) if U else np.full(len(u), NEG, np.float32)
            if log_sum:
                alpha[t, u] = lae(lae(np.full(len(u), NEG, np.float32), cb), cl)
            else:
                take = cl > cb
                alpha[t, u], bit[t, u] = np.where(take, cl, cb), take
        end = F(alpha[T - 1, U] + blk[T - 1, U])
    return alpha, bit, end


def align(lab, blk):
    """-> dict(start, end, conf [U], score, ok); ok = 0 (score -inf, arrays of zeros) when no path reaches END."""
    lab, blk, T, U = _shapes(lab, blk)
    _, bit, end = _walk(lab, blk, False)
    out = dict(start=np.zeros(U, np.int32), end=np.zeros(U, np.int32), conf=np.zeros(U, np.float32), score=NEG, ok=0)
    if not end > NEG:
        return out
    out["score"], out["ok"] = end, 1
    t, u = T - 1, U
    while (t, u) != (0, 0):
        if bit[t, u]:
            u -= 1
            out["start"][u] = out["end"][u] = t
        else:
            t -= 1
    if U:
        out["conf"] = np.asarray(_dexp(lab[out["start"], np.arange(U)]), np.float32)
    return out


def total(lab, blk):
    """-> dict(total, ok): the fp32 log-likelihood of the token string, the log-sum over every path from (0, 0) to END."""
    v = _walk(lab, blk, True)[2]
    return dict(total=v, ok=1 if v > NEG else 0)


def path_sums(lab, blk):
    """Every path from (0, 0) to END, enumerated: the fp32 left-to-right sum of each one's arc weights (for the tests of this file's walks)."""
    lab, blk, T, U = _shapes(lab, blk)
    out = []

    def go(t, u, acc):
        with np.errstate(all="ignore"):
            if t == T - 1 and u == U:
                out.append(F(acc + blk[t, u]))
                return
            if t + 1 < T:
                go(t + 1, u, F(acc + blk[t, u]))
            if u < U:
                go(t, u + 1, F(acc + lab[t, u]))
    go(0, 0, F(0.0))
    return np.asarray(out, np.float32)
