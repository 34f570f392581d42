"""The forward-algorithm total of a given token string under the TDT head, and the ordering rule of the TDT-rescored n-best list, in plain
numpy: the written specification of DESIGN.md section 5.5.3 that kernels/tdt_total.hip is compared against bit for bit.

The lattice and its arcs are those of tests/tdt_align_ref.py (lab [T][U], blk [T][U+1], dl [T][U+1][D]; blank i to (t + max(dur[i], 1), u),
label i to (t + dur[i], u + 1), one terminal END).  A blank with duration 0 and a blank with duration 1 are two distinct arcs to t + 1 and both
are summed, as the greedy loop takes either decision to the same place.
The walk is sum-product in pull form: alpha[0][0] = 0 and every other cell is a left fold with ctc_beam_ref.lae, starting from -inf, over its
candidates in the alignment's order -- blank i = 0 .. D-1 (from (t - max(dur[i], 1), u)), then label i = 0 .. D-1 (from (t - dur[i], u - 1)); a
candidate is alpha[src] + (x + dl), two fp32 adds in that order, and a candidate whose source frame is < 0 does not exist (folding -inf in
its place gives the same bits: lae(a, -inf) = a).  END is the same fold in the alignment's END order: source frames ascending, within a frame
blank before label, then by i.  ok = total > -inf.

The cells of one anti-diagonal t + u depend on earlier diagonals only, so forward_total folds a whole diagonal as numpy vectors: element-wise,
every cell sees exactly the scalar operations above."""
import numpy as np

import tdt_align_ref as A
from ctc_beam_ref import lae

F = np.float32
NEG = F(-np.inf)


def _shapes(lab, blk, dl, dur, dt):
    blk = np.ascontiguousarray(blk, dt)
    T, U = blk.shape[0], blk.shape[1] - 1
    lab = np.ascontiguousarray(lab, dt).reshape(T, U)
    dl = np.ascontiguousarray(dl, dt).reshape(T, U + 1, -1)
    D = len(dur)
    assert T >= 1 and 1 <= D <= 8 and dl.shape[2] == D
    return lab, blk, dl, T, U, D


def _forward(lab, blk, dl, dur, dt, add):
    """-> (alpha [T][U+1], END) in dtype dt; add(a, b) = log(exp a + exp b) element-wise."""
    lab, blk, dl, T, U, D = _shapes(lab, blk, dl, dur, dt)
    neg = dt(-np.inf)
    alpha = np.full((T, U + 1), neg, dt)
    alpha[0, 0] = dt(0.0)
    with np.errstate(all="ignore"):
        for d in range(1, T + U):
            u = np.arange(max(0, d - (T - 1)), min(d, U) + 1)
            t = d - u
            acc = np.full(len(u), neg, dt)
            for i in range(D):
                ts = t - max(int(dur[i]), 1)
                v, s = ts >= 0, np.maximum(ts, 0)
                cand = (alpha[s, u] + (blk[s, u] + dl[s, u, i]).astype(dt)).astype(dt)
                acc = add(acc, np.where(v, cand, neg)).astype(dt)
            if U >= 1:
                up = np.maximum(u - 1, 0)
                for i in range(D):
                    ts = t - int(dur[i])
                    v, s = (ts >= 0) & (u >= 1), np.maximum(ts, 0)
                    cand = (alpha[s, up] + (lab[s, up] + dl[s, up, i]).astype(dt)).astype(dt)
                    acc = add(acc, np.where(v, cand, neg)).astype(dt)
            alpha[t, u] = acc
        end = np.full(1, neg, dt)
        for t in range(max(0, T - 8), T):                           # durations are <= 8: no earlier frame has an arc to END
            for i in range(D):
                if t + max(int(dur[i]), 1) >= T:
                    end = add(end, dt(alpha[t, U] + dt(blk[t, U] + dl[t, U, i]))).astype(dt)
            if U >= 1:
                for i in range(D):
                    if t + int(dur[i]) >= T:
                        end = add(end, dt(alpha[t, U - 1] + dt(lab[t, U - 1] + dl[t, U - 1, i]))).astype(dt)
    return alpha, end[0]


def forward_total(lab, blk, dl, dur):
    """-> the fp32 log-likelihood of the token string: the log-sum over every path from (0, 0) to END (-inf when there is none)."""
    assert max(int(x) for x in dur) <= 8
    return F(_forward(lab, blk, dl, dur, np.float32, lae)[1])


def forward_total64(lab, blk, dl, dur):
    """The same sums in float64 with np.logaddexp."""
    assert max(int(x) for x in dur) <= 8
    return np.float64(_forward(lab, blk, dl, dur, np.float64, lambda a, b: np.logaddexp(a, np.atleast_1d(b)))[1])


def total(lab, blk, dl, dur):
    """-> dict(total, ok) as pk_tdt_total returns them."""
    v = forward_total(lab, blk, dl, dur)
    return dict(total=v, ok=1 if v > NEG else 0)


def combined(ctc, tdt, w):
    """fl(fl((1 - w) ctc) + fl(w tdt)) in fp32; 1 - w is formed in fp32 too."""
    w = F(w)
    with np.errstate(all="ignore"):
        return F(F(F(F(1.0) - w) * F(ctc)) + F(w * F(tdt)))


def rescore_order(lens, ctc, tdt, ok, w):
    """The ordering rule of pk_transcribe_pcm_nbest_rescored for ONE clip: slots j = 0 .. N-1 of the beam (lens[j], ctc[j]; an unfilled slot
    has lens 0 and score -inf), tdt[j] / ok[j] their TDT totals -> (order, combined[N]): stable, descending by combined; a filled slot with
    ok = 0 after every scored one; unfilled slots last.  Ties keep the beam's order.  combined is -inf for a slot that is not scored (the formula
    would give 0 * -inf there)."""
    N = len(ctc)
    unfilled = [int(lens[j]) == 0 and not F(ctc[j]) > NEG for j in range(N)]
    cls = [2 if unfilled[j] else (0 if ok[j] else 1) for j in range(N)]
    comb = np.asarray([combined(ctc[j], tdt[j], w) if cls[j] == 0 else NEG for j in range(N)], np.float32)
    for j in range(N):
        if np.isnan(comb[j]):                                       # from an infinite part: not scored
            cls[j], comb[j] = 1, NEG
    order = list(range(N))
    # insertion sort: j moves in front of k only when it is strictly better (lower class, or the same class 0 and a larger value)
    out = []
    for j in order:
        p = len(out)
        while p > 0:
            k = out[p - 1]
            better = cls[j] < cls[k] or (cls[j] == cls[k] == 0 and comb[j] > comb[k])
            if not better:
                break
            p -= 1
        out.insert(p, j)
    return out, comb


# ---- the cases of tests/test_gpu_tdt_total.py, shared with the fp32-vs-float64 bound of tests/test_tdt_total_ref.py --------------------------
# The shapes and duration sets of tests/test_gpu_tdt_align.py: the walk takes the same widths (64 / 256 threads), the same ring and the same limits.
FAMILIES = ["ties", "holes", "peaky"]
DURS = {"d01234": [0, 1, 2, 3, 4], "d01": [0, 1], "d124": [1, 2, 4], "d8": [4, 0, 1, 1, 2, 8, 3, 5]}
SMALL = [(1, 0), (1, 1), (1, 3), (2, 1), (5, 3), (8, 8)]
EDGES = [(66, 62), (66, 63), (66, 64), (258, 254), (258, 256), (514, 510), (514, 512), (3, 1535)]
LARGE = [(130, 40), (376, 90)]
BOUNDARY = ([(T, U, ("d01", "d01234", "d8")[k % 3], ("ties", "peaky")[k % 2]) for k, (T, U) in enumerate(EDGES)]
            + [(3, 1535, "d8", "ties"), (3, 1534, "d8", "peaky")]
            + [(T, U, dn, "peaky") for (T, U) in LARGE for dn in ("d01234", "d124")] + [(130, 40, "d8", "ties"), (130, 40, "d01", "holes")])
RAGGED = [(9, 3), (7, 0), (4, 5), (70, 66), (12, 12), (1, 0)]        # with d124; (4, 5): more tokens than frames and no zero duration


def small_lattices(T, U, dname, family):
    dur = DURS[dname]
    rng = np.random.default_rng(T * 1009 + U * 31 + len(dur) + 7 * FAMILIES.index(family))
    return [A.make_lattice(family, T, U, len(dur), rng) for _ in range(3)]


def boundary_lattice(T, U, dname, family):
    dur = DURS[dname]
    return A.make_lattice(family, T, U, len(dur), np.random.default_rng(T * 1009 + U * 31 + len(dur)))


def ragged_lattices():
    rng = np.random.default_rng(77)
    return [A.make_lattice("ties", T, U, 3, rng) for T, U in RAGGED]
