"""TDT forced alignment of a given token string, in plain numpy fp32: the written specification of DESIGN.md section 5.5.2 that
kernels/tdt_align.hip is compared against bit for bit.

One utterance: T >= 1 frames, U >= 0 tokens ids[U], durations dur[D] (1 <= D <= 8) and the lattice scores -- log-softmax outputs of the joint
at frame t with the prediction net having consumed ids[:u]:
    lab[T][U]      lab[t][u] the label log-prob of ids[u]
    blk[T][U+1]    the blank log-prob
    dl[T][U+1][D]  the duration log-probs
Arcs out of cell (t, u), as the greedy loop moves (src/tdt.cpp:62-106):
    blank i: to (t + max(dur[i], 1), u)      weight blk[t][u] + dl[t][u][i]
    label i: to (t + dur[i], u + 1), u < U   weight lab[t][u] + dl[t][u][i]
An arc whose target frame is >= T goes to the one terminal END when its target u is U and is dropped otherwise.
The walk is max-plus in pull form: alpha[0][0] = 0, every other cell -inf, and a cell takes the maximum over its candidates in the order
blank i = 0 .. D-1 (from (t - max(dur[i], 1), u)), then label i = 0 .. D-1 (from (t - dur[i], u - 1)); a candidate is alpha[src] + (x + dl),
two fp32 adds in that order; a strict > keeps the earlier candidate.  END pulls from the source frames in ascending order, within a frame blank
before label, then by i."""
import numpy as np

F = np.float32
NEG = F(-np.inf)
NONE = 255                                                          # back-pointer of a cell nothing reaches


def _dexp(x):
    import oracle
    return oracle.math_v("exp", np.ascontiguousarray(x, np.float32))


def _empty(U):
    return dict(start=np.zeros(U, np.int32), end=np.zeros(U, np.int32), dur_idx=np.zeros(U, np.int32), conf=np.zeros(U, np.float32),
                score=NEG, ok=0)


def walk(lab, blk, dl, dur):
    """The max-plus walk -> (alpha [T][U+1], back-pointers [T][U+1] (i: blank i, D + i: label i, NONE), END value, END's arc (t, code))."""
    blk = np.ascontiguousarray(blk, np.float32)
    T, U = blk.shape[0], blk.shape[1] - 1
    lab = np.ascontiguousarray(lab, np.float32).reshape(T, U)
    dl = np.ascontiguousarray(dl, np.float32).reshape(T, U + 1, -1)
    D = len(dur)
    assert T >= 1 and 1 <= D <= 8 and dl.shape[2] == D
    alpha = np.full((T, U + 1), NEG, np.float32)
    bp = np.full((T, U + 1), NONE, np.uint8)
    alpha[0, 0] = F(0.0)
    with np.errstate(all="ignore"):
        for t in range(T):
            for u in range(U + 1):
                if t == 0 and u == 0:
                    continue
                best, arg = NEG, NONE
                for i in range(D):
                    ts = t - max(int(dur[i]), 1)
                    if ts >= 0:
                        c = F(alpha[ts, u] + F(blk[ts, u] + dl[ts, u, i]))
                        if c > best:
                            best, arg = c, i
                if u >= 1:
                    for i in range(D):
                        ts = t - int(dur[i])
                        if ts >= 0:
                            c = F(alpha[ts, u - 1] + F(lab[ts, u - 1] + dl[ts, u - 1, i]))
                            if c > best:
                                best, arg = c, D + i
                alpha[t, u], bp[t, u] = best, arg
        end, earc = NEG, None
        for t in range(T):
            for i in range(D):
                if t + max(int(dur[i]), 1) >= T:
                    c = F(alpha[t, U] + F(blk[t, U] + dl[t, U, i]))
                    if c > end:
                        end, earc = c, (t, i)
            if U >= 1:
                for i in range(D):
                    if t + int(dur[i]) >= T:
                        c = F(alpha[t, U - 1] + F(lab[t, U - 1] + dl[t, U - 1, i]))
                        if c > end:
                            end, earc = c, (t, D + i)
    return alpha, bp, end, earc


def best_path(lab, blk, dl, dur):
    """-> (score, arcs) of the walk's path, arcs = [(t, u, code)] from (0, 0) to END (code i: blank i, D + i: label i); (-inf, None) when no
    path reaches END."""
    blk = np.ascontiguousarray(blk, np.float32)
    T, U = blk.shape[0], blk.shape[1] - 1
    D = len(dur)
    _, bp, end, earc = walk(lab, blk, dl, dur)
    if not end > NEG:
        return NEG, None
    t, code = earc
    u = U - 1 if code >= D else U                                   # the cell the arc leaves
    arcs = [(t, u, code)]
    while (t, u) != (0, 0):
        code = int(bp[t, u])
        assert code != NONE
        if code >= D:
            t, u = t - int(dur[code - D]), u - 1
        else:
            t = t - max(int(dur[code]), 1)
        arcs.append((t, u, code))
    return F(end), arcs[::-1]


def align(lab, blk, dl, dur):
    """-> dict(start, end, dur_idx, conf [U], score, ok); ok = 0 (score -inf, arrays of zeros) when no path reaches END."""
    blk = np.ascontiguousarray(blk, np.float32)
    T, U = blk.shape[0], blk.shape[1] - 1
    lab = np.ascontiguousarray(lab, np.float32).reshape(T, U)
    D = len(dur)
    score, arcs = best_path(lab, blk, dl, dur)
    out = _empty(U)
    if arcs is None:
        return out
    out["score"], out["ok"] = score, 1
    for t, u, code in arcs:
        if code >= D:                                               # token u emitted from (t, u) with duration index code - D
            i = code - D
            out["start"][u], out["end"][u], out["dur_idx"][u] = t, min(t + max(int(dur[i]), 1) - 1, T - 1), i
    if U:
        out["conf"] = np.asarray(_dexp(lab[out["start"], np.arange(U)]), np.float32)
    return out


def oracle_lattice(om, enc, ids):
    """The lattice of ONE utterance enc [T][d] from the oracle's teacher-forced scoring: row u is the tokens ids[:u] forced with the zero
    duration at frame 0, then T blanks of duration 1 -- step u + t is the joint at frame t after ids[:u]."""
    cfg = om.cfg
    dur = list(cfg.durations)
    i0, i1 = dur.index(0), dur.index(1)
    T, U, D = enc.shape[0], len(ids), len(dur)
    lab = np.zeros((T, U), np.float32); blk = np.zeros((T, U + 1), np.float32); dl = np.zeros((T, U + 1, D), np.float32)
    for u in range(U + 1):
        labels = np.asarray(list(ids[:u]) + [cfg.blank_id] * T, np.int32)
        didx = np.asarray([i0] * u + [i1] * T, np.int32)
        r = om.tdt_score(enc, labels, didx)
        assert r["n"] == u + T, (r["n"], u, T)
        rows = r["label_lp"][u:u + T]
        blk[:, u] = rows[:, cfg.blank_id]
        if u < U:
            lab[:, u] = rows[:, int(ids[u])]
        dl[:, u] = r["dur_lp"][u:u + T]
    return lab, blk, dl


def pack(lattices):
    """[(lab, blk, dl)] -> the packed arrays of pk_tdt_align: lab / blk / dl concatenated per utterance, n_frames[B], id_offsets[B + 1]."""
    n_frames = np.asarray([x[1].shape[0] for x in lattices], np.int32)
    off = np.zeros(len(lattices) + 1, np.int32)
    off[1:] = np.cumsum([x[1].shape[1] - 1 for x in lattices])
    cat = lambda k: np.concatenate([np.ascontiguousarray(x[k], np.float32).ravel() for x in lattices] + [np.zeros(0, np.float32)])
    return cat(0), cat(1), cat(2), n_frames, off


def make_lattice(family, T, U, D, rng):
    """The input families of the alignment tests (any fp32 values are a valid input of the walk).  "ties": every value one of a few exactly
    representable numbers, so that sums are exact and whole paths tie; "holes": the same with about 10 % of the entries -inf; "peaky":
    log-softmax rows (over a stand-in vocabulary of 4 / over D) with one dominant entry each."""
    if family == "peaky":
        def lsm(x):
            x = x - x.max(axis=-1, keepdims=True)
            return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)
        lx = rng.normal(size=(T, U + 1, 4)); dx = rng.normal(size=(T, U + 1, D))
        np.put_along_axis(lx, rng.integers(0, 4, size=(T, U + 1, 1)), 9.0, axis=-1)
        np.put_along_axis(dx, rng.integers(0, D, size=(T, U + 1, 1)), 9.0, axis=-1)
        l = lsm(lx)
        return np.ascontiguousarray(l[:, :U, 0]), np.ascontiguousarray(l[:, :, 3]), lsm(dx)
    vals = np.asarray([-0.25, -0.5, -1.0, -1.5, -2.0, -3.0], np.float32)
    lab, blk, dl = (vals[rng.integers(0, len(vals), size=sh)] for sh in ((T, U), (T, U + 1), (T, U + 1, D)))
    if family == "holes":
        for a in (lab, blk, dl):
            a[rng.random(size=a.shape) < 0.1] = NEG
    return lab, blk, dl
