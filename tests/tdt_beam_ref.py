"""TDT beam search with n-best output, in plain Python on fp32 scalars: the written specification of DESIGN.md section 5.5.5 that
kernels/tdt_beam.hip is compared against bit for bit.

One clip of T >= 1 frames and a callback joint(t, prefix) -> (logp[V], dl[D]): the log-softmax outputs of the joint at frame t with the
prediction net having consumed [blank, prefix...] (fp32).  The search is max-path over the lattice of section 5.5.2: a hypothesis is one
concrete path, its score that path's left-to-right fp32 sum, every arc score + (x + dl[i]) -- two fp32 adds in that order.

A hypothesis: prefix (tuple of ids), frame pointer t, score, and per emitted token (emission frame, duration index, label log-prob).
One step expands every live hypothesis (t < T) of the beam once:
    row         the K best non-blank labels by (log-prob descending, id ascending) and the blank, the K + 1 sorted together by the same rule;
    durations   the Kd best indices by (dl descending, index ascending);
    candidates  label rank, then duration rank; a label arc goes to (t + dur[i], prefix + id), a blank arc to (t + max(dur[i], 1), prefix);
                a hypothesis of max_tokens tokens forms no label candidates; a target frame >= T finishes the hypothesis at t = T;
    pool        the beam's finished hypotheses in beam order, then the candidates of the live ones by beam slot, then candidate order;
    duplicates  entries with the same (prefix, t) are one state: the better score stays, a strict > (the earlier entry stays on a tie);
                the state stands in the pool where the entry that stays stood;
    new beam    the W best by (score descending, pool position ascending).
The search ends when the beam holds no live hypothesis (or after T + max_tokens steps: every arc adds at least one to t + len(prefix), so
by then nothing is live).  Only finished hypotheses are returned, in beam order, the first N."""
import numpy as np

F = np.float32
NEG = F(-np.inf)


def _dexp(x):
    import oracle
    return oracle.math_v("exp", np.ascontiguousarray(x, np.float32))


def expand_row(logp, dl, blank, K, Kd):
    """-> (labels [(id, logp)] of K + 1 entries sorted, durations [(index, dl)] of Kd entries sorted)"""
    logp = np.asarray(logp, np.float32); dl = np.asarray(dl, np.float32)
    V, D = len(logp), len(dl)
    K, Kd = min(K, V - 1), min(Kd, D)
    order = lambda vals, ids: sorted(ids, key=lambda i: (-float(vals[i]), i))
    labs = order(logp, [i for i in range(V) if i != blank])[:K] + [blank]
    labs = order(logp, labs)
    durs = order(dl, list(range(D)))[:Kd]
    return [(i, F(logp[i])) for i in labs], [(i, F(dl[i])) for i in durs]


def step(beam, joint, T, blank, durations, W, K, Kd, max_tokens, info=None):
    """One step: beam = [(prefix, t, score, toks)] -> the new beam (at most W entries).  info (a dict) receives what the step decided beside
    the beam: "parent", the old beam's slot every new entry came from, and "merged", one (tokens, t, the entry that stays came from another
    slot) per pool entry that left as the duplicate of a state."""
    pool = [h for h in beam if h[1] >= T]
    src = [w for w, h in enumerate(beam) if h[1] >= T]             # the beam slot every pool entry came from
    for w, (prefix, t, score, toks) in enumerate(beam):
        if t >= T:
            continue
        logp, dl = joint(t, prefix)
        labs, durs = expand_row(logp, dl, blank, K, Kd)
        for i, x in labs:
            if i != blank and len(prefix) >= max_tokens:
                continue
            for d, y in durs:
                with np.errstate(all="ignore"):
                    s = F(score + F(x + y))
                if i == blank:
                    t2, p2, k2 = t + max(int(durations[d]), 1), prefix, toks
                else:
                    t2, p2, k2 = t + int(durations[d]), prefix + (i,), toks + ((t, d, x),)
                pool.append((p2, min(t2, T), s, k2))
                src.append(w)
    state = {}                                                      # (prefix, t) -> pool position of the entry that stays
    for pos, h in enumerate(pool):
        key = (h[0], h[1])
        if key not in state or h[2] > pool[state[key]][2]:
            state[key] = pos
    kept = sorted(state.values(), key=lambda pos: (-float(pool[pos][2]), pos))
    _report(info, pool, src, state, kept[:W])
    return [pool[pos] for pos in kept[:W]]


def _report(info, pool, src, state, kept):
    if info is not None:
        info["parent"] = [src[pos] for pos in kept]
        info["merged"] = [(len(h[0]), h[1], src[pos] != src[state[(h[0], h[1])]]) for pos, h in enumerate(pool) if state[(h[0], h[1])] != pos]


def search(joint, T, blank, durations, W, K, Kd, N, max_tokens, trace=None):
    """-> dict(ids, start, end, dur_idx [N][max_tokens] int32, conf [N][max_tokens] fp32, lens [N], score [N], ok, steps)"""
    assert T >= 1 and W >= 1 and K >= 1 and Kd >= 1 and 1 <= N <= W and max_tokens >= 1        # (the device: W, K <= 16, Kd <= 8)
    beam = [((), 0, F(0.0), ())]
    steps = 0
    while any(h[1] < T for h in beam) and steps < T + max_tokens:
        beam = step(beam, joint, T, blank, durations, W, K, Kd, max_tokens)
        steps += 1
        if trace is not None:
            trace.append(list(beam))
    done = [h for h in beam if h[1] >= T][:N]
    out = dict(ids=np.zeros((N, max_tokens), np.int32), start=np.zeros((N, max_tokens), np.int32), end=np.zeros((N, max_tokens), np.int32),
               dur_idx=np.zeros((N, max_tokens), np.int32), conf=np.zeros((N, max_tokens), np.float32), lens=np.zeros(N, np.int32),
               score=np.full(N, NEG, np.float32), ok=int(len(done) > 0), steps=steps)
    for n, (prefix, t, score, toks) in enumerate(done):
        U = len(prefix)
        out["lens"][n], out["score"][n] = U, score
        if U:
            out["ids"][n, :U] = prefix
            out["start"][n, :U] = [k[0] for k in toks]
            out["dur_idx"][n, :U] = [k[1] for k in toks]
            out["end"][n, :U] = [min(k[0] + max(int(durations[k[1]]), 1) - 1, T - 1) for k in toks]
            out["conf"][n, :U] = _dexp(np.asarray([k[2] for k in toks], np.float32))
    return out


def path_to(t, u, durations):
    """Some arc sequence [(is_label, duration index)] from (0, 0) to the lattice cell (frame t, u tokens), None when nothing reaches it."""
    seen = {(0, 0): None}
    todo = [(0, 0)]
    while todo and (t, u) not in seen:
        nxt = []
        for (a, b) in todo:
            for i, d in enumerate(durations):
                for cell, arc in (((a + max(int(d), 1), b), (0, i)), ((a + int(d), b + 1), (1, i))):
                    if cell[0] <= t and cell[1] <= u and cell not in seen:
                        seen[cell] = ((a, b), arc)
                        nxt.append(cell)
        todo = nxt
    if (t, u) not in seen:
        return None
    arcs, cell = [], (t, u)
    while seen[cell] is not None:
        cell, arc = seen[cell]
        arcs.append(arc)
    return arcs[::-1]


def oracle_joint(om, enc):
    """joint(t, prefix) of ONE clip enc [T][d] from the oracle's teacher-forced scoring (Oracle.tdt_score), memoised per (t, prefix): the
    oracle walks some path to the cell (frame t, prefix consumed) and one more step, whose recorded rows are the joint's outputs there."""
    cfg = om.cfg
    dur = list(cfg.durations)
    memo = {}

    def joint(t, prefix):
        key = (t, tuple(prefix))
        if key not in memo:
            arcs = path_to(t, len(prefix), dur)
            assert arcs is not None, key
            it = iter(prefix)
            labels = [next(it) if lab else cfg.blank_id for lab, _ in arcs] + [cfg.blank_id]
            didx = [i for _, i in arcs] + [0]
            r = om.tdt_score(enc, np.asarray(labels, np.int32), np.asarray(didx, np.int32))
            assert r["n"] == len(labels), (r["n"], key)
            memo[key] = (r["label_lp"][-1].copy(), r["dur_lp"][-1].copy())
        return memo[key]
    return joint
