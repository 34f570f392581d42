"""TDT beam search with n-gram language-model shallow fusion, in plain Python on fp32 scalars: the written specification of DESIGN.md
section 5.5.7 that the fused kernels of kernels/tdt_beam.hip are compared against bit for bit.

search of tests/tdt_beam_ref.py restated with the LM terms.  A hypothesis additionally carries hist (every symbol the model has seen: its
start symbols, then the prefix -- the dictionary scorer's form of the automaton state) and lm (fp32), the LM score of its token string:
the left-to-right sum of alpha * lookup + beta, every operation one fp32 rounding.  The start is (lm.start(), 0.0).
    blank arc   inherits hist and lm;
    label arc   with token c: lp = lookup(hist, c), lm2 = lm + ((alpha * lp) + beta) -- three roundings, no fma --, one lookup per
                (hypothesis, label): the Kd durations of a label share it.  </s> is never proposed or added;
    pruning     stays acoustic: the K best labels and the Kd best durations of a row are tdt_beam_ref.expand_row's, and a candidate's
                acoustic score stays s + (x + dl[i]);
    ranking     by f = score + lm (one fp32 add) wherever the unfused search decides by score: the duplicate rule (same (prefix, t): the
                better f stays, a strict >, so the earlier pool entry stays on a tie) and the choice of the W best (f down, pool position up).
lm is a function of the token string alone, so the entries of one state carry the same lm and hist, and the better f is the better
acoustic score -- except where the fp32 rounding of score + lm makes two different scores one f.  That tie is resolved as every tie is: the
earlier pool entry stays, with its own (possibly lower) acoustic score.
Pool order, max_tokens, finishing at t = T, the step cap and "only finished hypotheses are returned" are the unfused search's.  score of a
returned hypothesis is its path's acoustic log-probability, lm_score its lm; an unfilled slot has score -inf and lm_score 0.
With alpha = beta = 0 every lm is +0.0 (0 * lp is -0.0, -0.0 + 0 is +0.0, 0 + 0 is +0.0), f = score, and every output is the unfused
search's bit for bit.  The model is an ngram_lm_ref.RefLm (a dictionary scorer, no automaton)."""
import numpy as np

import tdt_beam_ref as R

F = np.float32
NEG = R.NEG


def step(beam, joint, lm, alpha, beta, T, blank, durations, W, K, Kd, max_tokens, info=None):
    """One step: beam = [(prefix, t, score, toks, hist, lm)] -> the new beam (at most W entries).  info: as tdt_beam_ref.step's."""
    pool = [h for h in beam if h[1] >= T]
    src = [w for w, h in enumerate(beam) if h[1] >= T]
    for w, (prefix, t, score, toks, hist, lmv) in enumerate(beam):
        if t >= T:
            continue
        logp, dl = joint(t, prefix)
        labs, durs = R.expand_row(logp, dl, blank, K, Kd)
        for i, x in labs:
            if i != blank and len(prefix) >= max_tokens:
                continue
            if i != blank:
                lp = lm.lookup(hist, i)[0]                          # one lookup per (hypothesis, label)
                with np.errstate(all="ignore"):
                    lm2 = F(lmv + F(F(alpha * lp) + beta))          # three roundings
            for d, y in durs:
                with np.errstate(all="ignore"):
                    s = F(score + F(x + y))
                if i == blank:
                    pool.append((prefix, min(t + max(int(durations[d]), 1), T), s, toks, hist, lmv))
                else:
                    pool.append((prefix + (i,), min(t + int(durations[d]), T), s, toks + ((t, d, x),), hist + (i,), lm2))
                src.append(w)
    with np.errstate(all="ignore"):
        f = [F(h[2] + h[5]) for h in pool]
    state = {}                                                      # (prefix, t) -> pool position of the entry that stays
    for pos, h in enumerate(pool):
        key = (h[0], h[1])
        if key not in state or f[pos] > f[state[key]]:
            state[key] = pos
    kept = sorted(state.values(), key=lambda pos: (-float(f[pos]), pos))
    R._report(info, pool, src, state, kept[:W])
    return [pool[pos] for pos in kept[:W]]


def search(joint, T, blank, durations, lm, alpha, beta, W, K, Kd, N, max_tokens, trace=None):
    """-> the dict of tdt_beam_ref.search (hypotheses in fused order, score acoustic) + lm_score [N] fp32"""
    assert T >= 1 and W >= 1 and K >= 1 and Kd >= 1 and 1 <= N <= W and max_tokens >= 1
    alpha, beta = F(alpha), F(beta)
    beam = [((), 0, F(0.0), (), lm.start(True), F(0.0))]
    steps = 0
    while any(h[1] < T for h in beam) and steps < T + max_tokens:
        beam = step(beam, joint, lm, alpha, beta, T, blank, durations, W, K, Kd, max_tokens)
        steps += 1
        if trace is not None:
            trace.append(list(beam))
    done = [h for h in beam if h[1] >= T][:N]
    out = dict(ids=np.zeros((N, max_tokens), np.int32), start=np.zeros((N, max_tokens), np.int32), end=np.zeros((N, max_tokens), np.int32),
               dur_idx=np.zeros((N, max_tokens), np.int32), conf=np.zeros((N, max_tokens), np.float32), lens=np.zeros(N, np.int32),
               score=np.full(N, NEG, np.float32), lm_score=np.zeros(N, np.float32), ok=int(len(done) > 0), steps=steps)
    for n, (prefix, t, score, toks, hist, lmv) in enumerate(done):
        U = len(prefix)
        out["lens"][n], out["score"][n], out["lm_score"][n] = U, score, lmv
        if U:
            out["ids"][n, :U] = prefix
            out["start"][n, :U] = [k[0] for k in toks]
            out["dur_idx"][n, :U] = [k[1] for k in toks]
            out["end"][n, :U] = [min(k[0] + max(int(durations[k[1]]), 1) - 1, T - 1) for k in toks]
            out["conf"][n, :U] = R._dexp(np.asarray([k[2] for k in toks], np.float32))
    return out


def flip_arpa(V, token, lp_token=-0.01, lp_rest=-3.0):
    """ARPA text of a unigram model over the ids 0 .. V - 2 that puts nearly all its mass on `token`."""
    lines = ["\\data\\", f"ngram 1={V - 1}", "", "\\1-grams:"]
    lines += [f"{lp_token if i == token else lp_rest:.6f}\t{i}" for i in range(V - 1)]
    return "\n".join(lines + ["", "\\end\\", ""])
