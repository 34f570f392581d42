"""CTC prefix beam search with n-gram language-model shallow fusion in plain Python: the written specification of DESIGN.md section
5.5.6 that ctc_beam_walk_kernel<true> (kernels/ctc_beam.hip) is compared against bit for bit.

beam_search of tests/ctc_beam_ref.py restated with the LM terms: a beam entry carries lm, the LM score of its token string (a function of
the string alone: the left-to-right sum of alpha * lookup + beta, every operation one fp32 rounding); a stay candidate inherits it, an
extension by c has lm + ((alpha * lookup(p, c)) + beta); candidates are selectable exactly as in the unfused search and are ordered by
f = score + lm (one fp32 add) where the unfused search orders by score.  Pruning to the K best tokens of a frame stays acoustic, merges
are the unfused search's.  The model is an ngram_lm_ref.RefLm (a dictionary scorer, no automaton)."""
import numpy as np

import ctc_beam_ref as R

F = np.float32
NEG = R.NEG


def beam_search_lm(lp, blank, lm, alpha, beta, beam_width=8, token_prune=16, n_best=1, trace=None):
    """lp [T][V] fp32 -> list of (ids tuple, acoustic score fp32, lm score fp32) in fused order, at most n_best entries."""
    lp = np.ascontiguousarray(lp, np.float32)
    T, V = lp.shape
    W, K = int(beam_width), max(1, min(int(token_prune), V - 1))
    alpha, beta = F(alpha), F(beta)
    h0 = lm.start(True)
    beam = [dict(p=(), pb=F(0.0), pnb=NEG, tot=F(0.0), lm=F(0.0))]
    with np.errstate(all="ignore"):
        for t in range(T):
            cid, cval = R.topk_tokens(lp[t], blank, K)
            kof = {int(c): k for k, c in enumerate(cid)}
            lpb = lp[t, blank]
            rank = {e["p"]: i for i, e in enumerate(beam)}
            nb = len(beam)
            npb = np.full(nb, NEG, np.float32); rep = np.full(nb, NEG, np.float32); mrg = np.full(nb, NEG, np.float32)
            for i, e in enumerate(beam):
                npb[i] = e["tot"] + lpb
                if e["p"]:
                    last = e["p"][-1]
                    k = kof.get(last)
                    if k is not None:
                        rep[i] = e["pnb"] + cval[k]
                        j = rank.get(e["p"][:-1])
                        if j is not None:
                            par = beam[j]
                            src = par["pb"] if (par["p"] and par["p"][-1] == last) else par["tot"]
                            mrg[i] = src + cval[k]
            npnb = R.lae(rep, mrg)
            sc = R.lae(npb, npnb)
            cands = []
            for i, e in enumerate(beam):
                if sc[i] > NEG:
                    f = F(sc[i] + e["lm"])                          # stay: the prefix's own lm
                    cands.append((-float(f), i, 0, 0, e["p"], npb[i], npnb[i], sc[i], e["lm"]))
                last = e["p"][-1] if e["p"] else -1
                for k in range(K):
                    c = int(cid[k])
                    q = e["p"] + (c,)
                    if q in rank:
                        continue                                    # merged into q's own entry above; the LM does not enter the merge
                    v = F((e["pb"] if c == last else e["tot"]) + cval[k])
                    if v > NEG:
                        lpc = lm.lookup(h0 + e["p"], c)[0]
                        lm2 = F(e["lm"] + F(F(alpha * lpc) + beta))  # three roundings
                        f = F(v + lm2)
                        cands.append((-float(f), i, 1, c, q, NEG, v, v, lm2))
            cands.sort(key=lambda x: x[:4])                         # f, then parent rank, stay before extend, token id
            beam = [dict(p=c[4], pb=F(c[5]), pnb=F(c[6]), tot=F(c[7]), lm=F(c[8])) for c in cands[:W]]
            if trace is not None:
                trace.append([e["p"] for e in beam])
    return [(e["p"], e["tot"], e["lm"]) for e in beam[:n_best]]


def search_batch_lm(lps, blank, lm, alpha, beta, beam_width, token_prune, n_best, timestamps=True):
    """The arrays pk_ctc_beam_search_lm returns: those of ctc_beam_ref.search_batch + lm_score [B][N] (0 in a slot the beam does not fill)."""
    B, N = len(lps), n_best
    Tmax = max(x.shape[0] for x in lps)
    ids = np.zeros((B, N, Tmax), np.int32); st = np.zeros((B, N, Tmax), np.int32); en = np.zeros((B, N, Tmax), np.int32)
    cf = np.zeros((B, N, Tmax), np.float32); lens = np.zeros((B, N), np.int32); score = np.full((B, N), NEG, np.float32)
    lms = np.zeros((B, N), np.float32)
    for b, lp in enumerate(lps):
        for j, (p, s, l) in enumerate(beam_search_lm(lp, blank, lm, alpha, beta, beam_width, token_prune, n_best)):
            L = len(p)
            ids[b, j, :L] = p; lens[b, j] = L; score[b, j] = s; lms[b, j] = l
            if timestamps:
                al = R.viterbi_align(lp, p, blank)
                assert al is not None, "a hypothesis of the search cannot be aligned"
                st[b, j, :L] = al["start"]; en[b, j, :L] = al["end"]; cf[b, j, :L] = al["conf"]
    return dict(ids=ids, lens=lens, score=score, start=st, end=en, conf=cf, lm_score=lms)


def flip_case():
    """A constructed input on which the acoustic 1-best and the fused 1-best differ -> (lp [T][V], blank, ARPA text, alpha, beta).
    Three frames, tokens 0 and 1: the acoustics prefer 0 slightly in the middle frame, the model makes 1 ten times as likely."""
    V, blank = 3, 2
    x = np.log(np.array([[0.05, 0.05, 0.90], [0.50, 0.45, 0.05], [0.05, 0.05, 0.90]]))
    lp = R.log_softmax32(x)
    text = "\n".join(["\\data\\", "ngram 1=2", "", "\\1-grams:", "-1.300000\t0", "-0.300000\t1", "", "\\end\\", ""])
    return lp, blank, text, 1.0, 0.0
