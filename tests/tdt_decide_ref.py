"""Plain numpy restatement of ONE greedy decision of the TDT / RNNT decode loop and of the CTC greedy decoders, on the state words of the device
kernel (kernels/decode_dev.hpp tdt_decide_one; kernels.hpp TdtState), for tests/test_gpu_tdt_decide.py, tests/test_gpu_ctc_greedy.py and the CPU checks of
tests/test_tdt_decide_ref.py.

Transcribed from the reference: src/tdt.cpp:62-106 (the loop), :157-187 (timestamps), src/rnnt.cpp:75-107, src/phrase_boost.cpp:52-66 (trie advance),
:301-336 (boosted argmax, unboosted confidence), and the oracle's tdt_greedy_ex (safety cap, margin).  One call of decide_step() is one launch: every live
utterance takes one decision -- or, with a frame window F > 1, walks through the blanks whose successor frame lies inside the window.

EXACT forms (exact / boost / score kernels): log-probs are the oracle's own rows (oracle.log_softmax_rows: max-subtracted, canonical sum64), the argmax is
the first maximum of those ROUNDED log-probs; every word is compared bit for bit.

FAST form (h_bf16, kernels/decode_dev.hpp FAST): not bit-identical by design.  lp_k = (x_k - m) - log(S), S = sum_i exp2((x_i - m) * log2e).  With u = 2^-24,
y_i = m - x_i >= 0 and e_i = exp(-y_i):
  * the argument fl(fl(x_i - m) * c): two roundings and the rounded constant, relative 3 u, i.e. a relative error ln2 * |arg| * 3 u = 3 u y_i of the term;
  * the hardware exp2: 1 ulp, relative 2^-23;            => relative error of S from its terms:  sum_i e_i (3 u y_i + 2^-23) / S
  * an fp32 sum of V positive terms in an unspecified order: relative (V - 1) u / (1 - (V - 1) u), plus u for the last partial sums
  * dlogf: 2 ulp of |lse| (and never less than u)
  * the two subtractions of the result: u (y_k + |lp_k|) each
fast_bound() returns the sum per element: |lp_fast - lp_float64| <= bound.  Two log-probs closer than 2 x bound in float64 may be ordered either way by an
implementation that compares computed log-probs: fast_margin_limit = 2 x max bound of the row.  (The duration head of the fast form is the exact form's code.)
"""
import numpy as np

F32 = np.float32
FILL32 = 0x7FC5A5A5
NEG = F32(-np.inf)
INF = F32(np.inf)
MAX_ACTIVE = 64                      # kernels.hpp kTrieMaxActive
MUTANTS = ("last_max", "raw_argmax", "boosted_conf", "end_unclamped", "blank_skip0", "commit_on_blank", "cap_off_by_one", "lens_unclamped", "margin_no_dur",
           "window_past_Tb", "window_cap_ignored", "runnerup_merge")
# the case (name in CASES) that catches each planted fault; tests/test_tdt_decide_ref.py asserts it
MUTANT_CAUGHT_BY = {"last_max": "ties-v600-d5", "raw_argmax": "rounded-ties-v1025", "boosted_conf": "boost-prefixes", "end_unclamped": "script-v65-d5",
                    "blank_skip0": "script-v65-d5", "commit_on_blank": "script-v65-d5", "cap_off_by_one": "script-cap", "lens_unclamped": "script-v65-d5",
                    "margin_no_dur": "ties-dur-d5", "window_past_Tb": "window-f4-vd70", "window_cap_ignored": "window-cap-f4", "runnerup_merge": "runnerup-v600-d5"}


def bf16_rne(x):
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def first_max(x, last=False):
    x = np.asarray(x)
    return int(x.size - 1 - np.argmax(x[::-1])) if last else int(np.argmax(x))


def second_best(x, k, same_wave_only=False):
    """the largest element besides k.  same_wave_only: the planted fault "runnerup_merge" -- a reduction that loses the runner-ups of the other waves (element i
    is held by thread i % 256, wave (i % 256) // 64)"""
    if x.size <= 1:
        return NEG
    keep = np.arange(x.size) != k
    if same_wave_only:
        keep &= (np.arange(x.size) % 256) // 64 == (k % 256) // 64
    return F32(np.max(x[keep])) if keep.any() else NEG


def fast_bound(x):
    """float64 log-softmax of the fp32 row x and the per-element bound on the fast form's error (module docstring)"""
    x64 = np.asarray(x, np.float64)
    u = 2.0 ** -24
    y = x64.max() - x64
    fin = np.isfinite(y)
    e = np.where(fin, np.exp(-np.where(fin, y, 0.0)), 0.0)
    S = e.sum()
    lse = np.log(S)
    n = x64.size
    rel = (e * (3 * u * np.where(fin, y, 0.0) + 2.0 ** -23)).sum() / S + (n - 1) * u / (1 - (n - 1) * u) + u + n * 2.0 ** -126 / S
    err_lse = rel + max(2 * np.spacing(F32(abs(lse))), u)
    lp = -y - lse
    bound = np.where(fin, err_lse + 2 * u * (np.where(fin, y, 0.0) + np.abs(np.where(fin, lp, 0.0))), 0.0)
    return lp, bound


class Trie:
    """CSR trie of kernels.hpp TrieDev: children of node i = entries off[i] .. off[i + 1] of (tok, node)"""

    def __init__(self, off, tok, node, boost):
        self.off, self.tok, self.node, self.boost = np.asarray(off), np.asarray(tok), np.asarray(node), F32(boost)

    def mask(self, states, V):                                   # get_boosted_tokens: phrase_boost.cpp:39-50
        m = np.zeros(V, bool)
        for s in states:
            for c in range(self.off[s], self.off[s + 1]):
                if 0 <= self.tok[c] < V:
                    m[self.tok[c]] = True
        return m

    def advance(self, states, tok):                              # phrase_boost.cpp:52-66: the root is always active
        nx = [0]
        for s in states:
            for c in range(self.off[s], self.off[s + 1]):
                if self.tok[c] == tok and self.node[c] not in nx:
                    nx.append(int(self.node[c]))
        return nx


def decide_step(sc, S, logits, hn, cn, lsm, mut=(), fast=False, log=None):
    """One launch on the state S (dict of arrays, B leading rows; changed in place).  logits [B F][V + D]; hn / cn [L][B][Hp].  lsm: the row log-softmax of the
    specification (oracle.log_softmax_rows).  fast: label log-probs in float64 (S["conf"] / S["margin"] then hold float64-derived values to compare within
    the bound); log (a list) receives one dict per decision of the fast form: b, m64 (the float64 margin between the winner's log-prob and the best log-prob of a
    DIFFERENT logit value -- equal logits give equal computed log-probs, so a tie of logits is decided by index and not by rounding), limit (fast_margin_limit),
    n_out (tokens stored so far), tok (the decision stores a token), bk (the winner's own bound), mg / emg (the decision's margin, duration head included, and the
    bound on the fast form's error of it)."""
    B, V, D, mt, blank = sc["B"], sc["V"], sc["D"], sc["max_tokens"], sc["blank"]
    trie, force = S.get("trie"), S.get("force")
    Fw = sc.get("F", 1) if (sc.get("F", 1) > 1 and trie is None and force is None) else 1
    dur_tab = list(sc.get("durations", [])) + [0] * 8
    for b in range(B):
        if S["done"][b]:
            continue
        n_force, f_off = 0, 0
        if force is not None:
            lab_f, dur_f, nf, nfb, stride = force
            n_force, f_off = int(nfb[b] if nfb is not None else nf), b * stride
            if n_force <= 0:
                S["lens"][b] = 0; S["done"][b] = 1; S["done_count"] += 1
                if S.get("need") is not None:
                    S["need"][b] = 0
                continue
        Tb = int(S["Tb"][b]) if S.get("Tb") is not None else sc["T"]
        row0 = int(S["row0"][b]) if S.get("row0") is not None else b * sc["T"]
        cap = sc["max_steps"]
        if S.get("Tb") is not None and cap > 0:
            cap = Tb * (sc["max_symbols"] + 1) + 16
        if "cap_off_by_one" in mut and cap > 0:
            cap += 1
        t, steps, nsym, f = int(S["t"][b]), int(S["steps"][b]), int(S["nsym"][b]), 0
        mg_run = S["margin"][b] if S.get("margin") is not None else None
        while True:
            row = np.ascontiguousarray(logits[b * Fw + f], F32)
            if fast:
                lp64, bound = fast_bound(row[:V])
                k = first_max(lp64)
                lab_lp = lp64
                if log is not None:
                    other = row[:V] != row[k]
                    m64 = lp64[k] - (np.max(lp64[other]) if other.any() else -np.inf)
                    ent = dict(b=b, m64=float(m64), limit=2 * float(bound.max()), n_out=int(S["n_out"][b]), tok=k != blank, bk=float(bound[k]), mg=np.inf, emg=0.0)
                    if V > 1:                                    # the runner-up as computed lies in [lp2 - bound of that element, max_i (lp_i + bound_i)]
                        rest = np.arange(V) != k
                        lp2 = np.max(lp64[rest])
                        k2 = np.flatnonzero(rest & (lp64 == lp2))[0]
                        ent["emg"] = float(bound[k] + max(np.max((lp64 + bound)[rest]) - lp2, bound[k2]))
                    log.append(ent)
            else:
                lab_lp = lsm(row[:V])
            score = lab_lp
            if trie is not None:
                act = [int(a) for a in S["act"][b, : S["n_act"][b]]]
                score = (lab_lp + np.where(trie.mask(act, V), trie.boost, F32(0))).astype(F32)
            if "raw_argmax" in mut:
                k = first_max(row[:V])
            else:
                k = first_max(score, last="last_max" in mut)
            skip, di, dur_lp = 1, 0, None
            if D > 0:
                dur_lp = lsm(row[V:])
                di = first_max(dur_lp, last="last_max" in mut)
                skip = dur_tab[di] if di < 8 else 1
            if mg_run is not None and trie is None:
                mg = lab_lp[k] - (second_best(score, k, "runnerup_merge" in mut) if not fast else (np.max(np.delete(lab_lp, k)) if V > 1 else -np.inf))
                if D > 0 and "margin_no_dur" not in mut:
                    dmg = F32(dur_lp[di] - second_best(dur_lp, di)) if D > 1 else INF
                    if fast and log is not None and dmg <= mg - log[-1]["emg"]:     # the duration head is the exact form's code: where it sets the margin
                        log[-1]["emg"] = 0.0                                        # whatever the label head's error, there is none
                    mg = min(mg, dmg)
                if fast and log is not None:
                    log[-1]["mg"] = float(mg)
                mg_run = mg if mg < mg_run else mg_run
            conf_lp = score[k] if "boosted_conf" in mut else lab_lp[k]
            if force is not None:
                if S.get("score_lab") is not None:
                    S["score_lab"][f_off + steps] = lab_lp
                if S.get("score_dur") is not None:
                    S["score_dur"][f_off + steps] = dur_lp
                kk = min(steps, n_force - 1)
                k = int(lab_f[f_off + kk])
                conf_lp = lab_lp[k]
                skip = dur_tab[int(dur_f[f_off + kk])]
            if Fw > 1 and k == blank:
                adv = max(skip, 1) if D > 0 else 1
                capped = cap > 0 and steps + 1 >= cap and "window_cap_ignored" not in mut
                inside = t + adv < Tb or "window_past_Tb" in mut
                if f + adv < Fw and inside and not capped:
                    f += adv; t += adv; steps += 1; nsym = 0
                    continue
            break
        if "last_f" in S:
            S["last_f"][b] = f
        if mg_run is not None and trie is None:
            S["margin"][b] = mg_run
        nsteps, n_out, commit = steps + 1, int(S["n_out"][b]), k != blank
        if not commit:
            if D > 0:
                t += skip if "blank_skip0" in mut else max(skip, 1)
            else:
                t += 1
            nsym = 0
        else:
            if n_out < mt:
                S["ids"][b, n_out] = k
                S["start"][b, n_out] = t
                e = t + max(skip, 1) - 1 if D > 0 else t
                S["end"][b, n_out] = e if (sc.get("keep_state") or e < Tb or "end_unclamped" in mut) else Tb - 1
                S["conf"][b, n_out] = np.exp(np.float64(conf_lp)) if fast else S["exp"](F32(conf_lp))
            S["token"][b] = k
            if trie is not None:
                nx = trie.advance(act, k)[:MAX_ACTIVE]
                S["act"][b, : len(nx)] = nx
                S["n_act"][b] = len(nx)
            n_out += 1
            if D > 0:
                if skip > 0:
                    t += skip
            else:
                nsym += 1
                if nsym >= sc["max_symbols"]:
                    t += 1; nsym = 0
        if commit or "commit_on_blank" in mut:
            S["h"][:, b] = hn[:, b]
            S["c"][:, b] = cn[:, b]
        if S.get("need") is not None:
            fin = t >= Tb or (cap > 0 and nsteps >= cap) or (force is not None and nsteps >= n_force)
            S["need"][b] = 1 if (commit and not fin) else 0
            if not commit and not fin:
                for fw in range(Fw):
                    tt = min(t + fw, Tb - 1)
                    s = (S["ep"][row0 + tt] + S["pp"][b]).astype(F32)
                    z = np.where(s > 0, s, F32(0)).astype(F32)
                    S["z"][b * Fw + fw] = bf16_rne(z) if sc.get("h_bf16") else z
        finished = t >= Tb or (force is not None and nsteps >= n_force)
        ln = n_out if "lens_unclamped" in mut else min(n_out, mt)
        if not finished and cap > 0 and nsteps >= cap:
            finished, ln = True, -1
        S["t"][b], S["steps"][b], S["n_out"][b], S["nsym"][b] = t, nsteps, n_out, nsym
        if finished:
            S["lens"][b] = ln; S["done"][b] = 1; S["done_count"] += 1


def run(o, lsm, expf, mut=(), fast=False, n_steps=None, log=None):
    """the reference after n_steps (default: all) launches of case o -> the state dict"""
    S = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o["st"].items()}
    S["exp"] = lambda x: expf(np.asarray([x], F32))[0]
    if S.get("trie") is not None:
        S["trie"] = Trie(*S["trie"])
    if fast:
        S["conf"] = S["conf"].astype(np.float64)
        if S.get("margin") is not None:
            S["margin"] = S["margin"].astype(np.float64)
    S["last_f"] = np.zeros(o["sc"]["B"], np.int32)                  # the window row of each utterance's last decision (not a word of the kernel's)
    lsm1 = lambda row: lsm(np.ascontiguousarray(row, F32)[None])[0]
    for k in range(o["logits"].shape[0] if n_steps is None else n_steps):
        decide_step(o["sc"], S, o["logits"][k], o["hn"][k], o["cn"][k], lsm1, mut, fast, log)
    return S


# ---- CTC ---------------------------------------------------------------------------------------------------------------------------------------
def ctc_greedy(lp, blank, trie=None):
    """ctc_greedy_decode_with_timestamps (src/ctc.cpp:93-123) / its boosted form (src/phrase_boost.cpp:70-171) on ONE utterance's log-probs [T][V]
    -> ids, start, end, lp of the emitted frames (confidence = exp of it)"""
    T, V = lp.shape
    ids, st, en, cl = [], [], [], []
    prev, act = -1, [0]
    for t in range(T):
        sc = lp[t] if trie is None else (lp[t] + np.where(trie.mask(act, V), trie.boost, F32(0))).astype(F32)
        best = first_max(sc)
        if best != prev:
            if prev != -1 and prev != blank and ids:
                en[-1] = t - 1
            if best != blank:
                ids.append(best); st.append(t); en.append(t); cl.append(lp[t, best])
                if trie is not None:
                    act = trie.advance(act, best)[:MAX_ACTIVE]
        prev = best
    if ids:
        en[-1] = T - 1
    return np.asarray(ids, np.int32), np.asarray(st, np.int32), np.asarray(en, np.int32), np.asarray(cl, F32)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
def form_of(sc, boost=False, score=False):
    """mirror of kernels/decode.hip tdt_decide_form (asserted against the diagnostic's answer on the GPU): (kernel, NC, row staging)"""
    VD, ns = sc["V"] + sc["D"], sc["L"] * sc["Hp"]
    kernel = "boost" if boost else "score" if score else "fast" if (sc.get("h_bf16") and VD <= 33 * 256 and sc["V"] >= 2) else "exact"
    nc = 12 if kernel in ("boost", "score") else 3 if ns <= 768 else 6 if ns <= 1536 else 12
    row = "window" if (kernel == "exact" and sc.get("F", 1) > 1) else "row5" if VD <= 1280 else "row33" if VD <= 8448 else "batch8"
    return kernel, nc, row


ALL_FORMS = ({("exact", nc, r) for nc in (3, 6, 12) for r in ("row5", "row33", "batch8", "window")} | {("fast", nc, r) for nc in (3, 6, 12) for r in ("row5", "row33")}
             | {(k, 12, r) for k in ("boost", "score") for r in ("row5", "row33", "batch8")})

TIE_PAIRS = [(7, 7 + 256), (7, 7 + 512), (3, 40), (200, 257 + 64), (0, -1), (5, 261, 300), (64, 128), (9, 9 + 256 * 20)]     # -1: the last valid index


def _case(name, fam, V, D, **kw):
    c = dict(name=name, fam=fam, V=V, D=D, L=1, Hp=16, B=5, T=6, F=1, J=0, n_steps=3, mt=4, max_steps=0, max_symbols=10, keep_state=0, h_bf16=0, ragged=False,
             need=False, trie=None, boost=0.0, score=False, p_blank=0.4, blank=None, seed=1, compare_act=True, stuck=(), capwalk=False)
    c.update(kw)
    return c


def _cases():
    cs = []
    vd = [(2, 0), (7, 5), (64, 1), (65, 5), (1275, 5), (1276, 5), (8193, 5), (8443, 5), (8444, 5), (9000, 8), (300, 9)]
    lh = [(1, 16), (1, 768), (1, 772), (2, 768), (2, 772), (4, 768)]
    bs = [1, 5, 64, 70]
    for i, (V, D) in enumerate(vd):
        L, Hp = lh[i % 6]
        B = bs[i % 4] if V < 8000 else (1, 5)[i % 2]
        cs.append(_case(f"form-v{V}-d{D}-l{L}h{Hp}-b{B}", "forms", V, D, L=L, Hp=Hp, B=B, seed=10 + i))
    for i, (L, Hp) in enumerate(lh):
        cs.append(_case(f"form-state-l{L}h{Hp}-b{bs[(i + 1) % 4]}", "forms", 65, 5, L=L, Hp=Hp, B=bs[(i + 1) % 4], seed=30 + i))
    for nc, (L, Hp) in ((3, (1, 16)), (6, (2, 768)), (12, (4, 768))):     # every NC on the longer rows as well
        cs.append(_case(f"form-v8193-nc{nc}", "forms", 8193, 5, L=L, Hp=Hp, B=2, n_steps=2, seed=40 + nc))
        cs.append(_case(f"form-v8444-nc{nc}", "forms", 8444, 5, L=L, Hp=Hp, B=2, n_steps=2, seed=50 + nc))
    cs.append(_case("ties-v600-d5", "ties", 600, 5, B=7, n_steps=4, seed=60))
    cs.append(_case("ties-v600-blank10", "ties", 600, 5, B=7, n_steps=4, blank=10, seed=61))
    cs.append(_case("ties-v8193", "ties", 8193, 5, B=7, n_steps=2, seed=62))
    cs.append(_case("ties-rnnt-v600", "ties", 600, 0, B=7, n_steps=4, max_symbols=3, seed=63))
    for D in (5, 8, 9):
        cs.append(_case(f"ties-dur-d{D}", "durties", 70, D, B=6, n_steps=4, seed=64 + D))
    # one winner, the runner-up(s) one level below it at the tie placements (both orders), everything else far below: the margin shows the runner-up reduction.
    # ONE launch: the running margin keeps the smallest, so a second decision would hide a lost runner-up of the first
    cs.append(_case("runnerup-v600-d5", "runnerup", 600, 5, B=20, n_steps=1, seed=66))
    cs.append(_case("runnerup-rnnt-v600", "runnerup", 600, 0, B=20, n_steps=1, seed=67))
    cs.append(_case("runnerup-v8193", "runnerup", 8193, 5, B=20, n_steps=1, seed=68))
    cs.append(_case("rounded-ties-v1025", "rounded", 1025, 5, B=6, n_steps=3, seed=70))
    cs.append(_case("rounded-ties-v8193", "rounded", 8193, 5, B=3, n_steps=2, seed=71))
    # scripts: random decisions with small limits, so that token overflow, the cap, duration 0 runs, finished utterances all occur
    cs.append(_case("script-v65-d5", "script", 65, 5, B=12, T=9, n_steps=60, mt=5, p_blank=0.35, seed=80, stuck=(1,)))
    cs.append(_case("script-cap", "script", 65, 5, B=8, T=90, n_steps=40, mt=50, max_steps=23, p_blank=0.15, seed=81, stuck=(2,)))
    cs.append(_case("script-keep-state", "script", 65, 5, B=8, T=7, n_steps=40, mt=30, keep_state=1, seed=82))
    cs.append(_case("script-ragged", "script", 65, 5, B=9, T=8, n_steps=120, mt=12, max_steps=500, ragged=True, max_symbols=2, p_blank=0.2, seed=83, stuck=(0,)))
    for ms in (1, 3):
        cs.append(_case(f"script-rnnt-ms{ms}", "script", 65, 0, B=8, T=8, n_steps=40, mt=9, max_symbols=ms, seed=84 + ms))
    for J in (16, 1024, 1040):
        cs.append(_case(f"script-need-j{J}", "script", 65, 5, B=6, T=8, n_steps=30, mt=9, need=True, J=J, ragged=(J == 1024), seed=90 + J))
    for F in (2, 4, 8):
        for VD in (70, 1280):
            cs.append(_case(f"window-f{F}-vd{VD}", "window", VD - 5, 5, B=min(8, 16 // F), T=12, F=F, n_steps=14, mt=6, need=True, J=32, max_steps=16,
                            ragged=(F == 4), p_blank=0.8, seed=100 + F + VD))
    for F in (2, 4, 8):                                                # runs of blanks that meet the cap at window row 0, 1 or 2 (capwalk in make_case)
        cs.append(_case(f"window-cap-f{F}", "window", 65, 5, B=max(3, min(8, 16 // F)), T=12, F=F, n_steps=2, mt=6, need=True, J=32, max_steps=4, capwalk=True, seed=104 + F))
    for nc, (L, Hp) in ((6, (2, 768)), (12, (4, 768))):
        cs.append(_case(f"window-f2-vd70-nc{nc}", "window", 65, 5, L=L, Hp=Hp, B=3, T=12, F=2, n_steps=6, mt=6, need=True, J=32, p_blank=0.7, seed=107 + nc))
    tries = {"root": [], "one": [[3, 9, 4]], "prefixes": [[3, 9, 4], [3, 9, 7, 2], [9, 4], [3], [4, 3, 9]], "overflow": [[5] * 70], "big-id": [[3, 99999], [99999, 4]]}
    for nm, ph in tries.items():
        cs.append(_case(f"boost-{nm}", "boost", 65, 5, B=6, T=40, n_steps=(75 if nm == "overflow" else 24), mt=80, trie=ph, boost=3.0, p_blank=0.1, seed=110 + len(nm),
                        compare_act=(nm != "overflow")))
    cs.append(_case("boost-zero", "boost", 65, 5, B=6, T=40, n_steps=12, mt=80, trie=tries["prefixes"], boost=0.0, p_blank=0.1, seed=120))
    cs.append(_case("boost-flips-tie", "boost", 65, 5, B=6, T=40, n_steps=6, mt=80, trie=tries["prefixes"], boost=0.25, p_blank=0.0, seed=123))
    cs.append(_case("boost-v8193", "boost", 8193, 5, B=2, T=40, n_steps=4, mt=80, trie=tries["prefixes"], boost=3.0, seed=121))
    cs.append(_case("boost-v8444", "boost", 8444, 5, B=2, T=40, n_steps=3, mt=80, trie=tries["prefixes"], boost=3.0, seed=122))
    cs.append(_case("score-v65", "score", 65, 5, B=5, T=10, n_steps=14, mt=20, score=True, seed=130))
    cs.append(_case("score-v8193", "score", 8193, 5, B=2, T=10, n_steps=3, mt=20, score=True, seed=131))
    cs.append(_case("score-v8444", "score", 8444, 5, B=2, T=10, n_steps=3, mt=20, score=True, seed=132))
    fast = []
    for c in cs:
        if c["fam"] in ("forms", "ties", "runnerup", "rounded", "script") and c["trie"] is None and c["V"] + c["D"] <= 8448 and c["V"] >= 2 and c["Hp"] % 2 == 0:
            fast.append(dict(c, name="fast-" + c["name"], h_bf16=1))
    return cs + fast


CASES = _cases()
TIE_FAMILIES = ("ties", "durties", "rounded")


def case_id(c):
    return c["name"]


def make_case(c):
    """-> dict(sc = the scalars, logits [n_steps][B F][V + D], hn / cn [n_steps][L][B][Hp], st = the state before the first launch)"""
    rng = np.random.default_rng(c["seed"])
    V, D, L, Hp, B, T, F, J, K, mt = (c[k] for k in ("V", "D", "L", "Hp", "B", "T", "F", "J", "n_steps", "mt"))
    blank = V - 1 if c["blank"] is None else c["blank"]
    half = bool(c["h_bf16"])
    sc = dict(B=B, T=T, V=V, D=D, L=L, Hp=Hp, blank=blank, max_symbols=c["max_symbols"], max_tokens=mt, max_steps=c["max_steps"], keep_state=c["keep_state"],
              h_bf16=int(half), F=F, J=J, durations=[0, 1, 2, 3, 4, 2, 1, 3][: min(D, 8)])
    R = B * F
    logits = (rng.integers(-8, 9, (K, R, V + D)) / 4.0).astype(F32)
    fam = c["fam"]
    tok_pool = np.unique(np.clip([0, 1, 3, 4, 5, 9, 40, 255, 256, 300, 1024, 4097, V - 2, V - 1], 0, V - 1))
    dmax = min(D, 8)
    for k in range(K):
        for r in range(R):
            row = logits[k, r]
            lab = blank if rng.random() < c["p_blank"] else int(rng.choice(tok_pool))
            if D > 0:
                di = int(rng.integers(0, dmax))
                if fam == "script" and rng.random() < 0.3:
                    di = 0                                      # duration 0: another symbol on the same frame / a blank that advances 1
                row[V + di] = 8.0
            idx = k * R + r
            if c["capwalk"]:                                    # blanks of duration 1, except one token at window row 1 of utterance 1
                row[:V], row[V:] = np.minimum(row[:V], 2.0), 0.0
                row[3 if (r // F == 1 and r % F == 1) else blank] = 8.0
                row[V + 1] = 8.0
                continue
            if r // F in c["stuck"]:                            # a run of duration-0 tokens on one frame: past max_tokens, into the cap
                row[3], row[V:] = 8.0, 0.0
                if D > 0:
                    row[V] = 8.0
                continue
            if fam == "ties":
                pr = [p % V for p in TIE_PAIRS[idx % len(TIE_PAIRS)]]
                if idx % 3 == 1:
                    pr = [blank] + [p for p in pr[1:] if p != blank] if blank < max(pr) else pr + [blank]
                row[:V] = np.minimum(row[:V], 2.0)
                row[pr] = 8.0
                ru = [(p + 17) % V for p in pr]                 # the runner-up likewise: two (three) equal values below the winners
                if idx % 2 == 0:
                    row[[q for q in ru if q not in pr]] = 7.0
            elif fam == "durties":
                pairs = [(0, dmax - 1), (1, 2), (dmax - 2, dmax - 1), (0, 1, 2)]
                row[V:] = np.minimum(row[V:], 2.0)
                row[[V + p for p in pairs[idx % 4]]] = 8.0
                row[lab] = 8.0                                  # the duration margin (a tie: 0) must win over the label margin, which is larger
            elif fam == "runnerup":
                live = r - r // 5                               # (every fifth utterance is finished: it takes no placement away)
                pr = [p % V for p in TIE_PAIRS[live % len(TIE_PAIRS)]]
                if (live // len(TIE_PAIRS)) % 2:
                    pr = pr[::-1]                               # the winner at the higher index
                row[:V] = np.minimum(row[:V], 2.0)
                row[pr[0]] = 8.0
                row[pr[1:]] = 7.0                               # one runner-up, or two equal ones
            elif fam == "rounded":
                row[:V] = 0.0
                i, j = (3, 700) if idx % 2 == 0 else (260, 261)
                row[i] = 1.0
                row[j] = np.nextafter(F32(1.0), F32(2.0))       # the HIGHER index carries the larger logit; both round to one log-prob under lse ~ 6 .. 8
                row[[10, 500, V - 1]] = -np.inf
            else:
                row[lab] = 8.0
    hn = rng.standard_normal((K, L, B, Hp)).astype(F32)
    cn = rng.standard_normal((K, L, B, Hp)).astype(F32)
    h0 = (np.arange(L * B * Hp, dtype=F32).reshape(L, B, Hp) + 0.5)     # every element distinct: a mis-addressed commit shows
    c0 = -h0
    if half:
        hn, h0 = bf16_rne(hn), (np.arange(L * B * Hp) + 1).astype(np.uint16).reshape(L, B, Hp)
    Tb = rng.integers(1, T + 1, B).astype(np.int32) if c["ragged"] else None
    if Tb is not None:
        Tb[0] = 1
    tb = Tb if Tb is not None else np.full(B, T, np.int32)
    fill_i = np.full((B, mt), FILL32, np.uint32).view(np.int32)
    st = dict(t=(rng.integers(0, 2, B) * rng.integers(0, tb)).astype(np.int32), steps=rng.integers(0, 3, B).astype(np.int32),
              n_out=rng.integers(0, 3, B).astype(np.int32), nsym=np.zeros(B, np.int32), done=(np.arange(B) % 5 == 4).astype(np.int32),
              token=rng.integers(0, V, B).astype(np.int32), lens=np.full(B, -7, np.int32), done_count=int((np.arange(B) % 5 == 4).sum()),
              h=h0, c=c0, ids=fill_i.copy(), start=fill_i.copy(), end=fill_i.copy(), conf=fill_i.copy().view(F32),
              margin=np.full(B, np.inf, F32))
    if c["capwalk"]:                                                # max_steps = 4: the walk meets the cap at window row 2, 1, 0
        st["t"][:], st["steps"] = 0, (1 + np.arange(B) % 3).astype(np.int32)
    if D == 0:
        st["nsym"] = rng.integers(0, c["max_symbols"], B).astype(np.int32)
    if Tb is not None:
        off = np.concatenate([[0], np.cumsum(Tb)])
        st["Tb"], st["row0"] = Tb, (off[:-1] + 2).astype(np.int32)      # (the rows need not start at 0)
    if c["need"]:
        rows = int(tb.sum()) + 2 if Tb is not None else B * T
        st["need"] = rng.integers(0, 2, B).astype(np.int32)
        st["pp"] = rng.standard_normal((B, J)).astype(F32)
        st["ep"] = rng.standard_normal((rows, J)).astype(F32)
        st["z"] = np.full((B, J), 0x7FC5, np.uint16) if half else np.full((R, J), FILL32, np.uint32).view(F32)
    if c["trie"] is not None:
        st["trie"] = csr(c["trie"]) + (c["boost"],)
        st["act"] = np.full((B, MAX_ACTIVE), FILL32, np.uint32).view(np.int32)
        st["act"][:, 0] = 0
        st["n_act"] = np.ones(B, np.int32)
        if c["name"] == "boost-overflow":                           # a run of one token walks the chain: depth 0 .. 70 active at once
            logits[:, :, :V] = np.minimum(logits[:, :, :V], 2.0)
            logits[:, :, 5] = 8.0
            logits[:, :, V:] = 0.0
            logits[:, :, V] = 8.0                                   # duration 0: stay on the frame
        if c["name"] == "boost-flips-tie":                          # token 2 (in no phrase) ties with token 9 (a child of the root): the boost decides
            logits[:, :, :V] = np.minimum(logits[:, :, :V], 2.0)
            logits[:, :, [2, 9]] = 8.0
        if c["boost"] == 3.0 and c["name"] != "boost-overflow":     # a boost that flips a decision: the trie's tokens sit 2.0 below the scripted winner
            logits[:, :, [3, 9, 4]] = 6.0
    if c["score"]:
        stride = 9
        nfb = np.asarray([(0, 1, 7, 9, 4)[b % 5] for b in range(B)], np.int32)
        st["force"] = (rng.choice(tok_pool.tolist() + [blank] * 4, B * stride).astype(np.int32), rng.integers(0, dmax, B * stride).astype(np.int32), 0, nfb, stride)
        st["steps"] = np.zeros(B, np.int32)
        st["score_lab"] = np.full((B * stride + 2, V), FILL32, np.uint32).view(F32)
        st["score_dur"] = np.full((B * stride + 2, D), FILL32, np.uint32).view(F32)
    return dict(sc=sc, logits=logits, hn=hn, cn=cn, st=st, boost=c["trie"] is not None, score=c["score"])


def csr(phrases):
    kids = [{}]
    for p in phrases:
        n = 0
        for tk in p:
            if tk not in kids[n]:
                kids[n][tk] = len(kids)
                kids.append({})
            n = kids[n][tk]
    off, tok, node = [0], [], []
    for k in kids:
        tok += list(k.keys()); node += list(k.values()); off.append(len(tok))
    return np.asarray(off, np.int32), np.asarray(tok, np.int32), np.asarray(node, np.int32)


STATE_WORDS = ("t", "steps", "n_out", "nsym", "done", "token", "lens", "ids", "start", "end")


def script_logits(V, D, labels, dur_idx):
    """the oracle's own decisions as logits: 8.0 at the chosen label and duration index, 0 elsewhere -> [n][V + D]"""
    x = np.zeros((len(labels), V + D), F32)
    x[np.arange(len(labels)), labels] = 8.0
    if D > 0:
        x[np.arange(len(labels)), V + np.asarray(dur_idx)] = 8.0
    return x


# ---- CTC cases -----------------------------------------------------------------------------------------------------------------------------------
CTC_TRIES = {"root": [], "one": [[3, 5, 4]], "prefixes": [[3, 5, 4], [3, 5, 7, 2], [5, 4], [3], [4, 3, 5]], "overflow": [[5] * 70], "big-id": [[3, 99999], [99999, 4]]}


def _ctc_cases():
    cs = []
    i = 0
    for n in (2, 8, 9, 64, 65, 1025):
        for ld in (n, n + 3):
            cs.append(dict(name=f"lsm-n{n}-ld{ld}-rows{(1, 5, 126 * 3 + 1)[i % 3]}", kind="random", n=n, ld=ld, B=1, T=(1, 5, 126 * 3 + 1)[i % 3], seed=200 + i))
            i += 1
    for n in (9, 700):
        cs.append(dict(name=f"ties-n{n}", kind="ties", n=n, ld=n + 3, B=3, T=8, seed=220 + n))
    for kind in ("all-blank", "one-token", "alternating"):
        cs.append(dict(name=kind, kind=kind, n=9, ld=9, B=3, T=7, seed=230))
    cs.append(dict(name="t1", kind="random", n=9, ld=9, B=4, T=1, seed=231))
    cs.append(dict(name="b65", kind="random", n=9, ld=12, B=65, T=6, seed=232))
    cs.append(dict(name="ragged-pitch", kind="random", n=9, ld=9, B=5, n_frames=[4, 1, 9, 2, 6], pitch=13, seed=233))
    cs.append(dict(name="ragged-b65", kind="random", n=8, ld=8, B=65, n_frames=[1 + (b * 7) % 5 for b in range(65)], pitch=6, seed=234))
    for nm in CTC_TRIES:
        cs.append(dict(name=f"boost-{nm}", kind="run" if nm == "overflow" else "random", n=65, ld=65, B=3, T=(150 if nm == "overflow" else 20), trie=nm, boost=3.0,
                       seed=240 + len(nm)))
    cs.append(dict(name="boost-zero", kind="random", n=65, ld=65, B=3, T=20, trie="prefixes", boost=0.0, seed=250))
    cs.append(dict(name="boost-flips-tie", kind="ties", n=65, ld=68, B=3, T=12, trie="prefixes", boost=0.25, seed=251))
    cs.append(dict(name="boost-ragged", kind="random", n=65, ld=65, B=4, n_frames=[7, 1, 12, 3], pitch=14, trie="prefixes", boost=3.0, seed=252))
    return cs


CTC_CASES = _ctc_cases()


def make_ctc_case(c):
    """-> logits [frames][ld] (levels: multiples of 0.25, so that equal maxima are exact ties), blank, frames per utterance"""
    rng = np.random.default_rng(c["seed"])
    n, ld, B = c["n"], c["ld"], c["B"]
    nf = np.asarray(c.get("n_frames") or [c["T"]] * B, np.int32)
    frames = int(nf.sum())
    blank = n - 1
    x = (rng.integers(-8, 9, (frames, ld)) / 4.0).astype(F32)
    x[:, n:] = 50.0                                               # the columns past n are not part of the row
    small = [0, 3, 4, 5, 7, 2, n - 2, blank]
    for r in range(frames):
        kind = c["kind"]
        if kind == "all-blank":
            x[r, blank] = 8.0
        elif kind == "one-token":
            x[r, 3] = 8.0
        elif kind == "alternating":
            x[r, (3, blank, 3, 4)[r % 4]] = 8.0
        elif kind == "run":
            x[r, (5, blank)[r % 2]] = 8.0                   # 75 emissions of one token: more than kTrieMaxActive depths active at once
        elif kind == "ties":
            pr = [p % n for p in TIE_PAIRS[r % len(TIE_PAIRS)]]
            if r % 3 == 1:
                pr = pr + [blank]
            x[r, :n] = np.minimum(x[r, :n], 2.0)
            x[r, pr] = 8.0
        elif rng.random() < 0.85:
            x[r, small[int(rng.integers(0, len(small)))] % n] = 8.0 if c.get("trie") is None else 4.0
    if n > 2 and frames > 2:
        x[1, 1] = -np.inf
    return dict(logits=x, n=n, blank=blank, n_frames=nf, uniform=c.get("n_frames") is None, pitch=c.get("pitch") or int(nf.max()),
                trie=(csr(CTC_TRIES[c["trie"]]) + (c["boost"],)) if c.get("trie") else None, phrases=CTC_TRIES[c["trie"]] if c.get("trie") else None,
                boost=c.get("boost", 0.0))
