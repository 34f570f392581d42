"""Float64 reference of the Transformer LM behind pk_nlm_* (n-best rescoring), an fp32 NumPy evaluation of the same function as a yardstick,
the re-ranking rule, and per-element error bounds for its two kernels.  Written from the rule in include/parakeet_amd.h / DESIGN.md section
5.5.11, not from the kernels.

The function.  For a token string ids[0..n): inputs x_0 = bos, x_i = ids[i-1]; P = n + 1 positions with an end term (eos >= 0), else P = n.
h_i = tok_emb[x_i] + pos_emb[i], then emb_norm_ if present; the blocks of TransformerEncoder (pre-norm: x + f(LN(x)); post-norm: LN(x + f(x));
ReLU feed-forward) with attention softmax(scale q_i . k_j over j <= i) V, scale = 1 / sqrt(head dim); final_norm_ if present;
logit_i[c] = h_i . W[c] (+ b[c]); lp_i = logit_i[target_i] - logsumexp_c logit_i[c], target_i = ids[i] for i < n and eos for i = n; total = the
left-to-right fp32 sum of lp_i.  The empty string scores 0 without an end term; P > max_positions is not scored (ok 0, total -inf).

Error bound of the causal attention kernel (per element of ctx).  It is attention_ref's fp32 bound (its docstring, items 1, 3 and 4) with the
position term absent (u = v = 0, no P) and, for query row i, the keys cut at j <= i: causal_head_reference calls
attention_ref.softmax_pv_bounds once per row on z_i[0..i], C_j = |q_i| . |k_j| and v[0..i], so T in its rounding counts is i + 1.  Keys j > i
have probability exactly 0 in the reference and must have it in the kernel; zeros added to a sum round nothing.

Error bound of the head kernel (per row; u = 2^-24, E = 2^-21 the relative error of the fp32 exp / log as in attention_ref.py, x_c the exact
logits, M their maximum, p_c = softmax(x)_c, S = sum_c e^(x_c - M), lse = M + ln S):
1. Logits.  x_c is an fma chain of d products from zero plus (with a bias) one add: |e_c| <= (d + 1) u (sum_k |h_k w_ck| + |b_c|).
2. logsumexp.  Perturbing every x_c by at most e = max_c |e_c| moves lse by at most e.  On top of that the fp32 evaluation of S:
   each exponent x_c - M' is one subtraction (relative u of its own size: e^(..) moves by u |x_c - M| relative, p-weighted: u sum_c p_c |x_c - M|),
   each exp is E relative, the Vlm positive terms are summed in some order ((Vlm - 1) u relative), and a running sum that follows a running
   maximum is rescaled -- one exp and one multiply, E + 2u relative -- at most once per column tile of 64 and once per level of a 16-way merge:
   n_resc = ceil(Vlm / 64) + 4.  A relative error r of S is an absolute error r of ln S (to first order; r < 1e-3 here).  Then ln itself
   (E |ln S|) and the add M + ln S (u |lse|).
       err(lse) <= e + u sum_c p_c |x_c - M| + E + (Vlm - 1) u + n_resc (E + 2u) + E |ln S| + u |lse|
3. The final subtraction: err(lp) <= |e_target| + err(lse) + u |lp|.
The mean error is not bounded separately: the terms above are dominated by the logit chain bound, which attention_ref's sigma treats.
"""
import numpy as np

import attention_ref as AR

U32 = 2.0 ** -24
E_EXP = 2.0 ** -21
NEG = -np.inf


# ---- causal attention ------------------------------------------------------------------------------------------------------------------------
def causal_head_reference(q, k, v, scale):
    """One (sequence, head): q, k, v [T][hd] -> ctx, bound, sigma [T][hd] (float64); row i sees keys 0 .. i only."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    T, hd = k.shape
    ctx, bound, sigma = (np.zeros((T, hd)) for _ in range(3))
    for i in range(T):
        z = (q[i: i + 1] @ k[: i + 1].T) * scale
        mag = np.abs(q[i: i + 1]) @ np.abs(k[: i + 1]).T
        ctx[i], bound[i], sigma[i] = (a[0] for a in AR.softmax_pv_bounds("fp32", z, mag, v[: i + 1], scale, hd))
    return ctx, bound, sigma


def masked_full_attention(q, k, v, scale):
    """full attention over all T keys with the upper triangle of the scores at -inf (float64)"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    T = k.shape[0]
    z = (q @ k.T) * scale
    z = np.where(np.arange(T)[None, :] <= np.arange(T)[:, None], z, NEG)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)) @ v


def causal_reference(qkv, lens, n_heads, scale):
    """what attention_ref.check takes: (packed row indices, head, ctx, bound, sigma) for every (sequence, head) of packed qkv [rows][3 d]"""
    qkv = np.asarray(qkv, np.float32)
    d = qkv.shape[1] // 3
    hd = d // n_heads
    out = []
    for r0, T in AR.utterances(qkv.shape[0], len(lens), lens):
        x = qkv[r0: r0 + T]
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            out.append((r0 + np.arange(T), h) + causal_head_reference(x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs], scale))
    return out


# ---- head ----------------------------------------------------------------------------------------------------------------------------------------
def head_logp_reference(h, W, b, targets=None):
    """h [rows][d], W [V][d], b [V] or None -> (lp, bound): for targets [rows] the [rows] arrays, for targets None the [rows][V] arrays of EVERY
    target (float64)"""
    h, W = np.asarray(h, np.float64), np.asarray(W, np.float64)
    rows, d = h.shape
    V = W.shape[0]
    x = h @ W.T
    mag = np.abs(h) @ np.abs(W).T
    if b is not None:
        x = x + np.asarray(b, np.float64)
        mag = mag + np.abs(np.asarray(b, np.float64))
    e_c = (d + 1) * U32 * mag
    M = x.max(axis=1, keepdims=True)
    ex = np.exp(x - M)
    S = ex.sum(axis=1, keepdims=True)
    p = ex / S
    lse = M + np.log(S)
    n_resc = -(-V // 64) + 4
    err_lse = (e_c.max(axis=1, keepdims=True) + U32 * (p * np.abs(x - M)).sum(axis=1, keepdims=True) + E_EXP + (V - 1) * U32 + n_resc * (E_EXP + 2 * U32)
               + E_EXP * np.abs(np.log(S)) + U32 * np.abs(lse))
    lp = x - lse
    bound = e_c + err_lse + U32 * np.abs(lp)
    if targets is None:
        return lp, bound
    t = np.asarray(targets)
    r = np.arange(rows)
    return lp[r, t], bound[r, t]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _ln(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    var = (xc * xc).mean(axis=-1, keepdims=True)
    return xc / np.sqrt(var + x.dtype.type(eps)) * g + b


def token_logp(W, cfg, ids, dtype=np.float64, prefix="", all_targets=False):
    """lp [P] of one string under the model W (dict of arrays), every operation in `dtype` (float64: the reference; float32: the yardstick).
    None when the string does not fit max_positions.  all_targets: the whole [P][Vlm] log-softmax instead of the targets' entries."""
    ids = [int(t) for t in ids]
    n, end = len(ids), 1 if cfg.eos_id >= 0 else 0
    P = n + end
    if P > cfg.max_positions:
        return None
    if P == 0:
        return np.zeros(0, dtype)
    t = cfg.transformer
    d, H = t.hidden_size, t.num_heads
    hd = d // H
    eps = t.layer_norm_eps if t.layer_norm_eps > 0 else 1e-5
    w = lambda name: np.asarray(W[prefix + name], dtype)
    lin = lambda x, name: x @ w(name + ".weight").T + w(name + ".bias")
    xin = ([cfg.bos_id] + ids)[:P]
    tgt = (ids + [cfg.eos_id])[:P]
    x = w("tok_emb_.weight")[xin] + w("pos_emb_.weight")[:P]
    if cfg.has_emb_norm:
        x = _ln(x, w("emb_norm_.weight"), w("emb_norm_.bias"), eps)
    scale = dtype(1.0) / np.sqrt(dtype(hd))
    causal = np.arange(P)[None, :] <= np.arange(P)[:, None]
    for l in range(t.num_layers):
        p = f"layers_.{l}."

        def attn(y):
            q, k, v = (lin(y, p + "mha_." + nm).reshape(P, H, hd).transpose(1, 0, 2) for nm in ("q_proj", "k_proj", "v_proj"))
            z = (q @ k.transpose(0, 2, 1)) * scale
            z = np.where(causal[None], z, dtype(NEG))
            e = np.exp(z - z.max(axis=-1, keepdims=True))
            a = e / e.sum(axis=-1, keepdims=True)
            return lin((a @ v).transpose(1, 0, 2).reshape(P, d), p + "mha_.out_proj")

        ffn = lambda y: lin(np.maximum(lin(y, p + "fc1_"), dtype(0)), p + "fc2_")
        n1 = lambda y: _ln(y, w(p + "norm1_.weight"), w(p + "norm1_.bias"), eps)
        n2 = lambda y: _ln(y, w(p + "norm2_.weight"), w(p + "norm2_.bias"), eps)
        if t.pre_ln:
            x = x + attn(n1(x))
            x = x + ffn(n2(x))
        else:
            x = n1(x + attn(x))
            x = n2(x + ffn(x))
    if t.has_final_norm:
        x = _ln(x, w("final_norm_.weight"), w("final_norm_.bias"), eps)
    logits = x @ (w("tok_emb_.weight") if cfg.tied_head else w("lm_head_.weight")).T
    if not cfg.tied_head and prefix + "lm_head_.bias" in W:
        logits = logits + w("lm_head_.bias")
    M = logits.max(axis=-1, keepdims=True)
    lse = M[:, 0] + np.log(np.exp(logits - M).sum(axis=-1))
    if all_targets:
        return logits - lse[:, None]
    return logits[np.arange(P), tgt] - lse


def total_of(lp):
    """the left-to-right fp32 sum"""
    t = np.float32(0.0)
    for x in np.asarray(lp, np.float32):
        t = np.float32(t + x)
    return t


# ---- re-ranking --------------------------------------------------------------------------------------------------------------------------------
def nlm_order(am, nlm, lens, ok, alpha, beta):
    """The rule of pk_nbest_rescore_nlm on one list -> (order, combined by slot): combined = am + ((alpha * nlm) + (beta * len)) in four
    separately rounded fp32 operations; stable, descending; a slot with ok = 0 or a NaN combined goes last with -inf; alpha = beta = 0 is the
    identity with combined = am."""
    f = np.float32
    am = np.asarray(am, f)
    N = len(am)
    if f(alpha) == 0 and f(beta) == 0:
        return list(range(N)), am.copy()
    comb, cls = np.zeros(N, f), [0] * N
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(N):
            a = f(f(alpha) * f(nlm[j]))
            b = f(f(beta) * f(lens[j]))
            c = f(am[j] + f(a + b))
            cls[j] = 0 if (ok[j] and not np.isnan(c)) else 1
            comb[j] = c if cls[j] == 0 else f(NEG)
    order = sorted(range(N), key=lambda j: (cls[j], -float(comb[j]) if cls[j] == 0 else 0.0))       # (sorted is stable)
    return order, comb
