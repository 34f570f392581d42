"""Float64 reference of the encoder's relative-position attention and a per-element checker for its two GPU kernels.

The reference is written from the model's definition (ConformerAttention::rel_position_attention, src/encoder.cpp:135-171, with rel_shift
:85-109), not from the oracle or the kernels:

    S = (q + u) K^T + rel_shift((q + v) P^T),   ctx = softmax(S / sqrt(hd)) V        per (utterance, head)

where P is the window pos[pos_T - T : pos_T + T - 1] of a table built for pos_T >= T frames.  rel_shift is applied literally (pad, reshape,
drop, reshape) whenever every row of an utterance is checked; when only a sample of rows is checked the closed form p = j - i + T - 1 is
gathered instead (tests/test_attention_ref.py proves the two equal).  For the bf16 kernel the operands are those of the specification above
oracle/pk_oracle.c attention(): q, k, v and P as the bf16 values passed, ONE biased query qu = bf16(float32(q + u)) for both score terms,
and the position term qu . P_p + c[p] with c[p] = (v - u) . P_p in float64.  Its two remaining roundings -- probabilities rounded to bf16
in the numerator and ctx stored as bf16 -- are not modelled; they are part of the bound.

Error bound (per element of ctx; u = 2^-24, u16 = 2^-8 the unit roundoffs of fp32 and bf16, z_j the exact scaled scores of one query row,
p_j its softmax, A_c = sum_j p_j |v_jc| >= |ctx_c|):

1. Score errors.  The kernel's scaled score is z_j + e_j.  Each dot product of hd terms accumulated in fp32 in any order is off by at most
   (hd - 1) u sum|terms| (bf16 x bf16 products are exact in fp32; fp32 x fp32 products add one rounding each); forming q + u (q + v) in
   fp32, adding c, adding content and position and the scale multiply add a few more roundings.  So, with C_j = |qu| . |k_j| + |qp| . |P_p|
   (+ |v - u| . |P_p| for the bf16 kernel's c term),  |e_j| <= d_j = scale (hd + 2) u C_j + 8 u (|z_j| + max_k |z_k|) + 2^-21, the middle
   term covering the relative rounding of the scale constant, of the multiply and of the subtraction of the running maximum, the last the
   relative error of the exponential (hardware exp2 or the fp32 polynomial, a few ulp; ln(1 + eps) <= eps).
   The perturbed probabilities are p_j e^{e_j} / E with E = sum_k p_k e^{e_k}, so |ln E| <= L = ln sum_k p_k e^{d_k} and
   |p~_j - p_j| <= p_j |e^{e_j - ln E} - 1| <= p_j (d_j + L) e^{d_j + L}.  Score term:  sum_j p_j (d_j + L) e^{d_j + L} |v_jc|.
2. bf16 kernel, the remaining roundings: probabilities rounded to bf16 relative to the running maximum (<= u16 relative each: u16 A),
   ctx stored as bf16 (<= u16 |ctx| <= u16 A), the P V accumulation over T keys in fp32 (T u A), the normaliser's fp32 sum over T keys
   (T u A), the online rescales (two roundings per 32-key tile: T/16 u A), rcp and the final multiply (2^-21 A + u A).
   Bound: score term + (2 u16 + (2T + T/16 + 8) u + 2^-21) A.
3. fp32 kernel: no bf16 roundings; the normaliser (T u), the division (u), the P V accumulation (T u + one rounding per product).
   Bound: score term + ((2T + 8) u + 2^-21) A.
4. Both: probabilities below 2^-126 relative to the row maximum may be flushed to zero: an absolute T 2^-120 max|v| is added.

Mean bound.  The bound above lets every rounding error take its extreme with a common sign.  Under the standard probabilistic model
(independent, zero-mean errors spread over their intervals) a single rounding of x to a grid of relative spacing 2 eps has E|err| <= eps |x| / 2
and a sum of n errors of bound b each has rms <= b sqrt(n / 3); E|X| <= rms X.  So per element
    sigma = score term (with (hd + 2) replaced by sqrt((hd + 2) / 3) in d_j) + sqrt(n_acc / 3) u A + 2^-21 A + floor
          + [bf16] u16 |ctx| / 2 + u16 sqrt(sum_j p_j^2 v_jc^2) / sqrt(3)
with n_acc the roundings counted in 2. / 3.  The checker asserts mean(err) <= 2 mean(sigma) over all checked elements (the factor 2 leaves
room for the spread of an empirical mean of a few hundred elements); with a spread softmax sigma is several times smaller than the bound,
so a systematic relative error of a fraction of a percent -- inside every per-element bound -- still fails.
"""
import numpy as np

U32 = 2.0 ** -24
U16 = 2.0 ** -8
E_EXP = 2.0 ** -21
GUARD_ROWS = 128
UNWRITTEN = {"fp32": 0x7FC5A5A5, "bf16": 0x7FC50000}


def bf16(x):
    """round to the nearest bf16 (ties to even), returned as float32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def rel_shift(x):
    """src/encoder.cpp:85-109 literally, on [..., n, 2n - 1]: pad one zero column in front, view as [2n][n], drop the first row,
    view as [n][2n - 1], keep the first n columns"""
    n, p = x.shape[-2:]
    lead = x.shape[:-2]
    x = np.concatenate([np.zeros(lead + (n, 1), x.dtype), x], axis=-1)
    x = x.reshape(lead + (p + 1, n))[..., 1:, :].reshape(lead + (n, p))
    return x[..., :n]


def band_gather(x, rows, T):
    """the closed form of rel_shift for the query rows `rows`: out[r][j] = x[r][j - rows[r] + T - 1]"""
    idx = np.arange(T)[None, :] - np.asarray(rows)[:, None] + T - 1
    return np.take_along_axis(x, idx, axis=1)


def head_reference(kind, q, k, v, Pw, u, vb, rows=None, scale=None):
    """One (utterance, head).  q, k, v [T][hd], Pw [2T - 1][hd] (the window), u / vb [hd]; rows: query rows to evaluate (None: all, literal
    rel_shift).  Returns ctx, bound, sigma [n_rows][hd] (float64)."""
    q, k, v, Pw = (np.asarray(a, np.float64) for a in (q, k, v, Pw))
    u, vb = np.asarray(u, np.float64), np.asarray(vb, np.float64)
    T, hd = k.shape
    scale = 1.0 / np.sqrt(hd) if scale is None else scale
    I = np.arange(T) if rows is None else np.asarray(rows)
    if kind == "bf16":
        qu = bf16((q[I] + u).astype(np.float32)).astype(np.float64)
        qp = qu
        c = Pw @ (vb - u)
        c_abs = np.abs(Pw) @ np.abs(vb - u)
    else:
        qu, qp = q[I] + u, q[I] + vb
        c = c_abs = 0.0
    pos = qp @ Pw.T + c
    pos_abs = np.abs(qp) @ np.abs(Pw).T + c_abs
    shift = (lambda x: rel_shift(x)) if rows is None else (lambda x: band_gather(x, I, T))
    z = (qu @ k.T + shift(pos)) * scale
    mag = np.abs(qu) @ np.abs(k).T + shift(pos_abs)
    return softmax_pv_bounds(kind, z, mag, v, scale, hd)


def softmax_pv_bounds(kind, z, mag, v, scale, hd, live=None):
    """ctx = softmax(z) v of one (utterance, head) with the bound and sigma of the docstring above.  z [n_rows][T] the exact scaled scores,
    mag [n_rows][T] the sums of |terms| of their dot products (C_j), v [T][hd].  live (boolean [n_rows][T], None: every key): False marks a
    key whose score was REPLACED by a mask constant (z holds that constant) -- its probability is exactly 0 in the reference and in any
    implementation, so it is left out of the |z| terms of the bound (a constant of 1e9 there would make the bound pass anything).
    Returns ctx, bound, sigma [n_rows][hd] (float64)."""
    T = v.shape[0]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    va = np.abs(v)
    ctx = p @ v
    A = p @ va
    az = np.abs(z)
    if live is not None:
        az, mag = np.where(live, az, 0.0), np.where(live, mag, 0.0)
    zabs = az + az.max(axis=1, keepdims=True)

    def score_term(n_dot):
        d = scale * n_dot * U32 * mag + 8 * U32 * zabs + E_EXP
        L = np.log((p * np.exp(d)).sum(axis=1, keepdims=True))
        return (p * (d + L) * np.exp(d + L)) @ va

    floor = T * 2.0 ** -120 * (va.max() if va.size else 0.0)
    if kind == "bf16":
        n_acc = 2 * T + T / 16 + 8
        bound = score_term(hd + 2) + (2 * U16 + n_acc * U32 + E_EXP) * A + floor
        sigma = (score_term(np.sqrt((hd + 2) / 3)) + (np.sqrt(n_acc / 3) * U32 + E_EXP) * A + floor
                 + U16 / 2 * np.abs(ctx) + U16 / np.sqrt(3) * np.sqrt((p * p) @ (v * v)))
    else:
        n_acc = 2 * T + 8
        bound = score_term(hd + 2) + (n_acc * U32 + E_EXP) * A + floor
        sigma = score_term(np.sqrt((hd + 2) / 3)) + (np.sqrt(n_acc / 3) * U32 + E_EXP) * A + floor
    return ctx, bound, sigma


def utterances(rows_total, B, lens):
    """[(first packed row, T)] of a uniform (lens None) or packed ragged batch"""
    if lens is None:
        T = rows_total // B
        return [(b * T, T) for b in range(B)]
    off = np.concatenate([[0], np.cumsum(lens)])
    return [(int(off[b]), int(lens[b])) for b in range(len(lens))]


def sample_rows(T, n):
    """n query rows of a T-frame utterance for the sampled reference: the ends, the 32- / 128-row block edges, the rest random"""
    if n is None or n >= T:
        return None
    edges = {0, 1, T - 2, T - 1}
    for b in (31, 32, 33, 127, 128, 129, 255, 256):
        for e in (b, T - 1 - b):
            if 0 <= e < T:
                edges.add(e)
    rng = np.random.default_rng(T)
    rest = rng.choice(T, size=max(0, n - len(edges)), replace=False)
    return np.unique(np.concatenate([sorted(edges), rest]).astype(np.int64))


def reference(kind, qkv, pos, bias_u, bias_v, n_heads, B=1, lens=None, max_rows=None, head_u=None, scale=None):
    """ctx / bound / sigma of every checked element: a list of (packed row indices, head, ctx, bound, sigma).  head_u(h) -> the u of head h
    (for the CPU mutants only)."""
    qkv = np.asarray(qkv, np.float32)
    pos = np.asarray(pos, np.float32)
    d = qkv.shape[1] // 3
    hd = d // n_heads
    pos_T = (pos.shape[0] + 1) // 2
    if kind == "bf16":
        qkv, pos = bf16(qkv), bf16(pos)
    out = []
    for r0, T in utterances(qkv.shape[0], B, lens):
        rows = sample_rows(T, max_rows)
        Pw = pos[pos_T - T: pos_T + T - 1]
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            x = qkv[r0: r0 + T]
            u = bias_u[cs] if head_u is None else head_u(h)
            ctx, bound, sigma = head_reference(kind, x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs], Pw[:, cs], u, bias_v[cs], rows, scale)
            out.append((r0 + (np.arange(T) if rows is None else rows), h, ctx, bound, sigma))
    return out


def check(kind, got, ref, n_heads, rows_total, what, guard=True):
    """Compare the kernel's ctx (with its guard rows when guard) with reference(...) output.  Asserts every valid element was written,
    no guard row was touched, err <= bound everywhere and mean(err) <= 2 mean(sigma).  Returns (max err / bound, mean err / mean sigma)."""
    got = np.asarray(got, np.float32)
    d = got.shape[1]
    hd = d // n_heads
    valid = got[:rows_total]
    if guard:
        assert got.shape[0] == rows_total + GUARD_ROWS, f"{what}: {got.shape[0]} rows returned, {rows_total} + {GUARD_ROWS} expected"
        g = got[rows_total:].view(np.uint32)
        bad = np.argwhere(g != UNWRITTEN[kind])
        assert bad.size == 0, f"{what}: guard row {bad[0][0]} column {bad[0][1]} was written ({bad.shape[0]} elements)"
    miss = np.argwhere(valid.view(np.uint32) == UNWRITTEN[kind]) if guard else np.zeros((0, 2), int)
    assert miss.size == 0, f"{what}: ctx row {miss[0][0]} column {miss[0][1]} was never written ({miss.shape[0]} elements)"
    nonfinite = np.argwhere(~np.isfinite(valid))
    assert nonfinite.size == 0, f"{what}: ctx row {nonfinite[0][0]} column {nonfinite[0][1]} is {valid[tuple(nonfinite[0])]}"
    worst, worst_at, err_sum, sig_sum, n = 0.0, None, 0.0, 0.0, 0
    for rows, h, ctx, bound, sigma in ref:
        err = np.abs(valid[rows][:, h * hd: (h + 1) * hd].astype(np.float64) - ctx)
        r = err / bound
        i = np.unravel_index(np.argmax(r), r.shape)
        if r[i] > worst:
            worst, worst_at = float(r[i]), (int(rows[i[0]]), h, int(i[1]), float(valid[rows[i[0]], h * hd + i[1]]), float(ctx[i]), float(bound[i]))
        err_sum += err.sum()
        sig_sum += sigma.sum()
        n += err.size
    mean_ratio = float(err_sum / max(sig_sum, 1e-300))
    assert worst <= 1.0, (f"{what}: max err / bound = {worst:.3g} at row {worst_at[0]} head {worst_at[1]} dv {worst_at[2]}: "
                          f"got {worst_at[3]!r}, reference {worst_at[4]!r}, bound {worst_at[5]:.3g}")
    assert mean_ratio <= 2.0, f"{what}: mean err = {mean_ratio:.3g} x mean sigma (bound: 2)"
    return worst, mean_ratio


# ---- inputs: every value exactly representable in bf16 (the bf16 kernel's host rounding is then the identity) ---------------------------
FAMILIES = ("random", "large", "key", "pos", "c")
KEY_PEAKS = (0, -1, 31, 32, 127, 128)          # key-peaked family: the peak key of head h (-1: the last valid key)
POS_OFFSETS = (0, 1, -1, "T-1", "-(T-1)")      # position-peaked family: the offset j - i the P rows of head h select


def make_inputs(family, lens, d, n_heads, pos_T, seed):
    """qkv [sum lens][3 d], pos [2 pos_T - 1][d], bias_u, bias_v [d] for a batch of utterances of lens[b] frames (uniform: all equal).
    random: near-uniform softmax.  large: |scores| up to ~60 (most exponentials underflow, the row maximum matters).  key: one key per
    (utterance, head) -- the first, the last valid, or 31 / 32 / 127 / 128 -- scores ~12 above the rest.  pos: content near zero, the P rows of
    one offset j - i (0, +-1, +-(T-1)) aligned with the queries.  c: u != v and (v - u) . P_p dominates the scores."""
    rng = np.random.default_rng(seed)
    hd = d // n_heads
    rows = int(sum(lens))
    P = 2 * pos_T - 1
    N = lambda s, *shape: rng.standard_normal(shape) * s
    w = np.where(rng.random(d) < 0.5, -1.0, 1.0)            # +-1 per column: one direction per head
    q, k, v = N(0.5, rows, d), N(0.5, rows, d), N(1.0, rows, d)
    pos = N(0.5, P, d)
    bu, bv = N(0.1, d), N(0.1, d)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    if family == "large":
        q, k, pos = N(4.0, rows, d), N(4.0, rows, d), N(1.0, P, d)
    elif family == "key":
        q = w + N(0.05, rows, d)
        k, pos, bu, bv = N(0.05, rows, d), N(0.05, P, d), N(0.02, d), N(0.02, d)
        gamma = 12.0 / np.sqrt(hd)                           # peak score (w . w) gamma / sqrt(hd) = 12
        for b, T in enumerate(lens):
            for h in range(n_heads):
                j = KEY_PEAKS[(h + seed) % len(KEY_PEAKS)]
                j = T - 1 if j < 0 or j >= T else j
                k[off[b] + j, h * hd: (h + 1) * hd] = w[h * hd: (h + 1) * hd] * gamma
    elif family == "pos":
        q = w + N(0.05, rows, d)
        k, pos, bu, bv = N(0.02, rows, d), N(0.05, P, d), N(0.02, d), N(0.02, d)
        gamma = 10.0 / np.sqrt(hd)
        for T in sorted(set(int(t) for t in lens)):
            for h in range(n_heads):
                o = POS_OFFSETS[(h + seed) % len(POS_OFFSETS)]
                o = {"T-1": T - 1, "-(T-1)": -(T - 1)}.get(o, o)
                p = pos_T - T + o + T - 1                    # table row of offset o in the window of a T-frame utterance
                if 0 <= p < P:
                    pos[p, h * hd: (h + 1) * hd] = w[h * hd: (h + 1) * hd] * gamma
    elif family == "c":
        q, k = N(0.05, rows, d), N(0.1, rows, d)
        pos = N(1.0, P, d)
        bu, bv = N(0.02, d), 3.0 * w + N(0.1, d)
    qkv = np.concatenate([q, k, v], axis=1)
    return bf16(qkv), bf16(pos), bf16(bu), bf16(bv)
