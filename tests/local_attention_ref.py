"""Float64 reference of the limited-context ("local", band) relative-position attention, in the format attention_ref.check consumes.

Definition (include/parakeet_amd.h pk_model_set_attention_context): query row i of a T-frame utterance attends to the keys j of its band
[lo_i, hi_i] = [max(0, i - left), min(T - 1, i + right)] only:

    S[i][j] = ((q_i + u) . k_j + (q_i + v) . Pl[j - i + left]) / sqrt(hd)      j in [lo_i, hi_i]
    ctx_i   = sum_j softmax_j(S[i][.]) v_j                                     (keys outside the band: weight exactly 0)

Pl is the local table [left + right + 1][d]; row r holds the projected position i - j = left - r, i.e. row j - i + left.

Error bound: attention_ref's derivation row by row, with the softmax extent T of a row replaced by its band width n_i = hi_i - lo_i + 1
(the fp32 sums of the normaliser and of the P V chain run over the window columns, but out-of-band terms are exact zeros and add no rounding).
Output mode 1 (ctx stored as bf16, the engine's gemm_bf16 mode) adds one bf16 rounding of ctx (U16 |ctx|) and the hardware reciprocal of the
normaliser (E_EXP A); sigma gets U16 / 2 |ctx|.
"""
import numpy as np

import attention_ref as ar


def band(T, left, right, rows=None):
    """lo, hi [n] of the query rows `rows` (None: all)"""
    I = np.arange(T) if rows is None else np.asarray(rows)
    return np.maximum(0, I - left), np.minimum(T - 1, I + right)


def head_reference(q, k, v, Pl, u, vb, left, right, rows=None, out_mode=0, scale=None, chunk=128):
    """One (utterance, head).  q, k, v [T][hd], Pl [left + right + 1][hd], u / vb [hd]; rows: query rows to evaluate (None: all).
    Returns ctx, bound, sigma [n_rows][hd] (float64)."""
    q, k, v, Pl = (np.asarray(a, np.float64) for a in (q, k, v, Pl))
    u, vb = np.asarray(u, np.float64), np.asarray(vb, np.float64)
    T, hd = k.shape
    scale = 1.0 / np.sqrt(hd) if scale is None else scale
    I_all = np.arange(T) if rows is None else np.asarray(rows)
    W = left + right + 1
    offs = np.arange(-left, right + 1)
    outs = []
    for c0 in range(0, len(I_all), chunk):
        I = I_all[c0: c0 + chunk]
        J = I[:, None] + offs[None, :]                               # [n][W] key of window column w (offset w - left)
        ok = (J >= 0) & (J < T)
        Jc = np.clip(J, 0, T - 1)
        qu, qp = q[I] + u, q[I] + vb
        kw, vw = k[Jc], v[Jc]                                        # [n][W][hd]
        z = (np.einsum("nh,nwh->nw", qu, kw) + qp @ Pl.T) * scale
        mag = np.einsum("nh,nwh->nw", np.abs(qu), np.abs(kw)) + np.abs(qp) @ np.abs(Pl).T
        z = np.where(ok, z, -np.inf)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        va = np.abs(vw) * ok[:, :, None]
        ctx = np.einsum("nw,nwh->nh", p, vw)
        A = np.einsum("nw,nwh->nh", p, va)
        zf = np.where(ok, z, 0.0)
        zabs = np.abs(zf) + np.abs(zf).max(axis=1, keepdims=True)
        nb = ok.sum(axis=1, keepdims=True).astype(np.float64)        # band width of each row

        def score_term(n_dot):
            dd = scale * n_dot * ar.U32 * mag + 8 * ar.U32 * zabs + ar.E_EXP
            L = np.log((p * np.exp(dd)).sum(axis=1, keepdims=True))
            return np.einsum("nw,nwh->nh", p * (dd + L) * np.exp(dd + L), va)

        floor = nb * 2.0 ** -120 * (np.abs(v).max() if v.size else 0.0)
        n_acc = 2 * nb + 8
        bound = score_term(hd + 2) + (n_acc * ar.U32 + ar.E_EXP) * A + floor
        sigma = score_term(np.sqrt((hd + 2) / 3)) + (np.sqrt(n_acc / 3) * ar.U32 + ar.E_EXP) * A + floor
        if out_mode == 1:
            bound = bound + ar.U16 * np.abs(ctx) + ar.E_EXP * A
            sigma = sigma + ar.U16 / 2 * np.abs(ctx)
        outs.append((ctx, bound, sigma))
        del kw, vw
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


def reference(qkv, pos_local, bias_u, bias_v, n_heads, left, right, B=1, lens=None, max_rows=None, out_mode=0, scale=None):
    """(packed row indices, head, ctx, bound, sigma) of every checked element, as attention_ref.reference returns them"""
    qkv = np.asarray(qkv, np.float32)
    Pl = np.asarray(pos_local, np.float32)
    assert Pl.shape[0] == left + right + 1
    d = qkv.shape[1] // 3
    hd = d // n_heads
    out = []
    for r0, T in ar.utterances(qkv.shape[0], B, lens):
        rows = ar.sample_rows(T, max_rows)
        x = qkv[r0: r0 + T]
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            ctx, bound, sigma = head_reference(x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs], Pl[:, cs], bias_u[cs], bias_v[cs], left, right,
                                               rows, out_mode, scale)
            out.append((r0 + (np.arange(T) if rows is None else rows), h, ctx, bound, sigma))
    return out


def local_table(pos_full, pos_T, left, right):
    """the local table [left + right + 1][d] cut from a full table [2 pos_T - 1][d] (row p = position pos_T - 1 - p): row r = position left - r.
    Rows whose position the full table does not hold are filled with a constant pattern (they belong to offsets no pair of a T <= pos_T
    utterance reaches)."""
    d = pos_full.shape[1]
    out = np.full((left + right + 1, d), 0.375, np.float32)
    for r in range(left + right + 1):
        p = pos_T - 1 - (left - r)
        if 0 <= p < pos_full.shape[0]:
            out[r] = pos_full[p]
    return out


def make_inputs(family, lens, d, n_heads, left, right, seed):
    """attention_ref.make_inputs for a local window: qkv, the local table [left + right + 1][d], bias_u, bias_v.  The full table is made for
    pos_T = max(max(lens), left + 1, right + 1) and cut (local_table), so every family's peaks keep their meaning (the key family's peaks at
    keys 0 / 31 / 32 / 127 / 128 / last lie outside most rows' bands)."""
    pos_T = max(max(int(t) for t in lens), left + 1, right + 1)
    qkv, pos, bu, bv = ar.make_inputs(family, lens, d, n_heads, pos_T, seed)
    return qkv, local_table(pos, pos_T, left, right), bu, bv
