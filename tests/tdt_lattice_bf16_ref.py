"""Float64 reference of the bf16 TDT lattice kernel (kernels/tdt_lattice_bf16.hip; pk_diag_tdt_lattice_bf16) with a per-value error bound.

For lattice row (b, t, u), on the operands the kernel sees (z and W16 are bit-defined, so there is no operand-rounding term):

    z = bf16(relu(fl32(ep[t] + pp[u B + b]))),  W16 = bf16(wld),  logit = z . W16[n] + bld[n]
    blk = logit[blank] - lse(logit[:V]),  lab = logit[ids[u]] - lse(logit[:V]) (u < U),  dl[i] = logit[V + i] - lse(logit[V:V + D])

Error bound (u = 2^-24; |.| of reference values).

1. Logit.  B[n] = 2e-6 (|z| . |W16[n]| + |bld[n]|) + 1e-6, the form every bf16 MFMA product of the project is held to (tests/test_gpu_bf16.py,
   tests/decode_gemv_ref.py section 1).
2. A log-prob is a logit minus a log-sum-exp, and the lse moves by at most the largest move of its arguments: B[n] + max_k B[k] over the head's own
   columns, + E, the fp32 evaluation error of the lse and of the last subtraction, from the shape of the kernel's summation:
   * A label column's term e^(x_k), x_k = logit_k - M <= 0 (M the row maximum), is formed in pieces: fl(v - m) against the lane's running maximum,
     one fl(m_old - m_new) per later rescaling in the lane's chain of nb = ceil(ceil((V + D) / 64) / 4) column blocks, one fl(m_p - M) in the merge
     of the 8 partials.  Every piece y is <= 0 and they sum to x_k.  A piece costs one rounding of the difference, one of the product with
     log2(e), the constant's own 2^-25: <= 2.5 u |y| on the exponent, and the exponential itself (v_exp_f32, dexpf) <= 4 u relative:
     2.5 u |x_k| + 4 u (nb + 2) in all.  Weighted by the terms' shares p_k of the sum, |x_k| = -ln p_k - ln S <= -ln p_k (S >= 1 with the maximum
     subtracted), so sum_k p_k |x_k| <= ln N, the entropy's bound for N columns.
   * Additions: a term passes <= 31 adds inside its block's sum, one multiply and one add per later block of the chain, one multiply and <= 8
     adds in the merge: (2 nb + 40) u.
   * dlogf <= 4 u relative on |ln S| <= ln N; lse = fl(M + ln S) and out = fl(logit - lse): u (|lse| + |out|).
   E = u (6.5 ln N + 6 nb + 48) + u (|lse| + |out|).
   The duration head has N = D <= 8 columns summed in one chain by one thread with dexpf: the same expression with nb = 1 covers it.
"""
import numpy as np

from decode_gemv_ref import bf16

U32 = 2.0 ** -24


def reference(ep, pp, wld, bld, ids, n_frames, V, D, blank):
    """-> (lab, blk, dl, bound_lab, bound_blk, bound_dl): float64, flat, packed as pk_diag_tdt_lattice_bf16 packs them (without guard words)"""
    B, VD = len(n_frames), V + D
    W = bf16(wld).astype(np.float64)
    nb = -(-(-(-VD // 64)) // 4)
    out = [[] for _ in range(6)]
    row0 = 0
    for b in range(B):
        T, U = int(n_frames[b]), len(ids[b])
        s = ep[row0:row0 + T, None, :] + pp[np.arange(U + 1) * B + b][None, :, :]        # fp32 + fp32 -> fp32
        z = bf16(np.where(s > 0, s, np.float32(0))).astype(np.float64).reshape(T * (U + 1), -1)
        row0 += T
        logit = z @ W.T + bld
        Bn = 2e-6 * (z @ np.abs(W).T + np.abs(bld)) + 1e-6

        def head(lo, hi, nbk):
            x = logit[:, lo:hi]
            m = x.max(1, keepdims=True)
            lse = m + np.log(np.exp(x - m).sum(1, keepdims=True))
            lp = x - lse
            e = U32 * (6.5 * np.log(hi - lo) + 6 * nbk + 48) + U32 * (np.abs(lse) + np.abs(lp))
            return lp, Bn[:, lo:hi] + Bn[:, lo:hi].max(1, keepdims=True) + e
        lp, bl = head(0, V, nb)
        dp, bd = head(V, VD, 1)
        cells = np.arange(T * (U + 1)).reshape(T, U + 1)
        at, col = cells[:, :U].ravel(), np.tile(np.asarray(ids[b], np.int64), T)
        for k, v in enumerate((lp[at, col], lp[:, blank], dp.ravel(), bl[at, col], bl[:, blank], bd.ravel())):
            out[k].append(v)
    return tuple(np.concatenate(o) for o in out)
