"""The bf16-MFMA band attention kernel alone (pk_diag_relpos_local_attention_bf16; kernels/attention_local_bf16.hip).

Every element against a plain float64 reference with the operands of the full bf16 kernel (attention_ref's docstring): q, k, v and the local
table Pl as the bf16 values passed, ONE biased query qu = bf16(float32(q + u)) for both score terms, the position term qu . Pl_p + c[p] with
c = Pl @ (v - u), out-of-band scores -inf.  The bound is the project's own for the bf16 kernel (attention_ref.softmax_pv_bounds / check:
per-element bound, mean <= 2 sigma, guard rows untouched, every element written, nothing non-finite); the full T in its accumulation term
instead of the band width loosens it by ~2 T 2^-24 A, negligible against its 2 2^-8 A.  Inputs are exactly representable in bf16.
Prints max(err / bound) and mean(err) / mean(sigma) per case (-s)."""
import numpy as np
import pytest

import attention_ref as ar
import local_attention_ref as lr
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

RAGGED, BF16, BAND = 2, 4, 8
PK_ERR_INVALID, PK_ERR_UNSUPPORTED = -1, -7
# one or two live keys per row; one-sided (edge tiles in which most rows of a wave have no live key); band edges on and off 32-key tile
# edges; the production windows
WINDOWS = [(0, 0), (1, 0), (0, 1), (40, 0), (0, 40), (31, 33), (70, 13), (128, 128), (256, 256)]
# one row; two tiles; a second query block of one row; shorter than the wide windows (band clipped at both ends); interior workgroups whose
# tiles all skip the mask (B = 2)
LENGTHS = [(1, 1), (1, 33), (1, 129), (1, 300), (2, 700)]
MIX = [1, 129, 33, 700, 128, 2, 300]
CASES = [(l, r, B, T, None) for l, r in WINDOWS for B, T in LENGTHS]
CASES += [(128, 128, 1, None, MIX), (70, 13, 1, None, MIX)]
CASES += [(T - 1, T + 6, 1, T, None) for T in (126, 300)]            # covering windows: the band masks nothing but j >= T


def _id(c):
    l, r, B, T, lens = c
    return f"L{l}R{r}-" + (f"lens{'-'.join(map(str, lens))}" if lens else f"B{B}xT{T}")


def reference(qkv, pl, bu, bv, H, left, right, B, lens):
    """(packed rows, head, ctx, bound, sigma) per (utterance, head), as attention_ref.check consumes them"""
    qkv, pl = ar.bf16(qkv).astype(np.float64), ar.bf16(pl).astype(np.float64)
    d = qkv.shape[1] // 3
    hd = d // H
    scale = 1.0 / np.sqrt(hd)
    out = []
    for r0, T in ar.utterances(qkv.shape[0], B, lens):
        off = np.arange(T)[None, :] - np.arange(T)[:, None]          # j - i
        band = (off <= right) & (-off <= left)
        idx = np.clip(off + left, 0, left + right)
        x = qkv[r0: r0 + T]
        for h in range(H):
            cs = slice(h * hd, (h + 1) * hd)
            q, k, v, P = x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs], pl[:, cs]
            u, vb = bu[cs].astype(np.float64), bv[cs].astype(np.float64)
            qu = ar.bf16((q + u).astype(np.float32)).astype(np.float64)
            pos = qu @ P.T + P @ (vb - u)
            pos_abs = np.abs(qu) @ np.abs(P).T + np.abs(P) @ np.abs(vb - u)
            z = np.where(band, (qu @ k.T + np.take_along_axis(pos, idx, axis=1)) * scale, -np.inf)
            mag = np.abs(qu) @ np.abs(k).T + np.take_along_axis(pos_abs, idx, axis=1)
            out.append((r0 + np.arange(T), h) + ar.softmax_pv_bounds("bf16", z, mag, v, scale, hd, live=band))
    return out


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_bf16_band_attention_vs_float64(case):
    left, right, B, T, lens = case
    n = CASES.index(case)
    hd, H, fam = (64, 128)[n % 2], 2, ar.FAMILIES[(n + n // len(LENGTHS)) % len(ar.FAMILIES)]   # (every length meets every family)
    ln = list(lens) if lens else [T] * B
    qkv, pl, bu, bv = lr.make_inputs(fam, ln, hd * H, H, left, right, 3000 + n)
    got, variant = capi.diag_relpos_local_attention_bf16(qkv, pl, bu, bv, H, left, right, B=B, lens=lens)
    assert variant == BAND | BF16 | (RAGGED if lens else 0), f"variant {variant}"
    ref = reference(qkv, pl, bu, bv, H, left, right, B, lens)
    worst, mean = ar.check("bf16", got, ref, H, qkv.shape[0], _id(case))
    print(f"\n{_id(case):>40} {fam:>6} hd{hd}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")


def test_refusals():
    def status(hd, l, r):
        qkv, pos, bu, bv = ar.make_inputs("random", [64], hd * 2, 2, 64, 7)
        try:
            capi.diag_relpos_local_attention_bf16(qkv, np.zeros((max(l + r, 0) + 1, hd * 2), np.float32), bu, bv, 2, l, r)
        except capi.PkError as e:
            return e.code
        return 0
    assert [status(hd, 8, 8) for hd in (32, 96, 64)] == [PK_ERR_UNSUPPORTED, PK_ERR_UNSUPPORTED, 0]
    assert [status(64, l, r) for l, r in ((-1, 5), (5, -1), (-2, -2), (-1, -1))] == [PK_ERR_INVALID] * 4
