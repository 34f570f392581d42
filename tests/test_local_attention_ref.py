"""CPU checks of the limited-context attention reference (tests/local_attention_ref.py).

It equals attention_ref.reference when the band covers the utterance, equals a literal masked full-matrix computation, and is
translation-invariant (row i is full attention on the slice of its band).  The existing checker (attention_ref.check), fed the local
reference, accepts the literal float64 implementation and rejects six mutants of the band rule, each on a named case."""
import numpy as np
import pytest

import attention_ref as ar
import local_attention_ref as lr


def _literal(qkv, pos_full, pos_T, bu, bv, n_heads, lens, left, right, lo_hi=None, mirror=False):
    """float64 band attention over full [T][T] score matrices: the position term gathered from the full table at offset j - i (mirror:
    i - j), -inf outside [lo_i, hi_i] = lo_hi(i, T) (default: the band).  Returns ctx [rows][d] float32."""
    qkv = np.asarray(qkv, np.float64)
    pos_full = np.asarray(pos_full, np.float64)
    bu, bv = np.asarray(bu, np.float64), np.asarray(bv, np.float64)
    d = qkv.shape[1] // 3
    hd = d // n_heads
    out = np.zeros((qkv.shape[0], d))
    for r0, T in ar.utterances(qkv.shape[0], 1, lens):
        i = np.arange(T)[:, None]
        j = np.arange(T)[None, :]
        lo, hi = (lo_hi or (lambda ii, TT: (np.maximum(0, ii - left), np.minimum(TT - 1, ii + right))))(i, T)
        inside = (j >= lo) & (j <= hi)
        o = (i - j) if mirror else (j - i)
        P = pos_full[pos_T - 1 + o]                                      # [T][T][d]: row of offset o (position -o)
        x = qkv[r0: r0 + T]
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            q, k, v = x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs]
            z = ((q + bu[cs]) @ k.T + np.einsum("ih,ijh->ij", q + bv[cs], P[:, :, cs])) / np.sqrt(hd)
            z = np.where(inside, z, -np.inf)
            e = np.exp(z - z.max(axis=1, keepdims=True))
            out[r0: r0 + T, cs] = (e / e.sum(axis=1, keepdims=True)) @ v
    return out.astype(np.float32)


def _inputs(family, lens, d, H, left, right, seed):
    """qkv, the full table (pos_T = max(lens, left + 1, right + 1)), its pos_T, the local table cut from it, bias_u, bias_v"""
    pos_T = max(max(lens), left + 1, right + 1)
    qkv, pos, bu, bv = ar.make_inputs(family, lens, d, H, pos_T, seed)
    return qkv, pos, pos_T, lr.local_table(pos, pos_T, left, right), bu, bv


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("T,left,right", [(1, 0, 0), (37, 36, 36), (50, 60, 49), (70, 69, 200)])
def test_covering_window_equals_full_reference(family, T, left, right):
    d, H = 64, 2
    qkv, pos, pos_T, pl, bu, bv = _inputs(family, [T], d, H, left, right, 11)
    full = ar.reference("fp32", qkv, pos[pos_T - T: pos_T + T - 1], bu, bv, H)
    loc = lr.reference(qkv, pl, bu, bv, H, left, right)
    for (ra, ha, ca, ba, sa), (rb, hb, cb, bb, sb) in zip(full, loc):
        assert np.array_equal(ra, rb) and ha == hb
        np.testing.assert_allclose(cb, ca, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(bb, ba, rtol=1e-9)
        np.testing.assert_allclose(sb, sa, rtol=1e-9)


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("lens,left,right", [([1, 40, 7], 0, 0), ([90], 1, 0), ([90], 0, 1), ([33, 100], 16, 16), ([120], 31, 33),
                                             ([150, 20], 70, 13)])
def test_band_reference_equals_literal_masked_matrix(family, lens, left, right):
    d, H = 64, 2
    qkv, pos, pos_T, pl, bu, bv = _inputs(family, lens, d, H, left, right, 12)
    lit = _literal(qkv, pos, pos_T, bu, bv, H, lens, left, right).astype(np.float64)
    for rows, h, ctx, bound, sigma in lr.reference(qkv, pl, bu, bv, H, left, right, lens=lens):
        np.testing.assert_allclose(ctx, lit[rows][:, h * 32: (h + 1) * 32], rtol=1e-6, atol=1e-7)
        assert np.all(bound > 0) and np.all(sigma > 0) and np.all(sigma <= bound)


@pytest.mark.parametrize("T,left,right", [(200, 16, 16), (300, 70, 13), (150, 0, 5)])
def test_band_reference_is_translation_invariant(T, left, right):
    """row i of the band = row i - lo of FULL attention over the slice [lo, hi] of its band (positions are relative)"""
    d, H = 64, 1
    qkv, pos, pos_T, pl, bu, bv = _inputs("random", [T], d, H, left, right, 13)
    _, _, ctx, _, _ = lr.reference(qkv, pl, bu, bv, H, left, right)[0]
    lo, hi = lr.band(T, left, right)
    for i in (0, 1, left, left + 1, T // 2, T - right - 1, T - 2, T - 1):
        a, b = int(lo[i]), int(hi[i])
        n = b - a + 1
        # full-attention table of an n-frame utterance: row p = offset p - (n - 1); offsets outside [-left, right] are never reached by row i
        Pw = np.full((2 * n - 1, d), 0.25, np.float32)
        for p in range(2 * n - 1):
            o = p - (n - 1)
            if -left <= o <= right:
                Pw[p] = pl[o + left]
        c, _, _ = ar.head_reference("fp32", qkv[a: b + 1, :d], qkv[a: b + 1, d: 2 * d], qkv[a: b + 1, 2 * d:], Pw, bu, bv)
        np.testing.assert_allclose(ctx[i], c[i - a], rtol=1e-12, atol=1e-14)


def _union(i, T, left, right):
    b0 = (i // 32) * 32
    return np.maximum(0, b0 - left), np.minimum(T - 1, b0 + 31 + right)


MUTANTS = {
    # name: (family, lens, left, right, literal kwargs)
    "band-one-wider-left": ("random", [160], 16, 16, dict(lo_hi=lambda i, T: (np.maximum(0, i - 17), np.minimum(T - 1, i + 16)))),
    "band-one-narrower-right": ("random", [160], 16, 16, dict(lo_hi=lambda i, T: (np.maximum(0, i - 16), np.minimum(T - 1, i + 15)))),
    "left-right-swapped": ("random", [200], 70, 13, dict(lo_hi=lambda i, T: (np.maximum(0, i - 13), np.minimum(T - 1, i + 70)))),
    "position-row-mirrored": ("pos", [160], 16, 16, dict(mirror=True)),
    "no-mask": ("random", [160], 16, 16, dict(lo_hi=lambda i, T: (np.zeros_like(i), np.full_like(i, T - 1)))),
    "union-band-per-32-row-block": ("random", [160], 16, 16, dict(lo_hi=lambda i, T: _union(i, T, 16, 16))),
}


def test_checker_accepts_the_literal_band_implementation():
    for fam in ar.FAMILIES:
        lens, left, right = [160, 33], 16, 16
        qkv, pos, pos_T, pl, bu, bv = _inputs(fam, lens, 64, 2, left, right, 14)
        got = _literal(qkv, pos, pos_T, bu, bv, 2, lens, left, right)
        ar.check("fp32", got, lr.reference(qkv, pl, bu, bv, 2, left, right, lens=lens), 2, qkv.shape[0], f"literal-{fam}", guard=False)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_checker_rejects_mutant(name):
    fam, lens, left, right, kw = MUTANTS[name]
    qkv, pos, pos_T, pl, bu, bv = _inputs(fam, lens, 64, 2, left, right, 15)
    got = _literal(qkv, pos, pos_T, bu, bv, 2, lens, left, right, **kw)
    with pytest.raises(AssertionError, match="max err / bound|mean err"):
        ar.check("fp32", got, lr.reference(qkv, pl, bu, bv, 2, left, right, lens=lens), 2, qkv.shape[0], name, guard=False)
