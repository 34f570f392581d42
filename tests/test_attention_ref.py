"""The float64 attention reference and its checker (tests/attention_ref.py) have power: CPU only.

* the literal rel_shift equals the closed-form gather p = j - i + T - 1;
* ACCEPT: an independent float32 implementation built to differ from the reference where the bf16 GPU kernel differs (32-key tiles with an
  online softmax, probabilities rounded to bf16 relative to the running maximum, an unrounded normaliser, ctx stored as bf16) passes the bf16
  bound on every input family; a plain float32 implementation passes the fp32 bound;
* REJECT: eight deliberately wrong variants of that implementation each fail on a named case.
"""
import numpy as np
import pytest
import torch

import attention_ref as ar
import torch_ref


def tiled_f32(qkv, pos, bias_u, bias_v, n_heads, lens, mut=None):
    """float32, 32-key tiles, online softmax, bf16 probabilities and ctx -- with optional mutation `mut`"""
    f = np.float32
    qkv, pos, bias_u, bias_v = (np.asarray(a, f) for a in (qkv, pos, bias_u, bias_v))
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    hd, pos_T = d // n_heads, (pos.shape[0] + 1) // 2
    out = np.zeros((rows, d), f)
    scale = f(1.0 / np.sqrt(d if mut == "scale_d" else hd))
    for r0, T in ar.utterances(rows, 1, lens):
        shift = 0 if mut == "window_unshifted" else pos_T - T
        Pw = pos[shift: shift + 2 * T - 1]
        Tk = T + 1 if mut == "extra_key" else T                      # one key past T, a copy of key T - 1 (clamped load, mask missed)
        kr = np.minimum(np.arange(Tk), T - 1)
        i = np.arange(T)[:, None]
        poff = {"pos_minus1": -1, "pos_plus1": 1}.get(mut, 0)
        pidx = np.clip(np.arange(Tk)[None, :] - i + T - 1 + poff, 0, 2 * T - 2)
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            x = qkv[r0: r0 + T]
            q, k, v = x[:, cs], x[:, d:][:, cs][kr], x[:, 2 * d:][:, cs][kr]
            u = bias_u[((h + 1) % n_heads) * hd:][:hd] if mut == "head_u_next" else bias_u[cs]
            qu = ar.bf16(q + u)
            c = Pw[:, cs] @ (bias_v[cs] - u)
            if mut == "no_c":
                c = np.zeros_like(c)
            G = qu @ Pw[:, cs].T + c[None, :]
            S = ((qu @ k.T) + np.take_along_axis(G, pidx, axis=1)) * scale
            m = np.full((T, 1), -np.inf, f)
            l = np.zeros((T, 1), f)
            O = np.zeros((T, hd), f)
            for t in range(0, Tk, 32):
                s = S[:, t: t + 32]
                m_new = np.maximum(m, s.max(axis=1, keepdims=True))
                alpha = np.exp(m - m_new)
                e = np.exp(s - m_new)
                l = l * alpha + e.sum(axis=1, keepdims=True, dtype=f)
                if not (mut == "tile_not_rescaled" and t == 32):
                    O = O * alpha
                O = O + ar.bf16(e) @ v[t: t + 32]
                m = m_new
            out[r0: r0 + T, cs] = ar.bf16(O / l)
    if mut == "swap_utterances":                                     # two equal-length utterances' rows exchanged in the packed batch
        off = np.concatenate([[0], np.cumsum(lens)])
        a, b = [i for i in range(len(lens)) if lens[i] == lens[1]][:2]
        ra, rb = slice(off[a], off[a + 1]), slice(off[b], off[b + 1])
        out[ra], out[rb] = out[rb].copy(), out[ra].copy()
    return out


def plain_f32(qkv, pos, bias_u, bias_v, n_heads, lens):
    """float32 throughout, the whole score row at once, exact-order-agnostic BLAS sums"""
    f = np.float32
    rows, d = qkv.shape[0], qkv.shape[1] // 3
    hd, pos_T = d // n_heads, (pos.shape[0] + 1) // 2
    out = np.zeros((rows, d), f)
    for r0, T in ar.utterances(rows, 1, lens):
        Pw = pos[pos_T - T: pos_T + T - 1]
        pidx = np.arange(T)[None, :] - np.arange(T)[:, None] + T - 1
        for h in range(n_heads):
            cs = slice(h * hd, (h + 1) * hd)
            x = qkv[r0: r0 + T]
            q, k, v = x[:, cs], x[:, d:][:, cs], x[:, 2 * d:][:, cs]
            S = (q + bias_u[cs]) @ k.T + np.take_along_axis((q + bias_v[cs]) @ Pw[:, cs].T, pidx, axis=1)
            S = S * f(1.0 / np.sqrt(hd))
            e = np.exp(S - S.max(axis=1, keepdims=True))
            out[r0: r0 + T, cs] = (e / e.sum(axis=1, keepdims=True)) @ v
    return out


def run_check(kind, got, qkv, pos, bu, bv, H, lens, what):
    ref = ar.reference(kind, qkv, pos, bu, bv, H, lens=lens)
    return ar.check(kind, got, ref, H, int(sum(lens)), what, guard=False)


@pytest.mark.parametrize("T", [1, 2, 3, 7, 32, 33, 64, 100])
def test_literal_rel_shift_is_the_closed_form(T):
    rng = np.random.default_rng(T)
    x = rng.standard_normal((2, 3, T, 2 * T - 1))
    lit = ar.rel_shift(x)
    tr = torch_ref.rel_shift(torch.from_numpy(x)).numpy()
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    closed = x[..., i, j - i + T - 1]
    assert np.array_equal(lit, tr) and np.array_equal(lit, closed)
    for b in range(2):
        for h in range(3):
            assert np.array_equal(ar.band_gather(x[b, h], np.arange(T), T), closed[b, h])
    rows = np.array([0, T - 1]) if T > 1 else np.array([0])
    assert np.array_equal(ar.band_gather(x[0, 0][rows], rows, T), closed[0, 0][rows])


# case families at small T: (hd, H, lens, pos_T)
SMALL = {
    "T33_hd64_H2": (64, 2, [33], 40),
    "T70_hd128_H2_pos": (128, 2, [70], 75),
    "T160_hd64_H3": (64, 3, [160], 160),
    "ragged_hd64_H2": (64, 2, [37, 5, 5, 129], 140),
}


def inputs(case, family, seed=3):
    hd, H, lens, pos_T = SMALL[case]
    qkv, pos, bu, bv = ar.make_inputs(family, lens, hd * H, H, pos_T, seed)
    return qkv, pos, bu, bv, H, lens


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("case", sorted(SMALL))
def test_checker_accepts_tiled_bf16_implementation(case, family):
    qkv, pos, bu, bv, H, lens = inputs(case, family)
    got = tiled_f32(qkv, pos, bu, bv, H, lens)
    worst, mean = run_check("bf16", got, qkv, pos, bu, bv, H, lens, f"tiled bf16 {case} {family}")
    print(f"tiled-bf16 {case:>20} {family:>6}: max err/bound {worst:.3f}  mean err/sigma {mean:.3f}")


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("case", sorted(SMALL))
def test_checker_accepts_plain_fp32_implementation(case, family):
    qkv, pos, bu, bv, H, lens = inputs(case, family)
    got = plain_f32(qkv, pos, bu, bv, H, lens)
    worst, mean = run_check("fp32", got, qkv, pos, bu, bv, H, lens, f"plain fp32 {case} {family}")
    print(f"plain-fp32 {case:>20} {family:>6}: max err/bound {worst:.3f}  mean err/sigma {mean:.3f}")


# every mutant and the (case, family) that catches it
MUTANTS = {
    "pos_minus1": ("T33_hd64_H2", "pos"),                 # position index j - i + T - 2
    "pos_plus1": ("T33_hd64_H2", "pos"),                  # position index j - i + T
    "no_c": ("T70_hd128_H2_pos", "c"),                    # (q + u) . P: the c = (v - u) . P term dropped
    "extra_key": ("T33_hd64_H2", "random"),               # key T admitted as a copy of key T - 1 in the last tile
    "window_unshifted": ("T70_hd128_H2_pos", "pos"),      # table rows from 0 instead of pos_T - T
    "tile_not_rescaled": ("T160_hd64_H3", "key"),         # the 32-key tile at key 32 skips the rescale of ctx when the maximum rises
    "head_u_next": ("T33_hd64_H2", "random"),             # head h biased with head h + 1's u
    "swap_utterances": ("ragged_hd64_H2", "random"),      # two utterances' rows exchanged in a packed batch
    "scale_d": ("T33_hd64_H2", "random"),                 # scale 1 / sqrt(d) instead of 1 / sqrt(hd)
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_checker_rejects_mutant(mut):
    case, family = MUTANTS[mut]
    qkv, pos, bu, bv, H, lens = inputs(case, family)
    got = tiled_f32(qkv, pos, bu, bv, H, lens, mut=mut)
    with pytest.raises(AssertionError, match="max err / bound|mean err"):
        run_check("bf16", got, qkv, pos, bu, bv, H, lens, f"mutant {mut} on {case} {family}")


def test_checker_flags_unwritten_and_guard_elements():
    qkv, pos, bu, bv, H, lens = inputs("T33_hd64_H2", "random")
    good = tiled_f32(qkv, pos, bu, bv, H, lens)
    ref = ar.reference("bf16", qkv, pos, bu, bv, H, lens=lens)
    sentinel = np.array([ar.UNWRITTEN["bf16"]], np.uint32).view(np.float32)[0]
    full = np.concatenate([good, np.full((ar.GUARD_ROWS, good.shape[1]), sentinel, np.float32)])
    ar.check("bf16", full, ref, H, 33, "clean")
    bad = full.copy()
    bad[33 + 5, 7] = 0.0
    with pytest.raises(AssertionError, match="guard row 5 column 7"):
        ar.check("bf16", bad, ref, H, 33, "guard")
    bad = full.copy()
    bad[32, 64] = sentinel
    with pytest.raises(AssertionError, match="row 32 column 64 was never written"):
        ar.check("bf16", bad, ref, H, 33, "unwritten")
