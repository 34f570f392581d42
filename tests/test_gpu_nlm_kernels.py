"""GPU: the two kernels of the Transformer LM alone (pk_diag_causal_attention, pk_diag_nlm_head_logp) against the float64 references and the
derived per-element bounds of tests/nlm_ref.py.  Output buffers are NaN-filled before the launch: rows past the packed extent must come back
unwritten."""
import numpy as np
import pytest

import attention_ref as AR
import nlm_ref as R
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

LENS = [1, 2, 31, 32, 33, 64, 65, 100]
UNWRITTEN = np.uint32(0x7FC5A5A5)


def att_inputs(lens, H, hd, seed):
    """packed qkv [rows][3 H hd] (q doubled: a sharper softmax than unit normals give)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((int(np.sum(lens)), 3 * H * hd)).astype(np.float32)
    x[:, : H * hd] *= 2.0
    return x


def pad_heads(qkv, H, hd, hdp):
    """every head of q | k | v zero-padded from hd to hdp columns, as TransformerEncoder pads its projections"""
    rows = qkv.shape[0]
    out = np.zeros((rows, 3, H, hdp), np.float32)
    out[..., :hd] = qkv.reshape(rows, 3, H, hd)
    return out.reshape(rows, 3 * H * hdp)


def run_causal(qkv, lens, H, hd, hdp):
    """the kernel on the (padded) rows -> ctx [rows + guard][H hd] with the pad columns checked to be exact zeros and dropped"""
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))
    ctx = capi.diag_causal_attention(pad_heads(qkv, H, hd, hdp) if hdp != hd else qkv, lens, H, scale)
    rows = qkv.shape[0]
    if hdp == hd:
        return ctx, scale
    c4 = ctx.reshape(ctx.shape[0], H, hdp)
    assert not c4[:rows, :, hd:].any(), "zero-padded head columns of ctx must be exact zeros"
    return np.ascontiguousarray(c4[:, :, :hd]).reshape(ctx.shape[0], H * hd), scale


@pytest.mark.parametrize("hd,hdp", [(24, 32), (64, 64)])
def test_causal_attention_packed_lengths(hd, hdp):
    H = 2
    qkv = att_inputs(LENS, H, hd, seed=hd)
    ctx, scale = run_causal(qkv, LENS, H, hd, hdp)
    worst, mean = AR.check("fp32", ctx, R.causal_reference(qkv, LENS, H, scale), H, qkv.shape[0], f"causal hd {hd}")
    print(f"causal attention hd {hd}: max err / bound {worst:.3g}, mean err / mean sigma {mean:.3g}")
    # row 0 of every sequence sees one key: ctx = v exactly
    off = np.concatenate([[0], np.cumsum(LENS)])[:-1]
    assert np.array_equal(ctx[off].view(np.uint32), qkv[off][:, 2 * H * hd:].view(np.uint32))


def test_causal_attention_one_sequence_of_512():
    H, hd = 2, 64
    qkv = att_inputs([512], H, hd, seed=512)
    ctx, scale = run_causal(qkv, [512], H, hd, hd)
    worst, mean = AR.check("fp32", ctx, R.causal_reference(qkv, [512], H, scale), H, 512, "causal 512")
    print(f"causal attention T 512: max err / bound {worst:.3g}, mean err / mean sigma {mean:.3g}")


@pytest.mark.parametrize("hd,hdp", [(24, 32), (64, 64)])
def test_causal_attention_does_not_leak_the_future(hd, hdp):
    H = 2
    qkv = att_inputs(LENS, H, hd, seed=7)
    base, _ = run_causal(qkv, LENS, H, hd, hdp)
    r100 = int(np.sum(LENS[:-1]))
    other = qkv.copy()
    other[r100 + 40] = np.random.default_rng(9).standard_normal(qkv.shape[1]).astype(np.float32) * 3
    got, _ = run_causal(other, LENS, H, hd, hdp)
    same = np.ones(qkv.shape[0], bool)
    same[r100 + 40:] = False
    assert np.array_equal(got[: qkv.shape[0]][same].view(np.uint32), base[: qkv.shape[0]][same].view(np.uint32)), "a row before position 40, or another sequence, changed"
    assert not np.array_equal(got[r100 + 40: r100 + 100], base[r100 + 40: r100 + 100]), "the change must reach the rows that may see it"


def head_case(V, rows, d, bias, seed):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((rows, d)).astype(np.float32)
    W = (rng.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.5 * rng.standard_normal(V)).astype(np.float32) if bias else None
    t = rng.integers(0, V, rows).astype(np.int32)
    t[0::3] = 0
    t[1::3] = V - 1
    peak = zero = None
    if rows >= 3:
        peak, zero = 2, 0
    elif d == 64:
        peak, t[0] = 0, V - 1
    else:
        zero = 0
    if zero is not None:
        h[zero] = 0.0                                                # every logit of this row is 0 (+ b[c]): all equal without a bias
    if peak is not None:                                             # one logit about 50 above the rest, in the last column tile: the maximum moves late
        hp = h[peak].astype(np.float64)
        W[V - 1] = (W[V - 1] + 50.0 * hp / (hp @ hp)).astype(np.float32)
    return h, W, b, t, peak, zero


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("V", [2, 33, 1025, 8194])
def test_head_logp_within_the_derived_bound(V, d):
    for rows in (1, 63, 130):
        for bias in (False, True):
            h, W, b, t, peak, zero = head_case(V, rows, d, bias, seed=V + rows + d)
            got = capi.diag_nlm_head_logp(h, W, b, t)
            assert np.all(got[rows:].view(np.uint32) == UNWRITTEN), "rows past the extent were written"
            assert np.all(got[:rows].view(np.uint32) != UNWRITTEN) and np.all(np.isfinite(got[:rows]))
            lp, bound = R.head_logp_reference(h, W, b, t)
            err = np.abs(got[:rows].astype(np.float64) - lp)
            r = err / bound
            print(f"head V {V} rows {rows} d {d} bias {bias}: max err / bound {r.max():.3g} (max err {err.max():.3g})")
            assert r.max() <= 1.0, (V, rows, d, bias, int(np.argmax(r)), float(err.max()))
            assert 0 in t and (V - 1) in t or rows == 1
            if peak is not None:
                x = h[peak].astype(np.float64) @ W.astype(np.float64).T + (0 if b is None else b)
                assert np.argmax(x) == V - 1 and (V == 2 or x[V - 1] - np.sort(x)[-2] > 40)
            if zero is not None and not bias:
                assert got[zero] == np.float32(-np.log(V)) or abs(float(got[zero]) + np.log(V)) <= bound[zero]


@pytest.mark.parametrize("V", [2, 33, 1025, 8194])
def test_head_logp_of_every_target_sums_to_one(V):
    d = 64
    rng = np.random.default_rng(V)
    h1 = rng.standard_normal(d).astype(np.float32)
    W = (2.0 * rng.standard_normal((V, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.5 * rng.standard_normal(V)).astype(np.float32)
    got = capi.diag_nlm_head_logp(np.tile(h1, (V, 1)), W, b, np.arange(V, dtype=np.int32))[:V]
    s = float(np.exp(got.astype(np.float64)).sum())
    print(f"head V {V}: sum of exp(lp) over every target = 1 + {s - 1:.3g}")
    assert abs(s - 1.0) <= V * 2.0 ** -20
    # the same row packed at any position of any tile gives the same logsumexp: lp[c] - logit[c] is one value up to the logits' own rounding
    lp, bound = R.head_logp_reference(h1[None], W, b)
    assert np.all(np.abs(got.astype(np.float64) - lp[0]) <= bound[0])
