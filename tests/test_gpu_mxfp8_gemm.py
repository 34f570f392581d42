"""The MXFP8 kernels alone (csrc/kernels/gemm_mxfp8.hip through pk_diag_mx_quantize / pk_diag_gemm_mxfp8) against tests/mxfp8_ref.py:
the quantiser bit for bit; the product EXACTLY on operands whose every partial sum is an integer below 2^24 (any layout, scale-byte or k-order
error shows); gaussian operands within an fp32-accumulation class measured for the instruction (8e-6 * sum|a w|; the bf16 products: 2e-6)."""
import numpy as np
import pytest

import mxfp8_ref as R
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu
FILL = np.frombuffer(np.uint32(capi.SKINNY_FILL32).tobytes(), np.uint8)


@pytest.mark.parametrize("src_bf16", [False, True])
def test_quantiser_bit_equal_and_pads_untouched(src_bf16):
    K, ld = 160, 200                                                   # five blocks: a K tile and a quarter, half a scale group
    x = np.concatenate([R.edge_rows(K, 1), R.edge_rows(K, 2)[:3]])     # 11 rows: 5 rows of the last 8-row block are never written
    if src_bf16:
        x = R.bf16_round(x)
    src = np.zeros((len(x), ld), np.float32)
    src[:, :K] = x
    q, s = capi.diag_mx_quantize(src, K=K, src_bf16=src_bf16)
    wq, ws = R.quantize(x)
    assert np.array_equal(s[:len(x), :K // 32], ws), "scale bytes"
    assert np.array_equal(q[:len(x), :K], wq), f"element bytes differ at {np.argwhere(q[:len(x), :K] != wq)[:4]}"
    # what the launch never wrote holds the fill: a chunk keeps its bytes' order, a scale byte of block kb lies at an offset = (kb >> 1) & 3 (mod 4)
    pad_q = np.broadcast_to(FILL[np.arange(q.shape[1]) % 4], q.shape)
    pad_s = np.broadcast_to(FILL[(np.arange(s.shape[1]) >> 1) & 3], s.shape)
    assert np.array_equal(q[len(x):], pad_q[len(x):]) and np.array_equal(q[:, K:], pad_q[:, K:]), "element bytes outside the operand"
    assert np.array_equal(s[len(x):], pad_s[len(x):]) and np.array_equal(s[:, K // 32:], pad_s[:, K // 32:]), "scale bytes outside the operand"


def run(A, W, bias, epi, resid=None, silu=False):
    """one product at pitches larger than the rows -> the fp32 output [M][N] (its pads checked), or the MX output (bytes, scale bytes) of M rows x N"""
    (M, K), N = A.shape, W.shape[0]
    r = capi.diag_gemm_mxfp8(A, W, bias, epi=epi, silu=silu, resid=resid, alpha=0.5, lda=K + 8, ldw=K + 4, ldo=N + 4, ldr=N + 8)
    if epi == "mx":
        assert np.all(r["q"][M:] == FILL[np.arange(r["q"].shape[1]) % 4]) and np.all(r["q"][:, N:] == FILL[np.arange(N, r["q"].shape[1]) % 4]), "bytes outside the output"
        return r["q"][:M, :N], r["s"][:M, :N // 32]
    out = r["out"].reshape(M, N + 4)
    assert np.all(out[:, N:] == capi.SKINNY_FILL32), "the padding behind the rows was written"
    return out[:, :N].view(np.float32)


@pytest.mark.parametrize("epi", ["f32", "mx", "resid"])
@pytest.mark.parametrize("K", [64, 128, 320, 1024])
def test_exact_products(K, epi):
    """integers in [-8, 8] times per-block powers of two (2^0 .. 2^3 each side): both quantisations are lossless and every partial sum is an integer
    below 1024 * 64 * 64 = 2^22, so the fp32 result has no rounding to hide behind"""
    bm, bn = capi.diag_gemm_mxfp8(np.zeros((1, 64), np.float32), np.zeros((32, 64), np.float32), epi=epi,
                                  resid=np.zeros((1, 32), np.float32) if epi == "resid" else None)["tile"]
    rng = np.random.default_rng(K)

    def operand(rows):
        return (rng.integers(-8, 9, (rows, K)) * np.repeat(2.0 ** rng.integers(0, 4, (rows, K // 32)), 32, axis=1)).astype(np.float32)
    Afull, Wfull = operand(bm + 1), operand(bn + 32)
    Afull[0, :32] = 0.0                                                # a block of zeros: scale byte 0 next to ordinary ones
    bias = rng.integers(-64, 65, bn + 32).astype(np.float32)
    resid = rng.integers(-1000, 1001, (bm + 1, bn + 32)).astype(np.float32)
    for M in (1, 33, bm, bm + 1):
        for N in (32, bn, bn + 32):
            A, W, b = Afull[:M], Wfull[:N], bias[:N]
            want = A.astype(np.float64) @ W.astype(np.float64).T + b
            ref, _ = R.product(A, W, b)
            assert np.array_equal(ref, want), "the reference itself must be lossless here"
            if epi == "mx":
                q, s = run(A, W, b, "mx")
                wq, ws = R.quantize(want)
                assert np.array_equal(s, ws) and np.array_equal(q, wq), f"M {M} N {N}: MX output differs at {np.argwhere(q != wq)[:4]} / scales {np.argwhere(s != ws)[:4]}"
            else:
                if epi == "resid":
                    want = resid[:M, :N] + 0.5 * want
                got = run(A, W, b, epi, resid=resid[:M, :N] if epi == "resid" else None)
                assert np.array_equal(got.astype(np.float64), want), f"M {M} N {N}: {np.argwhere(got != want)[:4]}"


@pytest.mark.parametrize("epi", ["f32", "mx", "resid"])
def test_gaussian_products(epi):
    """fp32 outputs: |err| <= 8e-6 * sum|a w| against float64 of the same quantised operands.  The bf16 products' 2e-6 is not met: the block-scaled
    instruction's internal summation is undocumented and measures a largest |err| / sum|a w| of 3.97e-6 on these shapes (1.99e-6 behind the
    residual's alpha = 0.5); the bound is twice that (profiles/ffn_mxfp8.md), far below the 1e-4 a wrong block would show.  The ratio is printed.
    MX outputs: the dequantised element within one e4m3 step, 2^-3 |ref| + 2^-9 amax_block(ref), of float64 SiLU of the float64 product, plus that bound."""
    rng = np.random.default_rng(5)
    M, N, K = 300, 320, 1088
    A = R.bf16_round(rng.standard_normal((M, K)) * rng.uniform(0.3, 3.0, (M, 1)))
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    acc, mag = R.product(A, W, bias)
    bound = 8e-6 * mag + 1e-6
    if epi == "mx":
        q, s = run(A, W, bias, "mx", silu=True)
        want = acc / (1.0 + np.exp(-acc))
        step = 2.0 ** -3 * np.abs(want) + 2.0 ** -9 * np.abs(want).reshape(M, N // 32, 32).max(axis=2).repeat(32, axis=1)
        err = np.abs(R.dequantize(q, s) - want)
        bound = bound + step
    else:
        want = resid + 0.5 * acc if epi == "resid" else acc
        err = np.abs(run(A, W, bias, epi, resid=resid if epi == "resid" else None) - want)
        if epi == "resid":
            bound = bound + 1.2e-7 * (np.abs(resid) + np.abs(want))    # the epilogue's own two roundings: alpha * v, then the sum
        print(f"{epi}: largest |err| / sum|a w| = {float((err / mag).max()):.3e}")
    assert np.all(err <= bound), f"max err {err.max():.3e} (bound there {float(bound.flat[err.argmax()]):.3e}) at {np.unravel_index(err.argmax(), err.shape)}"
