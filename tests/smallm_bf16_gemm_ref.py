"""The float64 reference of the small-M bf16 GEMM family (csrc/kernels/gemm_smallm_bf16.hip), on top of tests/bf16_gemm_ref.py (the product of operands rounded
to bf16, every epilogue function, the bounds and their derivations) and tests/smallm_gemm_ref.py (the streaming conv tail): the LayerNorm folded into the product,
the second norm in front of it, and the two layouts of the family -- the 8-row operand tiles of the activations between two products (GemmArgs::out_t8 / a_t8)
and the operand tiles of the weights (GemmArgs::W_t16).  Written from the comments of csrc/kernels/kernels.hpp (GemmArgs); no device code path is restated:
index arithmetic on whole arrays only."""
import numpy as np

from bf16_gemm_ref import (FILL16, FILL32, acc_bound, bf16_bits, bf16_round, bf16_value, check_bf16_rows, coherent_operands, excused_share,  # noqa: F401
                           fast_sigmoid_rel, out_bound, output_offsets, product, words_to_bf16)
from smallm_gemm_ref import stream_dwconv_f64  # noqa: F401


# ---- the folded norms ------------------------------------------------------------------------------------------------------------------------------
def layer_norm64(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last axis in float64 (mean, then the mean of the squared deviations)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def flip_allowance(X, W, epi):
    """The kernel's fp32 LayerNorm differs from float64's in the last bit of a few elements, and such an element may round to the neighbouring bf16 value (2^-8
    relative): a 2^-8 error on a few (four) operands per row, 4 * 2^-8 * max|a| * max|w| per output element, as tests/test_gpu_bf16.py derives it.  X: the
    normalised rows (fp32), W [N or 2N][K]; GLU: the allowances of the value and the gate column, summed."""
    Aq, Wq = np.abs(bf16_round(X)).astype(np.float64), np.abs(bf16_round(W)).astype(np.float64)
    flip = 4.0 * 2.0 ** -8 * (Aq.max(axis=1, keepdims=True) * Wq.max(axis=1)[None, :])
    if epi == "glu":
        N = W.shape[0] // 2
        return flip[:, :N] + flip[:, N:]
    return flip


def folded_product(A, gamma, beta, W, bias, epi, resid=None, alpha=1.0, eps=1e-5):
    """out = epi(bf16(LN(A)) bf16(W)^T + bias): LayerNorm in float64, cast to fp32, rounded to bf16, multiplied in float64.  -> product(...)'s dict + flip."""
    X = layer_norm64(A, gamma, beta, eps).astype(np.float32)
    p = product(X, W, bias, epi, resid, alpha)
    p["flip"] = flip_allowance(X, W, epi)
    return p


def pre_out_bound(y):
    """|pre_out - LN64(A; pre)|: the fp32 LayerNorm class of tests/test_gpu_bf16.py, 2e-6 (1 + max|y|)"""
    return 2e-6 * (1.0 + np.abs(y).max())


def ln_out_bound(p, epi, fast=False):
    """|out - want| of a product with a folded norm: the plain product's bound + the flipped operands"""
    return out_bound(p, epi, fast) + p["flip"]


# ---- the 8-row operand tiles of the activations (GemmArgs::out_t8 / a_t8) -------------------------------------------------------------------------------
def t8_offsets(M, cols):
    """[M][cols] element offsets of (row, k): per (8 rows, 32 k) one tile of 256 elements [(row % 8) + 8 (k / 8 % 4)][8 consecutive k], tiles ordered
    [rows / 8][cols / 32].  M % 8 == 0, cols % 32 == 0."""
    assert M % 8 == 0 and cols % 32 == 0
    row, k = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    tile = (row // 8) * (cols // 32) + k // 32
    return tile * 256 + ((row % 8) + 8 * ((k // 8) % 4)) * 8 + k % 8


def to_t8(x):
    """x [M][cols] -> the flat tiled buffer of M * cols elements"""
    x = np.asarray(x)
    buf = np.empty(x.size, x.dtype)
    buf[t8_offsets(*x.shape)] = x
    return buf


def from_t8(buf, M, cols):
    """Undoes to_t8"""
    return np.asarray(buf)[t8_offsets(M, cols)]


# ---- the operand tiles of the weights (GemmArgs::W_t16) -----------------------------------------------------------------------------------------------------
def w_t16_tiling(src, K=None):
    """The operand-tile copy: per (16 rows, 32 k) one KB [lane][8 elements], lane = (row % 16) + 16 (k / 8 % 4), tiles ordered [rows / 16][K / 32]:
    dst[tile][step][lane][e] = src[16 tile + lane % 16][32 step + 8 (lane / 16) + e], flattened.  src [rows][ld >= K], rows % 16 == 0, K % 32 == 0."""
    src = np.asarray(src)
    rows, ld = src.shape
    K = ld if K is None else K
    assert rows % 16 == 0 and K % 32 == 0 and ld >= K
    tile, step, lane, e = np.meshgrid(np.arange(rows // 16), np.arange(K // 32), np.arange(64), np.arange(8), indexing="ij")
    return src[16 * tile + lane % 16, 32 * step + 8 * (lane // 16) + e].reshape(-1)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------------
def coherent_ln_operands(rng, M, N, K, positive=False):
    """Rows, a norm and weights whose folded product has no cancellation: gamma = 1/4 and beta = 4 put every normalised element in about [3, 5], the weights
    are coherent_operands' (sign by column, magnitude ~ 1 / K): |want| ~ 4 x the column scale, so the flip allowance (~ 4 * 2^-8 * 5 * 1.5 / K of it) stays far
    below a bf16 ulp for K >= 1024.  positive: every column positive -- for SiLU, which squeezes a negative pre-activation to a value far below the allowance
    (absolute in the pre-activation) and would leave every such element within delta of a rounding boundary."""
    A = (rng.standard_normal((M, K)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))).astype(np.float32)
    _, W = coherent_operands(rng, M, N, K)
    if positive:
        W = np.abs(W)
    return A, np.full(K, 0.25, np.float32), np.full(K, 4.0, np.float32), W


# ---- the bf16-rows cases of tests/test_gpu_smallm_bf16_gemm.py (tests/test_smallm_bf16_gemm_ref.py measures the reference's own excused share on them) ------
BF16_ROWS_CASES = [(33, 272, 512, epi, False) for epi in ("none", "relu", "silu")] + [(17, 272, 2048, epi, True) for epi in ("none", "relu", "silu")]


def bf16_rows_case(M, N, K, epi, ln):
    """Operands without cancellation, the float64 reference and delta (the fp32-rows bound; SiLU on the hardware exp2 / rcp, as production sets it)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + (1 if ln else 0))
    bias = (0.01 * rng.standard_normal(N)).astype(np.float32)
    if ln:
        A, gamma, beta, W = coherent_ln_operands(rng, M, N, K, positive=epi == "silu")
        p = folded_product(A, gamma, beta, W, bias, epi)
        return dict(A=A, W=W, bias=bias, ln=(gamma, beta), p=p, delta=ln_out_bound(p, epi, fast=epi == "silu"))
    A, W = coherent_operands(rng, M, N, K)
    p = product(A, W, bias, epi)
    return dict(A=A, W=W, bias=bias, ln=None, p=p, delta=out_bound(p, epi, epi == "silu"))
