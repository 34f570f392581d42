"""Plain numpy statements of the layouts and the conv tail around the fp32 small-M GEMM family (csrc/kernels/gemm_smallm.hip), written from
the comments of csrc/kernels/kernels.hpp (GemmArgs::sigma_cols, W_sig, remap_*; DwTail) -- what tests/test_gpu_smallm_gemm.py undoes the
kernels' output layouts with.  No device code is restated here: index arithmetic on whole arrays only."""
import numpy as np


def sigma_perm(n):
    """Where natural column k of a row lands in the sigma layout: inside every block of 16 the 4 x 4 index matrix is transposed,
    k = 16 b + 4 q + j  ->  16 b + 4 j + q.  n must be a multiple of 16."""
    assert n % 16 == 0
    k = np.arange(n)
    b, q, j = k // 16, (k % 16) // 4, k % 4
    return 16 * b + 4 * j + q


def sigma_perm_inverse(n):
    """The natural column that sits at position p of the sigma layout."""
    inv = np.empty(n, np.int64)
    inv[sigma_perm(n)] = np.arange(n)
    return inv


def to_sigma(x, n_sigma=None):
    """x [..][cols] with its first n_sigma columns (default: all) moved to their sigma positions; the rest stay."""
    x = np.asarray(x)
    n = x.shape[-1] if n_sigma is None else n_sigma
    y = x.copy()
    y[..., sigma_perm(n)] = x[..., :n]
    return y


def from_sigma(y, n_sigma=None):
    """Undoes to_sigma."""
    y = np.asarray(y)
    n = y.shape[-1] if n_sigma is None else n_sigma
    x = y.copy()
    x[..., :n] = y[..., sigma_perm(n)]
    return x


def w_sig_tiling(src, K=None):
    """The tiled weight copy: dst[tile][chunk][q][lane][e] = src[16 tile + lane % 16][64 chunk + 16 q + 4 e + lane / 16], flattened.
    src [rows][ld >= K], rows % 16 == 0, K % 64 == 0."""
    src = np.asarray(src)
    rows, ld = src.shape
    K = ld if K is None else K
    assert rows % 16 == 0 and K % 64 == 0 and ld >= K
    tile, chunk, q, lane, e = np.meshgrid(np.arange(rows // 16), np.arange(K // 64), np.arange(4), np.arange(64), np.arange(4), indexing="ij")
    return src[16 * tile + lane % 16, 64 * chunk + 16 * q + 4 * e + lane // 16].reshape(-1)


def w_sig_source_index(rows, K):
    """For every word of the tiled copy, the flat index (row * K + k) of the source word it holds."""
    idx = np.arange(rows * K, dtype=np.int64).reshape(rows, K)
    return w_sig_tiling(idx)


def remap_offset(row, col, remap_rows, gs, rs, cs):
    """GemmArgs::remap_*: offset = (row / remap_rows) * remap_gs + (row % remap_rows) * remap_rs + col * remap_cs"""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    return (row // remap_rows) * gs + (row % remap_rows) * rs + col * cs


def output_offsets(M, N, ldo, sigma_cols=0, remap=None):
    """[M][N] offsets into the output buffer of the element (row, natural column col), as GemmArgs describes them."""
    row, col = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    if remap is not None:
        return remap_offset(row, col, *remap)
    pos = np.arange(N)
    if sigma_cols:
        pos[:sigma_cols] = sigma_perm(sigma_cols)
    return row.astype(np.int64) * ldo + pos[col]


def stream_dwconv_f64(glu, cache, has_cache, dw_w, dw_bias, bn_mean, bn_rstd, bn_g, bn_b):
    """The streaming conv module's middle (reference src/streaming_encoder.cpp:41-78) in float64: cat(cache or zeros [S][8][d], glu [S][c][d]),
    depthwise conv of 9 taps without padding, + bias, BatchNorm (inference form: (y - mean) * rstd * g + b), SiLU.
    -> (activations [S][c][d] float64, the new cache = the last 8 rows of the concatenation, in glu's dtype)."""
    glu = np.asarray(glu)
    S, c, d = glu.shape
    old = np.asarray(cache) if has_cache else np.zeros((S, 8, d), glu.dtype)
    cat = np.concatenate([old, glu], axis=1)
    c64 = cat.astype(np.float64)
    y = np.stack([(c64[:, t:t + 9, :] * np.asarray(dw_w, np.float64)[None]).sum(axis=1) for t in range(c)], axis=1) + np.asarray(dw_bias, np.float64)
    y = (y - np.asarray(bn_mean, np.float64)) * np.asarray(bn_rstd, np.float64) * np.asarray(bn_g, np.float64) + np.asarray(bn_b, np.float64)
    with np.errstate(over="ignore"):                                    # (exp(-y) = inf for very negative y: silu = -0)
        act = y / (1.0 + np.exp(-y))
    return act, cat[:, c:, :]
