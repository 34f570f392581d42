"""CPU checks of tests/smallm_gemm_ref.py, the layout reference of tests/test_gpu_smallm_gemm.py: the sigma permutation is an involution on blocks
of 16, the W_sig tiling is a bijection onto rows * K, a product of permuted operands is the natural product, and the tiled weights hand a lane the k
values the sigma rows hand it."""
import numpy as np
import pytest

import smallm_gemm_ref as R


@pytest.mark.parametrize("n", [16, 48, 512, 1024])
def test_sigma_permutation_is_an_involution_on_blocks_of_16(n):
    p = R.sigma_perm(n)
    assert sorted(p) == list(range(n))
    assert np.array_equal(p[p], np.arange(n)) and np.array_equal(R.sigma_perm_inverse(n), p)
    assert np.array_equal(p // 16, np.arange(n) // 16), "a column never leaves its block of 16"
    assert np.array_equal(p[:16], [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15])
    # the expression the kernels use
    k = np.arange(n)
    assert np.array_equal(p, (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3))
    x = np.arange(3 * n).reshape(3, n)
    assert np.array_equal(R.from_sigma(R.to_sigma(x)), x) and np.array_equal(R.to_sigma(R.to_sigma(x)), x)
    if n >= 32:
        y = R.to_sigma(x, n - 16)
        assert np.array_equal(y[:, n - 16:], x[:, n - 16:]) and np.array_equal(R.from_sigma(y, n - 16), x)


@pytest.mark.parametrize("rows,K", [(16, 64), (48, 192), (32, 1024)])
def test_w_sig_tiling_is_a_bijection(rows, K):
    idx = R.w_sig_source_index(rows, K)
    assert idx.shape == (rows * K,) and np.array_equal(np.sort(idx), np.arange(rows * K))
    # one (tile, chunk) block is 16 rows x 64 k = 1024 consecutive words, and holds exactly that tile's rows and that chunk's k
    blk = idx.reshape(rows // 16, K // 64, 1024)
    for t in range(rows // 16):
        for c in range(K // 64):
            r, k = blk[t, c] // K, blk[t, c] % K
            assert set(r) == set(range(16 * t, 16 * t + 16)) and set(k) == set(range(64 * c, 64 * c + 64))
    # a padded source: only the first K columns are read
    src = np.arange(rows * (K + 8), dtype=np.float32).reshape(rows, K + 8)
    assert np.array_equal(R.w_sig_tiling(src, K), R.w_sig_tiling(np.ascontiguousarray(src[:, :K])))


def test_tiled_weights_and_sigma_rows_pair_the_same_k():
    """Lane (r, kq) of a wave loads four consecutive words of the sigma row of A at 64 chunk + 16 q + 4 kq and word [q][lane][0..3] of the weight block:
    element e of both must be the same natural k."""
    K = 192
    a_nat_of_pos = R.sigma_perm_inverse(K)                          # natural k at every position of a sigma row
    w_k = (R.w_sig_source_index(16, K) % K).reshape(K // 64, 4, 64, 4)
    for chunk in range(K // 64):
        for q in range(4):
            for lane in range(64):
                kq = lane // 16
                a_k = a_nat_of_pos[64 * chunk + 16 * q + 4 * kq: 64 * chunk + 16 * q + 4 * kq + 4]
                assert np.array_equal(a_k, w_k[chunk, q, lane])


def test_product_of_permuted_operands_is_the_natural_product():
    rng = np.random.default_rng(5)
    A = rng.integers(-8, 9, (7, 128)).astype(np.float64)            # small integers: every sum is exact in any order
    W = rng.integers(-8, 9, (48, 128)).astype(np.float64)
    assert np.array_equal(R.to_sigma(A) @ R.to_sigma(W).T, A @ W.T)
    # ... and a partly permuted output (GemmArgs::sigma_cols) read back through output_offsets
    out = np.full(7 * 50, -1.0)
    off = R.output_offsets(7, 48, 50, sigma_cols=32)
    out[off] = A @ W.T
    got = R.from_sigma(out.reshape(7, 50)[:, :48], 32)
    assert np.array_equal(got, A @ W.T) and np.all(out.reshape(7, 50)[:, 48:] == -1.0)


def test_remap_offsets_are_the_subsampling_layout():
    """The engine's pattern (remap_rows = W3, gs = C W3, rs = 1, cs = W3) writes row (t, w) column c to out[t][c][w]."""
    W3, Cc, T = 10, 48, 5
    off = R.output_offsets(T * W3, Cc, 0, remap=(W3, Cc * W3, 1, W3))
    assert sorted(off.reshape(-1)) == list(range(T * Cc * W3))
    want = np.arange(T * Cc * W3).reshape(T, Cc, W3).transpose(0, 2, 1).reshape(T * W3, Cc)
    assert np.array_equal(off, want)


def test_stream_dwconv_reference_is_a_causal_conv_over_cache_and_chunk():
    rng = np.random.default_rng(9)
    S, c, d = 3, 2, 16
    glu, cache = rng.standard_normal((S, c, d)).astype(np.float32), rng.standard_normal((S, 8, d)).astype(np.float32)
    w = rng.standard_normal((9, d)).astype(np.float32)
    one, zero = np.ones(d, np.float32), np.zeros(d, np.float32)
    act, new = R.stream_dwconv_f64(glu, cache, True, w, zero, zero, one, one, zero)
    assert np.array_equal(new, np.concatenate([cache, glu], axis=1)[:, c:]) and new.dtype == np.float32
    y = sum(w[kk].astype(np.float64) * (cache[0, 1 + kk] if 1 + kk < 8 else glu[0, 1 + kk - 8]) for kk in range(9))   # frame 1 of stream 0
    assert np.allclose(act[0, 1], y / (1 + np.exp(-y)), rtol=1e-12, atol=0)
    act0, new0 = R.stream_dwconv_f64(glu, cache, False, w, zero, zero, one, one, zero)
    assert np.all(new0[:, :8 - c] == 0) and np.array_equal(new0[:, 8 - c:], glu)
