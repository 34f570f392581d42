"""GPU parity of the hand-placed single-buffered K loop of the fp32 tile GEMM (gemm_pipe_kernel SCHED = 2, gemm_pipe.hpp).

Every launcher branch that takes that loop -- the long-K 128x128 tile of 64 x 32 waves, the wide 128x128 tile of 32 x 64 waves with and without the
LayerNorm folded into the A staging, and the GLU product -- is compared bit for bit with the oracle: every epilogue at the encoder's headline shapes,
partial row and column tiles, the two-K-tile minimum, a K that is not a multiple of 64, and inputs whose magnitudes span 2^-10 .. 2^10 so that any
change in the k order of an output's fma chain shows up in the bits."""
import numpy as np
import pytest

from conftest import pk  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def wide_range(rng, shape):
    """Normal values scaled by 2^e, e uniform in [-10, 10]: partial sums cancel and round differently under any other k order."""
    return (rng.standard_normal(shape) * np.exp2(rng.uniform(-10.0, 10.0, shape))).astype(np.float32)


def reference(orc, A, W, b, epi, resid=None, alpha=1.0):
    if epi == "glu":
        N = W.shape[0] // 2
        v = orc.linear(A, W[:N], b[:N])
        gt = orc.linear(A, W[N:], b[N:])
        return v * orc.math_v("sigmoid", gt)
    y = orc.linear(A, W, b)
    if epi == "none":
        return y
    if epi == "relu":
        return np.where(y > 0, y, np.float32(0.0)).astype(np.float32)
    if epi == "silu":
        return orc.math_v("silu", y)
    if epi == "resid":
        return (resid + y * np.float32(alpha)).astype(np.float32)
    raise ValueError(epi)


# (M, N, K, epi, alpha): N is the output width (the GLU weight has 2N rows)
CASES = [
    (8064, 1536, 512, "none", 1.0),       # qkv
    (8064, 2048, 512, "relu", 1.0),       # fc1 shape, ReLU
    (8064, 2048, 512, "silu", 1.0),       # fc1 + SiLU
    (8064, 512, 2048, "resid", 0.5),      # fc2 + half-step residual (long-K tile)
    (8064, 512, 512, "resid", 1.0),       # out_proj / pw2 + residual
    (8064, 512, 512, "glu", 1.0),         # conv pw1 + GLU
    (8000, 1536, 512, "none", 1.0),       # M not a multiple of 128
    (1601, 2048, 512, "silu", 1.0),       # smallest M past the small-M kernels, partial row tile
    (8000, 512, 1024, "resid", 0.5),      # long-K tile with a partial row tile
    (2048, 1100, 512, "silu", 1.0),       # partial column tile
    (2048, 1100, 512, "resid", 0.5),
    (2048, 1024, 64, "none", 1.0),        # two K tiles: the minimum of the pipelined loop
    (2048, 520, 64, "glu", 1.0),          # two K tiles, GLU, partial column tile
    (2048, 1024, 96, "silu", 1.0),        # K % 64 != 0: three K tiles
]


@pytest.mark.parametrize("M,N,K,epi,alpha", CASES, ids=[f"{m}x{n}x{k}-{e}-{a}" for m, n, k, e, a in CASES])
def test_scheduled_loop_matches_oracle(capi, orc, M, N, K, epi, alpha):
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    rows = 2 * N if epi == "glu" else N
    A = wide_range(rng, (M, K))
    W = (wide_range(rng, (rows, K)) / np.float32(np.sqrt(K))).astype(np.float32)
    b = rng.standard_normal(rows).astype(np.float32)
    R = wide_range(rng, (M, N)) if epi == "resid" else None
    got = capi.diag_gemm(A, W, b, epi=epi, resid=R, alpha=alpha)
    want = reference(orc, A, W, b, epi, R, alpha)
    assert np.array_equal(bits(got), bits(want)), f"{int(np.sum(bits(got) != bits(want)))} of {got.size} results differ"


LN_CASES = [
    (8064, 2048, 512, "silu"),            # fc1: LayerNorm folded into the A staging
    (8064, 1536, 512, "none"),            # qkv
    (8064, 512, 512, "glu"),              # conv pw1
    (1601, 1100, 96, "relu"),             # partial row and column tiles, three K tiles
]


@pytest.mark.parametrize("M,N,K,epi", LN_CASES, ids=[f"{m}x{n}x{k}-{e}" for m, n, k, e in LN_CASES])
def test_scheduled_loop_with_folded_layernorm_matches_oracle(capi, orc, M, N, K, epi):
    rng = np.random.default_rng(M + N * 5 + K * 11)
    rows = 2 * N if epi == "glu" else N
    A = wide_range(rng, (M, K))
    g = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    be = (0.1 * rng.standard_normal(K)).astype(np.float32)
    W = (wide_range(rng, (rows, K)) / np.float32(np.sqrt(K))).astype(np.float32)
    b = rng.standard_normal(rows).astype(np.float32)
    got, _ = capi.diag_ln_gemm(A, g, be, W, b, epi=epi, fold=True)
    want = reference(orc, orc.layer_norm(A, g, be), W, b, epi)
    assert np.array_equal(bits(got), bits(want)), f"{int(np.sum(bits(got) != bits(want)))} of {got.size} results differ"
