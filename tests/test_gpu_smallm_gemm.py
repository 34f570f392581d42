"""The fp32 small-M GEMM family alone (csrc/kernels/gemm_smallm.hip through pk_diag_gemm_smallm: one product per call, staged as the engine stages it):
the chain kernel at every ring depth with natural and sigma operands, the two-row-tile kernel, the kernel with the LayerNorm folded in, its form with a
second norm in front and its form with the depthwise-conv tail -- and the layouts they read (launch_sigma_copy, LayerNorm with sigma columns).

Every product is compared BIT FOR BIT with the oracle (orc.linear / orc.layer_norm / orc.math_v): exact mode has no tolerance.  Inputs span 2^-10 .. 2^10
(wide_range of tests/test_gpu_gemm_schedule.py), so any change in the k order of an output's fma chain shows in the bits.  The output buffer comes back whole
and exactly as the kernel wrote it: the reference (tests/smallm_gemm_ref.py) says where every element belongs, and every other word must still hold the fill
pattern.  Each case names the form it is written for and compares it with the form the launcher's own function reports (no threshold is restated here);
test_every_form_has_a_case compares the union of those with the library's table, so an instantiation without a case fails the suite."""
import functools
import itertools

import numpy as np
import pytest

import smallm_gemm_ref as R
from conftest import pk  # noqa: F401
from test_gpu_gemm_schedule import bits, wide_range

pytestmark = pytest.mark.gpu

PK_ERR_UNSUPPORTED = -7
EPIS = ("none", "relu", "silu", "resid", "glu")
LN_EPIS = ("none", "relu", "silu", "glu")


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


def operands(seed, M, N, K, epi, lda=None):
    """A [M][lda] (columns past K are padding the kernels must not read into the result), asymmetric W, bias, residual."""
    rng = np.random.default_rng(seed)
    rows = 2 * N if epi == "glu" else N
    A = wide_range(rng, (M, lda or K))
    W = (wide_range(rng, (rows, K)) / np.float32(np.sqrt(K))).astype(np.float32)
    b = rng.standard_normal(rows).astype(np.float32)
    Rs = wide_range(rng, (M, N)) if epi == "resid" else None
    return A, W, b, Rs


def epilogue(orc, lin, lin_gate, epi, resid=None, alpha=1.0):
    """The epilogues as tests/test_gpu_gemm_schedule.py states them, on products the caller already has (lin = X W^T + bias; glu: value and gate halves)."""
    if epi == "glu":
        return lin * orc.math_v("sigmoid", lin_gate)
    if epi == "none":
        return lin
    if epi == "relu":
        return np.where(lin > 0, lin, np.float32(0.0)).astype(np.float32)
    if epi == "silu":
        return orc.math_v("silu", lin)
    return (resid + lin * np.float32(alpha)).astype(np.float32)


def product(orc, X, W, b, epi, resid=None, alpha=1.0):
    """epi(X W^T + b) from the oracle; b None: no bias is added at all."""
    if epi == "glu":
        N = W.shape[0] // 2
        return epilogue(orc, orc.linear(X, W[:N], None if b is None else b[:N]), orc.linear(X, W[N:], None if b is None else b[N:]), epi)
    return epilogue(orc, orc.linear(X, W, b), None, epi, resid, alpha)


def expect_buffer(capi, want, out_words, ldo, sigma_cols=0, remap=None):
    """The whole output buffer: `want` [M][N] at the offsets GemmArgs describes, the fill pattern everywhere else."""
    buf = np.full(out_words, capi.SKINNY_FILL32, np.uint32)
    off = R.output_offsets(want.shape[0], want.shape[1], ldo, sigma_cols, remap).reshape(-1)
    assert len(np.unique(off)) == off.size
    buf[off] = bits(want).reshape(-1)
    return buf


def assert_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[0]}: got {got[bad[0]]:#010x} want {want[bad[0]]:#010x}"


# ---- the chain kernel: natural and sigma operands ------------------------------------------------------------------------------------------------
CHAIN_DEPTH = {64: 1, 192: 1, 128: 2, 512: 8, 1024: 8}          # the ring depth each K is here for (1024: two rounds of the ring of 8)
CHAIN_M = (1, 16, 17, 50)                                        # one row, a full tile, a tile + 1, three full tiles + a partial one
# per M: bias?, alpha (resid), sigma_cols at N = 16 / 48 / 40
CHAIN_VARIANT = {1: (True, 0.5, (0, 0, 0)), 16: (True, 1.0, (16, 32, 32)), 17: (False, 0.5, (0, 48, 16)), 50: (True, 1.0, (16, 32, 0))}
CHAIN_CASES = [(K, epi) for K in CHAIN_DEPTH for epi in EPIS]


def chain_want(K, epi, sig):
    return ("chain", epi, CHAIN_DEPTH[K], sig, False, False)


@pytest.mark.parametrize("K,epi", CHAIN_CASES, ids=[f"K{k}-{e}" for k, e in CHAIN_CASES])
def test_chain_kernel_natural_and_sigma_operands_match_oracle(capi, orc, K, epi):
    """N = 16 / 48 with both operand layouts (the same inputs: both equal the oracle, so each other), N = 40 -- a partial column tile -- with the natural
    one; a padded output pitch, the partly permuted output, GLU and the other epilogues with and without bias."""
    for M, (N_i, N) in itertools.product(CHAIN_M, enumerate((16, 48, 40))):
        with_bias, alpha, scols = CHAIN_VARIANT[M]
        A, W, b, Rs = operands(K * 131 + M * 7 + N, M, N, K, epi)
        if not with_bias:
            b = None
        want = product(orc, A, W, b, epi, Rs, alpha)
        ldo, words = N + 3, M * (N + 3) + 5
        buf = expect_buffer(capi, want, words, ldo, scols[N_i])
        kw = dict(bias=b, epi=epi, resid=Rs, alpha=alpha, sigma_cols=scols[N_i], ldo=ldo, out_words=words)
        nat = capi.diag_gemm_smallm(A, W, **kw)
        assert nat["form"] == chain_want(K, epi, False)
        assert_words(nat["out"], buf, f"natural operands M={M} N={N}")
        if N % 16 == 0:
            sig = capi.diag_gemm_smallm(A, W, w_sig=True, a_sigma=True, **kw)
            assert sig["form"] == chain_want(K, epi, True)
            assert_words(sig["out"], buf, f"sigma operands M={M} N={N}")
            assert_words(sig["out"], nat["out"], f"sigma against natural operands M={M} N={N}")
            half = capi.diag_gemm_smallm(A, W, w_sig=True, a_sigma=False, **kw)   # the tiled copy without sigma rows: the natural kernel
            assert half["form"] == chain_want(K, epi, False)
            assert_words(half["out"], buf, f"natural rows beside a tiled weight copy M={M} N={N}")


@pytest.mark.parametrize("sig", [False, True], ids=["natural", "sigma"])
def test_chain_kernel_remapped_output(capi, orc, sig):
    """The last subsampling conv's pattern: row (t, w) column c goes to out[t][c][w] (remap_rows = W3, gs = C W3, rs = 1, cs = W3)."""
    W3, C, T, K = 10, 48, 5, 128
    M = T * W3
    A, W, b, _ = operands(77, M, C, K, "relu")
    remap = (W3, C * W3, 1, W3)
    words = T * C * W3 + 9
    got = capi.diag_gemm_smallm(A, W, bias=b, epi="relu", w_sig=sig, a_sigma=sig, remap=remap, out_words=words)
    assert got["form"] == chain_want(K, "relu", sig)
    want = product(orc, A, W, b, "relu")
    assert_words(got["out"], expect_buffer(capi, want, words, 0, remap=remap), "remapped output")
    assert np.array_equal(got["out"][:T * C * W3].reshape(T, C, W3), bits(want).reshape(T, W3, C).transpose(0, 2, 1))


def test_sigma_rows_without_the_tiled_weights_are_refused(capi):
    A, W, _, _ = operands(3, 4, 16, 64, "none")
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_smallm(A, W, w_sig=False, a_sigma=True)
    assert e.value.code == PK_ERR_UNSUPPORTED


# ---- two row tiles per wave ----------------------------------------------------------------------------------------------------------------------
# (M, N): 4 row tiles, the minimum; 7 row tiles -- the last wave's second tile wholly out of range, its first partial; 8 tiles, the last partial
RT2_SHAPES = [(64, 3072), (100, 1760), (113, 1536)]
RT2_EPIS = ("none", "relu", "silu", "resid")
RT2_BELOW = (64, 3056)                                           # one column tile fewer than the first shape: just below the wave count that switches


@functools.lru_cache(maxsize=None)
def rt2_operands(M, N, K):
    return operands(M * 3 + N + K, M, N, K, "resid")


@functools.lru_cache(maxsize=None)
def rt2_linear(M, N, K):
    import oracle
    A, W, b, _ = rt2_operands(M, N, K)
    lin = oracle.linear(A, W, b)
    lin.setflags(write=False)
    return lin


@pytest.mark.parametrize("K", [256, 512], ids=["K256-one-ring-round", "K512"])
@pytest.mark.parametrize("M,N", RT2_SHAPES, ids=[f"{m}x{n}" for m, n in RT2_SHAPES])
def test_two_row_tile_kernel_matches_oracle(capi, orc, M, N, K):
    A, W, b, Rs = rt2_operands(M, N, K)
    lin = rt2_linear(M, N, K)
    for epi in RT2_EPIS:
        alpha = 0.5 if M == 100 else 1.0
        scols = N if epi == "silu" else 0                        # fc1 writes every column in the sigma order
        words = M * N + 11
        got = capi.diag_gemm_smallm(A, W, bias=b, epi=epi, resid=Rs if epi == "resid" else None, alpha=alpha, w_sig=True, a_sigma=True, sigma_cols=scols,
                                    out_words=words)
        assert got["form"] == ("rt2", epi, 4, True, False, False)
        want = epilogue(orc, lin, None, epi, Rs, alpha)
        assert_words(got["out"], expect_buffer(capi, want, words, N, scols), f"{epi}")


@pytest.mark.parametrize("K", [256, 512])
def test_just_below_the_two_row_tile_switch_the_chain_kernel_gives_the_same_bits(capi, orc, K):
    """The first RT2 shape without its last column tile: one wave per tile again, and every column it shares with the two-row-tile launch holds the same bits."""
    M, Nb = RT2_BELOW
    A, W, b, Rs = rt2_operands(M, RT2_SHAPES[0][1], K)
    lin = rt2_linear(M, RT2_SHAPES[0][1], K)
    depth = {256: 2, 512: 8}[K]
    for epi in RT2_EPIS:
        kw = dict(epi=epi, alpha=0.5, w_sig=True, a_sigma=True)
        below = capi.diag_gemm_smallm(A, W[:Nb], bias=b[:Nb], resid=Rs[:, :Nb] if epi == "resid" else None, **kw)
        assert below["form"] == ("chain", epi, depth, True, False, False)
        full = capi.diag_gemm_smallm(A, W, bias=b, resid=Rs if epi == "resid" else None, **kw)
        assert full["form"] == ("rt2", epi, 4, True, False, False)
        want = epilogue(orc, lin, None, epi, Rs, 0.5)
        assert_words(below["out"], bits(want[:, :Nb]), f"{epi}: chain kernel below the switch")
        assert_words(below["out"].reshape(M, Nb), full["out"].reshape(M, -1)[:, :Nb], f"{epi}: chain against two-row-tile kernel")


# ---- LayerNorm folded in -------------------------------------------------------------------------------------------------------------------------
def ln_params(seed, K):
    rng = np.random.default_rng(seed)
    return (1 + 0.1 * rng.standard_normal(K)).astype(np.float32), (0.1 * rng.standard_normal(K)).astype(np.float32)


LN_CASES = [(K, epi) for K in (512, 1024) for epi in LN_EPIS]


@pytest.mark.parametrize("K,epi", LN_CASES, ids=[f"K{k}-{e}" for k, e in LN_CASES])
def test_folded_layernorm_matches_oracle_and_the_separate_launches(capi, orc, K, epi):
    """N = 528: an odd number of column tiles, the last workgroup's second chain wave has none; M = 1 / 5 / 33: partial row tiles whose rows are clamped;
    M = 5 / 33 with a row pitch above K.  fused = 0 is LayerNorm (sigma columns) + the sigma chain kernel."""
    for M, N in itertools.product((1, 5, 16, 33), (528, 512)):
        lda = K + 4 if M in (5, 33) else K
        A, W, b, _ = operands(K + M * 13 + N, M, N, K, epi, lda)
        if M == 5:
            b = None
        g, be = ln_params(K + M, K)
        scols = N if M == 16 else 0
        X = orc.layer_norm(np.ascontiguousarray(A[:, :K]), g, be)
        want = product(orc, X, W, b, epi)
        words = M * N + 7
        buf = expect_buffer(capi, want, words, N, scols)
        kw = dict(bias=b, epi=epi, w_sig=True, a_sigma=True, sigma_cols=scols, out_words=words, ln=(g, be), lda_cols=K)
        fused = capi.diag_gemm_smallm(A, W, fused=True, **kw)
        assert fused["form"] == ("ln", epi, K // 64, True, False, False)
        assert_words(fused["out"], buf, f"folded M={M} N={N}")
        sep = capi.diag_gemm_smallm(A, W, fused=False, **kw)
        assert sep["form"] == ("chain", epi, 8, True, False, False)
        assert_words(sep["out"], buf, f"separate launches M={M} N={N}")


def test_folded_layernorm_is_refused_where_the_engine_does_not_fold(capi):
    g, be = ln_params(1, 256)
    A, W, _, _ = operands(4, 8, 32, 256, "none")
    with pytest.raises(capi.PkError) as e:                        # K = 256 has no folded kernel
        capi.diag_gemm_smallm(A, W, w_sig=True, ln=(g, be))
    assert e.value.code == PK_ERR_UNSUPPORTED
    g, be = ln_params(1, 512)
    A, W, _, Rs = operands(4, 8, 32, 512, "resid")
    for kw in (dict(w_sig=False), dict(w_sig=True, epi="resid", resid=Rs)):   # no tiled weights; an epilogue it is not instantiated for
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm(A, W, ln=(g, be), **kw)
        assert e.value.code == PK_ERR_UNSUPPORTED


# ---- a second norm in front ----------------------------------------------------------------------------------------------------------------------
PRE_SHAPES = [(32, 512, 512), (6, 1024, 1024), (33, 512, 1024)]   # the last: as many column-tile workgroups as 64-column chunks of pre_out, a partial row tile


@pytest.mark.parametrize("M,N,K", PRE_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in PRE_SHAPES])
def test_norm_in_front_of_the_folded_norm(capi, orc, M, N, K):
    A, W, b, _ = operands(M + N + K, M, N, K, "silu")
    pg, pb = ln_params(K + 1, K)
    g, be = ln_params(K + 2, K)
    Y1 = orc.layer_norm(A, pg, pb)
    want = orc.math_v("silu", orc.linear(orc.layer_norm(Y1, g, be), W, b))
    kw = dict(bias=b, epi="silu", w_sig=True, a_sigma=True, sigma_cols=N, ln=(g, be), pre=(pg, pb), out_words=M * N + 7)
    fused = capi.diag_gemm_smallm(A, W, fused=True, **kw)
    assert fused["form"] == ("ln", "silu", K // 64, True, False, True)
    assert_words(fused["pre_out"], bits(Y1), "pre_out: every row of the partial tile, every 64-column chunk")
    assert_words(fused["out"], expect_buffer(capi, want, M * N + 7, N, N), "product")
    sep = capi.diag_gemm_smallm(A, W, fused=False, **kw)
    assert sep["form"] == ("chain", "silu", 8, True, False, False)
    assert_words(sep["pre_out"], fused["pre_out"], "pre_out of launch_layernorm2")
    assert_words(sep["out"], fused["out"], "separate launches")


def test_norm_in_front_is_refused_past_one_round_of_workgroups(capi):
    M, N, K = 128, 1056, 512                                       # 8 row tiles x 33 column-tile pairs
    A, W, b, _ = operands(1, M, N, K, "silu")
    g, be = ln_params(2, K)
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_smallm(A, W, bias=b, epi="silu", w_sig=True, ln=(g, be), pre=(g, be))
    assert e.value.code == PK_ERR_UNSUPPORTED
    assert capi.diag_gemm_smallm(A, W, bias=b, epi="silu", w_sig=True, ln=(g, be))["form"] == ("ln", "silu", 8, True, False, False)   # (the plain fold has no such limit)


# ---- the depthwise-conv tail ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dw_case(d, M):
    """Operands of a conv-module product of M rows and, from the oracle, its GLU values (the same for every chunking of the rows into streams)."""
    import oracle
    A, W, b, _ = operands(d + M, M, d, d, "glu")
    g, be = ln_params(d + M + 1, d)
    X = oracle.layer_norm(A, g, be)
    glu = oracle.linear(X, W[:d], b[:d]) * oracle.math_v("sigmoid", oracle.linear(X, W[d:], b[d:]))
    rng = np.random.default_rng(d * 3 + M)
    conv = dict(w=(rng.standard_normal((9, d)) / 3).astype(np.float32), bias=(0.1 * rng.standard_normal(d)).astype(np.float32),
                bn_mean=(0.1 * rng.standard_normal(d)).astype(np.float32), bn_rstd=rng.uniform(0.5, 2.0, d).astype(np.float32),
                bn_g=rng.uniform(0.5, 1.5, d).astype(np.float32), bn_b=(0.1 * rng.standard_normal(d)).astype(np.float32))
    cache = wide_range(rng, (M, 8, d))                              # (the first M / c streams of it are used)
    return A, W, b, g, be, glu, conv, cache


DW_CASES = [(d, c, M) for d in (512, 1024) for c in (1, 2, 4) for M in (4, 20, 64)]


@pytest.mark.parametrize("d,c,M", DW_CASES, ids=[f"d{d}-c{c}-M{m}" for d, c, m in DW_CASES])
def test_depthwise_conv_tail(capi, d, c, M):
    """M = 20: the last row tile holds 4 rows -- four, two or one stream.  Two guard streams behind the caches and a guard behind the activations."""
    A, W, b, g, be, glu, conv, cache_all = dw_case(d, M)
    S = M // c
    cache = np.ascontiguousarray(cache_all[:S])
    for has_cache, out_sigma in itertools.product((0, 1), (0, 1)):
        dw = dict(c=c, has_cache=has_cache, out_sigma=out_sigma, cache_in=cache, cache_streams=S + 2, **conv)
        kw = dict(bias=b, epi="glu", w_sig=True, a_sigma=True, ln=(g, be), dw=dw, out_words=M * d + 7)
        fused = capi.diag_gemm_smallm(A, W, fused=True, **kw)
        assert fused["form"] == ("ln", "glu", d // 64, True, True, False)
        sep = capi.diag_gemm_smallm(A, W, fused=False, **kw)
        assert sep["form"] == ("chain", "glu", 8, True, False, False)
        what = f"has_cache={has_cache} out_sigma={out_sigma}"
        assert_words(fused["out"], sep["out"], f"{what}: activations against the separate conv launch")
        assert_words(fused["cache_out"], sep["cache_out"], f"{what}: cache_out against the separate conv launch")
        co = fused["cache_out"]
        assert np.all(co[S:] == capi.SKINNY_FILL32), f"{what}: a cache word outside the {S} streams was written"
        assert np.all(fused["out"][M * d:] == capi.SKINNY_FILL32), f"{what}: a word behind the activations was written"
        assert_words(co[:S, 8 - c:], bits(glu.reshape(S, c, d)), f"{what}: the new cache rows are the oracle's GLU values")
        assert_words(co[:S, :8 - c], bits(cache[:, c:]) if has_cache else np.zeros((S, 8 - c, d), np.uint32), f"{what}: the old cache rows, shifted")
        want, _ = R.stream_dwconv_f64(glu.reshape(S, c, d), cache, has_cache, conv["w"], conv["bias"], conv["bn_mean"], conv["bn_rstd"], conv["bn_g"], conv["bn_b"])
        got = fused["out"][:M * d].view(np.float32).reshape(M, d)
        if out_sigma:
            got = R.from_sigma(got)
        err, bound = np.abs(got - want.reshape(M, d)).max(), 1e-5 * (1.0 + np.abs(want).max())
        print(f"d={d} c={c} M={M} {what}: max |got - float64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, what


def test_conv_tail_is_refused_outside_its_chunk_sizes(capi):
    A, W, b, g, be, _, conv, cache = dw_case(512, 20)
    for c, M in ((5, 20), (3, 18)):                                  # (5 frames per stream; 3 does not divide a group of four rows)
        dw = dict(c=c, has_cache=1, cache_in=np.ascontiguousarray(cache[:M // c]), **conv)
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm(A[:M], W, bias=b, epi="glu", w_sig=True, ln=(g, be), dw=dw, fused=True)
        assert e.value.code == PK_ERR_UNSUPPORTED


# ---- the layouts the products read ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,ld", [(16, 64, 64), (48, 192, 192), (32, 1024, 1024), (48, 192, 200)])
def test_sigma_copy_is_the_reference_tiling(capi, rows, K, ld):
    src = wide_range(np.random.default_rng(rows + K + ld), (rows, ld))
    assert_words(bits(capi.diag_sigma_copy(src, K)), bits(R.w_sig_tiling(src, K)), "W_sig")


# 4095 / 4096 rows: either side of launch_layernorm's switch between its few-rows launch and its batch launch
LN_ROWS = [(d, rows) for d in (128, 512, 1024) for rows in (1, 7, 130)] + [(128, 4095), (128, 4096)]


@pytest.mark.parametrize("d,rows", LN_ROWS, ids=[f"d{d}-{r}rows" for d, r in LN_ROWS])
def test_layernorm_with_sigma_columns(capi, orc, d, rows):
    x = wide_range(np.random.default_rng(d + rows), (rows, d))
    g1, b1 = ln_params(d, d)
    g2, b2 = ln_params(d + 1, d)
    y1 = orc.layer_norm(x, g1, b1)
    y2 = orc.layer_norm(y1, g2, b2)
    assert_words(bits(capi.diag_layernorm_sigma(x, g1, b1)), bits(R.to_sigma(y1)), "launch_layernorm mode 2")
    assert_words(bits(capi.diag_layernorm(x, g1, b1)), bits(y1), "launch_layernorm")
    for sig in (False, True):
        o1, o2 = capi.diag_layernorm2(x, g1, b1, g2, b2, y2_sigma=sig)
        assert_words(bits(o1), bits(y1), f"launch_layernorm2 y1 (y2 sigma {sig})")
        assert_words(bits(o2), bits(R.to_sigma(y2) if sig else y2), f"launch_layernorm2 y2 (sigma {sig})")


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------
def test_every_form_has_a_case(capi):
    """The union of the forms the cases above assert they launch is every form the launcher can take."""
    have = {chain_want(K, epi, sig) for K, epi in CHAIN_CASES for sig in (False, True)}
    have |= {("rt2", epi, 4, True, False, False) for epi in RT2_EPIS}
    have |= {("ln", epi, K // 64, True, False, False) for K, epi in LN_CASES}
    have |= {("ln", "silu", K // 64, True, False, True) for _, _, K in PRE_SHAPES}
    have |= {("ln", "glu", d // 64, True, True, False) for d, _, _ in DW_CASES}
    every = set(capi.diag_gemm_smallm_forms())
    assert len(every) == 46
    assert every - have == set(), f"forms no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for forms the library does not list: {sorted(have - every)}"
