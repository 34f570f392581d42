"""The fp32 tile GEMM family alone (csrc/kernels/gemm.hip + gemm_pipe.hpp through pk_diag_gemm_tile: one product per call): the one-K-tile kernel,
the double-buffered 64 x 64 and 128 x 64 tiles, the wide single-buffered 128 x 128 tile with and without the LayerNorm folded into its A staging, and the
long-K single-round tile -- every instantiation launch_gemm can take, at the smallest shapes that still reach it.

Every product is compared BIT FOR BIT with the oracle (orc.linear / orc.layer_norm / orc.math_v): exact mode has no tolerance.  Inputs span 2^-10 .. 2^10
(wide_range of tests/test_gpu_gemm_schedule.py), so any change in the k order of an output's fma chain shows in the bits.  The output buffer comes back whole
and exactly as the kernel wrote it: tests/smallm_gemm_ref.py says where every element belongs (row pitch, sigma columns, the subsampling remap), and every
other word must still hold the fill pattern.  The operand pitches are padded with NaN on the device.  Each case names the form it is written for and compares
it with the form the launcher's own function reports (no threshold is restated here); test_every_form_has_a_case compares the union of those with the
library's table, so an instantiation without a case fails the suite."""
import functools

import numpy as np
import pytest

import smallm_gemm_ref as R
from conftest import pk  # noqa: F401
from test_gpu_gemm_schedule import bits, wide_range
from test_gpu_smallm_gemm import assert_words, epilogue, expect_buffer, ln_params

pytestmark = pytest.mark.gpu

PK_ERR_UNSUPPORTED = -7
FOUR = ("none", "relu", "silu", "resid")
LN_EPIS = ("none", "relu", "silu")


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


def form(kind, epi, lna=False):
    """The capi.tile_form tuple a case is written for."""
    if kind == "nt64":
        return ("nt", (64, 64), 2, False, 0, epi)
    if kind == "nt128":
        return ("nt", (128, 128), 2, False, 0, epi)
    if kind == "longk":                                              # 2 x 4 waves of 64 x 32; without an epilogue function the compiler-placed loop
        return ("pipe", (2, 4, 2, 1), 1, False, 0 if epi == "none" else 2, epi)
    if kind == "wide":                                               # 4 x 2 waves of 32 x 64, single-buffered, hand-placed loop
        return ("pipe", (4, 2, 1, 2), 1, lna, 2, epi)
    if kind == "t128x64":
        return ("pipe", (2, 2, 2, 1), 2, False, 0, epi)
    assert kind == "t64x64"
    return ("pipe", (2, 2, 1, 1), 2, False, 0, epi)


@functools.lru_cache(maxsize=None)
def ops(M, N, K, glu):
    """A [M][K], asymmetric W [N or 2N][K], bias, residual [M][N]: one set per shape, shared by every case on it and never written."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + (1 << 20 if glu else 0))
    rows = 2 * N if glu else N
    out = (wide_range(rng, (M, K)), (wide_range(rng, (rows, K)) / np.float32(np.sqrt(K))).astype(np.float32), rng.standard_normal(rows).astype(np.float32),
           wide_range(rng, (M, N)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lin(M, N, K, glu, bias=True, ln=False):
    """The oracle's X W^T (+ bias) of ops(M, N, K, glu), X = A or LayerNorm(A; ln_params(K, K)): (product, None) or (value half, gate half).  Once per shape."""
    import oracle
    A, W, b, _ = ops(M, N, K, glu)
    X = oracle.layer_norm(A, *ln_params(K, K)) if ln else A
    if glu:
        out = (oracle.linear(X, W[:N], b[:N] if bias else None), oracle.linear(X, W[N:], b[N:] if bias else None))
    else:
        out = (oracle.linear(X, W, b if bias else None), None)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def launch(capi, want_form, A, W, b, Rs, want, epi, what, alpha=1.0, ln=None, ldo=None, sigma_cols=0, remap=None, words=None, **kw):
    """One product alone: the form it ran on is the one the case is written for, and the whole buffer is `want` where GemmArgs puts it, the fill elsewhere."""
    M, N = want.shape
    ldo_ = ldo or N
    words = words or (M - 1) * ldo_ + N + 7
    got = capi.diag_gemm_tile(A, W, bias=b, epi=epi, resid=Rs if epi == "resid" else None, alpha=alpha, ln=ln, ldo=ldo, sigma_cols=sigma_cols, remap=remap,
                              out_words=words, **kw)
    assert got["form"] == want_form, what
    assert_words(got["out"], expect_buffer(capi, want, words, ldo_, sigma_cols, remap), what)
    return got["out"]


def run(capi, orc, kind, M, N, K, epi, bias=True, alpha=1.0, ln=False, **kw):
    glu = epi == "glu"
    A, W, b, Rs = ops(M, N, K, glu)
    want = epilogue(orc, *lin(M, N, K, glu, bias, ln), epi, Rs, alpha)
    return launch(capi, form(kind, epi, ln), A, W, b if bias else None, Rs, want, epi, f"{kind} {M}x{N}x{K} {epi} bias={bias} alpha={alpha} ln={ln} {kw}",
                  alpha=alpha, ln=ln_params(K, K) if ln else None, **kw)


# ---- every form at the smallest shapes that reach it ------------------------------------------------------------------------------------------------
# The wide and the long-K tile finish their 128 rows in two bands of 64 (NPASS = 2).  1540 = 12 x 128 + 4, 1030 = 8 x 128 + 6 and 1550 = 12 x 128 + 14 end
# inside the first band of the last row tile, 1636 = 12 x 128 + 100 inside the second, 1600 = 12 x 128 + 64 exactly between them.
SHAPES = {
    "nt64": [(70, 70, 32), (1, 5, 32)],                             # K < 64; partial tiles both ways, one row
    "t64x64": [(70, 70, 96), (1540, 40, 64), (70, 70, 160)],        # M < 1024 through K % 64 != 0, 3 K tiles; N < 256, 2 K tiles; 5 K tiles
    # 33 K tiles, partial row and column tiles; N = 512 at the fewest rows and the shortest K that still take this tile (M >= 1024, K >= 1024 with
    # K % 64 != 0 -- a K % 64 == 0 this small is a single round of 128 x 128 tiles, the long-K form): 0.55 G multiply-adds, the largest product here
    "t128x64": [(1030, 260, 1056), (1024, 512, 1056)],
    "wide": [(1540, 260, 64), (1030, 260, 96), (1540, 1028, 128), (1550, 260, 96), (1636, 260, 96)],   # 2 / 3 / 4 K tiles
    "longk": [(1540, 260, 1024), (1600, 256, 1088)],                # 32 / 34 K tiles
}
GLU_SHAPES = {"nt128": [(130, 70, 32)], "wide": [(100, 40, 96), (1540, 260, 64)]}   # K < 64; one partial tile; 13 x 5 tiles
FORM_CASES = [(kind, M, N, K, epi) for kind, shapes in SHAPES.items() for M, N, K in shapes for epi in FOUR]
FORM_CASES += [(kind, M, N, K, "glu") for kind, shapes in GLU_SHAPES.items() for M, N, K in shapes]
LNA_CASES = [(1540, 1028, K, epi) for K in (64, 96) for epi in LN_EPIS] + [(1540, 40, 96, "glu")]
MAP_SHAPES = {"wide": (1540, 260, 64), "t128x64": (1030, 260, 1056), "t64x64": (1540, 40, 64)}   # the output mappings and pitches run on these
MAP_KINDS = tuple(MAP_SHAPES)


@pytest.mark.parametrize("kind,M,N,K,epi", FORM_CASES, ids=[f"{k}-{m}x{n}x{kk}-{e}" for k, m, n, kk, e in FORM_CASES])
def test_every_form_matches_oracle(capi, orc, kind, M, N, K, epi):
    run(capi, orc, kind, M, N, K, epi, alpha=0.5 if M % 4 == 2 else 1.0)


@pytest.mark.parametrize("M,N,K,epi", LNA_CASES, ids=[f"{m}x{n}x{k}-{e}" for m, n, k, e in LNA_CASES])
def test_layernorm_fold_matches_oracle_and_the_unfolded_product(capi, orc, M, N, K, epi):
    """The statistics pass + the fold into the A staging against LayerNorm + product from the oracle, and against the same tile without the fold on the
    oracle's normalised rows; the fold with a padded row pitch of A."""
    folded = run(capi, orc, "wide", M, N, K, epi, ln=True)
    glu = epi == "glu"
    A, W, b, Rs = ops(M, N, K, glu)
    X = orc.layer_norm(A, *ln_params(K, K))
    want = epilogue(orc, *lin(M, N, K, glu, True, True), epi)
    unfolded = launch(capi, form("wide", epi), X, W, b, Rs, want, epi, "un-folded product on the oracle's normalised rows")
    assert_words(folded, unfolded, "folded against un-folded")
    assert_words(run(capi, orc, "wide", M, N, K, epi, ln=True, lda=K + 4), folded, "fold with lda = K + 4")


def test_layernorm_fold_is_refused_on_the_long_k_tile(capi):
    M, N, K = 1540, 1028, 1024                                       # 13 x 9 tiles of 128 x 128: a single round, so the long-K tile -- it has no LNA form
    assert capi.diag_gemm_tile_form(M, N, K, epi="silu") == form("longk", "silu")
    with pytest.raises(capi.PkError) as e:
        capi.diag_gemm_tile(np.zeros((M, K), np.float32), np.zeros((N, K), np.float32), epi="silu", ln=ln_params(1, K))
    assert e.value.code == PK_ERR_UNSUPPORTED
    with pytest.raises(capi.PkError) as e:                           # (nor has any tile a fold in front of the residual epilogue)
        capi.diag_gemm_tile(np.zeros((M, 64), np.float32), np.zeros((N, 64), np.float32), epi="resid", resid=np.zeros((M, N), np.float32), ln=ln_params(1, 64))
    assert e.value.code == PK_ERR_UNSUPPORTED


# ---- output mappings and pitches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MAP_KINDS)
def test_sigma_columns_on_the_wide_and_the_scalar_epilogue(capi, orc, kind):
    """sigma_cols = 0, a multiple of 16 inside the row, and N rounded down to 16 (the columns behind it stay natural): through the LDS epilogue (ldo % 4 == 0)
    and, with ldo = N + 3, through the scalar one -- the same words at the same (row, column)."""
    M, N, K = MAP_SHAPES[kind]
    for sc in (0, 48 if N > 64 else 16, N // 16 * 16):
        for epi in ("none", "silu"):
            wide = run(capi, orc, kind, M, N, K, epi, sigma_cols=sc)
            scalar = run(capi, orc, kind, M, N, K, epi, sigma_cols=sc, ldo=N + 3)
            assert_words(scalar[R.output_offsets(M, N, N + 3, sc)], wide[R.output_offsets(M, N, N, sc)], f"sigma_cols={sc} {epi}: scalar against wide epilogue")


def test_sigma_columns_are_refused_where_no_tile_epilogue_has_them(capi):
    """GLU: the wide epilogue's sigma read knows no value / gate mapping.  Residual: the wide epilogue would add it by output position.  A status, no launch."""
    M, N, K = 100, 40, 96
    A, W, b, Rs = ops(M, N, K, True)
    for kw in (dict(epi="glu"), dict(epi="resid", resid=Rs)):
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_tile(A, W if kw["epi"] == "glu" else W[:N], sigma_cols=16, **kw)
        assert e.value.code == PK_ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_each_scalar_epilogue_selector_alone_gives_the_wide_epilogue_words(capi, orc, kind):
    """ldo = N + 3, ldr = N + 1 and N + 1 columns (N % 4 != 0) each send the product through the scalar epilogue; ldo = N + 4 and ldr = N + 4 keep it on the
    wide one with padded pitches.  All equal the oracle, so each other on the elements they share."""
    M, N, K = MAP_SHAPES[kind]
    A, W, b, Rs = ops(M, N + 1, K, False)                            # one more column than the tile-aligned product: its first N are the shared ones
    full = epilogue(orc, *lin(M, N + 1, K, False), "resid", Rs, 0.5)
    Wn, bn, Rn, want = W[:N], b[:N], np.ascontiguousarray(Rs[:, :N]), np.ascontiguousarray(full[:, :N])
    f = form(kind, "resid")
    base = launch(capi, f, A, Wn, bn, Rn, want, "resid", "wide epilogue", alpha=0.5).reshape(-1)[:M * N].reshape(M, N)
    for what, kw in (("ldo = N + 3", dict(ldo=N + 3)), ("ldr = N + 1", dict(ldr=N + 1)), ("ldo = N + 4", dict(ldo=N + 4)), ("ldr = N + 4", dict(ldr=N + 4))):
        got = launch(capi, f, A, Wn, bn, Rn, want, "resid", what, alpha=0.5, **kw)
        assert_words(got[R.output_offsets(M, N, kw.get("ldo", N))], base, f"{what} against the wide epilogue")
    got = launch(capi, f, A, W, b, Rs, full, "resid", "N % 4 != 0", alpha=0.5)
    assert_words(got[R.output_offsets(M, N + 1, N + 1)][:, :N], base, "N % 4 != 0 against the wide epilogue")


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_padded_operand_pitches_no_bias_and_alpha(capi, orc, kind):
    """lda = K + 4 and ldw = K + 8 with NaN behind every row: a load past K poisons the result.  No bias: nothing is added at all."""
    M, N, K = MAP_SHAPES[kind]
    for epi in ("silu", "resid"):
        dense = run(capi, orc, kind, M, N, K, epi, alpha=0.5)
        assert_words(run(capi, orc, kind, M, N, K, epi, alpha=0.5, lda=K + 4, ldw=K + 8), dense, f"{epi}: padded operand pitches")
    for epi in ("none", "resid"):
        run(capi, orc, kind, M, N, K, epi, bias=False, alpha=0.5)
        run(capi, orc, kind, M, N, K, epi, bias=False, alpha=0.5, ldo=N + 3)


def test_glu_pitches_no_bias_and_the_scalar_epilogue(capi, orc):
    M, N, K = GLU_SHAPES["wide"][1]
    dense = run(capi, orc, "wide", M, N, K, "glu")
    assert_words(run(capi, orc, "wide", M, N, K, "glu", lda=K + 4, ldw=K + 8), dense, "padded operand pitches")
    scalar = run(capi, orc, "wide", M, N, K, "glu", ldo=N + 3)
    assert_words(scalar[R.output_offsets(M, N, N + 3)].reshape(-1), dense[:M * N], "scalar against wide epilogue")
    run(capi, orc, "wide", M, N, K, "glu", ldo=N + 4)
    run(capi, orc, "wide", M, N, K, "glu", bias=False)
    run(capi, orc, "nt128", *GLU_SHAPES["nt128"][0], "glu", bias=False, ldo=75, lda=36, ldw=40)


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_subsampling_remap(capi, orc, kind):
    """The last subsampling conv's pattern on a tile kernel: row (t, w) column c goes to out[t][c][w] (remap_rows = W3, gs = C W3, rs = 1, cs = W3)."""
    M, C, K = MAP_SHAPES[kind]
    W3 = 10
    T = M // W3
    assert T * W3 == M
    words = T * C * W3 + 9
    got = run(capi, orc, kind, M, C, K, "relu", remap=(W3, C * W3, 1, W3), words=words)
    want = epilogue(orc, *lin(M, C, K, False), "relu")
    assert np.array_equal(got[:T * C * W3].reshape(T, C, W3), bits(want).reshape(T, W3, C).transpose(0, 2, 1))


# ---- the MFMA C layout ------------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_CASES = [("nt64", 70, 70, 32, "none"), ("nt128", 130, 70, 32, "glu"), ("t64x64", 70, 70, 96, "none"), ("t128x64", 1030, 260, 1056, "none"),
                   ("wide", 1540, 260, 64, "none"), ("wide", 1540, 260, 64, "glu"), ("longk", 1540, 260, 1024, "none"), ("longk", 1540, 260, 1024, "relu")]


@pytest.mark.parametrize("kind,M,N,K,epi", TRANSPOSE_CASES, ids=[f"{k}-{e}" for k, _, _, _, e in TRANSPOSE_CASES])
def test_identity_rows_return_the_transposed_weights(capi, orc, kind, M, N, K, epi):
    """A = the first M rows of I (zero rows below K), an asymmetric W of exact values and no bias: out[m][n] is W[n][m] itself (GLU: the gate weights are
    zero, so every value is multiplied by the oracle's sigmoid(0)) -- a row / column swap anywhere in the tile shows."""
    A = np.eye(M, K, dtype=np.float32)
    W = np.arange(N * K, dtype=np.float32).reshape(N, K) * np.float32(0.25)
    want = np.zeros((M, N), np.float32)
    want[:min(M, K)] = W.T[:min(M, K)]
    if epi == "glu":
        W = np.concatenate([W, np.zeros_like(W)])
        want = want * orc.math_v("sigmoid", np.zeros(1, np.float32))[0]
    launch(capi, form(kind, epi), A, W, None, None, want, epi, "A = I")


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_form_has_a_case(capi):
    """The union of the forms the cases above assert they launch is every form the launcher can take."""
    have = {form(kind, epi) for kind, _, _, _, epi in FORM_CASES} | {form("wide", epi, True) for _, _, _, epi in LNA_CASES}
    every = set(capi.diag_gemm_tile_forms())
    assert len(every) == 26
    assert every - have == set(), f"forms no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for forms the library does not list: {sorted(have - every)}"
