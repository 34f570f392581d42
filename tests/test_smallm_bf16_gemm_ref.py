"""tests/smallm_bf16_gemm_ref.py checked on the CPU: the layouts are bijections and round trips, the folded reference equals an independent numpy LayerNorm +
matmul, the reference's own excused share of every bf16-rows case of tests/test_gpu_smallm_bf16_gemm.py stays under the cap that file asserts -- and, host
arithmetic of the library, every case of that file is written for the form the launcher's own function reports for it."""
import numpy as np
import pytest

import smallm_bf16_gemm_ref as R
import test_gpu_smallm_bf16_gemm as G
from conftest import pk  # noqa: F401


@pytest.mark.parametrize("M,cols", [(8, 32), (16, 96), (128, 768), (24, 4096)])
def test_t8_offsets_are_a_bijection_and_round_trip(M, cols):
    off = R.t8_offsets(M, cols)
    assert np.array_equal(np.sort(off.reshape(-1)), np.arange(M * cols))
    x = np.arange(M * cols, dtype=np.int64).reshape(M, cols) * 3 + 1
    assert np.array_equal(R.from_t8(R.to_t8(x), M, cols), x)
    # the tile of (row, k) starts at 256 ((row / 8) (cols / 32) + k / 32); inside it 8 consecutive k are contiguous and the 8 rows of a k group 8 elements apart
    assert off[0, 0] == 0 and off[1, 0] == 8 and off[0, 8] == 64 and (cols == 32 or off[0, 32] == 256) and (M == 8 or off[8, 0] == 256 * (cols // 32))
    assert np.array_equal(off[:, 1:8] - off[:, 0:7], np.ones((M, 7), np.int64))


def test_w_t16_tiling_is_a_permutation_with_one_kb_per_tile():
    rows, K = 48, 96
    idx = np.arange(rows * (K + 8), dtype=np.int64).reshape(rows, K + 8)
    t = R.w_t16_tiling(idx, K)
    assert np.array_equal(np.sort(t), np.sort(idx[:, :K].reshape(-1)))
    tile = t.reshape(rows // 16, K // 32, 64, 8)
    assert tile[1, 2, 5 + 16 * 3, 4] == idx[16 + 5, 64 + 24 + 4]
    assert set((tile[2, 1] // (K + 8)).reshape(-1)) == set(range(32, 48)) and set((tile[2, 1] % (K + 8)).reshape(-1)) == set(range(32, 64))


@pytest.mark.parametrize("epi", ("none", "relu", "silu", "resid", "glu"))
def test_folded_reference_equals_numpy_layernorm_and_matmul(epi):
    rng = np.random.default_rng(11)
    M, N, K = 9, 24, 256
    A = (rng.standard_normal((M, K)) * 2 + 1).astype(np.float32)
    g, b = rng.uniform(0.5, 1.5, K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    W = rng.standard_normal((2 * N if epi == "glu" else N, K)).astype(np.float32) / 16
    bias = rng.standard_normal(W.shape[0]).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    p = R.folded_product(A, g, b, W, bias, epi, resid if epi == "resid" else None, 0.5)
    x = A.astype(np.float64)
    x = (x - x.mean(1)[:, None]) / np.sqrt(x.var(1)[:, None] + 1e-5) * g + b
    xq = R.bf16_value(R.bf16_bits(x.astype(np.float32))).astype(np.float64)
    wq = R.bf16_value(R.bf16_bits(W)).reshape(W.shape).astype(np.float64)
    z = np.einsum("mk,nk->mn", xq.reshape(M, K), wq) + bias
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    want = {"none": lambda: z, "relu": lambda: np.maximum(z, 0), "silu": lambda: z * sig(z), "resid": lambda: resid + 0.5 * z,
            "glu": lambda: z[:, :N] * sig(z[:, N:])}[epi]()
    assert np.allclose(p["want"], want, rtol=1e-12, atol=1e-12)
    assert p["flip"].shape == (M, N) and np.all(p["flip"] > 0)


@pytest.mark.parametrize("M,N,K,epi,ln", R.BF16_ROWS_CASES, ids=[f"{e}-{'ln' if l else 'a16'}" for _, _, _, e, l in R.BF16_ROWS_CASES])
def test_excused_share_of_the_reference_stays_under_the_cap(M, N, K, epi, ln):
    k = R.bf16_rows_case(M, N, K, epi, ln)
    share = R.excused_share(k["p"]["want"], k["delta"])
    print(f"{epi} ln={ln}: the reference excuses {100 * share:.2f} %")
    assert share <= 0.02
    R.check_bf16_rows(R.bf16_bits(k["p"]["want"].astype(np.float32)), k["p"]["want"], k["delta"])   # the correctly rounded reference passes its own check


def form_of(capi, form, M, N, K, c=0, **kw):
    return capi.diag_gemm_smallm_bf16_form(M, N, K, epi=form[0], a16=form[4], ln=form[5], pre=form[11], dw_c=c if form[8] else 0, w_tiles=form[7], a_t8=form[9], **kw)


def test_every_gpu_case_names_the_form_the_launcher_reports():
    """Host arithmetic, no device: the table of forms, and for every case of the GPU file the form its product would launch."""
    from parakeet_cpp_amd import capi
    every = capi.diag_gemm_smallm_bf16_forms()
    assert len(every) == 154 and len(set(every)) == 154 and {c[0] for c in G.CASES} == set(every)
    for form, M, N, K, c in G.CASES:
        assert form_of(capi, form, M, N, K, c) == form, (form, M, N, K)
    for form in G.PITCH_FORMS + G.WT_FORMS + G.AT_FORMS + G.EPI_FORMS + G.FAST_FORMS:
        M, N, K, c = G.shape_of(form)
        assert form_of(capi, form, M, N, K, c, lda=K + 8 if not form[9] else None, ldw=K + 8, ldo=N + 4, ldr=N + 12) == form
        for drop in (("wt", "al"), ("at",)):
            assert G.without(form, *drop) in every
    for form, M, N, K in G.T8_CASES:
        assert form_of(capi, form, M, N, K, out_bf16=True, out_t8=True) == form
    for form, c, S, _ in G.DW_CASES:
        N, K = (3072, 256) if form[3] == 16 else (272, 512)
        assert form_of(capi, form, c * S, N, K, c, cache_streams=S + 2) == form and form_of(capi, G.without(form, "dw"), c * S, N, K) == G.without(form, "dw")
    for M, N, K, epi, ln in R.BF16_ROWS_CASES:
        assert form_of(capi, (epi,) + G.BF16_FORMS[ln][1:], M, N, K, out_bf16=True, ldo=N + 3) == (epi,) + G.BF16_FORMS[ln][1:]


def test_every_refusal_of_the_gpu_file_is_refused_without_a_device():
    from parakeet_cpp_amd import capi
    for kw in G.REFUSED:
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm_bf16_form(**kw)
        assert e.value.code == G.PK_ERR_UNSUPPORTED, kw
    for kw in (dict(M=0, N=16, K=256), dict(M=8, N=16, K=256, lda=128), dict(M=8, N=16, K=256, ldo=8), dict(M=8, N=16, K=256, out_words=100),
               dict(M=8, N=16, K=256, out_bf16=True, out_words=63), dict(M=8, N=256, K=256, epi="silu", pre=True, ln=True, pre_out_words=100),
               dict(M=8, N=16, K=256, epi="resid", ldr=8), dict(M=8, N=16, K=256, epi="silu", resid_in_place=True), dict(M=8, N=256, K=256, epi="glu", dw_c=2, cache_streams=3)):
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm_bf16_form(**kw)
        assert e.value.code == -1, kw
