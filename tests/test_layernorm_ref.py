"""CPU checks of tests/layernorm_ref.py, the specification of tests/test_gpu_layernorm.py: the oracle's new {mean, rstd} are the numbers its layer_norm
normalises with and sit within the derived distance of float64; a planted fault does not; the bf16 checker accepts round-to-nearest-even alone on the
tie rows; and the case table reaches every instantiation the library lists."""
import numpy as np
import pytest

import bf16_gemm_ref as B
import layernorm_ref as R

STAT_WIDTHS = R.WIDTHS + R.NATURAL_WIDTHS


def family_rows(family, d, rows=9):
    return R.make_x(family, np.random.default_rng(1000 + d), rows, d)


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_statistics_are_within_the_derived_bound_of_float64(orc, family, eps):
    for d in STAT_WIDTHS:
        x = family_rows(family, d)
        st = orc.layer_norm_stats(x, eps)
        assert st.shape == (x.shape[0], 2) and st.dtype == np.float32
        err_mean, err_rstd = R.stats_errors(st, x, eps)
        e_mean, e_rstd = R.stats_bounds(x, eps)
        assert np.all(err_mean <= e_mean), (family, d, eps, float((err_mean - e_mean).max()))
        assert np.all(err_rstd <= e_rstd), (family, d, eps, float((err_rstd / e_rstd).max()))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_statistics_are_the_numbers_layer_norm_normalises_with(orc, family):
    """y of orc.layer_norm == fma((x - mean) * rstd, gamma, beta) with the {mean, rstd} orc.layer_norm_stats returns, bit for bit: gamma = 1 and beta = 0
    make the fma exact, so y is the product itself."""
    for d in STAT_WIDTHS:
        for eps in R.EPS:
            x = family_rows(family, d)
            st = orc.layer_norm_stats(x, eps)
            y = orc.layer_norm(x, np.ones(d, np.float32), np.zeros(d, np.float32), eps)
            want = (x - st[:, :1]) * st[:, 1:]
            R.assert_words(R.bits(y), R.bits(want + np.float32(0.0)), f"{family} d {d} eps {eps}")      # (+ 0: the fma's sum turns a -0 product into +0)
            R.assert_words(R.bits(st), R.bits(R.stats_emulated(x, eps)), f"numpy restatement, {family} d {d} eps {eps}")


def test_constant_rows_have_variance_zero_and_give_beta(orc):
    for d in STAT_WIDTHS:
        x = R.make_x("const", None, len(R.CONSTANTS), d)
        g, b = R.make_params(np.random.default_rng(d), d)
        for eps in R.EPS:
            st = orc.layer_norm_stats(x, eps)
            R.assert_words(R.bits(st[:, 0]), R.bits(R.CONSTANTS), f"mean of constant rows, d {d}")
            rstd = np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(eps))
            assert np.all(R.bits(st[:, 1]) == R.bits(rstd)), f"rstd of constant rows, d {d}, eps {eps}"
            R.assert_words(R.bits(orc.layer_norm(x, g, b, eps)), R.bits(np.tile(b, (x.shape[0], 1))), f"y == beta, d {d}, eps {eps}")


@pytest.mark.parametrize("fault", ["raw_moment", "bessel"])
def test_a_planted_fault_exceeds_the_bound(fault):
    """Rows of mean 1 and spread 1: a variance taken without subtracting the mean, or divided by d - 1, moves rstd past the bound in every row."""
    for d in (32, 160, 1024):
        x = (1.0 + np.random.default_rng(d).standard_normal((16, d))).astype(np.float32)
        _, e_rstd = R.stats_bounds(x, 1e-5)
        _, good = R.stats_errors(R.stats_emulated(x, 1e-5), x, 1e-5)
        _, bad = R.stats_errors(R.stats_emulated(x, 1e-5, fault), x, 1e-5)
        assert np.all(good <= e_rstd)
        assert np.all(bad > e_rstd), (fault, d, float((bad / e_rstd).min()))


@pytest.mark.parametrize("d", R.TIE_WIDTHS)
def test_the_bf16_checker_accepts_nearest_even_only(orc, d):
    """On the tie rows (constant x, so y == beta == the tie values) the checker takes the nearest-even store and rejects a truncating and a
    round-half-up one."""
    beta = R.tie_betas(d)
    R.assert_ties_tell_the_stores_apart(beta)
    assert np.all(np.isfinite(beta)) and np.all(np.abs(beta) >= 2.0 ** -9) and np.all(np.abs(beta) <= 2.0 ** 10)
    x = R.make_x("const", None, 5, d)
    g, _ = R.make_params(np.random.default_rng(d), d)
    y = orc.layer_norm(x, g, beta)
    R.assert_words(R.bits(y), R.bits(np.tile(beta, (5, 1))), "y == beta on constant rows")
    R.check_bf16_store(B.bf16_bits(y).reshape(-1), y, "nearest even")
    for wrong in (R.bf16_truncate, R.bf16_half_up):
        with pytest.raises(AssertionError):
            R.check_bf16_store(wrong(y).reshape(-1), y, wrong.__name__)
        buf = R.expect_buffer(wrong(y).reshape(-1), (y.size + 1) // 2 + 3)
        with pytest.raises(AssertionError):
            R.check_output(buf, y, 1, wrong.__name__)
    R.check_output(R.expect_buffer(B.bf16_bits(y).reshape(-1), (y.size + 1) // 2 + 3), y, 1, "nearest even, whole buffer")


def test_whole_buffer_checker_sees_a_store_outside_the_rows():
    y = np.arange(15, dtype=np.float32).reshape(3, 5)
    for mode, dt in ((0, np.uint32), (1, np.uint16)):
        buf = R.expect_buffer(R.payload(y, mode), 20)
        R.check_output(buf, y, mode, "clean")
        dirty = buf.copy()
        dirty.view(dt)[15] ^= 1                                   # the first element behind the rows
        with pytest.raises(AssertionError):
            R.check_output(dirty, y, mode, "one element past the end")
    y16 = np.arange(32, dtype=np.float32).reshape(2, 16)
    assert np.array_equal(R.payload(y16, 2)[:16].view(np.float32), [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15])


def test_case_table_reaches_every_instantiation():
    from parakeet_cpp_amd import capi
    every = capi.diag_layernorm_forms()
    assert len(every) == 15 and len(set(every)) == 15
    have = R.case_forms()
    assert set(every) - have == set(), f"instantiations no case launches: {sorted(set(every) - have)}"
    assert have - set(every) == set(), f"cases written for forms the library does not list: {sorted(have - set(every))}"
    # the table's own statements agree with the launchers' form functions
    for launcher, _, rows, d in R.all_cases():
        assert capi.diag_layernorm_form_of(launcher, rows, d) == R.want_form(launcher, rows, d), (launcher, rows, d)
    for _, mode, _, d in R.all_cases():
        assert mode != 2 or d % 16 == 0
