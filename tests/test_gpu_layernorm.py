"""The LayerNorm family alone (csrc/kernels/norm.hip through pk_diag_layernorm_form: exactly one launcher per call): launch_layernorm in its three output
modes and both of its branches, launch_layernorm2, launch_layernorm_stats and launch_layernorm_then_stats, at widths that fill a PER_LANE instantiation,
start one and leave its last 64-column chunk partial, and at row counts that leave the last workgroup of four waves partial.

Everything is BIT FOR BIT against the oracle (tests/layernorm_ref.py says how): fp32 values as they are, sigma columns through the reference permutation,
the bf16 store as the round-to-nearest-even of the oracle's fp32 value, the statistics as the numbers the oracle normalises with.  Every output buffer
comes back whole: the words behind the rows must still hold the fill pattern.  Every case first compares the form the library reports with the form the
case was written for (layernorm_ref.want_form); test_every_form_has_a_case compares the union of those with the library's table."""
import functools

import numpy as np
import pytest

import layernorm_ref as R
from conftest import pk  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


@functools.lru_cache(maxsize=None)
def params(d):
    """(g1, b1, g2, b2) of a width, the same for every case"""
    rng = np.random.default_rng(7000 + d)
    return R.make_params(rng, d) + R.make_params(rng, d)


def launch(capi, launcher, mode, x, p, eps=1e-5, in_place=False):
    """One launch; the form it reports is the form the case table states for it."""
    rows, d = x.shape
    got = capi.diag_layernorm_form(launcher, x, *p, eps=eps, mode=mode, in_place=in_place)
    assert got["form"] == R.want_form(launcher, rows, d), f"{launcher} {rows} x {d}: launched {got['form']}"
    return got


def launch_and_check(capi, orc, launcher, mode, x, p, eps=1e-5, what=""):
    got = launch(capi, launcher, mode, x, p, eps)
    R.check_launch(got, R.expected(orc, launcher, mode, x, *p, eps), f"{launcher} mode {mode} {x.shape[0]} x {x.shape[1]} eps {eps} {what}")
    return got


@pytest.mark.parametrize("d", R.WIDTHS)
def test_every_launcher_and_mode_matches_the_oracle(capi, orc, d):
    for rows in R.ROWS:
        x = R.make_x("wide", np.random.default_rng(rows * 2048 + d), rows, d)
        for launcher, mode in R.LAUNCHES:
            launch_and_check(capi, orc, launcher, mode, x, params(d))


@pytest.mark.parametrize("d", R.NATURAL_WIDTHS)
def test_widths_that_are_no_multiple_of_16(capi, orc, d):
    for rows in R.ROWS:
        x = R.make_x("wide", np.random.default_rng(rows * 2048 + d), rows, d)
        for launcher, mode in R.NATURAL_LAUNCHES:
            launch_and_check(capi, orc, launcher, mode, x, params(d))


@functools.lru_cache(maxsize=None)
def batch_rows(d):
    """4099 wide-range rows of a width (the shorter batches are its first rows)"""
    return R.make_x("wide", np.random.default_rng(4099 + d), 4099, d)


@pytest.mark.parametrize("rows", R.BATCH_ROWS)
@pytest.mark.parametrize("d", R.BATCH_WIDTHS)
def test_either_side_of_the_batch_branch(capi, orc, d, rows):
    x = np.ascontiguousarray(batch_rows(d)[:rows])
    for launcher, mode in R.LAUNCHES:
        launch_and_check(capi, orc, launcher, mode, x, params(d))


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_input_families_and_eps(capi, orc, family, eps):
    for d in R.FAMILY_WIDTHS:
        x = R.make_x(family, np.random.default_rng(31 * d + len(family)), R.FAMILY_ROWS, d)
        p = params(d)
        for launcher, mode in R.LAUNCHES:
            got = launch_and_check(capi, orc, launcher, mode, x, p, eps, family)
            if family == "const" and launcher == "stats":
                st = got["stats"][:2 * R.FAMILY_ROWS].view(np.float32).reshape(-1, 2)
                R.assert_words(R.bits(st[:, 0]), R.bits(R.CONSTANTS[:R.FAMILY_ROWS]), "mean of a constant row is the constant")
                rstd = np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(eps))
                assert np.all(R.bits(st[:, 1]) == R.bits(rstd)), f"rstd of a constant row is 1 / sqrt(eps): {st[:, 1]} vs {rstd}"
            if family == "const" and launcher == "norm" and mode == 0:
                y = got["y"][:x.size].view(np.float32).reshape(x.shape)
                R.assert_words(R.bits(y), R.bits(np.tile(p[1], (x.shape[0], 1))), "y of a constant row is beta")


@pytest.mark.parametrize("rows", R.TIE_ROWS)
@pytest.mark.parametrize("d", R.TIE_WIDTHS)
def test_bf16_store_rounds_ties_to_even(capi, orc, d, rows):
    """Constant rows give y == beta exactly; beta sits on, and one fp32 ulp either side of, the ties between bf16 numbers."""
    beta = R.tie_betas(d)
    R.assert_ties_tell_the_stores_apart(beta)
    x = R.make_x("const", None, rows, d)
    g1, _, g2, _ = params(d)
    n = rows * d
    want = np.tile(beta, (rows, 1))
    # launch_layernorm, mode 1
    p = (g1, beta, None, None)
    R.assert_words(R.bits(orc.layer_norm(x, g1, beta)), R.bits(want), "oracle: y == beta")
    got = launch_and_check(capi, orc, "norm", 1, x, p)
    R.check_bf16_store(got["y"].view(np.uint16)[:n], want, "launch_layernorm: bf16(beta)")
    # launch_layernorm2, y2 in mode 1: beta1 constant makes y1 a constant row again, so y2 == beta2
    p = (g1, np.full(d, 0.5, np.float32), g2, beta)
    got = launch_and_check(capi, orc, "norm2", 1, x, p)
    R.assert_words(got["y"][:n], R.bits(np.full(n, 0.5, np.float32)), "launch_layernorm2: y1 == beta1")
    R.check_bf16_store(got["y2"].view(np.uint16)[:n], want, "launch_layernorm2: bf16(beta2)")


@pytest.mark.parametrize("rows", R.IN_PLACE_ROWS)
@pytest.mark.parametrize("d", R.IN_PLACE_WIDTHS)
def test_in_place_gives_the_same_words(capi, orc, d, rows):
    """y == x (launch_layernorm, transformer.cpp) and y1 == x (launch_layernorm2, conformer_block.hpp; launch_layernorm_then_stats): every load of a row
    precedes its stores, so the aliased launch leaves the words of the separate one."""
    x = R.make_x("wide", np.random.default_rng(d + rows), rows, d)
    p = params(d)
    for launcher, mode in (("norm", 0), ("norm2", 0), ("norm2", 1), ("norm2", 2), ("then_stats", 0)):
        apart = launch_and_check(capi, orc, launcher, mode, x, p)
        aliased = launch(capi, launcher, mode, x, p, in_place=True)
        for name in apart:
            if name != "form":
                R.assert_words(aliased[name], apart[name], f"{launcher} mode {mode} in place: {name}")


@pytest.mark.parametrize("d", R.PLACE_WIDTHS)
def test_a_row_is_independent_of_its_place(capi, orc, d):
    """The same row alone, as row 3 of 5 and as row 4098 of 4099 (the last wave of a partial last workgroup; launch_layernorm's batch branch)."""
    row = R.make_x("wide", np.random.default_rng(99 + d), 1, d)
    p = params(d)
    places = ((1, 0), (5, 3), (4099, 4098))
    others = batch_rows(min(w for w in R.BATCH_WIDTHS if w >= d))    # the rows around it: any will do
    for launcher, mode in R.LAUNCHES:
        seen = []
        for rows, at in places:
            x = np.ascontiguousarray(others[:rows, :d])
            x[at] = row[0]
            got = launch(capi, launcher, mode, x, p)
            part = {}
            for name in got:
                if name == "form":
                    continue
                half = mode == 1 and name == ("y" if launcher == "norm" else "y2")
                width = 2 if name == "stats" else d
                elems = got[name].view(np.uint16) if half else got[name]
                part[name] = elems[at * width:(at + 1) * width].copy()
            seen.append(part)
        for other, (rows, at) in zip(seen[1:], places[1:]):
            for name in seen[0]:
                R.assert_words(other[name], seen[0][name], f"{launcher} mode {mode}: {name} of the row at {at} of {rows}")
    alone = R.expected(orc, "norm", 0, row, *p, 1e-5)["y"][0]
    R.assert_words(R.bits(alone), launch(capi, "norm", 0, row, p)["y"][:d], "the row alone")


def test_every_form_has_a_case(capi):
    """The union of the forms the cases above assert they launch (layernorm_ref.all_cases lists them) is every form the launchers can take."""
    have = R.case_forms()
    every = set(capi.diag_layernorm_forms())
    assert len(every) == 15
    assert every - have == set(), f"forms no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for forms the library does not list: {sorted(have - every)}"
