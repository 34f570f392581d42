"""The two references of the streaming encoder's cached attention (tests/stream_attention_ref.py) against each other: CPU only.

* ACCEPT: at every case tests/test_gpu_stream_attention.py runs, with the very inputs it runs them on (unused cache and table rows NaN), the
  bit-exact specification (a) -- float32 fma chains in natural order, the oracle's exp and sum -- passes attention_ref.check against the
  float64 definition (b): the reference alone stays inside the bound.
* REJECT: six deliberately wrong variants of (a) each fail that check on a named case (there the unused rows hold finite random values, so
  that a variant fails by its error and not by a NaN).
* the sigma column map is its own inverse, the cases cover every launch form, and the expected cache is what a hand-written example gives.
"""
import numpy as np
import pytest

import attention_ref as ar
import oracle as orc
import stream_attention_ref as sr

SEED0 = 500


def _seed(case):
    return SEED0 + sr.CASES.index(case)


@pytest.mark.parametrize("case", sr.CASES, ids=[c.name for c in sr.CASES])
def test_specification_is_inside_the_bound_of_the_definition(case):
    inp = sr.make_inputs(case, _seed(case))
    got = sr.spec_bits(orc, case, inp)
    worst, mean = ar.check("fp32", got, sr.definition(case, inp), case.H, case.S * case.c, case.name, guard=False)
    print(f"\n{case.name:>32} {case.family:>6}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")


# every mutant of (a) and the case that catches it
CAUGHT_BY = {
    "rel_shift": "tile64-left10-right1-c4",              # position row of key j for query i: off + j + (c - 1 - i)
    "off_minus1": "tile128-kv80-c1",                     # the table window one row early
    "mask_chunk_relative": "tile64-left6-right0-c4",      # dist = i - j instead of (kv - c + i) - j
    "cache_trimmed": "tile64-left10-right1-c4",          # the cache trimmed to `left` rows before the scores, not after
    "swap_uv": "tile64-nc0-c8",                          # q + v with the keys, q + u with the positions
    "swap_left_right": "tile128-left70-right3-c6",       # dist > right or -dist > left
}


def test_every_mutant_is_listed():
    assert set(CAUGHT_BY) == set(sr.MUTANTS)


@pytest.mark.parametrize("mut", sr.MUTANTS)
def test_checker_rejects_mutant_of_the_specification(mut):
    case = next(c for c in sr.CASES if c.name == CAUGHT_BY[mut])
    inp = sr.make_inputs(case, _seed(case), fill=0.5)
    ref = sr.definition(case, inp)
    ar.check("fp32", sr.spec_bits(orc, case, inp), ref, case.H, case.S * case.c, case.name, guard=False)
    with pytest.raises(AssertionError, match="max err / bound|mean err"):
        ar.check("fp32", sr.spec_bits(orc, case, inp, mut=mut), ref, case.H, case.S * case.c, f"mutant {mut} on {case.name}", guard=False)


def test_masked_keys_do_not_loosen_the_bound():
    """the -1e9 of a masked key stays out of the bound: it is what the same keys give when they are simply absent, to rounding"""
    case = sr._mk("hand", "random", "general-1w", 32, 4, 2, 11, 10, 0, cache_rows=11)        # kv 13, left 10: key 0 is masked for both queries
    inp = sr.make_inputs(case, 7)
    full = sr.definition(case, inp)
    short = case._replace(nc=10, cache_rows=10)
    inp2 = dict(inp, kcache=inp["kcache"][:, 1:], vcache=inp["vcache"][:, 1:])
    for (_, _, ctx, bound, sigma), (_, _, ctx2, bound2, sigma2) in zip(full, sr.definition(short, inp2)):
        assert np.allclose(ctx, ctx2, rtol=1e-12, atol=0) and np.all(bound < 1e-3 * (np.abs(ctx).max() + 1))
        assert np.allclose(bound, bound2, rtol=0.05) and np.allclose(sigma, sigma2, rtol=0.05)


def test_sigma_column_map_is_its_own_inverse():
    for d in (16, 80, 96, 128, 256):
        col = np.arange(d)
        s = sr.sigma_col(col)
        assert np.array_equal(np.sort(s), col) and np.array_equal(sr.sigma_col(s), col) and np.any(s != col)
        x = np.random.default_rng(d).standard_normal((3, d)).astype(np.float32)
        stored = np.empty_like(x)
        stored[:, s] = x                                                     # the kernel: natural column e goes to sigma(e)
        assert np.array_equal(sr.natural_columns(stored, True), x) and sr.natural_columns(x, False) is x


def test_cases_cover_every_form_and_the_boundaries():
    forms = {c.form for c in sr.CASES}
    assert forms == {"general-1w", "general-2w", "tiles-hd64", "tiles-hd128"}
    for c in sr.CASES:
        kv = c.nc + c.c
        tile = kv <= 80 and c.c <= 8 and c.hd in (64, 128)
        assert c.form == ((f"tiles-hd{c.hd}") if tile else ("general-2w" if kv > 64 else "general-1w")), c.name
        assert c.S in (1, 3) and c.H in (1, 2, 4) and (c.H * c.hd) % 16 == 0 and c.nc <= c.cache_rows and c.P >= kv and c.keep_max <= c.cache_rows
    seen = {(c.form, c.nc + c.c, c.c) for c in sr.CASES}
    assert {("tiles-hd64", 80, 8), ("tiles-hd128", 80, 8), ("tiles-hd64", 80, 1), ("tiles-hd128", 80, 1), ("tiles-hd64", 1, 1), ("tiles-hd128", 1, 1),
            ("general-2w", 81, 1), ("general-1w", 64, 9), ("general-2w", 65, 9)} <= seen
    for hd in (20, 32, 40, 96, 256):
        assert {c.nc + c.c for c in sr.CASES if c.hd == hd and c.name.startswith("general")} == {5, 24, 31, 64, 65, 130}


def test_expected_cache_by_hand():
    case = sr._mk("hand", "random", "general-1w", 4, 4, 2, 3, 4, 0, S=2, cache_rows=5)        # kv 5 > left 4: rows 1 .. 4 of [cache ; new]
    inp = sr.make_inputs(case, 1)
    d = 16
    for which, name in ((1, "kcache"), (2, "vcache")):
        got = sr.expected_cache(case, inp, which)
        assert got.shape == (2 * 5 + ar.GUARD_ROWS, d)
        for s in range(2):
            new = inp["qkv"][s][:, which * d: (which + 1) * d]
            want = np.concatenate([inp[name][s, 1:3], new]).view(np.uint32)
            assert np.array_equal(got[5 * s: 5 * s + 4], want) and np.all(got[5 * s + 4] == sr.UNWRITTEN)
        assert np.all(got[10:] == sr.UNWRITTEN)
        assert np.all(sr.expected_cache(case, inp, which, rotate=False) == sr.UNWRITTEN)
