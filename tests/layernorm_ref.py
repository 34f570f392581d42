"""The specification, the case table and the checkers of tests/test_gpu_layernorm.py (csrc/kernels/norm.hip through pk_diag_layernorm_form, one launcher
per call).  tests/test_layernorm_ref.py checks this module without a GPU.

Values.  y = orc.layer_norm(x, gamma, beta, eps), bit for bit (mode 0); the same values through smallm_gemm_ref.to_sigma (mode 2); bf16_gemm_ref.bf16_bits
of the same values (mode 1): the fp32 kernel equals the oracle exactly, so its bf16 store must be the round-to-nearest-even of that very number.
launch_layernorm2: y1 = the single norm (always fp32), y2 = the norm of y1 in the mode asked for.

Statistics.  {mean, rstd} = orc.layer_norm_stats(x, eps): the numbers orc.layer_norm itself normalises with (one body in oracle/pk_oracle.c).  The CPU test
holds them to float64 within a bound that follows from the depth of the canonical sum (oracle/pk_oracle_math.h orc_sum64), with u = 2^-24 and
gamma(n) <= 1.01 n u for the n used here:

  sum64 of d values: a lane adds at most ceil(d / 64) values one after the other (the first add, to 0, is exact), then six butterfly levels.  Every input
      passes through at most k = ceil(d / 64) + 6 rounded additions:  |fl(sum) - sum| <= gamma(k) sum|x_i|.
  mean = fl(fl(sum) / d), one more rounding:                           |mean - mu| <= gamma(k + 1) A =: E_mean,      A = sum|x_i| / d.
  variance.  With delta = mean - mu, sum((x_i - mean)^2) / d = sigma^2 + delta^2 exactly (the cross term sums to 0).  The computed terms are all
      non-negative, so the roundings (two in the square of the rounded difference, one for the square, k for the sum, one for the division) give a
      RELATIVE error:                                                  var = (sigma^2 + delta^2)(1 + theta), |theta| <= gamma(k + 4).
  rstd = fl(1 / fl(sqrt(fl(var + eps)))): the sum adds a relative u, the square root halves what it is given and adds u, the division adds u:
      |rstd / rstd64 - 1| <= 1.01 (0.5 (E_mean^2 + gamma(k + 5)(sigma^2 + E_mean^2 + eps)) / (sigma^2 + eps) + 2 u) =: E_rstd
  (1.01 for the second-order terms; a square that underflows adds at most 2^-126 to the variance, below u eps for every eps used here).  stats_bounds() evaluates E_mean and E_rstd for every row from x itself in float64.

The case table (all_cases) lists every (launcher, mode, rows, d) the GPU module launches; want_form says which instantiation each was written for, from
the tables PER_LANE_OF and BATCH_BRANCH below -- stated per width and per row count, not computed from a threshold."""
import numpy as np

import bf16_gemm_ref as B
import smallm_gemm_ref as S
from test_gpu_gemm_schedule import wide_range

FILL32 = 0x7FC5A5A5                                              # what a word of an output buffer no store reached comes back as
U = 2.0 ** -24

# ---- the case table -------------------------------------------------------------------------------------------------------------------------------
# every width with what it is here for, and the PER_LANE instantiation it was written for
PER_LANE_OF = {
    32: 2,        # half a wave
    96: 2,        # a partial second chunk of PER_LANE 2
    128: 2,       # PER_LANE 2, full
    160: 8,       # the first width of PER_LANE 8: two full chunks and half a third, five empty
    512: 8,       # PER_LANE 8, full
    544: 16,      # the first width of PER_LANE 16
    992: 16,      # a partial last chunk of PER_LANE 16
    1024: 16,     # PER_LANE 16, full: the widest row the family holds
    1: 2, 63: 2, 65: 2, 129: 8,                                  # natural fp32 only (sigma columns need d % 16 == 0): one lane, a wave less one, a wave plus one, 128 + 1
}
WIDTHS = (32, 96, 128, 160, 512, 544, 992, 1024)
NATURAL_WIDTHS = (1, 63, 65, 129)
ROWS = (1, 3, 4, 5, 130)                                         # a partial workgroup of four waves, a full one, one more, 32 full + a half
# launch_layernorm's branch for batches: the row counts either side of its switch, and a partial last workgroup on the batch side
BATCH_BRANCH = {1: False, 3: False, 4: False, 5: False, 130: False, 4095: False, 4096: True, 4099: True}
BATCH_ROWS = (4095, 4096, 4099)
BATCH_WIDTHS = (128, 544)
IN_PLACE_WIDTHS = (160, 1024)
IN_PLACE_ROWS = (5, 4099)
FAMILY_WIDTHS = (96, 544)
FAMILY_ROWS = 5
TIE_WIDTHS = (32, 160, 992)
TIE_ROWS = (5, 4099)
PLACE_WIDTHS = (96, 544)                                          # rows are independent of their place: alone, row 3 of 5, row 4098 of 4099
FAMILIES = ("wide", "offset", "const", "tiny", "spike")
EPS = (1e-5, 1e-3, 1e-12)
# (launcher, mode): every launcher in every output mode it has
LAUNCHES = (("norm", 0), ("norm", 1), ("norm", 2), ("norm2", 0), ("norm2", 1), ("norm2", 2), ("stats", 0), ("then_stats", 0))
NATURAL_LAUNCHES = tuple(lm for lm in LAUNCHES if lm[1] == 0)
RPW = 1                                                          # rows per wavefront: every instantiation the library builds today


def want_form(launcher, rows, d):
    """The form (capi.ln_form tuple) a case of this table was written for."""
    return launcher, PER_LANE_OF[d], RPW, launcher == "then_stats", launcher == "norm" and BATCH_BRANCH[rows]


def all_cases():
    """Every (launcher, mode, rows, d) tests/test_gpu_layernorm.py launches (each asserts want_form of it first)."""
    out = [(l, m, r, d) for d in WIDTHS for r in ROWS for l, m in LAUNCHES]
    out += [(l, m, r, d) for d in NATURAL_WIDTHS for r in ROWS for l, m in NATURAL_LAUNCHES]
    out += [(l, m, r, d) for d in BATCH_WIDTHS for r in BATCH_ROWS for l, m in LAUNCHES]
    out += [(l, m, FAMILY_ROWS, d) for d in FAMILY_WIDTHS for l, m in LAUNCHES]
    out += [(l, 1, r, d) for d in TIE_WIDTHS for r in TIE_ROWS for l in ("norm", "norm2")]
    out += [(l, m, r, d) for d in IN_PLACE_WIDTHS for r in IN_PLACE_ROWS for l, m in (("norm", 0), ("norm2", 0), ("norm2", 1), ("norm2", 2), ("then_stats", 0))]
    out += [(l, m, r, d) for d in PLACE_WIDTHS for r in (1, 5, 4099) for l, m in LAUNCHES]
    return out


def case_forms():
    return {want_form(l, r, d) for l, _, r, d in all_cases()}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
# constants whose sums over up to 1024 columns are exact in fp32 (at most four significant bits): mean == the constant, x - mean == 0, variance == 0
CONSTANTS = np.array([0.0, 1.0, -2.0, 0.5, 3.0, -0.75, 1024.0, -0.0078125], np.float32)


def make_x(family, rng, rows, d):
    if family == "wide":
        return wide_range(rng, (rows, d))
    if family == "offset":                                       # mean >> spread: the cancellation in x - mean
        return (1e3 + 1e-2 * rng.standard_normal((rows, d))).astype(np.float32)
    if family == "const":                                        # variance exactly 0; row 0 is all zero
        return np.repeat(CONSTANTS[np.arange(rows) % len(CONSTANTS)][:, None], d, axis=1)
    if family == "tiny":                                         # the squares underflow: variance 0 although the row is not constant
        return (1e-30 * rng.standard_normal((rows, d))).astype(np.float32)
    if family == "spike":                                        # one value in a zero row
        x = np.zeros((rows, d), np.float32)
        x[np.arange(rows), (7 * np.arange(rows) + 5) % d] = wide_range(rng, rows) + np.float32(0.5)
        return x
    raise ValueError(family)


def make_params(rng, d):
    """gamma around 1, beta around 0, nothing special about either"""
    return (1.0 + 0.5 * rng.standard_normal(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)


# ---- bf16 ties --------------------------------------------------------------------------------------------------------------------------------------
TIE_LOW = (0x8000, 0x7FFF, 0x8001)                                # exactly half-way between two bf16 numbers, one fp32 ulp below, one above


def tie_betas(d):
    """[d] fp32 values on and next to bf16 rounding ties: column i has sign (i >> 1) & 1, a lower bf16 neighbour of parity i & 1, and the low half
    TIE_LOW[(i >> 2) % 3]; exponents 2^-8 .. 2^8, so nothing is subnormal or overflows.  d >= 12 holds every combination."""
    i = np.arange(d, dtype=np.uint32)
    sign, parity, kind = (i >> 1) & 1, i & 1, (i >> 2) % 3
    exp = 119 + (i * 5) % 17
    mant7 = (((i * 37) % 128) & ~np.uint32(1)) | parity
    word = (sign << 31) | (exp << 23) | (mant7 << 16) | np.array(TIE_LOW, np.uint32)[kind]
    return word.astype(np.uint32).view(np.float32)


def bf16_truncate(x):
    """A WRONG bf16 store: the low half dropped"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_half_up(x):
    """A WRONG bf16 store: ties away from zero (add half an ulp of the bf16 number, drop the low half)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


def assert_ties_tell_the_stores_apart(y):
    """y (fp32, the values a bf16 store is about to round) separates round-to-nearest-even from truncation and from round-half-up, for both signs and
    both parities of the lower neighbour."""
    y = np.ascontiguousarray(y, np.float32).reshape(-1)
    u = y.view(np.uint32)
    rne, trunc, up = B.bf16_bits(y), bf16_truncate(y), bf16_half_up(y)
    for sign in (0, 1):
        for parity in (0, 1):
            sel = ((u >> 31) == sign) & (((u >> 16) & 1) == parity)
            tie = sel & ((u & 0xFFFF) == 0x8000)
            assert tie.any(), f"no exact tie with sign {sign}, parity {parity}"
            assert np.all((rne[tie] != trunc[tie]) == (parity == 1)), "a tie rounds away from an odd lower neighbour, stays on an even one"
            assert np.all((rne[tie] != up[tie]) == (parity == 0)), "round-half-up leaves an even lower neighbour, nearest-even does not"
            below, above = sel & ((u & 0xFFFF) == 0x7FFF), sel & ((u & 0xFFFF) == 0x8001)
            assert below.any() and above.any(), f"no neighbours of a tie with sign {sign}, parity {parity}"
            assert np.array_equal(rne[below], trunc[below]) and np.all(rne[above] != trunc[above])
            assert np.array_equal(rne[below], up[below]) and np.array_equal(rne[above], up[above])


# ---- the specification ----------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def payload(y, mode):
    """The elements a launch stores for the fp32 values y [rows][d] in an output mode: uint32 words (0: natural, 2: sigma columns) or bf16 halfwords (1)"""
    y = np.ascontiguousarray(y, np.float32)
    if mode == 1:
        return B.bf16_bits(y).reshape(-1)
    return bits(S.to_sigma(y) if mode == 2 else y).reshape(-1)


def expect_buffer(elems, total_words):
    """A whole output buffer of total_words 32-bit words: the elements (uint32 words, or uint16 halfwords two to a word, element 2 i in the low half of
    word i) from its start, the fill pattern in every word -- and the spare halfword of an odd count -- behind them."""
    buf = np.full(total_words, FILL32, np.uint32)
    if elems.dtype == np.uint16:
        assert elems.size < 2 * total_words
        buf.view(np.uint16)[:elems.size] = elems
    else:
        assert elems.dtype == np.uint32 and elems.size < total_words
        buf[:elems.size] = elems
    return buf


def assert_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ, first at {bad[0]}: got {int(got[bad[0]]):#010x} want {int(want[bad[0]]):#010x}"


def check_output(got_words, y, mode, what):
    """got_words: a whole buffer as it came back.  It must hold exactly payload(y, mode) and the fill pattern behind it."""
    assert_words(got_words, expect_buffer(payload(y, mode), np.asarray(got_words).size), what)


def check_bf16_store(got_halfwords, y, what):
    """The bf16 elements a launch stored for the fp32 values y: round to nearest, ties to even, bit for bit."""
    assert_words(np.asarray(got_halfwords, np.uint16), B.bf16_bits(np.ascontiguousarray(y, np.float32)).reshape(-1), what)


def expected(orc, launcher, mode, x, g1, b1, g2, b2, eps):
    """-> {buffer name: (fp32 values, mode)} for y / y2 and {"stats": fp32 [rows][2]}: what one launch must leave, from the oracle."""
    if launcher == "stats":
        return {"stats": orc.layer_norm_stats(x, eps)}
    y1 = orc.layer_norm(x, g1, b1, eps)
    if launcher == "norm":
        return {"y": (y1, mode)}
    if launcher == "norm2":
        return {"y": (y1, 0), "y2": (orc.layer_norm(y1, g2, b2, eps), mode)}
    return {"y": (y1, 0), "stats": orc.layer_norm_stats(y1, eps)}


def check_launch(got, want, what):
    """got: what capi.diag_layernorm_form returned; want: expected(...).  Every buffer whole: the payload bit for bit, the fill pattern elsewhere."""
    assert set(want) == set(got) - {"form"}, f"{what}: buffers {sorted(got)} vs {sorted(want)}"
    for name, w in want.items():
        if name == "stats":
            assert_words(got["stats"], expect_buffer(bits(w).reshape(-1), got["stats"].size), f"{what}: stats")
        else:
            check_output(got[name], w[0], w[1], f"{what}: {name} (mode {w[1]})")


# ---- the statistics against float64 ---------------------------------------------------------------------------------------------------------------
def stats64(x, eps):
    """(mean, rstd) of every row in float64; eps is the fp32 number the kernels are handed"""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=-1)
    var = ((x - mu[..., None]) ** 2).mean(axis=-1)
    return mu, 1.0 / np.sqrt(var + float(np.float32(eps)))


def stats_bounds(x, eps):
    """(E_mean absolute, E_rstd relative) per row: the module docstring's bounds"""
    x = np.asarray(x, np.float64)
    d = x.shape[-1]
    k = -(-d // 64) + 6
    gamma = lambda n: 1.01 * n * U
    mu = x.mean(axis=-1)
    var = ((x - mu[..., None]) ** 2).mean(axis=-1)
    e = float(np.float32(eps))
    e_mean = gamma(k + 1) * np.abs(x).mean(axis=-1)
    e_rstd = 1.01 * (0.5 * (e_mean ** 2 + gamma(k + 5) * (var + e_mean ** 2 + e)) / (var + e) + 2 * U)
    return e_mean, e_rstd


def stats_errors(stats, x, eps):
    """(|mean - mean64|, |rstd / rstd64 - 1|) per row"""
    mu, rstd = stats64(x, eps)
    st = np.asarray(stats, np.float64)
    return np.abs(st[..., 0] - mu), np.abs(st[..., 1] / rstd - 1.0)


def sum64_f32(x):
    """orc_sum64 over the last axis in numpy float32 arithmetic: lane l adds x[l], x[l + 64], ... in order, then the xor butterfly 32, 16, .. 1"""
    x = np.ascontiguousarray(x, np.float32)
    rows, d = x.shape
    p = np.zeros((rows, 64), np.float32)
    for j in range(0, d, 64):
        w = min(64, d - j)
        p[:, :w] = p[:, :w] + x[:, j:j + w]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lane ^ off]
    return p[:, 0]


def stats_emulated(x, eps, fault=None):
    """The statistics as oracle/pk_oracle.c computes them, restated in numpy float32 -- bit for bit the oracle with fault None (the CPU test checks it) --
    so that a fault can be planted: "raw_moment": the variance taken without subtracting the mean; "bessel": the variance divided by d - 1."""
    x = np.ascontiguousarray(x, np.float32)
    d = x.shape[-1]
    mean = sum64_f32(x) / np.float32(d)
    c = x if fault == "raw_moment" else x - mean[:, None]
    var = sum64_f32(c * c) / np.float32(d - 1 if fault == "bessel" else d)
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return np.stack([mean, rstd], axis=-1).astype(np.float32)
