"""The float64 reference of the bf16 tile GEMM family (csrc/kernels/gemm_bf16.hpp, gemm_bf16_glds.hpp): operands rounded to bf16 (nearest even) on the
host, the product and every epilogue function in float64, the output placed where GemmArgs puts it (row pitch, sigma columns, the subsampling remap through
tests/smallm_gemm_ref.py; the 32 x 16 blocked hand-off layout here), and the error bounds tests/test_gpu_bf16_tile_gemm.py asserts, each with its
derivation.  Written from the comments of csrc/kernels/kernels.hpp (GemmArgs); no device code is restated: arithmetic on whole arrays only."""
import numpy as np

from smallm_gemm_ref import output_offsets, to_sigma  # noqa: F401  (re-exported: the row-major placements)

FILL32 = 0x7FC5A5A5                                                  # what the diagnostic fills the output buffer with
FILL16 = (0xA5A5, 0x7FC5)                                            # ... seen as bf16 elements: even / odd element of a word (little endian)


# ---- bf16 on the host --------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the bf16 bit pattern (uint16), round to nearest, ties to even; a NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(bits):
    """bf16 bit patterns -> float32"""
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    return bf16_value(bf16_bits(x)).reshape(np.shape(x))


def bf16_neighbours(want):
    """For float64 `want`: (lo, hi, mid) float64 -- the bf16 values lo <= want <= hi next to it (lo == hi where want is one) and the rounding boundary
    between them (for a want that is a bf16 value: a point no farther than its nearest boundary).  Normal range only (8 significant bits: the spacing at |want| in [2^(e-1), 2^e) is 2^(e-8))."""
    want = np.asarray(want, np.float64)
    _, e = np.frexp(want)
    ulp = np.ldexp(1.0, e - 8)
    lo, hi = np.floor(want / ulp) * ulp, np.ceil(want / ulp) * ulp
    # (a want that IS a bf16 value, 0 after a ReLU for one, has its boundaries half an ulp away on either side -- a quarter below a power of two)
    return lo, hi, np.where(lo == hi, lo + 0.25 * ulp, 0.5 * (lo + hi))


def words_to_bf16(words):
    """The uint32 words of an output buffer -> its bf16 elements (uint16; element 2 i is the low half of word i)"""
    return np.ascontiguousarray(words, np.uint32).view(np.uint16)


# ---- the blocked hand-off layout (GemmArgs::out_blocked / a_blocked) ----------------------------------------------------------------------------------
def blocked_offsets(M, N, ld):
    """[M][N] element offsets of (row, col) in the blocked layout: block (row / 32, col / 16) holds 32 x 16 elements row-major, blocks ordered
    [row / 32][ld / 16]; ld % 16 == 0.  The buffer holds roundup32(M) * ld elements."""
    assert ld % 16 == 0 and N <= ld
    row, col = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64), indexing="ij")
    return ((row // 32) * (ld // 16) + col // 16) * 512 + (row % 32) * 16 + col % 16


def to_blocked(x, ld, fill):
    """x [M][N] -> the flat blocked buffer of roundup32(M) * ld elements, `fill` wherever no element of x lands"""
    x = np.asarray(x)
    M, N = x.shape
    buf = np.full((M + 31) // 32 * 32 * ld, fill, x.dtype)
    buf[blocked_offsets(M, N, ld)] = x
    return buf


def from_blocked(buf, M, N, ld):
    """Undoes to_blocked: the [M][N] elements of a flat blocked buffer"""
    return np.asarray(buf)[blocked_offsets(M, N, ld)]


# ---- the product and its epilogue functions in float64 -----------------------------------------------------------------------------------------------
def sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def product(A, W, bias, epi, resid=None, alpha=1.0):
    """out = epi(bf16(A) bf16(W)^T + bias) in float64.  A [M][K], W [N or 2N][K], bias [N or 2N] or None, resid [M][N] for epi "resid".
    -> dict(want, z (the pre-activation value; GLU: the value half), g (GLU: the gate's pre-activation), mag = |Aq| |Wq|^T + |bias| of z (float32
    arithmetic: a bound needs three digits), mag_g (GLU))."""
    Aq, Wq = bf16_round(A), bf16_round(W)
    A64, absA = Aq.astype(np.float64), np.abs(Aq)
    N = W.shape[0] // 2 if epi == "glu" else W.shape[0]

    def half(lo, hi):
        z = A64 @ Wq[lo:hi].astype(np.float64).T
        mag = (absA @ np.abs(Wq[lo:hi]).T).astype(np.float64)
        if bias is not None:
            z = z + np.asarray(bias[lo:hi], np.float64)
            mag = mag + np.abs(np.asarray(bias[lo:hi], np.float64))
        return z, mag

    z, mag = half(0, N)
    out = dict(z=z, mag=mag, g=None, mag_g=None)
    if epi == "none":
        out["want"] = z
    elif epi == "relu":
        out["want"] = np.maximum(z, 0.0)
    elif epi == "silu":
        out["want"] = z * sigmoid64(z)
    elif epi == "resid":
        out["want"] = np.asarray(resid, np.float64) + np.float64(np.float32(alpha)) * z
    else:
        assert epi == "glu"
        out["g"], out["mag_g"] = half(N, 2 * N)
        out["want"] = z * sigmoid64(out["g"])
    return out


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------------------
def acc_bound(mag):
    """The project's accumulation-class bound of a bf16 product with fp32 accumulation (tests/test_gpu_bf16.py): 2e-6 mag + 1e-6."""
    return 2e-6 * mag + 1e-6


def fast_sigmoid_rel(z):
    """Relative error of fast_sigmoidf(z) = rcp(1 + exp2(-z log2e)) against sigmoid(z), derived (u = 2^-24, every step rounded to nearest unless said):
      t = fl(z * -log2e): the constant is log2e rounded to float32 (relative 2^-25 at most) and the product is rounded once: t = -z log2e (1 + e1),
          |e1| <= 1.5 u.  exp2 turns an ABSOLUTE error |t e1| = |z| log2e 1.5 u of its argument into a relative error ln2 |t e1| = 1.5 u |z| of its value.
      e = v_exp_f32(t): 1 ulp = 2 u relative.
      s = fl(1 + e): one rounded add, u relative; the errors of e enter s scaled by e / (1 + e) < 1.
      r = v_rcp_f32(s): 1 ulp = 2 u relative.
    Sum: (1.5 |z| + 2 + 1 + 2) u = (5 + 1.5 |z|) u <= (4 + |z|) 2^-23 = (8 + 2 |z|) u, the figure the suite asserts."""
    return (4.0 + np.abs(z)) * 2.0 ** -23


def silu_slope(z):
    s = sigmoid64(z)
    return s * (1.0 + z * (1.0 - s))


def out_bound(p, epi, fast, K=None, resid_reg=False, resid=None):
    """|out - want| for fp32 rows out.  p = product(...).
      none / relu / polynomial silu / polynomial glu / resid: acc_bound(mag) (glu: of both halves' mag summed), the project's own bound.
      register residual epilogue: + 6e-8 (K / 16) |resid| -- the partial sums are added onto a value of the residual's magnitude (tests/test_gpu_bf16.py).
      fast silu: the kernel's pre-activation zk has |zk - z| <= d = acc_bound(mag); silu is Lipschitz on [z - d, z + d] with |silu'(z)| + d / 2 (|silu''| <= 1/2:
          never more than the global 1.1 d + d^2 / 2); then fast_siluf(zk) = zk * fast_sigmoidf(zk) adds (fast_sigmoid_rel + 2^-24) |want| (one more rounded product).
      fast glu: out = vk * fast_sigmoidf(gk): |vk - v| <= dv, |gk - g| <= dg, sigmoid' <= 1/4: dv sigmoid(g) + |v| dg / 4 + (fast_sigmoid_rel(g) + 2^-24) |want|."""
    d = acc_bound(p["mag"])
    if epi == "silu" and fast:
        return (np.abs(silu_slope(p["z"])) + 0.5 * d) * d + (fast_sigmoid_rel(p["z"]) + 2.0 ** -24) * np.abs(p["want"])
    if epi == "glu" and fast:
        dg = acc_bound(p["mag_g"])
        return d * sigmoid64(p["g"]) + np.abs(p["z"]) * dg / 4 + (fast_sigmoid_rel(p["g"]) + 2.0 ** -24) * np.abs(p["want"])
    if epi == "glu":
        return acc_bound(p["mag"] + p["mag_g"])
    if epi == "resid" and resid_reg:
        return d + 6e-8 * (K / 16) * np.abs(np.asarray(resid, np.float64))
    return d


def check_bf16_rows(got_bits, want, delta):
    """bf16 rows out: the kernel stores bf16(v) with |v - want| <= delta.  Then |out - want| <= delta + 2^-8 (|want| + delta): half a bf16 ulp of v, and with 8
    significant bits an ulp is up to 2^-7 of the value, so the unit roundoff is 2^-8 (NOT 2^-9: bf16(1 + 2^-8) is 1 or 1 + 2^-7, either 2^-8 away --
    tests/test_bf16_gemm_ref.py shows the correctly rounded reference itself exceeding a 2^-9 bound).  And out is bf16(want) wherever want is farther than delta from the rounding boundary between its two bf16 neighbours -- elsewhere
    ("excused") it is one of the two neighbours (delta is far below a bf16 ulp on the operands the suite uses; where it is not, the neighbours of
    want +- delta).  -> (worst |out - want| / bound, share of excused elements); asserts the rest."""
    out = bf16_value(got_bits).astype(np.float64).reshape(want.shape)
    err = np.abs(out - want)
    bound = delta + 2.0 ** -8 * (np.abs(want) + delta)
    assert np.all(err <= bound), f"bf16 rows: |out - want| exceeds delta + 2^-8 (|want| + delta) by up to {np.max(err - bound):.3e}"
    lo, hi, mid = bf16_neighbours(want)
    excused = np.abs(want - mid) <= delta
    exact = bf16_round(want.astype(np.float32)).astype(np.float64)     # (float32 first: a double rounding only where want is within 2^-25 of the boundary -- excused)
    bad = ~excused & (out != exact)
    assert not bad.any(), f"bf16 rows: {int(bad.sum())} elements are not bf16(want) although want is farther than delta from a rounding boundary"
    lo2, _, _ = bf16_neighbours(want - delta)
    _, hi2, _ = bf16_neighbours(want + delta)
    bad = excused & ((out < lo2) | (out > hi2))
    assert not bad.any(), f"bf16 rows: {int(bad.sum())} excused elements are no bf16 neighbour of want"
    return float(np.max(err / bound)), float(excused.mean())


def excused_share(want, delta):
    """The share of elements check_bf16_rows would excuse, from the float64 reference alone"""
    _, _, mid = bf16_neighbours(want)
    return float((np.abs(want - mid) <= delta).mean())


def coherent_operands(rng, M, N, K):
    """Operands whose products all have the sign of (row sign x column sign): no cancellation, so mag = |want| and the accumulation bound is ~2e-6 RELATIVE --
    far below the bf16 ulp (2^-8 relative), which keeps the excused share of check_bf16_rows small.  |z| is log-uniform in about [0.25, 4]; both signs."""
    s, t = rng.choice([-1.0, 1.0], M), rng.choice([-1.0, 1.0], N)
    r, c = 2.0 ** rng.uniform(-1, 1, M), 2.0 ** rng.uniform(-1, 1, N)
    A = (s * r)[:, None] * rng.uniform(0.5, 1.5, (M, K))
    W = (t * c)[:, None] * rng.uniform(0.5, 1.5, (N, K)) / K
    return A.astype(np.float32), W.astype(np.float32)
