"""The bf16 tile GEMM family alone (csrc/kernels/gemm.hip launch_gemm_bf16, gemm_bf16.hpp, gemm_bf16_glds.hpp through pk_diag_gemm_bf16_tile: one product
per call): the register-staged kernel on its three tiles with fp32 or bf16 A, and the direct-to-LDS kernel on both tile heights with the LDS epilogue, the
register epilogue on one tile per workgroup, the persistent walk and the register residual epilogue -- every instantiation launch_gemm_bf16 can take, at the
smallest shapes that still reach it, with the switches production sets (fast_act, bf16 rows out, the blocked hand-off both ways).

Reference: tests/bf16_gemm_ref.py -- the float64 product of the operands rounded to bf16 (nearest even), every epilogue function in float64, placed where
GemmArgs puts it.  The buffer comes back whole: every word no element belongs to must still hold the fill.  Each case names the form it is written for and
compares it with the form the launcher's own function reports (no threshold is restated here); test_every_form_has_a_case compares the union with the
library's table both ways.

Bounds (bf16_gemm_ref.out_bound / check_bf16_rows / fast_sigmoid_rel carry the derivations):
  * fp32 rows, polynomial or no activation: |err| <= 2e-6 mag + 1e-6, mag = |Aq| |Wq|^T + |bias| (GLU: both halves summed) -- the project's own
    accumulation-class bound (tests/test_gpu_bf16.py).  Register residual epilogue: + 6e-8 (K / 16) |resid|, the same file's term: the partial sums are
    added onto a value of the residual's magnitude.
  * fast_act: fast_sigmoidf(z) = rcp(1 + exp2(-z log2e)).  With u = 2^-24: the rounded product z log2e (constant rounded too) is off by 1.5 u relative,
    which exp2 turns into 1.5 u |z| relative; v_exp_f32 and v_rcp_f32 are 1 ulp = 2 u each; the add is rounded once, u.  (5 + 1.5 |z|) u, asserted as the
    rounder (4 + |z|) 2^-23.  SiLU / GLU multiply once more: + 2^-24.  The kernel applies it to ITS pre-activation, which is within the accumulation
    bound d of z: SiLU moves by at most (|silu'(z)| + d / 2) d (|silu''| <= 1/2; never more than 1.1 d + d^2 / 2), the GLU by dv sigmoid(g) + |v| dg / 4.
    test_fast_activations_alone checks the activation's own bound over [-30, 30] and the special values.
  * bf16 rows: the kernel stores bf16(v), |v - want| <= delta (the fp32-rows bound): |out - want| <= delta + 2^-8 (|want| + delta) (the unit roundoff of
    8 significant bits is 2^-8; a 2^-9 there is exceeded by the correctly rounded float64 reference itself, tests/test_bf16_gemm_ref.py), and out is
    bf16(want) wherever want is farther than delta from a rounding boundary; elsewhere ("excused", printed, at most 2 %) a bf16 neighbour.  These cases
    use operands without cancellation (bf16_gemm_ref.coherent_operands: mag = |want|, delta ~ 2e-6 relative against a bf16 ulp of 2^-8), for which
    tests/test_bf16_gemm_ref.py finds the excused share of the reference alone under the cap.
  * every comparison called "bit for bit" has no tolerance.
The register residual epilogue forms alpha (resid / alpha + bias + A W^T): its words differ from the LDS epilogue's resid + alpha (A W^T + bias) wherever
the residual or the bias is non-zero (gemm_bf16_glds.hpp says so: 'rounded at ITS ulp'), so the two are compared bit for bit on a zero residual without
bias at alpha = 1/2, and each against float64 within its bound otherwise."""
import functools

import numpy as np
import pytest

import bf16_gemm_ref as R
from conftest import pk  # noqa: F401

pytestmark = pytest.mark.gpu

PK_ERR_UNSUPPORTED = -7
FOUR = ("none", "relu", "silu", "resid")
REG = {"64x64": (2, 2, 1, 1), "128x64": (2, 2, 2, 1), "128x128": (4, 2, 1, 2)}
GL = {192: (2, 4, 3, 2), 256: (4, 2, 2, 4)}
WORST = {}                                                           # label -> worst |err| / bound seen (printed by test_every_form_has_a_case)


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


def reg_form(tile, a16, epi):
    return ("reg", REG[tile], a16, "lds", epi)


def gl_form(height, efo, epi):
    return ("glds", GL[height], True, efo, epi)


@functools.lru_cache(maxsize=4)
def ops(M, N, K, glu, kind="gauss"):
    """A [M][K], W [N or 2N][K] / sqrt(K), bias, residual [M][N]: one set per shape, shared by every case on it and never written.  kind "coherent": no
    cancellation (bf16 rows out)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + (1 << 20 if glu else 0))
    rows = 2 * N if glu else N
    if kind == "coherent":
        A, W = R.coherent_operands(rng, M, rows, K)
        b = (0.01 * rng.standard_normal(rows)).astype(np.float32)
    else:
        A = rng.standard_normal((M, K), dtype=np.float32)
        W = rng.standard_normal((rows, K), dtype=np.float32) / np.float32(np.sqrt(K))
        b = rng.standard_normal(rows).astype(np.float32)
    out = (A, W, b, rng.standard_normal((M, N), dtype=np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=3)
def ref(M, N, K, epi, bias=True, kind="gauss", alpha=1.0):
    """bf16_gemm_ref.product of ops(...): once per (shape, epilogue function), shared and never written"""
    A, W, b, Rs = ops(M, N, K, epi == "glu", kind)
    return R.product(A, W, b if bias else None, epi, Rs if epi == "resid" else None, alpha)


def check(capi, got, p, M, N, epi, what, fmt="f32", ldo=None, sigma_cols=0, remap=None, fast=False, K=None, resid_reg=False, resid=None):
    """The whole buffer: `want` within its bound where GemmArgs puts it, the fill everywhere else.  -> the elements, in natural order."""
    ldo = ldo or N
    bound = R.out_bound(p, epi, fast, K, resid_reg, resid)
    if fmt == "f32":
        off = R.output_offsets(M, N, ldo, sigma_cols, remap)
        words = got["out"]
        vals = words.view(np.float32)[off]
        err = np.abs(vals.astype(np.float64) - p["want"])
        worst = float(np.max(err / bound))
        print(f"{what}: worst |err| / bound = {worst:.3f}")
        assert np.all(err <= bound), f"{what}: |err| exceeds the bound at {int((err > bound).sum())} elements, worst ratio {worst:.3f}"
        rest = np.ones(words.size, bool)
        rest[off.reshape(-1)] = False
        assert np.all(words[rest] == R.FILL32), f"{what}: {int((words[rest] != R.FILL32).sum())} words outside the output were written"
    else:
        off = R.blocked_offsets(M, N, ldo) if fmt == "blocked" else R.output_offsets(M, N, ldo)
        el = R.words_to_bf16(got["out"])
        vals = el[off]
        worst, share = R.check_bf16_rows(vals, p["want"], bound)
        print(f"{what}: worst |err| / bound = {worst:.3f}, excused {100 * share:.2f} %")
        assert share <= 0.02, f"{what}: {100 * share:.2f} % of the elements lie within delta of a rounding boundary"
        rest = np.ones(el.size, bool)
        rest[off.reshape(-1)] = False
        fill = np.where(np.arange(el.size) % 2 == 0, R.FILL16[0], R.FILL16[1]).astype(np.uint16)
        assert np.array_equal(el[rest], fill[rest]), f"{what}: bf16 elements outside the output were written"
    WORST[what.split(":")[0]] = max(WORST.get(what.split(":")[0], 0.0), worst)
    return vals


def run(capi, want_form, M, N, K, epi, bias=True, alpha=1.0, kind="gauss", fmt="f32", fast=None, label=None, **kw):
    """One product alone: the form it ran on is the one the case is written for, and the buffer holds the reference within its bound."""
    glu = epi == "glu"
    fast = (epi in ("silu", "glu")) if fast is None else fast
    A, W, b, Rs = ops(M, N, K, glu, kind)
    p = ref(M, N, K, epi, bias, kind, alpha)
    a16 = want_form[2]
    what = f"{label or '-'.join(str(v) for v in want_form)}: {M}x{N}x{K} {epi} bias={bias} {fmt} {kw}"
    chk = {k: kw[k] for k in ("ldo", "sigma_cols", "remap") if k in kw}
    got = capi.diag_gemm_bf16_tile(A, W, bias=b if bias else None, epi=epi, resid=Rs if epi == "resid" else None, alpha=alpha, a16=a16, fast_act=fast,
                                   out_bf16=fmt != "f32", out_blocked=fmt == "blocked", **kw)
    assert got["form"] == want_form, what
    vals = check(capi, got, p, M, N, epi, what, fmt=fmt, fast=fast, K=K, resid_reg=want_form[3] == "resid_reg", resid=Rs, **chk)
    return vals, got["out"]


# ---- every form at the smallest shapes that reach it ------------------------------------------------------------------------------------------------
# Register-staged kernel.  (130, 70, 192): 3 x 2 tiles, 3 K tiles; (70, 72, 64): ONE K tile on the double-buffered loop; (1030, 260, 128): 9 x 5 = 45 tiles
# (no multiple of 8: the XCD remap's remainder) in a whole group of 8 tile rows and a last group of one; (1030, 1028, 128): 81 tiles; (65536, 256, 64): the
# tall-and-narrow branch of the 128 x 128 tile.
REG_SHAPES = {"64x64": [(70, 72, 64), (130, 70, 192)], "128x64": [(1030, 260, 128)], "128x128": [(1030, 1028, 128)]}
REG_CASES = [(tile, M, N, K, epi, a16) for tile, shapes in REG_SHAPES.items() for M, N, K in shapes for epi in FOUR for a16 in (False, True)]
REG_CASES += [("128x128", 100, 40, 64, "glu", a16) for a16 in (False, True)] + [("128x128", 1030, 520, 128, "glu", True), ("128x128", 65536, 256, 64, "none", True)]
# Direct-to-LDS kernel: (height, epilogue form, shape).  8200 = 42 x 192 + 136 = 32 x 256 + 8: a partial last row tile on both heights; 1040, 1520, 2064,
# 3056, 624, 880 and 2288 end inside a column tile with N % 16 == 0; K tiles 8, 16, 17 (odd), 20 and 27 (odd).  N % 16 != 0 with N % 4 == 0 (1044, 1524):
# the LDS epilogue.
GL_SHAPES = {(192, "direct"): (8200, 1040, 1088), (192, "persist"): (8200, 2064, 512), (256, "direct"): (8200, 1520, 1024), (256, "persist"): (8200, 3056, 512)}
GL_GLU = {(192, "direct"): (8200, 624, 1728), (192, "persist"): (8200, 1040, 1024), (256, "direct"): (8200, 880, 1280), (256, "persist"): (8200, 2288, 512)}
GL_LDS = {192: (8200, 1044, 1024), 256: (8200, 1524, 1024)}
GL_CASES = [(h, efo, *GL_SHAPES[h, efo], epi) for (h, efo) in GL_SHAPES for epi in ("none", "relu", "silu")]
GL_CASES += [(h, efo, *GL_GLU[h, efo], "glu") for (h, efo) in GL_GLU]
GL_CASES += [(h, "lds", *GL_LDS[h], epi) for h in GL_LDS for epi in FOUR + ("glu",)]
GL_CASES += [(h, "resid_reg", *GL_SHAPES[h, "direct"], "resid") for h in GL]


@pytest.mark.parametrize("tile,M,N,K,epi,a16", REG_CASES, ids=[f"{t}-{m}x{n}x{k}-{e}-{'a16' if a else 'a32'}" for t, m, n, k, e, a in REG_CASES])
def test_register_staged_forms_against_float64(capi, tile, M, N, K, epi, a16):
    run(capi, reg_form(tile, a16, epi), M, N, K, epi, alpha=0.5 if M % 4 == 2 else 1.0, fast=False)


@pytest.mark.parametrize("h,efo,M,N,K,epi", GL_CASES, ids=[f"{h}-{f}-{m}x{n}x{k}-{e}" for h, f, m, n, k, e in GL_CASES])
def test_direct_to_lds_forms_against_float64(capi, h, efo, M, N, K, epi):
    """The LDS cases run the polynomial activations (fast_act = 0), the register epilogues the hardware ones production asks for."""
    run(capi, gl_form(h, efo, epi), M, N, K, epi, alpha=0.5, fast=efo != "lds" and epi in ("silu", "glu"))


def test_fast_activations_on_the_register_staged_kernel_and_the_lds_epilogue(capi):
    """GemmArgs::fast_act through gp_epilogue: wide and scalar (ldo = N + 3), SiLU and GLU, on the register-staged kernel and the direct-to-LDS one."""
    for epi, tile, (M, N, K) in (("silu", "128x64", (1030, 260, 128)), ("glu", "128x128", (1030, 520, 128))):
        run(capi, reg_form(tile, True, epi), M, N, K, epi, fast=True)
        run(capi, reg_form(tile, True, epi), M, N, K, epi, fast=True, ldo=N + 3)
    run(capi, gl_form(192, "lds", "silu"), *GL_LDS[192], "silu", fast=True)


# ---- the production switches on the register epilogue -------------------------------------------------------------------------------------------------
SWITCH_CASES = [(h, efo, epi) for h in GL for efo in ("direct", "persist") for epi in ("silu", "glu", "none", "relu")]


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("h,efo,epi", SWITCH_CASES, ids=[f"{h}-{f}-{e}" for h, f, e in SWITCH_CASES])
def test_register_epilogue_row_formats(capi, h, efo, epi, bias):
    """fp32 rows, bf16 rows and the blocked bf16 hand-off, with and without bias; SiLU / GLU with fast_act as conformer_block.hpp sets it.  The blocked buffer,
    un-blocked here, is bit for bit the row-major bf16 output.  (A GLU product has fp32 rows only: bf16 rows are refused, test_refusals.)"""
    M, N, K = (GL_GLU if epi == "glu" else GL_SHAPES)[h, efo]
    f = gl_form(h, efo, epi)
    run(capi, f, M, N, K, epi, bias=bias, kind="coherent")
    if epi != "glu":
        rows, _ = run(capi, f, M, N, K, epi, bias=bias, kind="coherent", fmt="bf16")
        blocked, _ = run(capi, f, M, N, K, epi, bias=bias, kind="coherent", fmt="blocked")
        assert np.array_equal(blocked, rows), "the blocked buffer, un-blocked, against the row-major bf16 rows"


def test_bf16_rows_through_the_wide_lds_epilogue(capi):
    """out_bf16 on gp_epilogue's wide path: the register-staged kernel (fp32 and bf16 A) and the direct-to-LDS kernel with ldo = N + 4."""
    M, N, K = 1030, 260, 128
    for a16 in (False, True):
        for epi in ("none", "silu"):
            run(capi, reg_form("128x64", a16, epi), M, N, K, epi, kind="coherent", fmt="bf16", fast=epi == "silu")
    M, N, K = GL_SHAPES[192, "direct"]
    run(capi, gl_form(192, "lds", "silu"), M, N, K, "silu", kind="coherent", fmt="bf16", ldo=N + 4)


# ---- equalities the code comments claim, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,efo,epi", SWITCH_CASES, ids=[f"{h}-{f}-{e}" for h, f, e in SWITCH_CASES])
def test_register_epilogue_equals_lds_epilogue(capi, h, efo, epi):
    """gemm_bf16_glds.hpp: the swapped operands sum 'the same products in the same k order, so every result is bit for bit the other form's'.  ldo = N + 4 sends
    the same product to the LDS epilogue without changing a value."""
    M, N, K = (GL_GLU if epi == "glu" else GL_SHAPES)[h, efo]
    direct, _ = run(capi, gl_form(h, efo, epi), M, N, K, epi)
    lds, _ = run(capi, gl_form(h, "lds", epi), M, N, K, epi, ldo=N + 4)
    assert np.array_equal(direct.view(np.uint32), lds.view(np.uint32))


@pytest.mark.parametrize("h", list(GL))
def test_register_residual_epilogue_against_the_lds_one(capi, h):
    """Both within their bounds of float64 (ldr = N + 1: the scalar LDS epilogue; N % 16 != 0 in the form cases: the wide one); on a zero residual without
    bias the accumulators start at zero and alpha = 1/2 scales exactly: bit for bit."""
    M, N, K = GL_SHAPES[h, "direct"]
    run(capi, gl_form(h, "resid_reg", "resid"), M, N, K, "resid", alpha=0.5, ldr=N + 4)
    run(capi, gl_form(h, "lds", "resid"), M, N, K, "resid", alpha=0.5, ldr=N + 1)
    A, W, _, _ = ops(M, N, K, False)
    zero = np.zeros((M, N), np.float32)
    reg = capi.diag_gemm_bf16_tile(A, W, epi="resid", resid=zero, alpha=0.5, a16=True)
    lds = capi.diag_gemm_bf16_tile(A, W, epi="resid", resid=zero, alpha=0.5, a16=True, ldr=N + 1)
    assert reg["form"] == gl_form(h, "resid_reg", "resid") and lds["form"] == gl_form(h, "lds", "resid")
    assert np.array_equal(reg["out"], lds["out"])


@pytest.mark.parametrize("tile", list(REG))
def test_fp32_rows_of_a_equal_the_same_values_as_bf16_and_padded_pitches_equal_dense(capi, tile):
    """A16 hands over 'the rounding the staging path would apply -- same operand values' (kernels.hpp); lda / ldw padded with NaN behind every row."""
    M, N, K = REG_SHAPES[tile][-1]
    for epi in ("silu", "resid"):
        a32, _ = run(capi, reg_form(tile, False, epi), M, N, K, epi, fast=False)
        a16, _ = run(capi, reg_form(tile, True, epi), M, N, K, epi, fast=False)
        assert np.array_equal(a32.view(np.uint32), a16.view(np.uint32)), f"{epi}: fp32 A against bf16 A"
        for f, lda in ((reg_form(tile, False, epi), K + 4), (reg_form(tile, True, epi), K + 8)):
            pad, _ = run(capi, f, M, N, K, epi, fast=False, lda=lda, ldw=K + 8)
            assert np.array_equal(pad.view(np.uint32), a32.view(np.uint32)), f"{epi}: padded operand pitches"


def test_padded_pitches_on_the_direct_to_lds_kernel(capi):
    M, N, K = GL_SHAPES[192, "direct"]
    dense, _ = run(capi, gl_form(192, "direct", "silu"), M, N, K, "silu")
    pad, _ = run(capi, gl_form(192, "direct", "silu"), M, N, K, "silu", lda=K + 8, ldw=K + 16, ldo=N + 8)
    assert np.array_equal(pad.view(np.uint32), dense.view(np.uint32))


@pytest.mark.parametrize("h", list(GL))
def test_blocked_hand_off_fc1_to_fc2(capi, h):
    """fc1 (SiLU, fast_act, bf16 rows, blocked) -> fc2 (a_blocked, residual) against the same pair with a row-major hand-off, bit for bit, at M % 32 = 8; rows
    M .. roundup32(M) - 1 of the blocked buffer still hold the fill."""
    M, F, D = GL_SHAPES[h, "direct"]                                 # fc1: D -> F
    K2, D2 = F // 64 * 64, {192: 1024, 256: 1520}[h]                 # fc2: the first K2 of the F columns -> D2 (K % 64 == 0; the height fc1 ran on)
    A, W1, b1, _ = ops(M, F, D, False, "coherent")
    rng = np.random.default_rng(h)
    W2 = rng.standard_normal((D2, K2), dtype=np.float32) / 32
    Rs = rng.standard_normal((M, D2), dtype=np.float32)
    Mr = (M + 31) // 32 * 32
    hand = {}
    for fmt in ("bf16", "blocked"):
        got = capi.diag_gemm_bf16_tile(A, W1, bias=b1, epi="silu", a16=True, fast_act=True, out_bf16=True, out_blocked=fmt == "blocked")
        assert got["form"] == gl_form(h, "direct", "silu")
        el = R.words_to_bf16(got["out"])
        hand[fmt] = el[R.blocked_offsets(M, F, F)] if fmt == "blocked" else el[:M * F].reshape(M, F)
        if fmt == "blocked":
            tail = R.blocked_offsets(Mr, F, F)[M:]
            assert np.array_equal(el[tail], np.where(tail % 2 == 0, R.FILL16[0], R.FILL16[1])), "rows M .. roundup32(M) - 1 of the blocked buffer were written"
    assert np.array_equal(hand["bf16"], hand["blocked"])
    H = R.bf16_value(hand["bf16"])[:, :K2]                           # exact in bf16: the entry's rounding returns the same bits
    outs = []
    for blocked in (False, True):
        got = capi.diag_gemm_bf16_tile(H, W2, epi="resid", resid=Rs, alpha=0.5, a16=True, a_blocked=blocked, lda=F)
        assert got["form"] == gl_form(h, "resid_reg", "resid")
        outs.append(got["out"])
    assert np.array_equal(outs[0], outs[1]), "fc2 on the blocked hand-off against the row-major one"
    p = R.product(H, W2, None, "resid", Rs, 0.5)
    check(capi, dict(out=outs[1]), p, M, D2, "resid", f"fc2-a_blocked-{h}: ", K=K2, resid_reg=True, resid=Rs)


# ---- output mappings on the register-staged kernel and the LDS epilogue ---------------------------------------------------------------------------------
MAP_CASES = [("128x128", (1030, 1028, 128)), ("128x64", (1030, 260, 128)), ("64x64", (130, 70, 192))]


@pytest.mark.parametrize("tile,shape", MAP_CASES, ids=[t for t, _ in MAP_CASES])
def test_sigma_columns_and_scalar_epilogue(capi, tile, shape):
    """sigma_cols = 0, a multiple of 16 inside the row, N rounded down to 16, through the wide epilogue and (ldo = N + 3) the scalar one: the same words."""
    M, N, K = shape
    f = reg_form(tile, True, "silu")
    for sc in (0, 48, N // 16 * 16):
        wide, _ = run(capi, f, M, N, K, "silu", fast=False, sigma_cols=sc)
        scalar, _ = run(capi, f, M, N, K, "silu", fast=False, sigma_cols=sc, ldo=N + 3)
        assert np.array_equal(wide.view(np.uint32), scalar.view(np.uint32)), f"sigma_cols={sc}: scalar against wide epilogue"
    run(capi, reg_form(tile, True, "resid"), M, N + 1, K, "resid", alpha=0.5, fast=False)      # N % 4 != 0: the scalar epilogue


def test_sigma_columns_on_the_direct_to_lds_kernel(capi):
    M, N, K = GL_SHAPES[192, "direct"]
    run(capi, gl_form(192, "lds", "none"), M, N, K, "none", sigma_cols=N // 16 * 16)


@pytest.mark.parametrize("tile,shape", MAP_CASES[:2], ids=[t for t, _ in MAP_CASES[:2]])
def test_subsampling_remap(capi, tile, shape):
    """The last subsampling conv's pattern: row (t, w) column c goes to out[t][c][w] (remap_rows = W3, gs = C W3, rs = 1, cs = W3)."""
    M, C, K = shape
    W3 = 10
    assert M % W3 == 0
    run(capi, reg_form(tile, False, "relu"), M, C, K, "relu", fast=False, remap=(W3, C * W3, 1, W3), out_words=M * C + 9)


# ---- the MFMA C layout -----------------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [("reg", "64x64", "lds", (130, 70, 192), "f32"), ("reg", "128x64", "lds", (1030, 260, 128), "f32"), ("reg", "128x128", "lds", (1030, 1028, 128), "f32"),
                ("reg", "128x128", "lds", (1030, 1028, 128), "bf16")]
LAYOUT_CASES += [("glds", h, efo, GL_SHAPES[h, efo], fmt) for h in GL for efo in ("direct", "persist") for fmt in ("f32", "bf16", "blocked")]
LAYOUT_CASES += [("glds", h, "lds", GL_SHAPES[h, "direct"], fmt) for h in GL for fmt in ("f32", "bf16")] + [("glds", h, "resid_reg", GL_SHAPES[h, "direct"], "f32") for h in GL]


@pytest.mark.parametrize("kernel,geo,efo,shape,fmt", LAYOUT_CASES, ids=[f"{k}-{g}-{f}-{t}" for k, g, f, _, t in LAYOUT_CASES])
def test_identity_rows_return_the_transposed_weights(capi, kernel, geo, efo, shape, fmt):
    """A = the first M rows of I (zero rows below K) and an asymmetric W of values exact in bf16, no bias: out[m][n] is W[n][m] itself, in every row format --
    a swapped column group of the permlane32_swap repack, a transposed block or a wrong block offset shows as a wrong VALUE, not as a small error."""
    M, N, K = shape
    A = np.eye(M, K, dtype=np.float32)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    W = ((n * 7 + k * 13) % 251 - 125).astype(np.float32) * np.float32(0.25)     # 8 significant bits at most: exact in bf16; no symmetry in (n, k)
    want = np.zeros((M, N), np.float32)
    want[:min(M, K)] = W.T[:min(M, K)]
    resid = efo == "resid_reg"
    ldo = N + 4 if (kernel == "glds" and efo == "lds") else N
    got = capi.diag_gemm_bf16_tile(A, W, epi="resid" if resid else "none", resid=np.zeros((M, N), np.float32) if resid else None, a16=True,
                                   out_bf16=fmt != "f32", out_blocked=fmt == "blocked", ldo=ldo)
    assert got["form"] == ((kernel, REG[geo], True, efo, "none") if kernel == "reg" else gl_form(geo, efo, "resid" if resid else "none"))
    if fmt == "f32":
        assert np.array_equal(got["out"].view(np.float32)[R.output_offsets(M, N, ldo)], want)
    else:
        off = R.blocked_offsets(M, N, ldo) if fmt == "blocked" else R.output_offsets(M, N, ldo)
        assert np.array_equal(R.words_to_bf16(got["out"])[off], R.bf16_bits(want).reshape(M, N))


# ---- the activations alone ---------------------------------------------------------------------------------------------------------------------------------
def test_fast_activations_alone(capi):
    """fast_sigmoidf / fast_siluf (pk_diag_math) against float64 over [-30, 30]: within fast_sigmoid_rel (SiLU: + 2^-24); the special values."""
    x = np.concatenate([np.linspace(-30, 30, 400001), np.random.default_rng(3).uniform(-30, 30, 200000)]).astype(np.float32)
    x64 = x.astype(np.float64)
    sg, sl = capi.diag_math("fast_sigmoid", x).astype(np.float64), capi.diag_math("fast_silu", x).astype(np.float64)
    want = R.sigmoid64(x64)
    rel = np.abs(sg - want) / want
    print(f"fast_sigmoid: worst relative error / bound = {np.max(rel / R.fast_sigmoid_rel(x64)):.3f}")
    assert np.all(rel <= R.fast_sigmoid_rel(x64))
    nz = x64 != 0
    rel = np.abs(sl[nz] - x64[nz] * want[nz]) / np.abs(x64[nz] * want[nz])
    print(f"fast_silu: worst relative error / bound = {np.max(rel / (R.fast_sigmoid_rel(x64[nz]) + 2.0 ** -24)):.3f}")
    assert np.all(rel <= R.fast_sigmoid_rel(x64[nz]) + 2.0 ** -24)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 200.0, -200.0, np.nan], np.float32)
    sg, sl = capi.diag_math("fast_sigmoid", sp), capi.diag_math("fast_silu", sp)
    assert sg[0] == 0.5 and sg[1] == 0.5 and sg[2] == 1.0 and sg[3] == 0.0 and sg[4] == 1.0 and sg[5] == 0.0 and np.isnan(sg[6])
    assert sl[0] == 0.0 and sl[1] == 0.0 and sl[2] == np.inf and sl[4] == 200.0 and sl[5] == 0.0 and np.isnan(sl[6])
    assert np.isnan(sl[3])                                           # -inf * 0: the hardware form has no guard (the polynomial one returns -0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(capi):
    """What launch_gemm_bf16 aborts on, and what Model::run_gemm refuses for a bf16 output: a status before any launch."""
    M, N, K = GL_SHAPES[192, "direct"]
    q = capi.diag_gemm_bf16_tile_form
    assert q(M, N, K, epi="silu", a16=True, fast_act=True, out_bf16=True, out_blocked=True)[3] == "direct"
    bad = [dict(M=M, N=N, K=K, epi="silu", a16=True, fast_act=False, out_bf16=True, out_blocked=True),          # polynomial SiLU: the LDS epilogue
           dict(M=M, N=N, K=K, epi="none", a16=True, out_bf16=True, out_blocked=True, ldo=N + 16, sigma_cols=16),
           dict(M=1030, N=1040, K=128, epi="none", a16=True, out_bf16=True, out_blocked=True),                   # the register-staged kernel
           dict(M=1030, N=1040, K=128, epi="none", a16=True, a_blocked=True, lda=128),
           dict(M=M, N=N, K=K, epi="glu", a16=True, fast_act=True, out_bf16=True),
           dict(M=M, N=N, K=K, epi="resid", a16=True, out_bf16=True),
           dict(M=M, N=N, K=K, epi="none", a16=True, out_bf16=True, sigma_cols=16),
           dict(M=1030, N=260, K=128, epi="none", out_bf16=True, remap=(10, 2600, 1, 10)),
           dict(M=1030, N=262, K=128, epi="none", out_bf16=True, ldo=262),
           dict(M=1030, N=260, K=128, epi="glu", sigma_cols=16),
           dict(M=1030, N=260, K=128, epi="resid", sigma_cols=16),
           dict(M=64, N=260, K=256, epi="none")]                                                               # the small-M bf16 kernel's
    for kw in bad:
        with pytest.raises(capi.PkError) as e:
            q(**kw)
        assert e.value.code == PK_ERR_UNSUPPORTED, kw
    with pytest.raises(capi.PkError) as e:                           # ... and from the launching entry itself
        capi.diag_gemm_bf16_tile(np.zeros((1030, 128), np.float32), np.zeros((1040, 128), np.float32), a16=True, out_bf16=True, out_blocked=True)
    assert e.value.code == PK_ERR_UNSUPPORTED


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_form_has_a_case(capi):
    """The union of the forms the form cases above assert they launch is every form the launcher can take."""
    have = {reg_form(tile, a16, epi) for tile, _, _, _, epi, a16 in REG_CASES} | {gl_form(h, efo, epi) for h, efo, _, _, _, epi in GL_CASES}
    every = set(capi.diag_gemm_bf16_tile_forms())
    assert len(every) == 54
    assert every - have == set(), f"forms no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for forms the library does not list: {sorted(have - every)}"
    for k in sorted(WORST):
        print(f"worst |err| / bound  {k}: {WORST[k]:.3f}")
