"""The small-M bf16 GEMM family alone (csrc/kernels/gemm_smallm_bf16.hip through pk_diag_gemm_smallm_bf16: one product per call): every form
launch_gemm_smallm_bf16 can take -- five epilogues, K slices of 256 / 512 k, one or two row tiles per wave with 8 or 16 rows of a tile in use, fp32 / bf16 rows /
a folded LayerNorm, one or two column tiles per wave, natural or operand-tiled weights, the conv tail, 8-row activation tiles, LDS-DMA rows, the second norm -- at
small shapes that reach it, with operand pitches, NaN behind every row, and the whole of out / pre_out / cache_out handed back.

Reference: tests/smallm_bf16_gemm_ref.py (on tests/bf16_gemm_ref.py) -- the float64 product of the operands rounded to bf16, the LayerNorm in float64, every
epilogue function in float64, placed where GemmArgs puts it; every word no element belongs to must still hold the fill.  Each case names the form it is written
for and compares it with the form the launcher switched on (no threshold is restated here); test_every_form_has_a_case compares the union with the library's
table both ways.  tests/test_smallm_bf16_gemm_ref.py asks the host-side form function the same question for every case, without a device.

Bounds, the project's existing ones (bf16_gemm_ref / smallm_bf16_gemm_ref carry the derivations):
  * fp32 rows: |err| <= 2e-6 mag + 1e-6, mag = |Aq| |Wq|^T + |bias| (GLU: both halves summed);
  * a folded norm: + flip = 4 * 2^-8 * max|a| max|w| -- a last-bit difference of the fp32 LayerNorm may move a few operands to the neighbouring bf16 value;
    the second norm is applied to the fp32 pre_out the device returned, and pre_out itself is within 2e-6 (1 + max|y|) of float64;
  * fast_act: out_bound(..., fast=True), no further allowance;  bf16 rows: check_bf16_rows, at most 2 % of the elements excused;
  * the conv tail: the new cache rows ARE the GLU values (checked as the product's output); the activations against stream_dwconv_f64 of those values within
    1e-5 (1 + max|want|) (tests/test_gpu_smallm_gemm.py);
  * every comparison called "bit for bit" has no tolerance."""
import functools

import numpy as np
import pytest

import smallm_bf16_gemm_ref as R
from conftest import pk  # noqa: F401

pytestmark = pytest.mark.gpu

PK_ERR_UNSUPPORTED = -7
WORST = {}                                                           # form label -> worst |err| / bound seen (printed by test_every_form_has_a_case)


@pytest.fixture(scope="module")
def capi():
    from parakeet_cpp_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product has no CPU path"
    return capi


def F(epi, steps, rt, rvalid, flags=""):
    """A form as capi.smallm_bf16_form decodes it: (epi, STEPS, RT, rvalid, A16, LN, CT, WT, DW, AT, AL, PRE); flags: the words of "a16 ln ct2 wt dw at al pre"."""
    fl = flags.split()
    assert set(fl) <= {"a16", "ln", "ct2", "wt", "dw", "at", "al", "pre"}
    return (epi, steps, rt, rvalid, "a16" in fl, "ln" in fl, 2 if "ct2" in fl else 1, "wt" in fl, "dw" in fl, "at" in fl, "al" in fl, "pre" in fl)


def label(f):
    names = ("a16", "ln", None, "wt", "dw", "at", "al", "pre")
    return f"{f[0]}-s{f[1]}-rt{f[2]}-rv{f[3]}" + ("-ct2" if f[6] == 2 else "") + "".join(f"-{n}" for n, v in zip(names, f[4:]) if n and v)


# (epi, STEPS, RT, rvalid, flags, M, N, K, frames per stream of the conv tail): one case per form, at a shape that reaches it.  M in {1, 7, 8, 9, 16, 17, 33, 100,
# 128}: one row, a partial / a whole / one more than a whole 8-row and 16-row tile, a partial last group of 32, the limit; N in {16, 24, 272, 768, 784, 1030, ...}:
# one column tile, a partial one (ragged N: natural weights only), N % 32 == 16; K = 256 (one slice) ... 4352 / 4608 (more slices than waves; 17 slices of 256).
CASES = [
    ("glu", 8, 1, 8, "", 9, 272, 4608, 0),
    ("glu", 8, 1, 8, "dw", 7, 768, 4352, 1),
    ("glu", 8, 1, 8, "wt al", 1, 1536, 256, 0),
    ("glu", 8, 1, 8, "wt dw al", 8, 272, 2048, 4),
    ("glu", 8, 1, 8, "ln", 7, 1536, 256, 0),
    ("glu", 8, 1, 8, "ln dw", 8, 3088, 256, 2),
    ("glu", 8, 1, 8, "ln wt al", 33, 272, 512, 0),
    ("glu", 8, 1, 8, "ln wt dw al", 16, 16, 256, 4),
    ("glu", 8, 1, 8, "a16", 7, 3088, 256, 0),
    ("glu", 8, 1, 8, "a16 dw", 9, 768, 2048, 1),
    ("glu", 8, 1, 8, "a16 wt", 1, 768, 2048, 0),
    ("glu", 8, 1, 8, "a16 wt dw", 9, 272, 2304, 1),
    ("glu", 8, 1, 16, "", 100, 768, 512, 0),
    ("glu", 8, 1, 16, "dw", 33, 3088, 512, 1),
    ("glu", 8, 1, 16, "wt al", 9, 3088, 2048, 0),
    ("glu", 8, 1, 16, "wt dw al", 17, 3088, 256, 1),
    ("glu", 8, 1, 16, "ln", 100, 768, 512, 0),
    ("glu", 8, 1, 16, "ln dw", 100, 768, 512, 4),
    ("glu", 8, 1, 16, "ln wt al", 16, 3072, 512, 0),
    ("glu", 8, 1, 16, "ln wt dw al", 128, 768, 256, 1),
    ("glu", 8, 1, 16, "a16", 16, 3072, 512, 0),
    ("glu", 8, 1, 16, "a16 dw", 17, 1536, 512, 1),
    ("glu", 8, 1, 16, "a16 wt", 16, 3072, 256, 0),
    ("glu", 8, 1, 16, "a16 wt dw", 100, 768, 512, 1),
    ("none", 8, 1, 8, "", 100, 16, 256, 0),
    ("none", 8, 1, 8, "wt al", 16, 272, 4096, 0),
    ("none", 8, 1, 8, "ln", 7, 3088, 256, 0),
    ("none", 8, 1, 8, "ln wt al", 100, 272, 2048, 0),
    ("none", 8, 1, 8, "a16", 7, 272, 2048, 0),
    ("none", 8, 1, 8, "a16 wt", 16, 768, 256, 0),
    ("none", 8, 1, 16, "", 33, 1030, 2304, 0),
    ("none", 8, 1, 16, "wt al", 9, 3072, 256, 0),
    ("none", 8, 1, 16, "ct2", 128, 768, 512, 0),
    ("none", 8, 1, 16, "ct2 wt al", 128, 768, 512, 0),
    ("none", 8, 1, 16, "ln", 128, 3072, 256, 0),
    ("none", 8, 1, 16, "ln wt al", 33, 1536, 256, 0),
    ("none", 8, 1, 16, "ln ct2", 128, 768, 512, 0),
    ("none", 8, 1, 16, "ln ct2 wt al", 128, 768, 512, 0),
    ("none", 8, 1, 16, "a16", 128, 1030, 256, 0),
    ("none", 8, 1, 16, "a16 wt", 16, 3072, 2304, 0),
    ("none", 8, 2, 16, "", 100, 768, 512, 0),
    ("none", 8, 2, 16, "wt", 33, 3088, 512, 0),
    ("none", 8, 2, 16, "ln", 17, 3088, 2048, 0),
    ("none", 8, 2, 16, "ln wt", 17, 3088, 512, 0),
    ("none", 8, 2, 16, "a16", 128, 768, 512, 0),
    ("none", 8, 2, 16, "a16 wt", 128, 768, 512, 0),
    ("none", 16, 1, 8, "a16", 128, 24, 4608, 0),
    ("none", 16, 1, 8, "a16 wt", 9, 272, 4608, 0),
    ("none", 16, 1, 16, "a16", 17, 1536, 4096, 0),
    ("none", 16, 1, 16, "a16 wt", 9, 3072, 4096, 0),
    ("none", 16, 2, 16, "a16", 33, 1536, 4096, 0),
    ("none", 16, 2, 16, "a16 wt", 33, 1536, 4096, 0),
    ("relu", 8, 1, 8, "", 8, 24, 4096, 0),
    ("relu", 8, 1, 8, "wt al", 8, 272, 4352, 0),
    ("relu", 8, 1, 8, "ln", 7, 272, 2048, 0),
    ("relu", 8, 1, 8, "ln wt al", 7, 16, 2048, 0),
    ("relu", 8, 1, 8, "a16", 128, 272, 512, 0),
    ("relu", 8, 1, 8, "a16 wt", 1, 768, 256, 0),
    ("relu", 8, 1, 16, "", 33, 3072, 256, 0),
    ("relu", 8, 1, 16, "wt al", 16, 3072, 256, 0),
    ("relu", 8, 1, 16, "ct2", 128, 768, 512, 0),
    ("relu", 8, 1, 16, "ct2 wt al", 128, 768, 512, 0),
    ("relu", 8, 1, 16, "ln", 16, 3088, 2048, 0),
    ("relu", 8, 1, 16, "ln wt al", 17, 1536, 2048, 0),
    ("relu", 8, 1, 16, "ln ct2", 128, 768, 512, 0),
    ("relu", 8, 1, 16, "ln ct2 wt al", 128, 768, 512, 0),
    ("relu", 8, 1, 16, "a16", 9, 3072, 4352, 0),
    ("relu", 8, 1, 16, "a16 wt", 9, 3072, 4352, 0),
    ("relu", 8, 2, 16, "", 128, 1030, 512, 0),
    ("relu", 8, 2, 16, "wt", 17, 3088, 512, 0),
    ("relu", 8, 2, 16, "ln", 17, 3088, 2048, 0),
    ("relu", 8, 2, 16, "ln wt", 100, 768, 512, 0),
    ("relu", 8, 2, 16, "a16", 128, 768, 512, 0),
    ("relu", 8, 2, 16, "a16 wt", 128, 768, 512, 0),
    ("relu", 16, 1, 8, "a16", 128, 16, 4096, 0),
    ("relu", 16, 1, 8, "a16 wt", 16, 768, 4608, 0),
    ("relu", 16, 1, 16, "a16", 9, 3088, 4096, 0),
    ("relu", 16, 1, 16, "a16 wt", 9, 3088, 4096, 0),
    ("relu", 16, 2, 16, "a16", 33, 1536, 4096, 0),
    ("relu", 16, 2, 16, "a16 wt", 33, 1536, 4096, 0),
    ("resid", 8, 1, 8, "", 8, 24, 4608, 0),
    ("resid", 8, 1, 8, "wt al", 33, 768, 256, 0),
    ("resid", 8, 1, 8, "ln", 7, 768, 512, 0),
    ("resid", 8, 1, 8, "ln wt al", 128, 272, 512, 0),
    ("resid", 8, 1, 8, "a16", 9, 272, 256, 0),
    ("resid", 8, 1, 8, "a16 at", 8, 1030, 256, 0),
    ("resid", 8, 1, 8, "a16 wt", 100, 272, 2048, 0),
    ("resid", 8, 1, 8, "a16 wt at", 8, 784, 2304, 0),
    ("resid", 8, 1, 16, "", 17, 1536, 2304, 0),
    ("resid", 8, 1, 16, "wt al", 9, 3072, 4352, 0),
    ("resid", 8, 1, 16, "ct2", 128, 768, 512, 0),
    ("resid", 8, 1, 16, "ct2 wt al", 128, 768, 512, 0),
    ("resid", 8, 1, 16, "ln", 100, 1536, 256, 0),
    ("resid", 8, 1, 16, "ln wt al", 128, 3088, 256, 0),
    ("resid", 8, 1, 16, "ln ct2", 128, 768, 512, 0),
    ("resid", 8, 1, 16, "ln ct2 wt al", 128, 768, 512, 0),
    ("resid", 8, 1, 16, "a16", 17, 3072, 256, 0),
    ("resid", 8, 1, 16, "a16 at", 16, 3072, 2304, 0),
    ("resid", 8, 1, 16, "a16 wt", 17, 1536, 4352, 0),
    ("resid", 8, 1, 16, "a16 wt at", 16, 3088, 2048, 0),
    ("resid", 8, 2, 16, "", 17, 3088, 2304, 0),
    ("resid", 8, 2, 16, "wt", 128, 784, 512, 0),
    ("resid", 8, 2, 16, "ln", 33, 1536, 512, 0),
    ("resid", 8, 2, 16, "ln wt", 128, 784, 512, 0),
    ("resid", 8, 2, 16, "a16", 128, 768, 512, 0),
    ("resid", 8, 2, 16, "a16 at", 128, 768, 512, 0),
    ("resid", 8, 2, 16, "a16 wt", 128, 768, 512, 0),
    ("resid", 8, 2, 16, "a16 wt at", 128, 768, 512, 0),
    ("resid", 16, 1, 8, "a16", 1, 3088, 4096, 0),
    ("resid", 16, 1, 8, "a16 at", 8, 3088, 4608, 0),
    ("resid", 16, 1, 8, "a16 wt", 9, 784, 4608, 0),
    ("resid", 16, 1, 8, "a16 wt at", 8, 784, 4096, 0),
    ("resid", 16, 1, 16, "a16", 9, 3088, 4608, 0),
    ("resid", 16, 1, 16, "a16 at", 16, 3072, 4096, 0),
    ("resid", 16, 1, 16, "a16 wt", 9, 3072, 4608, 0),
    ("resid", 16, 1, 16, "a16 wt at", 16, 3072, 4096, 0),
    ("resid", 16, 2, 16, "a16", 33, 1536, 4096, 0),
    ("resid", 16, 2, 16, "a16 at", 128, 768, 4096, 0),
    ("resid", 16, 2, 16, "a16 wt", 33, 1536, 4096, 0),
    ("resid", 16, 2, 16, "a16 wt at", 128, 768, 4096, 0),
    ("silu", 8, 1, 8, "", 16, 768, 4096, 0),
    ("silu", 8, 1, 8, "wt al", 1, 3088, 2048, 0),
    ("silu", 8, 1, 8, "ln", 17, 272, 512, 0),
    ("silu", 8, 1, 8, "ln pre", 1, 784, 256, 0),
    ("silu", 8, 1, 8, "ln wt al", 9, 768, 2048, 0),
    ("silu", 8, 1, 8, "ln wt al pre", 7, 3072, 512, 0),
    ("silu", 8, 1, 8, "a16", 1, 1536, 256, 0),
    ("silu", 8, 1, 8, "a16 wt", 1, 768, 512, 0),
    ("silu", 8, 1, 16, "", 16, 3072, 512, 0),
    ("silu", 8, 1, 16, "wt al", 100, 3072, 256, 0),
    ("silu", 8, 1, 16, "ct2", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "ct2 wt al", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "ln", 100, 1536, 256, 0),
    ("silu", 8, 1, 16, "ln pre", 100, 784, 512, 0),
    ("silu", 8, 1, 16, "ln wt al", 17, 3072, 256, 0),
    ("silu", 8, 1, 16, "ln wt al pre", 33, 3088, 256, 0),
    ("silu", 8, 1, 16, "ln ct2", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "ln ct2 pre", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "ln ct2 wt al", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "ln ct2 wt al pre", 128, 768, 512, 0),
    ("silu", 8, 1, 16, "a16", 9, 3088, 512, 0),
    ("silu", 8, 1, 16, "a16 wt", 128, 768, 256, 0),
    ("silu", 8, 2, 16, "", 100, 1030, 512, 0),
    ("silu", 8, 2, 16, "wt", 17, 3088, 2304, 0),
    ("silu", 8, 2, 16, "ln", 100, 1030, 512, 0),
    ("silu", 8, 2, 16, "ln wt", 100, 784, 512, 0),
    ("silu", 8, 2, 16, "a16", 128, 768, 512, 0),
    ("silu", 8, 2, 16, "a16 wt", 128, 768, 512, 0),
    ("silu", 16, 1, 8, "a16", 8, 3072, 4608, 0),
    ("silu", 16, 1, 8, "a16 wt", 1, 1536, 4608, 0),
    ("silu", 16, 1, 16, "a16", 33, 1030, 4096, 0),
    ("silu", 16, 1, 16, "a16 wt", 17, 1536, 4608, 0),
    ("silu", 16, 2, 16, "a16", 33, 1536, 4096, 0),
    ("silu", 16, 2, 16, "a16 wt", 33, 1536, 4096, 0),
]
CASES = [(F(*c[:5]), *c[5:]) for c in CASES]
IDS = [f"{label(f)}-{M}x{N}x{K}" for f, M, N, K, _ in CASES]


def shape_of(form):
    """The case shape written for a form"""
    hit = [c[1:] for c in CASES if c[0] == form]
    assert len(hit) == 1, form
    return hit[0]


@functools.lru_cache(maxsize=8)
def ops(M, N, K, glu):
    """A [M][K] (rows of different scale and offset: a LayerNorm has something to do), W [N or 2N][K] / sqrt(K), bias, residual [M][N], two norms, the conv
    module's vectors and a cache for M streams: one set per shape, shared by every case on it and never written."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + (1 << 20 if glu else 0))
    rows = 2 * N if glu else N
    o = dict(A=(rng.standard_normal((M, K)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))).astype(np.float32),
             W=rng.standard_normal((rows, K), dtype=np.float32) / np.float32(np.sqrt(K)), b=rng.standard_normal(rows).astype(np.float32),
             resid=rng.standard_normal((M, N), dtype=np.float32),
             ln=(rng.uniform(0.5, 1.5, K).astype(np.float32), (0.2 * rng.standard_normal(K)).astype(np.float32)),
             pre=(rng.uniform(0.5, 1.5, K).astype(np.float32), (0.2 * rng.standard_normal(K)).astype(np.float32)),
             conv=dict(w=(rng.standard_normal((9, N)) / 3).astype(np.float32), bias=(0.1 * rng.standard_normal(N)).astype(np.float32),
                       bn_mean=(0.1 * rng.standard_normal(N)).astype(np.float32), bn_rstd=rng.uniform(0.5, 1.5, N).astype(np.float32),
                       bn_g=rng.uniform(0.5, 1.5, N).astype(np.float32), bn_b=(0.1 * rng.standard_normal(N)).astype(np.float32)),
             cache=rng.standard_normal((M, 8, N), dtype=np.float32))
    for a in (o["A"], o["W"], o["b"], o["resid"], o["cache"], *o["ln"], *o["pre"], *o["conv"].values()):
        a.setflags(write=False)
    return o


def slack_words(M, ld, bf16):
    """The words of a buffer of roundup32(M) + 8 rows (every row a partial last row group or one more 8-row tile could reach) and 7 more"""
    el = ((M + 31) // 32 * 32 + 8) * ld
    return ((el + 1) // 2 if bf16 else el) + 7


def fill16_outside(el, off, what):
    rest = np.ones(el.size, bool)
    rest[np.asarray(off).reshape(-1)] = False
    fill = np.where(np.arange(el.size) % 2 == 0, R.FILL16[0], R.FILL16[1]).astype(np.uint16)
    assert np.array_equal(el[rest], fill[rest]), f"{what}: {int((el[rest] != fill[rest]).sum())} bf16 elements outside the written ones hold something else than the fill"


def fill_outside(words, off, what):
    rest = np.ones(words.size, bool)
    rest[np.asarray(off).reshape(-1)] = False
    assert np.all(words[rest] == R.FILL32), f"{what}: {int((words[rest] != R.FILL32).sum())} words outside the written elements hold something else than the fill"


def check_f32(words, off, want, bound, what, key):
    vals = words.view(np.float32)[off]
    err = np.abs(vals.astype(np.float64) - want)
    worst = float(np.max(err / bound))
    print(f"{what}: worst |err| / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: |err| exceeds the bound at {int((err > bound).sum())} elements, worst ratio {worst:.3f}"
    fill_outside(words, off, what)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return vals


def run(capi, form, M, N, K, c=0, bias=True, alpha=0.5, fast=False, has_cache=True, out_bf16=False, out_t8=False, resid_in_place=False, spare_streams=2, **pitch):
    """One product alone on the form the case is written for: the form the launcher switched on is that form, and out / pre_out / cache_out hold the reference
    within its bound where GemmArgs puts it and the fill everywhere else.  -> (the output elements in natural order, the result dict)."""
    epi, a16, ln, wt, dw, at, pre = form[0], form[4], form[5], form[7], form[8], form[9], form[11]
    o = ops(M, N, K, epi == "glu")
    what = f"{label(form)}: {M}x{N}x{K} bias={bias} fast={fast} {pitch}"
    ldo = pitch.get("ldo", N)
    S = M // c if dw else 0
    conv = dict(c=c, has_cache=has_cache, cache_in=np.ascontiguousarray(o["cache"][:S]), cache_streams=S + spare_streams, **o["conv"]) if dw else None
    resid = o["resid"] if epi == "resid" else None
    if resid_in_place:
        pitch["ldr"] = ldo
    # whole rows past M: a store of the last row group that misses its row guard lands inside what comes back
    pitch.setdefault("out_words", slack_words(M, ldo, out_bf16))
    if pre:
        pitch.setdefault("pre_out_words", slack_words(M, pitch.get("pre_ldo", K), False))
    got = capi.diag_gemm_smallm_bf16(o["A"], o["W"], bias=o["b"] if bias else None, epi=epi, resid=resid, alpha=alpha, a16=a16, a_t8=at, w_tiles=wt, fast_act=fast,
                                     out_bf16=out_bf16, out_t8=out_t8, resid_in_place=resid_in_place, ln=o["ln"] if ln else None, pre=o["pre"] if pre else None,
                                     dw=conv, **pitch)
    assert got["form"] == form, f"{what}: launched {label(got['form'])}"
    b = o["b"] if bias else None
    if pre:
        pre_ldo = pitch.get("pre_ldo", K)
        y = R.layer_norm64(o["A"], *o["pre"])
        poff = R.output_offsets(M, K, pre_ldo)
        pv = got["pre_out"].view(np.float32)[poff]
        perr = np.abs(pv.astype(np.float64) - y).max()
        print(f"{what}: pre_out max err {perr:.3e}, bound {R.pre_out_bound(y):.3e}")
        assert perr <= R.pre_out_bound(y), f"{what}: pre_out"
        fill_outside(got["pre_out"], poff, what + " pre_out")
        p = R.folded_product(pv, *o["ln"], o["W"], b, epi)          # the second norm, on the fp32 rows the device wrote
    elif ln:
        p = R.folded_product(o["A"], *o["ln"], o["W"], b, epi, resid, alpha)
    else:
        p = R.product(o["A"], o["W"], b, epi, resid, alpha)
    bound = R.out_bound(p, epi, fast) + (p["flip"] if ln else 0.0)
    if dw:
        co = got["cache_out"].reshape(S + spare_streams, 8, N)
        assert np.all(co[S:] == R.FILL32), f"{what}: a cache word outside the {S} streams was written"
        assert got["out"].size > M * ldo and np.all(got["out"][M * ldo:] == R.FILL32), f"{what}: a word behind the activations was written"
        glu = co[:S, 8 - c:].view(np.float32)                       # the new cache rows: the GLU values themselves
        err = np.abs(glu.reshape(M, N).astype(np.float64) - p["want"])
        worst = float(np.max(err / bound))
        print(f"{what}: GLU rows in the cache, worst |err| / bound = {worst:.3f}")
        assert np.all(err <= bound), f"{what}: GLU rows, worst ratio {worst:.3f}"
        WORST[label(form)] = max(WORST.get(label(form), 0.0), worst)
        old = o["cache"][:S, c:].view(np.uint32) if has_cache else np.zeros((S, 8 - c, N), np.uint32)
        assert np.array_equal(co[:S, :8 - c], old), f"{what}: the old cache rows, shifted"
        want, _ = R.stream_dwconv_f64(glu, o["cache"][:S], has_cache, *(o["conv"][k] for k in ("w", "bias", "bn_mean", "bn_rstd", "bn_g", "bn_b")))
        off = R.output_offsets(M, N, ldo)
        act = got["out"].view(np.float32)[off]
        cerr, cbound = np.abs(act - want.reshape(M, N)).max(), 1e-5 * (1.0 + np.abs(want).max())
        print(f"{what}: conv tail max |got - float64| = {cerr:.3e}, bound {cbound:.3e}")
        assert cerr <= cbound, what
        fill_outside(got["out"], off, what)
        return act, got
    if out_bf16:
        el = R.words_to_bf16(got["out"])
        off = R.t8_offsets(M, N) if out_t8 else R.output_offsets(M, N, ldo)
        worst, share = R.check_bf16_rows(el[off], p["want"], bound)   # (operands with cancellation: the excused share is printed, not capped -- test_bf16_rows_out)
        print(f"{what} bf16 rows{' t8' if out_t8 else ''}: worst |err| / bound = {worst:.3f}, excused {100 * share:.2f} %")
        WORST[label(form) + "-bf16rows"] = max(WORST.get(label(form) + "-bf16rows", 0.0), worst)
        fill16_outside(el, off, what)
        return el[off], got
    return check_f32(got["out"], R.output_offsets(M, N, ldo), p["want"], bound, what, label(form)), got


# ---- every form ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,M,N,K,c", CASES, ids=IDS)
def test_forms_against_float64(capi, form, M, N, K, c):
    run(capi, form, M, N, K, c)


def test_every_form_has_a_case(capi):
    """The union of the forms the cases above assert they launch is every form the launcher can take."""
    have = {c[0] for c in CASES}
    every = set(capi.diag_gemm_smallm_bf16_forms())
    assert len(every) == 154 and len(CASES) == 154
    assert every - have == set(), f"forms no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for forms the library does not list: {sorted(have - every)}"
    for k in sorted(WORST):
        print(f"worst |err| / bound  {k}: {WORST[k]:.3f}")


# ---- pitches ----------------------------------------------------------------------------------------------------------------------------------------------
PITCH_FORMS = [F("silu", 8, 1, 16, "wt al"), F("silu", 8, 1, 8, ""), F("none", 8, 2, 16, "a16"), F("none", 8, 1, 8, "a16 wt"), F("relu", 8, 1, 16, "ln wt al"),
               F("relu", 8, 2, 16, "ln"), F("resid", 8, 1, 16, "a16 wt"), F("resid", 8, 2, 16, ""), F("resid", 16, 2, 16, "a16 wt"), F("glu", 8, 1, 16, "ln wt al"),
               F("silu", 8, 1, 16, "ln ct2 wt al pre")]


@pytest.mark.parametrize("form", PITCH_FORMS, ids=[label(f) for f in PITCH_FORMS])
def test_padded_pitches_equal_dense_bit_for_bit(capi, form):
    """lda = K + 8, ldw = K + 8, ldo = N + 4, ldr = N + 12 (the second norm: pre_ldo = K + 4), NaN behind every row: the same words as the dense run."""
    M, N, K, c = shape_of(form)
    dense, _ = run(capi, form, M, N, K, c)
    kw = dict(lda=K + 8, ldw=K + 8, ldo=N + 4)
    if form[0] == "resid":
        kw["ldr"] = N + 12
    if form[11]:
        kw["pre_ldo"] = K + 4
    pad, _ = run(capi, form, M, N, K, c, **kw)
    assert np.array_equal(pad.view(np.uint32), dense.view(np.uint32))


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------------------------
def without(form, *names):
    idx = dict(wt=7, dw=8, at=9, al=10)
    f = list(form)
    for n in names:
        f[idx[n]] = False
    return tuple(f)


WT_FORMS = [f for f, *_ in CASES if f[7] and not f[8]][::3]


@pytest.mark.parametrize("form", WT_FORMS, ids=[label(f) for f in WT_FORMS])
def test_operand_tiled_weights_equal_natural_weights_bit_for_bit(capi, form):
    """kernels.hpp: 'Same values in the same lanes: bit-identical results' -- and fp32 rows by LDS-DMA against per-lane loads."""
    M, N, K, c = shape_of(form)
    tiled, _ = run(capi, form, M, N, K, c)
    natural, _ = run(capi, without(form, "wt", "al"), M, N, K, c)
    assert np.array_equal(tiled.view(np.uint32), natural.view(np.uint32))


AT_FORMS = [f for f, *_ in CASES if f[9]]


@pytest.mark.parametrize("form", AT_FORMS, ids=[label(f) for f in AT_FORMS])
def test_rows_in_8_row_tiles_equal_plain_bf16_rows_bit_for_bit(capi, form):
    M, N, K, c = shape_of(form)
    tiles, _ = run(capi, form, M, N, K)
    rows, _ = run(capi, without(form, "at"), M, N, K)
    assert np.array_equal(tiles.view(np.uint32), rows.view(np.uint32))


T8_CASES = [(F("silu", 8, 1, 8, "ln wt al"), 8, 768, 2048), (F("silu", 8, 1, 16, "ln ct2 wt al"), 128, 768, 512), (F("none", 8, 2, 16, "a16"), 128, 768, 512),
            (F("relu", 8, 1, 8, "a16"), 16, 96, 512)]


@pytest.mark.parametrize("form,M,N,K", T8_CASES, ids=[label(f) for f, *_ in T8_CASES])
def test_out_t8_places_every_element_where_t8_offsets_says(capi, form, M, N, K):
    """out_t8 against plain bf16 rows: the same bf16 elements, found through smallm_bf16_gemm_ref.t8_offsets (written from GemmArgs's description, not read back
    by a consumer), each within the bf16-rows bound of float64; the tile rows behind the M N elements hold the fill."""
    fast = form[0] == "silu"
    rows, g1 = run(capi, form, M, N, K, fast=fast, out_bf16=True)
    tiles, g2 = run(capi, form, M, N, K, fast=fast, out_bf16=True, out_t8=True)
    assert np.array_equal(tiles, rows)
    assert np.array_equal(R.from_t8(R.words_to_bf16(g2["out"])[:M * N], M, N), rows)


def test_tile_copy_words(capi):
    """launch_tile_copy_bf16 against the host expectation, word for word; dense and padded source rows (the NaN padding never reaches the copy)."""
    rng = np.random.default_rng(5)
    for rows, K, ld in ((16, 32, 32), (48, 256, 256), (32, 512, 520)):
        src = np.zeros((rows, ld), np.float32)
        src[:, :K] = rng.standard_normal((rows, K), dtype=np.float32)
        got = capi.diag_tile_copy_bf16(src, K)
        assert np.array_equal(got, R.w_t16_tiling(R.bf16_bits(src).reshape(rows, ld), K))


# ---- epilogues ------------------------------------------------------------------------------------------------------------------------------------------------
EPI_FORMS = [F(e, 8, 1, 8, fl) for e in ("none", "relu", "silu", "resid", "glu") for fl in ("wt al", "a16", "ln")]


@pytest.mark.parametrize("form", EPI_FORMS, ids=[label(f) for f in EPI_FORMS])
def test_epilogues_without_bias(capi, form):
    """A null bias (the form cases all pass one)"""
    run(capi, form, *shape_of(form), bias=False)


@pytest.mark.parametrize("form", [F("resid", 8, 1, 8, "a16 wt"), F("resid", 8, 2, 16, "a16 wt at"), F("resid", 8, 1, 16, "ct2 wt al")], ids=label)
def test_residual_scale_and_in_place(capi, form):
    """alpha in {1, 1/2, -1/4}; resid == out (production's fc2) gives the words of the separate residual buffer."""
    M, N, K, _ = shape_of(form)
    for alpha in (1.0, 0.5, -0.25):
        apart, _ = run(capi, form, M, N, K, alpha=alpha)
    inplace, _ = run(capi, form, M, N, K, alpha=-0.25, resid_in_place=True)
    assert np.array_equal(inplace.view(np.uint32), apart.view(np.uint32))
    padded, _ = run(capi, form, M, N, K, alpha=-0.25, resid_in_place=True, ldo=N + 4)
    assert np.array_equal(padded.view(np.uint32), apart.view(np.uint32))


FAST_FORMS = [F("silu", 8, 1, 16, "wt al"), F("silu", 8, 2, 16, "a16 wt"), F("silu", 8, 1, 16, "ln ct2 wt al pre"), F("silu", 16, 1, 8, "a16 wt"),
              F("glu", 8, 1, 16, "wt al"), F("glu", 8, 1, 8, "a16"), F("glu", 8, 1, 16, "ln wt dw al")]


@pytest.mark.parametrize("form", FAST_FORMS, ids=[label(f) for f in FAST_FORMS])
def test_fast_activations(capi, form):
    """GemmArgs::fast_act: the hardware exp2 / rcp SiLU and sigmoid within out_bound(..., fast=True) -- no allowance on top"""
    run(capi, form, *shape_of(form), fast=True)


# ---- bf16 rows out ----------------------------------------------------------------------------------------------------------------------------------------------
BF16_FORMS = {False: F("none", 8, 1, 8, "a16 wt"), True: F("none", 8, 1, 8, "ln wt al")}


@pytest.mark.parametrize("M,N,K,epi,ln", R.BF16_ROWS_CASES, ids=[f"{e}-{'ln' if l else 'a16'}" for _, _, _, e, l in R.BF16_ROWS_CASES])
def test_bf16_rows_out(capi, M, N, K, epi, ln):
    """bf16 rows in, bf16 rows out (the qkv product) and fp32 rows through a folded norm (fc1): out is bf16(want) wherever want is farther than delta from a
    rounding boundary; odd ldo; the elements between the rows and behind them hold the fill."""
    k = R.bf16_rows_case(M, N, K, epi, ln)
    form = (epi,) + BF16_FORMS[ln][1:]
    for ldo in (N, N + 3):
        got = capi.diag_gemm_smallm_bf16(k["A"], k["W"], bias=k["bias"], epi=epi, a16=not ln, ln=k["ln"], fast_act=epi == "silu", out_bf16=True, ldo=ldo,
                                         out_words=slack_words(M, ldo, True))
        assert got["form"] == form
        el = R.words_to_bf16(got["out"])
        off = R.output_offsets(M, N, ldo)
        worst, share = R.check_bf16_rows(el[off], k["p"]["want"], k["delta"])
        print(f"{label(form)} bf16 rows ldo={ldo}: worst |err| / bound = {worst:.3f}, excused {100 * share:.2f} %")
        assert share <= 0.02
        fill16_outside(el, off, f"{label(form)} ldo={ldo}")
        WORST[label(form) + "-bf16rows"] = max(WORST.get(label(form) + "-bf16rows", 0.0), worst)


# ---- the conv tail -------------------------------------------------------------------------------------------------------------------------------------------------
DW_CASES = [(F("glu", 8, 1, 8, "ln wt dw al"), c, S, hc) for c, S in ((1, 7), (2, 5), (4, 3)) for hc in (False, True)]
DW_CASES += [(F("glu", 8, 1, 16, "ln wt dw al"), 2, 13, True), (F("glu", 8, 1, 16, "wt dw al"), 4, 5, False), (F("glu", 8, 1, 8, "a16 dw"), 1, 11, True)]


@pytest.mark.parametrize("form,c,S,has_cache", DW_CASES, ids=[f"{label(f)}-c{c}-S{S}-{'cache' if h else 'first'}" for f, c, S, h in DW_CASES])
def test_conv_tail(capi, form, c, S, has_cache):
    """c = 1 / 2 / 4 frames per stream, the first chunk (zero left padding) and a later one, stream counts whose rows end inside a tile, spare streams behind
    cache_out; the GLU rows the fused launch leaves in the cache are bit for bit the output of the same product without the tail."""
    N, K = (3072, 256) if form[3] == 16 else (272, 512)
    _, got = run(capi, form, c * S, N, K, c, has_cache=has_cache, spare_streams=2, fast=True)
    glu, _ = run(capi, without(form, "dw"), c * S, N, K, fast=True)
    assert np.array_equal(got["cache_out"].reshape(S + 2, 8, N)[:S, 8 - c:].reshape(c * S, N), glu.view(np.uint32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(M=129, N=256, K=256), dict(M=8, N=256, K=320), dict(M=8, N=256, K=256, ldw=260), dict(M=8, N=256, K=256, lda=258),
           dict(M=8, N=256, K=256, epi="resid", out_bf16=True), dict(M=8, N=256, K=256, epi="glu", out_bf16=True),
           dict(M=9, N=256, K=256, out_bf16=True, out_t8=True), dict(M=8, N=272, K=256, out_bf16=True, out_t8=True), dict(M=8, N=256, K=256, out_t8=True),
           dict(M=8, N=256, K=256, epi="silu", a16=True, a_t8=True), dict(M=9, N=256, K=256, epi="resid", a16=True, a_t8=True),
           dict(M=8, N=256, K=256, epi="resid", a_t8=True),                                                       # gemm_smallm_bf16_applies
           dict(M=8, N=256, K=2304, ln=True), dict(M=8, N=256, K=2048, epi="glu", ln=True), dict(M=8, N=256, K=512, a16=True, ln=True),   # ..._ln_applies
           dict(M=8, N=240, K=512, epi="silu", pre=True), dict(M=8, N=256, K=512, epi="relu", pre=True), dict(M=8, N=256, K=512, epi="silu", pre=True, pre_ldo=514),
           dict(M=8, N=256, K=512, epi="silu", pre=True, pre_ldo=508, pre_out_words=8 * 512),                      # ..._pre_applies
           dict(M=9, N=256, K=256, epi="glu", dw_c=3), dict(M=10, N=256, K=256, epi="glu", dw_c=4), dict(M=8, N=264, K=256, epi="glu", dw_c=2),
           dict(M=8, N=256, K=256, epi="silu", dw_c=2)]                                                            # ..._dw_applies


def test_refusals(capi):
    """What the four predicates refuse comes back as PK_ERR_UNSUPPORTED from the form query and from the launching entry, which writes nothing."""
    for kw in REFUSED:
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm_bf16_form(**kw)
        assert e.value.code == PK_ERR_UNSUPPORTED, kw
    o = ops(8, 256, 512, False)
    conv = dict(c=3, has_cache=True, cache_in=np.zeros((3, 8, 256), np.float32), **ops(8, 256, 512, True)["conv"])
    for kw in (dict(epi="silu", a16=True, a_t8=True), dict(epi="relu", ln=o["ln"], pre=o["pre"]), dict(ln=o["ln"], a16=True), dict(out_t8=True),
               dict(epi="glu", dw=conv)):
        left = dict(fill=0x5A5A5A5A)
        W = ops(8, 256, 512, True)["W"] if kw.get("epi") == "glu" else o["W"]
        with pytest.raises(capi.PkError) as e:
            capi.diag_gemm_smallm_bf16(o["A"], W, **kw, into=left)
        assert e.value.code == PK_ERR_UNSUPPORTED, kw
        assert left["args"].form == -1, kw
        for name in ("out", "pre_out", "cache_out"):
            assert left[name] is None or np.all(left[name] == 0x5A5A5A5A), f"{kw}: a refused call wrote {name}"
    with pytest.raises(capi.PkError) as e:                           # ... and the tile diagnostic names this one for the family's shapes
        capi.diag_gemm_bf16_tile_form(64, 260, 256)
    assert e.value.code == PK_ERR_UNSUPPORTED and "pk_diag_gemm_smallm_bf16" in str(e.value)
