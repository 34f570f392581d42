"""The strip form of the fp32 attention kernel (kernels/attention.hip: one wave per 16 query rows, the scores in registers, T <= 128) against
the block form it replaces for short sequences, through pk_diag_relpos_attention_form.

The strip form changes the data flow, not the arithmetic: every case runs both forms on the same inputs and requires ctx -- guard rows
included -- to be byte-identical.  A handful of shapes are also held against the float64 reference of tests/attention_ref.py (every valid
element inside its bound, no guard row touched), and the form selector is checked: shapes the strip form does not cover run the block form
by default and refuse a forced strip launch.

The block form itself is no longer reached by default below 129 frames, so it is held against float64 here too, forced: T in {1, 17, 32, 33,
126} and one ragged batch, hd 64 and 128, with and without the position table, in the three ctx layouts."""
import functools

import numpy as np
import pytest

import attention_ref as ar
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

# tile edges, a strip partly past T, the 64-column wrap of the sum tree, the pad of the AV chain to a multiple of 4
TS = [1, 15, 16, 17, 31, 33, 63, 64, 65, 126, 127, 128]
RAGGED = [[1, 128, 33, 126, 17], [64, 2, 2, 2]]


def _cases():
    cases = []
    for n, T in enumerate(TS):
        for fi, fam in enumerate(("random", "large")):
            hd, H = ((64, 1), (64, 9), (32, 4), (64, 2))[(n + 2 * fi) % 4]      # H = 9: padding slots of the grid
            B = (1, 3)[(n + fi) % 2]
            pos_T = (T, T + 1, T + 97, 2 * T + 5)[(n + fi) % 4]               # the window offset into a longer table
            mode = ("fp32", "sigma", "bf16")[(n + fi) % 3]
            cases.append((fam, hd, H, B, None, T, pos_T, mode))
    for n, T in enumerate((1, 17, 64, 65, 126, 128)):                          # no position table: the scale-only path
        cases.append((("large", "random")[n % 2], (64, 32)[n % 2], (9, 2)[n % 2], (3, 1)[n % 2], None, T, None, ("fp32", "sigma", "bf16")[n % 3]))
    for n, lens in enumerate(RAGGED):
        for fi, fam in enumerate(("random", "large")):
            hd, H = ((64, 9), (32, 4), (64, 2))[(n + fi) % 3]
            cases.append((fam, hd, H, 1, lens, None, max(lens) + (0, 40)[fi], ("fp32", "bf16", "sigma")[(n + fi) % 3]))
    cases.append(("large", 64, 1, 1, RAGGED[0], None, None, "fp32"))          # ragged, no position table
    return cases


CASES = _cases()
REF_CASES = [("random", 64, 2, 3, None, 126, 126), ("large", 64, 9, 1, None, 65, 162), ("key", 32, 4, 1, None, 128, 129),
             ("large", 64, 1, 3, None, 17, 17), ("pos", 64, 2, 1, RAGGED[0], None, 128), ("large", 32, 4, 1, RAGGED[1], None, 70)]


def _id(c):
    fam, hd, H, B, lens, T, pos_T = c[:7]
    shape = f"lens{'-'.join(map(str, lens))}" if lens else f"B{B}xT{T}"
    return f"{fam}-hd{hd}-H{H}-{shape}-posT{pos_T}" + (f"-{c[7]}" if len(c) > 7 else "")


def _inputs(fam, hd, H, B, lens, T, pos_T, seed):
    ln = list(lens) if lens else [T] * B
    qkv, pos, bu, bv = ar.make_inputs(fam, ln, hd * H, H, pos_T if pos_T else max(ln), seed)
    return (qkv, pos, bu, bv) if pos_T else (qkv, None, None, None)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_strip_is_byte_identical_to_block(case):
    fam, hd, H, B, lens, T, pos_T, mode = case
    qkv, pos, bu, bv = _inputs(fam, hd, H, B, lens, T, pos_T, 5000 + CASES.index(case))
    strip, ran_s = capi.diag_relpos_attention_form("strip", qkv, pos, bu, bv, H, B=B, lens=lens, out_mode=mode)
    block, ran_b = capi.diag_relpos_attention_form("block", qkv, pos, bu, bv, H, B=B, lens=lens, out_mode=mode)
    assert (ran_s, ran_b) == ("strip", "block")
    rows = qkv.shape[0]
    unwritten = capi.ATT_UNWRITTEN["bf16" if mode == "bf16" else "fp32"]
    assert not np.any(block[:rows].view(np.uint32) == unwritten), "the block form left valid elements unwritten"
    assert np.all(strip[rows:].view(np.uint32) == unwritten), "the strip form wrote into the guard rows"
    diff = strip.view(np.uint32) != block.view(np.uint32)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} words differ, first at {tuple(np.argwhere(diff)[0])}"


@pytest.mark.parametrize("case", REF_CASES, ids=[_id(c) for c in REF_CASES])
def test_strip_vs_float64(case):
    fam, hd, H, B, lens, T, pos_T = case
    qkv, pos, bu, bv = _inputs(fam, hd, H, B, lens, T, pos_T, 6000 + REF_CASES.index(case))
    got, ran = capi.diag_relpos_attention_form("strip", qkv, pos, bu, bv, H, B=B, lens=lens)
    assert ran == "strip"
    ref = ar.reference("fp32", qkv, pos, bu, bv, H, B=B, lens=lens, max_rows=None)
    worst, mean = ar.check("fp32", got, ref, H, qkv.shape[0], _id(case))
    print(f"\n{_id(case):>50}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")


@pytest.mark.parametrize("hd,H,T,lens", [(64, 2, 129, None), (128, 1, 33, None), (96, 1, 64, None), (64, 1, None, [129, 5])],
                         ids=["T129", "hd128", "hd96", "ragged-129"])
def test_uncovered_shapes_keep_the_block_form(hd, H, T, lens):
    ln = lens if lens else [T]
    qkv, pos, bu, bv = ar.make_inputs("random", ln, hd * H, H, max(ln), 7000)
    _, ran = capi.diag_relpos_attention_form("default", qkv, pos, bu, bv, H, B=1, lens=lens)
    assert ran == "block"
    with pytest.raises(capi.PkError):
        capi.diag_relpos_attention_form("strip", qkv, pos, bu, bv, H, B=1, lens=lens)


# ---- the block form forced below 129 frames, against float64 ------------------------------------------------------------------------------
BLOCK_LENS = [(1,), (17,), (32,), (33,), (126,), (1, 128, 33, 17)]
BLOCK_CASES = [(hd, lens, with_pos, mode) for hd in (64, 128) for lens in BLOCK_LENS for with_pos in (True, False) for mode in ("fp32", "bf16", "sigma")]


@functools.lru_cache(maxsize=None)
def _block_reference(hd, lens, with_pos):
    """inputs and the float64 reference of one shape, shared by its three output layouts.  Without the table the kernel computes
    softmax(q K^T / sqrt(hd)) V: the reference's definition with a zero table and zero biases."""
    H, ln = 2, list(lens)
    n = BLOCK_LENS.index(lens)
    qkv, pos, bu, bv = ar.make_inputs(("random", "large", "key")[(n + hd // 64) % 3], ln, hd * H, H, max(ln) + (0, 3)[n % 2], 8000 + 2 * n + with_pos)
    if not with_pos:
        pos, bu, bv = np.zeros_like(pos), np.zeros_like(bu), np.zeros_like(bv)
    ref = ar.reference("fp32", qkv, pos, bu, bv, H, B=1, lens=ln if len(ln) > 1 else None, max_rows=None)
    vmax = [float(np.abs(qkv[:, 2 * hd * H + h * hd: 2 * hd * H + (h + 1) * hd]).max()) for h in range(H)]
    return qkv, pos, bu, bv, ref, vmax


@pytest.mark.parametrize("case", BLOCK_CASES, ids=[f"hd{c[0]}-lens{'-'.join(map(str, c[1]))}-{'pos' if c[2] else 'nopos'}-{c[3]}" for c in BLOCK_CASES])
def test_forced_block_vs_float64(case):
    hd, lens, with_pos, mode = case
    H = 2
    qkv, pos, bu, bv, ref, vmax = _block_reference(hd, lens, with_pos)
    args = (qkv, pos, bu, bv) if with_pos else (qkv, None, None, None)
    got, ran = capi.diag_relpos_attention_form("block", *args, H, B=1, lens=list(lens) if len(lens) > 1 else None, out_mode=mode)
    assert ran == "block"
    if mode == "sigma":                                                        # the layout is its own inverse: back to natural columns
        got = got[:, capi.sigma16(got.shape[1])]
    if mode == "bf16":
        # the bf16 layout's extra roundings: ctx rounded to bf16 (u16 |ctx|), one hardware reciprocal and a multiplication in place of the
        # division (2^-21 A, A = sum_j p_j |v_jc| <= max |v| of the head); the hardware exp2 is inside the reference's 2^-21 already
        ref = [(rows, h, ctx, bound + ar.U16 * np.abs(ctx) + ar.E_EXP * vmax[h], sigma + ar.U16 / 2 * np.abs(ctx)) for rows, h, ctx, bound, sigma in ref]
    what = f"block hd{hd} lens {lens} {'pos' if with_pos else 'no pos'} {mode}"
    worst, mean = ar.check("bf16" if mode == "bf16" else "fp32", got, ref, H, qkv.shape[0], what)
    print(f"\n{what:>50}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")
