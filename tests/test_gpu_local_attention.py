"""The limited-context (band) attention kernel alone (pk_diag_relpos_local_attention).

Covering windows (left, right >= T - 1): the ctx must be bit-equal to the full fp32 kernel (pk_diag_relpos_attention kernel 0) fed the
matching window of the table.  Banded windows: every element against the float64 band reference (tests/local_attention_ref.py) through the
existing checker (attention_ref.check: per-element bound, mean bound, guard rows untouched, every element written).  `variant` is asserted
for every case.  Prints max(err / bound) and mean(err) / mean(sigma) per case (-s)."""
import numpy as np
import pytest

import attention_ref as ar
import local_attention_ref as lr
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

RAGGED, BAND, BF16_OUT = 2, 8, 16
# kernels/attention.hip relpos_local_attention_max_span(hd): the widest left + right whose [32][left + right + 32] score block fits LDS
MAX_SPAN = {32: 1136, 64: 1072, 96: 1008, 128: 1072}
PK_ERR_INVALID, PK_ERR_UNSUPPORTED = -1, -7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


COVER = [  # (hd, H, B, lens, T, left, right)
    (32, 4, 2, None, 70, 69, 69), (64, 2, 3, None, 33, 32, 40), (96, 2, 1, None, 300, 299, 299), (128, 2, 2, None, 126, 125, 200),
    (64, 8, 1, None, 1, 0, 0), (64, 2, 1, [1, 129, 33, 200, 128], None, 199, 199), (128, 3, 1, [257, 2, 31, 64], None, 256, 300),
    (32, 2, 1, [5, 77, 300], None, 299, 299), (96, 1, 1, [40, 41], None, 40, 45),
]


@pytest.mark.parametrize("case", COVER, ids=[f"hd{c[0]}-H{c[1]}-{'lens' + '-'.join(map(str, c[3])) if c[3] else f'B{c[2]}xT{c[4]}'}-L{c[5]}R{c[6]}" for c in COVER])
def test_covering_window_bit_equal_to_full_kernel(case):
    hd, H, B, lens, T, left, right = case
    d = hd * H
    ln = list(lens) if lens else [T] * B
    t_max = max(ln)
    fam = ar.FAMILIES[COVER.index(case) % len(ar.FAMILIES)]
    qkv, pos, bu, bv = ar.make_inputs(fam, ln, d, H, t_max, 500 + COVER.index(case))
    full, vf = capi.diag_relpos_attention("fp32", qkv, pos, bu, bv, H, B=B, lens=lens)
    loc, vl = capi.diag_relpos_local_attention(qkv, lr.local_table(pos, t_max, left, right), bu, bv, H, left, right, B=B, lens=lens)
    assert vf == (RAGGED if lens else 0)
    assert vl == BAND | (RAGGED if lens else 0)
    g, w = _bits(loc), _bits(full)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{len(bad)} elements differ from the full kernel; first at {tuple(bad[0])}: {loc[tuple(bad[0])]!r} vs {full[tuple(bad[0])]!r}"


def test_covering_window_bit_equal_to_forced_block_form():
    """at T <= 128 the full kernel above is the strip form by default: the band form is also pinned to the BLOCK form it is an instantiation of"""
    hd, H, T, left, right = 64, 2, 65, 64, 64
    qkv, pos, bu, bv = ar.make_inputs("random", [T], hd * H, H, T, 600)
    block, ran = capi.diag_relpos_attention_form("block", qkv, pos, bu, bv, H, B=1)
    loc, vl = capi.diag_relpos_local_attention(qkv, lr.local_table(pos, T, left, right), bu, bv, H, left, right, B=1)
    assert ran == "block" and vl == BAND
    bad = np.argwhere(_bits(loc) != _bits(block))
    assert bad.size == 0, f"{len(bad)} elements differ from the block form; first at {tuple(bad[0])}"


def _cases():
    cases = []   # (family, hd, H, B, lens, T, left, right, out_mode, max_rows)
    windows = [(0, 0), (1, 0), (0, 1), (16, 16), (31, 33), (70, 13), (128, 128), (256, 256)]
    Ts = [1, 2, 31, 33, 100, 300, 1000, 3000]
    heads = [(64, 2), (128, 2), (32, 4), (96, 1), (64, 8), (128, 1)]
    n = 0
    for wi, (l, r) in enumerate(windows):
        for ti, T in enumerate(Ts):
            if (wi + ti) % 2:                        # every other (window, T): each window meets short and long sequences
                continue
            fam = ar.FAMILIES[n % len(ar.FAMILIES)]
            hd, H = heads[n % len(heads)]
            B = (1, 2)[n % 2] if T < 1000 else 1
            cases.append((fam, hd, H, B, None, T, l, r, n % 3 == 2 and 1 or 0, 96 if T >= 1000 else None))
            n += 1
    for fi, fam in enumerate(ar.FAMILIES):           # every family on (128, 128) at a mid length, both output modes
        cases.append((fam, 64, 2, 1, None, 700, 128, 128, fi % 2, 128))
    for hi, hd in enumerate(sorted(MAX_SPAN)):       # the widest accepted window per head size
        s = MAX_SPAN[hd]
        cases.append((ar.FAMILIES[hi], hd, 1, 1, None, 2500, s // 2, s - s // 2, hi % 2, 96))
    cases.append(("key", 64, 2, 1, None, 20000, 64, 64, 0, 64))            # a long sequence, rows sampled
    cases.append(("random", 128, 1, 1, None, 20500, 256, 256, 1, 48))
    mix = [1, 129, 33, 700, 128, 2, 300]             # ragged: utterances shorter and longer than the window
    cases += [("key", 64, 2, 1, mix, None, 128, 128, 0, None), ("pos", 128, 2, 1, mix, None, 70, 13, 1, None),
              ("c", 32, 4, 1, [257, 2, 2, 31, 64], None, 16, 16, 0, None), ("large", 96, 1, 1, [1000, 40, 3], None, 256, 256, 1, 96),
              ("random", 64, 8, 1, [3000, 1, 500], None, 0, 1, 0, 96)]
    return cases


CASES = _cases()


def _id(c):
    fam, hd, H, B, lens, T, l, r, mode, _ = c
    shape = f"lens{'-'.join(map(str, lens))}" if lens else f"B{B}xT{T}"
    return f"{fam}-hd{hd}-H{H}-{shape}-L{l}R{r}-out{mode}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_band_attention_vs_float64(case):
    fam, hd, H, B, lens, T, left, right, mode, max_rows = case
    d = hd * H
    ln = list(lens) if lens else [T] * B
    qkv, pl, bu, bv = lr.make_inputs(fam, ln, d, H, left, right, 2000 + CASES.index(case))
    got, variant = capi.diag_relpos_local_attention(qkv, pl, bu, bv, H, left, right, B=B, lens=lens, out_mode=mode)
    assert variant == BAND | (RAGGED if lens else 0) | (BF16_OUT if mode else 0), f"variant {variant}"
    ref = lr.reference(qkv, pl, bu, bv, H, left, right, B=B, lens=lens, max_rows=max_rows, out_mode=mode)
    worst, mean = ar.check("bf16" if mode else "fp32", got, ref, H, qkv.shape[0], _id(case))
    print(f"\n{_id(case):>58}  variant {variant}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")


def _status(fn):
    try:
        fn()
    except capi.PkError as e:
        return e.code
    return 0


@pytest.mark.parametrize("hd", sorted(MAX_SPAN))
def test_refusals(hd):
    d, H, T = hd * 2, 2, 64
    qkv, pos, bu, bv = ar.make_inputs("random", [T], d, H, T, 7)
    s = MAX_SPAN[hd]
    wide = np.zeros((s + 2, d), np.float32)
    assert _status(lambda: capi.diag_relpos_local_attention(qkv, wide, bu, bv, H, s // 2 + 1, s - s // 2)) == PK_ERR_UNSUPPORTED
    ok = np.zeros((s + 1, d), np.float32)
    assert _status(lambda: capi.diag_relpos_local_attention(qkv, ok, bu, bv, H, s // 2, s - s // 2)) == 0
    one = np.zeros((1, d), np.float32)
    for l, r in ((-1, 5), (5, -1), (-2, -2), (-1, -1)):
        assert _status(lambda: capi.diag_relpos_local_attention(qkv, one, bu, bv, H, l, r)) == PK_ERR_INVALID, (l, r)
