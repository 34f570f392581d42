"""The relative-position attention kernels alone (pk_diag_relpos_attention) against the float64 reference of tests/attention_ref.py.

Every case checks each element of ctx against its derived bound (and the mean against the mean bound), that every valid element was written
and that none of the guard rows past the last valid row was touched; `variant` shows which instantiation ran (LDS / global scratch, uniform /
ragged).  Inputs are exactly representable in bf16.  Prints max(err / bound) and mean(err) / mean(sigma) per case (-s)."""
import numpy as np
import pytest

import attention_ref as ar
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

SCRATCH, RAGGED, BF16 = 1, 2, 4
# kernels/attention.hip relpos_attention_max_frames(hd): the longest sequence whose [32][T] score block fits the LDS of a CU
MAX_FRAMES = {32: 1168, 64: 1104, 96: 1040, 128: 1104}


def _bf16_cases():
    Ts = [1, 2, 31, 32, 33, 126, 127, 128, 129, 255, 256, 257, 376, 1000]
    heads = [(64, 1), (64, 2), (64, 8), (64, 9), (128, 1), (128, 3), (128, 8)]
    cases = []
    for n, T in enumerate(Ts):                      # every T with every family; head shapes, batch and table length rotate through their values
        for fi, fam in enumerate(ar.FAMILIES):
            hd, H = heads[(5 * n + fi) % len(heads)]
            B = (1, 3)[(n + fi) % 2]
            pos_T = (T, T + 1, T + 97, 2 * T + 5)[(n + 2 * fi) % 4]
            cases.append(("bf16", fam, hd, H, B, None, T, pos_T, 160 if T >= 1000 else None))
    for fam, hd in (("random", 64), ("key", 64), ("large", 128)):   # one long sequence at small H
        cases.append(("bf16", fam, hd, 1, 1, None, 3000, 3097, 96))
    mix = [26, 376, 100, 251, 63, 188, 313, 38]     # 2 .. 30 s of audio in one packed batch
    cases += [("bf16", "key", 64, 2, 1, [1, 129, 33, 376, 128], None, 376, None),
              ("bf16", "pos", 128, 3, 1, [1, 129, 33, 376, 128], None, 400, None),
              ("bf16", "random", 64, 9, 1, [257, 2, 2, 2, 2, 2], None, 257, None),
              ("bf16", "c", 128, 1, 1, [257, 2, 2, 2, 2, 2], None, 300, None),
              ("bf16", "random", 64, 8, 1, mix, None, 401, 96),
              ("bf16", "large", 64, 8, 1, mix, None, 380, 96)]
    return cases


def _fp32_cases():
    cases = []
    heads = {32: 4, 64: 2, 96: 2, 128: 2}
    for hi, hd in enumerate(sorted(heads)):
        for n, T in enumerate((1, 33, 126, 301)):
            fam = ar.FAMILIES[(hi + 2 * n) % len(ar.FAMILIES)]
            B = (1, 3)[(hi + n) % 2]
            pos_T = (T, T + 1, T + 97, 2 * T + 5)[(hi + n) % 4]
            cases.append(("fp32", fam, hd, heads[hd], B, None, T, pos_T, None))
        m = MAX_FRAMES[hd]
        cases.append(("fp32", ar.FAMILIES[hi], hd, 1, 1, None, m, m, 96))                       # the longest LDS score block
        cases.append(("fp32", ar.FAMILIES[hi + 1], hd, 1, 1, None, m + 1, m + 9, 96))           # the first scratch one
    cases.append(("fp32", "key", 64, 1, 1, None, 2000, 2000, 96))
    cases.append(("fp32", "pos", 128, 1, 1, None, 1999, 2100, 96))
    cases.append(("fp32", "random", 128, 2, 1, [1, 129, 33, 376, 128], None, 400, None))
    cases.append(("fp32", "c", 64, 2, 1, [1200, 33, 300, 2, 2], None, 1300, 64))                   # one clip past the LDS limit: ragged + scratch
    # hd 64, uniform: the two ends of the lengths whose block form runs the 32-row V chunk (one more resident workgroup than the 64-row chunk
    # allows), and the first length of the three-workgroups-per-CU build
    for n, T in enumerate((133, 200, 201)):
        cases.append(("fp32", ("large", "random", "pos")[n], 64, 2, 2, None, T, (T, T + 5, T)[n], None))
    return cases


CASES = _bf16_cases() + _fp32_cases()


def _id(c):
    kind, fam, hd, H, B, lens, T, pos_T, _ = c
    shape = f"lens{'-'.join(map(str, lens))}" if lens else f"B{B}xT{T}"
    return f"{kind}-{fam}-hd{hd}-H{H}-{shape}-posT{pos_T}"


def _expected_variant(kind, hd, lens, T):
    t_max = max(lens) if lens else T
    v = (BF16 if kind == "bf16" else 0) | (RAGGED if lens else 0)
    if kind == "fp32" and t_max > MAX_FRAMES[hd]:
        v |= SCRATCH
    return v


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_relpos_attention_vs_float64(case):
    kind, fam, hd, H, B, lens, T, pos_T, max_rows = case
    d = hd * H
    ln = list(lens) if lens else [T] * B
    seed = 1000 + CASES.index(case)
    qkv, pos, bu, bv = ar.make_inputs(fam, ln, d, H, pos_T, seed)
    got, variant = capi.diag_relpos_attention(kind, qkv, pos, bu, bv, H, B=B, lens=lens)
    assert variant == _expected_variant(kind, hd, lens, T), f"variant {variant}, expected {_expected_variant(kind, hd, lens, T)}"
    ref = ar.reference(kind, qkv, pos, bu, bv, H, B=B, lens=lens, max_rows=max_rows)
    worst, mean = ar.check(kind, got, ref, H, qkv.shape[0], _id(case))
    print(f"\n{_id(case):>58}  variant {variant}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")
