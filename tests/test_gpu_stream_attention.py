"""The cached attention of the streaming encoder alone (kernels/stream.hip through pk_diag_stream_attention: one launch per case and ctx layout),
in every launch form -- the general kernel with one and two wavefronts, the LDS-tile kernel at head size 64 and 128 -- and with the cache
rotation that rides on the same launch.

Every case (tests/stream_attention_ref.py CASES) asserts, for both layouts of ctx (natural columns and the sigma layout):
  * the form the library reports (the function the launcher switches on) is the one the case was written for;
  * attention_ref.check against the float64 definition: every element inside its bound, the mean inside the mean bound, every element
    written, no guard row touched, all finite;
  * ctx is bit-equal to the specification composed from the oracle's primitives;
  * the new K and V caches are bit-equal to the last min(keep_max, kv) rows of [cache ; chunk], and every other word of the two cache
    outputs (the rows keep .. cache_rows - 1 of every stream, the guard rows) still holds the unwritten pattern.
The cache rows past nc and the table rows below P - kv hold NaN: a clamped or over-read value that reached a result would show.
Prints max(err / bound) and mean(err) / mean(sigma) per case (-s)."""
import numpy as np
import pytest

import attention_ref as ar
import gpu_common as G
import oracle as orc
import stream_attention_ref as sr
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

PK_ERR_INVALID = -1


def _launch(case, inp, ctx_sigma, **kw):
    a = dict(qkv_new=inp["qkv"], kcache=inp["kcache"], vcache=inp["vcache"], nc=case.nc, pos=inp["pos"], bias_u=inp["bias_u"],
             bias_v=inp["bias_v"], n_heads=case.H, left=case.left, right=case.right, keep_max=case.keep_max, ctx_sigma=ctx_sigma)
    a.update(kw)
    return capi.diag_stream_attention(**a)


@pytest.mark.parametrize("case", sr.CASES, ids=[c.name for c in sr.CASES])
def test_stream_attention_alone(case):
    inp = sr.make_inputs(case, 500 + sr.CASES.index(case))
    rows = case.S * case.c
    want, ref = sr.spec_bits(orc, case, inp), sr.definition(case, inp)
    want_k, want_v = sr.expected_cache(case, inp, 1), sr.expected_cache(case, inp, 2)
    for sg in (0, 1):
        what = f"{case.name} ctx_sigma {sg}"
        ctx, ko, vo, form = _launch(case, inp, sg)
        assert form == case.form, f"{what}: launched as {form}, the case was written for {case.form}"
        nat = sr.natural_columns(ctx, sg)
        worst, mean = ar.check("fp32", nat, ref, case.H, rows, what)
        print(f"\n{case.name:>32} {case.family:>6} sigma {sg}  {form:>11}  max err/bound {worst:.4f}  mean err/sigma {mean:.4f}", end="")
        G.assert_bits_equal(nat[:rows], want, f"{what}: ctx against the specification")
        for got, exp, name in ((ko, want_k, "K"), (vo, want_v, "V")):
            bad = np.argwhere(got.view(np.uint32) != exp)
            assert bad.size == 0, (f"{what}: new {name} cache, buffer row {bad[0][0]} (of {case.cache_rows} per stream, keep {min(case.keep_max, case.nc + case.c)}) "
                                   f"column {bad[0][1]}: {got.view(np.uint32)[tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x} ({bad.shape[0]} words)")


def test_stream_attention_without_rotation_leaves_the_caches_alone():
    case = next(c for c in sr.CASES if c.name == "rotate-hd64-steady")
    inp = sr.make_inputs(case, 1)
    ctx, ko, vo, form = _launch(case, inp, 0, rotate=False)
    assert form == case.form
    G.assert_bits_equal(ctx[:case.S * case.c], sr.spec_bits(orc, case, inp), "ctx without the rotation")
    assert np.all(ko.view(np.uint32) == sr.UNWRITTEN) and np.all(vo.view(np.uint32) == sr.UNWRITTEN)


def _status(fn):
    try:
        fn()
    except capi.PkError as e:
        return e.code
    return 0


def test_stream_attention_rejections():
    """what the launcher cannot take is refused before anything is staged or launched"""
    case = next(c for c in sr.CASES if c.name == "rotate-hd32-steady")          # S 3, c 2, nc 10, cache_rows 10, P 23
    inp = sr.make_inputs(case, 2)
    assert _status(lambda: _launch(case, inp, 0)) == 0
    assert _status(lambda: _launch(case, inp, 0, nc=case.cache_rows + 1)) == PK_ERR_INVALID                      # nc > cache_rows
    assert _status(lambda: _launch(case, inp, 0, pos=inp["pos"][:case.nc + case.c - 1])) == PK_ERR_INVALID        # P < nc + c
    assert _status(lambda: _launch(case, inp, 0, pos=inp["pos"][-(case.nc + case.c):])) == 0                        # P == nc + c
    assert _status(lambda: _launch(case, inp, 0, qkv_new=inp["qkv"][:, :0])) == PK_ERR_INVALID                    # c == 0
    assert _status(lambda: _launch(case, inp, 0, keep_max=case.cache_rows + 1)) == PK_ERR_INVALID                 # a new cache longer than its buffer
    odd = sr._mk("odd", "random", "general-1w", 20, 2, 1, 3, 3, 0)                                                # d = 40: no sigma layout
    assert _status(lambda: _launch(odd, sr.make_inputs(odd, 3), 1)) == PK_ERR_INVALID
    assert _status(lambda: _launch(odd, sr.make_inputs(odd, 3), 0)) == 0
