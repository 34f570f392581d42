"""Host: the bf16 TDT spotting lattice entry points (kernels/tdt_kws_bf16.hip) are declared and exported, and pk_diag_tdt_kws_lattice_bf16 refuses
what the kernel does not take before it looks for a device."""
import os
import re

import numpy as np
import pytest

from parakeet_cpp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(J=64, D=4, L=(1, 3)):
    V, n = 20, len(L)
    f = lambda *s: np.zeros(s, np.float32)
    return capi.tdt_kws_lattice_bf16(f(5, J), f((max(L) + 1) * n, J), f(V + D, J), f(V + D), [np.ones(l, np.int32) for l in L], [5] * n, [0] * n,
                                     list(range(n)), n, V, D, V - 1)


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "parakeet_amd.h")).read()
    for name in ("pk_model_set_tdt_kws_bf16", "pk_model_get_tdt_kws_bf16", "pk_diag_tdt_kws_lattice_bf16"):
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(capi.lib(), name) is not None


@pytest.mark.parametrize("kw,codes", [(dict(L=(1, 0)), (-1,)), (dict(L=(65, 2)), (-1, -7)), (dict(J=48), (-1, -7)), (dict(D=9), (-1, -7))],
                         ids=["empty-keyword", "L65", "J48", "D9"])
def test_refusals_come_before_the_device(kw, codes):
    with pytest.raises(capi.PkError) as e:
        call(**kw)
    assert e.value.code in codes, str(e.value)


def test_valid_arguments_need_a_device():
    if capi.device_count() > 0:                                     # (with a device the call runs: tests/test_gpu_tdt_kws_bf16.py holds its values)
        assert all(np.all(x[:-capi.TDT_LATTICE_GUARD] <= 0) for x in call())
        return
    with pytest.raises(capi.PkError) as e:
        call()
    assert e.value.code == -4, str(e.value)
