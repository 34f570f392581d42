"""CPU self-test of tests/decode_gemv_ref.py, the float64 reference and error bound the GPU test of the decode GEMV kernels
(tests/test_gpu_decode_gemv.py) asserts: before the bound counts as a test, (a) a numpy fp32 emulation of the kernel's arithmetic -- bf16 operands,
fp32 accumulation in blocks of 32 k, the kernel's epilogue order, the oracle's sigmoid / tanh -- stays inside it on every case of the GPU test's
shape list, and (b) every planted fault leaves it on at least one checked element of every case it applies to."""
import numpy as np
import pytest

import decode_gemv_ref as R

IDS = [R.case_id(c) for c in R.CASES]


def _ratios(o, got, ref):
    rows = R.checked_rows(o)
    return {k: R.worst_ratio(got[k][rows], ref[k][0][rows], ref[k][1][rows], ref[k][2]) for k in ref if not (k == "pp" and not o["want_pp"])}


@pytest.fixture(scope="module")
def built(orc):
    """operands and reference of every case, computed once"""
    out = []
    for c in R.CASES:
        o = R.make_case(c)
        out.append((o, R.reference(o, orc.math_v)))
    return out


def test_case_list_covers_every_value_with_every_epilogue_and_all_18_instantiations():
    for epi in ("bias", "act", "cell"):
        cs = [c for c in R.CASES if c["epi"] == epi]
        assert {32, 64, 96, 128, 256, 288, 640, 1024} <= {c["K"] for c in cs}, epi
        assert {1, 15, 16, 17, 32, 63, 64, 65, 130} <= {c["B"] for c in cs}, epi
        cols = {32, 64, 20, 36, 640} if epi == "cell" else {16, 70, 128, 1030}
        assert cols <= {c["N"] for c in cs}, epi
    assert {2048, 2100} <= {c["B"] for c in R.CASES} and 8198 in {c["N"] for c in R.CASES}
    assert {"all", "none", "row0", "last", "alt", "tile", "random", None} == {c["need"] for c in R.CASES}
    assert len({R.instantiation(c) for c in R.CASES}) == 18
    assert len(set(IDS)) == len(IDS)
    for c in R.CASES:
        o = R.make_case(c)
        f = o["need_flags"]
        if c["need"] == "random":
            assert f.sum() % 16 != 0 and 0 < f.sum() < c["B"]
        if c["need"] == "tile":
            assert all(f[t0: t0 + 16].sum() == 1 for t0 in range(0, c["B"], 16))
        if c["epi"] == "cell" and not o["fused"]:
            r = o["gi_row"]
            if c["B"] >= 3:
                assert np.any(np.diff(r) < 0) and (c["B"] <= 11 or len(set(r.tolist())) < len(r))
        if c["epi"] == "act":
            rows = R.checked_rows(o)
            if rows.size >= 5:
                assert (o["t"][rows] == 0).any() and (o["t"][rows] == o["Tb_eff"][rows] - 1).any() and (o["t"][rows] >= o["Tb_eff"][rows]).any()
    cells = [R.make_case(c) for c in R.CASES if c["epi"] == "cell"]
    assert any(o["fused"] for o in cells) and any(not o["fused"] for o in cells)
    acts = [R.make_case(c) for c in R.CASES if c["epi"] == "act"]
    for key in ("bias", "Tb"):
        assert any(o[key] is None for o in acts) and any(o[key] is not None for o in acts)
    assert any(o["want_pp"] for o in acts) and any(not o["want_pp"] for o in acts)


def test_device_math_constant_against_float64(orc):
    """E_FN bounds |F - f| of the sigmoid / tanh the kernels evaluate (the oracle's math_v, bit for bit the device functions)"""
    x = np.concatenate([np.linspace(-20, 20, 400001), np.linspace(-0.6, 0.6, 100001)]).astype(np.float32)
    x64 = x.astype(np.float64)
    assert np.abs(orc.math_v("sigmoid", x) - 1.0 / (1.0 + np.exp(-x64))).max() <= R.E_FN
    assert np.abs(orc.math_v("tanh", x) - np.tanh(x64)).max() <= R.E_FN


def test_emulated_kernel_stays_inside_the_bound(built, orc):
    worst = {}
    for o, ref in built:
        for k, r in _ratios(o, R.emulate(o, orc.math_v), ref).items():
            worst[(o["epi"], k)] = max(worst.get((o["epi"], k), 0.0), r)
            assert r <= 1.0, (R.case_id(o), k, r)
    print("worst emulated err / allowed:", {f"{a}.{b}": round(v, 4) for (a, b), v in worst.items()})
    assert all(v > 0 for v in worst.values()), "degenerate: the emulation equals the reference"


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_leaves_the_bound(built, orc, fault):
    n = 0
    for o, ref in built:
        if not R.fault_applies(fault, o):
            continue
        r = _ratios(o, R.emulate(o, orc.math_v, fault=fault), ref)
        assert max(r.values()) > 1.0, (fault, R.case_id(o), r)
        n += 1
    assert n >= 3, f"{fault}: applied to {n} cases only"


def test_bf16_admissibility_is_the_rounding_of_a_value_inside_the_bound():
    """a bf16 output is admissible exactly when it is the RNE rounding of some value inside ref +- bound: the rounding of every such value passes,
    the bf16 value two steps past the rounding of the interval's end does not"""
    rng = np.random.default_rng(3)
    n = 20000
    ref = rng.standard_normal(n) * np.exp(rng.uniform(-6, 3, n))
    ref[:100] = 0.0
    bound = (np.abs(ref) + 1e-3) * 10.0 ** rng.uniform(-7, -3, n)
    for s in (-1.0, -0.3, 0.0, 0.6, 1.0):
        v = (ref + s * bound).astype(np.float32)                             # (the fp32 value a kernel would hold, itself rounded once)
        assert R.worst_ratio(R.bf16(v), ref, bound + np.abs(v - (ref + s * bound)), True) <= 1.0
    for sgn in (-1, 1):
        end = (ref + sgn * bound).astype(np.float32)
        bits = R.bf16_bits(end)
        away = np.where((end > 0) == (sgn > 0), bits + 2, bits - 2).astype(np.uint16)      # two bf16 steps further out than the end's rounding
        ok = (bits & 0x7FFF) > 2
        got = R.bf16_widen(away)
        assert np.all((R.excess(got, ref, True) > bound)[ok])
