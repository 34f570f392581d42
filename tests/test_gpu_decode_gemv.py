"""The bf16 decode GEMV kernels alone (kernels/decode_gemv_bf16.hip through pk_diag_skinny_gemm: one launch per case) against the float64 reference
and per-element bound of tests/decode_gemv_ref.py (derivation there; tests/test_decode_gemv_ref.py holds the bound against an emulation and
planted faults on the CPU).

Cases: decode_gemv_ref.CASES.  skinny_gemm_bf16_kernel<EPI, MODE, CHK> instantiation -> the case that runs it (B, columns, K, flags; the same
skeleton for the three epilogues, "cell" with Hp 32 / 20 / 64 / 36 in place of N 16 / 70 / 128 / 1030):
    MODE 1 (flags, B <= 16)   CHK: B 1 N 16 K 32 all; B 15 N 70 K 64 alternating; B 16 N 70 K 64 none      no CHK: B 16 N 128 K 96 random (cell: also B 1 Hp 32)
    MODE 2 (flags, B > 16)    CHK: B 17 N 1030 K 128 last; B 65 N 1030 K 1024 random; B 130 N 16 K 640 row 0   no CHK: B 32 N 128 K 256 one per tile; B 130 N 128 K 32 none
                              (cell: no CHK also B 65 Hp 640 K 640; CHK B 65 Hp 36 K 1024, B 2048 Hp 20; bias: B 17 N 8198, B 2048 N 16)
    MODE 0 (no flags)         CHK: B 63 N 70 K 288 (act: also B 2100 N 16)                                  no CHK: B 64 N 128 K 640 (cell: also B 9 Hp 640 K 96)
test_decode_gemv_ref.py asserts that the list reaches all 18.

Every output buffer is pattern-filled and longer (and, for the bias epilogue, wider) than the batch: rows without a flag, rows past B and columns past N
must come back untouched.

Worst observed max err / bound on the MI355X (pytest -s prints every case), per output over all cases: bias out 0.045, activation pp 0.049, activation
z 0.003, cell c' 0.018, cell h' 0.0006 (z and h' after taking off what their bf16 store explains).  The fp32 kernels (kernels/decode_gemv.hip) are held
bit for bit to the oracle's composition in the last test of this file.
"""
import numpy as np
import pytest

import decode_gemv_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]


def launch(o, bf16=True):
    from parakeet_cpp_amd import capi
    kw = dict(bf16=bf16, need=o["need_flags"])
    if o["epi"] == "bias":
        kw.update(bias=o["bias"])
    elif o["epi"] == "act":
        kw.update(bias=o["bias"], ep=o["ep"], t=o["t"], T=o["T"], Tb=o["Tb"], row0=o["row0"], want_pp=o["want_pp"])
    elif o["fused"]:
        kw.update(c=o["c"], X2=o["X2"], W2=o["W2"], bias2=o["bias2"])
    else:
        kw.update(c=o["c"], gi=o["gi"], gi_row=o["gi_row"])
    return capi.diag_skinny_gemm(o["epi"], o["X"], o["W"], **kw)


def outputs(o, res, bf16=True):
    """name -> (words as returned, fill word, values as float32)"""
    half = bf16 and o["epi"] != "bias"
    d = {"out": (res["out"], R.FILL16 if half else R.FILL32, R.bf16_widen(res["out"]) if half else res["out"].view(np.float32))}
    if res["cn"] is not None:
        d["cn"] = (res["cn"], R.FILL32, res["cn"].view(np.float32))
    if res["pp"] is not None:
        d["pp"] = (res["pp"], R.FILL32, res["pp"].view(np.float32))
    return d


def assert_untouched(o, outs):
    """rows without a flag, the rows past the batch and the columns past N still hold the fill pattern; flagged rows hold none of it"""
    B, N = o["B"], o["N"]
    rows = R.checked_rows(o)
    skipped = np.setdiff1d(np.arange(outs["out"][0].shape[0]), rows)
    for name, (words, fill, _) in outs.items():
        assert words.shape[0] > B
        assert np.all(words[skipped] == fill), f"{name}: {int((words[skipped] != fill).sum())} words written outside the flagged rows"
        assert np.all(words[:, N:] == fill), f"{name}: stores past column {N}"
        assert not np.any(words[rows, :N] == fill), f"{name}: {int((words[rows, :N] == fill).sum())} elements of flagged rows not written"


@pytest.fixture(scope="module")
def math_v(orc):
    return orc.math_v


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_bf16_kernel_against_float64(c, math_v):
    o = R.make_case(c)
    ref = R.reference(o, math_v)
    outs = outputs(o, launch(o))
    assert_untouched(o, outs)
    assert set(outs) == {k for k in ref if not (k == "pp" and not o["want_pp"])}
    rows = R.checked_rows(o)
    for name, (_, _, val) in outs.items():
        want, bound, rounded = ref[name]
        ratio = R.worst_ratio(val[rows, : o["N"]], want[rows], bound[rows], rounded)
        print(f"{R.case_id(c)} {R.instantiation(c)} {name}: max err / bound {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)
    if o["epi"] == "act" and rows.size * o["N"] >= 64:
        z = outs["out"][2][rows]
        assert 0.2 < (z != 0).mean() < 0.8, "degenerate: relu passes (or blocks) nearly everything"
    if o["epi"] == "cell" and rows.size:
        h = np.abs(outs["out"][2][rows])
        assert 0.05 < np.median(h) < 0.9, "degenerate: saturated gates"


@pytest.mark.parametrize("epi", ["bias", "act", "cell"])
def test_bf16_rows_are_independent_of_their_place(epi, math_v):
    """Rows repeating with period 7: every copy of a row carries the same bits, whichever wave, workgroup row or list position it lands in -- with the
    compacted list (random flags), with every row (no flags) and with predicates (B = 16)."""
    cols = 36 if epi == "cell" else 70
    n = 0
    for B, need, K, idx in ((130, "random", 96, 3), (130, None, 640, 4), (16, "all", 64, 5), (65, "alt", 288, 6)):
        o = R.make_case(dict(epi=epi, B=B, N=cols, K=K, need=need, idx=idx), period=7)
        outs = outputs(o, launch(o))
        assert_untouched(o, outs)
        rows = R.checked_rows(o)
        for name, (words, _, _) in outs.items():
            for r in range(7):
                same = rows[rows % 7 == r]
                assert np.all(words[same] == words[same[0]]), (epi, B, need, name, r)
                n += len(same) - 1
    assert n > 100


# ---- the fp32 kernels (kernels/decode_gemv.hip): no tolerance -- bit for bit the oracle's composition ---------------------------------------
# (epi, B, N or Hp, K, flags, idx, F).  K = 16, 48, 80: the runtime K loop with a partial last chunk; 1024: the same loop, 16 chunks; 640: the unrolled instantiation.
FP32_CASES = [("bias", 1, 16, 16, "all", 0, 1), ("bias", 15, 70, 48, "alt", 1, 1), ("bias", 17, 1030, 80, "last", 2, 1), ("bias", 64, 128, 640, None, 3, 1),
              ("bias", 65, 70, 1024, "random", 4, 1), ("bias", 130, 16, 640, "row0", 5, 1), ("bias", 16, 70, 48, "none", 6, 1),
              ("act", 1, 16, 16, "all", 0, 1), ("act", 16, 128, 48, "random", 1, 1), ("act", 32, 64, 80, "tile", 2, 1), ("act", 63, 48, 640, None, 3, 1),
              ("act", 130, 128, 1024, "random", 4, 1), ("act", 8, 64, 640, "all", 5, 2), ("act", 4, 48, 80, "alt", 6, 4), ("act", 2, 128, 16, "all", 7, 8),
              ("act", 130, 32, 48, "none", 8, 1),
              ("cell", 1, 16, 16, "all", 0, 1), ("cell", 15, 32, 48, "alt", 1, 1), ("cell", 17, 48, 80, "last", 2, 1), ("cell", 64, 64, 640, None, 3, 1),
              ("cell", 65, 16, 1024, "random", 4, 1), ("cell", 130, 32, 640, "row0", 5, 1), ("cell", 32, 16, 80, "tile", 7, 1)]


def fp32_expected(o, orc, F):
    """the oracle's composition in the epilogue order of decode_dev.hpp (= pk_oracle.c predict_step / joint_hidden): orc.linear is the natural-k chain"""
    f32 = np.float32
    acc = orc.linear(o["X"], o["W"])
    if o["epi"] == "bias":
        return {"out": acc + o["bias"] if o["bias"] is not None else acc}
    if o["epi"] == "act":
        p = acc + o["bias"] if o["bias"] is not None else acc
        z = np.zeros((o["B"], F, o["N"]), f32)
        for f in range(F):
            tt = np.minimum(o["t"].astype(np.int64) + f, o["Tb_eff"] - 1)
            s = o["ep"][o["row0_eff"] + tt] + p
            z[:, f] = np.where(s > 0, s, f32(0))
        return {"pp": p, "out": z.reshape(o["B"] * F, o["N"])}
    Hp = o["N"]
    gi = orc.linear(o["X2"], o["W2"]) + o["bias2"] if o["fused"] else o["gi"][o["gi_row"], : 4 * Hp]
    g4 = (gi + acc).reshape(o["B"], 4, Hp)
    ig, fg, gg, og = orc.math_v("sigmoid", g4[:, 0]), orc.math_v("sigmoid", g4[:, 1]), orc.math_v("tanh", g4[:, 2]), orc.math_v("sigmoid", g4[:, 3])
    t1, t2 = fg * o["c"], ig * gg
    cn = t1 + t2
    return {"cn": cn, "out": og * orc.math_v("tanh", cn)}


@pytest.mark.parametrize("epi,B,N,K,need,idx,F", FP32_CASES, ids=[f"{c[0]}-B{c[1]}-N{c[2]}-K{c[3]}-{c[4] or 'every'}-F{c[6]}" for c in FP32_CASES])
def test_fp32_kernel_bit_equal_to_the_oracle_composition(orc, epi, B, N, K, need, idx, F):
    from parakeet_cpp_amd import capi
    o = R.make_case(dict(epi=epi, B=B, N=N, K=K, need=need, idx=idx))
    kw = dict(bf16=False, need=o["need_flags"])
    if epi == "bias":
        kw.update(bias=o["bias"])
    elif epi == "act":
        kw.update(bias=o["bias"], ep=o["ep"], t=o["t"], T=o["T"], Tb=o["Tb"], row0=o["row0"], want_pp=o["want_pp"], F=F)
    elif o["fused"]:
        kw.update(c=o["c"], X2=o["X2"], W2=o["W2"], bias2=o["bias2"])
    else:
        kw.update(c=o["c"], gi=o["gi"], gi_row=o["gi_row"])
    res = capi.diag_skinny_gemm(epi, o["X"], o["W"], **kw)
    want = fp32_expected(o, orc, F)
    rows = R.checked_rows(o)
    for name, exp in want.items():
        words = res[name]
        if words is None:
            assert name == "pp" and not o["want_pp"]
            continue
        per = F if name == "out" else 1                        # (z holds F rows per utterance)
        wr = (rows[:, None] * per + np.arange(per)[None, :]).ravel()
        skipped = np.setdiff1d(np.arange(words.shape[0]), wr)
        assert np.all(words[skipped] == R.FILL32) and np.all(words[:, N:] == R.FILL32), f"{name}: stores outside the flagged rows / columns"
        got = words[wr, :N]
        assert not np.any(got == R.FILL32), f"{name}: elements of flagged rows not written"
        bad = got != np.ascontiguousarray(exp, np.float32).view(np.uint32)[wr]
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ from the oracle's composition"
    if epi == "act" and rows.size * N >= 64:
        z = res["out"].view(np.float32)[(rows[:, None] * F + np.arange(F)[None, :]).ravel()]
        assert 0.2 < (z != 0).mean() < 0.8
