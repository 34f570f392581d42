"""CPU checks of tests/bf16_gemm_ref.py, the reference of tests/test_gpu_bf16_tile_gemm.py: the host bf16 rounding against torch.bfloat16 on random bit
patterns and on the ties, the blocked layout against a brute-force index loop, the bf16 neighbours, and the share of elements the bf16-rows rule excuses on
the operands the GPU module uses (counted from the float64 reference alone, and by perturbing it by +- delta)."""
import numpy as np
import pytest
import torch

import bf16_gemm_ref as R


def torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_rounding_matches_torch_on_random_bit_patterns_and_ties():
    rng = np.random.default_rng(1)
    u = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 1 << 16, 4096, dtype=np.uint64).astype(np.uint32) << 16
    ties = np.concatenate([hi | 0x8000, hi | 0x7FFF, hi | 0x8001, hi])                  # exactly half way (both parities of the kept bit), just below, just above, exact
    u = np.concatenate([u, ties, np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0x00000001, 0x807FFFFF], np.uint32)])
    x = u.view(np.float32)
    finite = np.isfinite(x)
    got, want = R.bf16_bits(x), torch_bf16_bits(x)
    assert np.array_equal(got[finite], want[finite])
    assert np.all(np.isnan(R.bf16_value(got[np.isnan(x)]))) and np.array_equal(got[np.isinf(x)], want[np.isinf(x)])
    assert R.bf16_bits(np.array([1.00390625], np.float32))[0] == 0x3F80 and R.bf16_bits(np.array([1.01171875], np.float32))[0] == 0x3F82   # ties to even
    y = R.bf16_round(x[finite])
    assert np.array_equal(R.bf16_round(y).view(np.uint32), y.view(np.uint32)), "rounding is idempotent"


@pytest.mark.parametrize("M,N,ld", [(1, 16, 16), (40, 48, 64), (33, 20, 32), (64, 32, 32)])
def test_blocked_layout_against_an_index_loop(M, N, ld):
    off = R.blocked_offsets(M, N, ld)
    Mr = (M + 31) // 32 * 32
    for r in range(M):
        for c in range(N):
            blk = (r // 32) * (ld // 16) + c // 16
            assert off[r, c] == blk * 512 + (r % 32) * 16 + c % 16
    assert len(set(off.reshape(-1))) == M * N and off.max() < Mr * ld
    x = np.arange(M * N, dtype=np.int64).reshape(M, N)
    buf = R.to_blocked(x, ld, -1)
    assert buf.size == Mr * ld and np.array_equal(R.from_blocked(buf, M, N, ld), x) and (buf == -1).sum() == Mr * ld - M * N
    if M >= 32 and N >= 16:                                          # one block is 32 rows x 16 columns, row-major, contiguous
        assert np.array_equal(buf[:512].reshape(32, 16), x[:32, :16])


def test_bf16_neighbours_bracket_and_round():
    rng = np.random.default_rng(2)
    w = np.concatenate([rng.standard_normal(100000) * 2.0 ** rng.integers(-10, 10, 100000), [1.0, -1.0, 0.5, 1.00390625, -3.0, 0.0]])
    lo, hi, mid = R.bf16_neighbours(w)
    assert np.all(lo <= w) and np.all(w <= hi)
    for v in (lo, hi):
        assert np.array_equal(R.bf16_round(v.astype(np.float32)).astype(np.float64), v), "both neighbours are bf16 values"
    exact = R.bf16_round(w.astype(np.float32)).astype(np.float64)
    assert np.all((exact == lo) | (exact == hi))
    inner = (np.abs(w - mid) > 1e-7 * np.abs(w)) & (lo != hi)
    assert np.array_equal(exact[inner], np.where(w < mid, lo, hi)[inner])
    assert np.all(hi - lo <= np.abs(w) * 2.0 ** -7 + (w == 0)), "adjacent bf16 values: an ulp is at most 2^-7 of the value"


def test_sigma_and_pitch_placement_is_the_small_m_reference():
    off = R.output_offsets(3, 32, 40, 16)
    assert off[1, 1] == 40 + 4 and off[2, 17] == 80 + 17 and np.array_equal(R.to_sigma(np.arange(16)), [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15])


@pytest.mark.parametrize("epi,fast", [("none", False), ("relu", False), ("silu", False), ("silu", True)])
def test_excused_share_of_the_coherent_operands_stays_under_the_cap(epi, fast):
    """The bf16-rows rule of check_bf16_rows on the reference alone: the share within delta of a rounding boundary, and the flips of bf16(want +- delta)."""
    M, N, K = 1030, 260, 128
    A, W = R.coherent_operands(np.random.default_rng(M * 7 + N * 3 + K), M, N, K)
    b = (0.01 * np.random.default_rng(4).standard_normal(N)).astype(np.float32)
    p = R.product(A, W, b, epi)
    delta = R.out_bound(p, epi, fast)
    share = R.excused_share(p["want"], delta)
    nz = p["want"] != 0                                                # (a ReLU's zeros are exact: the pre-activations of these operands are far from 0)
    flips = np.mean((R.bf16_bits((p["want"] + delta).astype(np.float32)) != R.bf16_bits((p["want"] - delta).astype(np.float32))) & nz)
    print(f"{epi} fast={fast}: excused {100 * share:.2f} %, flips under +- delta {100 * flips:.2f} %")
    assert flips <= share + 1e-3 and share <= 0.02
    err = np.abs(R.bf16_round(p["want"].astype(np.float32)).astype(np.float64) - p["want"])
    assert np.any(err > 2.0 ** -9 * np.abs(p["want"]) + delta) or epi != "none", "the unit roundoff of bf16 is 2^-8: correct rounding alone exceeds 2^-9 |want|"
    # the reference, rounded, passes its own check; an element moved to the wrong side of a boundary it is far from does not
    bits = R.bf16_bits(p["want"].astype(np.float32))
    R.check_bf16_rows(bits, p["want"], delta)
    far = np.argmax(np.abs(p["want"] - R.bf16_neighbours(p["want"])[2]) - 4 * delta)
    bits.reshape(-1)[far] += 1
    with pytest.raises(AssertionError):
        R.check_bf16_rows(bits, p["want"], delta)


def test_bounds_are_the_stated_ones():
    z = np.array([-12.0, -1.0, 0.0, 3.0])
    assert np.allclose(R.fast_sigmoid_rel(z), (4 + np.abs(z)) * 2.0 ** -23) and np.all(np.abs(R.silu_slope(np.linspace(-30, 30, 6001))) <= 1.1)
    p = dict(z=z, want=z * R.sigmoid64(z), mag=np.full(4, 10.0), g=None, mag_g=None)
    d = R.acc_bound(p["mag"])
    assert np.allclose(d, 2.1e-5) and np.all(R.out_bound(p, "silu", True) <= 1.1 * d + 0.5 * d * d + ((4 + np.abs(z)) * 2.0 ** -23 + 2.0 ** -24) * np.abs(p["want"]))
    assert np.array_equal(R.out_bound(p, "resid", False, 512, True, np.full(4, 2.0)), d + 6e-8 * 32 * 2.0)
