"""The device resampler's specification against the host resampler, on the CPU: pk_resample_table is the table
tests/resample_ref.py builds with Python's math functions, bit for bit; the walk of resample_ref over that table reproduces pk_resample exactly
when one rate divides the other and within one fp32 rounding at a few samples otherwise; pk_resample_length is the host's output length.
No device is needed: the kernel is compared with resample_ref in tests/test_gpu_resample.py."""
import numpy as np
import pytest

import resample_ref as R
from parakeet_cpp_amd import capi

TABLE_RATES = [(48000, 16000), (44100, 16000), (8000, 16000), (11025, 16000), (16000, 8000)]
INTEGER = [(48000, 16000), (8000, 16000), (16000, 8000), (32000, 16000), (96000, 16000)]
FRACTIONAL = [(44100, 16000), (22050, 16000), (11025, 16000)]
SHORT = (1, 31, 32, 33, 1000)
_tables = {}


def lib_table(src, dst):
    if (src, dst) not in _tables:
        _tables[src, dst] = capi.resample_table(src, dst)
    return _tables[src, dst]


def clip(n, seed=7):
    return (np.random.default_rng(seed).standard_normal(n) * 0.1).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("src,dst", TABLE_RATES)
def test_table_is_the_python_table_bit_for_bit(src, dst):
    T, up, down = lib_table(src, dst)
    assert (up, down) == R.up_down(src, dst) and T.shape == (up, 32)
    assert np.array_equal(T.view(np.uint64), R.table(src, dst).view(np.uint64))


def test_table_refusals_and_sizes():
    for src, dst in ((3999, 16000), (384001, 16000), (16000, 3999), (16000, 384001)):
        with pytest.raises(capi.PkError) as e:
            capi.resample_table(src, dst)
        assert e.value.code == -7
        assert capi.lib().pk_resample_length(100, src, dst) == -1 and capi.resample_run(src, dst) == 0
    T, up, down = capi.resample_table(15999, 16000)
    assert (up, down) == (16000, 15999) and T.shape == (16000, 32)
    # the kernel's run: a multiple of 32 up to 1024 whose input span fits the 5632 floats staged per workgroup
    for src in (4000, 8000, 11025, 15999, 16000, 44100, 48000, 96000, 384000):
        for dst in (4000, 16000, 384000):
            run = capi.resample_run(src, dst)
            u, d = R.up_down(src, dst)
            assert 32 <= run <= 1024 and run % 32 == 0 and run * d // u + 34 <= 5632


@pytest.mark.parametrize("src,dst", INTEGER)
def test_walk_is_pk_resample_for_integer_ratios(src, dst):
    T = lib_table(src, dst)[0] if (src, dst) in TABLE_RATES else None
    for n in (10 * src,) + SHORT:
        x = clip(n)
        assert np.array_equal(bits(R.walk(x, src, dst, T)), bits(capi.resample(x, src, dst))), (src, dst, n)


@pytest.mark.parametrize("src,dst", FRACTIONAL)
def test_walk_is_pk_resample_within_one_rounding_for_fractional_ratios(src, dst):
    """pk_resample rounds i * src / dst to a double before it takes the tap distances; the table takes them from the exact fraction.  The weights
    differ by about 1e-10 relative, which now and then flips the fp32 rounding of an output: a difference is at most one fp32 ulp at the clip's peak plus
    the fp64 perturbation itself (1e-8 of the peak), and the share of such samples in 10 s is capped at 2e-3 (measured: profiles/resample.md)."""
    T = lib_table(src, dst)[0] if (src, dst) in TABLE_RATES else None
    for n in (10 * src,) + SHORT:
        x = clip(n)
        a, b = R.walk(x, src, dst, T), capi.resample(x, src, dst)
        assert a.shape == b.shape
        peak = float(np.max(np.abs(b))) if b.size else 0.0
        delta = np.abs(a.astype(np.float64) - b.astype(np.float64))
        differ = int(np.count_nonzero(bits(a) != bits(b)))
        print(f"{src} -> {dst}, n = {n}: {differ} of {a.size} samples differ, max |delta| = {delta.max() if a.size else 0.0:.3e}, peak = {peak:.4f}")
        assert np.all(delta <= float(np.spacing(np.float32(peak))) + 1e-8 * peak), (src, dst, n)
        if n == 10 * src:
            assert differ <= 2e-3 * a.size, (src, dst, differ)


def test_walk_centre_is_the_hosts_centre():
    """floor((double)i / (dst / src)) of the host loop is the integer centre i * down // up at every output of 10 s (what makes the two forms comparable)."""
    for src, dst in FRACTIONAL + INTEGER:
        up, down = R.up_down(src, dst)
        i = np.arange(R.out_len(10 * src, src, dst), dtype=np.int64)
        host = np.floor(i.astype(np.float64) / (float(dst) / float(src))).astype(np.int64)
        assert np.array_equal(host, i * down // up), (src, dst)


@pytest.mark.parametrize("src,dst", TABLE_RATES + [(22050, 16000)])
def test_length_is_the_hosts_output_length(src, dst):
    zeros = np.zeros(2000, np.float32)
    for n in range(0, 2001):
        assert capi.resample_length(n, src, dst) == R.out_len(n, src, dst) == capi.resample(zeros[:n], src, dst).size, n
    assert capi.resample_length(2 ** 31 - 1, src, dst) == R.out_len(2 ** 31 - 1, src, dst)
    with pytest.raises(capi.PkError) as e:
        capi.resample_length(2 ** 31, src, dst)
    assert e.value.code == -7
