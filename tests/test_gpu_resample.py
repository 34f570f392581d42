"""GPU: the resampling kernel (kernels/resample.hip, pk_resample_device) against its specification tests/resample_ref.py, bit for bit.

One packed batch per pair of rates with clips of 0, 1, 31, 32, 33, R - 1, R, R + 1 and 3 R + 7 input samples, R being what one workgroup's run
of outputs spans in input samples (pk_resample_run * down / up): empty and one-sample clips, clips shorter than the 32 taps, a clip that ends one
sample before, at and after a workgroup's boundary, and one of several workgroups with a ragged tail.  Every clip's output lies in a buffer
filled with a sentinel, with a gap before, between and after the outputs: the gaps come back untouched (no write outside an extent), and a clip's
result is the reference's result for that clip alone (no read across clips)."""
import numpy as np
import pytest

import resample_ref as R
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-77.25)
GAP = 5
# 48 k: one table row, downsampling; 8 k: upsampling; 44.1 k: 160 rows, the largest table kept in LDS; 11.025 k: 640 rows from global memory;
# 15 999: 16 000 rows (4 MB) from global memory
RATES = [(48000, 16000), (8000, 16000), (44100, 16000), (11025, 16000), (15999, 16000), (16000, 16000)]


def clip_lengths(src, dst):
    up, down = R.up_down(src, dst)
    run = capi.resample_run(src, dst)
    assert run > 0
    span = run * down // up
    lens = [0, 1, 31, 32, 33, span - 1, span, span + 1, 3 * span + 7]
    if (src, dst) == (15999, 16000):
        lens = [min(n, 2000) for n in lens[:-1]] + [2000]          # clips of at most 2000 samples at the 16 000-row table
    return lens


@pytest.mark.parametrize("src,dst", RATES)
def test_device_is_the_reference_bit_for_bit(src, dst):
    lens = clip_lengths(src, dst)
    rng = np.random.default_rng(11)
    clips = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in lens]
    T = capi.resample_table(src, dst)[0]                            # (pinned against resample_ref.table in tests/test_resample_ref.py)
    want = [R.walk(c, src, dst, T) for c in clips]
    out_lens = [capi.resample_length(n, src, dst) for n in lens]
    assert out_lens == [w.size for w in want]
    off = np.zeros(len(clips) + 1, np.int64)
    off[0] = GAP
    for i, m in enumerate(out_lens):
        off[i + 1] = off[i] + m + GAP
    buf = np.full(int(off[-1]), SENTINEL, np.float32)
    got = capi.resample_device(clips, src, dst, out=buf, out_offsets=off)
    inside = np.zeros(got.size, bool)
    for i, w in enumerate(want):
        a = got[off[i]: off[i] + out_lens[i]]
        inside[off[i]: off[i] + out_lens[i]] = True
        bad = np.flatnonzero(a.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, f"{src} -> {dst}: clip {i} ({lens[i]} samples) differs at {bad[:5]}: {a[bad[:5]]} vs {w[bad[:5]]}"
    assert np.all(got[~inside] == SENTINEL), f"{src} -> {dst}: written outside the clips' extents at {np.flatnonzero((got != SENTINEL) & ~inside)[:8]}"
    assert np.count_nonzero(~inside) == GAP * (len(clips) + 1)
    # the plain form (outputs back to back) gives the same clips
    for a, w in zip(capi.resample_device(clips, src, dst), want):
        assert np.array_equal(a.view(np.uint32), w.view(np.uint32))


def test_refusals():
    x = [np.zeros(100, np.float32)]
    for src, dst in ((3999, 16000), (384001, 16000), (16000, 3999)):
        with pytest.raises(capi.PkError) as e:
            capi.resample_device(x, src, dst)
        assert e.value.code == -7
    import ctypes as C
    L = capi.lib()
    off = np.array([0, 100], np.int64)
    ooff = np.array([0, 34], np.int64)
    out = np.zeros(34, np.float32)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pk_resample_device(0, None, i64(off), 1, 48000, 16000, f32(out), i64(ooff)) == -1
    assert L.pk_resample_device(0, f32(x[0]), None, 1, 48000, 16000, f32(out), i64(ooff)) == -1
    assert L.pk_resample_device(0, f32(x[0]), i64(off), 1, 48000, 16000, None, i64(ooff)) == -1
    assert L.pk_resample_device(0, f32(x[0]), i64(off), 1, 48000, 16000, f32(out), None) == -1
    ooff[1] = 33                                                    # one sample too little room for the clip's 34 outputs
    assert L.pk_resample_device(0, f32(x[0]), i64(off), 1, 48000, 16000, f32(out), i64(ooff)) == -1
    assert np.all(out == 0)
