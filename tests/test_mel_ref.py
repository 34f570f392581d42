"""CPU: the float64 specification of the mel front end (tests/mel_ref.py) against the oracle, on every case tests/test_gpu_mel_forms.py runs on the
device.  The oracle's front end -- offline and streaming -- stays inside the derived fp32 bound with no element excused (the check that the
bound is sound), and every wrong variant of the specification leaves it on a named case (the check that the bound can tell).

Every check prints its max err / bound (pytest -s); python tests/mel_ref.py prints the worst per input family.  The normalise bound is finite at
every element (mel_ref.normalize_bound asserts it), so no element is excused there either."""
import dataclasses

import numpy as np
import pytest

import mel_ref as R
from conftest import pk
from parakeet_cpp_amd import synth


@pytest.mark.parametrize("c", R.UNIFORM_CASES, ids=R.uniform_id)
def test_oracle_offline_inside_the_bound(orc, c):
    for k, x in enumerate(R.uniform_clips(c)):
        ref, bound = R.ref_of(x, c[3], c[5], c[6])
        feats, lm = orc.mel(x, n_mels=c[3], return_logmel=True, normalize=bool(c[4]), window_centered=bool(c[5]), power_via_abs=bool(c[6]))
        assert lm.shape == ref.shape == (c[3], c[0])
        R.check_logmel(lm, ref, bound, f"{R.uniform_id(c)} clip {k}")
        R.check_features(feats, lm, c[4], f"{R.uniform_id(c)} clip {k}")
        if c[7] == "zeros" and c[4]:
            assert not feats.any()


@pytest.mark.parametrize("c", R.RAGGED_CASES, ids=R.ragged_id)
def test_oracle_on_the_ragged_clips_inside_the_bound(orc, c):
    for k, x in enumerate(R.ragged_clips(c)):
        ref, bound = R.ref_of(x, c[1])
        feats, lm = orc.mel(x, n_mels=c[1], return_logmel=True, normalize=bool(c[2]))
        assert lm.shape == (c[1], c[0][k])
        R.check_logmel(lm, ref, bound, f"{R.ragged_id(c)} clip {k} ({R.ragged_families(c)[k]})")
        R.check_features(feats, lm, c[2], f"{R.ragged_id(c)} clip {k}")
        if R.ragged_families(c)[k] == "zeros" and c[2]:
            assert not feats.any()


@pytest.fixture(scope="module")
def stream_oracles(orc):
    """one oracle model per bin count: the oracle's streaming front end hangs on a model"""
    out = {}
    for n_mels in (80, 128):
        cfg = dataclasses.replace(pk.make_tiny_config(), mel_bins=n_mels, name=f"tiny-mel{n_mels}")
        out[n_mels] = orc.Model(cfg, synth.synth_weights(cfg, seed=42))
    return out


@pytest.mark.parametrize("c", R.STREAM_CASES, ids=R.stream_id)
def test_oracle_streaming_inside_the_bound(orc, stream_oracles, c):
    raw, pre = R.stream_clips(c)
    for k in range(c[2]):
        got = orc.Stream(stream_oracles[c[3]]).mel(raw[k])           # a fresh session's first chunk: pre-emphasis from a carried 0
        ref, bound = R.stream_logmel(pre[k], c[3])
        assert got.shape == ref.shape == (c[0], c[3])
        R.check_logmel(got, ref, bound, f"{R.stream_id(c)} session {k}")


def test_every_form_sees_every_family():
    assert {c[7] for c in R.UNIFORM_CASES} == set(R.FAMILIES)
    assert {f for c in R.RAGGED_CASES for f in R.ragged_families(c)} == set(R.FAMILIES)
    assert {c[4] for c in R.STREAM_CASES} == set(R.FAMILIES)
    assert {c[0] for c in R.UNIFORM_CASES} == {2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129}
    assert {x.size for c in R.UNIFORM_CASES if c[0] == 2 for x in R.uniform_clips(c)} == {257, 319}
    assert all(x.size >= 257 for c in R.RAGGED_CASES for x in R.ragged_clips(c))


# the case on which each wrong variant is shown to leave the bound (by its id in UNIFORM_CASES)
MUTANT_CASE = {
    "reflect_left": "nf31-r159-B1-m128-norm1-ctr0-abs1-imp0",         # the impulse at sample 0 is mirrored a sample off
    "reflect_right": "nf32-r0-B3-m40-norm0-ctr0-abs1-impN",           # ... the impulse at sample n - 1
    "preemph_after_pad": "nf63-r97-B1-m128-norm1-ctr0-abs1-tone",     # the mirrored samples take the wrong neighbour
    "window_shift": "nf33-r1-B1-m65-norm0-ctr0-abs1-tail",
    "hop159": "nf128-r1-B3-m40-norm1-ctr0-abs1-tail",                 # 127 samples of drift by the last frame
    "biased_variance": "nf2-r97-B1-m80-norm1-ctr0-abs1-noise",        # sqrt 2 at two frames
    "y0": "nf16-r1-B3-m65-norm1-ctr0-abs1-const",                     # 0.5 against 0.015 at sample 0
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_leaves_the_bound(mutant):
    c = {R.uniform_id(c): c for c in R.UNIFORM_CASES}[MUTANT_CASE[mutant]]
    x = R.uniform_clips(c)[0]
    ref, bound = R.ref_of(x, c[3], c[5], c[6])
    if mutant == "biased_variance":
        lm = ref.astype(np.float32)
        q, at = R.ratio(R.normalize(lm, biased=True), R.normalize(lm), R.normalize_bound(lm))
    else:
        q, at = R.ratio(R.logmel(x, c[3], bool(c[5]), bool(c[6]), mutant=mutant)[0], ref, bound)
    print(f"{mutant} on {MUTANT_CASE[mutant]}: max err / bound {q:.1f} at {at}")
    assert q > 1.0


def test_reference_pieces():
    """what the derivation leans on: the filterbank's triangles have area 1 in Hz, the window is symmetric with zero ends, the band lengths are the
    counts the bound uses, and the fp32 pre-emphasis of a chunk is the float64 one within its two roundings"""
    for n_mels in (40, 65, 80, 128):
        fb = R.filterbank(n_mels)
        assert fb.shape == (257, n_mels) and fb.min() >= 0
        K = R.band_lengths(n_mels)
        assert K.max() <= 257 and K.sum() <= 768                    # (kMelMaxTaps of the kernel: every bin count of the cases fits)
    w = R.hann_window()
    assert w[0] == 0 and abs(w[399]) < 1e-30 and np.allclose(w[:400], w[:400][::-1], atol=1e-15) and not w[400:].any()
    assert np.array_equal(R.hann_window(True)[56:456], w[:400])
    x = R.make_clip("noise", 700, 1)
    y = R.preemphasize_f32(x)
    d, a = R.offline_frames(x)
    assert y[0] == x[0] and np.all(np.abs(y[1:] - (x[1:].astype(np.float64) - 0.97 * x[:-1])) <= 3 * R.U * (np.abs(x[1:]) + np.abs(x[:-1])))
    assert d.shape == (5, 512) and d[0, 256] == x[0] and a[0, 256] == 0 and d[0, 255] == d[0, 257]
