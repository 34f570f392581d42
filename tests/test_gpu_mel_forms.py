"""GPU: the mel front end kernels alone (kernels/mel.hip through pk_diag_mel), in every launch form -- offline uniform, offline ragged, streaming --
at the frame counts where a 16-frame workgroup, a 64-frame normalise tile or a 4-frame streaming workgroup is exactly full, one short and one over,
at bin counts that are no multiple of 16 and just above 64, on inputs that put their energy at a clip's edges.

Per case: the log-mel within the derived fp32 bound of the float64 specification (tests/mel_ref.py) at every valid element; log-mel and features
bit-identical to the oracle; the features within the normalise bound of the float64 statistics of the log-mel the device returned; every pad
column, every spare word and (through the same mask) every word outside a clip's own block still the fill; the grid and the frame counts the case
names.  The cases and their references are mel_ref's, shared with tests/test_mel_ref.py, which holds the oracle to the same bound on the CPU."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
import mel_ref as R
from conftest import pk
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu

FILL = np.uint32(capi.MEL_FILL)


def assert_fill(buf, free, what):
    bad = np.flatnonzero(buf.view(np.uint32)[free] != FILL)
    assert bad.size == 0, f"{what}: {bad.size} words outside the valid region were written, first at {np.flatnonzero(free)[bad[:8]]}"


def check_clip(lm, ft, x, n_mels, normalize, centered, pabs, orc, what):
    """one clip's log-mel [n_mels][frames] and features [frames][n_mels] against the specification and the oracle"""
    ref, bound = R.ref_of(x, n_mels, centered, pabs)
    R.check_logmel(lm, ref, bound, what)
    of, ol = orc.mel(x, n_mels=n_mels, return_logmel=True, normalize=bool(normalize), window_centered=bool(centered), power_via_abs=bool(pabs))
    G.assert_bits_equal(lm, ol, f"{what}: log-mel against the oracle")
    G.assert_bits_equal(ft, of, f"{what}: features against the oracle")
    R.check_features(ft, lm, normalize, what)


@pytest.mark.parametrize("c", R.UNIFORM_CASES, ids=R.uniform_id)
def test_offline_uniform(orc, c):
    nf, r, B, n_mels, normalize, centered, pabs, family = c
    clips = R.uniform_clips(c)
    lm_buf, ft_buf, frames, grid = capi.diag_mel(clips, "uniform", n_mels, normalize, centered, pabs)
    assert list(frames) == [nf] * B
    assert grid == ((-(-nf // 16), B, 1024), (-(-n_mels // 16), B, 1024))
    assert lm_buf.size == B * n_mels * capi.mel_logmel_pitch(nf) + 64 and ft_buf.size == B * nf * n_mels + 64
    lms, fts, lm_free, ft_free = R.split_offline(lm_buf, ft_buf, n_mels, [nf] * B)
    assert_fill(lm_buf, lm_free, "log-mel buffer")
    assert_fill(ft_buf, ft_free, "feature buffer")
    assert lm_free.sum() == B * n_mels * (capi.mel_logmel_pitch(nf) - nf) + 64 and ft_free.sum() == 64
    for k in range(B):
        check_clip(lms[k], fts[k], clips[k], n_mels, normalize, centered, pabs, orc, f"{R.uniform_id(c)} clip {k}")
        if family == "zeros" and normalize:
            assert not fts[k].any(), "silence must normalise to exact zeros"


@pytest.mark.parametrize("c", R.RAGGED_CASES, ids=R.ragged_id)
def test_offline_ragged(orc, c):
    nfs, n_mels, normalize, _ = c
    clips = R.ragged_clips(c)
    lm_buf, ft_buf, frames, grid = capi.diag_mel(clips, "ragged", n_mels, normalize)
    assert list(frames) == list(nfs)
    assert grid == ((-(-max(nfs) // 16), len(nfs), 1024), (-(-n_mels // 16), len(nfs), 1024))     # (the grid covers the longest clip)
    lms, fts, lm_free, ft_free = R.split_offline(lm_buf, ft_buf, n_mels, nfs)
    assert lm_buf.size == n_mels * sum(capi.mel_logmel_pitch(t) for t in nfs) + 64 and ft_buf.size == n_mels * sum(nfs) + 64
    assert_fill(lm_buf, lm_free, "log-mel buffer")
    assert_fill(ft_buf, ft_free, "feature buffer")
    for k, x in enumerate(clips):
        what = f"{R.ragged_id(c)} clip {k} ({R.ragged_families(c)[k]}, {nfs[k]} frames)"
        check_clip(lms[k], fts[k], x, n_mels, normalize, False, True, orc, what)
        if R.ragged_families(c)[k] == "zeros" and normalize:
            assert not fts[k].any(), "silence must normalise to exact zeros"
        alone = capi.diag_mel(x, "uniform", n_mels, normalize)
        a_lm, a_ft, _, _ = R.split_offline(alone[0], alone[1], n_mels, [nfs[k]])
        G.assert_bits_equal(lms[k], a_lm[0], f"{what}: log-mel against the clip alone")
        G.assert_bits_equal(fts[k], a_ft[0], f"{what}: features against the clip alone")


@pytest.fixture(scope="module")
def stream_oracles(orc):
    out = {}
    for n_mels in (80, 128):
        cfg = dataclasses.replace(pk.make_tiny_config(), mel_bins=n_mels, name=f"tiny-mel{n_mels}")
        out[n_mels] = orc.Model(cfg, synth.synth_weights(cfg, seed=42))
    return out


@pytest.mark.parametrize("c", R.STREAM_CASES, ids=R.stream_id)
def test_streaming(orc, stream_oracles, c):
    nf, r, S, n_mels, family = c
    raw, pre = R.stream_clips(c)
    lm_buf, ft_buf, frames, grid = capi.diag_mel(pre, "stream", n_mels)
    assert list(frames) == [nf] * S
    assert grid == ((-(-nf // 4), S, 256), (0, 0, 0))
    assert lm_buf.size == S * nf * n_mels + 64 and ft_buf.size == 64
    assert np.all(lm_buf.view(np.uint32)[S * nf * n_mels:] == FILL), "spare words behind the log-mel were written"
    assert np.all(ft_buf.view(np.uint32) == FILL), "the streaming form has no feature launch"
    got = lm_buf[: S * nf * n_mels].reshape(S, nf, n_mels)
    for k in range(S):
        ref, bound = R.stream_logmel(pre[k], n_mels)
        R.check_logmel(got[k], ref, bound, f"{R.stream_id(c)} session {k}")
        G.assert_bits_equal(got[k], orc.Stream(stream_oracles[n_mels]).mel(raw[k]), f"{R.stream_id(c)} session {k}: against the oracle's first chunk")


# ---- wiring: the entry points that launch the front end for real give the bits of the diagnostic ----------------------------------------------
@pytest.fixture(scope="module")
def tiny_gpu(tmp_path_factory):
    cfg = pk.make_tiny_config()
    p = tmp_path_factory.mktemp("w") / "tiny.safetensors"
    synth.save_weights(str(p), synth.synth_weights(cfg, seed=42))
    gm = capi.Model(str(p), cfg, device=0)
    yield gm
    gm.close()


def test_model_mel_is_the_diagnostic(tiny_gpu):
    c = R.UNIFORM_CASES[9]                                          # 64 frames, 3 clips, 80 bins
    assert c[:4] == (64, 159, 3, 80) and tiny_gpu.cfg.mel_bins == 80
    clips = R.uniform_clips(c)
    feats, lm = tiny_gpu.mel(clips, return_logmel=True)
    lms, fts, _, _ = R.split_offline(*capi.diag_mel(clips, "uniform", 80, True)[:2], 80, [64] * 3)
    G.assert_bits_equal(lm, np.stack(lms), "Model.mel log-mel")
    G.assert_bits_equal(feats, np.stack(fts), "Model.mel features")


def test_model_mel_ragged_is_the_diagnostic(tiny_gpu):
    c = R.RAGGED_CASES[0]
    assert c[1] == 80
    clips = R.ragged_clips(c)
    got = tiny_gpu.mel_ragged(list(clips))
    _, fts, _, _ = R.split_offline(*capi.diag_mel(clips, "ragged", 80, True)[:2], 80, c[0])
    for k in range(len(clips)):
        G.assert_bits_equal(got[k], fts[k], f"Model.mel_ragged clip {k}")


def test_frontend_is_the_diagnostic():
    c = R.UNIFORM_CASES[1]                                          # 2 frames of 319 samples, 128 bins, not normalised
    assert c[3] == 128 and not c[4]
    fe = capi.Frontend(n_mels=128, normalize=False)
    for x in R.uniform_clips(c):
        _, fts, _, _ = R.split_offline(*capi.diag_mel(x, "uniform", 128, False)[:2], 128, [2])
        G.assert_bits_equal(fe.features(x), fts[0], "Frontend.features")
    fe.close()


def test_session_mel_is_the_diagnostic(tiny_gpu):
    c = R.STREAM_CASES[5]                                           # 4 frames + 159 samples, 3 sessions, 80 bins
    assert c[:4] == (4, 159, 3, 80)
    raw, pre = R.stream_clips(c)                                    # pre: the chunk pre-emphasised as a fresh session does, from a carried 0
    gs = capi.Stream(tiny_gpu, 3)
    got = gs.mel(raw)
    gs.close()
    lm_buf = capi.diag_mel(pre, "stream", 80)[0]
    G.assert_bits_equal(got, lm_buf[: 3 * 4 * 80].reshape(3, 4, 80), "Stream.mel, first chunk")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,pcm", [("uniform", np.zeros((1, 256), np.float32)),
                                      ("ragged", [np.zeros(400, np.float32), np.zeros(256, np.float32), np.zeros(700, np.float32)]),
                                      ("stream", np.zeros((2, 399), np.float32))], ids=["256-samples", "ragged-with-256", "399-streaming"])
def test_refusals_leave_the_buffers_alone(form, pcm):
    lm, ft = np.full(4096, -77.25, np.float32), np.full(4096, -77.25, np.float32)
    with pytest.raises(capi.PkError) as e:
        capi.diag_mel(pcm, form, 80, logmel=lm, feats=ft)
    assert e.value.code == -1
    assert np.all(lm == np.float32(-77.25)) and np.all(ft == np.float32(-77.25))
