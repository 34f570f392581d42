"""GPU: the one-call entry points on PCM at another rate than 16 kHz (pk_model_set_input_rate / pk_group_set_input_rate).

With the input rate set, pcm and offsets count input-rate samples and every batch is resampled on the device on its way in.  Everything behind
the resampler sees 16 kHz samples, so each call must answer, field for field and every float to the bit, what the same call at rate 16000
answers on the resampled clips: pk_resample's output at 48 kHz (the device is bit-identical to it for integer ratios) and pk_resample_device's
at 44.1 kHz.  Both ingestion sites are covered: pk_transcribe_pcm (and the group) go through the two-stream pipeline, the n-best search, the
alignment and the keyword spotting through the batch loop."""
import numpy as np
import pytest

from conftest import pk
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu

SECONDS = (0.3, 1.2, 0.75, 0.5, 1.0)
ONE = [3]


def bits(x):
    """x with every float replaced by its fp32 bit pattern, so that == on the result compares scores to the bit."""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(bits(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return ("f32", int(np.float32(x).view(np.uint32)))
    return x


def clips_at(rate):
    return [synth.synth_pcm(1, int(round(s * rate)), seed=40 + i, sr=rate)[0] for i, s in enumerate(SECONDS)]


def every_call(gm, clips):
    ids = [ONE] * len(clips)
    return bits(dict(tdt=gm.transcribe_pcm(clips, decoder="tdt", timestamps=True), ctc=gm.transcribe_pcm(clips, decoder="ctc", timestamps=True),
                     nbest=gm.transcribe_nbest(clips, 4, 16, 2, timestamps=True), align=gm.align(clips, ids=ids),
                     spot=gm.spot(clips, ids=[ONE, [5, 7]], max_hits=2)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    td = tmp_path_factory.mktemp("input_rate")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    assert gm.input_rate() == 16000
    yield gm, wp, vp, cfg
    gm.close()


def test_48k_route_is_the_16k_call_on_pk_resample(model):
    gm = model[0]
    raw = clips_at(48000)
    down = [capi.resample(c, 48000, 16000) for c in raw]
    want = every_call(gm, down)
    gm.set_input_rate(48000)
    try:
        assert gm.input_rate() == 48000
        got = every_call(gm, raw)
    finally:
        gm.set_input_rate(16000)
    for k in want:
        assert got[k] == want[k], k


def test_44k_route_is_the_16k_call_on_pk_resample_device(model):
    gm = model[0]
    raw = clips_at(44100)
    down = capi.resample_device(raw, 44100, 16000)
    want = every_call(gm, down)
    gm.set_input_rate(44100)
    try:
        got = every_call(gm, raw)
    finally:
        gm.set_input_rate(16000)
    for k in want:
        assert got[k] == want[k], k


def test_default_rate_is_the_plain_path_and_a_bad_rate_changes_nothing(model):
    gm = model[0]
    clips = clips_at(16000)
    want = every_call(gm, clips)
    gm.set_input_rate(8000)
    for bad in (3999, 384001, 0, -16000):
        with pytest.raises(capi.PkError) as e:
            gm.set_input_rate(bad)
        assert e.value.code == -7 and gm.input_rate() == 8000
    up = bits(gm.transcribe_pcm([capi.resample(c, 16000, 8000) for c in clips], timestamps=True))     # 8 kHz in: upsampled on the device
    assert len(up) == len(clips)
    gm.set_input_rate(16000)
    assert gm.input_rate() == 16000
    assert every_call(gm, clips) == want


def test_group_takes_input_rate_pcm(model):
    gm, wp, vp, cfg = model
    raw = clips_at(48000)
    want = bits(gm.transcribe_pcm([capi.resample(c, 48000, 16000) for c in raw], timestamps=True))
    grp = capi.Group(wp, cfg, vocab_path=vp, devices=[0, 0])
    try:
        with pytest.raises(capi.PkError) as e:
            grp.set_input_rate(3999)
        assert e.value.code == -7
        grp.set_input_rate(48000)
        got = bits(grp.transcribe_pcm(raw, timestamps=True))
        assert abs(grp.last_stats()["audio_seconds"] - sum(SECONDS)) < 1e-3
    finally:
        grp.close()
    assert got == want
