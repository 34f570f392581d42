"""GPU: pk_transcribe_pcm_vad on the synthetic model of the input-rate test.  The call cuts every clip at its pauses and
transcribes the pieces as ordinary clips, so it must answer, field for field and every float to the bit, what this test assembles itself:
pk_transcribe_pcm on the returned pieces given as separate clips, merged per clip by the rule of the header (tests/vad_ref.py: merge)."""
import numpy as np
import pytest

import vad_ref as V
from conftest import pk
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu

VAD = dict(max_piece_s=2.0)


def bits(x):
    """x with every float replaced by its fp32 bit pattern, so that == on the result compares to the bit."""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(bits(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return ("f32", int(np.float32(x).view(np.uint32)))
    return x


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    td = tmp_path_factory.mktemp("transcribe_vad")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    yield gm
    gm.close()


@pytest.fixture(scope="module")
def clips():
    sr = 16000
    silent = np.zeros(5 * sr, np.float32)
    n = 12 * sr + 700                                                     # bursts with pauses, the last one running to the very end
    a = synth.synth_pcm(1, n, seed=71)[0]
    for s, e in ((0.0, 0.9), (2.1, 2.6), (2.75, 2.9), (4.4, 6.0), (7.2, 7.25), (9.0, 10.5)):
        a[int(s * sr):int(e * sr)] = 0.0
    b = synth.synth_pcm(1, 10 * sr, seed=72)[0]                           # one burst of 7 s: longer than max_piece_s = 2
    b[:int(1.3 * sr)] = 0.0
    b[int(8.3 * sr):] = 0.0
    return [silent, a, b]


@pytest.fixture(scope="module")
def plain(model, clips):
    """a plain call before the VAD calls; test_plain_calls_are_unchanged repeats it after them"""
    return bits(model.transcribe_pcm(clips[1:], decoder="tdt", timestamps=True))


def expected_pieces(clips):
    out = []
    for i, c in enumerate(clips):
        runs, e = V.vad(c, **VAD)
        out += [(i, b, t) for b, t in V.plan(c.size, runs, e, **VAD)]
    return out


@pytest.mark.parametrize("decoder", ["ctc", "tdt"])
@pytest.mark.parametrize("timestamps", [False, True])
def test_vad_route_is_the_plain_call_on_the_pieces(model, clips, plain, decoder, timestamps):
    got, pieces = model.transcribe_pcm(clips, decoder=decoder, timestamps=timestamps, vad=VAD)
    assert pieces == expected_pieces(clips)
    per_clip = [[p for p in pieces if p[0] == i] for i in range(3)]
    assert per_clip[0] == [] and len(per_clip[1]) >= 3 and len(per_clip[2]) >= 4
    assert per_clip[1][-1][2] == clips[1].size                            # the last piece ends with the clip, not on the frame grid
    assert all(b % 1280 == 0 and 256 < t - b <= 2 * 16000 for _, b, t in pieces)
    parts = model.transcribe_pcm([clips[c][b:t] for c, b, t in pieces], decoder=decoder, timestamps=timestamps)
    want = V.merge(parts, pieces, len(clips), timestamps)
    assert bits(got) == bits(want)
    assert got[0]["text"] == "" and got[0]["token_ids"] == [] and (not timestamps or got[0]["words"] == [])
    assert sum(len(g["token_ids"]) for g in got[1:]) > 0
    if timestamps:
        assert any(g["words"] for g in got[1:])
        for g in got[1:]:
            assert g["start"] == sorted(g["start"]) and len(g["start"]) == len(g["end"]) == len(g["conf"]) == len(g["token_ids"])


def test_plain_calls_are_unchanged(model, clips, plain):
    model.transcribe_pcm(clips, vad=True)
    assert bits(model.transcribe_pcm(clips[1:], decoder="tdt", timestamps=True)) == plain


def test_another_input_rate_is_refused(model, clips):
    model.set_input_rate(48000)
    try:
        with pytest.raises(capi.PkError) as e:
            model.transcribe_pcm(clips, vad=True)
        assert e.value.code == -7
    finally:
        model.set_input_rate(16000)
    with pytest.raises(capi.PkError) as e:
        model.transcribe_pcm(clips, vad=dict(max_piece_s=0.1))
    assert e.value.code == -1
