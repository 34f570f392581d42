"""GPU: the _timed forms of the CTC / TDT beam searches (without a language model) and of the CTC / TDT forced alignments.  No time is
asserted.  A timed call returns the documented number of stage times, all finite and >= 0, and the untimed decode of the same input returns
right after it exactly what it returned right before it: the timed path leaves the model's workspaces usable and runs the same stages.
Each call still refuses reps = 0 and a non-positive n_frames entry with PK_ERR_INVALID."""
import math

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

T_LONG, T_SHORT = 20, 12
IDS = [np.asarray([1, 2, 3], np.int32), np.asarray([2], np.int32)]

# name -> (untimed decode, timed decode with reps, values a timed call returns)
CALLS = {
    "ctc_beam": (lambda gm, enc: gm.ctc_beam_decode(enc, 4, 8, 3, timestamps=True),
                 lambda gm, enc, reps: gm.ctc_beam_decode_timed(enc, 4, 8, 3, timestamps=True, reps=reps), 2),
    "tdt_beam": (lambda gm, enc: gm.tdt_beam_decode(enc, 4, 4, 2, 3),
                 lambda gm, enc, reps: gm.tdt_beam_decode_timed(enc, 4, 4, 2, 3, reps=reps), 2),
    "ctc_align": (lambda gm, enc: gm.ctc_align_decode(enc, IDS, total=True),
                  lambda gm, enc, reps: gm.ctc_align_decode_timed(enc, IDS, total=True, reps=reps), 2),
    "tdt_align": (lambda gm, enc: gm.tdt_align_decode(enc, IDS),
                  lambda gm, enc, reps: gm.tdt_align_decode_timed(enc, IDS, reps=reps), 4),
}


@pytest.fixture(scope="module")
def gm(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("timed_tiny"), pk.make_tiny_config(), seed=42, with_vocab=True)[2]


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, T_LONG, pk.make_tiny_config().hidden_size)).astype(np.float32)
    return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)


def batch(clips, form):
    """uniform: both clips at the longer length, [2][T_LONG][d]; ragged: the second cut to T_SHORT frames, one packed batch"""
    return clips if form == "uniform" else [clips[0], clips[1, :T_SHORT]]


def assert_same(a, b, what):
    """a decode's result (dicts / lists of arrays and numbers) equals another bit for bit"""
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            assert_same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{what}[{i}]")
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("form", ["uniform", "ragged"])
@pytest.mark.parametrize("name", list(CALLS))
def test_timed_call_returns_its_stage_times_and_leaves_the_decode_as_it_was(gm, clips, name, form):
    decode, timed, n_values = CALLS[name]
    enc = batch(clips, form)
    before = decode(gm, enc)
    ms = timed(gm, enc, 2)
    after = decode(gm, enc)
    assert len(ms) == n_values, ms
    assert all(math.isfinite(v) and v >= 0 for v in ms), ms
    assert_same(after, before, f"{name} {form}: the untimed decode after the timed call")


@pytest.mark.parametrize("name", list(CALLS))
def test_timed_call_refuses_zero_reps_and_an_empty_utterance(gm, clips, name):
    timed = CALLS[name][1]
    with pytest.raises(capi.PkError) as e:
        timed(gm, batch(clips, "ragged"), 0)
    assert e.value.code == -1, "reps = 0"
    with pytest.raises(capi.PkError) as e:
        timed(gm, [clips[0], clips[1, :0]], 2)
    assert e.value.code == -1, "n_frames[1] = 0"
