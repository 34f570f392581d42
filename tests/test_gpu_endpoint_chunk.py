"""GPU: the endpointing kernel and its rule alone (kernels/endpoint.hip through pk_endpoint_chunk_*) on host rows against the written specification,
tests/endpoint_ref.py, BIT FOR BIT: the level, the floor and the decision of every frame (fp32 as uint32), every event, over four chunkings; the
carried window where it wraps, the close, the reset, the truncation and the refusals.  The cases are tests/endpoint_cases.py's
(tests/test_endpoint_ref.py checks that none is vacuous)."""
import numpy as np
import pytest

from parakeet_cpp_amd import capi

import endpoint_cases as EC
import endpoint_ref as R

pytestmark = pytest.mark.gpu

bits = lambda x: np.asarray(x, np.float32).view(np.uint32)


def walk(w, name, chunks, what, close_at=None, close_mask=None):
    x = EC.case(name)
    want = EC.ref_pushes(name, chunks, close_at, close_mask)
    for i, (t, c) in enumerate(chunks):
        got = w.push(x["rows"][:, t:t + c])
        a, fl, sp, ev = want[i]
        assert np.array_equal(bits(got["level"]), bits(a)), f"{what} push {i} (frames {t} .. {t + c - 1}): level"
        assert np.array_equal(bits(got["floor"]), bits(fl)), f"{what} push {i} (frames {t} .. {t + c - 1}): floor"
        assert np.array_equal(got["speech0"], sp), f"{what} push {i}: speech0"
        assert got["n_events"] == len(ev) and got["events"] == ev, f"{what} push {i}: {got['events']} vs {ev}"
        if close_at == i:
            w.close_streams(close_mask)


@pytest.mark.parametrize("name", [n for n in EC.CASES if n != "f80_n512"])
def test_kernel_equals_the_specification(name):
    x = EC.case(name)
    w = capi.EndpointChunk(x["S"], x["F"], **x["kw"])
    try:
        for k, (cname, chunks) in enumerate(R.chunkings(x["n"]).items()):
            if k:
                w.reset()                                           # back to frame 0: the same rows give the same results
            walk(w, name, chunks, f"{name} {cname}")
    finally:
        w.close()


def test_call_of_512_frames():
    x = EC.case("f80_n512")
    w = capi.EndpointChunk(x["S"], x["F"], **x["kw"])
    try:
        walk(w, "f80_n512", [(0, 512)], "512 frames")
    finally:
        w.close()


def test_close_in_the_middle_of_an_utterance():
    name = "f80_w300"
    x = EC.case(name)
    start_at = max(next(e[4] for e in x["events"][s] if e[0] == R.START) for s in range(x["S"]))
    cut = start_at + 4                                              # every stream is inside its first utterance
    assert all(x["speech0"][s, cut:cut + 8].all() for s in range(x["S"]))
    chunks = [(0, cut)] + [(t + cut, c) for t, c in R.chunkings(x["n"] - cut)["alt"]]
    mask = [1, 0, 1]
    want = EC.ref_pushes(name, chunks, 0, mask)
    ev = [e for o in want for e in o[3]]
    # (the closed streams open a new utterance at the frame behind the close; the other one goes on)
    assert [e for e in ev if e[0] == 0 and e[1] == R.START][1][3] == cut and [e for e in ev if e[0] == 1 and e[1] == R.START][1][3] > cut + 20
    w = capi.EndpointChunk(x["S"], x["F"], **x["kw"])
    try:
        walk(w, name, chunks, "close", 0, mask)
    finally:
        w.close()


def test_truncation():
    name = "f80_w300"
    x = EC.case(name)
    all_ev = [(s,) + e for s in range(x["S"]) for e in x["events"][s]]
    assert len(all_ev) > 5
    w = capi.EndpointChunk(x["S"], x["F"], **x["kw"])
    try:
        got = w.push(x["rows"], want_rows=False, cap=5)
        assert got["n_events"] == len(all_ev) and got["events"] == all_ev[:5]
        w.reset()
        got = w.push(x["rows"], want_rows=False, cap=0)
        assert got["n_events"] == len(all_ev) and got["events"] == []
    finally:
        w.close()


def test_refusals():
    def refused(code, fn, *args, **kw):
        with pytest.raises(capi.PkError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (code, e.value.code, str(e.value))

    mk = lambda F=80, S=1, **kw: capi.EndpointChunk(S, F, **kw).close()
    refused(-1, mk, min_speech_ms=9)
    refused(-1, mk, min_silence_ms=0)
    refused(-1, mk, floor_window_ms=5)
    refused(-1, mk, min_speech_ms=100, max_utterance_s=0.1)
    refused(-1, mk, threshold_db=float("nan"))
    refused(-1, mk, eou_token_id=-2)
    refused(-1, mk, S=0)
    refused(-7, mk, floor_window_ms=10250)
    refused(-7, mk, F=513)
    mk(floor_window_ms=10240, F=512)                                # the limits themselves are served
    w = capi.EndpointChunk(2, 80, min_speech_ms=10, max_utterance_s=0.03)
    try:
        refused(-1, w.push, np.zeros((2, 0, 80), np.float32))
        refused(-7, w.push, np.zeros((2, 513, 80), np.float32))
        x = EC.case("f80_w300")
        got = w.push(x["rows"][:2, :40])                            # a refused call leaves the endpointer usable, at frame 0
        assert got["events"][0][5] < 40 and all(e[5] - e[3] + 1 <= 2 for e in got["events"])
    finally:
        w.close()
