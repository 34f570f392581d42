"""CPU: the written specification of the endpointing on live audio (tests/endpoint_ref.py) against itself and against brute force:
the chunking does not matter, the sliding minimum is exact, the rule honours its three lengths exactly, the token rule and the close behave as
written, the options are refused as listed -- and none of the cases the GPU tests use is vacuous."""
import numpy as np
import pytest

import endpoint_cases as EC
import endpoint_ref as R

bits = lambda x: np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_chunking_does_not_matter(name):
    x = EC.case(name)
    for cname, chunks in R.chunkings(x["n"]).items():
        out = EC.ref_pushes(name, chunks)
        a, fl, sp = (np.concatenate([o[k] for o in out], axis=1) for k in range(3))
        assert np.array_equal(bits(a), bits(x["a"])), (name, cname)
        assert np.array_equal(bits(fl), bits(x["floor"])), (name, cname)
        assert np.array_equal(sp, x["speech0"]), (name, cname)
        for s in range(x["S"]):
            assert [e[1:] for o in out for e in o[3] if e[0] == s] == x["events"][s], (name, cname, s)


def test_level_order():
    """the lane sums and the tree, written out per frame in scalar fp32"""
    rng = np.random.default_rng(3)
    for F in (1, 63, 64, 65, 80, 128, 200):
        rows = (rng.standard_normal((5, F)) * 7).astype(np.float32)
        want = []
        for r in rows:
            lane = [np.float32(0.0)] * 64
            for b in range(F):
                lane[b % 64] = np.float32(lane[b % 64] + r[b])
            for o in (32, 16, 8, 4, 2, 1):
                lane = [np.float32(lane[l] + lane[l + o]) for l in range(o)]
            want.append(lane[0])
        assert np.array_equal(bits(R.levels(rows)), bits(np.array(want, np.float32))), F


def test_key_is_order_preserving():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = R.key(v)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(bits(R.unkey(k)), bits(v))
    assert R.key(np.float32(np.nan))[0] == 0xFFFFFFFF and np.isnan(R.unkey(np.uint32(0xFFFFFFFF))[0])


@pytest.mark.parametrize("W", [1, 2, 5, 64, 300])
def test_sliding_minimum_against_brute_force(W):
    rng = np.random.default_rng(W)
    a = (rng.standard_normal(700) * 50).astype(np.float32)
    a[rng.integers(0, 700, 40)] = np.nan
    a[rng.integers(0, 700, 10)] = np.inf
    a[rng.integers(0, 700, 10)] = -np.inf
    a[100:100 + 2 * W] = np.nan                                     # windows that hold only NaN
    a[300:320] = a[300]
    fl = R.Floor(W)
    got = np.concatenate([fl.feed(a[t:t + c]) for t, c in R.chunkings(700)["mix"]])
    for f in range(700):
        w = a[max(0, f - W + 1):f + 1]
        if np.all(np.isnan(w)):
            assert np.isnan(got[f]), f
        else:
            assert bits(got[f]) == bits(np.nanmin(w)) or (got[f] == 0 and np.nanmin(w) == 0), f
    assert np.isnan(got[100 + 2 * W - 1])
    # a NaN level is not speech; a NaN floor leaves abs_thr in force
    sp = R.decide(np.array([np.nan, 5.0, -5.0], np.float32), np.array([1.0, np.nan, np.nan], np.float32), np.float32(0.0), np.float32(1.0))
    assert sp.tolist() == [0, 1, 0]


@pytest.mark.parametrize("name", list(EC.CASES))
def test_rule_honours_its_lengths(name):
    x = EC.case(name)
    o = x["opt"]
    for s in range(x["S"]):
        sp, ev = x["speech0"][s], x["events"][s]
        kinds = [e[0] for e in ev]
        assert kinds == [R.START, R.END] * (len(kinds) // 2) + [R.START] * (len(kinds) % 2), "START and END alternate"
        assert [e[4] for e in ev] == sorted(set(e[4] for e in ev)), "ordered, at most one per frame"
        open_start, prev_end_at = None, -1
        for kind, reason, start, end, at in ev:
            if kind == R.START:
                assert start == at - o.min_speech + 1 and end == at and np.all(sp[start:at + 1] == 1)
                # not a frame earlier: the run of speech began at `start` (or right behind the previous END)
                assert start == prev_end_at + 1 or sp[start - 1] == 0
                open_start = start
            else:
                assert start == open_start
                if reason == R.SILENCE:
                    assert at - end == o.min_silence and sp[end] == 1 and not sp[end + 1:at + 1].any()
                    assert at - start + 1 <= o.max_utterance
                else:
                    assert reason == R.MAX_LENGTH and end == at and at - start + 1 == o.max_utterance
                # no earlier frame of the utterance had min_silence frames without speech behind it
                run = 0
                for f in range(start, at):
                    run = 0 if sp[f] else run + 1
                    assert run < o.min_silence
                prev_end_at = at


@pytest.mark.parametrize("name", list(EC.CASES))
def test_cases_are_not_vacuous(name):
    x = EC.case(name)
    o = x["opt"]
    with np.errstate(all="ignore"):
        rel = (x["floor"] + o.margin).astype(np.float32)
    for s in range(x["S"]):
        ev = x["events"][s]
        assert sum(e[0] == R.END for e in ev) >= 2 and sum(e[0] == R.START for e in ev) >= 2, (name, s, ev)
        assert np.any(rel[s] > o.abs_thr) and np.any(rel[s] < o.abs_thr), (name, s)
        assert x["speech0"][s].any() and not x["speech0"][s].all()
        if EC.CASES[name].get("cut"):
            assert any(e[1] == R.MAX_LENGTH for e in ev), (name, s)
    if EC.CASES[name].get("special"):
        assert np.isnan(x["a"]).any() and np.isinf(x["a"]).any()
        assert not x["speech0"][np.isnan(x["a"])].any() and x["speech0"][np.isinf(x["a"])].all()


def test_close_and_token_rule():
    x = EC.case("f80_w300")
    o = R.Options(80, V=100, blank=99, eou_token_id=7, **x["kw"])
    start_at = next(e[4] for e in x["events"][0] if e[0] == R.START)
    rows = x["rows"][0]
    # the acoustic close in the middle of an utterance: the stream is outside, the speech that goes on opens a new utterance min_speech frames later
    e = R.Endpointer(o)
    _, _, _, ev = e.push(rows[:start_at + 5])
    assert ev[-1][0] == R.START and e.rule.in_utt
    ring, t = e.floor.ring.copy(), e.t
    e.rule.close()
    assert (e.rule.in_utt, e.rule.run_speech, e.rule.run_sil) == (0, 0, 0)
    assert np.array_equal(e.floor.ring, ring) and e.t == t           # the window and the frame numbering are not touched
    _, _, _, ev2 = e.push(rows[start_at + 5:start_at + 12])
    assert ev2[0][:3] == (R.START, R.NONE, start_at + 5) and ev2[0][4] == start_at + 5 + o.min_speech - 1
    # the token rule inside an utterance: END / TOKEN from the utterance's start to the push's last frame; the stream closes; the net restarts
    e = R.Endpointer(o)
    ev, reset = e.push_with_tokens(rows[:start_at + 5], [3, 7, 4])
    assert ev[-1] == (R.END, R.TOKEN, start_at - o.min_speech + 1, start_at + 4, start_at + 4) and reset and not e.rule.in_utt
    # ... outside one: start = the event's own frame
    e = R.Endpointer(o)
    ev, reset = e.push_with_tokens(rows[:10], [7])
    assert ev == [(R.END, R.TOKEN, 9, 9, 9)] and reset
    # ... another id, or no token rule: nothing
    ev, reset = e.push_with_tokens(rows[10:20], [3, 4])
    assert ev == [] and not reset
    e = R.Endpointer(R.Options(80, V=100, blank=99, **x["kw"]))
    assert e.push_with_tokens(rows[:10], [7]) == ([], False)
    # reset_decoder = 0: the event and the acoustic close stay, the prediction net goes on
    e = R.Endpointer(R.Options(80, V=100, blank=99, eou_token_id=7, reset_decoder=0, **x["kw"]))
    ev, reset = e.push_with_tokens(rows[:start_at + 5], [7])
    assert ev[-1][:2] == (R.END, R.TOKEN) and not reset and not e.rule.in_utt
    # an acoustic END asks for the restart too, and leaves what the frames behind it built up
    e = R.Endpointer(o)
    end_at = next(v[4] for v in x["events"][0] if v[0] == R.END)
    ev, reset = e.push_with_tokens(rows[:end_at + 1], [])
    assert ev[-1][0] == R.END and ev[-1][1] == R.SILENCE and reset
    # reset(): frame 0 again, the same events
    e.reset()
    assert e.push(rows[:end_at + 1])[3] == [v for v in x["events"][0] if v[4] <= end_at]


def test_options():
    d = R.Options(80)
    assert (d.W, d.min_speech, d.min_silence, d.max_utterance, d.eou_token_id, d.reset_decoder) == (300, 10, 50, 3000, -1, 1)
    assert d.abs_thr == np.float32(80 * -50.0 * np.log(10.0) / 10.0) and d.margin == np.float32(80 * 9.0 * np.log(10.0) / 10.0)
    assert R.Options(80, min_speech_ms=39).min_speech == 3            # integer division by 10

    def refused(code, F=80, **kw):
        with pytest.raises(R.Refused) as e:
            R.Options(F, V=100, blank=99, **kw)
        assert e.value.code == code, kw

    refused(R.INVALID, min_speech_ms=9)
    refused(R.INVALID, min_silence_ms=0)
    refused(R.INVALID, floor_window_ms=5)
    refused(R.INVALID, min_speech_ms=100, max_utterance_s=0.1)       # 10 frames < min_speech + 1
    R.Options(80, min_speech_ms=100, max_utterance_s=0.125)                     # 12 frames (0.11f * 100 is 10.99..: the product is truncated)
    refused(R.INVALID, threshold_db=float("nan"))
    refused(R.INVALID, eou_token_id=-2)
    refused(R.INVALID, eou_token_id=100)
    refused(R.INVALID, eou_token_id=99)
    refused(R.UNSUPPORTED, floor_window_ms=10250)
    R.Options(80, floor_window_ms=10240)
    refused(R.UNSUPPORTED, F=513)
    e = R.Endpointer(d)
    for n, code in ((0, R.INVALID), (513, R.UNSUPPORTED)):
        with pytest.raises(R.Refused) as ex:
            e.push(np.zeros((n, 80), np.float32))
        assert ex.value.code == code
