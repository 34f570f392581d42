"""CPU: the specification of the voice-activity segmentation (tests/vad_ref.py) on hand-worked cases of every rule, and
pk_vad_plan (host logic, no device) against vad_ref.plan."""
import math

import numpy as np
import pytest

import vad_ref as V
from parakeet_cpp_amd import capi

P0 = dict(min_speech_ms=0, min_silence_ms=0, pad_ms=0)          # no smoothing: the raw runs on the 8-frame grid


def flags(F, *runs):
    a = np.zeros(F, bool)
    for s, e in runs:
        a[s:e + 1] = True
    return a


def test_frames_and_energy_order():
    assert [V.n_frames(n) for n in (0, 1, 159, 160, 161, 1280)] == [0, 1, 1, 1, 2, 8]
    assert V.vad(np.zeros(0, np.float32)) == ([], pytest.approx(np.zeros(0)))
    x = np.zeros(161, np.float32)
    x[0], x[159], x[160] = 0.5, 2.0, 3.0
    assert V.energies(x).tolist() == [4.25, 9.0]                 # samples past the clip count as 0
    # the order is the specification: lane sums of 20 terms, then a tree of 8 -- not a left-to-right sum
    r = np.random.default_rng(1).standard_normal(160).astype(np.float32)
    sq = r * r
    lanes = []
    for l in range(8):
        acc = np.float32(0)
        for k in range(5):
            for j in range(4):
                acc = np.float32(acc + sq[4 * (l + 8 * k) + j])
        lanes.append(acc)
    t4 = [np.float32(lanes[i] + lanes[i + 4]) for i in range(4)]
    t2 = [np.float32(t4[i] + t4[i + 2]) for i in range(2)]
    assert V.energies(r)[0] == np.float32(t2[0] + t2[1])


def test_keys_rank_with_ties_and_nan():
    e = np.array([4.0, 1.0, np.nan, 1.0, 0.0, 1.0, 2.0, 1.0, 3.0, 1.0, 0.5], np.float32)      # sorted: 0 .5 1 1 1 1 1 2 3 4 nan
    assert V.keys(e)[2] == 0xFFFFFFFF and V.keys(e)[4] == 0
    assert [float(V.noise_floor(e, p)) for p in (0, 9, 10, 20, 60, 69, 70, 90)] == [0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 2.0, 4.0]
    assert math.isnan(V.noise_floor(e, 100))
    # a NaN frame is not speech, and a NaN floor leaves the absolute threshold in force
    p = V.params(floor_percent=100, threshold_db=-10.0)          # abs_thr = 16
    assert p["abs_thr"] == np.float32(16.0)
    e2 = np.array([np.nan, 17.0, 16.0, np.inf], np.float32)
    assert V.raw_decision(e2, p).tolist() == [False, True, False, True]


def test_constants_are_rounded_once_from_double():
    p = V.params()
    assert p["abs_thr"] == np.float32(160.0 * 10.0 ** -5.0) and p["ratio"] == np.float32(10.0 ** 0.9)
    assert (p["min_speech"], p["min_silence"], p["pad"], p["max_gap"], p["max_piece"]) == (10, 30, 20, 100, 3000)
    assert V.params(min_speech_ms=109)["min_speech"] == 10 and V.params(max_piece_s=0.16)["max_piece"] == 16


def test_floor_decides_when_it_is_above_the_absolute_threshold():
    e = np.array([1.0] * 9 + [7.9, 8.0, 8.1], np.float32)        # floor 1, ratio 10^0.9 = 7.943...
    p = V.params()
    assert V.raw_decision(e, p).tolist() == [False] * 10 + [True, True]
    assert V.raw_decision(e, V.params(threshold_db=-10.0)).tolist() == [False] * 12          # abs_thr 16 decides


def test_gap_of_min_silence_minus_one_is_filled_and_of_min_silence_is_not():
    p = V.params(min_silence_ms=120, min_speech_ms=0, pad_ms=0)
    assert V.smooth(flags(64, (8, 15), (27, 31)), p) == [(8, 31)]                 # gap 16 .. 26: 11 frames < 12
    assert V.smooth(flags(64, (8, 15), (28, 31)), p) == [(8, 15), (24, 31)]       # a gap of 12 frames stays (the second run snaps to 24)
    assert V.smooth(flags(64, (2, 5)), p) == [(0, 7)]                             # silence at the clip's ends has speech on one side only


def test_speech_run_of_min_speech_minus_one_is_dropped_and_of_min_speech_is_kept():
    p = V.params(min_speech_ms=40, min_silence_ms=0, pad_ms=0)
    assert V.smooth(flags(64, (8, 10), (32, 35)), p) == [(32, 39)]
    # filling comes first: two runs of 2 frames with a short gap are one run of 6
    p2 = V.params(min_speech_ms=40, min_silence_ms=30, pad_ms=0)
    assert V.smooth(flags(64, (8, 9), (12, 13)), p2) == [(8, 15)]
    assert V.smooth(flags(64, (8, 9), (13, 14)), p2) == []


def test_padding_at_both_clip_ends_and_snapping_that_merges():
    p = V.params(min_speech_ms=0, min_silence_ms=0, pad_ms=30)
    assert V.smooth(flags(37, (1, 2), (34, 35)), p) == [(0, 7), (24, 36)]         # max(0, 1 - 3); min(F - 1, ...) with a partial last grid cell
    assert V.pad_run(34, 35, 3, 37) == (24, 36) and V.pad_run(9, 9, 0, 100) == (8, 15) and V.pad_run(8, 15, 0, 100) == (8, 15)
    q = V.params(**P0)
    assert V.smooth(flags(64, (9, 10), (14, 14)), q) == [(8, 15)]                 # both snap to [8, 15]: overlap
    assert V.smooth(flags(64, (9, 10), (17, 17)), q) == [(8, 23)]                 # [8, 15] and [16, 23] touch
    assert V.smooth(flags(64, (9, 10), (25, 25)), q) == [(8, 15), (24, 31)]
    runs = V.smooth(flags(64, (9, 10), (25, 25), (40, 63)), q)
    assert all(s % 8 == 0 for s, _ in runs) and all(a[1] + 1 < b[0] for a, b in zip(runs, runs[1:]))


def test_whole_clip_from_samples():
    x = np.zeros(160 * 40 + 5, np.float32)
    x[160 * 12:160 * 30] = 0.1
    x[-5:] = 0.5                                                                  # the last, partial frame
    runs, e = V.vad(x, **P0)
    assert len(e) == 41 and runs == [(8, 31), (40, 40)]
    assert V.vad(x)[0] == [(0, 40)]                                                # defaults: the 5-sample frame is too short, padding reaches frame 0


def plan_both(n, runs, e, **kw):
    want = V.plan(n, runs, e, **kw)
    got = capi.vad_plan(n, runs, e, **kw)
    assert got == want
    return got


def test_plan_matches_the_library():
    F = 1000
    n = 160 * F - 7
    e = np.random.default_rng(3).random(F).astype(np.float32)
    kw = dict(max_piece_s=2.0, max_gap_ms=500)                                    # 200 frames, 50 frames
    assert plan_both(n, [], e, **kw) == []
    assert plan_both(n, [(8, 207)], e, **kw) == [(1280, 160 * 208)]               # exactly max_piece: not cut
    got = plan_both(n, [(8, 208)], e, **kw)                                       # max_piece + 1: cut in [108, 207] after a frame with (f + 1) % 8 == 0
    cand = [f for f in range(108, 208) if (f + 1) % 8 == 0]
    cut = min(cand, key=lambda f: (V.keys(e)[f], f))
    assert got == [(1280, 160 * (cut + 1)), (160 * (cut + 1), 160 * 209)]
    tie = np.ones(F, np.float32)
    tie[[119, 151, 183]] = 0.25                                                   # three equal minima: the earliest
    assert plan_both(n, [(8, 300)], tie, **kw) == [(1280, 160 * 120), (160 * 120, 160 * 301)]
    nan = tie.copy()
    nan[119] = np.nan                                                             # a NaN has the largest key
    assert plan_both(n, [(8, 300)], nan, **kw)[0] == (1280, 160 * 152)
    assert plan_both(n, [(0, 39), (90, 129)], e, **kw) == [(0, 160 * 130)]        # gap of max_gap = 50 frames joins
    assert plan_both(n, [(0, 39), (91, 129)], e, **kw) == [(0, 160 * 40), (160 * 91, 160 * 130)]
    assert plan_both(n, [(0, 99), (104, 199)], e, **kw) == [(0, 160 * 200)]       # joined span exactly max_piece
    assert plan_both(n, [(0, 99), (104, 200)], e, **kw) == [(0, 160 * 100), (160 * 104, 160 * 201)]
    assert plan_both(n, [(960, 999)], e, **kw) == [(160 * 960, n)]                # the piece ends with the clip
    long = plan_both(160 * 5000, [(0, 4999)], np.random.default_rng(4).random(5000).astype(np.float32), **kw)
    assert all(0 < b - a <= 160 * 200 for a, b in long) and all(a % 1280 == 0 for a, _ in long)
    assert long[0][0] == 0 and long[-1][1] == 160 * 5000 and all(x[1] == y[0] for x, y in zip(long, long[1:]))


def test_refusals_need_no_device():
    bad = [dict(max_piece_s=0.15), dict(max_piece_s=3600.01), dict(max_piece_s=float("nan")), dict(threshold_db=float("inf")),
           dict(threshold_db=-201.0), dict(threshold_db=61.0), dict(margin_db=-0.5), dict(margin_db=101.0), dict(margin_db=float("nan")),
           dict(floor_percent=-1), dict(floor_percent=101), dict(min_speech_ms=-1), dict(min_silence_ms=3600001), dict(pad_ms=-10),
           dict(max_gap_ms=-1)]
    x = np.zeros(1600, np.float32)
    for kw in bad:
        with pytest.raises(V.Refused):
            V.params(**kw)
        with pytest.raises(capi.PkError) as e:
            capi.vad_plan(1600, [], None, **kw)
        assert e.value.code == -1, kw
        with pytest.raises(capi.PkError) as e:                                    # refused before a device is looked for
            capi.vad([x], **kw)
        assert e.value.code == -1, kw
    capi.vad_plan(1600, [], None, max_piece_s=0.16)
    with pytest.raises(V.Refused):
        V.n_frames(1 << 31)
    L = capi.lib()
    import ctypes as C
    off = np.array([0, 1 << 31], np.int64)
    nr, rs = np.zeros(1, np.int32), np.zeros(8, np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    st = L.pk_vad_pcm(0, x.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, None, i32(nr), i32(rs), i32(rs), None)
    assert st == -7                                                               # PK_ERR_UNSUPPORTED: a clip of 2^31 samples, nothing touched
    for runs in ([(5, 4)], [(0, 10)], [(0, 3), (3, 5)]):                          # runs that are no runs of a clip of 10 frames
        with pytest.raises(capi.PkError) as e:
            capi.vad_plan(1600, runs, np.zeros(10, np.float32))
        assert e.value.code == -1
    assert capi.vad_run() == 256 and dict(capi.PkVadOptions._fields_).keys() == V.DEFAULTS.keys()
    o = capi.vad_options()
    assert {k: getattr(o, k) for k in V.DEFAULTS} == V.DEFAULTS
