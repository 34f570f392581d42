"""GPU: the voice-activity segmentation stage alone (pk_vad_pcm, kernels/vad.hip) against its specification tests/vad_ref.py, bit for bit: the
frame energies, and the runs after the exact noise-floor select, the raw decision and the three smoothing rules.

The content is built so that any raw pattern can be placed: a frame is silence, noise, or a burst whose energy comes out as an exact number.
One sample of 1.0 in lane 0 and j pairs of 2^-12 in lane 1 give e = 1 + j * 2^-23 (keys that differ in their low byte only); 2^6 and 2^-10
give keys that differ in the high byte; equal frames give ties.  One clip of random samples checks the summation order on ordinary data."""
import numpy as np
import pytest

import vad_ref as V
from parakeet_cpp_amd import capi

pytestmark = pytest.mark.gpu

G = capi.vad_run()
RAW = dict(min_speech_ms=0, min_silence_ms=0, pad_ms=0)
SMOOTH = dict(min_speech_ms=40, min_silence_ms=50, pad_ms=30)
WIDE = dict(min_speech_ms=100, min_silence_ms=6000, pad_ms=2000)            # gaps and padding far longer than a chunk
OPTIONS = (RAW, SMOOTH, {}, WIDE)


def frame(level):
    """160 samples of one frame: 0 silence, -1 noise (e = 2^-20), -2 loud (e = 2^12), j >= 1 a burst with e = 1 + (j - 1) * 2^-23"""
    x = np.zeros(160, np.float32)
    if level == -1:
        x[0] = 2.0 ** -10
    elif level == -2:
        x[0] = 64.0
    elif level >= 1:
        x[0] = 1.0
        lane1 = [4 * (1 + 8 * k) + j for k in range(5) for j in range(4)]
        x[lane1[:2 * (level - 1)]] = 2.0 ** -12
    return x


def clip(n, levels):
    x = np.concatenate([frame(v) for v in levels] + [np.zeros(0, np.float32)])[:n]
    assert x.size == n
    return np.ascontiguousarray(x)


def pattern(F, seed, p_speech=0.5):
    """levels with runs of 1 .. 12 frames, bursts of mixed energies, silence or noise between them"""
    r = np.random.default_rng(seed)
    out = []
    while len(out) < F:
        n = int(r.integers(1, 13))
        if r.random() < p_speech:
            out += [int(v) for v in r.choice([1, 1, 2, 3, 9, -2], n)]
        else:
            out += [int(v) for v in r.choice([0, 0, -1], n)]
    return out[:F]


def check(clips, **opt):
    got = capi.vad(clips, **opt)
    for i, (c, g) in enumerate(zip(clips, got)):
        runs, e = V.vad(c, **opt)
        assert np.array_equal(g["energy"].view(np.uint32), e.view(np.uint32)), (i, opt)
        assert g["runs"].tolist() == [list(r) for r in runs], (i, opt)
    return got


def test_shortest_clips_share_a_batch():
    lens = (0, 1, 159, 160, 161, 1280)
    clips = [clip(n, [1] * V.n_frames(n)) for n in lens]
    clips[1][0] = 0.5                                                     # a clip of one sample
    clips[4][160] = 0.25                                                  # a last frame of one sample
    clips[5][:160] = 0.0                                                  # (a silent frame: the floor of this clip is 0)
    for opt in OPTIONS:
        got = check(clips, **opt)
        assert len(got[0]["runs"]) == 0 and got[0]["energy"].size == 0
    assert check(clips, **RAW)[5]["runs"].tolist() == [[0, 7]]


def boundary_clips():
    out = []
    for k, n in enumerate((160 * G - 1, 160 * G, 160 * G + 1, 160 * (3 * G + 7) + 5)):
        F = V.n_frames(n)
        lv = [0] * F
        lv[0] = 1                                                         # speech at frame 0
        lv[F - 1] = 2                                                     # ... and at the last (here partial) frame
        for f in range(G - 9, G - 3):
            lv[f] = 3
        if F > G + 6:                                                     # a gap of 4 frames and a run of 3 straddling the chunk boundary
            lv[G - 3: G + 1] = [0, 0, -1, 0]
            lv[G + 1: G + 4] = [1, 9, 1]
        if F > 3 * G:                                                     # a run that ends a chunk, a run that starts one, a gap of two chunks
            lv[2 * G - 2: 2 * G] = [1, 1]
            lv[3 * G: 3 * G + 4] = [2, 2, -2, 2]
        out.append(clip(n, lv))
    return out


def test_chunk_boundaries():
    clips = boundary_clips()
    for opt in OPTIONS:
        check(clips, **opt)
    got = check(clips, **SMOOTH)[3]["runs"].tolist()
    assert [G - 16, G + 7] in got and got[-1] == [3 * G - 8, 3 * G + 7]                  # the gap across the boundary was filled
    raw = check(clips, **RAW)[3]["runs"].tolist()
    assert raw[0] == [0, 7] and raw[-1] == [3 * G, 3 * G + 7] and [2 * G - 8, 2 * G - 1] in raw and [2 * G - 8, 2 * G - 1] not in got


def test_random_patterns_and_random_samples():
    F = 3 * G + 8
    clips = [clip(160 * F - 31, pattern(F, 5)), clip(160 * (G + 1), pattern(G + 1, 6, 0.2)), clip(160 * 2 * G, pattern(2 * G, 7, 0.8))]
    noise = np.random.default_rng(8).standard_normal(160 * 300 + 77).astype(np.float32)
    noise[160 * 100:160 * 180] *= 1e-3
    noise[160 * 250] = np.nan                                             # a NaN frame: the largest key, never speech
    clips.append(noise)
    for opt in OPTIONS + (dict(floor_percent=0), dict(floor_percent=100), dict(floor_percent=50, margin_db=0.0)):
        check(clips, **opt)


def test_the_floor_decides():
    lv = np.zeros(400 * 160, np.float32)
    a = np.float32(0.1)
    lv[::160] = a                                                         # every frame e = 0.01: above the absolute threshold 1.6e-3
    lv[160 * 100:160 * 150:160] = np.float32(np.sqrt(0.05))               # below floor * ratio = 0.0794
    lv[160 * 200:160 * 260:160] = np.float32(np.sqrt(0.1))                # above
    got = check([lv], **RAW)[0]["runs"].tolist()
    assert got == [[200, 263]]
    assert check([lv], floor_percent=0, margin_db=0.0, threshold_db=-39.0, **RAW)[0]["runs"].tolist() == [[96, 151], [200, 263]]   # 0.0201: absolute


def test_a_second_order_gives_the_same_bits():
    clips = boundary_clips() + [clip(160 * 700, pattern(700, 11))]
    a = capi.vad(clips, **SMOOTH)
    order = [4, 2, 0, 3, 1]
    b = capi.vad([clips[i] for i in order], **SMOOTH)
    for k, i in enumerate(order):
        assert np.array_equal(a[i]["energy"].view(np.uint32), b[k]["energy"].view(np.uint32)) and a[i]["runs"].tolist() == b[k]["runs"].tolist()


def test_sentinels_around_and_between_the_clips_come_back():
    clips = boundary_clips()[2:] + [np.zeros(0, np.float32), clip(160 * 40, [0] * 10 + [1] * 20 + [0] * 10)]
    F = [V.n_frames(c.size) for c in clips]
    cap = [(f + 1) // 2 for f in F]
    S = -77
    rs, re = np.full(sum(cap) + 16, S, np.int32), np.full(sum(cap) + 16, S, np.int32)
    en = np.full(sum(F) + 16, -7.5, np.float32)
    got = capi.vad(clips, run_start=rs[8:], run_end=re[8:], energy=en[8:], **SMOOTH)
    r0 = 8
    for c, g, k in zip(clips, got, cap):
        runs, _ = V.vad(c, **SMOOTH)
        n = len(runs)
        assert g["runs"].tolist() == [list(r) for r in runs]
        assert rs[r0:r0 + n].tolist() == [r[0] for r in runs] and re[r0:r0 + n].tolist() == [r[1] for r in runs]
        assert np.all(rs[r0 + n:r0 + k] == S) and np.all(re[r0 + n:r0 + k] == S)
        r0 += k
    for a in (rs, re):
        assert np.all(a[:8] == S) and np.all(a[8 + sum(cap):] == S)
    assert np.all(en[:8] == -7.5) and np.all(en[8 + sum(F):] == -7.5) and not np.any(en[8:8 + sum(F)] == -7.5)


def test_state_is_carried_across_more_chunks_than_one_search_step_reads():
    F = G * (G + 3)                                                       # more than 256 chunks between the two ends of the gap
    x = np.zeros(160 * F, np.float32)
    x[0:160 * 12:160] = 1.0
    x[160 * (F - 12)::160] = 1.0
    opt = dict(min_silence_ms=3600000, min_speech_ms=100, pad_ms=0)
    got = capi.vad([x], **opt)[0]
    assert got["runs"].tolist() == [[0, F - 1]]
    assert np.array_equal(got["energy"].view(np.uint32), V.energies(x).view(np.uint32))
    opt["min_silence_ms"] = 10 * (F - 24)                                 # one frame too short to fill
    assert capi.vad([x], **opt)[0]["runs"].tolist() == [[0, 15], [F - 16, F - 1]]
