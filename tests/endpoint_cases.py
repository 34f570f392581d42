"""The cases the endpointing tests share (tests/test_endpoint_ref.py checks on the reference alone that none of them is vacuous;
tests/test_gpu_endpoint_chunk.py runs the kernel on them): synthetic log-mel rows of S streams, noise with bursts of "speech", a noisy first half
(the floor plus the margin decides) and a quiet second half (the absolute threshold decides: a minimum follows a drop at once), and what the
specification makes of them."""
import functools

import numpy as np

import endpoint_ref as R

# per-bin levels (natural log of power): threshold_db -50 is -11.5 per bin, margin_db 9 is +2.07 per bin
QUIET, NOISY, SPEECH = -14.0, -9.0, -4.0
BURSTS = ((0.08, 0.16), (0.27, 0.38), (0.58, 0.68), (0.80, 0.90))          # fractions of the sequence; the gaps are at least 0.10

CASES = {
    # F 80, 3 streams, a window longer than every chunk and shorter than the sequence (the ring wraps), min_speech 3, min_silence 30
    "f80_w300": dict(F=80, S=3, n=400, opt=dict(floor_window_ms=3000, min_speech_ms=30, min_silence_ms=300)),
    # one bin, one stream, a window of one frame: the floor is the level, so the margin is negative
    "f1_w1": dict(F=1, S=1, n=120, opt=dict(floor_window_ms=10, min_speech_ms=10, min_silence_ms=10, margin_db=-1.0)),
    # F 65 (one bin past a wave), a window shorter than a chunk, min_speech 1, min_silence 1
    "f65_w5": dict(F=65, S=3, n=150, opt=dict(floor_window_ms=50, min_speech_ms=10, min_silence_ms=10)),
    # F 128, max_utterance 40 frames: shorter than a burst of 0.10 x 500 frames, so every such burst is cut
    "f128_cut": dict(F=128, S=1, n=500, cut=True, opt=dict(floor_window_ms=3000, min_speech_ms=30, min_silence_ms=300, max_utterance_s=0.4)),
    # a NaN row, a +inf row and a stretch of equal rows in every stream
    "f80_special": dict(F=80, S=3, n=400, special=True, opt=dict(floor_window_ms=3000, min_speech_ms=30, min_silence_ms=300)),
    # one call of 512 frames
    "f80_n512": dict(F=80, S=1, n=512, opt=dict(floor_window_ms=3000, min_speech_ms=30, min_silence_ms=300)),
}


def make_rows(S, n, F, seed, special=False):
    rng = np.random.default_rng(seed)
    rows = np.empty((S, n, F), np.float32)
    for s in range(S):
        base = np.where(np.arange(n) < n // 2, NOISY, QUIET).astype(np.float64)
        shift = int(rng.integers(0, max(1, n // 50)))
        for a, b in BURSTS:
            base[int(a * n) + shift:int(b * n) + shift] = SPEECH
        rows[s] = (base[:, None] + 0.3 * rng.standard_normal((n, F))).astype(np.float32)
        if special:
            gap = int(0.45 * n)
            rows[s, gap:gap + 12] = rows[s, gap]                     # rows all equal (silence)
            rows[s, int(0.12 * n) + shift] = np.nan                  # a NaN row inside a burst
            rows[s, int(0.50 * n), F // 2] = np.nan                  # one NaN bin in silence
            rows[s, int(0.72 * n)] = np.inf                          # a +inf row in silence
    return rows


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rows [S][n][F] (read-only), opt (R.Options), a / floor / speech0 [S][n], events: per stream the specification's events of the whole
    sequence) -- computed once, shared, never changed"""
    c = CASES[name]
    rows = make_rows(c["S"], c["n"], c["F"], 1000 + list(CASES).index(name), c.get("special", False))
    rows.setflags(write=False)
    opt = R.Options(c["F"], **c["opt"])
    a, fl, sp, ev = [], [], [], []
    for s in range(c["S"]):
        e = R.Endpointer(opt)
        outs = [e.push(rows[s, t:t + k]) for t, k in R.chunkings(c["n"])["whole"]]
        a.append(np.concatenate([o[0] for o in outs])); fl.append(np.concatenate([o[1] for o in outs]))
        sp.append(np.concatenate([o[2] for o in outs])); ev.append(sum((o[3] for o in outs), []))
    return dict(rows=rows, opt=opt, kw=c["opt"], a=np.stack(a), floor=np.stack(fl), speech0=np.stack(sp), events=ev, **{k: c[k] for k in ("F", "S", "n")})


def ref_pushes(name, chunks, close_at=None, close_mask=None):
    """The specification over the given chunking [(t, c)...]: per push (a, floor, speech0 [S][c], events ordered by stream then by emission).  close_at:
    the index of the push after which the streams of close_mask are closed."""
    x = case(name)
    eps = [R.Endpointer(x["opt"]) for _ in range(x["S"])]
    out = []
    for i, (t, c) in enumerate(chunks):
        per = [e.push(x["rows"][s, t:t + c]) for s, e in enumerate(eps)]
        ev = [(s,) + e for s, p in enumerate(per) for e in p[3]]
        out.append((np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), ev))
        if close_at == i:
            for s, e in enumerate(eps):
                if close_mask[s]:
                    e.rule.close()
    return out
