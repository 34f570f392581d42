"""The specification of the voice-activity segmentation (kernels/vad.hip and pk_vad_plan reproduce it bit for bit).

Everything is defined on the 16 kHz samples of ONE clip.  Frame energies are numpy float32 arithmetic in the fixed order of `energies`; the rest
is integer logic on frames and on the uint32 keys of the energies."""
import math

import numpy as np

FRAME = 160
GRID = 8
DEFAULTS = dict(threshold_db=-50.0, margin_db=9.0, floor_percent=10, min_speech_ms=100, min_silence_ms=300, pad_ms=200, max_gap_ms=1000,
                max_piece_s=30.0)


class Refused(ValueError):
    pass


def params(**options):
    """the options as the stage takes them: thresholds rounded once from double to fp32, durations in frames"""
    o = dict(DEFAULTS)
    for k, v in options.items():
        if k not in o:
            raise TypeError(k)
        o[k] = v
    th, mg, mp = (float(np.float32(o[k])) for k in ("threshold_db", "margin_db", "max_piece_s"))      # the struct holds floats
    if not all(math.isfinite(v) for v in (th, mg, mp)):
        raise Refused("not finite")
    if not -200.0 <= th <= 60.0 or not 0.0 <= mg <= 100.0 or not 0 <= o["floor_percent"] <= 100:
        raise Refused("range")
    for k in ("min_speech_ms", "min_silence_ms", "pad_ms", "max_gap_ms"):
        if not 0 <= o[k] <= 3600000:
            raise Refused(k)
    max_piece = math.floor(mp * 100.0 + 0.5)
    if not 16 <= max_piece <= 360000:
        raise Refused("max_piece")
    return dict(abs_thr=np.float32(160.0 * math.pow(10.0, th / 10.0)), ratio=np.float32(math.pow(10.0, mg / 10.0)),
                floor_percent=int(o["floor_percent"]), min_speech=o["min_speech_ms"] // 10, min_silence=o["min_silence_ms"] // 10,
                pad=o["pad_ms"] // 10, max_gap=o["max_gap_ms"] // 10, max_piece=int(max_piece))


def n_frames(n):
    if n >= 1 << 31:
        raise Refused("a clip of 2^31 samples or more")
    return (n + FRAME - 1) // FRAME


def energies(x):
    """e[f]: the frame's 160 samples (zeros past the clip) are 40 groups of four; lane l = 0 .. 7 adds the squares of groups l, l + 8, .. l + 32 in
    ascending sample order (20 terms, each product and each sum rounded to fp32), then the eight lanes are added as a tree: l with l + 4, then
    l with l + 2, then l with l + 1."""
    x = np.asarray(x, np.float32)
    F = n_frames(x.size)
    if F == 0:
        return np.zeros(0, np.float32)
    p = np.zeros(F * FRAME, np.float32)
    p[:x.size] = x
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (p * p).reshape(F, 5, 8, 4)                 # [frame][k][lane][j]: sample 4 * (lane + 8 k) + j
        acc = sq[:, 0, :, 0].copy()
        for k in range(5):
            for j in range(4):
                if k or j:
                    acc = acc + sq[:, k, :, j]
        acc = acc[:, :4] + acc[:, 4:]
        acc = acc[:, :2] + acc[:, 2:]
        acc = acc[:, 0] + acc[:, 1]
    return acc.astype(np.float32)


def keys(e):
    e = np.asarray(e, np.float32)
    k = e.view(np.uint32).copy()
    k[np.isnan(e)] = 0xFFFFFFFF
    return k


def noise_floor(e, floor_percent):
    """the energy whose key has rank ((F - 1) * floor_percent) // 100 in ascending order (a NaN when that key is a NaN's)"""
    k = np.sort(keys(e), kind="stable")
    rank = ((len(k) - 1) * floor_percent) // 100
    return np.array([k[rank]], np.uint32).view(np.float32)[0]


def raw_decision(e, p):
    fl = noise_floor(e, p["floor_percent"])
    with np.errstate(over="ignore", invalid="ignore"):
        thr = np.fmax(p["abs_thr"], np.float32(fl * p["ratio"]))
        return np.asarray(e, np.float32) > thr          # (False for a NaN)


def runs_of(flags):
    out, s = [], None
    for f, v in enumerate(flags):
        if v and s is None:
            s = f
        if not v and s is not None:
            out.append((s, f - 1))
            s = None
    if s is not None:
        out.append((s, len(flags) - 1))
    return out


def pad_run(s, e, pad, F):
    s2 = GRID * (max(0, s - pad) // GRID)
    e2 = min(F - 1, GRID * -(-(min(F - 1, e + pad) + 1) // GRID) - 1)
    return s2, e2


def smooth(speech0, p):
    """the three smoothing rules in order -> the runs (inclusive frame ranges, ascending, disjoint, starts on the 8-frame grid)"""
    F = len(speech0)
    sp = [bool(v) for v in speech0]
    gaps = runs_of([not v for v in sp])
    for s, e in gaps:                                    # 1. short gaps with speech on both sides
        if s > 0 and e < F - 1 and e - s + 1 < p["min_silence"]:
            for f in range(s, e + 1):
                sp[f] = True
    kept = [(s, e) for s, e in runs_of(sp) if e - s + 1 >= p["min_speech"]]      # 2. short speech runs
    out = []
    for s, e in kept:                                    # 3. pad, snap, merge what overlaps or touches
        s2, e2 = pad_run(s, e, p["pad"], F)
        if out and s2 <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], e2))
        else:
            out.append((s2, e2))
    return out


def vad(x, **options):
    """-> (runs, energies) of one clip"""
    p = params(**options)
    e = energies(x)
    if e.size == 0:
        return [], e
    return smooth(raw_decision(e, p), p), e


def plan(n_samples, runs, e, **options):
    """the pieces of one clip as sample ranges [begin, end)"""
    p = params(**options)
    mp, k = p["max_piece"], keys(e) if e is not None else None
    pieces = []

    def take(s, t):
        if pieces and s - pieces[-1][1] - 1 <= p["max_gap"] and t - pieces[-1][0] + 1 <= mp:
            pieces[-1][1] = t
        else:
            pieces.append([s, t])
    for s, t in runs:
        while t - s + 1 > mp:
            cand = [f for f in range(s + mp // 2, s + mp) if (f + 1) % GRID == 0]
            cut = min(cand, key=lambda f: (int(k[f]), f))
            take(s, cut)
            s = cut + 1
        take(s, t)
    return [(FRAME * s, min(n_samples, FRAME * (t + 1))) for s, t in pieces]


def merge(results, pieces, n_clips, timestamps):
    """pk_transcribe_pcm_vad's merge rule: results[i] is the transcription (a dict of capi.transcribe_pcm) of pieces[i] = (clip, begin, end)"""
    out = [dict(text="", token_ids=[], **(dict(start=[], end=[], conf=[], words=[]) if timestamps else {})) for _ in range(n_clips)]
    for r, (c, b, _) in zip(results, pieces):
        off = b // (FRAME * GRID)
        o = out[c]
        if r["text"]:
            o["text"] = (o["text"] + " " + r["text"]) if o["text"] else r["text"]
        o["token_ids"] += r["token_ids"]
        if timestamps:
            o["start"] += [v + off for v in r["start"]]
            o["end"] += [v + off for v in r["end"]]
            o["conf"] += r["conf"]
            o["words"] += [(w, float(np.float32(np.float64(np.float32(s)) + off * 0.08)), float(np.float32(np.float64(np.float32(e)) + off * 0.08)), cf)
                           for w, s, e, cf in r["words"]]
    return out
