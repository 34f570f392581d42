"""The written specification of the endpointing on live audio (kernels/endpoint.hip): numpy, fp32 values, integer logic.
The device equals it bit for bit.

Everything is defined on the log-mel rows a streaming push leaves on the device: raw ln(mel + 2^-24), F bins per 10 ms frame, no normalisation.
Frames are numbered from the session's last reset; the streams are independent.

  level a[f]    the fp32 sum of the frame's F bins: lane l = 0 .. 63 starts at +0.0 and adds bins l, l + 64, ... in ascending order (every add rounded
                to fp32), then the 64 lane sums fold as a tree, l with l + 32, then l + 16, 8, 4, 2, 1 (own + higher).
  key(x)        the order-preserving map fp32 -> uint32: all bits of a negative value inverted, the sign bit of a non-negative one set; NaN ->
                0xFFFFFFFF.  unkey is its inverse (unkey(0xFFFFFFFF) is the NaN 0x7FFFFFFF).
  floor[f]      unkey(min key(a[g]) over g = max(0, f - W + 1) .. f): the exact sliding minimum of the last W = floor_window frames (section 5.8's
                percentile needs the whole clip).  A NaN level is ignored unless the window holds nothing else; then the floor is NaN.
  speech0[f]    a[f] > fmaxf(abs_thr, floor[f] + margin): one fp32 add; abs_thr = (float)(F threshold_db ln10 / 10), margin = (float)(F margin_db
                ln10 / 10), each computed in double and rounded once.  A NaN level is not speech; a NaN floor (or margin) leaves abs_thr in force.
  OnlineEndpoint  the START / END rule, fed one frame at a time, so its events do not depend on the chunking.
  token rule    (host) a token with id eou_token_id among the ids a push returns for a stream emits END / TOKEN.
  close         what an END does to the stream at the push boundary.

An event is (kind, reason, start, end, at) in frames.  START: start = utt_start, end = at = the frame that opened the utterance.  END: see the rule.
START and END of the acoustic rule alternate; an END / TOKEN may come with no utterance open (then start = at).

The close and the chunking.  The acoustic events depend on the rows alone.  The transcript after a close does depend on the chunking: the prediction
net restarts at the boundary of the push in which the END fired, and the tokens that push returned belong to the utterance that ended.  An acoustic
END has already left the stream outside an utterance with run_speech = 0 at the frame it fired; the frames of the same push behind it have been fed
since, and their state is kept (putting it back to "outside, 0" at the push boundary would make the acoustic events depend on the chunking).  An
END / TOKEN is not acoustic: it closes the acoustic state at the push boundary whether or not reset_decoder is set; reset_decoder governs the
prediction net alone."""
import math

import numpy as np

START, END = 1, 2
NONE, SILENCE, MAX_LENGTH, TOKEN = 0, 1, 2, 3
MAX_WINDOW, MAX_FRAMES, MAX_BINS = 1024, 512, 512
f32 = np.float32


class Refused(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


INVALID, UNSUPPORTED = -1, -7

DEFAULTS = dict(threshold_db=-50.0, margin_db=9.0, floor_window_ms=3000, min_speech_ms=100, min_silence_ms=500, max_utterance_s=30.0, eou_token_id=-1,
                reset_decoder=1)


class Options:
    """pk_endpoint_options in frames.  Milliseconds become frames by integer division by 10; max_utterance_s by (int)(s * 100)."""

    def __init__(self, F, V=None, blank=None, **kw):
        o = dict(DEFAULTS)
        o.update(kw)
        self.F = F
        self.threshold_db, self.margin_db = float(o["threshold_db"]), float(o["margin_db"])
        self.W = int(o["floor_window_ms"]) // 10
        self.min_speech = int(o["min_speech_ms"]) // 10
        self.min_silence = int(o["min_silence_ms"]) // 10
        s = float(f32(o["max_utterance_s"])) * 100.0                 # the field is a float; the product is taken in double and truncated
        self.max_utterance = int(min(max(s, -1.0), 2.0e9)) if not math.isnan(s) else 0
        self.eou_token_id, self.reset_decoder = int(o["eou_token_id"]), int(o["reset_decoder"])
        if self.min_speech < 1 or self.min_silence < 1 or self.W < 1:
            raise Refused(INVALID, "min_speech / min_silence / floor_window below one frame")
        if self.max_utterance < self.min_speech + 1:
            raise Refused(INVALID, "max_utterance < min_speech + 1 frames")
        if math.isnan(self.threshold_db) or math.isnan(self.margin_db):
            raise Refused(INVALID, "NaN threshold")
        if self.eou_token_id < -1 or (V is not None and (self.eou_token_id >= V or self.eou_token_id == blank)):
            raise Refused(INVALID, "eou_token_id outside [-1, V) or the blank")
        if self.W > MAX_WINDOW or F > MAX_BINS:
            raise Refused(UNSUPPORTED, "floor_window > 1024 frames or F > 512")
        if F < 1:
            raise Refused(INVALID, "F")
        self.abs_thr = f32(F * self.threshold_db * (math.log(10.0) / 10.0))
        self.margin = f32(F * self.margin_db * (math.log(10.0) / 10.0))


def levels(rows):
    """rows [n][F] fp32 -> a [n] fp32, in the order written above (vectorised over the frames: the order inside a frame is the specification's)."""
    rows = np.asarray(rows, f32)
    n, F = rows.shape
    lane = np.zeros((n, 64), f32)
    with np.errstate(all="ignore"):
        for b0 in range(0, F, 64):
            w = min(64, F - b0)
            lane[:, :w] = lane[:, :w] + rows[:, b0:b0 + w]
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane[:, :o] + lane[:, o:2 * o]
    return lane[:, 0].copy()


def key(x):
    b = np.atleast_1d(np.asarray(x, f32)).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return k


def unkey(k):
    k = np.atleast_1d(np.asarray(k, np.uint32))
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(f32)


class Floor:
    """The causal noise floor: the keys of the last W frames in a ring indexed by frame % W."""

    def __init__(self, W):
        self.W, self.t = W, 0
        self.ring = np.full(W, 0xFFFFFFFF, np.uint32)

    def feed(self, a):
        """a [n] levels of the next n frames -> floor [n]"""
        out = np.empty(len(a), f32)
        for i, k in enumerate(key(a)):
            self.ring[self.t % self.W] = k
            self.t += 1
            out[i] = unkey(self.ring.min())[0]                       # (a slot no frame has filled holds 0xFFFFFFFF, which a minimum ignores)
        return out


def decide(a, floor, abs_thr, margin):
    with np.errstate(all="ignore"):
        thr = np.fmax(f32(abs_thr), (np.asarray(floor, f32) + f32(margin)).astype(f32))
        return (np.asarray(a, f32) > thr).astype(np.int32)


class OnlineEndpoint:
    """The rule of one stream, one frame at a time."""

    def __init__(self, min_speech, min_silence, max_utterance):
        self.min_speech, self.min_silence, self.max_utterance = min_speech, min_silence, max_utterance
        self.in_utt, self.run_speech, self.run_sil, self.utt_start, self.last_speech = 0, 0, 0, 0, 0

    def feed(self, f, speech):
        """-> None or the event (kind, reason, start, end, at) of frame f"""
        if not self.in_utt:
            self.run_speech = self.run_speech + 1 if speech else 0
            if self.run_speech == self.min_speech:
                self.in_utt, self.utt_start, self.last_speech, self.run_sil = 1, f - self.min_speech + 1, f, 0
                return (START, NONE, self.utt_start, f, f)
            return None
        if speech:
            self.last_speech, self.run_sil = f, 0
        else:
            self.run_sil += 1
        if self.run_sil == self.min_silence:
            self.in_utt, self.run_speech = 0, 0
            return (END, SILENCE, self.utt_start, self.last_speech, f)
        if f - self.utt_start + 1 == self.max_utterance:
            self.in_utt, self.run_speech = 0, 0
            return (END, MAX_LENGTH, self.utt_start, f, f)
        return None

    def close(self):
        """the acoustic close: outside an utterance, run_speech = 0; nothing else is touched"""
        self.in_utt, self.run_speech, self.run_sil = 0, 0, 0

    def token(self, at):
        """the token rule's event for a push whose last mel frame was `at` (the caller closes the stream afterwards)"""
        return (END, TOKEN, self.utt_start if self.in_utt else at, at, at)


class Endpointer:
    """One stream: level, floor, decision and rule over pushes of rows; the frame count starts at the reset."""

    def __init__(self, opt):
        self.opt = opt
        self.reset()

    def reset(self):
        o = self.opt
        self.floor, self.rule, self.t = Floor(o.W), OnlineEndpoint(o.min_speech, o.min_silence, o.max_utterance), 0

    def push(self, rows):
        """rows [n][F] -> (a, floor, speech0 [n], events)"""
        rows = np.asarray(rows, f32)
        if rows.ndim != 2 or rows.shape[0] < 1:
            raise Refused(INVALID, "a call with no rows")
        if rows.shape[0] > MAX_FRAMES:
            raise Refused(UNSUPPORTED, "more than 512 frames in one call")
        a = levels(rows)
        fl = self.floor.feed(a)
        sp = decide(a, fl, self.opt.abs_thr, self.opt.margin)
        ev = []
        for i, s in enumerate(sp):
            e = self.rule.feed(self.t + i, int(s))
            if e:
                ev.append(e)
        self.t += len(sp)
        return a, fl, sp, ev

    def push_with_tokens(self, rows, ids):
        """One session push: the acoustic part over the rows the push fed, then the token rule over the ids it returned.
        -> (events, reset_decoder: the prediction net of this stream restarts before the next push)."""
        _, _, _, ev = self.push(rows)
        o = self.opt
        if o.eou_token_id >= 0 and o.eou_token_id in [int(v) for v in ids]:
            ev.append(self.rule.token(self.t - 1))
            self.rule.close()
        fired = any(e[0] == END for e in ev)
        return ev, bool(fired and o.reset_decoder)


def chunkings(n, rng=None):
    """the four chunkings of n frames the tests use: all at once (in calls of at most 512), one frame at a time, 14 / 15 alternating, irregular"""
    def cut(sizes):
        out, t, i = [], 0, 0
        while t < n:
            c = min(sizes[i % len(sizes)], n - t)
            out.append((t, c))
            t += c
            i += 1
        return out
    return {"whole": cut([MAX_FRAMES]), "ones": cut([1]), "alt": cut([14, 15]), "mix": cut([1, 37, 2, 160, 5, 16, 16, 3, 61])}
