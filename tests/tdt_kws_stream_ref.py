"""Streaming TDT keyword spotting, in plain numpy fp32: the written specification of DESIGN.md section 5.5.9 that kernels/tdt_kws_stream.hip
is compared against bit for bit.  The lattice, its normalisation and the recurrence are those of tests/tdt_kws_ref.py (section 5.5.8), unchanged:
enter at every frame with +0.0; candidates in the order blank 0 .. D-1 then label 0 .. D-1; strict > keeps the earlier candidate; b is copied
from the chosen source; the exit is folded over the D label arcs of column L-1.

ChunkWalk: the walk of tdt_kws_ref.walk, stopped at every chunk boundary and picked up again.  Frames are numbered from the start of the
session; a source frame < 0 does not exist, a source frame before the current chunk is read from the CARRIED STATE: for the last dur_max + 2
frames (a ring indexed by frame modulo dur_max + 2, of which a pull reads dur_max + 1), the 2 D candidates every column offered -- fl(a + w)
per blank arc and per label arc -- and the column's b.  It is all a later chunk may read, and all the kernel keeps.  The session has no last
frame: Ee[t] = t + max(dur[i*], 1) - 1 without the clamp of token_end (0 where E[t] is -inf).

OnlinePick: an ONLINE APPROXIMATION of the greedy non-overlapping peak picking of section 5.5.4, which needs every frame of the clip before it
picks the first hit.  One pending hit per pair; a better overlapping frame replaces it, a disjoint later frame or `patience` frames of silence
after its end release it.  A frame whose span starts at or before the end of the last hit that LEFT does not qualify (the offline rule's mask, which
keeps the events of a pair pairwise disjoint and ordered in time: without it a hit released by patience could be followed by a longer match that
began inside it).  What is lost against the offline rule: a pending hit that was replaced can no longer be reported, even if the hit that
replaced it is later replaced itself by one disjoint from the first -- the offline rule would then report both the last and the first."""
import numpy as np

from tdt_kws_ref import MAX_DUR, MAX_L, NEG, F, _w, make_lattice, normalise, plant  # noqa: F401  (make_lattice / plant: the tests' inputs)

MAX_CHUNK = 62


class ChunkWalk:
    """The walk of one (stream, keyword) pair.  push() takes the lattice rows of the next c >= 1 frames in the layouts of tdt_kws_ref.walk."""

    def __init__(self, L, dur):
        self.L, self.dur, self.D = int(L), [int(d) for d in dur], len(dur)
        assert 1 <= self.L <= MAX_L and 1 <= self.D <= 8 and all(0 <= d <= MAX_DUR for d in self.dur)
        self.R = max(self.dur) + 2
        self.reset()

    def reset(self):
        self.t0 = 0                                                 # frames seen so far
        self.cb = np.full((self.R, self.L, self.D), NEG, np.float32)     # [frame % R][u][i] the blank candidates column u offered at that frame
        self.cl = np.full((self.R, self.L, self.D), NEG, np.float32)     # ... the label candidates
        self.b = np.zeros((self.R, self.L), np.int32)

    def push(self, lab, blk, dl, top):
        """lab [c][L], blk [c][L+1], dl [c][L+1][D], top [c][L+1] -> E[c] fp32, Bs[c] int32, Ee[c] int32 (frames since the session began)."""
        nlab, nblk, ndl = normalise(lab, blk, dl, top)
        c, L, D, R, dur = nblk.shape[0], self.L, self.D, self.R, self.dur
        assert c >= 1 and nblk.shape[1] == L + 1 and ndl.shape[2] == D
        E = np.full(c, NEG, np.float32); Bs = np.zeros(c, np.int32); Ee = np.zeros(c, np.int32)
        with np.errstate(all="ignore"):
            for j in range(c):
                t = self.t0 + j
                for u in range(L):
                    if u == 0:
                        best, org = F(0.0), t
                    else:
                        best, org = NEG, 0
                        for i in range(D):
                            ts = t - max(dur[i], 1)
                            if ts >= 0:
                                cand = self.cb[ts % R, u, i]
                                if cand > best:
                                    best, org = cand, self.b[ts % R, u]
                        for i in range(D):
                            ts = t - dur[i]
                            if ts >= 0:
                                cand = self.cl[ts % R, u - 1, i]
                                if cand > best:
                                    best, org = cand, self.b[ts % R, u - 1]
                    for i in range(D):
                        self.cb[t % R, u, i] = F(best + _w(nblk[j, u], ndl[j, u, i]))
                        self.cl[t % R, u, i] = F(best + _w(nlab[j, u], ndl[j, u, i]))
                    self.b[t % R, u] = org
                e, arg = NEG, -1
                for i in range(D):
                    v = self.cl[t % R, L - 1, i]
                    if v > e:
                        e, arg = v, i
                E[j], Bs[j] = e, self.b[t % R, L - 1]
                Ee[j] = t + max(dur[arg], 1) - 1 if arg >= 0 else 0
        self.t0 += c
        return E, Bs, Ee


class OnlinePick:
    """The online hit rule of one pair, fed frame by frame.  An event is (score, start, end), frames since the session began, inclusive."""

    def __init__(self, min_score=NEG, patience=0):
        assert not min_score > 0 and patience >= 0
        self.min_score, self.patience = F(min_score), int(patience)
        self.reset()

    def reset(self):
        self.pending = None
        self.last_end = -1                                          # the end of the last hit that left
        self.events = []                                            # every event so far, in the order emitted

    def _emit(self, out):
        out.append(self.pending)
        self.events.append(self.pending)
        self.last_end = self.pending[2]
        self.pending = None

    def feed(self, t, e, bs, ee):
        """Frame t with its exit (E[t], Bs[t], Ee[t]) -> the events that leave at this frame (at most one)."""
        out = []
        e = F(e)
        if self.pending is not None and t > self.pending[2] + self.patience:                     # 1.
            self._emit(out)
        if e > NEG and e >= self.min_score and bs > self.last_end:                               # 2.
            cur = (e, int(bs), int(ee))
            if self.pending is None:                                                             # 3.
                self.pending = cur
            elif cur[1] <= self.pending[2] and self.pending[1] <= cur[2]:                        # 4.
                if e > self.pending[0]:
                    self.pending = cur
            else:                                                                                # 5.
                self._emit(out)
                self.pending = cur
        return out

    def feed_rows(self, t0, E, Bs, Ee):
        out = []
        for j in range(len(E)):
            out += self.feed(t0 + j, E[j], Bs[j], Ee[j])
        return out

    def flush(self):
        out = []
        if self.pending is not None:
            self._emit(out)
        return out


class Spotter:
    """ChunkWalk + OnlinePick of one pair: push() -> (E, Bs, Ee, the events of this push)."""

    def __init__(self, L, dur, min_score=NEG, patience=0):
        self.walk, self.rule = ChunkWalk(L, dur), OnlinePick(min_score, patience)

    def push(self, lab, blk, dl, top):
        t0 = self.walk.t0
        E, Bs, Ee = self.walk.push(lab, blk, dl, top)
        return E, Bs, Ee, self.rule.feed_rows(t0, E, Bs, Ee)

    def flush(self):
        return self.rule.flush()

    def reset(self):
        self.walk.reset()
        self.rule.reset()


def chunks_of(T, sizes):
    """[(t0, c)...] covering T frames: `sizes` repeated, the last chunk cut."""
    out, t, k = [], 0, 0
    while t < T:
        c = min(sizes[k % len(sizes)], T - t)
        out.append((t, c))
        t += c; k += 1
    return out


def cut(lat, t0, c):
    """the rows [t0, t0 + c) of a lattice (lab, blk, dl, top)"""
    return tuple(x[t0:t0 + c] for x in lat)
