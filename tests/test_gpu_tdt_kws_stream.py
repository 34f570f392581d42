"""GPU: the streaming TDT keyword spotting's chunked walk and online rule (kernels/tdt_kws_stream.hip) on host lattices against its written
specification, tests/tdt_kws_stream_ref.py, BIT FOR BIT: the exit rows of every push (scores as uint32), every event, the flush."""
import functools

import numpy as np
import pytest

from parakeet_cpp_amd import capi

import tdt_kws_ref as R
import tdt_kws_stream_ref as SR

pytestmark = pytest.mark.gpu

NEG = R.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)

T = 62
LS = (1, 2, 7, 64, 7)                                               # lane L - 1 = lane 0, lanes past L, a full wave; 5 pairs of mixed L in one call
DURS = {"d01234": [0, 1, 2, 3, 4], "d1": [1], "d08": [0, 8], "d0to7": list(range(8))}
CHUNKINGS = {"ones": [1], "threes": [3], "whole": [62], "mix": [1, 5, 2, 14, 1, 17]}
# (threshold, patience) of every chunking's walker: both thresholds and both patiences on every durations set and family
OPTS = {"ones": (False, 0), "threes": (True, 3), "whole": (True, 0), "mix": (False, 3)}


@functools.lru_cache(maxsize=None)
def case(dname, family):
    """the lattices of the 5 pairs and the reference's rows of the whole session (computed once, shared, never changed)"""
    dur = DURS[dname]
    rng = np.random.default_rng(500 + 2 * list(DURS).index(dname) + (family == "holes"))
    lats = [R.make_lattice(family, T, L, len(dur), rng) for L in LS]
    rows = [SR.ChunkWalk(L, dur).push(*lat) for L, lat in zip(LS, lats)]
    finite = np.concatenate([E[E > NEG] for E, _, _ in rows])
    for lat in lats:
        for x in lat:
            x.setflags(write=False)
    return lats, rows, np.float32(np.median(finite))


def ref_events(rows, min_score, patience, chunks):
    """-> per push the events ordered by pair then by emission, and the flush's"""
    picks = [SR.OnlinePick(min_score, patience) for _ in rows]
    per_push = []
    for t0, c in chunks:
        ev = []
        for p, (E, Bs, Ee) in enumerate(rows):
            ev += [(0, p, st, en, sc) for sc, st, en in picks[p].feed_rows(t0, E[t0:t0 + c], Bs[t0:t0 + c], Ee[t0:t0 + c])]
        per_push.append(ev)
    flush = []
    for p, pk in enumerate(picks):
        flush += [(0, p, st, en, sc) for sc, st, en in pk.flush()]
    return per_push, flush, picks


def same_events(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} events vs {len(want)}: {got} vs {want}"
    for g, w in zip(got, want):
        assert g[:4] == w[:4] and bits(g[4]) == bits(w[4]), f"{what}: {g} vs {w}"


def run_and_compare(w, lats, rows, min_score, patience, chunks, what):
    per_push, flush, picks = ref_events(rows, min_score, patience, chunks)
    for k, (t0, c) in enumerate(chunks):
        got = w.push([SR.cut(lat, t0, c) for lat in lats])
        for p, (E, Bs, Ee) in enumerate(rows):
            assert np.array_equal(bits(got["E"][p]), bits(E[t0:t0 + c])), f"{what}: push {k} pair {p} E"
            assert np.array_equal(got["Bs"][p], Bs[t0:t0 + c]), f"{what}: push {k} pair {p} Bs"
            assert np.array_equal(got["Ee"][p], Ee[t0:t0 + c]), f"{what}: push {k} pair {p} Ee"
        assert got["n_events"] == len(per_push[k])
        same_events(got["events"], per_push[k], f"{what}: push {k}")
    same_events(w.flush(), flush, f"{what}: flush")
    assert w.flush() == []                                          # nothing twice
    return per_push, picks


@pytest.mark.parametrize("chunking", list(CHUNKINGS))
@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("dname", list(DURS))
def test_pushes_equal_reference(dname, family, chunking):
    lats, rows, median = case(dname, family)
    dur = DURS[dname]
    thr, patience = OPTS[chunking]
    min_score = median if thr else NEG
    chunks = SR.chunks_of(T, CHUNKINGS[chunking])
    # on the reference alone: the case is not vacuous
    per_push, flush, picks = ref_events(rows, min_score, patience, chunks)
    assert sum(len(e) for e in per_push) >= 1, "no event leaves before the flush"
    if thr:
        assert any(np.any((E > NEG) & (E < min_score)) for E, _, _ in rows), "no frame below the threshold"
        assert any(np.any(E >= min_score) for E, _, _ in rows)
    w = capi.TdtKwsChunkWalk(LS, dur, min_score=None if not thr else float(min_score), patience=patience)
    try:
        run_and_compare(w, lats, rows, min_score, patience, chunks, f"{dname} {family} {chunking}")
    finally:
        w.close()


@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("dname", ["d01234", "d08"])
def test_offline_walk_equals_whole_session_chunk_walk(dname, family):
    """The offline kernel and the chunk kernel each hold the recurrence: the offline spotting's single hit is, bit for bit in score and exactly in
    span, the hit picked from the rows of the whole session pushed as ONE chunk, with Ee clamped to T - 1."""
    lats, rows, _ = case(dname, family)
    dur = DURS[dname]
    # on the reference alone: the case is not vacuous
    assert any(R.pick(E, Bs, np.minimum(Ee, T - 1))[0] == 1 for E, Bs, Ee in rows), "no pair has a hit"
    assert any(np.any((E > NEG) & (Ee > T - 1)) for E, _, Ee in rows), "the clamp changes no row"
    w = capi.TdtKwsChunkWalk(LS, dur)
    try:
        got = w.push(lats, rows=True)
    finally:
        w.close()
    off = capi.tdt_kws(lats, dur, max_hits=1, min_score=None)
    for p in range(len(LS)):
        n, st, en, sc = R.pick(got["E"][p], got["Bs"][p], np.minimum(got["Ee"][p], T - 1))
        what = f"{dname} {family} pair {p}"
        assert off["n_hits"][p] == n, what
        assert off["start"][p, 0] == st[0] and off["end"][p, 0] == en[0], f"{what}: [{off['start'][p, 0]}, {off['end'][p, 0]}] vs [{st[0]}, {en[0]}]"
        assert bits(off["score"][p, 0]) == bits(sc[0]), what


def test_reset_in_mid_stream_equals_a_fresh_walker():
    lats, rows, median = case("d01234", "ties")
    chunks = SR.chunks_of(T, CHUNKINGS["mix"])
    w = capi.TdtKwsChunkWalk(LS, DURS["d01234"], min_score=float(median), patience=3)
    try:
        for t0, c in chunks[:3]:
            w.push([SR.cut(lat, t0, c) for lat in lats])
        w.reset()
        run_and_compare(w, lats, rows, median, 3, chunks, "after reset")
        w.reset()                                                   # ... and after a flush
        run_and_compare(w, lats, rows, median, 3, SR.chunks_of(T, [3]), "after flush and reset")
    finally:
        w.close()


def test_cap_smaller_than_the_events_of_a_push():
    lats, rows, _ = case("d01234", "ties")
    per_push, _, _ = ref_events(rows, NEG, 0, [(0, T)])
    want = per_push[0]
    assert len(want) >= 3
    w = capi.TdtKwsChunkWalk(LS, DURS["d01234"])
    try:
        got = w.push(lats, cap=2)
        assert got["n_events"] == len(want)                         # the total is returned, the prefix alone is written
        same_events(got["events"], want[:2], "cap = 2")
        w.reset()
        got = w.push(lats, cap=0, rows=False)
        assert got["n_events"] == len(want) and got["events"] == []
    finally:
        w.close()


def test_refusals():
    rng = np.random.default_rng(2)
    dur = [0, 1]

    def refused(code, fn):
        with pytest.raises(capi.PkError) as e:
            fn()
        assert e.value.code == code, (code, e.value.code, str(e.value))

    refused(-7, lambda: capi.TdtKwsChunkWalk([65], dur))            # L = 65
    refused(-7, lambda: capi.TdtKwsChunkWalk([2], [0, 9]))          # a duration of 9
    w = capi.TdtKwsChunkWalk([2], dur)
    try:
        refused(-1, lambda: w.push([SR.cut(R.make_lattice("ties", 3, 2, 2, rng), 0, 0)]))       # c = 0
        refused(-7, lambda: w.push([R.make_lattice("ties", 63, 2, 2, rng)]))                   # c = 63
        lat = R.make_lattice("ties", 62, 2, 2, rng)                  # the walker is as it was: a full push still equals the reference
        E, Bs, Ee = SR.ChunkWalk(2, dur).push(*lat)
        got = w.push([lat])
        assert np.array_equal(bits(got["E"][0]), bits(E)) and np.array_equal(got["Bs"][0], Bs) and np.array_equal(got["Ee"][0], Ee)
    finally:
        w.close()
