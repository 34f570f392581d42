"""The specification of the streaming TDT keyword spotting (tests/tdt_kws_stream_ref.py): the chunked walk against the offline
walk of tests/tdt_kws_ref.py, the online rule's properties, and the argument refusals of pk_tdt_kws_chunk_create that need no device.  CPU only."""
import numpy as np
import pytest

from parakeet_cpp_amd import capi

import tdt_kws_ref as R
import tdt_kws_stream_ref as SR

NEG = R.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)

T = 40
DURS = ([0, 1, 2, 3, 4], [1], [0, 8])
CHUNKINGS = {"ones": [1], "threes": [3], "whole": [40], "mix": [1, 5, 2, 14, 1, 17]}


def rows_of(lat, L, dur, sizes):
    w = SR.ChunkWalk(L, dur)
    out = [w.push(*SR.cut(lat, t0, c)) for t0, c in SR.chunks_of(lat[1].shape[0], sizes)]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def events_of(E, Bs, Ee, min_score=NEG, patience=0, flush=True):
    p = SR.OnlinePick(min_score, patience)
    p.feed_rows(0, E, Bs, Ee)
    if flush:
        p.flush()
    return p.events


@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("L", [1, 2, 7])
@pytest.mark.parametrize("di", range(len(DURS)))
def test_chunked_rows_equal_the_offline_walk(di, L, family):
    dur = DURS[di]
    assert max(dur) + 2 > 3 or dur == [1]                            # 3-frame chunks lie below dur_max = 8 for [0, 8]
    rng = np.random.default_rng(1000 + 100 * di + 10 * L + (family == "holes"))
    lat = R.make_lattice(family, T, L, len(dur), rng)
    E0, Bs0, Ee0, _ = R.walk(*lat, dur)
    assert np.any(E0 > NEG)
    got = {}
    for name, sizes in CHUNKINGS.items():
        E, Bs, Ee = rows_of(lat, L, dur, sizes)
        assert np.array_equal(bits(E), bits(E0)), (name, "E")
        assert np.array_equal(Bs, Bs0), (name, "Bs")
        ok = E0 > NEG
        assert np.array_equal(np.minimum(Ee, T - 1)[ok], Ee0[ok]), (name, "Ee")
        assert np.all(Ee[~ok] == 0)
        got[name] = (E, Bs, Ee)
    # the online rule is fed frame by frame: its events cannot depend on the chunking
    ms = np.float32(np.median(E0[E0 > NEG]))
    for min_score, patience in ((NEG, 0), (ms, 0), (ms, 3)):
        ev = {name: events_of(*rows, min_score, patience) for name, rows in got.items()}
        assert all(e == ev["ones"] for e in ev.values())
        assert len(ev["ones"]) >= 1
        for k, (sc, st, en) in enumerate(ev["ones"]):              # disjoint, ordered in time, above the threshold
            assert sc >= min_score and st <= en
            if k:
                assert ev["ones"][k - 1][2] < st


def test_spotter_over_chunks_equals_rule_over_whole_rows():
    dur = [0, 1, 2, 3, 4]
    rng = np.random.default_rng(3)
    lat = R.make_lattice("ties", T, 3, len(dur), rng)
    E, Bs, Ee = rows_of(lat, 3, dur, [40])
    want = events_of(E, Bs, Ee, -2.0, 1)
    s = SR.Spotter(3, dur, -2.0, 1)
    got = []
    for t0, c in SR.chunks_of(T, CHUNKINGS["mix"]):
        got += s.push(*SR.cut(lat, t0, c))[3]
    got += s.flush()
    assert got == want and len(want) >= 2


def test_planted_path_is_the_only_event():
    rng = np.random.default_rng(5)
    dur = [0, 1, 2, 4]
    L = 4
    lab, blk, dl, top = R.make_lattice("ties", T, L, len(dur), rng)
    lab = np.minimum(lab, top[:, :L] - np.float32(0.5)).astype(np.float32)         # nothing else is greedy
    s, e = R.plant(lab, blk, dl, top, dur, 11, [([], 2), ([1], 0), ([], 1), ([3, 1], 2)])
    assert (s, e) == (11, 21)
    for sizes in CHUNKINGS.values():
        sp = SR.Spotter(L, dur, min_score=0.0)                      # min_score 0: only a greedy match counts
        ev = []
        for t0, c in SR.chunks_of(T, sizes):
            ev += sp.push(*SR.cut((lab, blk, dl, top), t0, c))[3]
        ev += sp.flush()
        assert len(ev) == 1 and ev[0][1:] == (s, e) and bits(ev[0][0]) == 0        # +0.0, sign bit clear


def test_flush_and_patience():
    E = np.full(30, NEG, np.float32); Bs = np.zeros(30, np.int32); Ee = np.zeros(30, np.int32)
    for t, (e, b, en) in {4: (-1.0, 2, 5), 5: (-0.5, 3, 6), 6: (-2.0, 3, 7), 15: (-1.0, 12, 16)}.items():
        E[t], Bs[t], Ee[t] = e, b, en
    left = {}
    for patience in (0, 3):
        p = SR.OnlinePick(NEG, patience)
        at = []
        for t in range(30):
            at += [(t, ev) for ev in p.feed(t, E[t], Bs[t], Ee[t])]
        left[patience] = at
        assert [ev for _, ev in at] == [(np.float32(-0.5), 3, 6), (np.float32(-1.0), 12, 16)]
        assert p.flush() == [] and p.flush() == []                  # nothing pending, nothing twice
    assert [t for t, _ in left[0]] == [7, 17] and [t for t, _ in left[3]] == [10, 20]          # end + patience + 1
    # a disjoint later hit releases the pending one at once, patience or not; flush emits the last
    p = SR.OnlinePick(NEG, 100)
    assert p.feed(4, -1.0, 2, 5) == [] and p.feed(9, -3.0, 7, 9) == [(np.float32(-1.0), 2, 5)]
    assert p.flush() == [(np.float32(-3.0), 7, 9)] and p.flush() == []
    # strict >: an equal overlapping score keeps the earlier hit; the threshold and -inf frames never qualify
    p = SR.OnlinePick(-2.0, 0)
    assert p.feed(0, -2.5, 0, 0) == [] and p.feed(1, NEG, 0, 0) == [] and p.pending is None
    p.feed(2, -1.0, 1, 3); p.feed(3, -1.0, 2, 4)
    assert p.flush() == [(np.float32(-1.0), 1, 3)]
    # what the online rule loses against the offline one: A replaced by B, B replaced by C disjoint from A -> C alone
    p = SR.OnlinePick(NEG, 10)
    for t, e, b, en in ((3, -3.0, 1, 3), (4, -2.0, 3, 5), (5, -1.0, 5, 6)):
        assert p.feed(t, e, b, en) == []
    assert p.flush() == [(np.float32(-1.0), 5, 6)]
    n, st, en, _ = R.pick(np.asarray([NEG, NEG, NEG, -3.0, -2.0, -1.0], np.float32), [0, 0, 0, 1, 3, 5], [0, 0, 0, 3, 5, 6], 4)
    assert n == 2 and list(st[:2]) == [5, 1]


def test_walker_refusals_need_no_device():
    def refused(code, **kw):
        a = dict(kw_len=[2, 3], durations=[0, 1, 2])
        a.update(kw)
        with pytest.raises(capi.PkError) as e:
            capi.TdtKwsChunkWalk(**a)
        assert e.value.code == code, (kw, e.value.code, str(e.value))

    refused(-7, kw_len=[65])
    refused(-7, durations=[0, 9])
    refused(-7, durations=[1] * 9)
    refused(-7, kw_len=[1] * 65537, durations=[1])
    refused(-7, kw_len=[64] * 40000, durations=[0, 1, 2, 3, 4, 5, 6, 8])       # more than 1 GiB at the 62-frame push limit
    refused(-1, kw_len=[2, 0])
    refused(-1, kw_len=[])
    refused(-1, patience=-1)
    refused(-1, min_score=0.5)
    refused(-1, min_score=float("nan"))
    if capi.device_count() == 0:                                    # valid arguments fail loudly without a device
        refused(-4)
    o = capi.stream_kws_options()
    assert o.min_score == -np.inf and o.patience == 0
