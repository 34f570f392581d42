"""GPU: the TDT keyword spotting's walk and picking (kernels/tdt_kws.hip) on host lattices against its written specification,
tests/tdt_kws_ref.py, BIT FOR BIT: scores, spans, counts, unused slots, the sign of +0.0."""
import numpy as np
import pytest

from parakeet_cpp_amd import capi

import tdt_kws_ref as R

pytestmark = pytest.mark.gpu

NEG = R.NEG
bits = lambda x: np.asarray(x, np.float32).view(np.uint32)

DURS = {"d0124": [0, 1, 2, 4], "d124": [1, 2, 4], "d0to7": list(range(8)), "d8": [8]}
# (max_hits, min_score) of the grid's calls: 1, 4 and 16 hits, with and without a threshold
OPTS = {"d0124": (4, None), "d124": (1, -6.0), "d0to7": (16, -4.0), "d8": (4, -8.0)}
TS = (1, 2, 7, 130)
LS = (1, 2, 3, 16, 17, 32, 33, 64)                                  # straddle a row of 16 lanes, the half-wave and the full wave


def same(got, b, want, what):
    """pair b of the library's arrays against the specification's dict"""
    assert got["n_hits"][b] == want["n_hits"], f"{what}: n_hits {got['n_hits'][b]} vs {want['n_hits']}"
    assert np.array_equal(got["start"][b], want["start"]), f"{what}: start {got['start'][b]} vs {want['start']}"
    assert np.array_equal(got["end"][b], want["end"]), f"{what}: end {got['end'][b]} vs {want['end']}"
    assert np.array_equal(bits(got["score"][b]), bits(want["score"])), f"{what}: score bits {got['score'][b]} vs {want['score']}"


def ref_of(lat, dur, H, ms):
    E, Bs, Ee, ties = R.walk(*lat, dur)
    n, st, en, sc = R.pick(E, Bs, Ee, H, NEG if ms is None else np.float32(ms))
    return dict(n_hits=n, start=st, end=en, score=sc), ties


@pytest.mark.parametrize("family", ["ties", "holes"])
@pytest.mark.parametrize("dname", list(DURS))
def test_grid_equals_reference(dname, family):
    dur = DURS[dname]
    H, ms = OPTS[dname]
    rng = np.random.default_rng(100 + list(DURS).index(dname) * 2 + (family == "holes"))
    shapes = [(T, L) for T in TS for L in LS]
    lats = [R.make_lattice(family, T, L, len(dur), rng) for T, L in shapes]
    want = [ref_of(lat, dur, H, ms) for lat in lats]
    if family == "ties" and dname != "d8":                          # on the reference alone: the case is not vacuous
        assert sum(t for _, t in want) > 0, "no tie-decided cell"
    if family == "ties" and dname == "d0124":
        assert any(w["n_hits"] == 4 for w, _ in want), "no clip with 4 hits"
    got = capi.tdt_kws(lats, dur, max_hits=H, min_score=ms)
    for b, (T, L) in enumerate(shapes):
        same(got, b, want[b][0], f"{family} {dname} T={T} L={L}")
        w = want[b][0]
        assert np.all(got["score"][b][w["n_hits"]:] == NEG) and np.all(got["start"][b][w["n_hits"]:] == 0) and np.all(got["end"][b][w["n_hits"]:] == 0)


def test_keyword_longer_than_the_clip_without_a_zero_duration_has_no_hit():
    dur = DURS["d124"]
    lat = R.make_lattice("ties", 63, 64, len(dur), np.random.default_rng(7))
    want, _ = ref_of(lat, dur, 4, None)
    assert want["n_hits"] == 0                                      # 63 label arcs of >= 1 frame each do not fit 63 frames
    got = capi.tdt_kws([lat], dur, max_hits=4)
    same(got, 0, want, "T=63 L=64")
    assert got["n_hits"][0] == 0 and np.all(got["score"][0] == NEG) and np.all(got["start"][0] == 0) and np.all(got["end"][0] == 0)


def test_ragged_batch_equals_reference_and_single_calls():
    dur = DURS["d0124"]
    rng = np.random.default_rng(11)
    shapes = [(T, L) for T in (1, 9, 64, 65, 130) for L in (1, 2, 5, 17, 40)]
    lats = [R.make_lattice("ties" if i % 2 else "holes", T, L, len(dur), rng) for i, (T, L) in enumerate(shapes)]
    got = capi.tdt_kws(lats, dur, max_hits=4, min_score=-5.0)
    for b, (T, L) in enumerate(shapes):
        same(got, b, ref_of(lats[b], dur, 4, -5.0)[0], f"ragged pair {b} T={T} L={L}")
    for b in (0, 7, 13, 24):
        alone = capi.tdt_kws([lats[b]], dur, max_hits=4, min_score=-5.0)
        for k in ("n_hits", "start", "end"):
            assert np.array_equal(alone[k][0], got[k][b]), (b, k)
        assert np.array_equal(bits(alone["score"][0]), bits(got["score"][b])), b


def test_planted_greedy_path_scores_plus_zero():
    rng = np.random.default_rng(5)
    dur = [0, 1, 2, 4]
    T, L = 70, 4
    lab, blk, dl, top = R.make_lattice("ties", T, L, len(dur), rng)
    lab = np.minimum(lab, top[:, :L] - np.float32(0.5)).astype(np.float32)         # nothing else is greedy
    s, e = R.plant(lab, blk, dl, top, dur, 41, [([], 2), ([1], 0), ([], 1), ([3, 1], 2)])
    want, _ = ref_of((lab, blk, dl, top), dur, 4, 0.0)
    assert want["n_hits"] == 1 and (want["start"][0], want["end"][0]) == (s, e) and bits(want["score"][0]) == 0
    got = capi.tdt_kws([(lab, blk, dl, top)], dur, max_hits=4, min_score=0.0)
    same(got, 0, want, "planted")
    assert bits(got["score"][0][0]) == 0, "+0.0 with the sign bit clear"


def test_refusals_of_the_walk_alone():
    rng = np.random.default_rng(2)
    lat = R.make_lattice("ties", 3, 2, 2, rng)

    def refused(code, *a, **kw):
        with pytest.raises(capi.PkError) as e:
            capi.tdt_kws(*a, **kw)
        assert e.value.code == code, (code, e.value.code, str(e.value))

    refused(-7, [lat], [0, 9])                                      # a duration of 9
    refused(-7, [R.make_lattice("ties", 3, 2, 9, rng)], [1] * 9)    # D = 9
    refused(-7, [R.make_lattice("ties", 2, 65, 2, rng)], [0, 1])    # L = 65
    refused(-7, [lat], [0, 1], max_hits=0)
    refused(-7, [lat], [0, 1], max_hits=17)
    refused(-1, [lat], [0, 1], min_score=0.5)
    empty = (np.zeros((3, 0), np.float32), lat[1][:, :1], lat[2][:, :1], lat[3][:, :1])
    refused(-1, [empty], [0, 1])                                    # an empty keyword
