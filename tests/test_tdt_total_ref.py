"""CPU: the specification of the TDT forward-algorithm total and of the rescored n-best ordering (tests/tdt_total_ref.py) against an enumeration of
every path, against its own float64 form, against the alignment on the same lattice, and the host-side parts of the library (the ordering rule,
the grouping of hypotheses, the argument checks of pk_tdt_total) that need no device."""
import ctypes

import numpy as np
import pytest

from parakeet_cpp_amd import capi

import tdt_align_ref as A
import tdt_total_ref as R

F = np.float32
NEG = F(-np.inf)


def all_path_sums(lab, blk, dl, dur):
    """The float64 log-weight of every path from (0, 0) to END."""
    lab, blk, dl = (np.asarray(a, np.float64) for a in (lab, blk, dl))
    T, U, D = blk.shape[0], blk.shape[1] - 1, len(dur)
    out = []

    def go(t, u, acc):
        for i in range(D):
            nxt, s = t + max(int(dur[i]), 1), acc + (blk[t, u] + dl[t, u, i])
            if nxt >= T:
                if u == U:
                    out.append(s)
            else:
                go(nxt, u, s)
        if u < U:
            for i in range(D):
                nxt, s = t + int(dur[i]), acc + (lab[t, u] + dl[t, u, i])
                if nxt >= T:
                    if u + 1 == U:
                        out.append(s)
                else:
                    go(nxt, u + 1, s)
    go(0, 0, 0.0)
    return out


@pytest.mark.parametrize("dur", [[0, 1, 2], [1, 2], [0, 1]], ids=lambda d: "d" + "".join(map(str, d)))
def test_float64_total_equals_the_sum_over_every_path(dur):
    rng = np.random.default_rng(5 + len(dur) + dur[0])
    n_paths = 0
    for T in range(1, 5):
        for U in range(0, 3):
            lat = A.make_lattice("peaky", T, U, len(dur), rng)
            sums = all_path_sums(*lat, dur)
            got = R.forward_total64(*lat, dur)
            if not sums:
                assert got == -np.inf, (T, U)
                continue
            want = np.logaddexp.reduce(np.asarray(sums, np.float64))
            assert abs(got - want) <= 1e-12, (T, U, got, want)
            n_paths += len(sums)
    assert n_paths > 100
    # a blank of duration 0 and a blank of duration 1 are two arcs to t + 1: one frame, no tokens, durations [0, 1] -> two paths, both summed
    if dur == [0, 1]:
        _, blk, dl = A.make_lattice("peaky", 1, 0, 2, rng)
        want = np.logaddexp(np.float64(blk[0, 0]) + np.float64(dl[0, 0, 0]), np.float64(blk[0, 0]) + np.float64(dl[0, 0, 1]))
        assert abs(R.forward_total64(np.zeros((1, 0)), blk, dl, dur) - want) <= 1e-12


# fp32 against float64 on the shapes of tests/test_gpu_tdt_total.py.  Measured over all of them (this test's own loop, the assertion replaced by a
# maximum): the largest |fp32 - float64| is 0.015640545 (T = 3, U = 1534, eight durations, "peaky": a total of -21895.76, where one fp32 ulp is
# 0.00195 -- a chain of ~1500 log-adds and adds at that magnitude sets the distance, not the kernel).  The bound is 4 x that value.
FP32_MEASURED = 0.015640545
FP32_BOUND = 4 * FP32_MEASURED


def fp32_close(lat, dur, what):
    a, b = R.forward_total(*lat, dur), R.forward_total64(*lat, dur)
    if not np.isfinite(b):
        assert b == -np.inf and a == NEG, what
        return False
    assert abs(float(a) - b) <= FP32_BOUND, (what, a, b)
    return True


def test_fp32_total_against_float64_small_and_ragged_shapes():
    n = 0
    for T, U in R.SMALL:
        for dn in R.DURS:
            for fam in R.FAMILIES:
                for k, lat in enumerate(R.small_lattices(T, U, dn, fam)):
                    n += fp32_close(lat, R.DURS[dn], (T, U, dn, fam, k))
    for k, lat in enumerate(R.ragged_lattices()):
        n += fp32_close(lat, R.DURS["d124"], ("ragged", k))
    assert n > 150


@pytest.mark.parametrize("T,U,dname,family", R.BOUNDARY)
def test_fp32_total_against_float64_boundary_shapes(T, U, dname, family):
    assert fp32_close(R.boundary_lattice(T, U, dname, family), R.DURS[dname], (T, U, dname, family)), "a boundary case has a finite total"


@pytest.mark.parametrize("family", R.FAMILIES)
def test_total_bounds_the_alignment_and_agrees_on_reachability(family):
    n_ok = n_not = 0
    for dn, dur in R.DURS.items():
        for T, U in R.SMALL + [(4, 5), (12, 12), (20, 7)]:
            for k, lat in enumerate(R.small_lattices(T, U, dn, family)):
                al, tot = A.align(*lat, dur), R.total(*lat, dur)
                assert tot["ok"] == al["ok"], (dn, T, U, k)            # the same arcs: neither is reachable alone
                if al["ok"]:
                    assert tot["total"] >= al["score"], (dn, T, U, k, tot["total"], al["score"])
                    n_ok += 1
                else:
                    assert tot["total"] == NEG
                    n_not += 1
    assert n_ok > 50
    if family == "holes":
        assert n_not >= 1, "the family with -inf entries must produce unreachable cases"


# ---- the ordering rule ------------------------------------------------------------------------------------------------------------------
def beam_slots(rng, N, n_filled, n_bad, ties=False):
    """N slots in beam order: n_filled filled (CTC scores descending), the last n_bad of them not scorable by the TDT head, the rest unfilled."""
    ctc = np.full(N, NEG, np.float32); tdt = np.full(N, NEG, np.float32)
    lens = np.zeros(N, np.int32); ok = np.zeros(N, np.int32)
    vals = (lambda n: -rng.integers(1, 4, size=n).astype(np.float32)) if ties else (lambda n: -rng.random(n).astype(np.float32) * 30)
    ctc[:n_filled] = np.sort(vals(n_filled))[::-1]
    lens[:n_filled] = rng.integers(0, 9, size=n_filled)                # (a filled slot may hold the empty hypothesis)
    good = n_filled - n_bad
    tdt[:good] = vals(good); ok[:good] = 1
    return lens, ctc, tdt, ok


@pytest.mark.parametrize("w", [0.0, 0.3, 0.5, 1.0])
def test_ordering_rule_and_its_host_implementation(w):
    rng = np.random.default_rng(int(w * 10) + 1)
    for N, nf, nb, ties in [(1, 1, 0, False), (4, 4, 0, False), (4, 3, 1, False), (8, 5, 2, True), (8, 8, 0, True), (8, 0, 0, False), (6, 6, 6, False),
                            (32, 20, 3, True)]:
        lens, ctc, tdt, ok = beam_slots(rng, N, nf, nb, ties)
        order, comb = R.rescore_order(lens, ctc, tdt, ok, w)
        assert sorted(order) == list(range(N))
        good = nf - nb
        assert sorted(order[:good]) == list(range(good)), "scored hypotheses first"
        assert order[good:nf] == list(range(good, nf)), "then the unscored ones in beam order"
        assert order[nf:] == list(range(nf, N)), "unfilled slots stay last"
        for a, b in zip(order[:good], order[1:good]):
            assert comb[a] > comb[b] or (comb[a] == comb[b] and a < b), "descending, ties keep the beam's order"
        for j in range(good):
            want = F(F(F(F(1.0) - F(w)) * ctc[j]) + F(F(w) * tdt[j]))
            assert comb[j].view(np.uint32) == want.view(np.uint32)
        assert np.all(comb[good:] == NEG)
        if w == 0.0:
            assert order == list(range(N)), "weight 0: the beam's own order"
            assert np.array_equal(comb[:good], ctc[:good])
        if w == 1.0:
            assert order[:good] == sorted(range(good), key=lambda j: (-tdt[j], j)), "weight 1: by the TDT total"
        got_order, got_comb = capi.rescore_order(lens, ctc, tdt, ok, w)
        assert got_order == order and np.array_equal(got_comb.view(np.uint32), comb.view(np.uint32)), "the library's host rule"
    with pytest.raises(capi.PkError) as e:
        capi.rescore_order([1], [-1.0], [-1.0], [1], float("nan"))
    assert e.value.code == -1


# ---- host side of the library ---------------------------------------------------------------------------------------------------------------
def test_grouping_of_hypotheses_is_host_arithmetic():
    dur, V, J = [0, 1, 2, 3, 4], 1025, 640
    g, n = capi.tdt_total_groups([126] * 600, [30] * 600, dur, V, J)
    assert n == 3 and g.tolist() == [0] * 256 + [1] * 256 + [2] * 88, "at most 256 hypotheses walk together"
    g, n = capi.tdt_total_groups([126] * 5, [30, 0, 1, 7, 30], dur, V, J, max_hyps=2)
    assert g.tolist() == [0, 0, 1, 1, 2] and n == 3
    # the scratch cap cuts a group: 4 (labs + cells (1 + D)) per hypothesis of T = 3000, U = 1500, D = 5 is 126 MB (+ chunk and prediction net)
    T, U = 3000, 1500
    one = 4 * (T * U + T * (U + 1) * 6)
    g, n = capi.tdt_total_groups([T] * 20, [U] * 20, dur, V, J)
    per = int(np.bincount(g).max())
    chunk = min(65536, max(128, (256 << 20) // ((V + 5) * 4) // 128 * 128))                       # rows of one heads product
    scratch = lambda k: k * one + chunk * (V + 5 + J) * 4 + (U + 1) * k * (J + 1) * 4
    assert n > 1 and scratch(per) <= 1 << 30 < scratch(per + 1), (per, n)
    assert np.all(np.diff(g) >= 0) and g[0] == 0 and g[-1] == n - 1
    for bad in (dict(n_frames_of_hyp=[30000], lengths=[1500]), dict(n_frames_of_hyp=[10], lengths=[1536])):
        with pytest.raises(capi.PkError) as e:
            capi.tdt_total_groups(durations=dur, V=V, J=J, **bad)
        assert e.value.code == -7
    with pytest.raises(capi.PkError) as e:
        capi.tdt_total_groups([10], [3], [0, 9], V, J)
    assert e.value.code == -7


def test_entry_points_are_exported_declared_and_check_their_arguments_without_a_device():
    import os
    import re
    from conftest import ROOT
    L = capi.lib()
    names = ("pk_tdt_total", "pk_tdt_total_decode", "pk_tdt_total_decode_ragged", "pk_tdt_total_decode_timed", "pk_tdt_score_pcm",
             "pk_transcribe_pcm_nbest_rescored", "pk_diag_tdt_total_groups", "pk_diag_rescore_order")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "parakeet_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", txt))
    for name in names:
        assert hasattr(L, name) and name in declared, name
    assert "pk_rescore_options" in txt
    lat = A.make_lattice("ties", 3, 1, 2, np.random.default_rng(0))
    z, zi = np.zeros(2, np.float32), np.zeros(2, np.int32)

    def call(dur, D, n_frames, B, off):
        lab, blk, dl = (np.ascontiguousarray(a.ravel()) for a in lat)
        return L.pk_tdt_total(capi._f(lab), capi._f(blk), capi._f(dl), capi._i(np.asarray(dur, np.int32)), D, capi._i(np.asarray(n_frames, np.int32)), B,
                              capi._i(np.asarray(off, np.int32)), capi._f(z), capi._i(zi))
    assert call([0, 1], 2, [3], 0, [0, 1]) == -1                    # PK_ERR_INVALID: B < 1
    assert call([0, 1], 2, [3], 1, [0, -1]) == -1                   # offsets that decrease
    assert call([0, 1], 2, [0], 1, [0, 1]) == -1                    # no frames
    assert call([0, 9], 2, [3], 1, [0, 1]) == -7                    # PK_ERR_UNSUPPORTED: a duration past 8
    assert call([0] * 9, 9, [3], 1, [0, 1]) == -7                   # D > 8
    assert call([0, 1], 2, [3], 1, [0, 1536]) == -7                 # more than 1535 tokens
    T, U = 60000, 1500                                              # the scratch cap without back-pointer bytes: 4 (labs + cells (1 + D)) > 2^30
    assert 4 * (T * U + T * (U + 1) * 3) > 1 << 30
    assert call([0, 1], 2, [T], 1, [0, U]) == -7
    buf = ctypes.create_string_buffer(2048)
    L.pk_last_error(buf, 2048)
    assert b"cap" in buf.value
