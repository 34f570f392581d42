"""CPU: the specification of the TDT forced alignment (tests/tdt_align_ref.py) against an enumeration of every path and its tie rule, against
the oracle model's own greedy path, and the argument checks of pk_tdt_align that need no device."""
import ctypes

import numpy as np
import pytest

from parakeet_cpp_amd import capi, synth

import tdt_align_ref as R

F = np.float32
NEG = F(-np.inf)
DURS = [[0, 1, 2, 3, 4], [0, 1], [1, 2, 4]]


def enumerate_paths(lab, blk, dl, dur):
    """Every path from (0, 0) to END -> list of (arcs [(t, u, code)], prefix sums after every arc): fp32, summed left to right, each arc's
    weight x + dl formed first."""
    T, U, D = blk.shape[0], blk.shape[1] - 1, len(dur)
    out = []

    def go(t, u, arcs, sums):
        acc = sums[-1] if sums else F(0.0)
        for i in range(D):
            nxt = t + max(int(dur[i]), 1)
            w = F(blk[t, u] + dl[t, u, i])
            a, s = arcs + [(t, u, i)], sums + [F(acc + w)]
            if nxt >= T:
                if u == U:
                    out.append((a, s))
            else:
                go(nxt, u, a, s)
        if u < U:
            for i in range(D):
                nxt = t + int(dur[i])
                w = F(lab[t, u] + dl[t, u, i])
                a, s = arcs + [(t, u, D + i)], sums + [F(acc + w)]
                if nxt >= T:
                    if u + 1 == U:
                        out.append((a, s))
                else:
                    go(nxt, u + 1, a, s)
    with np.errstate(all="ignore"):
        go(0, 0, [], [])
    return out


def tie_rule_path(paths, D):
    """Among the paths of maximal sum: the last arc first in END's order (source frame, blank before label, i); then, walking backwards, at
    every cell the prefixes of maximal sum, and among those the earliest incoming arc (blank i, then label i)."""
    best = max(p[1][-1] for p in paths)
    if not best > NEG:
        return NEG, None
    keep = [p for p in paths if p[1][-1] == best]
    key = min((a[-1][0], a[-1][2]) for a, _ in keep)
    keep = [p for p in keep if (p[0][-1][0], p[0][-1][2]) == key]
    back = 1                                                        # arcs fixed so far, counted from the end
    while True:
        keep = [p for p in keep if len(p[0]) >= back]
        heads = [p for p in keep if len(p[0]) == back]
        if heads:                                                   # the fixed suffix starts at (0, 0): every kept path is that path
            assert len(keep) == len(heads) == 1
            return best, heads[0][0]
        top = max(p[1][-back - 1] for p in keep)                    # the cell's alpha: the largest prefix sum that reaches it
        keep = [p for p in keep if p[1][-back - 1] == top]
        code = min(p[0][-back - 1][2] for p in keep)
        keep = [p for p in keep if p[0][-back - 1][2] == code]
        back += 1


@pytest.mark.parametrize("family", ["ties", "holes", "peaky"])
@pytest.mark.parametrize("dur", DURS, ids=lambda d: "d" + "".join(map(str, d)))
def test_reference_equals_the_enumeration_of_all_paths(dur, family):
    rng = np.random.default_rng(17 * len(dur) + len(family))
    D = len(dur)
    n_ok = n_tied = 0
    for T in range(1, 6):
        for U in range(0, 4):
            lab, blk, dl = R.make_lattice(family, T, U, D, rng)
            paths = enumerate_paths(lab, blk, dl, dur)
            want, arcs = tie_rule_path(paths, D) if paths else (NEG, None)
            r = R.align(lab, blk, dl, dur)
            assert r["ok"] == (0 if arcs is None else 1), (T, U)
            if arcs is None:
                assert r["score"] == NEG and not r["start"].any() and not r["end"].any() and not r["dur_idx"].any() and not r["conf"].any()
                continue
            n_ok += 1
            n_tied += sum(p[1][-1] == want for p in paths) > 1
            assert F(r["score"]).view(np.uint32) == F(want).view(np.uint32), (T, U, r["score"], want)
            score, got = R.best_path(lab, blk, dl, dur)
            assert got == arcs, (T, U, got, arcs)
            tok = [(t, u, c - D) for t, u, c in arcs if c >= D]
            assert [(int(r["start"][k]), k, int(r["dur_idx"][k])) for k in range(U)] == tok
            for t, k, i in tok:
                assert r["end"][k] == min(t + max(dur[i], 1) - 1, T - 1)
            assert np.all(r["start"][:-1] <= r["start"][1:])
    assert n_ok >= 8
    if family == "ties":
        assert n_tied >= 1, "the quantised family must produce ties between whole paths"


def test_more_tokens_than_frames_without_a_zero_duration_cannot_be_aligned():
    rng = np.random.default_rng(3)
    for T in (1, 4):
        lab, blk, dl = R.make_lattice("ties", T, T + 1, 3, rng)
        r = R.align(lab, blk, dl, [1, 2, 4])
        assert r["ok"] == 0 and r["score"] == NEG and not r["start"].any()
        assert R.align(*R.make_lattice("ties", T, T, 3, rng), [1, 2, 4])["ok"] == 1, "one token per frame fits"
        assert R.align(lab, blk, dl[:, :, :2], [0, 1])["ok"] == 1, "with a zero duration it can"


@pytest.mark.parametrize("dur", DURS + [[4, 0, 1, 1, 2, 8, 3, 5]], ids=lambda d: "d" + "".join(map(str, d)))
def test_empty_transcript_is_the_best_blank_chain(dur):
    rng = np.random.default_rng(11)
    T, D = 9, len(dur)
    _, blk, dl = R.make_lattice("ties", T, 0, D, rng)
    a = np.full(T + 1, NEG, np.float32)                             # a[t]: best chain of blanks from frame 0 to frame t; a[T] = END
    a[0] = 0.0
    for t in range(T):                                              # push form over the one column
        for i in range(D):
            n = min(t + max(dur[i], 1), T)
            a[n] = max(a[n], F(a[t] + F(blk[t, 0] + dl[t, 0, i])))
    r = R.align(np.zeros((T, 0), np.float32), blk, dl, dur)
    assert r["ok"] == 1 and F(r["score"]).view(np.uint32) == a[T].view(np.uint32) and len(r["start"]) == 0


@pytest.fixture(scope="module")
def tiny_oracle(orc):
    from conftest import pk
    cfg = pk.make_tiny_config()
    return cfg, orc.Model(cfg, synth.synth_weights(cfg, seed=42))


def greedy_arcs(cfg, g, T):
    """The oracle's greedy decisions as lattice arcs, or None when the walk is not a lattice path (max_symbols_per_step cut in)."""
    dur, D = list(cfg.durations), len(cfg.durations)
    t = u = 0
    arcs = []
    for lab, di in zip(g["labels"], g["dur_idx"]):
        if t >= T:
            return None
        if lab == cfg.blank_id:
            arcs.append((t, u, int(di))); t += max(dur[di], 1)
        else:
            arcs.append((t, u, D + int(di))); t += dur[di]; u += 1
    return arcs if t >= T else None


def test_aligning_the_oracles_own_greedy_transcript(tiny_oracle):
    cfg, om = tiny_oracle
    dur, D = list(cfg.durations), len(cfg.durations)
    n_equal = n_tokens = 0
    for seed, T in ((11, 24), (12, 17), (13, 9), (16, 4)):
        x = np.random.default_rng(seed).standard_normal((T, cfg.hidden_size)).astype(np.float32)
        enc = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
        g = om.tdt_score(enc)                                       # the greedy path, decision by decision
        ids = [int(v) for v in g["labels"] if v != cfg.blank_id]
        arcs = greedy_arcs(cfg, g, T)
        assert arcs is not None, "pick an input on which max_symbols_per_step does not cut in"
        lab, blk, dl = R.oracle_lattice(om, enc, ids)
        for k, (t, u, c) in enumerate(arcs):                        # the lattice holds the very values greedy saw
            x_ = lab[t, u] if c >= D else blk[t, u]
            assert F(x_).view(np.uint32) == F(g["label_lp"][k, g["labels"][k]]).view(np.uint32)
            assert np.array_equal(dl[t, u].view(np.uint32), g["dur_lp"][k].view(np.uint32))
        acc = F(0.0)
        for t, u, c in arcs:
            acc = F(acc + F((lab[t, u] if c >= D else blk[t, u]) + dl[t, u, c % D]))
        r = R.align(lab, blk, dl, dur)
        assert r["ok"] == 1 and r["score"] >= acc
        score, best = R.best_path(lab, blk, dl, dur)
        if best == arcs:
            assert F(score).view(np.uint32) == acc.view(np.uint32)
            n_equal += 1
        n_tokens += len(ids)
    assert n_tokens > 3, "degenerate test: nothing decoded"
    assert n_equal >= 2, "on two of these inputs greedy IS the best path: the equality must have been checked"


def test_entry_point_is_exported_and_checks_its_arguments_without_a_device():
    L = capi.lib()
    for name in ("pk_tdt_align", "pk_tdt_align_decode", "pk_tdt_align_decode_ragged", "pk_tdt_align_decode_timed", "pk_tdt_align_pcm",
                 "pk_diag_tdt_lattice"):
        assert hasattr(L, name), name
    lat = [R.make_lattice("ties", 3, 1, 2, np.random.default_rng(0))]
    z = np.zeros(8, np.float32)
    zi = np.zeros(2, np.int32)

    def call(dur, D, n_frames, B, off):
        lab, blk, dl = (np.ascontiguousarray(a.ravel()) for a in lat[0])
        return L.pk_tdt_align(capi._f(lab), capi._f(blk), capi._f(dl), capi._i(np.asarray(dur, np.int32)), D, capi._i(np.asarray(n_frames, np.int32)), B,
                              capi._i(np.asarray(off, np.int32)), capi._i(zi), capi._i(zi), capi._i(zi), capi._f(z), capi._f(z), capi._i(zi))
    assert call([0, 1], 2, [3], 0, [0, 1]) == -1                    # PK_ERR_INVALID: B < 1
    assert call([0, 1], 2, [3], 1, [0, -1]) == -1                   # offsets that decrease
    assert call([0, 1], 2, [0], 1, [0, 1]) == -1                    # no frames
    assert call([0, 9], 2, [3], 1, [0, 1]) == -7                    # PK_ERR_UNSUPPORTED: a duration past kTdtAlignMaxDur = 8
    assert call([0] * 9, 9, [3], 1, [0, 1]) == -7                   # D > 8
    assert call([0, 1], 2, [3], 1, [0, 1536]) == -7                 # more than kTdtAlignMaxTokens = 1535 tokens
    # the scratch cap, from the formula 4 (labs + cells (1 + D)) + cells <= 2^30 with cells = T (U + 1), labs = T U: T = 60000, U = 1500, D = 2
    T, U = 60000, 1500
    assert 4 * (T * U + T * (U + 1) * 3) + T * (U + 1) > 1 << 30
    assert call([0, 1], 2, [T], 1, [0, U]) == -7
    buf = ctypes.create_string_buffer(2048)
    L.pk_last_error(buf, 2048)
    assert b"cap" in buf.value
