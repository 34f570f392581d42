"""The three drivers of the greedy TDT / RNN-T decode loop (Model::run_tdt_loop, csrc/engine.cpp; pk_model_set_decode_loop) against the CPU oracle and against
each other, in every setting the loop runs in:
  "phases"      one launch per phase and step, the host polling "all finished" once per chunk of steps -- with the poll's copy enqueued two steps ahead;
  "graph"       the chunk captured once into a hipGraph and replayed -- by a key that must hold every argument the captured launches carry;
  "persistent"  the whole loop in one launch with grid barriers (kernels/decode_persist.hip).
Every driver is held to the oracle as tests/test_gpu_decode.py::check_tdt holds the default one (lens, steps, ids, start and end equal, confidences bit for bit),
and the drivers to each other on EVERY output word, the words behind `lens` included.  No tolerance anywhere: the drivers launch the same device code.  (The bf16
decode kernels are a tolerance-class mode against their oracle -- the statement of tests/test_gpu_bf16_decode_batch.py is repeated for them -- and bit-exact
between drivers.)

Where the engine does not run the driver that was asked for, the case says so: "persistent" runs the per-phase launches (without prediction-net caching) under
phrase boosting, with a carried streaming state and in the bf16 mode; "graph" runs everywhere here.  The equalities are asserted all the same.

A persistent kernel whose barrier times out reports lens = -1 (the entry point then fails): any -1 is a failure."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from test_gpu_bf16_decode_batch import agreement
from test_gpu_boost import phrases_from
from test_gpu_decode import _pair_with, enc_like

pytestmark = pytest.mark.gpu

WORDS = ("lens", "steps", "ids", "start", "end")
# the second "graph" call replays the graph the first one captured (same key)
LOOPS = ("phases", "graph", "graph", "persistent")


@pytest.fixture
def loop():
    """loop(gm, mode) sets a model's decode loop; every model it touched is back on "phases" afterwards."""
    touched = []

    def set_loop(gm, mode):
        if gm not in touched:
            touched.append(gm)
        gm.set_decode_loop(mode)

    try:
        yield set_loop
    finally:
        for gm in touched:
            gm.set_decode_loop("phases")


@pytest.fixture(scope="module")
def tiny_pair(tmp_path_factory):
    return G.make_pair(tmp_path_factory.mktemp("loops_tiny"), G.tiny())


def same_words(a, b, what):
    """every output word of two decodes, behind lens too"""
    for k in WORDS:
        if k in a:                                   # (a streaming chunk's result has no step counts)
            assert np.array_equal(a[k], b[k]), (what, k)
    G.assert_bits_equal(a["conf"], b["conf"], f"{what}: confidence")


def vs_oracle(g, o, what, keys=("ids", "start", "end")):
    """check_tdt of tests/test_gpu_decode.py on a finished decode"""
    assert (g["lens"] >= 0).all(), (what, "the loop hit its cap or the persistent kernel's barrier timed out", g["lens"])
    assert np.array_equal(g["lens"], o["lens"]), (what, g["lens"], o["lens"])
    if "steps" in o:
        assert np.array_equal(g["steps"], o["steps"]), (what, g["steps"], o["steps"])
    for b in range(len(o["lens"])):
        n = o["lens"][b]
        for k in keys:
            assert np.array_equal(g[k][b, :n], o[k][b, :n]), (what, k, b)
        G.assert_bits_equal(g["conf"][b, :n], o["conf"][b, :n], f"{what}: confidence of utterance {b}")


def run_loops(loop, gm, decode, modes=LOOPS):
    """-> [(mode, decode() under it)]"""
    out = []
    for mode in modes:
        loop(gm, mode)
        out.append((mode, decode()))
    loop(gm, "phases")
    return out


def hold(loop, gm, decode, o, what, modes=LOOPS, keys=("ids", "start", "end")):
    """every driver against the oracle's decode o, and against the first driver on every word"""
    runs = run_loops(loop, gm, decode, modes)
    for i, (mode, g) in enumerate(runs):
        vs_oracle(g, o, f"{what}: {mode} (call {i})", keys)
        same_words(runs[0][1], g, f"{what}: {runs[0][0]} vs {mode} (call {i})")
    return runs


def tdt_oracle(om, enc, **kw):
    o = om.tdt_greedy(enc, max_steps=0, **kw)
    assert not o["overflow"]
    return o


# ---- chunk geometry ---------------------------------------------------------------------------------------------------------------------------
# The host polls every `chunk` steps, chunk = T + 2 < 4 ? 4 : min(T + 2, 16): T = 1 -> 4; T = 2, 5, 6, 13 -> T + 2; T = 14, 57 -> 16.  The per-phase loop enqueues
# the poll's copy two steps before the chunk's end from chunk = 8 on (T >= 6).  B = 1 decodes through the frame window (F = 8), B = 3 without one.
# (T, B) -> a seed at which the oracle emits a token (and, from T = 5 on, takes a blank step), found on the CPU.
GEOMETRY = [(1, 1, 1003), (1, 3, 1002), (2, 1, 1002), (2, 3, 1002), (5, 1, 1002), (5, 3, 1001), (6, 1, 1002), (6, 3, 1001), (13, 1, 1001), (13, 3, 1000),
            (14, 1, 1001), (14, 3, 1000), (57, 1, 1000), (57, 3, 1000)]


@pytest.mark.parametrize("T,B,seed", GEOMETRY)
def test_chunk_geometry(tiny_pair, loop, T, B, seed):
    W, om, gm = tiny_pair
    enc = enc_like(B, T, om.cfg.hidden_size, seed)
    o = tdt_oracle(om, enc)
    assert o["lens"].sum() > 0, "degenerate case: the oracle emits nothing"
    assert T < 5 or (o["steps"] > o["lens"]).any(), "degenerate case: no blank step"
    hold(loop, gm, lambda: gm.tdt_decode(enc), o, f"T {T} B {B}")


# ---- where decoding ends in a chunk of 16 steps ------------------------------------------------------------------------------------------------
# Without a frame window (B = 3) the loop needs as many steps as its slowest utterance takes joint evaluations.  (T, seed, that count modulo 16): the batch is
# finished after the 14th step of a chunk (the step the early copy is enqueued behind), after the 15th and the 16th (which the early copy misses: the next chunk
# is enqueued whole), and after the first step of the next chunk.  Seeds found with the oracle on the CPU; its step counts then were
# [46 45 35], [31 31 30], [31 32 31] and [33 32 30].
CHUNK_ENDS = [(57, 2193, 14), (57, 2112, 15), (48, 3015, 0), (57, 2091, 1)]


@pytest.mark.parametrize("T,seed,residue", CHUNK_ENDS)
def test_decoding_ends_at_a_chunk_edge(tiny_pair, loop, T, seed, residue):
    W, om, gm = tiny_pair
    enc = enc_like(3, T, om.cfg.hidden_size, seed)
    o = tdt_oracle(om, enc)
    assert int(o["steps"].max()) % 16 == residue and o["steps"].max() > 16, ("the oracle changed: this is another case now", o["steps"])
    assert o["lens"].sum() > 0
    hold(loop, gm, lambda: gm.tdt_decode(enc), o, f"last step {o['steps'].max()} (residue {residue})")


# ---- token cap, long blank walks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_tokens", [1, 3])
def test_token_cap(tiny_pair, loop, max_tokens):
    """max_tokens below what the batch emits: the loop goes on to the end of every utterance (steps as uncapped), lens stop at the cap."""
    W, om, gm = tiny_pair
    enc = enc_like(5, 40, om.cfg.hidden_size, 77)
    assert (tdt_oracle(om, enc)["lens"] > max_tokens).all(), "degenerate case: the cap does not bind"
    o = tdt_oracle(om, enc, max_tokens=max_tokens)
    assert (o["lens"] == max_tokens).all() and (o["steps"] > 20).all()
    hold(loop, gm, lambda: gm.tdt_decode(enc, max_tokens=max_tokens), o, f"max_tokens {max_tokens}")


def test_all_blank_walk(tmp_path_factory, loop):
    """Weights pushed to blanks of duration 1 (the all-blank edit of test_single_utterance_frame_window): T decisions, no token -- the longest walk through the
    frame window (B = 1) and T steps of the lock-step loop (B = 3: the batch ends after step 57, the 9th of its chunk)."""
    def edit(W):
        W["tdt_joint_.label_proj_.bias"][-1] += 30.0
        W["tdt_joint_.duration_proj_.bias"][1] += 3.0

    om, gm = _pair_with(tmp_path_factory.mktemp("loops_blank"), G.tiny(name="tiny-loops-blank"), 21, edit)
    for B in (1, 3):
        enc = enc_like(B, 57, om.cfg.hidden_size, 40 + B)
        o = tdt_oracle(om, enc)
        assert (o["steps"] == 57).all() and o["lens"].sum() == 0, "the case is about blanks: the oracle must walk a blank per frame"
        hold(loop, gm, lambda: gm.tdt_decode(enc), o, f"all blank, B {B}")
        hold(loop, gm, lambda: gm.tdt_decode(enc, max_tokens=1), tdt_oracle(om, enc, max_tokens=1), f"all blank, B {B}, max_tokens 1")


# ---- heads and depth ------------------------------------------------------------------------------------------------------------------------------
def test_rnnt_head(tmp_path_factory, loop):
    """D = 0: no duration head.  The oracle's RNN-T decode reports ids, emission frames and confidences."""
    cfg = G.tiny(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("loops_rnnt"), cfg, seed=12)
    for B, T, seed in ((4, 50, 6), (1, 50, 7)):
        enc = enc_like(B, T, cfg.hidden_size, seed)
        o = om.rnnt_greedy(enc)
        assert o["lens"].sum() > 0
        hold(loop, gm, lambda: gm.tdt_decode(enc), o, f"rnnt B {B}", keys=("ids", "start"))


def test_two_lstm_layers(tmp_path_factory, loop):
    """P.cell[1]: the upper layer's fused input projection (X2 / W2 / bias2) under the graph and in the single launch."""
    cfg = G.tiny(num_lstm_layers=2, name="tiny2l")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("loops_2l"), cfg, seed=11)
    for B, T, seed in ((4, 60, 5), (1, 30, 8)):
        enc = enc_like(B, T, cfg.hidden_size, seed)
        o = tdt_oracle(om, enc)
        assert o["lens"].sum() > 0 and (o["steps"] > o["lens"]).all()
        hold(loop, gm, lambda: gm.tdt_decode(enc), o, f"two LSTM layers B {B}")


def test_110m_decoder_shapes(tmp_path_factory, loop):
    """The 110m decoder (Hp = J = 640: the K = 640 products, tdt_persistent_kernel<10>, vocabulary 1025) on one encoder layer."""
    cfg = dataclasses.replace(pk.make_110m_config(), num_layers=1, name="110m-1L-persist")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("loops_110m"), cfg, seed=9)
    enc = enc_like(16, 40, cfg.hidden_size, 3)
    o = tdt_oracle(om, enc)
    assert o["lens"].sum() > 16 and (o["steps"] > o["lens"]).all()
    hold(loop, gm, lambda: gm.tdt_decode(enc), o, "110m decoder")


# ---- ragged batches ----------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batches_and_changed_tables(tiny_pair, loop):
    """A packed batch of five lengths, then the same lengths in another order: same B, same longest utterance, same row total -- every pointer the loop is given
    stays, the frame-count and first-row tables behind two of them change.  A replayed graph must read the new tables.  Then the first batch again."""
    W, om, gm = tiny_pair
    rng = np.random.default_rng(5)

    def batch(lengths):
        xs = []
        for t in lengths:
            x = rng.standard_normal((t, om.cfg.hidden_size)).astype(np.float32)
            xs.append((x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True))
        want = [tdt_oracle(om, x[None]) for x in xs]
        mt = max(lengths) * om.cfg.max_symbols_per_step
        o = dict(lens=np.array([w["lens"][0] for w in want]), steps=np.array([w["steps"][0] for w in want]))
        for k in ("ids", "start", "end", "conf"):
            o[k] = np.stack([w[k][0, :].tolist() + [0] * (mt - w[k].shape[1]) for w in want]).astype(want[0][k].dtype)
        return xs, o

    xa, oa = batch([40, 1, 13, 57, 2])
    xb, ob = batch([2, 57, 40, 13, 1])
    assert oa["lens"].sum() > 5 and ob["lens"].sum() > 5 and not np.array_equal(oa["steps"], ob["steps"])
    runs = []
    for mode in ("phases", "graph", "persistent"):
        loop(gm, mode)
        runs.append((mode, [gm.tdt_decode_ragged(xs) for xs in (xa, xb, xa)]))
    loop(gm, "phases")
    for mode, rs in runs:
        for i, (g, o) in enumerate(zip(rs, (oa, ob, oa))):
            vs_oracle(g, o, f"ragged, {mode}, call {i}")
            same_words(runs[0][1][i], g, f"ragged call {i}: phases vs {mode}")


# ---- the bf16 decode kernels ---------------------------------------------------------------------------------------------------------------------------
def test_bf16_decode(tmp_path_factory, loop):
    """kernels/decode_gemv_bf16.hip under the graph: bit for bit what the per-phase launches give.  "persistent" exists for the fp32 phases only: in this mode it
    runs the per-phase launches over every row (no prediction-net caching), which is specified as bit-exact too.  Against the bf16 oracle: the statement of
    tests/test_gpu_bf16_decode_batch.py (a tolerance-class mode: agreement >= 0.95 of every utterance's tokens)."""
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("loops_b16"), cfg, seed=5)
    enc = enc_like(13, 40, cfg.hidden_size, 31)
    o = tdt_oracle(om, enc)
    assert o["lens"].sum() > 10 and (o["steps"] > o["lens"]).any()
    runs = run_loops(loop, gm, lambda: gm.tdt_decode(enc))
    for i, (mode, g) in enumerate(runs):
        assert (g["lens"] >= 0).all()
        same_words(runs[0][1], g, f"bf16: phases vs {mode} (call {i})")
    g = runs[0][1]
    for b in range(13):
        assert agreement(g["ids"][b, : g["lens"][b]].tolist(), o["ids"][b, : o["lens"][b]].tolist()) >= 0.95, b


# ---- phrase boosting under the graph -----------------------------------------------------------------------------------------------------------------------
def test_boost_changes_between_graph_decodes(tiny_pair, orc, loop):
    """One model, one (B, T) batch, the phrase trie changing between decodes: the captured launches carry the trie record and the boost score by value, so every
    change must lead to a new capture.  Under boosting "persistent" runs the per-phase launches (no prediction-net caching)."""
    W, om, gm = tiny_pair
    V, blank = om.cfg.vocab_size, om.cfg.blank_id
    enc = enc_like(6, 48, om.cfg.hidden_size, 4)
    u = tdt_oracle(om, enc)
    ph = phrases_from(u, np.random.default_rng(5), V, blank)
    rng = np.random.default_rng(6)
    other = [p[:-1] + [int((p[-1] + 1 + rng.integers(0, V - 2)) % (V - 1))] for p in ph]       # the same phrases with another last token: same token count
    big = phrases_from(u, np.random.default_rng(7), V, blank, n_random=80)
    assert sum(map(len, other)) == sum(map(len, ph)) and orc.Trie(big).size() >= 4 * orc.Trie(ph).size()

    def toks(o):
        return [o["ids"][b, : o["lens"][b]].tolist() for b in range(6)]

    def boosted(phrases, score):
        o = om.tdt_greedy_boosted(enc, orc.Trie(phrases), score)
        assert not o["overflow"]
        return o

    plan = [("unboosted", [], 0.0, u), ("phrases at 5.0", ph, 5.0, boosted(ph, 5.0)), ("the same phrases at 0.75", ph, 0.75, boosted(ph, 0.75)),
            ("other phrases", other, 5.0, boosted(other, 5.0)), ("a larger trie", big, 5.0, boosted(big, 5.0)), ("boosting off", [], 0.0, u)]
    assert u["lens"].sum() > 0
    assert toks(plan[1][3]) != toks(u) and toks(plan[1][3]) != toks(plan[2][3]), "degenerate case: a stale score would pass"
    assert toks(plan[3][3]) != toks(plan[1][3]) and toks(plan[4][3]) != toks(plan[1][3]), "degenerate case: a stale trie would pass"
    try:
        for what, phrases, score, o in plan:
            gm.set_boost_tokens(phrases, score)
            hold(loop, gm, lambda: gm.tdt_decode(enc), o, what, modes=("graph", "graph", "phases", "persistent"))
    finally:
        gm.set_boost_tokens([])


# ---- other work on the workspace between two graph decodes ------------------------------------------------------------------------------------------------
def test_graph_after_other_calls_grew_the_decode_buffers(tmp_path_factory, loop):
    """The beam search and the forced alignment use the greedy loop's z / pp / logits buffers and grow them for their own, larger batches: the graph captured
    before holds pointers into the buffers they replaced.  A fresh model, so that the buffers start at their smallest."""
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("loops_reuse"), G.tiny(name="tiny-loops-reuse"))
    d = om.cfg.hidden_size
    ea, eb = enc_like(3, 30, d, 61), enc_like(8, 30, d, 62)
    oa, ob = tdt_oracle(om, ea), tdt_oracle(om, eb)
    assert oa["lens"].sum() > 0 and ob["lens"].sum() > 0
    wide = enc_like(16, 60, d, 63)
    loop(gm, "graph")
    vs_oracle(gm.tdt_decode(ea), oa, "first graph decode")
    assert gm.tdt_beam_decode(wide, 8, 8, 2, 4)["ok"].all()
    vs_oracle(gm.tdt_decode(ea), oa, "after the beam search")
    assert len(gm.tdt_align_decode(wide, [[1, 2, 3, 4, 5, 6]] * 16)) == 16
    vs_oracle(gm.tdt_decode(ea), oa, "after the forced alignment")
    vs_oracle(gm.tdt_decode(eb), ob, "a larger batch")
    vs_oracle(gm.tdt_decode(ea), oa, "the first batch again")
    loop(gm, "phases")
    vs_oracle(gm.tdt_decode(ea), oa, "per-phase loop")


# ---- streaming chunks: carried state, the result copies riding on the poll ---------------------------------------------------------------------------------
def test_streaming_chunks(tmp_path_factory, orc, loop):
    """Two lock-step streams, chunks of 1 .. 14 encoder frames through pk_stream_decode (keep_state, Workspace::before_poll) with the model's loop on each driver:
    the tokens, frames and confidences of the oracle's streaming decode (tests/test_gpu_stream.py), chunk by chunk, and every word the same between drivers.
    A chunk of another length is another graph; two chunks of one length in a row replay one.  With a carried state "persistent" runs the per-phase launches.
    The model: the tiny one with the blank's bias lowered, so that chunks of a few frames emit tokens."""
    def edit(W):
        W["tdt_joint_.label_proj_.bias"][-1] -= 1.0

    from parakeet_cpp_amd import capi
    om, gm = _pair_with(tmp_path_factory.mktemp("loops_stream"), G.tiny(name="tiny-loops-stream"), 42, edit)
    S, sched = 2, [2, 2, 1, 3, 5, 14, 14, 2, 1, 7]
    chunks = [enc_like(S, c, om.cfg.hidden_size, 300 + i) for i, c in enumerate(sched)]
    os_ = [orc.Stream(om, 10, 1) for _ in range(S)]
    want = [[os_[s].decode(e[s]) for s in range(S)] for e in chunks]
    assert sum(len(r["ids"]) for rs in want for r in rs) > 10, "degenerate case: the streams emit nothing"
    got = {}
    for mode in ("phases", "graph", "persistent"):
        loop(gm, mode)
        gs = capi.Stream(gm, S, 10, 1)
        try:
            got[mode] = [gs.decode(e) for e in chunks]
        finally:
            gs.close()
    loop(gm, "phases")
    for mode, rs in got.items():
        for i, (g, ws) in enumerate(zip(rs, want)):
            for s, r in enumerate(ws):
                n = len(r["ids"])
                assert g["lens"][s] == n, (mode, i, s, g["lens"][s], n)
                for k in ("ids", "start", "end"):
                    assert np.array_equal(g[k][s, :n], r[k]), (mode, i, s, k)
                G.assert_bits_equal(g["conf"][s, :n], r["conf"], f"{mode}, chunk {i}, stream {s}: confidence")
            same_words(got["phases"][i], g, f"chunk {i}: phases vs {mode}")
