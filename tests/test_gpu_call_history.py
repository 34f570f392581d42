"""One model with a HISTORY of calls against models without one: the state a Model carries from call to call.

Almost every other GPU test builds a model, makes one call (or several of one shape) and compares.  A service keeps one model for hours and sends it
clips of every length, and the engine keeps between calls
  * the relative-position tables (Model::ensure_pos_tables, csrc/engine.cpp): built for the LONGEST sequence seen so far; a shorter sequence, and every
    utterance of a ragged batch, reads a window of them (pos_T > T).  Two sets side by side: the fp32 kernel's and the bf16 attention's;
  * the workspace buffers (Workspace::size_for / size_decode / size_ragged / set_uniform / set_ragged): grown, then serving smaller calls; the ragged tables
    of the last packed batch;
  * toggles: the decode loop driver, phrase boosting, the attention context, whatever a fused LM search left in the decode buffers.
A bug in any of these gives a wrong result only for a clip that FOLLOWS a particular other clip.

The reference of every fp32 assertion is the CPU oracle, which has no history: bit for bit (G.assert_bits_equal), no tolerance.  The bf16 mode is compared
(a) with the bf16-mode oracle within close() of tests/test_gpu_bf16.py and (b) BIT FOR BIT with a fresh model that is given only that one call -- the
assertion that holds ensure_pos_tables' claim "a row of the window is the row a table built for T would hold".  Every history asserts
Model.pos_table_frames() (pk_diag_pos_table_frames) after every call: it grows on a longer call and stays on a shorter one, so a shorter call demonstrably
ran with pos_T > T; a sequence that stops doing so fails instead of passing vacuously.

What (b) rests on.  The claim needs the pos_proj product to give a row the same bits whatever M = 2 T - 1 is, although run_gemm picks the kernel by M:
  * fp32: the small-M family up to 1536 rows, the tile family above -- one k-ordered chain per element in both.
    test_fp32_table_built_by_the_tile_family_serves_a_small_m_length holds across that switch (taken from pk_diag_gemm_tile_form);
  * bf16 mode: the small-M bf16 kernel takes up to 128 rows when K % 256 == 0, the tile kernels the rest.  The tiny config (hidden size 128) never reaches the
    small-M bf16 kernel, so its histories cannot see that switch.  From K = 512 on that kernel splits K over its waves and adds the partial sums afterwards,
    which is not the tile kernels' sum: test_bf16_table_rows_have_one_form_at_every_m runs both on the table's own sinusoid rows, asserts that they DO differ
    (so the rule below is needed) and prints how many fp32 sums and how many bf16 table elements do.  ensure_pos_tables therefore builds the table with
    GemmArgs::one_form -- the 64 x 64 tile at every M -- and the same test holds the rows of 127-, 129- and 1025-row tables to each other bit for bit.
    test_bf16_table_across_the_small_m_switch is the engine-level statement: the tiny config at hidden size 512, where 2 T - 1 = 127 / 129 straddles the
    switch (taken from pk_diag_gemm_smallm_bf16_form), a 64-frame clip after a 65-frame one against the same clip on a fresh model.

Sequences are at most 257 encoder frames (mel features of 8 T - 7 frames give T encoder frames), except the fp32 switch, which sits at 1536 table rows
(T = 768 / 769, one clip each).  Each model here is built for its test (a name of its own in gpu_common's cache: a shared model's tables are as long as the
longest clip any earlier test sent) and is closed, and taken out of that cache, when the module is done.

Out of scope: the one-call API's token-array shrink rule across calls (needs a slot above 64 MB), the switch back from the bf16 attention to the fp32 one
(needs tens of thousands of frames) and the thread safety of the lazy sigma_weights()."""
import dataclasses
import os

import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi
from test_gpu_bf16 import close
from test_gpu_decode import enc_like

pytestmark = pytest.mark.gpu

HISTORY = [5, 130, 33, 257, 1, 129, 257, 2]          # encoder frames per call, B alternating 1 and 3
AFTER_A_GROWTH = (33, 1, 129, 2)                     # the calls a fresh model is built for in the bf16 mode: each reads a window of a longer table
LOOPS = ("phases", "graph", "persistent")


_MINE = []                                           # the models this module built


@pytest.fixture(scope="module", autouse=True)
def close_models():
    """the models of this module leave the device, and gpu_common's cache, with it"""
    yield
    for gm in _MINE:
        gm.close()
    for k in [k for k, v in G._CACHE.items() if v[2] in _MINE]:
        del G._CACHE[k]
    _MINE.clear()


def pair(tmp_path_factory, cfg, seed=42):
    """(weights, weights path, oracle model, a product model no other test has called)"""
    tmp = tmp_path_factory.mktemp("hist")
    assert cfg.name.startswith("tiny-") and "history" in cfg.name, "gpu_common keys its cache by name, not by every size: a name of this module's own"
    W, om, gm = G.make_pair(tmp, cfg, seed=seed)
    _MINE.append(gm)
    wp = os.path.join(str(tmp), f"{cfg.name}_{cfg.num_layers}_{seed}.safetensors")
    assert os.path.exists(wp) and gm.pos_table_frames() == (0, 0), "the model of a history test must be new"
    return W, wp, om, gm


def feats_of(seed, B, T, bins=80):
    """mel features that give T encoder frames"""
    return np.random.default_rng(seed).standard_normal((B, 8 * T - 7, bins)).astype(np.float32)


def tables(gm, bf16, T, what):
    """the table set of this mode was built for T frames, the other one never"""
    assert gm.pos_table_frames() == ((0, T) if bf16 else (T, 0)), (what, gm.pos_table_frames())


def fresh_run(wp, cfg, call, T_built):
    """call(model) on a model that has seen nothing else; its table is as long as that call needs"""
    fresh = capi.Model(wp, cfg, device=0)
    try:
        out = call(fresh)
        tables(fresh, True, T_built, "fresh model")
    finally:
        fresh.close()
    return out


# ---- 1. fp32: against the oracle, bit for bit ------------------------------------------------------------------------------------------------------
def test_fp32_growing_and_shrinking_sequences(tmp_path_factory):
    W, wp, om, gm = pair(tmp_path_factory, G.tiny(name="tiny-history-fp32"))
    longest = 0
    for i, T in enumerate(HISTORY):
        B = 1 if i % 2 == 0 else 3
        feats = feats_of(100 + i, B, T)
        got = gm.encode(feats)
        assert got.shape == (B, T, om.cfg.hidden_size)
        longest = max(longest, T)
        tables(gm, False, longest, f"call {i} (T = {T})")
        G.assert_bits_equal(got, om.encoder(feats), f"call {i}: B = {B}, T = {T}, table built for {longest}")
    assert longest > HISTORY[-1], "the last calls must read a window"


# (lengths of a packed batch, or one length and a batch size for a uniform call): a packed batch shorter than the table, a uniform call right after it, a
# packed batch that grows the table, a uniform call right after it, a packed batch shorter than the table again, the shortest uniform call
RAGGED_HISTORY = [(130, 1), [33, 5, 1, 64, 2], (33, 3), [257, 7, 130, 1], (129, 1), [129, 2, 40], (2, 3)]


def ragged_feats(seed, lengths):
    return [feats_of(seed + j, 1, t)[0] for j, t in enumerate(lengths)]


def test_fp32_ragged_batches_between_uniform_calls(tmp_path_factory):
    W, wp, om, gm = pair(tmp_path_factory, G.tiny(name="tiny-history-fp32-ragged"))
    longest, windows = 0, 0
    for i, call in enumerate(RAGGED_HISTORY):
        if isinstance(call, list):
            fl = ragged_feats(200 + 10 * i, call)
            got = gm.encode_ragged(fl)
            windows += max(call) < longest
            longest = max(longest, max(call))
            tables(gm, False, longest, f"call {i} (ragged {call})")
            for j, f in enumerate(fl):
                G.assert_bits_equal(got[j], om.encoder(f[None])[0], f"call {i}: clip {j} ({call[j]} frames) of a packed batch, table built for {longest}")
        else:
            T, B = call
            feats = feats_of(200 + 10 * i, B, T)
            got = gm.encode(feats)
            longest = max(longest, T)
            tables(gm, False, longest, f"call {i} (T = {T})")
            G.assert_bits_equal(got, om.encoder(feats), f"call {i}: B = {B}, T = {T}, table built for {longest}")
    assert windows == 2, "two packed batches must run with rag.pos_T > T_max"


def fp32_switch():
    """(T_lo, T_hi): 2 T_lo - 1 rows are the longest table the small-M family builds, 2 T_hi - 1 the shortest one of the tile family -- by asking
    pk_diag_gemm_tile_form, which refuses (PK_ERR_UNSUPPORTED) the shapes launch_gemm sends to the small-M kernels"""
    d = G.tiny().hidden_size

    def tile(M):
        try:
            capi.diag_gemm_tile_form(M, d, d)
            return True
        except capi.PkError as e:
            assert e.code == -7
            return False
    assert not tile(1) and tile(1 << 16)
    lo, hi = 1, 1 << 16                                               # not tile(lo), tile(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if tile(mid) else (mid, hi)
    T_lo = (lo + 1) // 2
    assert not tile(2 * T_lo - 1) and tile(2 * T_lo + 1)
    return T_lo, T_lo + 1


def test_fp32_table_built_by_the_tile_family_serves_a_small_m_length(tmp_path_factory):
    """The fp32 pos_proj product changes its kernel FAMILY with the table's rows: a model that first sees T_hi builds the table on the tile kernels and serves
    T_lo from a window of it, a fresh model builds the table for T_lo on the small-M kernel.  Same bits, and the oracle's."""
    cfg = G.tiny(name="tiny-history-fp32-switch")
    W, wp, om, gm = pair(tmp_path_factory, cfg)
    T_lo, T_hi = fp32_switch()
    f_hi, f_lo = feats_of(31, 1, T_hi), feats_of(32, 1, T_lo)
    G.assert_bits_equal(gm.encode(f_hi), om.encoder(f_hi), f"T = {T_hi}: the table on the tile kernels")
    tables(gm, False, T_hi, "after the long call")
    got = gm.encode(f_lo)
    tables(gm, False, T_hi, "after the short call")
    fresh = capi.Model(wp, cfg, device=0)
    try:
        alone = fresh.encode(f_lo)
        tables(fresh, False, T_lo, "fresh model")
    finally:
        fresh.close()
    G.assert_bits_equal(got, alone, f"T = {T_lo}: a window of the table built for {T_hi} vs a fresh model's table")
    G.assert_bits_equal(got, om.encoder(f_lo), f"T = {T_lo}: a window of the table built for {T_hi} vs the oracle")


# ---- 2. bf16 mode: the bf16 oracle within close(), a fresh model bit for bit ---------------------------------------------------------------------------
def bf16_cfg(**kw):
    return G.tiny(subsampling_channels=64, gemm_bf16=True, **kw)      # the config of tests/test_gpu_bf16.py: every GEMM K a multiple of 64


def test_bf16_growing_and_shrinking_sequences(tmp_path_factory, orc):
    cfg = bf16_cfg(name="tiny-bf16-history")
    W, wp, om, gm = pair(tmp_path_factory, cfg, seed=5)
    longest, held = 0, 0
    for i, T in enumerate(HISTORY):
        B = 1 if i % 2 == 0 else 3
        feats = feats_of(300 + i, B, T)
        got = gm.encode(feats)
        window = T < longest
        longest = max(longest, T)
        tables(gm, True, longest, f"call {i} (T = {T})")
        oenc = om.encoder(feats)
        close(got, oenc, f"call {i}: B = {B}, T = {T}, table built for {longest}")
        if i == 1:                                                    # (the sanity assertion of tests/test_gpu_bf16.py, once)
            fp32 = orc.Model(dataclasses.replace(cfg, gemm_bf16=False), W).encoder(feats)
            assert np.abs(oenc - fp32).max() > 1e-3, "the bf16 oracle mode must actually differ from fp32"
        if T in AFTER_A_GROWTH:
            assert window
            alone = fresh_run(wp, cfg, lambda m: m.encode(feats), T)
            G.assert_bits_equal(got, alone, f"call {i}: B = {B}, T = {T}: a window of the table built for {longest} vs a fresh model")
            held += 1
    assert held == len(AFTER_A_GROWTH)


def test_bf16_ragged_batches_between_uniform_calls(tmp_path_factory):
    cfg = bf16_cfg(name="tiny-bf16-history-ragged")
    W, wp, om, gm = pair(tmp_path_factory, cfg, seed=5)
    longest = 0
    for i, call in enumerate(RAGGED_HISTORY):
        if isinstance(call, list):
            fl = ragged_feats(400 + 10 * i, call)
            got = gm.encode_ragged(fl)
            window = max(call) < longest
            longest = max(longest, max(call))
            tables(gm, True, longest, f"call {i} (ragged {call})")
            for j, f in enumerate(fl):
                close(got[j], om.encoder(f[None])[0], f"call {i}: clip {j} ({call[j]} frames) of a packed batch, table built for {longest}")
            if i == 1:                                                # the short packed batch: rag.pos_T > T_max
                assert window
                alone = fresh_run(wp, cfg, lambda m: m.encode_ragged(fl), max(call))
                for j in range(len(fl)):
                    G.assert_bits_equal(got[j], alone[j], f"call {i}: clip {j} ({call[j]} frames): a window of the table built for {longest} vs a fresh model")
        else:
            T, B = call
            feats = feats_of(400 + 10 * i, B, T)
            got = gm.encode(feats)
            window = T < longest
            longest = max(longest, T)
            tables(gm, True, longest, f"call {i} (T = {T})")
            close(got, om.encoder(feats), f"call {i}: B = {B}, T = {T}, table built for {longest}")
            if window:                                                # the uniform calls right after a packed batch, and the last one
                alone = fresh_run(wp, cfg, lambda m: m.encode(feats), T)
                G.assert_bits_equal(got, alone, f"call {i}: B = {B}, T = {T}: a window of the table built for {longest} vs a fresh model")


def bf16_switch(d):
    """(T_lo, T_hi): 2 T_lo - 1 rows are the longest table run_gemm would send to the small-M bf16 kernel, 2 T_hi - 1 the shortest it keeps on the tile kernels
    -- by asking pk_diag_gemm_smallm_bf16_form, which refuses (PK_ERR_UNSUPPORTED) what gemm_smallm_bf16_applies refuses.  The pos_proj product: fp32 rows
    in, bf16 rows out, no bias."""
    def smallm(M):
        try:
            capi.diag_gemm_smallm_bf16_form(M, d, d, bias=False, out_bf16=True, w_tiles=False)
            return True
        except capi.PkError as e:
            assert e.code == -7
            return False
    assert smallm(1) and not smallm(1 << 16)
    lo, hi = 1, 1 << 16                                               # smallm(lo), not smallm(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if smallm(mid) else (lo, mid)
    T_lo = (lo + 1) // 2
    assert smallm(2 * T_lo - 1) and not smallm(2 * T_lo + 1)
    return T_lo, T_lo + 1


def test_bf16_table_across_the_small_m_switch(tmp_path_factory):
    """The tiny config at hidden size 512 (eight heads of 64): K % 256 == 0, so a product of up to 128 rows may run on the small-M bf16 kernel, with K split
    over two waves.  A model that first sees T_hi frames builds its table on the tile kernel; T_lo and batches of shorter clips then read windows of it.  A
    fresh model builds the tables for those lengths itself -- on the small-M kernel, had ensure_pos_tables not set GemmArgs::one_form."""
    cfg = bf16_cfg(hidden_size=512, num_heads=8, ffn_intermediate=1024, name="tiny-bf16-d512-history")
    W, wp, om, gm = pair(tmp_path_factory, cfg, seed=5)
    T_lo, T_hi = bf16_switch(cfg.hidden_size)
    assert 1 < T_lo < T_hi <= 257
    f_hi = feats_of(51, 1, T_hi)
    close(gm.encode(f_hi), om.encoder(f_hi), f"T = {T_hi}")
    tables(gm, True, T_hi, "after the long call")
    for k, (T, B) in enumerate([(T_lo, 1), (33, 3), (T_lo - 1, 2)]):
        feats = feats_of(52 + k, B, T)
        got = gm.encode(feats)
        tables(gm, True, T_hi, f"after B = {B}, T = {T}")
        close(got, om.encoder(feats), f"B = {B}, T = {T}, table built for {T_hi}")
        alone = fresh_run(wp, cfg, lambda m: m.encode(feats), T)
        G.assert_bits_equal(got, alone, f"B = {B}, T = {T}: a window of the table built for {T_hi} vs a fresh model")


def sinusoid_rows(T, d):
    """the rows ensure_pos_tables projects for T frames: sinusoidal_position_embedding in float arithmetic, position T - 1 - p in row p"""
    i = np.arange(0, d, 2, dtype=np.float32)
    div = np.exp(i * np.float32(-np.log(np.float32(10000.0)) / np.float32(d))).astype(np.float32)
    pos = np.arange(T - 1, -T, -1, dtype=np.float32)[:, None]
    pe = np.empty((2 * T - 1, d), np.float32)
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe


@pytest.mark.parametrize("d", [512, 1024])
def test_bf16_table_rows_have_one_form_at_every_m(d):
    """The pos_proj product alone (fp32 rows in, bf16 rows out, no bias), as ensure_pos_tables launches it, on tables of 127, 129 and 1025 rows -- either side
    of the small-M switch, and past the 1024 rows at which gemm_bf16_form leaves the 64 x 64 tile.  With GemmArgs::one_form every launch reports that tile
    and the rows two tables share have the same bits.  Without it the 127-row table runs on the small-M bf16 kernel: the test asserts that its rows then do
    NOT all equal the tile kernel's (were they equal, the flag would be dead weight) and prints the counts, for fp32 and for bf16 rows out."""
    R64 = ("reg", (2, 2, 1, 1), False, "lds", "none")
    T_lo, T_hi = bf16_switch(d)
    W = (np.random.default_rng(d).standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)
    rows = {}
    for T in (T_lo, T_hi, 513):
        r = capi.diag_gemm_bf16_tile(sinusoid_rows(T, d), W, out_bf16=True, one_form=True)
        assert r["form"] == R64, (T, r["form"])
        rows[T] = r["out"].view(np.uint16)[: (2 * T - 1) * d].reshape(2 * T - 1, d)
    mid = lambda T, n: rows[T][T - n: T + n - 1]                     # the window a sequence of n frames reads  # noqa: E731
    assert np.array_equal(mid(T_hi, T_lo), rows[T_lo]) and np.array_equal(mid(513, T_lo), rows[T_lo]) and np.array_equal(mid(513, T_hi), rows[T_hi])
    assert capi.diag_gemm_bf16_tile_form(1025, d, d, bias=False, out_bf16=True) != R64, "1025 rows must be a shape whose form one_form changes"
    for out_bf16 in (False, True):
        s = capi.diag_gemm_smallm_bf16(sinusoid_rows(T_lo, d), W, out_bf16=out_bf16, w_tiles=False)["out"]
        t = capi.diag_gemm_bf16_tile(sinusoid_rows(T_hi, d), W, out_bf16=out_bf16)["out"]
        n = (2 * T_lo - 1) * d
        if out_bf16:
            s, t = s.view(np.uint16)[:n], t.view(np.uint16)[d: d + n]
            assert np.array_equal(t.reshape(-1, d), mid(T_hi, T_lo)), "one_form changes nothing where the dispatch takes the 64 x 64 tile anyway"
        else:
            s, t = s[:n], t[d: d + n]
        differ = int((s != t).sum())
        print(f"K = {d}, {'bf16' if out_bf16 else 'fp32'} rows out: {differ} of {n} elements differ between the small-M and the tile kernel")
        assert differ > 0, "the two families agree on every element: one_form would not be needed"


# ---- 3. decode after other shapes ----------------------------------------------------------------------------------------------------------------------
def same_decode(g, o, what, keys=("ids", "start", "end")):
    """lens, step counts, ids, first and last frame of every token (a TDT token's duration is in them), confidence bits"""
    assert (g["lens"] >= 0).all(), (what, g["lens"])
    assert np.array_equal(g["lens"], o["lens"]), (what, g["lens"], o["lens"])
    if "steps" in o and "steps" in g:
        assert np.array_equal(g["steps"], o["steps"]), (what, g["steps"], o["steps"])
    for b in range(len(o["lens"])):
        n = o["lens"][b]
        for k in keys:
            assert np.array_equal(g[k][b, :n], o[k][b, :n]), (what, k, b)
        G.assert_bits_equal(g["conf"][b, :n], o["conf"][b, :n], f"{what}: confidence of utterance {b}")


def tdt_oracle(om, enc):
    o = om.tdt_greedy(enc, max_steps=0)
    assert not o["overflow"]
    return o


def decode_both(gm, om, orc, enc, what):
    """one TDT and one CTC decode of a uniform batch against the oracle's; -> tokens the oracle emitted"""
    o = tdt_oracle(om, enc)
    same_decode(gm.tdt_decode(enc), o, f"{what}: TDT")
    lp = om.ctc_logprobs(enc)
    c = gm.ctc_decode(enc, return_logp=True)
    G.assert_bits_equal(c["logp"], lp, f"{what}: CTC log-probs")
    oc = orc.ctc_greedy(lp, om.cfg.blank_id)
    same_decode(c, oc, f"{what}: CTC")
    return int(o["lens"].sum()), int(oc["lens"].sum())


def decode_both_ragged(gm, om, orc, xs, what):
    g, c = gm.tdt_decode_ragged(xs), gm.ctc_decode_ragged(xs, return_logp=True)
    n = 0
    for i, x in enumerate(xs):
        o = tdt_oracle(om, x[None])
        k = o["lens"][0]
        assert g["lens"][i] == k and g["steps"][i] == o["steps"][0], (what, i, g["lens"][i], k)
        for key in ("ids", "start", "end"):
            assert np.array_equal(g[key][i, :k], o[key][0, :k]), (what, "TDT", key, i)
        G.assert_bits_equal(g["conf"][i, :k], o["conf"][0, :k], f"{what}: TDT confidence of clip {i}")
        lp = om.ctc_logprobs(x[None])
        G.assert_bits_equal(c["logp"][i], lp[0], f"{what}: CTC log-probs of clip {i}")
        oc = orc.ctc_greedy(lp, om.cfg.blank_id)
        m = oc["lens"][0]
        assert c["lens"][i] == m, (what, i, c["lens"][i], m)
        for key in ("ids", "start", "end"):
            assert np.array_equal(c[key][i, :m], oc[key][0, :m]), (what, "CTC", key, i)
        G.assert_bits_equal(c["conf"][i, :m], oc["conf"][0, :m], f"{what}: CTC confidence of clip {i}")
        n += k
    return int(n)


@pytest.mark.parametrize("mode", LOOPS)
def test_decode_after_other_shapes(tmp_path_factory, orc, mode):
    """Large, small, middle, a packed batch, one long utterance: the decode buffers grow on the first call and serve every later one; the packed batch leaves
    its frame-count tables behind for the uniform call after it.  tests/test_gpu_decode_loops.py::test_graph_after_other_calls_grew_the_decode_buffers holds the
    graph driver's keys after a GROWTH; this is the shrink direction, on every driver.  (T, B, seed) as that module's GEOMETRY found them: the oracle emits."""
    W, wp, om, gm = pair(tmp_path_factory, G.tiny(name=f"tiny-history-decode-{mode}"))
    d = om.cfg.hidden_size
    gm.set_decode_loop(mode)
    try:
        n = 0
        for B, T, seed in ((3, 57, 1000), (1, 5, 1002), (3, 14, 1000)):
            n += decode_both(gm, om, orc, enc_like(B, T, d, seed), f"{mode}: B = {B}, T = {T}")[0]
        xs = [enc_like(1, t, d, 1100 + t)[0] for t in (40, 1, 13, 57, 2)]
        n += decode_both_ragged(gm, om, orc, xs, f"{mode}: packed batch")
        n += decode_both(gm, om, orc, enc_like(1, 57, d, 1000), f"{mode}: B = 1, T = 57 after the packed batch")[0]
        assert n > 10, "degenerate case: the oracle emits next to nothing"
    finally:
        gm.set_decode_loop("phases")


# ---- 4. toggles that should leave nothing behind -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toggled(tmp_path_factory):
    """one model for the two decoder toggle tests, in either order: each leaves it as a fresh one, which is the statement"""
    return pair(tmp_path_factory, G.tiny(name="tiny-history-toggles"))


def test_boost_tokens_set_and_cleared(toggled, orc):
    """tests/test_gpu_decode_loops.py::test_boost_changes_between_graph_decodes ends on "boosting off" for the TDT decode of the SAME batch; here the CTC walk
    too, and the plain calls that follow have another shape than the boosted one."""
    W, wp, om, gm = toggled
    d = om.cfg.hidden_size
    enc = enc_like(3, 40, d, 77)
    decode_both(gm, om, orc, enc, "before the boost")
    try:
        gm.set_boost_tokens([[1, 2]], 5.0)
        gm._boosted = True
        trie = orc.Trie([[1, 2]])
        same_decode(gm.tdt_decode(enc), om.tdt_greedy_boosted(enc, trie, 5.0), "boosted TDT", keys=("ids", "start", "end"))
        same_decode(gm.ctc_decode(enc), orc.ctc_greedy_boosted(om.ctc_logprobs(enc), om.cfg.ctc_vocab_size - 1, trie, 5.0), "boosted CTC")
    finally:
        gm.set_boost_tokens([])
        gm._boosted = False
    assert gm.boost_trie_size() == 0
    n = decode_both(gm, om, orc, enc_like(2, 23, d, 78), "after the boost, a smaller batch")
    m = decode_both(gm, om, orc, enc, "after the boost, the first batch again")
    assert n[0] + m[0] > 0 and n[1] + m[1] > 0, "degenerate case: nothing decoded"


def test_fused_lm_beam_then_plain_greedy(toggled, orc):
    """The fused CTC beam search takes the model's CTC buffers (and its own) for a larger batch; the greedy CTC and TDT decodes after it are the oracle's."""
    from test_gpu_ctc_beam_lm import lm_pair
    W, wp, om, gm = toggled
    cfg = om.cfg
    _, lm = lm_pair("order3_sparse_unk", cfg.ctc_vocab_size)
    wide = enc_like(6, 48, cfg.hidden_size, 81)
    got = gm.ctc_beam_decode(wide, 8, 16, 4, timestamps=True, lm=lm, lm_alpha=1.5, lm_beta=-0.5)
    assert "lm_score" in got and (got["lens"][:, 0] >= 0).all()
    n = decode_both(gm, om, orc, enc_like(2, 31, cfg.hidden_size, 82), "after the fused search")
    xs = [enc_like(1, t, cfg.hidden_size, 83 + t)[0] for t in (7, 48, 1)]
    gm.ctc_beam_decode(xs, 4, 8, 4, timestamps=True, lm=lm)
    k = decode_both_ragged(gm, om, orc, xs, "after the fused search on a packed batch")
    assert n[0] + k > 0 and n[1] > 0, "degenerate case: nothing decoded"


def test_attention_context_set_and_cleared(tmp_path_factory):
    """tests/test_gpu_local_encoder.py::test_toggle_back_is_a_fresh_model repeats the SAME batch after (-1, -1).  Here the plain calls after the toggle have
    other lengths than the one before it, one of them between the table's length and the local call's: limited-context calls neither build nor grow the
    2 T - 1 tables, so the plain call must."""
    W, wp, om, gm = pair(tmp_path_factory, G.tiny(name="tiny-history-attention-context"))
    f40, f130, f90, f17 = feats_of(91, 2, 40), feats_of(92, 1, 130), feats_of(93, 1, 90), feats_of(94, 3, 17)
    plain = gm.encode(f40)
    tables(gm, False, 40, "the plain call")
    G.assert_bits_equal(plain, om.encoder(f40), "before the toggle")
    try:
        gm.set_attention_context(8, 2)
        loc = gm.encode(f40)
        gm.encode(f130)
        tables(gm, False, 40, "limited-context calls")
    finally:
        gm.set_attention_context(-1, -1)
    assert gm.attention_context() == (-1, -1) and not np.array_equal(loc, plain), "degenerate case: the window changed nothing"
    G.assert_bits_equal(gm.encode(f90), om.encoder(f90), "after the toggle, T = 90: longer than the table, shorter than the local call")
    tables(gm, False, 90, "the first plain call after the toggle")
    G.assert_bits_equal(gm.encode(f17), om.encoder(f17), "after the toggle, T = 17")
    tables(gm, False, 90, "the second plain call after the toggle")
