"""Streaming sessions (pk_stream_*, csrc/stream.cpp: StreamBatch) past the row-count switch of their products and across their history.

StreamBatch::encode_device picks the layouts of a chunk's Conformer blocks from rows = S * c: up to kSmallMRows (fp32) / kSmallMRowsBf16 (bf16 mode) the
small-M kernels, the sigma layout of ctx and the conv output, the tiled weight copies and possibly the conv fused into pw1; above, the tile family with
natural columns and the separate conv kernel.  The K/V and conv caches a chunk leaves are read by the next one, which may run under the other regime;
the tiled copies are latched by the first chunk that qualifies.  The other streaming tests run at most 16 streams, so they stay below the switch.

Here a session has hundreds of streams that carry the audio of 2 .. 4 distinct clips (stream s: clip s % n), so the CPU oracle runs 2 .. 4 streams and
EVERY stream of every chunk is compared with the oracle stream of its clip: fp32 bit for bit (log-mel, encoder rows, token ids, frames, confidence
bits -- the comparison of tests/test_gpu_stream.py::run_pair), the bf16 mode by the statements of test_stream_bf16_mode_vs_bf16_oracle plus bit equality
between a first pass, a pass after reset() and a fresh session.  The switches are asked of the library (fp32_switch / bf16_switch of
tests/test_gpu_call_history.py), the regime of every chunk is asked of the session (Stream.chunk_form -> pk_diag_stream_chunk_form), and a test that
stops crossing the switch fails.  The oracle's token counts are asserted, so that no case passes on empty output; the seeds were picked with the oracle."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth
from test_gpu_call_history import bf16_switch, decode_both, decode_both_ragged, feats_of, fp32_switch, ragged_feats
from test_gpu_decode import _pair_with, enc_like
from test_gpu_stream import DRIFT_MAX, DRIFT_MEAN, STREAM_SCHED, _token_statement

pytestmark = pytest.mark.gpu

S_TINY, S_110M, S_BF16 = 400, 200, 40          # asserted against the searched switches: 3 S <= M_lo < 4 S, 7 S <= M_lo < 8 S, 3 S <= M_lo_bf16 < 4 S
SCHED_110M = [10240, 10240, 8960, 1280, 2560, 10240, 1280, 10240, 8960, 2560]      # chunks of 7, 8, 7, 1, 2, 7, 1, 8, 7, 2 encoder frames


def rot(k, extra=()):
    return STREAM_SCHED[k:] + STREAM_SCHED[:k] + list(extra)


# ---- the switches, from the library ---------------------------------------------------------------------------------------------------------------------
def m_lo_fp32(widths=(128, 512)):
    """the largest row count launch_gemm sends to the fp32 small-M family, for every hidden size used here"""
    def tile(M, d):
        try:
            capi.diag_gemm_tile_form(M, d, d)
            return True
        except capi.PkError as e:
            assert e.code == -7
            return False
    T_lo, _ = fp32_switch()                                           # not tile(2 T_lo - 1), tile(2 T_lo + 1)
    M = 2 * T_lo if not tile(2 * T_lo, widths[0]) else 2 * T_lo - 1
    for d in widths:
        assert not tile(M, d) and tile(M + 1, d), (M, d)
    return M


def m_lo_bf16(d):
    def smallm(M):
        try:
            capi.diag_gemm_smallm_bf16_form(M, d, d, bias=False, out_bf16=True, w_tiles=False)
            return True
        except capi.PkError as e:
            assert e.code == -7
            return False
    T_lo, _ = bf16_switch(d)                                          # smallm(2 T_lo - 1), not smallm(2 T_lo + 1)
    M = 2 * T_lo if smallm(2 * T_lo) else 2 * T_lo - 1
    assert smallm(M) and not smallm(M + 1)
    return M


# ---- models ---------------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def close_models():
    yield
    for _, gm in _MODELS.values():
        gm.close()
    _MODELS.clear()


def _lower_blank(W):
    W["tdt_joint_.label_proj_.bias"][-1] -= 1.0                       # (tests/test_gpu_decode_loops.py::test_streaming_chunks: chunks of a few frames emit)


W_SEED = {9: 18, 31: 16}     # weight seeds at which the oracle emits on real audio, irregularly and with about ten distinct ids (picked with the oracle alone)


def low_pair(tmp_path_factory, kc=9):
    """(oracle model, product model): the tiny config with 2 layers and the blank's bias lowered; built once per conv size, closed with the module"""
    if kc not in _MODELS:
        cfg = G.tiny(num_layers=2, conv_kernel_size=kc, name=f"tiny-stream-history-k{kc}")
        _MODELS[kc] = _pair_with(tmp_path_factory.mktemp("sh"), cfg, W_SEED[kc], _lower_blank)
    return _MODELS[kc]


def pair_110m(tmp_path_factory):
    cfg = dataclasses.replace(pk.make_110m_config(), num_layers=2, name="110m-2L-stream")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("sh110"), cfg, seed=42)
    return om, gm


# ---- the oracle's side: computed once per (model, context, audio, schedule), shared by the passes that need it ------------------------------------------
def overlap_after(sched):
    """(mel frames of every push, samples the front end keeps after the last one) -- StreamingAudioPreprocessor::process_chunk's own arithmetic"""
    ov, frames = 0, []
    for n in sched:
        total = ov + n
        nf = 0 if total < 400 else (total - 400) // 160 + 1
        ov = total if nf == 0 else total - ((nf - 1) * 160 + 400)
        frames.append(nf)
    return frames, ov


def oracle_run(orc, om, left, right, pcm0, sched, mel_only_last=False, margins=False):
    """One oracle Stream per row of pcm0 through the pushes of sched -> per push dict(seg [n][samples], mel [n][f][F], enc [n][c][d] or None (the encoder
    did not run: no mel frame, or mel_only_last on the last push), tok: the n decode results or None)."""
    n = len(pcm0)
    os_ = [orc.Stream(om, left, right) for _ in range(n)]
    at = np.concatenate([[0], np.cumsum(sched)]).astype(np.int64)
    assert at[-1] <= pcm0.shape[1]
    out = []
    for i in range(len(sched)):
        seg = np.ascontiguousarray(pcm0[:, at[i]:at[i + 1]])
        mel = np.stack([o.mel(seg[k]) for k, o in enumerate(os_)])
        r = dict(seg=seg, mel=mel, enc=None, tok=None)
        if mel.shape[1] > 0 and not (mel_only_last and i == len(sched) - 1):
            r["enc"] = np.stack([o.encode(mel[k]) for k, o in enumerate(os_)])
            if r["enc"].shape[1] > 0:
                r["tok"] = [o.decode(r["enc"][k], margins=margins) for k, o in enumerate(os_)]
        out.append(r)
    for o in os_:
        o.close()
    assert [r["mel"].shape[1] for r in out] == overlap_after(sched)[0]
    return out


def n_tok(r):
    return 0 if r["tok"] is None else sum(len(t["ids"]) for t in r["tok"])


# ---- the comparisons (tests/test_gpu_stream.py::run_pair's, stream s against the oracle stream idx[s]) ----------------------------------------------------
def same_tokens(g, toks, idx, what, offs=None):
    """g: the product's token arrays of S streams; toks: the oracle's results; stream s must carry toks[idx[s]] (frames + offs[idx[s]])"""
    lens = np.array([len(t["ids"]) for t in toks], np.int32)
    bad = np.flatnonzero(g["lens"] != lens[idx])
    assert bad.size == 0, f"{what}: token counts of streams {bad[:8].tolist()}: {g['lens'][bad[:8]].tolist()}, the oracle emitted {lens[idx][bad[:8]].tolist()}"
    for k, t in enumerate(toks):
        rows, n = np.flatnonzero(idx == k), len(t["ids"])
        off = 0 if offs is None else offs[k]
        if rows.size == 0 or n == 0:
            continue
        assert np.array_equal(g["ids"][rows, :n], np.broadcast_to(t["ids"], (rows.size, n))), f"{what}: token ids of the streams of oracle stream {k}"
        assert np.array_equal(g["start"][rows, :n], np.broadcast_to(t["start"] + off, (rows.size, n))), f"{what}: first frames of the streams of oracle stream {k}"
        assert np.array_equal(g["end"][rows, :n], np.broadcast_to(t["end"] + off, (rows.size, n))), f"{what}: last frames of the streams of oracle stream {k}"
        G.assert_bits_equal(g["conf"][rows, :n], np.broadcast_to(t["conf"], (rows.size, n)), f"{what}: confidence of the streams of oracle stream {k}")


def staged_one(gs, idx, r, what, forms=None):
    """one push through pk_stream_mel / _encode / _decode against the oracle's record r; forms collects (frames, chunk_form, oracle tokens)"""
    gmel = gs.mel(np.ascontiguousarray(r["seg"][idx]))
    assert gmel.shape[1] == r["mel"].shape[1], what
    if gmel.shape[1] == 0:
        return
    G.assert_bits_equal(gmel, r["mel"][idx], f"{what}: stream log-mel")
    if r["enc"] is None:
        return
    genc = gs.encode(gmel)
    assert genc.shape[1] == r["enc"].shape[1], what
    if genc.shape[1] == 0:
        return
    G.assert_bits_equal(genc, r["enc"][idx], f"{what}: stream encoder")
    if forms is not None:
        forms.append((genc.shape[1], gs.chunk_form(), n_tok(r)))
    same_tokens(gs.decode(genc), r["tok"], idx, what)


def staged(gs, idx, ref, what, forms=None):
    for i, r in enumerate(ref):
        staged_one(gs, idx, r, f"{what}, push {i}", forms)


def pushed(gs, idx, ref, what):
    """the same pushes through pk_stream_push (device-resident between the stages, the pinned result copies)"""
    for i, r in enumerate(ref):
        g = gs.push(np.ascontiguousarray(r["seg"][idx]))
        if r["tok"] is None:
            assert not g["lens"].any(), f"{what}, push {i}: tokens from a push the oracle buffered"
        else:
            same_tokens(g, r["tok"], idx, f"{what}, push {i} (pk_stream_push)")


def regimes(forms, S, M_lo, key, first_small, what):
    """Both regimes ran, each direction of the switch was taken, the first chunk ran in the regime the case names, every chunk ran where rows = S * c says
    -- and the oracle emitted on both sides of a switch in each direction."""
    small = [f[key] == 1 for _, f, _ in forms]
    for (c, f, _), s in zip(forms, small):
        assert f["rows"] == S * c and s == (S * c <= M_lo), f"{what}: a chunk of {c} frames ran as {f}, the switch is at {M_lo} rows"
        assert (f["sg"], f["wt"]) == ((int(s), 0) if key == "sg" else (0, int(s))), f
        assert not f["fused_conv"] or s, f"{what}: the conv rode on pw1 outside the small-M regime: {f}"
    print(f"{what}: chunks (frames, rows, {key}, fused conv, oracle tokens) {[(c, f['rows'], f[key], f['fused_conv'], t) for c, f, t in forms]}; "
          f"oracle tokens {sum(t for _, _, t in forms)}")
    assert set(small) == {True, False}, f"{what}: one regime only"
    assert small[0] == first_small, f"{what}: the first chunk ran {'small-M' if small[0] else 'tile'}"
    for a, b in ((True, False), (False, True)):
        at = [i for i in range(1, len(small)) if (small[i - 1], small[i]) == (a, b)]
        assert at, f"{what}: no switch from {'small-M' if a else 'tile'} to {'small-M' if b else 'tile'}"
        assert any(forms[i - 1][2] > 0 and forms[i][2] > 0 for i in at), f"{what}: the oracle emits on one side only of every such switch"
    assert sum(t for _, _, t in forms) >= 10, f"{what}: degenerate case, the oracle emits next to nothing"


# ---- 1. fp32 sessions on both sides of the switch -----------------------------------------------------------------------------------------------------------
# (conv taps, rotation of STREAM_SCHED, is the first encoder chunk in the small-M regime, audio seed)
FP32_CASES = [(9, 6, False, 11), (9, 0, True, 12), (31, 6, False, 13)]


@pytest.mark.parametrize("kc,r,first_small,seed", FP32_CASES)
def test_fp32_tiny_session_crosses_the_switch(tmp_path_factory, orc, kc, r, first_small, seed):
    """400 streams, att (10, 1), chunks of 1 .. 5 frames: 1200 rows and fewer on the small-M family, 1600 and 2000 on the tiles.  (a) the first chunk is a
    tile chunk, so the tiled copies are latched later by a chunk that found caches written in natural columns; (b) the first chunk latches them.  With
    31 taps the separate conv kernel's second instantiation writes natural columns too."""
    om, gm = low_pair(tmp_path_factory, kc)
    M_lo, S = m_lo_fp32(), S_TINY
    assert 3 * S <= M_lo < 4 * S
    sched = rot(r)
    idx = np.arange(S) % 2
    ref = oracle_run(orc, om, 10, 1, synth.synth_pcm(2, sum(sched), seed=seed), sched)
    forms = []
    gs = capi.Stream(gm, S, 10, 1)
    try:
        assert gs.chunk_form() == dict(rows=0, sg=0, wt=0, fused_conv=0)
        staged(gs, idx, ref, f"{kc} taps, rotation {r}", forms)
    finally:
        gs.close()
    regimes(forms, S, M_lo, "sg", first_small, f"fp32 tiny, {kc} taps, rotation {r}, {S} streams")
    if kc == 31:
        assert not any(f["fused_conv"] for _, f, _ in forms)
    gs = capi.Stream(gm, S, 10, 1)                                   # a fresh session through the product call: the same tokens, frames, confidence bits
    try:
        pushed(gs, idx, ref, f"{kc} taps, rotation {r}")
    finally:
        gs.close()


def test_fp32_110m_cut_session_crosses_the_switch(tmp_path_factory, orc):
    """The LDS-tile attention (head size 64, att (70, 1)) and the d = 512 / 2048 products: 200 streams, chunks of 8 frames on the tile family, of 7, 2
    and 1 on the small-M kernels."""
    om, gm = pair_110m(tmp_path_factory)
    M_lo, S = m_lo_fp32(), S_110M
    assert 7 * S <= M_lo < 8 * S
    idx = np.arange(S) % 2
    ref = oracle_run(orc, om, 70, 1, synth.synth_pcm(2, sum(SCHED_110M), seed=77), SCHED_110M)
    assert sorted({r["enc"].shape[1] for r in ref}) == [1, 2, 7, 8]
    forms = []
    gs = capi.Stream(gm, S, 70, 1)
    try:
        staged(gs, idx, ref, "110m cut", forms)
    finally:
        gs.close()
    regimes(forms, S, M_lo, "sg", True, f"fp32 110m cut, {S} streams")
    gs = capi.Stream(gm, S, 70, 1)
    try:
        pushed(gs, idx, ref, "110m cut")
    finally:
        gs.close()


# ---- 2. bf16 mode across its switch -------------------------------------------------------------------------------------------------------------------------
def test_bf16_session_crosses_the_switch_and_does_not_depend_on_history(tmp_path_factory, orc):
    """110m-2L-stream-bf16, 40 streams of 3 clips, STREAM_SCHED from a tile-regime chunk on: chunks of up to 3 frames (120 rows) run on the small-M bf16 kernel
    with the operand tiles, chunks of 4 and 5 on the bf16 tile kernels with the folded norms.  Against the bf16 oracle: the statements and constants of
    test_stream_bf16_mode_vs_bf16_oracle, each side carrying its own caches.  With no tolerance: the same schedule after reset(), and on a fresh session,
    gives the first pass's encoder bits and tokens chunk by chunk -- the first pass begins with the operand tiles not yet built, the others with them."""
    cfg = dataclasses.replace(pk.make_110m_config(), num_layers=2, gemm_bf16=True, name="110m-2L-stream-bf16")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("shb16"), cfg, seed=42)
    fm = orc.Model(dataclasses.replace(cfg, gemm_bf16=False), W)
    M_lo, S, n = m_lo_bf16(cfg.hidden_size), S_BF16, 3
    assert 3 * S <= M_lo < 4 * S
    sched = rot(6)
    idx = np.arange(S) % n
    pcm0 = synth.synth_pcm(n, sum(sched), seed=77)
    ref = oracle_run(orc, om, 70, 1, pcm0, sched, margins=True)
    fref = oracle_run(orc, fm, 70, 1, pcm0[:1], sched)                # clip 0 in fp32: the size of the mode's own deviation

    def one_pass(gs):
        out = []
        for r in ref:
            gmel = gs.mel(np.ascontiguousarray(r["seg"][idx]))
            assert gmel.shape[1] == r["mel"].shape[1]
            G.assert_bits_equal(gmel, r["mel"][idx], "stream log-mel (no product in it: bit-equal in either mode)")
            genc = gs.encode(gmel)
            assert genc.shape[1] == r["enc"].shape[1] > 0
            out.append((genc, gs.chunk_form(), gs.decode(genc)))
        return out

    gs = capi.Stream(gm, S, 70, 1)
    try:
        first = one_pass(gs)
        gs.reset()
        again = one_pass(gs)
    finally:
        gs.close()
    gs = capi.Stream(gm, S, 70, 1)
    try:
        fresh = one_pass(gs)
    finally:
        gs.close()
    # (a) against the bf16 oracle
    g_ids = [[] for _ in range(S)]
    worst, worst_mean, dev_sum, gap_sum, n_el, n_gap, absmax = 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0
    for i, ((genc, f, g), r, fr) in enumerate(zip(first, ref, fref)):
        oenc = r["enc"][idx]
        d, mx = np.abs(genc - oenc), float(np.abs(oenc).max())
        worst, worst_mean, absmax = max(worst, d.max() / mx), max(worst_mean, d.mean() / mx), max(absmax, mx)
        dev_sum += float(d.sum()); n_el += d.size
        gap_sum += float(np.abs(r["enc"][0] - fr["enc"][0]).sum()); n_gap += fr["enc"][0].size
        print(f"push {i}: {genc.shape[1]} frames, {f}: max {d.max() / mx:.3e} mean {d.mean() / mx:.3e} of max|x|")
        assert d.max() <= DRIFT_MAX * mx and d.mean() <= DRIFT_MEAN * mx, f"chunk {i} ({f}): max {d.max():.3e} mean {d.mean():.3e} (max|x| {mx:.2f})"
        for s in range(S):
            g_ids[s] += g["ids"][s, : g["lens"][s]].tolist()
    o_ids = [[t for r in ref for t in r["tok"][k]["ids"].tolist()] for k in range(n)]
    o_lab = [[t for r in ref for t in r["tok"][k]["step_label"].tolist()] for k in range(n)]
    o_mg = [[t for r in ref for t in r["tok"][k]["step_margin"].tolist()] for k in range(n)]
    assert sum(map(len, o_ids)) >= 10, "degenerate case: the oracle emits next to nothing"
    dev, gap = dev_sum / n_el / absmax, gap_sum / n_gap / absmax
    div = [_token_statement(g_ids[s], o_lab[idx[s]], o_mg[idx[s]], cfg.blank_id, f"stream {s}") for s in range(S)]
    regimes([(genc.shape[1], f, n_tok(r)) for (genc, f, _), r in zip(first, ref)], S, M_lo, "wt", False, f"bf16 110m cut, {S} streams")
    print(f"bf16 mode, {S} streams: worst chunk max {worst:.2e} mean {worst_mean:.2e}, session mean {dev:.2e} of max|x| (the oracle's bf16-vs-fp32 gap {gap:.2e}); "
          f"oracle tokens {[len(x) for x in o_ids]}, streams with identical tokens {sum(a is None for a, _ in div)} of {S}")
    assert gap > 1e-4, "the bf16 oracle mode must actually differ from fp32"
    assert dev < gap, "the GPU should be closer to the bf16 oracle than the bf16 mode is to fp32"
    # (b) bit for bit: after reset() and on a fresh session
    for name, other in (("after reset()", again), ("a fresh session", fresh)):
        for i, ((e0, f0, g0), (e1, f1, g1)) in enumerate(zip(first, other)):
            assert f0 == f1, (name, i, f0, f1)
            G.assert_bits_equal(e1, e0, f"{name}, push {i} ({f0}): encoder rows vs the first pass")
            for k in ("lens", "ids", "start", "end"):
                assert np.array_equal(g1[k], g0[k]), (name, i, k)
            G.assert_bits_equal(g1["conf"], g0["conf"], f"{name}, push {i}: confidence vs the first pass")


# ---- 3. history of a session (fp32, tiny) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mel_only_last", [False, True])
def test_reset_from_a_dirty_state(tmp_path_factory, orc, mel_only_last):
    """reset() after a schedule that leaves mel leftovers, overlap samples and full K/V and conv caches written under both regimes (or, mel_only_last, after
    a push of which only pk_stream_mel ran); then OTHER audio in another rotation of the schedule: every stage is a fresh oracle stream's."""
    om, gm = low_pair(tmp_path_factory)
    S, left = S_TINY, 10
    idx = np.arange(S) % 2
    dirty, clean = rot(0, extra=[2100]), rot(6)
    ref1 = oracle_run(orc, om, left, 1, synth.synth_pcm(2, sum(dirty), seed=21), dirty, mel_only_last=mel_only_last)
    ref2 = oracle_run(orc, om, left, 1, synth.synth_pcm(2, sum(clean), seed=22), clean)
    mel_frames = sum(r["mel"].shape[1] for r in ref1[: len(ref1) - int(mel_only_last)])
    enc_frames = sum(r["enc"].shape[1] for r in ref1 if r["enc"] is not None)
    assert mel_frames - 8 * enc_frames > 0, "the dirty run must end with mel leftovers"
    assert overlap_after(dirty)[1] > 0, "the dirty run must end with overlap samples"
    assert enc_frames >= left + 1, "the dirty run must fill the K/V cache"
    assert ref1[-1]["mel"].shape[1] > 0 and (ref1[-1]["enc"] is None) == mel_only_last
    assert sum(map(n_tok, ref1)) >= 10 and sum(map(n_tok, ref2)) >= 10
    f1, f2 = [], []
    gs = capi.Stream(gm, S, left, 1)
    try:
        staged(gs, idx, ref1, "before the reset", f1)
        gs.reset()
        staged(gs, idx, ref2, "after the reset", f2)
    finally:
        gs.close()
    assert {f["sg"] for _, f, _ in f1} == {0, 1} == {f["sg"] for _, f, _ in f2}, "both runs must cross the switch"
    print(f"reset (mel only on the last push: {mel_only_last}): oracle tokens {sum(map(n_tok, ref1))} before, {sum(map(n_tok, ref2))} after; "
          f"rows after {[f['rows'] for _, f, _ in f2]}")


@pytest.fixture
def loop_driver():
    """sets the model's decode loop driver; back to the per-phase loop afterwards, whatever happened"""
    used = []

    def use(gm, mode):
        used.append(gm)
        gm.set_decode_loop(mode)
    yield use
    for gm in used:
        gm.set_decode_loop("phases")


@pytest.mark.parametrize("mode", ["phases", "graph"])
def test_two_sessions_pushed_alternately(tmp_path_factory, orc, loop_driver, mode):
    """Session A: 400 streams, att (10, 1); session B: 3 streams, att (70, 0), another rotation -- on one model, one push each in turn: the model's
    stream, its tiled weight copies and the decode loop's driver (and its graph cache) are shared, every cache is a session's own."""
    om, gm = low_pair(tmp_path_factory)
    sa, sb = rot(6), rot(3)
    ia, ib = np.arange(S_TINY) % 2, np.arange(3)
    ra = oracle_run(orc, om, 10, 1, synth.synth_pcm(2, sum(sa), seed=31), sa)
    rb = oracle_run(orc, om, 70, 0, synth.synth_pcm(3, sum(sb), seed=32), sb)
    assert sum(map(n_tok, ra)) >= 10 and sum(map(n_tok, rb)) >= 10
    assert any(x["enc"].shape[1] != y["enc"].shape[1] for x, y in zip(ra, rb)), "the two sessions' chunk sizes must differ within a round"
    fa, fb = [], []
    loop_driver(gm, mode)
    a, b = capi.Stream(gm, S_TINY, 10, 1), capi.Stream(gm, 3, 70, 0)
    try:
        for i, (x, y) in enumerate(zip(ra, rb)):
            staged_one(a, ia, x, f"{mode}: session A, push {i}", fa)
            staged_one(b, ib, y, f"{mode}: session B, push {i}", fb)
    finally:
        a.close(); b.close()
    assert {f["sg"] for _, f, _ in fa} == {0, 1} and {f["sg"] for _, f, _ in fb} == {1}
    print(f"{mode}: A rows {[f['rows'] for _, f, _ in fa]} ({sum(map(n_tok, ra))} oracle tokens), B rows {[f['rows'] for _, f, _ in fb]} ({sum(map(n_tok, rb))})")


@pytest.mark.parametrize("mode", ["phases", "graph"])
def test_offline_calls_between_the_pushes_of_a_live_session(tmp_path_factory, orc, loop_driver, mode):
    """Between the pushes of a 400-stream session the same Model serves a uniform encode, a TDT / CTC decode, a packed encode and a packed decode -- each the
    oracle's -- and the session's next pushes are still the oracle's."""
    om, gm = low_pair(tmp_path_factory)
    d, S = om.cfg.hidden_size, S_TINY
    sched = rot(6)
    idx = np.arange(S) % 2
    ref = oracle_run(orc, om, 10, 1, synth.synth_pcm(2, sum(sched), seed=41), sched)
    assert sum(map(n_tok, ref)) >= 10
    forms, n_off = [], 0
    loop_driver(gm, mode)
    gs = capi.Stream(gm, S, 10, 1)
    try:
        for i, r in enumerate(ref):
            staged_one(gs, idx, r, f"{mode}: push {i}", forms)
            what = f"{mode}: offline call after push {i}"
            if i % 3 == 0:
                feats = feats_of(500 + i, 2, 9 + i)
                G.assert_bits_equal(gm.encode(feats), om.encoder(feats), f"{what}: uniform encode")
            elif i % 3 == 1:
                n_off += decode_both(gm, om, orc, enc_like(3, 14 + i, d, 1000), f"{what}: uniform decode")[0]
            else:
                fl = ragged_feats(600 + 10 * i, [12, 3, 1, 7])
                got = gm.encode_ragged(fl)
                for j, f in enumerate(fl):
                    G.assert_bits_equal(got[j], om.encoder(f[None])[0], f"{what}: clip {j} of a packed encode")
                n_off += decode_both_ragged(gm, om, orc, [enc_like(1, t, d, 1100 + t)[0] for t in (13, 1, 40, 2)], f"{what}: packed decode")
    finally:
        gs.close()
    assert {f["sg"] for _, f, _ in forms} == {0, 1} and n_off > 0, "the session must cross the switch and the offline decodes must emit"
    print(f"{mode}: session rows {[f['rows'] for _, f, _ in forms]}, {sum(map(n_tok, ref))} oracle tokens; offline decodes emitted {n_off}")


def test_reset_decoder_on_every_third_of_400_streams(tmp_path_factory, orc):
    """reset_decoder(mask) in the middle of a 400-stream session: the masked streams go on as oracle streams whose prediction net starts over (a fresh
    oracle stream decodes their encoder rows; frames keep counting), the others as if nothing had happened."""
    om, gm = low_pair(tmp_path_factory)
    S, n = S_TINY, 2
    sched = rot(0)
    at_push = 5
    mask = (np.arange(S) % 3 == 0).astype(np.uint8)
    idx = np.arange(S) % n
    pcm0 = synth.synth_pcm(n, sum(sched), seed=51)
    ref = oracle_run(orc, om, 10, 1, pcm0, sched)
    offset = sum(r["enc"].shape[1] for r in ref[:at_push])
    fresh = [orc.Stream(om, 10, 1) for _ in range(n)]                 # decode only: the prediction net of a new stream on the old stream's encoder rows
    after = [[o.decode(r["enc"][k]) for k, o in enumerate(fresh)] for r in ref[at_push:]]
    for o in fresh:
        o.close()
    n_kept, n_reset = sum(map(n_tok, ref[at_push:])), sum(len(t["ids"]) for ts in after for t in ts)
    assert sum(map(n_tok, ref[:at_push])) > 0 and n_kept > 0 and n_reset > 0 and n_kept + n_reset >= 10
    assert any([t["ids"].tolist() for t in ts] != [t["ids"].tolist() for t in r["tok"]] for ts, r in zip(after, ref[at_push:])), \
        "degenerate case: the reset changes nothing the oracle emits"
    gs = capi.Stream(gm, S, 10, 1)
    try:
        staged(gs, idx, ref[:at_push], "before reset_decoder")
        gs.reset_decoder(mask)
        for i, (r, ts) in enumerate(zip(ref[at_push:], after)):
            what = f"push {at_push + i}, after reset_decoder"
            gmel = gs.mel(np.ascontiguousarray(r["seg"][idx]))
            G.assert_bits_equal(gmel, r["mel"][idx], f"{what}: stream log-mel")
            genc = gs.encode(gmel)
            G.assert_bits_equal(genc, r["enc"][idx], f"{what}: stream encoder")
            same_tokens(gs.decode(genc), r["tok"] + ts, idx + n * mask, what, offs=[0] * n + [offset] * n)
    finally:
        gs.close()
    print(f"reset_decoder at push {at_push} ({offset} frames in): oracle tokens after it {n_kept} on the streams kept, {n_reset} on the streams reset")


# ---- 4. streaming decode with carried state at large S ------------------------------------------------------------------------------------------------------
def test_stream_decode_with_carried_state_at_400_and_2100_streams(tmp_path_factory, orc):
    """pk_stream_decode on given encoder rows, chunks of 1, 2, 5 and 14 frames, 4 clips: 400 streams decode with prediction-net caching (the compacted row
    list, B <= kMaxListRows), 2100 run every row.  Every stream against the oracle's streaming decode of its clip; the two sessions agree."""
    om, gm = low_pair(tmp_path_factory)
    n, frames = 4, [2, 1, 5, 14, 1, 14, 2, 5]
    chunks = [enc_like(n, c, om.cfg.hidden_size, 300 + i) for i, c in enumerate(frames)]
    os_ = [orc.Stream(om, 10, 1) for _ in range(n)]
    want = [[os_[k].decode(e[k]) for k in range(n)] for e in chunks]
    for o in os_:
        o.close()
    per_clip = [sum(len(ts[k]["ids"]) for ts in want) for k in range(n)]
    assert sum(per_clip) >= 10 and all(per_clip), f"degenerate case: the oracle's tokens per clip {per_clip}"
    got = {}
    for S in (400, 2100):
        idx = np.arange(S) % n
        gs = capi.Stream(gm, S, 10, 1)
        try:
            got[S] = [gs.decode(np.ascontiguousarray(e[idx])) for e in chunks]
        finally:
            gs.close()
        for i, (g, ts) in enumerate(zip(got[S], want)):
            same_tokens(g, ts, idx, f"{S} streams, chunk {i} ({frames[i]} frames)")
    for i, (a, b) in enumerate(zip(got[400], got[2100])):
        for k in ("lens", "ids", "start", "end"):
            assert np.array_equal(a[k], b[k][:400]), (i, k)
        G.assert_bits_equal(a["conf"], b["conf"][:400], f"chunk {i}: confidence, 400 vs 2100 streams")
    print(f"streaming decode, 400 and 2100 streams: chunks of {frames} frames, oracle tokens per clip {per_clip}")
