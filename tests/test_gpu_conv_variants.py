"""GPU parity of every launch variant of the convolution kernels outside the GEMM -- conv1 + dw1 and dw2 of the subsampling stack
(kernels/subsample.hip), the conv module's depthwise conv + BatchNorm + SiLU (kernels/convmod.hip) and its streaming form (kernels/stream.hip) --
against the oracle, bit for bit.

Those launchers pick an instantiation by the number of rows in flight and by the model's sizes.  Every case below names the instantiation(s) it was
written for (its `want` tuples, the rows pk_diag_conv_instantiations lists), ASKS the library which one that model and batch take
(Model.conv_variants -> pk_diag_conv_variants: the functions the launchers switch on) and asserts the two agree before it compares bits: a case
that sits on a threshold fails, instead of silently covering another variant, when the threshold moves.  Batch sizes on either side of a row
threshold are searched through the same entry, not written down.  test_every_instantiation_has_a_case compares the union of the `want` tuples
with the library's list, so a new instantiation without a case fails the suite.

fp32: G.assert_bits_equal, no tolerance.  The one bf16-mode case takes the bounds of tests/test_gpu_bf16.py."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth
from test_gpu_stream import STREAM_CONV_CASES

pytestmark = pytest.mark.gpu

# ---- the instantiations, as pk_diag_conv_instantiations lists them: (launcher, id, p0, p1, p2) -------------------------------------------
# conv1 + dw1: (0, id, packed, XC, YS)
C1_X20_Y2, C1_X16_Y2, C1_PACKED, C1_X10_Y8, C1_X8_Y8 = (0, 0, 0, 20, 2), (0, 1, 0, 16, 2), (0, 2, 1, 4, 8), (0, 3, 0, 10, 8), (0, 4, 0, 8, 8)
# dw2: (1, id, 0, XO, 0)
DW2_X5, DW2_X4 = (1, 0, 0, 5, 0), (1, 1, 0, 4, 0)
# conv module: (2, id, KC, TT, body: 0 = all rows loaded first, 1 = sliding window)
DW = {(9, 2): (2, 0, 9, 2, 0), (9, 8): (2, 1, 9, 8, 0), (31, 2): (2, 2, 31, 2, 1), (31, 8): (2, 3, 31, 8, 1)}

# mel bins -> the conv1 + dw1 / dw2 instantiations that width was chosen for.  W2 = bins / 4 columns after dw1, W3 = bins / 8 after dw2:
#    8 -> W2  2 (one partial chunk of every width),             W3  1 (one column: a partial chunk of 4)
#   72 -> W2 18 (partial last chunk of 20 / 10 / 4),            W3  9 (chunks of 4, last one partial)
#   80 -> W2 20 (whole chunks of 20 / 10 / 4: the 110m shape),  W3 10 (chunks of 5)
#   96 -> W2 24 (chunks of 16 / 8: the last partial / whole),   W3 12 (chunks of 4)
#  128 -> W2 32 (whole chunks of 16 / 8 / 4: the 600m shape),   W3 16 (chunks of 4)
SMALL_OF = {8: C1_X20_Y2, 72: C1_X20_Y2, 80: C1_X20_Y2, 96: C1_X16_Y2, 128: C1_X16_Y2}
LARGE_C32_OF = {8: C1_X10_Y8, 72: C1_X10_Y8, 80: C1_X10_Y8, 96: C1_X8_Y8, 128: C1_X8_Y8}
DW2_OF = {8: DW2_X4, 72: DW2_X4, 80: DW2_X5, 96: DW2_X4, 128: DW2_X4}


def c1_want(C, bins, large):
    return SMALL_OF[bins] if not large else (LARGE_C32_OF[bins] if C == 32 else C1_PACKED)


def tiny_cfg(**kw):
    name = "cv-" + "-".join(f"{k}{v}" for k, v in sorted(kw.items()))
    return G.tiny(name=name, **kw)


def wide_cfg(d, **kw):
    base = {512: pk.make_110m_config, 1024: pk.make_tdt_600m_config}[d]()
    name = f"cv-d{d}-" + "-".join(f"{k}{v}" for k, v in sorted(kw.items()))
    return dataclasses.replace(base, num_layers=1, name=name, **kw)


def pair(tmp_path_factory, cfg, seed=42):
    return G.make_pair(tmp_path_factory.mktemp("cv"), cfg, seed=seed)


def first_batch_where(gm, pred, **kw):
    """Smallest batch size for which the library's own selection satisfies pred."""
    for B in range(1, 4097):
        if pred(gm.conv_variants(B=B, **kw)):
            return B
    raise AssertionError("no batch size up to 4096 switches the variant")


def feats_of(seed, B, Tm, bins):
    return np.random.default_rng(seed).standard_normal((B, Tm, bins)).astype(np.float32)


# ---- subsampling --------------------------------------------------------------------------------------------------------------------------
SUB_GRID = [(C, bins, large) for C in (32, 64, 256) for bins in (8, 72, 80, 96, 128) for large in (False, True)]


@pytest.mark.parametrize("C,bins,large", SUB_GRID)
def test_subsampling_grid(tmp_path_factory, C, bins, large):
    """Channels x mel widths x the last batch size with strips of 2 rows / the first with strips of 8 (10 s clips: Tm = 1001, H2 = 251 rows each)."""
    W, om, gm = pair(tmp_path_factory, tiny_cfg(mel_bins=bins, subsampling_channels=C, num_layers=1))
    Tm = 1001
    B8 = first_batch_where(gm, lambda v: v["c1d1"][4] == 8, Tm=Tm)
    assert B8 > 1
    B = B8 if large else B8 - 1
    v = gm.conv_variants(B=B, Tm=Tm)
    assert v["c1d1"] == c1_want(C, bins, large) and v["dw2"] == DW2_OF[bins], v
    feats = feats_of(C + bins, B, Tm, bins)
    G.assert_bits_equal(gm.subsample(feats), om.subsampling(feats), f"subsampling C={C} bins={bins} B={B} ({v['rows_h2']} rows after dw1)")


TM_EDGES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 31, 32, 33, 63, 65]      # every residue of Tm mod 8, H2 not a multiple of the 8-row strip, one-row images
SUB_EDGE_MODELS = [(32, 80), (32, 96), (64, 80), (64, 72)]


@pytest.mark.parametrize("Tm", TM_EDGES)
@pytest.mark.parametrize("C,bins", SUB_EDGE_MODELS)
def test_subsampling_short_images(tmp_path_factory, C, bins, Tm):
    """Images of 1 .. 17 rows after dw1: alone (strips of 2 rows) and in a batch large enough for the strips of 8 -- the last strip of every
    utterance partial, utterance edges every few rows of the packed row axis."""
    W, om, gm = pair(tmp_path_factory, tiny_cfg(mel_bins=bins, subsampling_channels=C, num_layers=1))
    B8 = first_batch_where(gm, lambda v: v["c1d1"][4] == 8, Tm=Tm)
    for B, large in ((1, False), (B8, True)):
        v = gm.conv_variants(B=B, Tm=Tm)
        assert v["c1d1"] == c1_want(C, bins, large) and v["dw2"] == DW2_OF[bins], v
        feats = feats_of(Tm, B, Tm, bins)
        G.assert_bits_equal(gm.subsample(feats), om.subsampling(feats), f"subsampling C={C} bins={bins} Tm={Tm} B={B}")


@pytest.mark.parametrize("d,B,Tm", [(512, 64, 1001), (1024, 32, 3001)])
def test_subsampling_benchmark_shapes(tmp_path_factory, d, B, Tm):
    """The shapes the benchmarks time: tdt-ctc-110m sizes at 64 x 10 s (uniform indexing of the packed kernel over 64 utterances: 64 x 32 row strips
    x 5 column chunks) and tdt-600m sizes (128 bins) at 32 x 30 s."""
    cfg = wide_cfg(d)
    W, om, gm = pair(tmp_path_factory, cfg, seed=3)
    v = gm.conv_variants(B=B, Tm=Tm)
    assert v["c1d1"] == C1_PACKED and v["dw2"] == DW2_OF[cfg.mel_bins], v
    feats = feats_of(d, B, Tm, cfg.mel_bins)
    G.assert_bits_equal(gm.subsample(feats), om.subsampling(feats), f"subsampling {cfg.name} B={B} Tm={Tm}")


# mel frames per clip: a 1-frame clip, clips of one strip or less, lengths that end mid-strip (H2 = 34, 51, 84, 126, 195, 251, 301: none a
# multiple of 8), enough of them to pass the strip threshold
RAGGED_TM = [1, 2, 3, 5, 9, 13, 29, 33, 37, 61, 67, 101, 133, 203, 333, 501, 777, 1001, 1203]


@pytest.mark.parametrize("C,bins,large", [(32, 80, True), (64, 96, True), (32, 96, True), (64, 96, False)])
def test_subsampling_ragged(tmp_path_factory, C, bins, large):
    """A packed batch of clips of many lengths through pk_encode_ragged (subsampling only): per clip the bits of the oracle's single-clip run."""
    W, om, gm = pair(tmp_path_factory, tiny_cfg(mel_bins=bins, subsampling_channels=C, num_layers=1))
    tm = RAGGED_TM if large else RAGGED_TM[:14]
    v = gm.conv_variants(n_mel_frames=tm)
    assert v["c1d1"] == c1_want(C, bins, large) and v["dw2"] == DW2_OF[bins], v
    rng = np.random.default_rng(C + bins)
    fl = [rng.standard_normal((t, bins)).astype(np.float32) for t in tm]
    got = gm.encode_ragged(fl, 0, 0)
    for i, f in enumerate(fl):
        G.assert_bits_equal(got[i], om.subsampling(f[None])[0], f"ragged subsampling C={C} bins={bins}, clip {i} ({tm[i]} mel frames)")


# ---- conv module --------------------------------------------------------------------------------------------------------------------------
def block_model(tmp_path_factory, d, kc):
    cfg = tiny_cfg(conv_kernel_size=kc, num_layers=1) if d == 128 else wide_cfg(d, conv_kernel_size=kc)
    return pair(tmp_path_factory, cfg, seed=3)


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("kc", [9, 31])
def test_conv_module_grid(tmp_path_factory, kc, d, large):
    """Taps x hidden sizes x the last batch with strips of 2 frames / the first with strips of 8, T = 126 (the last strip of 8 holds 6 frames):
    the encoder cut after the conv module of block 0 against the oracle's."""
    W, om, gm = block_model(tmp_path_factory, d, kc)
    Tm = 1001
    B8 = first_batch_where(gm, lambda v: v["dwconv"][3] == 8, Tm=Tm)
    assert B8 > 1
    B = B8 if large else B8 - 1
    v = gm.conv_variants(B=B, Tm=Tm)
    assert v["dwconv"] == DW[(kc, 8 if large else 2)], v
    feats = feats_of(kc + d, B, Tm, om.cfg.mel_bins)
    want = om.conformer_block(0, om.subsampling(feats), stop_after=3)
    G.assert_bits_equal(gm.encode(feats, stop_layer=0, stop_stage=3), want, f"conv module kc={kc} d={d} B={B} ({v['rows_t']} frames)")


T_EDGES = [1, 2, 3, 7, 8, 9, 14, 15, 16, 17, 30, 31, 32, 33, 126, 127]


@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("kc", [9, 31])
def test_conv_module_short_utterances(tmp_path_factory, kc, T):
    """One block on free inputs of T frames, alone and in a batch past the strip switch.  With 31 taps, T <= 15 means every window hangs over both
    ends of the utterance; T = 1 .. 9 puts an utterance edge inside (nearly) every strip of 8."""
    W, om, gm = block_model(tmp_path_factory, 128, kc)
    B8 = first_batch_where(gm, lambda v: v["dwconv"][3] == 8, T=T)
    pe = om_pos(T, 128)
    for B, tt in ((1, 2), (B8, 8)):
        v = gm.conv_variants(B=B, T=T)
        assert v["dwconv"] == DW[(kc, tt)] and v["rows_t"] == B * T, v
        x = np.random.default_rng(T).standard_normal((B, T, 128)).astype(np.float32)
        G.assert_bits_equal(gm.conformer_blocks(x), om.conformer_block(0, x, pe), f"block kc={kc} T={T} B={B}")


def om_pos(T, d):
    import oracle
    return oracle.pos_emb(T, d)


RAGGED_T = [1, 2, 7, 31, 32, 33, 64, 65, 100, 5]                    # tests/test_gpu_ragged.py::test_conformer_blocks_ragged_vs_uniform


@pytest.mark.parametrize("large", [False, True])
def test_conv_module_ragged_31_taps(tmp_path_factory, large):
    """31 taps on a packed batch: per clip the oracle's single-clip block and the engine's own single-clip run."""
    W, om, gm = block_model(tmp_path_factory, 128, 31)
    T = RAGGED_T + ([126, 127, 125] * 5 if large else [])
    tm = [8 * t - 7 for t in T]
    v = gm.conv_variants(n_mel_frames=tm)
    assert v["rows_t"] == sum(T) and v["dwconv"] == DW[(31, 8 if large else 2)], v
    rng = np.random.default_rng(3)
    xs = [rng.standard_normal((t, 128)).astype(np.float32) for t in T]
    got = gm.conformer_blocks_ragged(xs)
    for i, x in enumerate(xs):
        G.assert_bits_equal(got[i], om.conformer_block(0, x[None], om_pos(T[i], 128))[0], f"ragged 31 taps, clip {i} (T = {T[i]}) vs the oracle")
        G.assert_bits_equal(got[i], gm.conformer_blocks(x[None])[0], f"ragged 31 taps, clip {i} (T = {T[i]}) vs the engine's single-clip run")


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
def test_block_stages_past_every_switch_110m(tmp_path_factory, stage):
    """tdt-ctc-110m sizes, 17 x 10 s: 2142 frames -- past the conv module's strip switch, past the small-M GEMM rows and (4267 rows after dw1) past the
    subsampling's strip switch at once: every cut of block 0 against the oracle.  Between "stage-exact at B = 2" (tests/test_gpu_encoder.py) and
    "token-exact at B = 64" (tests/test_gpu_e2e.py)."""
    W, om, gm = block_model(tmp_path_factory, 512, 9)
    B, Tm = 17, 1001
    v = gm.conv_variants(B=B, Tm=Tm)
    assert v["dwconv"] == DW[(9, 8)] and v["c1d1"] == C1_PACKED and v["dw2"] == DW2_X5, v
    feats = feats_of(17, B, Tm, 80)
    want = om.conformer_block(0, om.subsampling(feats), stop_after=stage)
    G.assert_bits_equal(gm.encode(feats, stop_layer=0, stop_stage=stage), want, f"110m sizes, B = {B}: block 0 stage {stage}")


def test_conv_module_31_taps_bf16_output(tmp_path_factory, orc):
    """The kernel's bf16 store (the tolerance-class mode: its output is the next product's bf16 operand) with 31 taps, against the bf16-mode oracle
    within the bounds tests/test_gpu_bf16.py::test_bf16_tiny_model_vs_bf16_oracle applies."""
    from test_gpu_bf16 import close
    cfg = tiny_cfg(subsampling_channels=64, gemm_bf16=True, conv_kernel_size=31)
    W, om, gm = pair(tmp_path_factory, cfg, seed=5)
    pcm = synth.synth_pcm(3, 32000, seed=21)
    feats = gm.mel(pcm)
    v = gm.conv_variants(B=3, Tm=feats.shape[1])
    assert v["dwconv"] == DW[(31, 2)], v
    enc, oenc = gm.encode(feats), om.encoder(feats)
    close(enc, oenc, "tiny, 31 taps")
    fp32 = orc.Model(dataclasses.replace(cfg, gemm_bf16=False), W).encoder(feats)
    assert np.abs(oenc - fp32).max() > 1e-3, "the bf16 oracle mode must actually differ from fp32"
    assert np.abs(enc - oenc).mean() < np.abs(oenc - fp32).mean(), "GPU bf16 should be closer to the bf16 oracle than bf16 is to fp32"


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_has_a_case():
    """The union of what the cases of this module (and the streaming cases of tests/test_gpu_stream.py::test_stream_stages_tiny_conv_sizes) assert
    they launch is every instantiation the four launchers have."""
    have = set()
    for C, bins, large in SUB_GRID + [(C, b, l) for C, b in SUB_EDGE_MODELS for l in (False, True)]:
        have |= {c1_want(C, bins, large), DW2_OF[bins]}
    have |= {C1_PACKED}                                               # test_subsampling_benchmark_shapes, test_block_stages_past_every_switch_110m
    have |= {DW[(kc, tt)] for kc in (9, 31) for tt in (2, 8)}         # test_conv_module_grid, test_conv_module_short_utterances
    have |= {want for _, _, want in STREAM_CONV_CASES}
    every = set(capi.diag_conv_instantiations())
    assert len(every) >= 13
    assert every - have == set(), f"instantiations no case of this module launches: {sorted(every - have)}"
    assert have - every == set(), f"cases written for instantiations the library does not list: {sorted(have - every)}"
