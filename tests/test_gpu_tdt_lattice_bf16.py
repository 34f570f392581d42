"""GPU: the bf16 TDT lattice kernel (kernels/tdt_lattice_bf16.hip) against the float64 reference of tests/tdt_lattice_bf16_ref.py under its derived
bound, and the model route it opens for gemm_bf16 models (pk_model_set_tdt_lattice_bf16): the walks on the kernel's rows, the refusals around it."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

import tdt_align_ref as A
import tdt_lattice_bf16_ref as R
import tdt_total_ref as TT

pytestmark = pytest.mark.gpu

SHAPES = [(40, 1), (9, 12), (20, 0), (1, 0), (3, 70)]                # 431 lattice rows: utterance edges inside row tiles, U = 0, T = 1
LOGP_TOL, LOGP_MEAN = 3e-2, 8e-3                                      # tests/test_gpu_600m_depth.py: bf16 teacher-forced log-probs against the bf16 oracle


# (64, 78, 4): V + D = 82 inside one 64-column block pair; (128, 1025, 5): tdt-ctc-110m's heads; (640, 8193, 5): tdt-600m's, 96-row tiles;
# (1024, 300, 5): the 64-row tiles of the widest joints (the 128-row form runs the first two)
@pytest.mark.parametrize("J,V,D", [(64, 78, 4), (128, 1025, 5), (640, 8193, 5), (1024, 300, 5)])
def test_kernel_within_the_bound_of_the_float64_reference(J, V, D):
    rng = np.random.default_rng(J + V)
    n_frames = np.asarray([T for T, _ in SHAPES], np.int32)
    ids = [np.asarray(([0, V - 2, 5, 5] * 18)[:U], np.int32) for _, U in SHAPES]
    B, u_max, blank = len(SHAPES), max(U for _, U in SHAPES), V - 1
    ep = rng.standard_normal((int(n_frames.sum()), J)).astype(np.float32)
    pp = rng.standard_normal(((u_max + 1) * B, J)).astype(np.float32)
    wld = (rng.standard_normal((V + D, J)) / np.sqrt(J)).astype(np.float32)
    wld[2] *= 8                                                      # for some rows the maximum logit arrives in the first column block ...
    wld[V - 1] *= 8                                                  # ... for others in the last one that holds labels (a partial one)
    bld = (0.1 * rng.standard_normal(V + D)).astype(np.float32)
    want = R.reference(ep, pp, wld, bld, ids, n_frames, V, D, blank)
    assert max(b.max() for b in want[3:]) <= 1e-3, "a condition on the test: the bound must stay sharp enough to see a dropped column block"
    got = capi.tdt_lattice_bf16(ep, pp, wld, bld, ids, n_frames, V, D, blank)
    Gd = capi.TDT_LATTICE_GUARD
    for name, g, w, bound in zip(("lab", "blk", "dl"), got, want[:3], want[3:]):
        assert np.all(g[-Gd:].view(np.uint32) == 0x7FC5A5A5), f"{name}: a guard word was written"
        err = np.abs(g[:-Gd].astype(np.float64) - w)
        print(f"{name}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, max bound {bound.max():.3e}")
        assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} of {err.size} values outside the bound, worst {(err / bound).max():.2f} x"


@pytest.fixture(scope="module")
def bf16_model(tmp_path_factory):
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tlat")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tlat16"), cfg, seed=12)
    return cfg, om, gm


def refused(fn, *a, **k):
    with pytest.raises(capi.PkError) as e:
        fn(*a, **k)
    assert e.value.code == -7, str(e.value)


def test_model_route_walks_the_kernels_rows(bf16_model):
    cfg, om, gm = bf16_model
    dur = list(cfg.durations)
    rng = np.random.default_rng(3)
    shapes = [(40, 12), (33, 1), (9, 0)]
    encs = [rng.standard_normal((T, cfg.hidden_size)).astype(np.float32) for T, _ in shapes]
    ids = [rng.integers(0, cfg.blank_id, size=U).astype(np.int32) for _, U in shapes]
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 20000))]
    pids = [[1, 2, 3], [4], [5, 6]]
    assert not gm.tdt_lattice_bf16()
    refused(gm.tdt_align_decode, encs, ids)                         # off (the default): the gemm_bf16 refusal
    gm.set_tdt_lattice_bf16(True)
    try:
        assert gm.tdt_lattice_bf16()
        lat, guard = gm.tdt_lattice(encs, ids)
        assert np.all(guard == 0x7FC5A5A5)
        got = gm.tdt_align_decode(encs, ids)
        tot = gm.tdt_total_decode(encs, ids)
        worst, mean = 0.0, []
        for b, l in enumerate(lat):
            rows = (l["lab"], l["blk"], l["dl"])
            want = A.align(*rows, dur)                               # the walks are exact on the rows they get
            assert got[b]["ok"] == want["ok"] == 1
            for k in ("start", "end", "dur_idx"):
                assert np.array_equal(got[b][k], want[k]), (b, k)
            G.assert_bits_equal(np.float32(got[b]["score"]), np.float32(want["score"]), f"utterance {b}: score")
            G.assert_bits_equal(np.float32(tot[b]["total"]), np.float32(TT.total(*rows, dur)["total"]), f"utterance {b}: total")
            for g, w in zip(rows, A.oracle_lattice(om, encs[b], ids[b])):      # the bf16 oracle's teacher-forced rows
                d = np.abs(g.astype(np.float64) - w)
                if d.size:
                    worst = max(worst, d.max()); mean.append(d.mean())
        print(f"lattice vs the bf16 oracle: max {worst:.3e}, mean {max(mean):.3e}")
        assert worst <= LOGP_TOL and max(mean) <= LOGP_MEAN
        # from PCM: the one-call entry points equal their stages
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        stage, res = gm.tdt_align_decode(enc, [np.asarray(p, np.int32) for p in pids]), gm.align_tdt(clips, ids=pids)
        stot, sc = gm.tdt_total_decode(enc, [np.asarray(p, np.int32) for p in pids]), gm.score_tdt(clips, ids=pids)
        for i, r in enumerate(res):
            assert r["ok"] == stage[i]["ok"] == 1 and r["start"] == stage[i]["start"].tolist() and r["end"] == stage[i]["end"].tolist()
            G.assert_bits_equal(np.float32(r["score"]), np.float32(stage[i]["score"]), f"clip {i}: align_tdt score")
            G.assert_bits_equal(np.float32(sc[i]["total"]), np.float32(stot[i]["total"]), f"clip {i}: score_tdt total")
        refused(gm.tdt_kws_decode, encs[0][None], [np.asarray([1], np.int32)])      # not opened: keyword spotting, the beam
        refused(gm.tdt_beam_decode, encs[0][None], max_tokens=8)
    finally:
        gm.set_tdt_lattice_bf16(False)
    refused(gm.tdt_align_decode, encs, ids)                         # off again: the refusal is back
    refused(gm.score_tdt, clips, ids=pids)


def test_fp32_model_refuses_the_switch(tmp_path_factory):
    cfg = G.tiny()
    _, _, gm = G.make_pair(tmp_path_factory.mktemp("tlat32"), cfg, seed=31)
    refused(gm.set_tdt_lattice_bf16, True)
    assert not gm.tdt_lattice_bf16()
