"""GPU: the bf16 TDT spotting lattice kernel (kernels/tdt_kws_bf16.hip) against a float64 reference under a derived bound, and the model route it
opens for gemm_bf16 models (pk_model_set_tdt_kws_bf16): the walk on the kernel's arcs, the arcs against the bf16 oracle, the refusals around it."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth
from decode_gemv_ref import bf16

from test_gpu_tdt_kws_model import oracle_lattice, ref_arrays, same_arrays

pytestmark = pytest.mark.gpu

CLIP_T = [40, 9, 1]
SLOT_L = [1, 3, 12, 64]
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 3), (2, 0), (2, 2)]      # (clip, net slot): 1396 rows, pair edges at 80 / 240 / 760 / 796 / 1381 / 1383
LOGP_TOL, LOGP_MEAN = 3e-2, 8e-3                                      # tests/test_gpu_600m_depth.py: bf16 teacher-forced log-probs against the bf16 oracle


def reference(ep, pp, wld, bld, ids, T, row0, net_of, n_net, V, D, blank):
    """float64 arcs and their bounds, packed as the kernel packs them -> (lab, blk, dl, bound_lab, bound_blk, bound_dl).  B[n] = 2e-6 (|z| . |W[n]| +
    |bld[n]|) + 1e-6 per logit (the project's bound for a bf16 MFMA product); the computed maximum moves by at most max_k B[k] over the head's
    columns; the one fp32 subtraction adds 2^-24 |out|."""
    W = bf16(wld).astype(np.float64)
    out = [[] for _ in range(6)]
    for p, kw in enumerate(ids):
        L = len(kw)
        s = ep[row0[p]:row0[p] + T[p], None, :] + pp[np.arange(L + 1) * n_net + net_of[p]][None, :, :]          # fp32 + fp32 -> fp32
        z = bf16(np.where(s > 0, s, np.float32(0))).astype(np.float64).reshape(T[p] * (L + 1), -1)
        logit = z @ W.T + bld
        Bn = 2e-6 * (z @ np.abs(W).T + np.abs(bld)) + 1e-6

        def head(lo, hi):
            x = logit[:, lo:hi] - logit[:, lo:hi].max(1, keepdims=True)
            return x, Bn[:, lo:hi] + Bn[:, lo:hi].max(1, keepdims=True) + 2.0 ** -24 * np.abs(x)
        xl, bl = head(0, V)
        xd, bd = head(V, V + D)
        at, col = np.arange(T[p] * (L + 1)).reshape(T[p], L + 1)[:, :L].ravel(), np.tile(np.asarray(kw, np.int64), T[p])
        for k, v in enumerate((xl[at, col], xl[:, blank], xd.ravel(), bl[at, col], bl[:, blank], bd.ravel())):
            out[k].append(v)
    return tuple(np.concatenate(o) for o in out)


# (64, 78, 4): V + D = 82 inside one 64-column block pair; (128, 1025, 5): tdt-ctc-110m's heads (both 128-row tiles); (640, 8193, 5): tdt-600m's,
# 96-row tiles; (1024, 300, 5): the 64-row tiles of the widest joints
@pytest.mark.parametrize("J,V,D", [(64, 78, 4), (128, 1025, 5), (640, 8193, 5), (1024, 300, 5)])
def test_kernel_within_the_bound_of_the_float64_reference(J, V, D):
    rng = np.random.default_rng(J + V)
    T = [CLIP_T[c] for c, _ in PAIRS]
    row0 = [int(np.sum(CLIP_T[:c])) for c, _ in PAIRS]
    net_of = [k for _, k in PAIRS]
    slot_ids = [np.asarray(([0, V - 2, 5, 2] * 17)[k:k + L], np.int32) for k, L in enumerate(SLOT_L)]
    ids = [slot_ids[k] for k in net_of]
    n_net, blank = len(SLOT_L), V - 1
    ep = rng.standard_normal((sum(CLIP_T), J)).astype(np.float32)
    pp = rng.standard_normal(((max(SLOT_L) + 1) * n_net, J)).astype(np.float32)
    wld = (rng.standard_normal((V + D, J)) / np.sqrt(J)).astype(np.float32)
    wld[2] *= 8                                                      # for some rows the maximum logit arrives in the first column block ...
    wld[V - 1] *= 8                                                  # ... for others in the last one that holds labels (a partial one)
    bld = (0.1 * rng.standard_normal(V + D)).astype(np.float32)
    want = reference(ep, pp, wld, bld, ids, T, row0, net_of, n_net, V, D, blank)
    assert max(b.max() for b in want[3:]) <= 1e-3, "a condition on the test: the bound must stay sharp enough to see a dropped column block"
    got = capi.tdt_kws_lattice_bf16(ep, pp, wld, bld, ids, T, row0, net_of, n_net, V, D, blank)
    Gd = capi.TDT_LATTICE_GUARD
    for name, g, w, bound in zip(("lab", "blk", "dl"), got, want[:3], want[3:]):
        assert np.all(g[-Gd:].view(np.uint32) == 0x7FC5A5A5), f"{name}: a guard word was written"
        v = g[:-Gd]
        assert np.all(v <= 0) and not np.any(np.signbit(v) & (v == 0)), f"{name}: an arc above +0.0, NaN or -0.0"
        err = np.abs(v.astype(np.float64) - w)
        print(f"{name}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, max bound {bound.max():.3e}")
        assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} of {err.size} values outside the bound, worst {(err / bound).max():.2f} x"
    assert np.all(got[2][:-Gd].reshape(-1, D).max(1).view(np.uint32) == 0), "every row's largest duration arc is +0.0"
    assert np.any(got[0][:-Gd].view(np.uint32) == 0) and np.any(got[1][:-Gd].view(np.uint32) == 0), "degenerate test: no row whose label / blank leads"


def refused(fn, *a, msg="gemm_bf16", **k):
    with pytest.raises(capi.PkError) as e:
        fn(*a, **k)
    assert e.value.code == -7 and msg in str(e.value), str(e.value)


def test_model_route_walks_the_kernels_arcs(tmp_path_factory):
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tkws")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tkws16"), cfg, seed=12)
    dur = list(cfg.durations)
    rng = np.random.default_rng(9)
    encs = [rng.standard_normal((T, cfg.hidden_size)).astype(np.float32) for T in (40, 9, 21)]
    kws = [rng.integers(0, cfg.blank_id, size=L).astype(np.int32) for L in (3, 1, 12, 2)]
    clips = [synth.synth_pcm(1, n, seed=70 + i)[0] for i, n in enumerate((32000, 12345, 20000))]
    K, H, ms = len(kws), 4, np.float32(-30.0)
    assert not gm.tdt_kws_bf16()
    refused(gm.tdt_kws_decode, encs, kws)                            # off (the default): the gemm_bf16 refusal
    gm.set_tdt_lattice_bf16(True)                                    # the alignment's switch alone opens no spotting
    refused(gm.tdt_kws_decode, encs, kws)
    refused(gm.spot_tdt, clips, ids=[k.tolist() for k in kws])
    gm.set_tdt_lattice_bf16(False)
    gm.set_tdt_kws_bf16(True)
    try:
        assert gm.tdt_kws_bf16() and not gm.tdt_lattice_bf16()
        refused(gm.tdt_align_decode, encs, [kws[0]] * 3)             # ... and this one opens no alignment
        rep = [encs[c] for c in range(len(encs)) for _ in range(K)]
        lats, guard = gm.tdt_kws_lattice(rep, kws * len(encs))
        assert np.all(guard == 0x7FC5A5A5)
        assert all(np.all(l["top"].view(np.uint32) == 0) for l in lats), "top = +0.0: the arcs come back normalised"
        got = gm.tdt_kws_decode(encs, kws, max_hits=H, min_score=float(ms))
        same_arrays(got, ref_arrays(lats, dur, len(encs), K, H, ms), "the walk is exact on the arcs it gets")
        assert got["n_hits"].sum() > 0, "degenerate test: no hit anywhere"
        worst, mean = 0.0, []
        for p in (0, 4, 5, 6, 7):                                    # the bf16 oracle's teacher-forced rows, normalised the same way in float64
            l = lats[p]
            lab, blk, dl, top = (x.astype(np.float64) for x in oracle_lattice(om, rep[p], (kws * len(encs))[p]))
            for g, w in ((l["lab"], lab - top[:, :-1]), (l["blk"], blk - top), (l["dl"], dl - dl.max(2, keepdims=True))):
                d = np.abs(g.astype(np.float64) - w)
                worst = max(worst, d.max()); mean.append(d.mean())
        print(f"arcs vs the bf16 oracle: max {worst:.3e}, mean {max(mean):.3e}")
        assert worst <= 2 * LOGP_TOL and max(mean) <= 2 * LOGP_MEAN   # an arc is a difference of two log-probs
        assert len(gm.tdt_kws_decode_timed(encs, kws, max_hits=H, reps=2)) == 3
        # from PCM: the one-call entry point equals its stages
        enc = gm.encode_ragged(gm.mel_ragged(clips))
        res, stage = gm.spot_tdt(clips, ids=[k.tolist() for k in kws], max_hits=H), gm.tdt_kws_decode(list(enc), kws, max_hits=H)
        f32 = np.float32
        for c in range(len(clips)):
            for k in range(K):
                assert len(res[c][k]) == int(stage["n_hits"][c, k]), (c, k)
                for j, (s, e, v) in enumerate(res[c][k]):
                    assert f32(s) == f32(f32(stage["start"][c, k, j]) * f32(0.08)) and f32(e) == f32(f32(stage["end"][c, k, j] + 1) * f32(0.08)), (c, k, j)
                    G.assert_bits_equal(f32(v), f32(stage["score"][c, k, j]), f"clip {c} keyword {k} hit {j}: score")
        refused(gm.tdt_beam_decode, encs[0][None], max_tokens=8, msg="")     # not opened
    finally:
        gm.set_tdt_kws_bf16(False)
    refused(gm.tdt_kws_decode, encs, kws)                            # off again: the refusal is back
    refused(gm.spot_tdt, clips, ids=[k.tolist() for k in kws])


def test_fp32_model_refuses_the_switch(tmp_path_factory):
    _, _, gm = G.make_pair(tmp_path_factory.mktemp("tkws32"), G.tiny(), seed=31)
    with pytest.raises(capi.PkError) as e:
        gm.set_tdt_kws_bf16(True)
    assert e.value.code == -7
    assert not gm.tdt_kws_bf16()
