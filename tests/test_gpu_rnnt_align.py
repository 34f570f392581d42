"""GPU: forced alignment and transcript scoring of a model with the plain RNN-T head (the model of test_gpu_decode.py::test_rnnt_head) -- the lattice
the device computes from the model, and the walks on it through the model entry points."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(40, 12), (33, 1), (9, 0), (40, 12)]                      # 1115 lattice rows; chunk_rows = 40 puts chunk edges between and inside the utterances


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    cfg = G.tiny(head="rnnt", durations=[], joint_prefix="joint_.", ctc_vocab_size=0, name="tinyrnnt")
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tr"), cfg, seed=12)
    rng = np.random.default_rng(3)
    encs = []
    for T, _ in SHAPES:
        x = rng.standard_normal((T, cfg.hidden_size)).astype(np.float32)
        encs.append((x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True))
    ids = [rng.integers(0, cfg.blank_id, size=U).astype(np.int32) for _, U in SHAPES]
    lats, guard = gm.rnnt_lattice(encs, ids)
    assert np.all(guard == 0x7FC5A5A5)
    return cfg, W, gm, encs, ids, lats


def same(got, want, what):
    for k in want:
        G.assert_bits_equal(np.asarray(got[k]), np.asarray(want[k]), f"{what}: {k}")


def test_chunk_edges_change_no_bit(setup):
    cfg, W, gm, encs, ids, lats = setup
    got, guard = gm.rnnt_lattice(encs, ids, chunk_rows=40)
    assert np.all(guard == 0x7FC5A5A5), "a word past the written extent was touched"
    for b in range(len(SHAPES)):
        G.assert_bits_equal(got[b][0], lats[b][0], f"utterance {b}: label log-probs")
        G.assert_bits_equal(got[b][1], lats[b][1], f"utterance {b}: blank log-probs")


def test_model_walks_equal_the_walks_on_the_kept_values(setup):
    cfg, W, gm, encs, ids, lats = setup
    for b, (ga, gt, wa, wt) in enumerate(zip(gm.rnnt_align_decode(encs, ids), gm.rnnt_total_decode(encs, ids), capi.rnnt_align(lats), capi.rnnt_total(lats))):
        same(ga, wa, f"utterance {b}: alignment")
        same(gt, wt, f"utterance {b}: total")
        assert ga["ok"] == 1 and gt["total"] >= ga["score"]
    # two transcripts of one clip share its rows: clip_of
    two = gm.rnnt_total_decode(encs[:2], [ids[0], ids[1], ids[1]], clip_of=[0, 1, 1])
    same(two[0], capi.rnnt_total(lats[:1])[0], "clip_of, hypothesis 0")
    same(two[2], two[1], "clip_of, the same transcript twice")


def test_lattice_against_float64(setup):
    """The kept values against a float64 restatement of the prediction net and the joint from the same weights.  u = 2^-24, first order, every fp32 dot
    product of n terms (any order, fused or not) within n u sum|a_i b_i|:
      prediction net  a gate is 2 Hp products + 2 adds: dg <= (2 Hp + 2) u sum|.| + |W_hh| dh; each gate function moves by its own slope at the float64
                      value (s (1 - s), 1 - tanh^2) times dg, plus 4 u of its own; dc <= |c| df + f dc + |g| di + i dg + 3 u (|c| + 1);
                      dh <= |tanh c| do + o (1 - tanh^2 c) dc + 3 u -- carried as vectors over the U + 1 steps (with the largest slopes 1/4 and 1
                      in their place the recurrence grows without limit over a dozen steps and bounds nothing)
      joint input     enc_proj: (d + 1) u sum|.|; pred_proj: Hp u sum|.| + |W_p| dh; z = relu(sum): + u |z|
      logit           (J + 1) u sum_j |z_j w_vj| + |b_v|  (the J-term chain of the heads product)  + sum_j |w_vj| dz_j
      log-softmax     (x - m) - lse moves by at most twice the largest logit error of the row; the V-term sum of exponentials in [0, 1], its
                      dexpf / dlogf and the two subtractions add (V + 16) u + 2 u |out|
    The test prints the largest ratio of an error to its bound (profiles/rnnt_align.md records it).  Every term is a worst case, so the bound is loose: the
    measured ratio is 0.0009, about 1e-3 in a log-prob is tolerated in the first columns, and the recurrence through |W_hh| still grows with u: by u = 12 the
    bound is 0.4 and says nothing about those columns (measured there: 1e-6).  It catches a wrong index, weight, bias or softmax; it would not catch a bf16 product.
    The companion below it does for the short strings (utterances 1 and 2, RMS bound 1.2e-4 against 3e-7 measured): the RMS error, where roundings
    average out, is held to sqrt(n) instead of n per chain."""
    cfg, W, gm, encs, ids, lats = setup
    u = 2.0 ** -24
    f = lambda k: np.asarray(W[k], np.float64)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    Hp, J, V, d, q = cfg.pred_hidden, cfg.joint_hidden, cfg.vocab_size, cfg.hidden_size, "prediction_.lstm_.cells_.0."
    assert cfg.num_lstm_layers == 1
    Wih, bih, Whh, E = f(q + "input_proj_.weight"), f(q + "input_proj_.bias"), f(q + "hidden_proj_.weight"), f("prediction_.embed_.weight")
    We, be, Wp, Wo, bo = (f("joint_." + k) for k in ("enc_proj_.weight", "enc_proj_.bias", "pred_proj_.weight", "out_proj_.weight", "out_proj_.bias"))
    worst = 0.0
    for b, (enc, tok) in enumerate(zip(encs, ids)):
        h, c, dh, dc, pp, dpp = np.zeros(Hp), np.zeros(Hp), np.zeros(Hp), np.zeros(Hp), [], []
        for t in [cfg.blank_id] + list(tok):
            g = Wih @ E[t] + bih + Whh @ h
            dg = (2 * Hp + 2) * u * (np.abs(Wih) @ np.abs(E[t]) + np.abs(bih) + np.abs(Whh) @ np.abs(h)) + np.abs(Whh) @ dh
            si, sf, tg, so = (fn(x) for fn, x in zip((sig, sig, np.tanh, sig), np.split(g, 4)))
            di, df, dgg, do = (x * s + 4 * u for x, s in zip(np.split(dg, 4), (si * (1 - si), sf * (1 - sf), 1 - tg * tg, so * (1 - so))))
            dc = np.abs(c) * df + sf * dc + np.abs(tg) * di + si * dgg + 3 * u * (np.abs(c) + 1)
            c = sf * c + si * tg
            h, dh = so * np.tanh(c), np.abs(np.tanh(c)) * do + so * (1 - np.tanh(c) ** 2) * dc + 3 * u
            pp.append(Wp @ h)
            dpp.append(Hp * u * (np.abs(Wp) @ np.abs(h)) + np.abs(Wp) @ dh)
        x = enc.astype(np.float64)
        ep, dep = x @ We.T + be, (d + 1) * u * (np.abs(x) @ np.abs(We).T + np.abs(be))
        z = np.maximum(ep[:, None, :] + np.asarray(pp)[None], 0.0)                              # [T][U+1][J]
        dz = dep[:, None, :] + np.asarray(dpp)[None] + u * z
        logit = z @ Wo.T + bo
        dlogit = ((J + 1) * u * (z @ np.abs(Wo).T + np.abs(bo)) + dz @ np.abs(Wo).T).max(-1)    # the row's largest
        m = logit.max(-1, keepdims=True)
        out = logit - m - np.log(np.exp(logit - m).sum(-1, keepdims=True))
        want_blk = out[:, :, cfg.blank_id]
        for name, got, want, dl in (("blk", lats[b][1], want_blk, dlogit),
                                    ("lab", lats[b][0], out[:, np.arange(len(tok)), tok] if len(tok) else out[:, :0, 0], dlogit[:, :len(tok)])):
            bound = 2 * dl + (V + 16) * u + 2 * u * np.abs(want)
            ratio = np.abs(got.astype(np.float64) - want) / bound
            if ratio.size:
                worst = max(worst, float(ratio.max()))
                print(f"utterance {b} {name}: max |err| {np.abs(got - want).max():.3e}, max err / bound {ratio.max():.4f}")
            assert np.all(ratio <= 1.0), f"utterance {b} {name}: {ratio.max()} of the bound"
            # probabilistic companion: independent roundings add in quadrature, so the J-term and d-term chains cost sqrt(J), sqrt(d) roundings of
            # u x (the sum of magnitudes), not J and d: the worst-case bound shrunk by sqrt(min(J, d, Hp)) = 8 here bounds the RMS with room for the 3-sigma tail
            if ratio.size:
                rms = float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)))
                print(f"utterance {b} {name}: rms err {rms:.3e}, rms bound {float(np.sqrt(np.mean(bound ** 2))) / np.sqrt(min(J, d, Hp)):.3e}")
                assert rms <= float(np.sqrt(np.mean(bound ** 2))) / np.sqrt(min(J, d, Hp))
    print(f"largest ratio to the bound: {worst:.4f}")


def test_greedy_path_is_below_the_alignment_and_the_total(setup):
    """The greedy decode's own tokens, aligned: the alignment's score is >= the fp32 left-to-right sum of the greedy path through the same lattice
    (exactly: fp32 addition is monotone, so the max-plus walk dominates every path), and the total is >= the score."""
    cfg, W, gm, encs, ids, lats = setup
    x = np.random.default_rng(6).standard_normal((4, 50, cfg.hidden_size)).astype(np.float32)      # the input of test_gpu_decode.py::test_rnnt_head
    enc = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    g = gm.tdt_decode(enc)
    gids = [g["ids"][b, :g["lens"][b]].astype(np.int32) for b in range(4)]
    assert sum(len(x) for x in gids) > 0
    lat, _ = gm.rnnt_lattice(enc, gids)
    al, tt = gm.rnnt_align_decode(enc, gids), gm.rnnt_total_decode(enc, gids)
    for b in range(4):
        lab, blk = lat[b]
        T, U = blk.shape[0], blk.shape[1] - 1
        acc, k = F(0.0), 0
        for t in range(T):
            while k < U and g["start"][b, k] == t:
                acc, k = F(acc + lab[t, k]), k + 1
            acc = F(acc + blk[t, k])
        assert k == U and al[b]["ok"] == 1
        assert al[b]["score"] >= acc and tt[b]["total"] >= al[b]["score"], (b, al[b]["score"], acc, tt[b]["total"])


def test_ragged_form_equals_uniform_form_and_groups_change_no_bit(setup):
    """Uniform against ragged clip by clip; then 260 utterances in one call, which is two groups (256 + 4): the second group's offsets are rebased,
    and its results land behind the first group's."""
    cfg, W, gm, encs, ids, lats = setup
    enc, tok = np.stack([encs[0], encs[3]]), [ids[0], ids[3]]
    uni_a, uni_t = gm.rnnt_align_decode(enc, tok), gm.rnnt_total_decode(enc, tok)
    rag_a, rag_t = gm.rnnt_align_decode(encs, ids), gm.rnnt_total_decode(encs, ids)
    for i, b in enumerate((0, 3)):
        same(uni_a[i], rag_a[b], f"clip {b}: alignment")
        same(uni_t[i], rag_t[b], f"clip {b}: total")
    n = 260
    many = [ids[b % 4][:1 + b % 7] for b in range(n)]
    clip_of = [b % 4 for b in range(n)]
    tt = gm.rnnt_total_decode(encs, many, clip_of=clip_of)
    al = gm.rnnt_align_decode([encs[c] for c in clip_of], many)
    for b in (0, 5, 255, 256, 257, 259):
        same(tt[b], gm.rnnt_total_decode([encs[clip_of[b]]], [many[b]])[0], f"hypothesis {b} of {n}: total")
        same(al[b], gm.rnnt_align_decode([encs[clip_of[b]]], [many[b]])[0], f"utterance {b} of {n}: alignment")


def test_one_call_from_pcm_equals_the_stages(setup):
    cfg, W, gm, encs, ids, lats = setup
    clips = [synth.synth_pcm(1, n, seed=20 + i)[0] for i, n in enumerate((16000, 9000))]
    enc = gm.encode_ragged(gm.mel_ragged(clips))
    tok = [ids[0][:5], ids[1]]
    want_a, want_t = gm.rnnt_align_decode(enc, tok), gm.rnnt_total_decode(enc, tok)
    got_a, got_t = gm.align_rnnt(clips, ids=tok), gm.score_rnnt(clips, ids=tok)
    for b in range(2):
        assert got_a[b]["ok"] == want_a[b]["ok"] == 1 and got_a[b]["token_ids"] == tok[b].tolist()
        G.assert_bits_equal(np.float32(got_a[b]["score"]), want_a[b]["score"], f"clip {b}: score")
        assert got_a[b]["start"] == want_a[b]["start"].tolist() and got_a[b]["end"] == want_a[b]["end"].tolist()
        G.assert_bits_equal(np.asarray(got_a[b]["conf"], np.float32), want_a[b]["conf"], f"clip {b}: conf")
        same(got_t[b], want_t[b], f"clip {b}: total")


def test_refusals(setup, tmp_path_factory):
    cfg, W, gm, encs, ids, lats = setup
    _, _, tdt = G.make_pair(tmp_path_factory.mktemp("tt"), G.tiny(), seed=31)
    x = np.zeros((1, 4, 128), np.float32)
    for call in (lambda: tdt.rnnt_align_decode(x, [[1, 2]]), lambda: tdt.rnnt_total_decode(x, [[1, 2]]), lambda: tdt.rnnt_lattice(x, [[1, 2]])):
        with pytest.raises(capi.PkError) as e:
            call()
        assert e.value.code == -7 and "pk_tdt_align" in str(e.value)    # PK_ERR_UNSUPPORTED, naming the TDT entry point
    for bad in ([cfg.blank_id], [cfg.vocab_size], [-1]):
        with pytest.raises(capi.PkError) as e:
            gm.rnnt_align_decode(encs[:1], [bad])
        assert e.value.code == -1                                       # PK_ERR_INVALID
    with pytest.raises(capi.PkError) as e:
        gm.rnnt_align_decode(encs[:1], [np.zeros(1024, np.int32)])
    assert e.value.code == -7
