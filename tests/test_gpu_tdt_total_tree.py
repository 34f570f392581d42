"""GPU: the TDT totals of a clip's transcripts on ONE prefix tree per clip (kernels/tdt_tree.hip).  The walk on host tree
lattices against the fp32 specification tests/tdt_total_ref.py on every hypothesis's chain of columns, BIT FOR BIT, and inside the bound
tests/test_tdt_total_ref.py derives against float64; the model path with the switch on against the switch off, bit for bit; the refusals."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from conftest import pk
from parakeet_cpp_amd import capi, synth

import tdt_align_ref as A
import tdt_total_ref as R

pytestmark = pytest.mark.gpu

FP32_BOUND = 0.06256218                                            # tests/test_tdt_total_ref.py: 4 x the largest |fp32 - float64| up to U = 1534
DURS = {"d01234": [0, 1, 2, 3, 4], "d1": [1], "d08": [0, 8], "d8": R.DURS["d8"]}
# name -> (parents, end nodes); the random trees attach node k to one of the 3 nodes before it, so they are deep and branch
def bushy(n, seed):
    rng = np.random.default_rng(seed)
    par = [-1] + [int(rng.integers(max(0, k - 3), k)) for k in range(1, n)]
    return par, [n - 1, n // 2, int(rng.integers(0, n)), n - 2]
TREES = {
    "root": ([-1], [0]),
    "chain": ([-1, 0, 1, 2, 3, 4], [5]),
    "star": ([-1, 0, 0, 0, 0], [1, 2, 3, 4]),
    "last_token": ([-1, 0, 1, 2, 3, 3, 3], [4, 5, 6]),
    "duplicates": ([-1, 0, 1, 1], [2, 3, 2, 2]),
    "prefix_of_another": ([-1, 0, 1, 2, 3], [4, 2, 0]),
    "n64": bushy(64, 1), "n65": bushy(65, 2), "n257": bushy(257, 3),
}


def chain_of(lat, par, e):
    """tree-to-chain gather: the (lab, blk, dl) of pk_tdt_total over the columns from the root to node e"""
    path = [e]
    while par[path[-1]] >= 0:
        path.append(par[path[-1]])
    path = path[::-1]
    lab, blk, dl = lat
    return np.ascontiguousarray(lab[:, [k - 1 for k in path[1:]]]), np.ascontiguousarray(blk[:, path]), np.ascontiguousarray(dl[:, path])


def check(lats, pars, ends, clip_of, dur, what):
    tt, ok = capi.tdt_total_tree(lats, pars, ends, dur, clip_of)
    for h, e in enumerate(ends):
        c = h if clip_of is None else clip_of[h]
        ch = chain_of(lats[c], pars[c], e)
        want, w64 = R.forward_total(*ch, dur), R.forward_total64(*ch, dur)
        print(what, h, tt[h], want, w64)
        if np.isfinite(w64):                                       # first the specification itself, on the CPU, then the device
            assert abs(float(want) - w64) <= FP32_BOUND and abs(float(tt[h]) - w64) <= FP32_BOUND, (what, h, tt[h], want, w64)
        assert tt[h].view(np.uint32) == want.view(np.uint32) and ok[h] == (1 if want > R.NEG else 0), (what, h, tt[h], want)
    return tt, ok


@pytest.mark.parametrize("dname", list(DURS))
@pytest.mark.parametrize("T", [1, 2, 3, 9, 40])
@pytest.mark.parametrize("tree", list(TREES))
def test_tree_walk_equals_the_specification_on_every_chain(tree, T, dname):
    par, ends = TREES[tree]
    dur = DURS[dname]
    lat = A.make_lattice("peaky", T, len(par) - 1, len(dur), np.random.default_rng(T * 131 + len(par)))
    tt, ok = check([lat], [par], ends, [0] * len(ends), dur, f"{tree} T={T} {dname}")
    if tree == "chain":
        one = capi.tdt_total([lat], dur)[0]
        assert np.float32(one["total"]).view(np.uint32) == tt[0].view(np.uint32) and one["ok"] == ok[0], "a chain is pk_tdt_total's packing"


@pytest.mark.parametrize("dname", ["d01234", "d8"])
def test_tree_walk_at_the_node_limit(dname):
    par, ends = bushy(1536, 4)
    dur = DURS[dname]
    check([A.make_lattice("peaky", 3, 1535, len(dur), np.random.default_rng(9))], [par], ends, [0] * 4, dur, f"1536 nodes {dname}")


def test_ragged_batch_with_a_clip_nobody_asks_about_and_an_unreachable_edge():
    dur = DURS["d01234"]
    rng = np.random.default_rng(21)
    pars = [TREES["last_token"][0], [-1], TREES["n65"][0]]
    lats = [A.make_lattice("ties", T, len(p) - 1, len(dur), rng) for T, p in zip((9, 4, 12), pars)]
    lats[0][0][:, 3] = R.NEG                                       # the edge into node 4 of clip 0 (its hypothesis: ok = 0; siblings 5 and 6 stay finite)
    ends, clip_of = [64, 4, 5, 30, 6, 0], [2, 0, 0, 2, 0, 2]       # shuffled clip_of; clip 1 has no hypothesis
    tt, ok = check(lats, pars, ends, clip_of, dur, "ragged")
    assert ok.tolist() == [1, 0, 1, 1, 1, 1] and tt[1] == R.NEG


# ---- through a model ------------------------------------------------------------------------------------------------------------------------
def bits(res):
    return [(np.float32(r["total"]).view(np.uint32), r["ok"]) for r in res]


def test_model_switch_on_equals_off_equals_every_string_alone(tmp_path_factory):
    cfg = G.tiny()
    W, om, gm = G.make_pair(tmp_path_factory.mktemp("tree_tiny"), cfg, seed=31)
    rng = np.random.default_rng(6)
    encs = []
    for T in (40, 9):
        x = rng.standard_normal((T, cfg.hidden_size)).astype(np.float32)
        encs.append((x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True))
    a, b = (rng.integers(0, cfg.blank_id, size=12).astype(np.int32) for _ in range(2))
    ids = [a, a[:7], np.concatenate([a[:7], b[:3]]), b[:5], b[:4], np.concatenate([b[:4], a[:1]]), b[:4], np.zeros(0, np.int32)]
    clip_of = [0, 1, 0, 1, 0, 1, 1, 0]                             # four strings per clip, prefixes shared within a clip, a duplicate, an empty one
    node_off = capi.tdt_prefix_tree(ids, clip_of, 2)[0]
    n0, n1 = node_off[1], node_off[2] - node_off[1]
    assert n0 + n1 < sum(len(i) + 1 for i in ids) and (40 * n0 + 9 * n1) % 128 != 0
    off = gm.tdt_total_decode(encs, ids, clip_of)
    assert not gm.tdt_total_shared()
    gm.set_tdt_total_shared(True)
    try:
        assert gm.tdt_total_shared()
        on = gm.tdt_total_decode(encs, ids, clip_of)
        assert len(gm.tdt_total_decode_timed(encs, ids, clip_of, reps=1)) == 3
        held = capi.mem_info(gm)[2]
        with pytest.raises(capi.PkError) as e:                     # a tree of 1537 nodes: refused before anything is allocated
            gm.tdt_total_decode(encs[1][None], [np.ones(1536, np.int32)])
        assert e.value.code == -7 and capi.mem_info(gm)[2] == held
    finally:
        gm.set_tdt_total_shared(False)
    assert bits(on) == bits(off) and all(r["ok"] == 1 for r in on)
    for h in range(len(ids)):
        assert bits(gm.tdt_total_decode(encs[clip_of[h]][None], [ids[h]])) == bits(on[h:h + 1]), f"hypothesis {h} alone"


def test_rescored_nbest_and_pcm_scores_are_identical_on_and_off(tmp_path):
    cfg = dataclasses.replace(pk.make_tiny_config(), name="tiny-hybrid-tree")
    wp, vp = str(tmp_path / "m.safetensors"), str(tmp_path / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    try:
        clips = [synth.synth_pcm(1, n, seed=90 + i)[0] for i, n in enumerate((32000, 20000))]
        off = gm.transcribe_nbest_rescored(clips, 8, 16, 4, tdt_weight=0.5)
        ids = [h["token_ids"] for c in off for h in c]
        clip_of = [c for c, l in enumerate(off) for _ in l]
        s_off = gm.score_tdt(clips, ids=ids, clip_of=clip_of)
        gm.set_tdt_total_shared(True)
        on = gm.transcribe_nbest_rescored(clips, 8, 16, 4, tdt_weight=0.5)
        s_on = gm.score_tdt(clips, ids=ids, clip_of=clip_of)
        assert sum(len(c) for c in off) >= 6 and bits(s_on) == bits(s_off)
        for c in range(2):
            assert [(h["token_ids"], h["text"]) for h in on[c]] == [(h["token_ids"], h["text"]) for h in off[c]]
            for key in ("score", "ctc_score", "tdt_total"):
                assert [np.float32(h[key]).view(np.uint32) for h in on[c]] == [np.float32(h[key]).view(np.uint32) for h in off[c]], (c, key)
    finally:
        gm.close()


def test_a_gemm_bf16_model_is_refused(tmp_path):
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-tree")
    wp = str(tmp_path / "b.safetensors")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=12))
    m = capi.Model(wp, cfg, device=0)
    try:
        held = capi.mem_info(m)[2]
        with pytest.raises(capi.PkError) as e:
            m.set_tdt_total_shared(True)
        assert e.value.code == -7 and not m.tdt_total_shared() and capi.mem_info(m)[2] == held
    finally:
        m.close()
