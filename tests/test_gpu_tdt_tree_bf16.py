"""GPU: the bf16 prefix-tree TDT lattice kernel (kernels/tdt_tree_bf16.hip).  Alone: every value of the tree lattice against
the float64 reference of tests/tdt_lattice_bf16_ref.py under its derived bound and, BIT FOR BIT, against the chain kernel (kernels/tdt_lattice_bf16.hip)
on every root-to-end chain.  Through a gemm_bf16 model: the totals with pk_model_set_tdt_total_shared on against off, bit for bit, and the switches."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

import tdt_lattice_bf16_ref as R

pytestmark = pytest.mark.gpu


def tree_set(V):
    """-> (strings, clip_of, frames): 782 tree-lattice rows, tile edges inside clips.  Clip 0: four strings on one prefix whose last node has children on
    tokens 0 and 3 (one 64-column block, the first), 70 (a block of another wave) and V - 2 (the last label block); clip 1: a node with 40 children on
    consecutive tokens (several per lane in one block); a plain chain; the empty string alone (no lab); T = 1; a chain of 70 on 3 frames."""
    p, run = [5, 7], [0, V - 2, 5, 5] * 18
    ids = [p + [0, 6], p + [3], p + [70], p + [V - 2, V - 2]] + [[9, 10 + i] for i in range(40)] + [run[:12], [], [1, 2], run[:70]]
    return ids, [0] * 4 + [1] * 40 + [2, 3, 4, 5], np.asarray([40, 2, 9, 5, 1, 3], np.int32)


# the chain kernel's shapes: the row tables take the same 124 bytes per row, so the J thresholds are its own and these run every RS instantiation
# (128-row tiles twice, 96 at J = 640, 64 at J = 1024)
@pytest.mark.parametrize("J,V,D", [(64, 78, 4), (128, 1025, 5), (640, 8193, 5), (1024, 300, 5)])
def test_kernel_equals_the_chain_kernel_and_the_reference_on_every_chain(J, V, D):
    rng = np.random.default_rng(J + V)
    ids, clip_of, T = tree_set(V)
    blank, B = V - 1, len(ids)
    no, par, tok, end = capi.tdt_prefix_tree(ids, clip_of, len(T))
    ep = rng.standard_normal((int(T.sum()), J)).astype(np.float32)
    pp = rng.standard_normal((int(no[-1]), J)).astype(np.float32)      # one row per node
    wld = (rng.standard_normal((V + D, J)) / np.sqrt(J)).astype(np.float32)
    wld[2] *= 8                                                      # for some rows the maximum logit arrives in the first column block ...
    wld[V - 1] *= 8                                                  # ... for others in the last one that holds labels (a partial one)
    bld = (0.1 * rng.standard_normal(V + D)).astype(np.float32)
    got = capi.tdt_tree_lattice_bf16(ep, pp, wld, bld, no, par, tok, T, V, D, blank)

    # the same (frame, prefix) pairs as chains, one utterance per string: its clip's frames, the pp rows of the nodes on its path
    n, row0 = np.diff(no), np.concatenate([[0], np.cumsum(T)])
    cell0, lab0 = np.concatenate([[0], np.cumsum(T * n)]), np.concatenate([[0], np.cumsum(T * (n - 1))])
    ppc = np.zeros(((max(len(i) for i in ids) + 1) * B, J), np.float32)
    il, ib = [], []                                                  # tree word of every chain word, in the chain kernel's packing
    for h, c in enumerate(clip_of):
        path = [int(end[h])]
        while par[no[c] + path[-1]] >= 0:
            path.append(int(par[no[c] + path[-1]]))
        k = np.asarray(path[::-1])
        ppc[np.arange(len(k)) * B + h] = pp[no[c] + k]
        t = np.arange(T[c])[:, None]
        ib.append((cell0[c] + t * n[c] + k[None, :]).ravel())
        il.append((lab0[c] + t * (n[c] - 1) + k[None, 1:] - 1).ravel())
    il, ib = np.concatenate(il), np.concatenate(ib)
    epc = np.concatenate([ep[row0[c]:row0[c + 1]] for c in clip_of])
    idl = [np.asarray(i, np.int32) for i in ids]
    chain = capi.tdt_lattice_bf16(epc, ppc, wld, bld, idl, T[clip_of], V, D, blank)
    want = R.reference(epc, ppc, wld, bld, idl, T[clip_of], V, D, blank)
    assert max(b.max() for b in want[3:]) <= 1e-3, "a condition on the test: the bound must stay sharp enough to see a dropped column block"
    Gd = capi.TDT_LATTICE_GUARD
    idx = (il, ib, (ib[:, None] * D + np.arange(D)).ravel())
    for name, g, i, ck, w, bound in zip(("lab", "blk", "dl"), got, idx, chain, want[:3], want[3:]):
        assert np.all(g[-Gd:].view(np.uint32) == 0x7FC5A5A5), f"{name}: a guard word was written"
        body = g[:-Gd]
        assert np.array_equal(np.unique(i), np.arange(body.size)), "a condition on the test: every tree word lies on a chain"
        assert not np.isnan(body).any(), f"{name}: {int(np.isnan(body).sum())} words were left as the NaN fill"
        same = body[i].view(np.uint32) == ck[:-Gd].view(np.uint32)
        assert same.all(), f"{name}: {int((~same).sum())} of {same.size} values differ from the chain kernel's"
        err = np.abs(body[i].astype(np.float64) - w)
        print(f"{name}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, max bound {bound.max():.3e}")
        assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} of {err.size} values outside the bound, worst {(err / bound).max():.2f} x"


def bits(res):
    return [(np.float32(r["total"]).view(np.uint32), r["ok"]) for r in res]


def test_model_route_shared_equals_unshared_and_follows_the_lattice_switch(tmp_path_factory):
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name="tiny-bf16-ttree")
    _, _, gm = G.make_pair(tmp_path_factory.mktemp("ttree16"), cfg, seed=12)
    rng = np.random.default_rng(8)
    encs = [rng.standard_normal((T, cfg.hidden_size)).astype(np.float32) for T in (40, 9, 33)]
    clips = [synth.synth_pcm(1, m, seed=70 + i)[0] for i, m in enumerate((32000, 12345, 20000))]
    a, b = (rng.integers(0, cfg.blank_id, size=12).astype(np.int32) for _ in range(2))
    # 1 / 4 / 3 strings: shared prefixes, a duplicate, a string that is a prefix of another
    ids = [a[:5], a, a[:7], np.concatenate([a[:7], b[:3]]), a, b[:5], b[:4], np.concatenate([b[:4], a[:1]])]
    clip_of, pids = [0, 1, 1, 1, 1, 2, 2, 2], [i.tolist() for i in ids]

    def refused():
        held = capi.mem_info(gm)[2]
        with pytest.raises(capi.PkError) as e:
            gm.set_tdt_total_shared(True)
        assert e.value.code == -7 and not gm.tdt_total_shared() and capi.mem_info(gm)[2] == held
    refused()                                                        # the lattice switch is off
    gm.set_tdt_lattice_bf16(True)
    try:
        off, s_off = gm.tdt_total_decode(encs, ids, clip_of), gm.score_tdt(clips, ids=pids, clip_of=clip_of)
        gm.set_tdt_total_shared(True)
        assert gm.tdt_total_shared()
        on, s_on = gm.tdt_total_decode(encs, ids, clip_of), gm.score_tdt(clips, ids=pids, clip_of=clip_of)
        assert bits(on) == bits(off) and all(r["ok"] == 1 for r in on)
        assert bits(s_on) == bits(s_off) and all(r["ok"] == 1 for r in s_on)
        gm.set_tdt_lattice_bf16(False)                               # takes the shared switch with it
        assert not gm.tdt_total_shared()
        refused()
    finally:
        gm.set_tdt_lattice_bf16(False)
