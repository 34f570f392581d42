"""GPU: the RNN-T lattice walks alone (kernels/rnnt_lattice.hip: rnnt_walk_kernel in both folds, rnnt_trace_kernel) on host lattices against their
written specification, tests/rnnt_lattice_ref.py, BIT FOR BIT: every output word of pk_rnnt_align and pk_rnnt_total."""
import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi

import rnnt_lattice_ref as R

pytestmark = pytest.mark.gpu

# The kernel as built: thread u owns column u, one wave up to U + 1 = 64 columns, then up to 16 waves with one LDS word per wave boundary; one dword of
# back-pointer bits per 32 frames of a column; lattice values requested 16 diagonals ahead.
#   (1,0) the empty string  (1,1) (1,3) one frame  (2,1)  (33,5) a second bits dword of one frame  (5,63) the widest one-wave form  (7,64) the
#   narrowest many-wave form  (3,65) two columns past the boundary  (40,130) boundaries inside the string, T > 32  (64,1023) the limit, 16 waves
SHAPES = [(1, 0), (1, 1), (1, 3), (2, 1), (33, 5), (5, 63), (7, 64), (3, 65), (40, 130), (64, 1023)]


def lattice(T, U, seed=0):
    """gaussian log-softmax-like rows over a stand-in vocabulary of 6: column 0 the label, column 5 the blank"""
    x = np.random.default_rng(1000 * T + U + seed).normal(size=(T, U + 1, 6)) * 2.0
    l = (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)
    return np.ascontiguousarray(l[:, :U, 0]), np.ascontiguousarray(l[:, :, 5])


@pytest.fixture(scope="module")
def cases():
    lats = [lattice(T, U) for T, U in SHAPES]
    hole = lattice(9, 4, seed=5)
    hole[1][8, 4] = -np.inf                                          # the END arc itself: nothing reaches the end, ok = 0
    lats.append(hole)
    for T, U in ((12, 70), (6, 3)):                                  # -inf INSIDE the lattice: cells whose two candidates are both -inf, in both kernel forms
        lab, blk = lattice(T, U, seed=9)
        rng = np.random.default_rng(T)
        lab[rng.random(lab.shape) < 0.15] = -np.inf
        blk[rng.random(blk.shape) < 0.15] = -np.inf
        blk[T - 1, U] = -1.0
        lats.append((lab, blk))
    return lats, [(R.align(*x), R.total(*x)) for x in lats]


def same(got, want, what):
    assert got["ok"] == want["ok"], f"{what}: ok"
    for k in want:
        if k != "ok":
            G.assert_bits_equal(np.asarray(got[k]), np.asarray(want[k]), f"{what}: {k}")


@pytest.mark.parametrize("i", range(len(SHAPES) + 3), ids=[f"T{T}-U{U}" for T, U in SHAPES] + ["unreachable-end", "holes-T12-U70", "holes-T6-U3"])
def test_walks_equal_the_specification(cases, i):
    lats, want = cases
    same(capi.rnnt_align([lats[i]])[0], want[i][0], "alignment")
    same(capi.rnnt_total([lats[i]])[0], want[i][1], "total")
    if i < len(SHAPES):
        assert want[i][0]["ok"] == 1 and want[i][1]["total"] >= want[i][0]["score"]
    elif i == len(SHAPES):
        assert want[i][0]["ok"] == 0 and want[i][1]["ok"] == 0 and want[i][1]["total"] == -np.inf


def test_one_ragged_batch_of_all_of_them(cases):
    """Every workgroup is as wide as the longest string needs: the short strings run with idle waves beside them."""
    lats, want = cases
    for b, (ga, gt) in enumerate(zip(capi.rnnt_align(lats), capi.rnnt_total(lats))):
        same(ga, want[b][0], f"utterance {b}: alignment")
        same(gt, want[b][1], f"utterance {b}: total")


def test_more_than_1023_tokens_are_refused():
    lat = (np.zeros((1, 1024), np.float32), np.zeros((1, 1025), np.float32))
    for fn in (capi.rnnt_align, capi.rnnt_total):
        with pytest.raises(capi.PkError) as e:
            fn([lat])
        assert e.value.code == -7 and "1023" in str(e.value)       # PK_ERR_UNSUPPORTED
