"""The CTC greedy kernels alone (kernels/decode.hip through pk_diag_ctc_greedy): the row log-softmax + first-max argmax (wave_logsoftmax_argmax: its two bodies
switch at n = 8 | 9, a second trip of the lane loop starts at n = 65), launched with and without the log-prob rows, then ctc_collapse_kernel or, with a trie,
ctc_boosted_kernel -- uniform and ragged batches, an output pitch larger than the longest utterance.

Reference: the oracle (oracle.log_softmax_rows, ctc_greedy, ctc_greedy_boosted), every utterance on its own.  Log-probs, best_lp and conf bit for bit, integers
equal; the pattern-filled rows behind the batch, the entries behind an utterance's tokens and the columns past n untouched.  Cases: tdt_decide_ref.CTC_CASES
(tests/test_tdt_decide_ref.py holds the plain restatement of the same cases to the oracle on the CPU)."""
import numpy as np
import pytest

import tdt_decide_ref as R

pytestmark = pytest.mark.gpu
FILL = np.uint32(R.FILL32)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("c", R.CTC_CASES, ids=[c["name"] for c in R.CTC_CASES])
def test_ctc_kernels_against_the_oracle(c, orc):
    from parakeet_cpp_amd import capi
    o = R.make_ctc_case(c)
    n, blank, nf = o["n"], o["blank"], o["n_frames"]
    B, frames = len(nf), int(nf.sum())
    got = capi.diag_ctc_greedy(o["logits"], n, blank, B=B, T=int(nf[0]) if o["uniform"] else 0, n_frames=None if o["uniform"] else nf, pitch=o["pitch"],
                               trie=o["trie"])
    lp = orc.log_softmax_rows(o["logits"][:, :n])
    best = np.argmax(lp, axis=1).astype(np.int32)                    # first maximum of the rounded log-probs
    assert np.array_equal(u32(got["lp"][:frames]), u32(lp))
    for sfx in ("", "2"):
        assert np.array_equal(got["best_idx" + sfx][:frames], best), "best_idx" + sfx
        assert np.array_equal(u32(got["best_lp" + sfx][:frames]), u32(lp[np.arange(frames), best])), "best_lp" + sfx
        assert np.all(u32(got["best_idx" + sfx][frames:]) == FILL) and np.all(u32(got["best_lp" + sfx][frames:]) == FILL)
    assert np.all(u32(got["lp"][frames:]) == FILL)
    otrie = orc.Trie(o["phrases"]) if o["trie"] else None
    r0 = 0
    for b, T in enumerate(nf):
        u = lp[r0: r0 + T][None]
        g = orc.ctc_greedy_boosted(u, blank, otrie, o["boost"]) if otrie else orc.ctc_greedy(u, blank)
        k = int(g["lens"][0])
        assert got["lens"][b] == k, (b, got["lens"][b], k)
        for name in ("ids", "start", "end"):
            assert np.array_equal(got[name][b, :k], g[name][0, :k]), (name, b)
        assert np.array_equal(u32(got["conf"][b, :k]), u32(g["conf"][0, :k])), ("conf", b)
        for name in ("ids", "start", "end", "conf"):
            assert np.all(u32(got[name][b, k:]) == FILL), f"{name}[{b}]: stores behind the {k} tokens"
        r0 += T
    for name in ("ids", "start", "end", "conf", "lens"):
        assert np.all(u32(got[name][B:]) == FILL), f"{name}: stores behind the batch"
    if c["kind"] == "all-blank":
        assert not got["lens"][:B].any()
    if c["kind"] in ("one-token", "alternating", "run", "ties"):
        assert got["lens"][:B].all()
