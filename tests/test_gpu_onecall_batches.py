"""GPU: the one-call entry points (audio in, answer out) on a call that the packing policy cuts into TWO batches.

300 clips of 1 to 4 encoder frames in an order that is not the planner's (longest first, stable): 256 + 44, the clip cap closes the first batch.
Every entry point answers the 300-clip call exactly as it answers the clips [0:100), [100:200) and [200:300) given in calls of their own (one batch
each): tokens, texts, frames, words, ok and every score to the bit.  So the scatter of a batch's results back to the caller's clip order is
exercised across a batch boundary, and what a call keeps between batches (the language model's device copy) meets a second batch."""
import numpy as np
import pytest

from conftest import pk
from parakeet_cpp_amd import capi, synth

import ngram_lm_ref as NR

pytestmark = pytest.mark.gpu

LENS = (300, 4000, 1500, 257, 2600)                                  # samples, cycled: 1 to 4 encoder frames
N_CLIPS = 300
SLICES = ((0, 100), (100, 200), (200, 300))
W, N_BEST = 4, 2
ONE = [3]                                                           # the fixed one-token transcript
NAMES = ["nbest", "nbest_lm", "nbest_rescored", "nbest_tdt", "nbest_tdt_lm", "align", "align_tdt", "score_tdt", "score_tdt_first_batch_only", "spot"]


def bits(x):
    """x with every float replaced by its fp32 bit pattern, so that == on the result compares scores to the bit."""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(bits(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return ("f32", int(np.float32(x).view(np.uint32)))
    return x


class Calls:
    """The entry points on the clips [lo, hi) of the input, each with the arguments that belong to those clips."""

    def __init__(self, gm, lm, clips, frames):
        self.gm, self.lm, self.clips = gm, lm, clips
        first = [h[0]["token_ids"] if h else [] for h in gm.transcribe_nbest(clips, W, 16, N_BEST, timestamps=True)]
        # transcripts: the first hypothesis of the search; the fixed token where it is empty or longer than the clip has frames;
        # a repeated token (needs three frames) on every 7th clip, which the one- and two-frame clips among them cannot align: ok = 0
        self.ids = [list(t) if 0 < len(t) <= frames[i] else ONE for i, t in enumerate(first)]
        for i in range(0, len(clips), 7):
            self.ids[i] = ONE * 2
        self.keywords = [self.ids[1], self.ids[4], ONE]
        # hypotheses to score: none for the clips [100:200); elsewhere two, one, none by turns
        self.hyps = []                                              # (clip, ids)
        for i in range(len(clips)):
            if not 100 <= i < 200:
                self.hyps += [(i, self.ids[i]), (i, ONE)][: (2, 1, 0)[i % 3]]
        # ... and hypotheses for the 4000-sample clips only: the whole second batch has nothing to score and is not encoded
        self.hyps_long = [(i, self.ids[i]) for i in range(len(clips)) if LENS[i % len(LENS)] == 4000]

    def extra_clip(self, pcm):
        """One more clip at the end of the input (with a transcript, no hypothesis); undone by drop_clip."""
        self.clips = self.clips + [pcm]
        self.ids = self.ids + [ONE]

    def drop_clip(self):
        self.clips, self.ids = self.clips[:-1], self.ids[:-1]

    def _score(self, hyps, lo, hi):
        sel = [(c - lo, t) for c, t in hyps if lo <= c < hi]
        return self.gm.score_tdt(self.clips[lo:hi], ids=[t for _, t in sel], clip_of=[c for c, _ in sel])

    def __call__(self, name, lo, hi):
        gm, clips, lmkw = self.gm, self.clips[lo:hi], dict(lm=self.lm, lm_alpha=1.5, lm_beta=-0.5)
        if name == "nbest":
            return gm.transcribe_nbest(clips, W, 16, N_BEST, timestamps=True)
        if name == "nbest_lm":
            return gm.transcribe_nbest(clips, W, 16, N_BEST, timestamps=True, **lmkw)
        if name == "nbest_rescored":
            return gm.transcribe_nbest_rescored(clips, W, 16, N_BEST, timestamps=True)
        if name == "nbest_tdt":
            return gm.transcribe_nbest_tdt(clips, W, 4, 2, N_BEST, timestamps=True)
        if name == "nbest_tdt_lm":
            return gm.transcribe_nbest_tdt(clips, W, 4, 2, N_BEST, timestamps=True, **lmkw)
        if name == "align":
            return gm.align(clips, ids=self.ids[lo:hi])
        if name == "align_tdt":
            return gm.align_tdt(clips, ids=self.ids[lo:hi])
        if name == "score_tdt":
            return self._score(self.hyps, lo, hi)
        if name == "score_tdt_first_batch_only":
            return self._score(self.hyps_long, lo, hi)
        assert name == "spot"
        return gm.spot(clips, ids=self.keywords, max_hits=2)

    def n_results(self, name, lo, hi):
        """how many entries of the 300-clip answer belong to the clips [lo, hi), and where they start"""
        if not name.startswith("score_tdt"):
            return lo, hi - lo
        hyps = self.hyps if name == "score_tdt" else self.hyps_long
        return sum(c < lo for c, _ in hyps), sum(lo <= c < hi for c, _ in hyps)


@pytest.fixture(scope="module")
def onecall(tmp_path_factory):
    """The tiny hybrid model WITH a vocabulary (its own handle), a small language model over its ids, the 300 clips and the shared arguments."""
    td = tmp_path_factory.mktemp("onecall_batches")
    cfg = pk.make_tiny_config()
    wp, vp = str(td / "tiny.safetensors"), str(td / "vocab.txt")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    synth.save_vocab(vp, synth.synth_vocab(cfg.vocab_size - 1))
    gm = capi.Model(wp, cfg, vocab_path=vp, device=0)
    lm = capi.Lm.from_text(NR.make_arpa(cfg.vocab_size, order=3, density=0.5, unk=True, bos=False, seed=3))
    lens = [LENS[i % len(LENS)] for i in range(N_CLIPS)]
    clips = [synth.synth_pcm(1, n, seed=700 + i)[0] for i, n in enumerate(lens)]
    batch_of, pos, nb = capi.plan_batches(lens)
    assert nb == 2 and np.bincount(batch_of).tolist() == [256, 44], "the packing policy changed: this file needs a call of two batches, 256 + 44"
    assert np.any(np.diff(batch_of) < 0) and np.any(np.diff(batch_of) > 0), "the caller's order is the planner's: no result crosses back"
    frames = capi.ragged_extents(lens)[1]
    assert frames.min() == 1 and frames.max() == 4
    calls = Calls(gm, lm, clips, frames)
    whole = {}                                                      # name -> the answer of the 300-clip call, computed once
    yield calls, whole
    lm.close()
    gm.close()


def whole_of(onecall, name):
    calls, whole = onecall
    if name not in whole:
        whole[name] = calls(name, 0, N_CLIPS)
    return whole[name]


@pytest.mark.parametrize("name", NAMES)
def test_two_batches_answer_as_their_slices_alone(onecall, name):
    calls, _ = onecall
    got = whole_of(onecall, name)
    for lo, hi in SLICES:
        at, n = calls.n_results(name, lo, hi)
        if n == 0:                                                  # (score_tdt, clips [100:200): nothing to score, and a call of its own is refused)
            assert name == "score_tdt"
            with pytest.raises(capi.PkError) as e:
                calls(name, lo, hi)
            assert e.value.code == -1
            continue
        alone = calls(name, lo, hi)
        assert len(alone) == n
        for i in range(n):
            assert bits(alone[i]) == bits(got[at + i]), f"{name}: entry {at + i} of the 300-clip call vs entry {i} of the clips [{lo}:{hi}) alone"
    assert len(got) == sum(calls.n_results(name, lo, hi)[1] for lo, hi in SLICES)
    # not degenerate: tokens, timestamps, refused alignments and hits are all in the mix
    if name.startswith("nbest"):
        assert any(len(h) == N_BEST for h in got) and any(d["token_ids"] and d["words"] for h in got for d in h)
    elif name.startswith("align"):
        assert any(d["ok"] == 1 and d["words"] for d in got)
        if name == "align":                                         # (the TDT lattice emits several tokens on one frame: every transcript here fits)
            assert any(d["ok"] == 0 and "start" not in d for d in got)
    elif name.startswith("score"):
        assert any(d["ok"] == 1 and np.isfinite(d["total"]) for d in got)
    else:
        assert any(hits for clip in got for hits in clip)


@pytest.mark.parametrize("name", NAMES)
def test_a_short_last_clip_refuses_the_call_and_leaves_the_next_one_as_it_was(onecall, name):
    calls, _ = onecall
    lo, hi = N_CLIPS - 5, N_CLIPS                                   # (one clip of every length; every entry point has something to do on them)
    before = bits(calls(name, lo, hi))
    calls.extra_clip(np.zeros(256, np.float32))
    try:
        with pytest.raises(capi.PkError) as e:
            calls(name, lo, hi + 1)                                 # the same call with the short clip last
        assert e.value.code == -1 and "more than 256 samples" in str(e.value)
    finally:
        calls.drop_clip()
    assert bits(calls(name, lo, hi)) == before
