"""Seeded table joints for the TDT beam search kernels (kernels/tdt_beam.hip), and the step-by-step driver of their written specification.

A case is a joint WITHOUT a model: the raw logits row [V + D] of a hypothesis is a function of (seed + clip, t, len(prefix), last token)
alone, so the device test can hand the very rows to pk_diag_tdt_beam_step and tests/tdt_beam_ref.py can walk them through joint(t, prefix).
The rows become log-probs through the specification of the canonical row log-softmax, oracle.log_softmax_rows, label head and duration head
alike (what tests/tdt_decide_ref.py takes for both heads).  Rows that depend on so little make different hypotheses meet equal rows: exact
score ties in the pool and duplicate states are the rule here, not the exception.

The label families, each for one thing tdt_beam_expand_kernel can get wrong (a lane owns the ids congruent to it mod 64, keeps the best of
them that comes after the last pick, and rescans after it won a round):
    ties       3 to 4 integer levels: exact ties inside one lane's stride and across lanes, the top level rare enough to run out;
    one-lane   a few levels on the ids l, l + 64, l + 128, ... of one lane, everything else far below: K picks in a row from one lane;
    rising     within a lane's stride the value grows with the id: the scan must not stop at its first element;
    holes      all but a few labels -inf: fewer than K finite labels on some rows, the -inf picks ordered by id;
    peaky      plain normal rows;
    long       (the long-prefix case) the label is decided by len(prefix) alone and the zero duration is preferred: the beam holds the
               same token string at two frames, step after step, until max_tokens.
The blank's logit is drawn per row: above every label, below every label, tied with a picked label of lower id, of higher id.
The duration rows are 0.75 x an integer level in 0..2: ties among them."""
import functools

import numpy as np

import tdt_beam_lm_ref as RL
import tdt_beam_ref as R

F = np.float32
NEG = F(-np.inf)
BLANK_MODES = ("best", "worst", "tie-low", "tie-high")


def _lsm(x):
    import oracle
    return oracle.log_softmax_rows(np.ascontiguousarray(x, np.float32)[None])[0]


class Case:
    def __init__(self, name, family, V, durations, blank, W, K, Kd, N, Ts, max_tokens, seed):
        self.name, self.family, self.V, self.durations, self.blank = name, family, V, list(durations), blank
        self.D, self.W, self.K, self.Kd, self.N, self.Ts, self.max_tokens, self.seed = len(durations), W, K, Kd, N, list(Ts), max_tokens, seed
        self.B = len(self.Ts)
        self.cap = max(self.Ts) + max_tokens                        # the search's step cap of its longest clip
        assert 1 <= K <= V - 1 and 1 <= Kd <= self.D <= 8 and 0 <= blank < V and 1 <= N <= W
        self._rows, self._lp = {}, {}
        self.modes = {}                                             # blank placement -> rows drawn with it

    def scalars(self):
        return dict(B=self.B, W=self.W, K=self.K, Kd=self.Kd, N=self.N, V=self.V, D=self.D, blank=self.blank, max_tokens=self.max_tokens,
                    durations=self.durations)

    # ---- the rows -------------------------------------------------------------------------------------------------------------------
    def _labels(self, rng, n):
        V, fam = self.V, self.family
        if fam == "ties":
            q = min(0.1, 6.0 / V)
            return rng.choice(4, size=V, p=[0.55, 0.3, 0.15 - q, q]).astype(F)
        if fam == "one-lane":
            x = (-20.0 - rng.integers(0, 3, V)).astype(F)
            ids = np.arange(int(rng.integers(min(64, V))), V, 64)
            x[ids] = (4 + rng.integers(0, 3, len(ids))).astype(F)
            return x
        if fam == "rising":
            i = np.arange(V)
            return (rng.integers(0, 2, 64).astype(F)[i % 64] + F(0.125) * (i // 64).astype(F)).astype(F)      # (exact in fp32)
        if fam == "holes":
            x = np.full(V, NEG, F)
            ids = rng.choice(V, size=min(int(rng.integers(0, self.K + 3)), V), replace=False)
            x[ids] = rng.integers(0, 3, len(ids)).astype(F)
            return x
        if fam == "peaky":
            return (3.0 * rng.standard_normal(V)).astype(F)
        assert fam == "long", fam
        x = np.full(V, F(-8.0), F)
        x[n % (V - 1)] = 0.0
        return x

    def row(self, b, t, n, last):
        """the raw logits [V + D] of clip b's hypothesis at frame t with n tokens, the last one `last` (-1: none)"""
        key = (b, t, n, last)
        if key in self._rows:
            return self._rows[key]
        rng = np.random.default_rng([self.seed + b, t, n, last + 1])
        V, blank, K = self.V, self.blank, self.K
        x = self._labels(rng, n)
        if self.family == "long":
            x[blank] = -12.0
            dl = np.asarray([0.25, 0.0], F)
        else:
            mode = BLANK_MODES[int(rng.integers(4))]
            others = np.delete(np.arange(V), blank)
            fin = x[others][np.isfinite(x[others])]
            if mode in ("tie-low", "tie-high"):                     # the logit of a picked label on the wanted side; none there: the other side
                picks = [int(i) for i in others[np.lexsort((others, -x[others]))[:K]]]
                side = [[i for i in picks if i < blank], [i for i in picks if i > blank]]
                side = side if mode == "tie-low" else side[::-1]
                mode = mode if side[0] else ("tie-high" if mode == "tie-low" else "tie-low")
                x[blank] = x[(side[0] or side[1])[0]]
            elif mode == "best":
                x[blank] = (fin.max() if len(fin) else F(0.0)) + F(1.0)
            else:
                x[blank] = (fin.min() if len(fin) else F(0.0)) - F(1.0)
            if not np.isfinite(x).any():                            # (a row needs one finite logit)
                mode, x[blank] = "best", F(0.0)
            self.modes[mode] = self.modes.get(mode, 0) + 1
            dl = (0.75 * rng.integers(0, 3, self.D)).astype(F)
        out = np.concatenate([x, dl]).astype(F)
        out.setflags(write=False)
        self._rows[key] = out
        return out

    def logprobs(self, b, t, prefix):
        key = (b, t, len(prefix), prefix[-1] if prefix else -1)
        if key not in self._lp:
            x = self.row(*key)
            self._lp[key] = (_lsm(x[: self.V]), _lsm(x[self.V:]))
        return self._lp[key]

    def joint(self, b):
        return lambda t, prefix: self.logprobs(b, t, prefix)


# name: (family, V, durations, blank, W, K, Kd, N, frames per clip, max_tokens, seed)
D5, D8, D1, DU = [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7], [1], [2, 0, 8, 1, 4]
_TABLE = {
    "ties-v2-d1": ("ties", 2, D1, 0, 3, 1, 1, 3, [6], 6, 11),                                     # one label, one duration
    "ties-v64-w1": ("ties", 64, D5, 63, 1, 4, 5, 1, [1, 2, 6], 5, 12),                            # W = 1: R = 3, same-slot duplicates only
    "ties-v65": ("ties", 65, D5, 0, 3, 16, 5, 2, [1, 2, 6], 6, 13),                               # R = 9: a partial 4-row workgroup
    "rising-v128-d8": ("rising", 128, D8, 77, 5, 4, 8, 5, [6], 6, 14),                            # R = 5
    "ties-v129-unsorted-durations": ("ties", 129, DU, 128, 16, 16, 1, 16, [8], 6, 105),           # R = 16
    "peaky-v129": ("peaky", 129, D5, 64, 3, 4, 5, 3, [2, 6, 1], 6, 16),
    "one-lane-v129": ("one-lane", 129, D5, 128, 3, 4, 5, 2, [6, 1, 2], 6, 28),
    "holes-v65": ("holes", 65, D5, 64, 3, 4, 5, 3, [6, 2, 1], 6, 17),
    "one-lane-v1025": ("one-lane", 1025, D5, 1024, 16, 16, 5, 16, [6, 1, 2], 6, 18),              # R = 48
    "ties-v1025": ("ties", 1025, D5, 500, 3, 4, 5, 3, [2, 6, 1], 6, 19),
    "rising-v1025-d1": ("rising", 1025, D1, 0, 16, 16, 1, 4, [6], 6, 20),
    "holes-v1025": ("holes", 1025, DU, 1024, 3, 16, 5, 3, [6, 1, 2], 6, 21),
    "full-pool-v1025": ("ties", 1025, D8, 1024, 16, 16, 8, 16, [8], 6, 209),                     # W = K = 16, Kd = D = 8: P = 2192 keys
    "peaky-v8193": ("peaky", 8193, D5, 8192, 16, 16, 5, 16, [6, 2], 6, 23),                       # R = 32
    "one-lane-v8193": ("one-lane", 8193, D5, 4100, 16, 16, 5, 16, [6], 6, 24),                    # R = 16
    "ties-v8193": ("ties", 8193, D8, 0, 3, 4, 8, 3, [1, 6, 2], 6, 25),
    "rising-v8193": ("rising", 8193, D5, 8192, 5, 16, 1, 5, [8, 3, 1], 4, 109),
    "long-prefix": ("long", 5, [0, 1], 4, 2, 2, 2, 2, [2], 300, 27),                              # token strings past 256 tokens
}
CASES = {name: Case(name, *v) for name, v in _TABLE.items()}
# the fused search: (case, language model, alpha, beta)
LMS = {
    "order3_sparse_unk": dict(order=3, density=0.5, unk=True, bos=False, pool=64),
    "order2_dense_bos": dict(order=2, density=3.0, unk=False, bos=True, pool=64),
}
FUSED = [("ties-v129-unsorted-durations", "order3_sparse_unk", 0.5, 0.75), ("one-lane-v129", "order2_dense_bos", 1.5, -0.5),
         ("full-pool-v1025", "order2_dense_bos", 0.5, 0.75), ("one-lane-v1025", "order3_sparse_unk", 1.5, -0.5),
         ("holes-v1025", "order3_sparse_unk", 0.0, -0.5)]      # (alpha = 0: labels tied in the acoustic score stay tied in f)
assert all(CASES[c].blank == CASES[c].V - 1 for c, _, _, _ in FUSED)


def arpa_of(V, lm_name):
    """ARPA text over the ids 0 .. V - 2 (tests/ngram_lm_ref.py make_arpa): a case fused with it takes V - 1 as its blank"""
    import ngram_lm_ref as NR
    return NR.make_arpa(V, seed=V + len(lm_name), **LMS[lm_name])


def lm_state_of(ref, hist):
    """The automaton state (csrc/ngram_lm.hpp) of a history: 0 for the empty context, else 1 + the file-order index, among the n-grams of
    order < n, of the longest suffix of at most n - 1 symbols that is such an n-gram."""
    if not hasattr(ref, "_state_index"):
        ref._state_index = {g: 1 + i for i, g in enumerate(g for g in ref.table if len(g) < ref.order)}
    for k in range(min(len(hist), ref.order - 1), 0, -1):
        s = ref._state_index.get(tuple(hist[-k:]))
        if s is not None:
            return s
    return 0


def walk(case, b, lm=None, alpha=0.0, beta=0.0):
    """The specification's search of clip b, step by step -> [dict(before, after, info)] (one per step: the beams around it, what
    tdt_beam_ref.step reports beside them) and the dict of search().  lm (an ngram_lm_ref.RefLm): the fused search's beams, six fields wide."""
    T, joint = case.Ts[b], case.joint(b)
    a = (T, case.blank, case.durations, case.W, case.K, case.Kd, case.max_tokens)
    if lm is None:
        beam = [((), 0, F(0.0), ())]
        one = lambda bm, info: R.step(bm, joint, *a, info=info)
        out = R.search(joint, T, case.blank, case.durations, case.W, case.K, case.Kd, case.N, case.max_tokens)
    else:
        beam = [((), 0, F(0.0), (), lm.start(True), F(0.0))]
        one = lambda bm, info: RL.step(bm, joint, lm, F(alpha), F(beta), *a, info=info)
        out = RL.search(joint, T, case.blank, case.durations, lm, alpha, beta, case.W, case.K, case.Kd, case.N, case.max_tokens)
    steps = []
    while any(h[1] < T for h in beam) and len(steps) < T + case.max_tokens:
        info = {}
        new = one(beam, info)
        steps.append(dict(before=beam, after=new, info=info))
        beam = new
    assert len(steps) == out["steps"]
    return steps, out


@functools.lru_cache(maxsize=None)
def ref_lm(V, lm_name):
    import ngram_lm_ref as NR
    return NR.RefLm(arpa_of(V, lm_name))


@functools.lru_cache(maxsize=None)
def walk_of(name, b, lm_name=None, alpha=0.0, beta=0.0):
    """walk() of a case of CASES, computed once per process and shared by every test that needs it (nobody changes it)"""
    case = CASES[name]
    return walk(case, b, ref_lm(case.V, lm_name) if lm_name else None, alpha, beta)
