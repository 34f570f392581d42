"""Back-off n-gram language model over token ids in plain Python: the written specification of DESIGN.md section 5.5.6 that csrc/ngram_lm.cpp
(pk_lm_score) and the fused walk of kernels/ctc_beam.hip are compared against bit for bit.

Deliberately NOT an automaton: a dictionary from n-gram tuples to (log-prob, back-off) and the textbook recursion on the history's last
n - 1 symbols.  Values are natural-log fp32 (text -> float (strtod) -> * 2.302585092994046 in double -> fp32, once); a lookup is
acc = 0, then one fp32 add per back-off level, then acc + p.  make_arpa writes the synthetic models of the tests."""
import numpy as np

F = np.float32
LN10 = 2.302585092994046
BOS, EOS, UNK = "<s>", "</s>", "<unk>"


def _word(w):
    return w if w in (BOS, EOS, UNK) else int(w)


def parse(text):
    """ARPA text -> (order, {tuple of words: (lp fp32, back-off fp32)}).  Lenient: the refusals are the loader's business."""
    table, order, k = {}, 0, 0
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        if line.startswith("\\"):
            if line.endswith("-grams:"):
                k = int(line[1:-7])
                order = max(order, k)
            continue
        if k == 0:
            continue                                                # the header and the "ngram k=count" lines
        f = line.split()
        words = tuple(_word(w) for w in f[1:1 + k])
        bo = F(float(f[1 + k]) * LN10) if len(f) > 1 + k else F(0.0)
        table[words] = (F(float(f[0]) * LN10), bo)
    return order, table


class RefLm:
    def __init__(self, text):
        self.text = text
        self.order, self.table = parse(text)
        self.has_bos = (BOS,) in self.table
        self._memo = {}

    def start(self, bos=True):
        return (BOS,) if (bos and self.has_bos) else ()

    def lookup(self, hist, c):
        """log p(c | hist) -> (fp32 value, sum of |terms| in float64: what bounds every intermediate of the lookup, number of back-off weights
        added).  hist: every symbol so far (with <s> in front when the string starts there)."""
        n = self.order
        ctx = tuple(hist[-(n - 1):]) if n > 1 else ()
        key = (ctx, c)
        got = self._memo.get(key)
        if got is not None:
            return got
        acc, mag, levels = F(0.0), 0.0, 0
        while True:
            e = self.table.get(ctx + (c,))
            if e is not None:
                break
            if not ctx:
                e = self.table.get((UNK,))
                if e is None:
                    raise KeyError(f"{c!r} has no unigram and the model has no <unk>")
                break
            b = self.table.get(ctx)
            if b is not None:
                acc = F(acc + b[1])
                mag += abs(float(b[1]))
                levels += 1
            ctx = ctx[1:]
        out = (F(acc + e[0]), mag + abs(float(e[0])), levels)
        self._memo[key] = out
        return out

    def lookup64(self, hist, c):
        """the same value in float64 arithmetic on the fp32 table"""
        n = self.order
        ctx = tuple(hist[-(n - 1):]) if n > 1 else ()
        acc = 0.0
        while True:
            e = self.table.get(ctx + (c,))
            if e is not None:
                return acc + float(e[0])
            if not ctx:
                return acc + float(self.table[(UNK,)][0])
            b = self.table.get(ctx)
            if b is not None:
                acc += float(b[1])
            ctx = ctx[1:]

    def score(self, ids, bos=True, eos=False):
        """the fp32 left-to-right sum pk_lm_score returns"""
        hist = self.start(bos)
        s = F(0.0)
        for c in list(ids) + ([EOS] if eos else []):
            s = F(s + self.lookup(hist, c)[0])
            hist = hist + (c,)
        return s

    def score64(self, ids, bos=True):
        hist = self.start(bos)
        s = 0.0
        for c in ids:
            s += self.lookup64(hist, c)
            hist = hist + (c,)
        return s


def make_arpa(V, order, density, unk, bos, seed, pool=12):
    """Synthetic ARPA text over the ids 0 .. V - 2 (V - 1 is the acoustic model's blank and is never named).
    density: n-grams of order k per n-gram of order k - 1 (0.5: sparse, long back-off chains; 3: dense).  unk: <unk> is an entry and only
    about two thirds of the ids have a unigram, else every id has one.  bos: <s> and </s> are entries, some n-grams start with <s> and some
    end in </s>.  Higher orders draw their words from the `pool` lowest ids, so that short histories do meet them."""
    rng = np.random.default_rng(seed)
    ids = list(range(V - 1))
    uni = [i for i in ids if rng.random() < 0.67 or i < 2] if unk else ids
    grams = [[(w,) for w in uni]]
    if unk:
        grams[0].append((UNK,))
    if bos:
        grams[0] += [(BOS,), (EOS,)]
    have_uni = set(uni)
    small = [i for i in ids[:pool] if unk or i in have_uni]
    for k in range(2, order + 1):
        prev = [g for g in grams[-1] if g[-1] not in (EOS, UNK)]
        want = max(2, int(density * len(grams[-1])))
        seen = set()
        for _ in range(20 * want):
            if len(seen) >= want or not prev:
                break
            g = prev[int(rng.integers(len(prev)))]
            w = small[int(rng.integers(len(small)))]
            if bos and rng.random() < 0.1:
                w = EOS
            seen.add(g + (w,))
        grams.append(sorted(seen, key=lambda g: tuple(str(x) for x in g)))
    lines = ["", "\\data\\"] + [f"ngram {k + 1}={len(g)}" for k, g in enumerate(grams)]
    for k, gs in enumerate(grams):
        lines += ["", f"\\{k + 1}-grams:"]
        for g in gs:
            p = -99.0 if g == (BOS,) else -float(rng.uniform(0.1, 4.0))
            txt = f"{p:.6f}\t" + " ".join(str(x) for x in g)
            if k + 1 < order and g[-1] != EOS and rng.random() < 0.85:   # (some lines have no back-off column: 0)
                txt += f"\t{float(rng.uniform(-1.5, 0.3)):.6f}"
            lines.append(txt)
    lines += ["", "\\end\\", ""]
    return "\n".join(lines)
