#!/usr/bin/env python3
"""CTC prefix beam search with n-gram LM shallow fusion next to the unfused search (pk_ctc_beam_decode_lm_timed next to
pk_ctc_beam_decode_timed: HIP events on the model's stream, each call the median of --reps passes after a warm-up; the two are interleaved
--rounds times in one process and the median of the rounds is reported).  The shapes of tools/bench_ctc_beam.py: tdt-ctc-110m with synthetic
weights, 64 x 10 s and a ragged mix of 64 clips of 5-15 s, at W = 8, K = 16.  Synthetic 3-gram models over the 1024 token ids at two sizes:
"small" fits in the L2 cache, "large" has a few million n-grams.  One JSON line per (batch, model).
usage: python tools/bench_ctc_beam_lm.py [--clips 64] [--width 8] [--prune 16] [--reps 5] [--rounds 5] [--alpha 0.5] [--beta 0.0]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np


def synthetic_arpa(V, n2, n3, seed):
    """ARPA text of a 3-gram model over the ids 0 .. V - 2 with <unk> and <s>: every id has a unigram, n2 distinct random bigrams, n3 distinct
    random trigrams whose first two words are one of the bigrams.  Values are random: the search's cost does not depend on them."""
    rng = np.random.default_rng(seed)
    n = V - 1
    def distinct(x, k):                                              # k of the distinct values of x, chosen at random, sorted
        x = np.unique(x)
        rng.shuffle(x)
        return np.sort(x[:k])

    bi = distinct(rng.integers(0, n * n, size=int(n2 * 2)), n2)
    tri = distinct(rng.integers(0, len(bi), size=int(n3 * 1.2)).astype(np.int64) * n + rng.integers(0, n, size=int(n3 * 1.2)), n3)
    lines = ["\\data\\", f"ngram 1={n + 2}", f"ngram 2={len(bi)}", f"ngram 3={len(tri)}", "", "\\1-grams:", "-99\t<s>\t-0.3", "-3.5\t<unk>"]
    p1, b1 = rng.uniform(0.5, 4.0, n), rng.uniform(0.0, 1.0, n)
    lines += [f"-{p1[i]:.4f}\t{i}\t-{b1[i]:.4f}" for i in range(n)]
    p2, b2 = rng.uniform(0.3, 3.0, len(bi)), rng.uniform(0.0, 1.0, len(bi))
    lines += ["", "\\2-grams:"] + [f"-{p2[j]:.4f}\t{x // n} {x % n}\t-{b2[j]:.4f}" for j, x in enumerate(bi.tolist())]
    p3 = rng.uniform(0.1, 2.5, len(tri))
    lines += ["", "\\3-grams:"] + [f"-{p3[j]:.4f}\t{bi[x // n] // n} {bi[x // n] % n} {x % n}" for j, x in enumerate(tri.tolist())]
    lines += ["", "\\end\\", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--prune", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--large", type=int, nargs=2, default=[500000, 2500000], help="bigrams and trigrams of the large model")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config()
    V = cfg.ctc_vocab_size
    rng = np.random.default_rng(1)

    def rows(t):
        x = rng.standard_normal((t, cfg.hidden_size)).astype(np.float32)
        return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)

    frames = lambda sec: capi.lib().pk_encoder_num_frames(capi.lib().pk_mel_num_frames(int(sec * 16000)))
    lms = {}
    for name, (n2, n3) in (("small", (20000, 40000)), ("large", tuple(a.large))):
        t0 = time.time()
        text = synthetic_arpa(V, n2, n3, seed=7)
        t1 = time.time()
        lms[name] = capi.Lm.from_text(text)
        print(json.dumps({"lm": name, "order": lms[name].order, "ngrams": lms[name].num_ngrams, "arpa_bytes": len(text),
                          "write_s": round(t1 - t0, 2), "load_s": round(time.time() - t1, 2)}), flush=True)
        del text
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        uniform = np.stack([rows(frames(10.0)) for _ in range(a.clips)])
        ragged = [rows(frames(s)) for s in rng.uniform(5.0, 15.0, a.clips)]
        for name, enc, n_rows, t_max in (("64 x 10 s", uniform, uniform.shape[0] * uniform.shape[1], uniform.shape[1]),
                                         ("5-15 s ragged mix", ragged, sum(len(e) for e in ragged), max(len(e) for e in ragged))):
            for lm_name, lm in lms.items():
                plain, fused = [], []
                for _ in range(a.rounds):                            # interleaved: both see the same clocks and the same neighbours
                    plain.append(gm.ctc_beam_decode_timed(enc, a.width, a.prune, 1, False, a.reps)[1])
                    fused.append(gm.ctc_beam_decode_timed(enc, a.width, a.prune, 1, False, a.reps, lm=lm, lm_alpha=a.alpha, lm_beta=a.beta)[1])
                p, f = float(np.median(plain)), float(np.median(fused))
                # the walk is one workgroup per utterance and the utterances run side by side: the stage lasts as long as the longest walk
                print(json.dumps({"metric": "ctc beam search stage ms", "config": "tdt-ctc-110m", "batch": name, "clips": a.clips,
                                  "encoder_rows": int(n_rows), "longest_frames": int(t_max), "beam_width": a.width, "token_prune": a.prune,
                                  "lm": lm_name, "ngrams": lm.num_ngrams, "reps": a.reps, "rounds": a.rounds,
                                  "unfused_ms": round(p, 3), "fused_ms": round(f, 3), "unfused_spread_ms": [round(min(plain), 3), round(max(plain), 3)],
                                  "fused_spread_ms": [round(min(fused), 3), round(max(fused), 3)],
                                  "lm_us_per_frame": round(1e3 * (f - p) / t_max, 3),
                                  "lm_ns_per_lookup_slot": round(1e6 * (f - p) / (n_rows * a.width * a.prune), 3)}), flush=True)
        gm.close()


if __name__ == "__main__":
    main()
