#!/usr/bin/env python3
"""TDT beam search with n-gram LM shallow fusion next to the unfused search (pk_tdt_beam_decode_lm_timed next to pk_tdt_beam_decode_timed:
HIP events on the model's stream, each call the median of --reps passes after a warm-up; the two are interleaved --rounds times in one
process and the median of the rounds is reported).  The shapes of tools/bench_tdt_beam.py: decoder shapes of tdt-ctc-110m (64 x 10 s) and
tdt-600m (32 x 30 s) with synthetic weights, a one-layer encoder and random encoder rows, at W = 8, K = 8, Kd = 2.  The models of
tools/bench_ctc_beam_lm.py: synthetic 3-gram models over the token ids at two sizes, "small" fits in the L2 cache, "large" has about three
million n-grams.  The cost of the model is the fused stage minus the unfused stage of the same run, in ms and per step (each stage over the
steps its own host loop enqueued, pk_tdt_beam_last_steps: the model changes which hypotheses live, so the two need not take equal steps).  One JSON line per (shapes, model), then the table of profiles/tdt_beam_lm.md.
usage: python tools/bench_tdt_beam_lm.py [--width 8] [--labels 8] [--durations 2] [--reps 3] [--rounds 5] [--alpha 0.5] [--beta 0.0]"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import numpy as np

from bench_ctc_beam_lm import synthetic_arpa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--labels", type=int, default=8)
    ap.add_argument("--durations", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--large", type=int, nargs=2, default=[500000, 2500000], help="bigrams and trigrams of the large model")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    rng = np.random.default_rng(1)
    frames = lambda sec: capi.lib().pk_encoder_num_frames(capi.lib().pk_mel_num_frames(int(sec * 16000)))
    lms = {}                                                         # by vocabulary size: the two configurations may share their models

    def models(V):
        if V not in lms:
            lms[V] = {}
            for name, (n2, n3) in (("small", (20000, 40000)), ("large", tuple(a.large))):
                t0 = time.time()
                text = synthetic_arpa(V, n2, n3, seed=7)
                t1 = time.time()
                lms[V][name] = capi.Lm.from_text(text)
                print(json.dumps({"lm": name, "vocab": V, "order": lms[V][name].order, "ngrams": lms[V][name].num_ngrams, "arpa_bytes": len(text),
                                  "write_s": round(t1 - t0, 2), "load_s": round(time.time() - t1, 2)}), flush=True)
                del text
        return lms[V]

    table = ["| decoder shapes | batch | model | n-grams | unfused stage ms (min .. max) | steps | fused stage ms (min .. max) | steps | fused - unfused ms | "
             "unfused us / step | fused us / step | fused - unfused us / step |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for preset, make, clips, sec in (("tdt-ctc-110m", pk.make_110m_config, 64, 10.0), ("tdt-600m", pk.make_tdt_600m_config, 32, 30.0)):
        cfg = dataclasses.replace(make(), num_layers=1, name=preset + "-1L-tbeam-lm")
        T = frames(sec)
        x = rng.standard_normal((clips, T, cfg.hidden_size)).astype(np.float32)
        enc = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
        with tempfile.TemporaryDirectory() as td:
            wp = os.path.join(td, "w.safetensors")
            synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
            gm = capi.Model(wp, cfg, device=0)
            for lm_name, lm in models(cfg.vocab_size).items():
                plain, fused = [], []
                for _ in range(a.rounds):                            # interleaved: both see the same clocks and the same neighbours
                    plain.append(gm.tdt_beam_decode_timed(enc, a.width, a.labels, a.durations, 1, reps=a.reps)[1])
                    sp = gm.tdt_beam_last_steps()
                    fused.append(gm.tdt_beam_decode_timed(enc, a.width, a.labels, a.durations, 1, reps=a.reps, lm=lm, lm_alpha=a.alpha, lm_beta=a.beta)[1])
                    sf = gm.tdt_beam_last_steps()                    # (the model changes which hypotheses live: the two searches need not take equal steps)
                p, f = float(np.median(plain)), float(np.median(fused))
                out = {"metric": "tdt beam search stage ms", "config": preset, "batch": "%d x %g s" % (clips, sec), "frames": int(T), "beam_width": a.width,
                       "label_prune": a.labels, "duration_prune": a.durations, "lm": lm_name, "ngrams": lm.num_ngrams, "reps": a.reps, "rounds": a.rounds,
                       "unfused_ms": round(p, 3), "fused_ms": round(f, 3), "unfused_spread_ms": [round(min(plain), 3), round(max(plain), 3)],
                       "fused_spread_ms": [round(min(fused), 3), round(max(fused), 3)], "unfused_steps": sp, "fused_steps": sf,
                       "unfused_us_per_step": round(1e3 * p / sp, 3), "fused_us_per_step": round(1e3 * f / sf, 3), "lm_us_per_step": round(1e3 * (f / sf - p / sp), 3)}
                print(json.dumps(out), flush=True)
                table.append("| %s | %s | %s | %d | %.3f (%.3f .. %.3f) | %d | %.3f (%.3f .. %.3f) | %d | %+.3f | %.2f | %.2f | %+.2f |" % (
                    preset, out["batch"], lm_name, lm.num_ngrams, p, min(plain), max(plain), sp, f, min(fused), max(fused), sf, f - p, 1e3 * p / sp,
                    1e3 * f / sf, 1e3 * (f / sf - p / sp)))
            gm.close()
    print("\n".join(table), flush=True)


if __name__ == "__main__":
    main()
