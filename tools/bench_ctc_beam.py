#!/usr/bin/env python3
"""CTC prefix beam search next to the greedy CTC stage (pk_ctc_beam_decode_timed: HIP events on the model's stream, median of --reps passes
after a warm-up).  tdt-ctc-110m shapes with synthetic weights, encoder rows drawn at random (the search's cost depends on the shapes and
on how flat the rows are, not on what they mean; random weights give nearly flat rows: every frame has W (K + 1) live candidates).
Line 1: 64 x 10 s (126 frames each), W in --widths at K = --prune.  Line 2: a ragged mix of 64 clips of 5-15 s.
usage: python tools/bench_ctc_beam.py [--clips 64] [--widths 1 4 8 16 32] [--prune 16] [--reps 5] [--timestamps]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--prune", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timestamps", action="store_true")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config()
    rng = np.random.default_rng(1)

    def rows(t):
        x = rng.standard_normal((t, cfg.hidden_size)).astype(np.float32)
        return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)

    frames = lambda sec: capi.lib().pk_encoder_num_frames(capi.lib().pk_mel_num_frames(int(sec * 16000)))
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        uniform = np.stack([rows(frames(10.0)) for _ in range(a.clips)])
        ragged = [rows(frames(s)) for s in rng.uniform(5.0, 15.0, a.clips)]
        for name, enc, n_rows in (("64 x 10 s", uniform, uniform.shape[0] * uniform.shape[1]), ("5-15 s ragged mix", ragged, sum(len(e) for e in ragged))):
            out = {"metric": "ctc beam search stage ms", "config": "tdt-ctc-110m", "batch": name, "clips": a.clips, "encoder_rows": int(n_rows),
                   "token_prune": a.prune, "timestamps": bool(a.timestamps), "reps": a.reps, "beam_ms": {}}
            for w in a.widths:
                g, b = gm.ctc_beam_decode_timed(enc, w, a.prune, 1, a.timestamps, a.reps)
                out["beam_ms"][str(w)] = round(b, 3)
                out["greedy_ctc_stage_ms"] = round(g, 3)
            print(json.dumps(out), flush=True)
        gm.close()


if __name__ == "__main__":
    main()
