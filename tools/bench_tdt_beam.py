#!/usr/bin/env python3
"""TDT beam search next to the greedy TDT stage of the same run (pk_tdt_beam_decode_timed: HIP events on the model's stream, median of --reps
passes after a warm-up).  Decoder shapes of tdt-ctc-110m (64 x 10 s, 126 frames each) and tdt-600m (32 x 30 s, 376 frames each) with synthetic
weights and a one-layer encoder (the search never runs the encoder), encoder rows drawn at random: the cost depends on the shapes and on how
many steps the hypotheses take, not on what the rows mean.  Prints one JSON line per configuration and writes profiles/tdt_beam.md.
usage: python tools/bench_tdt_beam.py [--widths 1 4 8 16] [--labels 8] [--durations 2] [--reps 3] [--out profiles/tdt_beam.md]"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--labels", type=int, default=8)
    ap.add_argument("--durations", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdt_beam.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    rng = np.random.default_rng(1)
    frames = lambda sec: capi.lib().pk_encoder_num_frames(capi.lib().pk_mel_num_frames(int(sec * 16000)))
    lines = ["# TDT beam search stage next to the greedy TDT stage", "",
             "`tools/bench_tdt_beam.py`: `pk_tdt_beam_decode_timed`, HIP events on the model's stream, median of %d passes after a warm-up;" % a.reps,
             "synthetic weights, random encoder rows, K = %d labels and Kd = %d durations per expansion, N = 1." % (a.labels, a.durations), "",
             "| decoder shapes | batch | greedy TDT stage ms | " + " | ".join("W = %d ms" % w for w in a.widths) + " |",
             "|---|---|---|" + "---|" * len(a.widths)]
    for preset, make, clips, sec in (("tdt-ctc-110m", pk.make_110m_config, 64, 10.0), ("tdt-600m", pk.make_tdt_600m_config, 32, 30.0)):
        cfg = dataclasses.replace(make(), num_layers=1, name=preset + "-1L-tbeam")
        T = frames(sec)
        x = rng.standard_normal((clips, T, cfg.hidden_size)).astype(np.float32)
        enc = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
        with tempfile.TemporaryDirectory() as td:
            wp = os.path.join(td, "w.safetensors")
            synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
            gm = capi.Model(wp, cfg, device=0)
            out = {"metric": "tdt beam search stage ms", "config": preset, "batch": "%d x %g s" % (clips, sec), "frames": int(T), "label_prune": a.labels,
                   "duration_prune": a.durations, "reps": a.reps, "beam_ms": {}}
            for w in a.widths:
                g, b = gm.tdt_beam_decode_timed(enc, w, a.labels, a.durations, 1, reps=a.reps)
                out["beam_ms"][str(w)] = round(b, 3)
                out["greedy_tdt_stage_ms"] = round(g, 3)
            gm.close()
        print(json.dumps(out), flush=True)
        lines.append("| %s | %s | %.3f | " % (preset, out["batch"], out["greedy_tdt_stage_ms"]) + " | ".join("%.3f" % out["beam_ms"][str(w)] for w in a.widths) + " |")
    lines += ["", "The search is a host loop of ordinary launches, six and one per LSTM layer each step, over B W rows; the greedy stage is the lock-step decode loop of `pk_tdt_decode`.",
              "The widths are choices for this table, not recommendations."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
