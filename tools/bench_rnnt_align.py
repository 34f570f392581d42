#!/usr/bin/env python3
"""RNN-T forced alignment of given token strings (kernels/rnnt_lattice.hip): the four stage times of pk_rnnt_align_decode_timed (HIP events on the
model's stream, medians of --reps passes after a warm-up) -- prediction net over every prefix, lattice (activation + heads product + reduction,
in row chunks), walk, back-trace -- at rnnt-600m shapes with synthetic weights (one encoder layer: the encoder is not part of the measurement),
on the encoder's output for synthetic audio:
  64 x 10 s with 40-token transcripts, one 4-minute clip with 960 tokens (random ids: the stages' cost does not depend on the values).
Next to them, on the same clips and the same token strings: the walk + back-trace stage of pk_tdt_align_decode_timed at tdt-600m shapes (durations
0 .. 4), a lattice of the same T and U walked by tdt_align_kernel.
Writes profiles/rnnt_align.md's table with --write (the file's hand-written sections stay).
usage: python tools/bench_rnnt_align.py [--reps 5] [--write]"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np

MARK = "<!-- bench_rnnt_align.py -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    rng = np.random.default_rng(1)
    lines = []
    with tempfile.TemporaryDirectory() as td:
        def model(name, make):
            cfg = dataclasses.replace(make(), num_layers=1)
            wp = os.path.join(td, name + ".safetensors")
            synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
            return cfg, capi.Model(wp, cfg, device=0)
        rcfg, rm = model("rnnt-600m", pk.make_rnnt_600m_config)
        tcfg, tm = model("tdt-600m", pk.make_tdt_600m_config)
        top = min(rcfg.blank_id, tcfg.blank_id)
        for label, n, sec, U in (("64 x 10 s", 64, 10.0, 40), ("1 x 4 min", 1, 240.0, 960)):
            pcm = synth.synth_pcm(n, int(sec * 16000), seed=3)
            ids = [rng.integers(0, top, size=U).astype(np.int32) for _ in range(n)]
            enc = rm.encode(rm.mel(pcm))
            T = int(enc.shape[1])
            r = rm.rnnt_align_decode(enc, ids)                                        # warm-up of the buffers
            pred, lat, walk, trace = rm.rnnt_align_decode_timed(enc, ids, reps=a.reps)
            tenc = tm.encode(tm.mel(pcm))
            assert tenc.shape[1] == T
            tr = tm.tdt_align_decode(tenc, ids)
            _, _, twalk, _ = tm.tdt_align_decode_timed(tenc, ids, reps=a.reps)
            out = {"metric": "rnnt forced alignment ms", "batch": label, "frames": T, "tokens_per_clip": U, "lattice_cells": n * T * (U + 1), "ok": int(sum(q["ok"] for q in r)),
                   "reps": a.reps, "pred_net_stage_ms": round(pred, 3), "lattice_stage_ms": round(lat, 3), "walk_ms": round(walk, 3), "trace_ms": round(trace, 3),
                   "tdt_walk_and_trace_ms": round(twalk, 3), "tdt_ok": int(sum(q["ok"] for q in tr))}
            lines.append(out)
            print(json.dumps(out), flush=True)
        rm.close(); tm.close()
    if a.write:
        path = os.path.join(ROOT, "profiles", "rnnt_align.md")
        head = open(path).read().split(MARK)[0]
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
        keys = ["batch", "frames", "tokens_per_clip", "lattice_cells", "pred_net_stage_ms", "lattice_stage_ms", "walk_ms", "trace_ms", "tdt_walk_and_trace_ms"]
        with open(path, "w") as f:
            f.write(head + MARK + "\n\n## Stage times at rnnt-600m shapes\n\n`python tools/bench_rnnt_align.py --reps %d --write` on the tree that follows commit `%s`, one "
                    "MI355X; synthetic weights and audio, random token strings, HIP-event medians.\n\n" % (a.reps, commit))
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for o in lines:
                f.write("| " + " | ".join(str(o[k]) for k in keys) + " |\n")
            f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n")


if __name__ == "__main__":
    main()
