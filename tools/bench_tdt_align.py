#!/usr/bin/env python3
"""TDT forced alignment of given token strings (kernels/tdt_align.hip): the three stage times of pk_tdt_align_decode_timed (HIP events on the
model's stream, medians of --reps passes after a warm-up) -- prediction net over every prefix, lattice (enc_proj + activation + heads product
+ reduction, in row chunks), walk + back-trace -- on synthetic weights, on the encoder's output for synthetic audio:
  64 x 10 s at tdt-ctc-110m shapes, 32 x 30 s at tdt-600m shapes (one encoder layer: the encoder is not part of the measurement), one 5-minute
  clip at tdt-ctc-110m shapes; every clip is aligned with its own greedy TDT transcript (cut to one token per frame and the kernel's 1535 tokens).
Next to them, on the same batch in the same run: the greedy TDT decode (wall ms of pk_tdt_decode: upload, enc_proj, loop, download), for 110m
the CTC alignment stage (pk_ctc_align_decode_timed on the clip's greedy CTC output), and the heads product of one chunk alone (the fourth
timer of pk_tdt_align_decode_timed: the same launch the lattice stage makes per chunk, between its own events; pk_diag_gemm runs that product
too but has no device timer) with its flop rate and, scaled by cells / chunk_rows, what the bare products of the whole lattice would take.
Writes profiles/tdt_align.md with --write.
usage: python tools/bench_tdt_align.py [--reps 3] [--write]"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np

NOTES = """
## Reading the figures

- The three stages are HIP-event medians on the model's stream (`pk_tdt_align_decode_timed`): prediction net (uploads + `U_max + 1` lock-step
  steps), lattice (enc_proj + activation + heads product + reduction over all row chunks), walk + back-trace.
- `lattice_heads_tflops` counts only the heads product's `2 cells (V + D) J` flops against the WHOLE lattice stage.  `heads_one_chunk_ms` is the
  same launch the stage makes per chunk (`chunk_rows x (V + D) x J`), timed alone between its own events; `heads_alone_tflops` is its rate and
  `heads_alone_all_chunks_ms` scales it by `cells / chunk_rows`.  `lattice_stage_ms - heads_alone_all_chunks_ms` is what enc_proj, the activation
  kernel and the reduction kernel cost on top of the bare products.
- `greedy_tdt_decode_wall_ms` is a wall time of `pk_tdt_decode` (upload, enc_proj, loop, download), not a stage timer; it is there for scale.
- `ctc_align_stage_ms` is `pk_ctc_align_decode_timed`'s alignment stage on the same rows with the clip's greedy CTC output (110m only).
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    rng = np.random.default_rng(1)
    lines = []
    with tempfile.TemporaryDirectory() as td:
        models = {}

        def model(name):
            if name not in models:
                cfg = pk.make_110m_config() if name == "tdt-ctc-110m" else dataclasses.replace(pk.make_tdt_600m_config(), num_layers=1)
                wp = os.path.join(td, name + ".safetensors")
                synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
                models[name] = (cfg, capi.Model(wp, cfg, device=0))
            return models[name]
        for preset, label, n, sec in (("tdt-ctc-110m", "64 x 10 s", 64, 10.0), ("tdt-600m", "32 x 30 s", 32, 30.0), ("tdt-ctc-110m", "1 x 5 min", 1, 300.0)):
            cfg, gm = model(preset)
            pcm = synth.synth_pcm(n, int(sec * 16000), seed=3)
            enc = gm.encode(gm.mel(pcm))                                              # the encoder's own output on synthetic audio, as bench.py decodes it
            T = int(enc.shape[1])
            greedy = True
            try:
                g = gm.tdt_decode(enc)
                ids = [g["ids"][b, :min(int(g["lens"][b]), 1535, T)] for b in range(n)]     # (at most one token per frame and the kernel's 1535)
            except capi.PkError:                                                      # synthetic weights can run greedy into its safety cap: one random token per three frames
                greedy = False
                ids = [rng.integers(0, cfg.blank_id, size=min(T // 3, 1535)).astype(np.int32) for _ in range(n)]
            walls = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                try:
                    gm.tdt_decode(enc)
                except capi.PkError:
                    pass
                walls.append((time.perf_counter() - t0) * 1e3)
            r = gm.tdt_align_decode(enc, ids)                                         # warm-up of the buffers
            pred, lat, walk, heads = gm.tdt_align_decode_timed(enc, ids, reps=a.reps)
            V, D, J = cfg.vocab_size, len(cfg.durations), cfg.joint_hidden
            cells = int(sum(T * (len(i) + 1) for i in ids))
            flops = 2.0 * cells * (V + D) * J
            M = min(cells, max(128, min(65536, (256 << 20) // ((V + D) * 4) // 128 * 128)))
            out = {"metric": "tdt forced alignment ms", "config": preset, "batch": label, "frames": int(T), "tokens_per_clip": int(np.mean([len(i) for i in ids])),
                   "transcripts": "greedy" if greedy else "random, one token per 3 frames", "ok": int(sum(q["ok"] for q in r)), "reps": a.reps, "lattice_cells": cells, "pred_net_stage_ms": round(pred, 3), "lattice_stage_ms": round(lat, 3),
                   "walk_stage_ms": round(walk, 3), "lattice_heads_tflops": round(flops / (lat * 1e-3) / 1e12, 2), "chunk_rows": int(M),
                   "heads_one_chunk_ms": round(heads, 3), "heads_alone_tflops": round(2.0 * M * (V + D) * J / (heads * 1e-3) / 1e12, 2),
                   "heads_alone_all_chunks_ms": round(heads * cells / M, 3),
                   "greedy_tdt_decode_wall_ms": round(float(np.median(walls[1:])), 3)}
            if cfg.ctc_vocab_size > 0:
                c = gm.ctc_decode(enc)
                cids = [c["ids"][b, :c["lens"][b]] for b in range(n)]
                head, stage = gm.ctc_align_decode_timed(enc, cids, total=False, reps=a.reps)
                out["ctc_head_stage_ms"] = round(head, 3); out["ctc_align_stage_ms"] = round(stage, 3)
                out["ctc_tokens_per_clip"] = int(np.mean([len(i) for i in cids]))
            lines.append(out)
            print(json.dumps(out), flush=True)
        for _, gm in models.values():
            gm.close()
    if a.write:
        with open(os.path.join(ROOT, "profiles", "tdt_align.md"), "w") as f:
            f.write("# TDT forced alignment: stage times on one MI355X\n\n`python tools/bench_tdt_align.py --reps %d --write` (synthetic weights and audio, every clip aligned "
                    "with its own greedy TDT transcript; HIP-event medians unless a column says wall).\n\n" % a.reps)
            keys = ["config", "batch", "frames", "tokens_per_clip", "transcripts", "lattice_cells", "pred_net_stage_ms", "lattice_stage_ms", "walk_stage_ms", "lattice_heads_tflops",
                    "chunk_rows", "heads_one_chunk_ms", "heads_alone_tflops", "heads_alone_all_chunks_ms", "greedy_tdt_decode_wall_ms", "ctc_head_stage_ms", "ctc_align_stage_ms"]
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for o in lines:
                f.write("| " + " | ".join(str(o.get(k, "-")) for k in keys) + " |\n")
            f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n" + NOTES)


if __name__ == "__main__":
    main()
