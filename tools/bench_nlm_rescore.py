#!/usr/bin/env python3
"""Neural LM rescoring of n-best lists (kernels/neural_lm.hip, the causal attention form): stage times on 64 clips x 8
hypotheses x about 40 tokens through a Transformer LM of d 512, 8 layers, 8 heads, ffn 2048 at Vlm 1026 and Vlm 8194 (synthetic weights, random
token strings of 35 .. 45 tokens, end term on):
  the embedding, blocks and head stages of pk_nlm_score_timed (HIP events on the handle's stream, summed over the call's groups),
  the head kernel's share of the fp32 MFMA peak: 2 rows Vlm d flop over its stage time,
  next to them the CTC head and beam stages of pk_ctc_beam_decode_timed (W = 8, N = 8) on 64 x 10 s at tdt-ctc-110m shapes, the search that makes
  such lists.
There is no parent to compare with: a record, not a gate.  Writes profiles/nlm_rescore.md with --write.
usage: python tools/bench_nlm_rescore.py [--reps 3] [--write]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np

FP32_MFMA_PEAK_TFLOPS = 157.3        # MI355X, fp32 matrix (the vendor's data sheet figure)

NOTES = """
## Reading the figures

- `embed_ms`, `blocks_ms`, `head_ms`: `pk_nlm_score_timed`, HIP-event medians on the handle's stream.  `embed_ms` includes `emb_norm_` where the model
  has one, `blocks_ms` the final LayerNorm.  The host side (packing the tables, the copy of `lp` back, the sums) is not in them; `call_ms` is the wall
  time of one whole `pk_nlm_score`.
- `head_gflop` = 2 rows Vlm d; `head_peak_share` = that over `head_ms` over the fp32 MFMA peak of %.1f Tflop/s.
- `ctc_head_stage_ms` / `beam_stage_ms`: `pk_ctc_beam_decode_timed` on 64 x 10 s at tdt-ctc-110m shapes with synthetic weights, W = 8, N = 8: the
  search that produces lists of this size.  The strings the LM scores here are random, not that search's output: synthetic acoustic weights give
  hypotheses of arbitrary length, and the workload is fixed at about 40 tokens.
- `gpu_to_fp32_numpy_ratio`: `tests/test_gpu_nlm.py` prints, per model variant, the GPU's largest distance to the float64 reference over the
  fp32 NumPy evaluation's (the test requires at most 4).  Recorded on one MI355X with the test's models (d 64, 2 layers, Vlm 67): pre-LN / tied head
  0.56 with the end term and 1.0 without, post-LN / `emb_norm_` / untied head with bias 0.66 and 0.64 (distances of 2 .. 4e-5 on both sides).
""" % FP32_MFMA_PEAK_TFLOPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import time
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    lines = []
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as td:
        cfg = pk.make_110m_config()
        wp = os.path.join(td, "m.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        enc = gm.encode(gm.mel(synth.synth_pcm(64, 160000, seed=3)))
        head, beam = gm.ctc_beam_decode_timed(enc, 8, 16, 8, reps=a.reps)
        gm.close()
        for V in (1026, 8194):
            c = capi.nlm_config(vocab_size=V, max_positions=128, hidden_size=512, num_layers=8, num_heads=8, ffn_intermediate=2048, pre_ln=True,
                                has_final_norm=True, tied_head=True, bos_id=V - 2, eos_id=V - 1)
            lp = os.path.join(td, f"lm{V}.safetensors")
            synth.save_weights(lp, synth.synth_nlm_weights(c, seed=7))
            lm = capi.NeuralLm(lp, c)
            S = [rng.integers(0, V - 2, int(n)).astype(np.int32) for n in rng.integers(35, 46, 64 * 8)]
            rows = sum(len(s) + 1 for s in S)
            lm.score(S)                                              # warm-up of the buffers
            t0 = time.perf_counter()
            lm.score(S)
            call = (time.perf_counter() - t0) * 1e3
            e, b, h = lm.score_timed(S, reps=a.reps)
            gflop = 2.0 * rows * V * 512 / 1e9
            out = {"metric": "neural LM rescoring stage ms", "lm": "d 512, 8 layers, 8 heads, ffn 2048", "vlm": V, "strings": len(S), "rows": rows,
                   "groups": lm.last_groups(), "reps": a.reps, "embed_ms": round(e, 3), "blocks_ms": round(b, 3), "head_ms": round(h, 3),
                   "call_ms": round(call, 3), "head_gflop": round(gflop, 1), "head_peak_share": round(gflop / h / FP32_MFMA_PEAK_TFLOPS, 4),
                   "ctc_head_stage_ms": round(head, 3), "beam_stage_ms": round(beam, 3)}
            lm.close()
            lines.append(out)
            print(json.dumps(out), flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "nlm_rescore.md"), "w") as f:
            f.write("# Neural LM rescoring of n-best lists: stage times on one MI355X\n\n`python tools/bench_nlm_rescore.py --reps %d --write` (synthetic "
                    "weights and token strings; HIP-event medians).\n\n" % a.reps)
            keys = ["vlm", "strings", "rows", "groups", "embed_ms", "blocks_ms", "head_ms", "call_ms", "head_gflop", "head_peak_share", "ctc_head_stage_ms",
                    "beam_stage_ms"]
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for o in lines:
                f.write("| " + " | ".join(str(o.get(k, "-")) for k in keys) + " |\n")
            f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n" + NOTES)


if __name__ == "__main__":
    main()
