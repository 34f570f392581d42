#!/usr/bin/env python3
"""CTC n-best rescored by the TDT head (kernels/tdt_total.hip): stage times on 64 x 10 s at tdt-ctc-110m shapes (synthetic
weights and audio, the encoder's own output), beam width W = 8, N in {1, 4, 8} hypotheses per clip:
  the beam stage of pk_ctc_beam_decode_timed (CTC head stage next to it),
  the prediction-net, lattice and forward stages of pk_tdt_total_decode_timed on the beam's hypotheses (hypotheses of a clip share its frames),
  and the share of lattice columns (clip, prefix ids[:u]) that occur in more than one hypothesis of the clip: what a prefix-shared lattice would
  not compute twice.
Next to them, on the same batch in the same run, pk_tdt_align_decode_timed of the best hypothesis of every clip (one string per clip: the parent
feature's figures for scale).  Writes profiles/tdt_rescore.md with --write.
usage: python tools/bench_tdt_rescore.py [--reps 3] [--write]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np

NOTES = """
## Reading the figures

- Every stage is a HIP-event median on the model's stream.  `beam_stage_ms` / `ctc_head_stage_ms`: `pk_ctc_beam_decode_timed`.  `pred_net_stage_ms`,
  `lattice_stage_ms`, `forward_stage_ms`: `pk_tdt_total_decode_timed` on all hypotheses of the batch, summed over its groups (`groups`).
- `lattice_columns` counts (clip, hypothesis, u) for u = 0 .. U; `shared_column_share` is the fraction of them whose prefix `ids[:u]` occurs in
  more than one hypothesis of the same clip, counting every occurrence after the first: the columns a prefix-shared lattice would save.
- `align_*_ms`: `pk_tdt_align_decode_timed` on the first hypothesis of every clip alone (one string per clip).
- The arithmetic estimate of the lattice is `2 T (U + 1) (V + D) J` flop per hypothesis (`lattice_gflop` sums it).
"""


def shared_share(hyps_of_clip):
    cols = shared = 0
    for hyps in hyps_of_clip:
        seen = set()
        for ids in hyps:
            for u in range(len(ids) + 1):
                key = tuple(int(v) for v in ids[:u])
                cols += 1
                shared += key in seen
                seen.add(key)
    return cols, shared / max(cols, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    lines = []
    with tempfile.TemporaryDirectory() as td:
        cfg = pk.make_110m_config()
        wp = os.path.join(td, "m.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        n, W = 64, 8
        enc = gm.encode(gm.mel(synth.synth_pcm(n, 160000, seed=3)))
        T = int(enc.shape[1])
        V, D, J = cfg.vocab_size, len(cfg.durations), cfg.joint_hidden
        for N in (1, 4, 8):
            b = gm.ctc_beam_decode(enc, W, 16, N)
            head, beam = gm.ctc_beam_decode_timed(enc, W, 16, N, reps=a.reps)
            hyps_of_clip = [[b["ids"][c, j, :min(int(b["lens"][c, j]), 1535)] for j in range(N) if b["score"][c, j] > -np.inf] for c in range(n)]
            ids = [h for hy in hyps_of_clip for h in hy]
            clip_of = [c for c, hy in enumerate(hyps_of_clip) for _ in hy]
            r = gm.tdt_total_decode(enc, ids, clip_of)                                # warm-up of the buffers
            pred, lat, fwd = gm.tdt_total_decode_timed(enc, ids, clip_of, reps=a.reps)
            groups = capi.tdt_total_groups([T] * len(ids), [len(i) for i in ids], list(cfg.durations), V, J)[1]
            cols, share = shared_share(hyps_of_clip)
            first = [hy[0] for hy in hyps_of_clip]
            ap_, al_, aw_, _ = gm.tdt_align_decode_timed(enc, first, reps=a.reps)
            out = {"metric": "tdt rescoring of ctc n-best ms", "config": "tdt-ctc-110m", "batch": "64 x 10 s", "frames": T, "beam_width": W, "n_best": N,
                   "hypotheses": len(ids), "tokens_per_hypothesis": round(float(np.mean([len(i) for i in ids])), 1), "scored": int(sum(q["ok"] for q in r)),
                   "groups": int(groups), "reps": a.reps, "ctc_head_stage_ms": round(head, 3), "beam_stage_ms": round(beam, 3),
                   "pred_net_stage_ms": round(pred, 3), "lattice_stage_ms": round(lat, 3), "forward_stage_ms": round(fwd, 3),
                   "lattice_gflop": round(sum(2.0 * T * (len(i) + 1) * (V + D) * J for i in ids) / 1e9, 1),
                   "lattice_columns": cols, "shared_column_share": round(share, 4),
                   "align_pred_net_ms": round(ap_, 3), "align_lattice_ms": round(al_, 3), "align_walk_ms": round(aw_, 3)}
            lines.append(out)
            print(json.dumps(out), flush=True)
        gm.close()
    if a.write:
        with open(os.path.join(ROOT, "profiles", "tdt_rescore.md"), "w") as f:
            f.write("# CTC n-best rescored by the TDT head: stage times on one MI355X\n\n`python tools/bench_tdt_rescore.py --reps %d --write` (synthetic weights "
                    "and audio; HIP-event medians).\n\n" % a.reps)
            keys = ["n_best", "hypotheses", "tokens_per_hypothesis", "groups", "ctc_head_stage_ms", "beam_stage_ms", "pred_net_stage_ms", "lattice_stage_ms",
                    "forward_stage_ms", "lattice_gflop", "lattice_columns", "shared_column_share", "align_pred_net_ms", "align_lattice_ms", "align_walk_ms"]
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for o in lines:
                f.write("| " + " | ".join(str(o.get(k, "-")) for k in keys) + " |\n")
            f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n" + NOTES)


if __name__ == "__main__":
    main()
