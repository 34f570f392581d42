#!/usr/bin/env python3
"""CTC n-best rescored by the TDT head (kernels/tdt_total.hip): stage times on 64 x 10 s at tdt-ctc-110m shapes (synthetic
weights and audio, the encoder's own output), beam width W = 8, N in {1, 4, 8} hypotheses per clip:
  the beam stage of pk_ctc_beam_decode_timed (CTC head stage next to it),
  the prediction-net, lattice and forward stages of pk_tdt_total_decode_timed on the beam's hypotheses (hypotheses of a clip share its frames),
  and the share of lattice columns (clip, prefix ids[:u]) that occur in more than one hypothesis of the clip: what a prefix-shared lattice would
  not compute twice.
Next to them, on the same batch in the same run, pk_tdt_align_decode_timed of the best hypothesis of every clip (one string per clip: the parent
feature's figures for scale).  Writes profiles/tdt_rescore.md with --write.
--shared: instead, the three stages of pk_tdt_total_decode_timed with pk_model_set_tdt_total_shared off and on (kernels/tdt_tree.hip, DESIGN.md
section 5.5.3a), interleaved off / on / off / on ... in this one process on the same hypotheses, the totals compared bit for bit, and the share of
lattice columns the prefix trees save.  Writes profiles/tdt_rescore_shared.md with --write (its bench.py section is kept).
--shared --bf16: the same off / on comparison on gemm_bf16 models with pk_model_set_tdt_lattice_bf16 on (kernels/tdt_tree_bf16.hip, DESIGN.md section
5.5.3b) at the tdt-ctc-110m and tdt-600m head shapes (1-layer encoders; tdt-600m has no CTC head, so the n-best lists are synthetic: see
bf16_lists), with the lattice rows of both layouts.  Writes profiles/tdt_rescore_shared_bf16.md with --write.
usage: python tools/bench_tdt_rescore.py [--reps 3] [--write] [--shared [--rounds 3] [--bf16]]"""
import argparse
import dataclasses
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


def shared_rounds(gm, capi, enc, ids, clip_of, n_clips, reps, rounds):
    """-> dict: per-stage medians over the rounds of (off, on) run alternately, every round's pair, and the columns the trees save."""
    off = gm.tdt_total_decode(enc, ids, clip_of)
    gm.set_tdt_total_shared(True)
    on = gm.tdt_total_decode(enc, ids, clip_of)
    same = all(np.float32(x["total"]).view(np.uint32) == np.float32(y["total"]).view(np.uint32) and x["ok"] == y["ok"] for x, y in zip(off, on))
    pairs = []
    for _ in range(rounds):
        gm.set_tdt_total_shared(False)
        t_off = gm.tdt_total_decode_timed(enc, ids, clip_of, reps=reps)
        gm.set_tdt_total_shared(True)
        t_on = gm.tdt_total_decode_timed(enc, ids, clip_of, reps=reps)
        pairs.append([[round(float(v), 3) for v in t_off], [round(float(v), 3) for v in t_on]])
    gm.set_tdt_total_shared(False)
    cols = sum(len(i) + 1 for i in ids)
    nodes = int(capi.tdt_prefix_tree(ids, clip_of, n_clips)[0][-1])
    med = lambda k, s: round(float(np.median([p[k][s] for p in pairs])), 3)
    out = {"bit_identical": bool(same), "lattice_columns": cols, "tree_columns": nodes, "saved_column_share": round(1.0 - nodes / max(cols, 1), 4), "rounds": pairs}
    for s, name in enumerate(("pred_net", "lattice", "forward")):
        out[name + "_ms_off"], out[name + "_ms_on"] = med(0, s), med(1, s)
    out["total_ms_off"] = round(sum(out[k + "_ms_off"] for k in ("pred_net", "lattice", "forward")), 3)
    out["total_ms_on"] = round(sum(out[k + "_ms_on"] for k in ("pred_net", "lattice", "forward")), 3)
    return out


def bf16_lists(rng, n, T, N, blank):
    """-> (ids, clip_of): N strings per clip of T // 4 tokens; string j keeps all but the last 3 j tokens of the clip's first string and ends in 3 j
    tokens of its own -- the shape of a beam's n-best list, whose entries differ near the end."""
    ids, clip_of = [], []
    for c in range(n):
        base = rng.integers(0, blank, size=min(T // 4, 1535)).astype(np.int32)
        for j in range(N):
            ids.append(np.concatenate([base[:len(base) - 3 * j], rng.integers(0, blank, size=3 * j).astype(np.int32)]))
            clip_of.append(c)
    return ids, clip_of


def bench_shared_bf16(a, pk, capi, synth):
    rng = np.random.default_rng(1)
    lines = []
    with tempfile.TemporaryDirectory() as td:
        for preset, label, n, sec in (("tdt-ctc-110m", "64 x 10 s", 64, 10.0), ("tdt-600m", "32 x 30 s", 32, 30.0)):
            cfg = dataclasses.replace(pk.make_110m_config() if preset == "tdt-ctc-110m" else pk.make_tdt_600m_config(), num_layers=1, gemm_bf16=True)
            wp = os.path.join(td, preset + ".safetensors")
            synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
            gm = capi.Model(wp, cfg, device=0)
            gm.set_tdt_lattice_bf16(True)
            enc = gm.encode(gm.mel(synth.synth_pcm(n, int(sec * 16000), seed=3)))
            T = int(enc.shape[1])
            for N in (1, 4, 8):
                ids, clip_of = bf16_lists(rng, n, T, N, cfg.blank_id)
                out = {"metric": "tdt rescoring on the bf16 lattice kernels, prefix tree off / on, ms", "config": preset + " (1 layer, gemm_bf16)", "batch": label,
                       "frames": T, "n_best": N, "hypotheses": len(ids), "tokens_per_hypothesis": round(float(np.mean([len(i) for i in ids])), 1),
                       "reps": a.reps}
                out.update(shared_rounds(gm, capi, enc, ids, clip_of, n, a.reps, a.rounds))
                out["lattice_rows_off"], out["lattice_rows_on"] = T * out["lattice_columns"], T * out["tree_columns"]
                out["row_ratio"] = round(out["lattice_rows_on"] / out["lattice_rows_off"], 3)
                out["lattice_ms_ratio"] = round(out["lattice_ms_on"] / out["lattice_ms_off"], 3)
                lines.append(out)
                print(json.dumps(out), flush=True)
            gm.close()
    if a.write:
        keys = ["config", "n_best", "hypotheses", "tokens_per_hypothesis", "lattice_rows_off", "lattice_rows_on", "row_ratio", "lattice_ms_off", "lattice_ms_on",
                "lattice_ms_ratio", "pred_net_ms_off", "pred_net_ms_on", "forward_ms_off", "forward_ms_on", "total_ms_off", "total_ms_on", "bit_identical"]
        with open(os.path.join(ROOT, "profiles", "tdt_rescore_shared_bf16.md"), "w") as f:
            f.write("# TDT rescoring on one prefix tree per clip, gemm_bf16 models on the bf16 lattice kernels: the switch off and on, one MI355X\n\n"
                    "`python tools/bench_tdt_rescore.py --shared --bf16 --reps %d --rounds %d --write` (1-layer encoders, synthetic weights and audio; synthetic "
                    "n-best lists: string j of a clip shares all but its last 3 j tokens with the first).  Every figure is the median over the rounds of "
                    "`pk_tdt_total_decode_timed`'s HIP-event medians; off (kernels/tdt_lattice_bf16.hip, one lattice per hypothesis) and on "
                    "(kernels/tdt_tree_bf16.hip, one per clip) alternate inside one process on the same hypotheses.  `lattice_rows_*` = frames x lattice "
                    "columns of the layout; at n_best = 1 the tree is a chain and `lattice_ms_ratio` is the cost of the cursor walk.\n\n" % (a.reps, a.rounds))
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for o in lines:
                f.write("| " + " | ".join(str(o.get(k, "-")) for k in keys) + " |\n")
            f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n")


SHARED_MARK = "## bench.py headline"


def write_shared(lines, reps, rounds):
    path = os.path.join(ROOT, "profiles", "tdt_rescore_shared.md")
    keep = ""
    if os.path.exists(path):
        txt = open(path).read()
        keep = txt[txt.index(SHARED_MARK):] if SHARED_MARK in txt else ""
    keys = ["n_best", "hypotheses", "tokens_per_hypothesis", "lattice_columns", "tree_columns", "saved_column_share", "pred_net_ms_off", "pred_net_ms_on",
            "lattice_ms_off", "lattice_ms_on", "forward_ms_off", "forward_ms_on", "total_ms_off", "total_ms_on", "bit_identical"]
    with open(path, "w") as f:
        f.write("# TDT rescoring on one prefix tree per clip: the switch off and on, one MI355X\n\n`python tools/bench_tdt_rescore.py --shared --reps %d "
                "--rounds %d --write` (tdt-ctc-110m shapes, 64 x 10 s, W = 8, synthetic weights and audio).  Every figure is the median over the rounds of "
                "`pk_tdt_total_decode_timed`'s HIP-event medians; off and on alternate inside one process on the same hypotheses.\n\n" % (reps, rounds))
        f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
        for o in lines:
            f.write("| " + " | ".join(str(o.get(k, "-")) for k in keys) + " |\n")
        f.write("\n```\n" + "\n".join(json.dumps(o) for o in lines) + "\n```\n\n" + keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--shared", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bf16", action="store_true", help="with --shared: gemm_bf16 models on the bf16 lattice kernels (profiles/tdt_rescore_shared_bf16.md)")
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    if a.shared and a.bf16:
        return bench_shared_bf16(a, pk, capi, synth)
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
            if a.shared:
                out = {"metric": "tdt rescoring, prefix tree off / on, ms", "config": "tdt-ctc-110m", "batch": "64 x 10 s", "frames": T, "beam_width": W,
                       "n_best": N, "hypotheses": len(ids), "tokens_per_hypothesis": round(float(np.mean([len(i) for i in ids])), 1), "reps": a.reps}
                out.update(shared_rounds(gm, capi, enc, ids, clip_of, n, a.reps, a.rounds))
                lines.append(out)
                print(json.dumps(out), flush=True)
                continue
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
    if a.write and a.shared:
        write_shared(lines, a.reps, a.rounds)
    elif a.write:
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
