#!/usr/bin/env python3
"""TDT keyword spotting (kernels/tdt_kws.hip): the three stage timers of pk_tdt_kws_decode_timed (HIP events on the model's
stream, medians of --reps passes after a warm-up, summed over the groups of a call): prediction net, lattice, normalisation + walk + picking.
tdt-ctc-110m shapes (it has both heads) with synthetic weights, encoder rows drawn at random, keywords of 1 .. 8 tokens cut from the clips' own
greedy TDT output (the greedy CTC output where synthetic weights run the TDT loop into its safety cap).  Cases: 64 x 10 s and one 60-minute clip, each with 1 / 16 / 128 keywords.
Next to each, in the same run, the two existing comparables: pk_ctc_kws_decode_timed on the same keywords, and pk_tdt_align_decode_timed of the
same strings given as transcripts (one call per keyword, every clip aligned against it; summed over the keywords).
The lattice stage's rate: TF by the count 2 T L (V + D) J over the pairs (the columns the walk reads) and by the rows the product really
computes, T (L + 1) per pair (column L is packed and not read).  prefix_share: the fraction of the (keyword, column >= 1) prediction-net
states that another keyword of the call with the same prefix also has -- what a prefix-shared lattice could save.
With --pcm the 60-minute clip also goes through Model.spot_tdt from PCM with attention context [128,128] (wall ms of the whole call).
Writes the result lines and a table to --out (default profiles/tdt_kws.md).
usage: python tools/bench_tdt_kws.py [--reps 3] [--hits 1] [--pcm] [--no-align] [--out profiles/tdt_kws.md]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hits", type=int, default=1)
    ap.add_argument("--pcm", action="store_true")
    ap.add_argument("--no-align", action="store_true", help="skip the aligner's figure")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdt_kws.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config()
    rng = np.random.default_rng(1)
    V, D, J = cfg.vocab_size, len(cfg.durations), cfg.joint_hidden
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def rows(t):
        x = rng.standard_normal((t, cfg.hidden_size)).astype(np.float32)
        return (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)

    frames = lambda sec: capi.lib().pk_encoder_num_frames(capi.lib().pk_mel_num_frames(int(sec * 16000)))
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        for name, n, sec in (("64 x 10 s", 64, 10.0), ("1 x 60 min", 1, 3600.0)):
            enc = np.stack([rows(frames(sec)) for _ in range(n)])
            T = int(enc.shape[1])
            source = "greedy tdt"
            try:
                g = gm.tdt_decode(enc)
            except capi.PkError:                                     # synthetic weights can run greedy TDT into its safety cap: the CTC head's greedy output
                source = "greedy ctc"
                g = gm.ctc_decode(enc)
            said = [g["ids"][b, :g["lens"][b]] for b in range(n)]
            for n_kw in (1, 16, 128):
                kws = []
                for k in range(n_kw):                                # 1 .. 8 tokens from somewhere in some clip's greedy output
                    s = said[k % n]
                    L = 1 + k % 8
                    at = int(rng.integers(0, max(1, len(s) - L)))
                    kw = np.ascontiguousarray(s[at:at + L], np.int32)
                    if len(kw) < L:                                  # (a clip that decoded fewer tokens: pad with a fixed token)
                        kw = np.concatenate([kw, np.full(L - len(kw), 1, np.int32)])
                    kws.append(kw)
                r = gm.tdt_kws_decode(enc, kws, max_hits=a.hits)      # warm-up of the buffers
                walls = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = gm.tdt_kws_decode(enc, kws, max_hits=a.hits)
                    walls.append((time.perf_counter() - t0) * 1e3)
                net, lat, walk = gm.tdt_kws_decode_timed(enc, kws, max_hits=a.hits, reps=a.reps)
                sumL = int(sum(len(k) for k in kws))
                useful = 2.0 * n * T * sumL * (V + D) * J
                done = 2.0 * n * T * (sumL + n_kw) * (V + D) * J
                prefixes = {}
                for k in kws:
                    for u in range(1, len(k) + 1):
                        prefixes[tuple(k[:u])] = prefixes.get(tuple(k[:u]), 0) + 1
                shared = sum(c - 1 for c in prefixes.values())
                out = {"metric": "tdt keyword spotting ms", "config": "tdt-ctc-110m", "batch": name, "frames": T, "keywords": n_kw, "keywords_from": source, "max_hits": a.hits,
                       "exact_hits": int((r["score"][:, :, 0] == 0).sum()), "reps": a.reps,
                       "wall_ms_upload_encproj_spot_download": round(float(np.median(walls)), 3), "pred_net_ms": round(net, 3),
                       "lattice_ms": round(lat, 3), "walk_pick_ms": round(walk, 3),
                       "lattice_tf_2TL(V+D)J": round(useful / (lat * 1e-3) / 1e12, 1), "lattice_tf_rows_computed": round(done / (lat * 1e-3) / 1e12, 1),
                       "walk_us_per_keyword_frame": round(walk * 1e3 / (n_kw * T), 4), "prefix_share": round(shared / max(1, sumL), 3)}
                ch, cs = gm.ctc_kws_decode_timed(enc, kws, max_hits=a.hits, reps=a.reps)
                out["ctc_head_stage_ms"] = round(ch, 3)
                out["ctc_spot_stage_ms"] = round(cs, 3)
                if not a.no_align:
                    tot = np.zeros(3)
                    for kw in kws:                                   # the TDT aligner for the same strings: one call per keyword
                        tot += np.asarray(gm.tdt_align_decode_timed(enc, [kw] * n, reps=a.reps)[:3])
                    out["tdt_align_pred_lattice_walk_ms_sum_over_keywords"] = [round(float(v), 3) for v in tot]
                emit(out)
            if a.pcm and n == 1:
                gm.set_attention_context(128, 128)
                pcm = synth.synth_pcm(1, int(sec * 16000), seed=3)[0]
                t0 = time.perf_counter()
                res = gm.spot_tdt([pcm], ids=[k.tolist() for k in kws], max_hits=a.hits)
                emit({"metric": "pcm to hits wall ms, attention context [128,128]", "batch": name, "keywords": len(kws),
                      "wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "hits": int(sum(len(h) for h in res[0]))})
                gm.set_attention_context(-1, -1)
        gm.close()
    with open(a.out, "w") as f:
        f.write("# TDT keyword spotting: stage times (tools/bench_tdt_kws.py)\n\n")
        f.write("One MI355X, tdt-ctc-110m shapes, synthetic weights, random encoder rows, keywords of 1 .. 8 tokens cut from the clips' greedy output, "
                f"max_hits = {a.hits}, medians of {a.reps} passes.  Times in ms.\n\n")
        f.write("| batch | keywords | pred net | lattice | walk + pick | lattice TF, 2TL(V+D)J | lattice TF, rows computed | CTC head | CTC spotting | TDT align, summed (net / lattice / walk) |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|\n")
        for d in lines:
            if "pred_net_ms" not in d:
                continue
            al = d.get("tdt_align_pred_lattice_walk_ms_sum_over_keywords")
            f.write(f"| {d['batch']} (T = {d['frames']}) | {d['keywords']} | {d['pred_net_ms']} | {d['lattice_ms']} | {d['walk_pick_ms']} | "
                    f"{d['lattice_tf_2TL(V+D)J']} | {d['lattice_tf_rows_computed']} | {d['ctc_head_stage_ms']} | {d['ctc_spot_stage_ms']} | "
                    f"{' / '.join(map(str, al)) if al else '-'} |\n")
        f.write("\nResult lines:\n\n```\n" + "\n".join(json.dumps(d) for d in lines) + "\n```\n")


if __name__ == "__main__":
    main()
