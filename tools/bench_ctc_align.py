#!/usr/bin/env python3
"""CTC forced alignment of given token strings (kernels/ctc_align.hip): wall ms of the call and the alignment stage's ms
(pk_ctc_align_decode_timed: HIP events on the model's stream, median of --reps passes after a warm-up).  tdt-ctc-110m shapes with synthetic
weights, encoder rows drawn at random.  Four lines: 64 x 10 s aligning each clip's greedy CTC output; one 4-minute clip; one 60-minute clip
(the long clips align every third token of their greedy output: random weights give a token on nearly every frame, speech gives about one
on every third); the 60-minute clip again with 15000 tokens spread evenly over its greedy output (the capacity target T = 45000, L = 15000).
With --pcm the long clips also go through Model.align from PCM with attention context [128,128] (wall ms of the whole call).
With --compare-beam, two more lines: the alignment ctc_beam_align_kernel does for the beam search on the shapes it can do (64 x T = 126 and one
T = 3200): pk_ctc_beam_decode_timed at W = 1, K = 1, N = 1 with timestamps minus without, next to this kernel's alignment stage for the
same ids on the same rows.
usage: python tools/bench_ctc_align.py [--reps 5] [--total] [--pcm] [--compare-beam]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--total", action="store_true", help="also run the forward pass (the CTC log-likelihood)")
    ap.add_argument("--pcm", action="store_true")
    ap.add_argument("--compare-beam", action="store_true")
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
        for name, n, sec, every in (("64 x 10 s", 64, 10.0, 1), ("1 x 4 min", 1, 240.0, 3), ("1 x 60 min", 1, 3600.0, 3), ("1 x 60 min, 15000 tokens", 1, 3600.0, 0)):
            enc = np.stack([rows(frames(sec)) for _ in range(n)])
            g = gm.ctc_decode(enc)
            if every:
                ids = [g["ids"][b, :g["lens"][b]][::every] for b in range(n)]
            else:
                ids = [g["ids"][0, :g["lens"][0]][np.linspace(0, g["lens"][0] - 1, 15000).astype(np.int64)]]
            gm.ctc_align_decode(enc, ids, total=a.total)                                  # warm-up of the buffers
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = gm.ctc_align_decode(enc, ids, total=a.total)
                walls.append((time.perf_counter() - t0) * 1e3)
            head, stage = gm.ctc_align_decode_timed(enc, ids, total=a.total, reps=a.reps)
            out = {"metric": "ctc forced alignment ms", "config": "tdt-ctc-110m", "batch": name, "frames": int(enc.shape[1]),
                   "tokens_per_clip": int(np.mean([len(x) for x in ids])), "ok": int(sum(x["ok"] for x in r)), "total": bool(a.total), "reps": a.reps,
                   "wall_ms_upload_head_align_download": round(float(np.median(walls)), 3), "ctc_head_stage_ms": round(head, 3),
                   "align_stage_ms": round(stage, 3)}
            if a.pcm and n == 1:
                gm.set_attention_context(128, 128)
                pcm = synth.synth_pcm(1, int(sec * 16000), seed=3)[0]
                t0 = time.perf_counter()
                res = gm.align([pcm], ids=[ids[0]], total=a.total)
                out["pcm_to_timestamps_wall_ms_context_128_128"] = round((time.perf_counter() - t0) * 1e3, 1)
                out["pcm_ok"] = res[0]["ok"]
                gm.set_attention_context(-1, -1)
            print(json.dumps(out), flush=True)
        for n, T in ((64, 126), (1, 3200)) if a.compare_beam else ():
            enc = np.stack([rows(T) for _ in range(n)])
            _, with_ts = gm.ctc_beam_decode_timed(enc, 1, 1, 1, True, a.reps)
            _, without = gm.ctc_beam_decode_timed(enc, 1, 1, 1, False, a.reps)
            hyp = gm.ctc_beam_decode(enc, 1, 1, 1, timestamps=True)
            ids = [hyp["ids"][b, 0, :hyp["lens"][b, 0]] for b in range(n)]
            _, new = gm.ctc_align_decode_timed(enc, ids, total=False, reps=a.reps)
            al = gm.ctc_align_decode(enc, ids, total=False)
            same = all(np.array_equal(al[b]["start"], hyp["start"][b, 0, :len(ids[b])]) and np.array_equal(al[b]["end"], hyp["end"][b, 0, :len(ids[b])])
                       for b in range(n))
            print(json.dumps({"metric": "alignment of the beam search's hypothesis, old kernel vs new, ms", "clips": n, "frames": T,
                              "tokens_per_clip": int(np.mean([len(x) for x in ids])), "beam_W1_with_timestamps_ms": round(with_ts, 3),
                              "beam_W1_without_ms": round(without, 3), "old_alignment_ms": round(with_ts - without, 3),
                              "new_alignment_stage_ms": round(new, 3), "same_frames": bool(same)}), flush=True)
        gm.close()


if __name__ == "__main__":
    main()
