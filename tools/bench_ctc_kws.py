#!/usr/bin/env python3
"""CTC keyword spotting (kernels/ctc_kws.hip): wall ms of the call and the stage timers of pk_ctc_kws_decode_timed (HIP events on the model's
stream, medians of --reps passes after a warm-up): ms[0] the CTC head + log-softmax, ms[1] the spotting (keyword upload, row maxima, walk,
picking).  tdt-ctc-110m shapes with synthetic weights, encoder rows drawn at random, keywords of 1 .. 8 tokens cut from the clips' own greedy
CTC output.  Lines: 64 x 10 s with 1 / 16 / 128 keywords, one 60-minute clip with the same counts.
Next to each: the comparable existing cost, the alignment stage of pk_ctc_align_decode_timed for the same clips with the same strings given as
transcripts (one call per keyword, every clip aligned against it; the sum over the keywords) -- also a sequential walk over T frames per
string, but with a barrier per frame and back-pointer stores.
With --pcm the 60-minute clip also goes through Model.spot from PCM with attention context [128,128] (wall ms of the whole call).
usage: python tools/bench_ctc_kws.py [--reps 5] [--hits 1] [--pcm] [--no-align]"""
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
    ap.add_argument("--hits", type=int, default=1)
    ap.add_argument("--pcm", action="store_true")
    ap.add_argument("--no-align", action="store_true", help="skip the aligner's figure")
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
        for name, n, sec in (("64 x 10 s", 64, 10.0), ("1 x 60 min", 1, 3600.0)):
            enc = np.stack([rows(frames(sec)) for _ in range(n)])
            g = gm.ctc_decode(enc)
            said = [g["ids"][b, :g["lens"][b]] for b in range(n)]
            for n_kw in (1, 16, 128):
                kws = []
                for k in range(n_kw):                                # 1 .. 8 tokens from somewhere in some clip's greedy output
                    s = said[k % n]
                    L = 1 + k % 8
                    at = int(rng.integers(0, max(1, len(s) - L)))
                    kws.append(np.ascontiguousarray(s[at:at + L], np.int32))
                r = gm.ctc_kws_decode(enc, kws, max_hits=a.hits)      # warm-up of the buffers
                walls = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = gm.ctc_kws_decode(enc, kws, max_hits=a.hits)
                    walls.append((time.perf_counter() - t0) * 1e3)
                head, stage = gm.ctc_kws_decode_timed(enc, kws, max_hits=a.hits, reps=a.reps)
                out = {"metric": "ctc keyword spotting ms", "config": "tdt-ctc-110m", "batch": name, "frames": int(enc.shape[1]), "keywords": n_kw,
                       "max_hits": a.hits, "exact_hits": int((r["score"][:, :, 0] == 0).sum()), "reps": a.reps,
                       "wall_ms_upload_head_spot_download": round(float(np.median(walls)), 3), "ctc_head_stage_ms": round(head, 3),
                       "spot_stage_ms": round(stage, 3), "spot_us_per_keyword_frame": round(stage * 1e3 / (n_kw * enc.shape[1]), 4)}
                if not a.no_align:
                    tot = 0.0
                    for kw in kws:                                   # the aligner's walk for the same strings: one call per keyword
                        tot += gm.ctc_align_decode_timed(enc, [kw] * n, total=False, reps=a.reps)[1]
                    out["aligner_stage_ms_sum_over_keywords"] = round(tot, 3)
                    out["aligner_us_per_keyword_frame"] = round(tot * 1e3 / (n_kw * enc.shape[1]), 4)
                print(json.dumps(out), flush=True)
            if a.pcm and n == 1:
                gm.set_attention_context(128, 128)
                pcm = synth.synth_pcm(1, int(sec * 16000), seed=3)[0]
                t0 = time.perf_counter()
                res = gm.spot([pcm], ids=[k.tolist() for k in kws], max_hits=a.hits)
                print(json.dumps({"metric": "pcm to hits wall ms, attention context [128,128]", "batch": name, "keywords": len(kws),
                                  "wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "hits": int(sum(len(h) for h in res[0]))}), flush=True)
                gm.set_attention_context(-1, -1)
        gm.close()


if __name__ == "__main__":
    main()
