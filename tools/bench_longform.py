#!/usr/bin/env python3
"""Long-form offline transcription with limited-context attention (pk_model_set_attention_context): ONE long synthetic clip through
pk_transcribe_pcm, once per window, plus the stage path (mel -> encode -> decode) timed stage by stage.  Synthetic weights at the shapes
of --config (tdt-ctc-110m by default: tokens are meaningless, the work is the real work).  Prints one JSON line per window: audio seconds,
encoder frames, wall ms of pk_transcribe_pcm (median of --reps after one warm-up), RTFx and the stage wall times.
usage: python tools/bench_longform.py [--minutes 60] [--windows 128,128 256,256 full] [--decoder ctc] [--reps 2] [--config tdt-ctc-110m]"""
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
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--windows", nargs="+", default=["128,128", "256,256"], help="left,right pairs; full = full attention (-1, -1)")
    ap.add_argument("--decoder", default="ctc", choices=["tdt", "ctc"], help="ctc (default): the TDT loop of synthetic weights may emit a token per frame")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--config", default="tdt-ctc-110m", choices=["tdt-ctc-110m", "tdt-600m"])
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config() if a.config == "tdt-ctc-110m" else pk.make_tdt_600m_config()
    n = int(a.minutes * 60 * 16000)
    t = np.arange(n, dtype=np.float64) / 16000.0
    pcm = (0.05 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    del t
    T = capi.lib().pk_encoder_num_frames(1 + n // 160)
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        for w in a.windows:
            left, right = (-1, -1) if w == "full" else (int(v) for v in w.split(","))
            gm.set_attention_context(left, right)
            gm.transcribe_pcm([pcm], decoder=a.decoder)                       # warm-up: workspace, local tables
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = gm.transcribe_pcm([pcm], decoder=a.decoder)[0]
                walls.append((time.perf_counter() - t0) * 1e3)
            wall = float(np.median(walls))
            st = {}
            t0 = time.perf_counter()
            feats = gm.mel(pcm[None])
            st["mel_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            enc = gm.encode(feats)
            st["encode_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            (gm.tdt_decode if a.decoder == "tdt" else gm.ctc_decode)(enc)
            st["decode_ms"] = (time.perf_counter() - t0) * 1e3
            del feats, enc
            print(json.dumps({"metric": "longform RTFx", "config": a.config, "decoder": a.decoder, "window": [left, right],
                              "audio_seconds": n / 16000.0, "encoder_frames": T, "wall_ms": round(wall, 1),
                              "rtfx": round(n / 16000.0 / (wall / 1e3), 1), "n_tokens": len(r["token_ids"]),
                              "stage_ms_host_buffers": {k: round(v, 1) for k, v in st.items()}}), flush=True)
        gm.close()


if __name__ == "__main__":
    main()
