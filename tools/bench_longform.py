#!/usr/bin/env python3
"""Long-form offline transcription with limited-context attention (pk_model_set_attention_context): ONE long synthetic clip through
pk_transcribe_pcm, once per window, plus the stage path (mel -> encode -> decode) timed stage by stage.  Synthetic weights at the shapes
of --config (tdt-ctc-110m by default: tokens are meaningless, the work is the real work).  Prints one JSON line per window: audio seconds,
encoder frames, wall ms of pk_transcribe_pcm (median of --reps after one warm-up), RTFx and the stage wall times.
--bf16 builds a gemm_bf16 model.  --local-attention-bf16 (with --bf16) measures every window with the bf16 band kernel off AND on
(pk_model_set_local_attention_bf16), the timed calls of the two interleaved, one line each.  --kernels N adds, from a one-clip pk_batch of the
same audio, the device-side stage times (pk_batch_run_timed, median of N) and the attention launch per layer with the encoder share it makes up
(pk_batch_profile: HIP events around every launch, median of N).
usage: python tools/bench_longform.py [--minutes 60] [--windows 128,128 256,256 full] [--decoder ctc] [--reps 2] [--config tdt-ctc-110m]
                                      [--bf16 [--local-attention-bf16]] [--kernels 5]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np


def kernel_times(capi, gm, pcm, dec, n):
    """device-side figures of one un-pipelined step of a one-clip batch: stage ms (median of n timed runs) and, from n profiled runs, the
    attention launch per layer (us) and the sum of every encoder-layer launch's time it is a share of"""
    L = capi.lib()
    bt = capi.Batch(gm, 1, pcm.shape[0])
    try:
        bt.upload(pcm[None])
        bt.run({0: "ctc", 1: "tdt"}[dec]); bt.sync()
        stage = []
        for _ in range(n):
            ms = (C.c_float * 4)()
            capi.check(L.pk_batch_run_timed(bt._h, dec, ms))
            stage.append(list(ms))
        att, total = [], []
        for _ in range(n):
            stats = (capi.PkKernelStat * 64)()
            nk = max(0, min(L.pk_batch_profile(bt._h, dec, stats, 64), 64))
            by = {stats[i].name.decode(): (stats[i].total_ms, stats[i].launches) for i in range(nk)}
            a_ms, a_n = by["relpos_attention"]
            att.append(1e3 * a_ms / a_n)
            total.append(sum(v[0] for v in by.values()))
        mel, enc, decode, tot = (float(np.median([s[i] for s in stage])) for i in range(4))
        a_us = float(np.median(att))
        return {"batch_stage_ms": {"mel": round(mel, 2), "encoder": round(enc, 2), "decode": round(decode, 2), "total": round(tot, 2)},
                "attention_us_per_layer": round(a_us, 1), "attention_share_of_encoder": round(a_us * 1e-3 * a_n / enc, 4),
                "profiled_launch_sum_ms": round(float(np.median(total)), 2)}
    finally:
        bt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--windows", nargs="+", default=["128,128", "256,256"], help="left,right pairs; full = full attention (-1, -1)")
    ap.add_argument("--decoder", default="ctc", choices=["tdt", "ctc"], help="ctc (default): the TDT loop of synthetic weights may emit a token per frame")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--config", default="tdt-ctc-110m", choices=["tdt-ctc-110m", "tdt-600m"])
    ap.add_argument("--bf16", action="store_true", help="a gemm_bf16 model (the tolerance-class mode)")
    ap.add_argument("--local-attention-bf16", action="store_true", help="every window with the bf16 band kernel off and on, interleaved (needs --bf16)")
    ap.add_argument("--kernels", type=int, default=0, help="N > 0: device-side stage times and the attention launch per layer, medians of N")
    a = ap.parse_args()
    if a.local_attention_bf16 and not a.bf16:
        raise SystemExit("--local-attention-bf16 needs --bf16: the bf16 band kernel is refused on an fp32 model")
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config() if a.config == "tdt-ctc-110m" else pk.make_tdt_600m_config()
    if a.config == "tdt-600m" and a.decoder == "ctc" and cfg.ctc_vocab_size <= 0:
        cfg = dataclasses.replace(cfg, ctc_vocab_size=cfg.vocab_size)     # a CTC head of its own on the 600M shapes (synthetic weights)
    if a.bf16:
        cfg = dataclasses.replace(cfg, gemm_bf16=True)
    n = int(a.minutes * 60 * 16000)
    t = np.arange(n, dtype=np.float64) / 16000.0
    pcm = (0.05 * np.sin(2 * np.pi * 220.0 * t) + 0.02 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    del t
    T = capi.lib().pk_encoder_num_frames(1 + n // 160)
    dec = {"ctc": 0, "tdt": 1}[a.decoder]
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        for w in a.windows:
            left, right = (-1, -1) if w == "full" else (int(v) for v in w.split(","))
            gm.set_attention_context(left, right)
            modes = [False, True] if a.local_attention_bf16 and left >= 0 else [False]
            walls, last = {m: [] for m in modes}, {}
            for m in modes:                                                       # warm-up: workspace, local tables of both formats
                gm.set_local_attention_bf16(m) if a.bf16 else None
                gm.transcribe_pcm([pcm], decoder=a.decoder)
            for _ in range(a.reps):
                for m in modes:                                                   # interleaved: off, on, off, on, ...
                    gm.set_local_attention_bf16(m) if a.bf16 else None
                    t0 = time.perf_counter()
                    last[m] = gm.transcribe_pcm([pcm], decoder=a.decoder)[0]
                    walls[m].append((time.perf_counter() - t0) * 1e3)
            for m in modes:
                gm.set_local_attention_bf16(m) if a.bf16 else None
                wall = float(np.median(walls[m]))
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
                line = {"metric": "longform RTFx", "config": a.config, "bf16": bool(a.bf16), "local_attention_bf16": m, "decoder": a.decoder,
                        "window": [left, right], "audio_seconds": n / 16000.0, "encoder_frames": T, "wall_ms": round(wall, 1),
                        "rtfx": round(n / 16000.0 / (wall / 1e3), 1), "n_tokens": len(last[m]["token_ids"]),
                        "stage_ms_host_buffers": {k: round(v, 1) for k, v in st.items()}}
                print(json.dumps(line), flush=True)
                if a.kernels > 0:
                    print(json.dumps({"metric": "longform kernels", "config": a.config, "bf16": bool(a.bf16), "local_attention_bf16": m,
                                      "window": [left, right], **kernel_times(capi, gm, pcm, dec, a.kernels)}), flush=True)
            if a.bf16:
                gm.set_local_attention_bf16(False)
        gm.close()


if __name__ == "__main__":
    main()
