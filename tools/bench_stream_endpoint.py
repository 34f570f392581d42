#!/usr/bin/env python3
"""Endpointing on live audio (kernels/endpoint.hip): what watching for the end of the utterance costs a streaming session.
nemotron-600m shapes with synthetic weights, 16 lock-step streams, 160 ms chunks (2560 samples), synthetic audio.  On the same session:
  push                 wall ms per chunk of pk_stream_push
  push_endpoint        ... of pk_stream_push_endpoint (reset_decoder = 0: the closes are about one per utterance and not on the steady path)
  push_spot            ... of pk_stream_push_spot with one keyword (the yardstick: profiles/stream_kws.md's 0.10 ms, measured again in this run)
  push_endpoint + kws  ... of pk_stream_push_endpoint with one keyword (wake word, transcript and end of turn from one push)
  kernel               pk_stream_endpoint_timed on one chunk's mel rows: the chunk kernel alone, HIP events
medians over the chunks of a pass, then the median of --reps passes after one warm-up pass.
Synthetic weights and audio: the costs are those of the shapes, not of speech; real speech and more than 16 streams are not measured.
Writes the result lines and a table to --out (default profiles/stream_endpoint.md).
usage: python tools/bench_stream_endpoint.py [--reps 3] [--chunks 40] [--streams 16] [--out profiles/stream_endpoint.md]"""
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
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_endpoint.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_nemotron_600m_config()
    S, CH = a.streams, 2560
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        pcm = synth.synth_pcm(S, CH * a.chunks, seed=9)
        seg = lambda i: pcm[:, i * CH:(i + 1) * CH]
        st = capi.Stream(gm, S, 70, 1)

        def one_pass(fn):
            """-> median wall ms per chunk, and the END events seen"""
            st.reset()
            ms, ends = [], 0
            for i in range(a.chunks):
                t = time.perf_counter()
                r = fn(seg(i))
                dt = (time.perf_counter() - t) * 1e3
                ends += sum(1 for e in r.get("events", []) if len(e) == 6 and e[1] == capi.ENDPOINT_END)
                if i >= 2:                                          # (the first chunks have no cache yet and other shapes)
                    ms.append(dt)
            return float(np.median(ms)), ends

        def timed(fn):
            runs = [one_pass(fn) for _ in range(a.reps + 1)][1:]
            return float(np.median([r[0] for r in runs])), runs[-1][1]

        # the streams' own first greedy token as the one keyword, and one chunk's mel rows for the kernel timer
        mel1, kw = None, None
        for i in range(a.chunks):
            m = st.mel(seg(i))
            if m.shape[1]:
                mel1 = m
            e = st.encode(m) if m.shape[1] else m
            if e.shape[1]:
                r = st.decode(e)
                if kw is None and r["lens"].sum():
                    s0 = int(np.argmax(r["lens"] > 0))
                    kw = [int(r["ids"][s0, 0])]
        kw = kw or [1]
        # thresholds that cut the synthetic audio into utterances: its level in the middle of what the streams show
        lv = mel1.sum(axis=2)
        thr_db = float(np.median(lv) / cfg.mel_bins * 10.0 / np.log(10.0))
        opt = dict(threshold_db=thr_db, margin_db=0.0, min_silence_ms=100, min_speech_ms=30, reset_decoder=0)

        push_ms, _ = timed(st.push)
        st.set_endpointing(**opt)
        ep_ms, ends = timed(st.push_endpoint)
        push2_ms, _ = timed(st.push)
        st.reset()
        kernel_ms = st.endpoint_timed(mel1, reps=a.reps)
        emit(dict(case="push_endpoint", streams=S, chunk_ms=160, mel_frames_per_chunk=int(mel1.shape[1]), push_ms_per_chunk=round(push_ms, 4),
                  push_endpoint_ms_per_chunk=round(ep_ms, 4), push_ms_per_chunk_endpointing_set=round(push2_ms, 4), added_ms=round(ep_ms - push_ms, 4),
                  kernel_ms=round(kernel_ms, 4), end_events_per_pass=ends, threshold_db=round(thr_db, 2)))
        st.set_keywords(ids=[kw])
        spot_ms, _ = timed(st.push_spot)
        both_ms, _ = timed(lambda x: st.push_endpoint(x, spot=True))
        push3_ms, _ = timed(st.push)
        emit(dict(case="one_keyword", push_ms_per_chunk=round(push3_ms, 4), push_spot_ms_per_chunk=round(spot_ms, 4),
                  push_endpoint_kws_ms_per_chunk=round(both_ms, 4), spot_added_ms=round(spot_ms - push3_ms, 4),
                  endpoint_kws_added_ms=round(both_ms - push3_ms, 4)))
        st.close()
        gm.close()
    d0, d1 = lines
    with open(a.out, "w") as f:
        f.write("# Endpointing on live audio: cost per 160 ms chunk (tools/bench_stream_endpoint.py)\n\n")
        f.write(f"nemotron-600m shapes, synthetic weights and audio, {S} lock-step streams, {d0['mel_frames_per_chunk']} mel frames per chunk and stream, "
                f"medians of {a.reps} passes after a warm-up.\nReal speech and more than {S} streams are not measured.\n\n")
        f.write("| call | ms per chunk | added to pk_stream_push |\n|---|---|---|\n")
        f.write(f"| pk_stream_push | {d0['push_ms_per_chunk']} | |\n")
        f.write(f"| pk_stream_push_endpoint | {d0['push_endpoint_ms_per_chunk']} | {d0['added_ms']} |\n")
        f.write(f"| pk_stream_push, endpointing set | {d0['push_ms_per_chunk_endpointing_set']} | |\n")
        f.write(f"| pk_stream_push, one keyword set | {d1['push_ms_per_chunk']} | |\n")
        f.write(f"| pk_stream_push_spot, one keyword | {d1['push_spot_ms_per_chunk']} | {d1['spot_added_ms']} |\n")
        f.write(f"| pk_stream_push_endpoint, one keyword | {d1['push_endpoint_kws_ms_per_chunk']} | {d1['endpoint_kws_added_ms']} |\n")
        f.write(f"| endpoint_chunk_kernel alone (HIP events) | {d0['kernel_ms']} | |\n")
        f.write("\n```\n" + "\n".join(json.dumps(d) for d in lines) + "\n```\n")


if __name__ == "__main__":
    main()
