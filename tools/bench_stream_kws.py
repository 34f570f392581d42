#!/usr/bin/env python3
"""Streaming TDT keyword spotting (kernels/tdt_kws_stream.hip): what watching a keyword list costs a streaming session.
nemotron-600m shapes with synthetic weights, 16 lock-step streams, 160 ms chunks (2560 samples), synthetic audio.  For 1 / 8 / 64 keywords of
1 .. 8 tokens cut from the streams' own greedy output (random ids where that is too short):
  push / push_spot   wall ms per chunk of pk_stream_push and of pk_stream_push_spot on the same build, the same audio and fresh sessions: medians
                     over the chunks of a pass, then the median of --reps passes after one warm-up pass
  set_keywords       wall ms of pk_stream_set_keywords (the prediction net, once per distinct keyword, and the allocation of the carried state)
  lattice / walk     pk_stream_spot_timed on one chunk's encoder rows: HIP events, enc_proj + lattice, and normalisation + walk + rule
Synthetic weights and audio: the costs are those of the shapes, not of speech; real speech and keywords near 64 tokens are not measured.
Writes the result lines and a table to --out (default profiles/stream_kws.md).
usage: python tools/bench_stream_kws.py [--reps 3] [--chunks 40] [--streams 16] [--out profiles/stream_kws.md]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_kws.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_nemotron_600m_config()
    S, CH = a.streams, 2560
    rng = np.random.default_rng(1)
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

        def one_pass(st, fn):
            """-> median wall ms per chunk over the chunks that produced frames"""
            st.reset()
            ms = []
            for i in range(a.chunks):
                t = time.perf_counter()
                r = fn(seg(i))
                dt = (time.perf_counter() - t) * 1e3
                if i >= 2:                                          # (the first chunks have no cache yet and other shapes)
                    ms.append(dt)
            return float(np.median(ms)), r

        # the streams' own greedy tokens, and one chunk's encoder rows for the stage timers
        st = capi.Stream(gm, S, 70, 1)
        toks, enc1 = [], None
        for i in range(a.chunks):
            m = st.mel(seg(i))
            e = st.encode(m) if m.shape[1] else m
            if e.shape[1]:
                enc1 = e
                r = st.decode(e)
                toks += [r["ids"][s, :r["lens"][s]].tolist() for s in range(S)]
        flat = [t for row in toks for t in row if t != cfg.blank_id]
        source = "greedy tdt"
        if len(flat) < 64:
            source = "random ids"
            flat = [int(v) for v in rng.integers(0, cfg.vocab_size - 1, size=4096) if v != cfg.blank_id]

        def keywords(n):
            out, at = [], 0
            for k in range(n):
                L = 1 + k % 8
                out.append([flat[(at + j) % len(flat)] for j in range(L)])
                at += L
            return out

        passes = [one_pass(st, st.push)[0] for _ in range(a.reps + 1)][1:]
        push_ms = float(np.median(passes))
        emit(dict(case="push", streams=S, chunk_ms=160, ms_per_chunk=round(push_ms, 4), frames_per_chunk=int(enc1.shape[1])))
        for n_kw in (1, 8, 64):
            kws = keywords(n_kw)
            t = time.perf_counter()
            st.set_keywords(ids=kws)
            set_ms = (time.perf_counter() - t) * 1e3
            spot = float(np.median([one_pass(st, st.push_spot)[0] for _ in range(a.reps + 1)][1:]))
            again = float(np.median([one_pass(st, st.push)[0] for _ in range(a.reps + 1)][1:]))
            st.reset()
            lat_ms, walk_ms = st.spot_timed(enc1, reps=a.reps)
            emit(dict(case="push_spot", keywords=n_kw, pairs=S * n_kw, tokens=sum(len(k) for k in kws), source=source, set_keywords_ms=round(set_ms, 3),
                      push_spot_ms_per_chunk=round(spot, 4), push_ms_per_chunk_same_session=round(again, 4), added_ms=round(spot - again, 4),
                      lattice_ms=round(lat_ms, 4), walk_rule_ms=round(walk_ms, 4)))
        st.close()
        gm.close()
    with open(a.out, "w") as f:
        f.write("# Streaming TDT keyword spotting: cost per 160 ms chunk (tools/bench_stream_kws.py)\n\n")
        f.write(f"nemotron-600m shapes, synthetic weights and audio, {S} lock-step streams, medians of {a.reps} passes after a warm-up.\n")
        f.write("Real speech and keywords near 64 tokens are not measured.\n\n")
        f.write("| keywords | pairs | set_keywords ms | push ms/chunk | push_spot ms/chunk | added ms | lattice ms (events) | walk + rule ms (events) |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for d in lines:
            if d["case"] == "push_spot":
                f.write(f"| {d['keywords']} | {d['pairs']} | {d['set_keywords_ms']} | {d['push_ms_per_chunk_same_session']} | {d['push_spot_ms_per_chunk']} | "
                        f"{d['added_ms']} | {d['lattice_ms']} | {d['walk_rule_ms']} |\n")
        f.write("\n```\n" + "\n".join(json.dumps(d) for d in lines) + "\n```\n")


if __name__ == "__main__":
    main()
