#!/usr/bin/env python3
"""The device resampler (kernels/resample.hip) on 64 clips of 10 s at 48 kHz and at 44.1 kHz, tdt-ctc-110m shapes with synthetic weights.
Per rate, medians of --reps passes after a warm-up:
  stage      the resampling launch alone, HIP events around it (pk_resample_device_timed; input on the device, nothing read back)
  device     wall ms of Model.transcribe_pcm on the input-rate clips with set_input_rate(rate)
  host       what a caller does without it: pk_resample of every clip on the host (one thread), then transcribe_pcm at 16 kHz
  16 kHz     transcribe_pcm on the already resampled clips: the step the stage is added to
and how often the walk of tests/resample_ref.py differs from pk_resample on 10 s of N(0, 0.1) noise (seed 7), the input of
tests/test_resample_ref.py.  Writes profiles/resample.md.
usage: python tools/bench_resample.py [--reps 5] [--clips 64] [--seconds 10] [--out profiles/resample.md]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    import resample_ref as R
    cfg = pk.make_110m_config()
    lines = ["# Device resampler (kernels/resample.hip)", "",
             f"`python tools/bench_resample.py --reps {a.reps} --clips {a.clips} --seconds {a.seconds:g}`: {a.clips} clips of {a.seconds:g} s, tdt-ctc-110m shapes, "
             "synthetic weights, TDT decoder; medians.", "",
             "| input rate | stage alone (ms) | one call, device route (ms) | host pk_resample (ms) | 16 kHz call (ms) | host route = resample + call (ms) | "
             "host route / device route | stage / 16 kHz call |", "|---|---|---|---|---|---|---|---|"]
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        for rate in (48000, 44100):
            raw = [synth.synth_pcm(1, int(a.seconds * rate), seed=100 + i, sr=rate)[0] for i in range(a.clips)]
            stage = capi.resample_device_timed(raw, rate, 16000, reps=max(a.reps, 5))
            t0 = time.perf_counter()
            down = [capi.resample(c, rate, 16000) for c in raw]
            host = (time.perf_counter() - t0) * 1e3
            gm.set_input_rate(rate)
            dev_call = median_ms(lambda: gm.transcribe_pcm(raw), a.reps)
            gm.set_input_rate(16000)
            call16 = median_ms(lambda: gm.transcribe_pcm(down), a.reps)
            verdict = "" if dev_call < host + call16 else " **the device route is NOT faster**"
            lines.append(f"| {rate} | {stage:.3f} | {dev_call:.1f} | {host:.0f} | {call16:.1f} | {host + call16:.0f} | {(host + call16) / dev_call:.1f}x{verdict} | "
                         f"{100 * stage / call16:.2f} % |")
            print(lines[-1], flush=True)
        gm.close()
    lines += ["", "The device route uploads the input-rate samples (3x resp. 2.76x the bytes of the 16 kHz call) and adds the stage; the host route spends "
              "its time in `pk_resample`, one thread, before the call starts.", "",
              "## The table form against pk_resample", "",
              "10 s of N(0, 0.1) float32 noise (numpy default_rng(7)): samples at which the walk of `tests/resample_ref.py` (which the kernel reproduces bit for bit) "
              "differs from `pk_resample`.  `tests/test_resample_ref.py` caps the share at 2e-3 and every difference at ulp32(peak) + 1e-8 peak.", "",
              "| rates | differing samples | share | max abs difference | peak |", "|---|---|---|---|---|"]
    for src in (48000, 32000, 8000, 44100, 22050, 11025):
        x = (np.random.default_rng(7).standard_normal(10 * src) * 0.1).astype(np.float32)
        w, h = R.walk(x, src, 16000), capi.resample(x, src, 16000)
        d = np.abs(w.astype(np.float64) - h.astype(np.float64))
        n = int(np.count_nonzero(w.view(np.uint32) != h.view(np.uint32)))
        lines.append(f"| {src} -> 16000 | {n} of {w.size} | {n / w.size:.2e} | {d.max():.3e} | {np.abs(h).max():.4f} |")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
