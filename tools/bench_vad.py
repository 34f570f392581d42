#!/usr/bin/env python3
"""The voice-activity segmentation (kernels/vad.hip), tdt-ctc-110m shapes with synthetic weights.
  stage      the fourteen launches alone, HIP events around them (pk_vad_pcm_timed; input on the device, nothing read back), on 64 clips of 10 s
             and on one clip of 60 minutes, with the bytes of PCM read per second next to a device-to-device copy of the same bytes
  one call   a synthetic hour that is half silence (bursts of 2 .. 20 s between pauses): Model.transcribe_pcm(vad=True) next to the plain call on
             the whole hour with attention context [128, 128], wall ms; and what uploading the pieces a second time costs (a host-to-device copy
             of their bytes)
Writes profiles/vad.md.
usage: python tools/bench_vad.py [--reps 5] [--minutes 60] [--headline-ms X] [--out profiles/vad.md]"""
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


def copy_rates(n_bytes, reps):
    """(device-to-device GB/s counting the bytes read, host-to-device GB/s from pageable memory) of n_bytes through the HIP runtime, HIP events, medians"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def ok(st):
        if st != 0:
            raise RuntimeError(f"HIP error {st}")
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    host = np.zeros(n_bytes // 4, np.float32)

    def timed(to, frm, kind):
        t = []
        for r in range(reps + 1):
            ok(hip.hipEventRecord(e0, None))
            ok(hip.hipMemcpyAsync(to, frm, C.c_size_t(n_bytes), kind, None))
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(0)
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if r:
                t.append(ms.value)
        return float(np.median(t))
    try:
        d2d = timed(dst, src, 3)
        h2d = timed(src, vp(host.ctypes.data), 1)
    finally:
        hip.hipFree(src)
        hip.hipFree(dst)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    return n_bytes / d2d / 1e6, n_bytes / h2d / 1e6


def sparse_hour(minutes, synth):
    """`minutes` of 16 kHz audio, half of it silence: bursts of 2 .. 20 s of synth_pcm, each followed by a pause of the same length"""
    sr, r = 16000, np.random.default_rng(5)
    base = synth.synth_pcm(1, 20 * sr, seed=9)[0]
    x = np.zeros(int(minutes * 60 * sr), np.float32)
    pos = 0
    while pos < x.size:
        n = int(r.uniform(2, 20) * sr)
        m = min(n, x.size - pos)
        x[pos:pos + m] = base[:m]
        pos += 2 * n
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--headline-ms", type=float, default=None, help="bench.py's headline step on the parent commit on this box, to set the stage next to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad.md"))
    a = ap.parse_args()
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    cfg = pk.make_110m_config()
    lines = ["# Voice-activity segmentation (kernels/vad.hip)", "",
             f"`python tools/bench_vad.py --reps {a.reps} --minutes {a.minutes:g}`: tdt-ctc-110m shapes, synthetic weights, TDT decoder; medians.", "",
             "## The stage alone", "",
             "| shape | PCM bytes | stage (ms) | PCM read (GB/s) | device-to-device copy of the same bytes, bytes read (GB/s) | stage / copy time |", "|---|---|---|---|---|---|"]
    batch = [synth.synth_pcm(1, 160000, seed=100 + i)[0] for i in range(64)]
    hour = sparse_hour(a.minutes, synth)
    stage_batch = None
    for name, clips in ((f"64 x 10 s", batch), (f"1 x {a.minutes:g} min", [hour])):
        nb = 4 * sum(c.size for c in clips)
        ms = capi.vad_timed(clips, reps=max(a.reps, 5))
        stage_batch = ms if stage_batch is None else stage_batch
        d2d, _ = copy_rates(nb, max(a.reps, 5))
        lines.append(f"| {name} | {nb} | {ms:.3f} | {nb / ms / 1e6:.0f} | " + f"{d2d:.0f} | {ms / (nb / d2d / 1e6):.1f}x |")
        print(lines[-1], flush=True)
    lines += ["", "The copy reads and writes every byte, the stage reads the PCM once and writes 6 bytes per 640 read; its fourteen launches and two memsets each "
              "pass over at most a few bytes per frame after the first, so the small shape is bound by the launches and not by the bytes."]
    if a.headline_ms:
        lines += ["", f"The stage on 64 x 10 s is {100 * stage_batch / a.headline_ms:.2f} % of the headline step of `bench.py` ({a.headline_ms:.2f} ms, "
                  "the parent commit on the same box)."]
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "w.safetensors")
        synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
        gm = capi.Model(wp, cfg, device=0)
        res, pieces = gm.transcribe_pcm([hour], vad=True)
        vad_ms = median_ms(lambda: gm.transcribe_pcm([hour], vad=True), a.reps)
        gm.set_attention_context(128, 128)
        plain_ms = median_ms(lambda: gm.transcribe_pcm([hour]), a.reps)
        gm.close()
    piece_bytes = 4 * sum(e - b for _, b, e in pieces)
    _, h2d = copy_rates(piece_bytes, max(a.reps, 5))
    lines += ["", "## One call on a sparse recording", "",
              f"{a.minutes:g} minutes, half of them silence (bursts of 2 .. 20 s, each followed by a pause of its length): {len(pieces)} pieces, "
              f"{piece_bytes / 4 / 16000:.0f} s of audio in them.", "",
              "| route | wall (ms) |", "|---|---|",
              f"| `transcribe_pcm(vad=True)`: VAD, plan, the pieces packed into full-attention batches | {vad_ms:.0f} |",
              f"| `transcribe_pcm` on the whole recording, attention context [128, 128] | {plain_ms:.0f} |", "",
              f"The pieces route uploads its samples a second time: {piece_bytes} bytes, "
              f"{piece_bytes / h2d / 1e6:.1f} ms as one host-to-device copy from pageable memory at {h2d:.1f} GB/s, "
              f"{100 * piece_bytes / h2d / 1e6 / vad_ms:.1f} % of the call.  A device-side gather out of the VAD's staging buffer would remove it."]
    for ln in lines[-6:]:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
