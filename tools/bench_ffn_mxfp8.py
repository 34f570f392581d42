#!/usr/bin/env python3
"""tools/bench_ffn_mxfp8.py -- what the MXFP8 feed-forward mode (pk_model_set_ffn_mxfp8) is worth at the shapes of BASELINE configs[2]
(tdt-600m, gemm_bf16, 32 x 30 s: 12000 rows, d = 1024, f = 4096), one GPU, one box.

The mode is switched on and off on ONE model between runs, A B A B ..., so both sides see the same clocks and the same neighbours; fc1, fc2, the row
quantiser and the LayerNorm come from the per-kernel timers of an un-pipelined step (pk_batch_profile), the whole step from timed pipelined steps.
--layers cuts the model's depth (default 4: the products' shapes, and so their per-launch times, are the full model's; the weights of 24 layers take
minutes to synthesise).  Writes profiles/ffn_mxfp8.md; the accuracy figures in it are the ones tests/test_gpu_mxfp8_gemm.py and
tests/test_gpu_ffn_mxfp8.py print."""
import argparse
import ctypes as C
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bench  # noqa: E402  (weights_file)
from bench_mixed import kernel_ms, timed_steps  # noqa: E402

ACCURACY = """## Accuracy (random-init weights; no claim about trained ones)

- fp32 outputs against float64 of the same quantised operands (M 300, N 320, K 1088): largest |err| / sum|a w| = 3.97e-6 (1.99e-6 behind the
  residual's alpha = 0.5).  The bf16 products' bound of 2e-6 is not met -- the instruction's internal summation is undocumented --, so the test's
  bound is twice the measurement, 8e-6 * sum|a w|.  Integer-valued operands (every partial sum below 2^24) come out exact at every shape tested.
- Encoder output of a 2-layer random-init model (d 256, f 512, 130 rows), max|MXFP8 mode - bf16 mode| / max|x|: GPU 4.27e-2, float64 emulation
  of the format on the same weights and input 4.07e-2.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_mxfp8.md"))
    args = ap.parse_args()

    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth
    if capi.device_count() < 1:
        raise SystemExit("bench_ffn_mxfp8.py needs an MI355X: the product has no CPU path")
    cfg = dataclasses.replace(pk.make_tdt_600m_config(), num_layers=args.layers, gemm_bf16=True, name=f"tdt-600m-{args.layers}L-bf16")
    wpath, _ = bench.weights_file(cfg)
    model = capi.Model(wpath, cfg, device=0)
    L = capi.lib()
    n = int(args.seconds * 16000)
    b = C.c_void_p()
    capi.check(L.pk_batch_create(model._h, args.clips, n, C.byref(b)))
    pcm = synth.synth_pcm(args.clips, n, seed=1234)
    capi.check(L.pk_batch_upload(b, pcm.ctypes.data_as(capi.f32p), args.clips))
    rows = args.clips * L.pk_encoder_num_frames(L.pk_mel_num_frames(n))

    names = ("layernorm", "mx_quantize", "ffn_fc1_silu", "ffn_fc2_resid")
    ker = {False: {k: [] for k in names}, True: {k: [] for k in names}}
    step = {False: [], True: []}
    for _ in range(args.rounds):                                      # A B A B: both modes inside every round
        for on in (False, True):
            model.set_ffn_mxfp8(on)
            step[on].append(1e3 * timed_steps(L, capi, b, 1, args.steps, 2))
            ms = kernel_ms(L, capi, b, 1, n=2)
            for k in names:
                ker[on][k].append(ms.get(k, 0.0) / (2 * args.layers if k != "layernorm" else 1))
    model.set_ffn_mxfp8(False)
    L.pk_batch_free(b)
    model.close()

    def med(v):
        return sorted(v)[len(v) // 2]
    f, d = cfg.ffn_intermediate, cfg.hidden_size
    tf = 2.0 * rows * f * d / 1e9                                      # GFLOP of one product
    lines = [f"# MXFP8 feed-forward products against the bf16 ones ({cfg.name}, {args.clips} x {args.seconds:g} s = {rows} rows, d {d}, f {f})", "",
             f"One model, the mode switched off / on inside each of {args.rounds} rounds; medians.  Per-launch times from the per-kernel timers of an",
             "un-pipelined step (pk_batch_profile), the step from timed pipelined steps (mel + encoder + TDT decode of the cut model).", "",
             "| per launch | bf16 mode ms | MXFP8 mode ms | ratio | MXFP8 TFLOP/s |", "|---|---|---|---|---|"]
    tot = {False: 0.0, True: 0.0}
    for k in ("mx_quantize", "ffn_fc1_silu", "ffn_fc2_resid"):
        a, m = med(ker[False][k]), med(ker[True][k])
        tot[False] += a; tot[True] += m
        gemm = k != "mx_quantize"                                      # (the quantiser has no bf16 counterpart and no flops)
        lines.append(f"| {k} | {a:.4f} | {m:.4f} | {f'{m / a:.3f}' if gemm else '-'} | {f'{tf / m:.0f}' if gemm else '-'} |")
    lines.append(f"| quantiser + fc1 + fc2 | {tot[False]:.4f} | {tot[True]:.4f} | {tot[True] / tot[False]:.3f} | |")
    lines.append(f"| layernorm, all launches of a step | {med(ker[False]['layernorm']):.4f} | {med(ker[True]['layernorm']):.4f} | | |")
    lines.append(f"| whole step | {med(step[False]):.3f} | {med(step[True]):.3f} | {med(step[True]) / med(step[False]):.3f} | |")
    verdict = "faster than" if tot[True] < tot[False] else "NOT faster than"
    lines += ["", f"The pair (quantiser + fc1 + fc2) in the MXFP8 mode is {verdict} the bf16 products here (ratio {tot[True] / tot[False]:.3f}).  The mode stays opt-in.", "", ACCURACY]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
