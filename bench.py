#!/usr/bin/env python3
"""bench.py -- RTFx of the Parakeet hot path (mel -> FastConformer encoder -> TDT greedy decode) on MI355X.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line (metric, value, unit, ms_per_step, ...).  --full adds
what the headline figure does not need, after the timed steps: the sustained windows, the stage split and per-kernel timing with
the roofline of the dominant kernel, the parity of the timed batch against the CPU oracle with the CPU baselines, and the secondary
configurations (`also`).  --dump-outputs DIR writes what the last timed step computed (token ids, lengths, frames, confidences,
margins, as a caller of pk_batch_run reads them back) as DIR/<name>.npy in float32 / float64; the inputs are seeded, so two builds
can be compared output for output.

One "step" = one batch of 64 synthetic 10 s / 16 kHz clips (BASELINE.json configs[1]: tdt-ctc-110m, batch 64 x 10 s,
TDT decode, fp32), PCM already resident in HBM, through the C ABI (libparakeet_amd.so).  value = total audio seconds
of all ranks / wall seconds (max over ranks).  N > 1: one process per GPU, the batch dimension is sharded -- utterances are
independent, there is no collective on the data path (weak scaling); the barrier and the max-reduce of the wall time are RCCL
(torch.distributed backend "nccl").  `python bench.py --gpus N` on its own SPAWNS its ranks (re-executes itself under
`python -m torch.distributed.run --nproc-per-node N`, after checking that N devices are visible); under an external torchrun
(RANK / WORLD_SIZE set) it is a rank.  Random-init weights of the reference architecture (no checkpoints exist offline) ->
"data": "synthetic".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CLIP_SECONDS = 10.0
CLIP_SAMPLES = 160000
BATCH = 64
ENCODER_FLOP_PER_CLIP = 28.23e9        # 14.11 GMAC per 10 s clip, tdt-ctc-110m
PEAK_F32_MFMA_TFLOPS = 157.3           # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)
D_MODEL, FFN, ENC_FRAMES = 512, 2048, 126
FC1_KERNEL = {False: "gemm_pipe_kernel<4,2,1,2,32,EPI_SILU,1> (ffn_fc1_silu: fp32 v_mfma_f32_32x32x2_f32, 128x128 tile, 8 waves of 32x64, 1 LDS staging buffer, 4-byte staging stores)",
              True: "gemm_bf16_glds_kernel<4,2,2,4,EPI_SILU> (ffn_fc1_silu: v_mfma_f32_32x32x16_bf16 with swapped operands, 256x256 macro tile, 8 waves of 64x128, global_load_lds_dwordx4 staging into an XOR-swizzled LDS image, persistent one workgroup per CU, epilogue from registers into the blocked fc1 -> fc2 layout)"}
# committed rocprofv3 --pmc summaries (HBM bytes per launch of the dominant kernel), newest first, per (config, bf16)
PMC_FILES = {("tdt-600m", True): ("r06_m2_pmc_hbm_600m_bf16.json", "r05_m6_pmc_hbm_600m_bf16.json", "r05_m4_pmc_hbm_600m_bf16.json", "r05_m3_pmc_hbm_600m_bf16.json", "r05_m2_pmc_hbm_600m_bf16.json", "r05_m1_pmc_hbm_600m_bf16.json", "r04_m5_pmc_hbm_600m_bf16.json", "r04_m4_pmc_hbm_600m_bf16.json", "r04_m3_pmc_hbm_600m_bf16.json", "r04_m2_pmc_hbm_600m_bf16.json", "r04_m1_pmc_hbm_600m_bf16.json", "r03_m4_pmc_hbm_600m_bf16.json", "r03_m2_pmc_hbm_600m_bf16.json", "r03_m1_pmc_hbm_600m_bf16.json", "r02_pmc_hbm_600m_bf16.json"),
             ("tdt-ctc-110m", False): ("r06_m2_pmc_hbm.json", "r05_m6_pmc_hbm.json", "r05_m4_pmc_hbm.json", "r05_m3_pmc_hbm.json", "r05_m2_pmc_hbm.json", "r05_m1_pmc_hbm.json", "r04_m5_pmc_hbm.json", "r04_m4_pmc_hbm.json", "r04_m3_pmc_hbm.json", "r04_m2_pmc_hbm.json", "r04_m1_pmc_hbm.json", "r03_m4_pmc_hbm.json", "r03_m2_pmc_hbm.json", "r03_m1_pmc_hbm.json", "r02_pmc_hbm_v4.json", "r02_pmc_hbm_v3.json", "r02_pmc_hbm_v2.json", "r02_pmc_hbm.json", "r01_pmc_hbm.json")}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def weights_file(cfg, seed=42):
    """Seeded synthetic safetensors with the reference's tensor names; generated once per box."""
    import pkload
    pkload.load()
    from parakeet_cpp_amd import synth
    path = os.path.join(os.environ.get("PK_BENCH_CACHE", "/tmp"), f"pk_bench_{cfg.name}_seed{seed}.safetensors")
    if not os.path.exists(path):
        t = time.time()
        W = synth.synth_weights(cfg, seed=seed)
        tmp = path + f".{os.getpid()}.tmp"
        synth.save_weights(tmp, W)
        os.replace(tmp, path)
        log(f"[bench] generated {path} in {time.time() - t:.1f}s")
        return path, W
    return path, None


def cpu_port(cfg, weights, pcm_all, threads, budget_s=10.0, single_thread_sample=2):
    """The CPU oracle (oracle/libpk_oracle.so: a C restatement of the reference algorithm, AVX2 + OpenMP over clips) on ALL clips
    of the timed batch: it is the parity checker of the timed configuration and the `port` CPU figure."""
    import numpy as np
    import oracle
    oracle.set_threads(threads)
    om = oracle.Model(cfg, weights)
    nm = cfg.mel_bins
    om.tdt_greedy(om.encoder(np.stack([oracle.mel(pcm_all[0][:32000], n_mels=nm)])))     # warm the lazily built weight transposes (untimed)
    t_mel = t_enc = t_tdt = 0.0
    ids, n = [], len(pcm_all)
    chunk = 16
    for c0 in range(0, n, chunk):
        pcm = pcm_all[c0:c0 + chunk]
        t0 = time.time()
        feats = np.stack([oracle.mel(p, n_mels=nm) for p in pcm])
        t1 = time.time()
        enc = om.encoder(feats)
        t2 = time.time()
        r = om.tdt_greedy(enc)
        t3 = time.time()
        t_mel += t1 - t0; t_enc += t2 - t1; t_tdt += t3 - t2
        ids += [r["ids"][b, :r["lens"][b]].tolist() for b in range(len(pcm))]
    wall = t_mel + t_enc + t_tdt
    single = None
    try:                                   # the reference's own sources are single-threaded: same path, ONE thread, 2 clips
        if single_thread_sample > 0:
            oracle.set_threads(1)
            t0 = time.time()
            r1 = om.tdt_greedy(om.encoder(np.stack([oracle.mel(p, n_mels=nm) for p in pcm_all[:single_thread_sample]])))
            w1 = time.time() - t0
            single = {"value": round(single_thread_sample * CLIP_SECONDS / w1, 3), "cores": 1, "sample": f"{single_thread_sample} of the same clips, {w1:.1f} s"}
    finally:
        oracle.set_threads(threads)
    rep = {"value": round(n * CLIP_SECONDS / wall, 3), "unit": "RTFx (audio-s / wall-s)", "cores": threads, "kind": "port",
           "sample": f"{'all ' if n == BATCH else 'the first '}{n} clip(s) of rank 0's timed batch, mel+encoder+TDT, {wall:.1f} s of CPU work on oracle/libpk_oracle.so",
           "seconds": {"mel": round(t_mel, 3), "encoder": round(t_enc, 3), "tdt": round(t_tdt, 3)}, "single_thread": single}
    return rep, ids


def cpu_reference(cfg, wpath, pcm_all, threads, budget_s=14.0):
    """The REFERENCE'S OWN CODE on this host: parakeet::Transcriber::transcribe (include/parakeet/transcribe.hpp:99-179; mel, encoder,
    TDT greedy, detokenise) from oracle/_ref/libpk_ref_model.so = the reference sources compiled where they lie on the CPU stand-in
    for the un-vendored axiom tensor library (oracle/axiom_stub/: plain fp32 loops, OpenMP).  Bounded sample: clips of the timed
    batch, one call per clip (the reference API is single-utterance), until ~budget_s seconds of CPU work."""
    import refmodel
    import oracle
    from parakeet_cpp_amd import synth
    if not refmodel.available():
        return None, []
    oracle.set_threads(threads)            # one libgomp: the same thread count applies to the stand-in's OpenMP loops
    vpath = os.path.join(os.environ.get("PK_BENCH_CACHE", "/tmp"), f"pk_bench_{cfg.name}_vocab.txt")
    if not os.path.exists(vpath):
        synth.save_vocab(vpath, synth.synth_vocab(cfg.vocab_size - 1))
    tr = refmodel.Transcriber(cfg, wpath, vpath)
    tr.transcribe(pcm_all[0][:32000], "tdt")                            # first-touch of the weights, untimed
    ids, wall = [], 0.0
    for p in pcm_all:
        t0 = time.time()
        r = tr.transcribe(p, "tdt")
        wall += time.time() - t0
        ids.append(r["token_ids"].tolist())
        if wall >= budget_s:
            break
    n = len(ids)
    rep = {"value": round(n * CLIP_SECONDS / wall, 3), "unit": "RTFx (audio-s / wall-s)", "cores": threads, "kind": "reference",
           "sample": f"the first {n} clips of rank 0's timed batch through parakeet::Transcriber::transcribe (TDT), one call per clip, "
                     f"{wall:.1f} s of CPU work on oracle/_ref/libpk_ref_model.so (reference sources on the axiom CPU stand-in)"}
    return rep, ids


def cpu_torch(cfg, weights, pcm_all, gpu_ids, threads, n_clips=8, n_decode=1):
    """SURVEY.md 8(d) / BASELINE.md section 3: the torch-CPU (MKL) restatement of the same path -- tests/torch_ref.py, written after the
    reference author's own scripts/compare_encoder.py and compare_features.py -- on this host's cores: mel + encoder of `n_clips` clips of
    the timed batch as ONE batched call, then its TDT loop (one utterance at a time, a Python loop over torch GEMVs) on `n_decode` of them.
    torch picks its own summation orders, so it agrees with the oracle to fp32 round-off, not bit for bit: the decoded ids are compared
    with the GPU's and the agreement is reported, not asserted."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch_ref
    import oracle
    torch.set_num_threads(threads)
    n = min(n_clips, len(pcm_all))
    fb = oracle.mel_filterbank(n_mels=cfg.mel_bins)
    torch_ref.encoder(weights, cfg, torch_ref.mel_features(pcm_all[0][:32000], fb, n_mels=cfg.mel_bins, window_centered=False)[0][None])   # first touch, untimed
    t0 = time.time()
    feats = np.stack([torch_ref.mel_features(p, fb, n_mels=cfg.mel_bins, window_centered=False)[0] for p in pcm_all[:n]])
    t1 = time.time()
    enc = torch_ref.encoder(weights, cfg, feats)
    t2 = time.time()
    same = 0
    for b, ids_b in enumerate(torch_ref.tdt_greedy(weights, cfg, enc[:min(n_decode, n)])):
        same += int(list(ids_b) == list(gpu_ids[b]))
    t3 = time.time()
    nd = min(n_decode, n)
    # value = mel + encoder (the 99 % of the path's arithmetic, on MKL); the TDT loop of this restatement is a Python loop over torch GEMVs --
    # its time measures the interpreter, so it is reported beside the value (tdt_per_clip), not inside it
    return {"value": round(n * CLIP_SECONDS / (t2 - t0), 2), "unit": "RTFx (audio-s / wall-s), mel + encoder", "cores": threads,
            "kind": "port (torch-CPU / MKL restatement, tests/torch_ref.py)",
            "sample": f"mel + encoder of the first {n} clips of rank 0's timed batch as one batched torch call ({t2 - t0:.1f} s); its TDT loop on {nd} of them took {t3 - t2:.1f} s",
            "seconds": {"mel": round(t1 - t0, 3), "encoder": round(t2 - t1, 3), "tdt_per_clip": round((t3 - t2) / max(nd, 1), 3)},
            "token_ids_equal_gpu": f"{same} of {nd} decoded clips (fp32 round-off class vs the bit contract: reported, not asserted)"}


DEFAULT_OVERLAP = {}            # (config, bf16) -> pk_batch_set_decode_overlap default; filled from the measurements in DESIGN.md section 5
MARGIN_TOL_BF16 = 2e-2          # label log-prob error class of the bf16 mode at depth 24 (tests/test_gpu_600m_depth.py states the same bound)


LOGP_TOL_BF16 = 3e-2            # max |log-prob(gpu) - log-prob(bf16 oracle)| along the oracle's decision path (tests/test_gpu_600m_depth.py states the same bound)


def teacher_forced_parity(args, cfg, n, score_fn):
    """bf16 mode at the LOGITS: the GPU walks the bf16 oracle's decision path of the fixture's clips (pk_tdt_score; the loop of the reference's
    src/tdt.cpp:62-106 with the decisions given) and every step's label / duration log-probs are compared with the oracle's."""
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", "tdt600m_depth24_score_seed42.npz")
    if not os.path.exists(path):
        return None
    s = np.load(path, allow_pickle=False)
    worst, tot, cnt, flips, steps = 0.0, 0.0, 0, 0, 0
    for b in range(min(n, int(s["n_clips"]))):
        k = int(s["bf16_n"][b])
        r = score_fn(b, s["bf16_labels"][b, :k], s["bf16_dur_idx"][b, :k])
        if r["n"] != k:
            return {"error": f"clip {b}: {r['n']} steps walked, the oracle's path has {k}"}
        top = np.take_along_axis(r["label_lp"], s["bf16_top_ids"][b, :k].astype(np.int64), axis=1)
        d = np.concatenate([np.abs(top - s["bf16_top_lp"][b, :k]).ravel(), np.abs(r["dur_lp"] - s["bf16_dur_lp"][b, :k]).ravel()])
        worst, tot, cnt = max(worst, float(d.max())), tot + float(d.sum()), cnt + d.size
        flips += int((r["label_lp"].argmax(axis=1) != s["bf16_labels"][b, :k]).sum() + (r["dur_lp"].argmax(axis=1) != s["bf16_dur_idx"][b, :k]).sum())
        steps += k
    vs_fp32 = None
    if "bf16_on_fp32_top_lp" in s.files:
        # against the REFERENCE's arithmetic: the same bf16 GPU model along the FP32 oracle's path, next to the bf16 oracle's own distance from fp32
        gd, od = [], []
        for b in range(min(n, int(s["n_clips"]))):
            k = int(s["fp32_n"][b])
            r = score_fn(b, s["fp32_labels"][b, :k], s["fp32_dur_idx"][b, :k])
            if r["n"] != k:
                return {"error": f"clip {b}: {r['n']} steps walked, the fp32 oracle's path has {k}"}
            top = np.take_along_axis(r["label_lp"], s["fp32_top_ids"][b, :k].astype(np.int64), axis=1)
            gd += [np.abs(top - s["fp32_top_lp"][b, :k]).ravel(), np.abs(r["dur_lp"] - s["fp32_dur_lp"][b, :k]).ravel()]
            od += [np.abs(s["bf16_on_fp32_top_lp"][b, :k] - s["fp32_top_lp"][b, :k]).ravel(), np.abs(s["bf16_on_fp32_dur_lp"][b, :k] - s["fp32_dur_lp"][b, :k]).ravel()]
        gd, od = np.concatenate(gd), np.concatenate(od)
        vs_fp32 = {"gpu_bf16_vs_fp32_oracle": {"max_abs_dlogp": round(float(gd.max()), 5), "mean_abs_dlogp": round(float(gd.mean()), 6)},
                   "oracle_bf16_vs_fp32_oracle": {"max_abs_dlogp": round(float(od.max()), 5), "mean_abs_dlogp": round(float(od.mean()), 6)},
                   "ratio_max": round(float(gd.max() / od.max()), 3), "ratio_mean": round(float(gd.mean() / od.mean()), 3), "ratio_bound": 1.25,
                   "what": "along the FP32 oracle's path (the reference's arithmetic): |log-prob(bf16 GPU) - log-prob(fp32 oracle)| next to the bf16-mode "
                           "oracle's own distance on the same path; tests/test_gpu_600m_depth.py asserts the ratio bound"}
    return {"clips": min(n, int(s["n_clips"])), "steps": steps, "max_abs_dlogp": round(worst, 5), "mean_abs_dlogp": round(tot / max(1, cnt), 6),
            "bound": LOGP_TOL_BF16, "argmax_flips_along_path": flips, "decisions": 2 * steps, "vs_fp32_reference_path": vs_fp32,
            "what": "pk_tdt_score along the bf16 oracle's greedy path (every step's label and duration given): |delta log-prob| on the oracle's top-8 "
                    "labels and all duration log-probs of every step, encoder drift included",
            "fixture": "tests/golden/tdt600m_depth24_score_seed42.npz (tools/make_golden_600m_score.py)"}


def fixture_parity(args, cfg, pcm, gpu_ids, gpu_frames=None, model_score=None):
    """Parity of a tdt-600m run against the committed full-depth fixture.  fp32: token ids identical.  bf16: the tolerance statement for
    a greedy decode -- the GPU's tokens may leave the bf16 oracle's only at a decision whose top-1 / top-2 margin is within the mode's error
    (oracle/tolerance.py).  Returns (report, failed)."""
    import numpy as np
    from tolerance import first_divergence
    path = os.path.join(ROOT, "tests", "golden", "tdt600m_depth24_seed42.npz")
    if args.config != "tdt-600m" or not os.path.exists(path):
        return {"clips": 0, "checked_against": None, "note": "no full-depth fixture for this configuration"}, False
    g = np.load(path, allow_pickle=False)
    n = min(int(g["n_clips"]), len(gpu_ids))
    if not np.array_equal(np.asarray(pcm[:n], np.float64).sum(axis=1), g["pcm_digest"][:n]):
        return {"clips": 0, "error": "the batch's first clips are not the fixture's clips"}, True
    rep = {"clips": n, "fixture": "tests/golden/tdt600m_depth24_seed42.npz (24-layer oracle + reference-code outputs, tools/make_golden_600m.py)"}
    if not args.bf16:
        bad = [b for b in range(n) if gpu_ids[b] != g["fp32_ids"][b, :int(g["fp32_lens"][b])].tolist()]
        rep.update(token_mismatches=len(bad), tokens=int(g["fp32_lens"][:n].sum()),
                   checked_against="the fp32 oracle's token ids (bit contract) -- identical to the reference code's tdt_greedy_decode: "
                                   + str(bool(g["ref_ids_equal_oracle"].all()) if "ref_ids_equal_oracle" in g.files else None))
        return rep, bool(bad)
    per, failed = [], False
    for b in range(n):
        at, mg = first_divergence(gpu_ids[b], g["bf16_step_label"][b], g["bf16_step_margin"][b], cfg.blank_id,
                                  got_frames=(gpu_frames[0][b], gpu_frames[1][b]) if gpu_frames else None,
                                  oracle_frames=(g["bf16_start"][b], g["bf16_end"][b]))
        per.append({"clip": b, "gpu_tokens": len(gpu_ids[b]), "oracle_tokens": int(g["bf16_lens"][b]), "first_differing_token": at,
                    "oracle_margin_there": (None if mg is None else round(mg, 6))})
        if at is not None and mg > MARGIN_TOL_BF16:
            failed = True
    rep["teacher_forced"] = teacher_forced_parity(args, cfg, n, model_score) if model_score is not None else None
    if rep["teacher_forced"] and rep["teacher_forced"].get("max_abs_dlogp", 0.0) > LOGP_TOL_BF16:
        failed = True
    rep.update(per_clip=per, margin_tolerance=MARGIN_TOL_BF16,
               checked_against="the bf16-mode oracle's decode: tokens identical up to the first decision whose top-1/top-2 margin is within "
                               "the mode's error (random-weight models decide with margins down to 5e-5; see tests/test_gpu_600m_depth.py)")
    return rep, failed


def run_json(cmd, timeout_s):
    """one child process, its last stdout line parsed as JSON; errors come back as {"error": ...}"""
    import subprocess
    t0 = time.time()
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout_s, cwd=ROOT,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))
        lines = [ln for ln in p.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
        if not lines:
            return {"error": f"rc {p.returncode}, no JSON line", "stderr_tail": p.stderr.decode(errors="replace")[-400:], "seconds": round(time.time() - t0, 1)}
        d = json.loads(lines[-1])
        d["rc"], d["seconds"] = p.returncode, round(time.time() - t0, 1)
        return d
    except subprocess.TimeoutExpired:
        return {"error": f"timeout after {timeout_s} s"}
    except Exception as e:                      # noqa: BLE001  (report, never raise: the headline line must come out)
        return {"error": repr(e)}


def also_measurements(model, capi, synth, np):
    """The `also` array of the default line (outside `value`).  (a) BASELINE configs[2]: tdt-600m, 32 x 30 s, bf16 mode -- ms per step, the
    full-depth fixture parity (token contract + teacher-forced log-probs) and its roofline; (b) configs[4]: nemotron-600m streaming, 16
    lock-step streams, median ms per 160 ms chunk; (c) the headline configuration fed from HOST memory with distinct clips, uploads inside
    the clock (pk_transcribe_pcm: packing, PCIe, pipeline, results); (d) mixed-length batches (tools/bench_mixed.py)."""
    also = []
    # (c) first: it reuses the headline's resident model
    try:
        n_clips = 256
        pcm = synth.synth_pcm(n_clips, CLIP_SAMPLES, seed=777)
        clips = [pcm[i] for i in range(n_clips)]
        model.transcribe_pcm(clips[:64], decoder="tdt")                       # the pipeline's buffers exist after this
        packed = (pcm.reshape(-1), np.arange(n_clips + 1, dtype=np.int64) * CLIP_SAMPLES)      # the C ABI's input form: pcm + offsets
        best = 1e9
        for _ in range(2):
            t0 = time.perf_counter()
            res = model.transcribe_pcm(packed, decoder="tdt")
            best = min(best, time.perf_counter() - t0)
        also.append({"name": "pcie_inclusive", "workload": f"tdt-ctc-110m fp32, {n_clips} DISTINCT 10 s clips from host memory through pk_transcribe_pcm "
                     "(sort, pack into batches of <= 256 clips and <= 8192 encoder rows -- 65 / 65 / 65 / 61 clips here --, PCIe upload of batch k+1 under encoder k, TDT decode groups, "
                     "results copied back): uploads inside the clock",
                     "wall_s": round(best, 4), "rtfx": round(n_clips * CLIP_SECONDS / best, 1), "ms_per_64_clips_equivalent": round(best / (n_clips / 64) * 1e3, 3),
                     "tokens": int(sum(len(r["token_ids"]) for r in res))})
    except Exception as e:                      # noqa: BLE001
        also.append({"name": "pcie_inclusive", "error": repr(e)})
    py = sys.executable
    d = run_json([py, os.path.join(ROOT, "tools", "bench_mixed.py"), "--steps", "10", "--warmup", "3", "--clips", "256", "--oracle-sample", "2"], 240)
    also.append(dict({"name": "mixed_length (reference roadmap: batch inference, README.md:513 -- packed, no padding)"}, **d))
    d = run_json([py, os.path.abspath(__file__), "--config", "tdt-600m", "--bf16", "--steps", "10", "--warmup", "3", "--sustain-seconds", "0", "--no-also",
                  "--full"], 420)
    for k in ("kernels", "ms_per_step_per_rank", "collective_ranks", "collective_backend", "sustained"):
        d.pop(k, None)
    also.append(dict({"name": "configs[2] tdt-600m 32x30s bf16"}, **d))
    d = run_json([py, os.path.join(ROOT, "tools", "bench_stream.py"), "--chunks", "100", "--warmup", "10"], 300)
    also.append(dict({"name": "configs[4] nemotron-600m streaming, 16 streams/GPU"}, **d))
    d = run_json([py, os.path.join(ROOT, "tools", "bench_stream.py"), "--chunks", "100", "--warmup", "10", "--bf16"], 300)
    also.append(dict({"name": "configs[4] nemotron-600m streaming, 16 streams/GPU, tolerance-class mode (bf16 operands: kernels/gemm_smallm_bf16.hip)"}, **d))
    return also


def last_step_outputs(L, capi, batch, n_cap, dec):
    """What the last timed step computed, as a caller of pk_batch_run reads it back (pk_batch_results_back(0) after pk_batch_sync):
    token ids, start / end frames and confidences [clips][max_tokens] (-1 / 0 past each clip's length), lengths [clips] and, for TDT,
    the smallest top-1 / top-2 label log-prob margin of every clip.  Integers are stored as float64 (exact)."""
    import ctypes as C
    import numpy as np
    mt = L.pk_batch_max_tokens(batch)
    ids = np.zeros((n_cap, mt), np.int32); st = np.zeros((n_cap, mt), np.int32); en = np.zeros((n_cap, mt), np.int32)
    cf = np.zeros((n_cap, mt), np.float32); lens = np.zeros(n_cap, np.int32); n = C.c_int(0)
    capi.check(L.pk_batch_results_back(batch, 0, C.byref(n), ids.ctypes.data_as(capi.i32p), lens.ctypes.data_as(capi.i32p),
                                       st.ctypes.data_as(capi.i32p), en.ctypes.data_as(capi.i32p), cf.ctypes.data_as(capi.f32p)))
    B = n.value
    past = np.arange(mt)[None, :] >= np.maximum(lens[:B], 0)[:, None]
    out = {"token_ids": np.where(past, -1, ids[:B]).astype(np.float64), "token_lens": lens[:B].astype(np.float64),
           "token_start_frames": np.where(past, -1, st[:B]).astype(np.float64), "token_end_frames": np.where(past, -1, en[:B]).astype(np.float64),
           "token_confidence": np.where(past, 0.0, cf[:B]).astype(np.float32)}
    if dec == 1:
        mg = np.zeros(n_cap, np.float32)
        if L.pk_batch_margins(batch, 0, mg.ctypes.data_as(capi.f32p)) == 0:
            out["min_top1_top2_margin"] = mg[:B].copy()
    return out


def dump_outputs(dirname, outputs, rank, world):
    """--dump-outputs: one DIR/<name>.npy per array (DIR/<name>_rank<r>.npy when several ranks run)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = sum(a.nbytes for a in outputs.values())
    if total > 64 << 20:
        raise SystemExit(f"bench.py --dump-outputs: {total} bytes of outputs exceed the 64 MB bound")
    for name, a in outputs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dirname, f"{name}_rank{rank}.npy" if world > 1 else f"{name}.npy"), a)
    log(f"[bench] wrote {len(outputs)} arrays ({total} bytes) of the last timed step to {dirname}")


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_ranks(args):
    """--gpus N > 1 without a launcher: become the launcher.  One process per GPU under torch.distributed.run, rendezvous on 127.0.0.1."""
    import subprocess
    if not args.rendezvous_only:
        import pkload
        pkload.load()
        from parakeet_cpp_amd import capi
        n = capi.device_count()
        if n < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {n} MI355X device(s) visible on this node -- refusing to report a "
                             f"{args.gpus}-GPU figure from fewer devices")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("[bench] spawning ranks:", " ".join(cmd))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def rendezvous_only(args, rank, world):
    """Launcher / collective plumbing without a GPU (tests/test_sharding_gloo.py): the ranks meet over gloo, run the SAME barrier +
    max-reduce + per-rank gather the timed path uses and rank 0 prints the line skeleton.  No throughput claim is made ("dry_run")."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1:
        dist.init_process_group(backend="gloo")
        dist.barrier()
    elapsed = 0.001 * (rank + 1) * args.steps
    per_rank = [elapsed]
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        allr = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allr, tt)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, per_rank = float(tt.item()), [float(x.item()) for x in allr]
    if rank == 0:
        print(json.dumps({"metric": "RTFx (dry run: launcher and collectives only)", "value": None, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "dry_run": True, "backend": "gloo",
                          "ms_per_step_per_rank": [round(x / args.steps * 1e3, 3) for x in per_rank], "collective_ranks": world}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH, help="clips per step per GPU (BASELINE: 64)")
    ap.add_argument("--decoder", default="tdt", choices=["tdt", "ctc"])
    ap.add_argument("--config", default="tdt-ctc-110m", choices=["tdt-ctc-110m", "tdt-600m"],
                    help="tdt-ctc-110m = BASELINE configs[1] (the headline metric); tdt-600m = configs[2] shapes (32 x 30 s), run in fp32")
    ap.add_argument("--bf16", action="store_true", help="pk_config.gemm_bf16: encoder products on bf16 operands / fp32 accumulation "
                    "(the precision BASELINE configs[2] names); the headline metric stays fp32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--decode-group", type=int, default=int(os.environ.get("PK_BENCH_DECODE_GROUP", "-1")),
                    help="pk_batch_set_decode_group: TDT loops of this many consecutive steps decoded as one lock-step batch (1 = per step); "
                         "-1 = the configuration's default (4 for tdt-ctc-110m, 16 for tdt-600m: profiles/r03_decode_overlap_ab.txt)")
    ap.add_argument("--decode-loop", default="phases", choices=["phases", "persistent", "graph"],
                    help="pk_model_set_decode_loop: launch structure of the greedy loop (identical results)")
    ap.add_argument("--decode-overlap", type=int, default=-1, choices=[-1, 0, 1],
                    help="pk_batch_set_decode_overlap: 1 = decode under the next encoder on a second stream, 0 = on the encoder's stream after it; "
                         "-1 = the configuration's default (1 for tdt-ctc-110m)")
    ap.add_argument("--sustain-seconds", type=float, default=3.0,
                    help="with --full, after the timed K steps: keep stepping in windows of K for about this long and report the median window (0 = skip)")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the secondary configurations (`also`) the N = 1 headline run appends "
                    "after its own timed region: configs[2] tdt-600m bf16, configs[4] streaming, mixed-length batches, the PCIe-inclusive rate")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure and check what the headline figure does not need: "
                    "sustained windows, stage split, per-kernel timing and roofline, parity against the CPU oracle, CPU baselines, `also`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--rendezvous-only", action="store_true", help="launcher + collective plumbing over gloo without a GPU (CPU test hook)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)
    global CLIP_SECONDS, CLIP_SAMPLES, ENCODER_FLOP_PER_CLIP, D_MODEL, FFN, ENC_FRAMES
    exit_code = [0]
    big = args.config == "tdt-600m"
    if big:                                  # 470.9 GFLOP per 30 s clip
        CLIP_SECONDS, CLIP_SAMPLES, ENCODER_FLOP_PER_CLIP = 30.0, 480000, 470.9e9
        D_MODEL, FFN, ENC_FRAMES = 1024, 4096, 376
        if args.batch == BATCH:
            args.batch = 32

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    use_dist = "WORLD_SIZE" in os.environ          # under a launcher the collectives run even at world size 1 (same code path as at 8)
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE): the two must agree")
    n_gpus = world
    if args.rendezvous_only:
        return rendezvous_only(args, rank, world)

    import numpy as np
    import torch
    import torch.distributed as dist
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import capi, synth

    if not torch.cuda.is_available() or capi.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: the product has no CPU path")
    if capi.device_count() <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} wants device {local_rank}, {capi.device_count()} visible")
    torch.cuda.set_device(local_rank)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    cfg = pk.make_tdt_600m_config() if big else pk.make_110m_config()
    if args.bf16:
        import dataclasses
        cfg = dataclasses.replace(cfg, gemm_bf16=True)
    W = None
    if local_rank == 0:
        wpath, W = weights_file(cfg)
    barrier()
    if local_rank != 0:
        wpath, _ = weights_file(cfg)

    model = capi.Model(wpath, cfg, device=local_rank)
    model.set_decode_loop(args.decode_loop)
    L = capi.lib()
    import ctypes as C
    batch = C.c_void_p()
    capi.check(L.pk_batch_create(model._h, args.batch, CLIP_SAMPLES, C.byref(batch)))
    # every rank gets its own shard of synthetic clips (seeded by rank): utterance-batch data parallelism
    pcm = synth.synth_pcm(args.batch, CLIP_SAMPLES, seed=1234 + rank)
    capi.check(L.pk_batch_upload(batch, pcm.ctypes.data_as(capi.f32p), args.batch))
    dec = 1 if args.decoder == "tdt" else 0
    if args.decode_group < 0:
        args.decode_group = 16 if big else 4
    group = max(1, args.decode_group) if dec == 1 else 1
    if group > 1:
        capi.check(L.pk_batch_set_decode_group(batch, group))
    overlap = DEFAULT_OVERLAP.get((args.config, bool(args.bf16)), 1) if args.decode_overlap < 0 else args.decode_overlap
    capi.check(L.pk_batch_set_decode_overlap(batch, overlap))

    for _ in range(args.warmup):
        capi.check(L.pk_batch_run(batch, dec))
    capi.check(L.pk_batch_sync(batch))
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        capi.check(L.pk_batch_run(batch, dec))
    capi.check(L.pk_batch_sync(batch))
    barrier()
    elapsed = time.perf_counter() - t0
    # the token ids the TIMED steps produced (the runs of the last decode group), before the untimed profiling passes below
    timed_ids, timed_margin = [], float("inf")
    if dec == 1:
        mt_ = L.pk_batch_max_tokens(batch)
        for back in range(L.pk_batch_results_available(batch)):
            ids_ = np.zeros((args.batch, mt_), np.int32); lens_ = np.zeros(args.batch, np.int32); n_ = C.c_int(0)
            capi.check(L.pk_batch_results_back(batch, back, C.byref(n_), ids_.ctypes.data_as(capi.i32p), lens_.ctypes.data_as(capi.i32p), None, None, None))
            timed_ids.append([ids_[b, :lens_[b]].tolist() for b in range(n_.value)])
            mg_ = np.zeros(args.batch, np.float32)
            if L.pk_batch_margins(batch, back, mg_.ctypes.data_as(capi.f32p)) == 0:
                timed_margin = min(timed_margin, float(mg_[:n_.value].min()))
    last = last_step_outputs(L, capi, batch, args.batch, dec)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, rank, world)
    per_rank_s = [elapsed]
    if use_dist:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        allr = torch.zeros(world, dtype=torch.float64, device="cuda")
        dist.all_gather_into_tensor(allr, tt)                          # RCCL: every rank's own wall time of the timed region
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, per_rank_s = float(tt.item()), [float(x) for x in allr.tolist()]

    sustained, kernels, ms = None, {}, None
    if args.full:
        # Sustained figure (NOT `value`): the timed region of 20 steps lasts ~0.4 s -- too short for the driver's GPU-busy sampling to see and
        # ~1 % above the steady state.  Keep stepping in windows of K steps for --sustain-seconds and report the median window.
        if args.sustain_seconds > 0:
            if group > 1:
                capi.check(L.pk_batch_set_decode_group(batch, group))
            wins, t_all = [], time.perf_counter()
            while time.perf_counter() - t_all < args.sustain_seconds and len(wins) < 64:
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    capi.check(L.pk_batch_run(batch, dec))
                capi.check(L.pk_batch_sync(batch))
                wins.append((time.perf_counter() - t1) / args.steps * 1e3)
            ws = sorted(wins)
            sustained = {"windows": len(wins), "steps_per_window": args.steps, "seconds": round(time.perf_counter() - t_all, 2),
                         "ms_per_step_median": round(ws[len(ws) // 2], 3), "ms_per_step_min": round(ws[0], 3), "ms_per_step_max": round(ws[-1], 3),
                         "rtfx_median": round(args.batch * CLIP_SECONDS / (ws[len(ws) // 2] * 1e-3), 1)}
            # the same protocol with decode_group = 1 (round-1 protocol: decode(k) under encoder(k+1)), for round-over-round comparison
            if group > 1:
                capi.check(L.pk_batch_set_decode_group(batch, 1))
                for _ in range(2):
                    capi.check(L.pk_batch_run(batch, dec))
                capi.check(L.pk_batch_sync(batch))
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    capi.check(L.pk_batch_run(batch, dec))
                capi.check(L.pk_batch_sync(batch))
                sustained["decode_group_1_ms_per_step"] = round((time.perf_counter() - t1) / args.steps * 1e3, 3)
            elif dec == 1:
                capi.check(L.pk_batch_set_decode_group(batch, 1))

        if dec == 1:
            capi.check(L.pk_batch_set_decode_group(batch, 1))            # the stage / kernel timers below run one un-pipelined step at a time
        # stage split + per-kernel timing of one extra (untimed) step, hipEvents on the library's own stream
        ms = (C.c_float * 4)()
        capi.check(L.pk_batch_run_timed(batch, dec, ms))
        # per-kernel HIP-event timing (events on the library's own stream around every launch): three extra, untimed steps, averaged
        kernels = {}
        N_PROF = 3
        for _ in range(N_PROF):
            stats = (capi.PkKernelStat * 64)()
            nk = L.pk_batch_profile(batch, dec, stats, 64)
            for i in range(max(0, min(nk, 64))):
                s_ = stats[i]
                k = kernels.setdefault(s_.name.decode(), {"launches": 0, "ms": 0.0, "gflop": 0.0, "mbytes": 0.0})
                k["launches"] += s_.launches; k["ms"] += s_.total_ms; k["gflop"] += s_.flops / 1e9; k["mbytes"] += s_.bytes / 1e6
        for k in kernels.values():                       # back to per-step figures
            k["launches"] //= N_PROF
            k["ms"] = round(k["ms"] / N_PROF, 4); k["gflop"] = round(k["gflop"] / N_PROF, 3); k["mbytes"] = round(k["mbytes"] / N_PROF, 3)
        mt = L.pk_batch_max_tokens(batch)
        ids = np.zeros((args.batch, mt), np.int32)
        lens = np.zeros(args.batch, np.int32)
        st_fr = np.zeros((args.batch, mt), np.int32); en_fr = np.zeros((args.batch, mt), np.int32)
        capi.check(L.pk_batch_results(batch, ids.ctypes.data_as(capi.i32p), lens.ctypes.data_as(capi.i32p), st_fr.ctypes.data_as(capi.i32p),
                                      en_fr.ctypes.data_as(capi.i32p), None))

    if rank == 0:
        audio_s = args.steps * args.batch * CLIP_SECONDS * n_gpus
        value = audio_s / elapsed
        # Roofline of the dominant kernel = the MFMA GEMM instantiation that runs ffn fc1 (+ SiLU epilogue).  Algorithmic FLOP per
        # launch = 2*M*N*K (M = batch*126 frames, N = 2048, K = 512; tdt-600m: M = batch*376, N = 4096, K = 1024); duration = the HIP-event
        # average over its launches measured above, in this run.  Peak by arithmetic type (MI355X_MICROARCH.md): fp32 MFMA 157.3 TF,
        # dense bf16 MFMA 2500 TF.
        peak = PEAK_BF16_MFMA_TFLOPS if args.bf16 else PEAK_F32_MFMA_TFLOPS
        dom = kernels.get("ffn_fc1_silu")           # --full only: empty otherwise
        roof = None
        if dom and dom["launches"]:
            per_launch_flop = dom["gflop"] * 1e9 / dom["launches"]
            per_launch_s = dom["ms"] * 1e-3 / dom["launches"]
            ach = per_launch_flop / per_launch_s / 1e12
            enc_gemms = ("sub_pw", "sub_proj", "ffn_fc1_silu", "ffn_fc2_resid", "attn_qkv", "attn_out_resid", "conv_pw1_glu", "conv_pw2_resid")
            g_fl = sum(kernels[k]["gflop"] for k in enc_gemms if k in kernels)
            g_ms = sum(kernels[k]["ms"] for k in enc_gemms if k in kernels)
            # HBM traffic of that kernel comes from a separate rocprofv3 --pmc pass (counters cannot be read inside this process):
            # the committed summary of the same configuration, labelled with its source; null when there is none for this config.
            traffic, traffic_src = None, None
            for name in PMC_FILES.get((args.config, bool(args.bf16)), ()):
                f = os.path.join(ROOT, "profiles", name)
                if os.path.exists(f):
                    try:
                        traffic = json.load(open(f)).get("ffn_fc1_silu_bytes_per_launch")
                        traffic_src = "profiles/" + name + " (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command)"
                    except Exception:
                        traffic = None
                    if traffic:
                        break
            roof = {"bound": "mfma", "kernel": FC1_KERNEL[bool(args.bf16)], "achieved": round(ach, 2),
                    "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": int((2 if args.bf16 else 4) * (args.batch * ENC_FRAMES * (D_MODEL + FFN) + FFN * D_MODEL)),   # bf16 mode: A, W and the fc1 output are bf16
                    "flop_per_launch": per_launch_flop, "us_per_launch": round(per_launch_s * 1e6, 2),
                    "encoder_gemms": {"tflops": round(g_fl / max(g_ms, 1e-9), 2), "gflop": round(g_fl, 1), "ms": round(g_ms, 3),
                                      "frac_of_peak": round(g_fl / max(g_ms, 1e-9) / peak, 4)}}
        out = {
            "metric": f"RTFx (audio-sec/wall-sec), mel+encoder+TDT decode, {args.config} {int(CLIP_SECONDS)}s@b{args.batch}",
            "value": round(value, 1), "unit": "x real-time", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16" if args.bf16 else "f32", "data": "synthetic",
            "config": {"workload": f"{args.config}, batch={args.batch}x{int(CLIP_SECONDS)}s clips per GPU, {args.decoder.upper()} greedy decode{' (the loops of %d consecutive steps driven as one lock-step batch)' % group if group > 1 else ''}, {'bf16 GEMM operands / fp32 accumulate' if args.bf16 else 'fp32'} "
                                   f"(BASELINE configs[{2 if big else 1}]{' shapes; BASELINE names bf16, this run is fp32' if (big and not args.bf16) else ''})",
                       "clips_per_step_per_gpu": args.batch, "clip_seconds": CLIP_SECONDS, "parallelism": f"dp{n_gpus} (utterance shards, no data-path collective)",
                       "decode_group": group, "decode_loop": args.decode_loop, "decode_overlap": overlap},
            "ms_per_step_per_rank": [round(x / args.steps * 1e3, 3) for x in per_rank_s],
            "collective_ranks": (dist.get_world_size() if use_dist else 1), "collective_backend": ("nccl (RCCL)" if use_dist else None),
            # smallest top-1 / top-2 label log-prob margin over every decision of the timed runs read back: how far the closest greedy
            # decision was from another token (the early warning of the tolerance-class bf16 mode)
            "min_top1_top2_margin": (round(timed_margin, 6) if timed_margin != float("inf") else None),
            "decode_tokens_per_clip": round(float(last["token_lens"].mean()), 1),      # the last timed step
        }
        if args.full:
            enc_ms = float(ms[1])
            out.update({
                "sustained": sustained,
                "encoder_ms_per_clip": round(enc_ms / args.batch, 4),
                "stage_ms": {"mel": round(float(ms[0]), 3), "encoder": round(enc_ms, 3), "decode": round(float(ms[2]), 3), "total": round(float(ms[3]), 3)},
                "encoder_tflops": round(ENCODER_FLOP_PER_CLIP * args.batch / (enc_ms * 1e-3) / 1e12, 2),
                "encoder_frac_of_mfma_peak": round(ENCODER_FLOP_PER_CLIP * args.batch / (enc_ms * 1e-3) / 1e12 / peak, 4),
                "roofline": roof,
                "kernels": kernels,
            })
        # Parity of the TIMED configuration + CPU baselines, on this box's host cores (rank 0, N = 1 only).  The oracle decodes
        # every clip of the timed batch (bit-exact contract: token ids must be identical); the reference's own Transcriber decodes a
        # bounded prefix of it.  A mismatch against the oracle fails the run.  --full only.
        rc = 0
        full_cpu = args.full and n_gpus == 1 and not args.no_cpu_baseline and args.decoder == "tdt"
        gpu_ids = [ids[b, :lens[b]].tolist() for b in range(args.batch)] if full_cpu else None
        threads = min(8, os.cpu_count() or 1)
        if full_cpu and (big or args.bf16):
            # configs[2] / the bf16 mode: the 24-layer oracle is too slow for the whole batch, so parity comes from the committed full-depth
            # fixture (tests/golden/tdt600m_depth24_seed42.npz = the oracle's and the reference code's outputs for the FIRST clips of exactly
            # this batch, tools/make_golden_600m.py) and the CPU baseline is the fp32 oracle timed live on ONE clip (~10 s of CPU work).
            try:
                score_fn = (lambda b, lab, dur: model.tdt_score(model.encode(model.mel(pcm[b:b + 1]))[0], lab, dur)) if (big and args.bf16) else None
                out["parity"], bad = fixture_parity(args, cfg, pcm, gpu_ids, (st_fr, en_fr), model_score=score_fn)
                if bad:
                    rc = 3
                if W is None:
                    from safetensors.numpy import load_file
                    W = load_file(wpath)
                import dataclasses as _dc
                port, port_ids = cpu_port(_dc.replace(cfg, gemm_bf16=False), W, pcm[:1], threads, single_thread_sample=0)
                if not args.bf16 and port_ids[0] != gpu_ids[0]:
                    out["parity"]["live_oracle_clip0_mismatch"] = True
                    rc = 3
                out["cpu_baseline"] = port
            except Exception as e:
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        elif full_cpu:
            try:
                if W is None:
                    W = synth.synth_weights(cfg, seed=42)
                port, port_ids = cpu_port(cfg, W, pcm, threads)
                bad = [b for b in range(args.batch) if gpu_ids[b] != port_ids[b]]
                parity = {"clips": args.batch, "token_mismatches": len(bad), "tokens": int(lens.sum()),
                          "checked_against": "oracle/libpk_oracle.so on every clip of the timed batch (token ids identical)"}
                # the runs of the timed region itself (decoded in groups) against the same oracle ids
                bad_t = sum(1 for run_ids in timed_ids for b in range(len(run_ids)) if run_ids[b] != port_ids[b])
                parity["timed_runs_checked"] = len(timed_ids)
                parity["timed_runs_token_mismatches"] = bad_t
                if bad or bad_t:
                    parity["mismatching_clips"] = bad[:8]
                    rc = 3
                ref, ref_ids = (None, [])
                try:
                    ref, ref_ids = cpu_reference(cfg, wpath, pcm, threads)
                except Exception as e:
                    ref = {"value": None, "kind": "reference", "error": repr(e)}
                if ref_ids:
                    rbad = [b for b in range(len(ref_ids)) if gpu_ids[b] != ref_ids[b]]
                    parity["reference_clips"] = len(ref_ids)
                    parity["reference_token_mismatches"] = len(rbad)
                    parity["reference_checked_against"] = "parakeet::Transcriber::transcribe of oracle/_ref/libpk_ref_model.so (the reference's own sources) on the batch prefix"
                out["parity"] = parity
                try:
                    tmkl = cpu_torch(cfg, W, pcm, gpu_ids, threads)
                except Exception as e:
                    tmkl = {"value": None, "kind": "port (torch-CPU / MKL restatement)", "error": repr(e)}
                # headline CPU figure: the reference's own code when the prebuilt library travelled, the ports next to it
                if ref and ref.get("value"):
                    out["cpu_baseline"] = dict(ref, port=port, torch_mkl=tmkl)
                else:
                    out["cpu_baseline"] = dict(port, reference=ref, torch_mkl=tmkl)
            except Exception as e:  # the baseline is a report, never a reason to lose the GPU line
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        # Secondary configurations, AFTER the headline's timed region and outside `value` (round-3 verdict: configs[2] and configs[4] were only
        # ever builder-run): each is one short, bounded measurement -- own process where it needs another model -- and a failure or timeout
        # is reported inside its entry, never at the expense of the headline line.
        if args.full and n_gpus == 1 and not args.no_also and args.config == "tdt-ctc-110m" and not args.bf16 and args.decoder == "tdt":
            out["also"] = also_measurements(model, capi, synth, np)
        print(json.dumps(out), flush=True)
        if rc:
            log(f"[bench] PARITY FAILURE: GPU token ids differ from the oracle on clips {out['parity'].get('mismatching_clips')}")
            exit_code[0] = rc

    L.pk_batch_free(batch)
    model.close()
    if use_dist:
        dist.destroy_process_group()
    if exit_code[0]:
        sys.exit(exit_code[0])


if __name__ == "__main__":
    main()
