"""The mel front end's specification in float64 (the header comment of csrc/kernels/mel.hip), with a per-element error bound for
an fp32 implementation of the same chain, the cases tests/test_mel_ref.py (CPU: the oracle) and tests/test_gpu_mel_forms.py (the kernels) share,
and the wrong variants ("mutants") that show the bound can tell a wrong front end from a right one.  Plain NumPy; nothing here is taken from
oracle/pk_oracle.c.

The chain (offline, preprocess_audio):
  y[0] = x[0], y[i] = x[i] - 0.97 x[i - 1]                        pre-emphasis
  frame t, tap k (0 .. 511) = y[reflect(160 t + k - 256)]           centred frames, the pre-emphasised signal reflect-padded by 256:
                                                                    reflect(j) = -j for j < 0, 2 (n - 1) - j for j >= n
  times the symmetric Hann(400), 0.5 - 0.5 cos(2 pi k / 399), at taps 0 .. 399 (switch A1 off) or 56 .. 455 (on), zero elsewhere
  X = rfft_512, P = |X|^2 (through abs then square, or direct: the same number in float64)
  acc[m] = sum_f fb[f][m] P[f], fb the Slaney filterbank of n_mels triangles over 0 .. 8000 Hz, each of area 1 in Hz
  logmel[m][t] = log(acc + 2^-24)
  features[t][m] = (logmel[m][t] - mean_m) / (sd_m + 1e-5), sd_m from the unbiased variance over the clip's frames
Streaming (process_chunk): the signal is already pre-emphasised, frame t, tap k = y[160 t + k] for k < 400 under the left-aligned window, zero for
k >= 400 (no centring, no reflection), (n - 400) // 160 + 1 frames, log-mel [frames][n_mels], no normalisation.

THE BOUND on |logmel_fp32 - logmel_float64|, u = 2^-24 (every fp32 operation returns its exact result times 1 + e, |e| <= u; terms in u^2 are
kept where they are written below and dropped elsewhere).  Every count is an operation count of the chain above, done in fp32 in any order that
keeps the filterbank a chain of fused multiply-adds and the FFT nine radix-2 stages:

 1. the framed sample s = (x_i - c x_{i-1}) w_k.  With a = 0.97 |x_{i-1}| and d = |x_i - 0.97 x_{i-1}|:
      c = fl(0.97)                       u a          the rounded coefficient
      fl(c x_{i-1})                      u a          rounding 1
      fl(x_i - .)                        u (d + 2 u a)  rounding 2
      w_k = fl(W_k)                      u (d + 2 u a)  the rounded window entry
      fl(. w_k)                          u (d + 2 u a)  rounding 3
    e_k = u W_k (2 a + 3 (d + 2 u a)).  At sample 0 (y[0] = x[0]) a = 0.  Streaming: the sample is given, e_k = 2 u W_k |y| (window entry, product).
 2. the FFT.  The input error reaches bin f as |sum_k e_k omega^(f k)| <= ||e||_1.  One radix-2 stage maps z to z' = (a + w b, a - w b),
    ||z'||_2 = sqrt 2 ||z||_2.  In fp32: the twiddle's two components are rounded, |dw| <= u; t = w b by one product and one fused
    multiply-add per component, |dt_r| <= u |w_r b_r| + u |t_r| <= 2 u (|w_r b_r| + |w_i b_i|) <= 2 u |b|, so |dt| <= 2 sqrt 2 u |b|; the two sums are
    rounded, u |a +- t| each.  Over the stage: ||error||_2 <= sqrt 2 (1 + 2 sqrt 2) u ||b half||_2 + u ||z'||_2 <= eta ||z'||_2 with
    eta = (2 + 2 sqrt 2) u.  The eight later stages carry it on as sqrt 2 x unitary maps, so after nine stages
      ||dX||_2 <= 9 eta sqrt 512 ||s||_2       (s the frame as computed: ||s||_2 <= ||s exact||_2 + ||e||_2)
    and one bin has |dX_f| <= ||dX||_2: a bin that holds only leakage has an ABSOLUTE error set by the frame's norm, not a relative one.
      dX = ||e||_1 + 9 eta sqrt 512 (||s||_2 + ||e||_2)       for every bin of the frame
 3. the power.  |X|^2 moves by 2 |X_f| dX + dX^2.  re^2 + im^2 as one product and one fused multiply-add: relative 2 u; through abs: the root halves
    that and adds u (2 u), the square doubles it and adds u (5 u).  c_p = 5 (abs then square) or 2 (direct):
      dP_f = 2 |X_f| dX + dX^2 + c_p u (|X_f| + dX)^2
 4. the filterbank: a chain of K_m = f_hi - f_lo + 1 fused multiply-adds over non-negative terms (every partial sum <= the final one: K_m roundings of
    at most u acc each), weights rounded to fp32 (u more):
      dacc_m = sum_f fb[f][m] dP_f + (K_m + 1) u sum_f fb[f][m] (P_f + dP_f)
 5. the log.  fl(acc + 2^-24): u (acc + 2^-24).  The fp32 log itself: the project's logf is pinned within 2 ulp of libm's (tests/test_oracle_math.py),
    libm's within 1 ulp of the truth, an ulp is at most 2 u |value|: 6 u |logmel|, which is 6 u |logmel| (acc + 2^-24) in units of the argument.
      dacc_m += u (1 + 6 |logmel|) (acc + 2^-24)
      bound = dacc_m / (acc_m + 2^-24)
    This is the logarithm's bound to first order in r = dacc / (acc + 2^-24).  It is exact for an error upwards (log(1 + r) <= r).  An error downwards
    can reach -log(1 - r) = r + r^2 / 2 + ..., never more than log((acc + 2^-24) / 2^-24) because a computed acc is not negative: where r is not small
    (leakage bins, bins the floor dominates) the bound written here is NARROWER than a rigorous one by that factor, so it asks more of an implementation,
    not less.  It is kept in the first-order form in which it was set; the printed err / bound show how far a right implementation stays from it.

THE NORMALISE BOUND is separate: its reference is the float64 mean, unbiased variance and quotient OF THE LOG-MEL THE IMPLEMENTATION RETURNED (fp32
values, exact inputs), so it covers the sums and the division only.  A sum of n terms by 64 partial sums and a six-level tree rounds at most
D = min(n - 1, ceil(n / 64) + 5) times on any path: |d sum| <= D u sum |terms|.  With c_t = x_t - mean (sum_t c_t = 0), S = sum_t c_t^2:
      dmean = D u mean|x| + u |mean|                                      (sum, division)
      rho_t = u (|c_t| + dmean)                                           (the rounding of x_t - mean^)
      dc_t  = dmean + rho_t                                               (c^_t = c_t - dm + r_t, |dm| <= dmean, |r_t| <= rho_t)
      dS    = n dmean^2 + 2 sum_t (|c_t| + dmean) rho_t + sum_t rho_t^2   (sum_t (c_t - dm)^2 = S + n dm^2 because sum_t c_t = 0: the shift of the
                                                                           mean enters the sum of squares in the second order only)
      dvar  = (dS + (D + 1) u (S + dS)) / (n - 1) + u (var + ...)         (the squares and their sum: D + 1 roundings; the division)
      dsd   = min(dvar / sd, sqrt dvar) + u (sd + .)                      (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt |a - b|; the root)
      dden  = dsd + u 1e-5 + u (den + dsd)                                (the rounded 1e-5, the sum)
      lo    = max(den - dden, 1e-5 (1 - 3 u))                             (the fp32 denominator is fl(fl(sd) + fl(1e-5)) with fl(sd) >= 0: never
                                                                           below 1e-5 (1 - 2 u), however badly the root is determined)
      bound_t = dc_t / lo + |c_t| dden / (den lo) + u (|c_t| + dc_t) / lo     (c^/den^ - c/den = (c^ - c)/den^ + c (den - den^)/(den den^); the quotient)
The bound is finite at every element (normalize_bound asserts it).
With normalisation off the features ARE the log-mel, transposed: bound 0.

Running this file prints max(err / bound) of the oracle against this reference for every case (python tests/mel_ref.py).
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
N_FFT, HOP, WIN, PAD, SR = 512, 160, 400, 256, 16000.0
FLOOR = 2.0 ** -24
ETA = (2.0 + 2.0 * math.sqrt(2.0)) * U
MUTANTS = ("reflect_left", "reflect_right", "preemph_after_pad", "window_shift", "hop159", "biased_variance", "y0")


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def hann_window(centered=False, shift=0):
    w = np.zeros(N_FFT)
    off = ((N_FFT - WIN) // 2 if centered else 0) + shift
    w[off:off + WIN] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / (WIN - 1))
    return w


@functools.lru_cache(maxsize=None)
def filterbank(n_mels):
    """Slaney: mel = 3 f / 200 below 1 kHz, 15 + ln(f / 1000) / (ln(6.4) / 27) above; n_mels + 2 points equally spaced in mel over 0 .. 8000 Hz;
    triangle m rises over [p_m, p_m+1], falls over [p_m+1, p_m+2], scaled by 2 / (p_m+2 - p_m).  -> [257][n_mels]"""
    step = math.log(6.4) / 27.0
    hz2mel = lambda f: f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) / step
    mel2hz = lambda m: m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * step)
    top = hz2mel(SR / 2.0)
    pts = np.array([mel2hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)])
    f = np.arange(N_FFT // 2 + 1) * SR / N_FFT
    fb = np.zeros((N_FFT // 2 + 1, n_mels))
    for m in range(n_mels):
        lo, c, hi = pts[m], pts[m + 1], pts[m + 2]
        fb[:, m] = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c))) * 2.0 / (hi - lo)
    return fb


def band_lengths(n_mels):
    """K_m = f_hi - f_lo + 1 of every filter (0 for one without a tap)"""
    nz = filterbank(n_mels).astype(np.float32) != 0
    return np.array([(np.flatnonzero(c)[-1] - np.flatnonzero(c)[0] + 1) if c.any() else 0 for c in nz.T])


def offline_frames(x, mutant=None):
    """-> (d [frames][512]: the pre-emphasised, reflect-padded signal under every tap, a [frames][512]: 0.97 |predecessor| of that sample)"""
    x = np.asarray(x, np.float64)
    n = x.size
    nf = 1 + n // HOP
    hop = 159 if mutant == "hop159" else HOP
    j = hop * np.arange(nf)[:, None] + np.arange(N_FFT)[None, :] - PAD
    lo_off = 1 if mutant == "reflect_left" else 0                  # (-j - 1: the edge sample twice)
    hi_off = 1 if mutant == "reflect_right" else 0
    idx = np.where(j < 0, -j - lo_off, j)
    idx = np.where(idx >= n, 2 * (n - 1) - idx + hi_off, idx)
    if mutant == "preemph_after_pad":                              # the raw signal padded, every padded sample minus 0.97 x its left neighbour
        jp = j - 1
        prev = np.where(jp < 0, -jp, jp)
        prev = np.where(prev >= n, 2 * (n - 1) - prev, prev)
        first = j == j.min()
    else:
        prev = idx - 1
        first = idx == 0
    a = np.where(first, 0.0, 0.97 * np.abs(x[np.maximum(prev, 0)]))
    d = x[idx] - np.where(first, 0.0, 0.97 * x[np.maximum(prev, 0)])
    if mutant == "y0":
        d = np.where(idx == 0, x[0] - 0.97 * x[0], d)
        a = np.where(idx == 0, 0.97 * abs(x[0]), a)
    return d, a


def _logmel_of_frames(d, e_per_tap, w, n_mels, power_via_abs, c_p):
    """frames d [nf][512] under window w, per-tap input error e -> (logmel [nf][n_mels], bound [nf][n_mels])"""
    s = d * w
    e = e_per_tap * w
    Z = np.fft.rfft(s, axis=1)
    X = np.abs(Z)
    P = X * X if power_via_abs else Z.real ** 2 + Z.imag ** 2
    fb = filterbank(n_mels)
    acc = P @ fb
    lm = np.log(acc + FLOOR)
    dX = e.sum(axis=1) + 9.0 * ETA * math.sqrt(N_FFT) * (np.sqrt((s * s).sum(axis=1)) + np.sqrt((e * e).sum(axis=1)))
    dX = dX[:, None]
    dP = 2.0 * X * dX + dX * dX + c_p * U * (X + dX) ** 2
    K = band_lengths(n_mels)[None, :]
    dacc = dP @ fb + (K + 1) * U * ((P + dP) @ fb)
    dacc = dacc + U * (1.0 + 6.0 * np.abs(lm)) * (acc + FLOOR)
    return lm, dacc / (acc + FLOOR)


def logmel(x, n_mels=80, centered=False, power_via_abs=True, mutant=None):
    """offline: x [n] -> (logmel [n_mels][frames], bound [n_mels][frames]), both float64"""
    d, a = offline_frames(x, mutant)
    w = hann_window(centered, 1 if mutant == "window_shift" else 0)
    e = U * (2.0 * a + 3.0 * (np.abs(d) + 2.0 * U * a))
    lm, bd = _logmel_of_frames(d, e, w, n_mels, power_via_abs, 5.0 if power_via_abs else 2.0)
    return lm.T.copy(), bd.T.copy()


def preemphasize_f32(x, last=0.0):
    """what a streaming session does to a chunk before it frames it, in fp32: y[i] = x[i] - fl(0.97f x[i - 1]), the carried sample in front"""
    x = np.asarray(x, np.float32)
    p = np.concatenate([[np.float32(last)], x[:-1]]).astype(np.float32) * np.float32(0.97)
    return (x - p).astype(np.float32)


def stream_logmel(y, n_mels=80):
    """streaming: y [n] already pre-emphasised -> (logmel [frames][n_mels], bound), float64"""
    y = np.asarray(y, np.float64)
    nf = (y.size - WIN) // HOP + 1
    d = np.zeros((nf, N_FFT))
    d[:, :WIN] = y[HOP * np.arange(nf)[:, None] + np.arange(WIN)[None, :]]
    return _logmel_of_frames(d, 2.0 * U * np.abs(d), hann_window(False), n_mels, True, 5.0)


def normalize(lm, biased=False):
    """logmel [n_mels][frames] -> features [frames][n_mels], float64"""
    lm = np.asarray(lm, np.float64)
    n = lm.shape[1]
    c = lm - lm.mean(axis=1, keepdims=True)
    var = (c * c).sum(axis=1, keepdims=True) / (n if biased else n - 1)
    return (c / (np.sqrt(var) + 1e-5)).T.copy()


def normalize_bound(lm):
    """logmel [n_mels][frames] as the implementation returned it -> bound [frames][n_mels] on |features_fp32 - normalize(lm)|, finite everywhere"""
    lm = np.asarray(lm, np.float64)
    n = lm.shape[1]
    D = min(n - 1, -(-n // 64) + 5)
    mean = lm.mean(axis=1, keepdims=True)
    c = np.abs(lm - mean)
    dmean = D * U * np.abs(lm).mean(axis=1, keepdims=True) + U * np.abs(mean)
    rho = U * (c + dmean)
    dc = dmean + rho
    S = (c * c).sum(axis=1, keepdims=True)
    dS = n * dmean * dmean + (2.0 * (c + dmean) * rho + rho * rho).sum(axis=1, keepdims=True)
    var = S / (n - 1)
    dvar = (dS + (D + 1) * U * (S + dS)) / (n - 1)
    dvar = dvar + U * (var + dvar)
    sd = np.sqrt(var)
    dsd = np.minimum(np.where(sd > 0, dvar / np.where(sd > 0, sd, 1.0), np.inf), np.sqrt(dvar))
    dsd = dsd + U * (sd + dsd)
    den = sd + 1e-5
    dden = dsd + U * 1e-5 + U * (den + dsd)
    lo = np.maximum(den - dden, 1e-5 * (1.0 - 3.0 * U))
    bound = dc / lo + c * dden / (den * lo) + U * (c + dc) / lo
    assert np.all(np.isfinite(bound)), "the normalise bound must be finite at every element"
    return bound.T.copy()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("noise", "quiet", "zeros", "const", "tone", "imp0", "impN", "tail")


def make_clip(family, n, seed, k=0):
    """one clip of n samples; k = its place in the batch (so that the clips of a batch differ where the family allows it)"""
    rng = np.random.default_rng([seed, k, FAMILIES.index(family)])
    x = np.zeros(n, np.float32)
    amp = (1.0, -0.5, 0.25)[k % 3]
    if family == "noise":
        x[:] = rng.uniform(-1.0, 1.0, n)
    elif family == "quiet":                                         # the log floor 2^-24 dominates every bin
        x[:] = 1e-6 * rng.uniform(-1.0, 1.0, n)
    elif family == "const":                                         # the pre-emphasis step at sample 0: y = 0.5, 0.015, 0.015, ...
        x[:] = 0.5 * amp
    elif family == "tone":                                          # the centre of FFT bin 40: most bins hold only leakage
        x[:] = 0.5 * amp * np.sin(2.0 * np.pi * 40.0 * np.arange(n) / N_FFT + 0.3 * k)
    elif family == "imp0":
        x[0] = amp
    elif family == "impN":
        x[n - 1] = amp
    elif family == "tail":                                          # the right-hand reflection is the only source of the last frames' right half
        x[n - 100:] = rng.uniform(-1.0, 1.0, 100)
    return x


def samples_for(nf, r):
    return HOP * (nf - 1) + r


# offline uniform: (frames, r, clips, n_mels, normalize, centered window, power through abs, family); n = 160 (frames - 1) + r
UNIFORM_CASES = [
    (2, 97, 1, 80, 1, 0, 1, "noise"), (2, 159, 3, 128, 0, 0, 1, "quiet"), (15, 0, 1, 40, 1, 0, 1, "zeros"), (16, 1, 3, 65, 1, 0, 1, "const"),
    (17, 97, 3, 80, 0, 0, 1, "tone"), (31, 159, 1, 128, 1, 0, 1, "imp0"), (32, 0, 3, 40, 0, 0, 1, "impN"), (33, 1, 1, 65, 0, 0, 1, "tail"),
    (63, 97, 1, 128, 1, 0, 1, "tone"), (64, 159, 3, 80, 1, 0, 1, "impN"), (65, 0, 1, 65, 1, 0, 1, "noise"), (128, 1, 3, 40, 1, 0, 1, "tail"),
    (129, 97, 1, 80, 0, 0, 1, "imp0"),
    (17, 1, 1, 80, 1, 1, 1, "noise"), (64, 0, 3, 128, 1, 1, 1, "const"),        # switch A1
    (33, 159, 3, 80, 1, 0, 0, "quiet"), (65, 97, 1, 128, 0, 0, 0, "tone"),      # power without the root
]
# offline ragged: (frames of every clip, n_mels, normalize); clip k takes r = (0, 1, 97, 159)[k % 4] (two frames: 97 / 159) and family (first + k) % 8
RAGGED_CASES = [
    ((2, 129, 16, 17), 80, 1, 0), ((129, 2, 2, 2), 128, 0, 4), ((33, 64, 65, 15, 16), 65, 1, 1), ((33,), 40, 1, 6),
]
# streaming: (frames, r, sessions, n_mels, family); n = 400 + 160 (frames - 1) + r
STREAM_CASES = [
    (1, 0, 1, 80, "noise"), (1, 159, 3, 128, "quiet"), (3, 0, 3, 80, "zeros"), (3, 159, 1, 128, "const"), (4, 0, 1, 128, "tone"), (4, 159, 3, 80, "imp0"),
    (5, 0, 3, 128, "impN"), (5, 159, 1, 80, "tail"), (8, 0, 1, 80, "const"), (8, 159, 3, 128, "noise"), (9, 0, 3, 80, "tail"), (9, 159, 1, 128, "tone"),
]


def uniform_id(c):
    return f"nf{c[0]}-r{c[1]}-B{c[2]}-m{c[3]}-norm{c[4]}-ctr{c[5]}-abs{c[6]}-{c[7]}"


def ragged_id(c):
    return "nf" + "_".join(str(v) for v in c[0]) + f"-m{c[1]}-norm{c[2]}"


def stream_id(c):
    return f"nf{c[0]}-r{c[1]}-S{c[2]}-m{c[3]}-{c[4]}"


@functools.lru_cache(maxsize=None)
def uniform_clips(c):
    nf, r, B = c[:3]
    out = np.stack([make_clip(c[7], samples_for(nf, r), 100 + nf, k) for k in range(B)])
    out.setflags(write=False)
    return out


def ragged_families(c):
    return [FAMILIES[(c[3] + k) % 8] for k in range(len(c[0]))]


@functools.lru_cache(maxsize=None)
def ragged_clips(c):
    out = []
    for k, (nf, fam) in enumerate(zip(c[0], ragged_families(c))):
        r = (97, 159)[k % 2] if nf == 2 else (0, 1, 97, 159)[k % 4]
        x = make_clip(fam, samples_for(nf, r), 200 + nf, k)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stream_clips(c):
    """-> (raw [S][n], pre-emphasised as a session's first chunk [S][n])"""
    nf, r, S = c[:3]
    raw = np.stack([make_clip(c[4], WIN + samples_for(nf, r), 300 + nf, k) for k in range(S)])
    pre = np.stack([preemphasize_f32(x) for x in raw])
    raw.setflags(write=False), pre.setflags(write=False)
    return raw, pre


@functools.lru_cache(maxsize=None)
def ref_logmel(x_bytes, n_mels, centered, power_via_abs):
    """the reference log-mel and bound of one clip (cached: the CPU and the GPU test, the ragged and the uniform form share them)"""
    lm, bd = logmel(np.frombuffer(x_bytes, np.float32), n_mels, bool(centered), bool(power_via_abs))
    lm.setflags(write=False), bd.setflags(write=False)
    return lm, bd


def ref_of(x, n_mels, centered=False, power_via_abs=True):
    return ref_logmel(np.ascontiguousarray(x, np.float32).tobytes(), n_mels, bool(centered), bool(power_via_abs))


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound, and where (an exact element counts 0 whatever its bound; a NaN counts as infinite)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()), tuple(int(v) for v in np.unravel_index(int(q.argmax()), q.shape))


def check_logmel(got, ref, bound, what):
    q, at = ratio(got, ref, bound)
    print(f"{what}: log-mel max err / bound {q:.4f} at {at}")
    assert q <= 1.0, f"{what}: log-mel leaves the bound at {at}: {got[at]!r} vs {ref[at]!r}, bound {bound[at]:.3e}"
    return q


def check_features(feats, lm, normalized, what):
    """feats [frames][n_mels] against the float64 statistics of the fp32 log-mel lm [n_mels][frames] it was made from"""
    if not normalized:
        assert np.array_equal(feats.view(np.uint32), np.ascontiguousarray(lm.T).view(np.uint32)), f"{what}: un-normalised features are not the log-mel"
        return 0.0
    q, at = ratio(feats, normalize(lm), normalize_bound(lm))
    print(f"{what}: normalise max err / bound {q:.4f} at {at}")
    assert q <= 1.0, f"{what}: features leave the normalise bound at {at}"
    return q


def split_offline(lm_buf, ft_buf, n_mels, frames):
    """The whole buffers of an offline launch (uniform or ragged: clip after clip) -> (logmel [n_mels][frames] per clip, features [frames][n_mels] per
    clip, the words of lm_buf / ft_buf no launch should have written)"""
    lms, fts = [], []
    lm_free, ft_free = np.ones(lm_buf.size, bool), np.ones(ft_buf.size, bool)
    lo = fo = 0
    for nf in frames:
        pitch = (nf + 15) & ~15
        blk = lm_buf[lo:lo + n_mels * pitch].reshape(n_mels, pitch)
        lms.append(blk[:, :nf].copy())
        keep = np.zeros((n_mels, pitch), bool)
        keep[:, :nf] = True
        lm_free[lo:lo + n_mels * pitch] = ~keep.reshape(-1)
        fts.append(ft_buf[fo:fo + nf * n_mels].reshape(nf, n_mels).copy())
        ft_free[fo:fo + nf * n_mels] = False
        lo += n_mels * pitch
        fo += nf * n_mels
    return lms, fts, lm_free, ft_free


if __name__ == "__main__":
    import dataclasses
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    import oracle
    import pkload
    pk = pkload.load()
    from parakeet_cpp_amd import synth
    worst, worst_norm = {}, 0.0

    def offline(x, fam, n_mels, norm, centered=0, pabs=1):
        global worst_norm
        lm, bd = ref_of(x, n_mels, centered, pabs)
        ft, got = oracle.mel(x, n_mels=n_mels, return_logmel=True, normalize=bool(norm), window_centered=bool(centered), power_via_abs=bool(pabs))
        worst[fam] = max(worst.get(fam, 0.0), ratio(got, lm, bd)[0])
        if norm:
            worst_norm = max(worst_norm, ratio(ft, normalize(got), normalize_bound(got))[0])

    for c in UNIFORM_CASES:
        for x in uniform_clips(c):
            offline(x, c[7], c[3], c[4], c[5], c[6])
    for c in RAGGED_CASES:
        for x, fam in zip(ragged_clips(c), ragged_families(c)):
            offline(x, fam, c[1], c[2])
    for c in STREAM_CASES:
        cfg = dataclasses.replace(pk.make_tiny_config(), mel_bins=c[3], name=f"tiny-mel{c[3]}")
        om = oracle.Model(cfg, synth.synth_weights(cfg, seed=42))
        raw, pre = stream_clips(c)
        for k in range(c[2]):
            lm, bd = stream_logmel(pre[k], c[3])
            worst[c[4]] = max(worst.get(c[4], 0.0), ratio(oracle.Stream(om).mel(raw[k]), lm, bd)[0])
    print("oracle, worst log-mel err / bound per family:", {k: round(v, 4) for k, v in worst.items()})
    print("oracle, worst normalise err / bound:", round(worst_norm, 4))
