"""The specification of the device resampler (kernels/resample.hip): the polyphase form of the host's Kaiser-windowed
sinc resampler (csrc/wav.cpp sinc_resample).

    g = gcd(src, dst), up = dst / g, down = src / g
    T[r][k], r = 0 .. up - 1, k = 0 .. 31: the weight of the tap at distance ((r * down) % up) / up + (15 - k), in the host's expressions
    output i = q * up + r of a clip of n samples: centre c = q * down + (r * down) // up; tap k reads j = c - 15 + k, skipped outside [0, n);
    sum += float64(x[j]) * T[r][k], wsum += T[r][k] for k ascending, every operation rounded on its own (no fused multiply-add);
    out = float32(sum / wsum) if wsum > 1e-10 else 0;   out_len = ceil(n * up / down);   src == dst copies.

table() is written with Python's math functions (the C library's sin / sqrt that the host uses); walk() takes any table, so a test can pin the
library's table against table() and then walk over either."""
import math

import numpy as np

HALF_WIDTH = 16
BETA = 7.857
TAPS = 2 * HALF_WIDTH


def _bessel_i0(x):
    s, term = 1.0, 1.0
    for k in range(1, 30):
        term *= (x * x) / (4.0 * k * k)
        s += term
        if term < 1e-12 * s:
            break
    return s


def _kaiser(n, N, beta):
    arg = 2.0 * n / N - 1.0
    val = 1.0 - arg * arg
    if val < 0.0:
        val = 0.0
    return _bessel_i0(beta * math.sqrt(val)) / _bessel_i0(beta)


def up_down(src, dst):
    g = math.gcd(src, dst)
    return dst // g, src // g


def out_len(n, src, dst):
    up, down = up_down(src, dst)
    return (n * up + down - 1) // down


def table(src, dst):
    """T[up][32] in float64, from the expressions of sinc_resample."""
    up, down = up_down(src, dst)
    ratio = float(src) / float(dst)
    cutoff = min(1.0, 1.0 / max(ratio, 1.0))
    filter_scale = cutoff
    width_factor = max(1.0, ratio)
    T = np.zeros((up, TAPS), np.float64)
    for r in range(up):
        frac = float((r * down) % up) / float(up)
        for k in range(TAPS):
            dist = frac + float(HALF_WIDTH - 1 - k)
            window_pos = dist / width_factor
            assert abs(window_pos) <= HALF_WIDTH          # the host loop's skip never fires for these distances
            w = _kaiser(window_pos + HALF_WIDTH, 2.0 * HALF_WIDTH, BETA)
            x = dist * cutoff * math.pi
            sinc = 1.0 if abs(x) < 1e-10 else math.sin(x) / x
            T[r, k] = sinc * w * filter_scale
    return T


def walk(x, src, dst, T=None):
    """One clip through the table T (default: table(src, dst)) -> float32[out_len]."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if src == dst:
        return x.copy()
    up, down = up_down(src, dst)
    if T is None:
        T = table(src, dst)
    assert T.shape == (up, TAPS) and T.dtype == np.float64
    n = x.size
    m = out_len(n, src, dst)
    i = np.arange(m, dtype=np.int64)
    q, r = i // up, i % up
    c = q * down + (r * down) // up
    xd = x.astype(np.float64)
    s = np.zeros(m, np.float64)
    ws = np.zeros(m, np.float64)
    for k in range(TAPS):
        j = c - (HALF_WIDTH - 1) + k
        ok = (j >= 0) & (j < n)
        w = T[r, k]
        xv = xd[np.clip(j, 0, max(n - 1, 0))] if n else np.zeros(m)
        s = np.where(ok, s + xv * w, s)                   # (a product and a sum, each rounded: numpy does not fuse them)
        ws = np.where(ok, ws + w, ws)
    good = ws > 1e-10
    out = np.zeros(m, np.float32)
    out[good] = (s[good] / ws[good]).astype(np.float32)
    return out
