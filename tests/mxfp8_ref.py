"""The MXFP8 format of the feed-forward products (OCP MX: e4m3 elements, one E8M0 scale per 32 k), restated in numpy / torch.

A block v of 32 elements along K: amax = max|v|; e = clamp(floor(log2(amax)) - 8, -127, 127), -127 for amax == 0; scale byte = e + 127;
element = e4m3 (OCP "fn") of clamp(v / 2^e, -448, 448), round to nearest even.  v / 2^e is exact, so every element is rounded once.
NaN / Inf inputs are out of scope."""
import numpy as np
import torch


def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


def quantize(x):
    """x [rows][K], K % 32 == 0 -> (element bytes uint8 [rows][K], scale bytes uint8 [rows][K / 32])"""
    x = np.ascontiguousarray(x, np.float64)
    rows, K = x.shape
    b = x.reshape(rows, K // 32, 32)
    amax = np.abs(b).max(axis=2)
    e = np.where(amax > 0, np.frexp(amax)[1] - 1 - 8, -127)           # frexp: amax = m 2^ex with 0.5 <= m < 1, so floor(log2) = ex - 1, exactly
    e = np.clip(e, -127, 127).astype(np.int64)
    scaled = np.clip(b / np.exp2(e.astype(np.float64))[:, :, None], -448.0, 448.0)   # the clamp comes first: e4m3fn has no infinity to saturate to
    q = torch.from_numpy(scaled.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q.reshape(rows, K), (e + 127).astype(np.uint8)


def dequantize(q, s):
    """-> float64 [rows][K]: exactly the values the matrix instruction multiplies"""
    v = torch.from_numpy(np.ascontiguousarray(q)).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    return v * np.repeat(np.exp2(s.astype(np.float64) - 127.0), 32, axis=1)


def qdq(x):
    return dequantize(*quantize(x))


def product(a, w, bias=None):
    """float64 out = sum over blocks of 2^(ea + ew) sum_k qa qw + bias of the QUANTISED operands, and sum |a w| + |bias| (what error bounds scale with)"""
    a, w = qdq(a), qdq(w)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float64)
    return a @ w.T + b, np.abs(a) @ np.abs(w).T + np.abs(b)


def edge_rows(K=128, seed=0):
    """Rows that meet every branch of the quantiser: zeros among values, a block of all zeros, amax exactly a power of two, amax just under one
    (scaled: just under 512 -> clamped to 448), values between 448 and 512 after scaling, tiny and large magnitudes, plain gaussians."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((8, K)).astype(np.float32)
    x[0, ::3] = 0.0
    x[1, 32:64] = 0.0
    x[2, :32] = rng.uniform(-1, 1, 32); x[2, 5] = 8.0
    x[3, :32] = rng.uniform(-0.5, 0.5, 32); x[3, 7] = np.float32(1.0) - np.float32(2.0 ** -24)
    x[4, :32] = rng.uniform(-200, 200, 32); x[4, 3] = 480.0; x[4, 4] = -500.0; x[4, 9] = 449.0
    x[5] *= np.float32(2.0 ** -100)
    x[6] *= np.float32(2.0 ** 100)
    return x
