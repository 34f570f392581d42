"""Two references of the streaming encoder's cached attention (kernels/stream.hip) and the cases its kernels are tested at.

(a) spec_bits: the SPECIFICATION, bit for bit.  The kernels promise the oracle's bits (oracle/pk_oracle.c stream_attention); this composes them
    from the oracle's exported primitives per (stream, head): the two natural-k fma chains from zero (orc.linear) of q + u with the keys and
    of q + v with the position rows off .. off + kv - 1, off = P - kv; (cs + ps) * scale in float32 with scale = 1 / sqrt(hd) formed in
    float32 as the oracle forms it; masked scores REPLACED by -1e9; the row maximum; orc.math_v("exp") of the differences; orc.sum64; a
    float32 divide; the natural-k fma chain of the probabilities with the values.
(b) definition: the DEFINITION in float64, written from the model (src/streaming_encoder.cpp StreamingConformerAttention::forward_cached
    :162-272), with its quirks: the position scores are the rightmost kv columns of (q + v) P^T WITHOUT rel_shift (:215-232), the scores use
    the untrimmed [cache ; chunk] although the cache is trimmed to `left` rows for the next chunk (:186-208), query i sits at position
    kv - c + i of the keys and masked scores are replaced, not added to (:239-261).  It returns what attention_ref.check takes: per element the
    fp32 bound and sigma of attention_ref's docstring (section 3) with T := kv, masked keys left out of the |z| terms.

The expected new cache is plain numpy: the last min(keep_max, kv) rows of [cache[:nc] ; new] per stream, every other word the unwritten pattern.
"""
import collections

import numpy as np

import attention_ref as ar

UNWRITTEN = ar.UNWRITTEN["fp32"]
F32 = np.float32


def sigma_col(col):
    """column of ctx in the sigma layout (the out-projection's A operand): the two low bit pairs of the column exchanged"""
    col = np.asarray(col)
    return (col & ~15) | ((col & 3) << 2) | ((col >> 2) & 3)


Case = collections.namedtuple("Case", "name family S H hd c nc left right cache_rows keep_max P form")


def _mk(name, family, form, hd, H, c, nc, left, right, S=1, cache_rows=None, keep_max=None, P=None):
    """cache_rows / keep_max / P default to what a session passes: max(left, 1) rows (never fewer than nc), keep_max = left, the table of
    left + c frames"""
    if cache_rows is None:
        cache_rows = max(left, nc, 1)
    if keep_max is None:
        keep_max = max(left, 0)
    if P is None:
        P = 2 * (max(left, nc) + c) - 1
    return Case(name, family, S, H, hd, c, nc, left, right, cache_rows, keep_max, P, form)


def _cases():
    out = []
    fam = lambda: ar.FAMILIES[len(out) % 4]                       # random, large, key, pos in turn
    # ---- the LDS-tile form, both head sizes: the edges of what it takes, masked future keys (c > right + 1), short and long left contexts
    for hd, H, form in ((64, 2, "tiles-hd64"), (128, 1, "tiles-hd128")):
        t = f"tile{hd}"
        out.append(_mk(f"{t}-kv80-c8", fam(), form, hd, H, 8, 72, 72, 0, S=3))
        out.append(_mk(f"{t}-kv80-c1", fam(), form, hd, H, 1, 79, 79, 0))
        out.append(_mk(f"{t}-nc0-c1-kv1", fam(), form, hd, H, 1, 0, 70, 0, S=3))
        out.append(_mk(f"{t}-nc0-c8", fam(), form, hd, H, 8, 0, 70, 1))
        out.append(_mk(f"{t}-left6-right0-c4", fam(), form, hd, H, 4, 6, 6, 0))
        out.append(_mk(f"{t}-left10-right1-c4", fam(), form, hd, H, 4, 10, 10, 1, S=3))
        out.append(_mk(f"{t}-left70-right3-c6", fam(), form, hd, H, 6, 70, 70, 3, P=76))      # P == kv: the table read from row 0
    out.append(_mk("tile128-H2-left70-right1-c2", "key", "tiles-hd128", 128, 2, 2, 70, 70, 1))
    # ---- the switch between the forms
    out.append(_mk("switch-hd64-kv81-c1", fam(), "general-2w", 64, 2, 1, 80, 80, 0))
    out.append(_mk("switch-hd64-kv81-c8", fam(), "general-2w", 64, 2, 8, 73, 73, 1, S=3))
    out.append(_mk("switch-hd128-c9-kv64", fam(), "general-1w", 128, 1, 9, 55, 55, 2))
    out.append(_mk("switch-hd128-c9-kv65", fam(), "general-2w", 128, 1, 9, 56, 56, 0))
    out.append(_mk("switch-hd64-c9-kv65", fam(), "general-2w", 64, 4, 9, 56, 60, 3))
    # ---- the general kernel's head sizes: the 16 / 8 / 1 float4 steps of the score loop (hd 32: 8; 40: 8 + 1 + 1; 96: 16 + 8; 20: 1 x 5;
    # 256: 16 x 4, and two output-column rounds at 64 threads), the 24 / 8 / 1 rows of the value loop (kv 5: 1 x 5; 24: 24; 31: 24 + 7 x 1;
    # 64: 2 x 24 + 2 x 8; 65: + 1; 130: 5 x 24 + 8 + 2 x 1), one wavefront up to 64 keys and two beyond.  left = nc - 2: the two oldest keys are
    # masked for the first query of the chunk and one more for every later one; the new cache is shorter than the old one.
    for hd, H in ((32, 4), (40, 2), (96, 1), (20, 4), (256, 1)):
        for n, kv in enumerate((5, 24, 31, 64, 65, 130)):
            c = (1, 3, 2, 5, 4, 7)[(n + hd // 4) % 6]
            c = min(c, kv)
            nc = kv - c
            left = max(nc - 2, 1)
            out.append(_mk(f"general-hd{hd}-kv{kv}-c{c}", fam(), "general-2w" if kv > 64 else "general-1w", hd, H, c, nc, left,
                           (0, 1, 2)[(n + hd // 8) % 3], S=(1, 3)[(n + hd // 4) % 2], cache_rows=max(left, nc)))
    # ---- no mask: nothing is kept, the cache outputs stay untouched
    out.append(_mk("nomask-hd32-kv23", "random", "general-1w", 32, 4, 3, 20, -1, -1, S=3, cache_rows=20))
    out.append(_mk("nomask-hd64-kv12", "large", "tiles-hd64", 64, 2, 2, 10, -1, -1, cache_rows=10))
    # ---- the rotation on both kernels: the whole new cache from the chunk (keep < c), a filling cache, exactly full, the steady state, left = 0
    for hd, H, form in ((64, 2, "tiles-hd64"), (32, 4, "general-1w")):
        t = f"rotate-hd{hd}"
        out.append(_mk(f"{t}-left6-c8", fam(), form, hd, H, 8, 6, 6, 0, S=3))
        out.append(_mk(f"{t}-left1-c3", fam(), form, hd, H, 3, 1, 1, 1))
        out.append(_mk(f"{t}-filling", fam(), form, hd, H, 2, 3, 10, 0, S=3))
        out.append(_mk(f"{t}-exactly-full", fam(), form, hd, H, 2, 8, 10, 1))
        out.append(_mk(f"{t}-steady", fam(), form, hd, H, 2, 10, 10, 0, S=3))
        out.append(_mk(f"{t}-left0", fam(), form, hd, H, 2, 0, 0, 1))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def make_inputs(case, seed, fill=np.nan):
    """-> dict(qkv [S][c][3 d], kcache, vcache [S][cache_rows][d], pos [P][d], bias_u, bias_v [d]), float32.
    The families of attention_ref.make_inputs on the stream's geometry: random (near-uniform softmax), large (|scores| up to ~60), key (one
    key per (stream, head) -- the oldest, the newest, the last cached, the first of the chunk -- ~12 above the rest), pos (the position row of
    one key aligned with the queries).  Unlike there nothing is rounded to bf16 and every column e of the head carries its own magnitude: the
    products q_e k_e span 2^-3 .. 2^3 around their mean and the operands another 2^-2 .. 2^2 against each other, so the terms of a chain are
    inexact and of different sizes and a change of the k order moves bits.
    The cache rows nc .. cache_rows - 1 and the position rows below P - kv are set to `fill` (NaN: any use of them shows)."""
    rng = np.random.default_rng(seed)
    S, H, hd, c, nc = case.S, case.H, case.hd, case.c, case.nc
    d, kv, P = H * hd, nc + case.c, case.P
    off = P - kv
    N = lambda s, *shape: rng.standard_normal(shape) * s
    w = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    q, k, v = N(0.5, S, c, d), N(0.5, S, kv, d), N(1.0, S, kv, d)
    pos = N(0.5, P, d)
    bu, bv = N(0.1, d), N(0.1, d)
    fam = case.family
    if fam == "large":
        q, k, pos = N(4.0, S, c, d), N(4.0, S, kv, d), N(1.0, P, d)
    elif fam == "key":
        q = w + N(0.05, S, c, d)
        k, pos, bu, bv = N(0.05, S, kv, d), N(0.05, P, d), N(0.02, d), N(0.02, d)
        gamma = 12.0 / np.sqrt(hd)
        peaks = (0, kv - 1, max(nc - 1, 0), min(nc, kv - 1))
        for s in range(S):
            for h in range(H):
                k[s, peaks[(h + s + seed) % 4], h * hd: (h + 1) * hd] = w[h * hd: (h + 1) * hd] * gamma
    elif fam == "pos":
        q = w + N(0.05, S, c, d)
        k, pos, bu, bv = N(0.02, S, kv, d), N(0.05, P, d), N(0.02, d), N(0.02, d)
        gamma = 10.0 / np.sqrt(hd)
        peaks = (kv - 1, max(kv - c, 0), max(kv - c - 1, 0), 0)
        for h in range(H):
            pos[off + peaks[(h + seed) % 4], h * hd: (h + 1) * hd] = w[h * hd: (h + 1) * hd] * gamma
    t = 2.0 ** rng.uniform(-3, 3, d)                             # size of the products of column e ...
    t = t / np.sqrt((t * t).reshape(H, hd).mean(axis=1)).repeat(hd)
    g = 2.0 ** rng.uniform(-2, 2, d)                             # ... and how it is split between the two operands
    q, bu, bv = q * np.sqrt(t) * g, bu * np.sqrt(t) * g, bv * np.sqrt(t) * g
    k, pos = k * np.sqrt(t) / g, pos * np.sqrt(t) / g
    v = v * 2.0 ** rng.uniform(-3, 3, d)
    qkv = np.concatenate([q, k[:, nc:], v[:, nc:]], axis=2).astype(F32)
    kcache, vcache = (np.full((S, case.cache_rows, d), fill, F32) for _ in range(2))
    kcache[:, :nc], vcache[:, :nc] = k[:, :nc], v[:, :nc]
    if not np.isnan(fill):
        kcache[:, nc:], vcache[:, nc:] = N(1.0, S, case.cache_rows - nc, d), N(1.0, S, case.cache_rows - nc, d)
    pos = pos.astype(F32)
    pos[:off] = fill if np.isnan(fill) else N(0.5, off, d)
    return dict(qkv=qkv, kcache=kcache, vcache=vcache, pos=pos, bias_u=bu.astype(F32), bias_v=bv.astype(F32))


def masked(case, kv, left=None, right=None, chunk_relative=False):
    """[c][kv] True where the score is replaced (:239-253): dist = (kv - c + i) - j, dist > left or -dist > right; no mask unless left >= 0 or
    right >= 0"""
    left = case.left if left is None else left
    right = case.right if right is None else right
    i, j = np.arange(case.c)[:, None], np.arange(kv)[None, :]
    if not (left >= 0 or right >= 0):
        return np.zeros((case.c, kv), bool)
    dist = (i if chunk_relative else kv - case.c + i) - j
    return (dist > left) | (-dist > right)


def _head(case, inp, s, h):
    """q [c][hd], K, V [kv][hd] = [cache[:nc] ; chunk], u, v [hd] of one (stream, head)"""
    d, hd, nc = case.H * case.hd, case.hd, case.nc
    cs = slice(h * hd, (h + 1) * hd)
    x = inp["qkv"][s]
    K = np.concatenate([inp["kcache"][s, :nc, cs], x[:, d:][:, cs]])
    V = np.concatenate([inp["vcache"][s, :nc, cs], x[:, 2 * d:][:, cs]])
    return x[:, cs], K, V, inp["bias_u"][cs], inp["bias_v"][cs]


MUTANTS = ("rel_shift", "off_minus1", "mask_chunk_relative", "cache_trimmed", "swap_uv", "swap_left_right")


def spec_bits(orc, case, inp, mut=None):
    """(a): ctx [S c][d] float32, the oracle's bits.  mut: one of MUTANTS, the deliberately wrong variants of tests/test_stream_attention_ref.py."""
    S, H, hd, c, nc = case.S, case.H, case.hd, case.c, case.nc
    d, kv = H * hd, nc + c
    off = case.P - kv - (1 if mut == "off_minus1" else 0)
    scale = F32(1.0) / np.sqrt(F32(hd))
    left, right = (case.right, case.left) if mut == "swap_left_right" else (case.left, case.right)
    mask = masked(case, kv, left, right, chunk_relative=mut == "mask_chunk_relative")
    if mut == "cache_trimmed":                                   # the keys the next chunk's cache drops are already gone
        mask = mask | (np.arange(kv)[None, :] < kv - min(max(case.left, 0), kv))
    ctx = np.zeros((S * c, d), F32)
    for s in range(S):
        for h in range(H):
            q, K, V, u, v = _head(case, inp, s, h)
            if mut == "swap_uv":
                u, v = v, u
            Ph = inp["pos"][:, h * hd: (h + 1) * hd]
            cs = orc.linear(q + u, K)
            if mut == "rel_shift":                               # row of key j for query i: off + j + (c - 1 - i), as a shifted table would give
                ps = np.stack([orc.linear((q + v)[i: i + 1], Ph[np.clip(off + np.arange(kv) + c - 1 - i, 0, case.P - 1)])[0] for i in range(c)])
            else:
                ps = orc.linear(q + v, Ph[off: off + kv])
            sc = ((cs + ps) * scale).astype(F32)
            sc = np.where(mask, F32(-1e9), sc)
            e = orc.math_v("exp", sc - sc.max(axis=1, keepdims=True))
            p = np.stack([row / orc.sum64(row) for row in e]).astype(F32)
            ctx[s * c: (s + 1) * c, h * hd: (h + 1) * hd] = orc.linear(p, np.ascontiguousarray(V.T))
    return ctx


def definition(case, inp):
    """(b): [(ctx rows, head, ctx, bound, sigma)] in float64, the argument attention_ref.check takes"""
    S, H, hd, c, nc = case.S, case.H, case.hd, case.c, case.nc
    kv = nc + c
    scale = 1.0 / np.sqrt(hd)
    mask = masked(case, kv)
    out = []
    for s in range(S):
        for h in range(H):
            q, K, V, u, v = (np.asarray(a, np.float64) for a in _head(case, inp, s, h))
            p = np.asarray(inp["pos"][:, h * hd: (h + 1) * hd], np.float64)
            content = (q + u) @ K.T                              # :215
            with np.errstate(invalid="ignore"):                  # (the rows of the table that the slice below drops may hold anything)
                pos_score = (q + v) @ p.T                        # :221
                pos_mag = np.abs(q + v) @ np.abs(p).T
            if pos_score.shape[1] > kv:                          # the rightmost kv columns :225-232
                pos_score, pos_mag = pos_score[:, pos_score.shape[1] - kv:], pos_mag[:, pos_mag.shape[1] - kv:]
            z = (content + pos_score) * scale                    # :234
            z = np.where(mask, -1e9, z)                          # masked_fill :260
            mag = np.abs(q + u) @ np.abs(K).T + pos_mag
            ctx, bound, sigma = ar.softmax_pv_bounds("fp32", z, mag, V, scale, hd, live=~mask)
            out.append((s * c + np.arange(c), h, ctx, bound, sigma))
    return out


def expected_cache(case, inp, which, rotate=True):
    """the K (which = 1) or V (2) cache buffer after the launch, as bits: [S cache_rows + GUARD_ROWS][d] uint32"""
    S, c, nc, d = case.S, case.c, case.nc, case.H * case.hd
    kv = nc + c
    keep = min(case.keep_max, kv) if rotate else 0
    out = np.full((S * case.cache_rows + ar.GUARD_ROWS, d), UNWRITTEN, np.uint32)
    old = inp["kcache" if which == 1 else "vcache"]
    for s in range(S):
        cat = np.concatenate([old[s, :nc], inp["qkv"][s][:, which * d: (which + 1) * d]])
        if keep > 0:
            out[s * case.cache_rows: s * case.cache_rows + keep] = cat[kv - keep:].view(np.uint32)
    return out


def natural_columns(ctx, ctx_sigma):
    """ctx as the kernel stored it -> natural column order"""
    ctx = np.asarray(ctx, F32)
    return ctx[:, sigma_col(np.arange(ctx.shape[1]))] if ctx_sigma else ctx
