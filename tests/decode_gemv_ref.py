"""Float64 reference of the decode loop's skinny products (kernels/decode_gemv_bf16.hip; kernels.hpp SkinnyArgs) with a per-element error
bound, the shape list the GPU test runs (tests/test_gpu_decode_gemv.py) and a numpy emulation of the kernel's arithmetic that the CPU self-test
(tests/test_decode_gemv_ref.py) holds the bound against -- clean, and with planted faults.

The three epilogues, from the operands the kernel sees (X, W, X2, W2 bf16-exact: no operand-rounding term; everything else fp32, taken exactly):

    bias:        out[b][n] = X[b] . W[n] (+ bias[n])                                                                   fp32
    activation:  p = X[b] . W[n] (+ bias[n]) -> pp_out (fp32);  z = relu(ep[r0_b + min(t_b, Tb_b - 1)][n] + p)          bf16
    cell:        gate_g = gi_g + X[b] . W[g Hp + j],  gi = the g1 row gi_row[b]  or  X2[b] . W2[g Hp + j] + bias2[g Hp + j];  g = i, f, g, o
                 c' = sigmoid(f) c + sigmoid(i) tanh(g)   (fp32);   h' = sigmoid(o) tanh(c')                             bf16

Error bound (u = 2^-24; every |.| of the reference value).

1. Product.  The form the project holds its bf16 MFMA products to (tests/test_gpu_bf16.py): B_p = 2e-6 (|X| |W|^T + |bias|) + 1e-6.  bf16 x bf16
   products are exact in fp32, so the error is the fp32 accumulation's: at most (K / 32 + 5) roundings of partial sums below sum|x w| when a
   32-k block is summed as a tree and the blocks as a chain -- (K / 32 + 5) u <= 37 u = 2.2e-6 at K = 1024 in the worst case with every rounding
   at its extreme and a common sign, 2e-6 = 33.5 u; K <= 1024 here, and the form is the one every bf16 product of the project is held to.
2. Activation.  s = fl(ep + p): B_s = B_p + u (|s| + B_p).  relu is 1-Lipschitz: B_z = B_s.  pp_out is compared with B_p.
3. Outputs rounded to bf16 (z, h').  A stored value is admissible when it is the RNE bf16 rounding of SOME value inside ref +- bound.  That is
   evaluated exactly (bf16_slack): the reals that round to `got` reach half way to its bf16 neighbours, so got is admissible when
   |got - ref| - (half the gap between got and its neighbour on ref's side) <= bound.  (A closed form would be bound + 2^-8 |v|: bf16 keeps 8
   significant bits, its unit roundoff is 2^-8.  With 2^-9 in its place a correctly rounded store of the exact value already fails, which the
   emulation of test_decode_gemv_ref.py shows at once; the exact test is tighter than either closed form.)
4. Cell.  oracle/tolerance.py holds no constant for the device sigmoid / tanh (pk_devmath.h dsigmoidf / dtanhf), so the reference evaluates them with
   the oracle's own math_v -- bit for bit the device functions (tests/test_gpu_primitives.py) -- at the fp32 rounding of its float64 argument.  The
   kernel evaluates the SAME function at a neighbouring argument: |F(a) - F(b)| <= |f(a) - f(b)| + 2 E_FN <= L |a - b| + 2 E_FN with f the true
   function, L its Lipschitz constant (sigmoid 1/4, tanh 1) and E_FN = 2^-22 >= max |F - f| (both functions are bounded by 1 and a few ulp
   accurate; test_decode_gemv_ref.py checks E_FN against float64 over a dense grid of [-20, 20]).  With the layer-0 form the gate is
   fl(gi + acc): B_gate = 2e-6 (|X| |W|^T + |gi|) + 1e-6 + 2 u |gate| (one rounding of the sum, one of the reference's own fp32 argument); with
   the fused upper-layer form gi = fl(acc2 + bias2): B_gate = 2e-6 (|X| |W|^T + |X2| |W2|^T + |bias2|) + 2e-6 + 3 u (|gate| + |gi|).
       B_i = B_gate_i / 4 + 2 E_FN,  B_f, B_o alike,  B_g = B_gate_g + 2 E_FN
       t1 = fl(f c):  B_t1 = B_f |c| + u |t1|         t2 = fl(i g):  B_t2 = B_i |g| + B_g |i| + B_i B_g + u |t2|
       c' = fl(t1 + t2):  B_c = (B_t1 + B_t2)(1 + u) + u |c'|
       T = tanh(c'):  B_T = B_c + 2 E_FN + u |c'| (the reference's fp32 argument)
       h' = fl(o T):  B_h = B_o |T| + B_T |o| + B_o B_T + u |h'|,  then 3. for the bf16 store.
"""
import numpy as np

U32 = 2.0 ** -24
E_FN = 2.0 ** -22
FILL32, FILL16 = 0x7FC5A5A5, 0x7FC5


def bf16_bits(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16(x):
    """round to the nearest bf16 (ties to even), returned as float32"""
    return bf16_widen(bf16_bits(x))


# ---- the shape list -------------------------------------------------------------------------------------------------------------------------
# (epi, B, N or Hp, K, need pattern or None, options).  Every K of {32, 64, 96, 128, 256, 288, 640, 1024}, every B of {1, 15, 16, 17, 32, 63, 64, 65, 130}
# and every column count of the issue's list appears with every epilogue; the kernel instantiation <EPI, MODE, CHK> a case runs follows from it
# (instantiation() below): MODE 1 = flags with B <= 16, MODE 2 = flags with B > 16, MODE 0 = no flags; CHK = column-tile count not a multiple of 8.
_SKEL = [(1, 0, 32, "all"), (15, 1, 64, "alt"), (16, 2, 96, "random"), (17, 3, 128, "last"), (32, 2, 256, "tile"), (63, 1, 288, None),
         (64, 2, 640, None), (65, 3, 1024, "random"), (130, 0, 640, "row0"), (16, 1, 64, "none"), (130, 2, 32, "none")]
_COLS = {"bias": [16, 70, 128, 1030], "act": [16, 70, 128, 1030], "cell": [32, 20, 64, 36]}


def _cases():
    out = []
    for epi in ("bias", "act", "cell"):
        for i, (B, ci, K, need) in enumerate(_SKEL):
            out.append(dict(epi=epi, B=B, N=_COLS[epi][ci], K=K, need=need, idx=i))
    out[2 * len(_SKEL) + 7]["N"] = 640                                           # cell, B 65: the 110m / 600m shape Hp = K = 640 (160 tiles)
    out[2 * len(_SKEL) + 7]["K"] = 640
    out.append(dict(epi="cell", B=65, N=36, K=1024, need="random", idx=11))      # (K = 1024 with the cell, moved from the line above)
    out.append(dict(epi="bias", B=17, N=8198, K=64, need="all", idx=12))         # the 600m heads' tail
    out.append(dict(epi="bias", B=2048, N=16, K=32, need="random", idx=13))      # eight flags per thread in the row-list scan
    out.append(dict(epi="act", B=2100, N=16, K=32, need=None, idx=14))           # 33 workgroup rows
    out.append(dict(epi="cell", B=2048, N=20, K=32, need="alt", idx=15))
    out.append(dict(epi="cell", B=9, N=640, K=96, need=None, idx=17))            # MODE 0 under one row tile, with the fused projection
    return out


CASES = _cases()


def case_id(c):
    return f"{c['epi']}-B{c['B']}-N{c['N']}-K{c['K']}-{c['need'] or 'every'}"


def instantiation(c):
    """(EPI, MODE, CHK) of skinny_gemm_bf16_kernel the launcher picks for this case (launch_skinny_bf16_epi)"""
    tiles = c["N"] // 4 if c["epi"] == "cell" else (c["N"] + 15) // 16
    mode = 0 if c["need"] is None else (1 if c["B"] <= 16 else 2)
    return c["epi"], mode, tiles % 8 != 0


def need_flags(pattern, B, rng):
    if pattern is None:
        return None
    f = np.zeros(B, np.int32)
    if pattern == "all":
        f[:] = 1
    elif pattern == "row0":
        f[0] = 1
    elif pattern == "last":
        f[-1] = 1
    elif pattern == "alt":
        f[::2] = 1
    elif pattern == "tile":                                   # one set row per 16-row tile, at a different place in each
        for t0 in range(0, B, 16):
            f[min(B - 1, t0 + (5 * (t0 // 16) + 3) % 16)] = 1
    elif pattern == "random":
        f[:] = rng.random(B) < 0.45
        f[0] = 1
        if f.sum() % 16 == 0:
            f[np.flatnonzero(f == 0)[0]] = 1
    return f


def make_case(c, period=0):
    """Seeded operands of one case (period > 0: the rows repeat with that period, the flags do not)."""
    rng = np.random.default_rng(1000 * c["idx"] + 7 * c["B"] + c["N"] + c["K"] + {"bias": 0, "act": 1, "cell": 2}[c["epi"]])
    epi, B, N, K, i = c["epi"], c["B"], c["N"], c["K"], c["idx"]
    rows = N * 4 if epi == "cell" else N
    rep = (np.arange(B) % period) if period else np.arange(B)
    o = dict(c)
    o["X"] = bf16(rng.standard_normal((B, K)))[rep]
    o["W"] = bf16(rng.standard_normal((rows, K)) / np.sqrt(K))
    o["need_flags"] = need_flags(c["need"], B, rng)
    if epi == "bias":
        o["bias"] = (0.3 * rng.standard_normal(N)).astype(np.float32) if i % 3 != 1 else None
    elif epi == "act":
        o["bias"] = (0.3 * rng.standard_normal(N)).astype(np.float32) if i % 2 == 0 else None
        o["want_pp"] = i % 3 != 0
        ragged = i % 2 == 1
        T = 5
        if ragged:
            Tb = (1 + (np.arange(B) * 3 + i) % 6).astype(np.int32)[rep]
            row0 = (np.concatenate([[0], np.cumsum(Tb)[:-1]]) + 2).astype(np.int32)     # (two unused rows in front)
            ep_rows = int(row0[-1] + Tb[-1]) + 1
            o["Tb"], o["row0"] = Tb, row0
        else:
            Tb, row0, ep_rows = np.full(B, T, np.int32), (np.arange(B) * T).astype(np.int32), B * T
            o["Tb"] = o["row0"] = None
        o["T"] = T
        ep = rng.standard_normal((ep_rows, N)).astype(np.float32)
        if period:                                            # a copy reads its own enc_proj rows: make them equal to the original's
            for b in range(B):
                ep[row0[b]: row0[b] + Tb[b]] = ep[row0[rep[b]]: row0[rep[b]] + Tb[rep[b]]]
        o["ep"] = ep
        kind = np.arange(B)[rep] % 5                              # frame pointer: 0, the last frame, one and four past the end (clamped), anywhere
        o["t"] = np.where(kind == 0, 0, np.where(kind == 1, Tb - 1, np.where(kind == 2, Tb, np.where(kind == 3, Tb + 3, (7 * np.arange(B)[rep]) % Tb)))).astype(np.int32)
        o["Tb_eff"], o["row0_eff"] = Tb, row0
    else:
        o["c"] = rng.standard_normal((B, N)).astype(np.float32)[rep]
        o["fused"] = i % 2 == 1
        if o["fused"]:
            o["X2"] = bf16(rng.standard_normal((B, K)))[rep]
            o["W2"] = bf16(rng.standard_normal((rows, K)) / np.sqrt(K))
            o["bias2"] = (0.3 * rng.standard_normal(rows)).astype(np.float32)
        else:
            V = 11
            o["gi"] = rng.standard_normal((V, rows + 3)).astype(np.float32)              # (row stride wider than 4 Hp)
            o["gi_row"] = ((np.arange(B) * 7 + 3) % V)[::-1].astype(np.int32)[rep]       # repeated, out-of-order token ids
    return o


def checked_rows(o):
    f = o["need_flags"]
    return np.arange(o["B"]) if f is None else np.flatnonzero(f)


# ---- float64 reference ----------------------------------------------------------------------------------------------------------------------
def product(X, W, bias=None):
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    val, mag = X @ W.T, np.abs(X) @ np.abs(W).T
    if bias is not None:
        val, mag = val + np.asarray(bias, np.float64), mag + np.abs(np.asarray(bias, np.float64))
    return val, mag


def ep_rows_of(o, shift=0, clamp=True):
    t, Tb, r0 = o["t"].astype(np.int64), o["Tb_eff"].astype(np.int64), o["row0_eff"].astype(np.int64)
    tt = np.minimum(t, Tb - 1) if clamp else t
    return (r0 + tt + shift) % o["ep"].shape[0]


def reference(o, math_v=None):
    """-> dict name -> (value, bound, rounded_to_bf16) over ALL rows of the batch (float64 [B][N])"""
    epi = o["epi"]
    if epi == "bias":
        val, mag = product(o["X"], o["W"], o["bias"])
        return {"out": (val, 2e-6 * mag + 1e-6, False)}
    if epi == "act":
        p, mag = product(o["X"], o["W"], o["bias"])
        Bp = 2e-6 * mag + 1e-6
        s = o["ep"][ep_rows_of(o)].astype(np.float64) + p
        Bs = Bp + U32 * (np.abs(s) + Bp)
        return {"pp": (p, Bp, False), "out": (np.maximum(s, 0.0), Bs, True)}
    Hp, B = o["N"], o["B"]
    acc, mag = product(o["X"], o["W"])
    if o["fused"]:
        gi, mag2 = product(o["X2"], o["W2"], o["bias2"])
        gate = gi + acc
        Bg = 2e-6 * (mag + mag2) + 2e-6 + 3 * U32 * (np.abs(gate) + np.abs(gi))
    else:
        gi = o["gi"][o["gi_row"], : 4 * Hp].astype(np.float64)
        gate = gi + acc
        Bg = 2e-6 * (mag + np.abs(gi)) + 1e-6 + 2 * U32 * np.abs(gate)
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    sig = lambda x: math_v("sigmoid", f32(x)).astype(np.float64)
    tanh = lambda x: math_v("tanh", f32(x)).astype(np.float64)
    g4 = gate.reshape(B, 4, Hp)
    b4 = Bg.reshape(B, 4, Hp)
    i_, f_, g_, o_ = sig(g4[:, 0]), sig(g4[:, 1]), tanh(g4[:, 2]), sig(g4[:, 3])
    Bi, Bf, Bgg, Bo = b4[:, 0] / 4 + 2 * E_FN, b4[:, 1] / 4 + 2 * E_FN, b4[:, 2] + 2 * E_FN, b4[:, 3] / 4 + 2 * E_FN
    c = o["c"].astype(np.float64)
    t1, t2 = f_ * c, i_ * g_
    Bt1 = Bf * np.abs(c) + U32 * np.abs(t1)
    Bt2 = Bi * np.abs(g_) + Bgg * np.abs(i_) + Bi * Bgg + U32 * np.abs(t2)
    cn = t1 + t2
    Bc = (Bt1 + Bt2) * (1 + U32) + U32 * np.abs(cn)
    T = tanh(cn)
    BT = Bc + 2 * E_FN + U32 * np.abs(cn)
    h = o_ * T
    Bh = Bo * np.abs(T) + BT * np.abs(o_) + Bo * BT + U32 * np.abs(h)
    return {"cn": (cn, Bc, False), "out": (h, Bh, True)}


def bf16_slack(got, ref):
    """got: bf16-exact values.  Half the distance from got to the neighbouring bf16 value on ref's side: every real closer to got than that rounds (RNE) to got."""
    got = np.ascontiguousarray(got, np.float32)
    mag = (got.view(np.uint32) >> 16).astype(np.int64) & 0x7FFF
    a = np.abs(got.astype(np.float64))
    up = bf16_widen((mag + 1).astype(np.uint16)).astype(np.float64)
    down = bf16_widen(np.maximum(mag - 1, 0).astype(np.uint16)).astype(np.float64)
    outward = np.where(np.signbit(got), -ref, ref) > a                      # ref lies further from zero than got, on got's side
    return np.where(outward, up - a, a - down) / 2


def excess(got, ref, rounded):
    """how far the kernel's fp32 value must have been from ref at least: |got - ref|, less -- for a bf16 output -- what the store's rounding explains"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    return np.maximum(d - bf16_slack(got, ref), 0.0) if rounded else d


def worst_ratio(got, ref, bound, rounded):
    """max over the elements of excess / bound; <= 1: every element is admissible"""
    return float((excess(got, ref, rounded) / bound).max()) if ref.size else 0.0


# ---- numpy emulation of the kernel's arithmetic (self-test only) ---------------------------------------------------------------------------
FAULTS = ("drop_block", "swap_blocks", "tile_neighbour", "row_next", "gate_perm", "c_for_cnew", "ep_next_frame", "no_clamp")


def fault_applies(fault, o):
    epi, nblk = o["epi"], o["K"] // 32
    rows = checked_rows(o)
    if rows.size == 0:
        return False
    if fault == "swap_blocks":
        return nblk >= 2
    if fault == "tile_neighbour":
        return o["N"] >= (8 if epi == "cell" else 32)
    if fault == "row_next":
        return o["B"] >= 2
    if fault in ("gate_perm", "c_for_cnew"):
        return epi == "cell"
    if fault == "ep_next_frame":
        return epi == "act"
    if fault == "no_clamp":
        return epi == "act" and bool((o["t"][rows] >= o["Tb_eff"][rows]).any())
    return True


def _chain(X, W, fault, o):
    """fp32 accumulation in blocks of 32 k (a block's 32 exact products summed, rounded once, added to the chain)"""
    X, W = np.asarray(X, np.float32).copy(), np.asarray(W, np.float32).copy()
    K, nblk = X.shape[1], X.shape[1] // 32
    if fault == "swap_blocks":
        W[:, 0:32], W[:, 32:64] = W[:, 32:64].copy(), W[:, 0:32].copy()
    if fault == "tile_neighbour":
        if o["epi"] == "cell":
            Hp = o["N"]
            for g in range(4):
                W[g * Hp: g * Hp + 4] = W[g * Hp + 4: g * Hp + 8]
        else:
            W[0:16] = W[16:32]
    if fault == "row_next":
        b = int(checked_rows(o)[0])
        X[b] = X[b + 1 if b + 1 < X.shape[0] else b - 1]
    acc = np.zeros((X.shape[0], W.shape[0]), np.float32)
    for blk in range(nblk):
        if fault == "drop_block" and blk == nblk // 2:
            continue
        k = slice(32 * blk, 32 * blk + 32)
        acc = (acc + (X[:, k].astype(np.float64) @ W[:, k].astype(np.float64).T).astype(np.float32)).astype(np.float32)
    return acc


def emulate(o, math_v=None, fault=None):
    """-> dict name -> float32 [B][N] (z / h' already rounded to bf16), the kernel's operation order"""
    epi = o["epi"]
    acc = _chain(o["X"], o["W"], fault, o)
    if epi == "bias":
        return {"out": acc + o["bias"] if o["bias"] is not None else acc}
    if epi == "act":
        p = acc + o["bias"] if o["bias"] is not None else acc
        e = o["ep"][ep_rows_of(o, shift=1 if fault == "ep_next_frame" else 0, clamp=fault != "no_clamp")]
        s = (e + p).astype(np.float32)
        return {"pp": p, "out": bf16(np.maximum(s, np.float32(0)))}
    Hp, B = o["N"], o["B"]
    if o["fused"]:
        gi = (_chain(o["X2"], o["W2"], fault, o) + o["bias2"]).astype(np.float32)
    else:
        gi = o["gi"][o["gi_row"], : 4 * Hp]
    g4 = (gi + acc).astype(np.float32).reshape(B, 4, Hp)
    order = (1, 0, 2, 3) if fault == "gate_perm" else (0, 1, 2, 3)
    ig, fg = math_v("sigmoid", g4[:, order[0]]), math_v("sigmoid", g4[:, order[1]])
    gg, og = math_v("tanh", g4[:, order[2]]), math_v("sigmoid", g4[:, order[3]])
    t1, t2 = (fg * o["c"]).astype(np.float32), (ig * gg).astype(np.float32)
    cn = (t1 + t2).astype(np.float32)
    h = (og * math_v("tanh", o["c"] if fault == "c_for_cnew" else cn)).astype(np.float32)
    return {"cn": cn, "out": bf16(h)}
