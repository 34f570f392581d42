"""Float64 torch restatement of a conformer block with limited-context (band) attention: torch_ref.conformer_block with the attention of
row i restricted to keys [max(0, i - left), min(T - 1, i + right)] and the position term taken from a local table of left + right + 1 rows
(row r = position i - j = left - r, the float formula of torch_ref.pos_emb).  Independent of the engine and of the oracle; the band
attention is evaluated in row chunks, so host memory stays bounded for utterances of tens of thousands of frames."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def pos_emb_local(left, right, d):
    pe = np.zeros((left + right + 1, d), np.float32)
    i = np.arange(0, d, 2, dtype=np.float32)
    div = np.exp(i * np.float32(-np.log(np.float32(10000.0)) / np.float32(d))).astype(np.float32)
    for r in range(left + right + 1):
        pos = np.float32(left - r)
        pe[r, 0::2] = np.sin(pos * div)
        pe[r, 1::2] = np.cos(pos * div)
    return pe


def band_attention(q, k, v, u, vb, P, left, right, chunk=512):
    """q, k, v [H][T][hd], u / vb [H][1][hd], P [H][left + right + 1][hd] -> ctx [H][T][hd]"""
    H, T, hd = q.shape
    offs = torch.arange(-left, right + 1)
    out = torch.empty_like(q)
    for c0 in range(0, T, chunk):
        I = torch.arange(c0, min(T, c0 + chunk))
        J = I[:, None] + offs[None, :]
        ok = (J >= 0) & (J < T)
        Jc = J.clamp(0, T - 1)
        kw, vw = k[:, Jc], v[:, Jc]                                   # [H][n][W][hd]
        qi = q[:, I]
        s = torch.einsum("hnd,hnwd->hnw", qi + u, kw) + (qi + vb) @ P.transpose(-1, -2)
        s = (s / math.sqrt(hd)).masked_fill(~ok[None], -math.inf)
        out[:, I] = torch.einsum("hnw,hnwd->hnd", torch.softmax(s, dim=-1), vw)
    return out


def conformer_block(W, layer, x, n_heads, left, right, stop_after=0):
    """x [B][T][d] (float) -> float64 numpy, one utterance per batch row (all T frames valid)"""
    q = f"encoder_.layers_.{layer}."
    w = lambda name: t64(W[q + name])
    x = t64(x)
    d = x.shape[-1]
    hd = d // n_heads

    def ln(name, v):
        return F.layer_norm(v, (d,), w(name + ".weight"), w(name + ".bias"), 1e-5)

    def ffn(name, v):
        h = F.linear(ln(name + ".norm_", v), w(name + ".fc1_.weight"), w(name + ".fc1_.bias"))
        return v + 0.5 * F.linear(F.silu(h), w(name + ".fc2_.weight"), w(name + ".fc2_.bias"))

    x = ffn("ffn1_", x)
    if stop_after == 1:
        return x.numpy()
    n = ln("attn_.norm_", x)
    B, T, _ = n.shape
    proj = lambda nm: F.linear(n, w(f"attn_.mha_.{nm}.weight"), w(f"attn_.mha_.{nm}.bias")).view(B, T, n_heads, hd).transpose(1, 2)
    qq, kk, vv = proj("q_proj"), proj("k_proj"), proj("v_proj")
    u = w("attn_.pos_bias_u_").view(n_heads, 1, hd)
    vb = w("attn_.pos_bias_v_").view(n_heads, 1, hd)
    P = F.linear(t64(pos_emb_local(left, right, d)), w("attn_.pos_proj_.weight")).view(-1, n_heads, hd).transpose(0, 1)
    o = torch.stack([band_attention(qq[b], kk[b], vv[b], u, vb, P, left, right) for b in range(B)]).transpose(1, 2).reshape(B, T, d)
    x = x + F.linear(o, w("attn_.mha_.out_proj.weight"), w("attn_.mha_.out_proj.bias"))
    if stop_after == 2:
        return x.numpy()
    n = ln("conv_.norm_", x).transpose(1, 2)
    y = F.glu(F.conv1d(n, w("conv_.pointwise_conv1_.weight"), w("conv_.pointwise_conv1_.bias")), dim=1)
    K = W[q + "conv_.depthwise_conv_.weight"].shape[-1]
    y = F.conv1d(y, w("conv_.depthwise_conv_.weight"), w("conv_.depthwise_conv_.bias"), padding=(K - 1) // 2, groups=d)
    y = F.batch_norm(y, w("conv_.batch_norm_.running_mean"), w("conv_.batch_norm_.running_var"), w("conv_.batch_norm_.weight"),
                     w("conv_.batch_norm_.bias"), training=False, eps=1e-5)
    y = F.conv1d(F.silu(y), w("conv_.pointwise_conv2_.weight"), w("conv_.pointwise_conv2_.bias"))
    x = x + y.transpose(1, 2)
    if stop_after == 3:
        return x.numpy()
    x = ffn("ffn2_", x)
    if stop_after == 4:
        return x.numpy()
    return ln("final_norm_", x).numpy()


def conformer_blocks(W, cfg, x, left, right, first_layer=0, n_layers=None):
    n_layers = cfg.num_layers - first_layer if n_layers is None else n_layers
    y = np.asarray(x, np.float64)
    for l in range(first_layer, first_layer + n_layers):
        y = conformer_block(W, l, y, cfg.num_heads, left, right)
    return y
