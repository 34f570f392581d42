"""The MXFP8 feed-forward mode through the engine (pk_model_set_ffn_mxfp8) on a small random-init bf16-mode model: refused on an fp32 model; on, it
changes the encoder output of a batch above the small-M bf16 kernel's rows by no more than twice what a float64 emulation of the format shows on the
same weights and input; off again, and on a batch inside the small-M range, the bf16 mode's bits."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

import gpu_common as G
import mxfp8_ref as R
import torch_ref
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu
PK_ERR_UNSUPPORTED = -7


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    cfg = G.tiny(hidden_size=256, ffn_intermediate=512, num_heads=4, name="tiny-mx")
    W = synth.synth_weights(cfg, seed=77)
    wp = os.path.join(str(tmp_path_factory.mktemp("mx")), "tiny_mx.safetensors")
    synth.save_weights(wp, W)
    g32, g16 = capi.Model(wp, cfg, device=0), capi.Model(wp, dataclasses.replace(cfg, gemm_bf16=True), device=0)
    yield cfg, W, g32, g16
    g32.close()
    g16.close()


def emulation(W, cfg, x, mx):
    """torch_ref's blocks in the bf16 mode; mx: the operands of the four feed-forward linears (the only [f][d] / [d][f] weights) through the reference
    quantiser, and those products in float64"""
    f, d = cfg.ffn_intermediate, cfg.hidden_size

    def linear(v, w, b=None):
        if not mx or sorted(w.shape) != [d, f]:
            return torch.nn.functional.linear(v, w, b)
        a = torch.from_numpy(R.qdq(v.reshape(-1, v.shape[-1]).numpy())).reshape(v.shape)
        return torch.nn.functional.linear(a, torch.from_numpy(R.qdq(w.numpy())), b.double()).float()
    shim = types.SimpleNamespace(**{k: getattr(torch.nn.functional, k) for k in ("layer_norm", "silu", "pad", "glu", "conv1d", "batch_norm")}, linear=linear)
    pe, real = torch_ref.pos_emb(x.shape[1], d), torch_ref.F
    torch_ref.F = shim
    try:
        for l in range(cfg.num_layers):
            x = torch_ref.conformer_block(W, l, x, pe, cfg.num_heads, bf16=True)
    finally:
        torch_ref.F = real
    return x


def test_mode_on_off_and_small_batches(models):
    cfg, W, g32, g16 = models
    with pytest.raises(capi.PkError) as e:
        g32.set_ffn_mxfp8(True)
    assert e.value.code == PK_ERR_UNSUPPORTED and not g32.ffn_mxfp8()
    rng = np.random.default_rng(3)
    big, small = (rng.standard_normal((1, T, cfg.hidden_size)).astype(np.float32) for T in (130, 128))   # rows just above / at the small-M limit
    off = [g16.conformer_blocks(v) for v in (big, small)]
    g16.set_ffn_mxfp8(True)
    assert g16.ffn_mxfp8()
    on = [g16.conformer_blocks(v) for v in (big, small)]
    g16.set_ffn_mxfp8(False)
    again = [g16.conformer_blocks(v) for v in (big, small)]
    assert np.isfinite(on[0]).all() and not np.array_equal(on[0], off[0]), "the mode changed nothing"
    assert np.array_equal(G.bits(on[1]), G.bits(off[1])), "a small-M batch must keep the bf16 mode's bits"
    assert all(np.array_equal(G.bits(a), G.bits(b)) for a, b in zip(again, off)), "mode off again: the bf16 mode's bits"
    e16, emx = emulation(W, cfg, big, False), emulation(W, cfg, big, True)
    dist = np.abs(on[0] - off[0]).max() / np.abs(off[0]).max()
    dist_emu = np.abs(emx - e16).max() / np.abs(e16).max()
    print(f"MXFP8 vs bf16 feed-forwards, max|diff| / max|x|: GPU {dist:.3e}, float64 emulation {dist_emu:.3e}")
    assert dist <= 2.0 * dist_emu
