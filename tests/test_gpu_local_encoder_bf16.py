"""The bf16 band attention kernel through the engine (pk_model_set_local_attention_bf16) on small random-init bf16-mode models, head size 64
(the tiny bf16 config of tests/test_gpu_bf16.py) and 128: on, the encoder stays within the gemm_bf16 mode's standing 2e-2 max|x| of the fp32
model's local-mode output and is not the fp32 band kernel's bits; ragged clips are bit-identical to their single-clip runs; off again, the
bits of a model that never had it on; an fp32 model refuses it."""
import dataclasses

import numpy as np
import pytest

import gpu_common as G
from parakeet_cpp_amd import capi, synth

pytestmark = pytest.mark.gpu
PK_ERR_UNSUPPORTED = -7
WINDOW = (64, 64)


def _feats(B, Tm, F, seed):
    return np.random.default_rng(seed).standard_normal((B, Tm, F)).astype(np.float32)


@pytest.fixture(scope="module", params=[64, 128], ids=["hd64", "hd128"])
def models(request, tmp_path_factory):
    """(config, bf16 model with the switch to test, bf16 model that never sets it, fp32 model), all with the window set"""
    kw = {} if request.param == 64 else {"num_heads": 1}
    cfg = G.tiny(subsampling_channels=64, gemm_bf16=True, name=f"tiny-bf16-hd{request.param}", **kw)
    assert cfg.hidden_size // cfg.num_heads == request.param
    wp = str(tmp_path_factory.mktemp("loc16") / "w.safetensors")
    synth.save_weights(wp, synth.synth_weights(cfg, seed=42))
    ms = [capi.Model(wp, cfg, device=0), capi.Model(wp, cfg, device=0), capi.Model(wp, dataclasses.replace(cfg, gemm_bf16=False), device=0)]
    for m in ms:
        m.set_attention_context(*WINDOW)
    yield (cfg, *ms)
    for m in ms:
        m.close()


def test_on_within_bound_of_fp32_local_and_off_restores_the_bits(models):
    cfg, g16, fresh, g32 = models
    f = _feats(2, 4001, cfg.mel_bins, 8)
    want32, off = g32.encode(f), fresh.encode(f)
    g16.set_local_attention_bf16(True)
    assert g16.local_attention_bf16() and not fresh.local_attention_bf16()
    try:
        on = g16.encode(f)
    finally:
        g16.set_local_attention_bf16(False)
    assert not g16.local_attention_bf16()
    err, mx = np.abs(on - want32).max(), np.abs(want32).max()
    print(f"\n{cfg.name}: max |bf16 band - fp32 local| {err:.3e} = {err / mx:.3e} max|x|; switch off {np.abs(off - want32).max() / mx:.3e}", end="")
    assert err <= 2e-2 * mx
    assert not np.array_equal(on, off), "the switch changed nothing: the bf16 band kernel did not run"
    G.assert_bits_equal(g16.encode(f), off, "switch off again vs a model that never had it on")


def test_ragged_clips_bit_identical_to_single_runs(models):
    cfg, g16, fresh, g32 = models
    feats = [_feats(1, n, cfg.mel_bins, 40 + i)[0] for i, n in enumerate((4001, 301))]
    g16.set_local_attention_bf16(True)
    try:
        rag = g16.encode_ragged(feats)
        for i, f in enumerate(feats):
            G.assert_bits_equal(rag[i], g16.encode(f[None])[0], f"{cfg.name}: ragged clip {i} vs alone")
    finally:
        g16.set_local_attention_bf16(False)


def test_fp32_model_refuses(models):
    cfg, g16, fresh, g32 = models
    with pytest.raises(capi.PkError) as e:
        g32.set_local_attention_bf16(True)
    assert e.value.code == PK_ERR_UNSUPPORTED and not g32.local_attention_bf16()
