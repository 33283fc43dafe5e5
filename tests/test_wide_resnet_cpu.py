"""RN50x4 / RN50x16, host side: build_model infers exactly their BACKBONES entries, clip.load reads RN50x4.pt / RN50x16.pt by name from
download_root (the reference's file names), a missing checkpoint is the usual "downloading is disabled" error, and available_models()
keeps its five names; the relaxed preconditions refuse before any launch (fake pointers, never dereferenced)."""
import ctypes

import pytest
import torch

from proto_clip_amd import _lib
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict


def _inferred(m):
    v = m.visual
    return dict(embed_dim=v.output_dim, image_resolution=v.input_resolution,
                vision_layers=tuple(len(getattr(v, f"layer{i}")) for i in (1, 2, 3, 4)), vision_width=v.conv3.weight.shape[0],
                vision_patch_size=None, context_length=m.context_length, vocab_size=m.vocab_size, transformer_width=m.transformer.width,
                transformer_heads=m.transformer_heads, transformer_layers=m.transformer.layers)


@pytest.mark.parametrize("name,res,pool", [("RN50x4", 288, 82), ("RN50x16", 384, 145)])
def test_build_model_infers_wide_resnets(name, res, pool):
    kw = BACKBONES[name]
    sd = random_state_dict(seed=3, **kw)
    assert sd["visual.attnpool.positional_embedding"].shape[0] == pool
    m = build_model(sd)
    assert _inferred(m) == kw
    assert m.visual.heads * 64 == kw["vision_width"] * 32
    assert m.visual.chunk == 256


def test_clip_load_rn50x4_by_name_on_cpu(tmp_path):
    from proto_clip_amd import clip
    sd = random_state_dict(seed=5, **BACKBONES["RN50x4"])
    torch.save(sd, tmp_path / "RN50x4.pt")
    m, pre = clip.load("RN50x4", device="cpu", download_root=str(tmp_path))
    assert pre.n_px == 288 and _inferred(m) == BACKBONES["RN50x4"]
    assert torch.equal(m.visual.layer1[0].conv1.weight, sd["visual.layer1.0.conv1.weight"].to(m.visual.layer1[0].conv1.weight.dtype))


def test_clip_load_missing_rn50x16_is_refused(tmp_path):
    from proto_clip_amd import clip
    with pytest.raises(RuntimeError, match="RN50x16.pt not found and downloading is disabled"):
        clip.load("RN50x16", device="cpu", download_root=str(tmp_path))


def test_available_models_unchanged():
    from proto_clip_amd.clip import available_models
    assert available_models() == ["RN50", "RN101", "ViT-B/32", "ViT-B/16", "ViT-L/14"]


@pytest.mark.parametrize("call,msg", [
    (lambda lib, p: lib.pclip_gemm_f16(p, 88, p, 88, p, 64, 16, 64, 84, None, 0, None, None), b"K=84 must be a multiple of 8"),
    (lambda lib, p: lib.pclip_gemm_bn_f16(p, 88, p, 88, p, 64, 16, 64, 84, p, p, 1, None), b"K=84 must be a multiple of 8"),
    (lambda lib, p: lib.pclip_gemm_bn_res_f16(p, 80, p, 80, p, 80, 16, 80, 80, p, p, p, None), b"N=80 a multiple of 64"),
    (lambda lib, p: lib.pclip_conv3x3_bn_f16(p, p, p, 1, 5, 5, 36, 40, p, p, 1, p, None), b"Cin=36"),
    (lambda lib, p: lib.pclip_conv3x3_bn_f16(p, p, p, 1, 5, 5, 40, 20, p, p, 1, p, None), b"Cout=20"),
])
def test_tail_preconditions_refuse_before_launch(call, msg):
    lib = _lib.load()
    assert call(lib, ctypes.c_void_p(0x1000)) == -1
    assert msg in lib.pclip_last_error(), lib.pclip_last_error()
