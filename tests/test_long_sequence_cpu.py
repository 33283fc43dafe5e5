"""Long-sequence attention (csrc/pclip_attention_long.hip) and the ViT-L/14@336px backbone, host side: the new entry's argument
validation refuses before any launch (fake pointers, never dereferenced), the routing by L, and build_model's inference of the
336-px architecture from a state dict."""
import ctypes

import pytest

from proto_clip_amd import _lib


def _call(lib, ptr, B=1, L=577, Lq=577, H=2, dh=64, causal=0, ldq=None, ldkv=None, k_off=None, v_off=None, qbs=None):
    W = H * 64
    ldq = 3 * W if ldq is None else ldq
    ldkv = 3 * W if ldkv is None else ldkv
    k_off = W if k_off is None else k_off
    v_off = 2 * W if v_off is None else v_off
    qbs = L * 3 * W if qbs is None else qbs
    return lib.pclip_attention_long_q_f16(ptr, ldq, qbs, ptr, ldkv, k_off, v_off, ptr, B, L, Lq, H, dh, causal, None)


@pytest.mark.parametrize("kw,msg", [(dict(L=4097, Lq=4097), b"L <= 4096"), (dict(causal=1), b"causal"), (dict(dh=32), b"head dim"),
                                    (dict(Lq=578), b"Lq <= L"), (dict(Lq=0), b"Lq <= L"), (dict(H=0), b"bad B"),
                                    (dict(ldq=3 * 128 + 4), b"multiples of 8"), (dict(k_off=132), b"multiples of 8"),
                                    (dict(qbs=577 * 384 + 2), b"multiples of 8"), (dict(v_off=3 * 128), b"row layout"),
                                    (dict(ldkv=128), b"row layout")])
def test_long_attention_argument_validation(kw, msg):
    lib = _lib.load()
    buf = ctypes.c_void_p(0x1000)      # never dereferenced: validation rejects first
    assert _call(lib, buf, **kw) == -1
    assert msg in lib.pclip_last_error(), lib.pclip_last_error()
    assert lib.pclip_attention_long_q_f16(None, 384, 577 * 384, buf, 384, 128, 256, buf, 1, 577, 577, 2, 64, 0, None) == -1
    assert b"null pointer" in lib.pclip_last_error()
    assert _call(lib, buf, B=0) == 0                   # an empty batch launches nothing
    assert lib.pclip_attention_f16(buf, buf, 1, 577, 2, 64, 0, None) == -1      # the resident-K/V entries keep their bound
    assert lib.pclip_attention_q_f16(buf, 384, 577 * 384, buf, 384, 128, 256, buf, 1, 577, 577, 2, 64, 0, None) == -1


def test_long_attention_symbol_is_declared_and_bound():
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "pclip_attention_long_q_f16(" in open(os.path.join(repo, "include", "pclip.h")).read()
    assert "pclip_attention_long_q_f16" in _lib.EXPORTED_SYMBOLS
    assert _lib.load().pclip_abi_version() == 1


def test_attention_route_follows_sequence_length(monkeypatch):
    """ops picks the entry by L alone: <= 288 the resident-K/V entries (as before), longer the streamed one, for the fused and the
    first-queries forms alike."""
    import torch
    from proto_clip_amd import ops
    calls = []

    class Rec:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a[8:11])) or 0
    monkeypatch.setattr(_lib, "load", lambda: Rec())
    monkeypatch.setattr(ops, "require_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(ops, "ptr", lambda t: None)
    x = torch.empty(0)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: x)
    for L in (257, 288, 289, 577):
        ops.attention(x, 2, L, 4)
        ops.attention_first_queries(x, x, 2, L, 1, 4)
    names = [c[0] for c in calls]
    assert names == ["pclip_attention_f16", "pclip_attention_q_f16"] * 2 + ["pclip_attention_long_q_f16"] * 4
    assert calls[4][1] == (2, 289, 289) and calls[7][1] == (2, 577, 1)


def test_build_model_infers_336px():
    from proto_clip_amd.clip import available_models
    from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict
    kw = BACKBONES["ViT-L/14@336px"]
    assert kw == dict(BACKBONES["ViT-L/14"], image_resolution=336)
    sd = random_state_dict(seed=3, **kw)
    assert sd["visual.positional_embedding"].shape[0] == 577        # 24 x 24 patches + the class token
    m = build_model(sd)
    assert m.visual.input_resolution == 336 and m.visual.patch_size == 14 and m.visual.width == 1024
    assert "ViT-L/14@336px" not in available_models()
