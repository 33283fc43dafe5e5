"""CPU-side checks of the contrastive forward (reference clip/model.py:356-370): the rounding points the cosine-logit kernel implements reproduce
the reference's own fp16 logits from its own fp16 features (fixtures of tests/golden/make_golden_contrastive.py), the one-rounding variant of the
scale does not, and pclip_cosine_logits_f16 refuses everything outside its envelope before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import golden, observe
from contrastive_ref import grade, l2norm_rows_ref, scaled_rows
from proto_clip_amd import _lib


def restated(g, scale):
    xn, yn = l2norm_rows_ref(torch.from_numpy(g["img_f16"])), l2norm_rows_ref(torch.from_numpy(g["txt_f16"]))
    return scaled_rows(xn, scale), yn


@pytest.mark.parametrize("tag", ["tiny", "small"])
def test_rounding_points_reproduce_the_reference_logits(tag):
    g = golden("contrastive_" + tag)
    s32 = float(np.exp(np.float32(g["logit_scale"])))
    s16 = float(np.float16(s32))                                   # the 0-dim logit_scale.exp() is cast to fp16 before it multiplies the fp16 tensor
    if tag == "tiny":
        assert s16 == 14.2890625 and abs(s32 - 1 / 0.07) < 1e-5
    xs, yn = restated(g, s16)
    ref = torch.from_numpy(g["logits_f16"])
    assert ref.shape == (int(g["n_img"]), int(g["n_txt"]))
    worst, differ = grade(ref, xs, yn)
    observe(f"contrastive {tag} (CPU restatement): |reference - exact| / tolerance", worst, 1.0)
    observe(f"contrastive {tag} (CPU restatement): share of elements != r16(exact)", differ, 1.0)
    assert worst <= 1.0, worst


def test_a_single_rounding_of_the_scale_does_not_reproduce_them():
    g = golden("contrastive_tiny")
    s32 = float(np.exp(np.float32(g["logit_scale"])))
    xs, yn = restated(g, s32)                                      # r16(s * x) with the fp32 scale
    worst, _ = grade(torch.from_numpy(g["logits_f16"]), xs, yn)
    assert worst > 1.0, worst


BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first


def call(a=BUF, lda=64, M=4, b=BUF, ldb=64, T=5, D=64, scale=1.0, flags=0, logits=BUF, ldl=8, argmax=None, topk_v=None, topk_i=None, k=0, ws=None,
         ws_bytes=0):
    return _lib.load().pclip_cosine_logits_f16(a, lda, M, b, ldb, T, D, scale, flags, logits, ldl, argmax, topk_v, topk_i, k, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, text", [
    (dict(a=None), b"null"),
    (dict(b=None), b"null"),
    (dict(logits=None), b"no output"),
    (dict(M=0), b"positive"),
    (dict(T=0), b"positive"),
    (dict(lda=56), b"lda"),
    (dict(lda=68), b"lda"),
    (dict(ldb=56), b"ldb"),
    (dict(ldb=76), b"ldb"),
    (dict(ldl=4), b"ldl"),
    (dict(ldl=12), b"ldl"),
    (dict(D=72, lda=72, ldb=72), b"multiple of 64"),
    (dict(D=4160, lda=4160, ldb=4160), b"multiple of 64"),
    (dict(D=0), b"multiple of 64"),
    (dict(k=17, T=40, ldl=40, topk_v=BUF, topk_i=BUF), b"k=17"),
    (dict(k=6, topk_v=BUF, topk_i=BUF), b"k=6"),
    (dict(k=-1), b"k=-1"),
    (dict(k=2, topk_v=BUF), b"top-k outputs"),
    (dict(k=0, topk_i=BUF), b"top-k outputs"),
    (dict(flags=4), b"flag"),
    (dict(flags=0x13), b"flag"),
    (dict(T=4097, ldl=4104, argmax=BUF), b"4096"),
    (dict(T=4097, ldl=4104, logits=None, k=5, topk_v=BUF, topk_i=BUF), b"4096"),
    (dict(a=ctypes.c_void_p(0x1008)), b"aligned"),
    (dict(flags=2), b"workspace"),
])
def test_argument_validation_precedes_any_launch(kw, text):
    assert call(**kw) == -1
    assert text in _lib.load().pclip_last_error(), _lib.load().pclip_last_error()


def test_workspace_is_sized_and_checked():
    lib = _lib.load()
    assert lib.pclip_workspace_bytes(_lib.OP_LOGITS, 50000, 1000, 512) >= 1000 * 512 * 2
    assert call(flags=2, ws=BUF, ws_bytes=16) == -3
    assert b"workspace" in lib.pclip_last_error()


def test_host_layer_refuses_what_the_kernel_cannot_take():
    from proto_clip_amd import PclipError, ops, utils
    x = torch.zeros(4, 64, dtype=torch.float16)
    with pytest.raises(PclipError):
        ops.cosine_logits(x, x, 1.0)                               # CPU tensors
    with pytest.raises(PclipError):
        ops.cosine_logits(x.float(), x, 1.0)
    with pytest.raises(PclipError):
        utils.clip_logits(x, x.float())
    with pytest.raises(PclipError, match="matches neither"):           # the shape check, before anything looks at the device
        utils.clip_zero_shot(x, torch.zeros(5, 32, dtype=torch.float16))
    sq = torch.zeros(64, 64, dtype=torch.float16)
    with pytest.raises(PclipError, match=r"is not \[N, D\]"):
        utils.clip_logits(x, torch.zeros(64, 5, dtype=torch.float16), layout="nd")
    with pytest.raises(PclipError, match=r"is not \[D, N\]"):
        utils.clip_zero_shot(x, torch.zeros(5, 64, dtype=torch.float16), layout="dn")
    with pytest.raises(PclipError, match="layout"):
        utils.clip_logits(x, sq, layout="rows")
    assert math.isclose(float(torch.tensor(math.log(1 / 0.07)).exp().half()), 14.2890625)
