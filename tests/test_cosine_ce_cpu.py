"""The float64 helper of the cosine cross-entropy kernels (tests/cosine_ce_ref.py) against central finite differences, and what pclip_cosine_ce_f16 /
pclip_cosine_ce_backward_f16 can be asked without a GPU: the declarations, the exports, the argument validation (before any launch) and the workspace size."""
import ctypes
import os
import re

import pytest
import torch

from cosine_ce_ref import chain_normalisation, cluster_labels, clustered, loss64, reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pclip_cosine_ce_f16", "pclip_cosine_ce_backward_f16")


def central_difference(f, x, h=1e-6):
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = float(f())
        flat[i] = keep - h
        down = float(f())
        flat[i] = keep
        gf[i] = (up - down) / (2 * h)
    return g


@pytest.mark.parametrize("symmetric,normalize", [(False, False), (False, True), (True, True)])
def test_helper_gradients_agree_with_finite_differences(symmetric, normalize):
    M, T, D, scale = (3, 3, 64, 14.2857) if symmetric else (3, 5, 64, 14.2857)
    a16, b16 = clustered(M, T, D, 1)
    labels = None if symmetric else cluster_labels(M, T, 2)
    ref = reference(a16, b16, scale, labels, symmetric, normalize, normalize)
    # the same function of float64 leaves, normalised exactly where the helper chains through the normalisation
    a, b, sc = a16.double(), b16.double(), torch.tensor(float(torch.tensor(scale, dtype=torch.float32)), dtype=torch.float64)
    unit = (lambda x: x / x.norm(dim=1, keepdim=True)) if normalize else (lambda x: x)
    f = lambda: loss64(unit(a), unit(b), sc, labels, symmetric)[0]
    if normalize:
        # the helper evaluates dL/dx' at the fp16-rounded x' and chains at the exact x: compare its chain rule on the exact x' instead
        ap, bp = unit(a).clone().requires_grad_(True), unit(b).clone().requires_grad_(True)
        loss64(ap, bp, sc, labels, symmetric)[0].backward()
        want_a, want_b = chain_normalisation(a16, ap.grad), chain_normalisation(b16, bp.grad)
    else:
        want_a, want_b = ref["da"], ref["db"]
    for x, want in ((a, want_a), (b, want_b)):
        fd = central_difference(f, x)
        assert (fd - want).abs().max().item() <= 1e-6 * (1 + want.abs().max().item())
    if not normalize:
        h = 1e-6
        fd = (float(loss64(a, b, sc + h, labels, symmetric)[0]) - float(loss64(a, b, sc - h, labels, symmetric)[0])) / (2 * h)
        assert abs(fd - float(ref["dscale"])) <= 1e-6 * (1 + abs(float(ref["dscale"])))
    else:
        # and the fp16 rounding of x' moves the helper's own gradient by no more than that rounding allows (unit 2^-11 on every element of x')
        assert (ref["da"] - want_a).abs().max().item() <= 2.0 ** -8 * scale * (1 + want_a.abs().max().item())


def test_header_declares_and_library_exports_the_entry_points():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    for const in ("PCLIP_OP_COSINE_CE 5", "PCLIP_OP_COSINE_CE_BACKWARD 6", "PCLIP_CE_NORMALIZE_A 0x1", "PCLIP_CE_NORMALIZE_B 0x2", "PCLIP_CE_SYMMETRIC 0x4",
                  "PCLIP_CE_LABELS_I64 0x8"):
        assert "#define " + const in header, const
    assert "clip/model.py:356-370" in header.split("int pclip_cosine_ce_f16")[0].split("pclip_cosine_logits_f16(")[-1]
    assert "clip/model.py:356-370" in header.split("int pclip_cosine_ce_backward_f16")[0].split("int pclip_cosine_ce_f16")[-1]


BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first
BIG = 1 << 40


def forward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=100.0, flags=0, labels=BUF, lse_row=BUF, lse_col=None, row_loss=BUF, loss=BUF, ws=BUF,
            ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_ce_f16(a, lda, M, b, ldb, T, D, scale, flags, labels, lse_row, lse_col, row_loss, loss, ws, ws_bytes, None)


def backward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=100.0, flags=0, labels=BUF, lse_row=BUF, lse_col=None, weight=0.125, direction=0, grad=BUF,
             dscale=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_ce_backward_f16(a, lda, M, b, ldb, T, D, scale, flags, labels, lse_row, lse_col, weight, direction, grad, dscale, ws,
                                                    ws_bytes, None)


REFUSED = [
    (dict(D=96, lda=96, ldb=96), b"multiple of 64"),
    (dict(D=2112, lda=2112, ldb=2112), b"past the envelope"),
    (dict(D=4096, lda=4096, ldb=4096), b"past the envelope"),
    (dict(flags=0x4, labels=None, lse_col=BUF, M=8, T=9), b"symmetric mode needs M == T"),
    (dict(lda=68), b"lda=68"),
    (dict(ldb=60), b"ldb=60"),
    (dict(a=ctypes.c_void_p(0x1008)), b"aligned"),
    (dict(M=0), b"positive"),
    (dict(flags=0x10), b"unknown flag"),
    (dict(labels=None), b"needs labels"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
@pytest.mark.parametrize("call", [forward, backward])
def test_argument_validation_precedes_any_launch(call, kw, text):
    from proto_clip_amd import _lib
    assert call(**kw) == -1
    assert text in _lib.load().pclip_last_error(), _lib.load().pclip_last_error()


def test_backward_direction_is_checked():
    from proto_clip_amd import _lib
    assert backward(direction=2) == -1 and b"direction=2" in _lib.load().pclip_last_error()


def test_workspace_is_checked_and_does_not_grow_with_m_times_t():
    from proto_clip_amd import _lib
    lib = _lib.load()
    for call, op in ((forward, _lib.OP_COSINE_CE), (backward, _lib.OP_COSINE_CE_BACKWARD)):
        need = lib.pclip_workspace_bytes(op, 8, 8, 64)
        assert need > 0
        assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.pclip_last_error()
        assert call(ws=None) == -1 and b"workspace" in lib.pclip_last_error()
    M = T = 32768
    D = 512
    slack = 1 << 16
    fwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE, M, T, D)
    panels = M // 16                                                   # the smallest panel the kernel uses
    assert T * D * 2 <= fwd <= T * D * 2 + panels * T * 8 + M * 4 + slack
    bwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE_BACKWARD, M, T, D)
    assert 2 * T * D * 2 <= bwd <= 2 * (max(M, T) + 64) * D * 2 + 4 * (M + T) * D * 4 + 8 * panels * 4 + slack     # (+ the partial panels of a split walk)
    assert fwd + bwd < M * T * 2 // 4                                  # the fp16 matrix alone is 2 GB
    # linear in M at fixed T, not in M T: the labelled shape of the benchmark against one eight times as tall
    f1 = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE, 50000, 1000, 512)
    f8 = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE, 400000, 1000, 512)
    assert f8 - f1 <= (400000 - 50000) * 4 + slack
    b1 = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE_BACKWARD, 50000, 1000, 512)
    b8 = lib.pclip_workspace_bytes(_lib.OP_COSINE_CE_BACKWARD, 400000, 1000, 512)
    assert b8 <= 8 * b1 + slack
