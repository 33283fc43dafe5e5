"""What the grouped cosine cross-entropy (pclip_cosine_ce_grouped_f16 / _backward_f16 / _workspace) can be asked without a GPU: the declarations, the
exports, the argument validation (before any launch, on pointers that are never dereferenced), the workspace size, and the refusals of the `ops` wrappers."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pclip_cosine_ce_grouped_f16", "pclip_cosine_ce_grouped_backward_f16", "pclip_cosine_ce_grouped_workspace")

BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first
BIG = 1 << 40


def forward(a=BUF, lda=64, gsa=512, M=8, b=BUF, ldb=64, gsb=512, T=8, D=64, G=3, scale=100.0, flags=0, labels=BUF, lse_row=BUF, row_loss=BUF, loss=BUF, ws=BUF,
            ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_ce_grouped_f16(a, lda, gsa, M, b, ldb, gsb, T, D, G, scale, flags, labels, lse_row, row_loss, loss, ws, ws_bytes, None)


def backward(a=BUF, lda=64, gsa=512, M=8, b=BUF, ldb=64, gsb=512, T=8, D=64, G=3, scale=100.0, flags=0, labels=BUF, lse_row=BUF, weight=0.125, direction=0,
             grad=BUF, dscale=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_ce_grouped_backward_f16(a, lda, gsa, M, b, ldb, gsb, T, D, G, scale, flags, labels, lse_row, weight, direction, grad, dscale,
                                                            ws, ws_bytes, None)


def test_header_declares_and_library_exports_the_entry_points():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None


REFUSED = [
    (dict(G=0), b"G=0"),
    (dict(G=65536), b"G=65536"),
    (dict(gsa=516), b"gsa=516"),
    (dict(gsb=4), b"gsb=4"),
    (dict(flags=0x4, labels=None), b"PCLIP_CE_SYMMETRIC"),
    (dict(flags=0x4), b"PCLIP_CE_SYMMETRIC"),
    (dict(labels=None), b"needs labels"),
    (dict(D=96, lda=96, ldb=96, gsa=768, gsb=768), b"multiple of 64"),
    (dict(D=2112, lda=2112, ldb=2112, gsa=8 * 2112, gsb=8 * 2112), b"past the envelope"),
    (dict(lda=68), b"lda=68"),
    (dict(a=ctypes.c_void_p(0x1008)), b"aligned"),
    (dict(M=0), b"positive"),
    (dict(flags=0x10), b"unknown flag"),
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


def test_a_short_workspace_is_its_own_error():
    from proto_clip_amd import _lib
    lib = _lib.load()
    for call, bwd in ((forward, 0), (backward, 1)):
        need = lib.pclip_cosine_ce_grouped_workspace(bwd, 3, 8, 8, 64)
        assert need > 0
        assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.pclip_last_error()
        assert call(ws=None) == -1 and b"workspace" in lib.pclip_last_error()


@pytest.mark.parametrize("M,T,D", [(1, 37, 512), (8, 8, 64), (17, 130, 64), (130, 5, 64), (1, 1000, 1024)])
def test_one_group_takes_the_plain_workspace_and_g_groups_g_of_them(M, T, D):
    from proto_clip_amd import _lib
    lib = _lib.load()
    for bwd, op in ((0, _lib.OP_COSINE_CE), (1, _lib.OP_COSINE_CE_BACKWARD)):
        plain = lib.pclip_workspace_bytes(op, M, T, D)
        assert plain > 0 and lib.pclip_cosine_ce_grouped_workspace(bwd, 1, M, T, D) == plain
        assert lib.pclip_cosine_ce_grouped_workspace(bwd, 19, M, T, D) == 19 * plain
    assert lib.pclip_cosine_ce_grouped_workspace(0, 0, M, T, D) == 0


def test_host_layer_refuses_what_the_kernel_cannot_take():
    """Types and shapes are checked before the device, so every refusal can be provoked with CPU tensors; each names its argument."""
    from proto_clip_amd import PclipError, ops
    a = torch.zeros(3, 2, 64, dtype=torch.float16)
    b = torch.zeros(3, 5, 64, dtype=torch.float16)
    y = torch.zeros(3, 2, dtype=torch.int64)
    lse = torch.zeros(3, 2)
    calls = (lambda *args: ops.cosine_cross_entropy_grouped(args[0], args[1], 100.0, args[2]),
             lambda *args: ops.cosine_cross_entropy_grouped_backward(args[0], args[1], 100.0, lse, args[2]))
    for call in calls:
        with pytest.raises(PclipError, match=": a: expected a device tensor"):          # CPU tensors
            call(a, b, y)
        with pytest.raises(PclipError, match=": a: expected a float16 tensor"):
            call(a.float(), b, y)
        with pytest.raises(PclipError, match=": b: expected a float16 tensor"):
            call(a, b.double(), y)
        with pytest.raises(PclipError, match=r"labels must be .* \[G=3, M=2\]"):
            call(a, b, y[:, :1])
        with pytest.raises(PclipError, match=r"labels must be"):
            call(a, b, y.float())
        with pytest.raises(PclipError, match="a has 3 groups, b has 2"):
            call(a, b[:2], y)
        with pytest.raises(PclipError, match="a has 64 columns, b has 128"):
            call(a, torch.zeros(3, 5, 128, dtype=torch.float16), y)
