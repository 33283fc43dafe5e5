"""The float64 helper of the sigmoid-loss kernels (tests/cosine_sigmoid_ref.py) against central finite differences; a float64 emulation of the kernels' documented
roundings against the helper's tolerances, and four wrong kernels that must leave them; and what pclip_cosine_sigmoid_f16 / pclip_cosine_sigmoid_backward_f16 can
be asked without a GPU: the declarations, the exports, the argument validation (before any launch) and the workspace size."""
import ctypes
import os
import re

import pytest
import torch

from contrastive_ref import l2norm_rows_ref
from cosine_sigmoid_ref import case_ids, chain_normalisation, clustered, loss64, positives, reference, worst_ratio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("pclip_cosine_sigmoid_f16", 17), ("pclip_cosine_sigmoid_backward_f16", 20))
PAIRS = [(10.0, -10.0), (14.2857, -5.0), (100.0, -95.0)]
ITEMS = [("loss", "tol_loss"), ("rows", "tol_rows"), ("da", "tol_da"), ("db", "tol_db"), ("dscale", "tol_dscale"), ("dbias", "tol_dbias")]


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


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("diagonal", [False, True])
def test_helper_gradients_agree_with_finite_differences(diagonal, normalize):
    M, T, D, scale, bias = (3, 3, 64, 14.2857, -5.0) if diagonal else (3, 5, 64, 14.2857, -5.0)
    a16, b16 = clustered(M, T, D, 1)
    ia, ib = (None, None) if diagonal else (torch.tensor([0, 1, -1]), torch.tensor([0, 1, 2, 0, 1]))
    ref = reference(a16, b16, scale, bias, ia, ib, normalize, normalize)
    y = positives(M, T, ia, ib)
    f32 = lambda v: torch.tensor(float(torch.tensor(v, dtype=torch.float32)), dtype=torch.float64)
    a, b, sc, bi = a16.double(), b16.double(), f32(scale), f32(bias)
    unit = (lambda x: x / x.norm(dim=1, keepdim=True)) if normalize else (lambda x: x)
    f = lambda: loss64(unit(a), unit(b), sc, bi, y)[0]
    if normalize:
        # the helper evaluates dL/dx' at the fp16-rounded x' and chains at the exact x: compare its chain rule on the exact x' instead
        ap, bp = unit(a).clone().requires_grad_(True), unit(b).clone().requires_grad_(True)
        loss64(ap, bp, sc, bi, y)[0].backward()
        want_a, want_b = chain_normalisation(a16, ap.grad), chain_normalisation(b16, bp.grad)
    else:
        want_a, want_b = ref["da"], ref["db"]
    for x, want in ((a, want_a), (b, want_b)):
        fd = central_difference(f, x)
        assert (fd - want).abs().max().item() <= 1e-6 * (1 + want.abs().max().item())
    if not normalize:
        h = 1e-6
        fd = (float(loss64(a, b, sc + h, bi, y)[0]) - float(loss64(a, b, sc - h, bi, y)[0])) / (2 * h)
        assert abs(fd - float(ref["dscale"])) <= 1e-6 * (1 + abs(float(ref["dscale"])))
        fd = (float(loss64(a, b, sc, bi + h, y)[0]) - float(loss64(a, b, sc, bi - h, y)[0])) / (2 * h)
        assert abs(fd - float(ref["dbias"])) <= 1e-6 * (1 + abs(float(ref["dbias"])))
    else:
        assert (ref["da"] - want_a).abs().max().item() <= 2.0 ** -8 * scale * (1 + want_a.abs().max().item())


def emulate(a16, b16, scale, bias, ids_a, ids_b, na, nb, wrong=None):
    """The kernels' documented roundings restated on the CPU: fp32 dot products, one fp32 logit, fp32 terms and row sums, sigma rounded to fp16 at 2^14 for the
    second product, an exact target tile, fp32 sums, the chain through the normalisation in fp32.  wrong: one of WRONG."""
    M, T = a16.shape[0], b16.shape[0]
    ap = (l2norm_rows_ref(a16) if na else a16).float()
    bp = (l2norm_rows_ref(b16) if nb else b16).float()
    sc, bi = float(torch.tensor(scale, dtype=torch.float32)), float(torch.tensor(bias, dtype=torch.float32))
    cos = ap @ bp.t()
    x = (sc * cos.double() + (0.0 if wrong == "no bias" else bi)).float()
    y = positives(M, T, ids_a, ids_b).float()
    z = 2 * y - 1
    xd = x.double()
    term = (torch.clamp(-z.double() * xd, min=0) + torch.log1p(torch.exp(-xd.abs()))).float()
    rows = term.sum(1)
    over = T if wrong == "mean over T" else M
    loss = (rows.double().sum() / over).float()
    w = 1.0 / over
    E = torch.sigmoid(-xd if wrong == "sigma(-x)" else xd).float()
    E16 = (E * 16384.0).half().float() / 16384.0
    tgt = 0.0 if wrong == "no target term" else y
    G16, G = E16 - tgt, E - tgt
    mul = torch.tensor(w, dtype=torch.float32) * torch.tensor(sc, dtype=torch.float32)
    da, db = mul * (G16 @ bp), mul * (G16.t() @ ap)
    dscale, dbias = torch.tensor(w, dtype=torch.float32) * (G * cos).sum(), torch.tensor(w, dtype=torch.float32) * G.sum()
    if na:
        da = chain_normalisation(a16, da.double()).float()
    if nb:
        db = chain_normalisation(b16, db.double()).float()
    return dict(loss=loss, rows=rows, da=da, db=db, dscale=dscale, dbias=dbias)


CASES = [(3, 5, 64), (17, 37, 128), (33, 100, 512), (130, 70, 64), (65, 65, 64)]
WRONG = ["no target term", "no bias", "sigma(-x)", "mean over T"]


def operands(M, T, D):
    a16, b16 = clustered(M, T, D, 7 + M)
    ia, ib = (None, None) if M == T else case_ids(M, T, M % 2 == 1)
    return a16, b16, ia, ib


@pytest.mark.parametrize("scale,bias", PAIRS)
@pytest.mark.parametrize("M,T,D", CASES)
def test_documented_roundings_stay_inside_every_tolerance(M, T, D, scale, bias):
    a16, b16, ia, ib = operands(M, T, D)
    for na, nb in ((False, False), (True, True), (True, False)):
        ref = reference(a16, b16, scale, bias, ia, ib, na, nb)
        got = emulate(a16, b16, scale, bias, ia, ib, na, nb)
        ratios = {name: worst_ratio(got[name], ref[name], ref[tol]) for name, tol in ITEMS}
        print((M, T, D, scale, bias, na, nb), {k: round(v, 4) for k, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("scale,bias", PAIRS)
@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_kernel_leaves_a_tolerance(wrong, scale, bias):
    """On the rectangular case (17, 37, 128) — the mean over T is only wrong where M != T — at every (scale, bias) pair."""
    a16, b16, ia, ib = operands(17, 37, 128)
    ref = reference(a16, b16, scale, bias, ia, ib, True, True)
    got = emulate(a16, b16, scale, bias, ia, ib, True, True, wrong)
    ratios = {name: worst_ratio(got[name], ref[name], ref[tol]) for name, tol in ITEMS}
    print(wrong, (scale, bias), {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) > 1.0, (wrong, ratios)


def test_header_declares_and_library_exports_the_entry_points():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib._SIGS[name]) == nargs, name
        assert getattr(lib, name).argtypes == _lib._SIGS[name] and getattr(lib, name).restype is ctypes.c_int
    for const in ("PCLIP_OP_COSINE_SIGMOID 8", "PCLIP_OP_COSINE_SIGMOID_BACKWARD 9", "PCLIP_SIG_NORMALIZE_A 0x1", "PCLIP_SIG_NORMALIZE_B 0x2", "PCLIP_SIG_IDS_I64 0x8"):
        assert "#define " + const in header, const
    assert (_lib.OP_COSINE_SIGMOID, _lib.OP_COSINE_SIGMOID_BACKWARD) == (8, 9)
    assert (_lib.SIG_NORMALIZE_A, _lib.SIG_NORMALIZE_B, _lib.SIG_IDS_I64) == (0x1, 0x2, 0x8)
    assert lib.pclip_abi_version() == 1


BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first
BIG = 1 << 40


def forward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=10.0, bias=-10.0, flags=0, ids_a=BUF, ids_b=BUF, row_loss=BUF, loss=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_sigmoid_f16(a, lda, M, b, ldb, T, D, scale, bias, flags, ids_a, ids_b, row_loss, loss, ws, ws_bytes, None)


def backward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=10.0, bias=-10.0, flags=0, ids_a=BUF, ids_b=BUF, weight=0.125, direction=0, grad=BUF,
             dscale=BUF, dbias=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_sigmoid_backward_f16(a, lda, M, b, ldb, T, D, scale, bias, flags, ids_a, ids_b, weight, direction, grad, dscale, dbias, ws,
                                                         ws_bytes, None)


REFUSED = [
    (dict(D=96, lda=96, ldb=96), b"D=96"),
    (dict(D=2112, lda=2112, ldb=2112), b"D=2112"),
    (dict(D=4096, lda=4096, ldb=4096), b"D=4096"),
    (dict(lda=68), b"lda=68"),
    (dict(ldb=60), b"ldb=60"),
    (dict(a=ctypes.c_void_p(0x1008)), b"aligned"),
    (dict(ids_a=None, ids_b=None, M=8, T=9), b"M == T"),
    (dict(ids_a=None), b"ids_a and ids_b"),
    (dict(ids_b=None), b"ids_a and ids_b"),
    (dict(scale=float("inf")), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(bias=float("-inf")), b"bias"),
    (dict(bias=float("nan")), b"bias"),
    (dict(M=0), b"M=0"),
    (dict(flags=0x4), b"flag"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
@pytest.mark.parametrize("call", [forward, backward])
def test_argument_validation_precedes_any_launch(call, kw, text):
    from proto_clip_amd import _lib
    assert call(**kw) == -1
    assert text in _lib.load().pclip_last_error(), _lib.load().pclip_last_error()


def test_backward_direction_and_weight_are_checked():
    from proto_clip_amd import _lib
    assert backward(direction=2) == -1 and b"direction=2" in _lib.load().pclip_last_error()
    assert backward(weight=float("nan")) == -1 and b"weight" in _lib.load().pclip_last_error()
    assert backward(grad=None) == -1 and b"grad" in _lib.load().pclip_last_error()


def test_workspace_is_checked_and_does_not_grow_with_m_times_t():
    from proto_clip_amd import _lib
    lib = _lib.load()
    for call, op in ((forward, _lib.OP_COSINE_SIGMOID), (backward, _lib.OP_COSINE_SIGMOID_BACKWARD)):
        need = lib.pclip_workspace_bytes(op, 8, 8, 64)
        assert need > 0
        assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.pclip_last_error()
        assert call(ws=None) == -1 and b"workspace" in lib.pclip_last_error()
    M = T = 32768
    D = 512
    slack = 1 << 16
    fwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID, M, T, D)
    assert T * D * 2 <= fwd <= T * D * 2 + slack
    bwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID_BACKWARD, M, T, D)
    panels = M // 16                                                   # the smallest panel the kernel uses
    assert 2 * T * D * 2 <= bwd <= 2 * (max(M, T) + 64) * D * 2 + 4 * (M + T) * D * 4 + 16 * panels * 4 + slack     # (+ the partial panels of a split walk)
    assert fwd + bwd < M * T * 2 // 4                                  # the fp16 matrix alone is 2 GB
    # the forward does not depend on M at all; the backward is linear in the larger side at a fixed smaller one
    assert lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID, 400000, 1000, 512) == lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID, 50000, 1000, 512)
    b1 = lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID_BACKWARD, 50000, 1000, 512)
    b8 = lib.pclip_workspace_bytes(_lib.OP_COSINE_SIGMOID_BACKWARD, 400000, 1000, 512)
    assert b8 <= 8 * b1 + slack
    assert b1 <= 2 * (50000 + 64) * 512 * 2 + 4 * 51000 * 512 * 4 + slack
