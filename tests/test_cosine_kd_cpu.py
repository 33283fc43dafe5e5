"""What the distillation entries (pclip_cosine_kd_f16 / pclip_cosine_kd_backward_f16) and ProGrad's projection can be asked without a GPU: the declarations,
the exports, the argument validation (before any launch), the workspace size; the float64 helper of tests/cosine_kd_ref.py against the cross-entropy helper
on a planted one-hot teacher; an fp32 emulation of the documented walk inside the derived tolerances on the GPU test's inputs, and wrong walks outside."""
import ctypes
import os
import re

import pytest
import torch

import cosine_ce_ref
import cosine_kd_ref as kr
from cosine_ce_ref import clustered, worst_ratio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pclip_cosine_kd_f16", "pclip_cosine_kd_backward_f16")


def test_header_declares_library_exports_and_makefile_lists():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    for const in ("PCLIP_OP_COSINE_KD 10", "PCLIP_OP_COSINE_KD_BACKWARD 11", "PCLIP_KD_NORMALIZE_A 0x1", "PCLIP_KD_NORMALIZE_B 0x2", "PCLIP_KD_NORMALIZE_TA 0x4",
                  "PCLIP_KD_NORMALIZE_TB 0x8"):
        assert "#define " + const in header, const
    assert (_lib.OP_COSINE_KD, _lib.OP_COSINE_KD_BACKWARD) == (10, 11)
    assert (_lib.KD_NORMALIZE_A, _lib.KD_NORMALIZE_B, _lib.KD_NORMALIZE_TA, _lib.KD_NORMALIZE_TB) == (1, 2, 4, 8)
    assert "clip/model.py:356-370" in header.split("int pclip_cosine_kd_f16")[0].split("pclip_cosine_ce_grouped_workspace(")[-1]
    makefile = open(os.path.join(REPO, "proto-clip_amd", "csrc", "Makefile")).read()
    assert "pclip_cosine_kd.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()


BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first
BIG = 1 << 40


def forward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=100.0, ta=BUF, ldta=64, tb=BUF, ldtb=64, Dt=64, tscale=100.0, flags=0, lse_row=BUF, tlse_row=BUF,
            row_loss=BUF, loss=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_kd_f16(a, lda, M, b, ldb, T, D, scale, ta, ldta, tb, ldtb, Dt, tscale, flags, lse_row, tlse_row, row_loss, loss, ws, ws_bytes,
                                           None)


def backward(a=BUF, lda=64, M=8, b=BUF, ldb=64, T=8, D=64, scale=100.0, ta=BUF, ldta=64, tb=BUF, ldtb=64, Dt=64, tscale=100.0, flags=0, lse_row=BUF, tlse_row=BUF,
             weight=0.125, direction=0, grad=BUF, dscale=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_cosine_kd_backward_f16(a, lda, M, b, ldb, T, D, scale, ta, ldta, tb, ldtb, Dt, tscale, flags, lse_row, tlse_row, weight, direction,
                                                    grad, dscale, ws, ws_bytes, None)


REFUSED = [
    (dict(D=96, lda=96, ldb=96), b"D=96 must be a multiple of 64"),
    (dict(Dt=96, ldta=96, ldtb=96), b"Dt=96 must be a multiple of 64"),
    (dict(D=2112, lda=2112, ldb=2112), b"past the envelope"),
    (dict(Dt=2112, ldta=2112, ldtb=2112), b"Dt=2112 is past the envelope"),
    (dict(lda=68), b"lda=68"),
    (dict(ldta=68), b"ldta=68"),
    (dict(ldtb=60), b"ldtb=60"),
    (dict(Dt=128, ldta=128), b"ldtb=64"),
    (dict(ta=ctypes.c_void_p(0x1008)), b"aligned"),
    (dict(tb=None), b"null operand"),
    (dict(M=0), b"positive"),
    (dict(flags=0x10), b"unknown flag"),
    (dict(tscale=float("inf")), b"must be finite"),
    (dict(tscale=float("nan")), b"must be finite"),
    (dict(scale=float("-inf")), b"must be finite"),
    (dict(tlse_row=None), b"required"),
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


def test_workspace_is_checked_sized_by_the_wider_operand_and_linear():
    from proto_clip_amd import _lib
    lib = _lib.load()
    for call, op in ((forward, _lib.OP_COSINE_KD), (backward, _lib.OP_COSINE_KD_BACKWARD)):
        need = lib.pclip_workspace_bytes(op, 8, 8, 64)
        assert need > 0
        assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.pclip_last_error()
        assert call(ws=None) == -1 and b"workspace" in lib.pclip_last_error()
        wide = lib.pclip_workspace_bytes(op, 8, 8, 128)
        assert wide > need
        assert call(Dt=128, ldta=128, ldtb=128, ws_bytes=wide - 1) == -3          # the teacher's width counts
    slack = 1 << 16
    M, T, D = 50000, 1000, 768
    fwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_KD, M, T, D)
    assert fwd <= 3 * T * D * 2 + 3 * M * 4 + slack                    # two normalised class operands, the cross-entropy forward's, three row vectors
    bwd = lib.pclip_workspace_bytes(_lib.OP_COSINE_KD_BACKWARD, M, T, D)
    assert bwd <= 3 * (M + 64) * D * 2 + 4 * (M + T) * D * 4 + slack   # two normalised walked operands and a transpose, the partial panels of a split walk
    assert fwd + bwd < 2 * M * T * 4                                   # two fp32 [M, T] matrices are 400 MB; autograd keeps two sets of logits and two softmaxes
    # linear in M at fixed T, not in M T
    f8 = lib.pclip_workspace_bytes(_lib.OP_COSINE_KD, 8 * M, T, D)
    assert f8 - fwd <= 7 * M * 12 + slack
    assert lib.pclip_workspace_bytes(_lib.OP_COSINE_KD_BACKWARD, 8 * M, T, D) <= 8 * bwd + slack


def test_teacher_that_requires_grad_is_refused():
    from proto_clip_amd import autograd as pag
    from proto_clip_amd._lib import PclipError
    a, b = clustered(4, 5, 64, 1)
    for kw in (dict(teacher_a=a.clone().requires_grad_(True)), dict(teacher_b=b.float().requires_grad_(True)),
               dict(teacher_scale=torch.tensor(100.0, requires_grad=True))):
        args = dict(teacher_a=a, teacher_b=b, teacher_scale=100.0)
        args.update(kw)
        with pytest.raises(PclipError, match="requires grad"):
            pag.cosine_kd(a, b.float().requires_grad_(True), 100.0, **args)
    with pytest.raises(PclipError, match="temperature"):
        pag.cosine_kd(a, b, 100.0, a, b, 100.0, temperature=0.0)


# ---- the float64 helper, the emulation of the documented walk, the wrong walks ----------------------------------------------------------------------

def gpu_case(M, T, D, Dt, seed=3):
    a16, b16 = clustered(M, T, D, seed)
    ta16, tb16 = kr.teacher_like(M, T, Dt, seed)
    return a16, b16, ta16, tb16


def test_float64_identities_of_the_helper():
    a16, b16, ta16, tb16 = gpu_case(17, 37, 64, 64)
    ref = kr.reference(a16, b16, 20.0, ta16, tb16, 50.0, True, True, True, True)
    assert float(ref["rows"].min()) > 0 and abs(float(ref["rows"].mean() - ref["loss"])) < 1e-12
    same = kr.reference(a16, b16, 100.0, a16, b16, 100.0, True, True, True, True)
    assert float(same["loss"].abs()) < 1e-12 and float(same["da"].abs().max()) < 1e-12 and float(same["db"].abs().max()) < 1e-12
    assert float(same["tol_loss"]) > 0 and float(same["tol_da"].min()) > 0                 # teacher == student is graded against 0 with a bound that is not 0


@pytest.mark.parametrize("M,T,D,Dt", [(17, 37, 64, 64), (33, 65, 512, 768)])
def test_planted_teacher_gives_the_cross_entropy_in_float64(M, T, D, Dt):
    a16, b16, ta16, tb16, labels = kr.planted(M, T, D, Dt, 5)
    kd = kr.reference(a16, b16, 100.0, ta16, tb16, kr.PLANTED_TSCALE, True, True, True, True)
    ce = cosine_ce_ref.reference(a16, b16, 100.0, labels, False, True, True)
    p = kd["p"]
    assert torch.equal(p.argmax(1), labels) and float((p.sum(1) - p.max(1)[0]).max()) < 1e-60          # one-hot in float64
    assert worst_ratio(kd["loss"], ce["loss"], kd["tol_loss"] + ce["tol_loss"]) <= 1.0
    for k in ("da", "db", "dscale"):
        assert worst_ratio(kd[k], ce[k], kd["tol_" + k] + ce["tol_" + k]) <= 1.0, k


CASES = [(17, 37, 64, 64, 100.0, 100.0, False), (33, 65, 512, 768, 20.0, 50.0, False), (15, 577, 64, 64, 100.0, 100.0, False),
         (33, 64, 512, 768, 20.0, 50.0, True), (33, 64, 512, 512, 50.0, 20.0, True)]
GRADED = (("loss", "tol_loss"), ("rows", "tol_rows"), ("lse_row", "tol_lse"), ("tlse_row", "tol_tlse"), ("da", "tol_da"), ("db", "tol_db"), ("dscale", "tol_dscale"))


def ratios(got, ref):
    return {k: worst_ratio(got[k], ref[k], ref[t]) for k, t in GRADED}


def case_operands(M, T, D, Dt, far):
    a16, b16, ta16, tb16 = gpu_case(M, T, D, Dt)
    if far:
        b16, tb16 = kr.with_far_class(b16, tb16, 3)
    return a16, b16, ta16, tb16


@pytest.mark.parametrize("M,T,D,Dt,scale,tscale,far", CASES)
def test_documented_walk_is_inside_the_tolerances(M, T, D, Dt, scale, tscale, far):
    a16, b16, ta16, tb16 = case_operands(M, T, D, Dt, far)
    ref = kr.reference(a16, b16, scale, ta16, tb16, tscale, True, True, True, True)
    r = ratios(kr.emulate(a16, b16, scale, ta16, tb16, tscale, True, True, True, True), ref)
    print("documented", {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("walk", kr.WALKS[1:])
def test_wrong_walks_are_outside_the_tolerances(walk):
    """On the case with a class no sample is near, teacher the softer side (scale 50 against 20): the far class's entries of E are the teacher's p, about
    2^-26 — the entries whose relative unit the 2^14 scaling keeps."""
    M, T, D, Dt, scale, tscale, far = CASES[-1]
    a16, b16, ta16, tb16 = case_operands(M, T, D, Dt, far)
    ref = kr.reference(a16, b16, scale, ta16, tb16, tscale, True, True, True, True)
    r = ratios(kr.emulate(a16, b16, scale, ta16, tb16, tscale, True, True, True, True, walk=walk), ref)
    print(walk, {k: round(v, 4) for k, v in r.items()})
    assert max(r["da"], r["db"], r["dscale"]) > 1.0, (walk, r)


def test_emulation_of_teacher_equal_student_is_within_tolerance_of_zero():
    a16, b16 = clustered(17, 37, 64, 3)
    ref = kr.reference(a16, b16, 100.0, a16, b16, 100.0, True, True, True, True)
    got = kr.emulate(a16, b16, 100.0, a16, b16, 100.0, True, True, True, True)
    assert abs(float(got["loss"])) <= float(ref["tol_loss"])
    assert worst_ratio(got["da"], torch.zeros_like(ref["da"]), ref["tol_da"]) <= 1.0


# ---- ProGrad's projection -------------------------------------------------------------------------------------------------------------------------------

class _Rule:
    lam = 1.0


def project(g_ce, g_kl, lam=1.0):
    from proto_clip_amd.prograd import ProGrad
    rule = _Rule()
    rule.lam = lam
    return ProGrad.project_(rule, g_ce.clone(), g_kl)


def test_project_keeps_an_agreeing_gradient_and_a_zero_teacher_gradient():
    g_ce, g_kl = torch.tensor([1.0, 2.0, -1.0]), torch.tensor([0.5, 0.0, 0.25])
    assert torch.equal(project(g_ce, g_kl), g_ce)                                         # <g_ce, g_kl> = 0.25 >= 0
    assert torch.equal(project(g_ce, torch.tensor([0.0, 1.0, 2.0])), g_ce)                 # exactly orthogonal
    assert torch.equal(project(g_ce, torch.zeros(3)), g_ce)                               # no teacher gradient: nothing to project on, and no NaN
    neg = torch.tensor([-1.0, 0.0, 0.0])
    assert torch.equal(project(neg, torch.zeros(3)), neg)


def test_project_removes_the_conflicting_component():
    g_ce, g_kl = torch.tensor([1.0, 1.0, 0.0, 2.0]), torch.tensor([-2.0, 0.0, 0.0, 0.0])
    out = project(g_ce, g_kl)
    assert torch.equal(out, torch.tensor([0.0, 1.0, 0.0, 2.0]))                            # d = -2, <g_kl, g_kl> = 4: g_ce + 0.5 g_kl
    assert float((out * g_kl).sum()) == 0.0
    half = project(g_ce, g_kl, lam=0.5)
    assert torch.equal(half, torch.tensor([0.5, 1.0, 0.0, 2.0]))
    # a matrix-shaped parameter is one vector
    assert torch.equal(project(g_ce.view(2, 2), g_kl.view(2, 2)), out.view(2, 2))


def test_project_is_homogeneous_in_a_common_loss_scale():
    g = torch.Generator().manual_seed(0)
    for trial in range(8):
        g_ce, g_kl = torch.randn(16, 64, generator=g), torch.randn(16, 64, generator=g)
        if trial % 2:
            g_kl = -g_ce + 0.5 * g_kl                                                     # a conflict for certain
        out = project(g_ce, g_kl)
        assert torch.equal(project(g_ce * 1024.0, g_kl * 1024.0), out * 1024.0)
        if trial % 2:
            assert not torch.equal(out, g_ce)


def test_project_refuses_other_dtypes():
    from proto_clip_amd._lib import PclipError
    with pytest.raises(PclipError):
        project(torch.zeros(3, dtype=torch.float16), torch.zeros(3, dtype=torch.float16))
