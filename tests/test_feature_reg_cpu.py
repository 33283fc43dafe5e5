"""What the feature-regulariser entries (pclip_feature_reg_f16 / pclip_feature_reg_backward_f16) can be asked without a GPU: the declarations, the exports,
the constants, every refusal (before any launch), the workspace size; the numpy-float32 emulation of the documented walk (tests/feature_reg_ref.py) inside
the derived tolerances on every case the GPU test grades, float64 alone leaving almost no L1 element undecided there, and four wrong walks outside."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feature_reg_ref as fr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pclip_feature_reg_f16", "pclip_feature_reg_backward_f16")
MODES = [("l1", False), ("l1", True), ("cos", False), ("cos", True)]


def test_header_declares_library_exports_and_makefile_lists():
    from proto_clip_amd import _lib
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert re.search(r"\bsize_t\s+pclip_feature_reg_workspace\s*\(", header) and "pclip_feature_reg_workspace" in _lib.EXPORTED_SYMBOLS
    for const in ("PCLIP_FREG_L1 0", "PCLIP_FREG_COS 1", "PCLIP_FREG_CHUNK 1024"):
        assert "#define " + const in header, const
    assert (_lib.FREG_L1, _lib.FREG_COS, _lib.FREG_CHUNK) == (0, 1, 1024) and fr.CHUNK == _lib.FREG_CHUNK
    doc = header.split("int pclip_feature_reg_f16")[0].split("PCLIP_KD_NORMALIZE_TB 0x8")[-1]
    assert "clip/model.py:361-362" in doc and "F.l1_loss(" in doc and "cosine_similarity(" in doc          # the torch expressions the entry replaces
    makefile = open(os.path.join(REPO, "proto-clip_amd", "csrc", "Makefile")).read()
    assert "pclip_feature_reg.hip" in re.search(r"^SRCS = (.*)$", makefile, flags=re.M).group(1).split()
    rule = re.search(r"^pclip_feature_reg\.o:.*\n\t(.*)$", makefile, flags=re.M)
    assert rule and "-ffp-contract=off" in rule.group(1)          # the emulation is graded bit for bit: nothing may fuse
    src = open(os.path.join(REPO, "proto-clip_amd", "csrc", "pclip_feature_reg.hip")).read()
    assert "atomic" not in src.split('#include "pclip_common.h"')[1]


BUF = ctypes.c_void_p(0x1000)          # never dereferenced: validation rejects first
BIG = 1 << 40


def forward(x=BUF, ldx=64, t=BUF, ldt=64, M=8, D=64, mode=0, normalize_t=0, loss=BUF, rows=BUF, inv_norm=BUF, ws=BUF, ws_bytes=BIG):
    from proto_clip_amd import _lib
    return _lib.load().pclip_feature_reg_f16(x, ldx, t, ldt, M, D, mode, normalize_t, loss, rows, inv_norm, ws, ws_bytes, None)


def backward(x=BUF, ldx=64, t=BUF, ldt=64, M=8, D=64, mode=0, normalize_t=0, weight=0.125, dx=BUF):
    from proto_clip_amd import _lib
    return _lib.load().pclip_feature_reg_backward_f16(x, ldx, t, ldt, M, D, mode, normalize_t, weight, dx, None)


REFUSED = [
    (dict(D=12, ldx=16, ldt=16), b"D=12 must be a multiple of 8 in 8..4096"),
    (dict(D=0), b"D=0 must be a multiple of 8"),
    (dict(D=4104, ldx=4104, ldt=4104), b"D=4104 must be a multiple of 8 in 8..4096"),
    (dict(M=-1), b"M=-1 must not be negative"),
    (dict(mode=2), b"mode=2 is neither"),
    (dict(normalize_t=2), b"normalize_t=2"),
    (dict(ldx=68), b"ldx=68"),
    (dict(ldx=56), b"ldx=56"),
    (dict(ldt=68), b"ldt=68"),
    (dict(ldt=56), b"ldt=56"),
    (dict(x=None), b"null operand"),
    (dict(t=None), b"null operand"),
    (dict(x=ctypes.c_void_p(0x1008)), b"16-byte aligned"),
    (dict(t=ctypes.c_void_p(0x1008)), b"16-byte aligned"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
@pytest.mark.parametrize("call", [forward, backward])
def test_argument_validation_precedes_any_launch(call, kw, text):
    from proto_clip_amd import _lib
    assert call(**kw) == -1
    assert text in _lib.load().pclip_last_error(), _lib.load().pclip_last_error()


def test_outputs_and_workspace_are_checked():
    from proto_clip_amd import _lib
    lib = _lib.load()
    for kw, text in ((dict(loss=None), b"loss is required"), (dict(rows=None), b"rows and inv_norm"), (dict(inv_norm=None), b"rows and inv_norm")):
        assert forward(**kw) == -1 and text in lib.pclip_last_error()
    assert backward(dx=None) == -1 and b"dx is required" in lib.pclip_last_error()
    assert backward(dx=ctypes.c_void_p(0x1008)) == -1 and b"dx must be 16-byte aligned" in lib.pclip_last_error()
    ws = lib.pclip_feature_reg_workspace
    assert [ws(M) for M in (-1, 0, 1, 1024)] == [0, 0, 0, 0]          # one chunk: the loss is reduced from the rows themselves
    assert ws(1025) >= 8 and ws(1 << 20) >= 4 << 10 and ws(1 << 20) <= (4 << 10) + 256
    assert ws(2 ** 31 - 1) >= 4 * 2 ** 21                              # no overflow at the end of the range
    assert forward(M=1025, ws=None) == -1 and b"need a workspace" in lib.pclip_last_error()
    assert forward(M=1025, ws_bytes=ws(1025) - 1) == -3 and b"workspace" in lib.pclip_last_error()
    assert backward(M=0, x=None, t=None, dx=None) == 0                 # nothing to do, nothing looked at


def test_wrappers_refuse_before_any_launch():
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import ops, utils
    from proto_clip_amd._lib import PclipError
    x, t = torch.zeros(4, 64, dtype=torch.float16), torch.zeros(4, 64, dtype=torch.float16)
    for call, text in ((lambda: ops.feature_reg(x, t, "l2"), "neither 'l1' nor 'cos'"),
                       (lambda: ops.feature_reg(x.float(), t), "x must be a 2-D float16"),
                       (lambda: ops.feature_reg(x, t[0]), "t must be a 2-D float16"),
                       (lambda: ops.feature_reg(x, t[:3]), r"x is \(4, 64\), the target \(3, 64\)"),
                       (lambda: ops.feature_reg(x[:, :12], t[:, :12]), "D=12 must be a multiple of 8"),
                       (lambda: ops.feature_reg(x, t), "device tensors only"),
                       (lambda: ops.feature_reg_backward(x, t, torch.zeros(3), "l1", False), "device tensors only|inv_norm must be"),
                       (lambda: pag.feature_reg(x, t.float().requires_grad_(True)), "t requires grad, but the target receives no gradient"),
                       (lambda: utils.clip_feature_l1_loss(x, t.clone().requires_grad_(True)), "requires grad"),
                       (lambda: utils.clip_feature_cosine_loss(x.requires_grad_(False), t.clone().requires_grad_(True)), "requires grad")):
        with pytest.raises(PclipError, match=text):
            call()


# ---- the emulation of the documented walk against float64, and the wrong walks ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,nt", MODES)
@pytest.mark.parametrize("M,D", fr.GPU_SHAPES + [(9, 72)])
def test_documented_walk_is_inside_the_tolerances_and_float64_decides_the_signs(M, D, mode, nt):
    x16, t16 = fr.make_case(M, D, fr.case_seed(M, D), cluster=0.5)
    ref = fr.reference(x16, t16, mode, nt)
    assert float(ref["undecided"].mean()) <= 1e-3                      # float64 alone: at most 0.1 % of a case's elements (here: none, or nearly)
    r = fr.grade(fr.emulate(x16, t16, mode, nt), x16, t16, mode, nt)
    print(M, D, mode, nt, {k: round(v, 4) for k, v in r.items()})
    assert max(r[k] for k in ("loss", "rows", "inv_norm", "dx")) <= 1.0, r


def planted():
    return fr.make_case(33, 520, 3, planted_equal_rows=3, cluster=0.5)


def ratios(walk, mode, nt):
    x16, t16 = planted()
    ref = fr.reference(x16, t16, mode, nt)
    e = fr.emulate(x16, t16, mode, nt, walk=walk)
    return {k: fr.worst_ratio(e[k], ref[k], ref["tol_" + k]) for k in ("loss", "rows", "dx")}


@pytest.mark.parametrize("mode,nt", MODES)
def test_documented_walk_on_the_planted_case(mode, nt):
    """Three rows of t ARE x's: under normalize_t their differences are exact zeros in float64 and in the walk (tolerance 0, error 0)."""
    r = ratios("documented", mode, nt)
    assert max(r.values()) <= 1.0, r


def test_wrong_walks_are_outside_the_tolerances():
    r = ratios("n_rounded_to_fp16", "l1", False)
    assert r["rows"] > 1.0 and r["dx"] > 1.0, r                         # torch's fp16 restatement: the normalised row rounded to fp16
    r = ratios("n_rounded_to_fp16", "cos", True)
    assert r["rows"] > 1.0 and r["dx"] > 1.0, r
    r = ratios("sgn0_is_plus", "l1", True)
    assert r["dx"] > 1.0 and r["rows"] <= 1.0, r                        # only the gradient at an exact zero tells
    for mode, nt in MODES:
        r = ratios("no_projection", mode, nt)
        assert r["dx"] > 1.0 and r["loss"] <= 1.0, (mode, nt, r)
    r = ratios("l1_mean_over_rows_only", "l1", False)
    assert r["loss"] > 1.0 and r["dx"] > 1.0 and r["rows"] <= 1.0, r


def test_float64_identities():
    x16, t16 = fr.make_case(17, 64, 2)
    same = fr.reference(x16, x16, "l1", True)
    assert same["loss"] == 0.0 and not same["dx"].any() and not same["tol_dx"].any()          # exactly zero, graded with a tolerance of zero
    cos = fr.reference(x16, x16, "cos", True)
    assert abs(cos["loss"]) < 1e-15 and np.abs(cos["dx"]).max() < 1e-15 and cos["tol_dx"].min() > 0
    # dx is orthogonal to x (the loss does not depend on the length of x), in either mode
    for mode in ("l1", "cos"):
        ref = fr.reference(x16, t16, mode, False)
        assert np.abs((ref["dx"] * x16.astype(np.float64)).sum(1)).max() < 1e-15
    # a zero row is NaN in its own term and the loss only
    z = x16.copy()
    z[5] = 0
    ref, base = fr.reference(z, t16, "l1", False, mean_over=17), fr.reference(x16, t16, "l1", False)
    keep = np.arange(17) != 5
    assert np.isnan(ref["loss"]) and np.isnan(ref["rows"][5]) and np.array_equal(ref["rows"][keep], base["rows"][keep])
    assert np.isnan(ref["dx"][5]).all() and np.array_equal(ref["dx"][keep], base["dx"][keep])
    emu = fr.emulate(z, t16, "l1", False)
    assert np.isnan(emu["loss"]) and np.isnan(emu["dx"][5]).all() and np.isfinite(emu["dx"][keep]).all()


def test_block_sum_order_and_empty_loss():
    a = (np.arange(1, 2052, dtype=np.float32) * np.float32(1.0001)).astype(np.float32)
    one = fr.loss_of(a[:1024], 1024)
    two = fr.loss_of(a, 2051)
    assert one.dtype == np.float32 and two.dtype == np.float32
    assert abs(float(two) - a.astype(np.float64).sum() / 2051) <= 2.0 ** -24 * 30 * float(two)
    assert fr.loss_of(np.zeros(0, dtype=np.float32), 1).view(np.int32) == 0
