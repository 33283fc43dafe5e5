"""The tolerances of the fp32 training kernels (tests/train_f32_ref.py) checked without a GPU: a plain fp32 emulation of every kernel stays inside them at every case of
the lists the GPU test runs (the GEMM and the column sum in two summation orders, on the split and the unsplit route), wrong-on-purpose kernels land at >= 10 x the tolerance
where they differ, the restated route conditions give the slab counts the cases are named for, the float64 references equal autograd of the formulas, and the entries
refuse bad shapes and null pointers before any launch.  The printed ratios are the record of the bounds' headroom (quoted in train_f32_ref's docstring)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_f32_ref as ref                                         # noqa: E402
from train_f32_ref import worst_ratio                               # noqa: E402


def _soft_args(case):
    di, dt, labels, dp = ref.soft_inputs(case)
    return di, dt, labels, dp, case.Q + case.q_extra


def _grade_nll_grad(case, variant=None):
    di, dt, labels, _, qt = _soft_args(case)
    want, tol, p, tol_p = ref.nll_grad_reference(di, dt, labels, case.alpha, case.beta, qt)
    got = ref.nll_grad_emulate(di, dt, labels, case.alpha, case.beta, qt, variant)
    ratios = [worst_ratio(got[k], want[k], tol[k]) for k in ("gi", "gt", "rowsum", "nll")]
    return max(ratios + [ref.grade_argmax(got["argmax"], got["pmax"], p, tol_p, ref.tie_classes(di, dt, case.beta))])


def _grade_fuse(case, variant=None):
    di, dt, _, dp, _ = _soft_args(case)
    want, tol = ref.fuse_bwd_reference(di, dt, dp, case.alpha, case.beta)
    got = ref.fuse_bwd_emulate(di, dt, dp, case.alpha, case.beta, variant)
    return max(worst_ratio(got[k], want[k], tol[k]) for k in ("gi", "gt", "rowsum"))


def _grade_nll_rows(case, variant=None):
    p32, labels = ref.soft_p32(case), ref.soft_inputs(case)[2]
    nll, tol, pmax, am = ref.nll_rows_reference(p32, labels)
    g_nll, g_pmax, g_am = ref.nll_rows_emulate(p32, labels, variant)
    exact = torch.equal(g_am, am) and torch.equal(g_pmax, pmax)
    return max(worst_ratio(g_nll, nll, tol), 0.0 if exact else float("inf"))


def _grade_gemm(case, S, kper, descending=False, variant=None):
    want, tol = ref.gemm_reference(case, S)
    return worst_ratio(ref.gemm_emulate(case, S, kper, descending, variant), want, tol)


def _grade_colsum(case, rb, descending=False, variant=None):
    want, tol = ref.colsum_reference(case)
    return worst_ratio(ref.colsum_emulate(case, rb, descending, variant), want, tol)


def _grade_ce(R, C, family, variant=None):
    S, scale = ref.ce_inputs(R, C, family)
    (loss, dS), (tol_loss, tol_dS) = ref.ce_reference(S, scale)
    g_loss, g_dS = ref.ce_emulate(S, scale, variant)
    return max(worst_ratio(g_loss, loss, tol_loss), worst_ratio(g_dS, dS, tol_dS))


def _grade_l2_bwd(R, D, family, accumulate, variant=None):
    x, gy, gx0 = ref.l2_inputs(R, D, family)
    want, tol = ref.l2_bwd_reference(x, gy, gx0 if accumulate else None)
    return worst_ratio(ref.l2_bwd_emulate(x, gy, gx0 if accumulate else None, variant=variant), want, tol)


# ---- the reference stays inside ---------------------------------------------------------------------------------------------------------------------------------------
def test_gemm_emulation_stays_inside():
    worst = {False: 0.0, True: 0.0}
    for case in ref.GEMM_CASES:
        S, kper = ref.gemm_slabs(case)
        for route in {(S, kper), (1, case.K)}:                      # a split case also runs unsplit: both must grade
            for desc in (False, True):
                r = _grade_gemm(case, *route, descending=desc)
                worst[desc] = max(worst[desc], r)
                assert r <= 1.0, (case, route, desc, r)
    print(f"gemm_f32: fp32 emulation at {worst[False]:.3f} (k ascending), {worst[True]:.3f} (k descending) of the tolerance over {len(ref.GEMM_CASES)} cases")


def test_colsum_emulation_stays_inside():
    worst = {False: 0.0, True: 0.0}
    for case in ref.COLSUM_CASES:
        for rb in {ref.colsum_route(case.R, case.C, ref.colsum_ws_bytes(case)), 1}:
            for desc in (False, True):
                r = _grade_colsum(case, rb, desc)
                worst[desc] = max(worst[desc], r)
                assert r <= 1.0, (case, rb, desc, r)
    print(f"colsum_f32: fp32 emulation at {worst[False]:.3f} (rows ascending), {worst[True]:.3f} (descending) of the tolerance")


def test_addscaled_emulation_stays_inside():
    worst = 0.0
    for R, D, fam in ref.ADDSCALED_CASES:
        c, x, rs, s = ref.addscaled_inputs(R, D, fam)
        worst = max(worst, worst_ratio(ref.addscaled_emulate(c, x, rs, s), *ref.addscaled_reference(c, x, rs, s)))
    print(f"addscaled_rows: fp32 emulation at {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_softmax_emulations_stay_inside():
    cases = ref.SOFT_CASES + [ref.SOFT_BIG]
    for name, grade in (("nll_grad", _grade_nll_grad), ("fuse_probs_backward", _grade_fuse), ("nll_rows", _grade_nll_rows)):
        ratios = {c: grade(c) for c in cases}
        print(f"{name}: fp32 emulation at {max(ratios.values()):.3f} of the tolerance over {len(cases)} cases")
        assert max(ratios.values()) <= 1.0, (name, max(ratios, key=ratios.get))
    worst = 0.0
    for case in cases:
        p32, labels = ref.soft_p32(case), ref.soft_inputs(case)[2]
        want, tol = ref.nll_mean_bwd_reference(p32, labels, 0.37)
        got = ref.nll_mean_bwd_emulate(p32, labels, 0.37)
        assert bool((got[want == 0] == 0).all())
        worst = max(worst, worst_ratio(got, want, tol))
    print(f"nll_mean_backward: fp32 emulation at {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_softmax_cases_cover_the_issue():
    cases = ref.SOFT_CASES
    assert {c.beta for c in cases} == {-3.0, 0.0, 0.7, 12.0, 100.0} and {c.alpha for c in cases} == {0.0, 0.2, 1.0}
    assert {c.Q for c in cases} == {1, 3, 4, 5, 23} and {c.N for c in cases} == {1, 2, 63, 64, 65, 130, 1000}
    assert any(c.q_extra for c in cases) and {c.family for c in cases} >= {"dist", "ties", "offset", "tiny", "normal"}
    for c in cases + [ref.SOFT_BIG]:
        di, dt, labels, _ = ref.soft_inputs(c)
        assert int(labels.min()) >= 0 and int(labels.max()) < c.N                     # labels are always inside [0, N)
        if c.family == "dist":
            assert float(di.min()) >= 0 and float(di.max()) <= 4.0001
    di, _, _, _ = ref.soft_inputs(ref.SOFT_BIG)
    assert not torch.equal(di[:5], di[ref.ROW_SWEEP:])                                # rows r and r + 32 768 differ


def test_softmax_ce_and_l2norm_emulations_stay_inside():
    worst = max(_grade_ce(*c) for c in ref.CE_CASES)
    print(f"softmax_ce_rows: fp32 emulation at {worst:.3f} of the tolerance")
    assert worst <= 1.0
    fwd = 0.0
    assert {c[0] for c in ref.L2_CASES} == {1, 3, 4, 5, 23} and {c[1] for c in ref.L2_CASES} == {1, 2, 63, 64, 65, 130, 1000}          # the rows and widths launched
    assert ref.L2_BIG[0] == ref.ROW_SWEEP + 5
    for R, D, fam in ref.L2_CASES:
        x, _, _ = ref.l2_inputs(R, D, fam)
        assert x.shape == (R, D)
        want, tol = ref.l2_reference(x)
        got = ref.l2_emulate(x)
        zero, sub = ref.l2_special(R, fam)
        if zero is not None:
            assert bool((got[zero] == 0).all())                                       # the zero row
        if sub is not None:
            assert float(x[sub].norm()) < ref.L2_EPS and bool(x[sub].any())           # the row below eps
        fwd = max(fwd, worst_ratio(got, want, tol))
    bwd = max(_grade_l2_bwd(R, D, fam, acc) for R, D, fam in ref.L2_CASES for acc in (False, True))
    print(f"l2norm_rows_f32: fp32 emulation at {fwd:.3f} of the tolerance; backward at {bwd:.3f}")
    assert fwd <= 1.0 and bwd <= 1.0


# ---- wrong kernels are rejected ---------------------------------------------------------------------------------------------------------------------------------------
def _variant_ratios(variant):
    if variant in ("last_k_dropped", "edge_row_dropped", "edge_col_dropped", "slab_missing", "slab_twice", "beta_per_slab", "alpha_twice"):
        return {c: _grade_gemm(c, *ref.gemm_slabs(c), variant=variant) for c in ref.GEMM_CASES if ref.gemm_variant_differs(c, variant)}
    if variant in ("last_block_dropped", "scale_per_partial"):
        routed = {c: ref.colsum_route(c.R, c.C, ref.colsum_ws_bytes(c)) for c in ref.COLSUM_CASES}
        return {c: _grade_colsum(c, rb, variant=variant) for c, rb in routed.items() if rb > 1 and (variant == "last_block_dropped" or c.mean)}
    if variant == "no_max_subtraction":
        return {c: _grade_nll_grad(c, variant) for c in ref.SOFT_CASES if c.beta == 100.0}
    if variant == "oma_is_alpha":
        out = {("nll_grad", c): _grade_nll_grad(c, variant) for c in ref.SOFT_CASES if c.N > 1 and c.beta != 0}
        out.update({("fuse", c): _grade_fuse(c, variant) for c in ref.SOFT_CASES if c.N > 1 and c.beta != 0})
        return out
    if variant == "Q_for_q_total":
        return {c: _grade_nll_grad(c, variant) for c in ref.SOFT_CASES if c.q_extra and c.N > 1}
    if variant == "label_off_by_one":                                                 # (at beta = 0 every column holds 1 / N: the label's place does not matter)
        return {c: _grade_nll_grad(c, variant) for c in ref.SOFT_CASES if c.N > 1 and c.beta != 0}
    if variant == "ties_highest":
        out = {("nll_grad", c): _grade_nll_grad(c, variant) for c in ref.SOFT_CASES if c.family == "ties" or (c.beta == 0 and c.N > 1)}
        out.update({("nll_rows", c): _grade_nll_rows(c, variant) for c in ref.SOFT_CASES if c.family == "ties"})
        return out
    if variant == "diag_at_0":
        return {c: _grade_ce(*c, variant=variant) for c in ref.CE_CASES if c[0] > 1}
    if variant == "eps_ignored":
        return {c + (acc,): _grade_l2_bwd(*c, acc, variant=variant) for c in ref.L2_CASES for acc in (False, True)
                if ref.l2_special(c[0], c[2]) != (None, None)}
    raise KeyError(variant)


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_wrong_kernels_are_rejected(variant):
    ratios = _variant_ratios(variant)
    assert ratios, f"no listed case at which {variant} differs from the kernel"
    best, least = max(ratios.values()), min(ratios.values())
    print(f"{variant}: {best:.1e} x the tolerance at its clearest case, {least:.1e} at its faintest, {len(ratios)} cases")
    assert best >= 10.0, (variant, ratios)
    if variant == "no_max_subtraction":                                               # the overflow / underflow shows as a non-finite result
        assert best == float("inf")
    if variant in ("ties_highest", "label_off_by_one", "oma_is_alpha", "slab_missing", "slab_twice", "diag_at_0"):
        assert least >= 10.0, (variant, ratios)                                       # these differ clearly wherever they differ


# ---- routes, references, casts ----------------------------------------------------------------------------------------------------------------------------------------
def test_restated_routes_give_the_named_slab_counts():
    for case in ref.GEMM_SPLIT:
        S, kper = ref.gemm_slabs(case)
        assert S == ref.GEMM_EXPECT_S[(case.M, case.N, case.K)], (case, S)
        assert kper % 32 == 0 or S == 1
        if S > 1:                                                                     # four bytes short: the single pass
            assert ref.gemm_route(case.M, case.N, case.K, S * case.M * case.N * 4) == (S, kper)
            assert ref.gemm_route(case.M, case.N, case.K, S * case.M * case.N * 4 - 4) == (1, case.K)
    assert ref.gemm_route(1, 64, 1025, 1 << 20) == (4, 288) and 1025 - 3 * 288 == 161
    assert ref.gemm_route(1, 64, 1024, 0) == (1, 1024)
    assert [ref.colsum_route(R, 64, 1 << 20) for R in (128, 129, 2048, 2049, 4100)] == [1, 5, 64, 64, 64]
    for case in ref.COLSUM_CASES:
        rb = ref.colsum_route(case.R, case.C, ref.colsum_ws_bytes(case))
        assert (rb > 1) == (case.ws is True and case.R > 128), case
        if case.ws is True:                                                           # room for any split: an untouched workspace then proves the condition said no
            assert ref.colsum_ws_bytes(case) == 64 * case.C * 4
    assert any(c.ws is True and c.R == 128 for c in ref.COLSUM_CASES) and any(c.ws is True and c.R == 129 for c in ref.COLSUM_CASES)
    assert {c.R for c in ref.COLSUM_CASES} == {0, 1, 3, 4, 5, 128, 129, 2048, 2049, 4100} and {c.C for c in ref.COLSUM_CASES} == {1, 63, 64, 65, 130}
    assert {c.M for c in ref.GEMM_SMALL} == {c.N for c in ref.GEMM_SMALL} == {1, 33, 64, 65, 129} and {c.K for c in ref.GEMM_SMALL} == {1, 2, 31, 32, 33, 65, 203}


def test_references_equal_autograd():
    case = ref.Soft(5, 65, 0.2, 12.0, 3, "dist")
    di, dt, labels, dp = ref.soft_inputs(case)
    al, oma, be = ref.f32(0.2), ref.f32(1.0 - 0.2), ref.f32(12.0)
    a, b = di.double().requires_grad_(True), dt.double().requires_grad_(True)
    p = al * F.softmax(-be * a, 1) + oma * F.softmax(-be * b, 1)
    (F.nll_loss(torch.log(p), labels, reduction="sum") / 8).backward()
    want, _, p_ref, _ = ref.nll_grad_reference(di, dt, labels, 0.2, 12.0, 8)
    assert torch.allclose(want["gi"], a.grad, rtol=1e-10, atol=1e-14) and torch.allclose(want["gt"], b.grad, rtol=1e-10, atol=1e-14)
    assert torch.allclose(p_ref, p.detach(), rtol=1e-12)
    a.grad, b.grad = None, None
    p = al * F.softmax(-be * a, 1) + oma * F.softmax(-be * b, 1)
    (p * dp.double()).sum().backward()
    want, _ = ref.fuse_bwd_reference(di, dt, dp, 0.2, 12.0)
    assert torch.allclose(want["gi"], a.grad, rtol=1e-10, atol=1e-14) and torch.allclose(want["gt"], b.grad, rtol=1e-10, atol=1e-14)
    x, gy, _ = ref.l2_inputs(5, 64, "normal")
    xd = x.double().requires_grad_(True)
    (F.normalize(xd, dim=1, eps=ref.f32(ref.L2_EPS)) * gy.double()).sum().backward()
    want, _ = ref.l2_bwd_reference(x, gy)
    assert torch.allclose(want[:3], xd.grad[:3], rtol=1e-10, atol=1e-14)          # (rows 3 and 4 are the edge rows: below eps the kernel's documented formula is not autograd's)
    S, scale = ref.ce_inputs(5, 65, "normal")
    Sd = S.double().requires_grad_(True)
    loss = F.cross_entropy(Sd, torch.arange(5), reduction="none")
    (ref.f32(scale) * loss.sum()).backward()
    (w_loss, w_dS), _ = ref.ce_reference(S, scale)
    assert torch.allclose(w_loss, loss.detach(), rtol=1e-12) and torch.allclose(w_dS, Sd.grad, rtol=1e-10, atol=1e-16)


def test_cast_reference_is_round_to_nearest_even():
    """numpy's conversion (the reference of the GPU test) against torch's, and the edges by hand."""
    x = ref.cast_f32_input(100000)
    assert ref.half_bits_equal(x.half(), x)
    sp = ref.cast_f32_specials()
    with np.errstate(over="ignore"):
        h = sp.numpy().astype(np.float16).astype(np.float64)
    by = {float(v): float(o) for v, o in zip(sp.tolist(), h.tolist()) if v == v}
    assert by[2.0 ** -25] == 0.0 and by[3 * 2.0 ** -25] == 2.0 ** -23 and by[5 * 2.0 ** -25] == 2.0 ** -23 and by[2.0 ** -24] == 2.0 ** -24          # ties to even
    assert by[float(np.float32(1.0 + 2.0 ** -11))] == 1.0 and by[float(np.float32(1.0 + 3 * 2.0 ** -11))] == 1.0 + 2.0 ** -9
    assert by[65504.0] == 65504.0 and by[65519.0] == 65504.0 and by[65520.0] == float("inf") and by[-65520.0] == float("-inf") and by[ref.f32(1e38)] == float("inf")
    assert np.isnan(h[[i for i, v in enumerate(sp.tolist()) if v != v]]).all()
    assert np.signbit(sp.numpy().astype(np.float16)[1]) and not np.signbit(sp.numpy().astype(np.float16)[0])                                    # -0 stays -0


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from proto_clip_amd import _lib as L
    return L.load()


P = ctypes.c_void_p(0x1000)                                                           # a placeholder pointer: never dereferenced, the entries refuse (or return) before any launch


@pytest.mark.parametrize("call,msg", [
    (lambda L: L.pclip_gemm_f32(P, 1, 8, 1, P, 0, 8, 1, P, 8, 4, 8, 0, 1.0, 0.0, None, 0, None), b"pclip_gemm_f32: bad shape M=4 N=8 K=0 ldc=8"),
    (lambda L: L.pclip_gemm_f32(P, 1, 8, 1, P, 0, 8, 1, P, 7, 4, 8, 8, 1.0, 0.0, None, 0, None), b"pclip_gemm_f32: bad shape M=4 N=8 K=8 ldc=7"),
    (lambda L: L.pclip_gemm_f32(P, 1, 8, 1, P, 0, 8, 1, None, 8, 4, 8, 8, 1.0, 0.0, None, 0, None), b"pclip_gemm_f32: null pointer"),
    (lambda L: L.pclip_gemm_f32(None, 1, 8, 1, P, 0, 8, 1, P, 8, 4, 8, 8, 1.0, 0.0, None, 0, None), b"pclip_gemm_f32: null pointer"),
    (lambda L: L.pclip_colsum_f32(P, 7, 4, 8, 1.0, P, 0, None, 0, None), b"pclip_colsum_f32: bad shape R=4 C=8 ld=7"),
    (lambda L: L.pclip_colsum_f32(P, 8, 4, 8, 1.0, None, 0, None, 0, None), b"pclip_colsum_f32: null pointer"),
    (lambda L: L.pclip_addscaled_rows_f32(P, 7, P, 8, P, 1.0, 4, 8, None), b"pclip_addscaled_rows_f32: bad shape"),
    (lambda L: L.pclip_addscaled_rows_f32(P, 8, P, 8, None, 1.0, 4, 8, None), b"pclip_addscaled_rows_f32: null pointer"),
    (lambda L: L.pclip_softmax_ce_rows(P, 8, 5, 4, 1.0, P, 8, P, None), b"pclip_softmax_ce_rows: bad R=5 C=4"),
    (lambda L: L.pclip_softmax_ce_rows(P, 8, 4, 8, 1.0, P, 8, None, None), b"pclip_softmax_ce_rows: null pointer"),
    (lambda L: L.pclip_nll_grad(P, P, P, 4, 3, 8, 8, 0.5, 0.5, 1.0, P, P, P, P, P, P, None), b"pclip_nll_grad: bad Q=4 q_total=3 N=8 ldd=8"),
    (lambda L: L.pclip_nll_grad(P, P, P, 4, 4, 8, 7, 0.5, 0.5, 1.0, P, P, P, P, P, P, None), b"pclip_nll_grad: bad Q=4 q_total=4 N=8 ldd=7"),
    (lambda L: L.pclip_nll_grad(P, P, None, 4, 4, 8, 8, 0.5, 0.5, 1.0, P, P, P, P, P, P, None), b"pclip_nll_grad: null pointer"),
    (lambda L: L.pclip_nll_grad(P, P, P, 4, 4, 8, 8, 0.5, 0.5, 1.0, P, P, P, P, P, None, None), b"pclip_nll_grad: null pointer"),
    (lambda L: L.pclip_fuse_probs_backward(P, P, P, 7, 4, 8, 8, 0.5, 0.5, 1.0, P, P, P, None), b"pclip_fuse_probs_backward: bad Q=4 N=8 ldd=8 ldp=7"),
    (lambda L: L.pclip_fuse_probs_backward(P, P, None, 8, 4, 8, 8, 0.5, 0.5, 1.0, P, P, P, None), b"pclip_fuse_probs_backward: null pointer"),
    (lambda L: L.pclip_nll_mean_backward(P, 8, P, 4, 8, P, P, 7, None), b"pclip_nll_mean_backward: bad Q=4 N=8 ldp=8 lddp=7"),
    (lambda L: L.pclip_nll_mean_backward(P, 8, P, 4, 8, None, P, 8, None), b"pclip_nll_mean_backward: null pointer"),
    (lambda L: L.pclip_nll_rows(P, 7, P, 4, 8, P, P, P, None), b"pclip_nll_rows: bad Q=4 N=8 ld=7"),
    (lambda L: L.pclip_nll_rows(P, 8, None, 4, 8, P, P, P, None), b"pclip_nll_rows: null pointer"),
    (lambda L: L.pclip_l2norm_rows_f32(P, P, 4, 0, 1e-12, None), b"pclip_l2norm_rows_f32: bad shape R=4 D=0"),
    (lambda L: L.pclip_l2norm_rows_f32(P, None, 4, 8, 1e-12, None), b"pclip_l2norm_rows_f32: null pointer"),
    (lambda L: L.pclip_l2norm_rows_backward_f32(P, P, None, 4, 8, 1e-12, 0, None), b"pclip_l2norm_rows_backward_f32: null pointer"),
    (lambda L: L.pclip_cast_f16_f32(None, P, 8, None), b"pclip_cast_f16_f32: null pointer"),
    (lambda L: L.pclip_cast_f32_f16(P, None, 8, None), b"pclip_cast_f32_f16: null pointer"),
])
def test_entries_refuse_before_launch(call, msg):
    L = _lib()
    assert call(L) == -1
    assert msg in L.pclip_last_error(), L.pclip_last_error()


@pytest.mark.parametrize("call", [
    lambda L: L.pclip_gemm_f32(P, 1, 8, 1, P, 0, 8, 1, P, 8, 0, 8, 8, 1.0, 0.0, None, 0, None),          # M = 0
    lambda L: L.pclip_gemm_f32(P, 1, 8, 1, P, 0, 8, 1, P, 8, 4, 0, 8, 1.0, 0.0, None, 0, None),          # N = 0
    lambda L: L.pclip_addscaled_rows_f32(P, 8, P, 8, P, 1.0, 0, 8, None),
    lambda L: L.pclip_nll_grad(P, P, P, 0, 4, 8, 8, 0.5, 0.5, 1.0, P, P, P, P, P, P, None),
    lambda L: L.pclip_fuse_probs_backward(P, P, P, 8, 0, 8, 8, 0.5, 0.5, 1.0, P, P, P, None),
    lambda L: L.pclip_nll_mean_backward(P, 8, P, 0, 8, P, P, 8, None),
    lambda L: L.pclip_nll_rows(P, 8, P, 0, 8, P, P, P, None),
    lambda L: L.pclip_softmax_ce_rows(P, 8, 0, 8, 1.0, P, 8, P, None),
    lambda L: L.pclip_l2norm_rows_f32(P, P, 0, 8, 1e-12, None),
    lambda L: L.pclip_l2norm_rows_backward_f32(P, P, P, 0, 8, 1e-12, 0, None),
    lambda L: L.pclip_cast_f16_f32(P, P, 0, None),
    lambda L: L.pclip_cast_f32_f16(P, P, 0, None),
])
def test_empty_calls_return_ok_without_a_launch(call):
    assert call(_lib()) == 0
