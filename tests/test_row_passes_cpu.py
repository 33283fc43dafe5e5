"""The tolerances of the forward row passes (tests/row_passes_ref.py) checked without a GPU: an fp32 emulation of the lane layout stays inside them for every
operation, width, input family and summation order; every wrong kernel lands outside on the family named for it here (a variant that passes on all families fails
the test); on the benign families the tolerance stays near one fp16 rounding of the result, so it cannot have been loosened until everything passes; no element
of these families is undecided between finite and infinite; the gather_eot model agrees with torch.argmax on every token pattern the GPU test runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_passes_ref as ref                                        # noqa: E402
from conftest import observe                                        # noqa: E402

WIDTHS = (8, 64, 520, 768, 1032, 2056, 4096)
R = 24                                                              # four rows of every family
BENIGN = ("normal", "large", "tiny", "outlier")
MEDIAN_CAP = 1.5
# variant -> (the families on which it must be rejected, the widths at which it differs from the right kernel at all)
#   one_pass_variance           cancels only where mean^2 >> var: `offset` (at D = 8 the few terms leave E[x^2] - mean^2 inside the tolerance)
#   no_eps                      matters only where var <~ eps: `constant` (1 / 0) and `tiny`
#   tail_chunk_dropped          `outlier` loses the column that IS its statistics, `normal` and `large` 8 of D terms
#   divide_by_padded_width      D = 4096 is its own padded width
#   affine_from_previous_chunk  needs a second chunk
#   stale_row                   neighbouring rows belong to different families
REJECTED_ON = {
    "one_pass_variance": (("offset",), tuple(D for D in WIDTHS if D >= 64)),
    "no_eps": (("constant", "tiny"), WIDTHS),
    "tail_chunk_dropped": (("normal", "large", "outlier"), WIDTHS),
    "divide_by_padded_width": (("normal", "large", "outlier"), tuple(D for D in WIDTHS if D != 4096)),
    "affine_from_previous_chunk": (("normal", "tiny"), tuple(D for D in WIDTHS if D > 512)),
    "stale_row": (ref.FAMILIES, WIDTHS),
}
_cache = {}


def case(D, half_affine=False):
    key = (D, half_affine)
    if key not in _cache:
        x = ref.rows(R, D, seed=40 + D)
        g, b = ref.affine(D, seed=D, half=half_affine)
        _cache[key] = (x, g, b, ref.ln_reference(x, g, b))
    return _cache[key]


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bound_holds_every_order(D):
    for half_affine in (False, True):
        x, g, b, (want, tol) = case(D, half_affine)
        for order in ref.ORDERS:
            fams = ref.by_family(ref.emulate_ln(x, g, b, order=order).half(), want, tol, R)
            for fam, ratio in fams.items():
                print(f"layernorm D={D} {'fp16' if half_affine else 'fp32'} affine {order} {fam}: emulation at {ratio:.3f} of the bound")
                observe(f"row passes emulation, layernorm, {fam}: |emu - float64| / derived tolerance", ratio, 1.0)
                assert ratio <= 1.0, (D, order, fam, ratio)


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bound_is_one_rounding_on_benign_rows(D):
    x, g, b, (want, tol) = case(D)
    for i, fam in enumerate(ref.FAMILIES):
        w, t = want[i::6], tol[i::6]
        med = float((t / (ref.U11 * w.abs().clamp_min(2.0 ** -14))).median())
        print(f"layernorm D={D} {fam}: median tolerance {med:.2f} fp16 roundings of the result")
        if fam in BENIGN:
            observe(f"row passes, layernorm tolerance, {fam}: median in fp16 roundings of the result", med, MEDIAN_CAP)
            assert med < MEDIAN_CAP, (D, fam, med)
        else:
            assert med > MEDIAN_CAP, (D, fam, med)                  # the conditioning of `offset` and `constant` is in the bound: a fixed ulp count is none
        assert ref.undecided_share(w, t) == 0.0, (D, fam)


@pytest.mark.parametrize("variant", ref.LN_VARIANTS)
def test_layernorm_wrong_kernels_are_rejected(variant):
    families, widths = REJECTED_ON[variant]
    for D in widths:
        x, g, b, (want, tol) = case(D)
        fams = ref.by_family(ref.emulate_ln(x, g, b, variant=variant).half(), want, tol, R)
        print(f"{variant} D={D}: " + ", ".join(f"{k} {v:.3g}" for k, v in fams.items()))
        assert max(fams.values()) > 1.0, (variant, D, "passes on every family")
        for fam in families:
            assert fams[fam] > 1.0, (variant, D, fam, fams[fam])


def blend_case(D, ratio, l2norm):
    h, g, b, _ = case(D, True)
    res = ref.rows(R, D, seed=90 + D)
    omr = ref.f32(1 - ref.f32(ratio))
    want, tol, (lo, hi) = ref.blend_parts(h, g, b, res, ratio, omr)
    zone = None
    if l2norm:
        want, tol, zone = ref.norm_parts(want, tol)
    return h, g, b, res, omr, want, tol, lo, hi, zone


def grade_blend(y, sq, want, tol, lo, hi, zone):
    """family -> worst of: element grade, the monotone interval (no normalise), exact zeros behind an infinite norm, sq_out against the stored values."""
    out = ref.by_family(y, want, tol, R)
    for i, fam in enumerate(ref.FAMILIES):
        extra = ref.grade_sq(sq[i::6], y[i::6])
        if zone is None:
            extra = max(extra, ref.grade_interval(y[i::6], lo[i::6], hi[i::6]))
        else:
            extra = max(extra, ref.grade_zero_rows(y[i::6], zone[i::6]))
        out[fam] = max(out[fam], extra)
    return out


@pytest.mark.parametrize("l2norm", (False, True))
@pytest.mark.parametrize("ratio", (0.2, 1.0, 0.0))
@pytest.mark.parametrize("D", WIDTHS)
def test_blend_bound_holds_every_order(D, ratio, l2norm):
    h, g, b, res, omr, want, tol, lo, hi, zone = blend_case(D, ratio, l2norm)
    if zone is not None:
        assert bool((zone != 0).all()), "a row's norm is undecided between finite and infinite"
        assert bool((zone[3::6] == 1).all()) == (ratio != 1.0)      # the `large` residual rows overflow the norm unless omr = 0
    for order in ref.ORDERS:
        y, sq = ref.emulate_blend(h, g, b, res, ratio, omr, l2norm, order=order)
        for fam, ratio_ in grade_blend(y, sq, want, tol, lo, hi, zone).items():
            print(f"blend D={D} ratio={ratio} l2norm={l2norm} {order} {fam}: emulation at {ratio_:.3f} of the bound")
            observe(f"row passes emulation, layernorm_blend{' + l2norm' if l2norm else ''}, {fam}: worst ratio", ratio_, 1.0)
            assert ratio_ <= 1.0, (D, ratio, l2norm, order, fam, ratio_)
    if ratio == 0.0 and not l2norm:
        assert torch.equal(y, res)                                  # 0 x LN + 1 x res: the residual itself


# residual_unrounded: r16(a + fp32(omr res)) against r16(a + r16(omr res)).  A skipped rounding moves the result TOWARDS the mathematical blend, so the tolerance alone
#   cannot see it; the monotone interval can: c is known exactly, and on `normal` rows (a and c of one size) the two sums round apart on a few per cent of the
#   elements, by more than a's own uncertainty allows.  (`large` residuals are multiples of 16 or 32 times 0.8: no product lies near enough to a rounding boundary.)
# norm_unrounded: the `large` residual rows have a norm that rounds to fp16's infinity: the kernel stores zeros, the variant finite quotients.
@pytest.mark.parametrize("variant,l2norm,family", (("residual_unrounded", False, "normal"), ("norm_unrounded", True, "large")))
def test_blend_wrong_kernels_are_rejected(variant, l2norm, family):
    for D in (520, 1032, 4096):
        h, g, b, res, omr, want, tol, lo, hi, zone = blend_case(D, 0.2, l2norm)
        y, sq = ref.emulate_blend(h, g, b, res, 0.2, omr, l2norm, variant=variant)
        fams = grade_blend(y, sq, want, tol, lo, hi, zone)
        print(f"{variant} D={D}: " + ", ".join(f"{k} {v:.3g}" for k, v in fams.items()))
        assert fams[family] > 1.0, (variant, D, fams)


@pytest.mark.parametrize("D", WIDTHS)
def test_l2norm_bound_holds_every_order(D):
    x = ref.l2norm_rows_input(R, D, seed=60 + D)
    want, tol, zone = ref.norm_parts(x.double(), torch.zeros(x.shape, dtype=torch.float64))
    assert bool((zone != 0).all()) and int(zone[-1]) == 1 and int(zone[-2]) == -1 and bool((zone[3:R:6] == 1).all())
    for order in ref.ORDERS:
        y, sq = ref.emulate_l2norm(x, order)
        ratio = max(ref.grade(y, want, tol), ref.grade_zero_rows(y, zone), ref.grade_sq(sq, y))
        print(f"l2norm_rows D={D} {order}: emulation at {ratio:.3f} of the bound")
        observe("row passes emulation, l2norm_rows: worst ratio", ratio, 1.0)
        assert ratio <= 1.0, (D, order, ratio)
    # a norm left unrounded misses the zeros of the overflowing rows and the subnormal row's 3 x 2^-24 (D = 8: 2.83 x 2^-24)
    n = x.float().pow(2).sum(-1, keepdim=True).sqrt()
    wrong = (x.float() / n).half()
    assert ref.grade_zero_rows(wrong, zone) > 1.0


@pytest.mark.parametrize("L", (1, 6, 64, 65, 77, 130))
def test_gather_eot_model_is_argmax(L):
    pats = ref.eot_patterns(L)
    pats["all_negative"] = ref.eot_all_negative(L)
    toks = torch.stack(list(pats.values()))
    want = torch.argmax(toks, dim=1)
    assert torch.equal(ref.eot_index(toks), want), (list(pats), ref.eot_index(toks), want)
    assert int(want[list(pats).index("all_negative")]) == L // 2 if L > 1 else True
    # the wrong kernels: a last maximum differs wherever the maximum occurs twice, a tie by lane where the later position sits in the lower lane
    for variant, names in (("last_maximum", ("all_equal", "twice_across_lanes", "twice_in_a_lane")), ("lane_order_tie", ("later_position_in_lower_lane",))):
        got = ref.eot_index(toks, variant)
        for name in names:
            if name in pats and L > 1:
                i = list(pats).index(name)
                assert int(got[i]) != int(want[i]), (variant, name, L)
    if L in (77, 130):
        assert "later_position_in_lower_lane" in pats and "twice_in_a_lane" in pats


def test_exact_sums_round_once():
    """r16(fp32(a + b)) of two fp16 values is the correctly rounded sum: the fp32 chain the kernels run equals the float64 sum rounded once, on every pair of
    magnitudes the families hold."""
    x = torch.cat([ref.rows(R, 520, 1), ref.rows(R, 520, 2).flip(0)])
    y = torch.cat([ref.rows(R, 520, 3).flip(0), ref.rows(R, 520, 4)])
    assert torch.equal((x.float() + y.float()).half(), ref.r16_sum(x, y))


def test_pools_bound_holds():
    g = torch.Generator().manual_seed(3)
    for B, HW, C in ((1, 1, 8), (2, 49, 64), (3, 144, 2048)):
        x, pos = torch.randn(B * HW, C, generator=g).half(), (0.5 * torch.randn(HW + 1, C, generator=g)).half()
        want, tol, exact = ref.attnpool_reference(x, pos, B, HW, C)
        acc = torch.zeros(B, C)
        for p in range(HW):
            acc = acc + x.view(B, HW, C)[:, p].float()
        got = ((acc / HW).half().float() + pos[0].float()).half()
        assert ref.grade(got, want, tol) <= 1.0
        assert torch.equal(exact, (x.view(B, HW, C).float() + pos[1:].float()).half())
    for k in (2, 3):
        B, H, W, C = 2, 6, 12, 24
        x = torch.randn(B * H * W, C, generator=g).half()
        want, tol = ref.avgpool_reference(x, B, H, W, C, k)
        v = x.float().view(B, H // k, k, W // k, k, C)
        acc = torch.zeros(B, H // k, W // k, C)
        for dy in range(k):
            for dx in range(k):
                acc = acc + v[:, :, dy, :, dx]
        got = (acc * torch.tensor(1.0 / (k * k), dtype=torch.float32)).half().reshape(-1, C)
        assert ref.grade(got, want, tol) <= 1.0
        assert ref.grade(torch.roll(got, 1, 0), want, tol) > 1.0    # the neighbouring window
