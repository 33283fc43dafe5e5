"""The forward row passes between the GEMMs (csrc/pclip_layernorm.hip: layernorm_kernel, layernorm_pf_kernel with and without its LDS copy of gamma / beta,
add_layernorm_kernel; csrc/pclip_stem.hip: vit_embed_ln_kernel, assemble_tokens_kernel, text_embed_kernel, gather_eot_kernel; csrc/pclip_proto.hip:
l2norm_rows_kernel, row_sqnorm_kernel; csrc/pclip_resnet.hip: attnpool_tokens_kernel, avgpool_kernel) in float64 torch from the fp16 operands, with the per-element
tolerance they are graded with (tests/test_row_passes_cpu.py, tests/test_gpu_row_passes.py), an fp32 emulation of the lane layout in several summation orders,
wrong kernels the tolerance must reject, and the input families.  The reference is the MATHEMATICAL function of the fp16 operands, not the rounded chain.  Nothing
in a tolerance is chosen: every term is a rounding the kernels' source shows.

ROUNDING POINTS (mirrored at the top of csrc/pclip_layernorm.hip).  Units u11 = 2^-11 (an fp16 rounding), u24 = 2^-24 (an fp32 rounding), 2^-25 the absolute
error of an fp16 rounding in the subnormal range, gamma_k = k u24 / (1 - k u24) for k fp32 roundings in a row.  A wave owns a row: NCH = 1, 2, 4, 8 chunks of
512 columns for D <= 512, 1024, 2048, 4096, lane l holding columns c 512 + 8 l .. + 7 of chunk c; a lane whose columns lie beyond D adds exact zeros.
LayerNorm, n = 8 NCH + 6 (a lane's 8 NCH terms one after the other, then the six levels lane ^ 32, 16, 8, 4, 2, 1 of the butterfly; any order of that depth passes):
    s     in-lane v_add_f32, butterfly v_add_f32 (DPP / permlane swaps)        |s - sum x| <= gamma_n sum |x|
    mean  = s / D, the IEEE division (v_div_scale, v_rcp, the fma chain, v_div_fmas, v_div_fixup: correctly rounded)
                                                                                e_m = gamma_n sum |x| / D + u24 (|m| + ..)
    t     = v - mean, v_sub_f32                                                 e_t = e_m + u24 (|t| + e_m)
    q     += t t by v_fma_f32 / v_fmac_f32 (ln_sq_acc), then the butterfly      e_q = sum (2 |t| + e_t) e_t + gamma_n sum (|t| + e_t)^2
    V     = q / D + eps: the division, v_add_f32                                e_V = e_q / D + 2 u24 (V + e_q / D)          (eps is the fp32 operand)
    rstd  = 1 / sqrtf(V): v_sqrt_f32 corrected by two v_fma_f32 residuals to the correctly rounded root (the listing has no v_rsq_f32), the IEEE division
                                                                                e_r = (1 - e_V / V)^-1/2 (1 + u24)^2 - 1     (relative)
    o     = (t rstd) g + b: v_(pk_)mul_f32 twice, v_(pk_)add_f32 — contraction is off in ln_affine_dev
                                                                                e_p = rstd |g| ((|t| + e_t) (1 + e_r) (1 + u24)^2 - |t|)
                                                                                e_o = e_p + u24 (|ref| + e_p)
    y     = r16(o), v_cvt_pk_f16_f32                                            tol = e_o + u11 (|ref| + e_o) + 2^-25
On rows of moderate values e_o is a few u24 and tol is one fp16 rounding of the result.  On a row 1000 +- 1.5 the mean's error gamma_n 1000 is multiplied by rstd ~ 1
into several fp16 roundings, and on a constant row t is nothing BUT the mean's error, multiplied by eps^-1/2 = 316: the tolerance follows the conditioning.
add_layernorm        xs = r16(x + delta): the fp32 sum of two fp16 values rounded to fp16 is the correctly rounded sum (24 >= 2 11 + 2 bits: the double rounding is
                     innocuous; the listing has v_pk_add_f16): BIT equality with the float64 sum rounded once; y: the LayerNorm tolerance on xs.
vit_embed_ln         tokens = r16([class ; patch] + pos) as above (exact), x0 = LN_pre(tokens) with the LayerNorm tolerance, and h is graded against LN_1 of the
                     x0 THE KERNEL RETURNED: an exact input, no propagation of x0's tolerance through the second LayerNorm — the tighter of the two options.
layernorm_blend      fp16 gamma / beta (exact operands).  l = r16(o); a = r16(ratio l): v_fma_mixlo_f16 (ONE rounding of the product) or v_mul_f32 + cvt;
                     c = r16(omr res) likewise; y = r16(a + c): v_pk_add_f16, one rounding.  ratio and omr are the fp32 operands.
                       e_l = tol above;   e_a = ratio e_l + u24 ratio (|LN| + e_l), then + u11 (|ratio LN| + ..) + 2^-25
                       e_c = u24 |omr res|, then + u11 (|omr res| + ..) + 2^-25;   e_y = e_a + e_c;   tol = e_y + u11 (|ref| + e_y) + 2^-25
                     c depends on no summation order: it is one of r16(fp32(omr res)) and r16(omr res), and rounding is monotone, so besides the tolerance
                     y must lie in [r16(ratio LN - e_a + min c), r16(ratio LN + e_a + max c)] (`blend_parts`, `grade_interval`): a blend that skips c's rounding leaves it.
                     l2norm_out: ss = sum y^2 (fp16 squares are exact in fp32; 8 NCH in-lane additions and the butterfly), n = r16(sqrtf(ss)), z = r16(y / n)
                     by the IEEE division:  |‖y‖ - N| <= ‖tol‖_2,  e_N = ‖tol‖ + (gamma_n / 2 + u24) (N + ‖tol‖), then + max(u11 (N + ..), 2^-25): the norm's
                     own fp16 rounding, a relative u11 on EVERY element of the row;  e_z = (tol + |ref_z| e_N) / (N - e_N), then + (u24 + u11) (|ref_z| + ..) + 2^-25.
                     N - e_N > 65520: n = inf and z = y / inf = 0 exactly; N + e_N < 65520: finite; between the two the row is undecided (`norm_zone`).
                     sq_out = sum of the squares of the fp16 values the kernel STORED, n additions of exact squares: |sq - sum z^2| <= (n + 1) u24 sum z^2.
l2norm_rows          y = r16(x / r16(‖x‖)): the chain above with an exact x (tol = 0): ss, the correctly rounded sqrtf, r16, then RowDiv (pclip_common.h): v_rcp_f32
                     refined once, q0 = x y, two residual steps of two v_fma_f32 each — the fma chain of the IEEE division on unscaled operands, the correctly
                     rounded quotient (u24) for a divisor in [2^-60, 2^60]; an infinite or zero divisor takes the compiler's division.
row_sqnorm, sq_out   fp32 sums of exact squares: (n + 1) u24 sum x^2.
attnpool_tokens      row 0: acc += x over HW rows one after the other (v_add_f32), acc / HW (IEEE division), r16, + pos[0] in fp32 (exact enough: above), r16:
                       e_s = (gamma_HW sum |x| / HW + u24 |mean|);  e_1 = e_s + u11 (|mean| + e_s) + 2^-25;  tol = e_1 + u11 (|ref| + e_1) + 2^-25
                     rows 1 .. HW: r16(x + pos), bit equality.
avgpool_nhwc         acc over k^2 values, times fp32(1 / k^2) (relative u24 of its own), one fp16 rounding (v_fma_mixlo_f16 or mul + cvt):
                       e = (gamma_{k^2} + 2 u24) mean |x|;  tol = e + u11 (|ref| + e) + 2^-25
vit_assemble_tokens, text_embed   r16(a + pos): bit equality (text_embed clamps ids to [0, vocab - 1]).   gather_eot: the row of torch.argmax, bit equality.
OVERFLOW of an element follows gemm_fwd_ref.grade; no LayerNorm result of the families below comes near 65520 (`undecided_share` is 0)."""
import numpy as np
import torch

from attention_bwd_ref import U11, U24, U25, r16                     # noqa: F401
from gemm_fwd_ref import F16_EDGE, grade, r16x, undecided_share      # noqa: F401

FAMILIES = ("normal", "offset", "constant", "large", "tiny", "outlier")
ORDERS = ("kernel", "desc", "pairwise")
LN_VARIANTS = ("one_pass_variance", "no_eps", "tail_chunk_dropped", "divide_by_padded_width", "affine_from_previous_chunk", "stale_row")
BLEND_VARIANTS = ("residual_unrounded", "norm_unrounded")
EOT_VARIANTS = ("last_maximum", "lane_order_tie")
SUB_MIN = 2.0 ** -24                                                  # the smallest fp16 subnormal
F16_MIN_NORMAL = 2.0 ** -14


def nch(D):
    return 1 if D <= 512 else 2 if D <= 1024 else 4 if D <= 2048 else 8


def gam(k):
    return k * U24 / (1 - k * U24)


def f32(x):
    return float(np.float32(x))


def r32(x):
    return x.to(torch.float32).to(torch.float64)


def r16_sum(a16, b16):
    """r16(a + b) of two fp16 tensors as ONE rounding of the exact (float64) sum, as fp16."""
    return r16x((a16.double() + b16.double()).cpu()).half()


# ---- references and tolerances (float64, on the operands' device) -------------------------------------------------------------------------------------------
def ln_parts(x16, gamma, beta, eps=1e-5):
    """(ref, e_o, tol) of LayerNorm over the last axis: e_o is the error of the fp32 result before its fp16 rounding."""
    x, g, b = x16.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    n, eps = 8 * nch(D) + 6, f32(eps)
    kd = dict(dim=-1, keepdim=True)
    m = x.mean(**kd)
    t = x - m
    V = (t * t).sum(**kd) / D + eps
    rstd = V.rsqrt()
    ref = t * rstd * g + b
    e_m = gam(n) * x.abs().sum(**kd) / D
    e_m = e_m + U24 * (m.abs() + e_m)
    e_t = e_m + U24 * (t.abs() + e_m)
    e_q = ((2 * t.abs() + e_t) * e_t).sum(**kd) + gam(n) * ((t.abs() + e_t) ** 2).sum(**kd)
    e_V = e_q / D + 2 * U24 * (V + e_q / D)
    e_r = (1 - (e_V / V).clamp(max=1.0)).rsqrt() * (1 + U24) ** 2 - 1          # (infinite where the statistics carry no information: e_V >= V)
    e_p = rstd * g.abs() * ((t.abs() + e_t) * (1 + e_r) * (1 + U24) ** 2 - t.abs())
    e_o = e_p + U24 * (ref.abs() + e_p)
    return ref, e_o, e_o + U11 * (ref.abs() + e_o) + U25


def ln_reference(x16, gamma, beta, eps=1e-5):
    ref, _, tol = ln_parts(x16, gamma, beta, eps)
    return ref, tol


def blend_parts(h16, gamma16, beta16, res16, ratio, omr, eps=1e-5):
    """The blend before the optional row normalise: (ref, tol, (lo, hi)) with the monotone interval of the docstring (fp16 values as float64)."""
    ratio, omr = f32(ratio), f32(omr)
    ln, _, e_l = ln_parts(h16, gamma16, beta16, eps)
    res = res16.double()
    a, c = ratio * ln, omr * res
    e_a = abs(ratio) * e_l + U24 * abs(ratio) * (ln.abs() + e_l)
    e_a = e_a + U11 * (a.abs() + e_a) + U25
    e_c = U24 * c.abs()
    e_c = e_c + U11 * (c.abs() + e_c) + U25
    ref, e_y = a + c, e_a + e_c
    tol = e_y + U11 * (ref.abs() + e_y) + U25
    c1, c2 = r16(r32(c)), r16x(c.cpu()).to(c.device)
    wide = e_a * (1 + 1e-9) + 1e-30                                            # (the float64 arithmetic of this very line)
    lo = r16x((a - wide + torch.minimum(c1, c2)).cpu()).to(c.device)
    hi = r16x((a + wide + torch.maximum(c1, c2)).cpu()).to(c.device)
    return ref, tol, (lo, hi)


def norm_parts(ref, tol):
    """Row normalise behind values `ref` known to `tol` (tol = 0: exact fp16 operands): (ref_z, tol_z, zone) with zone [R] = +1 where the rounded norm is
    certainly infinite (z must be exact zeros: ref_z = 0, tol_z = 0), -1 where it is certainly finite, 0 undecided."""
    D = ref.shape[-1]
    n = 8 * nch(D) + 6
    kd = dict(dim=-1, keepdim=True)
    N = (ref * ref).sum(**kd).sqrt()
    tn = (tol * tol).sum(**kd).sqrt() if torch.is_tensor(tol) else torch.zeros_like(N)
    e_N = tn + (gam(n) / 2 + U24) * (N + tn)
    e_N = e_N + torch.maximum(U11 * (N + e_N), torch.full_like(N, U25))
    zone = torch.where(N - e_N > F16_EDGE, 1, torch.where(N + e_N < F16_EDGE, -1, 0)).squeeze(-1)
    z = ref / N
    e_z = (tol + z.abs() * e_N) / (N - e_N).clamp_min(1e-300)
    e_z = torch.where(N > e_N, e_z, torch.full_like(e_z, float("inf")))
    tol_z = e_z + (U24 + U11) * (z.abs() + e_z) + U25
    inf_row = (zone == 1).unsqueeze(-1)
    return torch.where(inf_row, torch.zeros_like(z), z), torch.where(inf_row, torch.zeros_like(z), tol_z), zone


def sq_bound(y16):
    """(sum y^2 in float64, bound) of the fp32 sum of the exact squares of the fp16 values `y16` [R, D]."""
    D = y16.shape[-1]
    s = (y16.double() ** 2).sum(-1)
    return s, (8 * nch(D) + 7) * U24 * s


def grade_sq(sq, y16):
    """worst |sq - sum y^2| / bound; a row of zeros must give exactly 0; infinity for a NaN."""
    s, bound = sq_bound(y16)
    sq = sq.double().to(s.device)
    if bool(torch.isnan(sq).any()):
        return float("inf")
    err = (sq - s).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def grade_interval(got, lo, hi):
    """0 where every element of `got` lies in [lo, hi], infinity otherwise."""
    got = got.double().to(lo.device)
    return 0.0 if bool(((got >= lo) & (got <= hi)).all()) else float("inf")


def grade_zero_rows(got, zone):
    """Rows whose rounded norm is certainly infinite must hold zeros (of either sign)."""
    rows = (zone == 1).to(got.device)
    return 0.0 if bool((got[rows] == 0).all()) else float("inf")


def attnpool_reference(x16, pos16, B, HW, C):
    """tokens [B, HW + 1, C]: (ref, tol) of row 0 as [B, C] and the exact rows 1 .. HW as fp16 [B, HW, C]."""
    x, pos = x16.double().view(B, HW, C), pos16.double()
    mean = x.mean(1)
    e_s = gam(HW) * x.abs().sum(1) / HW
    e_s = e_s + U24 * (mean.abs() + e_s)
    e_1 = e_s + U11 * (mean.abs() + e_s) + U25
    ref = mean + pos[0]
    return ref, e_1 + U11 * (ref.abs() + e_1) + U25, r16_sum(x16.view(B, HW, C), pos16[1:].unsqueeze(0).expand(B, HW, C))


def avgpool_reference(x16, B, H, W, C, k):
    """(ref, tol) [B * (H / k) * (W / k), C] of nn.AvgPool2d(k) on NHWC rows."""
    x = x16.double().view(B, H // k, k, W // k, k, C)
    ref, mag = x.mean((2, 4)).reshape(-1, C), x.abs().mean((2, 4)).reshape(-1, C)
    e = (gam(k * k) + 2 * U24) * mag
    return ref, e + U11 * (ref.abs() + e) + U25


def assemble_reference(patch16, cls16, pos16, B, G2, W):
    """fp16 [B (G2 + 1), W]: r16([class ; patch] + pos), exact."""
    tok = torch.cat([cls16.view(1, 1, W).expand(B, 1, W), patch16.view(B, G2, W)], 1)
    return r16_sum(tok, pos16.view(1, G2 + 1, W).expand(B, G2 + 1, W)).view(B * (G2 + 1), W)


def text_embed_reference(tokens, emb16, pos16):
    B, L = tokens.shape
    ids = tokens.long().clamp(0, emb16.shape[0] - 1)
    return r16_sum(emb16[ids], pos16.view(1, L, -1).expand(B, L, -1)).view(B * L, -1)


# ---- emulation: the lane layout in fp32 on the CPU -----------------------------------------------------------------------------------------------------------
_IDX = torch.arange(64)


def _butterfly(v, levels=(32, 16, 8, 4, 2, 1)):
    for off in levels:
        v = v + v[:, _IDX ^ off]
    return v[:, :1]


def _layout(v, D, cols=None):
    """[R, D] float32 -> per lane its 8 NCH values in the kernel's order [R, 64, 8 NCH] (zeros beyond D) and the mask of the first `cols` (default D) columns
    [64, 8 NCH]."""
    R, N = v.shape[0], nch(D) * 512
    p = torch.zeros(R, N, dtype=torch.float32)
    p[:, :D] = v
    mask = torch.arange(N) < (D if cols is None else cols)
    lay = lambda a: a.view(-1, nch(D), 64, 8).permute(0, 2, 1, 3).reshape(-1, 64, nch(D) * 8)
    return lay(p), lay(mask.view(1, N))[0]


def wave_reduce(terms, order="kernel", square=False):
    """Row sums [R, 1] (float32) of `terms` [R, 64, K] in the lane layout: in-lane in `order`, then across the lanes.  square: the terms are t, accumulated
    as q = fma(t, t, q) (kernel / desc) or as rounded squares (pairwise)."""
    K = terms.shape[-1]
    if order == "pairwise":
        leaves = [(terms[..., k] * terms[..., k]) if square else terms[..., k] for k in range(K)]
        while len(leaves) > 1:
            leaves = [leaves[i] + leaves[i + 1] for i in range(0, len(leaves), 2)]
        return _butterfly(leaves[0], (1, 2, 4, 8, 16, 32))
    acc = torch.zeros(terms.shape[:2], dtype=torch.float32)
    for k in (range(K - 1, -1, -1) if order == "desc" else range(K)):
        t = terms[..., k]
        acc = (acc.double() + t.double() * t.double()).float() if square else acc + t          # the product of two fp32 values is exact in float64: one rounding
    return _butterfly(acc)


def emulate_ln(x16, gamma, beta, eps=1e-5, order="kernel", variant=None):
    """The kernels' LayerNorm chain on the CPU: the fp32 result before its fp16 rounding, [R, D] float32.  variant: None or one of LN_VARIANTS, the WRONG kernels:
      one_pass_variance           E[x^2] - mean^2 in fp32
      no_eps                      rstd = 1 / sqrt(var)
      tail_chunk_dropped          the last 8 columns are missing from the statistics
      divide_by_padded_width      sums divided by 512 NCH
      affine_from_previous_chunk  gamma / beta of column d - 512 from the second chunk on
      stale_row                   mean and rstd of the previous row (row 0: of the last)"""
    assert variant is None or variant in LN_VARIANTS, variant
    x = x16.float()
    R, D = x.shape
    v, mask = _layout(x, D)
    stat = _layout(x[:1], D, D - 8)[1] if variant == "tail_chunk_dropped" else mask
    Dd = torch.tensor(float(nch(D) * 512 if variant == "divide_by_padded_width" else D), dtype=torch.float32)
    mean = wave_reduce(v * stat, order) / Dd
    if variant == "one_pass_variance":
        var = wave_reduce(v * stat, order, square=True) / Dd - mean * mean
    else:
        var = wave_reduce((v - mean.unsqueeze(-1)) * stat, order, square=True) / Dd
    rstd = 1.0 / torch.sqrt(var if variant == "no_eps" else var + torch.tensor(eps, dtype=torch.float32))
    if variant == "stale_row":
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    g, b = gamma.float(), beta.float()
    if variant == "affine_from_previous_chunk":
        g, b = torch.cat([g[:512], g[:-512]]), torch.cat([b[:512], b[:-512]])
    return ((x - mean) * rstd) * g + b


def emulate_blend(h16, gamma16, beta16, res16, ratio, omr, l2norm=False, eps=1e-5, order="kernel", variant=None):
    """(y fp16, sq_out float32 [R]) of MODE 1.  variant: residual_unrounded (a + omr res without c's own fp16 rounding), norm_unrounded (y / sqrtf(ss))."""
    assert variant is None or variant in BLEND_VARIANTS, variant
    ratio, omr = torch.tensor(ratio, dtype=torch.float32), torch.tensor(omr, dtype=torch.float32)
    D = h16.shape[-1]
    l = emulate_ln(h16, gamma16, beta16, eps, order).half().float()
    c = omr * res16.float()
    y = ((ratio * l).half().float() + (c if variant == "residual_unrounded" else c.half().float())).half()
    if l2norm:
        n = torch.sqrt(wave_reduce(_layout(y.float(), D)[0], order, square=True))
        y = (y.float() / (n if variant == "norm_unrounded" else n.half().float())).half()
    return y, wave_reduce(_layout(y.float(), D)[0], order, square=True)[:, 0]


def emulate_l2norm(x16, order="kernel"):
    n = torch.sqrt(wave_reduce(_layout(x16.float(), x16.shape[-1])[0], order, square=True)).half().float()
    y = (x16.float() / n).half()
    return y, wave_reduce(_layout(y.float(), x16.shape[-1])[0], order, square=True)[:, 0]


def eot_index(tokens, variant=None):
    """gather_eot_kernel's position per row of `tokens` [B, L] (int64): lane l keeps the first maximum over l, l + 64, .. (ids as fp32), the wave the greatest
    value with the lowest position.  variant: last_maximum (>= in the lane and the highest position across lanes), lane_order_tie (a tie across lanes goes to
    the lower LANE, not the lower position)."""
    assert variant is None or variant in EOT_VARIANTS, variant
    out = []
    for row in tokens.tolist():
        best = []                                                    # (value, position, lane)
        for lane in range(min(64, len(row))):
            bv, bi = -float("inf"), 0x7fffffff
            for l in range(lane, len(row), 64):
                t = f32(row[l])
                if t > bv or (variant == "last_maximum" and t == bv):
                    bv, bi = t, l
            best.append((bv, bi, lane))
        top = max(b[0] for b in best)
        tied = [b for b in best if b[0] == top]
        out.append(max(b[1] for b in tied) if variant == "last_maximum" else min(tied, key=lambda b: b[2])[1] if variant == "lane_order_tie"
                   else min(b[1] for b in tied))
    return torch.tensor(out)


# ---- input families ------------------------------------------------------------------------------------------------------------------------------------------
def family_rows(family, R, D, g):
    """[R, D] float32 draws of one family (rounded to fp16 by `rows`):
      normal    N(0.3, 2)
      offset    1000 + 0.5 k, k an integer in [-3, 3]: the mean's fp32 error times rstd ~ 1 is several fp16 roundings of the result; one-pass variances cancel
      constant  every element equal (+-(1 .. 4)): the variance is 0, eps and the mean's rounding decide the result
      large     magnitude uniform in [3e4, 6.5e4], random sign
      tiny      N(0, 3e-4): the variance is below eps
      outlier   N(0, 0.05) with the LAST column at 60 000: the tail chunk dominates the statistics"""
    rn = lambda *s: torch.randn(*s, generator=g)
    if family == "normal":
        return 0.3 + 2 * rn(R, D)
    if family == "offset":
        return 1000 + 0.5 * torch.randint(-3, 4, (R, D), generator=g).float()
    if family == "constant":
        c = (1 + 3 * torch.rand(R, 1, generator=g)) * (torch.randint(0, 2, (R, 1), generator=g).float() * 2 - 1)
        return c.expand(R, D).clone()
    if family == "large":
        return (3e4 + 3.5e4 * torch.rand(R, D, generator=g)) * (torch.randint(0, 2, (R, D), generator=g).float() * 2 - 1)
    if family == "tiny":
        return 3e-4 * rn(R, D)
    if family == "outlier":
        x = 0.05 * rn(R, D)
        x[:, -1] = 60000.0
        return x
    raise KeyError(family)


def rows(R, D, seed, families=FAMILIES):
    """fp16 [R, D], row i of family i mod len(families); `row_families` names them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(R, D)
    for i, fam in enumerate(families):
        k = len(range(i, R, len(families)))
        if k:
            x[i::len(families)] = family_rows(fam, k, D, g)
    return x.half()


def row_families(R, families=FAMILIES):
    return [families[i % len(families)] for i in range(R)]


def l2norm_rows_input(R, D, seed):
    """`rows` with two edge rows appended: the smallest subnormals (+-2^-24) and a row of 30 000s, whose norm (>= 84 852) rounds to fp16's infinity."""
    g = torch.Generator().manual_seed(seed + 1)
    sub = SUB_MIN * (torch.randint(0, 2, (1, D), generator=g).float() * 2 - 1)
    return torch.cat([rows(R, D, seed), sub.half(), torch.full((1, D), 30000.0).half()])


def affine(D, seed, half=False):
    """gamma = 1 + 0.3 N(0, 1), beta = 0.2 N(0, 1): fp32, or rounded to fp16 for the blend's fp16 affine."""
    g = torch.Generator().manual_seed(seed + 7)
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    return (gamma.half(), beta.half()) if half else (gamma, beta)


def by_family(got, ref, tol, R, families=FAMILIES):
    """family -> worst ratio over its rows (row i belongs to families[i mod len(families)]; a family may be named more than once)."""
    out = {}
    for i, fam in enumerate(families):
        if i < R:
            out[fam] = max(out.get(fam, 0.0), grade(got[i::len(families)], ref[i::len(families)], tol[i::len(families)]))
    return out


# ---- gather_eot token patterns -------------------------------------------------------------------------------------------------------------------------------
def eot_patterns(L, seed=0):
    """name -> int64 row [L] of token ids; only the patterns that exist at this L."""
    g = torch.Generator().manual_seed(seed + L)
    base = lambda: torch.randint(1, 400, (L,), generator=g)
    out = {}
    t = base(); t[0] = 49407; out["max_first"] = t
    t = base(); t[L - 1] = 49407; out["max_last"] = t
    if L > 64:
        t = base(); t[64] = 49407; out["max_at_64"] = t
        t = base(); t[0] = 49407; t[64] = 49407; out["twice_in_a_lane"] = t          # lane 0 holds positions 0 and 64
    if L > 67:
        t = base(); t[5] = 49407; t[67] = 49407; out["later_position_in_lower_lane"] = t          # position 67 is lane 3's, position 5 lane 5's
    if L > 1:
        t = base(); t[L // 2] = 49407; t[L - 1] = 49407; out["twice_across_lanes"] = t
    out["all_equal"] = torch.full((L,), 7, dtype=torch.int64)
    t = torch.randint(49000, 49407, (L,), generator=g); t[(2 * L) // 3] = 49407; out["eot_among_high_ids"] = t
    t = torch.randint(-500, 500, (L,), generator=g); t[L // 3] = 600; out["mixed_sign"] = t
    if L > 1:
        t = -torch.randint(1, 500, (L,), generator=g); t[L - 1] = 0; out["negative_but_last"] = t
    return {k: v.long() for k, v in out.items()}


def eot_all_negative(L, seed=0):
    """A row of negative ids, its greatest one twice: torch.argmax takes the first.  (A library built before the kernel's fix reads out of bounds on it.)"""
    g = torch.Generator().manual_seed(seed + 31 * L)
    t = -torch.randint(10, 500, (L,), generator=g)
    t[L // 2] = -3
    t[L - 1] = -3
    return t.long()
