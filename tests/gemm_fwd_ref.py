"""The forward linear kernels (csrc/pclip_linear.hip: linear_fast_kernel on five tile configurations, linear_generic_kernel, linear_small_kernel as the ring
kernel and as split-K with splitk_reduce_kernel; csrc/pclip_gemm4w.hip: linear4w_kernel) with every epilogue of csrc/pclip_epilogue.h, in float64 torch from the
fp16 operands, with the per-element tolerance they are graded with (tests/test_gemm_forward_cpu.py, tests/test_gpu_gemm_forward.py), an fp32 emulation of the
documented chain in several summation orders, wrong kernels the tolerance must reject, and the input families.  The reference is the MATHEMATICAL function of
the exact product of the fp16 operands, not the rounded chain.  Nothing in the tolerance is chosen: every term is a rounding of the kernels.

ROUNDING POINTS (mirrored at the top of csrc/pclip_epilogue.h; the instructions are those of the gfx950 listing).  Units u11 = 2^-11 (an fp16 rounding),
u24 = 2^-24 (an fp32 rounding), 2^-25 for the absolute error of an fp16 rounding in the subnormal range.  acc = sum_k a w over K, z = acc + bias:
    A     = (K + 1) u24 (|bias| + sum_k |a| |w|)          fp32 MFMA accumulation of K exact products (fp16 x fp16 is exact in fp32); the fp32 copy of the
                                                          bias is the accumulators' INITIAL value, so r16(acc + bias) is one rounding.  The convention of e_S
                                                          in attention_fwd_ref.py.  The generic kernel starts from zero and adds the bias in fp32 behind the
                                                          K-loop: the same K + 1 additions.  Split-K: S slabs from zero, added in slice order from zero
                                                          (v_pk_add_f32), then the bias: A = (K + S + 1) u24 (..).
    e_h   = A + u11 (|z| + A) + 2^-25                     h = r16(z), v_cvt(_pk)_f16_f32: the one rounding of act 0, with or without bias; tol = e_h
    act 6 (bias + residual)   y = r16(res + h): ONE v_pk_add_f16 of two fp16 values       tol = e_h + u11 (|ref| + e_h) + 2^-25
    act 2 / 3 (BatchNorm)     c = r16(acc); y = r16(c sc + sh) is ONE v_fma_mixlo/hi_f16: the fp32 product and sum are never rounded to fp32, the fma's exact
                              result is rounded to fp16 once.                              e_v = |sc| e_h,  tol = e_v + u11 (|ref| + e_v) + 2^-25
                              ReLU (v_max_f32) is exact and 1-Lipschitz: the same tolerance around relu(ref).
                              (Compiled as two fp32 operations it would add u24 (|c sc| + |y|); `emulate(fma=False)` runs that chain too.)
    act 5 (BN + res + ReLU)   y2 = relu(r16(y + res)): one v_add_f16 more                  tol = tol_bn + u11 (|ref'| + tol_bn) + 2^-25, ref' before the ReLU
    act 1 (QuickGELU)         h = r16(z); t = r16(1.702f h) is ONE v_fma_mixlo_f16 (no fp32 rounding of the product); the exponent's argument
                              fma(t, -log2(e), 0) is a v_fma_mix_f32: one fp32 rounding, relative u24 on an argument of size |t| log2 e, i.e. |t| u24 relative
                              on the exponential ex, and the same again for the rounded fp32 constant log2(e); v_exp_f32 is 1 ulp (2 u24 on ex; the instruction
                              set manual's figure).  A relative error d on ex moves s = 1 / (1 + ex) by s (1 - s) d = sigmoid'(t) d: it acts like an error
                              d on t.  1 + ex is a v_pk_add_f32 (u24 on s), v_rcp_f32 1 ulp (2 u24 on s); s = r16(..); y = r16(h s) is ONE v_pk_mul_f16.
                                e_t  = 1.702 e_h + u24 |t| + u11 (|t| + 1.702 e_h) + 2^-25           (u24 |t|: 1.702f against 1.702)
                                e_s  = S' (e_t + (2 |t| + 2) u24) + 3 u24 s, then + u11 (s + ..) + 2^-25
                                                                                                      S' = sup of sigmoid' over t +- e_t = sigmoid'(max(|t| - e_t, 0))
                                tol  = s e_h + |z| e_s, then + u11 (|ref| + ..) + 2^-25
                              Where 1.702 |h| leaves fp16's range t is +-inf, the exponential 0 or +inf, s exactly 1 or 0 and y = h or -0: that pushes t AWAY
                              from zero, where sigmoid' only falls, so S' taken at |t| - e_t covers it.
OVERFLOW.  fp16 rounds to infinity from 65520 on.  Where |ref| - tol > 65520 the result must be the infinity of ref's sign; where |ref| + tol < 65520 it must be
finite (and within tol); between the two either is accepted, and `undecided_share` states how many elements that is.  An INTERMEDIATE rounding that overflows
(h, c, y of the chains above) gives an infinite result whatever follows it; the `large` family keeps what follows small (|res|, |shift| <= 4, 1 <= scale <= 1.0625,
and u11 65520 = 32 > 4), so that an intermediate overflow always means |ref| + tol >= 65520.  QuickGELU of h = -inf is -inf x 0 = NaN in the kernels as in
the reference model's own fp16 arithmetic; it is not graded: the QuickGELU draw of `large` keeps the negative pre-activations inside -6.4e4."""
import math

import numpy as np
import torch

from attention_bwd_ref import U11, U24, U25, r16, worst_ratio   # noqa: F401

F16_EDGE = 65520.0
C1702 = float(np.float32(1.702))
LOG2E32 = float(np.float32(1.4426950408889634))
# name -> (bias operand, act): every epilogue the kernels instantiate
EPILOGUES = {"plain": (False, 0), "bias": (True, 0), "gelu": (False, 1), "bias_gelu": (True, 1), "res": (True, 6),
             "bn": (False, 2), "bn_relu": (False, 3), "bn_res_relu": (False, 5)}
# (kind, chunk): k ascending / descending in chunks, chunk partials added pairwise; "bias_last": from zero, the bias added behind the K-loop (generic kernel)
ORDERS = (("asc", 16), ("asc", 32), ("asc", 64), ("desc", 64), ("pairwise", 32), ("bias_last", 64))
VARIANTS = ("drop_tail_chunk", "bias_after_round", "round_between_ktiles", "slab_twice", "slab_dropped", "stale_strip", "residual_neighbour_row",
            "relu_before_residual", "gelu_nan")


def r16x(x):
    """ONE rounding of a float64 tensor to fp16 (numpy converts directly; torch's cast goes through fp32), back as float64; overflows to infinity."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))


def r32(x):
    return x.to(torch.float32).to(torch.float64)


def splitk_slices(K):
    """(S, K-tiles per slice) of splitk_plan (csrc/pclip_linear.hip): a function of K only."""
    steps = K // 64
    per = max(steps // 8, 2)
    return -(-steps // per), per


# ---- reference and tolerance ------------------------------------------------------------------------------------------------------------------------------
def products(op, device="cpu"):
    """(sum_k a w, sum_k |a| |w|) in float64: what every epilogue's reference starts from (pass it to `reference` as `pre` to compute it once)."""
    a, w = op["a"].to(device).double(), op["w"].to(device).double()
    return a @ w.t(), a.abs() @ w.abs().t()


def reference(op, epilogue, S=1, device="cpu", pre=None):
    """(ref, tol) in float64, [M, N], of `epilogue` on the operands `op` (a dict as `operands` returns); S > 1: split-K in S slices."""
    has_bias, act = EPILOGUES[epilogue]
    d = lambda t: t.to(device).double()
    K = op["a"].shape[1]
    acc, mag = pre if pre is not None else products(op, device)
    bias = d(op["bias"]) if has_bias else torch.zeros(acc.shape[1], dtype=torch.float64, device=device)
    z = acc + bias
    A = (K + 1 + (S if S > 1 else 0)) * U24 * (bias.abs() + mag)
    e_h = A + U11 * (z.abs() + A) + U25
    if act == 0:
        return z, e_h
    if act == 6:
        ref = d(op["res"]) + z
        return ref, e_h + U11 * (ref.abs() + e_h) + U25
    if act in (2, 3, 5):
        sc, sh = d(op["scale"]), d(op["shift"])
        v = acc * sc + sh
        e_v = sc.abs() * e_h
        tol = e_v + U11 * (v.abs() + e_v) + U25
        if act == 2:
            return v, tol
        if act == 3:
            return v.clamp_min(0), tol
        r = v + d(op["res"])
        return r.clamp_min(0), tol + U11 * (r.abs() + tol) + U25
    t = 1.702 * z
    e_t = 1.702 * e_h + U24 * t.abs()
    e_t = e_t + U11 * (t.abs() + e_t) + U25
    near = torch.sigmoid((t.abs() - e_t).clamp_min(0))
    s = torch.sigmoid(t)
    e_s = near * (1 - near) * (e_t + (2 * t.abs() + 2) * U24) + 3 * U24 * s
    e_s = e_s + U11 * (s + e_s) + U25
    ref = z * s
    e_y = s * e_h + z.abs() * e_s
    return ref, e_y + U11 * (ref.abs() + e_y) + U25


def bn_act_reference(x16, scale, shift, res16=None, relu=True):
    """ops.bn_act (bn_act_kernel of csrc/pclip_resnet.hip) on an fp16 tensor: the BatchNorm chain above with an EXACT input (e_h = 0)."""
    v = x16.double() * scale.double() + shift.double()
    tol = U11 * v.abs() + U25
    if res16 is not None:
        v = v + res16.double()
        tol = tol + U11 * (v.abs() + tol) + U25
    return (v.clamp_min(0) if relu else v), tol


def _zones(ref, tol):
    must_inf, must_fin = ref.abs() - tol > F16_EDGE, ref.abs() + tol < F16_EDGE
    return must_inf, must_fin


def undecided_share(ref, tol):
    """Share of the elements for which the tolerance accepts a finite result and an infinity alike."""
    must_inf, must_fin = _zones(ref, tol)
    return float((~(must_inf | must_fin)).double().mean())


def grade(got, ref, tol):
    """worst |got - ref| / tol with the overflow rule of the docstring; infinity for a NaN, a wrong or missing infinity, an infinity where none may be."""
    got = torch.as_tensor(got).double().to(ref.device)
    must_inf, must_fin = _zones(ref, tol)
    fin = torch.isfinite(got)
    inf_ok = torch.isinf(got) & (torch.sign(got) == torch.sign(ref))
    bad = torch.isnan(got) | (must_inf & ~inf_ok) | (must_fin & ~fin) | ~(fin | inf_ok)
    if bool(bad.any()):
        return float("inf")
    err = torch.where(fin, got - ref, torch.zeros_like(ref)).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


# ---- emulation: the documented chain in fp32 on the CPU ---------------------------------------------------------------------------------------------------
def _chunks(K, c):
    return [(k, min(k + c, K)) for k in range(0, K, c)]


def accumulate(op, has_bias, order=("asc", 64), S=1, variant=None):
    """The fp32 accumulator [M, N] (a float32 tensor): K exact products added in `order`, the bias as the initial value.  S > 1: per slice from zero in
    ascending 64-chunks, slices added in order from zero, then the bias."""
    a, w = op["a"].float(), op["w"].float()
    M, K = a.shape
    N = w.shape[0]
    if variant == "drop_tail_chunk":
        assert K % 64, "the K-tail instantiation only"
        K -= 8
    bias = op["bias"].float().expand(M, N) if has_bias else torch.zeros(M, N)
    part = lambda k0, k1: a[:, k0:k1] @ w[:, k0:k1].t()
    if S > 1:
        per = splitk_slices(K)[1] * 64
        tot = torch.zeros(M, N)
        for s in range(S):
            sl = torch.zeros(M, N)
            for k0, k1 in _chunks(min(K, (s + 1) * per) - s * per, 64):
                sl = sl + part(s * per + k0, s * per + k1)
            reps = 0 if (variant == "slab_dropped" and s == S - 1) else 2 if (variant == "slab_twice" and s == 1) else 1
            for _ in range(reps):
                tot = tot + sl
        return tot + bias
    kind, c = order
    if variant in ("bias_after_round", "round_between_ktiles"):
        kind, c = "asc", 64
    if kind == "pairwise":
        leaves = [bias.clone()] + [part(k0, k1) for k0, k1 in _chunks(K, c)]
        while len(leaves) > 1:
            leaves = [leaves[i] + leaves[i + 1] if i + 1 < len(leaves) else leaves[i] for i in range(0, len(leaves), 2)]
        return leaves[0]
    late = kind == "bias_last" or variant == "bias_after_round"
    acc = torch.zeros(M, N) if late else bias.clone()
    ch = _chunks(K, c)
    for k0, k1 in (reversed(ch) if kind == "desc" else ch):
        acc = acc + part(k0, k1)
        if variant == "round_between_ktiles":
            acc = acc.half().float()
    if variant == "bias_after_round":
        return acc.half().float() + bias                          # r16(r16(acc) + bias) once the epilogue rounds it again
    return acc + bias if late else acc


def emulate(op, epilogue, order=("asc", 64), fma=True, S=1, variant=None, bn_tile=64, acc=None):
    """The kernels' result (fp16 values as float64, infinities included) by their documented chain.  fma=False: every fused operation as separate fp32
    operations.  variant: None or one of VARIANTS, the WRONG kernels:
      drop_tail_chunk         the last 8-column chunk of a K-tail is not multiplied
      bias_after_round        r16(r16(acc) + bias): the bias added behind the fp16 rounding
      round_between_ktiles    the accumulator rounded to fp16 after every K-tile
      slab_twice / _dropped   split-K: slab 1 added twice / the last slab not added
      stale_strip             BatchNorm: scale / shift of the previous column tile (`bn_tile` columns back) from the second column tile on
      residual_neighbour_row  the residual of row m + 1 (the last row: row 0)
      relu_before_residual    act 5: relu(bn) + residual, no ReLU behind the add
      gelu_nan                QuickGELU: NaN where t overflows on the negative side"""
    assert variant is None or variant in VARIANTS, variant
    has_bias, act = EPILOGUES[epilogue]
    acc = (accumulate(op, has_bias, order, S, variant) if acc is None else acc).double()       # acc: what `accumulate` returned for these arguments
    h = r16(acc)                                                     # fp32 -> fp16: one rounding
    if act == 0:
        return h
    res = op["res"].double() if act in (5, 6) else None
    if variant == "residual_neighbour_row":
        res = torch.roll(res, -1, 0)
    if act == 6:
        return r16x(res + h)                                         # the sum of two fp16 values is exact in float64
    if act in (2, 3, 5):
        sc, sh = op["scale"].double(), op["shift"].double()
        if variant == "stale_strip":
            sc, sh = torch.cat([sc[:bn_tile], sc[:-bn_tile]]), torch.cat([sh[:bn_tile], sh[:-bn_tile]])
        y = r16x(h * sc + sh) if fma else r16(r32(r32(h * sc) + sh))    # h sc has 35 significant bits: exact in float64
        if act == 2:
            return y
        if act == 3 or variant == "relu_before_residual":
            y = y.clamp_min(0)
        if act == 3:
            return y
        y = r16x(y + res)
        return y if variant == "relu_before_residual" else y.clamp_min(0)
    t = r16x(C1702 * h) if fma else r16(r32(C1702 * h))
    ex = r32(torch.exp2(r32(t * -LOG2E32)))
    s = r16(r32(1.0 / r32(1.0 + ex)))
    y = r16x(h * s)
    if variant == "gelu_nan":
        y = torch.where(torch.isinf(t) & (t < 0), torch.full_like(y, math.nan), y)
    return y


# ---- input families: fp16 operands from a seed ------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "cancel", "large", "tiny", "subnormal", "integer")


def _signs(g, *shape):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def operands(family, M, N, K, seed, epilogue="bias"):
    """dict a [M, K], w [N, K], bias [N], res [M, N] (fp16), scale, shift [N] (fp32), deterministic from the seed.
      normal     a ~ 0.5 N(0, 1), w ~ K^-0.5 N(0, 1), bias 0.1 N(0, 1), res N(0, 1): the operands of test_gpu_encoder.py::test_gemm_epilogues
      cancel     a = [x, x], w = [y, -(1 - 2^-9) y] with x, y >= 0 (times a sign per row and column): every row's products cancel to about 2^-10 of
                 sum |a| |w|, so the accumulation term A carries the tolerance
      large      a = x_m p, w = (3e4 / K) y_n p with a sign vector p, 1 <= x_m <= 1.5, 1 <= y_n <= 1.55, a sign per row, 2 % noise: results over
                 +-(3e4 .. 7e4), both sides of 65520, no cancellation (A is small and the undecided band narrow); what follows the product is small
                 (docstring, OVERFLOW).  For QuickGELU the negative rows are scaled by 0.9: pre-activations beyond -38 500, where t overflows, inside -6.4e4
      tiny       normal operands (|a| in 2^-10 .. 2^-9, |w| in 2^-7 .. 2^-6 over sqrt K), results, bias and residual in fp16's subnormal range
      subnormal  a is fp16-subnormal (|a| < 2^-14), w ~ 64 N(0, 1): results of a few hundredths
      integer    small integers everywhere: every intermediate is exact"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    if family == "normal":
        a, w = 0.5 * rn(M, K), K ** -0.5 * rn(N, K)
        bias, res, scale, shift = 0.1 * rn(N), rn(M, N), 1 + 0.3 * rn(N), 0.2 * rn(N)
    elif family == "cancel":
        h = K // 2
        x, y = rn(M, h).abs().half().float(), (K ** -0.5 * rn(N, h).abs()).half().float()
        a = torch.cat([x, x, torch.zeros(M, K - 2 * h)], 1) * _signs(g, M, 1)
        w = torch.cat([y, -(1 - 2.0 ** -9) * y, torch.zeros(N, K - 2 * h)], 1) * _signs(g, N, 1)
        s = 2.0 ** -10 * K ** 0.5
        bias, res, scale, shift = s * rn(N), s * rn(M, N), 1 + 0.3 * rn(N), s * rn(N)
    elif family == "large":
        p = _signs(g, 1, K)
        sgn = _signs(g, M, 1)
        x = (1 + 0.5 * ru(M, 1)) * torch.where(sgn < 0, 0.9 if EPILOGUES[epilogue][1] == 1 else 1.0, 1.0)
        a = sgn * x * p * (1 + 0.02 * rn(M, K))
        w = (3e4 / K) * (1 + 0.55 * ru(N, 1)) * p * (1 + 0.02 * rn(N, K))
        bias, res = torch.randint(-4, 5, (N,), generator=g).float(), torch.randint(-4, 5, (M, N), generator=g).float()
        scale, shift = 1 + torch.randint(0, 5, (N,), generator=g).float() / 64, torch.randint(-4, 5, (N,), generator=g).float()
    elif family == "tiny":
        a = _signs(g, M, K) * (0.5 + 0.5 * ru(M, K)) * 2.0 ** -9
        w = _signs(g, N, K) * (0.5 + 0.5 * ru(N, K)) * 2.0 ** -6 * K ** -0.5
        bias, res, scale, shift = 2.0 ** -17 * rn(N), 2.0 ** -16 * rn(M, N), 1 + 0.3 * rn(N), 2.0 ** -17 * rn(N)
    elif family == "subnormal":
        a = _signs(g, M, K) * torch.randint(1, 1024, (M, K), generator=g).float() * 2.0 ** -24
        w = 64 * rn(N, K)
        s = 2.0 ** -9 * K ** 0.5
        bias, res, scale, shift = s * rn(N), s * rn(M, N), 1 + 0.3 * rn(N), s * rn(N)
    elif family == "integer":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        a, w = ri(-3, 3, M, K), ri(-2, 2, N, K)
        bias, res, scale, shift = ri(-4, 4, N), ri(-8, 8, M, N), ri(1, 2, N) * _signs(g, N), ri(-4, 4, N)
    else:
        raise KeyError(family)
    return dict(a=a.half(), w=w.half(), bias=bias.half(), res=res.half(), scale=scale.float().contiguous(), shift=shift.float().contiguous())


def integer_exact(op, epilogue):
    """The exact result on the `integer` family (fp16 values; QuickGELU is not exact and has none).  Asserts that every value is an fp16 integer."""
    has_bias, act = EPILOGUES[epilogue]
    assert act != 1
    z = op["a"].double() @ op["w"].double().t() + (op["bias"].double() if has_bias else 0)
    if act == 6:
        z = z + op["res"].double()
    if act in (2, 3, 5):
        z = z * op["scale"].double() + op["shift"].double()
    if act == 5:
        z = z + op["res"].double()
    assert float(z.abs().max()) <= 2048, "beyond the integers fp16 holds exactly"
    return (z.clamp_min(0) if act in (3, 5) else z).half()


# ---- the shapes of the graded cases: (M, N, K) per kernel, taken from the tile sizes in the code (tests/test_gpu_gemm_forward.py says why) ---------------
CUS = 4                                                              # stands in for the device's CU count: slots = 4 (8 for the two-workgroup configurations)
PERSISTENT = {                                                       # cfg -> (BM, BN), plain shape, K-tail / ragged-N shape
    # THREE (256 x 32 with N % 64 == 0: six) column tiles against 4 or 8 workgroups (a workgroup steps by the grid: 4 and 8 are no multiples of 3, 8 none of 6, so its next tile is always another column
    # tile: `walks` below, asserted in the tests) and 4 (8) full row blocks + 1 row: 15 tiles on 4 workgroups, 27 on 8 — three or four tiles per workgroup
    0: ((128, 128), (1025, 384, 192), (1025, 328, 136)),
    1: ((256, 128), (1025, 384, 192), (1025, 328, 168)),
    2: ((256, 256), (1025, 768, 192), (1025, 584, 248)),
    3: ((256, 64), (1025, 192, 192), (1025, 168, 136)),
    4: ((256, 32), (2049, 192, 192), (2049, 88, 168)),             # (six column tiles: act 5 takes N % 64 == 0; 8 workgroups step by 2 of 6)
}
# act 5 takes N % 64 == 0 only (pclip_gemm_bn_res_f16): its tail shapes are ragged against the 128- and 256-column tiles, whole tiles of 64 and 32 columns
TAIL_N_ACT5 = {0: 320, 1: 320, 2: 576, 3: 192, 4: 192, "ring": 192}
PERSISTENT_KS = (64, 128, 256)                                       # 1, 2 and 4 K-tiles (K = 64: the explicit wait for the next tile's strip in linear_fast_kernel)
RING = ((300, 192, 320), (300, 168, 296))                            # 128 x 64 tiles, five K-tiles on four slots; ragged N and a 40-column K-tail
FOUR_WAVE = (1025, 768, 320)                                         # 15 tiles of 256 x 256 (three column tiles) on 4 workgroups, five K-tiles on the five-slot ring
GENERIC = ((257, 104, 128), (257, 100, 136))                         # forced on an aligned call; N % 8 != 0 with a K-tail: nothing else takes it
SPLITK = ((29, 128, 512), (200, 192, 960))                           # S = 4; S = 8 with a last slice of one K-tile
RING_KS = tuple(64 * t for t in range(1, 10)) + (72, 232, 440)       # 1 .. 9 K-tiles on the four-slot ring; K % 64 in {8, 40, 56}
FOUR_WAVE_KS = tuple(64 * t for t in range(3, 9))                    # 3 .. 8 K-tiles on the five-slot ring
ROW_SPLIT = (1300, 768, 192)                                         # under CUS = 4: a launch of full rounds and one for the remaining rows (the report says so)
BN_ACT = tuple((R, C) for C in (8, 16, 64, 2048) for R in (1, 126, 257))      # ops.bn_act: a thread takes 8 columns, 256 threads a block: no row count here fills one


def main_shapes():
    """name -> ((M, N, K), S, epilogues): the shape every (epilogue, family) is graded at, per kernel."""
    every, linear = tuple(EPILOGUES), ("plain", "bias", "gelu", "bias_gelu", "res")
    out = {}
    for cfg, (_, plain, tail) in PERSISTENT.items():
        out[f"cfg{cfg}"], out[f"cfg{cfg}_tail"] = (plain, 1, every), (tail, 1, every[:7])
        out[f"cfg{cfg}_tail_act5"] = ((tail[0], TAIL_N_ACT5[cfg], tail[2]), 1, every[7:])
    out["ring"], out["ring_tail"] = (RING[0], 1, every), (RING[1], 1, every[:7])
    out["ring_tail_act5"] = ((RING[1][0], TAIL_N_ACT5["ring"], RING[1][2]), 1, every[7:])
    out["four_wave"] = (FOUR_WAVE, 1, linear)
    out["generic"], out["generic_unaligned"] = (GENERIC[0], 1, every[:7]), (GENERIC[1], 1, every[:7])
    out["splitk4"], out["splitk8"] = (SPLITK[0], splitk_slices(SPLITK[0][2])[0], linear[:4]), (SPLITK[1], splitk_slices(SPLITK[1][2])[0], linear[:4])
    return out


def xcd_remap(bid, nwg):
    """pgemm::xcd_remap (csrc/pclip_gemm.h): the linear tile a workgroup starts at."""
    q, r, xcd, idx = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def walks(tiles_m, tiles_n, grid, rev=False, band=0):
    """Per workgroup, the (row block, column tile) pairs it computes, in its order: `decomp` of linear_fast_kernel / `origin` of linear4w_kernel — tiles start at
    xcd_remap(block, grid) and step by the grid; descending: linear id ntiles - 1 - t; band > 0: bands of `band` column tiles, row blocks fastest inside one."""
    ntiles = tiles_m * tiles_n
    out = []
    for bid in range(min(grid, ntiles)):
        walk, t = [], xcd_remap(bid, min(grid, ntiles))
        while t < ntiles:
            u = ntiles - 1 - t if rev else t
            if band <= 0 or band >= tiles_n:
                walk.append((u // tiles_n, u % tiles_n))
            else:
                bnd, r = divmod(u, tiles_m * band)
                w = min(band, tiles_n - bnd * band)
                walk.append((r // w, bnd * band + r % w))
            t += min(grid, ntiles)
        out.append(walk)
    return out


def crosses_column_tiles(walk_list, least=3):
    """Every workgroup computes at least `least` tiles and no two consecutive ones in the same column tile: the strip copied one tile ahead (bias / scale / shift),
    the next tile's operand descriptors and the carried bias fragment always belong to ANOTHER column tile than the one being computed."""
    return all(len(w) >= least and all(a[1] != b[1] for a, b in zip(w, w[1:])) for w in walk_list)
