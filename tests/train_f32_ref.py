"""The fp32 stages of the training step (csrc/pclip_train.hip: gemm_f32_kernel with its split-K reduction, colsum_kernel / colsum_part_kernel,
addscaled_rows_kernel, nll_grad_kernel, fuse_probs_backward_kernel, nll_mean_backward_kernel, nll_rows_kernel, softmax_ce_rows_kernel, l2norm_rows_f32_kernel,
l2norm_rows_backward_f32_kernel, cast_f16_f32_kernel; csrc/pclip_proto.hip: cast_f32_f16_kernel) in float64 torch from the exact operands the kernels receive, with
the per-element tolerances they are graded with (tests/test_train_f32_cpu.py without a GPU, tests/test_gpu_train_f32.py on one), fp32 emulations in more than one
summation order, wrong kernels the tolerances must reject (VARIANTS), the restated route conditions, the input families and the case lists.

Units: U24 = 2^-24 (one fp32 rounding, relative), TINY = 2^-126 (the absolute error of a result that underflows), rel(r1, r2, ..) = prod (1 + r) - 1.  pclip_train.hip is
compiled without fast-math: `/`, sqrtf are the correctly rounded IEEE operations (U24 each); contraction into fma may REMOVE a rounding listed below, never add one.
E_ULP = 2: the error of the device expf / logf in ulps (1 ulp <= 2 U24 relative).  ROCm ships no math-function accuracy table with its toolchain (no
document under its share/ or include/ trees states one), so the fallback of 2 ulps is used; it was fixed before any GPU run and is not fitted.

GEMM_F32   C = alpha op(A) op(B) + beta C0.  With S = sum_k |a| |b| (float64) per element:
               tol = |alpha| (K + n_slabs + 2) U24 S + U24 |want|  (+ U24 |beta C0| when beta != 0)
           A sum of K products added in ANY order has at most K roundings on every path from a leaf to the root (the fma chain of v_mfma_f32_32x32x2_f32: one per k, or two
           per pair of k if the pair's partial sum is rounded; the unsplit route has n_slabs = 1); the ordered sum of the n_slabs raw slab sums adds n_slabs - 1; alpha acc is
           one more and the second-order terms of (1 + U24)^(K + n_slabs) stay below one U24 S for K <= 8192: (K + n_slabs + 2) U24 S.  The last operation
           (v_fma_f32(beta, C0, alpha acc) or the product alone) rounds the result: U24 |want|; U24 |beta C0| covers an unfused beta C0.
COLSUM     out = (out0 +) scale sum_r x[r]:  t = scale sum, tol = |scale| (R + 8) U24 sum_r |x| + U24 |t|  (+ U24 |out0 + t| when accumulating)
           single pass: ceil(R / 4) in-wave additions, 3 across the waves, the product; two-pass: the same over a row block, then over the <= 64 partial rows: <= R + 8.
ADDSCALED  c' = fma(fl(s rs), x, c):  tol = 3 U24 (|s rs x| + |c|): the rounding of s rs, of the product where it is not fused, of the sum.
SOFTMAX    (nll_grad, fuse_probs_backward: s_x = softmax(-beta d_x) per bank.)  u_c = fl(beta (-d_c)), m = fl(beta (-d_ref)) with d_ref the row's min (beta >= 0) or max,
           t_c = fl(u_c - m):  e_arg = U24 (|beta d_c| + |beta d_ref| + |t_c|)  — the two roundings of beta d - max and the subtraction's own.
           e_c = expf(t_c): relative r_e = expm1(e_arg) + 2 E_ULP U24, plus TINY absolute;  sum s of N positive terms in any order: r_s = sum e_c r_e / s + N U24;
           a_c = e_c / s: r_a = rel(r_e, r_s, U24).   p = fl(fl(alpha a) + fl(oma b)):  e_p = alpha a rel(r_a, U24) + oma b rel(r_b, U24) + U24 (p + ..) + 2 TINY.
           nll = -logf(p_y):  tol = -log1p(-e_p / p_y) + 2 E_ULP U24 |nll| + TINY.   gy = -1 / (q_total p_y): r_g = 1 / (1 - e_p / p_y) rel(U24, U24) - 1.
           k_x = fl(fl(w_x gy) a_y): rel(r_g, U24, r_a(y), U24);  du = [c == y] fl(fl(w_x gy) a_c) - fl(a_c k_x), g = fl(-beta du):
               tol_g = |beta| (|T1| rel(r_g, U24, r_a, U24) + |T2| rel(r_k, r_a, U24)) (1 + U24) + 2 U24 |want| + TINY,   T1 = [c == y] w gy a_c, T2 = w gy a_c a_y
           (at c == y the two terms cancel as a_y -> 1: the tolerance follows |T1| + |T2|, not |want|).  alpha = 0 (oma = 0): every term is 0 and so is the tolerance:
           exact zeros.   rowsum = sum_c fl(gi + gt) over N terms in any order:  tol = sum_c (tol_gi + tol_gt) + (N + 1) U24 sum_c (|gi| + |gt| + tol_gi + tol_gt).
           fuse_probs_backward: K_x = sum_k fma(dp_k, a_k, .):  e_K = sum |dp_k| a_k r_a + (N + 1) U24 sum |dp_k| a_k;  diff = fl(dp_c - K): e_d = e_K + U24 (|diff| + e_K);
               v = w a_c diff through two products: e_v = w a_c (1 + R) e_d + |v| R, R = rel(r_a, U24, U24);  tol = |beta| e_v (1 + U24) + U24 |want| + TINY.
           argmax: the LOWEST index among equal maxima, bit for bit.  Columns with identical (d_i, d_t) entries — every column at beta = 0 — give identical bits in the kernel: the
           index returned must be the lowest of its class; it must be a maximum within p's tolerance (want_p + tol at it >= max (want_p - tol)), and pmax must be the graded p
           at that index within p's tolerance.  nll_rows reads a materialised p: argmax and pmax are exact (the first maximum of the fp32 row), nll = -logf(p_y): 2 E_ULP U24 |nll|.
SOFTMAX_CE loss[r] = logsumexp(S[r]) - S[r, r], dS = scale (softmax - I).  t_c = fl(S_c - mx): e_arg = U24 |t_c| (the operands are exact);  r_e, r_s, r_a as above with C terms;
               tol_dS = |scale| (a r_a + U24 (|a - [c == r]| + a r_a)) + U24 |want| + TINY
               tol_loss = -log1p(-r_s) + 2 E_ULP U24 |log s| + U24 |log s + mx| + U24 |loss| + TINY
L2NORM     ss = sum of D squares in any order: relative (D + 1) U24;  n = sqrtf(ss): r_n = rel((D + 1) U24 / 2, U24);  den = max(n, eps): |error| <= n r_n (max is 1-Lipschitz),
           r_den = n r_n / den;  y = x / den:  tol = |y| (1 / (1 - r_den) rel(U24) .. ) = |y| ((1 + U24) / (1 - r_den) - 1) + TINY.
           backward  t = (gy - (x / den) (dot / den)) / den,  dot = sum x gy:  e_dot = (D + 1) U24 sum |x gy|;  q = 1 / (1 - r_den);
               yg = dot / den: e_yg = (e_dot q + |dot| (q (1 + U24) - 1)) / den;  xn = x / den: r_xn = q (1 + U24) - 1;  prod = xn yg: e_p = |xn| (1 + r_xn) e_yg + |prod| rel(r_xn, U24)
               diff = gy - prod: e_d = e_p + U24 (|diff| + e_p);   t: e_t = e_d q (1 + U24) / den + |t| (q (1 + U24) - 1);   tol = e_t (+ U24 (|gx0 + t| + e_t) when accumulating) + TINY
NLL_MEAN_BACKWARD  dp[q, y_q] = fl(fl(-g / Q) / p): two divisions, tol = rel(U24, U24) |want|; exact zeros elsewhere.
CASTS      bit for bit: fp16 -> fp32 is exact, fp32 -> fp16 is round-to-nearest-even with subnormals, overflow to +-inf, NaN and +-0 (numpy's conversion is the reference).

What tests/test_train_f32_cpu.py prints (CPU, torch float32 emulations; the headroom of the bounds):
    emulation / tolerance, worst over the case lists:  gemm_f32 0.196 (k ascending), 0.196 (k descending; both at K = 1, where the bound is 5 U24 — 0.02 and below from
    K = 1024 on: the any-order bound grows with K, the error of a real sum with sqrt K);  colsum 0.218 / 0.211;  addscaled_rows 0.524;  nll_grad 0.361;
    fuse_probs_backward 0.504;  nll_rows 0.249;  nll_mean_backward 0.572;  softmax_ce_rows 0.405;  l2norm 0.248;  l2norm backward 0.579
    wrong kernels, clearest / faintest ratio over the listed cases where they differ:  last_k_dropped 3.4e6 / 3.4e2, edge_row_dropped 3.4e6 / 1.9e4, edge_col_dropped
    3.4e6 / 1.9e4, slab_missing 4.6e3 / 26, slab_twice 4.6e3 / 25, beta_per_slab 2.1e2 / 84, alpha_twice 4.9e4 / 58, last_block_dropped 2.5e4 / 3.4 (five rows of 4100
    N(0, 1) rows against an R-term bound), scale_per_partial 1.2e5 / 88, no_max_subtraction inf / 6.3e3, oma_is_alpha inf / 6.6e3, Q_for_q_total 4.4e5 / 5.4e3,
    label_off_by_one inf / 2.2e5, ties_highest inf / inf, diag_at_0 2.1e37 / 1.5e7, eps_ignored inf / 1.3e8   (inf: a non-finite result, a wrong index, or a non-zero
    where the tolerance is an exact zero)"""
import functools
from collections import namedtuple

import numpy as np
import torch

from train_bwd_ref import U24, worst_ratio                             # noqa: F401

E_ULP = 2
TINY = 2.0 ** -126
P_FLOOR = 1e-30                                                        # the softmax cases keep p[q, y_q] above this (float64)
ROW_SWEEP = 4 * 8192                                                   # rows one sweep of a row kernel's grid covers (one wave per row, four per workgroup, 8192 workgroups)
FLAT_SWEEP = 16384 * 256                                               # elements one sweep of a flat kernel's grid covers
VARIANTS = ("last_k_dropped",        # gemm: the last k left out at an odd K
            "edge_row_dropped",      # gemm: the last row of an edge tile not written
            "edge_col_dropped",      # gemm: the last column of an edge tile not written
            "slab_missing",          # gemm split-K: one slab left out of the reduction
            "slab_twice",            # gemm split-K: one slab counted twice
            "beta_per_slab",         # gemm split-K: beta C added once per slab
            "alpha_twice",           # gemm split-K: alpha applied to the slabs and again to their sum
            "last_block_dropped",    # colsum two-pass: the last row block missing
            "scale_per_partial",     # colsum two-pass: scale applied per partial row and again at the end
            "no_max_subtraction",    # softmax of nll_grad without the maximum
            "oma_is_alpha",          # nll_grad / fuse_probs_backward: alpha used for 1 - alpha
            "Q_for_q_total",         # nll_grad: the mean over Q instead of q_total
            "label_off_by_one",      # nll_grad: column y + 1 taken for the label
            "ties_highest",          # argmax ties resolved to the highest index
            "diag_at_0",             # softmax_ce_rows: the diagonal term at c == 0
            "eps_ignored")           # l2norm backward: n instead of max(n, eps)


def f32(x):
    return float(np.float32(x))


def rel(*rs):
    out = 1.0
    for r in rs:
        out = out * (1.0 + r)
    return out - 1.0


def t32(v):
    return torch.tensor(v, dtype=torch.float32)


def fma32(a, b, c):
    """fl(a b + c) of float32 tensors with ONE rounding (the product of two fp32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def draw(family, shape, g):
    """normal N(0, 1); offset N(8, 1): sums of absolute values far above the result, cancellation in differences; tiny N(0, 1) 2^-20."""
    x = torch.randn(*shape, generator=g)
    if family == "normal":
        return x
    if family == "offset":
        return x + 8.0
    if family == "tiny":
        return x * 2.0 ** -20
    raise KeyError(family)


def first_max(p):
    """The lowest index of the maximum of every row (torch.argmax returns the first of equal maxima)."""
    return torch.argmax(p, dim=1)


# ---- gemm_f32 ---------------------------------------------------------------------------------------------------------------------------------------------------------
Gemm = namedtuple("Gemm", "M N K ta tb a16 b16 alpha beta family split pad")


def _g(M, N, K, ta=False, tb=False, a16=True, b16=False, alpha=1.0, beta=0.0, family="normal", split=False, pad=0):
    return Gemm(M, N, K, ta, tb, a16, b16, alpha, beta, family, split, pad)


def gemm_route(M, N, K, ws_bytes):
    """(S, kper) of pclip_gemm_f32 for a non-null workspace of ws_bytes (0: no workspace), restated from the entry."""
    tiles = -(-N // 64) * -(-M // 64)
    if ws_bytes > 0 and tiles <= 128 and K >= 1024:
        S = min(512 // tiles, K // 256, 32)
        kper = -(--(-K // S) // 32) * 32
        S = -(-K // kper)
        if S >= 2 and ws_bytes >= S * M * N * 4:
            return S, kper
    return 1, K


_FAM3 = ("normal", "offset", "tiny")
GEMM_SMALL = [_g(M, N, K, family=_FAM3[i % 3], a16=i % 2 == 0, b16=i % 3 == 0)
              for i, (M, N, K) in enumerate([(1, 1, 1), (1, 33, 2), (33, 1, 31), (64, 65, 32), (65, 64, 33), (129, 33, 65), (33, 129, 203), (64, 64, 1), (65, 65, 31),
                                             (129, 129, 33), (1, 64, 203), (64, 1, 65)])]
GEMM_TRANS = [_g(65, 33, 203, ta=ta, tb=tb) for ta in (False, True) for tb in (False, True)]
GEMM_DTYPES = [_g(33, 65, 33, ta=ta, tb=tb, a16=a16, b16=b16, family="offset") for ta in (False, True) for tb in (False, True) for a16 in (False, True) for b16 in (False, True)]
GEMM_SCALARS = [_g(65, 64, 65, alpha=a, beta=b, family=fam) for (a, b), fam in zip([(1.0, 0.0), (-2.0, 0.0), (0.5, 1.0), (1.0, -1.0)], ("normal", "offset", "offset", "normal"))]
GEMM_PADDED = [_g(33, 65, 65, a16=False, alpha=0.5, beta=1.0, pad=3), _g(33, 65, 65, ta=True, tb=True, b16=True, pad=3)]
# split-K: (M, N, K) -> S: (1, 64, 1024) 4; (1, 64, 1025) 4, a last slab of 161; (1, 64, 1023) none; (1, 8192, 1024) 128 tiles: 4; (1, 8193, 1024) 129 tiles: none;
# (40, 50, 8192) the cap of 32; (40, 50, 8191) 29; (130, 70, 3000) 11 with beta = 1
GEMM_SPLIT = [_g(1, 64, 1024, split=True), _g(1, 64, 1025, split=True, family="offset", alpha=-2.0), _g(1, 64, 1023, split=True), _g(1, 8192, 1024, split=True, b16=True),
              _g(1, 8193, 1024, split=True, b16=True), _g(40, 50, 8192, split=True, ta=True, family="offset"), _g(40, 50, 8191, split=True, a16=False, alpha=0.5, beta=-1.0),
              _g(130, 70, 3000, split=True, ta=True, alpha=0.5, beta=1.0)]
GEMM_EXPECT_S = {(1, 64, 1024): 4, (1, 64, 1025): 4, (1, 64, 1023): 1, (1, 8192, 1024): 4, (1, 8193, 1024): 1, (40, 50, 8192): 32, (40, 50, 8191): 29, (130, 70, 3000): 11}
GEMM_CASES = GEMM_SMALL + GEMM_TRANS + GEMM_DTYPES + GEMM_SCALARS + GEMM_PADDED + GEMM_SPLIT


def gemm_slabs(case):
    """(S, kper) a case takes with the workspace the public wrapper hands over (32 M N floats); unsplit cases: (1, K)."""
    return gemm_route(case.M, case.N, case.K, 32 * case.M * case.N * 4) if case.split else (1, case.K)


@functools.lru_cache(maxsize=None)
def gemm_inputs(case):
    """(a, b, c0): a as stored ([K, M] when transposed) in its dtype, fp16 operands rounded first; c0 fp32 [M, N] (used when beta != 0)."""
    g = torch.Generator().manual_seed(100003 * case.M + 1009 * case.N + 7 * case.K + 2 * case.ta + case.tb)
    a = draw(case.family, (case.K, case.M) if case.ta else (case.M, case.K), g)
    b = draw(case.family, (case.N, case.K) if case.tb else (case.K, case.N), g)
    c0 = draw(case.family, (case.M, case.N), g)
    return (a.half() if case.a16 else a), (b.half() if case.b16 else b), c0


def gemm_ops(case, dtype=torch.float64):
    """op(A) [M, K], op(B) [K, N], C0 in `dtype`, and alpha, beta as the fp32 values the entry receives."""
    a, b, c0 = gemm_inputs(case)
    A, B = a.to(dtype), b.to(dtype)
    return (A.t() if case.ta else A), (B.t() if case.tb else B), c0.to(dtype), f32(case.alpha), f32(case.beta)


@functools.lru_cache(maxsize=None)
def gemm_reference(case, n_slabs=1):
    A, B, c0, alpha, beta = gemm_ops(case)
    want = alpha * (A @ B) + (beta * c0 if beta != 0 else 0)
    tol = abs(alpha) * (case.K + n_slabs + 2) * U24 * (A.abs() @ B.abs()) + U24 * want.abs() + (U24 * (beta * c0).abs() if beta != 0 else 0)
    return want, tol


def gemm_emulate(case, S=1, kper=None, descending=False, variant=None):
    """The fp32 arithmetic of gemm_f32_kernel (+ gemm_f32_reduce_kernel for S > 1) on the CPU: an fma chain over k per slab, the slabs added in order, alpha and beta at the
    end.  descending: k and the slabs from the top.  variant: a WRONG kernel (VARIANTS)."""
    A, B, c0, alpha, beta = gemm_ops(case, torch.float32)
    K = case.K - 1 if variant == "last_k_dropped" else case.K
    kper = K if S == 1 else kper

    def chain(k0, k1):
        acc = torch.zeros(case.M, case.N)
        for k in (range(k1 - 1, k0 - 1, -1) if descending else range(k0, k1)):
            acc = fma32(A[:, k:k + 1], B[k:k + 1, :], acc)
        return acc
    slabs = [chain(z * kper, min((z + 1) * kper, K)) for z in range(S)]
    if variant == "slab_missing":
        del slabs[1]
    if variant == "slab_twice":
        slabs.append(slabs[0])
    if variant == "alpha_twice":
        slabs = [t32(alpha) * s for s in slabs]
    acc = torch.zeros(case.M, case.N)
    for s in (reversed(slabs) if descending else slabs):
        acc = acc + s if len(slabs) > 1 else s
    t = t32(alpha) * acc
    nb = S if variant == "beta_per_slab" else 1
    out = t if beta == 0 else fma32(t32(beta * nb), c0, t)
    if variant == "edge_row_dropped":
        out[-1, :] = c0[-1, :] if beta != 0 else 0.0
    if variant == "edge_col_dropped":
        out[:, -1] = c0[:, -1] if beta != 0 else 0.0
    return out


def gemm_variant_differs(case, variant):
    S, _ = gemm_slabs(case)
    return {"last_k_dropped": case.K % 2 == 1 and not case.split, "edge_row_dropped": case.M % 64 != 0 and not case.split, "edge_col_dropped": case.N % 64 != 0 and not case.split,
            "slab_missing": S > 1, "slab_twice": S > 1, "beta_per_slab": S > 1 and case.beta != 0, "alpha_twice": S > 1 and case.alpha != 1.0}[variant]


# ---- colsum_f32 -------------------------------------------------------------------------------------------------------------------------------------------------------
Colsum = namedtuple("Colsum", "R C accumulate mean ws family")          # mean: scale = 1 / R; ws: a workspace is handed over ("short": four bytes too small)
COLSUM_CASES = [Colsum(0, 1, True, False, False, "normal"), Colsum(1, 63, False, False, False, "offset"), Colsum(3, 64, True, False, False, "tiny"),
                Colsum(4, 65, False, True, False, "normal"), Colsum(5, 130, True, True, False, "offset"), Colsum(128, 1, False, True, True, "normal"),
                Colsum(129, 63, True, True, True, "offset"), Colsum(2048, 64, False, True, True, "normal"), Colsum(2049, 65, True, False, True, "tiny"),
                Colsum(4100, 130, False, True, True, "offset"), Colsum(4100, 1, True, True, True, "normal"), Colsum(129, 130, False, True, "short", "normal"),
                Colsum(2049, 64, True, False, False, "offset")]


def colsum_route(R, C, ws_bytes):
    """Row blocks of pclip_colsum_f32 (1: the single pass) for a workspace of ws_bytes (0: none), restated from the entry."""
    rb = min(-(-R // 32), 64) if R > 128 else 1
    return rb if rb > 1 and ws_bytes > 0 and ws_bytes >= rb * C * 4 else 1


def colsum_ws_bytes(case):
    """The workspace a case offers: room for the most row blocks the entry ever asks for (64 C floats) — also at R <= 128, so that an untouched workspace proves the
    condition said no, not that a split would not have fitted —, or four bytes less than the case's own rb C floats ("short")."""
    if not case.ws:
        return 0
    rb = min(-(-case.R // 32), 64) if case.R > 128 else 1
    return rb * case.C * 4 - 4 if case.ws == "short" else 64 * case.C * 4


@functools.lru_cache(maxsize=None)
def colsum_inputs(case):
    g = torch.Generator().manual_seed(7 * case.R + case.C)
    return draw(case.family, (max(case.R, 1), case.C), g)[:case.R], draw(case.family, (case.C,), g), f32(1.0 / case.R) if case.mean else 1.0


def colsum_reference(case):
    x, out0, scale = colsum_inputs(case)
    t = scale * x.double().sum(0)
    want = out0.double() + t if case.accumulate else t
    tol = abs(scale) * (case.R + 8) * U24 * x.double().abs().sum(0) + U24 * t.abs() + (U24 * want.abs() if case.accumulate else 0)
    return want, tol


def _colsum_block(x, descending):
    """colsum_kernel's sum of the rows of x: wave w adds rows w, w + 4, .. one after the other, then ((w0 + w1) + w2) + w3."""
    parts = []
    for w in range(4):
        s = torch.zeros(x.shape[1])
        rows = list(range(w, x.shape[0], 4))
        for r in (reversed(rows) if descending else rows):
            s = s + x[r]
        parts.append(s)
    return ((parts[3] + parts[2]) + parts[1]) + parts[0] if descending else ((parts[0] + parts[1]) + parts[2]) + parts[3]


def colsum_emulate(case, rb=1, descending=False, variant=None):
    x, out0, scale = colsum_inputs(case)
    if rb > 1:
        rows_per = -(-case.R // rb)
        blocks = [x[b * rows_per:min((b + 1) * rows_per, case.R)] for b in range(rb)]
        if variant == "last_block_dropped":
            blocks = [b for b in blocks if b.shape[0]][:-1]
        part = torch.stack([_colsum_block(b, descending) for b in blocks])
        if variant == "scale_per_partial":
            part = t32(scale) * part
        total = _colsum_block(part, descending)
    else:
        total = _colsum_block(x, descending)
    t = t32(scale) * total
    return out0 + t if case.accumulate else t


# ---- addscaled_rows ---------------------------------------------------------------------------------------------------------------------------------------------------
ADDSCALED_CASES = [(1, 1, "normal"), (3, 63, "offset"), (5, 65, "tiny"), (23, 130, "normal")]          # (R, D, family); the GPU test adds 4099 x 1024


def addscaled_inputs(R, D, family, seed=0):
    g = torch.Generator().manual_seed(R * 1000 + D + seed)
    return draw(family, (R, D), g), draw(family, (R, D), g), draw("normal", (R,), g), -2.0


def addscaled_reference(c, x, rs, s):
    """(want, tol) in the operands' device."""
    t = (f32(s) * rs.double()).unsqueeze(1) * x.double()
    return c.double() + t, 3 * U24 * (t.abs() + c.double().abs())


def addscaled_emulate(c, x, rs, s):
    return (t32(s) * rs).unsqueeze(1) * x + c


# ---- the softmax kernels: nll_grad, fuse_probs_backward, nll_rows, nll_mean_backward -------------------------------------------------------------------------------
Soft = namedtuple("Soft", "Q N alpha beta q_extra family")
SOFT_CASES = [Soft(1, 1, 0.2, 12.0, 0, "dist"), Soft(1, 2, 1.0, 0.7, 3, "offset"), Soft(3, 63, 0.0, 12.0, 0, "dist"), Soft(4, 64, 0.2, 100.0, 0, "dist"),
              Soft(5, 65, 0.2, -3.0, 7, "normal"), Soft(23, 130, 0.2, 0.0, 0, "dist"), Soft(23, 1000, 0.2, 12.0, 0, "ties"), Soft(5, 130, 1.0, 100.0, 0, "offset"),
              Soft(4, 65, 0.0, 100.0, 2, "normal"), Soft(3, 64, 0.2, 12.0, 0, "tiny"), Soft(5, 63, 0.2, 0.7, 0, "ties"), Soft(23, 2, 0.2, 12.0, 0, "ties"),
              Soft(5, 1000, 0.2, 100.0, 0, "ties"), Soft(23, 65, 0.2, -3.0, 0, "ties")]
SOFT_BIG = Soft(ROW_SWEEP + 5, 5, 0.2, 12.0, 0, "dist")                 # the row loop's second iteration; rows r and r + 32 768 are different draws


def unit_rows(n, D, g):
    x = torch.randn(n, D, generator=g)
    return x / x.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def soft_inputs(case):
    """(d2i, d2t, labels, dp) fp32 / int64.  dist: squared distances of unit vectors (D = 16) in [0, 4]; ties: the same with the winning column of every row copied to two
    further columns (three equal maxima; the lowest index wins); offset / normal / tiny: `draw`.  The label of a row is drawn among the columns with p >= 1e-20."""
    Q, N = case.Q, case.N
    g = torch.Generator().manual_seed(1000 * Q + N + int(case.beta))
    if case.family in ("dist", "ties"):
        q = unit_rows(Q, 16, g)
        di, dt = ((q.unsqueeze(1) - unit_rows(N, 16, g).unsqueeze(0)) ** 2).sum(-1), ((q.unsqueeze(1) - unit_rows(N, 16, g).unsqueeze(0)) ** 2).sum(-1)
    else:
        di, dt = draw(case.family, (Q, N), g), draw(case.family, (Q, N), g)
    di, dt = di.float().contiguous(), dt.float().contiguous()
    if case.family == "ties" and N > 1:
        top = first_max(soft_probs(di, dt, case.alpha, case.beta)[0])
        for r in range(Q):
            others = [c for c in torch.randperm(N, generator=g).tolist() if c != int(top[r])][:2]
            for c in others:
                di[r, c], dt[r, c] = di[r, top[r]], dt[r, top[r]]
    p = soft_probs(di, dt, case.alpha, case.beta)[0]
    score = torch.where(p >= 1e-20, torch.rand(Q, N, generator=g, dtype=torch.float64), torch.full((Q, N), -1.0, dtype=torch.float64))
    labels = score.argmax(1)
    dp = draw("normal", (Q, N), g)
    return di, dt, labels, dp


def _soft_bank(d, beta):
    """float64 softmax(-beta d) over the rows and its relative error bound r_a (module docstring)."""
    d = d.double()
    dref = d.min(1, keepdim=True)[0] if beta >= 0 else d.max(1, keepdim=True)[0]
    t = -beta * d + beta * dref
    e_arg = U24 * ((beta * d).abs() + (beta * dref).abs() + t.abs())
    r_e = torch.expm1(e_arg) + 2 * E_ULP * U24
    e = torch.exp(t)
    s = e.sum(1, keepdim=True)
    r_s = (e * r_e).sum(1, keepdim=True) / s + d.shape[1] * U24
    return e / s, rel(r_e, r_s, U24)


def soft_probs(di, dt, alpha, beta):
    """(p, tol_p, a, r_a, b, r_b) of p = alpha softmax(-beta d_i) + (1 - alpha) softmax(-beta d_t) with the fp32 alpha, 1 - alpha and beta the entry receives."""
    al, oma, be = f32(alpha), f32(1.0 - alpha), f32(beta)
    a, r_a = _soft_bank(di, be)
    b, r_b = _soft_bank(dt, be)
    p = al * a + oma * b
    e_p = al * a * rel(r_a, U24) + oma * b * rel(r_b, U24) + 2 * TINY
    return p, e_p + U24 * (p + e_p), a, r_a, b, r_b


def nll_grad_reference(di, dt, labels, alpha, beta, q_total):
    """want / tol dicts of gi, gt, rowsum, nll and (p, tol_p) for the argmax grade, on the operands' device."""
    al, oma, be = f32(alpha), f32(1.0 - alpha), f32(beta)
    p, e_p, a, r_a, b, r_b = soft_probs(di, dt, alpha, beta)
    y = labels.long().view(-1, 1)
    py, e_py = p.gather(1, y), e_p.gather(1, y)
    assert bool((py >= P_FLOOR).all()), "a softmax case left the domain p[q, y_q] >= 1e-30"
    nll = -torch.log(py)
    tol_nll = -torch.log1p(-e_py / py) + 2 * E_ULP * U24 * nll.abs() + TINY
    gy = -1.0 / (q_total * py)
    r_g = rel(U24, U24) / (1 - e_py / py) + (1 / (1 - e_py / py) - 1)
    onehot = torch.zeros_like(p).scatter_(1, y, 1.0)
    want, tol = {}, {}
    for key, w, s, r in (("gi", al, a, r_a), ("gt", oma, b, r_b)):
        sy, r_y = s.gather(1, y), r.gather(1, y)
        r_k = rel(r_g, U24, r_y, U24)
        T1, T2 = onehot * w * gy * s, w * gy * s * sy
        want[key] = -be * (T1 - T2)
        tol[key] = abs(be) * (T1.abs() * rel(r_g, U24, r, U24) + T2.abs() * rel(r_k, r, U24)) * (1 + U24) + 2 * U24 * want[key].abs() + (TINY if w != 0 else 0)
    N = p.shape[1]
    want["rowsum"] = (want["gi"] + want["gt"]).sum(1)
    tsum = (tol["gi"] + tol["gt"]).sum(1)
    tol["rowsum"] = tsum + (N + 1) * U24 * ((want["gi"].abs() + want["gt"].abs()).sum(1) + tsum)
    want["nll"], tol["nll"] = nll.squeeze(1), tol_nll.squeeze(1)
    return want, tol, p, e_p


def tie_classes(di, dt, beta):
    """[Q, N]: the lowest column with the same (d_i, d_t) entries as column c — every column at beta = 0."""
    if beta == 0:
        return torch.zeros(di.shape, dtype=torch.long, device=di.device)
    out = torch.empty(di.shape, dtype=torch.long, device=di.device)
    for r0 in range(0, di.shape[0], 4096):
        a, b = di[r0:r0 + 4096], dt[r0:r0 + 4096]
        same = (a.unsqueeze(2) == a.unsqueeze(1)) & (b.unsqueeze(2) == b.unsqueeze(1))
        out[r0:r0 + 4096] = same.int().argmax(2)
    return out


def grade_argmax(am, pmax, p, tol_p, classes):
    """0 where every row's argmax is the lowest index of its class of bit-equal columns, a maximum within p's tolerance, and pmax the graded p there; else infinity."""
    am = am.long().view(-1, 1).to(p.device)
    if not bool(((am >= 0) & (am < p.shape[1])).all()):
        return float("inf")
    lowest = bool((classes.gather(1, am) == am).all())
    is_max = bool((p.gather(1, am) + tol_p.gather(1, am) >= (p - tol_p).max(1, keepdim=True)[0]).all())
    pm_ok = bool(((pmax.double().view(-1, 1).to(p.device) - p.gather(1, am)).abs() <= tol_p.gather(1, am)).all())
    return 0.0 if lowest and is_max and pm_ok else float("inf")


def _soft32(d, beta, variant=None):
    """The kernels' softmax of -beta d in torch float32: fl(beta (-d)), the maximum as fl(beta (-d_ref)), expf, the row sum, the division."""
    be = t32(beta)
    u = be * -d
    m = be * -(d.min(1, keepdim=True)[0] if beta >= 0 else d.max(1, keepdim=True)[0])
    e = torch.exp(u if variant == "no_max_subtraction" else u - m)
    return e / e.sum(1, keepdim=True)


def _pick(p, highest=False):
    if not highest:
        return first_max(p)
    return p.shape[1] - 1 - first_max(p.flip(1))


def nll_grad_emulate(di, dt, labels, alpha, beta, q_total, variant=None):
    al, oma, be = t32(alpha), t32(f32(1.0 - alpha)), f32(beta)
    if variant == "oma_is_alpha":
        oma = al
    if variant == "Q_for_q_total":
        q_total = di.shape[0]
    y = labels.long().view(-1, 1)
    if variant == "label_off_by_one":
        y = (y + 1) % di.shape[1]
    a, b = _soft32(di, be, variant), _soft32(dt, be, variant)
    p = al * a + oma * b
    am = _pick(p, variant == "ties_highest")
    py = p.gather(1, y)
    gy = -1.0 / (t32(float(q_total)) * py)
    onehot = torch.zeros_like(p).scatter_(1, y, 1.0)
    out = {}
    for key, w, s in (("gi", al, a), ("gt", oma, b)):
        k = (w * gy) * s.gather(1, y)
        out[key] = -t32(be) * (onehot * ((w * gy) * s) - s * k)
    out["rowsum"] = (out["gi"] + out["gt"]).sum(1)
    out["nll"] = -torch.log(py).squeeze(1)
    out["pmax"], out["argmax"] = p.gather(1, am.view(-1, 1)).squeeze(1), am
    return out


def fuse_bwd_reference(di, dt, dp, alpha, beta):
    al, oma, be = f32(alpha), f32(1.0 - alpha), f32(beta)
    _, _, a, r_a, b, r_b = soft_probs(di, dt, alpha, beta)
    g = dp.double()
    N = g.shape[1]
    want, tol = {}, {}
    for key, w, s, r in (("gi", al, a, r_a), ("gt", oma, b, r_b)):
        Kx = (g * s).sum(1, keepdim=True)
        e_K = (g.abs() * s * r).sum(1, keepdim=True) + (N + 1) * U24 * (g.abs() * s).sum(1, keepdim=True)
        diff = g - Kx
        e_d = e_K + U24 * (diff.abs() + e_K)
        R = rel(r, U24, U24)
        v = w * s * diff
        e_v = abs(w) * s * (1 + R) * e_d + v.abs() * R
        want[key] = -be * v
        tol[key] = abs(be) * e_v * (1 + U24) + U24 * want[key].abs() + (TINY if w != 0 and be != 0 else 0)
    want["rowsum"] = (want["gi"] + want["gt"]).sum(1)
    tsum = (tol["gi"] + tol["gt"]).sum(1)
    tol["rowsum"] = tsum + (N + 1) * U24 * ((want["gi"].abs() + want["gt"].abs()).sum(1) + tsum)
    return want, tol


def fuse_bwd_emulate(di, dt, dp, alpha, beta, variant=None):
    al, oma, be = t32(alpha), t32(f32(1.0 - alpha)), f32(beta)
    if variant == "oma_is_alpha":
        oma = al
    out = {}
    for key, w, d in (("gi", al, di), ("gt", oma, dt)):
        s = _soft32(d, be)
        k = (dp * s).sum(1, keepdim=True)
        out[key] = -t32(be) * (w * s * (dp - k))
    out["rowsum"] = (out["gi"] + out["gt"]).sum(1)
    return out


def soft_p32(case):
    """A materialised fp32 p [Q, N] of a case for nll_rows / nll_mean_backward (the fp32 emulation's p: duplicated columns stay bit-equal)."""
    di, dt, _, _ = soft_inputs(case)
    be = f32(case.beta)
    return t32(case.alpha) * _soft32(di, be) + t32(f32(1.0 - case.alpha)) * _soft32(dt, be)


def nll_rows_reference(p32, labels):
    """(nll, tol, pmax, argmax): pmax and argmax exact."""
    py = p32.double().gather(1, labels.long().view(-1, 1)).squeeze(1)
    nll = -torch.log(py)
    return nll, 2 * E_ULP * U24 * nll.abs() + TINY, p32.max(1)[0], first_max(p32)


def nll_rows_emulate(p32, labels, variant=None):
    am = _pick(p32, variant == "ties_highest")
    return -torch.log(p32.gather(1, labels.long().view(-1, 1)).squeeze(1)), p32.gather(1, am.view(-1, 1)).squeeze(1), am


def nll_mean_bwd_reference(p32, labels, g):
    """(want, tol): -g / (Q p[q, y_q]) at the label with two roundings, exact zeros elsewhere."""
    y = labels.long().view(-1, 1)
    want = torch.zeros(p32.shape, dtype=torch.float64, device=p32.device).scatter_(1, y, -f32(g) / p32.shape[0] / p32.double().gather(1, y))
    return want, rel(U24, U24) * want.abs()


def nll_mean_bwd_emulate(p32, labels, g):
    y = labels.long().view(-1, 1)
    return torch.zeros_like(p32).scatter_(1, y, (-t32(g) / t32(float(p32.shape[0]))) / p32.gather(1, y))


# ---- softmax_ce_rows --------------------------------------------------------------------------------------------------------------------------------------------------
CE_CASES = [(1, 1, "normal"), (1, 2, "offset"), (3, 63, "steep"), (4, 64, "normal"), (5, 65, "offset"), (23, 130, "tiny"), (23, 1000, "steep"), (5, 5, "normal"),
            (3, 1000, "normal")]          # (R, C, family), C >= R; steep: N(0, 1) x 30, most terms underflow against the maximum


def ce_inputs(R, C, family):
    g = torch.Generator().manual_seed(31 * R + C)
    return (draw("normal", (R, C), g) * 30.0 if family == "steep" else draw(family, (R, C), g)), 0.25


def ce_reference(S32, scale):
    S = S32.double()
    R, C = S.shape
    mx = S.max(1, keepdim=True)[0]
    t = S - mx
    r_e = torch.expm1(U24 * t.abs()) + 2 * E_ULP * U24
    e = torch.exp(t)
    s = e.sum(1, keepdim=True)
    r_s = (e * r_e).sum(1, keepdim=True) / s + C * U24 + C * TINY / s
    a, r_a = e / s, rel(r_e, r_s, U24)
    eye = torch.zeros_like(S)
    eye[:, :R] = torch.eye(R, dtype=torch.float64, device=S.device)
    sc = f32(scale)
    dS = sc * (a - eye)
    tol_dS = abs(sc) * (a * r_a + U24 * ((a - eye).abs() + a * r_a)) + U24 * dS.abs() + TINY
    ls = torch.log(s)
    loss = (ls + mx).squeeze(1) - S.diagonal()
    tol_loss = (-torch.log1p(-r_s) + 2 * E_ULP * U24 * ls.abs() + U24 * (ls + mx).abs()).squeeze(1) + U24 * loss.abs() + TINY
    return (loss, dS), (tol_loss, tol_dS)


def ce_emulate(S32, scale, variant=None):
    R, C = S32.shape
    mx = S32.max(1, keepdim=True)[0]
    e = torch.exp(S32 - mx)
    s = e.sum(1, keepdim=True)
    eye = torch.zeros_like(S32)
    if variant == "diag_at_0":
        eye[:, 0] = 1.0
    else:
        eye[:, :R] = torch.eye(R)
    return ((torch.log(s) + mx).squeeze(1) - S32.diagonal()), t32(scale) * (e / s - eye)


# ---- l2norm_rows_f32 and its backward ---------------------------------------------------------------------------------------------------------------------------------
# (R, D, family): R in {1, 3, 4, 5, 23} are the rows LAUNCHED.  From R = 3 on the last two rows are the edge rows (zeros; a norm of ~1e-14 sqrt(D), below eps); R = 1 has
# them as families of their own.
L2_CASES = [(1, 1, "normal"), (1, 64, "zero"), (1, 63, "subeps"), (3, 2, "offset"), (4, 63, "tiny"), (5, 64, "normal"), (23, 65, "offset"), (5, 130, "normal"), (3, 1000, "offset"),
            (23, 1000, "normal"), (4, 130, "normal"), (1, 1000, "offset")]
L2_BIG = (ROW_SWEEP + 5, 5, "normal")                                  # the row loop's second iteration
L2_EPS = 1e-12


def l2_special(R, family):
    """(index of the zero row, index of the row below eps) of a case, None where it has none."""
    if R >= 3:
        return R - 2, R - 1
    return (0 if family == "zero" else None), (0 if family == "subeps" else None)


def l2_inputs(R, D, family, seed=0):
    """(x, gy, gx0) fp32 [R, D]; the edge rows of `l2_special` inside the R rows."""
    g = torch.Generator().manual_seed(100 * R + D + seed)
    x = draw(family if family not in ("zero", "subeps") else "normal", (R, D), g)
    zero, sub = l2_special(R, family)
    if zero is not None:
        x[zero] = 0.0
    if sub is not None:
        x[sub] = 1e-14 * torch.randn(D, generator=g)
    return x, draw("normal", (R, D), g), draw("normal", (R, D), g)


def _l2_den(x, eps):
    D = x.shape[1]
    n = (x * x).sum(1, keepdim=True).sqrt()
    r_n = rel((D + 1) * U24 / 2, U24)
    den = n.clamp_min(f32(eps))
    return den, n * r_n / den


def l2_reference(x32, eps=L2_EPS):
    x = x32.double()
    den, r_den = _l2_den(x, eps)
    y = x / den
    return y, y.abs() * ((1 + U24) / (1 - r_den) - 1) + TINY


def l2_bwd_reference(x32, gy32, gx0=None, eps=L2_EPS):
    x, gy = x32.double(), gy32.double()
    D = x.shape[1]
    den, r_den = _l2_den(x, eps)
    q = 1 / (1 - r_den)
    dot = (x * gy).sum(1, keepdim=True)
    e_dot = (D + 1) * U24 * (x * gy).abs().sum(1, keepdim=True)
    yg = dot / den
    e_yg = (e_dot * q + dot.abs() * (q * (1 + U24) - 1)) / den
    xn, r_xn = x / den, q * (1 + U24) - 1
    prod = xn * yg
    e_p = xn.abs() * (1 + r_xn) * e_yg + prod.abs() * rel(r_xn, U24)
    diff = gy - prod
    e_d = e_p + U24 * (diff.abs() + e_p)
    t = diff / den
    e_t = e_d * q * (1 + U24) / den + t.abs() * (q * (1 + U24) - 1)
    if gx0 is None:
        return t, e_t + TINY
    want = gx0.double() + t
    return want, e_t + U24 * (want.abs() + e_t) + TINY


def l2_emulate(x, eps=L2_EPS):
    return x / (x * x).sum(1, keepdim=True).sqrt().clamp_min(eps)


def l2_bwd_emulate(x, gy, gx0=None, eps=L2_EPS, variant=None):
    n = (x * x).sum(1, keepdim=True).sqrt()
    if variant != "eps_ignored":
        n = n.clamp_min(eps)
    t = (gy - (x / n) * ((x * gy).sum(1, keepdim=True) / n)) / n
    return t if gx0 is None else gx0 + t


# ---- casts ------------------------------------------------------------------------------------------------------------------------------------------------------------
def cast_f32_specials():
    """fp32 values around every edge of the conversion to fp16: +-0, fp16 subnormals and the ties between them, the smallest normal, ties to even in the normal range, the
    largest finite value, the overflow threshold 65520, infinities, NaN, fp32 subnormals."""
    v = [0.0, -0.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
         2.0 ** -14 * (1 - 2.0 ** -12), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 - 2.0 ** -12, 65504.0, 65519.0, 65519.996, 65520.0, -65520.0, 65536.0,
         1e38, -1e38, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1e-40, 0.1, -0.1, 1 / 3]
    return torch.tensor(v, dtype=torch.float32)


def cast_f32_input(n, seed=0):
    """n fp32 values: the specials, then random BIT PATTERNS (every exponent, NaNs and infinities included) and N(0, 1) draws."""
    g = torch.Generator().manual_seed(seed + n)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.where(torch.rand(n, generator=g) < 0.5, bits, torch.randn(n, generator=g) * 100)
    sp = cast_f32_specials()[:n]
    x[:sp.numel()] = sp
    return x


def half_bits_equal(got16, x32):
    """got16 == RNE(x32) bit for bit (numpy's conversion is the reference); NaN compares as NaN (any payload, any sign)."""
    with np.errstate(over="ignore"):
        want = torch.from_numpy(x32.cpu().numpy().astype(np.float16))
    got = got16.cpu()
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
