"""References for the feature regularisers (csrc/pclip_feature_reg.hip): the float64 function, a numpy-float32 emulation of the walk the file's header
documents (every numpy float32 operation is one correctly rounded operation, as every operation of the kernel is), the per-output tolerances, and four
deliberately wrong walks.

Tolerances, by the project's rule — the number of rounded fp32 operations on a term's path, times u = 2^-24, times the sum of |terms| — to first order in u:
    A     = 8 ceil(D / 512) + 6      additions on a column's path through a LANE SUM and the wave butterfly
    e_inv = A + 2                    1 / sqrt(ss): the sum's A (halved by the root, not taken), the root, the division
    e_n   = e_inv + 1                n_d = x_d inv;  e_t = e_n under normalize_t, else 0 (f32(t_d) is exact)
    L1  rows[m]:  u sum_d ( e_n |n_d| + e_t |t'_d| + (1 + A) |n_d - t'_d| )                       (the subtraction, then the additions)
    COS rows[m]:  u ( sum_d (e_n + e_t + 1 + A) |n_d t'_d| + |rows[m]| )                          (the product, the additions, the final 1 - S)
    loss:         ( sum_m tol_rows[m] + u (B + 2) sum_m |rows[m]| ) / denom,  B = the additions on a row term's path through the BLOCK SUM stages
                  (ceil(n / 256) + 6 + 3 per stage); + 2: the division and the rounding of the quotient
    dx:  e_w = 1 (the weight is rounded once);  e_dn = e_w (L1: dn = +-weight) or e_w + e_t + 1 (COS: dn = -weight t'_d)
         err_dot = u sum_d (e_n + e_dn + 1 + A) |n_d dn_d|
         tol_dx_d = ( e_dn u |dn_d| + |n_d| err_dot + (e_n + 1) u |n_d dot| + u |dn_d - n_d dot| ) / ||x|| + (e_inv + 1) u |dx_d|
L1's sign: the computed difference has the sign of the exact one whenever |n_d - t'_d| > u (e_n |n_d| + e_t |t'_d|) (the subtraction itself never flips a
sign); an element at or below that bound is UNDECIDED — either sign, or none, is a correct result there, and `reference(..., sign=)` takes the one to grade
the row with.  `undecided` marks them."""
import itertools
import math

import numpy as np

U = 2.0 ** -24
CHUNK = 1024                     # PCLIP_FREG_CHUNK
WALKS = ("documented", "n_rounded_to_fp16", "sgn0_is_plus", "no_projection", "l1_mean_over_rows_only")


def make_case(M, D, seed, planted_equal_rows=0, cluster=0.0):
    """x, t [M, D] float16: normal rows of uneven scale; `cluster` pulls t towards x (a regulariser's working point); the first `planted_equal_rows` rows of
    t ARE x's (the difference is exactly zero there under normalize_t)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((M, D)) * np.exp(g.standard_normal((M, 1)))
    t = g.standard_normal((M, D)) * np.exp(g.standard_normal((M, 1)))
    if cluster:
        t = cluster * x + (1 - cluster) * t
    x16, t16 = x.astype(np.float16), t.astype(np.float16)
    t16[:planted_equal_rows] = x16[:planted_equal_rows]
    return x16, t16


def case_seed(M, D):
    return 11 + M + D


# the shapes the GPU test grades (tests/test_gpu_feature_reg.py explains the choice); the CPU test walks the same cases
GPU_SHAPES = [(1, 8), (1, 64), (3, 72), (33, 520), (65, 512), (1000, 512), (4, 1024), (5, 2056), (3, 4096), (1024, 8), (1025, 16), (2051, 8)]


def weight_of(M, D, mode, grad=1.0, mean_over=None):
    over = M if mean_over is None else mean_over
    return float(grad) / (over * D if mode == "l1" else over)


def _adds(D):
    return 8 * math.ceil(D / 512) + 6


def _block_adds(n):
    return math.ceil(n / 256) + 6 + 3


def reference(x16, t16, mode, normalize_t, grad=1.0, mean_over=None, sign=None):
    """float64 values and the derived tolerances: loss, rows, inv_norm, dx, tol_*, undecided [M, D] bool (L1).  sign [M, D] in {-1, 0, 1}: the sign to use at
    the undecided elements (default: float64's own)."""
    x, t = x16.astype(np.float64), t16.astype(np.float64)
    M, D = x.shape
    A = _adds(D)
    e_inv, e_n = A + 2, A + 3
    e_t = e_n if normalize_t else 0
    with np.errstate(all="ignore"):
        inv = 1.0 / np.sqrt((x * x).sum(1, keepdims=True))
        n = x * inv
        tp = t * (1.0 / np.sqrt((t * t).sum(1, keepdims=True))) if normalize_t else t          # (n's own expression: t == x gives an exact 0 here too)
        w = weight_of(M, D, mode, grad, mean_over)
        out = {"inv_norm": inv[:, 0], "tol_inv_norm": e_inv * U * np.abs(inv[:, 0])}
        if mode == "l1":
            d = n - tp
            rows = np.abs(d).sum(1)
            tol_rows = U * (e_n * np.abs(n) + e_t * np.abs(tp) + (1 + A) * np.abs(d)).sum(1)
            denom = M * D
            und = np.abs(d) <= U * (e_n * np.abs(n) + e_t * np.abs(tp))
            s = np.sign(d)
            if sign is not None:
                s = np.where(und, sign, s)
            dn, e_dn = w * s, 1
            out["undecided"] = und
        else:
            prod = n * tp
            rows = 1.0 - prod.sum(1)
            tol_rows = U * ((e_n + e_t + 1 + A) * np.abs(prod).sum(1) + np.abs(rows))
            denom = M
            dn, e_dn = -w * tp, 1 + e_t + 1
            out["undecided"] = np.zeros((M, D), dtype=bool)
        B = _block_adds(min(M, CHUNK)) + (_block_adds(math.ceil(M / CHUNK)) if M > CHUNK else 0)
        out["rows"], out["tol_rows"] = rows, tol_rows
        out["loss"] = rows.sum() / denom if M else 0.0
        out["tol_loss"] = (tol_rows.sum() + U * (B + 2) * np.abs(rows).sum()) / denom if M else 0.0
        dot = (n * dn).sum(1, keepdims=True)
        err_dot = U * ((e_n + e_dn + 1 + A) * np.abs(n * dn)).sum(1, keepdims=True)
        dx = (dn - n * dot) * inv
        out["dx"] = dx
        out["tol_dx"] = (e_dn * U * np.abs(dn) + np.abs(n) * err_dot + (e_n + 1) * U * np.abs(n * dot) + U * np.abs(dn - n * dot)) * inv + (e_inv + 1) * U * np.abs(dx)
    return out


# ---- the documented walk in numpy float32 -----------------------------------------------------------------------------------------------------------------

_LANES = np.arange(64)


def _butterfly(p):
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[..., _LANES ^ off]
    return p


def lane_sum(q):
    """S_d q_d of the header for q [M, D] float32: [M] float32."""
    M, D = q.shape
    nvec = D // 8
    per_lane = -(-nvec // 64)
    pad = np.zeros((M, per_lane * 64 * 8), dtype=np.float32)
    pad[:, :D] = q
    pad = pad.reshape(M, per_lane, 64, 8)
    acc = np.zeros((M, 64), dtype=np.float32)
    for i in range(per_lane):
        has = (_LANES + 64 * i) < nvec
        for k in range(8):
            acc = np.where(has, acc + pad[:, i, :, k], acc)
    return _butterfly(acc)[:, 0]


def block_sum(a):
    """The BLOCK SUM of the header for a [n] float32."""
    n = a.shape[0]
    steps = -(-n // 256) if n else 0
    pad = np.zeros(max(steps, 1) * 256, dtype=np.float32)
    pad[:n] = a
    pad = pad.reshape(-1, 256)
    idx = np.arange(256)
    acc = np.zeros(256, dtype=np.float32)
    for j in range(steps):
        acc = np.where(idx + 256 * j < n, acc + pad[j], acc)
    w = _butterfly(acc.reshape(4, 64))[:, 0]
    return np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])


def loss_of(rows, denom):
    M = rows.shape[0]
    if M == 0:
        return np.float32(0.0)
    if M <= CHUNK:
        R = block_sum(rows)
    else:
        R = block_sum(np.array([block_sum(rows[c:c + CHUNK]) for c in range(0, M, CHUNK)], dtype=np.float32))
    return np.float32(np.float64(R) / np.float64(denom))


def emulate(x16, t16, mode, normalize_t, grad=1.0, mean_over=None, walk="documented"):
    """loss, rows, inv_norm (float32) and dx [M, D] float32 by the header's walk, or by one of the wrong WALKS."""
    assert walk in WALKS
    M, D = x16.shape
    x, t = x16.astype(np.float32), t16.astype(np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        inv = (one / np.sqrt(lane_sum(x * x)))[:, None]
        n = x * inv
        tp = t * (one / np.sqrt(lane_sum(t * t)))[:, None] if normalize_t else t
        if walk == "n_rounded_to_fp16":
            n = n.astype(np.float16).astype(np.float32)
            tp = tp.astype(np.float16).astype(np.float32)
        l1_denom_rows_only = walk == "l1_mean_over_rows_only" and mode == "l1"
        w = np.float32(weight_of(M, 1 if l1_denom_rows_only else D, mode, grad, mean_over))
        if mode == "l1":
            d = n - tp
            rows = lane_sum(np.abs(d))
            denom = M if l1_denom_rows_only else M * D
            s = np.sign(d)
            if walk == "sgn0_is_plus":
                s = np.where(d == 0, one, s)
            dn = (w * s).astype(np.float32)
            dn = np.where(s == 0, np.float32(0.0), dn)
        else:
            rows = one - lane_sum(n * tp)
            denom = M
            dn = (-w) * tp
        dot = lane_sum(n * dn)[:, None]
        dx = dn * inv if walk == "no_projection" else (dn - n * dot) * inv
    return {"loss": loss_of(rows, denom), "rows": rows, "inv_norm": inv[:, 0], "dx": dx.astype(np.float32)}


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a non-finite result as infinity)."""
    got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got.reshape(want.shape) - want)
    with np.errstate(all="ignore"):
        return float(np.where(err == 0, 0.0, err / np.broadcast_to(tol, err.shape)).max())


def grade(got, x16, t16, mode, normalize_t, grad=1.0, mean_over=None, max_per_row=6):
    """Worst ratios of got = {loss, rows, inv_norm, dx} to the tolerances, and the share of undecided elements.  A row of dx with undecided elements is graded
    against the float64 row of whichever signs there bring it inside (each undecided element may be -1, 0 or +1): the first combination that fits, or the
    float64 signs' ratio if none does."""
    ref = reference(x16, t16, mode, normalize_t, grad, mean_over)
    r = {k: worst_ratio(got[k], ref[k], ref["tol_" + k]) for k in ("loss", "rows", "inv_norm")}
    und = ref["undecided"]
    clean = ~und.any(1)
    r["dx"] = worst_ratio(np.asarray(got["dx"])[clean], ref["dx"][clean], ref["tol_dx"][clean])
    for m in np.nonzero(~clean)[0]:
        cols = np.nonzero(und[m])[0]
        assert len(cols) <= max_per_row, f"row {m}: {len(cols)} undecided elements"
        best = float("inf")
        for combo in itertools.product((0.0, -1.0, 1.0), repeat=len(cols)):
            sign = np.zeros((1, x16.shape[1]))
            sign[0, cols] = combo
            one = reference(x16[m:m + 1], t16[m:m + 1], mode, normalize_t, grad, x16.shape[0] if mean_over is None else mean_over, sign=sign)
            best = min(best, worst_ratio(np.asarray(got["dx"])[m:m + 1], one["dx"], one["tol_dx"]))
            if best <= 1.0:
                break
        r["dx"] = max(r["dx"], best)
    r["undecided_share"] = float(und.mean()) if und.size else 0.0
    return r
