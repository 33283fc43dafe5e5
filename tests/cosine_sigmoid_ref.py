"""The pairwise sigmoid (SigLIP) loss over cosine logits (pclip_cosine_sigmoid_f16 / pclip_cosine_sigmoid_backward_f16) in float64 torch with autograd, from the
fp16 operands, and the tolerances the kernels are graded with, derived from their documented roundings (csrc/pclip_cosine_sigmoid.hip, ROUNDING POINTS;
tests/test_cosine_sigmoid_cpu.py, tests/test_gpu_cosine_sigmoid.py).

The function:  a' / b' = the fp16 rows, or their fp16 normalisation;  cos = a' b'^T,  x = scale cos + bias (scale, bias as fp32);
    y[m, t] = 1 iff ids_a[m] == ids_b[t] and ids_a[m] >= 0 (no ids: the diagonal),  z = 2 y - 1
    rows[m] = sum_t softplus(-z x[m, t]),  loss = sum_m rows[m] / M
The kernel's roundings: cos is an fp32 summation of D exact products, x one fma; exp(-|x|) carries a relative (|x| + 2) 2^-22, log1p of it a relative 2^-20
(the compensated form); a row is an fp32 sum T / 32 + 10 additions deep; sigma(x) enters the second matrix product rounded to fp16 as 2^14 sigma (unit 2^-11);
the target tile is exact; weight and scale act in fp32; the sums over the walked index are fp32; the scalars and the mean end in one fp64 sum.

    ds[m, t]   = scale D 2^-24 ||a'_m|| ||b'_t|| + 2^-24 |x|                                    (the error of a logit)
    term       : sigma(-z x) ds + 2^-22 (|x| + 2) sigma(-|x|) + 2^-20 term
                 (softplus(-z x) has slope sigma(-z x) in x; d log1p(e) / de = 1 / (1 + e) and e / (1 + e) = sigma(-|x|); the rest is relative)
    rows       : sum_t of that + (T / 32 + 10) 2^-24 rows        (a chain of that many fp32 additions of non-negative terms)
    loss       : mean_m of the rows' bounds + 2^-24 loss          (the fp64 sum is exact at this scale; one rounding to fp32)
    eps        = 2^-11 + expm1(2 max ds) + max(M, T) 2^-24
    dL/da'     : c scale (eps W |b'| + max(M, T) 2^-24 (W + Y) |b'|),  W = w sigma(x),  Y = w y,  w = 1 / M,  c = 2      (the cross-entropy's form)
    dL/db'     : the transpose, with |a'|
    dL/dscale  : c (eps sum W |cos| + sum W ds / scale + M T 2^-24 sum (W + Y) |cos|)
    dL/dbias   : the same with |cos| replaced by 1
Chained through the normalisation with cosine_ce_ref.chain_tolerance, as there."""
import numpy as np
import torch
import torch.nn.functional as F

from contrastive_ref import l2norm_rows_ref
from cosine_ce_ref import C, U11, U20, U24, chain_normalisation, chain_tolerance, clustered, worst_ratio  # noqa: F401  (re-exported for the tests)

U22 = 2.0 ** -22


def positives(M, T, ids_a=None, ids_b=None):
    """y [M, T] bool.  ids are compared as int64, never used as indices."""
    if ids_a is None:
        assert ids_b is None and M == T
        return torch.eye(M, dtype=torch.bool)
    ia, ib = ids_a.cpu().long(), ids_b.cpu().long()
    return (ia[:, None] == ib[None, :]) & (ia[:, None] >= 0)


def case_ids(M, T, i64):
    """The ids of the GPU tests: i % k and j % k, k = min(4, M, T), every fifth id of a set to -1; int32, or int64."""
    k = max(1, min(4, M, T))
    ia, ib = torch.arange(M) % k, torch.arange(T) % k
    ia[4::5] = -1
    return (ia, ib) if i64 else (ia.int(), ib.int())


def loss64(ap, bp, sc, bi, y, mean_over=None):
    """The function itself on float64 tensors: (loss, rows, x, cos)."""
    cos = ap @ bp.t()
    x = sc * cos + bi
    z = y.double() * 2 - 1
    rows = F.softplus(-z * x).sum(1)
    return rows.sum() / (mean_over or ap.shape[0]), rows, x, cos


def reference(a16, b16, scale, bias, ids_a=None, ids_b=None, normalize_a=False, normalize_b=False, a_unit16=None, b_unit16=None):
    """Everything the kernels deliver, in float64, and the tolerance of each item.  a_unit16 / b_unit16: the normalised fp16 rows as `ops.l2norm_rows` delivers
    them, where a side is normalised — the kernels' a' / b' by definition (cosine_ce_ref.reference says why).
    Returns a dict: loss, rows, da / db (wrt the operands as passed: chained where normalised), dscale, dbias, and tol_loss, tol_rows, tol_da, tol_db,
    tol_dscale, tol_dbias; x, cos, y for the tests that want them."""
    a16, b16 = a16.cpu(), b16.cpu()
    M, T, D = a16.shape[0], b16.shape[0], a16.shape[1]
    ap16 = (l2norm_rows_ref(a16) if a_unit16 is None else a_unit16.cpu()) if normalize_a else a16
    bp16 = (l2norm_rows_ref(b16) if b_unit16 is None else b_unit16.cpu()) if normalize_b else b16
    ap, bp = ap16.double().requires_grad_(True), bp16.double().requires_grad_(True)
    sc = torch.tensor(float(np.float32(scale)), dtype=torch.float64, requires_grad=True)
    bi = torch.tensor(float(np.float32(bias)), dtype=torch.float64, requires_grad=True)
    y = positives(M, T, ids_a, ids_b)
    loss, rows, x, cos = loss64(ap, bp, sc, bi, y)
    loss.backward()
    with torch.no_grad():
        x, cos, rows = x.detach(), cos.detach(), rows.detach()
        apd, bpd, s = ap.detach(), bp.detach(), sc.detach().abs()
        z = y.double() * 2 - 1
        ds = s * D * U24 * apd.norm(dim=1)[:, None] * bpd.norm(dim=1)[None, :] + U24 * x.abs()
        term = F.softplus(-z * x)
        tol_term = torch.sigmoid(-z * x) * ds + U22 * (x.abs() + 2) * torch.sigmoid(-x.abs()) + U20 * term
        tol_rows = tol_term.sum(1) + (T / 32 + 10) * U24 * rows
        tol_loss = tol_rows.mean() + U24 * loss.detach()
        w = 1.0 / M
        W, Y = w * torch.sigmoid(x), w * y.double()
        big = max(M, T)
        eps = U11 + torch.expm1(2 * ds.max()) + big * U24
        tol_da = C * s * (eps * W @ bpd.abs() + big * U24 * (W + Y) @ bpd.abs())
        tol_db = C * s * (eps * W.t() @ apd.abs() + big * U24 * (W + Y).t() @ apd.abs())
        tol_ds = C * (eps * (W * cos.abs()).sum() + (W * ds).sum() / s + M * T * U24 * ((W + Y) * cos.abs()).sum())
        tol_dbi = C * (eps * W.sum() + (W * ds).sum() / s + M * T * U24 * (W + Y).sum())
        da, db = ap.grad, bp.grad
        if normalize_a:
            tol_da = chain_tolerance(a16, tol_da, da)
            da = chain_normalisation(a16, da)
        if normalize_b:
            tol_db = chain_tolerance(b16, tol_db, db)
            db = chain_normalisation(b16, db)
    return dict(loss=loss.detach(), rows=rows, da=da, db=db, dscale=sc.grad, dbias=bi.grad, tol_loss=tol_loss, tol_rows=tol_rows, tol_da=tol_da, tol_db=tol_db,
                tol_dscale=tol_ds, tol_dbias=tol_dbi, x=x, cos=cos, y=y)
