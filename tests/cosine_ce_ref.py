"""Cross-entropy over cosine logits (pclip_cosine_ce_f16 / pclip_cosine_ce_backward_f16) in float64 torch with autograd, from the fp16 operands, and the
tolerances the kernels are graded with, derived from their documented roundings (tests/test_cosine_ce_cpu.py, tests/test_gpu_cosine_ce.py).

The function:  a' / b' = the fp16 rows, or their fp16 normalisation (contrastive_ref.l2norm_rows_ref);  cos = a' b'^T,  s = scale * cos (scale as fp32);
    labelled:   loss = mean_m (lse_t s[m, :] - s[m, y_m])
    symmetric:  loss = 1/2 (mean_m (lse_t s[m, :] - s[m, m]) + mean_t (lse_m s[:, t] - s[t, t]))
The kernel's roundings: cos is an fp32 summation of D exact products (any order), s one fp32 product; the exp tile exp(s - lse) enters the second matrix
product rounded to fp16 (unit 2^-11); weights, scale and the target term act in fp32; every sum is fp32 (the means are fp64).

    ds[m, t]  = scale D 2^-24 ||a'_m|| ||b'_t|| + 2^-24 |s|
    loss, lse:  max ds + 2^-20 (1 + max |lse|)                                   (lse is 1-Lipschitz in the max norm; the rest pays for exp / log / the sums)
    eps       = 2^-11 + expm1(2 max ds) + max(M, T) 2^-24
    dL/da'    : c scale (eps W |b'| + max(M, T) 2^-24 (W + Y) |b'|),  W = w_r softmax_rows + w_c softmax_cols,  Y = w_d [target],  c = 2
    dL/db'    : the transpose, with |a'|
    dL/dscale : c (eps sum W |cos| + sum W ds / scale + M T 2^-24 sum (W + Y) |cos|)
Chained through the normalisation x -> x / ||x|| (both sides take the fp16 rounding of x' as the identity and differentiate the exact map at the fp16 x):
J = (I - y y^T) / n is applied in fp32 by the kernel, so a bound t on dL/dx' becomes |J| t + 8 D 2^-24 |J| |dL/dx'| with |J| v = (v + |y| (|y| . v)) / n:
the first term is the bound carried through the linear map, the second the fp32 evaluation of two D-term dot products and the cancellation in g - y (y . g)."""
import numpy as np
import torch

from contrastive_ref import l2norm_rows_ref

C = 2.0
U24, U20, U11 = 2.0 ** -24, 2.0 ** -20, 2.0 ** -11


def clustered(M, T, D, seed, spread=0.35, clusters=4):
    """fp16 rows of a [M, D] and b [T, D] around min(clusters, M, T) shared unit centres (row i belongs to cluster i % k): at scale 100 the softmax of a row
    is peaked on the rows of its own cluster and every row of either side has partners there, so that no row of a gradient consists of underflow alone."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(clusters, M, T))
    cen = torch.randn(k, D, generator=g)
    cen = cen / cen.norm(dim=1, keepdim=True)
    a = cen[torch.arange(M) % k] + spread * torch.randn(M, D, generator=g) / D ** 0.5
    b = cen[torch.arange(T) % k] + spread * torch.randn(T, D, generator=g) / D ** 0.5
    return a.half(), b.half()


def cluster_labels(M, T, seed, clusters=4):
    """A label in the row's own cluster for most rows, any class for every fifth."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(clusters, M, T))
    m = torch.arange(M)
    per = (T - 1 - (m % k)) // k + 1                                   # classes of cluster m % k: m % k, m % k + k, ...
    own = (m % k) + k * (torch.rand(M, generator=g) * per).long().clamp(max=(per - 1).clamp(min=0))
    anyc = torch.randint(0, T, (M,), generator=g)
    return torch.where(m % 5 == 4, anyc, own)


def chain_normalisation(x16, g):
    """dL/dx from dL/dx' for x' = x / ||x||, float64."""
    x = x16.double()
    n = x.norm(dim=1, keepdim=True)
    y = x / n
    return (g - y * (y * g).sum(1, keepdim=True)) / n


def chain_tolerance(x16, tol, g):
    x = x16.double()
    n = x.norm(dim=1, keepdim=True)
    y = (x / n).abs()
    absj = lambda v: (v + y * (y * v).sum(1, keepdim=True)) / n
    return absj(tol) + 8 * x.shape[1] * U24 * absj(g.abs())


def loss64(ap, bp, sc, labels=None, symmetric=False):
    """The function itself on float64 tensors: (loss, per-row terms, lse_row, lse_col | None, s, cos)."""
    M = ap.shape[0]
    cos = ap @ bp.t()
    s = sc * cos
    lse_row = torch.logsumexp(s, 1)
    if symmetric:
        assert M == bp.shape[0] and labels is None
        lse_col = torch.logsumexp(s, 0)
        d = torch.diagonal(s)
        rows = 0.5 * ((lse_row - d) + (lse_col - d))
    else:
        lse_col = None
        rows = lse_row - s[torch.arange(M), labels.cpu().long()]
    return rows.mean(), rows, lse_row, lse_col, s, cos


def reference(a16, b16, scale, labels=None, symmetric=False, normalize_a=False, normalize_b=False, a_unit16=None, b_unit16=None):
    """Everything the kernels deliver, in float64, and the tolerance of each item.  a_unit16 / b_unit16: the normalised fp16 rows as `ops.l2norm_rows`
    delivers them, where a side is normalised — the kernels' a' / b' by definition; without them the CPU restatement l2norm_rows_ref stands in, which
    sums the squares in another order and so rounds a row's fp16 norm the other way about once in 10^4 rows (2^-11 on every element of that row).
    Returns a dict:
    loss, lse_row, lse_col (None if labelled), rows (per-row loss terms), da / db (wrt the operands as passed: chained where normalised), dscale,
    and tol_loss (also the bound of the lse vectors and the row terms), tol_da, tol_db, tol_dscale."""
    a16, b16 = a16.cpu(), b16.cpu()
    M, T, D = a16.shape[0], b16.shape[0], a16.shape[1]
    ap16 = (l2norm_rows_ref(a16) if a_unit16 is None else a_unit16.cpu()) if normalize_a else a16
    bp16 = (l2norm_rows_ref(b16) if b_unit16 is None else b_unit16.cpu()) if normalize_b else b16
    ap, bp = ap16.double().requires_grad_(True), bp16.double().requires_grad_(True)
    sc = torch.tensor(float(np.float32(scale)), dtype=torch.float64, requires_grad=True)
    loss, rows, lse_row, lse_col, s, cos = loss64(ap, bp, sc, labels, symmetric)
    if symmetric:
        w_r = w_c = 0.5 / M
        w_d = 1.0 / M
        tgt = torch.arange(M)
    else:
        tgt = labels.cpu().long()
        w_r, w_c, w_d = 1.0 / M, 0.0, 1.0 / M
    loss.backward()
    with torch.no_grad():
        s, cos = s.detach(), cos.detach()
        apd, bpd = ap.detach(), bp.detach()
        ds = sc * D * U24 * apd.norm(dim=1)[:, None] * bpd.norm(dim=1)[None, :] + U24 * s.abs()
        lses = lse_row if lse_col is None else torch.cat([lse_row, lse_col])
        tol_loss = ds.max() + U20 * (1 + lses.detach().abs().max())
        W = w_r * torch.softmax(s, 1) + (w_c * torch.softmax(s, 0) if symmetric else 0.0)
        Y = torch.zeros_like(s)
        Y[torch.arange(M), tgt] = w_d
        big = max(M, T)
        eps = U11 + torch.expm1(2 * ds.max()) + big * U24
        tol_da = C * sc * (eps * W @ bpd.abs() + big * U24 * (W + Y) @ bpd.abs())
        tol_db = C * sc * (eps * W.t() @ apd.abs() + big * U24 * (W + Y).t() @ apd.abs())
        tol_ds = C * (eps * (W * cos.abs()).sum() + (W * ds).sum() / sc + M * T * U24 * ((W + Y) * cos.abs()).sum())
        da, db = ap.grad, bp.grad
        if normalize_a:
            tol_da = chain_tolerance(a16, tol_da, da)
            da = chain_normalisation(a16, da)
        if normalize_b:
            tol_db = chain_tolerance(b16, tol_db, db)
            db = chain_normalisation(b16, db)
    return dict(loss=loss.detach(), lse_row=lse_row.detach(), lse_col=None if lse_col is None else lse_col.detach(), rows=rows.detach(), da=da, db=db,
                dscale=sc.grad, tol_loss=tol_loss.detach(), tol_da=tol_da.detach(), tol_db=tol_db.detach(), tol_dscale=tol_ds.detach(), s=s)


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0)."""
    got, want, tol = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double(), torch.as_tensor(tol).double()
    err = (got - want).abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.expand_as(err))
    return float(r.max())
