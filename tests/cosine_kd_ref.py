"""The distillation loss over cosine logits (pclip_cosine_kd_f16 / pclip_cosine_kd_backward_f16) in float64 torch with autograd, from the fp16 operands, the
tolerances the kernels are graded with, derived from their documented roundings, and an fp32 emulation of the documented walk with its wrong variants
(tests/test_cosine_kd_cpu.py, tests/test_gpu_cosine_kd.py).

The function:  a' / b' / ta' / tb' = the fp16 rows, or their fp16 normalisation;  s = scale a' b'^T,  z = tscale ta' tb'^T (scales as fp32);
    p = softmax_t z,  q = softmax_t s,  rows[m] = sum_t p (z - s) - lse_t z + lse_t s,  loss = mean_m rows[m];  the teacher is a constant.
The kernel's roundings: each cos is an fp32 summation of D (Dt) exact products, each logit one fp32 product; p = exp(z - tlse) in fp32; the signed tile
E = q - p enters the second matrix product rounded to fp16 as 2^14 E (unit 2^-11, and below fp16's normal range the absolute unit 2^-25, i.e. 2^-39 of E);
weight and scale act in fp32; every sum is fp32 (the mean and the dscale total are fp64).

    ds[m, t]  = scale D 2^-24 ||a'_m|| ||b'_t|| + 2^-24 |s|,     dz[m, t] = tscale Dt 2^-24 ||ta'_m|| ||tb'_t|| + 2^-24 |z|
    lse_row   : max ds + 2^-20 (1 + max |lse|)          tlse_row: the same with dz                           (as cosine_ce_ref: lse is 1-Lipschitz)
    rows[m]   : sum_t p (ds + dz + 2^-24 |z - s|)                                   the logits' errors and the subtraction
                + sum_t p ep |z - s|,  ep = expm1(dz + tol_tlse + 2^-24 |z - tlse|) + 2^-22           the error of p = exp(z - tlse)
                + T 2^-24 sum_t p |z - s|                                           the fp32 sums
                + tol_lse + tol_tlse + 2^-22 (|sum| + |tlse| + |lse|)               the two lse and the last two additions
    loss      : max_m of the above (a mean in fp64)
    eps       = 2^-11 + expm1(2 max(ds, dz)) + max(M, T) 2^-24                      on the E tile, whose weight is |E| <= p + q =: (M W)
    dL/da'    : c scale ((eps W + 2^-39 / M) |b'| + max(M, T) 2^-24 W |b'|),  W = (p + q) / M,  c = 2
    dL/db'    : the transpose, with |a'|
    dL/dscale : c (eps sum W |cos_s| + sum W ds / scale + M T 2^-24 sum W |cos_s|)
Chained through the normalisation by cosine_ce_ref.chain_tolerance (the kernel applies the Jacobian in fp32)."""
import numpy as np
import torch

from contrastive_ref import l2norm_rows_ref
from cosine_ce_ref import C, U11, U20, U24, chain_normalisation, chain_tolerance, clustered

U22, U39 = 2.0 ** -22, 2.0 ** -39
ESCALE = 2.0 ** 14


def teacher_like(M, T, Dt, seed, spread=0.15):
    """A plausible zero-shot teacher for `clustered(M, T, D, .)`: rows around cluster centres of its own width with the SAME cluster of every row and class
    (row i in cluster i % k) and a smaller spread — its prediction is peaked on the student's cluster, not equal to the student's."""
    return clustered(M, T, Dt, seed + 1000, spread=spread)


def with_far_class(b16, tb16, seed):
    """One more class on both sides that no sample is near (a random unit row: cos about 0 against every cluster).  At a scale of 20 its softmax entries
    are about e^-18 = 2^-26 — below fp16's subnormal unit 2^-25 as they are, a normal fp16 number as 2^14 times themselves: what the scaling of the E
    tile is for, and what a walk that rounds the tile or the target unscaled gets wrong by the whole entry."""
    g = torch.Generator().manual_seed(seed + 31)
    far = lambda D: torch.nn.functional.normalize(torch.randn(1, D, generator=g), dim=1).half()
    return torch.cat([b16, far(b16.shape[1])]), torch.cat([tb16, far(tb16.shape[1])])


def kd64(ap, bp, sc, tap, tbp, tsc):
    """The function itself on float64 tensors: (loss, per-row terms, lse_row, tlse_row, s, z, cos_s)."""
    cos = ap @ bp.t()
    s = sc * cos
    z = tsc * (tap @ tbp.t())
    lse, tlse = torch.logsumexp(s, 1), torch.logsumexp(z, 1)
    p = torch.exp(z - tlse[:, None])
    rows = (p * (z - s)).sum(1) - tlse + lse
    return rows.mean(), rows, lse, tlse, s, z, cos


def _unit(x16, on, given):
    return ((l2norm_rows_ref(x16) if given is None else given.cpu()) if on else x16)


def reference(a16, b16, scale, ta16, tb16, tscale, normalize_a=False, normalize_b=False, normalize_ta=False, normalize_tb=False, a_unit16=None, b_unit16=None,
              ta_unit16=None, tb_unit16=None):
    """Everything the kernels deliver, in float64, and the tolerance of each item.  *_unit16: the normalised fp16 rows as `ops.l2norm_rows` delivers them,
    where a side is normalised (cosine_ce_ref.reference says why).  Returns a dict: loss, rows, lse_row, tlse_row, da / db (wrt the operands as passed:
    chained where normalised), dscale, and tol_lse, tol_tlse, tol_rows [M], tol_loss, tol_da, tol_db, tol_dscale."""
    a16, b16, ta16, tb16 = a16.cpu(), b16.cpu(), ta16.cpu(), tb16.cpu()
    M, T, D, Dt = a16.shape[0], b16.shape[0], a16.shape[1], ta16.shape[1]
    ap16, bp16 = _unit(a16, normalize_a, a_unit16), _unit(b16, normalize_b, b_unit16)
    tap16, tbp16 = _unit(ta16, normalize_ta, ta_unit16), _unit(tb16, normalize_tb, tb_unit16)
    ap, bp = ap16.double().requires_grad_(True), bp16.double().requires_grad_(True)
    tap, tbp = tap16.double(), tbp16.double()
    sc = torch.tensor(float(np.float32(scale)), dtype=torch.float64, requires_grad=True)
    tsc = torch.tensor(float(np.float32(tscale)), dtype=torch.float64)
    loss, rows, lse, tlse, s, z, cos = kd64(ap, bp, sc, tap, tbp, tsc)
    loss.backward()
    with torch.no_grad():
        s, z, cos, lse, tlse, rows = s.detach(), z.detach(), cos.detach(), lse.detach(), tlse.detach(), rows.detach()
        apd, bpd = ap.detach(), bp.detach()
        scd = sc.detach()
        ds = scd * D * U24 * apd.norm(dim=1)[:, None] * bpd.norm(dim=1)[None, :] + U24 * s.abs()
        dz = tsc * Dt * U24 * tap.norm(dim=1)[:, None] * tbp.norm(dim=1)[None, :] + U24 * z.abs()
        tol_lse = ds.max() + U20 * (1 + lse.abs().max())
        tol_tlse = dz.max() + U20 * (1 + tlse.abs().max())
        p, q = torch.exp(z - tlse[:, None]), torch.exp(s - lse[:, None])
        diff = (z - s).abs()
        ep = torch.expm1(dz + tol_tlse + U24 * (z - tlse[:, None]).abs()) + U22
        tot = (p * (z - s)).sum(1)
        tol_rows = ((p * (ds + dz + U24 * diff)).sum(1) + (p * ep * diff).sum(1) + T * U24 * (p * diff).sum(1) + tol_lse + tol_tlse
                    + U22 * (tot.abs() + tlse.abs() + lse.abs()))
        tol_loss = tol_rows.max()
        W = (p + q) / M
        big = max(M, T)
        eps = U11 + torch.expm1(2 * torch.maximum(ds.max(), dz.max())) + big * U24
        tol_da = C * scd * ((eps * W + U39 / M) @ bpd.abs() + big * U24 * W @ bpd.abs())
        tol_db = C * scd * ((eps * W + U39 / M).t() @ apd.abs() + big * U24 * W.t() @ apd.abs())
        tol_ds = C * (eps * (W * cos.abs()).sum() + (W * ds).sum() / scd + M * T * U24 * (W * cos.abs()).sum())
        da, db = ap.grad, bp.grad
        if normalize_a:
            tol_da = chain_tolerance(a16, tol_da, da)
            da = chain_normalisation(a16, da)
        if normalize_b:
            tol_db = chain_tolerance(b16, tol_db, db)
            db = chain_normalisation(b16, db)
    return dict(loss=loss.detach(), rows=rows, lse_row=lse, tlse_row=tlse, da=da, db=db, dscale=sc.grad, tol_lse=tol_lse, tol_tlse=tol_tlse, tol_rows=tol_rows,
                tol_loss=tol_loss, tol_da=tol_da.detach(), tol_db=tol_db.detach(), tol_dscale=tol_ds.detach(), p=p, q=q)


WALKS = ("documented", "e_unscaled", "teacher_lse_for_student", "sign_of_p_dropped", "target_rounded_first")


def emulate(a16, b16, scale, ta16, tb16, tscale, normalize_a=False, normalize_b=False, normalize_ta=False, normalize_tb=False, walk="documented"):
    """The documented walk in fp32 torch (its order of operations up to the summation order inside a dot product): fp32 cos, fp32 logits, fp32 lse,
    p = exp(z - tlse), E = q - p rounded to fp16 as 2^14 E, the second products and the weight in fp32, the normalisation chained in fp32.
    walk: "documented", or one of the mistakes the tolerances must catch:
      e_unscaled               E rounded to fp16 as it is (entries below 2^-24 vanish, below 2^-14 lose their relative unit)
      teacher_lse_for_student  q formed as exp(s - tlse)
      sign_of_p_dropped        E = q + p
      target_rounded_first     p rounded to fp16 (unscaled) before the subtraction from a nearly equal q
    Returns a dict of fp32 tensors: loss, rows, lse_row, tlse_row, da, db, dscale."""
    f = torch.float32
    unit = lambda x16, on: (l2norm_rows_ref(x16) if on else x16).to(f)
    ap, bp, tap, tbp = unit(a16, normalize_a), unit(b16, normalize_b), unit(ta16, normalize_ta), unit(tb16, normalize_tb)
    M = ap.shape[0]
    sc, tsc = torch.tensor(scale, dtype=f), torch.tensor(tscale, dtype=f)
    cos = ap @ bp.t()
    s, z = sc * cos, tsc * (tap @ tbp.t())
    lse, tlse = torch.logsumexp(s, 1), torch.logsumexp(z, 1)
    p = torch.exp(z - tlse[:, None])
    rows = ((p * (z - s)).sum(1) - tlse) + lse
    q = torch.exp(s - (tlse if walk == "teacher_lse_for_student" else lse)[:, None])
    if walk == "target_rounded_first":
        p = p.half().to(f)
    E = q + p if walk == "sign_of_p_dropped" else q - p
    E16 = E.half().to(f) if walk == "e_unscaled" else (E * ESCALE).half().to(f) / ESCALE
    w = torch.tensor(1.0 / M, dtype=f)
    da, db = (w * sc) * (E16 @ bp), (w * sc) * (E16.t() @ ap)
    dscale = w * (E.double() * cos.double()).sum().to(f)

    def chain(x16, g):
        x = x16.to(f)
        ss = (x * x).sum(1, keepdim=True)
        return (g - (x * g).sum(1, keepdim=True) / ss * x) / ss.sqrt()
    if normalize_a:
        da = chain(a16, da)
    if normalize_b:
        db = chain(b16, db)
    return dict(loss=rows.double().mean().to(f), rows=rows, lse_row=lse, tlse_row=tlse, da=da, db=db, dscale=dscale)


def planted(M, T, D, Dt, seed):
    """Operands of the one-hot identity: a student pair from `clustered`, labels, and a teacher whose float64 prediction is one-hot on the label — unit
    Gaussian class rows tb and ta[m] = tb[y_m], so that cos_t is 1 at the label and at most about 4 / sqrt(Dt) elsewhere; at PLANTED_TSCALE every other
    class sits below e^-150 (tests/test_cosine_kd_cpu.py checks that float64 itself then returns the cross-entropy)."""
    a16, b16 = clustered(M, T, D, seed)
    g = torch.Generator().manual_seed(seed + 7)
    tb = torch.randn(T, Dt, generator=g)
    tb16 = (tb / tb.norm(dim=1, keepdim=True)).half()
    labels = torch.randint(0, T, (M,), generator=g)
    return a16, b16, tb16[labels].clone(), tb16, labels


PLANTED_TSCALE = 400.0
