"""The backward kernels of the transformer towers (pclip_attention_backward_f16 and the small kernels of csrc/pclip_tower_bwd.hip) in float64 torch,
from the fp16 operands, with the per-element tolerances they are graded with (tests/test_tower_backward_cpu.py, tests/test_gpu_attention_backward.py).
Nothing below is chosen: every bound follows from the roundings the kernels document.

Attention (csrc/pclip_attention_bwd.hip, "ROUNDING POINTS").  Units u11 = 2^-11 (an fp16 rounding), u24 = 2^-24 (an fp32 rounding), and 2^-25 for
the absolute error of an fp16 rounding in the subnormal range.  Per (sequence, head), S = q k^T / 8, P = softmax(S), dP = dO V^T:
    e_S   = 64 u24 |q| |k|^T / 8 + 2 u24 |S|                    fp32 accumulation of 64 exact products, the fp32 scaling
    eps_P = 2 expm1(2 max e_S + 4 u24 (1 + 2 max |S|)) + (L + 16) u24
                                                                  relative error of an fp32 P: the score error and the fused scale-and-subtract through
                                                                  exp (numerator and denominator), v_exp_f32, the L-term row sum and the reciprocal
    e_dP  = 64 u24 |dO| |V|^T                                     fp32 accumulation
    e_del = sum_k P (eps_P |dP| + e_dP) + 2 L u24 sum_k P |dP|    delta = sum_k P dP in fp32 (online accumulation)
    e_dS  = (u11 + eps_P + 2 u24) |dS| + P (e_dP + e_del) + 2^-25 dS = P (dP - delta) in fp32, then ONE fp16 rounding
    e_P16 = (u11 + eps_P) P + 2^-25                               P rounded to fp16 for dV
    A_dQ  = (e_dS |K| + L u24 |dS| |K|) / 8      A_dK = (e_dS^T |Q| + L u24 |dS|^T |Q|) / 8      A_dV = e_P16^T |dO| + L u24 P^T |dO|
    tol   = A + u11 (|ref| + A) + 2^-25                           the fp32 accumulator, rounded to fp16 once
QuickGELU backward: du = r16(dy g(u)), g in fp32 from ~10 operations with v_exp_f32 and an IEEE division (16 u24), the exponential's argument t log2 e
rounded twice in fp32 (relative 4 |t| u24 on exp(-t)): tol = (u11 + (16 + 4 |t|) u24) |ref| + 2^-25.
Column sums: fp32, rows of a slice added one after the other, slices by pclip_colsum_f32 (a tree over <= 128 partials): every partial sum is bounded
by sum |x|, so tol = (ceil(R / nslice) + nslice) u24 sum_r |x|.
LayerNorm backward (fp32 statistics, fp32 gamma): the wave sums are 64-lane trees after <= 32 in-lane terms (chains of <= 38 additions), every other
step a handful of fp32 operations; with E = rstd (|gy| + mean |gy| + |xh| mean |gy xh|) the fp32 evaluation of rstd (gy - a - xh b) (+ residual) is
within 64 u24 (E + |residual|), followed by one fp16 rounding: tol_dx = 64 u24 (E + |res|) + u11 (|ref| + 64 u24 (E + |res|)) + 2^-25.  dgamma / dbeta are
fp32 sums over the R rows (a workgroup's rows one after the other, four waves, <= 256 partials by pclip_colsum_f32) of terms with relative error
<= 64 u24: tol = (R + 64) u24 sum_r |term|."""
import math

import torch

U11, U24, U25 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25


def r16(x):
    """Round a float64 tensor to fp16 (RNE, subnormals kept) and back."""
    return x.to(torch.float32).to(torch.float16).to(torch.float64) if x.dtype != torch.float16 else x.double()


def clustered_qkv(B, L, H, seed, amp=5.0, spread=0.6, clusters=4):
    """fp16 qkv [B, L, 3 H 64] and dout [B, L, H 64]: per head, queries and keys sit around min(clusters, L) shared centres of norm `amp` (token i
    belongs to cluster i % k), so that a query's scores are a few units above the rest on the keys of its own cluster — a softmax that is neither flat
    nor one-hot, every row with partners — and no row of dS underflows to zeros in fp16 (cosine_ce_ref.clustered's construction).  v and dout are N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(clusters, L))
    cen = torch.randn(B, H, k, 64, generator=g)
    cen = amp * cen / cen.norm(dim=-1, keepdim=True)
    idx = torch.arange(L) % k
    q = cen[:, :, idx] + spread * torch.randn(B, H, L, 64, generator=g)
    kk = cen[:, :, idx] + spread * torch.randn(B, H, L, 64, generator=g)
    v = torch.randn(B, H, L, 64, generator=g)
    do = torch.randn(B, H, L, 64, generator=g)
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, H * 64)
    qkv = torch.cat([pack(q), pack(kk), pack(v)], dim=2).half().contiguous()
    return qkv, pack(do).half().contiguous()


def split_heads(qkv, B, L, H):
    """[B, L, 3 H 64] -> q, k, v [B, H, L, 64] float64."""
    t = qkv.double().cpu().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def merge_heads(dq, dk, dv):
    B, H, L, _ = dq.shape
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, H * 64)
    return torch.cat([pack(dq), pack(dk), pack(dv)], dim=2)


def causal_mask(L):
    return torch.ones(L, L, dtype=torch.bool).tril()


def attention64(q, k, v, causal):
    s = q @ k.transpose(-1, -2) / 8.0
    if causal:
        s = s.masked_fill(~causal_mask(q.shape[-2]), -math.inf)
    p = torch.softmax(s, dim=-1)
    return p @ v, p, s


def reference(qkv16, dout16, B, L, H, causal):
    """dqkv [B, L, 3 H 64] by float64 autograd from the fp16 operands, and its tolerance (same shape)."""
    q, k, v = (t.clone().requires_grad_(True) for t in split_heads(qkv16, B, L, H))
    do = dout16.double().cpu().view(B, L, H, 64).permute(0, 2, 1, 3)
    o, p, s = attention64(q, k, v, causal)
    (o * do).sum().backward()
    with torch.no_grad():
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        sv = torch.where(torch.isfinite(s), s, torch.zeros_like(s)).abs()
        e_s = 64 * U24 * (qd.abs() @ kd.abs().transpose(-1, -2)) / 8 + 2 * U24 * sv
        if causal:
            e_s = e_s * causal_mask(L)
        eps_p = 2 * math.expm1(2 * float(e_s.max()) + 4 * U24 * (1 + 2 * float(sv.max()))) + (L + 16) * U24
        dp = do @ vd.transpose(-1, -2)
        e_dp = 64 * U24 * (do.abs() @ vd.abs().transpose(-1, -2))
        delta = (p * dp).sum(-1, keepdim=True)
        e_del = (p * (eps_p * dp.abs() + e_dp)).sum(-1, keepdim=True) + 2 * L * U24 * (p * dp.abs()).sum(-1, keepdim=True)
        ds = p * (dp - delta)
        pos = (p > 0).double()                                          # masked pairs are exact zeros in the kernel: no rounding term there
        e_ds = (U11 + eps_p + 2 * U24) * ds.abs() + p * (e_dp + e_del) + U25 * pos
        e_p16 = (U11 + eps_p) * p + U25 * pos
        a_dq = (e_ds @ kd.abs() + L * U24 * (ds.abs() @ kd.abs())) / 8
        a_dk = (e_ds.transpose(-1, -2) @ qd.abs() + L * U24 * (ds.abs().transpose(-1, -2) @ qd.abs())) / 8
        a_dv = e_p16.transpose(-1, -2) @ do.abs() + L * U24 * (p.transpose(-1, -2) @ do.abs())
        ref = merge_heads(q.grad, k.grad, v.grad)
        a = merge_heads(a_dq, a_dk, a_dv)
        tol = a + U11 * (ref.abs() + a) + U25
    return ref, tol


def emulate(qkv16, dout16, B, L, H, causal, variant=None, want_ds=False):
    """The kernel's arithmetic with exactly its documented roundings (P and dS to fp16 as they enter their products, every output rounded once), everything
    else float64.  variant: None, or one of the WRONG kernels the bounds must reject — "no_rowsum" (dS = P dP), "no_scale" (dQ, dK without the 1/8),
    "non_causal" (the mask ignored)."""
    q, k, v = split_heads(qkv16, B, L, H)
    do = dout16.double().cpu().view(B, L, H, 64).permute(0, 2, 1, 3)
    _, p, _ = attention64(q, k, v, causal and variant != "non_causal")
    dp = do @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp if variant == "no_rowsum" else dp - delta)
    p16, ds16 = r16(p), r16(ds)
    sc = 1.0 if variant == "no_scale" else 0.125
    dq = r16(ds16 @ k * sc)
    dk = r16(ds16.transpose(-1, -2) @ q * sc)
    dv = r16(p16.transpose(-1, -2) @ do)
    out = merge_heads(dq, dk, dv)
    return (out, ds16) if want_ds else out


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a non-finite result as infinity)."""
    got, want, tol = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu(), torch.as_tensor(tol).double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol.expand_as(err)).max())


# ---- the small kernels -----------------------------------------------------------------------------------------------------------------
def quick_gelu_backward_ref(u16, dy16):
    u, dy = u16.double().cpu(), dy16.double().cpu()
    t = 1.702 * u
    s = torch.sigmoid(t)
    ref = dy * s * (1 + t * (1 - s))
    return ref, (U11 + (16 + 4 * t.abs()) * U24) * ref.abs() + U25


def colsum_ref(x16, nslice):
    x = x16.double().cpu()
    R = x.shape[0]
    return x.sum(0), (math.ceil(R / nslice) + nslice) * U24 * x.abs().sum(0)


def layernorm_backward_ref(x16, gamma32, dy16, res16=None, eps=1e-5):
    """(dx, dgamma, dbeta) and their tolerances for y = LN(x) * gamma + beta with fp16 x / dy (/ residual) and fp32 gamma."""
    x, g, dy = x16.double().cpu(), gamma32.double().cpu(), dy16.double().cpu()
    R, D = x.shape
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    gy = dy * g
    a, b = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    dx = rstd * (gy - a - xh * b)
    res = torch.zeros_like(dx) if res16 is None else res16.double().cpu()
    ref = dx + res
    e = 64 * U24 * (rstd * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True)) + res.abs())
    tol_dx = e + U11 * (ref.abs() + e) + U25
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    tol_dg, tol_db = (R + 64) * U24 * (dy * xh).abs().sum(0), (R + 64) * U24 * dy.abs().sum(0)
    return (ref, dgamma, dbeta), (tol_dx, tol_dg, tol_db)


# ---- one residual block (clip/model.py:171-190) in float64: the backward the host code runs, written out -------------------------------------
BLOCK_KEYS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
              "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


def random_block(W, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).double()
    return {"ln_1.weight": 1 + rn(W, std=0.1), "ln_1.bias": rn(W, std=0.1), "attn.in_proj_weight": rn(3 * W, W, std=W ** -0.5),
            "attn.in_proj_bias": rn(3 * W, std=0.02), "attn.out_proj.weight": rn(W, W, std=W ** -0.5), "attn.out_proj.bias": rn(W, std=0.02),
            "ln_2.weight": 1 + rn(W, std=0.1), "ln_2.bias": rn(W, std=0.1), "mlp.c_fc.weight": rn(4 * W, W, std=W ** -0.5),
            "mlp.c_fc.bias": rn(4 * W, std=0.02), "mlp.c_proj.weight": rn(W, 4 * W, std=(4 * W) ** -0.5), "mlp.c_proj.bias": rn(W, std=0.02)}


def _ln64(x, w, b, eps=1e-5):
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    return (x - mu) * rstd * w + b, (x - mu) * rstd, rstd


def _ln64_backward(xh, rstd, w, dy):
    gy = dy * w
    dx = rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def _attn64_backward(qkv, da, B, L, H, causal):
    W = H * 64
    t = qkv.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    do = da.view(B, L, H, 64).permute(0, 2, 1, 3)
    o, p, _ = attention64(q, k, v, causal)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (do * o).sum(-1, keepdim=True))                      # the issue's form: rowsum(dO o O)
    return merge_heads(ds @ k / 8, ds.transpose(-1, -2) @ q / 8, p.transpose(-1, -2) @ do).reshape(B * L, 3 * W)


def block_forward_backward64(x, P, gy, B, L, H, causal):
    """y = block(x) for x [B L, W] float64 and, for the upstream gradient gy, (dx, {name: gradient}) by the explicit formulas of autograd.TowerTailFn."""
    W = x.shape[1]
    h1, xh1, rstd1 = _ln64(x, P["ln_1.weight"], P["ln_1.bias"])
    qkv = h1 @ P["attn.in_proj_weight"].t() + P["attn.in_proj_bias"]
    t = qkv.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    a = attention64(t[0], t[1], t[2], causal)[0].permute(0, 2, 1, 3).reshape(B * L, W)
    xm = x + a @ P["attn.out_proj.weight"].t() + P["attn.out_proj.bias"]
    h2, xh2, rstd2 = _ln64(xm, P["ln_2.weight"], P["ln_2.bias"])
    u = h2 @ P["mlp.c_fc.weight"].t() + P["mlp.c_fc.bias"]
    f = u * torch.sigmoid(1.702 * u)
    y = xm + f @ P["mlp.c_proj.weight"].t() + P["mlp.c_proj.bias"]
    G = {}
    G["mlp.c_proj.weight"], G["mlp.c_proj.bias"] = gy.t() @ f, gy.sum(0)
    df = gy @ P["mlp.c_proj.weight"]
    tt = 1.702 * u
    s = torch.sigmoid(tt)
    du = df * s * (1 + tt * (1 - s))
    G["mlp.c_fc.weight"], G["mlp.c_fc.bias"] = du.t() @ h2, du.sum(0)
    dln, G["ln_2.weight"], G["ln_2.bias"] = _ln64_backward(xh2, rstd2, P["ln_2.weight"], du @ P["mlp.c_fc.weight"])
    gm = gy + dln
    G["attn.out_proj.weight"], G["attn.out_proj.bias"] = gm.t() @ a, gm.sum(0)
    dqkv = _attn64_backward(qkv, gm @ P["attn.out_proj.weight"], B, L, H, causal)
    G["attn.in_proj_weight"], G["attn.in_proj_bias"] = dqkv.t() @ h1, dqkv.sum(0)
    dln, G["ln_1.weight"], G["ln_1.bias"] = _ln64_backward(xh1, rstd1, P["ln_1.weight"], dqkv @ P["attn.in_proj_weight"])
    return y, gm + dln, G


def block_forward_torch(x, P, B, L, H, causal):
    """The same block as a plain torch restatement (F.layer_norm, F.multi_head_attention_forward, QuickGELU) for autograd to differentiate."""
    F = torch.nn.functional
    W = x.shape[1]
    h = F.layer_norm(x, (W,), P["ln_1.weight"], P["ln_1.bias"], 1e-5).view(B, L, W).transpose(0, 1)              # [L, B, W]
    mask = None
    if causal:
        mask = torch.full((L, L), -math.inf, dtype=x.dtype).triu(1)
    a = F.multi_head_attention_forward(h, h, h, W, H, P["attn.in_proj_weight"], P["attn.in_proj_bias"], None, None, False, 0.0,
                                       P["attn.out_proj.weight"], P["attn.out_proj.bias"], training=False, need_weights=False, attn_mask=mask)[0]
    xm = x + a.transpose(0, 1).reshape(B * L, W)
    h2 = F.layer_norm(xm, (W,), P["ln_2.weight"], P["ln_2.bias"], 1e-5)
    u = F.linear(h2, P["mlp.c_fc.weight"], P["mlp.c_fc.bias"])
    return xm + F.linear(u * torch.sigmoid(1.702 * u), P["mlp.c_proj.weight"], P["mlp.c_proj.bias"])
