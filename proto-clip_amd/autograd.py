"""torch.autograd.Function wrappers that make the reference's OWN training loop run on the HIP kernels with only the import swap
(reference main.py:260-310, main.qt.py:198-250):

    zs_imgs = visual_embeddings.weight.view(-1, K, ndim); ... z_img_proto = ...            # the caller's eager tensors
    zq_imgs = adapter(zq_imgs).float()                                                      # Adapter / Adapter_FC  -> here
    p = P(zq_imgs, z_img_proto, z_text_proto, alpha, beta)                                  # utils.P               -> here
    ... = compute_loss_and_matches(p, zq_labels, z_img_proto, z_text_proto, cfg)            # NLL / InfoNCE         -> here
    optimizer.zero_grad(); train_loss.backward(retain_graph=True); optimizer.step()         # torch autograd + torch.optim.AdamW

Every forward is the inference kernel of that stage, every backward the explicit backward kernel `train.ProtoClipTrainer` uses
(csrc/pclip_train.hip, pclip_adapter.hip) — the trainer stays the fast path (no tape, fused NLL + P, one flat all-reduce); this
module is the drop-in contract of SURVEY 8(b): "nn.Module semantics".  Gradients are returned in the dtype of the input they
belong to (fp16 parameters get fp16 gradients, as autograd on the reference's fp16 modules delivers them).

Not differentiated: the INPUT of the conv adapter (the reference feeds it constants: rows of the frozen key bank, main.py:265-266,
or encode_image outputs under no_grad, main.qt.py:199-201) — asking for it raises."""
import numpy as np
import torch

from . import ops
from ._lib import PclipError
from .tower import _block_params, residual_block, vit_stem

INFO_NCE_TEMPERATURE = 0.1      # info-nce-pytorch default


def _like(g32: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """fp32 gradient -> dtype / shape of the tensor it belongs to."""
    if g32 is None:
        return None
    g = g32.reshape(ref.shape)
    return ops.cast_f16(g.contiguous()) if ref.dtype == torch.float16 else g


class AdapterConvFn(torch.autograd.Function):
    """Adapter.forward (model.py:49-78); backward = pclip_adapter_conv_backward_f16 (forward recomputed in LDS)."""

    @staticmethod
    def forward(ctx, x, three_x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b):
        ctx.three_x = bool(three_x)
        ctx.save_for_backward(x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b)
        return ops.adapter_conv(x, three_x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b)

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the conv adapter's INPUT gradient is not on the Proto-CLIP path (its input rows are constants, "
                                      "main.py:265-266 / main.qt.py:199-201); detach the features")
        x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b = ctx.saved_tensors
        gr = ops.adapter_conv_backward(x, g.contiguous(), ctx.three_x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b)
        f = lambda name, ref: _like(gr.get(name), ref)
        # conv-2x never touches conv2 / bn2: their gradient stays None, as in the reference
        return (None, None, f("conv1.weight", conv1), f("bn1.weight", ln1w), f("bn1.bias", ln1b), f("conv2.weight", conv2),
                f("bn2.weight", ln2w), f("bn2.bias", ln2b), f("conv3.weight", conv3), f("bn3.weight", ln3w), f("bn3.bias", ln3b))


class AdapterFcFn(torch.autograd.Function):
    """Adapter_FC.forward (model.py:81-95) stage by stage (the saved activations are exactly the tensors the output was formed
    from) and its backward: two LayerNorm backwards + fp32 MFMA GEMMs for the weight / activation gradients."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2):
        with ops.low_latency(False):
            h1 = ops.gemm(x, w1)
            a1 = ops.layernorm(h1, g1.float(), b1.float())
            h2 = ops.gemm(a1, w2)
        out = ops.layernorm_blend(h2, g2, b2, x, ratio=0.2)
        ctx.save_for_backward(x, h1, a1, h2, w1, g1, w2, g2)
        return out

    @staticmethod
    def backward(ctx, g):
        x, h1, a1, h2, w1, g1, w2, g2 = ctx.saved_tensors
        g = g.contiguous()
        dh2, dg2, db2 = ops.layernorm_backward(h2, g2, g, dy_scale=0.2)             # ratio * LN(h2) (model.py:93-94)
        dw2 = ops.gemm_f32(dh2, a1, trans_a=True)
        da1 = ops.cast_f16(ops.gemm_f32(dh2, w2))
        dh1, dg1, db1 = ops.layernorm_backward(h1, g1, da1)
        dw1 = ops.gemm_f32(dh1, x, trans_a=True)
        dx = None
        if ctx.needs_input_grad[0]:                                                 # 0.8 * g through the blend + the first Linear
            dx32 = ops.gemm_f32(dh1, w1)
            dx32 = dx32 + 0.8 * g.float()
            dx = _like(dx32, x)
        return dx, _like(dw1, w1), _like(dg1, g1), _like(db1, g1), _like(dw2, w2), _like(dg2, g2), _like(db2, g2)


class TipLogitsFn(torch.autograd.Function):
    """Tip-Adapter-F's logits `100. * features @ clip_weights + alpha * exp(-(beta - beta * features @ keys^T)) @ cache_values` as fp32 [Q, N] (nothing rounded to
    fp16, unlike the inference call), differentiable in the KEY ROWS [NK, D] only — upstream trains nothing else.  backward = pclip_tip_keys_backward_f16, which
    recomputes the exponentials: only the operands are saved."""

    @staticmethod
    def forward(ctx, key_rows, features, seg, clip_rows, alpha, beta):
        ctx.alpha, ctx.beta = float(alpha), float(beta)
        ctx.save_for_backward(key_rows, features, seg)
        return ops.tip_logits(features, key_rows, seg, clip_rows, alpha, beta, want_logits=False, want_f32=True, layout="nd")[1]

    @staticmethod
    def backward(ctx, g):
        key_rows, features, seg = ctx.saved_tensors
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            raise NotImplementedError("TipLogitsFn: only the cache keys get a gradient (features and clip_weights are constants of Tip-Adapter-F)")
        dk = ops.tip_keys_backward(features, key_rows, seg, g.float().contiguous(), ctx.alpha, ctx.beta, layout="nd")
        return _like(dk, key_rows), None, None, None, None, None


class PFn(torch.autograd.Function):
    """utils.P (utils.py:225-244) on fp32 operands: exact-fp32 MFMA distances + softmax fusion; backward through both softmaxes
    (pclip_fuse_probs_backward) and cdist(...)**2:  dq = sum_c 2 G[q,c] (q - z_c),  dz_c = sum_q 2 G[q,c] (z_c - q)."""

    @staticmethod
    def forward(ctx, zq, zi, zt, alpha, beta):
        q32, i32, t32 = (t.float().contiguous() for t in (zq, zi, zt))
        d2i, d2t, _ = ops.sqdist_f32(q32, i32, t32)
        N = i32.shape[0]
        p, _, _, _ = ops.fuse_probs(d2i, d2t, N, alpha, beta, want_p=True)
        ctx.alpha, ctx.beta, ctx.N = float(alpha), float(beta), N
        ctx.dtypes = (zq.dtype, zi.dtype, zt.dtype)
        ctx.save_for_backward(q32, i32, t32, d2i, d2t)
        return p

    @staticmethod
    def backward(ctx, dp):
        q32, i32, t32, d2i, d2t = ctx.saved_tensors
        N = ctx.N
        gi, gt, rs = ops.fuse_probs_backward(d2i, d2t, dp.float().contiguous(), N, ctx.alpha, ctx.beta)
        gi_v, gt_v = gi[:, :N], gt[:, :N]
        gq = gimg = gtxt = None
        if ctx.needs_input_grad[0]:
            gq = ops.gemm_f32(gi_v, i32, alpha=-2.0)
            ops.gemm_f32(gt_v, t32, alpha=-2.0, out=gq, beta=1.0)
            ops.addscaled_rows_(gq, q32, rs, 2.0)
        if ctx.needs_input_grad[1]:
            gimg = ops.gemm_f32(gi_v, q32, trans_a=True, alpha=-2.0)
            ops.addscaled_rows_(gimg, i32, ops.colsum_f32(gi, cols=N), 2.0)
        if ctx.needs_input_grad[2]:
            gtxt = ops.gemm_f32(gt_v, q32, trans_a=True, alpha=-2.0)
            ops.addscaled_rows_(gtxt, t32, ops.colsum_f32(gt, cols=N), 2.0)
        cast = lambda g, dt: None if g is None else (ops.cast_f16(g) if dt == torch.float16 else g)
        return cast(gq, ctx.dtypes[0]), cast(gimg, ctx.dtypes[1]), cast(gtxt, ctx.dtypes[2]), None, None


class NllMeanFn(torch.autograd.Function):
    """nn.NLLLoss()(torch.log(p), target) (utils.py:90-93): mean over the rows of -log p[q, y_q]."""

    @staticmethod
    def forward(ctx, p, target):
        if p.dtype != torch.float32 or not p.is_contiguous():
            p = p.float().contiguous()
        nll, _, _ = ops.nll_rows(p, target)
        ctx.save_for_backward(p, target)
        return ops.colsum_f32(nll.view(-1, 1), scale=1.0 / p.shape[0])[0]

    @staticmethod
    def backward(ctx, g):
        p, target = ctx.saved_tensors
        return ops.nll_mean_backward(p, target, g), None


class InfoNceFn(torch.autograd.Function):
    """InfoNCE()(A, B) of utils.py:72-77 (info-nce-pytorch defaults: temperature 0.1, both sides normalised, cross entropy against
    the diagonal, mean) with its gradient wrt both operands."""

    @staticmethod
    def forward(ctx, A, B):
        a, b = A.float().contiguous(), B.float().contiguous()
        an, bn = ops.l2norm_rows_f32(a), ops.l2norm_rows_f32(b)
        n = a.shape[0]
        S = ops.gemm_f32(an, bn, trans_b=True, alpha=1.0 / INFO_NCE_TEMPERATURE)
        rows, dS = ops.softmax_ce_rows(S, 1.0 / n)
        ctx.save_for_backward(a, b, an, bn, dS)
        ctx.dtypes = (A.dtype, B.dtype)
        return ops.colsum_f32(rows.view(n, 1), scale=1.0 / n)[0]

    @staticmethod
    def backward(ctx, g):
        a, b, an, bn, dS = ctx.saved_tensors
        scale = 1.0 / INFO_NCE_TEMPERATURE
        ga = gb = None
        if ctx.needs_input_grad[0]:
            dan = ops.gemm_f32(dS, bn, alpha=scale)
            ga = ops.l2norm_rows_backward_f32_(torch.empty_like(a), a, dan, accumulate=False) * g
        if ctx.needs_input_grad[1]:
            dbn = ops.gemm_f32(dS, an, trans_a=True, alpha=scale)
            gb = ops.l2norm_rows_backward_f32_(torch.empty_like(b), b, dbn, accumulate=False) * g
        cast = lambda t, dt: None if t is None else (ops.cast_f16(t.contiguous()) if dt == torch.float16 else t)
        return cast(ga, ctx.dtypes[0]), cast(gb, ctx.dtypes[1])


class CosineCeFn(torch.autograd.Function):
    """Cross-entropy over the cosine logits scale * a' @ b'^T (ops.cosine_cross_entropy): labelled, or CLIP's symmetric loss.  Saves the operands and the
    lse vectors — nothing of size M T; the backward recomputes logit tiles (pclip_cosine_ce_backward_f16).  a, b: fp16, or fp32 (cast once; the gradient
    comes back fp32).  scale: a Python float, or a 0-dim tensor that then receives a gradient (its VALUE is read on the host: one sync, and no graph capture)."""

    @staticmethod
    def forward(ctx, a, b, scale, labels, symmetric, normalize_a, normalize_b):
        a16 = a if a.dtype == torch.float16 else ops.cast_f16(a.float().contiguous())
        b16 = b if b.dtype == torch.float16 else ops.cast_f16(b.float().contiguous())
        ctx.scale = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
        ctx.mode = (bool(symmetric), bool(normalize_a), bool(normalize_b))
        ctx.refs = tuple((t.dtype, t.shape) if isinstance(t, torch.Tensor) else None for t in (a, b, scale))      # what each gradient is cast back to
        loss, lse_row, lse_col = ops.cosine_cross_entropy(a16, b16, ctx.scale, labels, *ctx.mode)
        ctx.save_for_backward(a16, b16, lse_row, lse_col, labels)
        return loss

    @staticmethod
    def backward(ctx, g):
        a16, b16, lse_row, lse_col, labels = ctx.saved_tensors
        symmetric, na, nb = ctx.mode
        need_a, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ga, gb, gs = ops.cosine_cross_entropy_backward(a16, b16, ctx.scale, lse_row, lse_col, labels, symmetric, na, nb,
                                                       want_a=need_a, want_b=need_b, want_scale=need_s)
        g = g.float()

        def cast(t, ref):
            if t is None:
                return None
            t = (t * g).reshape(ref[1])
            return ops.cast_f16(t.contiguous()) if ref[0] == torch.float16 else t.to(ref[0])
        return (cast(ga, ctx.refs[0]) if need_a else None, cast(gb, ctx.refs[1]) if need_b else None, cast(gs, ctx.refs[2]) if need_s else None,
                None, None, None, None)


def cosine_cross_entropy(a, b, scale, labels=None, symmetric=False, normalize_a=False, normalize_b=False):
    """The loss of `CosineCeFn` with a tape where one is wanted, the bare forward under torch.no_grad() or for constants."""
    if wants_grad(a, b, scale if isinstance(scale, torch.Tensor) else None):
        return CosineCeFn.apply(a, b, scale, labels, symmetric, normalize_a, normalize_b)
    a16 = a if a.dtype == torch.float16 else ops.cast_f16(a.detach().float().contiguous())
    b16 = b if b.dtype == torch.float16 else ops.cast_f16(b.detach().float().contiguous())
    s = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
    return ops.cosine_cross_entropy(a16.detach(), b16.detach(), s, labels, symmetric, normalize_a, normalize_b)[0]


def _f16_operand(t):
    return t if t.dtype == torch.float16 else ops.cast_f16(t.float().contiguous())


class CosineKdFn(torch.autograd.Function):
    """Distillation loss over cosine logits (ops.cosine_kd): mean_m KL(softmax(tscale ta' @ tb'^T / tau) || softmax(scale a' @ b'^T / tau)) tau^2.  Saves the
    operands and the two lse vectors — nothing of size M T; the backward recomputes both logit tiles (pclip_cosine_kd_backward_f16).  a, b: fp16, or fp32
    (cast once; the gradient comes back fp32).  scale: a Python float, or a 0-dim tensor that then receives a gradient (its VALUE is read on the host).  The
    teacher (ta, tb fp16 constants, tscale a number or a constant 0-dim tensor) receives no gradient: `cosine_kd` refuses one that asks for it."""

    @staticmethod
    def forward(ctx, a, b, scale, ta, tb, tscale, temperature, normalize_a, normalize_b, normalize_ta, normalize_tb):
        a16, b16 = _f16_operand(a), _f16_operand(b)
        ta16 = a16 if ta is a else _f16_operand(ta)
        tb16 = b16 if tb is b else _f16_operand(tb)
        tau = float(temperature)
        ctx.scale = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
        ctx.tscale = float(tscale.detach()) if isinstance(tscale, torch.Tensor) else float(tscale)
        ctx.tau = tau
        ctx.mode = (bool(normalize_a), bool(normalize_b), bool(normalize_ta), bool(normalize_tb))
        ctx.refs = tuple((t.dtype, t.shape) if isinstance(t, torch.Tensor) else None for t in (a, b, scale))      # what each gradient is cast back to
        loss, lse_row, tlse_row = ops.cosine_kd(a16, b16, ctx.scale / tau, ta16, tb16, ctx.tscale / tau, *ctx.mode)
        ctx.same = (ta16 is a16, tb16 is b16)
        ctx.save_for_backward(a16, b16, None if ctx.same[0] else ta16, None if ctx.same[1] else tb16, lse_row, tlse_row)
        return loss * (tau * tau) if tau != 1.0 else loss

    @staticmethod
    def backward(ctx, g):
        a16, b16, ta16, tb16, lse_row, tlse_row = ctx.saved_tensors
        ta16 = a16 if ctx.same[0] else ta16
        tb16 = b16 if ctx.same[1] else tb16
        need_a, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        tau = ctx.tau
        ga, gb, gs = ops.cosine_kd_backward(a16, b16, ctx.scale / tau, ta16, tb16, ctx.tscale / tau, lse_row, tlse_row, *ctx.mode, want_a=need_a, want_b=need_b,
                                            want_scale=need_s, grad=tau * tau)
        g = g.float()

        def cast(t, ref, mul=1.0):
            if t is None:
                return None
            t = (t * g if mul == 1.0 else t * (g * mul)).reshape(ref[1])
            return ops.cast_f16(t.contiguous()) if ref[0] == torch.float16 else t.to(ref[0])
        # d/dscale of a function of scale / tau: the kernel's dscale is taken with respect to its own scale argument
        return (cast(ga, ctx.refs[0]) if need_a else None, cast(gb, ctx.refs[1]) if need_b else None, cast(gs, ctx.refs[2], 1.0 / tau) if need_s else None,
                None, None, None, None, None, None, None, None)


def cosine_kd(a, b, scale, teacher_a, teacher_b, teacher_scale, temperature=1.0, normalize_a=False, normalize_b=False, normalize_teacher_a=False,
              normalize_teacher_b=False):
    """The loss of `CosineKdFn` with a tape where one is wanted, the bare forward under torch.no_grad() or for constants.  temperature: both sets of logits
    are divided by it and the loss multiplied by its square (Hinton's convention: the gradient keeps its size).  A teacher that requires grad is refused."""
    for name, t in (("teacher_a", teacher_a), ("teacher_b", teacher_b), ("teacher_scale", teacher_scale)):
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise PclipError(f"cosine_kd: {name} requires grad, but the teacher receives no gradient (pass {name}.detach() to say so)")
    tau = float(temperature)
    if not (tau > 0.0 and np.isfinite(tau)):
        raise PclipError(f"cosine_kd: temperature={temperature} must be positive and finite")
    if wants_grad(a, b, scale if isinstance(scale, torch.Tensor) else None):
        return CosineKdFn.apply(a, b, scale, teacher_a, teacher_b, teacher_scale, tau, normalize_a, normalize_b, normalize_teacher_a, normalize_teacher_b)
    a16, b16 = _f16_operand(a.detach()), _f16_operand(b.detach())
    ta16 = a16 if teacher_a is a else _f16_operand(teacher_a)
    tb16 = b16 if teacher_b is b else _f16_operand(teacher_b)
    s = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
    ts = float(teacher_scale.detach()) if isinstance(teacher_scale, torch.Tensor) else float(teacher_scale)
    loss = ops.cosine_kd(a16, b16, s / tau, ta16, tb16, ts / tau, normalize_a, normalize_b, normalize_teacher_a, normalize_teacher_b)[0]
    return loss * (tau * tau) if tau != 1.0 else loss


class FeatureRegFn(torch.autograd.Function):
    """A feature-level regulariser (ops.feature_reg): the L1 distance ("l1", PromptSRC) or one minus the cosine ("cos", KgCoOp) of the L2-normalised rows of
    x from a constant target.  Saves x, the target and the inverse norms; the backward is one launch (pclip_feature_reg_backward_f16) that recomputes the
    normalised rows.  x: fp16, or fp32 (cast once; the gradient comes back fp32).  The target (fp16, or fp32 cast once) receives no gradient:
    `feature_reg` refuses one that asks for it."""

    @staticmethod
    def forward(ctx, x, t, mode, normalize_t):
        x16, t16 = _f16_operand(x), _f16_operand(t)
        ctx.mode = (str(mode), bool(normalize_t))
        ctx.ref = (x.dtype, x.shape)
        loss, inv = ops.feature_reg(x16, t16, *ctx.mode)
        ctx.save_for_backward(x16, t16, inv)
        return loss

    @staticmethod
    def backward(ctx, g):
        x16, t16, inv = ctx.saved_tensors
        dx = (ops.feature_reg_backward(x16, t16, inv, *ctx.mode) * g.float()).reshape(ctx.ref[1])
        return (ops.cast_f16(dx.contiguous()) if ctx.ref[0] == torch.float16 else dx.to(ctx.ref[0])), None, None, None


def feature_reg(x, t, mode="l1", normalize_t=False):
    """The loss of `FeatureRegFn` with a tape where one is wanted, the bare forward under torch.no_grad() or for a constant x.  A target that requires grad
    is refused."""
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise PclipError("feature_reg: t requires grad, but the target receives no gradient (pass t.detach() to say so)")
    if wants_grad(x):
        return FeatureRegFn.apply(x, t, mode, normalize_t)
    return ops.feature_reg(_f16_operand(x.detach()), _f16_operand(t), mode, normalize_t)[0]


class GroupedCosineCeFn(torch.autograd.Function):
    """G independent labelled cross-entropies over cosine logits in one call (ops.cosine_cross_entropy_grouped): a [G, M, D] (or [G, D]), b [G, T, D],
    labels [G, M].  Returns the [G] VECTOR of group losses — the caller chooses the reduction — each the bits of `CosineCeFn` on that group alone.
    The backward takes g [G], runs the grouped backward with weight 1 / M and multiplies group q's gradient by g[q] in fp32 (one broadcast multiply), then
    casts back as `CosineCeFn` does.  A 0-dim tensor `scale` receives sum_q g[q] * dscale[q]: the products rounded to fp32, then added one by one in
    ASCENDING q in fp32 (on the host: the tensor-scale path reads the scale's value there anyway — one more sync, and no graph capture)."""

    @staticmethod
    def forward(ctx, a, b, scale, labels, normalize_a, normalize_b):
        a16, b16 = _f16_operand(a), _f16_operand(b)
        ctx.scale = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
        ctx.mode = (bool(normalize_a), bool(normalize_b))
        ctx.refs = tuple((t.dtype, t.shape) if isinstance(t, torch.Tensor) else None for t in (a, b, scale))      # what each gradient is cast back to
        loss, lse_row, _ = ops.cosine_cross_entropy_grouped(a16, b16, ctx.scale, labels, *ctx.mode)
        ctx.save_for_backward(a16, b16, lse_row, labels)
        return loss

    @staticmethod
    def backward(ctx, g):
        a16, b16, lse_row, labels = ctx.saved_tensors
        need_a, need_b, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ga, gb, gs = ops.cosine_cross_entropy_grouped_backward(a16, b16, ctx.scale, lse_row, labels, *ctx.mode, want_a=need_a, want_b=need_b, want_scale=need_s)
        g = g.float()

        def cast(t, ref):
            if t is None:
                return None
            t = (t * g.view(-1, 1, 1)).reshape(ref[1])
            return ops.cast_f16(t.contiguous()) if ref[0] == torch.float16 else t.to(ref[0])
        if need_s:
            total = np.cumsum((gs * g).cpu().numpy(), dtype=np.float32)[-1]                           # ((p0 + p1) + p2) + ..: numpy accumulates in index order
            gs = torch.full(ctx.refs[2][1], float(total), dtype=torch.float32, device=g.device).to(ctx.refs[2][0])
        return (cast(ga, ctx.refs[0]) if need_a else None, cast(gb, ctx.refs[1]) if need_b else None, gs if need_s else None, None, None, None)


def cosine_cross_entropy_grouped(a, b, scale, labels, normalize_a=False, normalize_b=False):
    """The [G] losses of `GroupedCosineCeFn` with a tape where one is wanted, the bare forward under torch.no_grad() or for constants."""
    if wants_grad(a, b, scale if isinstance(scale, torch.Tensor) else None):
        return GroupedCosineCeFn.apply(a, b, scale, labels, normalize_a, normalize_b)
    s = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
    return ops.cosine_cross_entropy_grouped(_f16_operand(a.detach()), _f16_operand(b.detach()), s, labels, normalize_a, normalize_b)[0]


class CosineSigmoidFn(torch.autograd.Function):
    """SigLIP's pairwise sigmoid loss over scale * a' @ b'^T + bias, multi-positive by ids (ops.cosine_sigmoid).  Saves the operands and the ids — nothing of
    size M T, and nothing from the forward; the backward recomputes logit tiles (pclip_cosine_sigmoid_backward_f16).  a, b: fp16, or fp32 (cast once; the
    gradient comes back fp32).  scale, bias: each a Python float, or a 0-dim tensor that then receives a gradient (its VALUE is read on the host: one sync,
    and no graph capture)."""

    @staticmethod
    def forward(ctx, a, b, scale, bias, ids_a, ids_b, normalize_a, normalize_b):
        a16 = a if a.dtype == torch.float16 else ops.cast_f16(a.float().contiguous())
        b16 = b if b.dtype == torch.float16 else ops.cast_f16(b.float().contiguous())
        ctx.scale = float(scale.detach()) if isinstance(scale, torch.Tensor) else float(scale)
        ctx.bias = float(bias.detach()) if isinstance(bias, torch.Tensor) else float(bias)
        ctx.mode = (bool(normalize_a), bool(normalize_b))
        ctx.refs = tuple((t.dtype, t.shape) if isinstance(t, torch.Tensor) else None for t in (a, b, scale, bias))      # what each gradient is cast back to
        ctx.has_ids = ids_a is not None
        loss = ops.cosine_sigmoid(a16, b16, ctx.scale, ctx.bias, ids_a, ids_b, *ctx.mode)
        ctx.save_for_backward(*((a16, b16, ids_a, ids_b) if ctx.has_ids else (a16, b16)))
        return loss

    @staticmethod
    def backward(ctx, g):
        a16, b16 = ctx.saved_tensors[:2]
        ids_a, ids_b = ctx.saved_tensors[2:] if ctx.has_ids else (None, None)
        need = ctx.needs_input_grad[:4]
        got = ops.cosine_sigmoid_backward(a16, b16, ctx.scale, ctx.bias, ids_a, ids_b, *ctx.mode, want_a=need[0], want_b=need[1], want_scale=need[2],
                                          want_bias=need[3])
        g = g.float()

        def cast(t, ref):
            if t is None:
                return None
            t = (t * g).reshape(ref[1])
            return ops.cast_f16(t.contiguous()) if ref[0] == torch.float16 else t.to(ref[0])
        return tuple(cast(t, ref) if n else None for t, ref, n in zip(got, ctx.refs, need)) + (None, None, None, None)


def cosine_sigmoid_loss(a, b, scale, bias, ids_a=None, ids_b=None, normalize_a=False, normalize_b=False):
    """The loss of `CosineSigmoidFn` with a tape where one is wanted, the bare forward under torch.no_grad() or for constants."""
    tensor = lambda v: v if isinstance(v, torch.Tensor) else None
    if wants_grad(a, b, tensor(scale), tensor(bias)):
        return CosineSigmoidFn.apply(a, b, scale, bias, ids_a, ids_b, normalize_a, normalize_b)
    a16 = a if a.dtype == torch.float16 else ops.cast_f16(a.detach().float().contiguous())
    b16 = b if b.dtype == torch.float16 else ops.cast_f16(b.detach().float().contiguous())
    value = lambda v: float(v.detach()) if isinstance(v, torch.Tensor) else float(v)
    return ops.cosine_sigmoid(a16.detach(), b16.detach(), value(scale), value(bias), ids_a, ids_b, normalize_a, normalize_b)


def wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---- fine-tuning the transformer towers: a differentiable tail of residual blocks + final LayerNorm + projection ---------------------------------
# (clip/model.py:171-190 per block, 233-236 / 348-352 for the heads.)  The taped forward walks the blocks with tower.residual_block, the one statement of a
# block that the frozen walk (tower._run_blocks) issues too, so its features equal the untaped ones bit for bit; its recorder keeps the tensors the
# backward reads (copies where the residual stream is updated in place).  The backward is a sequence of library kernels: pclip_gemm_f16 for dX = dY W
# (W^T cached per weight version) and dW = dY^T X (transposed operands, the token count padded to a multiple of 8 with zero rows), pclip_colsum_f16
# for the bias gradients, pclip_quick_gelu_backward_f16 on the recomputed c_fc pre-activation, pclip_layernorm_backward_g32_f16 (which also adds the
# gradient that passes the LayerNorm on the residual stream: one rounding per add) and pclip_attention_backward_f16.  The activation-gradient stream is
# fp16; parameter gradients arrive in the parameter's dtype.

TOWER_MAX_L = 288      # the attention backward's envelope (the forward's resident-K/V kernels)


def _pad_rows8(t):
    """Zero rows up to a multiple of 8: the contraction length of dW = dY^T X (pclip_gemm_f16 needs K % 8 == 0)."""
    pad = (-t.shape[0]) % 8
    return t if pad == 0 else torch.cat([t, t.new_zeros(pad, t.shape[1])], dim=0)


def _weight_grad(dy, x):
    """dW [N, K] = dY^T X for y = x W^T: pclip_gemm_f16 on the two transposed operands."""
    return ops.gemm(ops.transpose(_pad_rows8(dy)), ops.transpose(_pad_rows8(x)))


def _bias_grad(dy):
    return ops.cast_f16(ops.colsum_f16(dy))


class TowerTailFn(torch.autograd.Function):
    """x [B*L, W] (the residual stream entering the first taped block: a constant, or — learned prompt rows, `PromptEmbedFn` — a tensor on the tape,
    which then receives the stream gradient that leaves the first block) -> features [B, E] through `len(blocks)` residual blocks, the row pick
    (class token / EOT row), the final LayerNorm and the projection.  Arguments after the bookkeeping: the 12 parameters of every taped block (block
    order, each in _block_params' order), then ln.weight, ln.bias, proj.  The backward issues a weight / bias gradient only for a parameter that
    requires one: a frozen tower under a trainable input pays for none.

    deep (prompt learning; None otherwise): fp32 [n_deep, P, W], a tensor on the tape; deep_off, the ninth entry of `meta` (None without a pack): the first
    of the pack's rows in a sequence — L - P for visual prompts behind the patch rows (VPT), 1 for the context rows of a causal text tower (MaPLe).  Before
    taped block i's ln_1, 1 <= i <= n_deep, rows deep_off .. deep_off + P - 1 of every sequence are REPLACED by r16(deep[i - 1]) (ops.rows_replace_); the
    backward sums those rows of the stream gradient that leaves block i's ln_1 backward into ddeep[i - 1] and clears them in the same pass (ops.rows_grad,
    clear): a replaced row passes no gradient to the block below.  Called with nothing that requires a gradient (under torch.no_grad()) the forward issues
    the same kernels and keeps nothing for a backward."""

    @staticmethod
    def forward(ctx, x, h0, deep, meta, *params):
        B, L, heads, causal, select, sel_rows, first_token, cache, deep_off = meta
        nb = (len(params) - 3) // 12
        ctx.meta, ctx.nb = meta, nb
        n_deep = 0 if deep is None else deep.shape[0]
        ctx.deep_shape = None if deep is None else tuple(deep.shape)
        taping = any(ctx.needs_input_grad)                                     # under torch.no_grad() nothing is kept: no copies, no tape
        if ctx.needs_input_grad[0] and nb > 0:                                 # the blocks update the stream in place: a taped input keeps its values
            x = x.clone()
        tape = []
        if nb > 0:
            h = h0 if h0 is not None else ops.layernorm(x, params[0], params[1])
        for i in range(nb):
            last = i == nb - 1
            rec = {} if taping else None
            x, _ = residual_block(x, h, params[12 * i:12 * i + 12], B, L, heads, causal, select if last else None, first_token, rec=rec)
            if not last:
                if i < n_deep:                                                 # block i + 1 reads its own prompt rows: replaced before its ln_1
                    ops.rows_replace_(x, deep[i], B, L, deep_off)
                h = ops.layernorm(x, params[12 * (i + 1)], params[12 * (i + 1) + 1])
            if taping:
                tape.append(rec)
        if select is not None and nb == 0:
            x = select(x)
        lnw, lnb, proj = params[-3:]
        y = ops.layernorm(x, lnw, lnb)
        projT = cache.get("tail_projT", proj, lambda t: t.t().contiguous())
        ctx.tape, ctx.x_out, ctx.y = tape, x, y
        ctx.save_for_backward(*params)
        return ops.gemm(y, projT)

    @staticmethod
    def backward(ctx, g):
        B, L, heads, causal, select, sel_rows, first_token, cache, deep_off = ctx.meta
        params = ctx.saved_tensors
        nb = ctx.nb
        grads = [None] * len(params)
        need = ctx.needs_input_grad[4:]
        ddeep = None
        if ctx.deep_shape is not None and ctx.needs_input_grad[2]:
            ddeep = torch.zeros(ctx.deep_shape, dtype=torch.float32, device=g.device)
        n_deep = 0 if ctx.deep_shape is None else ctx.deep_shape[0]
        wgrad = lambda k, dy, x: _weight_grad(dy, x) if need[k] else None      # a frozen parameter's gradient is not computed at all
        bgrad = lambda k, dy: _bias_grad(dy) if need[k] else None
        lnw, lnb, proj = params[-3:]
        g = g.contiguous()
        if g.dtype != torch.float16:
            g = ops.cast_f16(g.float())
        # features = y proj: dproj = y^T g, dy = g proj^T
        if need[-1]:
            grads[-1] = ops.gemm(ops.transpose(_pad_rows8(ctx.y)), ops.transpose(_pad_rows8(g)))
        dy = ops.gemm(g, proj)
        gx, dg, db = ops.layernorm_backward_f32(ctx.x_out, lnw, dy)
        grads[-3], grads[-2] = dg, db
        W = ctx.x_out.shape[1]

        def wT(key, w):
            return cache.get(key, w, lambda t: t.t().contiguous())

        for i in range(nb - 1, -1, -1):
            ln1w, ln1b, win, bin_, wout, bout, ln2w, ln2b, wfc, bfc, wpr, bpr = params[12 * i:12 * i + 12]
            rec = ctx.tape[i]
            o = 12 * i
            # x_out = x_mid + c_proj(f), f = QuickGELU(u), u = c_fc(h2), h2 = ln_2(x_mid)
            grads[o + 10], grads[o + 11] = wgrad(o + 10, gx, rec["f"]), bgrad(o + 11, gx)
            df = ops.gemm(gx, wT(("tail_wT", i, "pr"), wpr))
            u = ops.gemm(rec["h2"], wfc, bfc)                                  # the pre-activation, recomputed (the forward's epilogue keeps only f)
            du = ops.quick_gelu_backward(u, df)
            del u, df
            grads[o + 8], grads[o + 9] = wgrad(o + 8, du, rec["h2"]), bgrad(o + 9, du)
            dh2 = ops.gemm(du, wT(("tail_wT", i, "fc"), wfc))
            del du
            gx, grads[o + 6], grads[o + 7] = ops.layernorm_backward_f32(rec["x_mid"], ln2w, dh2, residual=gx)
            # x_mid = x_in + out_proj(a)
            grads[o + 4], grads[o + 5] = wgrad(o + 4, gx, rec["a"]), bgrad(o + 5, gx)
            da = ops.gemm(gx, wT(("tail_wT", i, "out"), wout))
            if rec["picked"]:                                                  # only B rows left the block: zeros on the others
                full = torch.zeros(B * L, W, dtype=torch.float16, device=gx.device)
                full[sel_rows] = da
                da = full
                full = torch.zeros(B * L, W, dtype=torch.float16, device=gx.device)
                full[sel_rows] = gx
                gx = full
            if "qkv" in rec:
                qkv = rec["qkv"]
            else:                                                              # class-token form: queries of the other rows are never read (their dO is zero)
                qkv = torch.zeros(B * L, 3 * W, dtype=torch.float16, device=gx.device)
                qkv[:, W:] = rec["kv"]
                qkv[sel_rows, :W] = rec["q"]
            dqkv = ops.attention_backward(qkv, da, B, L, heads, causal=causal)
            del qkv, da
            grads[o + 2], grads[o + 3] = wgrad(o + 2, dqkv, rec["h1"]), bgrad(o + 3, dqkv)
            dh1 = ops.gemm(dqkv, wT(("tail_wT", i, "in"), win))
            del dqkv
            gx, grads[o + 0], grads[o + 1] = ops.layernorm_backward_f32(rec["x_in"], ln1w, dh1, residual=gx)
            if 1 <= i <= n_deep:                                               # the replaced rows: their gradient is deep[i - 1]'s and goes no further
                d = ops.rows_grad(gx, B, L, deep_off, ctx.deep_shape[1], clear=True)
                if ddeep is not None:
                    ddeep[i - 1] = d
        dx = None
        if ctx.needs_input_grad[0]:                                            # the stream gradient that leaves the first taped block (block 0's ln_1 backward)
            dx = gx
            if select is not None and nb == 0:                                 # heads only: the picked rows are all that reached the final LayerNorm
                dx = torch.zeros(B * L, W, dtype=torch.float16, device=gx.device)
                dx[sel_rows] = gx
        out = [gr.reshape(p.shape) if n else None for p, gr, n in zip(params, grads, need)]
        return (dx, None, ddeep, None) + tuple(out)


def run_tower_tail(tw, x, h0, first, B, L, pick, what, deep=None, deep_off=None):
    """The taped tail of tower `tw` (a tower.Tower): blocks[first:] + final LayerNorm + projection on the residual stream x [B*L, W] (h0: ln_1 of
    blocks[first] when the caller already has it).  pick = (select, rows) from `tw.pick`, or (None, None) when x already holds the picked rows.
    deep: TowerTailFn's pack of deep prompt rows, fp32 [n_deep, P, W] with n_deep < len(blocks) - first and P < L; deep_off: the first of the P rows in a
    sequence, deep_off + P <= L (None: the last P rows, L - P)."""
    blocks, (select, rows) = tw.blocks, pick
    if ops.splitk_active(B) or ops.splitk_active(B * L):
        raise PclipError(f"{what}: a differentiable pass inside ops.low_latency() is not supported (the split-K linears have no backward); "
                         f"leave the context or freeze the tower (B={B}, L={L})")
    if L > TOWER_MAX_L and first < len(blocks):
        raise PclipError(f"{what}: sequences of L={L} tokens exceed the attention backward's envelope (L <= {TOWER_MAX_L}); "
                         "this tower can only run frozen")
    params = [p for blk in blocks[first:] for p in _block_params(blk)] + [tw.ln.weight, tw.ln.bias, tw.proj]
    for p in params:
        if p.requires_grad and p.dtype not in (torch.float16, torch.float32):
            raise PclipError(f"{what}: unsupported parameter dtype {p.dtype}")
    if deep is not None:
        if deep.dtype != torch.float32 or deep.dim() != 3 or deep.shape[2] != x.shape[1] or not 1 <= deep.shape[1] < L:
            raise PclipError(f"{what}: deep prompts {deep.dtype} {tuple(deep.shape)} are not float32 [n_deep, P, {x.shape[1]}] with 1 <= P < L={L}")
        if not 1 <= deep.shape[0] < len(blocks) - first:
            raise PclipError(f"{what}: {deep.shape[0]} deep prompt layers, but only blocks {first + 1}..{len(blocks) - 1} can take one")
    if deep_off is not None:
        if deep is None:
            raise PclipError(f"{what}: deep_off={deep_off} without a pack of deep prompt rows")
        deep_off = int(deep_off)
        if deep_off < 0 or deep_off + deep.shape[1] > L:
            raise PclipError(f"{what}: deep prompt rows deep_off .. deep_off + P - 1 = {deep_off} .. {deep_off + deep.shape[1] - 1} do not lie inside a "
                             f"sequence of L={L} tokens")
    if deep is not None and deep_off is None:
        deep_off = L - deep.shape[1]
    meta = (B, L, tw.heads, tw.causal, select, None if select is None else rows(), tw.first_token, tw.cache, deep_off)
    return TowerTailFn.apply(x, h0, deep, meta, *params)


# ---- the stages in front of block 0: whole-tower fine-tuning (CLIP.unfreeze(stem=...)) ---------------------------------------------------------------
# Both Functions put the residual stream that enters block 0 on the tape with the same kernels, hence the same bits, as the frozen path; TowerTailFn
# (taped from block 0) hands back the stream gradient.  A gradient is computed only for a parameter that requires one and arrives in its dtype.

def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


def _stem_dx(dx):
    dx = dx.contiguous()
    return dx if dx.dtype == torch.float16 else ops.cast_f16(dx.float())


class VitStemFn(torch.autograd.Function):
    """(img, conv1.weight, class_embedding, positional_embedding, ln_pre.weight, ln_pre.bias) -> x [B*L, W] fp16 = ln_pre([class ; conv1(img)] + pos)
    (clip/model.py:222-227): im2col + GEMM, token assembly, LayerNorm — the bits of the fused pclip_vit_embed_ln_f16 pass.  Kept for the backward: the
    pre-LayerNorm tokens; the im2col matrix is recomputed from the image (the caller holds the image anyway; the matrix would be a second copy of
    it).  backward: pclip_layernorm_backward_g32_f16 -> dt, dln_pre; pclip_vit_embed_backward_f16 -> dpos (row 0 = dclass), dpatch;
    dconv1 = dpatch^T cols, cut from the padded columns.  The pixels get no gradient."""

    @staticmethod
    def forward(ctx, img, wconv, cls, pos, lnw, lnb, P, cache):
        B, W = img.shape[0], wconv.shape[0]
        G2 = (img.shape[2] // P) ** 2
        kp = 3 * P * P
        tokens = vit_stem(cache, img, wconv, cls, pos, P)
        ctx.shape = (B, G2 + 1, W, P, kp)
        ctx.save_for_backward(img, tokens, wconv, cls, pos, lnw, lnb)
        return ops.layernorm(tokens, _f32(lnw), _f32(lnb))

    @staticmethod
    def backward(ctx, dx):
        img, tokens, wconv, cls, pos, lnw, lnb = ctx.saved_tensors
        B, L, W, P, kp = ctx.shape
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("VitStemFn: the pixels get no gradient; detach the images")
        need = ctx.needs_input_grad
        dt, dg, db = ops.layernorm_backward_f32(tokens, _f32(lnw), _stem_dx(dx))
        dpos, dpatch = ops.vit_embed_backward(dt, B, L, want_pos=need[2] or need[3], want_patch=need[1])
        dw = None                                                          # (dclass is a copy of dpos' row 0: the two .grad tensors must not share storage)
        if need[1]:
            dw = _weight_grad(dpatch, ops.im2col_patches(img, P))[:, :kp].reshape(wconv.shape)          # fp16 [W, kpad] -> [W, 3, P, P]
            dw = dw.contiguous() if wconv.dtype == torch.float16 else dw.float()
        return (None, dw, _like(dpos[0].clone(), cls) if need[2] else None, _like(dpos, pos) if need[3] else None,
                _like(dg, lnw) if need[4] else None, _like(db, lnb) if need[5] else None, None, None)


class TextEmbedFn(torch.autograd.Function):
    """(tokens, token_embedding.weight, positional_embedding) -> x [B*L, W] fp16 = token_embedding[tokens] + positional_embedding (clip/model.py:342-344),
    the bits of ops.text_embed.  backward: pclip_text_embed_backward (dense fp32 dE by a fixed-order segmented reduction, dpos summed over the prompts)."""

    @staticmethod
    def forward(ctx, tokens, emb, pos, cache):
        emb16 = cache.get("tok", emb, lambda t: t.half().contiguous())
        pos16 = cache.get("pos", pos, lambda t: t.half().contiguous())
        tokens = tokens.to(torch.int64).contiguous()
        ctx.save_for_backward(tokens, emb, pos)
        return ops.text_embed(tokens, emb16, pos16)

    @staticmethod
    def backward(ctx, dx):
        tokens, emb, pos = ctx.saved_tensors
        dE, dpos = ops.text_embed_backward(_stem_dx(dx), tokens, emb.shape[0], want_emb=ctx.needs_input_grad[1], want_pos=ctx.needs_input_grad[2])
        return None, _like(dE, emb), _like(dpos, pos), None


# ---- learned prompt context (CoOp): the embedded prompts as a function of the fp32 context rows ---------------------------------------------------

class PromptEmbedFn(torch.autograd.Function):
    """(ctx, tokens, emb16, pos16, n_ctx, L_out) -> x [N * L_out, W] fp16, the residual stream that enters block 0 of the text tower: the fp32 context
    rows `ctx` ([n_ctx, W] shared, or [N, n_ctx, W]) at positions 1 .. n_ctx, the token embeddings elsewhere, plus the positional embedding
    (pclip_prompt_embed_f16).  backward: dctx in fp32 (pclip_prompt_ctx_grad_f32: a fixed summation order over the classes, no atomics); nothing else
    gets a gradient."""

    @staticmethod
    def forward(ctx, ctx_rows, tokens, emb16, pos16, n_ctx, L_out):
        if ctx_rows.shape[-2] != n_ctx:
            raise PclipError(f"PromptEmbedFn: context {tuple(ctx_rows.shape)} does not hold n_ctx={n_ctx} rows")
        ctx.shape = (tokens.shape[0], int(L_out), int(n_ctx), ctx_rows.dim() == 3)
        return ops.prompt_embed(ctx_rows, tokens, emb16, pos16, L_out)

    @staticmethod
    def backward(ctx, dx):
        N, L_out, n_ctx, per_class = ctx.shape
        dx = dx.contiguous()
        if dx.dtype != torch.float16:
            dx = ops.cast_f16(dx.float())
        return ops.prompt_ctx_grad(dx, N, L_out, n_ctx, per_class), None, None, None, None, None


# ---- MaPLe's coupling function: the visual prompt rows of every depth as a linear function of that depth's text rows ----------------------------------

class CoupleFn(torch.autograd.Function):
    """(x [depth, P, Wt], weight [depth, Wv, Wt], bias [depth, Wv], all fp32) -> y [depth, P, Wv] fp32 = x[d] @ weight[d].T + bias[d]: every depth in one
    launch (pclip_couple_fwd_f32).  backward: pclip_couple_bwd_f32 issues only the gradients `needs_input_grad` asks for — dx = dy[d] @ weight[d],
    dweight = dy[d].T @ x[d], dbias = dy[d].sum(0) — each in the one summation order csrc/pclip_maple.hip documents."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return ops.couple(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dy.dtype != torch.float32:
            raise PclipError(f"CoupleFn: the gradient of the coupled rows must be float32, got {dy.dtype}")
        return ops.couple_backward(dy.contiguous(), x, weight, want_x=need[0], want_weight=need[1], want_bias=need[2])


# ---- CoCoOp: the per-image shift of the context rows and the prompts assembled with it ------------------------------------------------------------------

class MetaNetFn(torch.autograd.Function):
    """(f [B, E] fp16, w1 [Hd, E], b1 [Hd], w2 [Wt, Hd], b2 [Wt], the four fp32) -> pi [B, Wt] fp32 = relu(f @ w1.T + b1) @ w2.T + b2
    (pclip_metanet_fwd_f32).  backward: pclip_metanet_bwd_f32 issues only the gradients `needs_input_grad` asks for, each in the one summation order
    csrc/pclip_cocoop.hip documents; f (cached, normalised image features) is a constant and gets none."""

    @staticmethod
    def forward(ctx, f, w1, b1, w2, b2):
        h, pi = ops.metanet(f, w1, b1, w2, b2)
        ctx.save_for_backward(f, h, w1, w2)
        return pi

    @staticmethod
    def backward(ctx, dpi):
        f, h, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        if dpi.dtype != torch.float32:
            raise PclipError(f"MetaNetFn: the gradient of the shift must be float32, got {dpi.dtype}")
        return (None,) + ops.metanet_backward(dpi.contiguous(), f, h, w1, w2, want_w1=need[1], want_b1=need[2], want_w2=need[3], want_b2=need[4])


class CondPromptEmbedFn(torch.autograd.Function):
    """(ctx [n_ctx, W] fp32, pi [B, W] fp32, tokens [N, L_tok], emb16, pos16, L_out) -> x [B * N * L_out, W] fp16, the residual stream that enters block 0
    of the text tower for B images x N classes: the rows r16(ctx[j] + pi[b]) at positions 1 .. n_ctx of image b's prompts, the token embeddings elsewhere,
    plus the positional embedding (pclip_prompt_embed_cond_f16).  backward: (dctx, dpi) in fp32 (pclip_prompt_cond_grad_f32: fixed orders over classes,
    images and rows, no atomics); nothing else gets a gradient."""

    @staticmethod
    def forward(ctx, ctx_rows, pi, tokens, emb16, pos16, L_out):
        ctx.shape = (pi.shape[0], tokens.shape[0], int(L_out), ctx_rows.shape[0])
        return ops.prompt_embed_cond(ctx_rows, pi, tokens, emb16, pos16, L_out)

    @staticmethod
    def backward(ctx, dx):
        B, N, L_out, n_ctx = ctx.shape
        dx = dx.contiguous()
        if dx.dtype != torch.float16:
            dx = ops.cast_f16(dx.float())
        dctx, dpi, _ = ops.prompt_cond_grad(dx, B, N, L_out, n_ctx)
        return dctx, dpi, None, None, None, None


# ---- visual prompt tuning (VPT): the stream that enters block 0 as a function of the first layer's fp32 prompt rows ------------------------------------

class VptEmbedFn(torch.autograd.Function):
    """(ctx0 [P, W] fp32, t [B * L0, W] fp16, ln_pre.weight, ln_pre.bias, B, L0) -> x [B * (L0 + P), W] fp16 = ln_pre(append(t, ctx0)): the stem's
    tokens (class + patches + positional embedding, a constant of the frozen stem) with the prompt rows behind them, then ln_pre (clip/model.py:227).
    backward: only the B * P prompt rows of dx have a consumer while the stem is frozen — they are gathered into a compact buffer, taken through the
    LayerNorm backward against their pre-LayerNorm values (r16(ctx0) in every sequence: rebuilt, not kept) and summed over the batch in
    pclip_vpt_grad_f32's fixed order.  ln_pre's parameters and t get no gradient here."""

    @staticmethod
    def forward(ctx, ctx0, t, lnw, lnb, B, L0):
        ctx.shape = (int(B), int(L0), ctx0.shape[0])
        ctx.save_for_backward(ctx0, lnw)
        return ops.layernorm(ops.vpt_append(t, ctx0, B, L0), _f32(lnw), _f32(lnb))

    @staticmethod
    def backward(ctx, dx):
        ctx0, lnw = ctx.saved_tensors
        B, L0, P = ctx.shape
        W = ctx0.shape[1]
        if any(ctx.needs_input_grad[1:4]):
            raise NotImplementedError("VptEmbedFn: only the prompt rows get a gradient (the stem and ln_pre are frozen under visual prompt tuning)")
        dy = _stem_dx(dx).view(B, L0 + P, W)[:, L0:, :].reshape(B * P, W)        # the prompt rows, compact
        rows = ops.vpt_append(None, ctx0, B, 0)                                   # what ln_pre read on those rows
        dt, _, _ = ops.layernorm_backward_f32(rows, _f32(lnw), dy)
        return ops.vpt_grad(dt, B, 0, P), None, None, None, None, None
