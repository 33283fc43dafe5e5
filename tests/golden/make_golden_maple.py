#!/usr/bin/env python3
"""Generates tests/golden/maple_grad_<case>.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's import shim (the recipe of
make_golden_vpt.py / make_golden_coop.py): the reference's own `build_model(...)`, `encode_text` and `encode_image` on seeded towers (random_state_dict +
trained_like_), with MaPLe's prompts put into both towers by hooks alone:

  text    a forward hook on the reference's `token_embedding` overwrites rows 1 .. n_ctx of its output by ctx[0] (where CoOp's fixture splices them); forward
          pre-hooks on `transformer.resblocks[i]`, 1 <= i < depth, replace rows 1 .. n_ctx of their input (layout [L, B, W]) by ctx[i];
  vision  make_golden_vpt.py's hooks: a forward pre-hook on `visual.ln_pre` concatenates vctx[0] behind the patch rows, forward pre-hooks on
          `visual.transformer.resblocks[i]` replace the last n_ctx rows by vctx[i];
  vctx[d] = ctx[d] @ couple_weight[d].T + couple_bias[d], computed in torch here.
This file holds no reference code, only calls into it.

    python tests/golden/make_golden_maple.py            # the fixtures
    python tests/golden/make_golden_maple.py sgd        # the five-step loss decrease tests/test_gpu_maple.py quotes

The loss is the float64 cross-entropy of scale * normalize(image features) @ normalize(text features).T against seeded labels, both feature matrices cast to
float64 and both on the tape; scale = exp(float32(log 20)).

Two runs per case:
  f64      the reference model `.double()` with the float64 LayerNorm swap (see make_golden_tower_grad.py), float64 prompts and coupling: `g_ctx_f64`,
           `g_weight_f64`, `g_bias_f64`, the gradients every implementation is graded against, `img_f64`, `txt_f64` and `loss_f64`;
  fp16     the reference's own fp16 chain on the CPU with fp32 prompts and an fp32 coupling function (cast to fp16 where they enter the stream): `loss_f16`,
           e_ref_<ctx|weight|bias>[d] = ||g_fp16chain[d] - g_f64[d]||_2 / ||g_f64[d]||_2 per depth slice, and img_e_ref / txt_e_ref, the same relative distance
           over the features.
tests/test_gpu_maple.py asks ||g_ours[d] - g_f64[d]||_2 / ||g_f64[d]||_2 <= 2 e_ref[d] per slice and the same of the features, with no floor (recorded as 0).

The parameters, the tokens, the images and the labels are regenerated in the test from the seeds stored here (tests/maple_ref.py: fixture_inputs)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
sys.path.insert(0, os.path.dirname(HERE))
import maple_ref                                                    # noqa: E402  (the cases and the seeded inputs, shared with tests/test_gpu_maple.py)
from make_golden_vpt import hooked_features as hooked_image, models   # noqa: E402  (the vision-side hooks and the seeded reference models)

FLOOR = 0.0


def hooked_text(model, ctx, tokens):
    """The reference's encode_text with ctx [depth, P, Wt] spliced in by hooks."""
    depth, P = ctx.shape[0], ctx.shape[1]

    def splice(_module, _args, out):
        out = out.clone()
        out[:, 1:1 + P] = ctx[0].to(out.dtype)
        return out

    def replace_with(i):
        def replace(_module, args):
            x = args[0]                                              # [L, B, W]
            rows = ctx[i].to(x.dtype)[:, None, :].expand(-1, x.shape[1], -1)
            return (torch.cat([x[:1], rows, x[1 + P:]], dim=0),)
        return replace

    handles = [model.token_embedding.register_forward_hook(splice)]
    handles += [model.transformer.resblocks[i].register_forward_pre_hook(replace_with(i)) for i in range(1, depth)]
    try:
        return model.encode_text(tokens)
    finally:
        for h in handles:
            h.remove()


def features(model, ctx, weight, bias, tokens, images):
    vctx = torch.einsum("dpt,dvt->dpv", ctx, weight) + bias[:, None, :]          # the coupling function, in the parameters' dtype
    return hooked_image(model, vctx, images), hooked_text(model, ctx, tokens)


def grad(model, params, tokens, images, labels):
    ctx, weight, bias = (p.clone().requires_grad_(True) for p in params)
    img, txt = features(model, ctx, weight, bias, tokens, images)
    loss = maple_ref.loss64(img, txt, labels)
    loss.backward()
    return (float(loss.detach()), [p.grad.detach().double().clone() for p in (ctx, weight, bias)], img.detach().double().clone(),
            txt.detach().double().clone())


def run(ref_clip_model, kw, sd_seed, B, P, depth, N, seed, l_eff):
    m16, m64 = models(ref_clip_model, kw, sd_seed, (torch.float16, torch.float64))
    ctx, weight, bias, tokens, images, labels = maple_ref.fixture_inputs(kw, B, P, depth, N, seed, l_eff)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        l64, g64, i64, t64 = grad(m64, (ctx.double(), weight.double(), bias.double()), tokens, images, labels)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    l16, g16, i16, t16 = grad(m16, (ctx, weight, bias), tokens, images, labels)
    out = dict(loss_f16=l16, loss_f64=l64, img_f64=i64.float(), txt_f64=t64.float(), img_e_ref=float((i16 - i64).norm() / i64.norm()),
               txt_e_ref=float((t16 - t64).norm() / t64.norm()))
    for name, a, b in zip(("ctx", "weight", "bias"), g16, g64):
        out[f"g_{name}_f64"] = b.float()
        out[f"e_ref_{name}"] = np.asarray([float((a[d] - b[d]).norm() / b[d].norm()) for d in range(depth)], np.float64)
    return out


def sgd_decrease(ref_clip_model):
    """The loss decrease of five SGD steps on the reference's fp32 CPU chain, the case and the step rule of test_five_sgd_steps_of_run_maple_lower_the_loss
    (run_maple: SGD on the three tensors, momentum 0.9, cosine schedule over the five steps, one batch of all images)."""
    tag, sd_seed, B, P, depth, N, seed, lr = maple_ref.SGD_CASE
    kw = maple_ref.towers()[tag]
    (m32,) = models(ref_clip_model, kw, sd_seed, (torch.float32,))
    ctx, weight, bias, tokens, images, labels = maple_ref.fixture_inputs(kw, B, P, depth, N, seed)
    params = [p.clone().requires_grad_(True) for p in (ctx, weight, bias)]
    opt = torch.optim.SGD(params, lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 5)
    losses = []
    for _ in range(5):
        loss = maple_ref.loss64(*features(m32, *params, tokens, images), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(maple_ref.loss64(*features(m32, *params, tokens, images), labels)))
    print("reference fp32 chain, five SGD steps (lr %g):" % lr, " ".join(f"{v:.6f}" for v in losses), " decrease %.6f" % (losses[0] - losses[-1]))


def main():
    ref_clip_model = mg.import_reference()[4]
    if sys.argv[1:] == ["sgd"]:
        return sgd_decrease(ref_clip_model)
    for name, (tag, sd_seed, B, P, depth, N, seed, l_eff) in maple_ref.FIXTURES.items():
        out = run(ref_clip_model, maple_ref.towers()[tag], sd_seed, B, P, depth, N, seed, l_eff)
        e_refs = [e for k in ("ctx", "weight", "bias") for e in out[f"e_ref_{k}"]] + [out["img_e_ref"], out["txt_e_ref"]]
        print(f"{name}: loss f64 {out['loss_f64']:.6f} fp16 chain {out['loss_f16']:.6f}  e_ref "
              + "  ".join(k + " " + " ".join(f"{e:.3e}" for e in out[f"e_ref_{k}"]) for k in ("ctx", "weight", "bias"))
              + f"  features e_ref image {out['img_e_ref']:.3e} text {out['txt_e_ref']:.3e}")
        assert all(math.isfinite(e) and e > 0 for e in e_refs)
        mg.savez(name, logit_scale=float(np.float32(maple_ref.LOGIT_SCALE)), floor=FLOOR, e_ref_source="reference fp16 chain on the CPU", tag=tag,
                 sd_seed=sd_seed, B=B, P=P, depth=depth, N=N, seed=seed, l_eff=0 if l_eff is None else l_eff, **out)


if __name__ == "__main__":
    main()
