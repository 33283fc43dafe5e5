#!/usr/bin/env python3
"""Generates tests/golden/promptsrc_grad_<case>.npz and promptsrc_sgd_tiny.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's
import shim (the recipe of make_golden_maple.py): the reference's own `build_model(...)`, `encode_text` and `encode_image` on seeded towers
(random_state_dict + trained_like_), with PromptSRC's independent prompts put into both towers by hooks alone:

  text    `hooked_text` of make_golden_maple.py with ctx [depth_text, n_ctx_text, Wt];
  vision  `hooked_features` of make_golden_vpt.py with vctx [depth_vision, n_ctx_vision, Wv] — its own tensor, row count and depth, no coupling function.
The teacher is the same reference model without hooks: its `encode_image` of the same images, and its `encode_text` of the hand-written templates' token rows
(tests/promptsrc_ref.py: two templates; the mean of the UN-normalised features, then one normalisation).  This file holds no reference code, only calls
into it.

    python tests/golden/make_golden_promptsrc.py            # the fixtures
    python tests/golden/make_golden_promptsrc.py sgd        # the five-step decrease of the total loss, stored in promptsrc_sgd_tiny.npz

The loss is promptsrc_ref.terms64 / total64 — cross-entropy + 25 text L1 + 10 image L1 + (1 / N) batch-mean KL to the zero-shot logits — in float64 on the
delivered features, the student's on the tape and the teacher's constants; scale = exp(float32(log 20)).

Two runs per case:
  f64      the reference model `.double()` with the float64 LayerNorm swap (see make_golden_tower_grad.py) and float64 prompts: `g_ctx_f64`, `g_vctx_f64`, the
           gradients every implementation is graded against, `img_f64`, `txt_f64`, the four terms `ce_f64`, `l_text_f64`, `l_image_f64`, `kd_f64` and
           `loss_f64`;
  fp16     the reference's own fp16 chain on the CPU with fp32 prompts (cast to fp16 where they enter the stream), the teacher's features from the same fp16
           model: `loss_f16`, the four terms `*_f16`, e_ref_<ctx|vctx>[d] = ||g_fp16chain[d] - g_f64[d]||_2 / ||g_f64[d]||_2 per depth slice, and
           img_e_ref / txt_e_ref, the same relative distance over the features.
tests/test_gpu_promptsrc.py asks ||g_ours[d] - g_f64[d]||_2 / ||g_f64[d]||_2 <= 2 e_ref[d] per slice, the same of the features, and
|loss_ours - loss_f64| <= 2 |loss_f16 - loss_f64|.  The floor is recorded as 0: `main` asserts that no e_ref lies below the feature kernel's own derived
tolerance (a relative 2^-24 times a few dozen operations), where a floor would be due.

The parameters, the tokens, the images and the labels are regenerated in the test from the seeds stored here (tests/promptsrc_ref.py: fixture_inputs)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
sys.path.insert(0, os.path.dirname(HERE))
import promptsrc_ref as pr                                          # noqa: E402  (the cases, the seeded inputs and the float64 loss, shared with the tests)
from make_golden_maple import hooked_text                           # noqa: E402  (the text-side hooks)
from make_golden_vpt import hooked_features as hooked_image, models   # noqa: E402  (the vision-side hooks and the seeded reference models)

FLOOR = 0.0
KERNEL_TOLERANCE = 64 * 2.0 ** -24           # csrc/pclip_feature_reg.hip: a few dozen rounded fp32 operations on a term's path (tests/feature_reg_ref.py)


def teacher(model, teacher_tokens, images):
    """The frozen model's constants: (un-normalised image features, fixed text rows), in the model's dtype."""
    with torch.no_grad():
        zs_img = model.encode_image(images)
        fixed = pr.fixed_text64([model.encode_text(t) for t in teacher_tokens])
    return zs_img, fixed


def terms(model, ctx, vctx, tokens, teacher_tokens, images, labels):
    zs_img, fixed = teacher(model, teacher_tokens, images)
    img, txt = hooked_image(model, vctx, images), hooked_text(model, ctx, tokens)
    return pr.terms64(img, txt, zs_img, fixed, labels), img, txt


def grad(model, params, tokens, teacher_tokens, images, labels, N):
    ctx, vctx = (p.clone().requires_grad_(True) for p in params)
    four, img, txt = terms(model, ctx, vctx, tokens, teacher_tokens, images, labels)
    loss = pr.total64(four, N)
    loss.backward()
    return (float(loss.detach()), [float(t.detach()) for t in four], [p.grad.detach().double().clone() for p in (ctx, vctx)], img.detach().double().clone(),
            txt.detach().double().clone())


def run(ref_clip_model, kw, sd_seed, B, N, Pt, Dt, Pv, Dv, seed):
    m16, m64 = models(ref_clip_model, kw, sd_seed, (torch.float16, torch.float64))
    ctx, vctx, tokens, teacher_tokens, images, labels = pr.fixture_inputs(kw, B, N, Pt, Dt, Pv, Dv, seed)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        l64, t64, g64, i64, x64 = grad(m64, (ctx.double(), vctx.double()), tokens, teacher_tokens, images, labels, N)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    l16, t16, g16, i16, x16 = grad(m16, (ctx, vctx), tokens, teacher_tokens, images, labels, N)
    out = dict(loss_f16=l16, loss_f64=l64, img_f64=i64.float(), txt_f64=x64.float(), img_e_ref=float((i16 - i64).norm() / i64.norm()),
               txt_e_ref=float((x16 - x64).norm() / x64.norm()))
    for key, a, b in zip(("ce", "l_text", "l_image", "kd"), t16, t64):
        out[f"{key}_f16"], out[f"{key}_f64"] = a, b
    for name, a, b, depth in zip(("ctx", "vctx"), g16, g64, (Dt, Dv)):
        out[f"g_{name}_f64"] = b.float()
        out[f"e_ref_{name}"] = np.asarray([float((a[d] - b[d]).norm() / b[d].norm()) for d in range(depth)], np.float64)
    return out


def sgd_decrease(ref_clip_model):
    """The decrease of the total loss over five SGD steps on the reference's fp32 CPU chain, the case and the step rule of
    test_five_steps_of_run_promptsrc_lower_the_loss (run_promptsrc: SGD on the two tensors, momentum 0.9, cosine schedule over the five steps, one batch
    of all images)."""
    tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed, lr = pr.SGD_CASE
    kw = pr.towers()[tag]
    (m32,) = models(ref_clip_model, kw, sd_seed, (torch.float32,))
    ctx, vctx, tokens, teacher_tokens, images, labels = pr.fixture_inputs(kw, B, N, Pt, Dt, Pv, Dv, seed)
    params = [p.clone().requires_grad_(True) for p in (ctx, vctx)]
    opt = torch.optim.SGD(params, lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 5)
    losses = []
    for _ in range(5):
        loss = pr.total64(terms(m32, *params, tokens, teacher_tokens, images, labels)[0], N)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(pr.total64(terms(m32, *params, tokens, teacher_tokens, images, labels)[0], N)))
    print("reference fp32 chain, five SGD steps (lr %g):" % lr, " ".join(f"{v:.6f}" for v in losses), " decrease %.6f" % (losses[0] - losses[-1]))
    mg.savez(pr.SGD_FIXTURE, losses=np.asarray(losses, np.float64), decrease=losses[0] - losses[-1], lr=lr, seed=seed, tag=tag, sd_seed=sd_seed)


def main():
    ref_clip_model = mg.import_reference()[4]
    if sys.argv[1:] == ["sgd"]:
        return sgd_decrease(ref_clip_model)
    for name, (tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed) in pr.FIXTURES.items():
        out = run(ref_clip_model, pr.towers()[tag], sd_seed, B, N, Pt, Dt, Pv, Dv, seed)
        e_refs = [e for k in ("ctx", "vctx") for e in out[f"e_ref_{k}"]] + [out["img_e_ref"], out["txt_e_ref"]]
        print(f"{name}: loss f64 {out['loss_f64']:.6f} fp16 chain {out['loss_f16']:.6f}  terms f64 "
              + " ".join(f"{k} {out[k + '_f64']:.6f}" for k in ("ce", "l_text", "l_image", "kd")) + "  e_ref "
              + "  ".join(k + " " + " ".join(f"{e:.3e}" for e in out[f"e_ref_{k}"]) for k in ("ctx", "vctx"))
              + f"  features e_ref image {out['img_e_ref']:.3e} text {out['txt_e_ref']:.3e}")
        assert all(math.isfinite(e) and e > KERNEL_TOLERANCE for e in e_refs)            # no floor is due: the reference's own distance is far above the kernel's
        mg.savez(name, logit_scale=float(np.float32(pr.LOGIT_SCALE)), floor=FLOOR, e_ref_source="reference fp16 chain on the CPU", tag=tag, sd_seed=sd_seed,
                 B=B, N=N, Pt=Pt, Dt=Dt, Pv=Pv, Dv=Dv, seed=seed, w_text=pr.W_TEXT, w_image=pr.W_IMAGE, w_logits=pr.W_LOGITS, **out)


if __name__ == "__main__":
    main()
