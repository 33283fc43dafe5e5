#!/usr/bin/env python3
"""Generates tests/golden/vpt_grad_<case>.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's import shim (the recipe of
make_golden_coop.py): the reference's own `build_model(...)` and `encode_image` on seeded towers (random_state_dict + trained_like_), with learned visual
prompts put into the image tower's sequence by hooks alone — a forward pre-hook on the reference's `visual.ln_pre` concatenates ctx[0] behind the patch
rows, forward pre-hooks on `visual.transformer.resblocks[i]`, 1 <= i < depth, replace the last P rows of their input (layout [L, B, W]) by ctx[i].  This
file holds no reference code, only calls into it.

    python tests/golden/make_golden_vpt.py            # the fixtures
    python tests/golden/make_golden_vpt.py sgd        # the five-step loss decrease tests/test_gpu_vpt.py quotes

The loss is the float64 cross-entropy of scale * normalize(features) @ normalize(text).T against seeded labels, on seeded text weights (fp16-exact values)
and the image features cast to float64; scale = exp(float32(log 20)).

Two runs per case:
  f64      the reference model `.double()` with the float64 LayerNorm swap (see make_golden_tower_grad.py) and float64 prompts: `g_f64` [depth, P, W], the
           gradient every implementation is graded against, `feat_f64` and `loss_f64`;
  fp16     the reference's own fp16 chain on the CPU with the fp32 prompts (cast to fp16 where they enter the stream): `loss_f16`,
           e_ref[i] = ||g_fp16chain[i] - g_f64[i]||_2 / ||g_f64[i]||_2 per depth slice, and feat_e_ref, the same relative distance over the features.
tests/test_gpu_vpt.py asks ||g_ours[i] - g_f64[i]||_2 / ||g_f64[i]||_2 <= 2 e_ref[i] and the same of the features, with no floor (recorded as 0).

The prompts, the images, the text weights and the labels are regenerated in the test from the seeds stored here (tests/vpt_ref.py: fixture_inputs)."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
from proto_clip_amd.clip.model import random_state_dict            # noqa: E402
from spec import trained_like_                                      # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import vpt_ref                                                      # noqa: E402  (the cases and the seeded inputs, shared with tests/test_gpu_vpt.py)

FLOOR = 0.0


def hooked_features(model, ctx, images):
    """The reference's encode_image with ctx [depth, P, W] spliced in by hooks."""
    vis = model.visual
    depth, P = ctx.shape[0], ctx.shape[1]

    def append(_module, args):
        x = args[0]                                                  # [B, L0, W]
        return (torch.cat([x, ctx[0].to(x.dtype).expand(x.shape[0], -1, -1)], dim=1),)

    def replace_with(i):
        def replace(_module, args):
            x = args[0]                                              # [L, B, W]
            return (torch.cat([x[:-P], ctx[i].to(x.dtype)[:, None, :].expand(-1, x.shape[1], -1)], dim=0),)
        return replace

    handles = [vis.ln_pre.register_forward_pre_hook(append)]
    handles += [vis.transformer.resblocks[i].register_forward_pre_hook(replace_with(i)) for i in range(1, depth)]
    try:
        return model.encode_image(images)
    finally:
        for h in handles:
            h.remove()


def grad(model, ctx, images, text, labels):
    ctx = ctx.clone().requires_grad_(True)
    feats = hooked_features(model, ctx, images)
    loss = vpt_ref.loss64(feats, text, labels)
    loss.backward()
    return float(loss.detach()), ctx.grad.detach().double().clone(), feats.detach().double().clone()


def models(ref_clip_model, kw, sd_seed, dtypes):
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(vpt_ref.LOGIT_SCALE, dtype=torch.float32)
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for dt in dtypes:
            m = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
            out.append(m if dt == torch.float16 else m.to(dt))
    for m in out:
        for p in m.parameters():
            p.requires_grad_(False)
    return out


def run(ref_clip_model, kw, sd_seed, B, P, depth, N, seed):
    m16, m64 = models(ref_clip_model, kw, sd_seed, (torch.float16, torch.float64))
    ctx, images, text, labels = vpt_ref.fixture_inputs(kw, B, P, depth, N, seed)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        l64, g64, f64 = grad(m64, ctx.double(), images, text, labels)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    l16, g16, f16 = grad(m16, ctx, images, text, labels)
    e_ref = [float((g16[i] - g64[i]).norm() / g64[i].norm()) for i in range(depth)]
    return dict(loss_f16=l16, loss_f64=l64, g_f64=g64.float(), e_ref=np.asarray(e_ref, np.float64), feat_f64=f64.float(),
                feat_e_ref=float((f16 - f64).norm() / f64.norm()))


def sgd_decrease(ref_clip_model):
    """The loss decrease of five SGD steps on the reference's fp32 CPU chain, the case and the step rule of test_five_sgd_steps_of_run_vpt_lower_the_loss
    (run_vpt: SGD, momentum 0.9, cosine schedule over the five steps, one batch of all images)."""
    tag, sd_seed, B, P, depth, N, seed, lr = vpt_ref.SGD_CASE
    kw = vpt_ref.towers()[tag]
    (m32,) = models(ref_clip_model, kw, sd_seed, (torch.float32,))
    ctx, images, text, labels = vpt_ref.fixture_inputs(kw, B, P, depth, N, seed)
    ctx = ctx.clone().requires_grad_(True)
    opt = torch.optim.SGD([ctx], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 5)
    losses = []
    for _ in range(5):
        loss = vpt_ref.loss64(hooked_features(m32, ctx, images), text, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(vpt_ref.loss64(hooked_features(m32, ctx, images), text, labels)))
    print("reference fp32 chain, five SGD steps (lr %g):" % lr, " ".join(f"{v:.6f}" for v in losses), " decrease %.6f" % (losses[0] - losses[-1]))


def main():
    ref_clip_model = mg.import_reference()[4]
    if sys.argv[1:] == ["sgd"]:
        return sgd_decrease(ref_clip_model)
    for name, (tag, sd_seed, B, P, depth, N, seed) in vpt_ref.FIXTURES.items():
        out = run(ref_clip_model, vpt_ref.towers()[tag], sd_seed, B, P, depth, N, seed)
        print(f"{name}: loss f64 {out['loss_f64']:.6f} fp16 chain {out['loss_f16']:.6f}  |g| per layer "
              + " ".join(f"{float(out['g_f64'][i].norm()):.3e}" for i in range(depth)) + "  e_ref " + " ".join(f"{e:.3e}" for e in out["e_ref"])
              + f"  features e_ref {out['feat_e_ref']:.3e}")
        assert all(math.isfinite(e) and e > 0 for e in list(out["e_ref"]) + [out["feat_e_ref"]])
        mg.savez(name, logit_scale=float(np.float32(vpt_ref.LOGIT_SCALE)), floor=FLOOR, e_ref_source="reference fp16 chain on the CPU", tag=tag,
                 sd_seed=sd_seed, B=B, P=P, depth=depth, N=N, seed=seed, **out)


if __name__ == "__main__":
    main()
