#!/usr/bin/env python3
"""Generates tests/golden/cocoop_grad_<case>.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's import shim (the recipe of
make_golden_coop.py): the reference's own `build_model(...)` and `encode_text` on seeded towers (spec.TINY / spec.SMALL, random_state_dict +
trained_like_), with CoCoOp's per-image context put into the prompts by a forward hook on the reference's `token_embedding` that overwrites rows
1 .. n_ctx of its output by ctx + pi_b — where CoOp's fixture splices its context.  The B * N prompts are the N token rows repeated per image.  The meta-net
is stated in plain torch here: pi = relu(f @ W1.T + b1) @ W2.T + b2 on the L2-normalised image features f.  This file holds no reference code, only calls
into it.

    python tests/golden/make_golden_cocoop.py            # the fixtures
    python tests/golden/make_golden_cocoop.py sgd        # the five-step loss decrease tests/cocoop_ref.py quotes

The loss is the mean over the images of the float64 cross-entropy of scale * normalize(f_b) . normalize(text[b, :]) against seeded labels, on seeded image
features (fp16-exact values) and the text features cast to float64; scale = exp(float32(log 20)).

Two runs per case:
  f64      the reference model `.double()` with the float64 LayerNorm swap (see make_golden_tower_grad.py), float64 context and meta-net: `g_<name>_f64` for
           the five tensors (ctx, w1, b1, w2, b2), `text_f64` and `loss_f64`;
  fp16     the reference's own fp16 chain on the CPU with the fp32 parameters cast to fp16 where they are used (the meta-net runs in fp16, as upstream's
           does): `loss_f16`, e_ref_<name> = ||g_fp16chain - g_f64||_2 / ||g_f64||_2 per tensor and `text_e_ref`, the same relative distance over the features.
tests/test_gpu_cocoop.py asks ||g_ours - g_f64||_2 / ||g_f64||_2 <= 2 e_ref per tensor and the same of the features, with no floor (recorded as 0).

The ReLU condition, asserted here: the smallest |pre-activation| of the float64 run is at least 16 times the largest |pre-activation difference| between
the fp16-chain run and the float64 run, so every chain agrees on the mask; both numbers are stored (`relu_min_pre`, `relu_max_diff`).

The parameters, the tokens, the features and the labels are regenerated in the test from the seeds stored here (tests/cocoop_ref.py: fixture_inputs)."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
sys.path.insert(0, os.path.dirname(HERE))
import cocoop_ref                                                   # noqa: E402  (the cases and the seeded inputs, shared with tests/test_gpu_cocoop.py)
from make_golden_vpt import models                                  # noqa: E402  (the seeded reference models)

FLOOR = 0.0
NAMES = ("ctx", "w1", "b1", "w2", "b2")


def text_features(model, params, tokens, feats, dtype):
    """(text [B, N, E], pre [B, Hd]) through the reference's encode_text with ctx + pi_b written over rows 1 .. n_ctx of image b's N prompts."""
    ctx, w1, b1, w2, b2 = (p.to(dtype) for p in params)
    B, N, n_ctx = feats.shape[0], tokens.shape[0], ctx.shape[0]
    f = feats.double() if dtype == torch.float64 else feats.float()
    f = (f / f.norm(dim=1, keepdim=True)).to(dtype)
    pre = torch.nn.functional.linear(f, w1, b1)
    pi = torch.nn.functional.linear(torch.relu(pre), w2, b2)
    rows = (ctx[None] + pi[:, None, :]).repeat_interleave(N, dim=0)                # [B * N, n_ctx, W]

    def splice(_module, _args, out):
        out = out.clone()
        out[:, 1:1 + n_ctx] = rows.to(out.dtype)
        return out

    handle = model.token_embedding.register_forward_hook(splice)
    try:
        text = model.encode_text(tokens.repeat(B, 1))
    finally:
        handle.remove()
    return text.reshape(B, N, -1), pre


def grad(model, params, tokens, feats, labels, dtype):
    params = [p.clone().requires_grad_(True) for p in params]
    text, pre = text_features(model, params, tokens, feats, dtype)
    loss = cocoop_ref.loss64(feats, text, labels)
    loss.backward()
    return float(loss.detach()), [p.grad.detach().double().clone() for p in params], text.detach().double().clone(), pre.detach().double().clone()


def run(ref_clip_model, kw, sd_seed, B, N, n_ctx, seed, l_eff):
    m16, m64 = models(ref_clip_model, kw, sd_seed, (torch.float16, torch.float64))
    *params, tokens, feats, labels = cocoop_ref.fixture_inputs(kw, B, N, n_ctx, seed, l_eff)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        l64, g64, t64, p64 = grad(m64, [p.double() for p in params], tokens, feats, labels, torch.float64)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    l16, g16, t16, p16 = grad(m16, params, tokens, feats, labels, torch.float16)
    out = dict(loss_f16=l16, loss_f64=l64, text_f64=t64.float(), text_e_ref=float((t16 - t64).norm() / t64.norm()),
               relu_min_pre=float(p64.abs().min()), relu_max_diff=float((p16 - p64).abs().max()))
    for name, a, b in zip(NAMES, g16, g64):
        out[f"g_{name}_f64"] = b.float()
        out[f"e_ref_{name}"] = float((a - b).norm() / b.norm())
    return out


def sgd_decrease(ref_clip_model):
    """The loss decrease of five SGD steps on the reference's fp32 CPU chain, the case and the step rule of test_five_sgd_steps_of_run_cocoop_lower_the_loss
    (run_cocoop: SGD on the five tensors, momentum 0.9, cosine schedule over the five steps, one batch of all images)."""
    tag, sd_seed, B, N, n_ctx, seed, lr = cocoop_ref.SGD_CASE
    kw = cocoop_ref.towers()[tag]
    (m32,) = models(ref_clip_model, kw, sd_seed, (torch.float32,))
    *params, tokens, feats, labels = cocoop_ref.fixture_inputs(kw, B, N, n_ctx, seed)
    params = [p.clone().requires_grad_(True) for p in params]
    opt = torch.optim.SGD(params, lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 5)
    losses = []
    for _ in range(5):
        loss = cocoop_ref.loss64(feats, text_features(m32, params, tokens, feats, torch.float32)[0], labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(cocoop_ref.loss64(feats, text_features(m32, params, tokens, feats, torch.float32)[0], labels)))
    print("reference fp32 chain, five SGD steps (lr %g):" % lr, " ".join(f"{v:.6f}" for v in losses), " decrease %.6f" % (losses[0] - losses[-1]))


def main():
    ref_clip_model = mg.import_reference()[4]
    if sys.argv[1:] == ["sgd"]:
        return sgd_decrease(ref_clip_model)
    for name, (tag, sd_seed, B, N, n_ctx, seed, l_eff) in cocoop_ref.FIXTURES.items():
        out = run(ref_clip_model, cocoop_ref.towers()[tag], sd_seed, B, N, n_ctx, seed, l_eff)
        e_refs = [out[f"e_ref_{k}"] for k in NAMES] + [out["text_e_ref"]]
        print(f"{name}: loss f64 {out['loss_f64']:.6f} fp16 chain {out['loss_f16']:.6f}  e_ref " + "  ".join(f"{k} {out[f'e_ref_{k}']:.3e}" for k in NAMES)
              + f"  features e_ref {out['text_e_ref']:.3e}  relu: min |pre| {out['relu_min_pre']:.3e}, max |diff| {out['relu_max_diff']:.3e}")
        assert all(math.isfinite(e) and e > 0 for e in e_refs)
        assert out["relu_min_pre"] >= cocoop_ref.RELU_MARGIN * out["relu_max_diff"], (name, "the ReLU condition fails for this seed: pick another")
        mg.savez(name, logit_scale=float(np.float32(cocoop_ref.LOGIT_SCALE)), floor=FLOOR, e_ref_source="reference fp16 chain on the CPU", tag=tag,
                 sd_seed=sd_seed, B=B, N=N, n_ctx=n_ctx, seed=seed, l_eff=0 if l_eff is None else l_eff, **out)


if __name__ == "__main__":
    main()
