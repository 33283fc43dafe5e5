#!/usr/bin/env python3
"""Generates tests/golden/tower_grad_<tag>_b<n>_p<k>.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's import shim:
the reference's own `build_model(...)`, its `encode_image` / `encode_text` (plain differentiable modules, clip/model.py:338-354) on seeded towers
(spec.TINY / spec.SMALL, random_state_dict + trained_like_), a fixed scalar loss, and `loss.backward()` with the last n residual blocks of both
towers plus ln_post / proj / ln_final / text_projection trainable.

    python tests/golden/make_golden_tower_grad.py

The loss is CLIP's symmetric contrastive loss, evaluated in float64 torch on the features (cast to float64): both sides L2-normalised,
logits = exp(logit_scale) * img @ txt.T, loss = (CE(logits, arange) + CE(logits.T, arange)) / 2.  This file holds no reference code, only calls
into it; the one intervention is that the float64 run replaces the forward of the reference's LayerNorm subclass (which casts its input to fp32
whatever the module's precision) by the plain torch.nn.LayerNorm forward, so that the float64 run is float64 throughout.

Two runs per case:
  f64      the reference model `.double()` — weights are the fp16 values exactly — giving the gradients every implementation is graded against;
  fp16     the reference's own fp16 chain on the CPU (fp16 linears and attention, fp32 LayerNorms, fp16 gradients for the fp16 parameters), giving
           e_ref = ||g_fp16chain - g_f64||_2 / ||g_f64||_2 per parameter tensor: the reference's own distance from float64 in the precision it runs in.
tests/test_gpu_tower_backward.py asks ||g_ours - g_f64||_2 / ||g_f64||_2 <= 2 e_ref of every tensor.

Floor.  A tensor's e_ref cannot be resolved below the fp32 storage of g_f64 and the fp32 summations of this implementation's fp32-typed gradients (the
LayerNorm affines: sums over R = B * L rows in fp32, unit 2^-24, worst-case growth R 2^-24 relative to sum |terms|).  The generator prints every e_ref;
all of them come out between 3.6e-3 and 5.0e-2 (the gradient stream of a mean loss over a handful of rows sits at 1e-6 .. 1e-3 per element, partly in
fp16's subnormal range, where a rounding costs 2^-25 absolute), two orders above R 2^-24 (R <= 616 rows: 4e-5 worst case, ~ sqrt(R) 2^-24 = 1.5e-6 typical).  The test therefore applies NO floor; FLOOR below is recorded in the fixture as 0.

Files.  No committed file may exceed 1 MiB, and one residual block of the SMALL vision tower alone has 3 MB of fp32 gradients, so a case is
written as numbered parts (tensors packed greedily, 900 KiB of raw data per part; part 0 carries the seeds, tokens, losses and the e_ref table).
SMALL is generated for the last block only (two blocks would add 4 MB more)."""
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
from proto_clip_amd import synth                                   # noqa: E402
from proto_clip_amd.clip.model import random_state_dict            # noqa: E402
from spec import SMALL, TINY, trained_like_                         # noqa: E402

# tag -> (tower, weight seed, batch (images = prompts), image seed, token seed, logit_scale, block counts)
CASES = {"tiny": (TINY, 71, 6, 19, 27, math.log(20.0), (1, 2)),
         "small": (SMALL, 72, 8, 20, 28, math.log(20.0), (1,))}
FLOOR = 0.0
PART_BYTES = 900 * 1024


def trainable(model, n_blocks):
    """(name, parameter) of the last n_blocks residual blocks of both towers and the heads, after freezing everything else."""
    for p in model.parameters():
        p.requires_grad_(False)
    nv, nt = len(model.visual.transformer.resblocks), len(model.transformer.resblocks)
    names = []
    for name, p in model.named_parameters():
        parts = name.split(".")
        on = name in ("visual.proj", "text_projection") or name.startswith(("visual.ln_post.", "ln_final."))
        if name.startswith("visual.transformer.resblocks."):
            on = int(parts[3]) >= nv - n_blocks
        elif name.startswith("transformer.resblocks."):
            on = int(parts[2]) >= nt - n_blocks
        if on:
            p.requires_grad_(True)
            names.append((name, p))
    return names


def contrastive64(fi, ft, logit_scale):
    fi, ft = fi.double(), ft.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    logits = math.exp(float(np.float32(logit_scale))) * fi @ ft.t()
    tgt = torch.arange(fi.shape[0])
    ce = torch.nn.functional.cross_entropy
    return 0.5 * (ce(logits, tgt) + ce(logits.t(), tgt))


def grads(model, n_blocks, imgs, toks, logit_scale):
    named = trainable(model, n_blocks)
    loss = contrastive64(model.encode_image(imgs), model.encode_text(toks), logit_scale)
    loss.backward()
    out = {name: p.grad.detach().double().clone() for name, p in named}
    for _, p in named:
        p.grad = None
    return float(loss.detach()), out


def run(ref_clip_model, kw, sd_seed, n, image_seed, token_seed, logit_scale, n_blocks):
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(logit_scale, dtype=torch.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        m16 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
        m64 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()}).double()
    imgs = synth.make_images(n, kw["image_resolution"], seed=image_seed, n_class=n)
    toks = mg.synth_tokens(n, kw["vocab_size"], seed=token_seed)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout (see the docstring)
    try:
        loss64, g64 = grads(m64, n_blocks, imgs.double(), toks, logit_scale)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    loss16, g16 = grads(m16, n_blocks, imgs, toks, logit_scale)
    e_ref = {k: float((g16[k] - g64[k]).norm() / g64[k].norm()) for k in g64}
    return imgs, toks, loss16, loss64, g64, e_ref


def main():
    ref_clip_model = mg.import_reference()[4]
    for tag, (kw, sd_seed, n, image_seed, token_seed, logit_scale, block_counts) in CASES.items():
        for nb in block_counts:
            imgs, toks, loss16, loss64, g64, e_ref = run(ref_clip_model, kw, sd_seed, n, image_seed, token_seed, logit_scale, nb)
            names = sorted(g64)
            print(f"{tag} b{nb}: loss f64 {loss64:.6f} fp16 chain {loss16:.6f}")
            for k in names:
                print(f"    {k:<60s} |g| {float(g64[k].norm()):.3e}  e_ref {e_ref[k]:.3e}")
            assert all(math.isfinite(e_ref[k]) and e_ref[k] > 0 for k in names)
            meta = dict(sd_seed=sd_seed, image_seed=image_seed, token_seed=token_seed, n=n, n_blocks=nb, logit_scale=float(np.float32(logit_scale)),
                        tokens=toks, loss_f64=loss64, loss_f16=loss16, names=np.array(names), e_ref=np.array([e_ref[k] for k in names]),
                        floor=FLOOR, e_ref_source="reference fp16 chain on the CPU")
            parts, cur, size = [], {}, 0
            for k in names:
                nbytes = g64[k].numel() * 4
                if cur and size + nbytes > PART_BYTES:
                    parts.append(cur)
                    cur, size = {}, 0
                cur["g__" + k] = g64[k].float()
                size += nbytes
            parts.append(cur)
            meta["n_parts"] = len(parts)
            for i, part in enumerate(parts):
                mg.savez(f"tower_grad_{tag}_b{nb}_p{i}", **(dict(meta, **part) if i == 0 else part))


if __name__ == "__main__":
    main()
