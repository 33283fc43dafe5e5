#!/usr/bin/env python3
"""Generates tests/golden/coop_grad_<tag>_<shared|specific>.npz by RUNNING THE REFERENCE ITSELF under autograd, through make_golden.py's import shim
(the recipe of make_golden_tower_grad.py): the reference's own `build_model(...)` and `encode_text` on seeded towers (spec.TINY / spec.SMALL,
random_state_dict + trained_like_), with learned context rows put into the prompt by a forward hook on the reference's `token_embedding` that overwrites
rows 1 .. n_ctx of its output — where CoOp concatenates its context.  This file holds no reference code, only calls into it.

    python tests/golden/make_golden_coop.py

The loss is the float64 cross-entropy of scale * normalize(img) @ normalize(text).T against seeded labels, on seeded image features (fp16-exact values)
and the text features cast to float64; scale = exp(float32(log 20)).

Two runs per case:
  f64      the reference model `.double()` with the float64 LayerNorm swap (see make_golden_tower_grad.py) and a float64 context: `g_f64`, the gradient
           of the context every implementation is graded against, and `loss_f64`;
  fp16     the reference's own fp16 chain on the CPU with the fp32 context (cast to fp16 where `encode_text` casts the embeddings): `loss_f16` and
           e_ref = ||g_fp16chain - g_f64||_2 / ||g_f64||_2, the reference's own distance from float64 in the precision it runs in.
tests/test_gpu_coop.py asks ||g_ours - g_f64||_2 / ||g_f64||_2 <= 2 e_ref, with no floor (recorded as 0).  The text features of both runs give
`text_f64` and `text_e_ref` (the same relative distance over the whole [N, E] matrix), graded by the same rule.

Besides the four gradient cases (TINY and SMALL, shared and class-specific context) there is one case per prompt length in LENGTHS: prompts whose largest
EOT position + 1 is that length, for the test that runs the tower truncated to it.

The context (N(0, 0.02) rows), the image features and the labels are regenerated in the test from the seeds stored here (tests/coop_ref.py: fixture_inputs is the shared
definition); the tokens are stored."""
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
from spec import SMALL, TINY, trained_like_                         # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
from coop_ref import fixture_inputs as inputs                       # noqa: E402  (the seeded inputs, shared with tests/test_gpu_coop.py)

# tag -> (tower, weight seed, N, n_ctx, Q, input seed)
CASES = {"tiny": (TINY, 81, 6, 4, 12, 41),
         "small": (SMALL, 82, 10, 16, 24, 42)}
# prompts of a given L_eff = (largest EOT position) + 1, on either side of the attention's 32-key tiles and at the full context: coop_grad_small_len<L>.npz
# (SMALL, shared context, N = 5, n_ctx = 2, Q = 10)
LENGTHS = (6, 32, 33, 65, 77)
LENGTH_CASE = (SMALL, 83, 5, 2, 10, 43)
LOGIT_SCALE = math.log(20.0)
FLOOR = 0.0


def loss64(feats, text, labels):
    fi, ft = feats.double(), text.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    return torch.nn.functional.cross_entropy(math.exp(float(np.float32(LOGIT_SCALE))) * fi @ ft.t(), labels)


def grad(model, ctx, tokens, feats, labels, n_ctx):
    """(loss, d loss / d ctx, text features) through the reference's encode_text with `ctx` written over rows 1 .. n_ctx of the token embeddings."""
    ctx = ctx.clone().requires_grad_(True)

    def splice(_module, _args, out):
        out = out.clone()
        out[:, 1:1 + n_ctx] = ctx.to(out.dtype)
        return out

    handle = model.token_embedding.register_forward_hook(splice)
    try:
        text = model.encode_text(tokens)
        loss = loss64(feats, text, labels)
        loss.backward()
    finally:
        handle.remove()
    return float(loss.detach()), ctx.grad.detach().double().clone(), text.detach().double().clone()


def run(ref_clip_model, kw, sd_seed, N, n_ctx, Q, seed, class_specific, l_eff=None):
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(LOGIT_SCALE, dtype=torch.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        m16 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
        m64 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()}).double()
    for m in (m16, m64):
        for p in m.parameters():
            p.requires_grad_(False)
    ctx, tokens, feats, labels = inputs(kw, N, n_ctx, Q, seed, class_specific, l_eff)
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        l64, g64, t64 = grad(m64, ctx.double(), tokens, feats, labels, n_ctx)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    l16, g16, t16 = grad(m16, ctx, tokens, feats, labels, n_ctx)
    return dict(tokens=tokens, loss_f16=l16, loss_f64=l64, g_f64=g64.float(), e_ref=float((g16 - g64).norm() / g64.norm()),
                text_f64=t64.float(), text_e_ref=float((t16 - t64).norm() / t64.norm()))


def write(name, out, **meta):
    print(f"{name}: loss f64 {out['loss_f64']:.6f} fp16 chain {out['loss_f16']:.6f}  |g| {float(out['g_f64'].norm()):.3e}  e_ref {out['e_ref']:.3e}"
          f"  features e_ref {out['text_e_ref']:.3e}")
    assert all(math.isfinite(out[k]) and out[k] > 0 for k in ("e_ref", "text_e_ref"))
    mg.savez(name, logit_scale=float(np.float32(LOGIT_SCALE)), floor=FLOOR, e_ref_source="reference fp16 chain on the CPU", **meta, **out)


def main():
    ref_clip_model = mg.import_reference()[4]
    for tag, (kw, sd_seed, N, n_ctx, Q, seed) in CASES.items():
        for class_specific in (False, True):
            out = run(ref_clip_model, kw, sd_seed, N, n_ctx, Q, seed, class_specific)
            write(f"coop_grad_{tag}_{'specific' if class_specific else 'shared'}", out, tag=tag, sd_seed=sd_seed, N=N, n_ctx=n_ctx, Q=Q, seed=seed,
                  class_specific=class_specific, l_eff=0)
    kw, sd_seed, N, n_ctx, Q, seed = LENGTH_CASE
    for l_eff in LENGTHS:
        out = run(ref_clip_model, kw, sd_seed, N, n_ctx, Q, seed, False, l_eff)
        write(f"coop_grad_small_len{l_eff}", out, tag="small", sd_seed=sd_seed, N=N, n_ctx=n_ctx, Q=Q, seed=seed, class_specific=False, l_eff=l_eff)


if __name__ == "__main__":
    main()
