#!/usr/bin/env python3
"""Generates tests/golden/tower_prefix_grad_<tag>_p<k>.npz by RUNNING THE REFERENCE ITSELF under autograd with EVERYTHING of both towers trainable — the
patch convolution, the class / positional / token embeddings and ln_pre included — through make_golden.py's import shim, exactly as
make_golden_tower_grad.py does for a tail of blocks: the reference's own `build_model(...)`, its `encode_image` / `encode_text` on seeded towers
(spec.TINY / spec.SMALL / spec.ODD, random_state_dict + trained_like_), CLIP's symmetric contrastive loss in float64 torch on the features, and
`loss.backward()`.  Only logit_scale stays frozen (the loss takes it as a constant).

    python tests/golden/make_golden_prefix_grad.py

This file holds no reference code, only calls into it; the one intervention is make_golden_tower_grad.py's: the float64 run replaces the forward of the
reference's LayerNorm subclass (which casts its input to fp32 whatever the module's precision) by the plain torch.nn.LayerNorm forward, so that the
float64 run is float64 throughout.

Two runs per case, as there: f64 (the reference model `.double()`: the gradients every implementation is graded against) and the reference's own fp16
chain on the CPU, giving e_ref = ||g_fp16chain - g_f64||_2 / ||g_f64||_2 per parameter tensor.  tests/test_gpu_tower_prefix.py asks
||g_ours - g_f64||_2 / ||g_f64||_2 <= 2 e_ref of every tensor: the prefix parameters, and the blocks and heads of the same run.

token_embedding.weight: only the rows whose id occurs in the prompts are stored (`rows__token_embedding.weight` holds the ids); every other row of the
gradient is exactly zero in both runs, so e_ref over the stored rows is e_ref over the tensor.

Floor.  This implementation sums its fp32-typed gradients over R rows in fp32 (LayerNorm affines and the positional tables: R <= n * L rows; a token
embedding row: as many rows as the id occurs), worst case R 2^-24 relative to sum |terms|.  The generator prints every e_ref and that floor and asserts
that every e_ref is finite and positive.  Case that occurred (printed values): the floors are 2.75e-5 (tiny, 462 rows), 3.67e-5 (small, 616 rows)
and 2.29e-5 (odd, 385 rows); e_ref spans [2.54e-3, 3.03e-2] (tiny), [7.94e-3, 1.29e-1] (small) and [3.89e-3, 1.73e-2] (odd), its smallest value (2.54e-3,
visual.class_embedding of `tiny`) a factor 90 above the floor.  NO e_ref falls under the floor: `floor` is recorded as 0 and the test applies none.
e_ref of the prefix parameters:
    tiny   conv1 5.19e-3  class 2.54e-3  vis pos 2.78e-3  ln_pre w 5.32e-3  b 2.99e-3  token_embedding 3.64e-3  pos 3.83e-3
    small  conv1 1.08e-2  class 1.05e-2  vis pos 1.06e-2  ln_pre w 1.17e-2  b 1.47e-2  token_embedding 1.00e-2  pos 9.08e-3
    odd    conv1 4.67e-3  class 5.79e-3  vis pos 5.69e-3  ln_pre w 4.60e-3  b 7.00e-3  token_embedding 5.70e-3  pos 6.07e-3

Files.  No committed file may exceed 1 MiB: a case is written as numbered parts (tensors packed greedily, 900 KiB of raw fp32 data per part, a tensor
larger than that cut into row slabs `g__<name>__s<i>`; part 0 carries the seeds, tokens, losses and the e_ref table)."""
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
from make_golden_tower_grad import contrastive64                    # noqa: E402
from proto_clip_amd import synth                                   # noqa: E402
from proto_clip_amd.clip.model import random_state_dict            # noqa: E402
from spec import ODD, SMALL, TINY, trained_like_                    # noqa: E402

# tag -> (tower, weight seed, batch (images = prompts), image seed, token seed, logit_scale)
CASES = {"tiny": (TINY, 81, 6, 29, 37, math.log(20.0)),
         "small": (SMALL, 82, 8, 30, 38, math.log(20.0)),
         "odd": (ODD, 83, 5, 31, 39, math.log(20.0))}
PART_BYTES = 900 * 1024
TOKEN_EMBEDDING = "token_embedding.weight"


def grads(model, imgs, toks, logit_scale):
    named = [(n, p) for n, p in model.named_parameters() if n != "logit_scale"]
    for n, p in model.named_parameters():
        p.requires_grad_(n != "logit_scale")
    loss = contrastive64(model.encode_image(imgs), model.encode_text(toks), logit_scale)
    loss.backward()
    out = {name: p.grad.detach().double().clone() for name, p in named}
    for _, p in named:
        p.grad = None
    return float(loss.detach()), out


def run(ref_clip_model, kw, sd_seed, n, image_seed, token_seed, logit_scale):
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
        loss64, g64 = grads(m64, imgs.double(), toks, logit_scale)
    finally:
        ref_clip_model.LayerNorm.forward = keep
    loss16, g16 = grads(m16, imgs, toks, logit_scale)
    e_ref = {k: float((g16[k] - g64[k]).norm() / g64[k].norm()) for k in g64}
    return imgs, toks, loss16, loss64, g64, e_ref


def main():
    ref_clip_model = mg.import_reference()[4]
    for tag, (kw, sd_seed, n, image_seed, token_seed, logit_scale) in CASES.items():
        imgs, toks, loss16, loss64, g64, e_ref = run(ref_clip_model, kw, sd_seed, n, image_seed, token_seed, logit_scale)
        names = sorted(g64)
        L_vis = (kw["image_resolution"] // kw["vision_patch_size"]) ** 2 + 1
        floor_rows = n * max(77, L_vis)
        floor = floor_rows * 2.0 ** -24
        print(f"{tag}: loss f64 {loss64:.6f} fp16 chain {loss16:.6f}; fp32 summation floor {floor_rows} rows * 2^-24 = {floor:.2e}")
        for k in names:
            print(f"    {k:<60s} |g| {float(g64[k].norm()):.3e}  e_ref {e_ref[k]:.3e}")
        assert all(math.isfinite(e_ref[k]) and e_ref[k] > 0 for k in names)
        under = [k for k in names if e_ref[k] < floor]
        print(f"    e_ref in [{min(e_ref.values()):.3e}, {max(e_ref.values()):.3e}]; under the floor: {under or 'none'}")
        ids = torch.unique(toks)
        gE = g64[TOKEN_EMBEDDING]
        rest = torch.ones(gE.shape[0], dtype=torch.bool)
        rest[ids] = False
        assert not gE[rest].any()                                                # the rows that do not occur carry no gradient
        g64[TOKEN_EMBEDDING] = gE[ids]
        meta = dict(sd_seed=sd_seed, image_seed=image_seed, token_seed=token_seed, n=n, logit_scale=float(np.float32(logit_scale)), tokens=toks,
                    loss_f64=loss64, loss_f16=loss16, names=np.array(names), e_ref=np.array([e_ref[k] for k in names]),
                    floor=floor if under else 0.0, e_ref_source="reference fp16 chain on the CPU")
        meta["rows__" + TOKEN_EMBEDDING] = ids
        pieces = []
        for k in names:
            g = g64[k].float()
            if g.numel() * 4 <= PART_BYTES:
                pieces.append(("g__" + k, g))
                continue
            rows = max(1, PART_BYTES // (4 * g[0].numel()))
            pieces += [(f"g__{k}__s{i}", g[r:r + rows]) for i, r in enumerate(range(0, g.shape[0], rows))]
        parts, cur, size = [], {}, 0
        for key, g in pieces:
            nbytes = g.numel() * 4
            if cur and size + nbytes > PART_BYTES:
                parts.append(cur)
                cur, size = {}, 0
            cur[key] = g
            size += nbytes
        parts.append(cur)
        meta["n_parts"] = len(parts)
        for i, part in enumerate(parts):
            mg.savez(f"tower_prefix_grad_{tag}_p{i}", **(dict(meta, **part) if i == 0 else part))


if __name__ == "__main__":
    main()
