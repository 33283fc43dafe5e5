#!/usr/bin/env python3
"""Generates tests/golden/contrastive_tiny.npz and contrastive_small.npz by RUNNING THE REFERENCE ITSELF, through make_golden.py's
import shim: the reference's own `build_model(...)(images, tokens)` (CLIP.forward, clip/model.py:356-370) on two seeded random towers
with fp16 weights (its GPU-path precision, here on the CPU) and again as `.float()`.  Outputs only: the logits of both precisions, the
fp16 encode_image / encode_text features, the token ids and the seeds; the tests regenerate weights and images from the seeds.

    python tests/golden/make_golden_contrastive.py [--scan]

The towers are defined here (spec.py's TINY / SMALL hyper-parameters; LayerNorm affines and outlier channels of a trained model through
spec.trained_like_, so that the prompts do not all land on one direction); `logit_scale` is the drawn ln(1 / 0.07) for the tiny tower
and ln 100 for the small one.  A fixture is only written if at least 3/4 of its rows are DECIDED — reference top-2 margin above
2 * tol with tol = 2 * max|logits_f16 - logits_f32| — which is what tests/test_gpu_contrastive.py grades the top-1 on.
"""
import contextlib
import io
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
from proto_clip_amd import synth                                   # noqa: E402
from proto_clip_amd.clip.model import random_state_dict            # noqa: E402
from spec import SMALL, TINY, trained_like_                         # noqa: E402

# tag -> (tower, weight seed, images, prompts, image seed, token seed, logit_scale or None = as drawn)
CASES = {"tiny": (TINY, 61, 5, 3, 9, 17, None),
         "small": (SMALL, 62, 9, 17, 10, 18, math.log(100.0))}


def state_dict(kw, sd_seed, logit_scale):
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    if logit_scale is not None:
        sd["logit_scale"] = torch.tensor(logit_scale, dtype=torch.float32)
    return sd


def run(ref_clip_model, kw, sd_seed, n_img, n_txt, image_seed, token_seed, logit_scale):
    sd = state_dict(kw, sd_seed, logit_scale)
    with contextlib.redirect_stdout(io.StringIO()):
        m16 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
        m32 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()}).float()
    imgs = synth.make_images(n_img, kw["image_resolution"], seed=image_seed, n_class=n_img)
    toks = mg.synth_tokens(n_txt, kw["vocab_size"], seed=token_seed)
    with torch.no_grad():
        l16, lt16 = m16(imgs, toks)
        l32, _ = m32(imgs, toks)
        f16, t16 = m16.encode_image(imgs), m16.encode_text(toks)
    assert l16.dtype == torch.float16 and torch.equal(lt16, l16.t())
    tol = 2 * (l16.float() - l32).abs().max().item()
    top2 = l32.topk(min(2, n_txt), dim=1).values
    decided = ((top2[:, 0] - top2[:, 1]) > 2 * tol).float().mean().item()
    return dict(logits_f16=l16, logits_f32=l32, img_f16=f16, txt_f16=t16, tokens=toks, sd_seed=sd_seed, image_seed=image_seed, token_seed=token_seed,
                n_img=n_img, n_txt=n_txt, logit_scale=float(sd["logit_scale"])), tol, decided


def main():
    ref_clip_model = mg.import_reference()[4]
    for tag, (kw, sd_seed, n_img, n_txt, image_seed, token_seed, logit_scale) in CASES.items():
        if "--scan" in sys.argv:                                    # choosing seeds: print the decided share of a few
            for s in range(sd_seed, sd_seed + 40, 2):
                _, tol, decided = run(ref_clip_model, kw, s, n_img, n_txt, image_seed, token_seed, logit_scale)
                print(f"{tag}: sd_seed {s}: tol {tol:.4f}, decided {decided:.2f}")
            continue
        out, tol, decided = run(ref_clip_model, kw, sd_seed, n_img, n_txt, image_seed, token_seed, logit_scale)
        print(f"{tag}: tol {tol:.4f}, decided rows {decided:.2f}, logits in [{out['logits_f32'].min():.2f}, {out['logits_f32'].max():.2f}]")
        assert decided >= 0.75, f"{tag}: only {decided:.2f} of the rows are decided: choose other seeds"
        mg.savez("contrastive_" + tag, **out)


if __name__ == "__main__":
    main()
