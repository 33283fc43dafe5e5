#!/usr/bin/env python3
"""Generates tests/golden/encoder_vitl14_336.npz by RUNNING THE REFERENCE ITSELF, through make_golden.py's import shim:
the reference's own build_model / encode_image (clip/model.py:221-238, 338-339, 397-434) at the architecture it infers from
OpenAI's ViT-L-14-336px checkpoint (24 x 1024, patch 14, 336 px: 577 tokens), on seeded random-init weights and synthetic
images, with fp16 weights (its GPU-path precision) and as the fp32 model clip.load(device='cpu') yields.  Outputs only; the
weight seed and image count are stored beside them, and the tests regenerate the inputs.

    python tests/golden/make_golden_long.py
"""
import contextlib
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (sets up the repository path and the shim)
from proto_clip_amd import synth                                   # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, random_state_dict  # noqa: E402

BACKBONE, SD_SEED, N_IMG = "ViT-L/14@336px", 16, 2


def main():
    ref_clip_model = mg.import_reference()[4]
    kw = BACKBONES[BACKBONE]
    sd = random_state_dict(seed=SD_SEED, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        m16 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
        m32 = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()}).float()
    assert m16.visual.input_resolution == 336 and m16.visual.positional_embedding.shape[0] == 577
    imgs = synth.make_images(N_IMG, kw["image_resolution"], seed=5, n_class=6)
    with torch.no_grad():
        f32 = m32.encode_image(imgs)
        f16 = m16.encode_image(imgs)
    mg.savez("encoder_vitl14_336", img_f16=f16, img_f32=f32, sd_seed=SD_SEED, n_img=N_IMG, image_seed=5)


if __name__ == "__main__":
    main()
