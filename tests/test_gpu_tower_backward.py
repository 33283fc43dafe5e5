"""Fine-tuning the transformer towers (autograd.TowerTailFn behind CLIP.encode_image / encode_text): parameter gradients against the reference's own
float64 autograd (fixtures of tests/golden/make_golden_tower_grad.py), graded per tensor at twice the reference's own fp16-chain distance e_ref, and the
behaviour of the public surface: where gradients land, that the taped forward keeps the untaped bits, that the frozen default builds no tape, that
training lowers the loss, that a scaled loss scales the gradients, and the refusals."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, observe
from spec import ODD, RESNET, SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

FIXTURES = {"tiny": TINY, "small": SMALL}
VITB16_2L = dict(embed_dim=512, image_resolution=224, vision_layers=2, vision_width=768, vision_patch_size=16, context_length=77, vocab_size=512,
                 transformer_width=128, transformer_heads=2, transformer_layers=1)                       # 12 heads, L = 197
L257 = dict(embed_dim=64, image_resolution=224, vision_layers=2, vision_width=128, vision_patch_size=14, context_length=77, vocab_size=300,
            transformer_width=64, transformer_heads=1, transformer_layers=1)                             # ViT-L/14's sequence: L = 257
L577 = dict(L257, image_resolution=336, vision_layers=1)                                                 # ViT-L/14@336px's: L = 577


def tokens(n, vocab, seed):
    """SOT, a random body, EOT (the highest id: the argmax the towers gather at), zero padding."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(n, 77, dtype=torch.long)
    for i in range(n):
        ln = int(torch.randint(3, 23, (1,), generator=g))
        t[i, 0] = vocab - 2
        t[i, 1:ln] = torch.randint(1, vocab - 2, (ln - 1,), generator=g)
        t[i, ln] = vocab - 1
    return t


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(math.log(20.0), dtype=torch.float32)
    return build_model(sd).cuda()


def load_fixture(tag, nb):
    paths = sorted(glob.glob(os.path.join(GOLDEN, f"tower_grad_{tag}_b{nb}_p*.npz")))
    if not paths:
        pytest.skip(f"fixture tower_grad_{tag}_b{nb} not generated")
    parts = [np.load(p, allow_pickle=False) for p in paths]
    meta = parts[0]
    assert int(meta["n_parts"]) == len(parts)
    grads = {k[3:]: torch.from_numpy(part[k]) for part in parts for k in part.files if k.startswith("g__")}
    return meta, grads


def contrastive64(fi, ft, logit_scale):
    """The generator's loss: float64 torch on the features."""
    fi, ft = fi.double(), ft.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    logits = math.exp(float(np.float32(logit_scale))) * fi @ ft.t()
    tgt = torch.arange(fi.shape[0], device=fi.device)
    ce = torch.nn.functional.cross_entropy
    return 0.5 * (ce(logits, tgt) + ce(logits.t(), tgt))


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("tag,nb", [("tiny", 1), ("tiny", 2), ("small", 1)])
def test_parameter_gradients_against_the_reference(tag, nb, loss_scale):
    """Per parameter tensor ||g - g_f64|| / ||g_f64|| <= 2 e_ref (e_ref: the reference's own fp16 chain against its float64 run; no floor, see the generator).
    With the loss scaled by 1024 the gradients, divided by 1024, meet the same bound: the fp16 stream neither overflows nor gains from the scaling."""
    from proto_clip_amd import synth
    from proto_clip_amd.clip.model import build_model, random_state_dict
    meta, g64 = load_fixture(tag, nb)
    kw, sd_seed, n = FIXTURES[tag], int(meta["sd_seed"]), int(meta["n"])
    assert float(meta["floor"]) == 0.0
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(float(meta["logit_scale"]), dtype=torch.float32)
    model = build_model(sd).cuda()
    imgs = synth.make_images(n, kw["image_resolution"], seed=int(meta["image_seed"]), n_class=n).cuda()
    toks = torch.from_numpy(meta["tokens"]).cuda()
    params = model.unfreeze(visual_blocks=nb, text_blocks=nb)
    loss = contrastive64(model.encode_image(imgs), model.encode_text(toks), float(meta["logit_scale"]))
    assert abs(float(loss.detach()) - float(meta["loss_f64"])) <= 2 * abs(float(meta["loss_f16"]) - float(meta["loss_f64"])) + 1e-4
    (loss * loss_scale).backward()
    named = {name: p for name, p in model.named_parameters() if p.requires_grad}
    assert sorted(named) == sorted(g64) == sorted(str(s) for s in meta["names"]) and len(params) == len(named)
    e_ref = {str(k): float(e) for k, e in zip(meta["names"], meta["e_ref"])}
    worst = 0.0
    for name in sorted(named):
        g = named[name].grad.double().cpu() / loss_scale
        want = g64[name].double()
        rel = float((g - want).norm() / want.norm())
        ratio = rel / (2 * e_ref[name])
        print(f"{tag} b{nb} x{loss_scale:g} {name:<58s} rel {rel:.3e}  e_ref {e_ref[name]:.3e}  ratio {ratio:.3f}")
        worst = max(worst, ratio)
        observe(f"tower backward {tag} b{nb} x{loss_scale:g}: worst ||g - g64|| / ||g64|| / (2 e_ref)", ratio, 1.0)
    assert worst <= 1.0, worst


def test_gradients_land_on_the_unfrozen_parameters():
    from proto_clip_amd import synth
    model = make_model(SMALL, 5)
    imgs = synth.make_images(6, SMALL["image_resolution"], seed=3, n_class=6).cuda()
    toks = tokens(6, SMALL["vocab_size"], 4).cuda()
    params = model.unfreeze(visual_blocks=1, text_blocks=2)
    want = {n for n, _ in model.named_parameters() if n.startswith(("visual.transformer.resblocks.2.", "transformer.resblocks.1.", "transformer.resblocks.2.",
                                                                      "visual.ln_post.", "ln_final.")) or n in ("visual.proj", "text_projection")}
    assert {n for n, p in model.named_parameters() if p.requires_grad} == want and len(params) == len(want)
    fi, ft = model.encode_image(imgs), model.encode_text(toks)
    assert fi.requires_grad and ft.requires_grad and fi.dtype == ft.dtype == torch.float16
    model.contrastive_loss(fi, ft).backward()
    for name, p in model.named_parameters():
        if name in want:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, name
            assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
            assert p.dtype == (torch.float32 if ".ln_" in name or name.startswith("ln_") else torch.float16), name
        else:
            assert p.grad is None, name


BIT_CASES = {"tiny": (TINY, 4), "small": (SMALL, 4), "odd": (ODD, 3), "vitb16_2l": (VITB16_2L, 2), "l257": (L257, 2)}


@pytest.mark.parametrize("tag", list(BIT_CASES))
def test_taped_features_keep_the_untaped_bits(tag):
    from proto_clip_amd import synth
    kw, n = BIT_CASES[tag]
    model = make_model(kw, 9)
    imgs = synth.make_images(n, kw["image_resolution"], seed=6, n_class=n).cuda()
    toks = tokens(n, kw["vocab_size"], 7).cuda()
    with torch.no_grad():
        fi0, ft0 = model.encode_image(imgs), model.encode_text(toks)
    for vb, tb in ((0, 0), (1, 1), (kw["vision_layers"], kw["transformer_layers"])):      # heads only; the last block; every block (the stem's fused ln_1 feeds the tape)
        for p in model.parameters():
            p.requires_grad_(False)
        model.unfreeze(visual_blocks=vb, text_blocks=tb)
        fi, ft = model.encode_image(imgs), model.encode_text(toks)
        assert fi.requires_grad and ft.requires_grad
        assert torch.equal(fi.detach(), fi0) and torch.equal(ft.detach(), ft0), (vb, tb)


def test_frozen_model_builds_no_tape():
    from proto_clip_amd import synth
    model = make_model(TINY, 5)
    imgs = synth.make_images(3, TINY["image_resolution"], seed=3, n_class=3).cuda()
    toks = tokens(3, TINY["vocab_size"], 4).cuda()
    assert not any(p.requires_grad for p in model.parameters())
    fi, ft = model.encode_image(imgs), model.encode_text(toks)                             # grad mode on, everything frozen
    assert not fi.requires_grad and not ft.requires_grad and fi.grad_fn is None and ft.grad_fn is None
    model.unfreeze(visual_blocks=1, text_blocks=1)
    with torch.no_grad():
        gi, gt = model.encode_image(imgs), model.encode_text(toks)
    assert not gi.requires_grad and not gt.requires_grad and gi.grad_fn is None and gt.grad_fn is None
    assert torch.equal(gi, fi) and torch.equal(gt, ft)
    li, lt = model(imgs, toks)                                                             # CLIP.forward stays a constant
    assert not li.requires_grad and not lt.requires_grad


def test_sgd_on_the_unfrozen_tail_lowers_the_loss():
    from proto_clip_amd import synth
    model = make_model(SMALL, 6)
    imgs = synth.make_images(8, SMALL["image_resolution"], seed=8, n_class=8).cuda()
    toks = tokens(8, SMALL["vocab_size"], 9).cuda()
    opt = torch.optim.SGD(model.unfreeze(visual_blocks=1, text_blocks=1), lr=0.3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))))
    print("contrastive loss over five SGD steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_refusals_name_the_parameter_or_the_shape():
    from proto_clip_amd import ops, synth
    from proto_clip_amd._lib import PclipError
    model = make_model(TINY, 5)
    imgs = synth.make_images(2, TINY["image_resolution"], seed=3, n_class=2).cuda()
    toks = tokens(2, TINY["vocab_size"], 4).cuda()
    # a trainable parameter in the frozen prefix of either tower
    model.visual.conv1.weight.requires_grad_(True)
    with pytest.raises(PclipError, match=r"visual\.conv1\.weight"):
        model.encode_image(imgs)
    model.visual.conv1.weight.requires_grad_(False)
    model.positional_embedding.requires_grad_(True)
    with pytest.raises(PclipError, match="positional_embedding"):
        model.encode_text(toks)
    model.positional_embedding.requires_grad_(False)
    # a taped pass inside ops.low_latency()
    model.unfreeze(visual_blocks=1, text_blocks=1)
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            model.encode_image(imgs)
        with pytest.raises(PclipError, match="low_latency"):
            model.encode_text(toks)
    # the ModifiedResNet towers have no backward
    rn = make_model(RESNET, 5, trained=False)
    rn.visual.attnpool.c_proj.weight.requires_grad_(True)
    with pytest.raises(PclipError, match=r"attnpool\.c_proj\.weight"):
        rn.encode_image(synth.make_images(2, RESNET["image_resolution"], seed=3, n_class=2).cuda())
    with pytest.raises(PclipError, match="ModifiedResNet"):
        rn.unfreeze(visual_blocks=1)
    # sequences beyond the attention backward's envelope
    long = make_model(L577, 5, trained=False)
    long.unfreeze(visual_blocks=1, text_blocks=0)
    with pytest.raises(PclipError, match="L=577"):
        long.encode_image(synth.make_images(1, 336, seed=3, n_class=1).cuda())
