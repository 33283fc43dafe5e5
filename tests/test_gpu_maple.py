"""MaPLe on the GPU (proto_clip_amd.maple, autograd.CoupleFn / TowerTailFn with deep_off, csrc/pclip_maple.hip): the row kernels and the coupling function
bit for bit against the CPU emulations of their documented orders (tests/maple_ref.py) and inside the derived tolerances of float64, the learner against the
reference's own float64 autograd (fixtures of tests/golden/make_golden_maple.py, graded at twice the reference's own fp16-chain distance e_ref per depth
slice, no floor), composition with unfrozen tails, the equivalences with CoOp and VPT at depth 1, the bits of everything that existed before, the refusals,
and training."""
import math

import pytest
import torch

import maple_ref
import vpt_ref
from conftest import golden, observe
from spec import RESNET, SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(maple_ref.LOGIT_SCALE, dtype=torch.float32)
    return build_model(sd).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---- the row kernels ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [64, 512])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_rows_at_an_offset_follow_the_torch_expression_and_the_documented_order(B, W):
    """Replace: the bits of the torch expression, the rows outside the window keep theirs.  Gradient: the bits of the emulated walk, inside the derived
    tolerance of float64; with clear only the window is zeroed (exact +0) and dctx equals the non-clearing call; at off = L - P the bits of the VPT entries."""
    from proto_clip_amd import ops
    for P in (1, 4):
        for L, off in ((9, 1), (9, 0), (P + 3, 3), (32, 1), (33, 1)):
            g = torch.Generator().manual_seed(100 * B + 10 * P + L + off)
            x = torch.randn(B * L, W, generator=g).half()
            ctx = torch.randn(P, W, generator=g) * torch.logspace(-6, 1, W)      # values across fp16's range, subnormal results included
            ctx[0, :4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, -2.0 ** -26])      # ties to even, overflow, underflow
            xd = x.cuda()
            back = ops.rows_replace_(xd, ctx.cuda(), B, L, off)
            assert back.data_ptr() == xd.data_ptr()
            want = maple_ref.replace(x, ctx, B, L, off)
            assert torch.equal(bits(xd), bits(want)), (P, L, off)
            keep = torch.ones(L, dtype=torch.bool)
            keep[off:off + P] = False
            assert torch.equal(bits(xd.cpu().view(B, L, W)[:, keep]), bits(x.view(B, L, W)[:, keep]))

            g16 = vpt_ref.synth_g(B, L, W, 7 * B + P + L + off)
            gd = g16.cuda()
            got = ops.rows_grad(gd, B, L, off, P)
            assert got.dtype == torch.float32 and got.shape == (P, W)
            assert torch.equal(got.cpu(), maple_ref.emulate_rows_grad(g16, B, L, off, P)), (P, L, off)
            assert torch.equal(bits(gd), bits(g16))                              # no clear: the stream is only read
            ratio = maple_ref.worst_ratio(got.cpu(), maple_ref.rows_grad64(g16, B, L, off, P), maple_ref.tol_rows_grad(g16, B, L, off, P))
            observe("rows_grad: |dctx - float64| / ((n + k) u sum|terms|)", ratio, 1.0)
            assert ratio <= 1.0, ratio
            if off + P == L:                                                     # the VPT entries' bits
                assert torch.equal(ops.vpt_grad(gd, B, L - P, P), got)
                assert torch.equal(bits(ops.vpt_replace_(x.cuda(), ctx.cuda(), B, L - P)), bits(xd))
            cleared = ops.rows_grad(gd, B, L, off, P, clear=True)
            assert torch.equal(cleared, got)
            after = gd.cpu().view(B, L, W)
            assert torch.equal(bits(after[:, keep]), bits(g16.view(B, L, W)[:, keep]))
            assert not bits(after[:, off:off + P]).any()                         # exact +0: no sign bit either


# ---- the coupling function -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["decades", "cancel"])
@pytest.mark.parametrize("Wt,Wv", [(64, 128), (64, 192), (128, 256), (512, 768)])
@pytest.mark.parametrize("depth", [1, 3])
def test_coupling_follows_the_documented_order(depth, Wt, Wv, family):
    """Forward and the three gradients: the bits of the emulation, inside the derived tolerance of float64 ((rounded operations on a term's path) u sum|terms|),
    the same bits twice; a gradient that is not asked for is not returned and the others keep their bits.  (torch.autograd.gradcheck does not apply: fp32.)"""
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import ops
    for P in (1, 2, 5, 16):
        X, Wc, bc, dY = maple_ref.synth_couple(depth, P, Wt, Wv, 1000 * depth + 10 * P + Wv, family)
        Xd, Wd, bd, dYd = X.cuda(), Wc.cuda(), bc.cuda(), dY.cuda()
        y = ops.couple(Xd, Wd, bd)
        assert y.dtype == torch.float32 and y.shape == (depth, P, Wv)
        assert torch.equal(y.cpu(), maple_ref.emulate_couple_fwd(X, Wc, bc)), (P, float((y.cpu() - maple_ref.emulate_couple_fwd(X, Wc, bc)).abs().max()))
        ratio = maple_ref.worst_ratio(y.cpu(), maple_ref.couple_fwd64(X, Wc, bc), maple_ref.tol_couple_fwd(X, Wc, bc))
        observe("couple forward: |y - float64| / ((Wt / 16 + 6) u sum|terms|)", ratio, 1.0)
        assert ratio <= 1.0, ratio
        assert torch.equal(ops.couple(Xd, Wd, bd), y)
        grads = ops.couple_backward(dYd, Xd, Wd)
        want = maple_ref.emulate_couple_bwd(dY, X, Wc)
        for name, got, w, w64, tol in zip(("dx", "dweight", "dbias"), grads, want, maple_ref.couple_bwd64(dY, X, Wc), maple_ref.tol_couple_bwd(dY, X, Wc)):
            assert got.dtype == torch.float32 and got.shape == w.shape
            assert torch.equal(got.cpu(), w), (name, P, float((got.cpu() - w).abs().max()))
            ratio = maple_ref.worst_ratio(got.cpu(), w64, tol)
            observe(f"couple backward {name}: |g - float64| / (derived tolerance)", ratio, 1.0)
            assert ratio <= 1.0, (name, ratio)
        again = ops.couple_backward(dYd, Xd, Wd)
        assert all(torch.equal(a, b) for a, b in zip(again, grads))
        for skip in range(3):                                                    # one gradient not asked for: None for it, the others keep their bits
            flags = [i != skip for i in range(3)]
            part = ops.couple_backward(dYd, Xd, Wd, want_x=flags[0], want_weight=flags[1], want_bias=flags[2])
            assert part[skip] is None and all(torch.equal(part[i], grads[i]) for i in range(3) if i != skip)
        only_bias = ops.couple_backward(dYd, Xd, Wd, want_x=False, want_weight=False)
        assert only_bias[0] is None and only_bias[1] is None and torch.equal(only_bias[2], grads[2])
        # the autograd Function over the two entries
        leaves = [t.clone().requires_grad_(i != 1) for i, t in enumerate((Xd, Wd, bd))]                  # the weight frozen: no gradient issued for it
        out = pag.CoupleFn.apply(*leaves)
        assert torch.equal(out, y)
        out.backward(dYd)
        assert leaves[1].grad is None and torch.equal(leaves[0].grad, grads[0]) and torch.equal(leaves[2].grad, grads[2])


# ---- the learner against the reference ----------------------------------------------------------------------------------------------------------------------

def fixture_case(name):
    meta = golden(name)
    kw = maple_ref.towers()[str(meta["tag"])]
    assert float(meta["floor"]) == 0.0
    l_eff = int(meta["l_eff"]) or None
    ctx, weight, bias, tokens, images, labels = maple_ref.fixture_inputs(kw, int(meta["B"]), int(meta["P"]), int(meta["depth"]), int(meta["N"]),
                                                                         int(meta["seed"]), l_eff)
    return meta, make_model(kw, int(meta["sd_seed"])), (ctx, weight, bias), tokens, images.cuda(), labels.cuda()


def make_learner(model, params, tokens, **kw):
    from proto_clip_amd import maple
    ctx, weight, bias = params
    learner = maple.MultiModalPromptLearner([f"class{i}" for i in range(tokens.shape[0])], model, n_ctx=ctx.shape[1], depth=ctx.shape[0],
                                            tokenized_prompts=tokens, **kw)
    with torch.no_grad():
        learner.ctx.copy_(ctx.cuda())
        learner.couple_weight.copy_(weight.cuda())
        learner.couple_bias.copy_(bias.cuda())
    return learner


def run_case(model, params, tokens, images, labels, loss_scale, truncate=True):
    from proto_clip_amd import maple
    learner = make_learner(model, params, tokens, truncate=truncate)
    head = maple.MaPLe(model, learner)
    loss = head.loss(images, labels)
    (loss * loss_scale).backward()
    with torch.no_grad():
        img, txt = learner.image_features(images), learner.text_features()
    return learner, loss, img, txt


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", list(maple_ref.FIXTURES))
def test_learner_against_the_reference(name, loss_scale):
    """Both feature matrices: ||f - f64|| / ||f64|| <= 2 e_ref.  Every depth slice of the three gradients: ||g[d] - g_f64[d]|| / ||g_f64[d]|| <= 2 e_ref[d]
    (e_ref: the reference's own fp16 chain against its float64 run; no floor), the gradient of the 1024-fold loss divided back.  Taped and no_grad features
    are equal bit for bit.  The truncated case also runs at the full context length and must give the same bits."""
    meta, model, params, tokens, images, labels = fixture_case(name)
    depth = int(meta["depth"])
    learner, loss, img, txt = run_case(model, params, tokens, images, labels, loss_scale)
    assert all(p.grad is None for p in model.parameters())
    taped_img, taped_txt = learner.image_features(images), learner.text_features()
    assert taped_img.requires_grad and taped_txt.requires_grad and taped_img.dtype == taped_txt.dtype == torch.float16
    assert torch.equal(taped_img.detach(), img) and torch.equal(taped_txt.detach(), txt) and not img.requires_grad
    worst = {}
    for key, f in (("img", img), ("txt", txt)):
        f64 = torch.from_numpy(meta[f"{key}_f64"]).double()
        worst[key] = float((f.double().cpu() - f64).norm() / f64.norm()) / (2 * float(meta[f"{key}_e_ref"]))
        observe(f"maple {key} features: ||f - f64|| / ||f64|| / (2 e_ref)", worst[key], 1.0)
    for key, p in (("ctx", learner.ctx), ("weight", learner.couple_weight), ("bias", learner.couple_bias)):
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        g, g64 = p.grad.double().cpu() / loss_scale, torch.from_numpy(meta[f"g_{key}_f64"]).double()
        ratios = [float((g[d] - g64[d]).norm() / g64[d].norm()) / (2 * float(meta[f"e_ref_{key}"][d])) for d in range(depth)]
        worst[key] = max(ratios)
        for r in ratios:
            observe(f"maple {key} gradient x{loss_scale:g}: ||g - g64|| / ||g64|| / (2 e_ref), per depth slice", r, 1.0)
        print(f"{name} x{loss_scale:g} {key}: gradient ratios " + " ".join(f"{r:.3f}" for r in ratios)
              + " (e_ref " + " ".join(f"{float(e):.3e}" for e in meta[f"e_ref_{key}"]) + ")")
    print(f"{name} x{loss_scale:g}: MaPLe.loss {float(loss.detach()):.6f}, f64 {float(meta['loss_f64']):.6f}; feature ratios image {worst['img']:.3f} "
          f"text {worst['txt']:.3f}")
    if int(meta["l_eff"]):
        assert learner.run_length == int(meta["l_eff"])
        full, _, img_full, txt_full = run_case(model, params, tokens, images, labels, loss_scale, truncate=False)
        assert full.run_length == 77
        assert torch.equal(txt_full, txt) and torch.equal(img_full, img)
        for a, b in zip(full.parameters(), learner.parameters()):
            assert torch.equal(a.grad, b.grad)
    assert max(worst.values()) <= 1.0, worst


# ---- composition and invariants ------------------------------------------------------------------------------------------------------------------------------

def small_case(depth=2, P=3, B=4, N=6, seed=3, kw=SMALL):
    model = make_model(kw, 31)
    ctx, weight, bias, tokens, images, labels = maple_ref.fixture_inputs(kw, B, P, depth, N, seed)
    return model, (ctx, weight, bias), tokens, images.cuda(), labels.cuda()


def test_composes_with_an_unfrozen_block_of_each_tower():
    from proto_clip_amd import maple
    model, params, tokens, images, labels = small_case()
    learner = make_learner(model, params, tokens)
    head = maple.MaPLe(model, learner)
    (head.loss(images, labels) * 1024.0).backward()
    frozen = [p.grad.clone() for p in learner.parameters()]
    for p in learner.parameters():
        p.grad = None
    model.unfreeze(visual_blocks=1, text_blocks=1)
    (head.loss(images, labels) * 1024.0).backward()
    lv, lt = len(model.visual.transformer.resblocks) - 1, len(model.transformer.resblocks) - 1
    want = {n for n, _ in model.named_parameters()
            if n.startswith((f"visual.transformer.resblocks.{lv}.", "visual.ln_post.", f"transformer.resblocks.{lt}.", "ln_final."))
            or n in ("visual.proj", "text_projection")}
    for n, p in model.named_parameters():
        if n in want:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, n
            assert bool(torch.isfinite(p.grad.float()).all()) and bool(p.grad.any()), n
        else:
            assert p.grad is None, n
    for p, f in zip(learner.parameters(), frozen):
        assert bool(torch.isfinite(p.grad).all()) and all(bool(p.grad[d].any()) for d in range(p.shape[0]))
        assert torch.equal(p.grad, f)                                            # the prompts' gradient does not depend on what else is asked for


def test_the_model_is_untouched_by_a_learner_and_a_step_and_classify_is_the_dense_argmax():
    from proto_clip_amd import maple, ops, utils
    model, params, tokens, images, labels = small_case(depth=3)
    with torch.no_grad():
        before_img, before_txt = model.encode_image(images), model.encode_text(tokens.cuda())
    learner = make_learner(model, params, tokens)
    head = maple.MaPLe(model, learner)
    opt = torch.optim.SGD(learner.parameters(), lr=0.01)
    (head.loss(images, labels) * 1024.0).backward()
    opt.step()
    assert torch.equal(model.encode_image(images), before_img) and torch.equal(model.encode_text(tokens.cuda()), before_txt)
    assert not any(p.requires_grad for p in model.parameters())
    pred = head.classify(images)
    rows = head.text_rows()
    assert rows.dtype == torch.float16 and rows.shape == (tokens.shape[0], SMALL["embed_dim"]) and not rows.requires_grad
    with torch.no_grad():
        dense = utils.clip_logits(ops.l2norm_rows(learner.image_features(images)), rows, scale=float(head.logit_scale()), layout="nd")
    assert pred.dtype == torch.int64 and torch.equal(pred, dense.argmax(1))
    _, values, indices = head.classify(images, topk=2)
    assert torch.equal(indices[:, 0].long(), pred)


def test_depth_one_is_coop_on_the_text_side_and_vpt_on_the_vision_side():
    """Text: the features of coop.PromptLearner with the same context, bit for bit.  Vision: with couple_weight zeroed the coupled rows are couple_bias[0] in
    every row — the bits of vpt.VisualPromptLearner with that `ctx`."""
    from proto_clip_amd import coop, vpt
    model, params, tokens, images, labels = small_case(depth=1, P=4)
    learner = make_learner(model, params, tokens)
    names = [f"class{i}" for i in range(tokens.shape[0])]
    theirs = coop.PromptLearner(names, model, n_ctx=4, tokenized_prompts=tokens)
    with torch.no_grad():
        theirs.ctx.copy_(learner.ctx[0])
        learner.couple_weight.zero_()
    assert torch.equal(learner.text_features().detach(), theirs().detach())
    with torch.no_grad():
        assert torch.equal(learner.text_features(), theirs())
    visual = vpt.VisualPromptLearner(model, n_ctx=4, depth=1)
    with torch.no_grad():
        visual.ctx.copy_(learner.couple_bias[0].expand(1, 4, -1))
        assert torch.equal(learner.visual_rows(), visual.ctx)
        assert torch.equal(learner.image_features(images), visual(images))
    assert torch.equal(learner.image_features(images).detach(), visual(images).detach())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_path():
    from proto_clip_amd import maple, ops
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.clip.model import BACKBONES, CLIP
    model, params, tokens, images, labels = small_case(kw=TINY)
    names = [f"class{i}" for i in range(tokens.shape[0])]
    new = lambda m=model, **kw: maple.MultiModalPromptLearner(names, m, **{"n_ctx": 3, "depth": 2, "tokenized_prompts": tokens, **kw})  # noqa: E731
    with pytest.raises(PclipError, match=r"ModifiedResNet"):
        new(make_model(RESNET, 6, trained=False), tokenized_prompts=torch.zeros(6, 77, dtype=torch.int64))
    odd = make_model(TINY, 5)
    odd.visual.heads = 4
    with pytest.raises(PclipError, match=r"vision tower of width 128 with 4 heads \(head dimension 64 only\)"):
        new(odd)
    odd = make_model(TINY, 5)
    odd.transformer_heads = 2
    with pytest.raises(PclipError, match=r"text tower of width 64 with 2 heads \(head dimension 64 only\)"):
        new(odd)
    with pytest.raises(PclipError, match=r"depth=3 outside 1\.\.2"):
        new(depth=3)
    with pytest.raises(PclipError, match=r"n_ctx=17 outside 1\.\.16"):
        new(n_ctx=17)
    big = BACKBONES["ViT-L/14@336px"]
    with torch.device("meta"):
        tower = CLIP(big["embed_dim"], big["image_resolution"], big["vision_layers"], big["vision_width"], big["vision_patch_size"], big["context_length"],
                     big["vocab_size"], big["transformer_width"], big["transformer_heads"], big["transformer_layers"])
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx = 577 \+ 3 = 580 vision tokens exceed the attention envelope of 288"):
        new(tower)
    early = tokens.clone()
    early[2] = 0
    early[2, 0], early[2, 3] = TINY["vocab_size"] - 2, TINY["vocab_size"] - 1
    with pytest.raises(PclipError, match=r"EOT of prompt 2 .* sits at position 3, at or before the last of the n_ctx=3 context rows"):
        new(tokenized_prompts=early)
    with pytest.raises(PclipError, match=r"class_specific"):
        new(class_specific=True)
    learner = make_learner(model, params, tokens)
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            learner.image_features(images)
        with pytest.raises(PclipError, match="low_latency"):
            learner.text_features()
    assert learner.image_features(images).requires_grad and learner.text_features().requires_grad
    learner.couple_bias.data = learner.couple_bias.data.half()
    with pytest.raises(PclipError, match=r"couple_bias must be torch.float32, got torch.float16"):
        learner.image_features(images)
    with pytest.raises(PclipError, match=r"couple_bias must be torch.float32, got torch.float16"):
        learner.text_features()
    learner.couple_bias.data = learner.couple_bias.data.float()
    model.unfreeze(stem="visual", heads=False)
    with pytest.raises(PclipError, match=r"unfreeze\(stem=\.\.\.\)"):
        learner.image_features(images)
    other, params, tokens, images, labels = small_case(kw=TINY)
    learner = make_learner(other, params, tokens)
    other.unfreeze(stem="text", heads=False)
    with pytest.raises(PclipError, match=r"text embeddings have been opted in through unfreeze\(stem=\.\.\.\)"):
        learner.text_features()
    # the kernels' own envelope (PCLIP_REQUIRE) and the wrappers' checks
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(PclipError, match=r"P=17 rows outside 1 \.\. 16"):
        ops.couple(z(1, 17, 64), z(1, 128, 64), z(1, 128))
    with pytest.raises(PclipError, match=r"Wt=96 must be a positive multiple of 64"):
        ops.couple(z(1, 2, 96), z(1, 128, 96), z(1, 128))
    with pytest.raises(PclipError, match=r"Wv=12 must be a positive multiple of 8"):
        ops.couple_backward(z(1, 2, 12), z(1, 2, 64), z(1, 12, 64))
    with pytest.raises(PclipError, match=r"bias \(1, 64\) is not \[1, 128\]"):
        ops.couple(z(1, 2, 64), z(1, 128, 64), z(1, 64))
    with pytest.raises(PclipError, match=r"weight must be float32"):
        ops.couple(z(1, 2, 64), z(1, 128, 64).half(), z(1, 128))
    x16 = torch.zeros(2 * 9, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(PclipError, match=r"rows off \.\. off \+ P - 1 = 8 \.\. 9 do not lie inside a sequence of L=9 rows"):
        ops.rows_replace_(x16, z(2, 64), 2, 9, 8)
    with pytest.raises(PclipError, match=r"rows off \.\. off \+ P - 1 = -1 \.\. 0 do not lie inside"):
        ops.rows_grad(x16, 2, 9, -1, 2)
    with pytest.raises(PclipError, match=r"L = 289 tokens exceed the attention envelope of 288"):
        ops.rows_grad(torch.zeros(289, 64, dtype=torch.float16, device="cuda"), 1, 289, 1, 2)
    from proto_clip_amd.tower import run_tower
    tw = model.text_tower
    with pytest.raises(PclipError, match=r"deep_off \.\. deep_off \+ P - 1 = 8 \.\. 10 do not lie inside a sequence of L=10 tokens"):
        run_tower(tw, x16.new_zeros(20, 64), 2, 10, (0, False), tw.pick(2, 10, x16.device, tokens[:2, :10].cuda()), deep=z(1, 3, 64), deep_off=8)


# ---- training ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_five_sgd_steps_of_run_maple_lower_the_loss():
    """maple_ref.SGD_CASE: TINY, 8 images in one batch, 2 context rows at depth 2, SGD on the three tensors with momentum 0.9 at learning rate 0.03 under a
    cosine schedule over the five steps, loss scale 1024.  The reference's fp32 chain on the CPU, with the fixtures' hooks and the same step rule
    (`make_golden_maple.py sgd`), goes 1.770919 1.758501 1.754799 1.746484 1.742640 -> 1.741962: a decrease of 0.028957.  At least half of that is required."""
    from proto_clip_amd import maple
    tag, sd_seed, B, P, depth, N, seed, lr = maple_ref.SGD_CASE
    kw = maple_ref.towers()[tag]
    model = make_model(kw, sd_seed)
    ctx, weight, bias, tokens, images, labels = maple_ref.fixture_inputs(kw, B, P, depth, N, seed)
    images, labels = images.cuda(), labels.cuda()
    cfg = {"maple_epochs": 5, "maple_batch": B, "maple_lr": lr, "maple_loss_scale": 1024.0, "seed": seed}
    start = make_learner(model, (ctx, weight, bias), tokens)                     # the measured case starts from the fixture's parameters
    learner, losses = maple.run_maple(cfg, images, labels, start.classnames, model, learner=start)
    assert learner is start and len(losses) == 5 and all(math.isfinite(v) for v in losses)
    with torch.no_grad():
        final = float(maple.MaPLe(model, learner).loss(images, labels))
    print("run_maple loss over five SGD steps:", " ".join(f"{v:.6f}" for v in losses), f"-> {final:.6f}; decrease {losses[0] - final:.6f}"
          f" (reference fp32 chain: {maple_ref.SGD_REFERENCE_DECREASE:.6f})")
    observe("run_maple: half the reference's five-step decrease / the decrease here", 0.5 * maple_ref.SGD_REFERENCE_DECREASE / max(losses[0] - final, 1e-9), 1.0)
    assert losses[0] - final >= 0.5 * maple_ref.SGD_REFERENCE_DECREASE, (losses, final)
