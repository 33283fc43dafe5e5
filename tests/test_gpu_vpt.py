"""Visual prompt tuning on the GPU (proto_clip_amd.vpt, autograd.VptEmbedFn / TowerTailFn with its deep-prompt pack, csrc/pclip_vpt.hip): the three kernels
bit for bit against their torch expressions and the CPU emulation of the documented summation order (tests/vpt_ref.py), the learner against the reference's
own float64 autograd (fixtures of tests/golden/make_golden_vpt.py, graded at twice the reference's own fp16-chain distance e_ref, no floor), composition with
an unfrozen tail and with a coupled `ctx`, the bits of everything that existed before (profiles/vpt.txt), the refusals, and training."""
import hashlib
import math
import os

import pytest
import torch

import vpt_ref
from conftest import REPO, golden, observe
from spec import RESNET, SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(vpt_ref.LOGIT_SCALE, dtype=torch.float32)
    return build_model(sd).cuda()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [64, 192, 768])
def test_append_and_replace_have_the_bits_of_the_torch_expression(W):
    from proto_clip_amd import ops
    g = torch.Generator().manual_seed(W)
    for L0, P in ((17, 1), (26, 7), (197, 8), (257, 31)):
        for B in (1, 5):
            t = torch.randn(B * L0, W, generator=g).half()
            ctx = torch.randn(P, W, generator=g) * torch.logspace(-6, 1, W)      # values across fp16's range, subnormal results included
            ctx[0, :4] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 70000.0, -2.0 ** -26])      # ties to even, overflow, underflow
            got = ops.vpt_append(t.cuda(), ctx.cuda(), B, L0)
            want = torch.cat([t.view(B, L0, W), ctx.half().expand(B, P, W)], 1).reshape(B * (L0 + P), W)
            assert got.dtype == torch.float16 and got.shape == want.shape
            assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), (L0, P, B)
            assert torch.equal(want, vpt_ref.append(t, ctx, B, L0))
            x = torch.randn(B * (L0 + P), W, generator=g).half()
            ctx2 = torch.randn(P, W, generator=g) * 0.02
            xd = x.cuda()
            back = ops.vpt_replace_(xd, ctx2.cuda(), B, L0)
            assert back.data_ptr() == xd.data_ptr()
            want = x.clone().view(B, L0 + P, W)
            want[:, L0:] = ctx2.half()
            assert torch.equal(xd.cpu().view(torch.int16), want.reshape(-1, W).view(torch.int16)), (L0, P, B)
    only = ops.vpt_append(None, ctx.cuda(), 3, 0)                              # no stem rows: the broadcast prompts alone
    assert torch.equal(only.cpu(), ctx.half().expand(3, -1, -1).reshape(-1, W))


@pytest.mark.parametrize("W", [64, 768])
@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 256])
def test_prompt_gradient_follows_the_documented_order(B, P, W):
    """Strided (L0 = 5 rows in front of the prompt rows) and compact (L0 = 0): the bits of the emulated walk, inside the derived tolerance of float64, the
    same bits twice; with clear exactly the prompt rows are +0 afterwards and every other element keeps its bits."""
    from proto_clip_amd import ops
    for L0 in (5, 0):
        g16 = vpt_ref.synth_g(B, L0 + P, W, 7 * B + P + L0)
        want = vpt_ref.emulate_grad(g16, B, L0, P)
        gd = g16.cuda()
        got = ops.vpt_grad(gd, B, L0, P)
        assert got.dtype == torch.float32 and got.shape == (P, W)
        assert torch.equal(got.cpu(), want), (L0, float((got.cpu() - want).abs().max()))
        assert torch.equal(gd.cpu().view(torch.int16), g16.view(torch.int16))  # no clear: the stream is only read
        ratio = vpt_ref.worst_ratio(got.cpu(), vpt_ref.grad64(g16, B, L0, P), vpt_ref.tol_grad(g16, B, L0, P))
        observe("vpt_grad: |dctx - float64| / ((n + k) u sum|terms|)", ratio, 1.0)
        assert ratio <= 1.0, ratio
        assert torch.equal(ops.vpt_grad(gd, B, L0, P), got)
        cleared = ops.vpt_grad(gd, B, L0, P, clear=True)
        assert torch.equal(cleared, got)
        after = gd.cpu().view(B, L0 + P, W)
        assert torch.equal(after[:, :L0].contiguous().view(torch.int16), g16.view(B, L0 + P, W)[:, :L0].contiguous().view(torch.int16))
        assert not after[:, L0:].contiguous().view(torch.int16).any()           # exact +0: no sign bit either


# ---- the learner against the reference ------------------------------------------------------------------------------------------------------------------

def fixture_case(name):
    meta = golden(name)
    kw = vpt_ref.towers()[str(meta["tag"])]
    assert float(meta["floor"]) == 0.0
    ctx, images, text, labels = vpt_ref.fixture_inputs(kw, int(meta["B"]), int(meta["P"]), int(meta["depth"]), int(meta["N"]), int(meta["seed"]))
    return meta, make_model(kw, int(meta["sd_seed"])), ctx, images.cuda(), text.cuda(), labels.cuda()


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", list(vpt_ref.FIXTURES))
def test_learner_against_the_reference(name, loss_scale):
    """Features: ||f - feat_f64|| / ||feat_f64|| <= 2 feat_e_ref.  Every depth slice of ctx.grad: ||g[i] - g_f64[i]|| / ||g_f64[i]|| <= 2 e_ref[i] (e_ref: the
    reference's own fp16 chain against its float64 run; no floor), the gradient of the 1024-fold loss divided back.  Taped and no_grad features are equal bit
    for bit, and an image alone has the feature row it has inside the batch."""
    from proto_clip_amd import vpt
    meta, model, ctx, images, text, labels = fixture_case(name)
    depth, P = int(meta["depth"]), int(meta["P"])
    learner = vpt.VisualPromptLearner(model, n_ctx=P, depth=depth)
    with torch.no_grad():
        learner.ctx.copy_(ctx.cuda())
    head = vpt.VPT(model, learner)
    loss = head.loss(images, text, labels, layout="nd")
    (loss * loss_scale).backward()
    assert learner.ctx.grad.dtype == torch.float32 and learner.ctx.grad.shape == learner.ctx.shape
    assert all(p.grad is None for p in model.parameters())
    taped = learner(images)
    with torch.no_grad():
        untaped = learner(images)
        alone = torch.cat([learner(images[i:i + 1]) for i in range(images.shape[0])])
    assert taped.requires_grad and taped.dtype == torch.float16 and not untaped.requires_grad
    assert torch.equal(taped.detach(), untaped)
    assert torch.equal(alone, untaped)
    f64 = torch.from_numpy(meta["feat_f64"]).double()
    f_ratio = float((untaped.double().cpu() - f64).norm() / f64.norm()) / (2 * float(meta["feat_e_ref"]))
    g = learner.ctx.grad.double().cpu() / loss_scale
    g64 = torch.from_numpy(meta["g_f64"]).double()
    ratios = [float((g[i] - g64[i]).norm() / g64[i].norm()) / (2 * float(meta["e_ref"][i])) for i in range(depth)]
    loss_feat = float(vpt_ref.loss64(untaped.cpu(), text.cpu(), labels.cpu()))
    print(f"{name} x{loss_scale:g}: VPT.loss {float(loss.detach()):.6f}, float64 loss of the features {loss_feat:.6f}, f64 {float(meta['loss_f64']):.6f};"
          f" feature ratio {f_ratio:.3f} (e_ref {float(meta['feat_e_ref']):.3e}); gradient ratios " + " ".join(f"{r:.3f}" for r in ratios)
          + " (e_ref " + " ".join(f"{float(e):.3e}" for e in meta["e_ref"]) + ")")
    observe("vpt features: ||f - f64|| / ||f64|| / (2 e_ref)", f_ratio, 1.0)
    for r in ratios:
        observe(f"vpt prompt gradient x{loss_scale:g}: ||g - g64|| / ||g64|| / (2 e_ref), per depth slice", r, 1.0)
    assert f_ratio <= 1.0, f_ratio
    assert max(ratios) <= 1.0, ratios


# ---- composition ----------------------------------------------------------------------------------------------------------------------------------------

def small_case(depth=2, P=5, B=4, N=6, seed=3):
    model = make_model(SMALL, 31)
    ctx, images, text, labels = vpt_ref.fixture_inputs(SMALL, B, P, depth, N, seed)
    return model, ctx.cuda(), images.cuda(), text.cuda(), labels.cuda()


def test_composes_with_an_unfrozen_last_block():
    from proto_clip_amd import vpt
    model, ctx, images, text, labels = small_case()
    learner = vpt.VisualPromptLearner(model, n_ctx=5, depth=2)
    head = vpt.VPT(model, learner)
    (head.loss(images, text, labels, layout="nd") * 1024.0).backward()
    frozen_grad = learner.ctx.grad.clone()
    learner.ctx.grad = None
    model.unfreeze(visual_blocks=1)
    (head.loss(images, text, labels, layout="nd") * 1024.0).backward()
    last = len(model.visual.transformer.resblocks) - 1
    want = {n for n, _ in model.named_parameters() if n.startswith((f"visual.transformer.resblocks.{last}.", "visual.ln_post.")) or n == "visual.proj"}
    for n, p in model.named_parameters():
        if n in want:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, n
            assert bool(torch.isfinite(p.grad.float()).all()) and bool(p.grad.any()), n
        else:
            assert p.grad is None, n
    assert bool(torch.isfinite(learner.ctx.grad).all()) and bool(learner.ctx.grad[0].any()) and bool(learner.ctx.grad[1].any())
    assert torch.equal(learner.ctx.grad, frozen_grad)                           # the prompts' gradient does not depend on what else is asked for


def test_a_coupled_ctx_back_propagates_into_its_source():
    """`ctx` as a non-leaf: an fp32 linear map of another parameter (MaPLe's coupling in miniature).  The source's gradient is the chain rule applied to the
    gradient the parameter form receives, in fp32."""
    from proto_clip_amd import vpt
    model, ctx, images, text, labels = small_case()
    W = SMALL["vision_width"]
    learner = vpt.VisualPromptLearner(model, n_ctx=5, depth=2)
    with torch.no_grad():
        learner.ctx.copy_(ctx)
    g = torch.Generator().manual_seed(9)
    source = (torch.randn(2, 5, 48, generator=g) * 0.1).cuda().requires_grad_(True)
    weight = (torch.randn(W, 48, generator=g) * 0.05).cuda()
    coupled = torch.nn.functional.linear(source, weight)                        # [2, 5, W] fp32, a non-leaf on the tape
    assert not coupled.is_leaf and coupled.dtype == torch.float32
    head = vpt.VPT(model, learner)
    feats = learner(images, ctx=coupled)
    from proto_clip_amd import autograd as pag
    loss = pag.cosine_cross_entropy(feats, text, head.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)
    (loss * 1024.0).backward()
    assert learner.ctx.grad is None and source.grad is not None and bool(torch.isfinite(source.grad).all()) and bool(source.grad.any())
    with torch.no_grad():
        learner.ctx.copy_(coupled.detach())
    (head.loss(images, text, labels, layout="nd") * 1024.0).backward()
    want = learner.ctx.grad @ weight                                            # d loss / d source = d loss / d ctx  W
    # two fp32 dot products of length W over the same terms: each within W u sum|terms| of the exact value
    tol = 2 * W * vpt_ref.U32 * (learner.ctx.grad.double().abs() @ weight.double().abs())
    assert bool(((source.grad.double() - want.double()).abs() <= tol).all())


# ---- nothing existing moves ---------------------------------------------------------------------------------------------------------------------------------

def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def recorded_digests():
    out = {}
    for line in open(os.path.join(REPO, "profiles", "vpt.txt")):
        if line.startswith("digest "):
            _, key, value = line.split()
            out[key] = value
    return out


def parent_case():
    """The taped encode_image whose bits were recorded on the parent commit (tools/vpt_bench.py --digests): SMALL, two trainable blocks."""
    model = make_model(SMALL, 41)
    _, images, text, labels = vpt_ref.fixture_inputs(SMALL, 6, 1, 1, 5, 11)
    return model, images.cuda(), text.cuda(), labels.cuda()


def tail_digests(model, images, text, labels):
    from proto_clip_amd import autograd as pag
    params = model.unfreeze(visual_blocks=2)
    feats = model.encode_image(images)
    loss = pag.cosine_cross_entropy(feats, text, 20.0, labels=labels, normalize_a=True, normalize_b=True)
    (loss * 1024.0).backward()
    out = {"encode_image.features": digest(feats)}
    names = {id(p): n for n, p in model.named_parameters()}
    for p in params:
        if p.grad is not None:
            out["grad." + names[id(p)]] = digest(p.grad)
    return out


def test_the_taped_tail_keeps_the_bits_recorded_on_the_parent():
    want = recorded_digests()
    got = tail_digests(*parent_case())
    grads = [k for k in want if k.startswith("grad.visual.")]
    assert len(grads) == 2 * 12 + 3 and "encode_image.features" in want        # two blocks, the two heads' tensors
    assert set(got) == set(want)
    differing = [k for k in want if got[k] != want[k]]
    assert not differing, differing


def test_encode_image_is_untouched_by_a_learner_and_a_step():
    from proto_clip_amd import vpt
    model, ctx, images, text, labels = small_case()
    with torch.no_grad():
        before = model.encode_image(images)
    learner = vpt.VisualPromptLearner(model, n_ctx=5, depth=3)
    head = vpt.VPT(model, learner)
    opt = torch.optim.SGD(learner.parameters(), lr=0.01)
    (head.loss(images, text, labels, layout="nd") * 1024.0).backward()
    opt.step()
    assert torch.equal(model.encode_image(images), before)
    assert not any(p.requires_grad for p in model.parameters())
    pred = head.classify(images, text, layout="nd")
    with torch.no_grad():
        from proto_clip_amd import ops, utils
        dense = utils.clip_logits(ops.l2norm_rows(learner(images)), ops.l2norm_rows(text), scale=float(head.logit_scale()), layout="nd")
    assert pred.dtype == torch.int64 and torch.equal(pred, dense.argmax(1))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_path():
    from proto_clip_amd import ops, vpt
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.clip.model import BACKBONES, CLIP
    model = make_model(TINY, 5)
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx = 17 \+ 272 = 289"):
        vpt.VisualPromptLearner(model, n_ctx=272)
    with pytest.raises(PclipError, match=r"L0 \+ P = 257 \+ 32 = 289 tokens exceed"):
        ops.vpt_append(torch.zeros(257, 64, dtype=torch.float16, device="cuda"), torch.zeros(32, 64, device="cuda"), 1, 257)
    with pytest.raises(PclipError, match=r"ModifiedResNet"):
        vpt.VisualPromptLearner(make_model(RESNET, 6, trained=False))
    big = BACKBONES["ViT-L/14@336px"]                                           # 577 tokens of its own: refused at construction, no weights needed
    with torch.device("meta"):
        tower = CLIP(big["embed_dim"], big["image_resolution"], big["vision_layers"], big["vision_width"], big["vision_patch_size"], big["context_length"],
                     big["vocab_size"], big["transformer_width"], big["transformer_heads"], big["transformer_layers"])
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx = 577 \+ 1 = 578"):
        vpt.VisualPromptLearner(tower, n_ctx=1)
    learner = vpt.VisualPromptLearner(model, n_ctx=2, depth=2)
    images = torch.zeros(3, 3, 32, 32, device="cuda")
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            learner(images)
    assert learner(images).requires_grad
    model.unfreeze(stem="visual", heads=False)
    with pytest.raises(PclipError, match=r"unfreeze\(stem=\.\.\.\)"):
        learner(images)


# ---- training -------------------------------------------------------------------------------------------------------------------------------------------------

def test_five_sgd_steps_of_run_vpt_lower_the_loss():
    """vpt_ref.SGD_CASE: TINY, 8 images in one batch, 4 prompt rows at depth 2, SGD with momentum 0.9 at learning rate 0.03 under a cosine schedule over the five
    steps, loss scale 1024.  The reference's fp32 chain on the CPU, with the fixtures' hooks and the same step rule (`make_golden_vpt.py sgd`), goes
    1.743831 1.580559 1.539177 1.502075 1.499822 -> 1.496508: a decrease of 0.247323.  At least half of that is required here."""
    from proto_clip_amd import vpt
    tag, sd_seed, B, P, depth, N, seed, lr = vpt_ref.SGD_CASE
    kw = vpt_ref.towers()[tag]
    model = make_model(kw, sd_seed)
    ctx, images, text, labels = vpt_ref.fixture_inputs(kw, B, P, depth, N, seed)
    images, text, labels = images.cuda(), text.cuda(), labels.cuda()
    cfg = {"vpt_epochs": 5, "vpt_batch": B, "vpt_lr": lr, "vpt_loss_scale": 1024.0, "seed": seed}
    start = vpt.VisualPromptLearner(model, n_ctx=P, depth=depth)                # the measured case starts from the fixture's prompts
    with torch.no_grad():
        start.ctx.copy_(ctx.cuda())
    learner, losses = vpt.run_vpt(cfg, images, labels, text.t().contiguous(), model, learner=start)
    assert learner is start
    assert isinstance(learner, vpt.VisualPromptLearner) and len(losses) == 5 and all(math.isfinite(v) for v in losses)
    with torch.no_grad():
        final = float(vpt.VPT(model, learner).loss(images, text, labels, layout="nd"))
    print("run_vpt loss over five SGD steps:", " ".join(f"{v:.6f}" for v in losses), f"-> {final:.6f}; decrease {losses[0] - final:.6f}"
          f" (reference fp32 chain: {vpt_ref.SGD_REFERENCE_DECREASE:.6f})")
    observe("run_vpt: half the reference's five-step decrease / the decrease here", 0.5 * vpt_ref.SGD_REFERENCE_DECREASE / max(losses[0] - final, 1e-9), 1.0)
    assert losses[0] - final >= 0.5 * vpt_ref.SGD_REFERENCE_DECREASE, (losses, final)
