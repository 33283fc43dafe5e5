"""PromptSRC without a device: the Gaussian weights and the aggregate over the epochs against float64, `train_prompts`' new hook (absent: the statements of
before), the learner's parameters, the refusals that come before any launch, and the fixtures' own arithmetic."""
import inspect
import sys

import numpy as np
import pytest
import torch

import coop_ref
import promptsrc_ref as pr
from conftest import golden
from spec import RESNET, SMALL, TINY

U32 = 2.0 ** -24


def make_model(kw, seed):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    return build_model(random_state_dict(seed=seed, **kw))


# ---- the Gaussian weights and the aggregate ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epochs,mean,std", [(1, 15, 1), (5, 15, 1), (20, 15, 1), (50, 45, 5), (50, 6.4, 10), (20, 14.6, 1), (3, 1000, 0.5), (7, -3, 2)])
def test_gpa_weights(epochs, mean, std):
    from proto_clip_amd.promptsrc import gpa_weights
    w = gpa_weights(epochs, mean, std)
    assert w.dtype == np.float64 and w.shape == (epochs,)
    assert abs(w.sum() - 1.0) <= 1e-15 and (w >= 0).all()
    if epochs == 1:
        assert w.tolist() == [1.0]
    peak = min(max(int(round(mean)), 1), epochs)                       # inside the epochs: at round(mean); outside: at the nearer end
    assert int(w.argmax()) + 1 == peak
    x = np.arange(1, epochs + 1, dtype=np.float64)
    if 1 <= mean <= epochs:                                            # upstream's own formula, where it does not underflow
        g = np.exp(-0.5 * ((x - mean) / std) ** 2) / (std * np.sqrt(2 * np.pi))
        assert np.allclose(w, g / g.sum(), rtol=1e-13, atol=0)


def test_gpa_weights_refusals():
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.promptsrc import gpa_weights
    for args in ((0, 15, 1), (5, 15, 0), (5, 15, -1), (5, float("nan"), 1), (5, 15, float("inf"))):
        with pytest.raises(PclipError, match="gpa_weights"):
            gpa_weights(*args)


@pytest.mark.parametrize("mean,std", [(15, 1), (3, 1), (2.5, 4)])
def test_aggregate_of_five_snapshots_is_the_float64_weighted_sum(mean, std):
    """|acc - sum_e w_e theta_e| <= (E + 1) u sum_e |w_e theta_e| per element: the rounding of w_e to fp32, the product (or its fusion into the addition),
    and at most E additions of which the first is exact."""
    from proto_clip_amd.promptsrc import GaussianAggregate, gpa_weights
    E = 5
    g = torch.Generator().manual_seed(int(10 * mean + std))
    params = [torch.nn.Parameter(torch.randn(3, 4, 64, generator=g) * 0.02), torch.nn.Parameter(torch.randn(2, 5, 128, generator=g))]
    w = gpa_weights(E, mean, std)
    agg = GaussianAggregate(params, w)
    snaps = []
    for e in range(E):
        with torch.no_grad():
            for p in params:
                p.add_(torch.randn(p.shape, generator=g) * 0.01)       # an epoch of training
        snaps.append([p.detach().clone() for p in params])
        agg.add()
    agg.finish_()
    for i, p in enumerate(params):
        want, mag = pr.gpa_sum64(w, [s[i] for s in snaps])
        err = (p.detach().double() - want).abs()
        assert p.dtype == torch.float32 and bool((err <= (E + 1) * U32 * mag).all()), float((err / ((E + 1) * U32 * mag)).max())
    from proto_clip_amd._lib import PclipError
    with pytest.raises(PclipError, match="after all 5 epochs"):
        agg.add()
    with pytest.raises(PclipError, match="after 1 of 5 epochs"):
        short = GaussianAggregate(params, w)
        short.add()
        short.finish_()


# ---- train_prompts: the hook, and its absence --------------------------------------------------------------------------------------------------------------

def run_loop(on_epoch_end, record=None):
    from proto_clip_amd import prompt_train
    g = torch.Generator().manual_seed(0)
    target = torch.randn(12, 8, generator=g)
    p = torch.nn.Parameter(torch.zeros(8))
    lines = []
    code = prompt_train.train_prompts.__code__

    def tracer(frame, event, arg):
        if frame.f_code is code:
            if event == "line":
                lines.append(frame.f_lineno)
            return tracer
        return None
    kw = {} if on_epoch_end is None else {"on_epoch_end": (lambda epoch: on_epoch_end(epoch, p))}
    sys.settrace(tracer)
    try:
        res, losses = prompt_train.train_prompts("toy", [p], lambda idx: ((p - target[idx]) ** 2).mean(), 12, torch.device("cpu"), epochs=3, batch=5, lr=0.1,
                                                 momentum=0.9, loss_scale=1024.0, seed=3, **kw)
    finally:
        sys.settrace(None)
    return p.detach().clone(), losses, lines


def test_train_prompts_without_the_hook_executes_the_statements_of_before(capsys):
    """on_epoch_end absent: no line of the hook's call runs, and the lines that run are those of a run WITH a hook minus that call; the results are equal bit
    for bit (the hook only looks).  The hook sees epochs 0, 1, 2, each after the epoch's last step."""
    from proto_clip_amd import prompt_train
    src, first = inspect.getsourcelines(prompt_train.train_prompts)
    call = [first + i for i, text in enumerate(src) if text.strip() == "on_epoch_end(epoch)"]
    assert len(call) == 1
    assert inspect.signature(prompt_train.train_prompts).parameters["on_epoch_end"].default is None
    seen = []
    p0, losses0, lines0 = run_loop(None)
    p1, losses1, lines1 = run_loop(lambda epoch, p: seen.append((epoch, p.detach().clone())))
    assert call[0] not in lines0 and lines1.count(call[0]) == 3
    assert [n for n in lines1 if n != call[0]] == lines0               # the same statements in the same order
    assert torch.equal(p0, p1) and losses0 == losses1
    assert [e for e, _ in seen] == [0, 1, 2] and torch.equal(seen[-1][1], p1) and not torch.equal(seen[0][1], seen[1][1])


# ---- the learner and the refusals ------------------------------------------------------------------------------------------------------------------------------

def small_learner(model=None, kw=SMALL, **over):
    from proto_clip_amd import promptsrc
    model = make_model(kw, 3) if model is None else model
    tokens = coop_ref.prompt_tokens(4, 2, kw["vocab_size"], 5)
    args = dict(n_ctx_text=2, n_ctx_vision=5, depth_text=1, depth_vision=3, tokenized_prompts=tokens)
    args.update(over)
    return model, promptsrc.IndependentPromptLearner(pr.names(4), model, **args)


def test_parameters_are_exactly_the_two_tensors():
    from proto_clip_amd import promptsrc
    model, learner = small_learner()
    got = dict(learner.named_parameters())
    assert sorted(got) == ["ctx", "vctx"]
    assert got["ctx"].shape == (1, 2, SMALL["transformer_width"]) and got["vctx"].shape == (3, 5, SMALL["vision_width"])      # unequal rows and depths
    assert all(p.dtype == torch.float32 and p.requires_grad for p in got.values())
    _, again = small_learner(model)
    assert all(torch.equal(p, q) for p, q in zip(learner.parameters(), again.parameters()))                                  # the seed decides
    _, other = small_learner(model, seed=2)
    assert not torch.equal(other.ctx, learner.ctx) and not torch.equal(other.vctx, learner.vctx)
    head = promptsrc.PromptSRC(model, learner, torch.zeros(4, SMALL["embed_dim"], dtype=torch.float16))
    assert list(head.parameters()) == list(learner.parameters())
    assert not any(p.requires_grad for p in model.parameters())
    from proto_clip_amd import IndependentPromptLearner, PromptSRC, run_promptsrc  # noqa: F401


def test_refusals_that_need_no_device():
    from proto_clip_amd import promptsrc
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.clip.model import BACKBONES, CLIP
    model = make_model(TINY, 4)
    tokens = coop_ref.prompt_tokens(4, 2, TINY["vocab_size"], 5)
    new = lambda m=model, **kw: small_learner(m, TINY, **{"depth_vision": 2, "tokenized_prompts": tokens, **kw})[1]  # noqa: E731
    with pytest.raises(PclipError, match=r"ModifiedResNet"):
        new(make_model(RESNET, 6), tokenized_prompts=coop_ref.prompt_tokens(4, 2, RESNET["vocab_size"], 5))
    for side in ("text", "vision"):
        for depth in (0, 3):
            with pytest.raises(PclipError, match=r"depth_%s=%d outside 1\.\.2" % (side, depth)):
                new(**{"depth_" + side: depth})
    with pytest.raises(PclipError, match=r"n_ctx_vision=0 must be at least 1"):
        new(n_ctx_vision=0)
    with pytest.raises(PclipError, match=r"n_ctx=0 must be at least 1"):
        new(n_ctx_text=0)
    with pytest.raises(PclipError, match=r"class_specific"):
        new(class_specific=True)
    with pytest.raises(PclipError, match=r"class_specific"):
        promptsrc.run_promptsrc({"promptsrc_epochs": 1, "class_specific": True}, None, None, pr.names(4), (), model)
    big = BACKBONES["ViT-L/14@336px"]                                           # 577 vision tokens of its own: refused at construction, no weights needed
    with torch.device("meta"):
        tower = CLIP(big["embed_dim"], big["image_resolution"], big["vision_layers"], big["vision_width"], big["vision_patch_size"], big["context_length"],
                     big["vocab_size"], big["transformer_width"], big["transformer_heads"], big["transformer_layers"])
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx_vision = 577 \+ 5 = 582 vision tokens exceed the attention envelope of 288"):
        new(tower, tokenized_prompts=torch.zeros(4, 77, dtype=torch.int64))
    odd = make_model(TINY, 4)
    odd.transformer_heads = 2
    with pytest.raises(PclipError, match=r"text tower of width 64 with 2 heads \(head dimension 64 only\)"):
        new(odd)
    odd = make_model(TINY, 4)
    odd.visual.heads = 4
    with pytest.raises(PclipError, match=r"vision tower of width 128 with 4 heads \(head dimension 64 only\)"):
        new(odd)
    # the head: its teacher's rows, and a frozen model
    learner = new()
    fixed = torch.zeros(4, TINY["embed_dim"], dtype=torch.float16)
    for bad, text in ((fixed.float(), "2-D float16"), (fixed[:3], "3 rows, the prompt learner 4 classes"), (fixed.clone().requires_grad_(True), "requires grad")):
        with pytest.raises(PclipError, match=text):
            promptsrc.PromptSRC(model, learner, bad)
    with pytest.raises(PclipError, match="another CLIP model"):
        promptsrc.PromptSRC(make_model(TINY, 4), learner, fixed)


@pytest.mark.parametrize("how", [dict(visual_blocks=1), dict(text_blocks=1), dict(heads=True), dict(stem="visual", heads=False), dict(stem="text", heads=False)])
def test_promptsrc_is_refused_on_an_unfrozen_tower_before_any_launch(how):
    """CPU tensors: a launch would be refused with another message ("device tensors only"); the refusal asked for comes first."""
    from proto_clip_amd import promptsrc
    from proto_clip_amd._lib import PclipError
    model, learner = small_learner(kw=TINY, depth_vision=2)
    head = promptsrc.PromptSRC(model, learner, torch.zeros(4, TINY["embed_dim"], dtype=torch.float16))
    model.unfreeze(**how)
    images, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    for call in (lambda: head.loss(images, labels), lambda: head.loss_terms(images, labels),
                 lambda: promptsrc.run_promptsrc({"promptsrc_epochs": 1}, images, labels, pr.names(4), (), model, learner=learner, fixed_text=head.fixed_text)):
        with pytest.raises(PclipError, match=r"PromptSRC: .*the teacher of the regularisers is the frozen\s+pre-trained model"):
            call()


# ---- the fixtures' own arithmetic ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pr.FIXTURES))
def test_fixture_terms_add_up_and_inputs_regenerate(name):
    meta = golden(name)
    tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed = pr.FIXTURES[name]
    assert (str(meta["tag"]), int(meta["sd_seed"]), int(meta["B"]), int(meta["N"]), int(meta["seed"])) == (tag, sd_seed, B, N, seed)
    assert float(meta["floor"]) == 0.0
    for chain in ("f64", "f16"):
        total = float(meta["ce_" + chain]) + pr.W_TEXT * float(meta["l_text_" + chain]) + pr.W_IMAGE * float(meta["l_image_" + chain]) \
            + pr.W_LOGITS / N * float(meta["kd_" + chain])
        assert abs(total - float(meta["loss_" + chain])) <= 1e-12 * abs(total)
    kw = pr.towers()[tag]
    ctx, vctx, tokens, teacher, images, labels = pr.fixture_inputs(kw, B, N, Pt, Dt, Pv, Dv, seed)
    assert meta["g_ctx_f64"].shape == tuple(ctx.shape) == (Dt, Pt, kw["transformer_width"])
    assert meta["g_vctx_f64"].shape == tuple(vctx.shape) == (Dv, Pv, kw["vision_width"])
    assert meta["img_f64"].shape == (B, kw["embed_dim"]) and meta["txt_f64"].shape == (N, kw["embed_dim"])
    assert len(meta["e_ref_ctx"]) == Dt and len(meta["e_ref_vctx"]) == Dv and min(meta["e_ref_ctx"].min(), meta["e_ref_vctx"].min()) > 0
    assert len(teacher) == len(pr.TEMPLATES) and not torch.equal(teacher[0], teacher[1])
    tok = pr.template_tokenizer(teacher, N)
    assert torch.equal(tok([pr.TEMPLATES[1].format("class2")])[0], teacher[1][2])
    assert bool((tokens[:, 1:1 + Pt] == 1).all()) and not bool((teacher[0][:, 1:1 + Pt] == 1).any())       # placeholders against real words


def test_float64_terms_identities():
    g = torch.Generator().manual_seed(1)
    img, txt = torch.randn(3, 64, generator=g, dtype=torch.float64), torch.randn(7, 64, generator=g, dtype=torch.float64)
    labels = torch.tensor([0, 3, 6])
    ce, l_text, l_image, kd = pr.terms64(img, txt, img * 3.0, pr.unit(txt), labels)          # the student IS the teacher (up to a row's length)
    assert float(l_text) < 1e-16 and float(l_image) < 1e-16 and abs(float(kd)) < 1e-15
    assert abs(float(ce) - float(coop_ref.loss64(img, txt, labels, pr.LOGIT_SCALE))) < 1e-15
    feats = [torch.randn(7, 64, generator=g, dtype=torch.float64) * s for s in (1.0, 5.0)]
    fixed = pr.fixed_text64(feats)
    assert torch.allclose(fixed.norm(dim=1), torch.ones(7, dtype=torch.float64), atol=1e-15)
    clip_way = pr.unit(torch.stack([pr.unit(f) for f in feats]).mean(0))                      # normalise, mean, normalise: NOT the convention
    assert float((fixed - clip_way).abs().max()) > 1e-2
