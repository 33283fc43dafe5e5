"""PromptSRC on the GPU (proto_clip_amd.promptsrc on autograd.feature_reg / cosine_kd / cosine_cross_entropy and the taped towers): the learner and the
four-term loss against the reference's own float64 autograd (fixtures of tests/golden/make_golden_promptsrc.py, graded at twice the reference's own
fp16-chain distance e_ref per depth slice and per feature matrix, no floor), the loss as the weighted sum of its terms, what a weight of 0 removes, the
equivalence with CoOp at depth 1, the frozen pass and its cached form, the passes per step, five steps of `run_promptsrc` against the reference's fp32
chain, the Gaussian aggregate of the epochs, and KgCoOp's loss on CoOp."""
import math

import pytest
import torch

import promptsrc_ref as pr
from conftest import golden, observe
from spec import trained_like_

pytestmark = pytest.mark.gpu

_MODELS = {}


def make_model(tag, sd_seed):
    """One model per (tower, seed), shared between the tests: PromptSRC never touches it."""
    if (tag, sd_seed) not in _MODELS:
        from proto_clip_amd.clip.model import build_model, random_state_dict
        sd = trained_like_(random_state_dict(seed=sd_seed, **pr.towers()[tag]), sd_seed)
        sd["logit_scale"] = torch.tensor(pr.LOGIT_SCALE, dtype=torch.float32)
        _MODELS[(tag, sd_seed)] = build_model(sd).cuda()
    return _MODELS[(tag, sd_seed)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def build(case, truncate=True):
    """(model, head, images, labels) of a case (tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed): the learner at the seeded parameters, the text target through
    `frozen_text_features` on the two templates' token rows."""
    from proto_clip_amd import promptsrc
    tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed = case
    kw = pr.towers()[tag]
    model = make_model(tag, sd_seed)
    ctx, vctx, tokens, teacher, images, labels = pr.fixture_inputs(kw, B, N, Pt, Dt, Pv, Dv, seed)
    learner = promptsrc.IndependentPromptLearner(pr.names(N), model, n_ctx_text=Pt, n_ctx_vision=Pv, depth_text=Dt, depth_vision=Dv,
                                                 tokenized_prompts=tokens, truncate=truncate)
    with torch.no_grad():
        learner.ctx.copy_(ctx.cuda())
        learner.vctx.copy_(vctx.cuda())
    fixed = promptsrc.frozen_text_features(pr.names(N), pr.TEMPLATES, model, tokenize=pr.template_tokenizer(teacher, N))
    return model, promptsrc.PromptSRC(model, learner, fixed), images.cuda(), labels.cuda(), teacher


def grads_of(head, loss, scale=1024.0):
    for p in head.learner.parameters():
        p.grad = None
    (loss * scale).backward()
    return [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in head.learner.parameters()]          # (a term that does not reach a tensor)


# ---- against the reference ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", list(pr.FIXTURES))
def test_learner_and_loss_against_the_reference(name, loss_scale):
    """Both feature matrices: ||f - f64|| / ||f64|| <= 2 e_ref.  Every depth slice of both gradients: ||g[d] - g_f64[d]|| / ||g_f64[d]|| <= 2 e_ref[d] (e_ref:
    the reference's own fp16 chain against its float64 run; no floor), the gradient of the 1024-fold loss divided back.  The total loss:
    |loss - loss_f64| <= 2 |loss_f16 - loss_f64|.  Taped and no_grad features are equal bit for bit; the text target is float64's within fp16's rounding.

    Measured on MI355X: features 0.49 - 0.76 of their bound, the total loss 0.31 - 0.60, the gradient slices 0.38 - 0.86.  The text L1 term's gradient is
    the SIGN of normalise(txt) - fixed_text, so it is as sensitive to the target's rounding as to the features': with a target rounded three times to fp16
    (the prototype kernel's mean, norm and quotient) `ctx[1]` of promptsrc_grad_small_t4d3_v4d3 lay at 1.27 — three of 2176 signs off float64's, the
    reference's own fp16 chain has one — and with `frozen_text_features`' single rounding it lies at 0.75."""
    meta = golden(name)
    assert float(meta["floor"]) == 0.0
    model, head, images, labels, teacher = build(pr.FIXTURES[name])
    learner = head.learner
    loss = head.loss(images, labels)
    (loss * loss_scale).backward()
    assert all(p.grad is None for p in model.parameters())
    with torch.no_grad():
        img, txt = learner.image_features(images), learner.text_features()
    taped_img, taped_txt = learner.image_features(images), learner.text_features()
    assert taped_img.requires_grad and taped_txt.requires_grad and taped_img.dtype == taped_txt.dtype == torch.float16
    assert torch.equal(bits(taped_img), bits(img)) and torch.equal(bits(taped_txt), bits(txt)) and not img.requires_grad
    worst = {}
    for key, f in (("img", img), ("txt", txt)):
        f64 = torch.from_numpy(meta[f"{key}_f64"]).double()
        worst[key] = float((f.double().cpu() - f64).norm() / f64.norm()) / (2 * float(meta[f"{key}_e_ref"]))
        observe(f"promptsrc {key} features: ||f - f64|| / ||f64|| / (2 e_ref)", worst[key], 1.0)
    for key, p, depth in (("ctx", learner.ctx, int(meta["Dt"])), ("vctx", learner.vctx, int(meta["Dv"]))):
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        g, g64 = p.grad.double().cpu() / loss_scale, torch.from_numpy(meta[f"g_{key}_f64"]).double()
        ratios = [float((g[d] - g64[d]).norm() / g64[d].norm()) / (2 * float(meta[f"e_ref_{key}"][d])) for d in range(depth)]
        worst[key] = max(ratios)
        for r in ratios:
            observe(f"promptsrc {key} gradient x{loss_scale:g}: ||g - g64|| / ||g64|| / (2 e_ref), per depth slice", r, 1.0)
        print(f"{name} x{loss_scale:g} {key}: gradient ratios " + " ".join(f"{r:.3f}" for r in ratios)
              + " (e_ref " + " ".join(f"{float(e):.3e}" for e in meta[f"e_ref_{key}"]) + ")")
    l64, l16 = float(meta["loss_f64"]), float(meta["loss_f16"])
    worst["loss"] = abs(float(loss.detach()) - l64) / (2 * abs(l16 - l64))
    observe("promptsrc total loss: |loss - f64| / (2 |fp16 chain - f64|)", worst["loss"], 1.0)
    with torch.no_grad():
        terms = [float(t) for t in head.loss_terms(images, labels)]
    print(f"{name} x{loss_scale:g}: loss {float(loss.detach()):.6f}, f64 {l64:.6f}, fp16 chain {l16:.6f}; terms "
          + " ".join(f"{k} {v:.6f} (f64 {float(meta[k + '_f64']):.6f})" for k, v in zip(("ce", "l_text", "l_image", "kd"), terms))
          + f"; ratios image {worst['img']:.3f} text {worst['txt']:.3f} loss {worst['loss']:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_frozen_text_features_is_mean_then_normalise():
    """Against float64 on the model's own per-template features: the mean of the UN-normalised rows, then one normalisation, rounded to fp16 ONCE — a row
    of norm 1 lies within 2^-11 of float64's (fp16's unit roundoff: half a unit in the last of 11 significand bits is at most 2^-11 of the element; 2^-25
    absolute for an element in fp16's subnormal range; 1e-6 for the fp32 mean and norm), and far from normalise-mean-normalise on rows of unequal length."""
    from proto_clip_amd import promptsrc
    case = pr.FIXTURES["promptsrc_grad_small_t4d3_v4d3"]
    model, head, images, labels, teacher = build(case)
    N = case[3]
    with torch.no_grad():
        per_template = [model.encode_text(t.cuda()) for t in teacher]
    want = pr.fixed_text64([f.cpu() for f in per_template])
    got = head.fixed_text
    assert got.dtype == torch.float16 and got.shape == (N, pr.towers()[case[0]]["embed_dim"]) and not got.requires_grad
    err = (got.double().cpu() - want).norm(dim=1)
    bound = 2.0 ** -11 + math.sqrt(got.shape[1]) * 2.0 ** -25 + 1e-6
    observe("frozen_text_features: row distance from float64 / (2^-11 + sqrt(E) 2^-25 + 1e-6)", float(err.max()) / bound, 1.0)
    assert float(err.max()) <= bound
    assert float((got.float().norm(dim=1) - 1).abs().max()) <= 2.0 ** -9
    one = promptsrc.frozen_text_features(pr.names(N), pr.TEMPLATES[:1], model, tokenize=pr.template_tokenizer(teacher, N))
    from proto_clip_amd import ops
    assert float((one.float() - ops.l2norm_rows(per_template[0]).float()).abs().max()) <= 2.0 ** -10          # one template: the normalised features


# ---- the loss and its terms --------------------------------------------------------------------------------------------------------------------------------

CASE = pr.FIXTURES["promptsrc_grad_small_t2d1_v5d3"]


def test_loss_is_the_weighted_sum_of_its_terms_and_a_zero_weight_removes_its_term():
    model, head, images, labels, _ = build(CASE)
    N = CASE[3]
    ce, l_text, l_image, kd = head.loss_terms(images, labels)
    total = head.loss(images, labels)
    assert torch.equal(total, ce + pr.W_TEXT * l_text + pr.W_IMAGE * l_image + (pr.W_LOGITS / N) * kd)
    assert torch.equal(head.loss(images, labels, w_text=3.0, w_image=0.5, w_logits=2.0), ce + 3.0 * l_text + 0.5 * l_image + (2.0 / N) * kd)
    full = grads_of(head, total)
    # the gradient of each term alone, and of the sums without one term: d(sum) is the sum autograd forms from the same per-term contributions
    for off, hand in ((dict(w_text=0.0), lambda t: t[0] + pr.W_IMAGE * t[2] + (pr.W_LOGITS / N) * t[3]),
                      (dict(w_image=0.0), lambda t: t[0] + pr.W_TEXT * t[1] + (pr.W_LOGITS / N) * t[3]),
                      (dict(w_logits=0.0), lambda t: t[0] + pr.W_TEXT * t[1] + pr.W_IMAGE * t[2])):
        got = grads_of(head, head.loss(images, labels, **off))
        want = grads_of(head, hand(head.loss_terms(images, labels)))
        assert all(torch.equal(a, b) for a, b in zip(got, want)), off
        assert not all(torch.equal(a, b) for a, b in zip(got, full)), off                # the term was pulling
    # the text term reaches ctx alone, the image term vctx alone
    g_text = grads_of(head, head.loss_terms(images, labels)[1])
    g_image = grads_of(head, head.loss_terms(images, labels)[2])
    assert bool(g_text[0].any()) and not bool(g_text[1].any()) and bool(g_image[1].any()) and not bool(g_image[0].any())


def test_all_weights_zero_is_the_plain_cross_entropy_bit_for_bit():
    from proto_clip_amd import autograd as pag
    model, head, images, labels, _ = build(CASE)
    got_loss = head.loss(images, labels, w_text=0.0, w_image=0.0, w_logits=0.0)
    got = grads_of(head, got_loss)
    learner = head.learner
    plain = pag.cosine_cross_entropy(learner.image_features(images), learner.text_features(), head.logit_scale(), labels=labels, normalize_a=True,
                                     normalize_b=True)
    want = grads_of(head, plain)
    assert torch.equal(got_loss, plain) and all(torch.equal(a, b) for a, b in zip(got, want))


def test_cached_frozen_features_give_the_same_bits_and_a_tensor_on_the_tape_is_refused():
    from proto_clip_amd._lib import PclipError
    model, head, images, labels, _ = build(CASE)
    cached = head.frozen_image_features(images)
    assert torch.equal(cached, model.encode_image(images)) and not cached.requires_grad
    a, b = head.loss(images, labels), head.loss(images, labels, zs_image_features=cached)
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(grads_of(head, a), grads_of(head, b)))
    with pytest.raises(PclipError, match="zs_image_features requires grad"):
        head.loss(images, labels, zs_image_features=cached.clone().requires_grad_(True))


def test_one_frozen_and_one_prompted_pass_per_step(monkeypatch):
    """Counted at the Python entries: per `loss` one frozen vision pass (encode_image), one prompted pass of each tower on the tape, the four loss calls; with
    cached frozen features no frozen pass; with the image and logit weights at 0 none either; per backward one walk of each tape."""
    from proto_clip_amd import autograd as pag, ops
    model, head, images, labels, _ = build(CASE)
    calls = {"frozen": 0, "tower_fwd": 0, "tower_bwd": 0, "vpt_embed": 0, "prompt_embed": 0, "freg": 0, "kd": 0, "ce": 0}

    def count(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(model, "encode_image", count("frozen", model.encode_image))
    monkeypatch.setattr(pag.TowerTailFn, "forward", staticmethod(count("tower_fwd", pag.TowerTailFn.forward)))
    monkeypatch.setattr(pag.TowerTailFn, "backward", staticmethod(count("tower_bwd", pag.TowerTailFn.backward)))
    monkeypatch.setattr(pag.VptEmbedFn, "forward", staticmethod(count("vpt_embed", pag.VptEmbedFn.forward)))
    monkeypatch.setattr(pag.PromptEmbedFn, "forward", staticmethod(count("prompt_embed", pag.PromptEmbedFn.forward)))
    monkeypatch.setattr(ops, "feature_reg", count("freg", ops.feature_reg))
    monkeypatch.setattr(ops, "cosine_kd", count("kd", ops.cosine_kd))
    monkeypatch.setattr(ops, "cosine_cross_entropy", count("ce", ops.cosine_cross_entropy))
    loss = head.loss(images, labels)
    assert calls == {"frozen": 1, "tower_fwd": 2, "tower_bwd": 0, "vpt_embed": 1, "prompt_embed": 1, "freg": 2, "kd": 1, "ce": 1}, calls
    (loss * 1024.0).backward()
    assert calls["tower_bwd"] == 2 and calls["tower_fwd"] == 2 and calls["frozen"] == 1, calls
    cached = head.frozen_image_features(images)
    before = dict(calls)
    head.loss(images, labels, zs_image_features=cached)
    assert calls["frozen"] == before["frozen"] and calls["tower_fwd"] == before["tower_fwd"] + 2, calls
    head.loss(images, labels, w_image=0.0, w_logits=0.0)
    assert calls["frozen"] == before["frozen"] and calls["freg"] == before["freg"] + 3 and calls["kd"] == before["kd"] + 1, calls


def test_depth_one_text_side_is_coop_bit_for_bit():
    from proto_clip_amd import coop
    case = pr.FIXTURES["promptsrc_grad_tiny_shallow"]
    model, head, images, labels, _ = build(case)
    learner = head.learner
    assert learner.depth_text == 1 and learner.depth_vision == 1
    theirs = coop.PromptLearner(pr.names(case[3]), model, n_ctx=case[4], tokenized_prompts=learner._text.tokenized_prompts.cpu())
    with torch.no_grad():
        theirs.ctx.copy_(learner.ctx[0])
        assert torch.equal(bits(learner.text_features()), bits(theirs()))
    assert torch.equal(bits(learner.text_features()), bits(theirs()))


def test_classify_is_the_dense_argmax_and_the_model_is_untouched():
    from proto_clip_amd import ops, utils
    model, head, images, labels, _ = build(CASE)
    with torch.no_grad():
        before = model.encode_image(images)
    grads_of(head, head.loss(images, labels))
    torch.optim.SGD(head.learner.parameters(), lr=0.01).step()
    assert torch.equal(model.encode_image(images), before) and not any(p.requires_grad for p in model.parameters())
    pred, rows = head.classify(images), head.text_rows()
    assert rows.dtype == torch.float16 and rows.shape == (CASE[3], pr.towers()[CASE[0]]["embed_dim"]) and not rows.requires_grad
    with torch.no_grad():
        dense = utils.clip_logits(ops.l2norm_rows(head.learner.image_features(images)), rows, scale=float(head.logit_scale()), layout="nd")
    assert pred.dtype == torch.int64 and torch.equal(pred, dense.argmax(1))
    _, values, indices = head.classify(images, topk=2)
    assert torch.equal(indices[:, 0].long(), pred)


# ---- training ------------------------------------------------------------------------------------------------------------------------------------------------

def test_five_steps_of_run_promptsrc_lower_the_loss_and_the_parameters_are_the_gaussian_sum():
    """promptsrc_ref.SGD_CASE: TINY, 8 images in one batch, SGD on the two tensors with momentum 0.9 at learning rate 0.03 under a cosine schedule over the
    five steps, loss scale 1024, upstream's weights.  The reference's fp32 chain with the same step rule (`make_golden_promptsrc.py sgd`, stored in
    promptsrc_sgd_tiny.npz) lowers the total loss by `decrease`; at least half of that is required of the five training steps here (the Gaussian of mean 5
    and deviation 1 then mixes the epochs; the aggregate's own loss is printed).  The parameters afterwards are the Gaussian-weighted sum of the recorded
    per-epoch snapshots within (E + 1) u sum |w theta|."""
    from proto_clip_amd import promptsrc
    want = golden(pr.SGD_FIXTURE)
    tag, sd_seed, B, N, Pt, Dt, Pv, Dv, seed, lr = pr.SGD_CASE
    assert float(want["lr"]) == lr and int(want["seed"]) == seed and str(want["tag"]) == tag
    model, head, images, labels, _ = build(pr.SGD_CASE[:9])
    cfg = {"promptsrc_epochs": 5, "promptsrc_batch": B, "promptsrc_lr": lr, "promptsrc_loss_scale": 1024.0, "seed": seed, "gpa_mean": 5, "gpa_std": 1}
    snapshots = []
    learner, losses = promptsrc.run_promptsrc(cfg, images, labels, head.learner.classnames, pr.TEMPLATES, model, learner=head.learner,
                                              fixed_text=head.fixed_text, snapshots=snapshots)
    assert learner is head.learner and len(losses) == 5 and len(snapshots) == 5 and all(math.isfinite(v) for v in losses)
    w = promptsrc.gpa_weights(5, 5, 1)
    for i, p in enumerate((learner.ctx, learner.vctx)):
        want_p, mag = pr.gpa_sum64(w, [s[i].cpu() for s in snapshots])
        err = (p.detach().double().cpu() - want_p).abs()
        ratio = float((err / (6 * 2.0 ** -24 * mag)).max())
        observe("run_promptsrc: |parameter - float64 Gaussian sum| / ((E + 1) u sum |w theta|)", ratio, 1.0)
        assert ratio <= 1.0, ratio
    with torch.no_grad():
        aggregate = float(head.loss(images, labels))
        for p, s in zip((learner.ctx, learner.vctx), snapshots[-1]):
            p.copy_(s)                                                   # the parameters after the fifth step
        final = float(head.loss(images, labels))
    ref = [float(v) for v in want["losses"]]
    print("run_promptsrc loss over five SGD steps:", " ".join(f"{v:.6f}" for v in losses), f"-> {final:.6f}; decrease {losses[0] - final:.6f}; the aggregate's "
          f"loss {aggregate:.6f}", "(reference fp32 chain:", " ".join(f"{v:.6f}" for v in ref), f"decrease {float(want['decrease']):.6f})")
    observe("run_promptsrc: half the reference's five-step decrease / the decrease here", 0.5 * float(want["decrease"]) / max(losses[0] - final, 1e-9), 1.0)
    assert losses[0] - final >= 0.5 * float(want["decrease"]), (losses, final)
    assert aggregate < losses[0]


# ---- KgCoOp on CoOp ------------------------------------------------------------------------------------------------------------------------------------------

def test_kg_loss_is_the_cross_entropy_plus_eight_times_the_cosine_term_bit_for_bit():
    from proto_clip_amd import autograd as pag, coop
    case = pr.FIXTURES["promptsrc_grad_small_t4d3_v4d3"]
    model, head, images, labels, _ = build(case)
    N, Pt = case[3], case[4]
    learner = coop.PromptLearner(pr.names(N), model, n_ctx=Pt, tokenized_prompts=head.learner._text.tokenized_prompts.cpu())
    student = coop.CoOp(model, learner)
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(12, pr.towers()[case[0]]["embed_dim"], generator=g).half().cuda()
    y = torch.randint(0, N, (12,), generator=g).cuda()
    got = student.kg_loss(feats, y, head.fixed_text)
    text = learner()
    ce = student.loss(feats, y)
    cos = pag.feature_reg(text, head.fixed_text, "cos", True)
    assert torch.equal(got, ce + 8.0 * cos) and float(cos.detach()) > 0
    learner.ctx.grad = None
    (got * 1024.0).backward()
    g_got = learner.ctx.grad.clone()
    learner.ctx.grad = None
    text = learner()
    both = pag.cosine_cross_entropy(feats, text, student.logit_scale(), labels=y, normalize_a=True, normalize_b=True) + 8.0 * pag.feature_reg(text, head.fixed_text,
                                                                                                                                      "cos", True)
    (both * 1024.0).backward()
    assert torch.equal(g_got, learner.ctx.grad) and bool(g_got.any())
    assert torch.equal(student.kg_loss(feats, y, head.fixed_text, weight=2.0), ce + 2.0 * cos)
