"""CoOp on the GPU (proto_clip_amd.coop, autograd.PromptEmbedFn / TowerTailFn with a differentiable input, csrc/pclip_prompt.hip): the two kernels bit for bit
against their CPU restatement (tests/coop_ref.py), the assembled prompts through the tower against `encode_text`'s bits, the tower truncated to L_eff, the
context gradient against the reference's own float64 autograd (fixtures of tests/golden/make_golden_coop.py, graded at twice the reference's own fp16-chain
distance e_ref, no floor), what a frozen tower pays for, training, and the refusals."""
import math

import numpy as np
import pytest
import torch

import coop_ref
import cosine_ce_ref
from conftest import golden, observe
from spec import E2E, ODD, SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

TOWERS = {"tiny": TINY, "small": SMALL, "odd": ODD}
FIXTURES = ["coop_grad_tiny_shared", "coop_grad_tiny_specific", "coop_grad_small_shared", "coop_grad_small_specific"]
LENGTHS = (6, 32, 33, 65, 77)


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(math.log(20.0), dtype=torch.float32)
    return build_model(sd).cuda()


def names(n):
    return [f"class{i}" for i in range(n)]


# ---- the kernels against the CPU restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("class_specific", [False, True], ids=["shared", "specific"])
@pytest.mark.parametrize("W", [72, 512])
def test_kernels_match_the_cpu_restatement_bit_for_bit(W, class_specific):
    """Forward and context gradient for n_ctx in (1, 4, 16), N in (1, 7, 130) (130: nine class slices, the last of two classes) and L_out in (6, 77), with
    token ids outside the vocabulary on both sides.  n_ctx = 16 at L_out = 6 cuts the context itself: the rows that remain are assembled, the others get a
    zero gradient."""
    from proto_clip_amd import ops
    vocab = 200
    g = torch.Generator().manual_seed(W + class_specific)
    emb16 = (torch.randn(vocab, W, generator=g) * 0.02).half()
    pos16 = (torch.randn(77, W, generator=g) * 0.01).half()
    for n_ctx in (1, 4, 16):
        for N in (1, 7, 130):
            ctx = torch.randn(*((N, n_ctx, W) if class_specific else (n_ctx, W)), generator=g) * 0.02
            tokens = coop_ref.prompt_tokens(N, n_ctx, vocab, 11 * N + n_ctx)
            tokens[0, 40], tokens[N - 1, 30], tokens[N // 2, 5 if n_ctx < 5 else 20] = -3, vocab + 100, 2 ** 40
            for L_out in (6, 77):
                x = ops.prompt_embed(ctx.cuda(), tokens.cuda(), emb16.cuda(), pos16.cuda(), L_out)
                want = coop_ref.prompt_embed(ctx, tokens, emb16, pos16, L_out)
                assert x.shape == want.shape and torch.equal(x.cpu(), want), (n_ctx, N, L_out)
                scale = torch.logspace(-4, 0, N * L_out)[torch.randperm(N * L_out, generator=g)][:, None]
                dx = (torch.randn(N * L_out, W, generator=g) * scale).half()
                got = ops.prompt_ctx_grad(dx.cuda(), N, L_out, n_ctx, class_specific)
                ref = coop_ref.prompt_ctx_grad(dx, N, L_out, n_ctx, class_specific)
                assert got.dtype == torch.float32 and got.shape == ref.shape and torch.equal(got.cpu(), ref), (n_ctx, N, L_out)
                again = ops.prompt_ctx_grad(dx.cuda(), N, L_out, n_ctx, class_specific)
                assert torch.equal(again, got)


def test_context_gradient_is_the_row_walk_at_offset_one():
    """pclip_prompt_ctx_grad_f32 and pclip_rows_grad_f32 are one walk (csrc/pclip_rows.h): the shared context's gradient has the bits of `rows_grad` at
    off = 1, the class-specific one is the rows themselves, and neither writes the stream.  N = 1, 16, 17, 33: one slice, a full slice, one and two slice
    boundaries crossed; W = 72 is no multiple of 64."""
    from proto_clip_amd import ops
    L_out, n_ctx, W = 6, 4, 72
    g = torch.Generator().manual_seed(72)
    for N in (1, 16, 17, 33):
        dx = torch.randn(N * L_out, W, generator=g).half().cuda()
        before = dx.clone()
        assert torch.equal(ops.prompt_ctx_grad(dx, N, L_out, n_ctx), ops.rows_grad(dx, N, L_out, 1, n_ctx)), N
        assert torch.equal(ops.prompt_ctx_grad(dx, N, L_out, n_ctx, class_specific=True), dx.view(N, L_out, W)[:, 1:1 + n_ctx].float()), N
        assert torch.equal(dx, before), N


def test_fp16_exact_context_rows_give_text_embed_bits():
    from proto_clip_amd import ops
    vocab, W, N, n_ctx = 300, 128, 9, 4
    g = torch.Generator().manual_seed(2)
    emb16 = (torch.randn(vocab, W, generator=g) * 0.02).half().cuda()
    pos16 = (torch.randn(77, W, generator=g) * 0.01).half().cuda()
    tokens = coop_ref.prompt_tokens(N, n_ctx, vocab, 3).cuda()
    ids = torch.randint(2, vocab - 2, (N, n_ctx), generator=g).cuda()
    real = tokens.clone()
    real[:, 1:1 + n_ctx] = ids
    assert torch.equal(ops.prompt_embed(emb16[ids].float(), tokens, emb16, pos16), ops.text_embed(real, emb16, pos16))
    real[:, 1:1 + n_ctx] = ids[0]
    assert torch.equal(ops.prompt_embed(emb16[ids[0]].float(), tokens, emb16, pos16), ops.text_embed(real, emb16, pos16))
    from proto_clip_amd._lib import PclipError
    with pytest.raises(PclipError, match="float32"):
        ops.prompt_embed(emb16[ids[0]], tokens, emb16, pos16)


# ---- the same bits as encode_text --------------------------------------------------------------------------------------------------------------------

def real_id_learner(model, kw, N, n_ctx, class_specific, seed, **kwargs):
    """A PromptLearner whose context holds the embeddings of real token ids, and the token matrix with those ids in place of the placeholders."""
    from proto_clip_amd import coop
    tokens = coop_ref.prompt_tokens(N, n_ctx, kw["vocab_size"], seed)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, kw["vocab_size"] - 2, (N, n_ctx) if class_specific else (n_ctx,), generator=g)
    real = tokens.clone()
    real[:, 1:1 + n_ctx] = ids
    learner = coop.PromptLearner(names(N), model, n_ctx=n_ctx, class_specific=class_specific, tokenized_prompts=tokens, **kwargs).cuda()
    with torch.no_grad():
        learner.ctx.copy_(model.token_embedding.weight[ids.cuda()].float())
    return learner, real.cuda()


@pytest.mark.parametrize("class_specific", [False, True], ids=["shared", "specific"])
@pytest.mark.parametrize("tag", list(TOWERS))
def test_real_token_rows_give_the_bits_of_encode_text(tag, class_specific):
    kw = TOWERS[tag]
    model = make_model(kw, 9)
    learner, real = real_id_learner(model, kw, 5, 4, class_specific, 7, truncate=False)
    with torch.no_grad():
        want = model.encode_text(real)
        untaped = learner()
    assert not untaped.requires_grad and untaped.grad_fn is None and torch.equal(untaped, want)
    taped = learner()
    assert taped.requires_grad and taped.dtype == torch.float16 and torch.equal(taped.detach(), want)
    learner.ctx.requires_grad_(False)                                        # nothing trainable: grad mode on builds no tape
    frozen = learner()
    assert not frozen.requires_grad and torch.equal(frozen, want)


# ---- truncation ---------------------------------------------------------------------------------------------------------------------------------------

def fixture_case(name):
    """(meta, model, ctx, tokens, image features, labels) of a reference fixture, the inputs regenerated from its seeds."""
    meta = golden(name)
    kw = TOWERS[str(meta["tag"])]
    assert float(meta["floor"]) == 0.0
    l_eff = int(meta["l_eff"]) or None
    ctx, tokens, feats, labels = coop_ref.fixture_inputs(kw, int(meta["N"]), int(meta["n_ctx"]), int(meta["Q"]), int(meta["seed"]), bool(meta["class_specific"]),
                                                        l_eff)
    assert torch.equal(tokens, torch.from_numpy(meta["tokens"]))
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = trained_like_(random_state_dict(seed=int(meta["sd_seed"]), **kw), int(meta["sd_seed"]))
    sd["logit_scale"] = torch.tensor(float(meta["logit_scale"]), dtype=torch.float32)
    return meta, build_model(sd).cuda(), ctx, tokens, feats.cuda(), labels.cuda()


def graded_run(meta, model, ctx, tokens, feats, labels, truncate, loss_scale=1.0):
    """One taped step of CoOp.loss: (text features, loss, ctx.grad, gradient ratio to 2 e_ref, feature ratio to 2 text_e_ref, learner, float64 loss of the
    text features, CoOp.loss against the float64 helper of the cosine cross-entropy kernel in units of its derived tolerance)."""
    from proto_clip_amd import coop, ops
    learner = coop.PromptLearner(names(tokens.shape[0]), model, n_ctx=int(meta["n_ctx"]), class_specific=bool(meta["class_specific"]),
                                 tokenized_prompts=tokens, truncate=truncate).cuda()
    with torch.no_grad():
        learner.ctx.copy_(ctx.cuda())
    head = coop.CoOp(model, learner)
    loss = head.loss(feats, labels)
    (loss * loss_scale).backward()
    with torch.no_grad():
        text = learner()
    g = learner.ctx.grad.double().cpu() / loss_scale
    assert learner.ctx.grad.dtype == torch.float32 and learner.ctx.grad.shape == learner.ctx.shape
    g64, t64 = torch.from_numpy(meta["g_f64"]).double(), torch.from_numpy(meta["text_f64"]).double()
    g_ratio = float((g - g64).norm() / g64.norm()) / (2 * float(meta["e_ref"]))
    t_ratio = float((text.double().cpu() - t64).norm() / t64.norm()) / (2 * float(meta["text_e_ref"]))
    loss_feat = float(coop_ref.loss64(feats, text, labels, float(meta["logit_scale"])))
    # the kernel's own function: the cross-entropy over the fp16 unit rows ops.l2norm_rows delivers (tests/cosine_ce_ref.py), under its derived tolerance
    ref = cosine_ce_ref.reference(feats, text, float(head.logit_scale()), labels, False, True, True, a_unit16=ops.l2norm_rows(feats), b_unit16=ops.l2norm_rows(text))
    k_ratio = cosine_ce_ref.worst_ratio(loss.detach(), ref["loss"], ref["tol_loss"])
    return text, float(loss.detach()), learner.ctx.grad.clone(), g_ratio, t_ratio, learner, loss_feat, k_ratio


@pytest.mark.parametrize("l_eff", LENGTHS)
def test_truncated_tower_passes_the_full_length_grading(l_eff):
    """Prompts whose largest EOT position + 1 is l_eff (either side of the attention's 32-key tiles, and the untruncated limit): the run at l_eff tokens and the
    run at 77 both meet the float64 grading of features and context gradient, and they agree bit for bit — the causal walk of a query stops at its own key
    tile and GEMM / LayerNorm rows are independent, so the leading positions do not see the cut (measured on MI355X before it was asserted: 0 differing
    elements of features and ctx.grad at every length)."""
    meta, model, ctx, tokens, feats, labels = fixture_case(f"coop_grad_small_len{l_eff}")
    full = graded_run(meta, model, ctx, tokens, feats, labels, truncate=False)
    cut = graded_run(meta, model, ctx, tokens, feats, labels, truncate=True)
    assert full[5].run_length == 77 and cut[5].run_length == cut[5].l_eff == l_eff
    for tag, (text, loss, grad, g_ratio, t_ratio, _, _, _) in (("77 tokens", full), ("L_eff", cut)):
        print(f"L_eff {l_eff} at {tag}: loss {loss:.6f} (f64 {float(meta['loss_f64']):.6f})  gradient ratio {g_ratio:.3f}  feature ratio {t_ratio:.3f}")
        observe(f"coop truncation, {tag}: ||g - g64|| / ||g64|| / (2 e_ref)", g_ratio, 1.0)
        observe(f"coop truncation, {tag}: ||t - t64|| / ||t64|| / (2 e_ref)", t_ratio, 1.0)
        assert g_ratio <= 1.0 and t_ratio <= 1.0, (tag, g_ratio, t_ratio)
    d_text = float((full[0] != cut[0]).float().mean())
    d_grad = float((full[2] != cut[2]).float().mean())
    print(f"L_eff {l_eff}: truncated vs full length — features differ in {d_text:.4f} of the elements, ctx.grad in {d_grad:.4f}")
    observe("coop truncation: fraction of feature elements that differ from the 77-token run", d_text, 1.0)
    observe("coop truncation: fraction of ctx.grad elements that differ from the 77-token run", d_grad, 1.0)
    assert torch.equal(full[0], cut[0]) and torch.equal(full[2], cut[2])


# ---- the context gradient against the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_context_gradient_against_the_reference(name, loss_scale):
    """||g - g_f64|| / ||g_f64|| <= 2 e_ref at both `truncate` settings (e_ref: the reference's fp16 chain against its float64 run; no floor), the gradient of
    the 1024-fold loss divided back.

    The loss: as in test_gpu_tower_backward.py, the float64 loss of the delivered features is within 2 |loss_f16 - loss_f64| + 1e-4 of loss_f64.  The value
    CoOp.loss itself returns is a different function of those features: pclip_cosine_ce_f16 takes the fp16-ROUNDED unit rows as its operands by definition
    (include/pclip.h), the fixtures normalise in float64.  It is asserted against the kernel's float64 helper under that helper's derived tolerance, and its
    distance from loss_f64 is recorded: on MI355X at most 1.35 of the features' slack (coop_grad_tiny_shared: |1.774907 - 1.774627| = 2.80e-4 against
    2.07e-4; the other fixtures are inside), the excess being the 2^-11 rounding of the unit rows under a scale of 20."""
    meta, model, ctx, tokens, feats, labels = fixture_case(name)
    worst = 0.0
    for truncate in (True, False):
        _, loss, _, g_ratio, t_ratio, _, loss_feat, k_ratio = graded_run(meta, model, ctx, tokens, feats, labels, truncate, loss_scale)
        l64 = float(meta["loss_f64"])
        slack = 2 * abs(float(meta["loss_f16"]) - l64) + 1e-4
        print(f"{name} x{loss_scale:g} truncate={truncate}: float64 loss of the features {loss_feat:.6f}, CoOp.loss {loss:.6f}, f64 {l64:.6f} (slack {slack:.2e});"
              f" CoOp.loss / kernel tolerance {k_ratio:.3f};  gradient ratio {g_ratio:.3f}  e_ref {float(meta['e_ref']):.3e}  feature ratio {t_ratio:.3f}")
        observe(f"coop context gradient x{loss_scale:g}: ||g - g64|| / ||g64|| / (2 e_ref)", g_ratio, 1.0)
        observe("coop loss of the features (float64): |loss - loss_f64| / (2 |loss_f16 - loss_f64| + 1e-4)", abs(loss_feat - l64) / slack, 1.0)
        observe("coop CoOp.loss (fp16 unit rows), recorded: |loss - loss_f64| / (2 |loss_f16 - loss_f64| + 1e-4)", abs(loss - l64) / slack, 1.0)
        observe("coop CoOp.loss: |loss - float64 helper| / derived tolerance", k_ratio, 1.0)
        observe("coop text features: ||t - t64|| / ||t64|| / (2 e_ref)", t_ratio, 1.0)
        assert abs(loss_feat - l64) <= slack, (loss_feat, l64, slack)
        assert k_ratio <= 1.0, k_ratio
        assert t_ratio <= 1.0, t_ratio
        worst = max(worst, g_ratio)
    assert worst <= 1.0, worst


# ---- a frozen tower pays for no parameter gradient ------------------------------------------------------------------------------------------------------

def test_frozen_tower_issues_no_parameter_gradient(monkeypatch):
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import coop
    model = make_model(SMALL, 5)
    N, n_ctx = 6, 4
    tokens = coop_ref.prompt_tokens(N, n_ctx, SMALL["vocab_size"], 4)
    learner = coop.PromptLearner(names(N), model, n_ctx=n_ctx, tokenized_prompts=tokens).cuda()
    head = coop.CoOp(model, learner)
    g = torch.Generator().manual_seed(1)
    feats, labels = torch.randn(12, SMALL["embed_dim"], generator=g).half().cuda(), torch.randint(0, N, (12,), generator=g).cuda()
    calls = {"w": 0, "b": 0}
    keep_w, keep_b = pag._weight_grad, pag._bias_grad

    def count_w(dy, x):
        calls["w"] += 1
        return keep_w(dy, x)

    def count_b(dy):
        calls["b"] += 1
        return keep_b(dy)

    monkeypatch.setattr(pag, "_weight_grad", count_w)
    monkeypatch.setattr(pag, "_bias_grad", count_b)
    head.loss(feats, labels).backward()
    assert calls == {"w": 0, "b": 0}
    assert learner.ctx.grad is not None and bool(learner.ctx.grad.any()) and bool(torch.isfinite(learner.ctx.grad).all())
    assert all(p.grad is None for p in model.parameters())
    frozen_grad = learner.ctx.grad.clone()
    # the last block and the heads unfrozen beside the context: their tensors and nothing else receive a gradient; the context's keeps its bits
    learner.ctx.grad = None
    model.unfreeze(text_blocks=1)
    head.loss(feats, labels).backward()
    last = len(model.transformer.resblocks) - 1
    want = {n for n, _ in model.named_parameters() if n.startswith((f"transformer.resblocks.{last}.", "ln_final.")) or n == "text_projection"}
    assert calls == {"w": 4, "b": 4}                                          # the four linears of one block
    for n, p in model.named_parameters():
        if n in want:
            assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape and bool(p.grad.any()), n
        else:
            assert p.grad is None, n
    assert torch.equal(learner.ctx.grad, frozen_grad)


# ---- training ---------------------------------------------------------------------------------------------------------------------------------------------

def test_five_sgd_steps_lower_the_loss():
    from proto_clip_amd import coop
    model = make_model(SMALL, 6)
    N, n_ctx = 8, 4
    learner = coop.PromptLearner(names(N), model, n_ctx=n_ctx, tokenized_prompts=coop_ref.prompt_tokens(N, n_ctx, SMALL["vocab_size"], 8)).cuda()
    head = coop.CoOp(model, learner)
    g = torch.Generator().manual_seed(2)
    feats, labels = torch.randn(32, SMALL["embed_dim"], generator=g).half().cuda(), torch.randint(0, N, (32,), generator=g).cuda()
    opt = torch.optim.SGD(learner.parameters(), lr=0.002, momentum=0.9)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)                    # fp32 ctx and gradient: torch's optimizer and scaler work unchanged
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = head.loss(feats, labels)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(head.loss(feats, labels)))
    print("CoOp loss over five SGD steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_run_coop_on_a_synthetic_split_and_classify():
    """The trainer on cached synthetic features with the real tokenizer (spec.E2E: the SMALL towers with CLIP's vocabulary): the accuracy after training is no
    lower than at the `ctx_init` start, and `classify` is the arg-max of the dense fp16 logits on the learned rows."""
    from proto_clip_amd import coop, ops, synth, utils
    model = make_model(E2E, 17, trained=False)
    classnames = ["airplane", "tabby_cat", "golden_retriever", "oak_tree", "fire_truck", "coffee_mug"]
    N, K, D = len(classnames), 8, E2E["embed_dim"]
    split = synth.make_split(N, K, D, 8, 96, seed=5, sigma=0.5)
    train_f = split.visual_memory_keys.t().contiguous().cuda()
    train_y = torch.arange(N).repeat_interleave(K).cuda()
    test_f, test_y = split.test_features.cuda(), split.test_labels.cuda()
    cfg = {"coop_epochs": 10, "n_ctx": 16, "ctx_init": "a photo of a"}
    head = coop.run_coop(cfg, train_f, train_y, test_f, test_y, classnames, model)
    res = head.results
    assert isinstance(head, coop.CoOp) and head.prompt_learner.n_ctx == 4 and len(res["epochs"]) == 10
    print("run_coop: start %.2f -> %.2f, losses %s" % (res["start_test_acc"], res["test_acc"], " ".join(f"{e['loss']:.3f}" for e in res["epochs"])))
    assert res["test_acc"] >= res["start_test_acc"] and res["epochs"][-1]["loss"] < res["epochs"][0]["loss"]
    rows = head.text_rows()
    assert rows.shape == (N, D) and rows.dtype == torch.float16 and not rows.requires_grad
    dense = utils.clip_logits(test_f, rows, scale=float(head.logit_scale()), layout="nd")
    pred, tv, ti = head.classify(test_f, topk=3)
    assert torch.equal(pred, dense.argmax(1)) and torch.equal(head.classify(test_f), pred)
    assert torch.equal(ti[:, 0], pred) and torch.equal(tv, dense.topk(3, dim=1).values)
    assert 100.0 * float((pred == test_y).float().mean()) == pytest.approx(res["test_acc"])


# ---- refusals on the device path --------------------------------------------------------------------------------------------------------------------------

def test_refusals_on_the_device_path():
    from proto_clip_amd import coop, ops
    from proto_clip_amd._lib import PclipError
    model = make_model(TINY, 5)
    learner = coop.PromptLearner(names(3), model, n_ctx=2, tokenized_prompts=coop_ref.prompt_tokens(3, 2, TINY["vocab_size"], 4)).cuda()
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            learner()
        with torch.no_grad():                                                # the untaped pass has no such limit
            assert learner().shape == (3, TINY["embed_dim"])
    model.positional_embedding.requires_grad_(True)
    with pytest.raises(PclipError, match="positional_embedding"):
        learner()
    model.positional_embedding.requires_grad_(False)
    model.token_embedding.weight.requires_grad_(True)
    with pytest.raises(PclipError, match=r"token_embedding\.weight"):
        learner()
    model.token_embedding.weight.requires_grad_(False)
    assert learner().requires_grad
