"""ProGrad on the GPU (proto_clip_amd.prograd on autograd.cosine_kd / cosine_cross_entropy and the taped text tower): the two context gradients and their
projection against the reference's own float64 autograd (fixtures of tests/golden/make_golden_prograd.py, each graded at twice the reference's own
fp16-chain distance e_ref, no floor) with float64's branch; the second walk of the one tape against a walk of a fresh tape, bit for bit; one tower forward
for both losses; five steps of `run_prograd` against the reference's fp32 chain."""
import math

import pytest
import torch

import prograd_ref as pr
from conftest import golden, observe
from spec import SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

TOWERS = {"tiny": TINY, "small": SMALL}


def names(n):
    return [f"class{i}" for i in range(n)]


_MODELS = {}


def fixture_case(name):
    """(meta, model, ctx, tokens, image features, labels, teacher rows) of a reference fixture, the inputs regenerated from its seeds."""
    meta = golden(name)
    kw = TOWERS[str(meta["tag"])]
    assert float(meta["floor"]) == 0.0 and float(meta["lam"]) == pr.LAM
    ctx, tokens, _, feats = pr.fixture_inputs(kw, int(meta["N"]), int(meta["n_ctx"]), int(meta["Q"]), int(meta["seed"]))
    assert torch.equal(tokens, torch.from_numpy(meta["tokens"]))
    key = (str(meta["tag"]), int(meta["sd_seed"]))
    if key not in _MODELS:
        from proto_clip_amd.clip.model import build_model, random_state_dict
        sd = trained_like_(random_state_dict(seed=int(meta["sd_seed"]), **kw), int(meta["sd_seed"]))
        sd["logit_scale"] = torch.tensor(float(meta["logit_scale"]), dtype=torch.float32)
        _MODELS[key] = build_model(sd).cuda()
    return meta, _MODELS[key], ctx, tokens, feats.cuda(), torch.from_numpy(meta["labels"]).cuda(), torch.from_numpy(meta["teacher"]).cuda()


def prograd_of(meta, model, ctx, tokens, teacher):
    from proto_clip_amd import coop, prograd
    learner = coop.PromptLearner(names(tokens.shape[0]), model, n_ctx=int(meta["n_ctx"]), tokenized_prompts=tokens).cuda()
    with torch.no_grad():
        learner.ctx.copy_(ctx.cuda())
    return prograd.ProGrad(model, learner, teacher, lam=pr.LAM)


def rel(got, want):
    got, want = got.double().cpu(), want.double()
    return float((got - want).norm() / want.norm())


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("name", list(pr.FIXTURES))
def test_two_gradients_and_the_projection_against_the_reference(name, loss_scale):
    """||x - x_f64|| / ||x_f64|| <= 2 e_ref for g_ce, g_kl and the projected gradient (the gradients of the 1024-fold losses divided back), and the branch
    float64 took.  The fixtures are decided cases (|cos_f64| >= 0.1, the reference's fp16 chain on float64's branch): none is skipped."""
    meta, model, ctx, tokens, feats, labels, teacher = fixture_case(name)
    head = prograd_of(meta, model, ctx, tokens, teacher)
    ce, kl = head.losses(feats, labels)
    params = [head.prompt_learner.ctx]
    g_ce = torch.autograd.grad(ce * loss_scale, params, retain_graph=True)[0]
    g_kl = torch.autograd.grad(kl * loss_scale, params, retain_graph=True)[0]
    head.backward(ce, kl, scale=loss_scale)
    g = head.prompt_learner.ctx.grad
    assert g.dtype == torch.float32 and g.shape == ctx.shape
    conflict = not torch.equal(g, g_ce)
    cos = float((g_ce * g_kl).sum() / (g_ce.norm() * g_kl.norm()))
    ratios = {}
    for key, got, e in (("g_ce", g_ce, "e_ref_ce"), ("g_kl", g_kl, "e_ref_kl"), ("g", g, "e_ref")):
        ratios[key] = rel(got / loss_scale, torch.from_numpy(meta[key + "_f64"])) / (2 * float(meta[e]))
        observe(f"prograd {key} x{loss_scale:g}: ||x - x64|| / ||x64|| / (2 e_ref)", ratios[key], 1.0)
    print(f"{name} x{loss_scale:g}: ce {float(ce.detach()):.6f} (f64 {float(meta['loss_ce_f64']):.6f}) kl {float(kl.detach()):.6f} (f64 {float(meta['loss_kl_f64']):.6f})  cos {cos:+.4f}"
          f" (f64 {float(meta['cos_f64']):+.4f})  conflict {conflict} (f64 {bool(meta['conflict'])})  ratios", {k: round(v, 3) for k, v in ratios.items()})
    assert conflict == bool(meta["conflict"])
    assert max(ratios.values()) <= 1.0, ratios


def test_second_walk_of_the_tape_gives_the_bits_of_a_fresh_walk():
    """TowerTailFn and PromptEmbedFn keep their tape and recompute what they need: d kl / d ctx walked second, after d ce / d ctx with retain_graph, equals
    d kl / d ctx walked alone on a new forward, and walking ce twice gives the same bits twice."""
    meta, model, ctx, tokens, feats, labels, teacher = fixture_case("prograd_grad_small_derange")
    head = prograd_of(meta, model, ctx, tokens, teacher)
    p = [head.prompt_learner.ctx]
    ce, kl = head.losses(feats, labels)
    first_ce = torch.autograd.grad(ce * 1024.0, p, retain_graph=True)[0]
    second_kl = torch.autograd.grad(kl * 1024.0, p, retain_graph=True)[0]
    again_ce = torch.autograd.grad(ce * 1024.0, p)[0]
    ce2, kl2 = head.losses(feats, labels)
    fresh_kl = torch.autograd.grad(kl2 * 1024.0, p)[0]
    ce3, _ = head.losses(feats, labels)
    fresh_ce = torch.autograd.grad(ce3 * 1024.0, p)[0]
    assert torch.equal(ce, ce2) and torch.equal(kl, kl2)
    assert torch.equal(second_kl, fresh_kl) and torch.equal(first_ce, fresh_ce) and torch.equal(again_ce, first_ce)
    assert float(second_kl.abs().max()) > 0 and float(first_ce.abs().max()) > 0


def test_losses_share_one_tower_forward(monkeypatch):
    """Counted at the Python entries: one prompt assembly and one taped tower walk per `losses`, two backward walks of it per `backward`."""
    from proto_clip_amd import autograd as pag, ops
    meta, model, ctx, tokens, feats, labels, teacher = fixture_case("prograd_grad_tiny_derange")
    head = prograd_of(meta, model, ctx, tokens, teacher)
    calls = {"embed": 0, "tower_fwd": 0, "tower_bwd": 0}
    embed, fwd, bwd = ops.prompt_embed, pag.TowerTailFn.forward, pag.TowerTailFn.backward

    def count(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, "prompt_embed", count("embed", embed))
    monkeypatch.setattr(pag.TowerTailFn, "forward", staticmethod(count("tower_fwd", fwd)))
    monkeypatch.setattr(pag.TowerTailFn, "backward", staticmethod(count("tower_bwd", bwd)))
    ce, kl = head.losses(feats, labels)
    assert calls == {"embed": 1, "tower_fwd": 1, "tower_bwd": 0}, calls
    head.backward(ce, kl, scale=1024.0)
    assert calls == {"embed": 1, "tower_fwd": 1, "tower_bwd": 2}, calls
    assert head.prompt_learner.ctx.grad is not None


def test_five_steps_of_run_prograd_lower_the_cross_entropy():
    """prograd_ref.SGD_CASE: TINY, the deranged labels, all 12 samples in one batch, SGD with momentum 0.9 under a cosine schedule over five steps, loss scale
    1024, lambda 1.  The reference's fp32 chain with the same step rule (tests/golden/make_golden_prograd.py, stored in prograd_sgd_tiny.npz) lowers the
    cross-entropy by `decrease`; at least half of that is required here."""
    from proto_clip_amd import prograd
    name, lr = pr.SGD_CASE
    want = golden(pr.SGD_FIXTURE)
    assert str(want["case"]) == name and float(want["lr"]) == lr
    meta, model, ctx, tokens, feats, labels, teacher = fixture_case(name)
    assert int(want["seed"]) == int(meta["seed"])
    N, Q = int(meta["N"]), int(meta["Q"])
    cfg = {"coop_epochs": 5, "coop_batch": Q, "coop_lr": lr, "coop_loss_scale": 1024.0, "n_ctx": int(meta["n_ctx"]), "seed": int(meta["seed"])}
    head = prograd.run_prograd(cfg, feats, labels, feats, labels, names(N), model, tokenized_prompts=tokens, teacher_weights=teacher)
    assert isinstance(head, prograd.ProGrad)
    losses = [e["loss"] for e in head.results["epochs"]]
    with torch.no_grad():
        final = float(head.losses(feats, labels)[0])
    ref = [float(v) for v in want["ce"]]
    print("run_prograd ce over five steps:", " ".join(f"{v:.6f}" for v in losses), f"-> {final:.6f}; decrease {losses[0] - final:.6f}",
          "(reference fp32 chain:", " ".join(f"{v:.6f}" for v in ref), f"decrease {float(want['decrease']):.6f})")
    assert len(losses) == 5 and all(math.isfinite(v) for v in losses)
    observe("run_prograd: half the reference's five-step decrease / the decrease here", 0.5 * float(want["decrease"]) / max(losses[0] - final, 1e-9), 1.0)
    assert losses[0] - final >= 0.5 * float(want["decrease"]), (losses, final)
