#!/usr/bin/env python3
"""Generates tests/golden/prograd_grad_<tag>_<agree|derange>.npz and prograd_sgd_tiny.npz by RUNNING THE REFERENCE ITSELF under autograd, by the recipe of
make_golden_coop.py: make_golden.py's import shim, the reference's own `build_model(...)` and `encode_text` on seeded towers (spec.TINY / spec.SMALL,
random_state_dict + trained_like_), the learned context rows put into the prompt by a forward hook on the reference's `token_embedding`.  This file holds
no reference code, only calls into it.

    python tests/golden/make_golden_prograd.py

The teacher is the same seeded tower's `encode_text` of the UN-SPLICED prompts (prograd_ref.teacher_tokens: real token ids where the context goes), in
the reference's own fp16 chain, stored as fp16 rows: the frozen hand-crafted classifier.  Two losses on seeded image features, both float64 functions of
the text features (prograd_ref.ce64 / kl64; scale = exp(float32(log 20))), two gradients of the context, and upstream's projection of them
(prograd_ref.project64, lambda = 1).  The labels are the teacher's arg-max ("agree": no conflict expected, g = g_ce) or a fixed derangement of it
("derange": a conflict); they are stored.

Two runs per case, as for CoOp: f64 (the model `.double()` with the float64 LayerNorm swap, a float64 context) gives g_ce_f64, g_kl_f64, the projected
g_f64, the losses and cos_f64 = <g_ce, g_kl> / (|g_ce| |g_kl|); the reference's own fp16 chain on the CPU gives e_ref for each of the three vectors,
||x_fp16chain - x_f64|| / ||x_f64||.  tests/test_gpu_prograd.py asks ||x_ours - x_f64|| / ||x_f64|| <= 2 e_ref of each, with no floor, and float64's
branch.  A case is written only if it is DECIDED: |cos_f64| >= 0.1, the branch the case is named for, and the fp16 chain on the same branch; otherwise
the next input seed is tried (the seed used is stored).

prograd_sgd_tiny.npz: the cross-entropy over five ProGrad steps of the reference's fp32 chain on the CPU (SGD, momentum 0.9, cosine schedule over the
five steps, one batch of all samples, the context of `coop.PromptLearner(seed=...)`), the figure `run_prograd` is compared with."""
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
from proto_clip_amd.clip.model import random_state_dict            # noqa: E402
from spec import SMALL, TINY, trained_like_                         # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
import prograd_ref as pr                                            # noqa: E402

TOWERS = {"tiny": TINY, "small": SMALL}
LOGIT_SCALE = math.log(20.0)
FLOOR = 0.0
MIN_COS = 0.1


def models(ref_clip_model, kw, sd_seed, dtypes):
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(LOGIT_SCALE, dtype=torch.float32)
    out = []
    for dt in dtypes:
        with contextlib.redirect_stdout(io.StringIO()):
            m = ref_clip_model.build_model({k: v.clone() for k, v in sd.items()})
        m = m.double() if dt == torch.float64 else (m.float() if dt == torch.float32 else m)
        for p in m.parameters():
            p.requires_grad_(False)
        out.append(m)
    return out


def spliced_text(model, ctx, tokens, n_ctx):
    def splice(_module, _args, out):
        out = out.clone()
        out[:, 1:1 + n_ctx] = ctx.to(out.dtype)
        return out
    handle = model.token_embedding.register_forward_hook(splice)
    try:
        return model.encode_text(tokens)
    finally:
        handle.remove()


def two_gradients(model, ctx, tokens, feats, labels, teacher16, n_ctx):
    """(ce, kl, d ce / d ctx, d kl / d ctx) through the reference's encode_text: one forward, two walks."""
    ctx = ctx.clone().requires_grad_(True)
    text = spliced_text(model, ctx, tokens, n_ctx)
    ce, kl = pr.ce64(feats, text, labels, LOGIT_SCALE), pr.kl64(feats, text, teacher16, LOGIT_SCALE)
    (g_ce,) = torch.autograd.grad(ce, ctx, retain_graph=True)
    (g_kl,) = torch.autograd.grad(kl, ctx)
    return float(ce.detach()), float(kl.detach()), g_ce.detach().double(), g_kl.detach().double()


def with_f64_layernorm(ref_clip_model, fn):
    keep = ref_clip_model.LayerNorm.forward
    ref_clip_model.LayerNorm.forward = torch.nn.LayerNorm.forward                # float64 throughout
    try:
        return fn()
    finally:
        ref_clip_model.LayerNorm.forward = keep


def run(ref_clip_model, kw, sd_seed, N, n_ctx, Q, seed, how):
    m16, m64 = models(ref_clip_model, kw, sd_seed, (torch.float16, torch.float64))
    ctx, tokens, ttokens, feats = pr.fixture_inputs(kw, N, n_ctx, Q, seed)
    with torch.no_grad():
        teacher16 = m16.encode_text(ttokens).half()
    z = pr.unit(feats.double()) @ pr.unit(teacher16.double()).t()
    labels = pr.labels_from(z.argmax(1), N, how)
    ce64, kl64, gce64, gkl64 = with_f64_layernorm(ref_clip_model, lambda: two_gradients(m64, ctx.double(), tokens, feats, labels, teacher16, n_ctx))
    ce16, kl16, gce16, gkl16 = two_gradients(m16, ctx, tokens, feats, labels, teacher16, n_ctx)
    g64, conflict64, cos64 = pr.project64(gce64, gkl64)
    g16, conflict16, cos16 = pr.project64(gce16, gkl16)
    rel = lambda x, y: float((x - y).norm() / y.norm())
    out = dict(tokens=tokens, teacher=teacher16, labels=labels, loss_ce_f64=ce64, loss_kl_f64=kl64, loss_ce_f16=ce16, loss_kl_f16=kl16, g_ce_f64=gce64.float(),
               g_kl_f64=gkl64.float(), g_f64=g64.float(), cos_f64=cos64, cos_f16=cos16, conflict=conflict64, e_ref_ce=rel(gce16, gce64), e_ref_kl=rel(gkl16, gkl64),
               e_ref=rel(g16, g64))
    decided = abs(cos64) >= MIN_COS and conflict64 == (how == "derange") and conflict16 == conflict64
    return out, decided


def sgd(ref_clip_model):
    """Five ProGrad steps of the reference's fp32 chain, the case and step rule of test_five_steps_of_run_prograd_lower_the_cross_entropy."""
    name, lr = pr.SGD_CASE
    meta = np.load(os.path.join(HERE, name + ".npz"))
    tag, sd_seed, N, n_ctx, Q, _, _ = pr.FIXTURES[name]
    kw, seed = TOWERS[tag], int(meta["seed"])
    (m32,) = models(ref_clip_model, kw, sd_seed, (torch.float32,))
    _, tokens, _, feats = pr.fixture_inputs(kw, N, n_ctx, Q, seed)
    teacher16, labels = torch.from_numpy(meta["teacher"]), torch.from_numpy(meta["labels"])
    g = torch.Generator().manual_seed(seed)                                   # coop.PromptLearner(seed=seed): N(0, 0.02) rows from torch's CPU generator
    ctx = (torch.randn(n_ctx, kw["transformer_width"], generator=g) * 0.02).requires_grad_(True)
    opt = torch.optim.SGD([ctx], lr=lr, momentum=0.9)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 5)
    ces, conflicts = [], []
    for _ in range(5):
        text = spliced_text(m32, ctx, tokens, n_ctx)
        ce, kl = pr.ce64(feats, text, labels, LOGIT_SCALE), pr.kl64(feats, text, teacher16, LOGIT_SCALE)
        (g_ce,) = torch.autograd.grad(ce, ctx, retain_graph=True)
        (g_kl,) = torch.autograd.grad(kl, ctx)
        proj, conflict, _ = pr.project64(g_ce, g_kl)
        opt.zero_grad()
        ctx.grad = proj.float()
        opt.step()
        sched.step()
        ces.append(float(ce.detach()))
        conflicts.append(conflict)
    with torch.no_grad():
        ces.append(float(pr.ce64(feats, spliced_text(m32, ctx, tokens, n_ctx), labels, LOGIT_SCALE)))
    print("reference fp32 chain, five ProGrad steps (lr %g): ce" % lr, " ".join(f"{v:.6f}" for v in ces), " decrease %.6f" % (ces[0] - ces[-1]),
          " conflicts", conflicts)
    assert ces[0] - ces[-1] > 0
    mg.savez(pr.SGD_FIXTURE, case=name, lr=lr, ce=np.asarray(ces), decrease=ces[0] - ces[-1], conflicts=np.asarray(conflicts), seed=seed)


def main():
    ref_clip_model = mg.import_reference()[4]
    for name, (tag, sd_seed, N, n_ctx, Q, seed0, how) in pr.FIXTURES.items():
        for seed in range(seed0, seed0 + 1000, 10):
            out, decided = run(ref_clip_model, TOWERS[tag], sd_seed, N, n_ctx, Q, seed, how)
            print(f"{name} seed {seed}: ce {out['loss_ce_f64']:.6f} kl {out['loss_kl_f64']:.6f}  cos f64 {out['cos_f64']:+.4f} fp16 chain {out['cos_f16']:+.4f}"
                  f"  conflict {out['conflict']}  e_ref ce {out['e_ref_ce']:.3e} kl {out['e_ref_kl']:.3e} projected {out['e_ref']:.3e}"
                  + ("" if decided else "  -- not decided, next seed"))
            if decided:
                break
        else:
            raise SystemExit(f"{name}: no decided seed")
        assert all(math.isfinite(out[k]) and out[k] > 0 for k in ("e_ref", "e_ref_ce", "e_ref_kl"))
        mg.savez(name, logit_scale=float(np.float32(LOGIT_SCALE)), floor=FLOOR, lam=pr.LAM, e_ref_source="reference fp16 chain on the CPU", tag=tag,
                 sd_seed=sd_seed, N=N, n_ctx=n_ctx, Q=Q, seed=seed, how=how, **out)
    sgd(ref_clip_model)


if __name__ == "__main__":
    main()
