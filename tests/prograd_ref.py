"""The shared definitions of the ProGrad fixtures (tests/golden/make_golden_prograd.py) and their test (tests/test_gpu_prograd.py): the seeded inputs, the two
float64 losses on delivered text features, and the projection rule in float64."""
import numpy as np
import torch

import coop_ref

LAM = 1.0
# name -> (tower tag, weight seed, N, n_ctx, Q, first input seed, labels: "agree" = the teacher's arg-max, "derange" = a fixed derangement of it)
FIXTURES = {"prograd_grad_tiny_agree": ("tiny", 91, 6, 4, 12, 51, "agree"),
            "prograd_grad_tiny_derange": ("tiny", 91, 6, 4, 12, 51, "derange"),
            "prograd_grad_small_agree": ("small", 92, 10, 16, 24, 52, "agree"),
            "prograd_grad_small_derange": ("small", 92, 10, 16, 24, 52, "derange")}
# five steps of run_prograd: (fixture whose case is trained, learning rate)
SGD_CASE = ("prograd_grad_tiny_derange", 0.05)
SGD_FIXTURE = "prograd_sgd_tiny"


def teacher_tokens(tokens, n_ctx, vocab, seed):
    """The un-spliced prompts of the teacher: the fixture's prompts with seeded real token ids in place of the n_ctx placeholders (a hand-written
    "a photo of a", the same words for every class)."""
    g = torch.Generator().manual_seed(seed + 500)
    ids = torch.randint(2, vocab - 2, (n_ctx,), generator=g)
    out = tokens.clone()
    out[:, 1:1 + n_ctx] = ids
    return out


def fixture_inputs(kw, N, n_ctx, Q, seed):
    """Seeded (ctx fp32 [n_ctx, W], tokens [N, 77], teacher tokens, image features [Q, E] fp16): coop_ref.fixture_inputs' shared-context case.  The labels
    come from the teacher's prediction and are stored in the fixture."""
    ctx, tokens, feats, _ = coop_ref.fixture_inputs(kw, N, n_ctx, Q, seed, False)
    return ctx, tokens, teacher_tokens(tokens, n_ctx, kw["vocab_size"], seed), feats


def labels_from(teacher_argmax, N, how):
    """"agree": the teacher's arg-max; "derange": class (arg-max + 1 + arg-max % (N - 1)) % N — never the arg-max itself."""
    t = teacher_argmax.long()
    return t if how == "agree" else (t + 1 + t % (N - 1)) % N


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def scale_of(logit_scale):
    return float(np.exp(np.float64(np.float32(logit_scale))))


def ce64(feats, text, labels, logit_scale):
    return coop_ref.loss64(feats, text, labels, logit_scale)


def kl64(feats, text, teacher16, logit_scale):
    """mean_q KL(softmax(scale f' @ teacher'^T) || softmax(scale f' @ text'^T)) in float64, every side normalised there."""
    f = unit(feats.double())
    s = scale_of(logit_scale) * f @ unit(text.double()).t()
    z = scale_of(logit_scale) * f @ unit(teacher16.double()).t()
    logp, logq = torch.log_softmax(z, 1), torch.log_softmax(s, 1)
    return (logp.exp() * (logp - logq)).sum(1).mean()


def project64(g_ce, g_kl, lam=LAM):
    """Upstream's rule in float64: (projected gradient, conflict?, cos of the two gradients)."""
    g_ce, g_kl = g_ce.double(), g_kl.double()
    d, n = float((g_ce * g_kl).sum()), float((g_kl * g_kl).sum())
    cos = d / (float(g_ce.norm()) * n ** 0.5) if n > 0 and float(g_ce.norm()) > 0 else 0.0
    if d >= 0 or n == 0:
        return g_ce.clone(), False, cos
    return g_ce - lam * d / n * g_kl, True, cos
