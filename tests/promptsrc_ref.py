"""The shared definitions of the PromptSRC fixtures (tests/golden/make_golden_promptsrc.py) and their tests (tests/test_gpu_promptsrc.py,
tests/test_promptsrc_cpu.py): the cases, the seeded inputs, the hand-written templates' token rows, and the four-term loss in float64."""
import numpy as np
import torch

import coop_ref
import maple_ref
import prograd_ref

LOGIT_SCALE = maple_ref.LOGIT_SCALE
W_TEXT, W_IMAGE, W_LOGITS = 25.0, 10.0, 1.0          # upstream's weights
TEMPLATES = ("T0 {}.", "T1 {}.")                     # two hand-written templates: seeded real tokens where the learner has its placeholders

# name -> (tower tag, weight seed, images B, classes N, text rows, text depth, vision rows, vision depth, input seed)
FIXTURES = {
    "promptsrc_grad_tiny_t2d2_v3d2": ("tiny", 111, 2, 6, 2, 2, 3, 2, 71),
    "promptsrc_grad_small_t4d3_v4d3": ("small", 112, 3, 17, 4, 3, 4, 3, 72),
    "promptsrc_grad_small_t2d1_v5d3": ("small", 112, 3, 17, 2, 1, 5, 3, 73),          # unequal row counts and depths: what MaPLe's coupling cannot express
    "promptsrc_grad_tiny_shallow": ("tiny", 113, 2, 6, 2, 1, 3, 1, 74),               # depth 1 on both sides
}
# five steps of run_promptsrc: (tower tag, weight seed, images, classes, text rows, text depth, vision rows, vision depth, input seed, learning rate)
SGD_CASE = ("tiny", 115, 8, 6, 2, 2, 3, 2, 77, 0.03)
SGD_FIXTURE = "promptsrc_sgd_tiny"


def towers():
    return maple_ref.towers()


def names(n):
    return [f"class{i}" for i in range(n)]


def fixture_inputs(kw, B, N, Pt, Dt, Pv, Dv, seed):
    """Seeded (ctx fp32 [Dt, Pt, Wt], vctx fp32 [Dv, Pv, Wv], tokens [N, 77], teacher tokens [len(TEMPLATES)][N, 77], images [B, 3, R, R] fp16-exact fp32,
    labels [B]) — torch's CPU generator."""
    g = torch.Generator().manual_seed(seed)
    Wt, Wv, R = kw["transformer_width"], kw["vision_width"], kw["image_resolution"]
    ctx = torch.randn(Dt, Pt, Wt, generator=g) * 0.02
    vctx = torch.randn(Dv, Pv, Wv, generator=g) * 0.02
    images = torch.randn(B, 3, R, R, generator=g).half().float()
    labels = torch.randint(0, N, (B,), generator=g)
    tokens = coop_ref.prompt_tokens(N, Pt, kw["vocab_size"], seed + 1000)
    teacher = [prograd_ref.teacher_tokens(tokens, Pt, kw["vocab_size"], seed + 10 * k) for k in range(len(TEMPLATES))]
    return ctx, vctx, tokens, teacher, images, labels


def template_tokenizer(teacher, N):
    """A `tokenize` callable for `frozen_text_features`: the texts TEMPLATES[k].format("class<i>") map to row i of teacher[k]."""
    table = {TEMPLATES[k].format(f"class{i}"): teacher[k][i] for k in range(len(TEMPLATES)) for i in range(N)}
    return lambda texts: torch.stack([table[t] for t in ([texts] if isinstance(texts, str) else texts)])


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def scale_of(logit_scale=LOGIT_SCALE):
    return float(np.exp(np.float64(np.float32(logit_scale))))


def fixed_text64(per_template_features):
    """PromptSRC's text target: the mean over the templates of the UN-normalised features [T][N, E], then one normalisation, in float64."""
    return unit(torch.stack([f.double() for f in per_template_features]).mean(0))


def terms64(img, txt, zs_img, fixed_text, labels, logit_scale=LOGIT_SCALE):
    """(ce, text L1, image L1, batch-mean KL) in float64 on delivered features; img and txt carry the tape, zs_img and fixed_text are constants
    (fixed_text normalised already, zs_img not)."""
    scale = scale_of(logit_scale)
    fi, ft, fz, fx = unit(img.double()), unit(txt.double()), unit(zs_img.double()), fixed_text.double()
    s, z = scale * fi @ ft.t(), scale * fz @ fx.t()
    ce = torch.nn.functional.cross_entropy(s, labels)
    l_text = (ft - fx).abs().mean()
    l_image = (fi - fz).abs().mean()
    logp, logq = torch.log_softmax(z, 1), torch.log_softmax(s, 1)
    kd = (logp.exp() * (logp - logq)).sum(1).mean()
    return ce, l_text, l_image, kd


def total64(terms, N, w_text=W_TEXT, w_image=W_IMAGE, w_logits=W_LOGITS):
    ce, l_text, l_image, kd = terms
    return ce + w_text * l_text + w_image * l_image + (w_logits / N) * kd


def gpa_sum64(weights, snapshots):
    """The float64 Gaussian-weighted sum of per-epoch snapshots [E][...], and sum_e |w_e theta_e| for its tolerance."""
    w = np.asarray(weights, dtype=np.float64)
    terms = [float(w[e]) * snapshots[e].double() for e in range(len(snapshots))]
    return sum(terms), sum(t.abs() for t in terms)
