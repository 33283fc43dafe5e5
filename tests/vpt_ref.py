"""References for visual prompt tuning (csrc/pclip_vpt.hip), on the CPU, derived from the header comment of that file:

  * the torch expressions of the append and the replace (a prompt element is rounded once, fp32 -> fp16, round to nearest even; stem rows keep their bits);
  * an emulation of the gradient's summation ORDER with fp32 accumulators (numpy float32: one rounded addition per `+`): slices of 16 consecutive images,
    ascending image order inside a slice into one accumulator, then the slices in ascending order into one accumulator, every sum starting from its first
    term — with three deliberately wrong walks;
  * the float64 sum and the tolerance derived from that order, the rule of tests/tower_prefix_ref.py: n images in k slices are at most n additions inside
    the slices and k - 1 merges -> (n + k) u sum |terms| per element, u = 2^-24;
  * the seeded inputs of the reference fixtures (tests/golden/make_golden_vpt.py generates them, tests/test_gpu_vpt.py regenerates them)."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24
SLICE = 16          # PCLIP_VPT_SLICE
MAX_L = 288         # PCLIP_VPT_MAX_L

# the long fixture's tower: 224 px at patch 14 -> L0 = 257 rows, 31 prompt rows fill the 288-token envelope (nine full key tiles, the eight-wave backward)
LONG = dict(embed_dim=64, image_resolution=224, vision_layers=2, vision_width=128, vision_patch_size=14, context_length=77, vocab_size=64,
            transformer_width=64, transformer_heads=1, transformer_layers=1)


def append(t16, ctx0, B, L0):
    """[B * (L0 + P), W] fp16: torch.cat([t.view(B, L0, W), ctx0.half().expand(B, P, W)], 1)."""
    P, W = ctx0.shape
    return torch.cat([t16.reshape(B, L0, W), ctx0.half().expand(B, P, W)], 1).reshape(B * (L0 + P), W)


def replace(x16, ctx, B, L0):
    """A copy of the stream x [B * (L0 + P), W] with rows L0 .. L0 + P - 1 of every sequence set to ctx.half()."""
    P, W = ctx.shape
    out = x16.clone().reshape(B, L0 + P, W)
    out[:, L0:] = ctx.half()
    return out.reshape(B * (L0 + P), W)


def prompt_rows(g16, B, L0, P):
    """[B, P, W]: the rows the gradient kernel reads."""
    return g16.reshape(B, L0 + P, -1)[:, L0:]


def emulate_grad(g16, B, L0, P, variant=None):
    """dctx [P, W] fp32 by the documented walk.  variant "drop_last_slice": the merge forgets the last slice; "double_slice": it adds the second slice
    twice; "clear_first": the clearing form stores its zeros BEFORE the load, so every term read is zero."""
    x = prompt_rows(g16, B, L0, P).float().numpy()
    if variant == "clear_first":
        x = np.zeros_like(x)
    parts = []
    for n0 in range(0, B, SLICE):
        acc = x[n0].copy()
        for n in range(n0 + 1, min(B, n0 + SLICE)):
            acc = (acc + x[n]).astype(np.float32)
        parts.append(acc)
    if variant == "drop_last_slice":
        parts = parts[:-1]
    out = parts[0].copy()
    for k, p in enumerate(parts[1:], 1):
        out = (out + p).astype(np.float32)
        if variant == "double_slice" and k == 1:
            out = (out + p).astype(np.float32)
    return torch.from_numpy(out)


def grad64(g16, B, L0, P):
    return prompt_rows(g16, B, L0, P).double().sum(0)


def tol_grad(g16, B, L0, P):
    """[P, W]: (n + k) u sum_b |g[b, L0 + j, d]| for n = B images in k = ceil(B / 16) slices."""
    k = (B + SLICE - 1) // SLICE
    return (B + k) * U32 * prompt_rows(g16, B, L0, P).double().abs().sum(0)


def worst_ratio(got, want, tol):
    """max |got - want| / tol; where tol is 0 the values must be equal (inf otherwise).  A NaN anywhere is inf."""
    err = (got.double() - want.double()).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    zero = tol == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / tol[~zero]).max())


def synth_g(B, L, W, seed):
    """fp16 gradient rows spread over three decades, as a gradient stream is."""
    g = torch.Generator().manual_seed(seed)
    rows = max(B * L, 2)
    scale = torch.logspace(-3, 0, rows)[torch.randperm(rows, generator=g)][:B * L, None]
    return (torch.randn(B * L, W, generator=g) * scale).half()


# ---- the reference fixtures ---------------------------------------------------------------------------------------------------------------------------

# name -> (tower tag, weight seed, images B, prompt rows P, depth, classes N, input seed)
FIXTURES = {
    "vpt_grad_tiny_p4_d1": ("tiny", 91, 5, 4, 1, 6, 51),
    "vpt_grad_tiny_p4_d2": ("tiny", 91, 5, 4, 2, 6, 52),
    "vpt_grad_small_p15_d3": ("small", 92, 6, 15, 3, 7, 53),        # L = 32: the last row of a 32-key tile
    "vpt_grad_small_p16_d3": ("small", 92, 6, 16, 3, 7, 54),        # L = 33: one row into the next tile
    "vpt_grad_odd_p7_d2": ("odd", 93, 4, 7, 2, 5, 55),              # L0 = 26, W = 192
    "vpt_grad_long_p31_d2": ("long", 94, 3, 31, 2, 4, 56),          # L0 = 257, L = 288: the envelope's edge
}
LOGIT_SCALE = math.log(20.0)
# five SGD steps of run_vpt (tower tag, weight seed, images, prompt rows, depth, classes, input seed, learning rate)
SGD_CASE = ("tiny", 95, 8, 4, 2, 6, 57, 0.03)
SGD_REFERENCE_DECREASE = 0.247323      # loss(ctx_0) - loss(ctx_5) on the reference's fp32 CPU chain: `make_golden_vpt.py sgd` prints it


def towers():
    from spec import ODD, SMALL, TINY
    return {"tiny": TINY, "small": SMALL, "odd": ODD, "long": LONG}


def fixture_inputs(kw, B, P, depth, N, seed):
    """Seeded (ctx fp32 [depth, P, W], images [B, 3, R, R] fp16-exact fp32, text weights [N, E] fp16, labels [B]) — torch's CPU generator."""
    g = torch.Generator().manual_seed(seed)
    W, E, R = kw["vision_width"], kw["embed_dim"], kw["image_resolution"]
    ctx = torch.randn(depth, P, W, generator=g) * 0.02
    images = torch.randn(B, 3, R, R, generator=g).half().float()
    text = torch.randn(N, E, generator=g).half()
    labels = torch.randint(0, N, (B,), generator=g)
    return ctx, images, text, labels


def loss64(feats, text, labels, logit_scale=LOGIT_SCALE):
    """The fixtures' loss: float64 cross-entropy of exp(float32(logit_scale)) * normalize(feats) @ normalize(text).T, on the features cast to float64."""
    fi, ft = feats.double(), text.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    return torch.nn.functional.cross_entropy(float(np.exp(np.float64(np.float32(logit_scale)))) * fi @ ft.t(), labels)
