"""References for CoCoOp's kernels (csrc/pclip_cocoop.hip), on the CPU, derived from the header comments of that file and of csrc/pclip_small_linear.h:

  * a numpy-float32 emulation of the meta-net's forward and backward in exactly the documented order — every product rounded on its own, every `+` one
    rounded fp32 addition, every accumulator starting at +0, the biases added last; layer 1 and the weight / bias gradients are the shared walks of
    tests/maple_ref.py (emulate_rowdot16, emulate_dw_db) at depth 1 — with the float64 statements and the tolerances derived from that order
    by the project's rule: (rounded operations on the path of one term) x u x sum |terms|, u = 2^-24, plus what an input's own tolerance contributes where
    a stage reads the previous stage's result;
  * the conditional assembly (tests/coop_ref.py's restatement with the rows r16(ctx[j] + pi[b])) with its float64 statement and the tolerance of its
    three roundings (one fp32, two fp16);
  * the conditional context gradient: tests/coop_ref.py's slice-sum walk per image, then the images in ascending order (dctx) and the rows in ascending order
    (dpi), with the float64 sums and their tolerances;
  * deliberately wrong walks: descending b, a slice length of 8, pi added after the rounding to fp16, the bias added first, a fused multiply-add;
  * the seeded inputs of the reference fixtures (tests/golden/make_golden_cocoop.py generates them, tests/test_gpu_cocoop.py regenerates them)."""
import math

import numpy as np
import torch

import coop_ref
import maple_ref
import vpt_ref

U32 = vpt_ref.U32
U16 = 2.0 ** -11            # fp16's unit roundoff
TINY16 = 2.0 ** -25         # half the spacing of fp16's subnormals: the absolute error of a rounding into that range
SLICE = coop_ref.CTX_SLICE  # PCLIP_PROMPT_CTX_SLICE: classes per slice of the conditional context gradient
MAX_B = 16                  # PCLIP_COCOOP_MAX_B

worst_ratio = vpt_ref.worst_ratio


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


_madd = maple_ref.madd


# ---- the meta-net -------------------------------------------------------------------------------------------------------------------------------------------

def emulate_metanet_fwd(f16, W1, b1, W2, b2, variant=None):
    """(h [B, Hd], pi [B, Wt]) fp32 by the documented walks.  Layer 1: maple_ref.emulate_rowdot16 at depth 1, then h = +0 where pre <= 0.  Layer 2:
    ascending u into one accumulator from +0, the bias last.  variant "bias_first": both accumulators start at the bias instead (lane 0's in layer 1);
    "fma": every multiply-add is fused."""
    f, W1, b1, W2, b2 = _f32(f16.float()), _f32(W1), _f32(b1), _f32(W2), _f32(b2)
    fused = variant == "fma"
    B, Wt = f.shape[0], W2.shape[0]
    Hd = W1.shape[0]
    pre = maple_ref.emulate_rowdot16(f[None], W1[None], b1[None], "first" if variant == "bias_first" else "last", fused)[0]
    h = np.where(pre <= 0, np.float32(0), pre).astype(np.float32)
    out = np.zeros((B, Wt), np.float32)
    if variant == "bias_first":
        out = out + b2[None, :]
    for u in range(Hd):
        out = _madd(out, h[:, u, None], W2[None, :, u], fused)
    if variant != "bias_first":
        out = (out + b2[None, :]).astype(np.float32)
    return _t(h), _t(out)


def metanet_fwd64(f16, W1, b1, W2, b2):
    """(pre, h, pi) in float64."""
    pre = f16.double() @ W1.double().t() + b1.double()
    h = pre.clamp_min(0)
    return pre, h, h @ W2.double().t() + b2.double()


def tol_metanet_fwd(f16, W1, b1, W2, b2):
    """(tol_h, tol_pi).  h: 1 product + E / 16 chain additions + 4 butterfly additions + 1 bias addition on a term's path (relu does not enlarge an error).
    pi: 1 product + Hd additions + 1 bias addition over the magnitudes with |h| + tol_h for |h|, plus what h's own tolerance carries through |W2|."""
    E, Hd = f16.shape[1], W1.shape[0]
    tol_h = (E // 16 + 6) * U32 * (f16.double().abs() @ W1.double().abs().t() + b1.double().abs())
    h = metanet_fwd64(f16, W1, b1, W2, b2)[1].abs() + tol_h
    w2 = W2.double().abs()
    return tol_h, (Hd + 2) * U32 * (h @ w2.t() + b2.double().abs()) + tol_h @ w2.t()


def emulate_metanet_dpre(dpi, h, W2, fused=False):
    """dpre [B, Hd] fp32 (numpy): dh sums over t in ascending order in one accumulator from +0; dpre = dh where h > 0, else +0."""
    dpi, h, W2 = _f32(dpi), _f32(h), _f32(W2)
    dh = np.zeros(h.shape, np.float32)
    for t in range(dpi.shape[1]):
        dh = _madd(dh, dpi[:, t, None], W2[None, t, :], fused)
    return np.where(h > 0, dh, np.float32(0)).astype(np.float32)


def emulate_metanet_bwd(dpi, f16, h, W2, variant=None):
    """(dW1, db1, dW2, db2) fp32 by the documented walks: dW2 with db2 from (dpi, h) and dW1 with db1 from (dpre, f) by maple_ref.emulate_dw_db at depth
    1, dpre by emulate_metanet_dpre.  variant "descending_b": the images are added from the last to the first; "fma": every multiply-add is fused."""
    dpi, f, h, W2 = _f32(dpi), _f32(f16.float()), _f32(h), _f32(W2)
    fused, descending = variant == "fma", variant == "descending_b"
    dW2, db2 = maple_ref.emulate_dw_db(dpi[None], h[None], descending, fused)
    dpre = emulate_metanet_dpre(dpi, h, W2, fused)
    dW1, db1 = maple_ref.emulate_dw_db(dpre[None], f[None], descending, fused)
    return _t(dW1[0]), _t(db1[0]), _t(dW2[0]), _t(db2[0])


def metanet_bwd64(dpi, f16, h, W2):
    """(dW1, db1, dW2, db2) in float64 of the backward as the kernel is given it: the mask is h > 0 of the h it reads."""
    g, hh, w2 = dpi.double(), h.double(), W2.double()
    dpre = (g @ w2) * (hh > 0)
    return dpre.t() @ f16.double(), dpre.sum(0), g.t() @ hh, g.sum(0)


def tol_metanet_bwd(dpi, f16, h, W2):
    """dW2: 1 product + B additions; db2: B additions; dpre: 1 product + Wt additions; dW1 / db1: 1 product + B additions / B additions over |dpre| + tol_dpre,
    plus what dpre's own tolerance carries."""
    g, hh, w2, f = dpi.double().abs(), h.double().abs(), W2.double().abs(), f16.double().abs()
    B, Wt = dpi.shape
    mask = (h > 0).double()
    tol_dpre = (1 + Wt) * U32 * (g @ w2) * mask
    dpre = (dpi.double() @ W2.double()).abs() * mask + tol_dpre
    return ((1 + B) * U32 * (dpre.t() @ f) + tol_dpre.t() @ f, B * U32 * dpre.sum(0) + tol_dpre.sum(0), (1 + B) * U32 * (g.t() @ hh), B * U32 * g.sum(0))


def synth_metanet(B, E, Hd, Wt, seed, family="decades"):
    """(f [B, E] fp16 normalised, W1, b1, W2, b2, dpi) fp32.  "decades": rows spread over three decades; "cancel": every odd column of W1 is the negated even
    one plus a 2^-10 relative perturbation while f's odd column repeats the even one, and dpi / the rows of W2 likewise in t — sums far below their terms.
    Pre-activations of both signs occur in either family."""
    g = torch.Generator().manual_seed(seed)

    def spread(*shape):
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        scale = torch.logspace(-3, 0, max(rows, 2))[torch.randperm(max(rows, 2), generator=g)][:rows].reshape(*shape[:-1], 1)
        return torch.randn(*shape, generator=g) * scale

    f = torch.randn(B, E, generator=g)
    W1, b1, W2, b2, dpi = spread(Hd, E), torch.randn(Hd, generator=g) * 0.05, spread(Wt, Hd) * 0.1, torch.randn(Wt, generator=g) * 0.01, spread(B, Wt)
    if family == "cancel":
        f[:, 1::2] = f[:, 0::2]
        W1[:, 1::2] = -W1[:, 0::2] * (1 + 2.0 ** -10 * torch.randn(Hd, E // 2, generator=g))
        b1 = b1 * 1e-3
        dpi[:, 1::2] = dpi[:, 0::2]
        W2[1::2, :] = -W2[0::2, :] * (1 + 2.0 ** -10 * torch.randn(Wt // 2, Hd, generator=g))
    f = (f / f.norm(dim=1, keepdim=True)).half()
    return f.contiguous(), W1.contiguous(), b1.contiguous(), W2.contiguous(), b2.contiguous(), dpi.contiguous()


# ---- the conditional assembly -------------------------------------------------------------------------------------------------------------------------------------

def prompt_embed_cond(ctx, pi, tokens, emb16, pos16, L_out=None, variant=None):
    """x [B * N * L_out, W] fp16 = r16(f32(src) + f32(pos16[l])): src = r16(ctx[l - 1] + pi[b]) on 1 <= l <= n_ctx (one fp32 addition, one rounding to
    fp16), the token embedding of the clamped id elsewhere.  variant "pi_after_r16": src = r16(f32(r16(ctx[l - 1])) + pi[b])."""
    N, L_tok = tokens.shape
    vocab, W = emb16.shape
    B = pi.shape[0]
    L_out = L_tok if L_out is None else L_out
    assert ctx.dtype == pi.dtype == torch.float32 and emb16.dtype == pos16.dtype == torch.float16
    src = emb16[tokens[:, :L_out].clamp(0, vocab - 1)].clone()[None].repeat(B, 1, 1, 1)      # [B, N, L_out, W] fp16
    k = min(ctx.shape[0], L_out - 1)                                                          # context rows at l >= L_out do not exist in the output
    base = ctx[:k].half().float() if variant == "pi_after_r16" else ctx[:k]
    src[:, :, 1:1 + k] = (base[None] + pi[:, None, :]).half()[:, None]
    return (src.float() + pos16[:L_out].float()).half().reshape(B * N * L_out, W)


def prompt_embed_cond64(ctx, pi, tokens, emb16, pos16, L_out=None):
    """(x64, tol): the float64 statement and the tolerance of the kernel's roundings — a context element: u32 |s| for the fp32 addition, then (u16 |s| +
    2^-25) and (u16 |s + p| + 2^-25) for the two roundings to fp16 (second-order terms: a factor 1 + 2 u16); a token element: the last of these alone."""
    N, L_tok = tokens.shape
    vocab, W = emb16.shape
    B = pi.shape[0]
    L_out = L_tok if L_out is None else L_out
    src = emb16[tokens[:, :L_out].clamp(0, vocab - 1)].double()[None].repeat(B, 1, 1, 1)
    k = min(ctx.shape[0], L_out - 1)
    s = (ctx[:k].double()[None] + pi.double()[:, None, :])[:, None].expand(B, N, k, W)
    src[:, :, 1:1 + k] = s
    x = src + pos16[:L_out].double()
    tol = U16 * x.abs() + TINY16
    tol[:, :, 1:1 + k] = (1 + 2 * U16) * (U32 * s.abs() + U16 * s.abs() + TINY16 + U16 * x[:, :, 1:1 + k].abs() + TINY16)
    return x.reshape(B * N * L_out, W), tol.reshape(B * N * L_out, W)


# ---- the conditional context gradient -------------------------------------------------------------------------------------------------------------------------------

def emulate_cond_grad(dx16, B, N, L_out, n_ctx, variant=None):
    """(dctx [n_ctx, W], dpi [B, W], dshift [B, n_ctx, W]) fp32 by the documented walk: coop_ref.prompt_ctx_grad (slices of 16 classes) on each image's N
    prompts, then the images in ascending order from b = 0 (dctx) and the rows that exist in ascending order from j = 0 (dpi).  variant "descending_b":
    dctx adds the images from the last to the first; "slice8": slices of 8 classes."""
    W = dx16.shape[1]
    d = dx16.reshape(B, N * L_out, W)
    dshift = torch.stack([coop_ref.prompt_ctx_grad(d[b], N, L_out, n_ctx, False, 8 if variant == "slice8" else SLICE) for b in range(B)])
    order = list(range(B - 1, -1, -1) if variant == "descending_b" else range(B))
    dctx = dshift[order[0]].clone()
    for b in order[1:]:
        dctx = dctx + dshift[b]
    avail = min(n_ctx, L_out - 1)
    dpi = torch.zeros(B, W)
    if avail > 0:
        dpi = dshift[:, 0].clone()
        for j in range(1, avail):
            dpi = dpi + dshift[:, j]
    return dctx, dpi, dshift


def _ctx_rows64(dx16, B, N, L_out, n_ctx):
    """[B, N, n_ctx, W] float64: the context rows of dx, zeros where a row does not exist."""
    W = dx16.shape[1]
    rows = torch.zeros(B, N, n_ctx, W, dtype=torch.float64)
    k = min(n_ctx, L_out - 1)
    rows[:, :, :k] = dx16.reshape(B, N, L_out, W)[:, :, 1:1 + k].double()
    return rows


def cond_grad64(dx16, B, N, L_out, n_ctx):
    rows = _ctx_rows64(dx16, B, N, L_out, n_ctx)
    return rows.sum((0, 1)), rows.sum((1, 2)), rows.sum(1)


def tol_cond_grad(dx16, B, N, L_out, n_ctx):
    """dshift: N classes in k slices, at most N additions inside the slices and k - 1 merges -> (N + k) u sum |terms| (vpt_ref's rule); dctx: B - 1 further
    additions on a term's path; dpi: n_ctx - 1 further additions."""
    mag = _ctx_rows64(dx16, B, N, L_out, n_ctx).abs()
    k = (N + SLICE - 1) // SLICE
    return (N + k + B) * U32 * mag.sum((0, 1)), (N + k + n_ctx) * U32 * mag.sum((1, 2)), (N + k) * U32 * mag.sum(1)


def synth_dx(B, N, L_out, W, seed):
    return vpt_ref.synth_g(B * N, L_out, W, seed)


# ---- the reference fixtures -----------------------------------------------------------------------------------------------------------------------------

# name -> (tower tag, weight seed, images B, classes N, n_ctx, input seed, l_eff or None)
FIXTURES = {
    "cocoop_grad_tiny_b2_n6": ("tiny", 111, 2, 6, 4, 71, None),
    "cocoop_grad_small_b3_n17": ("small", 112, 3, 17, 4, 83, None),            # N one past a slice of 16 classes
    "cocoop_grad_small_b1_n10_p16": ("small", 112, 1, 10, 16, 73, None),
    "cocoop_grad_small_len33": ("small", 113, 2, 5, 4, 80, 33),                # L_eff = 33: run truncated and untruncated, equal bits required
}
LOGIT_SCALE = vpt_ref.LOGIT_SCALE
RELU_MARGIN = 16.0      # min |pre-activation| of the float64 run >= 16 x max |pre-activation difference| of the fp16-chain run: every chain agrees on the mask
# five SGD steps on the five tensors (tower tag, weight seed, images, classes, n_ctx, input seed, learning rate)
SGD_CASE = ("tiny", 115, 4, 6, 4, 76, 0.1)
SGD_REFERENCE_DECREASE = 0.024019      # loss(0) - loss(5) on the reference's fp32 CPU chain: `make_golden_cocoop.py sgd` prints it


def towers():
    from spec import SMALL, TINY
    return {"tiny": TINY, "small": SMALL}


def fixture_inputs(kw, B, N, n_ctx, seed, l_eff=None):
    """Seeded (ctx fp32 [n_ctx, Wt], W1 [Hd, E], b1 [Hd], W2 [Wt, Hd], b2 [Wt], tokens [N, 77], image features [B, E] fp16, labels [B]) — torch's CPU
    generator; Hd = E // 16; the meta-net in nn.Linear's default ranges U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)).  The fixtures' seeds are those for which
    every pre-activation stands clear of zero (RELU_MARGIN; the generator asserts it)."""
    g = torch.Generator().manual_seed(seed)
    Wt, E = kw["transformer_width"], kw["embed_dim"]
    Hd = E // 16
    ctx = torch.randn(n_ctx, Wt, generator=g) * 0.02
    r1, r2 = 1.0 / math.sqrt(E), 1.0 / math.sqrt(Hd)
    W1 = (torch.rand(Hd, E, generator=g) * 2 - 1) * r1
    b1 = (torch.rand(Hd, generator=g) * 2 - 1) * r1
    W2 = (torch.rand(Wt, Hd, generator=g) * 2 - 1) * r2
    b2 = (torch.rand(Wt, generator=g) * 2 - 1) * r2
    feats = torch.randn(B, E, generator=g).half()
    labels = torch.randint(0, N, (B,), generator=g)
    tokens = coop_ref.prompt_tokens(N, n_ctx, kw["vocab_size"], seed + 1000, l_eff)
    return ctx, W1, b1, W2, b2, tokens, feats, labels


def loss64(feats, text, labels, logit_scale=LOGIT_SCALE):
    """The fixtures' loss: the mean over the images of the float64 cross-entropy of exp(float32(logit_scale)) * normalize(feats[b]) . normalize(text[b, :]),
    text [B, N, E]."""
    fi, ft = feats.double(), text.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=2, keepdim=True)
    logits = float(np.exp(np.float64(np.float32(logit_scale)))) * torch.einsum("be,bne->bn", fi, ft)
    return torch.nn.functional.cross_entropy(logits, labels)
