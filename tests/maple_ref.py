"""References for MaPLe's kernels (csrc/pclip_maple.hip), on the CPU, derived from the header comments of that file and of csrc/pclip_small_linear.h:

  * the torch expression of the replace at an offset, and the emulation of the row gradient's summation ORDER (tests/vpt_ref.py's rule applied to the window
    off .. off + P - 1 of sequences of L rows) with its float64 sum and tolerance;
  * a numpy-float32 emulation of the coupling function's forward and backward in exactly the documented order — every product rounded on its own, every
    `+` one rounded fp32 addition, every accumulator starting at +0 — with the float64 results and the tolerances derived from that order by the project's
    rule: (rounded operations on the path of one term) x u x sum |terms|, u = 2^-24.  A term's path holds its product's rounding (1) and the additions
    that follow it;
  * deliberately wrong walks: the window one row off, the bias dropped, one depth's weights used for another, the dX merge forgetting its last slice;
  * the seeded inputs of the reference fixtures (tests/golden/make_golden_maple.py generates them, tests/test_gpu_maple.py regenerates them)."""
import math

import numpy as np
import torch

import coop_ref
import vpt_ref

U32 = vpt_ref.U32
SLICE = vpt_ref.SLICE       # PCLIP_VPT_SLICE: sequences per slice of the row gradient
COUPLE_SLICE = 32           # PCLIP_COUPLE_SLICE: rows of Wc per slice of dX
COUPLE_MAX_P = 16           # PCLIP_COUPLE_MAX_P


# ---- prompt rows at an offset ---------------------------------------------------------------------------------------------------------------------------

def replace(x16, ctx, B, L, off):
    """A copy of the stream x [B * L, W] with rows off .. off + P - 1 of every sequence set to ctx.half()."""
    P, W = ctx.shape
    out = x16.clone().reshape(B, L, W)
    out[:, off:off + P] = ctx.half()
    return out.reshape(B * L, W)


def window(g16, B, L, off, P):
    """[B * P, W]: the rows the gradient kernel reads, compact."""
    W = g16.shape[-1]
    return g16.reshape(B, L, W)[:, off:off + P].reshape(B * P, W)


def emulate_rows_grad(g16, B, L, off, P, variant=None):
    """dctx [P, W] fp32 by vpt_ref's walk over the window.  variant "off_by_one": the window starts one row late (one row early at the sequence's end)."""
    if variant == "off_by_one":
        off = off + 1 if off + P < L else off - 1
        variant = None
    return vpt_ref.emulate_grad(window(g16, B, L, off, P), B, 0, P, variant)


def rows_grad64(g16, B, L, off, P):
    return vpt_ref.grad64(window(g16, B, L, off, P), B, 0, P)


def tol_rows_grad(g16, B, L, off, P):
    """(n + k) u sum_b |g[b, off + j, d]|: vpt_ref's tolerance on the window."""
    return vpt_ref.tol_grad(window(g16, B, L, off, P), B, 0, P)


# ---- the coupling function ------------------------------------------------------------------------------------------------------------------------------

def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def madd(acc, a, b, fused=False):
    """acc + a * b: the product rounded on its own and then added — or, fused, one rounding of the exact sum (the product of two fp32 numbers is exact
    in float64; the float64 addition's own rounding is 29 bits below fp32's)."""
    if fused:
        return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    return (acc + (a * b).astype(np.float32)).astype(np.float32)


# The walks of csrc/pclip_small_linear.h, in numpy float32: the one emulation of each behind the coupling function (here) and the meta-net (cocoop_ref.py).

def emulate_rowdot16(X, W, b, bias="last", fused=False):
    """pre [D, P, R] fp32 of X [D, P, K], W [D, R, K], b [D, R]: lane l of 16 owns columns 64 k + 4 l + j, ascending k then j into one accumulator from +0;
    butterfly at distances 8, 4, 2, 1; the bias last.  bias "first": lane 0's accumulator starts at the bias instead; None: the bias is dropped.  fused:
    every multiply-add of the chain is fused."""
    D, P, K = X.shape
    R = W.shape[1]
    xs = X.reshape(D, P, 1, K // 64, 16, 4)
    ws = W.reshape(D, 1, R, K // 64, 16, 4)
    acc = np.zeros((D, P, R, 16), np.float32)
    if bias == "first":
        acc[..., 0] = b[:, None, :]
    for k in range(K // 64):
        for j in range(4):
            acc = madd(acc, xs[:, :, :, k, :, j], ws[:, :, :, k, :, j], fused)
    lanes = np.arange(16)
    for m in (8, 4, 2, 1):
        acc = (acc + acc[..., lanes ^ m]).astype(np.float32)
    y = acc[..., 0]
    if bias == "last":
        y = (y + b[:, None, :]).astype(np.float32)
    return y


def emulate_dw_db(dY, X, descending=False, fused=False):
    """(dW [D, R, K], db [D, R]) fp32 of dY [D, P, R], X [D, P, K]: the P rows in ascending order (descending: from the last to the first) into one
    accumulator from +0."""
    D, P, R = dY.shape
    dW, db = np.zeros((D, R, X.shape[2]), np.float32), np.zeros((D, R), np.float32)
    for p in (range(P - 1, -1, -1) if descending else range(P)):
        dW = madd(dW, dY[:, p, :, None], X[:, p, None, :], fused)
        db = (db + dY[:, p, :]).astype(np.float32)
    return dW, db


def emulate_couple_fwd(X, Wc, bc, variant=None):
    """Y [depth, P, Wv] fp32 by the documented walk (emulate_rowdot16).  variant "no_bias": the bias is dropped; "wrong_depth": depth d reads the weights
    of depth d - 1."""
    X, Wc, bc = _f32(X), _f32(Wc), _f32(bc)
    if variant == "wrong_depth":
        Wc = np.roll(Wc, 1, axis=0)
    y = emulate_rowdot16(X, Wc, bc, None if variant == "no_bias" else "last")
    return torch.from_numpy(np.ascontiguousarray(y))


def couple_fwd64(X, Wc, bc):
    return torch.einsum("dpt,dvt->dpv", X.double(), Wc.double()) + bc.double()[:, None, :]


def tol_couple_fwd(X, Wc, bc):
    """1 product + Wt / 16 chain additions + 4 butterfly additions + 1 bias addition on a term's path."""
    Wt = X.shape[2]
    mag = torch.einsum("dpt,dvt->dpv", X.double().abs(), Wc.double().abs()) + bc.double().abs()[:, None, :]
    return (Wt // 16 + 6) * U32 * mag


def emulate_couple_bwd(dY, X, Wc, variant=None):
    """(dX, dWc, dbc) fp32 by the documented walks (dWc, dbc: emulate_dw_db).  variant "drop_last_slice": the merge of dX forgets the last slice of 32
    rows; "wrong_depth": dX of depth d reads the weights of depth d - 1."""
    dY, X, Wc = _f32(dY), _f32(X), _f32(Wc)
    if variant == "wrong_depth":
        Wc = np.roll(Wc, 1, axis=0)
    D, P, Wt = X.shape
    Wv = Wc.shape[1]
    dW, db = emulate_dw_db(dY, X)
    parts = []
    for v0 in range(0, Wv, COUPLE_SLICE):
        acc = np.zeros((D, P, Wt), np.float32)
        for v in range(v0, min(Wv, v0 + COUPLE_SLICE)):
            prod = (dY[:, :, v, None] * Wc[:, None, v, :]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
        parts.append(acc)
    if variant == "drop_last_slice":
        parts = parts[:-1]
    dX = parts[0].copy()
    for part in parts[1:]:
        dX = (dX + part).astype(np.float32)
    return torch.from_numpy(dX), torch.from_numpy(dW), torch.from_numpy(db)


def couple_bwd64(dY, X, Wc):
    dY, X, Wc = dY.double(), X.double(), Wc.double()
    return torch.einsum("dpv,dvt->dpt", dY, Wc), torch.einsum("dpv,dpt->dvt", dY, X), dY.sum(1)


def tol_couple_bwd(dY, X, Wc):
    """dX: 1 product + at most 32 additions inside a slice + nslice - 1 merges; dWc: 1 product + P additions; dbc: P additions."""
    a, x, w = dY.double().abs(), X.double().abs(), Wc.double().abs()
    P, Wv = dY.shape[1], Wc.shape[1]
    nslice = (Wv + COUPLE_SLICE - 1) // COUPLE_SLICE
    return ((1 + min(COUPLE_SLICE, Wv) + nslice - 1) * U32 * torch.einsum("dpv,dvt->dpt", a, w),
            (1 + P) * U32 * torch.einsum("dpv,dpt->dvt", a, x),
            P * U32 * a.sum(1))


worst_ratio = vpt_ref.worst_ratio


def synth_couple(depth, P, Wt, Wv, seed, family="decades"):
    """(X, Wc, bc, dY) fp32.  "decades": rows spread over three decades, as `vpt_ref.synth_g`'s; "cancel": every odd column of X repeats the even one before
    it while Wc's odd column is the negated even one plus a 2^-10 relative perturbation, and dY / the rows of Wc likewise in v — sums far below their terms."""
    g = torch.Generator().manual_seed(seed)

    def spread(*shape):
        rows = int(np.prod(shape[:-1]))
        scale = torch.logspace(-3, 0, max(rows, 2))[torch.randperm(max(rows, 2), generator=g)][:rows].reshape(*shape[:-1], 1)
        return torch.randn(*shape, generator=g) * scale

    X, Wc, bc, dY = spread(depth, P, Wt), spread(depth, Wv, Wt) * 0.05, spread(depth, Wv), spread(depth, P, Wv)
    if family == "cancel":
        X[..., 1::2] = X[..., 0::2]
        Wc[..., 1::2] = -Wc[..., 0::2] * (1 + 2.0 ** -10 * torch.randn(depth, Wv, Wt // 2, generator=g))
        dY[..., 1::2] = dY[..., 0::2]
        Wc[:, 1::2, :] = -Wc[:, 0::2, :] * (1 + 2.0 ** -10 * torch.randn(depth, Wv // 2, Wt, generator=g))
        bc = bc * 1e-3
    return X.contiguous(), Wc.contiguous(), bc.contiguous(), dY.contiguous()


# ---- the reference fixtures -----------------------------------------------------------------------------------------------------------------------------

# name -> (tower tag, weight seed, images B, n_ctx P, depth, classes N, input seed, l_eff or None)
FIXTURES = {
    "maple_grad_tiny_p2_d1": ("tiny", 101, 5, 2, 1, 6, 61, None),
    "maple_grad_tiny_p2_d2": ("tiny", 101, 5, 2, 2, 6, 62, None),
    "maple_grad_small_p4_d3": ("small", 102, 6, 4, 3, 7, 63, None),
    "maple_grad_small_p16_d2": ("small", 102, 6, 16, 2, 7, 64, None),       # P at the coupling envelope's edge; vision L = 17 + 16 = 33
    "maple_grad_tiny_p3_d2_trunc": ("tiny", 103, 4, 3, 2, 5, 65, 12),       # L_eff = 12: run truncated and untruncated, equal bits required
}
LOGIT_SCALE = vpt_ref.LOGIT_SCALE
# five SGD steps of run_maple (tower tag, weight seed, images, n_ctx, depth, classes, input seed, learning rate)
SGD_CASE = ("tiny", 105, 8, 2, 2, 6, 67, 0.03)
SGD_REFERENCE_DECREASE = 0.028957      # loss(0) - loss(5) on the reference's fp32 CPU chain: `make_golden_maple.py sgd` prints it


def towers():
    from spec import SMALL, TINY
    return {"tiny": TINY, "small": SMALL}


def fixture_inputs(kw, B, P, depth, N, seed, l_eff=None):
    """Seeded (ctx fp32 [depth, P, Wt], couple_weight [depth, Wv, Wt], couple_bias [depth, Wv], tokens [N, 77], images [B, 3, R, R] fp16-exact fp32,
    labels [B]) — torch's CPU generator; the coupling in nn.Linear's default range U(-1 / sqrt(Wt), 1 / sqrt(Wt))."""
    g = torch.Generator().manual_seed(seed)
    Wt, Wv, R = kw["transformer_width"], kw["vision_width"], kw["image_resolution"]
    ctx = torch.randn(depth, P, Wt, generator=g) * 0.02
    bound = 1.0 / math.sqrt(Wt)
    weight = (torch.rand(depth, Wv, Wt, generator=g) * 2 - 1) * bound
    bias = (torch.rand(depth, Wv, generator=g) * 2 - 1) * bound
    images = torch.randn(B, 3, R, R, generator=g).half().float()
    labels = torch.randint(0, N, (B,), generator=g)
    tokens = coop_ref.prompt_tokens(N, P, kw["vocab_size"], seed + 1000, l_eff)
    return ctx, weight, bias, tokens, images, labels


loss64 = vpt_ref.loss64
