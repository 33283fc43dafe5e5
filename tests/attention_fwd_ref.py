"""The forward attention kernels (pclip_attention_f16 / _q_f16 / _long_q_f16: attn_key_tiles and attn_store_tile of csrc/pclip_attention_tile.h) in
float64 torch from the fp16 operands, with the per-element tolerance they are graded with (tests/test_attention_forward_cpu.py,
tests/test_gpu_attention_forward.py), an emulation of the kernel's walk, wrong walks the tolerance must reject, and the input families that drive the
online-softmax state machine.  Nothing in the tolerance is chosen: every term is a rounding of the kernel.

ROUNDING POINTS (mirrored at the top of attn_key_tiles).  Units u11 = 2^-11 (an fp16 rounding), u24 = 2^-24 (an fp32 rounding), and 2^-25 for the absolute
error of an fp16 rounding in the subnormal range.  Per (sequence, head), S = q k^T / 8, P = softmax(S), O = P V:
    e_S   = 64 u24 |q| |k|^T / 8 + 2 u24 |S|            S^T = K Q^T: fp32 MFMA accumulation of 64 exact products; kScale = log2(e) / 8 is a rounded fp32
                                                          constant and the scale-and-subtract s kScale - max is ONE fma (or v_pk_fma_f32) in the log2 domain
    eps_P = 2 expm1(2 max e_S + 4 u24 (1 + 2 max |S|)) + (L + 16) u24
                                                          relative error of a normalised fp32 P: the score error and the rounding of the fma's result (of size
                                                          <= 2 max |S| log2 e) through v_exp_f32, in the numerator and in the denominator; the rescale factors
                                                          alpha = exp2(mrun - mnew), whose exponents are fp32 differences that telescope to <= 2 max |S| log2 e
                                                          over a row (the maximum only rises) and which multiply lrun and o alike; the row sum; 1.f / lrun and
                                                          the product o * inv of attn_store_tile.
                                                          (L + 16) u24 covers the sum and the per-rescale roundings together: a lane adds its 16 or 32
                                                          probabilities of a key-tile pair one after the other (two interleaved chains with VAR & 2), the
                                                          half-waves are added, then lrun += psum — a chain of at most min(L - 1, 34 + L / 64) roundings that
                                                          are not additions of exact zeros — and each of the <= ceil(L / 64) - 1 rescales of a non-zero state
                                                          adds one v_exp_f32 and one product per side: at most 3 L / 64 more.
    e_P16 = (u11 + eps_P) P + 2^-25  (unmasked pairs)     P rounded to fp16 as it enters O^T = V^T P^T, taken against the RUNNING maximum, which with the
                                                          deferred maximum (VAR & 1) may be stale by up to kAttDefer = 2 in the log2 domain: the rounded
                                                          value is as large as 4 instead of 1, exact in fp32, and the fp16 rounding is relative.  The
                                                          absolute 2^-25 of the subnormal range is taken at the unnormalised scale; the pair that last set the
                                                          maximum contributed exp2(0) = 1 to the row sum and every later alpha is <= 1, so the final row sum is
                                                          >= 1 and an absolute error of 2^-25 made at any pair is at most 2^-25 after the later rescales and
                                                          the normalisation.  Masked pairs are exp2(-inf) = 0 exactly and carry no term.
    A     = e_P16 |V| + L u24 P |V|                       fp32 MFMA accumulation of the second contraction over L keys
    tol   = A + u11 (|ref| + A) + 2^-25                   (half_t)(o * inv): the single fp16 rounding of the output
The walk itself (which maximum a probability is taken against, when the state is rescaled) changes none of these terms: it is exact algebra on the
softmax, and `emulate` below runs it to show that the roundings alone stay inside the bound while a wrong walk does not."""
import math

import torch

from attention_bwd_ref import U11, U24, U25, attention64, causal_mask, clustered_qkv, r16, split_heads, worst_ratio   # noqa: F401

LOG2E = 1.4426950408889634
DEFER = 2.0                                     # kAttDefer: log2 units
F16_MAX = 65504.0
VARIANTS = ("stale_sum", "stale_out", "drop_last_key", "mask_off_by_one", "first_tile_only_max")


def _pack(t):
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * 64)


def _qkv(q, k, v):
    return torch.cat([_pack(q), _pack(k), _pack(v)], dim=2).half().contiguous()


def reference(qkv16, B, L, H, causal, Lq=None):
    """Attention output of the first Lq query rows [B, Lq, H 64] in float64 from the fp16 operands, and its tolerance (same shape)."""
    Lq = L if Lq is None else Lq
    q, k, v = split_heads(qkv16, B, L, H)
    o, p, s = attention64(q, k, v, causal)
    o, p, s, q = o[..., :Lq, :], p[..., :Lq, :], s[..., :Lq, :], q[..., :Lq, :]
    vis = causal_mask(L)[:Lq] if causal else torch.ones(Lq, L, dtype=torch.bool)
    sv = torch.where(vis, s, torch.zeros_like(s)).abs()
    e_s = (64 * U24 * (q.abs() @ k.abs().transpose(-1, -2)) / 8 + 2 * U24 * sv) * vis
    eps_p = 2 * math.expm1(2 * float(e_s.max()) + 4 * U24 * (1 + 2 * float(sv.max()))) + (L + 16) * U24
    e_p16 = (U11 + eps_p) * p + U25 * vis
    a = e_p16 @ v.abs() + L * U24 * (p @ v.abs())
    ref, a = _pack(o), _pack(a)
    return ref, a + U11 * (ref.abs() + a) + U25


def emulate(qkv16, B, L, H, causal, variant=None, stats=None):
    """The kernel's walk in float64 with exactly its documented roundings: keys in pairs of 32-key tiles (64 keys; what is left at the end is the last pair
    or a lone tile), the running maximum deferred by kAttDefer per ROW, P rounded to fp16 against the running maximum as it enters the second contraction,
    one fp16 rounding of the output.  variant: None, or one of the WRONG kernels the bound must reject —
      "stale_sum"            the row sum is not rescaled when the maximum moves
      "stale_out"            the output accumulators are not rescaled
      "drop_last_key"        key L - 1 is masked
      "mask_off_by_one"      causal: key q + 1 is visible
      "first_tile_only_max"  the maximum never moves after the first pair; a probability beyond fp16's range enters the contraction as 65504
    stats (a dict): receives "moves" (rescales of a non-empty state, summed over rows) and "pmax" (the largest unnormalised probability)."""
    assert variant is None or variant in VARIANTS, variant
    q, k, v = split_heads(qkv16, B, L, H)
    s2 = q @ k.transpose(-1, -2) * (0.125 * LOG2E)
    vis = torch.ones(L, L, dtype=torch.bool)
    if causal:
        vis = causal_mask(L)
        if variant == "mask_off_by_one":
            vis = torch.ones(L, L, dtype=torch.bool).tril(1)
    if variant == "drop_last_key":
        vis = vis.clone()
        vis[:, L - 1] = False
    s2 = s2.masked_fill(~vis, -math.inf)
    o = torch.zeros(B, H, L, 64, dtype=torch.float64)
    mrun = torch.full((B, H, L, 1), -math.inf, dtype=torch.float64)
    lrun = torch.zeros(B, H, L, 1, dtype=torch.float64)
    moves, pmax = 0, 0.0
    for k0 in range(0, L, 64):
        st = s2[..., k0:k0 + 64]
        tmax = st.max(dim=-1, keepdim=True).values
        moved = tmax > mrun + DEFER                                     # -inf + 2 = -inf: the first visible key sets the maximum
        if variant == "first_tile_only_max" and k0 > 0:
            moved = torch.zeros_like(moved)
        mnew = torch.where(moved, torch.maximum(mrun, tmax), mrun)
        live = torch.isfinite(mnew)                                     # rows that have seen a key (every row, but for "drop_last_key" at L = 1)
        p = torch.where(live, torch.exp2(st - torch.where(live, mnew, torch.zeros_like(mnew))), torch.zeros_like(st))
        alpha = torch.where(moved & torch.isfinite(mrun), torch.exp2(mrun - mnew), torch.ones_like(mrun))
        moves += int((moved & torch.isfinite(mrun)).sum())
        pmax = max(pmax, float(p.max()))
        lrun = lrun * (1.0 if variant == "stale_sum" else alpha) + p.sum(-1, keepdim=True)
        o = o * (1.0 if variant == "stale_out" else alpha) + r16(p.clamp(max=F16_MAX)) @ v[..., k0:k0 + 64, :]
        mrun = mnew
    if stats is not None:
        stats.update(moves=moves, pmax=pmax)
    return _pack(r16(o / lrun))


# ---- input families: fp16 qkv [B, L, 3 H 64] from a seed, every (sequence, head) its own draw ----------------------------------------------------------
def _unit(g, B, H):
    u = torch.randn(B, H, 1, 64, generator=g)
    return u / u.norm(dim=-1, keepdim=True)


def normal(B, L, H, seed):
    """N(0, 1.5^2): the input of test_gpu_encoder.py::test_attention.  The running maximum is nearly settled after the first pair of key tiles."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, L, 3 * H * 64, generator=g) * 1.5).half().contiguous()


def _along(B, L, H, seed, coord, qamp, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    u = _unit(g, B, H)
    q = qamp * u + noise * torch.randn(B, H, L, 64, generator=g)
    k = coord.view(1, 1, L, 1) * u + noise * torch.randn(B, H, L, 64, generator=g)
    return _qkv(q, k, torch.randn(B, H, L, 64, generator=g))


def ramp(B, L, H, seed, qamp=6.0):
    """Keys along one unit direction scaled by linspace(-8, 8, L), queries `qamp` along it, noise 0.3: the scores rise by 16 qamp / 8 over the sequence
    (17 in the log2 domain at qamp = 6: more than kAttDefer per pair of key tiles up to L = 385), so the maximum moves on every pair."""
    return _along(B, L, H, seed, torch.linspace(-8, 8, L), qamp)


def steep(B, L, H, seed):
    """`ramp` at four times the slope (69 in the log2 domain): a maximum held from the first pair on would push probabilities past fp16's range."""
    return ramp(B, L, H, seed, qamp=24.0)


def creep(B, L, H, seed, qamp=4.5):
    """Key coordinate 2.2 k / 64 along the direction: at qamp = 4.5 the scores rise by 2.2 * 4.5 / 8 * log2(e) = 1.79 per pair of key tiles, just under
    kAttDefer = 2 in the kernel's log2 domain — the maximum is held, probabilities exceed 1 for a pair or two, then it moves."""
    return _along(B, L, H, seed, 2.2 * torch.arange(L, dtype=torch.float32) / 64, qamp)


def descend(B, L, H, seed):
    """`ramp` reversed: the first tile sets the maximum and later probabilities underflow towards fp16's subnormals and zero."""
    return _along(B, L, H, seed, torch.linspace(8, -8, L), 6.0)


def hot25(B, L, H, seed):
    """attention_bwd_ref.clustered_qkv at amp 25: |S| of about 87."""
    return clustered_qkv(B, L, H, seed, amp=25.0)[0]


def hot40(B, L, H, seed):
    """attention_bwd_ref.clustered_qkv at amp 40: |S| of about 213."""
    return clustered_qkv(B, L, H, seed, amp=40.0)[0]


def onehot(B, L, H, seed):
    """k = q with |q| = 12: a row's own key scores 18, the others around 0 +- 2."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, 64, generator=g)
    q = 12 * q / q.norm(dim=-1, keepdim=True)
    return _qkv(q, q, torch.randn(B, H, L, 64, generator=g))


def flat(B, L, H, seed):
    """q = 0: a uniform softmax over the L keys."""
    g = torch.Generator().manual_seed(seed)
    k, v = 1.5 * torch.randn(B, H, L, 64, generator=g), 1.5 * torch.randn(B, H, L, 64, generator=g)
    return _qkv(torch.zeros(B, H, L, 64), k, v)


def bigv(B, L, H, seed):
    """`normal` with V of magnitude 200, its sign alternating between neighbouring keys: the output is a cancellation, sum P |V| much larger than |O|."""
    g = torch.Generator().manual_seed(seed)
    q, k = 1.5 * torch.randn(B, H, L, 64, generator=g), 1.5 * torch.randn(B, H, L, 64, generator=g)
    sign = (1 - 2 * (torch.arange(L) % 2)).view(1, 1, L, 1)
    return _qkv(q, k, sign * (200 + 20 * torch.randn(B, H, L, 64, generator=g)))


def mixed_rows(B, L, H, seed):
    """`ramp` keys and values under queries that differ from row to row inside every 32-row tile: row i is a `ramp` query (i % 3 == 0: its maximum moves on
    every pair), zero (i % 3 == 1: flat, it never moves again) or 16 along the noise part of key i (i % 3 == 2: one-hot, it moves once, at key i's pair)."""
    g = torch.Generator().manual_seed(seed)
    u = _unit(g, B, H)
    n = 0.3 * torch.randn(B, H, L, 64, generator=g)
    k = torch.linspace(-8, 8, L).view(1, 1, L, 1) * u + n
    kind = (torch.arange(L) % 3).view(1, 1, L, 1)
    q = torch.where(kind == 0, 6.0 * u + 0.3 * torch.randn(B, H, L, 64, generator=g),
                    torch.where(kind == 1, torch.zeros(B, H, L, 64), 16 * n / n.norm(dim=-1, keepdim=True)))
    return _qkv(q, k, torch.randn(B, H, L, 64, generator=g))


FAMILIES = {"normal": normal, "ramp": ramp, "creep": creep, "descend": descend, "hot25": hot25, "hot40": hot40, "onehot": onehot, "flat": flat, "bigv": bigv}
