"""CPU restatement of the three kernels of csrc/pclip_tower_optim.hip (optim.TowerAdamW) in fp32 torch / IEEE doubles, operation by operation as the
file's header documents them, and the tolerances under which the restatement itself is graded against float64 (tests/test_tower_optim_cpu.py).
The GPU kernels are graded bit for bit against the restatement (tests/test_gpu_tower_optim.py).

SUM OF SQUARES (derived, not measured).  A chunk's partial is a sum of non-negative terms; on its longest path a term passes 16 fused multiply-adds in
its lane, 6 additions of the wave butterfly and 3 additions over the four waves: SUMSQ_ROUNDINGS = 25, so partial = exact * prod (1 + d_i), |d_i| <=
2^-24, and the relative error is at most (1 + 2^-24)^25 - 1 = SUMSQ_REL_BOUND.  The double-precision sum over the chunks adds n_chunks * 2^-53, which
sumsq_bound() includes; the norm's relative error is half of it (sqrt) plus one rounding to fp32.

UPDATE (measured).  C_UPDATE is twice the worst |w_restated - w_float64| / ulp32(max(|w|, |update|)) that the restatement shows against
torch.optim.AdamW + clip_grad_norm_ in float64 on the master weights over 10 steps, over gradient magnitudes {1e-6, 1e-3, 1}, lr {1e-5, 1e-3}, clipping
on and off (test_tower_optim_cpu.py::test_restatement_against_float64 prints every ratio and asserts the bound):
    `python tests/tower_optim_ref.py` (measure_update_ratios(): torch 2.10 CPU, seed 0, 3000 elements, |w| in [0.02, 0.5], loss scale 1024, wd 0.01):
        worst ratio per case 6.23 .. 9.42, the worst at g 1e-3, lr 1e-5 (9.421 after the tenth step)  ->  C_UPDATE = 18.85
    Most of it is systematic, not noise: the documented sequence rounds 1 - lr wd to fp32 (1 - 1e-7 becomes 1 - 2^-23), a relative bias of 1.9e-8 of
    |w| per step, and every step rounds w twice; ten steps add up almost linearly.
(ulp32(x) = 2^(floor(log2 |x|) - 23), the spacing of fp32 at x; `update` is the float64 step's own |w_after - w_before|.)"""
import math

import numpy as np
import torch

CHUNK = 4096
U32 = 2.0 ** -24
SUMSQ_ROUNDINGS = 25
SUMSQ_REL_BOUND = (1.0 + U32) ** SUMSQ_ROUNDINGS - 1.0
C_UPDATE = 18.85

f32 = np.float32
_INF = float("inf")


def sumsq_bound(n_chunks=0):
    """Relative error bound of a chunk partial (n_chunks = 0) or of the double-precision total over n_chunks partials."""
    return SUMSQ_REL_BOUND + n_chunks * 2.0 ** -53


def t32(x):
    """A Python double rounded once to an fp32 0-dim tensor (how the host hands scalars to the kernels)."""
    return torch.tensor(float(x), dtype=torch.float32)


def fma(a, b, c):
    """Exact fused multiply-add of fp32 tensors: the product is exact in float64, the sum is rounded to odd in float64 (TwoSum supplies the
    sticky bit), so the final rounding to fp32 is the single rounding of a hardware fma."""
    a, b, c = torch.broadcast_tensors(torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32),
                                      torch.as_tensor(c, dtype=torch.float32))
    p, cd = a.double() * b.double(), c.double()
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)
    even = (s.contiguous().view(torch.int64) & 1) == 0
    fix = torch.isfinite(s) & (err != 0) & even
    toward = torch.where(err > 0, torch.full_like(s, _INF), torch.full_like(s, -_INF))
    return torch.where(fix, torch.nextafter(s, toward), s).float()


def chunk_partials(grads, numels):
    """pclip_tower_grad_sumsq: fp32 partials in chunk order.  grads: raw fp16 / fp32 gradient tensors, or None (a zero gradient)."""
    out = []
    for g, n in zip(grads, numels):
        nch = -(-n // CHUNK)
        x = torch.zeros(nch * CHUNK, dtype=torch.float32)
        if g is not None:
            x[:n] = g.detach().reshape(-1).float().cpu()
        seq = x.reshape(nch, 2, 256, 8).permute(0, 2, 1, 3).reshape(nch, 256, 16)         # thread t: elements 2048 j + 8 t + k in (j, k) order
        s = torch.zeros(nch, 256, dtype=torch.float32)
        for i in range(16):
            s = fma(seq[:, :, i], seq[:, :, i], s)                                       # an absent element adds fma(0, 0, s) = s
        w = s.reshape(nch, 4, 64)
        for half in (32, 16, 8, 4, 2, 1):                                                 # the butterfly as lane 0 sees it
            w = w[..., :half] + w[..., half:2 * half]
        w = w[..., 0]
        out.append(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    return torch.cat(out)


def new_state(loss_scale=2.0 ** 16):
    return dict(b1t=1.0, b2t=1.0, total=0.0, scale=float(f32(loss_scale)), tracker=0, step=0, found_inf=0, grad_norm=0.0, clip_coef=0.0, inv_scale=0.0,
                bc1=0.0, sqrt_bc2=0.0, gmul=0.0)


def finish(partials, st, max_norm, beta1, beta2, growth=2.0, backoff=0.5, growth_interval=2000, dynamic=True):
    """pclip_tower_optim_finish on a state dict (fields of optim.STATE_DTYPE; fp32 fields hold fp32 values as Python floats).  Returns the new state."""
    p = [float(x) for x in partials.detach().cpu().tolist()]
    n = len(p)
    per = -(-n // 256)
    total = 0.0
    for t in range(256):
        s = 0.0
        for i in range(t * per, min((t + 1) * per, n)):
            s += p[i]
        total += s
    st = dict(st)
    with np.errstate(all="ignore"):
        scale = f32(st["scale"])
        inv = f32(1.0) / scale
        found = not math.isfinite(total)
        st.update(total=total, found_inf=int(found), inv_scale=float(inv))
        if found:
            st.update(grad_norm=_INF, clip_coef=0.0, gmul=0.0)
            if dynamic:
                st.update(scale=float(scale * f32(backoff)), tracker=0)
            return st
        grad_norm = f32(math.sqrt(total) / float(scale))
        clip = f32(1.0)
        if max_norm is not None and max_norm > 0.0:
            clip = f32(max_norm) / (grad_norm + f32(1e-6))
            clip = clip if clip < f32(1.0) else f32(1.0)
        b1t, b2t = st["b1t"] * beta1, st["b2t"] * beta2
        st.update(grad_norm=float(grad_norm), clip_coef=float(clip), gmul=float(clip * inv), b1t=b1t, b2t=b2t, step=st["step"] + 1,
                  bc1=float(f32(1.0 - b1t)), sqrt_bc2=float(f32(math.sqrt(1.0 - b2t))))
        if dynamic:
            ok = st["tracker"] + 1
            if ok == growth_interval:
                grown = scale * f32(growth)
                if np.isfinite(grown):
                    st["scale"] = float(grown)
                st["tracker"] = 0
            else:
                st["tracker"] = ok
    return st


def update(g_raw, master, m, v, st, lr, wd, decays, beta1=0.9, beta2=0.999, eps=1e-8):
    """pclip_tower_adamw for one tensor, on CPU fp32 tensors; returns (master, m, v) after the step (unchanged after an overflow).  The parameter is
    master.half() for an fp16 parameter and master itself for an fp32 one."""
    if st["found_inf"]:
        return master, m, v
    b1, omb1, b2, omb2, epsf = t32(beta1), t32(1.0 - beta1), t32(beta2), t32(1.0 - beta2), t32(eps)
    gmul, bc1, sbc2 = t32(st["gmul"]), t32(st["bc1"]), t32(st["sqrt_bc2"])
    lr32, wd32 = t32(lr), t32(wd)
    keep, step_size = 1.0 - lr32 * wd32, lr32 / bc1
    g = (torch.zeros_like(master) if g_raw is None else g_raw.detach().cpu().float().reshape(master.shape)) * gmul
    m = fma(omb1, g, b1 * m)
    v = fma(omb2 * g, g, b2 * v)
    w = master * keep if decays else master
    den = torch.sqrt(v) / sbc2 + epsf
    w = w - (step_size * m) / den
    return w, m, v


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor in, float64 out; the smallest normal's spacing below it)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


def run_against_float64(gmag, lr, clip, steps=10, n=3000, seed=0, loss_scale=1024.0, wd=0.01, eps=1e-8):
    """`steps` restated steps (one fp16-parameter tensor of n elements, fp16 gradients scaled by loss_scale) beside torch.optim.AdamW +
    clip_grad_norm_ in float64 on the master weights.  Returns (worst update ratio, worst relative error of grad_norm, worst relative error of the
    partials)."""
    gen = torch.Generator().manual_seed(seed)
    w0 = ((torch.rand(n, generator=gen) * 0.48 + 0.02) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).half().float()
    master, m, v = w0.clone(), torch.zeros(n), torch.zeros(n)
    p64 = torch.nn.Parameter(w0.double())
    opt = torch.optim.AdamW([p64], lr=lr, betas=(0.9, 0.999), eps=eps, weight_decay=wd)
    st = new_state(loss_scale)
    worst = worst_norm = worst_part = 0.0
    for _ in range(steps):
        g16 = (torch.randn(n, generator=gen) * gmag * loss_scale).half()
        part = chunk_partials([g16], [n])
        exact = torch.stack([c.double().pow(2).sum() for c in g16.split(CHUNK)])
        worst_part = max(worst_part, float(((part.double() - exact).abs() / exact).max()))
        st = finish(part, st, clip, 0.9, 0.999, dynamic=False)
        p64.grad = g16.double() / loss_scale
        norm64 = float(torch.nn.utils.clip_grad_norm_([p64], clip)) if clip else float(p64.grad.norm())
        worst_norm = max(worst_norm, abs(st["grad_norm"] - norm64) / norm64)
        before = p64.detach().clone()
        opt.step()
        master, m, v = update(g16, master, m, v, st, lr, wd, True, eps=eps)
        upd = (p64.detach() - before).abs()
        ratio = (master.double() - p64.detach()).abs() / ulp32(torch.maximum(p64.detach().abs(), upd))
        worst = max(worst, float(ratio.max()))
    return worst, worst_norm, worst_part


MEASURE_CASES = [(gmag, lr, clip) for gmag in (1e-6, 1e-3, 1.0) for lr in (1e-5, 1e-3) for clip in (None, 1.0)]


def measure_update_ratios():
    return {case: run_against_float64(*case) for case in MEASURE_CASES}


if __name__ == "__main__":
    for case, (r, rn, rp) in measure_update_ratios().items():
        print("g %-6g lr %-6g clip %-4s  update ratio %.3f ulp32   grad_norm rel %.2e   partial rel %.2e (bound %.2e)" % (*case, r, rn, rp, SUMSQ_REL_BOUND))
