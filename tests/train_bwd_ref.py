"""The backward kernels of the training step — the conv adapter (csrc/pclip_adapter.hip: adapter_conv3x_bwd_mfma_kernel, adapter_conv_backward_kernel;
csrc/pclip_adapter_w.hip: adapter_conv_w_backward_kernel), and layernorm_backward_kernel, proto_backward_kernel and adamw_f16_kernel of csrc/pclip_train.hip —
in float64 torch from the fp16 operands, with the per-element tolerances they are graded with (tests/test_train_backward_cpu.py without a GPU,
tests/test_gpu_train_backward.py on one).  Units: U11 = 2^-11 (an fp16 rounding), U24 = 2^-24 (an fp32 rounding), U25 = 2^-25 (an fp16 rounding in the
subnormal range, absolute).

CONV ADAPTER.  `conv_reference` is float64 autograd of the reference's formula (model.py:49-78 with the LayerNorm shape taken from the weights).
`conv_emulate` is the same float64 graph with a straight-through rounding node behind every tensor that fp16 autograd materialises, as the kernels' header
comments say they round: forward r16(x), backward r16(grad), behind conv1 / LN1 / conv2 / LN2 / conv3 / LN3 and the residual add.  Parameter gradients stay
unrounded (the kernels emit fp32 per-row contributions).  rounding="stochastic" rounds every value to one of its two fp16 neighbours with probability
proportional to proximity.  `variant` names kernels that are WRONG on purpose (VARIANTS) and that the tolerance has to reject.
    tol[e] = C_CONV max(sigma[e], rms(sigma over the tensor) / 4) + A[e]
sigma[e]: RMS distance of N_SIGMA = 16 stochastic emulations from the float64 reference — how far the chain's own fp16 roundings move this element.
A[e]: fp32 arithmetic, derived.  A leaf of a parameter gradient is one product of a row (da xh, da, dt x, dt2 a1 ...); it passes through at most n fp32
additions, n = the pixel chain of its row (conv weights only: <= s^2) + the accumulation over rows, min(B, ceil(B / P) + P) for P partial rows (a workgroup's
rows one after the other, then pclip_colsum_f32 over the partial rows; B - 1 bounds ANY order of adding B rows), and the leaf itself is within 64 U24 of
its scale (LayerNorm statistics are 64-lane trees behind <= 64 in-lane terms, the rest a handful of fp32 operations; xh = (t - mu) rstd is judged at
|xh| + rstd (|t| + |mu|): the subtraction cancels):   A = (n + 64) U24 sum_r |leaf|.   bn3.bias is the plain sum of the exact fp16 g over the rows: sigma = 0
there and it is graded by A = min(B, ceil(B / P) + P) U24 sum_r |g| alone.  The absolute sums come from one RNE emulation of the batch.
C_CONV is MEASURED, not chosen: over CONV_SHAPES (= the GPU test's list) the worst |emulation - float64| / max(sigma, rms sigma / 4) of the RNE emulation
and of N_HELD = 4 stochastic runs held out of the sigma estimate, times 2 (what the emulation does not model: fp32 instead of float64 accumulation flips
fp16 near-ties, which acts like one more rounding draw).
    measured on the CPU (tests/test_train_backward_cpu.py prints them per shape): RNE <= 6.19, held out <= 8.01  ->  C_CONV = 16.1
    the wrong kernels of VARIANTS sit at 3.5e1 ... 1.6e5 times the tolerance (>= 10 at every shape where they differ from the kernel).

LAYERNORM BACKWARD, fp16 gamma, dy_scale (layernorm_backward_kernel).  ANALYTIC, as attention_bwd_ref.layernorm_backward_ref for fp32 gamma: gv = dy if
dy_scale == 1 else r16(f32(dy_scale) dy), e_gv = U11 |gv| + U25 (0 at dy_scale 1); with gy = gv gamma and E = rstd (|gy| + mean |gy| + |xh| mean |gy xh|):
    tol_dx = e + U11 (|ref| + e) + U25,   e = 64 U24 E + rstd (e_gy + mean e_gy + |xh| mean(e_gy |xh|)),  e_gy = e_gv |gamma|
    tol_dgamma = (R + P + 64) U24 sum_r |gv| (|xh| + rstd (|x| + |mu|)) + sum_r e_gv |xh|,   tol_dbeta = (R + P) U24 sum_r |gv| + sum_r e_gv        (P partial rows)

PROTOTYPE CHAIN BACKWARD (proto_backward_kernel).  The SIGMA METHOD: `proto_emulate` is the kernel's r16s sequence (its header comment) in float64 with RNE or
stochastic rounding, tol = C_PROTO max(sigma, rms sigma / 4) + (2^-10 |ref| + U24), sigma from 16 stochastic emulations.  The second term is one fp16 ulp of
the output: the last rounding alone puts a stochastic run on either neighbour, a Bernoulli draw that sixteen runs do not sample at an element that sits close
to an fp16 value (the conv gradients are sums of thousands of rounded leaves and have no such tail).  C_PROTO = 2 x the worst
(|emulation - float64| - that ulp)+ / max(sigma, rms sigma / 4) of the RNE emulation and 4 held-out runs over PROTO_CASES:
    measured RNE <= 3.54, held out <= 7.07  ->  C_PROTO = 14.2.

ADAMW.  `adamw_step` restates the documented sequence of adamw_f16_kernel in fp32 torch on the CPU; the kernel is graded bit for bit against it."""
import functools
import math

import torch
import torch.nn.functional as F

U11, U24, U25 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
N_SIGMA, N_HELD = 16, 4
C_CONV = 16.1
C_PROTO = 14.2
CONV_KEYS = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight", "bn3.bias")
VARIANTS = ("circular_halo",      # (a) conv2's halo read circularly instead of as zeros (the transposed convolution's dt2 operand)
            "unmirrored_taps",    # (b) taps not mirrored in the transposed convolution
            "last_row_dropped",   # (c) the last row of the batch dropped
            "stats_over_D",       # (d) LayerNorm statistics over the first D pixels instead of all s^2
            "ln2_tile_skipped")   # (e) the last 64-pixel tile left out of the LN2 dgamma / dbeta sums


def r16(x):
    """Round a float64 tensor to fp16 (RNE, subnormals kept) and back."""
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def stochastic_r16(x, generator):
    """Each value to one of its two fp16 neighbours, the nearer one with the higher probability (a representable value stays)."""
    _, e = torch.frexp(x)
    ulp = torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-14) - 10)
    lo = torch.floor(x / ulp)
    up = torch.rand(x.shape, generator=generator, dtype=torch.float64) < (x / ulp - lo)
    return (lo + up.to(x.dtype)) * ulp


def rounder(rounding, generator=None):
    if rounding is None:
        return lambda t: t
    if rounding == "rne":
        return r16
    assert rounding == "stochastic" and generator is not None
    return lambda t: stochastic_r16(t, generator)


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a non-finite result as infinity)."""
    got, want, tol = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu(), torch.as_tensor(tol).double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got.reshape(want.shape) - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol.expand_as(err)).max())


# ---- conv adapter ----------------------------------------------------------------------------------------------------------------------
def side(D):
    return int(math.ceil(math.sqrt(D)))


def conv_inputs(kind, W, D, B, seed=0):
    """x unit rows, g ~ 1e-2 N(0, 1) (the scale of the existing tests: inner gradients reach the fp16 subnormal range), both fp16, and fp16 parameters:
    the constructor's draws of Adapter(D, kind, width=W) followed by golden.spec.randomize_adapter_."""
    from golden.spec import randomize_adapter_
    from proto_clip_amd.model import Adapter
    torch.manual_seed(1000 * W + D + seed)
    ad = randomize_adapter_(Adapter(D, c_type=kind, width=W, dtype=torch.half), seed=B + seed)
    params = {k: v.detach().clone() for k, v in ad.state_dict().items()}
    gen = torch.Generator().manual_seed(7 * D + W + seed)
    x = F.normalize(torch.randn(B, D, generator=gen), dim=-1).half()
    g = (torch.randn(B, D, generator=gen) * 1e-2).half()
    return x, g, params


def _leaves(params):
    return {k: v.double().clone().requires_grad_(True) for k, v in params.items()}


def conv_reference(x16, g16, params, kind):
    """{name: gradient} by float64 autograd of the reference's formula."""
    B, D = x16.shape
    s = side(D)
    p = _leaves(params)
    W = p["conv1.weight"].shape[0]
    xi = F.pad(x16.double(), (0, s * s - D)).view(-1, 1, s, s)
    out = F.layer_norm(F.conv2d(xi, p["conv1.weight"]), [W, s, s], p["bn1.weight"], p["bn1.bias"])
    if kind == "conv-3x":
        out = F.layer_norm(F.conv2d(out, p["conv2.weight"], padding=1), [W, s, s], p["bn2.weight"], p["bn2.bias"])
    out = F.layer_norm(F.conv2d(out, p["conv3.weight"]), [1, s, s], p["bn3.weight"], p["bn3.bias"])
    out = (out + xi).view(-1, 1, s * s)[:, :, :D].reshape(-1, D)
    (out * g16.double()).sum().backward()
    return {k: v.grad.detach() for k, v in p.items() if v.grad is not None}


class _Round(torch.autograd.Function):
    """Straight-through rounding node: r(x) forward, r(grad) backward."""
    @staticmethod
    def forward(ctx, x, rnd):
        ctx.rnd = rnd
        return rnd(x)

    @staticmethod
    def backward(ctx, grad):
        return ctx.rnd(grad), None


class _Conv2(torch.autograd.Function):
    """The 3x3 convolution with its backward written out: dW2 = sum_p dt2[co, p] a1[ci, p + tap], da1 = the correlation of the zero-padded dt2 with w2
    transposed and mirrored.  variant "circular_halo" pads dt2 circularly, "unmirrored_taps" leaves the taps as they are."""
    @staticmethod
    def forward(ctx, a, w, variant):
        ctx.save_for_backward(a, w)
        ctx.variant = variant
        return F.conv2d(a, w, padding=1)

    @staticmethod
    def backward(ctx, d):
        a, w = ctx.saved_tensors
        gw = torch.nn.grad.conv2d_weight(a, w.shape, d, padding=1)
        wt = w.transpose(0, 1)
        if ctx.variant != "unmirrored_taps":
            wt = wt.flip(2, 3)
        dp = F.pad(d, (1, 1, 1, 1), mode="circular") if ctx.variant == "circular_halo" else F.pad(d, (1, 1, 1, 1))
        return F.conv2d(dp, wt), gw, None


def _ln(t, w, b, D=None):
    """LayerNorm over (C, s, s) written out; D: the WRONG statistics of variant "stats_over_D" (the first D pixels of every channel)."""
    Bn, C, s, _ = t.shape
    src = t if D is None else t.reshape(Bn, C, s * s)[:, :, :D]
    mu = src.reshape(Bn, -1).mean(1).view(Bn, 1, 1, 1)
    var = ((src - (mu if D is None else mu.view(Bn, 1, 1))) ** 2).reshape(Bn, -1).mean(1).view(Bn, 1, 1, 1)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    return (t - mu) * rstd * w + b, mu, rstd


def conv_emulate(x16, g16, params, kind, rounding="rne", generator=None, variant=None, want_sums=False):
    """{name: gradient} of the float64 graph with the kernels' rounding points (module docstring); rounding=None: no rounding at all (= conv_reference).
    want_sums: also {name: sum over the rows of the |leaves| of that gradient} for the accumulation term A."""
    assert variant is None or variant in VARIANTS
    if variant == "last_row_dropped":
        x16, g16 = x16[:-1], g16[:-1]
    B, D = x16.shape
    s = side(D)
    s2 = s * s
    three = kind == "conv-3x"
    p = _leaves(params)
    W = p["conv1.weight"].shape[0]
    if B == 0:
        return {k: torch.zeros_like(v) for k, v in p.items() if three or "2" not in k}
    rnd = rounder(rounding, generator)
    R = lambda t: _Round.apply(t, rnd)
    dstat = D if variant == "stats_over_D" else None
    xi = F.pad(x16.double(), (0, s2 - D)).view(-1, 1, s, s)
    t1 = R(F.conv2d(xi, p["conv1.weight"]))
    y1, mu1, rs1 = _ln(t1, p["bn1.weight"], p["bn1.bias"], dstat)
    a1 = R(y1)
    last = a1
    if three:
        t2 = R(_Conv2.apply(a1, p["conv2.weight"], variant))
        y2, mu2, rs2 = _ln(t2, p["bn2.weight"], p["bn2.bias"], dstat)
        last = a2 = R(y2)
    u = R(F.conv2d(last, p["conv3.weight"]))
    y3, mu3, rs3 = _ln(u, p["bn3.weight"], p["bn3.bias"], dstat)
    out = R(R(y3) + xi)
    kept = [t1, a1, u] + ([t2, a2] if three else [])
    if want_sums:
        for t in kept:
            t.retain_grad()
    gfull = F.pad(g16.double(), (0, s2 - D)).view(-1, 1, s, s)
    (out * gfull).sum().backward()
    grads = {k: v.grad.detach() for k, v in p.items() if v.grad is not None}
    if variant == "ln2_tile_skipped" and three:
        lo = 64 * ((s2 + 63) // 64 - 1)
        for k in ("bn2.weight", "bn2.bias"):
            grads[k] = grads[k].clone()
            grads[k].view(W, s2)[:, lo:] = 0
    if not want_sums:
        return grads
    with torch.no_grad():
        xh_scale = lambda t, mu, rs: ((t - mu) * rs).abs() + rs * (t.abs() + mu.abs())
        dt1, da1, du = (rnd(t.grad).abs() for t in (t1, a1, u))
        sums = {"conv1.weight": (dt1 * xi.abs()).sum((0, 2, 3)).view(W, 1, 1, 1), "bn1.weight": (da1 * xh_scale(t1, mu1, rs1)).sum(0), "bn1.bias": da1.sum(0),
                "conv3.weight": (du * last.abs()).sum((0, 2, 3)).view(1, W, 1, 1), "bn3.weight": (gfull.abs() * xh_scale(u, mu3, rs3)).sum(0),
                "bn3.bias": gfull.abs().sum(0)}
        if three:
            dt2, da2 = rnd(t2.grad).abs(), rnd(a2.grad).abs()
            sums.update({"conv2.weight": torch.nn.grad.conv2d_weight(a1.abs(), p["conv2.weight"].shape, dt2, padding=1),
                         "bn2.weight": (da2 * xh_scale(t2, mu2, rs2)).sum(0), "bn2.bias": da2.sum(0)})
    return grads, sums


def accumulation_steps(B, partial_rows=None):
    """fp32 additions a row's contribution passes on its way into the sum over B rows: a workgroup's rows one after the other and the column sum over the P
    partial rows, ceil(B / P) + P; never more than B (any order of adding B rows)."""
    if not partial_rows:
        return B
    return min(B, -(-B // partial_rows) + partial_rows)


def conv_accumulation_bound(sums, B, D, partial_rows=None, leaf_error=True):
    """A of the module docstring, {name: tensor}.  leaf_error=False: the bound on the difference of two fp32 summations of the SAME leaves (a batch against its
    rows one at a time): the pixel chains of both (conv weights) and the row accumulation only."""
    s2 = side(D) ** 2
    n = accumulation_steps(B, partial_rows)
    out = {}
    for k, v in sums.items():
        if k == "bn3.bias":
            out[k] = n * U24 * v
        elif leaf_error:
            out[k] = (n + 64 + (s2 if k.startswith("conv") else 0)) * U24 * v
        else:
            out[k] = (n + 1 + (2 * max(s2, 32) if k.startswith("conv") else 0)) * U24 * v
    return out


def floored(sigma):
    return torch.maximum(sigma, 0.25 * sigma.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def conv_case(kind, W, D, B, seed=0):
    """Inputs, float64 reference, sigma (N_SIGMA stochastic emulations), N_HELD held-out stochastic runs, the RNE emulation and the absolute sums of a shape —
    computed once per process and shared by the CPU and the GPU tests; nothing in it is modified afterwards."""
    x, g, params = conv_inputs(kind, W, D, B, seed)
    ref = conv_reference(x, g, params, kind)
    gen = torch.Generator().manual_seed(991 + D + W)
    sq = {k: torch.zeros_like(v) for k, v in ref.items()}
    for _ in range(N_SIGMA):
        run = conv_emulate(x, g, params, kind, "stochastic", gen)
        for k in sq:
            sq[k] += (run[k] - ref[k]) ** 2
    sigma = {k: (v / N_SIGMA).sqrt() for k, v in sq.items()}
    held = [conv_emulate(x, g, params, kind, "stochastic", gen) for _ in range(N_HELD)]
    rne, sums = conv_emulate(x, g, params, kind, "rne", want_sums=True)
    return dict(kind=kind, W=W, D=D, B=B, x=x, g=g, params=params, ref=ref, sigma=sigma, held=held, rne=rne, sums=sums)


def conv_tolerance(case, partial_rows=None, c=None):
    """{name: per-element tolerance} of a conv_case."""
    c = C_CONV if c is None else c
    A = conv_accumulation_bound(case["sums"], case["B"], case["D"], partial_rows)
    return {k: (c * floored(case["sigma"][k]) if k != "bn3.bias" else 0) + A[k] for k in case["ref"]}


def conv_sigma_ratios(case):
    """(worst RNE ratio, worst held-out ratio) against max(sigma, rms sigma / 4): the two numbers C_CONV is set from (bn3.bias has sigma = 0: not counted)."""
    keys = [k for k in case["ref"] if k != "bn3.bias"]
    rne = max(worst_ratio(case["rne"][k], case["ref"][k], floored(case["sigma"][k])) for k in keys)
    held = max(worst_ratio(h[k], case["ref"][k], floored(case["sigma"][k])) for h in case["held"] for k in keys)
    return rne, held


# the GPU test's shapes (kind, W, D, B, chunk), each for an edge (s = ceil(sqrt(D)), NT = ceil(s^2 / 64)):
CONV_MFMA = [("conv-3x", 16, D, 16, 512) for D in (3, 64, 65, 200, 256, 257, 512, 576)]          # the persistent MFMA kernel
# the per-row VALU kernel at width 16; chunk 5 walks 16 rows as 5 + 5 + 5 + 1: a ragged last chunk that is a single row
CONV_VALU = [("conv-3x", 16, 577, 16, 5), ("conv-3x", 16, 1024, 16, 5), ("conv-2x", 16, 100, 16, 5), ("conv-2x", 16, 640, 16, 5), ("conv-2x", 16, 1024, 16, 5)]
# widths 8 / 24 / 32 with chunk=16: rows per launch = 16 * 16 // W = 32 (one chunk), 10 (10 + 6), 8 (8 + 8)
CONV_WIDTHS = [(kind, W, D, 16, 16) for W in (8, 24, 32) for kind, D in (("conv-3x", 200), ("conv-3x", 1024), ("conv-2x", 640))]
CONV_SHAPES = CONV_MFMA + CONV_VALU + CONV_WIDTHS


# ---- LayerNorm backward with fp16 gamma and dy_scale ----------------------------------------------------------------------------------------
def ln_inputs(R, D, seed=0):
    gen = torch.Generator().manual_seed(1000 * R + D + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return (rn(R, D) * 1.5 + 0.2).half(), (1 + 0.2 * rn(D)).half(), (rn(R, D) * 0.01).half()


def _ln_gv(dy16, dy_scale):
    if dy_scale == 1.0:
        return dy16.double(), torch.zeros(dy16.shape, dtype=torch.float64)
    gv = (torch.tensor(dy_scale, dtype=torch.float32) * dy16.float()).half().double()            # the kernel's r16s(dy_scale * dy), dy_scale an fp32
    return gv, U11 * gv.abs() + U25


def ln_backward_ref(x16, gamma16, dy16, dy_scale=1.0, partial_rows=None, eps=1e-5):
    """(dx, dgamma, dbeta) of sum(dy_scale * LN(x) * dy) in float64 and their tolerances (module docstring)."""
    x, gam, dy = x16.double(), gamma16.double(), dy16.double()
    R, D = x.shape
    P = max(1, min(256, (R + 3) // 4)) if partial_rows is None else partial_rows
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    gv = float(torch.tensor(dy_scale, dtype=torch.float32)) * dy if dy_scale != 1.0 else dy
    _, e_gv = _ln_gv(dy16, dy_scale)
    gy, e_gy = gv * gam, e_gv * gam.abs()
    m = lambda t: t.mean(1, keepdim=True)
    dx = rstd * (gy - m(gy) - xh * m(gy * xh))
    E = rstd * (gy.abs() + m(gy.abs()) + xh.abs() * m((gy * xh).abs()))
    e = 64 * U24 * E + rstd * (e_gy + m(e_gy) + xh.abs() * m(e_gy * xh.abs()))
    tol_dx = e + U11 * (dx.abs() + e) + U25
    dg, db = (gv * xh).sum(0), gv.sum(0)
    tol_dg = (R + P + 64) * U24 * (gv.abs() * (xh.abs() + rstd * (x.abs() + mu.abs()))).sum(0) + (e_gv * xh.abs()).sum(0)
    tol_db = (R + P) * U24 * gv.abs().sum(0) + e_gv.sum(0)
    return (dx, dg, db), (tol_dx, tol_dg, tol_db)


def ln_backward_emulate(x16, gamma16, dy16, dy_scale=1.0, eps=1e-5, variant=None):
    """The kernel's r16s sequence: gv = r16(dy_scale dy) (dy_scale != 1), dx rounded once, dgamma / dbeta fp32 sums (float64 here).  variant "scale_dropped":
    a WRONG kernel that ignores dy_scale."""
    x, gam = x16.double(), gamma16.double()
    gv, _ = _ln_gv(dy16, 1.0 if variant == "scale_dropped" else dy_scale)
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    gy = gv * gam
    dx = r16(rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True)))
    return dx, (gv * xh).sum(0), gv.sum(0)


LN_ROWS, LN_WIDTHS, LN_SCALES = (1, 3, 4, 5, 1024), (1, 63, 64, 65, 640, 2048), (1.0, 0.2)


# ---- prototype chain backward -----------------------------------------------------------------------------------------------------------
def proto_inputs(N, K, D, seed=0):
    gen = torch.Generator().manual_seed(N * K + D + seed)
    return (torch.randn(N * K, D, generator=gen) * 0.7).half(), (torch.randn(N, D, generator=gen) * 0.05).float()


def proto_reference(mem16, g32, N, K, per_shot, final):
    """Gradient wrt the rows by float64 autograd of the chain (main.py:260-264), no rounding anywhere."""
    mem = mem16.double().clone().requires_grad_(True)
    zs = mem.view(N, K, -1)
    if per_shot:
        zs = zs / zs.norm(dim=-1, keepdim=True)
    z = zs.mean(dim=1)
    if final:
        z = z / z.norm(dim=-1, keepdim=True)
    (z * g32.double()).sum().backward()
    return mem.grad.detach()


def proto_emulate(mem16, g32, N, K, per_shot, final, rounding="rne", generator=None, variant=None):
    """proto_backward_kernel's sequence (its header comment) with every r16s a rounding of the chosen kind.  variant "norm_term_dropped": a WRONG kernel
    without the gradient through the shot's norm (dx2)."""
    rnd = rounder(rounding, generator)
    v = mem16.double().view(N, K, -1)
    g = g32.double()
    nk = rnd(v.norm(dim=-1, keepdim=True))
    zh = rnd(v / nk) if per_shot else v
    m = rnd(zh.mean(dim=1))
    if final:
        nrm = m.norm(dim=-1, keepdim=True)
        gm = (g - (m / nrm) * ((m * g).sum(-1, keepdim=True) / nrm)) / nrm
    else:
        gm = g
    gk = rnd(rnd(gm) / K).unsqueeze(1).expand(N, K, -1)
    if not per_shot:
        return gk.reshape(N * K, -1).clone()
    dn = rnd(rnd(-gk * rnd(zh / nk)).sum(-1, keepdim=True))
    if variant == "norm_term_dropped":
        return rnd(gk / nk).reshape(N * K, -1)
    return rnd(rnd(gk / nk) + rnd(v * rnd(dn / nk))).reshape(N * K, -1)


# K in {1, 2, 32}, D in {70 (D % 8 != 0: the kernel without the LDS copy of the rows), 512, 3072}, N in {1, 5, 1000} (one wave per class, four per workgroup:
# 250 workgroups), per_shot x final_norm.  N = 1000 at the (K, D) where sixteen float64 emulations take seconds, K = 32 there with both normalisations only.
PROTO_FLAGS = [(True, True), (True, False), (False, True), (False, False)]
PROTO_CASES = ([(N, K, D, ps, fin) for N in (1, 5) for K in (1, 2, 32) for D in (70, 512, 3072) for ps, fin in PROTO_FLAGS]
               + [(1000, K, D, ps, fin) for K, D in ((1, 70), (2, 512)) for ps, fin in PROTO_FLAGS] + [(1000, 32, 70, True, True)])


@functools.lru_cache(maxsize=None)
def proto_case(N, K, D, per_shot, final):
    mem, g = proto_inputs(N, K, D)
    ref = proto_reference(mem, g, N, K, per_shot, final)
    gen = torch.Generator().manual_seed(17 + N + K + D)
    sq = torch.zeros_like(ref)
    for _ in range(N_SIGMA):
        sq += (proto_emulate(mem, g, N, K, per_shot, final, "stochastic", gen) - ref) ** 2
    sigma = (sq / N_SIGMA).sqrt()
    held = [proto_emulate(mem, g, N, K, per_shot, final, "stochastic", gen) for _ in range(N_HELD)]
    rne = proto_emulate(mem, g, N, K, per_shot, final, "rne")
    return dict(mem=mem, g=g, ref=ref, sigma=sigma, held=held, rne=rne)


def proto_final_rounding(case):
    """One fp16 ulp of the output: which of its two neighbours the LAST rounding picks."""
    return 2.0 ** -10 * case["ref"].abs() + U24


def proto_tolerance(case, c=None):
    return (C_PROTO if c is None else c) * floored(case["sigma"]) + proto_final_rounding(case)


def proto_sigma_ratios(case):
    """(RNE, worst held-out run): max (|emulation - float64| - one output ulp)+ / max(sigma, rms sigma / 4)."""
    fl, fin = floored(case["sigma"]) + 1e-300, proto_final_rounding(case)
    excess = lambda t: float((((t - case["ref"]).abs() - fin).clamp_min(0) / fl).max())
    return excess(case["rne"]), max(excess(h) for h in case["held"])


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------
def adamw_step(p16, g16, m16, v16, lr, step, beta1=0.9, beta2=0.999, eps=1e-4, weight_decay=0.05):
    """One step of adamw_f16_kernel's documented sequence on CPU fp16 tensors, in place; fp32 opmath, the scalars prepared in double and cast once:
       p = r16(p (1 - lr wd));  m = r16(fma(1 - b1, g - m, m));  v = r16(fma((1 - b2) g, g, r16(v b2)))
       denom = r16(r16(r16(sqrt v) / sqrt(bc2)) + eps);  p = r16(p + (-step_size m) / denom)
    The two fused multiply-adds round once: their products are formed exactly in float64."""
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    h = lambda t: t.to(torch.float16).to(torch.float32)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    decay, w1, b2, omb2 = f32(1.0 - lr * weight_decay), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)
    bc2s, epsf, nss = f32(math.sqrt(bc2)), f32(eps), f32(-(lr / bc1))
    assert float(w1) < 0.5                                                                          # torch's lerp takes its other branch at weight >= 0.5
    g, p, m0 = g16.float(), h(p16.float() * decay), m16.float()
    m = h((w1.double() * (g - m0).double() + m0.double()).float())
    v = h(v16.float() * b2)
    v = h(((omb2 * g).double() * g.double() + v.double()).float())
    den = h(h(h(torch.sqrt(v)) / bc2s) + epsf)
    p = h(p + (nss * m) / den)
    p16.copy_(p.half())
    m16.copy_(m.half())
    v16.copy_(v.half())
    return p16
