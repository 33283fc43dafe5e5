"""Tip-Adapter's cache logits (pclip_tip_logits_f16 / pclip_tip_grid_f16 / pclip_tip_keys_backward_f16, csrc/pclip_tip.hip) in float64 torch from the fp16 operands,
with autograd for the key gradient, and the per-element tolerances the kernels are graded with, derived from their documented roundings
(tests/test_tip_adapter_cpu.py, tests/test_gpu_tip_adapter.py).

The function (include/pclip.h), f [Q, D], keys [NK, D] sorted by class, seg [N + 1], w [N, D] fp16; alpha, beta, scale as fp32 numbers:
    aff = f keys^T,  x = beta (aff - 1),  E = exp(x),  S[q, n] = sum of E[q, j] over class n's rows,
    c = r16(scale f) w^T,  v = c + alpha S  (the fp32 logits of the taped path),  logit = r16(v).
r16(scale f) is part of the function's definition, as in tests/contrastive_ref.py: it is what `100. * features` is in upstream's fp16 tensors and what
utils.clip_logits computes, so it is an operand here, not an error term (against the unrounded 100 f w^T it moves a logit by up to 2^-11 scale |f| . |w|).

The kernel's roundings and what each may cost, per element (U24 = 2^-24, the unit of one fp32 rounding):
    c      fp32 summation of D exact products, any order:          dc    = D U24 ||r16(scale f_q)|| ||w_n||
    aff    the same:                                               daff  = D U24 ||f_q|| ||keys_j||
    x      one fma, the argument error beta d(aff):                dx    = beta daff + U24 |x|
    E      hardware exp2 of x log2(e) (include/pclip.h):           relE  = expm1(dx) + (|x| + 2) 2^-22;  an E below 2^-126 may flush to zero: + 2^-126
    S      K_n - 1 sequential fp32 additions of positive terms:    dS    = sum_j (E relE + 2^-126) + (K_n - 1) U24 sum_j E (1 + relE)
    v      one fma:                                                tol32 = dc + alpha dS + U24 (|v| + dc + alpha dS)
    logit  the one fp16 rounding:                                  tol16 = tol32 + ulp16(|v| + tol32) / 2
A query is a PROVEN near-tie when its float64 top-two gap is at most the sum of the two elements' tol16: only there may an argmax differ from float64's.

Key gradient, for a loss L of the fp32 logits with upstream gradient dL [Q, N] (fp32):   dkeys[j, :] = alpha beta sum_q dL[q, class(j)] E[q, j] f[q, :].
The kernel recomputes E (relE as above), forms G = dL E in fp32 (one rounding), rounds 2^s G to fp16 for the second matrix product (s an exact power of two from
max |dL|, 2^s max |dL| in (2^13, 2^14]: unit 2^-11 down to |G| = 2^-27 max |dL| and an absolute 2^-38 max |dL| below that; the bound here keeps the coarser
2^-25 max |dL| for that floor), sums over q in fp32 and multiplies by alpha beta in fp32:
    tol_dkeys[j, d] = c alpha beta ( sum_q |dL| E (relE + 2^-11 + (Q + 2) U24) |f[q, d]|  +  2^-25 max|dL| sum_q |f[q, d]| ),   c = 2
(c pays for second-order terms, as in tests/cosine_ce_ref.py)."""
import numpy as np
import torch

from contrastive_ref import scaled_rows, ulp16

U24, U22, U11 = 2.0 ** -24, 2.0 ** -22, 2.0 ** -11
TINY = 2.0 ** -126
C = 2.0
SCALE = 100.0

# (alpha, beta) points every case is graded at
POINTS = [(1.0, 5.5), (0.1, 0.1), (3.0, 7.0), (17.0, 1.0), (50.0, 50.0), (0.0, 5.5)]

# name -> (N, shots per class, D, Q, sigma); shared = 2 throughout
CASES = {
    "ragged3": (3, [1, 5, 70], 64, 70, 2.0),            # a segment longer than a 64-row tile, a segment of one, NK = 76
    "gap": (5, [3, 0, 4, 0, 2], 64, 17, 2.0),           # empty classes
    "pets": (37, [4] * 37, 512, 130, 3.0),              # mid-sized class count; a query equal to a cache key is appended (Q = 131)
    "eurosat": (10, [16] * 10, 512, 300, 3.0),          # few classes, many shots
    "caltech1": (100, [1] * 100, 1024, 160, 3.0),       # one shot per class
    "imagenet_sub": (1000, [16] * 1000, 512, 256, 3.0),  # NK = 16 000
    "one": (37, [4] * 37, 512, 1, 3.0),                 # Q = 1
    "many": (37, [4] * 37, 512, 20000, 3.0),            # more query panels than any launch has workgroups resident
    "d2048": (5, [3] * 5, 2048, 20, 2.0),               # the envelope's edge in D
}


# Shapes past the thresholds at which the launchers take their widest query panels (the panel shrinks until a launch has 512 workgroups): 64 rows per panel
# from Q = 32 705 at D <= 512, 32 rows from Q = 16 353 at D = 1024 (forward), and the grid's 32-row panels.  Small N and NK keep them cheap.
WIDE_CASES = {
    "wide512": (3, [2, 1, 3], 512, 32768 + 5, 2.0),
    "wide1024": (4, [1, 3, 0, 2], 1024, 16384 + 3, 2.0),
}
CASES_ALL = dict(CASES, **WIDE_CASES)


def tip_split(N, shots, D, Q, seed=1, sigma=3.0, shared=2.0):
    """Seeded Tip-Adapter inputs on the portable generator of proto_clip_amd.synth: class centres c_n ~ N(0, I), an image feature (cache key or query) is
    normalize(c_n + sigma eps + shared u) with ONE u ~ N(0, I) added to every image feature — the common direction that puts affinities where CLIP's lie
    (own class ~ (1 + shared^2) / (1 + sigma^2 + shared^2), other classes ~ shared^2 / (...)); text rows as synth.make_split makes them.
    Returns a dict: keys [NK, D] fp16 sorted by class, key_labels [NK], seg [N + 1] int32, text [N, D] fp16, features [Q, D] fp16, labels [Q] int64."""
    from proto_clip_amd import synth
    shots = [int(s) for s in shots]
    assert len(shots) == N
    key_labels = np.repeat(np.arange(N), shots)
    NK = int(key_labels.shape[0])
    centres = synth.normal((N, D), seed, 0)
    u = synth.normal((D,), seed, 7)
    sup = centres[key_labels] + sigma * synth.normal((NK, D), seed, 1) + shared * u
    keys = synth._l2n_f16(torch.from_numpy(sup).float())
    text = synth._l2n_f16(torch.from_numpy(centres + 0.5 * synth.normal((N, D), seed, 2)).float())
    y = synth.randint(Q, N, seed, 100)
    feats = synth._l2n_f16(torch.from_numpy(centres[y] + sigma * synth.normal((Q, D), seed, 3) + shared * u).float())
    seg = np.zeros(N + 1, dtype=np.int32)
    seg[1:] = np.cumsum(shots)
    return dict(keys=keys, key_labels=torch.from_numpy(key_labels), seg=torch.from_numpy(seg), text=text, features=feats, labels=torch.from_numpy(y),
                N=N, D=D, NK=NK, shots=shots)


_SPLITS = {}


def case(name):
    """The inputs of a named case (built once, never modified)."""
    if name not in _SPLITS:
        N, shots, D, Q, sigma = CASES_ALL[name]
        s = tip_split(N, shots, D, Q, seed=11 + len(name), sigma=sigma)
        if name == "pets":                              # a query equal to a cache key: affinity 1 up to rounding, the exponent at zero
            s["features"] = torch.cat([s["features"], s["keys"][5:6]])
            s["labels"] = torch.cat([s["labels"], s["key_labels"][5:6]])
        _SPLITS[name] = s
    return _SPLITS[name]


def f32(v):
    return float(np.float32(v))


def segment_sum(E, seg):
    """[Q, NK] -> [Q, N]: the sum over each class's rows (float64; differentiable)."""
    seg = [int(s) for s in seg]
    cols = [E[:, seg[n]:seg[n + 1]].sum(1) for n in range(len(seg) - 1)]
    return torch.stack(cols, 1)


class Exact:
    """Everything that does not depend on (alpha, beta), in float64, for one set of operands."""

    def __init__(self, f16, keys16, seg, w16, scale=SCALE):
        self.f16, self.keys16, self.w16 = f16.cpu(), keys16.cpu(), w16.cpu()
        self.seg = [int(s) for s in seg]
        self.N, self.D = self.w16.shape[0], self.f16.shape[1]
        f, k, w = self.f16.double(), self.keys16.double(), self.w16.double()
        xs = scaled_rows(self.f16, f32(scale)).double()
        self.aff = f @ k.t()
        self.c = xs @ w.t()
        self.dc = self.D * U24 * xs.norm(dim=1)[:, None] * w.norm(dim=1)[None, :]
        self.daff = self.D * U24 * f.norm(dim=1)[:, None] * k.norm(dim=1)[None, :]
        self.counts = torch.tensor([self.seg[n + 1] - self.seg[n] for n in range(self.N)], dtype=torch.float64)

    def E_and_rel(self, beta):
        b = f32(beta)
        x = b * (self.aff - 1.0)
        E = torch.exp(x)
        rel = torch.expm1(b * self.daff + U24 * x.abs()) + (x.abs() + 2.0) * U22
        return E, rel

    def at(self, alpha, beta):
        """dict: v (the float64 logits), tol32, tol16, S, and the near-tie data (top1, gap, allowance)."""
        a = f32(alpha)
        E, rel = self.E_and_rel(beta)
        S = segment_sum(E, self.seg)
        dS = segment_sum(E * rel + TINY, self.seg) + (self.counts - 1).clamp_min(0)[None, :] * U24 * segment_sum(E * (1 + rel), self.seg)
        v = self.c + a * S
        err = self.dc + a * dS
        tol32 = err + U24 * (v.abs() + err)
        tol16 = tol32 + 0.5 * ulp16(v.abs() + tol32)
        return dict(v=v, S=S, tol32=tol32, tol16=tol16)


def near_ties(v, tol16):
    """(argmax [Q], proven near-tie mask [Q]) of float64 logits: the top-two gap is at most the sum of the two elements' tolerances.  N = 1 has none."""
    if v.shape[1] < 2:
        return v.argmax(1), torch.zeros(v.shape[0], dtype=torch.bool)
    top = v.topk(2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    allow = tol16.gather(1, top.indices).sum(1)
    return top.indices[:, 0], gap <= allow


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the elements (0 / 0 counts as 0; a non-finite result is inf)."""
    got, want, tol = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double(), torch.as_tensor(tol).double()
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.expand_as(err))
    return float(r.max())


def upstream_fp16_chain(f16, keys16, seg, w16, alpha, beta, scale=SCALE):
    """Upstream's fp16 tensor chain restated on the CPU (a yardstick, nothing is graded against it): every tensor op of
        affinity = features @ cache_keys;  cache_logits = ((-1) * (beta - beta * affinity)).exp() @ cache_values;  100. * features @ clip_weights + cache_logits * alpha
    rounds its result to fp16 (matrix products accumulate in fp32 first, as the GPU BLAS does)."""
    h = lambda t: t.half().float()
    f, k, w = f16.float(), keys16.float(), w16.float()
    aff = h(f @ k.t())
    e = h(torch.exp(h(-h(f32(beta) - h(f32(beta) * aff)))))
    onehot = torch.zeros(k.shape[0], w.shape[0])
    for n in range(w.shape[0]):
        onehot[int(seg[n]):int(seg[n + 1]), n] = 1.0
    cache_logits = h(e @ onehot)
    clip_logits = h(h(f32(scale) * f) @ w.t())
    return h(clip_logits + h(cache_logits * f32(alpha))).half()


# ---- the documented walk with its roundings emulated in numpy (and the wrong walks the tolerance must catch) ----------------------------------

WRONG_WALKS = ("aff_fp16", "boundary_off_by_one", "alpha_on_zero_shot", "no_one_minus", "class_sum_fp16")


def emulate(ex, alpha, beta, wrong=None):
    """(fp32 logits, fp16 logits) of the kernel's walk: float64 dot products rounded to fp32 where the kernel holds an fp32 accumulator, the fma and the exponential
    rounded once, the class sums as sequential fp32 additions in ascending row order, one fp16 rounding at the end.  wrong: one of WRONG_WALKS."""
    a, b = np.float32(alpha), np.float32(beta)
    aff = ex.aff.numpy().astype(np.float32)
    if wrong == "aff_fp16":
        aff = aff.astype(np.float16).astype(np.float32)
    x = (np.float64(b) * aff.astype(np.float64) - np.float64(b)).astype(np.float32)          # one fma
    if wrong == "no_one_minus":
        x = (-(np.float64(b) * aff.astype(np.float64))).astype(np.float32)
    E = np.exp(x.astype(np.float64)).astype(np.float32)
    seg = list(ex.seg)
    if wrong == "boundary_off_by_one":
        seg = [seg[0]] + [min(s + 1, seg[-1]) for s in seg[1:-1]] + [seg[-1]]
    Q, N = aff.shape[0], ex.N
    acc_t = np.float16 if wrong == "class_sum_fp16" else np.float32
    S = np.zeros((Q, N), dtype=acc_t)
    lens = np.array([seg[n + 1] - seg[n] for n in range(N)])
    starts = np.array(seg[:-1])
    for i in range(int(lens.max()) if N else 0):                                            # the i-th row of every class that has one: ascending j per class
        live = np.nonzero(lens > i)[0]
        S[:, live] = (S[:, live] + E[:, starts[live] + i].astype(acc_t)).astype(acc_t)
    S = S.astype(np.float32)
    c = ex.c.numpy().astype(np.float32)
    if wrong == "alpha_on_zero_shot":
        v = (np.float64(a) * c.astype(np.float64) + S.astype(np.float64)).astype(np.float32)
    else:
        v = (np.float64(a) * S.astype(np.float64) + c.astype(np.float64)).astype(np.float32)  # one fma
    return torch.from_numpy(v), torch.from_numpy(v.astype(np.float16))


# ---- the key gradient ----------------------------------------------------------------------------------------------------------------------------

def keys_backward(ex, alpha, beta, dL):
    """(dkeys float64 [NK, D] by autograd, tolerance [NK, D]) for the upstream gradient dL [Q, N] (taken as its fp32 values)."""
    a, b = f32(alpha), f32(beta)
    dL = dL.float().double().cpu()
    k = ex.keys16.double().requires_grad_(True)
    f = ex.f16.double()
    S = segment_sum(torch.exp(b * (f @ k.t() - 1.0)), ex.seg)
    ((a * S) * dL).sum().backward()
    E, rel = ex.E_and_rel(beta)
    cls = torch.repeat_interleave(torch.arange(ex.N), ex.counts.long())
    g = dL[:, cls].abs() * E                                                                 # |G| [Q, NK]
    Q = f.shape[0]
    gmax = float(dL.abs().max())
    tol = C * a * b * ((g * (rel + U11 + (Q + 2) * U24)).t() @ f.abs() + 2.0 ** -25 * gmax * f.abs().sum(0)[None, :])
    return k.grad, tol


def ce_grad(v, labels, mean_over=None, loss_scale=1.0):
    """dL/dv of loss_scale * F.cross_entropy(v, labels) on float64 logits (mean over `mean_over` rows, default all), as fp32."""
    v = v.detach().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(v, labels.long(), reduction="sum") / (mean_over or v.shape[0]) * loss_scale
    loss.backward()
    return v.grad.float(), float(loss)
