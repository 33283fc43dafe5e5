"""The arithmetic of the contrastive forward (reference clip/model.py:356-370) restated in torch on the CPU, and the derived tolerance
the cosine-logit kernel is graded with (tests/test_contrastive_cpu.py, tests/test_gpu_contrastive.py)."""
import torch


def r16(x):
    return x.half().float()


def l2norm_rows_ref(x16):
    """r16(x / r16(||x||)), ||x|| = sqrt of the fp32 sum of squares (pclip_l2norm_rows_f16)."""
    x = x16.float()
    n16 = r16(x.pow(2).sum(-1, keepdim=True).sqrt())
    return (x / n16).half()


def scaled_rows(x16, scale):
    """r16(scale * x): the fp32 product rounded to fp16."""
    return (torch.tensor(scale, dtype=torch.float32) * x16.float()).half()


def exact_logits(xs16, yn16):
    """float64 dot products of the fp16 operands [M, D] x [T, D] -> [M, T]."""
    return xs16.double() @ yn16.double().t()


def ulp16(v):
    """Spacing of fp16 at magnitude v (float64 tensor): 2^(floor(log2 v) - 10), 2^-24 in the subnormal range."""
    e = torch.floor(torch.log2(v.clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def logit_tolerance(xs16, yn16, exact):
    """|got - exact| <= delta + ulp16(|exact| + delta) / 2 with delta = D 2^-24 ||xs|| ||yn||: the worst error of an fp32 summation of D exact products in
    any order (each of the D - 1 additions rounds a partial sum bounded by ||xs|| ||yn|| by at most 2^-24 of it), plus the one rounding to fp16."""
    D = xs16.shape[1]
    delta = D * 2.0 ** -24 * xs16.double().norm(dim=1)[:, None] * yn16.double().norm(dim=1)[None, :]
    return delta + 0.5 * ulp16(exact.abs() + delta)


def grade(got16, xs16, yn16):
    """(worst |got - exact| / tolerance, share of elements that differ from r16(exact) at all)."""
    exact = exact_logits(xs16, yn16)
    tol = logit_tolerance(xs16, yn16, exact)
    got = got16.double().cpu()
    worst = ((got - exact).abs() / tol).max().item()
    differ = (got16.cpu() != exact.half()).double().mean().item()
    return worst, differ
