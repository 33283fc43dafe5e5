#!/usr/bin/env python3
"""The Tip-Adapter kernels (ops.tip_logits / tip_grid / tip_keys_backward) timed with HIP events against torch's own ops on the same GPU, warmed and alternated
in one process:

    python tools/tip_adapter_bench.py [--out profiles/tip_adapter.txt] [--rounds 5]

Shapes: the ImageNet test split (Q = 50 000, N = 1000, K = 16, D = 512 and 1024), OxfordPets (3669 x 37 x 16) and EuroSAT (8100 x 10 x 16).  Each is timed as
  argmax        the fused call, one (alpha, beta), argmax only (no matrix in memory),
  logits        the fused call with the fp16 [Q, N] matrix written,
  torch dense   upstream's chain: `f @ keys.t()`, the exp, `@ cache_values.half()`, `100 * f @ w.t() + alpha * .`, `.argmax(1)`,
  torch segment the stronger torch form: the same affinity and exp, then a reshape-sum over each class's K contiguous rows in place of the one-hot product,
  grid          the full 200 x 20 search on one launch; the torch side is timed on 2 betas x 20 alphas of the segment form and EXTRAPOLATED x 100 (said so in the row),
and one Tip-Adapter-F step at B = 256 on the ImageNet cache, forward + backward of the cache keys, against torch autograd of the dense chain.
A variant's time is the median over the rounds of (events around n back-to-back launches) / n; the rounds visit the variants in turn.
It also records how far upstream's fp16 chain and this kernel sit from float64 on the test cases of tests/tip_adapter_ref.py.

    python tools/tip_adapter_bench.py --grid-only --lib proto-clip_amd/libpclip_nbg2.so --note "beta chunk 2"

times the grid rows alone on another build of the library (`hipcc -DPCLIP_TIP_NBG=2` for csrc/pclip_tip.hip, linked with the other objects): the grid kernel's
beta chunk against an alternative."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from proto_clip_amd import _lib, ops, tip_adapter  # noqa: E402

SHAPES = [("ImageNet test split, D=512", 50000, 1000, 16, 512), ("ImageNet test split, D=1024", 50000, 1000, 16, 1024), ("OxfordPets", 3669, 37, 16, 512),
          ("EuroSAT", 8100, 10, 16, 512)]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                     # us per launch


def unit_rows(n, d, g):
    x = torch.randn(n, d, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).half().cuda()


def median_rounds(variants, rounds, n):
    out = {k: [] for k in variants}
    for k, fn in variants.items():                           # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(timed(fn, n[k] if isinstance(n, dict) else n))
    return {k: statistics.median(v) for k, v in out.items()}


def bench_shape(tag, Q, N, K, D, rounds, lines, grid_too, grid_only=False):
    g = torch.Generator().manual_seed(1)
    f, keys, w = unit_rows(Q, D, g), unit_rows(N * K, D, g), unit_rows(N, D, g)
    seg = ops.tip_segments(torch.arange(N).repeat_interleave(K).cuda(), N)
    values = torch.nn.functional.one_hot(torch.arange(N).repeat_interleave(K), N).half().cuda()
    labels = torch.randint(0, N, (Q,), generator=g).cuda()
    alpha, beta = 1.0, 5.5
    keys_t, w_t = keys.t().contiguous(), w.t().contiguous()

    def torch_dense():
        aff = f @ keys_t
        return (100. * f @ w_t + ((-1) * (beta - beta * aff)).exp() @ values * alpha).argmax(1)

    def torch_segment(b=beta, alphas=(alpha,)):
        e = ((-1) * (b - b * (f @ keys_t))).exp().view(Q, N, K).sum(2)
        z = 100. * f @ w_t
        return [(z + e * a).argmax(1) for a in alphas]

    variants = {"argmax": lambda: ops.tip_logits(f, keys, seg, w, alpha, beta, want_logits=False, want_argmax=True, layout="nd"),
                "logits": lambda: ops.tip_logits(f, keys, seg, w, alpha, beta, layout="nd"),
                "torch dense": torch_dense, "torch segment": torch_segment}
    lines.append(f"{tag}: Q={Q} N={N} K={K} D={D}")
    if grid_only:
        variants = {}
    n = 3 if Q * N * K > 1e8 else 20
    t = median_rounds(variants, rounds, n)
    for k, v in t.items():
        lines.append(f"    {k:<14s} {v:12.1f} us")
    if not grid_only:
        for name in ("argmax", "logits"):
            label = "fused argmax" if name == "argmax" else "logits written"
            lines.append(f"    {label} vs torch dense {t['torch dense'] / t[name]:.2f}x, vs torch segment {t['torch segment'] / t[name]:.2f}x"
                         + ("  LOSES" if t[name] > min(t["torch dense"], t["torch segment"]) else ""))
    if grid_too:
        betas, alphas = tip_adapter.search_lists({"search_scale": [7, 3], "search_step": [200, 20]})
        gv = {"grid 200x20": lambda: ops.tip_grid(f, keys, seg, w, betas, alphas, labels, layout="nd"),
              "torch 2x20": lambda: [[(p == labels).sum() for p in torch_segment(b, alphas)] for b in betas[:2]]}
        tg = median_rounds(gv, max(2, rounds // 2), 1)
        ext = tg["torch 2x20"] * 100
        lines.append(f"    grid 200 x 20  {tg['grid 200x20'] / 1e3:12.1f} ms   torch segment form, 2 betas x 20 alphas timed: {tg['torch 2x20'] / 1e3:.1f} ms, EXTRAPOLATED x 100 = "
                     f"{ext / 1e3:.0f} ms  ({ext / tg['grid 200x20']:.2f}x)" + ("  LOSES" if tg["grid 200x20"] > ext else ""))


def bench_step(rounds, lines):
    B, N, K, D = 256, 1000, 16, 512
    g = torch.Generator().manual_seed(2)
    f, keys, w = unit_rows(B, D, g), unit_rows(N * K, D, g), unit_rows(N, D, g)
    seg = ops.tip_segments(torch.arange(N).repeat_interleave(K).cuda(), N)
    values = torch.nn.functional.one_hot(torch.arange(N).repeat_interleave(K), N).half().cuda()
    labels = torch.randint(0, N, (B,), generator=g).cuda()
    adapter = tip_adapter.TipAdapterF(keys, layout="nd")
    lin = torch.nn.Linear(D, N * K, bias=False).half().cuda()
    lin.weight = torch.nn.Parameter(keys.clone())
    w_t = w.t().contiguous()

    def ours():
        adapter.weight.grad = None
        torch.nn.functional.cross_entropy(adapter.logits(f, None, w, 1.0, 5.5, seg=seg, layout="nd"), labels).backward()

    def torch_step():
        lin.weight.grad = None
        aff = lin(f)
        tip = 100. * f @ w_t + ((-1) * (5.5 - 5.5 * aff)).exp() @ values * 1.0
        torch.nn.functional.cross_entropy(tip, labels).backward()

    t = median_rounds({"fused": ours, "torch autograd": torch_step}, rounds, 10)
    lines.append(f"Tip-Adapter-F step, forward + backward of the keys: B={B} N={N} K={K} D={D}")
    lines.append(f"    fused {t['fused']:.1f} us   torch autograd {t['torch autograd']:.1f} us   ({t['torch autograd'] / t['fused']:.2f}x)"
                 + ("  LOSES" if t["fused"] > t["torch autograd"] else ""))


def distances(lines):
    import tip_adapter_ref as ref
    lines.append("distance to float64, max |logit - float64| over the (alpha, beta) points of tests/tip_adapter_ref.py:   this kernel (fp16 logits) | upstream's fp16 chain")
    for name in ref.CASES:
        if name == "many":
            continue
        s = ref.case(name)
        ex = ref.Exact(s["features"], s["keys"], s["seg"], s["text"])
        f, keys, seg, w = s["features"].cuda(), s["keys"].cuda(), s["seg"].cuda(), s["text"].cuda()
        mine = up = 0.0
        for alpha, beta in ref.POINTS:
            v = ex.at(alpha, beta)["v"]
            got = ops.tip_logits(f, keys, seg, w, alpha, beta, layout="nd")[0].cpu().double()
            mine = max(mine, float((got - v).abs().max()))
            up = max(up, float((ref.upstream_fp16_chain(s["features"], s["keys"], s["seg"], s["text"], alpha, beta).double() - v).abs().max()))
        lines.append(f"    {name:<14s} {mine:10.4f} | {up:10.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-grid", action="store_true")
    ap.add_argument("--grid-only", action="store_true", help="the grid rows alone (with --lib: another build of the library)")
    ap.add_argument("--lib", default=None, help="path of the libpclip build to load instead of the package's own")
    ap.add_argument("--note", default="beta chunk 4 (PCLIP_TIP_NBG in csrc/pclip_tip.hip)")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    lines = [f"tools/tip_adapter_bench.py on {torch.cuda.get_device_name(0)}; medians over {a.rounds} rounds; library {os.path.basename(_lib.LIB_PATH)}: {a.note}"]
    for i, (tag, Q, N, K, D) in enumerate(SHAPES):
        if a.grid_only and i not in (0, 2, 3):
            continue
        bench_shape(tag, Q, N, K, D, a.rounds, lines, grid_too=(i in (0, 2, 3)) and not a.no_grid, grid_only=a.grid_only)
    if not a.grid_only:
        bench_step(a.rounds, lines)
        distances(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
