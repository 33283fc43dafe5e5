#!/usr/bin/env python3
"""The sigmoid-loss kernels (ops.cosine_sigmoid + ops.cosine_sigmoid_backward: the loss, both row gradients, dscale and dbias) timed with HIP events against
torch eager on the same GPU, warmed and alternated in one process:

    python tools/cosine_sigmoid_bench.py [--out profiles/cosine_sigmoid.txt] [--rounds 5]

The torch side is the chain a user would write: F.normalize of both fp16 sides (where the shape normalises), the matmul, `scale * . + bias`,
`-F.logsigmoid(z * x).sum() / M` against a +-1 matrix z built ONCE outside the timed region (in torch's favour), `.backward()` into both operands and the two
0-dim scalars.  Shapes, all at D = 512: 4096^2 and 32 768^2 with the positives on the diagonal; a 16-shot few-shot batch, 1600 x 1600 with 100 ids (16 positives
per row); the ImageNet one-vs-rest probe, 50 000 samples x 1000 classes, operands as they are.  A variant's time is the median over the rounds of (events around
n back-to-back steps) / n; the rounds visit the variants in turn.  Peak memory is torch's max_memory_allocated over what was allocated before the step (the
operands, z for torch, the ids for the kernels), one step from a released workspace."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from proto_clip_amd import ops  # noqa: E402

D = 512
# tag, M, T, ids (None: diagonal; an int k: i % k against j % k; "probe": labels against arange), normalise, (scale, bias)
SHAPES = [("4096^2 diagonal", 4096, 4096, None, True, (10.0, -10.0)), ("32768^2 diagonal", 32768, 32768, None, True, (10.0, -10.0)),
          ("few-shot 16 x 100 ids, 1600 x 1600", 1600, 1600, 100, True, (10.0, -10.0)),
          ("ImageNet one-vs-rest probe, 50000 x 1000", 50000, 1000, "probe", False, (100.0, -95.0))]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                     # us per step


def peak_over(fn):
    ops.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench_shape(tag, M, T, ids, norm, scale, bias, rounds, lines):
    g = torch.Generator().manual_seed(1)
    k = 16
    cen = F.normalize(torch.randn(k, D, generator=g), dim=1)
    a = (cen[torch.arange(M) % k] + 0.35 * torch.randn(M, D, generator=g) / D ** 0.5).half().cuda()
    b = (cen[torch.arange(T) % k] + 0.35 * torch.randn(T, D, generator=g) / D ** 0.5).half().cuda()
    if not norm:
        a, b = F.normalize(a.float(), dim=1).half(), F.normalize(b.float(), dim=1).half()
    if ids is None:
        ia = ib = None
        ra, rb = torch.arange(M, device="cuda"), torch.arange(T, device="cuda")
    elif ids == "probe":
        ia = torch.randint(0, T, (M,), generator=g).cuda()
        ib = torch.arange(T).cuda()
        ra, rb = ia, ib
    else:
        ia, ib = (torch.arange(M) % ids).cuda(), (torch.arange(T) % ids).cuda()
        ra, rb = ia, ib
    z = ((ra[:, None] == rb[None, :]).half() * 2 - 1)                                 # +-1 [M, T] fp16, built once
    at, bt = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    st, bi = torch.tensor(scale, device="cuda", requires_grad=True), torch.tensor(bias, device="cuda", requires_grad=True)

    def torch_step():
        at.grad = bt.grad = st.grad = bi.grad = None
        an, bn = (F.normalize(at, dim=1), F.normalize(bt, dim=1)) if norm else (at, bt)
        x = st * (an @ bn.t()) + bi
        loss = -F.logsigmoid(z * x).float().sum() / M
        loss.backward()
        return loss.detach(), at.grad, bt.grad, st.grad, bi.grad

    def fused_step():
        loss = ops.cosine_sigmoid(a, b, scale, bias, ia, ib, norm, norm)
        return (loss,) + ops.cosine_sigmoid_backward(a, b, scale, bias, ia, ib, norm, norm)

    variants = {"fused": fused_step, "torch eager": torch_step}
    n = 3 if M * T > 1e8 else 20
    for fn in variants.values():                                                      # warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, n))
    t = {name: statistics.median(v) for name, v in times.items()}
    spread = {name: (min(v), max(v)) for name, v in times.items()}
    mem = {name: peak_over(fn) for name, fn in variants.items()}
    lf, lt = float(fused_step()[0]), float(torch_step()[0])
    lines.append(f"{tag}: M={M} T={T} D={D} scale={scale} bias={bias} normalise={'both' if norm else 'no'}   loss fused {lf:.6f} | torch fp16 chain {lt:.6f}")
    for name in variants:
        lines.append(f"    {name:<12s} {t[name] / 1e3:10.3f} ms  (min {spread[name][0] / 1e3:.3f}, max {spread[name][1] / 1e3:.3f})   peak memory over the operands "
                     f"{mem[name] / 2 ** 20:10.1f} MiB")
    lines.append(f"    fused vs torch eager {t['torch eager'] / t['fused']:.2f}x in time, {mem['torch eager'] / max(mem['fused'], 1):.1f}x in memory"
                 + ("  LOSES" if t["fused"] > t["torch eager"] else ""))
    del z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/cosine_sigmoid_bench.py needs a GPU: nothing is timed without one")
    lines = [f"$ python tools/cosine_sigmoid_bench.py --out profiles/cosine_sigmoid.txt",
             f"tools/cosine_sigmoid_bench.py on {torch.cuda.get_device_name(0)}; forward + backward (dL/da, dL/db, dscale, dbias); medians over {a.rounds} rounds"]
    for tag, M, T, ids, norm, (scale, bias) in SHAPES:
        bench_shape(tag, M, T, ids, norm, scale, bias, a.rounds, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
