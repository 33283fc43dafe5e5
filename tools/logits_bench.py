#!/usr/bin/env python3
"""ops.cosine_logits timed with HIP events against torch's own ops on the same GPU, warmed and alternated in one process:

    python tools/logits_bench.py [--out profiles/cosine_logits.txt] [--rounds 7]

Shapes: the ImageNet zero-shot split (M = 50 000 cached features x T = 1000 prompts, D = 512 and 1024), OxfordPets (3669 x 37 x 512) and two serving
shapes (M = 1, T = 1000; M = 8, T = 3).  Each is timed as
  logits     the new call with the [M, T] matrix written,
  fused      the new call with argmax + top-5 only (no matrix in memory),
  torch mm   torch's `(s * f) @ w.t()`,
  torch all  the same followed by `.argmax(1)` and `.topk(5)`,
  ops.gemm   (T % 8 == 0 only) the project's GEMM on pre-scaled rows — what the zero-shot line could run on before this kernel.
A variant's time is the median over the rounds of (events around n back-to-back launches) / n; the rounds visit the variants in turn.
floor = max(2 M T D / 2.5 PFLOP/s, algorithmic bytes / 8 TB/s) (spec peaks of the MI355X: fp16 MFMA, HBM3E); bytes = the fp16 operands once + the outputs
(with logits: + 2 M T; fused: + 4 M + 30 M for argmax and top-5).  `share` = floor / time; the bound named is the larger of the two terms.

    python tools/logits_bench.py --ce [--out profiles/cosine_ce.txt]

times the training side instead: ops.cosine_cross_entropy (forward) and forward + ops.cosine_cross_entropy_backward (both row gradients and dscale) against
torch eager on the same GPU — normalise both sides, `s * a @ b.t()`, F.cross_entropy on the fp32 logits (CLIP's symmetric pair of them in symmetric mode),
`.backward()` — at 50 000 x 1000 x 512 and 3669 x 37 x 512 labelled, 4096^2 x 512 and 32 768^2 x 512 symmetric, with the peak memory each side allocates
on top of the operands.  floor = 2 M T D (forward) or 8 M T D (forward + backward: the logits twice more, two gradient products) / 2.5 PFLOP/s."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import _lib, ops  # noqa: E402

PEAK_FLOPS, PEAK_BW = 2.5e15, 8.0e12
SHAPES = [("ImageNet zero-shot, D=512", 50000, 1000, 512), ("ImageNet zero-shot, D=1024", 50000, 1000, 1024), ("OxfordPets", 3669, 37, 512),
          ("serving, one image", 1, 1000, 512), ("serving, 8 images x 3 prompts", 8, 3, 512)]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                     # us per launch


def floor_us(M, T, D, with_logits):
    flops = 2.0 * M * T * D
    nbytes = 2.0 * (M * D + T * D) + (2.0 * M * T if with_logits else 34.0 * M)
    tf, tb = flops / PEAK_FLOPS * 1e6, nbytes / PEAK_BW * 1e6
    return max(tf, tb), ("MFMA" if tf >= tb else "HBM"), nbytes


CE_SHAPES = [("ImageNet linear probe, labelled", 50000, 1000, 512, False), ("CLIP batch 4096, symmetric", 4096, 4096, 512, True),
             ("CLIP batch 32768, symmetric", 32768, 32768, 512, True), ("OxfordPets, labelled", 3669, 37, 512, False)]


def peak_over(fn):
    """Peak bytes fn allocates on top of what is live before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main_ce(args):
    import torch.nn.functional as F
    lines = ["$ python tools/logits_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    for name, M, T, D, symmetric in CE_SHAPES:
        s = 14.2857 if symmetric else 100.0                      # CLIP's initial temperature / the zero-shot line's scale
        g = torch.Generator(device="cuda").manual_seed(M + T)
        a = torch.randn(M, D, device="cuda", generator=g).half()
        b = (a[:T] + 0.5 * torch.randn(T, D, device="cuda", generator=g).half()) if symmetric else torch.randn(T, D, device="cuda", generator=g).half()
        y = None if symmetric else torch.randint(0, T, (M,), device="cuda", generator=g)
        at, bt = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        diag = torch.arange(M, device="cuda") if symmetric else None

        def torch_fwd():
            an, bn = at / at.norm(dim=-1, keepdim=True), bt / bt.norm(dim=-1, keepdim=True)
            L = (s * an @ bn.t()).float()
            return 0.5 * (F.cross_entropy(L, diag) + F.cross_entropy(L.t(), diag)) if symmetric else F.cross_entropy(L, y)

        def torch_both():
            at.grad = bt.grad = None
            torch_fwd().backward()

        def torch_fwd_only():
            with torch.no_grad():
                return torch_fwd()

        def ours_fwd():
            return ops.cosine_cross_entropy(a, b, s, y, symmetric, True, True)

        def ours_both():
            loss, lse_row, lse_col = ours_fwd()
            return loss, ops.cosine_cross_entropy_backward(a, b, s, lse_row, lse_col, y, symmetric, True, True)

        variants = [("forward", ours_fwd, 2.0), ("fwd + bwd", ours_both, 8.0), ("torch fwd", torch_fwd_only, 2.0), ("torch f + b", torch_both, 8.0)]
        n = 3 if M * T >= 10 ** 8 else (10 if M * T >= 10 ** 7 else 100)
        for _, fn, _ in variants:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {v[0]: [] for v in variants}
        for _ in range(args.rounds):
            for vname, fn, _ in variants:
                times[vname].append(timed(fn, n))
        loss, grads = ours_both()
        # agreement with torch autograd on fp32 copies of the operands (the timed fp16 chain underflows: its logit gradients are 1 / (2 M) softmax in fp16)
        a32, b32 = a.float().requires_grad_(True), b.float().requires_grad_(True)
        L = s * (a32 / a32.norm(dim=-1, keepdim=True)) @ (b32 / b32.norm(dim=-1, keepdim=True)).t()
        l32 = 0.5 * (F.cross_entropy(L, diag) + F.cross_entropy(L.t(), diag)) if symmetric else F.cross_entropy(L, y)
        l32.backward()
        dl = abs(float(loss) - float(l32))
        da = (grads[0] - a32.grad).abs().max().item() / a32.grad.abs().max().item()
        del L, l32, a32, b32
        ops.release_workspaces()
        mem_ours, mem_torch = peak_over(ours_both), peak_over(torch_both)
        lines.append(f"{name}: M={M} T={T} D={D}  ({n} launches x {args.rounds} rounds; |loss - torch fp32's| = {dl:.2e}, max |dL/da - torch fp32's| = {da:.1e} of its largest)")
        for vname, _, mult in variants:
            t = statistics.median(times[vname])
            fl = mult * M * T * D / PEAK_FLOPS * 1e6
            lines.append(f"  {vname:<12s} {t:10.1f} us  (min {min(times[vname]):9.1f}, max {max(times[vname]):9.1f})   floor {fl:8.2f} us (MFMA)   share {fl / t:6.1%}")
        t_o, t_t = statistics.median(times["fwd + bwd"]), statistics.median(times["torch f + b"])
        lines.append(f"  fwd + bwd is {t_t / t_o:.2f}x torch's ({'a win' if t_o < t_t else 'A LOSS'}); peak memory over the operands: {mem_ours / 2 ** 20:.1f} MiB here, "
                     f"{mem_torch / 2 ** 20:.1f} MiB torch (the fp16 logits alone are {M * T * 2 / 2 ** 20:.1f} MiB)")
        lines.append("")
        print("\n".join(lines[-(len(variants) + 3):]), flush=True)
        del at, bt, a, b
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ce", action="store_true", help="time the cross-entropy forward / backward against torch eager instead")
    args = ap.parse_args()
    _lib.load()
    if args.ce:
        return main_ce(args)
    lines = ["$ python tools/logits_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    s = 100.0
    for name, M, T, D in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + T)
        f = ops.l2norm_rows(torch.randn(M, D, device="cuda", generator=g).half())
        w = ops.l2norm_rows(torch.randn(T, D, device="cuda", generator=g).half())
        fs = (s * f).half()

        def torch_all():
            L = (s * f) @ w.t()
            return L.argmax(1), L.topk(min(5, T))

        variants = [("logits", lambda: ops.cosine_logits(f, w, s), True),
                    ("fused", lambda: ops.cosine_logits(f, w, s, want_logits=False, want_argmax=True, topk=min(5, T)), False),
                    ("torch mm", lambda: (s * f) @ w.t(), True),
                    ("torch all", torch_all, True)]
        if T % 8 == 0:
            variants.append(("ops.gemm", lambda: ops.gemm(fs, w), True))
        n = 10 if M * T >= 10 ** 7 else 100
        for _, fn, _ in variants:                              # warm every variant at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {v[0]: [] for v in variants}
        for _ in range(args.rounds):
            for vname, fn, _ in variants:
                times[vname].append(timed(fn, n))
        same = torch.equal(ops.cosine_logits(f, w, s)[0], ((s * f) @ w.t()))
        lines.append(f"{name}: M={M} T={T} D={D}  ({n} launches x {args.rounds} rounds; logits bit-identical to torch's: {same})")
        for vname, _, with_logits in variants:
            t = statistics.median(times[vname])
            fl, bound, nbytes = floor_us(M, T, D, with_logits)
            lines.append(f"  {vname:<10s} {t:9.1f} us  (min {min(times[vname]):8.1f}, max {max(times[vname]):8.1f})   floor {fl:7.2f} us ({bound}, {nbytes / 1e6:7.2f} MB)"
                         f"   share {fl / t:6.1%}")
        lines.append("")
        print("\n".join(lines[-(len(variants) + 2):]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
