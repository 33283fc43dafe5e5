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
(with logits: + 2 M T; fused: + 4 M + 30 M for argmax and top-5).  `share` = floor / time; the bound named is the larger of the two terms."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    _lib.load()
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
