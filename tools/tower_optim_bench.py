#!/usr/bin/env python3
"""One optimizer step of optim.TowerAdamW timed with HIP events against the torch chain a user would otherwise write, on the same GPU, warmed and
alternated in one process:

    python tools/tower_optim_bench.py [--out profiles/tower_optim.txt] [--rounds 7] [--quick]

Parameter sets: everything `CLIP.unfreeze` can make trainable in both ViT-B/16 towers (12 + 12 residual blocks and the heads), the last block of each
tower with the heads, and the heads alone (six tensors: launch-bound).  Gradients are fixed random tensors in the parameters' dtypes, scaled by the loss scale (the backward is not part of the step).
The torch chain is the amp pattern with fp32 master copies: _foreach_copy_ of the fp16 gradients into fp32 master gradients,
_amp_foreach_non_finite_check_and_unscale_ (what GradScaler.unscale_ runs), clip_grad_norm_(foreach), torch.optim.AdamW(fused=True) on the masters,
_amp_update_scale_, _foreach_copy_ of the masters back into the fp16 parameters.  (Its step is not skipped on overflow: less work than GradScaler.step.)
bytes = what TowerAdamW's three launches must move: the gradient twice, master / m / v read and written, an fp16 parameter written; floor = bytes /
6.3 TB/s.  A variant's time is the median over the rounds of (events around n back-to-back steps) / n; the rounds visit the variants in turn.
Launch counts: 3 for TowerAdamW by construction; the torch chain's kernels are counted with torch.profiler in one extra step after the timing."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import _lib  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402
from proto_clip_amd.optim import TowerAdamW  # noqa: E402

PEAK_BW = 6.3e12
SCALE = 1024.0


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                     # us per step


def alternate(variants, n, rounds, warm=3):
    for _, fn in variants:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(timed(fn, n))
    return times


class TorchChain:
    """fp32 master copies + foreach unscale + clip_grad_norm_ + fused AdamW + copy back."""

    def __init__(self, params, lr, max_norm):
        self.model_params = [p.detach().clone() for p in params]
        self.model_grads = [p.grad.detach().clone() for p in params]
        self.masters = [torch.nn.Parameter(p.float()) for p in self.model_params]
        for m in self.masters:
            m.grad = torch.zeros_like(m)
        self.master_grads = [m.grad for m in self.masters]
        self.opt = torch.optim.AdamW(self.masters, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, fused=True)
        dev = params[0].device
        self.scale = torch.full((), SCALE, device=dev)
        self.tracker = torch.zeros((), dtype=torch.int32, device=dev)
        self.found_inf = torch.zeros((), device=dev)
        self.max_norm = max_norm

    @torch.no_grad()
    def step(self):
        torch._foreach_copy_(self.master_grads, self.model_grads)
        self.found_inf.zero_()
        torch._amp_foreach_non_finite_check_and_unscale_(self.master_grads, self.found_inf, self.scale.reciprocal())
        torch.nn.utils.clip_grad_norm_(self.masters, self.max_norm, foreach=True)
        self.opt.step()
        torch._amp_update_scale_(self.scale, self.tracker, self.found_inf, 2.0, 0.5, 2000)
        torch._foreach_copy_(self.model_params, self.masters)


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def step_bytes(params):
    total = 0
    for p in params:
        total += p.numel() * (2 * p.grad.element_size() + 24 + (2 if p.dtype == torch.float16 else 0))
    return total


def bench_set(lines, losses, name, model, vb, tb, rounds, n):
    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    params = model.unfreeze(visual_blocks=vb, text_blocks=tb)
    g = torch.Generator(device="cuda").manual_seed(vb + tb)
    for p in params:
        p.grad = (torch.randn(p.shape, device="cuda", generator=g) * 1e-3 * SCALE).to(p.dtype)
    numel, nbytes = sum(p.numel() for p in params), step_bytes(params)
    chain = TorchChain(params, 1e-5, 1.0)
    opt = TowerAdamW(params, lr=1e-5, max_grad_norm=1.0, loss_scale=SCALE)
    opt.step()                                                # uploads the tables; the capture below finds nothing to upload
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    variants = [("TowerAdamW.step", opt.step), ("TowerAdamW (hipGraph replay)", graph.replay), ("torch amp chain", chain.step)]
    times = alternate(variants, n, rounds)
    floor = nbytes / PEAK_BW * 1e6
    lines.append(f"{name}: {len(params)} tensors, {numel / 1e6:.2f} M elements, {opt.nchunks} chunks, {nbytes / 1e9:.3f} GB per step, floor {floor:.1f} us "
                 f"at 6.3 TB/s   ({n} steps x {rounds} rounds)")
    med = {}
    for vname, _ in variants:
        t = med[vname] = statistics.median(times[vname])
        lines.append(f"  {vname:<30s} {t:10.1f} us  (min {min(times[vname]):9.1f}, max {max(times[vname]):9.1f})   {nbytes / t / 1e3:8.1f} GB/s of TowerAdamW's "
                     f"bytes   floor share {floor / t:6.1%}")
    for vname in ("TowerAdamW.step", "TowerAdamW (hipGraph replay)"):
        r = med[vname] / med["torch amp chain"]
        lines.append(f"  {vname} takes {r:.2f}x the torch chain's time ({'a win' if r < 1 else 'A LOSS'})")
        if r >= 1:
            losses.append(f"{name}: {vname} LOSES to the torch chain ({med[vname]:.1f} against {med['torch amp chain']:.1f} us)")
    if med["TowerAdamW (hipGraph replay)"] > med["TowerAdamW.step"]:
        losses.append(f"{name}: the hipGraph replay LOSES to the eager step ({med['TowerAdamW (hipGraph replay)']:.1f} against {med['TowerAdamW.step']:.1f} us): three "
                      "launches leave a graph nothing to save")
    best = min(med["TowerAdamW.step"], med["TowerAdamW (hipGraph replay)"])
    losses.append(f"{name}: {best / floor:.2f}x the bandwidth floor ({best - floor:.1f} us over it)"
                  + (" — a working set near or below the 256 MiB Infinity Cache: the HBM floor need not bind" if nbytes < 256e6 * 1.5 else ""))
    print("\n".join(lines[-6:]), flush=True)
    return opt, chain, len(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="two blocks per tower: a rehearsal of the script, not a measurement")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the torch.profiler pass that counts the torch chain's kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tower_optim_bench.py measures on the GPU; there is none here")
    _lib.load()
    layers = 2 if args.quick else 12
    kw = dict(BACKBONES["ViT-B/16"], vocab_size=512, vision_layers=layers, transformer_layers=layers)       # (the token embedding stays frozen: its size is irrelevant)
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    lines = ["$ python tools/tower_optim_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    sets = [(f"both ViT-B/16 towers, {layers} + {layers} blocks + heads", layers, layers, 10), ("last block of each tower + heads", 1, 1, 50),
            ("the heads alone (ln_post, proj, ln_final, text_projection)", 0, 0, 100)]
    counted, losses = [], []
    for name, vb, tb, n in sets:
        opt, chain, at = bench_set(lines, losses, name, model, vb, tb, args.rounds, n)
        counted.append((at, chain))
        lines.append("")

    lines.append("Where it loses, and what is left on the table:")
    lines.extend("  " + t for t in losses)
    lines.append("  not measured: anything but ViT-B/16 shapes, fp32 gradients for fp16 parameters, unaligned tensors (the element-by-element path)")
    print("\n".join(lines[-(len(losses) + 2):]), flush=True)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    save()
    if not args.no_launch_count:
        for at, chain in reversed(counted):
            try:
                k = f"  launches per step: TowerAdamW 3 (by construction), torch amp chain {count_kernels(chain.step)} kernels (torch.profiler, one step)"
            except Exception as e:                                  # the count is an extra: the timings above stand without it
                k = f"  launches per step: TowerAdamW 3 (by construction), torch amp chain not measured ({type(e).__name__})"
            lines.insert(at, k)
            print(k, flush=True)
        save()


if __name__ == "__main__":
    main()
