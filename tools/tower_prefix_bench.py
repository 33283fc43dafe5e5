#!/usr/bin/env python3
"""The backward of the stages in front of block 0 timed with HIP events against torch's own ops on the same GPU, warmed and alternated in one process:

    python tools/tower_prefix_bench.py [--out profiles/tower_prefix.txt] [--rounds 7] [--quick]

Part 1, the two kernels alone.
  text side, 1024 prompts x 77 tokens x 512, V = 49 408 (ViT-B/16's text tower; synthetic prompts: SOT, 2 - 21 body tokens, EOT, zero padding; and
      64 prompts, a small batch):
      ops.text_embed_backward (torch's stable sort of the ids + memset + the two passes of the segmented reduction + the positional sums), and the same
      without the sort (the ids sorted once outside the window), against torch: the backward of F.embedding into a dense fp32 [V, 512] weight (its fp32
      upstream gradient is cast outside the timed window) plus dx.view(B, L, W).sum(0, dtype=float32).
  vision side, 256 images x 197 tokens x 768 (ViT-B/16's vision tower; and 16 images): ops.vit_embed_backward against dt.view(B, L, W).sum(0, dtype=float32) plus the
      contiguous copy of dt.view(B, L, W)[:, 1:].
  floor = the bytes each call must move (read dx once, write the outputs once; the text side also the cleared dE) / 8 TB/s.
Part 2, a full forward + backward of both ViT-B/16 towers at 256 image / text pairs under CLIP's contrastive loss, every block and the heads trainable, with
and without unfreeze(stem=True).
A variant's time is the median over the rounds of (events around n back-to-back calls) / n; the rounds visit the variants in turn."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import _lib, ops  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402

PEAK_BYTES = 8.0e12


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                     # us per call


def alternate(variants, n, rounds, warm=2):
    for _, fn in variants:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(timed(fn, n))
    return times


def prompts(B, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, 23, (B,), generator=g)
    body = torch.randint(1, vocab - 2, (B, 77), generator=g)
    pos = torch.arange(77)[None]
    t = torch.where(pos < lens[:, None], body, torch.zeros_like(body))
    t[:, 0] = vocab - 2
    t[torch.arange(B), lens] = vocab - 1
    return t


def report(lines, variants, times, floor_us, ours, theirs):
    for vname, _ in variants:
        t = statistics.median(times[vname])
        lines.append(f"  {vname:<46s} {t:10.1f} us  (min {min(times[vname]):9.1f}, max {max(times[vname]):9.1f})   floor {floor_us:6.1f} us (HBM)  share {floor_us / t:6.1%}")
    t_o, t_t = statistics.median(times[ours]), statistics.median(times[theirs])
    lines.append(f"  {ours} takes {t_o / t_t:.2f}x torch's time ({'a win' if t_o < t_t else 'A LOSS'})")
    lines.append("")


def kernel_part(lines, rounds, quick):
    for B in ((64,) if quick else (1024, 64)):
        text_kernel(lines, rounds, B)
    for B in ((16,) if quick else (256, 16)):
        vision_kernel(lines, rounds, B)


def text_kernel(lines, rounds, B):
    L, W, V = 77, 512, 49408
    tokens = prompts(B, V, 5).cuda()
    g = torch.Generator(device="cuda").manual_seed(7)
    dx = (torch.randn(B * L, W, device="cuda", generator=g) * 1e-2).half()
    dx32 = dx.float().view(B, L, W)
    E = torch.zeros(V, W, device="cuda", requires_grad=True)
    x = F.embedding(tokens, E)
    ids, order = torch.sort(tokens.reshape(-1), stable=True)
    dE = torch.empty(V, W, device="cuda")
    dpos = torch.empty(L, W, device="cuda")
    part = torch.empty((B * L + ops.EMBED_BWD_CHUNK - 1) // ops.EMBED_BWD_CHUNK, 2, W, device="cuda")
    lib = _lib.load()

    def ours():
        return ops.text_embed_backward(dx, tokens, V)

    def ours_presorted():
        _lib.check(lib.pclip_text_embed_backward(_lib.ptr(dx), _lib.ptr(ids), _lib.ptr(order), B, L, W, V, _lib.ptr(dE), _lib.ptr(dpos), _lib.ptr(part),
                                                 _lib.stream()), "pclip_text_embed_backward")

    def torch_bwd():
        return torch.autograd.grad(x, E, dx32, retain_graph=True)[0], dx.view(B, L, W).sum(0, dtype=torch.float32)

    variants = [("text_embed_backward (sort + kernels)", ours), ("text_embed_backward, ids sorted beforehand", ours_presorted),
                ("torch: F.embedding backward + sum(0)", torch_bwd)]
    times = alternate(variants, 5, rounds)
    a, b = ours(), torch_bwd()
    err = (float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
    pad = int((tokens == 0).sum())
    lines.append(f"text embedding backward: B={B} L={L} W={W} V={V}, {pad} of {B * L} rows are padding, chunk {ops.EMBED_BWD_CHUNK}  "
                 f"(5 calls x {rounds} rounds; max |dE - torch's| = {err[0]:.2e}, max |dpos - torch's| = {err[1]:.2e})")
    floor = (B * L * W * 2 + 2 * V * W * 4 + L * W * 4) / PEAK_BYTES * 1e6
    report(lines, variants, times, floor, "text_embed_backward (sort + kernels)", "torch: F.embedding backward + sum(0)")
    print("\n".join(lines[-6:]), flush=True)


def vision_kernel(lines, rounds, B):
    L, W = 197, 768
    g = torch.Generator(device="cuda").manual_seed(8)
    dt = (torch.randn(B * L, W, device="cuda", generator=g) * 1e-2).half()

    def ours_v():
        return ops.vit_embed_backward(dt, B, L)

    def torch_v():
        v = dt.view(B, L, W)
        return v.sum(0, dtype=torch.float32), v[:, 1:].contiguous()

    variants = [("vit_embed_backward", ours_v), ("torch: sum(0) + slice copy", torch_v)]
    times = alternate(variants, 5, rounds)
    a, b = ours_v(), torch_v()
    lines.append(f"vision token-assembly backward: B={B} L={L} W={W}  (5 calls x {rounds} rounds; max |dpos - torch's| = {float((a[0] - b[0]).abs().max()):.2e}, "
                 f"dpatch bit-equal: {torch.equal(a[1], b[1].view(-1, W))})")
    floor = (B * L * W * 2 + B * (L - 1) * W * 2 + L * W * 4) / PEAK_BYTES * 1e6
    report(lines, variants, times, floor, "vit_embed_backward", "torch: sum(0) + slice copy")
    print("\n".join(lines[-5:]), flush=True)


def step_part(lines, rounds, quick):
    kw = dict(BACKBONES["ViT-B/16"])
    if quick:
        kw.update(vision_layers=2, transformer_layers=2)
    B = 8 if quick else 256
    imgs = torch.randn(B, 3, 224, 224, device="cuda").half()
    toks = prompts(B, kw["vocab_size"], 11).cuda()
    models = {}
    for name, stem in (("blocks + heads", False), ("blocks + heads + stem", True)):
        m = build_model(random_state_dict(seed=3, **kw)).cuda()
        models[name] = (m, m.unfreeze(visual_blocks=kw["vision_layers"], text_blocks=kw["transformer_layers"], stem=stem))

    def step(name):
        m, params = models[name]

        def run():
            for p in params:
                p.grad = None
            (m.contrastive_loss(m.encode_image(imgs), m.encode_text(toks)) * 1024.0).backward()
        return run

    variants = [(name, step(name)) for name in models]
    times = alternate(variants, 1, rounds)
    lines.append(f"ViT-B/16, both towers ({kw['vision_layers']} + {kw['transformer_layers']} blocks), forward + backward at {B} image / text pairs, contrastive loss x 1024  "
                 f"(1 step x {rounds} rounds after 2 warm-up steps per variant)")
    for name in models:
        n = sum(p.numel() for p in models[name][1])
        t = statistics.median(times[name]) / 1e3
        lines.append(f"  {name:<24s} {len(models[name][1]):4d} tensors {n / 1e6:7.1f} M parameters  {t:9.2f} ms  (min {min(times[name]) / 1e3:8.2f}, max {max(times[name]) / 1e3:8.2f})")
    t0, t1 = (statistics.median(times[n]) for n in models)
    lines.append(f"  the stem adds {(t1 - t0) / 1e3:.2f} ms: the step with it takes {t1 / t0:.3f}x the step without ({'no cost' if t1 <= t0 else 'A LOSS of that much for the first layers'})")
    m, params = models["blocks + heads + stem"]
    names = {id(p): n for n, p in m.named_parameters()}
    prefix = [p for p in params if names[id(p)] in ("visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight",
                                                     "visual.ln_pre.bias", "token_embedding.weight", "positional_embedding")]
    ok = all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in prefix)
    lines.append(f"  all {len(prefix)} prefix gradients finite and non-zero: {ok}")
    lines.append("")
    print("\n".join(lines[-6:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the small batches only and two blocks per tower: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tower_prefix_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/tower_prefix_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    kernel_part(lines, args.rounds, args.quick)
    step_part(lines, args.rounds, args.quick)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
