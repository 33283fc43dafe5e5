#!/usr/bin/env python3
"""Visual prompt tuning (proto_clip_amd.vpt, csrc/pclip_vpt.hip) measured with HIP events, warmed and alternated in one process:

    python tools/vpt_bench.py [--out profiles/vpt.txt] [--rounds 7] [--quick]
    python tools/vpt_bench.py --digests [--autograd FILE]

1. The three kernels alone at 256 x (197 + 8) x 768 and 1024 x (50 + 8) x 768 (ViT-B/16 and ViT-B/32 with 8 prompt rows), each against its HBM floor —
   the bytes it must move over the device's peak bandwidth (--hbm-gbs, default 8000: MI355X) — and against the torch expression of the same result on the
   same GPU (torch.cat / an indexed copy_ / a float sum over the batch).
2. One training step, forward plus backward to ctx.grad: the real ViT-B/16 vision tower (seeded random weights), 256 images, P = 8, depth 1 and 12.  Against
   (c) a plain-torch restatement with scaled_dot_product_attention (fp16 linears, LayerNorm in fp32, QuickGELU, the tower frozen), and against (d) the frozen
   `encode_image` of the same 256 images — a forward only, whose launches VPT runs at 205 / 197 of the rows.
3. Peak memory of a step above what is resident before it (weights, images).

--digests prints SHA-256 digests (first 24 hex digits) of the features and of every parameter gradient of a taped `encode_image` with
`unfreeze(visual_blocks=2)` on the SMALL test tower — the case tests/test_gpu_vpt.py replays.  With --autograd FILE the package's autograd module is loaded
from FILE instead: a copy of the parent commit's autograd.py records the parent's bits (the library's existing kernels are unchanged)."""
import argparse
import hashlib
import importlib.util
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import proto_clip_amd  # noqa: E402
from proto_clip_amd import _lib, ops  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                               # ms


def alternate(variants, rounds, warm=2):
    for _, fn in variants:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(timed(fn))
    return times


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------------------------

def kernel_part(lines, B, L0, P, W, rounds, hbm_gbs):
    L = L0 + P
    g = torch.Generator(device="cuda").manual_seed(B)
    t = torch.randn(B * L0, W, device="cuda", generator=g).half()
    x = torch.randn(B * L, W, device="cuda", generator=g).half()
    ctx = torch.randn(P, W, device="cuda", generator=g) * 0.02
    inner = 20                                                               # launches per timed interval: a flat pass takes tens of microseconds

    def rep(fn):
        def run():
            for _ in range(inner):
                fn()
        return run

    xv = x.view(B, L, W)
    variants = [
        ("append: this library", rep(lambda: ops.vpt_append(t, ctx, B, L0))),
        ("append: torch.cat", rep(lambda: torch.cat([t.view(B, L0, W), ctx.half().expand(B, P, W)], 1))),
        ("replace: this library", rep(lambda: ops.vpt_replace_(x, ctx, B, L0))),
        ("replace: torch copy_", rep(lambda: xv[:, L0:].copy_(ctx.half()))),
        ("grad: this library", rep(lambda: ops.vpt_grad(x, B, L0, P))),
        ("grad + clear: this library", rep(lambda: ops.vpt_grad(x, B, L0, P, clear=True))),
        ("grad: torch float sum", rep(lambda: xv[:, L0:].float().sum(0))),
        ("grad + clear: torch sum, zero_", rep(lambda: (xv[:, L0:].float().sum(0), xv[:, L0:].zero_()))),
    ]
    times = alternate(variants, rounds)
    floor_bytes = {"append": 2 * B * L * W * 2 - B * P * W * 2 + P * W * 4,      # read t and ctx, write t'
                   "replace": B * P * W * 2 + P * W * 4,                      # read ctx, write the prompt rows
                   "grad:": B * P * W * 2 + P * W * 4,                        # read the prompt rows, write dctx (the partials stay in cache-sized buffers)
                   "grad + clear": 2 * B * P * W * 2 + P * W * 4}
    lines.append(f"kernels at {B} x ({L0} + {P}) x {W}  ({inner} launches per interval x {rounds} rounds; HBM floor at {hbm_gbs:g} GB/s)")
    for name, _ in variants:
        us = statistics.median(times[name]) / inner * 1e3
        key = next(k for k in floor_bytes if name.startswith(k))
        floor = floor_bytes[key] / (hbm_gbs * 1e9) * 1e6
        lines.append(f"  {name:<34s} {us:9.2f} us  (min {min(times[name]) / inner * 1e3:8.2f})   floor {floor:7.2f} us  -> {us / floor:6.1f}x the floor")
    med = {name: statistics.median(times[name]) for name, _ in variants}
    for ours, other in (("append: this library", "append: torch.cat"), ("replace: this library", "replace: torch copy_"),
                        ("grad: this library", "grad: torch float sum"), ("grad + clear: this library", "grad + clear: torch sum, zero_")):
        r = med[ours] / med[other]
        lines.append(f"  {ours} / {other.split(': ')[1]} = {r:.2f} ({'a win' if r < 1 else 'A LOSS'})")
    lines.append("")
    print("\n".join(lines[-(len(variants) + 6):]), flush=True)


# ---- 2. and 3. one training step ---------------------------------------------------------------------------------------------------------------------------

def torch_features(model, ctx, images):
    """Plain torch: the prompted vision tower in the reference's op order, fp16 with LayerNorm in fp32 and SDPA."""
    vis = model.visual
    B, W, heads = images.shape[0], vis.width, vis.heads
    depth, P = ctx.shape[0], ctx.shape[1]
    c = lambda t: t.half()
    ln = lambda t, m: c(F.layer_norm(t.float(), (W,), m.weight.float(), m.bias.float(), 1e-5))
    x = F.conv2d(c(images), c(vis.conv1.weight), stride=vis.patch_size).reshape(B, W, -1).permute(0, 2, 1)
    x = torch.cat([c(vis.class_embedding).expand(B, 1, W), x], dim=1) + c(vis.positional_embedding)
    L0 = x.shape[1]
    x = ln(torch.cat([x, c(ctx[0]).expand(B, P, W)], dim=1), vis.ln_pre)
    L = L0 + P
    for i, blk in enumerate(vis.transformer.resblocks):
        if 1 <= i < depth:
            x = torch.cat([x[:, :L0], c(ctx[i]).expand(B, P, W)], dim=1)
        qkv = F.linear(ln(x, blk.ln_1), c(blk.attn.in_proj_weight), c(blk.attn.in_proj_bias)).view(B, L, 3, heads, 64)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, W)
        x = x + F.linear(a, c(blk.attn.out_proj.weight), c(blk.attn.out_proj.bias))
        u = F.linear(ln(x, blk.ln_2), c(blk.mlp.c_fc.weight), c(blk.mlp.c_fc.bias))
        x = x + F.linear(u * torch.sigmoid(1.702 * u), c(blk.mlp.c_proj.weight), c(blk.mlp.c_proj.bias))
    return ln(x[:, 0], vis.ln_post) @ c(vis.proj)


def step_part(lines, model, B, P, depth, N, rounds):
    from proto_clip_amd import vpt
    E, R = model.visual.output_dim, model.visual.input_resolution
    g = torch.Generator(device="cuda").manual_seed(depth)
    images = torch.randn(B, 3, R, R, device="cuda", generator=g).half()
    text = F.normalize(torch.randn(N, E, device="cuda", generator=g), dim=1).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    learner = vpt.VisualPromptLearner(model, n_ctx=P, depth=depth, seed=3)
    head = vpt.VPT(model, learner)
    ctx_t = learner.ctx.detach().clone().requires_grad_(True)
    scale = 1024.0

    def ours():
        learner.ctx.grad = None
        (head.loss(images, text, labels, layout="nd") * scale).backward()

    def plain():
        ctx_t.grad = None
        f = torch_features(model, ctx_t, images).float()
        logits = model.logit_scale.float().exp() * F.normalize(f, dim=1) @ F.normalize(text.float(), dim=1).t()
        (F.cross_entropy(logits, labels) * scale).backward()

    def frozen():
        with torch.no_grad():
            model.encode_image(images)

    def forward_only():
        with torch.no_grad():
            learner(images)

    variants = [("(a) this library, step", ours), ("(b) this library, no_grad forward", forward_only), ("(c) plain torch + SDPA, step", plain),
                ("(d) frozen encode_image (forward)", frozen)]
    times = alternate(variants, rounds)
    med = {name: statistics.median(times[name]) for name, _ in variants}
    L0 = learner.l0
    lines.append(f"one step: ViT-B/16 vision tower, {B} images, P = {P}, depth = {depth}, {N} classes, loss scale {scale:g}  (1 step x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<36s} {med[name]:9.2f} ms  (min {min(times[name]):8.2f}, max {max(times[name]):8.2f})")
    a, b, c, d = (med[name] for name, _ in variants)
    lines.append(f"  (a) / (c) = {a / c:.2f} ({'a win' if a < c else 'A LOSS'});  (b) / (d) = {b / d:.3f} against the row ratio {L0 + P} / {L0} = {(L0 + P) / L0:.3f};  (a) / (d) = {a / d:.2f}")
    # gradient agreement of the two fp16 streams (not a gate: the fixtures grade the library against float64)
    ours()
    plain()
    ga, gc = learner.ctx.grad / scale, ctx_t.grad / scale
    lines.append(f"  ||ctx.grad (a) - ctx.grad (c)|| / ||(c)|| per depth slice: " + " ".join(f"{float((ga[i] - gc[i]).norm() / gc[i].norm()):.2e}" for i in range(depth)))
    # peak memory of a step above what is resident (weights, images, text)
    for name, fn in (("(a) this library", ours), ("(c) plain torch + SDPA", plain)):
        learner.ctx.grad = None
        ctx_t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        lines.append(f"  peak memory of a step above the {base / 2 ** 20:.0f} MiB resident before it, {name}: {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB")
    lines.append("")
    print("\n".join(lines[-11:]), flush=True)
    learner.ctx.grad = None
    ctx_t.grad = None
    torch.cuda.empty_cache()


# ---- the bits of the taped tail ----------------------------------------------------------------------------------------------------------------------------

def digests(autograd_file):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import vpt_ref
    from spec import SMALL, trained_like_
    if autograd_file:
        spec = importlib.util.spec_from_file_location("proto_clip_amd.autograd", autograd_file)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["proto_clip_amd.autograd"] = mod
        spec.loader.exec_module(mod)
        proto_clip_amd.autograd = mod
    from proto_clip_amd import autograd as pag
    sd = trained_like_(random_state_dict(seed=41, **SMALL), 41)
    model = build_model(sd).cuda()
    _, images, text, labels = vpt_ref.fixture_inputs(SMALL, 6, 1, 1, 5, 11)
    params = model.unfreeze(visual_blocks=2)
    feats = model.encode_image(images.cuda())
    loss = pag.cosine_cross_entropy(feats, text.cuda(), 20.0, labels=labels.cuda(), normalize_a=True, normalize_b=True)
    (loss * 1024.0).backward()
    dg = lambda t: hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]
    names = {id(p): n for n, p in model.named_parameters()}
    out = [f"digest encode_image.features {dg(feats)}"]
    out += [f"digest grad.{names[id(p)]} {dg(p.grad)}" for p in params if p.grad is not None]
    print(f"# taped encode_image, SMALL tower, unfreeze(visual_blocks=2), autograd from {autograd_file or 'this tree'}")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the floors are computed from")
    ap.add_argument("--quick", action="store_true", help="32 images and a 2-block tower: a rehearsal of the script, not a measurement")
    ap.add_argument("--digests", action="store_true")
    ap.add_argument("--autograd", default=None, help="with --digests: load proto_clip_amd.autograd from this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vpt_bench.py measures on the GPU; there is none here")
    _lib.load()
    if args.digests:
        return digests(args.autograd)
    lines = ["$ python tools/vpt_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    for B, L0 in ((256, 197), (1024, 50)) if not args.quick else ((32, 197),):
        kernel_part(lines, B, L0, 8, 768, args.rounds, args.hbm_gbs)
    kw = dict(BACKBONES["ViT-B/16"], transformer_layers=1)                   # the vision tower is ViT-B/16's; the text tower is not run
    if args.quick:
        kw["vision_layers"] = 2
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    layers = len(model.visual.transformer.resblocks)
    for depth in (1, layers):
        step_part(lines, model, 32 if args.quick else 256, 8, depth, 100, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
