#!/usr/bin/env python3
"""The tower backward timed with HIP events against torch's own ops on the same GPU, warmed and alternated in one process:

    python tools/tower_backward_bench.py [--out profiles/tower_backward.txt] [--rounds 7] [--quick]

Part 1, the attention backward alone (ops.attention_backward: S and P recomputed, nothing saved) at the ViT-B/16 shape (B = 256, H = 12, L = 197) and the
text shape (B = 1024, H = 8, L = 77, causal), against the backward of torch's scaled_dot_product_attention on the same fp16 operands (its forward, which
saves what its backward needs, is run once outside the timed window; the timed call is torch.autograd.grad with retain_graph).  floor = 10 B H L^2 64 FLOP
(the five products of an attention backward; half of it under the causal mask) / 2.5 PFLOP/s; this kernel runs nine products (csrc/pclip_attention_bwd.hip).
Part 2, a forward + backward step of the ViT-B/16 vision tower at 256 images with the last 1, 4 and 12 residual blocks (+ ln_post / proj) unfrozen:
model.encode_image under grad mode, a sum-of-squares-free linear loss (features * fixed weights).sum(), .backward() — against a plain-torch restatement of
the same towers' trainable tail on the same GPU (fp16 nn.functional linears, LayerNorm in fp32, scaled_dot_product_attention, QuickGELU; its frozen prefix
runs on this library under no_grad for both sides, so the difference is the tail alone).
A variant's time is the median over the rounds of (events around n back-to-back calls) / n; the rounds visit the variants in turn."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import _lib, ops  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, _run_blocks, build_model, random_state_dict  # noqa: E402

PEAK_FLOPS = 2.5e15
ATT_SHAPES = [("ViT-B/16 vision", 256, 12, 197, False), ("text tower", 1024, 8, 77, True)]


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


def attention_part(lines, rounds, quick):
    for name, B, H, L, causal in ATT_SHAPES:
        if quick:
            B = max(1, B // 16)
        W = H * 64
        g = torch.Generator(device="cuda").manual_seed(B + L)
        qkv = torch.randn(B * L, 3 * W, device="cuda", generator=g).half()
        dout = torch.randn(B * L, W, device="cuda", generator=g).half()
        q, k, v = (qkv.view(B, L, 3, H, 64)[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(3))
        do = dout.view(B, L, H, 64).permute(0, 2, 1, 3).contiguous()
        o = F.scaled_dot_product_attention(q, k, v, is_causal=causal)

        def torch_bwd():
            return torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

        def ours():
            return ops.attention_backward(qkv, dout, B, L, H, causal=causal)

        def ours_fwd():
            return ops.attention(qkv, B, L, H, causal=causal)

        variants = [("attention_backward", ours), ("torch SDPA backward", torch_bwd), ("(attention forward)", ours_fwd)]
        times = alternate(variants, 5, rounds)
        dq, dk, dv = torch_bwd()
        got = ours().view(B, L, 3, H, 64)
        err = max(float((got[:, :, i].permute(0, 2, 1, 3).float() - t.float()).abs().max()) for i, t in enumerate((dq, dk, dv)))
        fl = 10.0 * B * H * L * L * 64 * (0.5 if causal else 1.0) / PEAK_FLOPS * 1e6
        lines.append(f"{name}: B={B} H={H} L={L} causal={causal}  (5 calls x {rounds} rounds; max |dqkv - torch's| = {err:.2e})")
        for vname, _ in variants:
            t = statistics.median(times[vname])
            lines.append(f"  {vname:<22s} {t:10.1f} us  (min {min(times[vname]):9.1f}, max {max(times[vname]):9.1f})"
                         + (f"   floor {fl:7.2f} us (MFMA)   share {fl / t:6.1%}" if "forward" not in vname else ""))
        t_o, t_t = statistics.median(times["attention_backward"]), statistics.median(times["torch SDPA backward"])
        lines.append(f"  attention_backward takes {t_o / t_t:.2f}x torch's time ({'a win' if t_o < t_t else 'A LOSS'})")
        lines.append("")
        print("\n".join(lines[-(len(variants) + 3):]), flush=True)
        del q, k, v, o, qkv, dout


def torch_tail(x, blocks, B, L, heads, ln_post, proj):
    """Plain torch: blocks + class token + ln_post + proj on the residual stream x [B*L, W] fp16 (the reference's op order)."""
    W = x.shape[1]
    ln = lambda t, m: F.layer_norm(t.float(), (W,), m.weight, m.bias, 1e-5).half()
    for blk in blocks:
        qkv = F.linear(ln(x, blk.ln_1), blk.attn.in_proj_weight, blk.attn.in_proj_bias).view(B, L, 3, heads, 64)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * L, W)
        x = x + F.linear(a, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
        u = F.linear(ln(x, blk.ln_2), blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
        x = x + F.linear(u * torch.sigmoid(1.702 * u), blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
    return ln(x.view(B, L, W)[:, 0], ln_post) @ proj


def step_part(lines, rounds, quick):
    kw = dict(BACKBONES["ViT-B/16"], transformer_layers=1, vocab_size=512)
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    vis = model.visual
    B = 16 if quick else 256
    L, heads = (224 // 16) ** 2 + 1, vis.heads
    imgs = torch.randn(B, 3, 224, 224, device="cuda").half()
    wts = torch.randn(B, kw["embed_dim"], device="cuda").half() * 0.01
    blocks = vis.transformer.resblocks
    lines.append(f"ViT-B/16 vision tower, forward + backward step at {B} images (1 step x {rounds} rounds after 2 warm-up steps per variant)")
    for nb in (1, 4, 12):
        for p in model.parameters():
            p.requires_grad_(False)
        params = model.unfreeze(visual_blocks=nb, text_blocks=0, heads=True)
        params = [p for p in params if p is not model.ln_final.weight and p is not model.ln_final.bias and p is not model.text_projection]
        first = len(blocks) - nb

        def zero():
            for p in params:
                p.grad = None

        def ours():
            zero()
            (model.encode_image(imgs) * wts).sum().backward()

        def ours_fwd_only():
            with torch.no_grad():
                model.encode_image(imgs)

        def prefix():
            with torch.no_grad():
                cols = ops.im2col_patches(imgs, 16)
                patch = ops.gemm(cols, vis._cache.get("conv1", vis.conv1.weight, lambda w: w.reshape(vis.width, -1).contiguous()))
                cls16 = vis._cache.get("cls", vis.class_embedding, lambda t: t.half())
                pos16 = vis._cache.get("pos", vis.positional_embedding, lambda t: t.half().contiguous())
                x = ops.vit_assemble_tokens(patch, cls16, pos16, B, L - 1, vis.width)
                x = ops.layernorm(x, vis.ln_pre.weight, vis.ln_pre.bias)
                if first > 0:
                    x, _ = _run_blocks(x, blocks[:first], B, L, heads, causal=False)
            return x

        def torch_step():
            zero()
            (torch_tail(prefix(), list(blocks)[first:], B, L, heads, vis.ln_post, vis.proj) * wts).sum().backward()

        variants = [("this library", ours), ("plain torch tail", torch_step), ("(frozen forward)", ours_fwd_only)]
        times = alternate(variants, 1, rounds)
        ours()
        g_o = [p.grad.float().clone() for p in params]
        torch_step()
        rel = max(float((a - p.grad.float()).norm() / p.grad.float().norm().clamp_min(1e-30)) for a, p in zip(g_o, params))
        lines.append(f"  last {nb:2d} block(s) + heads trainable   (largest ||g - torch's|| / ||torch's|| over the parameter tensors: {rel:.2e})")
        for vname, _ in variants:
            t = statistics.median(times[vname]) / 1e3
            lines.append(f"    {vname:<18s} {t:9.2f} ms  (min {min(times[vname]) / 1e3:8.2f}, max {max(times[vname]) / 1e3:8.2f})")
        t_o, t_t = statistics.median(times["this library"]), statistics.median(times["plain torch tail"])
        lines.append(f"    the step takes {t_o / t_t:.2f}x the plain-torch tail's time ({'a win' if t_o < t_t else 'A LOSS'})")
        print("\n".join(lines[-5:]), flush=True)
        zero()
        torch.cuda.empty_cache()
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the batch: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tower_backward_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/tower_backward_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    attention_part(lines, args.rounds, args.quick)
    step_part(lines, args.rounds, args.quick)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
