#!/usr/bin/env python3
"""MaPLe (proto_clip_amd.maple, csrc/pclip_maple.hip) measured with HIP events, warmed and alternated in one process:

    python tools/maple_bench.py [--out profiles/maple.txt] [--rounds 7] [--quick]

1. The coupling function, forward plus backward to all three gradients, at ViT-B/16's widths (512 -> 768), P = 2 and 4, depth 9 and 12: autograd.CoupleFn
   against (b) a per-depth F.linear + autograd loop and (c) one torch.baddbmm form on the same GPU, and against the HBM floor of the bytes that must move
   (Wc read by the forward and by the backward, dWc written: three passes over depth x Wv x Wt x 4 bytes; --hbm-gbs, default 8000: MI355X).
2. The row kernels at 1000 x 30 x 512 (ImageNet's class names, rows 1 .. 2) against the torch indexing expressions of the same result.
3. One full step, forward plus backward to the three parameters: the real ViT-B/16 towers (seeded random weights), 1000 and 37 class names, batches of 4 and
   32 images, depth 9, n_ctx 2.  Against a plain-torch restatement of the same chain with scaled_dot_product_attention (fp16 linears, LayerNorm in fp32,
   QuickGELU, both towers frozen, the text tower at the same truncated length), with the peak memory of a step above what is resident before it."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from proto_clip_amd import _lib, ops  # noqa: E402
from proto_clip_amd import autograd as pag  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402
from vpt_bench import alternate, torch_features  # noqa: E402  (the timing loop and the plain-torch prompted vision tower)


def verdict(r):
    return "a win" if r < 1 else "LOSES"


# ---- 1. the coupling function ----------------------------------------------------------------------------------------------------------------------------------

def couple_part(lines, depth, P, Wt, Wv, rounds, hbm_gbs):
    g = torch.Generator(device="cuda").manual_seed(depth * 10 + P)
    bound = Wt ** -0.5
    leaves = [(torch.randn(depth, P, Wt, device="cuda", generator=g) * 0.02).requires_grad_(True),
              ((torch.rand(depth, Wv, Wt, device="cuda", generator=g) * 2 - 1) * bound).requires_grad_(True),
              ((torch.rand(depth, Wv, device="cuda", generator=g) * 2 - 1) * bound).requires_grad_(True)]
    dy = torch.randn(depth, P, Wv, device="cuda", generator=g)
    inner = 10

    def rep(forward):
        def run():
            for _ in range(inner):
                for t in leaves:
                    t.grad = None
                forward(*leaves).backward(dy)
        return run

    variants = [("(a) this library, CoupleFn", rep(pag.CoupleFn.apply)),
                ("(b) torch, per-depth F.linear loop", rep(lambda x, w, b: torch.stack([F.linear(x[d], w[d], b[d]) for d in range(depth)]))),
                ("(c) torch, one baddbmm", rep(lambda x, w, b: torch.baddbmm(b[:, None, :], x, w.transpose(1, 2))))]
    times = alternate(variants, rounds)
    floor = 3 * depth * Wv * Wt * 4 / (hbm_gbs * 1e9) * 1e6
    lines.append(f"coupling forward + backward (dx, dweight, dbias), depth {depth}, P = {P}, {Wt} -> {Wv}  ({inner} steps per interval x {rounds} rounds; "
                 f"HBM floor of three passes over Wc at {hbm_gbs:g} GB/s: {floor:.2f} us)")
    med = {name: statistics.median(times[name]) / inner * 1e3 for name, _ in variants}
    for name, _ in variants:
        lines.append(f"  {name:<38s} {med[name]:9.2f} us  (min {min(times[name]) / inner * 1e3:8.2f}, max {max(times[name]) / inner * 1e3:8.2f})"
                     f"  -> {med[name] / floor:6.1f}x the floor")
    a, b, c = (med[name] for name, _ in variants)
    lines.append(f"  (a) / (b) = {a / b:.2f} ({verdict(a / b)});  (a) / (c) = {a / c:.2f} ({verdict(a / c)})")
    lines.append("")
    if len(lines) > 6:
        print("\n".join(lines[-6:]), flush=True)


# ---- 2. the row kernels ------------------------------------------------------------------------------------------------------------------------------------------

def rows_part(lines, B, L, off, P, W, rounds, hbm_gbs):
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B * L, W, device="cuda", generator=g).half()
    ctx = torch.randn(P, W, device="cuda", generator=g) * 0.02
    inner = 20

    def rep(fn):
        def run():
            for _ in range(inner):
                fn()
        return run

    xv = x.view(B, L, W)
    variants = [("replace: this library", rep(lambda: ops.rows_replace_(x, ctx, B, L, off))),
                ("replace: torch copy_", rep(lambda: xv[:, off:off + P].copy_(ctx.half()))),
                ("grad: this library", rep(lambda: ops.rows_grad(x, B, L, off, P))),
                ("grad: torch float sum", rep(lambda: xv[:, off:off + P].float().sum(0))),
                ("grad + clear: this library", rep(lambda: ops.rows_grad(x, B, L, off, P, clear=True))),
                ("grad + clear: torch sum, zero_", rep(lambda: (xv[:, off:off + P].float().sum(0), xv[:, off:off + P].zero_())))]
    times = alternate(variants, rounds)
    floor_bytes = {"replace": B * P * W * 2 + P * W * 4, "grad:": B * P * W * 2 + P * W * 4, "grad + clear": 2 * B * P * W * 2 + P * W * 4}
    lines.append(f"row kernels at {B} x {L} x {W}, rows {off} .. {off + P - 1}  ({inner} launches per interval x {rounds} rounds; HBM floor at {hbm_gbs:g} GB/s)")
    med = {name: statistics.median(times[name]) / inner * 1e3 for name, _ in variants}
    for name, _ in variants:
        floor = floor_bytes[next(k for k in floor_bytes if name.startswith(k))] / (hbm_gbs * 1e9) * 1e6
        lines.append(f"  {name:<34s} {med[name]:9.2f} us  (min {min(times[name]) / inner * 1e3:8.2f})   floor {floor:7.3f} us")
    for i in range(0, len(variants), 2):
        ours, other = variants[i][0], variants[i + 1][0]
        r = med[ours] / med[other]
        lines.append(f"  {ours} / {other.split(': ')[1]} = {r:.2f} ({verdict(r)})")
    lines.append("")
    print("\n".join(lines[-(len(variants) + 5):]), flush=True)


# ---- 3. one full step --------------------------------------------------------------------------------------------------------------------------------------------

def prompts(N, n_ctx, vocab, seed):
    """[N, 77] int64: SOT, n_ctx placeholders, a class name of 1 .. 6 tokens, a full stop, EOT (the highest id)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(N, 77, dtype=torch.long)
    for i in range(N):
        n = int(torch.randint(1, 7, (1,), generator=g))
        t[i, 0] = vocab - 2
        t[i, 1:1 + n_ctx] = 343
        t[i, 1 + n_ctx:1 + n_ctx + n] = torch.randint(1000, vocab - 2, (n,), generator=g)
        t[i, 1 + n_ctx + n] = 269
        t[i, 2 + n_ctx + n] = vocab - 1
    return t


def torch_text(model, ctx, tokens, L):
    """Plain torch: the prompted text tower in the reference's op order at L tokens, fp16 with LayerNorm in fp32 and causal SDPA."""
    W, heads = model.transformer.width, model.transformer_heads
    N, depth, P = tokens.shape[0], ctx.shape[0], ctx.shape[1]
    c = lambda t: t.half()
    ln = lambda t, m: c(F.layer_norm(t.float(), (W,), m.weight.float(), m.bias.float(), 1e-5))
    rows = lambda i: c(ctx[i]).expand(N, P, W)
    emb = c(model.token_embedding.weight)[tokens[:, :L]]
    x = torch.cat([emb[:, :1], rows(0), emb[:, 1 + P:]], dim=1) + c(model.positional_embedding)[:L]
    for i, blk in enumerate(model.transformer.resblocks):
        if 1 <= i < depth:
            x = torch.cat([x[:, :1], rows(i), x[:, 1 + P:]], dim=1)
        qkv = F.linear(ln(x, blk.ln_1), c(blk.attn.in_proj_weight), c(blk.attn.in_proj_bias)).view(N, L, 3, heads, 64)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(N, L, W)
        x = x + F.linear(a, c(blk.attn.out_proj.weight), c(blk.attn.out_proj.bias))
        u = F.linear(ln(x, blk.ln_2), c(blk.mlp.c_fc.weight), c(blk.mlp.c_fc.bias))
        x = x + F.linear(u * torch.sigmoid(1.702 * u), c(blk.mlp.c_proj.weight), c(blk.mlp.c_proj.bias))
    eot = tokens[:, :L].argmax(dim=1)
    return ln(x[torch.arange(N, device=x.device), eot], model.ln_final) @ c(model.text_projection)


def step_part(lines, model, N, B, P, depth, rounds):
    from proto_clip_amd import maple
    R = model.visual.input_resolution
    g = torch.Generator(device="cuda").manual_seed(N + B)
    images = torch.randn(B, 3, R, R, device="cuda", generator=g).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    tokens = prompts(N, P, model.vocab_size, N)
    learner = maple.MultiModalPromptLearner([f"class{i}" for i in range(N)], model, n_ctx=P, depth=depth, tokenized_prompts=tokens, seed=3)
    head = maple.MaPLe(model, learner)
    mine = list(learner.parameters())
    theirs = [p.detach().clone().requires_grad_(True) for p in mine]
    tok, L, scale = tokens.cuda(), learner.run_length, 1024.0

    def ours():
        for p in mine:
            p.grad = None
        (head.loss(images, labels) * scale).backward()

    def plain():
        for p in theirs:
            p.grad = None
        ctx, weight, bias = theirs
        vctx = torch.baddbmm(bias[:, None, :], ctx, weight.transpose(1, 2))
        fi, ft = torch_features(model, vctx, images).float(), torch_text(model, ctx, tok, L).float()
        logits = model.logit_scale.float().exp() * F.normalize(fi, dim=1) @ F.normalize(ft, dim=1).t()
        (F.cross_entropy(logits, labels) * scale).backward()

    variants = [("(a) this library, step", ours), ("(b) plain torch + SDPA, step", plain)]
    times = alternate(variants, rounds)
    med = {name: statistics.median(times[name]) for name, _ in variants}
    lines.append(f"one step: ViT-B/16 towers, {N} class names at {L} tokens, {B} images, n_ctx = {P}, depth = {depth}, loss scale {scale:g}  "
                 f"(1 step x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<32s} {med[name]:9.2f} ms  (min {min(times[name]):8.2f}, max {max(times[name]):8.2f})")
    a, b = (med[name] for name, _ in variants)
    lines.append(f"  (a) / (b) = {a / b:.2f} ({verdict(a / b)})")
    ours()
    plain()
    for name, p, q in zip(("ctx", "couple_weight", "couple_bias"), mine, theirs):                       # not a gate: the fixtures grade against float64
        lines.append(f"  ||{name}.grad (a) - (b)|| / ||(b)|| per depth slice: "
                     + " ".join(f"{float((p.grad[i] - q.grad[i]).norm() / q.grad[i].norm()):.1e}" for i in range(depth)))
    for name, fn in (("(a) this library", ours), ("(b) plain torch + SDPA", plain)):
        for p in mine + theirs:
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        lines.append(f"  peak memory of a step above the {base / 2 ** 20:.0f} MiB resident before it, {name}: "
                     f"{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB")
    lines.append("")
    print("\n".join(lines[-10:]), flush=True)
    for p in mine + theirs:
        p.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the floors are computed from")
    ap.add_argument("--quick", action="store_true", help="2-block towers and small cases: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/maple_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/maple_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    couple_part([], 9, 2, 512, 768, args.rounds, args.hbm_gbs)                  # a discarded pass: the first intervals of a process run at ramping clocks
    for depth in (9, 12) if not args.quick else (2,):
        for P in (2, 4):
            couple_part(lines, depth, P, 512, 768, args.rounds, args.hbm_gbs)
    rows_part(lines, 1000 if not args.quick else 37, 30, 1, 2, 512, args.rounds, args.hbm_gbs)
    kw = dict(BACKBONES["ViT-B/16"])
    if args.quick:
        kw["vision_layers"] = kw["transformer_layers"] = 2
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    depth = min(9, len(model.visual.transformer.resblocks), len(model.transformer.resblocks))
    for N in (1000, 37) if not args.quick else (37,):
        for B in (4, 32) if not args.quick else (4,):
            step_part(lines, model, N, B, 2, depth, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
