#!/usr/bin/env python3
"""CoCoOp (proto_clip_amd.cocoop, csrc/pclip_cocoop.hip) measured with HIP events, warmed and alternated in one process:

    python tools/cocoop_bench.py [--out profiles/cocoop.txt] [--rounds 7] [--quick]

1. The four kernels alone at ViT-B/16's text widths (E = 512, Hd = 32, Wt = 512), against the torch expressions of the same results on the same GPU and
   against the HBM floor of the bytes that must move (--hbm-gbs, default 8000: MI355X): the meta-net forward plus backward (autograd.MetaNetFn against an
   F.linear chain under autograd; floor: W1 and W2 read by the forward, read or written once more by the backward), the conditional assembly (against
   torch.cat + a broadcast add), the conditional context gradient (against float sums over the class and row axes).
2. One full step, forward plus backward to the five tensors: the real ViT-B/16 text tower (seeded random weights), n_ctx = 4, 1000 class names x B = 1 and 4,
   37 class names x B = 1 and 16.  Against a plain-torch restatement of the same chain with scaled_dot_product_attention (fp16 linears, LayerNorm in fp32,
   QuickGELU, the tower frozen, the same truncated length, one dense [B, N] cross-entropy), with the peak memory of a step above what is resident before it.
3. The share of the loss in that step: the grouped call over the B images and its backward alone on the step's own text features (against the per-image
   loop it replaced: tools/cosine_ce_grouped_bench.py)."""
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
from maple_bench import prompts, verdict  # noqa: E402  (the synthetic class prompts)
from vpt_bench import alternate  # noqa: E402  (the timing loop)


def rep(fn, inner):
    def run():
        for _ in range(inner):
            fn()
    return run


def report(lines, title, variants, times, inner, floors, unit="us"):
    k = 1e3 if unit == "us" else 1.0
    lines.append(title)
    med = {name: statistics.median(times[name]) / inner * k for name, _ in variants}
    for name, _ in variants:
        floor = floors.get(name.split(":")[0])
        tail = "" if floor is None else f"   floor {floor:7.3f} us -> {med[name] / floor:6.1f}x"
        lines.append(f"  {name:<44s} {med[name]:9.2f} {unit}  (min {min(times[name]) / inner * k:8.2f}, max {max(times[name]) / inner * k:8.2f}){tail}")
    for i in range(0, len(variants), 2):
        ours, other = variants[i][0], variants[i + 1][0]
        r = med[ours] / med[other]
        lines.append(f"  {ours} / {other.split(': ')[-1]} = {r:.2f} ({verdict(r)})")
    lines.append("")
    print("\n".join(lines[-(2 + len(variants) + len(variants) // 2):]), flush=True)
    return med


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------------------------------------

def metanet_part(lines, B, E, Hd, Wt, rounds, hbm_gbs):
    g = torch.Generator(device="cuda").manual_seed(B)
    f = F.normalize(torch.randn(B, E, device="cuda", generator=g), dim=1).half()
    r1, r2 = E ** -0.5, Hd ** -0.5
    leaves = [((torch.rand(Hd, E, device="cuda", generator=g) * 2 - 1) * r1).requires_grad_(True),
              ((torch.rand(Hd, device="cuda", generator=g) * 2 - 1) * r1).requires_grad_(True),
              ((torch.rand(Wt, Hd, device="cuda", generator=g) * 2 - 1) * r2).requires_grad_(True),
              ((torch.rand(Wt, device="cuda", generator=g) * 2 - 1) * r2).requires_grad_(True)]
    dpi = torch.randn(B, Wt, device="cuda", generator=g)
    f32 = f.float()
    inner = 10

    def step(forward):
        def run():
            for t in leaves:
                t.grad = None
            forward(*leaves).backward(dpi)
        return run

    variants = [("metanet: this library, MetaNetFn", rep(step(lambda w1, b1, w2, b2: pag.MetaNetFn.apply(f, w1, b1, w2, b2)), inner)),
                ("metanet: torch, F.linear chain", rep(step(lambda w1, b1, w2, b2: F.linear(torch.relu(F.linear(f32, w1, b1)), w2, b2)), inner))]
    times = alternate(variants, rounds)
    floor = (2 * Hd * E + 3 * Wt * Hd) * 4 / (hbm_gbs * 1e9) * 1e6             # W1 read + dW1 written; W2 read twice + dW2 written
    report(lines, f"meta-net forward + backward (dw1, db1, dw2, db2), B = {B}, {E} -> {Hd} -> {Wt}  ({inner} steps per interval x {rounds} rounds; HBM floor "
           f"at {hbm_gbs:g} GB/s)", variants, times, inner, {"metanet": floor})


def rows_part(lines, B, N, L, n_ctx, W, rounds, hbm_gbs):
    g = torch.Generator(device="cuda").manual_seed(B + N)
    vocab = 49408
    emb16 = (torch.randn(vocab, W, device="cuda", generator=g) * 0.02).half()
    pos16 = (torch.randn(77, W, device="cuda", generator=g) * 0.01).half()
    ctx = torch.randn(n_ctx, W, device="cuda", generator=g) * 0.02
    pi = torch.randn(B, W, device="cuda", generator=g) * 0.02
    tokens = prompts(N, n_ctx, vocab, N).cuda()
    dx = torch.randn(B * N * L, W, device="cuda", generator=g).half()
    head = tokens[:, :L]
    inner = 10

    def torch_embed():
        e = emb16[head]                                                          # [N, L, W]
        rows = (ctx[None] + pi[:, None, :]).half()                               # [B, n_ctx, W]
        x = torch.cat([e[None, :, :1].expand(B, N, 1, W), rows[:, None].expand(B, N, n_ctx, W), e[None, :, 1 + n_ctx:].expand(B, N, L - 1 - n_ctx, W)], dim=2)
        return (x.float() + pos16[:L].float()).half()

    def torch_grad():
        rows = dx.view(B, N, L, W)[:, :, 1:1 + n_ctx].float()
        dshift = rows.sum(1)
        return dshift.sum(0), dshift.sum(1), dshift

    variants = [("embed: this library, prompt_embed_cond", rep(lambda: ops.prompt_embed_cond(ctx, pi, tokens, emb16, pos16, L), inner)),
                ("embed: torch, cat + broadcast add", rep(torch_embed, inner)),
                ("grad: this library, prompt_cond_grad", rep(lambda: ops.prompt_cond_grad(dx, B, N, L, n_ctx), inner)),
                ("grad: torch, float sums", rep(torch_grad, inner))]
    times = alternate(variants, rounds)
    floors = {"embed": 2 * B * N * L * W * 2 / (hbm_gbs * 1e9) * 1e6,           # every output element written, one fp16 source element read
              "grad": B * N * n_ctx * W * 2 / (hbm_gbs * 1e9) * 1e6}            # the context rows of dx read
    report(lines, f"assembly and context gradient at B = {B}, N = {N}, L = {L}, n_ctx = {n_ctx}, W = {W}  ({inner} launches per interval x {rounds} rounds; "
           f"HBM floor at {hbm_gbs:g} GB/s)", variants, times, inner, floors)


# ---- 2. one full step ------------------------------------------------------------------------------------------------------------------------------------------------

def torch_text(model, rows, tokens, L):
    """Plain torch: the text tower in the reference's op order at L tokens on prompts whose rows 1 .. n_ctx are `rows` [M, n_ctx, W] fp16; tokens [M, 77]."""
    W, heads = model.transformer.width, model.transformer_heads
    M, P = rows.shape[0], rows.shape[1]
    c = lambda t: t.half()
    ln = lambda t, m: c(F.layer_norm(t.float(), (W,), m.weight.float(), m.bias.float(), 1e-5))
    emb = c(model.token_embedding.weight)[tokens[:, :L]]
    x = torch.cat([emb[:, :1], rows, emb[:, 1 + P:]], dim=1) + c(model.positional_embedding)[:L]
    for blk in model.transformer.resblocks:
        qkv = F.linear(ln(x, blk.ln_1), c(blk.attn.in_proj_weight), c(blk.attn.in_proj_bias)).view(M, L, 3, heads, 64)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(M, L, W)
        x = x + F.linear(a, c(blk.attn.out_proj.weight), c(blk.attn.out_proj.bias))
        u = F.linear(ln(x, blk.ln_2), c(blk.mlp.c_fc.weight), c(blk.mlp.c_fc.bias))
        x = x + F.linear(u * torch.sigmoid(1.702 * u), c(blk.mlp.c_proj.weight), c(blk.mlp.c_proj.bias))
    eot = tokens[:, :L].argmax(dim=1)
    return ln(x[torch.arange(M, device=x.device), eot], model.ln_final) @ c(model.text_projection)


def step_part(lines, model, N, B, n_ctx, rounds):
    from proto_clip_amd import cocoop
    E = model.text_projection.shape[1]
    g = torch.Generator(device="cuda").manual_seed(N + B)
    feats = torch.randn(B, E, device="cuda", generator=g).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    tokens = prompts(N, n_ctx, model.vocab_size, N)
    learner = cocoop.ConditionalPromptLearner([f"class{i}" for i in range(N)], model, n_ctx=n_ctx, tokenized_prompts=tokens, seed=3)
    head = cocoop.CoCoOp(model, learner)
    mine = list(learner.parameters())
    theirs = [p.detach().clone().requires_grad_(True) for p in mine]
    tok, L, scale = tokens.cuda().repeat(B, 1), learner.run_length, 1024.0
    fn32 = F.normalize(feats.float(), dim=1)

    def ours():
        for p in mine:
            p.grad = None
        (head.loss(feats, labels) * scale).backward()

    def plain():
        for p in theirs:
            p.grad = None
        ctx, w1, b1, w2, b2 = theirs
        pi = F.linear(torch.relu(F.linear(fn32.half().float(), w1, b1)), w2, b2)
        rows = (ctx[None] + pi[:, None, :]).half().repeat_interleave(N, dim=0)
        ft = torch_text(model, rows, tok, L).float().view(B, N, E)
        logits = model.logit_scale.float().exp() * torch.einsum("be,bne->bn", fn32, F.normalize(ft, dim=2))
        (F.cross_entropy(logits, labels) * scale).backward()

    with torch.no_grad():
        text = learner(feats)
    scale_t = head.logit_scale()

    def losses_alone():
        t = text.detach().requires_grad_(True)
        (pag.cosine_cross_entropy_grouped(feats.unsqueeze(1), t, scale_t, labels.view(-1, 1), normalize_a=True, normalize_b=True).mean() * scale).backward()

    variants = [("step: this library", ours), ("step: plain torch + SDPA", plain)]
    times = alternate(variants, rounds)
    med = report(lines, f"one step: ViT-B/16 text tower, {N} class names at {L} tokens, {B} images ({B * N} prompts), n_ctx = {n_ctx}, loss scale {scale:g}  "
                 f"(1 step x {rounds} rounds after 2 warm-ups)", variants, times, 1, {}, unit="ms")
    lines.pop()
    lt = alternate([("loss", losses_alone)], rounds)["loss"]
    share = statistics.median(lt) / med["step: this library"]
    lines.append(f"  the loss over the {B} images (one grouped call) with its backward, alone: {statistics.median(lt):.3f} ms (min {min(lt):.3f}) = "
                 f"{100 * share:.1f} % of the step")
    ours()
    plain()
    lines.append("  ||grad (a) - (b)|| / ||(b)||: " + "  ".join(f"{name} {float((p.grad - q.grad).norm() / q.grad.norm()):.1e}"
                                                                for name, p, q in zip(cocoop.PARAMETERS, mine, theirs)))      # not a gate: the fixtures grade
    for name, fn in (("this library", ours), ("plain torch + SDPA", plain)):
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
    print("\n".join(lines[-5:]), flush=True)
    for p in mine + theirs:
        p.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the floors are computed from")
    ap.add_argument("--quick", action="store_true", help="a 2-block tower and small cases: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cocoop_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/cocoop_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    metanet_part([], 4, 512, 32, 512, args.rounds, args.hbm_gbs)                # a discarded pass: the first intervals of a process run at ramping clocks
    for B in (1, 4, 16):
        metanet_part(lines, B, 512, 32, 512, args.rounds, args.hbm_gbs)
    for B, N in ((4, 1000), (16, 37)) if not args.quick else ((2, 37),):
        rows_part(lines, B, N, 12, 4, 512, args.rounds, args.hbm_gbs)
    kw = dict(BACKBONES["ViT-B/16"])
    kw["vision_layers"] = 1                                                     # cached features: the image tower is not run
    if args.quick:
        kw["transformer_layers"] = 2
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    for N, B in ((1000, 1), (1000, 4), (37, 1), (37, 16)) if not args.quick else ((37, 2),):
        step_part(lines, model, N, B, 4, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
