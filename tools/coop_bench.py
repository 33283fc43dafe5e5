#!/usr/bin/env python3
"""One CoOp training step (proto_clip_amd.coop: context rows -> frozen text tower -> fused cosine cross-entropy -> ctx.grad) timed with HIP events against a
plain-torch restatement on the same GPU, warmed and alternated in one process:

    python tools/coop_bench.py [--out profiles/coop.txt] [--rounds 7] [--quick]

Shape: the real ViT-B/16 text tower (12 blocks x 512, 8 heads, CLIP's vocabulary; seeded random weights), n_ctx = 16 shared context rows, 32 cached image
features per step, and the prompts "X .. X <classname>." of ImageNet's 1000 class names (tests/golden/imagenet_classnames.txt) through the project's
tokenizer; OxfordPets' 37 breeds are the second shape.  Variants:
  (a) this library, the tower truncated to L_eff = (largest EOT position) + 1 tokens (`truncate=True`, the default);
  (b) this library at the full 77 tokens (`truncate=False`);
  (c) plain torch at 77 tokens: fp16 nn.functional linears, LayerNorm in fp32, scaled_dot_product_attention with the causal mask, QuickGELU, the EOT pick,
      ln_final, the projection, normalised features, logits, F.cross_entropy, autograd down to the context (the tower frozen: torch skips its weight gradients too);
  (d) the same restatement cut to L_eff tokens.
A step is zero_grad + loss + backward (no optimizer: 8192 floats).  A variant's time is the median over the rounds of one step between two events; the rounds
visit the variants in turn.  The file also records whether (a) and (b) give the same bits (features and ctx.grad), and how far the fp16 gradient streams — this library's and the
restatement's, without and with a loss scale of 4096 — are from an fp32 run of the restatement."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from proto_clip_amd import _lib, coop  # noqa: E402
from proto_clip_amd.clip import tokenize  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402

PETS = ["abyssinian", "american_bulldog", "american_pit_bull_terrier", "basset_hound", "beagle", "bengal", "birman", "bombay", "boxer", "british_shorthair",
        "chihuahua", "egyptian_mau", "english_cocker_spaniel", "english_setter", "german_shorthaired", "great_pyrenees", "havanese", "japanese_chin",
        "keeshond", "leonberger", "maine_coon", "miniature_pinscher", "newfoundland", "persian", "pomeranian", "pug", "ragdoll", "russian_blue",
        "saint_bernard", "samoyed", "scottish_terrier", "shiba_inu", "siamese", "sphynx", "staffordshire_bull_terrier", "wheaten_terrier", "yorkshire_terrier"]


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


def torch_text_features(model, ctx, tokens, L, dtype=torch.float16):
    """Plain torch: the prompts with `ctx` at positions 1 .. n_ctx through the text tower at L tokens (the reference's op order), features [N, E] in `dtype`
    (fp16: the reference's precision; fp32: the same weights cast up, the yard-stick of the gradient comparison)."""
    N, W, heads = tokens.shape[0], model.transformer.width, model.transformer_heads
    n_ctx = ctx.shape[0]
    c = lambda t: t.to(dtype)
    emb = c(model.token_embedding.weight)[tokens[:, :L]]
    x = torch.cat([emb[:, :1], c(ctx)[None].expand(N, -1, -1), emb[:, 1 + n_ctx:]], dim=1) + c(model.positional_embedding)[:L]
    x = x.reshape(N * L, W)
    ln = lambda t, m: c(F.layer_norm(t.float(), (W,), m.weight, m.bias, 1e-5))
    for blk in model.transformer.resblocks:
        qkv = F.linear(ln(x, blk.ln_1), c(blk.attn.in_proj_weight), c(blk.attn.in_proj_bias)).view(N, L, 3, heads, 64)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(N * L, W)
        x = x + F.linear(a, c(blk.attn.out_proj.weight), c(blk.attn.out_proj.bias))
        u = F.linear(ln(x, blk.ln_2), c(blk.mlp.c_fc.weight), c(blk.mlp.c_fc.bias))
        x = x + F.linear(u * torch.sigmoid(1.702 * u), c(blk.mlp.c_proj.weight), c(blk.mlp.c_proj.bias))
    eot = coop.eot_positions(tokens[:, :L])
    return ln(x.view(N, L, W)[torch.arange(N, device=x.device), eot], model.ln_final) @ c(model.text_projection)


def torch_loss(model, ctx, tokens, L, feats, labels, dtype=torch.float16):
    t = torch_text_features(model, ctx, tokens, L, dtype).float()
    f = feats.float()
    logits = model.logit_scale.float().exp() * F.normalize(f, dim=1) @ F.normalize(t, dim=1).t()
    return F.cross_entropy(logits, labels)


def shape_part(lines, model, title, classnames, rounds, n_ctx=16, Q=32):
    N, E = len(classnames), model.text_projection.shape[1]
    learners = {tr: coop.PromptLearner(classnames, model, n_ctx=n_ctx, truncate=tr, seed=3).cuda() for tr in (True, False)}
    heads = {tr: coop.CoOp(model, pl) for tr, pl in learners.items()}
    tokens, l_eff = learners[True].tokenized_prompts, learners[True].l_eff
    g = torch.Generator(device="cuda").manual_seed(N)
    feats = F.normalize(torch.randn(Q, E, device="cuda", generator=g), dim=1).half()
    labels = torch.randint(0, N, (Q,), device="cuda", generator=g)
    ctx_t = learners[True].ctx.detach().clone().requires_grad_(True)

    def ours(tr):
        def step():
            learners[tr].ctx.grad = None
            heads[tr].loss(feats, labels).backward()
        return step

    def plain(L):
        def step():
            ctx_t.grad = None
            torch_loss(model, ctx_t, tokens, L, feats, labels).backward()
        return step

    variants = [(f"(a) this library, {l_eff} tokens", ours(True)), ("(b) this library, 77 tokens", ours(False)),
                ("(c) plain torch, 77 tokens", plain(77)), (f"(d) plain torch, {l_eff} tokens", plain(l_eff))]
    times = alternate(variants, rounds)
    ours(True)()
    ours(False)()
    with torch.no_grad():
        fa, fb = learners[True](), learners[False]()
    ga, gb = learners[True].ctx.grad.clone(), learners[False].ctx.grad.clone()
    same_f, same_g = torch.equal(fa, fb), torch.equal(ga, gb)
    # how far the fp16 gradient streams are from an fp32 run of the restatement (the same weights cast up), without and with a loss scale of 4096
    ctx_t.grad = None
    torch_loss(model, ctx_t, tokens, l_eff, feats, labels, torch.float32).backward()
    g32 = ctx_t.grad.clone()
    dist = lambda g: float((g.float() - g32).norm() / g32.norm())
    rels = {}
    for scale in (1.0, 4096.0):
        learners[True].ctx.grad = None
        (heads[True].loss(feats, labels) * scale).backward()
        rels["this library", scale] = dist(learners[True].ctx.grad / scale)
        ctx_t.grad = None
        (torch_loss(model, ctx_t, tokens, l_eff, feats, labels) * scale).backward()
        rels["plain torch fp16", scale] = dist(ctx_t.grad / scale)
    lines.append(f"{title}: N = {N} prompts, n_ctx = {n_ctx}, L_eff = {l_eff}, {Q} cached features  (1 step x {rounds} rounds after 2 warm-up steps per variant)")
    med = {}
    for name, _ in variants:
        med[name] = statistics.median(times[name])
        lines.append(f"  {name:<32s} {med[name]:9.2f} ms  (min {min(times[name]):8.2f}, max {max(times[name]):8.2f})")
    a, b, c, d = (med[name] for name, _ in variants)
    lines.append(f"  truncation: (a) takes {a / b:.2f}x (b)'s time;  against torch at the same length: (a) / (d) = {a / d:.2f} ({'a win' if a < d else 'A LOSS'}), "
                 f"(b) / (c) = {b / c:.2f} ({'a win' if b < c else 'A LOSS'});  (a) / (c) = {a / c:.2f}")
    lines.append(f"  (a) and (b) bit-equal: features {same_f}, ctx.grad {same_g}")
    lines.append(f"  ||ctx.grad - g32|| / ||g32|| at {l_eff} tokens (g32: the restatement in fp32, |g32| = {float(g32.norm()):.2e}): "
                 + ";  ".join(f"{who} x{scale:g}: {r:.2e}" for (who, scale), r in rels.items()))
    lines.append("")
    print("\n".join(lines[-9:]), flush=True)
    for pl in learners.values():
        pl.ctx.grad = None
    ctx_t.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--classnames", default=os.path.join(REPO, "tests", "golden", "imagenet_classnames.txt"), help="one class name per line")
    ap.add_argument("--quick", action="store_true", help="the first 64 class names only: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/coop_bench.py measures on the GPU; there is none here")
    _lib.load()
    with open(args.classnames) as fh:
        imagenet = [ln.strip() for ln in fh if ln.strip()]
    if args.quick:
        imagenet = imagenet[:64]
    kw = dict(BACKBONES["ViT-B/16"], vision_layers=1)                       # the text tower is ViT-B/16's; the vision tower is not run
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    assert tokenize("X").shape == (1, 77)
    lines = ["$ python tools/coop_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    shape_part(lines, model, "ImageNet class names", imagenet, args.rounds)
    shape_part(lines, model, "OxfordPets class names", PETS, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
