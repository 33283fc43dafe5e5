#!/usr/bin/env python3
"""The grouped cosine cross-entropy (csrc/pclip_cosine_ce.hip, ops.cosine_cross_entropy_grouped) against the loop of single calls it replaces, measured with
HIP events, warmed and alternated in one process:

    python tools/cosine_ce_grouped_bench.py [--out profiles/cosine_ce_grouped.txt] [--rounds 7] [--quick]

1. The kernel level, forward plus both backward directions with dscale, G x M x T x D = 16 x 1 x 37 x 512 (CoCoOp at 37 names x 16 images), 4 x 1 x 1000 x 512,
   1 x 1 x 1000 x 512 (one group: the grouped entry against the plain one) and 16 x 16 x 100 x 512 (episodes): one grouped call per pass against G plain
   calls per pass on the same operands.
2. One CoCoOp step, forward plus backward to the five tensors, on the real ViT-B/16 text tower (seeded random weights), n_ctx = 4, the four cases of
   tools/cocoop_bench.py: `CoCoOp.loss` as it stands (one grouped call) against the same step with the per-image loop it replaced, restated here; then the
   loss and its backward alone, both ways, on the step's own text features, and their share of their step."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from proto_clip_amd import _lib, ops  # noqa: E402
from proto_clip_amd import autograd as pag  # noqa: E402
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402
from maple_bench import prompts, verdict  # noqa: E402  (the synthetic class prompts)
from vpt_bench import alternate  # noqa: E402  (the timing loop)


def report(lines, title, variants, times, inner, unit):
    k = 1e3 if unit == "us" else 1.0
    lines.append(title)
    med = {name: statistics.median(times[name]) / inner * k for name, _ in variants}
    for name, _ in variants:
        lines.append(f"  {name:<52s} {med[name]:9.2f} {unit}  (min {min(times[name]) / inner * k:8.2f}, max {max(times[name]) / inner * k:8.2f})")
    for i in range(0, len(variants), 2):
        ours, other = variants[i][0], variants[i + 1][0]
        r = med[ours] / med[other]
        lines.append(f"  {ours} / {other.split(': ')[-1]} = {r:.2f} ({verdict(r)})")
    lines.append("")
    print("\n".join(lines[-(2 + len(variants) + len(variants) // 2):]), flush=True)
    return med


def kernel_part(lines, G, M, T, D, rounds):
    g = torch.Generator(device="cuda").manual_seed(G + M + T)
    a = torch.randn(G, M, D, device="cuda", generator=g).half()
    b = torch.randn(G, T, D, device="cuda", generator=g).half()
    labels = torch.randint(0, T, (G, M), device="cuda", generator=g)
    inner, scale = 5, 100.0

    def grouped():
        for _ in range(inner):
            _, lse, _ = ops.cosine_cross_entropy_grouped(a, b, scale, labels, True, True)
            ops.cosine_cross_entropy_grouped_backward(a, b, scale, lse, labels, True, True)

    def loop():
        for _ in range(inner):
            for q in range(G):
                _, lse, _ = ops.cosine_cross_entropy(a[q], b[q], scale, labels[q], False, True, True)
                ops.cosine_cross_entropy_backward(a[q], b[q], scale, lse, None, labels[q], False, True, True)

    variants = [("kernels: one grouped call", grouped), (f"kernels: the loop of {G} single calls", loop)]
    times = alternate(variants, rounds)
    report(lines, f"forward + dL/da + dL/db + dscale, both sides normalised, G x M x T x D = {G} x {M} x {T} x {D}  ({inner} passes per interval x {rounds} "
           f"rounds)", variants, times, inner, "us")


def step_part(lines, model, N, B, n_ctx, rounds):
    from proto_clip_amd import cocoop
    E = model.text_projection.shape[1]
    g = torch.Generator(device="cuda").manual_seed(N + B)
    feats = torch.randn(B, E, device="cuda", generator=g).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    tokens = prompts(N, n_ctx, model.vocab_size, N)
    learner = cocoop.ConditionalPromptLearner([f"class{i}" for i in range(N)], model, n_ctx=n_ctx, tokenized_prompts=tokens, seed=3)
    head = cocoop.CoCoOp(model, learner)
    mine, scale = list(learner.parameters()), 1024.0

    def loop_loss(text, scale_t):
        terms = [pag.cosine_cross_entropy(feats[q:q + 1].contiguous(), text[q], scale_t, labels=labels[q:q + 1], normalize_a=True, normalize_b=True)
                 for q in range(B)]
        return torch.stack([t.reshape(()) for t in terms]).mean()

    def grouped_loss(text, scale_t):
        return pag.cosine_cross_entropy_grouped(feats.unsqueeze(1), text, scale_t, labels.view(-1, 1), normalize_a=True, normalize_b=True).mean()

    def step(loss_of):
        def run():
            for p in mine:
                p.grad = None
            (loss_of(learner(feats), head.logit_scale()) * scale).backward()
        return run

    def as_it_stands():
        for p in mine:
            p.grad = None
        (head.loss(feats, labels) * scale).backward()

    variants = [("step: CoCoOp.loss (one grouped call)", as_it_stands), ("step: the per-image loop it replaced", step(loop_loss))]
    times = alternate(variants, rounds)
    med = report(lines, f"one step: ViT-B/16 text tower, {N} class names at {learner.run_length} tokens, {B} images ({B * N} prompts), n_ctx = {n_ctx}, loss scale "
                 f"{scale:g}  (1 step x {rounds} rounds after 2 warm-ups)", variants, times, 1, "ms")
    lines.pop()
    with torch.no_grad():
        text = learner(feats)
    scale_t = head.logit_scale()

    def alone(loss_of):
        def run():
            (loss_of(text.detach().requires_grad_(True), scale_t) * scale).backward()
        return run

    pair = [("loss: one grouped call, with its backward", alone(grouped_loss)), (f"loss: the {B} per-image calls, with their backward", alone(loop_loss))]
    lt = alternate(pair, rounds)
    for (name, _), (sname, _) in zip(pair, variants):
        m = statistics.median(lt[name])
        lines.append(f"  {name:<52s} {m:9.3f} ms  (min {min(lt[name]):8.3f}, max {max(lt[name]):8.3f}) = {100 * m / med[sname]:.1f} % of its step")
    as_it_stands()
    got = [p.grad.clone() for p in mine]
    step(loop_loss)()
    lines.append("  the five gradients of the two steps bit for bit: " + ("equal" if all(torch.equal(x, p.grad) for x, p in zip(got, mine)) else "DIFFERENT"))
    lines.append("")
    print("\n".join(lines[-4:]), flush=True)
    for p in mine:
        p.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a 2-block tower and one small case: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cosine_ce_grouped_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/cosine_ce_grouped_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    kernel_part([], 4, 1, 37, 512, args.rounds)                                 # a discarded pass: the first intervals of a process run at ramping clocks
    for G, M, T, D in ((16, 1, 37, 512), (4, 1, 1000, 512), (1, 1, 1000, 512), (16, 16, 100, 512)):
        kernel_part(lines, G, M, T, D, args.rounds)
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
