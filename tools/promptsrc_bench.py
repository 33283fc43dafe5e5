#!/usr/bin/env python3
"""The feature regularisers (csrc/pclip_feature_reg.hip, ops.feature_reg / feature_reg_backward) and a PromptSRC step (proto_clip_amd/promptsrc.py),
measured with HIP events, warmed and alternated in one process:

    python tools/promptsrc_bench.py [--out profiles/promptsrc.txt] [--rounds 7] [--quick]

1. The kernel pair, forward + backward, the target normalised by the flag, both modes: against torch eager on the same GPU (F.normalize, F.l1_loss or
   cosine_similarity, .backward() to x) at 1000 x 512 and 4 x 512 — both sit at launch cost: three launches against torch's sixteen or so — and at
   50 000 x 1024, the one shape that can show bandwidth: as a fraction of its HBM floor (x and t read twice, dx written once).  Peak memory above the
   operands, both ways.
2. A PromptSRC step (one frozen and one prompted vision pass, one prompted text pass, four loss calls, one backward) on the real ViT-B/16 towers (seeded
   random weights), 4 + 4 rows at depth 9, 1000 and 37 class names, 4 and 32 images: against a plain-torch restatement with SDPA (tools/vpt_bench's and
   tools/maple_bench's towers, F.l1_loss, F.kl_div), against the MaPLe step of the same shape, and the share of the step spent in the four loss calls
   (forward and backward, measured on the step's own features)."""
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
from maple_bench import prompts, torch_text, verdict  # noqa: E402
from vpt_bench import alternate, torch_features  # noqa: E402  (the timing loop and the plain-torch prompted vision tower)


def peak_above(fn):
    """Peak device memory of one call above what is allocated before it, in MiB (the workspace cache of ops counts: it is part of the call's footprint)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_part(lines, M, D, mode, rounds, hbm_gbs):
    g = torch.Generator(device="cuda").manual_seed(M + D)
    x = torch.randn(M, D, device="cuda", generator=g).half()
    t = (0.5 * x.float() + 0.5 * torch.randn(M, D, device="cuda", generator=g)).half()
    small = M * D <= 1 << 20
    inner = 10 if small else 1
    state = {"inner": inner}

    def ours():
        for _ in range(state["inner"]):
            _, inv = ops.feature_reg(x, t, mode, True)
            ops.feature_reg_backward(x, t, inv, mode, True)

    leaf = x.clone().requires_grad_(True)

    def eager():
        for _ in range(state["inner"]):
            leaf.grad = None
            n, tn = F.normalize(leaf, dim=1), F.normalize(t, dim=1)
            (F.l1_loss(n, tn) if mode == "l1" else 1.0 - F.cosine_similarity(n, tn, dim=1).mean()).backward()

    variants = [("this library: feature_reg + feature_reg_backward", ours), ("torch eager: normalize, loss, backward (fp16 tensors)", eager)]
    times = alternate(variants, rounds)
    k, unit = (1e3, "us") if small else (1.0, "ms")
    med = {name: statistics.median(times[name]) / inner * k for name, _ in variants}
    lines.append(f"mode {mode}, forward + backward, M x D = {M} x {D}, target normalised by the flag  ({inner} passes per interval x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<56s} {med[name]:10.2f} {unit}  (min {min(times[name]) / inner * k:9.2f}, max {max(times[name]) / inner * k:9.2f})")
    r = med[variants[0][0]] / med[variants[1][0]]
    lines.append(f"  feature_reg / torch eager = {r:.2f} ({verdict(r)})" + ("  — launch cost on both sides: 3 launches here" if small else ""))
    if not small:
        floor_ms = (2 * 2 * M * D * 2 + M * D * 4) / (hbm_gbs * 1e9) * 1e3          # x and t (fp16) read twice, dx (fp32) written once
        lines.append(f"  HBM floor at {hbm_gbs:.0f} GB/s: {floor_ms:.3f} ms; this library runs at {floor_ms / med[variants[0][0]]:.2f} of it")
    state["inner"] = 1
    lines.append(f"  peak memory above the operands: feature_reg {peak_above(ours):.1f} MiB, torch eager {peak_above(eager):.1f} MiB "
                 f"(one fp32 [M, D] matrix: {M * D * 4 / 2 ** 20:.1f} MiB)")
    lines.append("")
    print("\n".join(lines[-7:]), flush=True)
    leaf.grad = None
    torch.cuda.empty_cache()


def step_part(lines, model, N, B, P, depth, rounds):
    from proto_clip_amd import maple, promptsrc
    R, E = model.visual.input_resolution, model.text_projection.shape[1]
    g = torch.Generator(device="cuda").manual_seed(N + B)
    images = torch.randn(B, 3, R, R, device="cuda", generator=g).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    fixed = F.normalize(torch.randn(N, E, device="cuda", generator=g), dim=1).half()
    tokens = prompts(N, P, model.vocab_size, N)
    names = [f"class{i}" for i in range(N)]
    learner = promptsrc.IndependentPromptLearner(names, model, n_ctx_text=P, n_ctx_vision=P, depth_text=depth, depth_vision=depth, tokenized_prompts=tokens,
                                                 seed=3)
    head = promptsrc.PromptSRC(model, learner, fixed)
    coupled = maple.MultiModalPromptLearner(names, model, n_ctx=P, depth=depth, tokenized_prompts=tokens, seed=3)
    maple_head = maple.MaPLe(model, coupled)
    mine = list(learner.parameters())
    theirs = [p.detach().clone().requires_grad_(True) for p in mine]
    tok, L, scale = tokens.cuda(), learner.run_length, 1024.0
    ls = float(head.logit_scale())
    none = torch.zeros(1, 0, model.visual.width, device="cuda")

    def ours():
        for p in mine:
            p.grad = None
        (head.loss(images, labels) * scale).backward()

    def maple_step():
        for p in coupled.parameters():
            p.grad = None
        (maple_head.loss(images, labels) * scale).backward()

    def plain():
        for p in theirs:
            p.grad = None
        ctx, vctx = theirs
        with torch.no_grad():
            zs = F.normalize(torch_features(model, none, images).float(), dim=1)
            z = ls * zs @ fixed.float().t()
        fi, ft = F.normalize(torch_features(model, vctx, images).float(), dim=1), F.normalize(torch_text(model, ctx, tok, L).float(), dim=1)
        s = ls * fi @ ft.t()
        kd = F.kl_div(torch.log_softmax(s, 1), torch.log_softmax(z, 1), reduction="sum", log_target=True) / s.numel()
        loss = F.cross_entropy(s, labels) + 25.0 * F.l1_loss(ft, fixed.float()) + 10.0 * F.l1_loss(fi, zs) + kd
        (loss * scale).backward()

    with torch.no_grad():
        img16, txt16, zs16 = learner.image_features(images), learner.text_features(), head.frozen_image_features(images)
    leaves = [img16.clone().requires_grad_(True), txt16.clone().requires_grad_(True)]

    def four_losses():
        for t in leaves:
            t.grad = None
        fi, ft = leaves
        loss = pag.cosine_cross_entropy(fi, ft, ls, labels=labels, normalize_a=True, normalize_b=True) + 25.0 * pag.feature_reg(ft, fixed, "l1", False) \
            + 10.0 * pag.feature_reg(fi, zs16, "l1", True) + (1.0 / N) * pag.cosine_kd(fi, ft, ls, zs16, fixed, ls, normalize_a=True, normalize_b=True,
                                                                                      normalize_teacher_a=True)
        (loss * scale).backward()

    variants = [("(a) this library, PromptSRC step", ours), ("(b) plain torch + SDPA, the same step", plain), ("(c) this library, MaPLe step", maple_step),
                ("(d) this library, the four loss calls alone", four_losses)]
    times = alternate(variants, rounds)
    med = {name: statistics.median(times[name]) for name, _ in variants}
    lines.append(f"one step: ViT-B/16 towers, {N} class names at {L} tokens, {B} images, {P} + {P} rows at depth {depth}, loss scale {scale:g}  "
                 f"(1 step x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<46s} {med[name]:9.2f} ms  (min {min(times[name]):8.2f}, max {max(times[name]):8.2f})")
    a, b, c, d = (med[name] for name, _ in variants)
    lines.append(f"  (a) / (b) = {a / b:.2f} ({verdict(a / b)});  (a) / (c) = {a / c:.2f} (the frozen vision pass and three more loss calls);  "
                 f"(d) / (a) = {d / a:.3f} of the step in the four loss calls, forward and backward")
    ours()
    plain()
    for name, p, q in zip(("ctx", "vctx"), mine, theirs):                       # not a gate: the fixtures grade against float64
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
    print("\n".join(lines[-12:]), flush=True)
    for p in mine + theirs + list(coupled.parameters()):
        p.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the floor is computed from")
    ap.add_argument("--quick", action="store_true", help="2-block towers and small cases: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/promptsrc_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/promptsrc_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    kernel_part([], 1000, 512, "l1", args.rounds, args.hbm_gbs)                 # a discarded pass: the first intervals of a process run at ramping clocks
    for M, D in ((1000, 512), (4, 512), (50000, 1024)) if not args.quick else ((100, 512), (3000, 1024)):
        for mode in ("l1", "cos"):
            kernel_part(lines, M, D, mode, args.rounds, args.hbm_gbs)
    kw = dict(BACKBONES["ViT-B/16"])
    if args.quick:
        kw["vision_layers"] = kw["transformer_layers"] = 2
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    depth = min(9, len(model.visual.transformer.resblocks), len(model.transformer.resblocks))
    for N in (1000, 37) if not args.quick else (37,):
        for B in (4, 32) if not args.quick else (4,):
            step_part(lines, model, N, B, 4, depth, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
