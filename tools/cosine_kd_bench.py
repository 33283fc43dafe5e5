#!/usr/bin/env python3
"""The distillation loss over cosine logits (csrc/pclip_cosine_kd.hip, ops.cosine_kd / cosine_kd_backward) and a ProGrad step (proto_clip_amd/prograd.py),
measured with HIP events, warmed and alternated in one process:

    python tools/cosine_kd_bench.py [--out profiles/cosine_kd.txt] [--rounds 7] [--quick]

1. The kernels, forward + dL/da + dL/db + dscale, all four operands normalised, scales 100 / 100, teacher features = student features unless Dt differs:
   against torch eager on the same GPU (normalise, two matmuls, F.kl_div(log_softmax, softmax), .backward() to a, b and the scale) and against
   ops.cosine_cross_entropy forward + backward on the same shape (a distillation call makes two first products where the cross-entropy makes one, and its
   forward runs the cross-entropy's forward twice for the two lse vectors).  Peak memory above the operands, both ways.
2. A ProGrad step (one tower forward, two backward walks, the projection) on the real ViT-B/16 text tower (seeded random weights), n_ctx = 16, 32 cached
   features, 1000 and 37 class names: against a plain-torch restatement with SDPA (tools/maple_bench.torch_text at depth 1, two autograd.grad walks, the
   same projection) and against the CoOp step of the same tree (one forward, ONE backward walk)."""
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
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict  # noqa: E402
from maple_bench import prompts, torch_text, verdict  # noqa: E402
from vpt_bench import alternate  # noqa: E402  (the timing loop)


def peak_above(fn):
    """Peak device memory of one call above what is allocated before it, in MiB (the workspace cache of ops counts: it is part of the call's footprint)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_part(lines, M, T, D, Dt, rounds):
    g = torch.Generator(device="cuda").manual_seed(M + T + Dt)
    a = torch.randn(M, D, device="cuda", generator=g).half()
    b = torch.randn(T, D, device="cuda", generator=g).half()
    ta = a if Dt == D else torch.randn(M, Dt, device="cuda", generator=g).half()
    tb = torch.randn(T, Dt, device="cuda", generator=g).half()
    labels = torch.randint(0, T, (M,), device="cuda", generator=g)
    inner = 5 if M * T <= 1 << 22 else 1
    on = (True, True, True, True)

    def kd():
        for _ in range(inner):
            _, lse, tlse = ops.cosine_kd(a, b, 100.0, ta, tb, 100.0, *on)
            ops.cosine_kd_backward(a, b, 100.0, ta, tb, 100.0, lse, tlse, *on)

    def ce():
        for _ in range(inner):
            _, lse, _ = ops.cosine_cross_entropy(a, b, 100.0, labels, False, True, True)
            ops.cosine_cross_entropy_backward(a, b, 100.0, lse, None, labels, False, True, True)

    leaves = [a.clone().requires_grad_(True), b.clone().requires_grad_(True), torch.tensor(100.0, device="cuda", requires_grad=True)]

    def eager():
        for _ in range(inner):
            for t in leaves:
                t.grad = None
            s = leaves[2] * F.normalize(leaves[0].float(), dim=1).half() @ F.normalize(leaves[1].float(), dim=1).half().t()
            with torch.no_grad():
                z = 100.0 * F.normalize(ta.float(), dim=1).half() @ F.normalize(tb.float(), dim=1).half().t()
                p = torch.softmax(z.float(), 1)
            F.kl_div(torch.log_softmax(s.float(), 1), p, reduction="batchmean").backward()

    variants = [("this library: cosine_kd + cosine_kd_backward", kd), ("torch eager: normalise, 2 matmuls, kl_div, backward", eager),
                ("this library: cosine_cross_entropy + backward", ce)]
    times = alternate(variants, rounds)
    k = 1e3 if M * T <= 1 << 22 else 1.0
    unit = "us" if k == 1e3 else "ms"
    med = {name: statistics.median(times[name]) / inner * k for name, _ in variants}
    lines.append(f"forward + dL/da + dL/db + dscale, M x T = {M} x {T}, D = {D}, Dt = {Dt}  ({inner} passes per interval x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<54s} {med[name]:10.2f} {unit}  (min {min(times[name]) / inner * k:9.2f}, max {max(times[name]) / inner * k:9.2f})")
    r_t, r_c = med[variants[0][0]] / med[variants[1][0]], med[variants[0][0]] / med[variants[2][0]]
    lines.append(f"  cosine_kd / torch eager = {r_t:.2f} ({verdict(r_t)});  cosine_kd / cosine_cross_entropy = {r_c:.2f}"
                 + (" (above 2: the teacher's walk does not overlap, and the forward walks the student twice)" if r_c > 2 else ""))
    inner = 1
    lines.append(f"  peak memory above the operands: cosine_kd {peak_above(kd):.1f} MiB, torch eager {peak_above(eager):.1f} MiB "
                 f"(one fp32 [M, T] matrix: {M * T * 4 / 2 ** 20:.1f} MiB)")
    lines.append("")
    print("\n".join(lines[-7:]), flush=True)
    for t in leaves:
        t.grad = None
    torch.cuda.empty_cache()


def step_part(lines, model, N, B, n_ctx, rounds):
    from proto_clip_amd import coop, prograd
    E = model.text_projection.shape[1]
    g = torch.Generator(device="cuda").manual_seed(N + B)
    feats = F.normalize(torch.randn(B, E, device="cuda", generator=g), dim=1).half()
    teacher = F.normalize(torch.randn(N, E, device="cuda", generator=g), dim=1).half()
    labels = torch.randint(0, N, (B,), device="cuda", generator=g)
    tokens = prompts(N, n_ctx, model.vocab_size, N)
    learner = coop.PromptLearner([f"class{i}" for i in range(N)], model, n_ctx=n_ctx, tokenized_prompts=tokens, seed=3)
    head = prograd.ProGrad(model, learner, teacher)
    plain = coop.CoOp(model, learner)
    tok, L, scale = tokens.cuda(), learner.run_length, 1024.0
    theirs = learner.ctx.detach().clone().requires_grad_(True)
    ls = float(head.logit_scale())

    def ours():
        ce, kl = head.losses(feats, labels)
        head.backward(ce, kl, scale=scale)

    def coop_step():
        learner.ctx.grad = None
        (plain.loss(feats, labels) * scale).backward()

    def torch_step():
        text = torch_text(model, theirs[None], tok, L)
        s = ls * F.normalize(feats.float(), dim=1) @ F.normalize(text.float(), dim=1).t()
        with torch.no_grad():
            p = torch.softmax(ls * F.normalize(feats.float(), dim=1) @ F.normalize(teacher.float(), dim=1).t(), 1)
        ce, kl = F.cross_entropy(s, labels), F.kl_div(torch.log_softmax(s, 1), p, reduction="batchmean")
        g_ce = torch.autograd.grad(ce * scale, [theirs], retain_graph=True)[0]
        g_kl = torch.autograd.grad(kl * scale, [theirs])[0]
        theirs.grad = head.project_(g_ce.clone(), g_kl)

    variants = [("this library: ProGrad step (1 forward, 2 backward walks)", ours), ("plain torch (SDPA): the same step", torch_step),
                ("this library: CoOp step (1 forward, 1 backward walk)", coop_step)]
    times = alternate(variants, rounds)
    med = {name: statistics.median(times[name]) for name, _ in variants}
    lines.append(f"one step: ViT-B/16 text tower, {N} class names at {L} tokens, {B} cached features, n_ctx = {n_ctx}, loss scale {scale:g}  "
                 f"(1 step x {rounds} rounds after 2 warm-ups)")
    for name, _ in variants:
        lines.append(f"  {name:<58s} {med[name]:9.3f} ms  (min {min(times[name]):8.3f}, max {max(times[name]):8.3f})")
    r_t, r_c = med[variants[0][0]] / med[variants[1][0]], med[variants[0][0]] / med[variants[2][0]]
    lines.append(f"  ProGrad / plain torch = {r_t:.2f} ({verdict(r_t)});  ProGrad / CoOp = {r_c:.2f}")
    lines.append("")
    print("\n".join(lines[-6:]), flush=True)
    learner.ctx.grad = None
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a 2-block tower and small cases: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cosine_kd_bench.py measures on the GPU; there is none here")
    _lib.load()
    lines = ["$ python tools/cosine_kd_bench.py " + " ".join(sys.argv[1:]), f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    kernel_part([], 32, 37, 512, 512, args.rounds)                              # a discarded pass: the first intervals of a process run at ramping clocks
    shapes = ((32, 1000, 512, 512), (3669, 37, 512, 512), (50000, 1000, 512, 512), (4096, 4096, 512, 512), (50000, 1000, 512, 768))
    for M, T, D, Dt in shapes if not args.quick else ((32, 100, 512, 512), (300, 37, 512, 768)):
        kernel_part(lines, M, T, D, Dt, args.rounds)
    kw = dict(BACKBONES["ViT-B/16"])
    kw["vision_layers"] = 1                                                     # cached features: the image tower is not run
    if args.quick:
        kw["transformer_layers"] = 2
    model = build_model(random_state_dict(seed=3, **kw)).cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    for N in (1000, 37) if not args.quick else (37,):
        step_part(lines, model, N, 32, 16, args.rounds)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
