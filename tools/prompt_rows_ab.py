#!/usr/bin/env python3
"""Interleaved A/B of the prompt-row entries (pclip_vpt_replace_f16, pclip_vpt_grad_f32, pclip_rows_replace_f16, pclip_rows_grad_f32,
pclip_prompt_ctx_grad_f32, pclip_prompt_cond_grad_f32) and of the small fp32 layers (pclip_couple_fwd_f32, pclip_couple_bwd_f32, pclip_metanet_fwd_f32,
pclip_metanet_bwd_f32) between two builds of libpclip (proto-clip_amd/libpclip.so against libpclip_old.so, tools/ab_lib.py's convention), through ctypes in
one process on the same tensors, at the shapes of tools/vpt_bench.py, tools/maple_bench.py, tools/coop_bench.py and tools/cocoop_bench.py.

    python tools/prompt_rows_ab.py [--rounds 7] [--iters 20] [--out FILE]

Every round times the series old, new, old' (the old build a second time) in ABBA order, HIP events around `iters` launches.  old against old' is the
spread of the machine on that day: the largest |median(old) - median(old')| / median(old) over the cases.  The gate, per case: median(new) <=
median(old) * (1 + spread).  The outputs of both builds must be torch.equal.  Exit status 1 when a case misses either."""
import argparse
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_bench import timeit  # noqa: E402
from proto_clip_amd import _lib  # noqa: E402

ENTRIES = ("pclip_vpt_replace_f16", "pclip_vpt_grad_f32", "pclip_rows_replace_f16", "pclip_rows_grad_f32", "pclip_prompt_ctx_grad_f32", "pclip_couple_fwd_f32",
           "pclip_couple_bwd_f32", "pclip_metanet_fwd_f32", "pclip_metanet_bwd_f32", "pclip_prompt_cond_grad_f32")


def load(name):
    lib = ctypes.CDLL(os.path.join(REPO, "proto-clip_amd", name))
    for entry in ENTRIES:
        getattr(lib, entry).argtypes = _lib._SIGS[entry]
        getattr(lib, entry).restype = ctypes.c_int
    return lib


def cases():
    """(title, make): make() -> (stream tensor, call(lib, stream tensor) -> the tensors the entry wrote)."""
    P_ = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="cuda")

    def stream_rows(B, L, W, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(B * L, W, generator=g) * 0.1).half().cuda()

    def replace(entry, B, L, off, P, W):
        def make():
            x, ctx = stream_rows(B, L, W, 1), torch.randn(P, W, generator=torch.Generator().manual_seed(2)).cuda()

            def call(lib, x):
                args = (P_(x), P_(ctx), B, off, P, W, st()) if entry == "pclip_vpt_replace_f16" else (P_(x), P_(ctx), B, L, off, P, W, st())
                assert getattr(lib, entry)(*args) == 0
                return (x,)
            return x, call
        return make

    def grad(entry, B, L, off, P, W, clear):
        def make():
            g = stream_rows(B, L, W, 3)
            nslice = (B + 15) // 16
            dctx, part = f32(P, W), f32(nslice, P * W) if nslice > 1 else None

            def call(lib, g):
                head = (P_(g), B, off, P, W) if entry == "pclip_vpt_grad_f32" else (P_(g), B, L, off, P, W)
                assert getattr(lib, entry)(*head, clear, P_(dctx), P_(part), nslice, st()) == 0
                return dctx, g
            return g, call
        return make

    def ctx_grad(N, L, n_ctx, W, specific):
        def make():
            dx = stream_rows(N, L, W, 4)
            nslice = 0 if specific else (N + 15) // 16
            dctx, part = f32(*((N, n_ctx, W) if specific else (n_ctx, W))), f32(nslice, n_ctx * W) if nslice > 1 else None

            def call(lib, dx):
                assert lib.pclip_prompt_ctx_grad_f32(P_(dx), N, L, n_ctx, W, int(specific), P_(dctx), P_(part), nslice, st()) == 0
                return dctx, dx
            return dx, call
        return make

    def couple(backward, depth, P, Wt, Wv):
        def make():
            g = torch.Generator().manual_seed(5)
            X, Wc, bc, dY = (torch.randn(*s, generator=g).cuda() * k for s, k in (((depth, P, Wt), 0.02), ((depth, Wv, Wt), Wt ** -0.5), ((depth, Wv), 0.05),
                                                                                  ((depth, P, Wv), 1.0)))
            nslice = (Wv + _lib.COUPLE_SLICE - 1) // _lib.COUPLE_SLICE
            Y, dW, db, dX, part = f32(depth, P, Wv), f32(depth, Wv, Wt), f32(depth, Wv), f32(depth, P, Wt), f32(depth, nslice, P * Wt)

            def call(lib, X):
                if backward:
                    assert lib.pclip_couple_bwd_f32(P_(dY), P_(X), P_(Wc), depth, P, Wt, Wv, P_(dW), P_(db), P_(dX), P_(part), nslice, st()) == 0
                    return dW, db, dX
                assert lib.pclip_couple_fwd_f32(P_(X), P_(Wc), P_(bc), depth, P, Wt, Wv, P_(Y), st()) == 0
                return (Y,)
            return X, call
        return make

    def metanet(backward, B, E, Hd, Wt):
        def make():
            g = torch.Generator().manual_seed(6)
            f = torch.nn.functional.normalize(torch.randn(B, E, generator=g), dim=1).half().cuda()
            W1, b1, W2, b2, dpi = (torch.randn(*s, generator=g).cuda() * k for s, k in (((Hd, E), E ** -0.5), ((Hd,), 0.05), ((Wt, Hd), Hd ** -0.5), ((Wt,), 0.01),
                                                                                        ((B, Wt), 1.0)))
            h_in = torch.relu(f.float() @ W1.t() + b1).contiguous()              # what the backward reads: any hidden layer with zeros in it will do
            h, pi, dW1, db1, dW2, db2, dpre = f32(B, Hd), f32(B, Wt), f32(Hd, E), f32(Hd), f32(Wt, Hd), f32(Wt), f32(B, Hd)

            def call(lib, f):
                if backward:
                    assert lib.pclip_metanet_bwd_f32(P_(dpi), P_(f), P_(h_in), P_(W2), B, E, Hd, Wt, P_(dW1), P_(db1), P_(dW2), P_(db2), P_(dpre), st()) == 0
                    return dW1, db1, dW2, db2
                assert lib.pclip_metanet_fwd_f32(P_(f), P_(W1), P_(b1), P_(W2), P_(b2), B, E, Hd, Wt, P_(h), P_(pi), st()) == 0
                return h, pi
            return f, call
        return make

    def cond_grad(B, N, L, n_ctx, W):
        def make():
            dx = stream_rows(B * N, L, W, 7)
            nslice = (N + 15) // 16
            dshift, dctx, dpi, part = f32(B, n_ctx, W), f32(n_ctx, W), f32(B, W), f32(B, nslice, n_ctx * W) if nslice > 1 else None

            def call(lib, dx):
                assert lib.pclip_prompt_cond_grad_f32(P_(dx), B, N, L, n_ctx, W, P_(dshift), P_(dctx), P_(dpi), P_(part), nslice, st()) == 0
                return dctx, dpi, dshift, dx
            return dx, call
        return make

    out = []
    for B, L0, P, W in ((256, 197, 8, 768), (1024, 50, 8, 768)):                     # tools/vpt_bench.py
        shape = f"{B} x ({L0} + {P}) x {W}"
        out.append((f"vpt_replace        {shape}", replace("pclip_vpt_replace_f16", B, L0 + P, L0, P, W)))
        out.append((f"vpt_grad           {shape}", grad("pclip_vpt_grad_f32", B, L0 + P, L0, P, W, 0)))
        out.append((f"vpt_grad + clear   {shape}", grad("pclip_vpt_grad_f32", B, L0 + P, L0, P, W, 1)))
    B, L, off, P, W = 1000, 30, 1, 2, 512                                             # tools/maple_bench.py: the text tower's context rows
    shape = f"{B} x {L} x {W}, rows {off} .. {off + P - 1}"
    out.append((f"rows_replace       {shape}", replace("pclip_rows_replace_f16", B, L, off, P, W)))
    out.append((f"rows_grad          {shape}", grad("pclip_rows_grad_f32", B, L, off, P, W, 0)))
    out.append((f"rows_grad + clear  {shape}", grad("pclip_rows_grad_f32", B, L, off, P, W, 1)))
    for specific in (False, True):                                                    # tools/coop_bench.py: ImageNet's class names, L_eff = 30
        out.append((f"prompt_ctx_grad    1000 x 30 x 512, n_ctx 16, {'class-specific' if specific else 'shared'}", ctx_grad(1000, 30, 16, 512, specific)))
    for depth in (9, 12):                                                             # tools/maple_bench.py: the coupling function at ViT-B/16's widths
        for P in (2, 4):
            shape = f"depth {depth}, P = {P}, 512 -> 768"
            out.append((f"couple_fwd         {shape}", couple(False, depth, P, 512, 768)))
            out.append((f"couple_bwd         {shape}", couple(True, depth, P, 512, 768)))
    for B in (1, 4, 16):                                                              # tools/cocoop_bench.py: the meta-net and the conditional gradient
        out.append((f"metanet_fwd        B = {B}, 512 -> 32 -> 512", metanet(False, B, 512, 32, 512)))
        out.append((f"metanet_bwd        B = {B}, 512 -> 32 -> 512", metanet(True, B, 512, 32, 512)))
    for B, N in ((4, 1000), (16, 37)):
        out.append((f"prompt_cond_grad   {B} x {N} x 12 x 512, n_ctx 4", cond_grad(B, N, 12, 4, 512)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    libs = {"old": load("libpclip_old.so"), "new": load("libpclip.so")}
    series = (("old", "old"), ("new", "new"), ("old'", "old"))
    rows = []
    for title, make in cases():
        t, call = make()
        wrote = {}
        for name, lib in libs.items():                                                # the same input, a fresh copy for each build
            wrote[name] = [o.clone() for o in call(lib, t.clone())]
        same = all(torch.equal(a, b) for a, b in zip(wrote["old"], wrote["new"]))
        times = {label: [] for label, _ in series}
        for r in range(args.rounds):                                                  # ABBA: whichever series runs first in a round pays the clock ramp
            for label, name in (series if r % 2 == 0 else series[::-1]):
                times[label].append(timeit(lambda: call(libs[name], t), iters=args.iters, warm=3) * 1e6)
        rows.append((title, {label: sorted(v)[len(v) // 2] for label, v in times.items()}, same))
    spread = max(abs(m["old"] - m["old'"]) / m["old"] for _, m, _ in rows)
    lines = [f"prompt-row entries, old build against new build: medians of {args.rounds} rounds x {args.iters} launches, us per call",
             f"old-against-old spread of this run (largest |old - old'| / old over the cases): {100 * spread:.2f} %"]
    bad = 0
    for title, m, same in rows:
        ok, again = m["new"] <= m["old"] * (1 + spread) and same, m["old'"]
        bad += not ok
        lines.append(f"{title:72s} old {m['old']:8.2f}  new {m['new']:8.2f} ({100 * (m['new'] / m['old'] - 1):+6.2f} %)  old' {again:8.2f}  "
                     f"identical {same}  {'ok' if ok else 'MISSED'}")
    lines.append("every case within the gate" if not bad else f"{bad} case(s) missed the gate")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
