#!/usr/bin/env python3
"""Conv adapter forward on cached features (the reference's per-epoch validation pass): rows/s at ImageNet size."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd.model import Adapter
for D, kind in ((512, "conv-3x"), (512, "conv-2x"), (768, "conv-3x"), (1024, "conv-3x")):
    torch.manual_seed(0)
    ad = Adapter(D, kind, dtype=torch.half).cuda()
    x = torch.nn.functional.normalize(torch.randn(50000, D, device="cuda"), dim=-1).half()
    with torch.no_grad():
        y = ad(x, l2norm_out=True); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5): y = ad(x, l2norm_out=True)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
    print(f"D={D} {kind}: 50000 rows {dt*1e3:6.2f} ms = {50000/dt/1e6:5.2f} M rows/s  checksum {y.float().sum().item():.4f} {y.view(torch.int16).to(torch.int64).sum().item()}", flush=True)


# ---- widths 8 / 16 / 24 / 32 and the fc adapter's shapes (profiles/adapter_widths.txt) ------------------------------------------------
# Median of `reps` device-timed calls after two warm-up calls, with the spread (min .. max) beside it.  The torch column is the same chain as
# plain torch ops on the same fp16 state dict (F.conv2d + F.layer_norm): what a user runs without the fused kernels.
import math
import torch.nn.functional as F
from proto_clip_amd import ops
from proto_clip_amd.model import Adapter_FC


def timed(fn, reps=7):
    for _ in range(2): fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def torch_conv_chain(ad, x):
    B, D = x.shape
    s = int(math.ceil(math.sqrt(D)))
    W = ad.conv1.out_channels
    xi = F.pad(x, (0, s * s - D)).view(-1, 1, s, s)
    out = F.layer_norm(F.conv2d(xi, ad.conv1.weight), [W, s, s], ad.bn1.weight, ad.bn1.bias)
    if ad.c_type == "conv-3x":
        out = F.layer_norm(F.conv2d(out, ad.conv2.weight, padding=1), [W, s, s], ad.bn2.weight, ad.bn2.bias)
    out = F.layer_norm(F.conv2d(out, ad.conv3.weight), [1, s, s], ad.bn3.weight, ad.bn3.bias) + xi
    out = out.view(-1, 1, s * s)[:, :, :D].reshape(-1, D)
    return out / out.norm(dim=-1, keepdim=True)


def torch_fc_chain(ad, x):
    fc = ad.fc
    h = F.layer_norm(F.linear(x, fc[0].weight), [fc[0].out_features], fc[1].weight, fc[1].bias)
    h = F.layer_norm(F.linear(h, fc[2].weight), [x.shape[1]], fc[3].weight, fc[3].bias)
    out = 0.2 * h + 0.8 * x
    return out / out.norm(dim=-1, keepdim=True)


fmt = lambda t: f"{t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"
with torch.no_grad():
    for kind in ("conv-3x", "conv-2x"):
        for D in (512, 1024):
            for W in (8, 16, 24, 32):
                torch.manual_seed(0)
                ad = Adapter(D, kind, width=W, dtype=torch.half).cuda()
                x = F.normalize(torch.randn(50000, D, device="cuda"), dim=-1).half()
                tk = timed(lambda: ad(x, l2norm_out=True))
                tt = timed(lambda: torch_conv_chain(ad, x), reps=5)
                print(f"width {W:2d} D={D:4d} {kind}: 50000 rows  kernel {fmt(tk)}  torch {fmt(tt)}  torch / kernel {tt[0] / tk[0]:5.2f}", flush=True)
    for D, r, B in ((640, 4, 50000), (640, 4, 1), (768, 4, 50000), (768, 4, 1), (768, 8, 50000), (512, 16, 50000)):
        torch.manual_seed(0)
        ad = Adapter_FC(D, reduction=r, dtype=torch.half).cuda()
        x = F.normalize(torch.randn(B, D, device="cuda"), dim=-1).half()
        tk = timed(lambda: ad(x, l2norm_out=True))
        tt = timed(lambda: torch_fc_chain(ad, x), reps=5)
        print(f"fc D={D:4d} H={D // r:3d}: {B:5d} rows  kernel {fmt(tk)}  torch {fmt(tt)}  torch / kernel {tt[0] / tk[0]:5.2f}", flush=True)
    for kind in ("conv-3x", "conv-2x"):
        for D in (512, 1024):
            for W in (8, 16, 24, 32):
                torch.manual_seed(0)
                ad = Adapter(D, kind, width=W, dtype=torch.half).cuda()
                x = F.normalize(torch.randn(512, D, device="cuda"), dim=-1).half()
                g = (torch.randn(512, D, device="cuda") * 1e-2).half()
                tb = timed(lambda: ops.adapter_conv_backward(x, g, kind == "conv-3x", ad.conv1.weight, ad.bn1.weight, ad.bn1.bias, ad.conv2.weight, ad.bn2.weight,
                                                             ad.bn2.bias, ad.conv3.weight, ad.bn3.weight, ad.bn3.bias), reps=3)
                print(f"width {W:2d} D={D:4d} {kind}: backward of 512 rows (kernel + column sums) {fmt(tb)}", flush=True)
