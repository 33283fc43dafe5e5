#!/usr/bin/env python3
"""The stride-1 3x3 convolutions of RN50x4 / RN50x16 whose channel counts are outside {32, 64k}: the implicit-GEMM tail kernel
(ops.conv3x3_bn) against the materialised path it replaces (ops.im2col3x3 + ops.gemm_bn), us per call and useful TFLOP/s
(2 * pixels * Cout * 9 * Cin), 256 images per pass as ModifiedResNet.chunk runs them."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import ops

SHAPES = [("RN50x4 stem conv2", 144, 40, 40), ("RN50x4 stem conv3", 144, 40, 80), ("RN50x4 layer1 conv2", 72, 80, 80),
          ("RN50x4 layer2 conv2 b0", 72, 160, 160), ("RN50x4 layer2 conv2", 36, 160, 160),
          ("RN50x16 stem conv2", 192, 48, 48), ("RN50x16 stem conv3", 192, 48, 96), ("RN50x16 layer1 conv2", 96, 96, 96)]


def t(fn, n=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
for name, H, Cin, Cout in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(1)
    x = (torch.randn(B * H * H, Cin, device="cuda", generator=g) * 0.7).half()
    w = (torch.randn(Cout, (9 * Cin + 63) // 64 * 64, device="cuda", generator=g) * (9 * Cin) ** -0.5).half()
    w[:, 9 * Cin:] = 0
    sc, sh = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
    fl = 2.0 * B * H * H * Cout * 9 * Cin
    imp = t(lambda: ops.conv3x3_bn(x, w, sc, sh, B, H, H, Cin))
    col = t(lambda: ops.gemm_bn(ops.im2col3x3(x, (H * H * Cin, H * Cin, Cin, 1), B, H, H, Cin, 1), w, sc, sh))
    print(f"B={B:4d} {name:23s} {Cin:3d}->{Cout:3d} {H:3d}x{H:<3d}: implicit {imp:8.1f} us ({fl / imp * 1e-6:5.0f} TFLOP/s)   "
          f"im2col + gemm_bn {col:8.1f} us ({fl / col * 1e-6:5.0f} TFLOP/s)   implicit x{col / imp:.2f}", flush=True)
    del x, w
    torch.cuda.empty_cache()
