#!/usr/bin/env python3
"""ops.attention timed with HIP events (20 launches after 3 warm-up) at the streamed-K/V kernel's sequence lengths and, for comparison,
at ViT-L/14's 257 tokens on the resident-K/V kernel; TFLOP/s = 4 L^2 64 B H / time."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd import ops, _lib
_lib.load()
def run(B, L, H):
    W = H * 64
    qkv = torch.randn(B * L, 3 * W, device="cuda").half()
    for _ in range(3): ops.attention(qkv, B, L, H)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n): ops.attention(qkv, B, L, H)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    fl = 4.0 * L * L * 64 * B * H
    print(f"attention B={B} L={L} H={H}: {us:9.1f} us  {fl / us / 1e6:7.1f} TFLOP/s", flush=True)
run(512, 257, 16)
run(256, 577, 16)
run(256, 289, 16)
run(64, 1025, 16)
