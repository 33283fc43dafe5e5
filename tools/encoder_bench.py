#!/usr/bin/env python3
"""encode_image throughput of every backbone the reference lists (RN50x4 / RN50x16 included), and ViT-L/14@336px (random-init weights,
synthetic images).  Optional arguments: backbone names to run only those (e.g. `ViT-L/14@336px ViT-L/14`, `RN50x4 RN50x16`)."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict


def resnet_gflop(kw):
    """GFLOP per image of the ModifiedResNet tower as the reference computes it (clip/model.py:10-152): 2 M N K of every convolution
    (stem 3x3 / stride 2, 3x3, 3x3; per bottleneck conv1 at the input resolution, conv2 before the anti-aliasing pool, conv3 and the
    downsample after it) and of the attention pool (q / k / v projections of all HW + 1 tokens, scores and weighted sum for every query, c_proj)."""
    R, w, layers, D = kw["image_resolution"], kw["vision_width"], kw["vision_layers"], kw["embed_dim"]
    H, f = R // 2, 0.0
    f += 2 * H * H * (w // 2) * 27 + 2 * H * H * (w // 2) * 9 * (w // 2) + 2 * H * H * w * 9 * (w // 2)
    H, inpl = H // 2, w
    for planes, n, stride in zip((w, 2 * w, 4 * w, 8 * w), layers, (1, 2, 2, 2)):
        for b in range(n):
            s = stride if b == 0 else 1
            Ho = H // s
            f += 2 * H * H * planes * inpl + 2 * H * H * planes * 9 * planes + 2 * Ho * Ho * 4 * planes * planes
            if b == 0 and (s > 1 or inpl != 4 * planes):
                f += 2 * Ho * Ho * 4 * planes * inpl
            inpl, H = 4 * planes, Ho
    E, L = 32 * w, H * H + 1
    f += 3 * 2 * L * E * E + 2 * 2 * L * L * E + 2 * L * E * D
    return f / 1e9


# GFLOP per image (336 px: same count at 577 tokens); the wide ResNets from their layer shapes
GF = {"ViT-B/32": 8.8, "ViT-B/16": 35.1, "ViT-L/14": 162.0, "ViT-L/14@336px": 381.0, "RN50": 12.2, "RN101": 19.6}
for _n, _ref in (("RN50", 12.2), ("RN101", 19.6)):      # the function against the published figures of the towers it also covers
    assert abs(resnet_gflop(BACKBONES[_n]) - _ref) < 0.01 * _ref, (_n, resnet_gflop(BACKBONES[_n]))
GF.update({n: round(resnet_gflop(BACKBONES[n]), 2) for n in ("RN50x4", "RN50x16")})
RUNS = (("ViT-B/32", 1024), ("ViT-B/16", 1024), ("ViT-L/14", 512), ("ViT-L/14@336px", 256), ("RN50", 256), ("RN50", 1024), ("RN101", 256), ("RN101", 1024),
        ("RN50x4", 256), ("RN50x4", 1024), ("RN50x16", 256), ("RN50x16", 1024))
unknown = [a for a in sys.argv[1:] if a not in GF]
if unknown:
    sys.exit(f"unknown backbone(s) {unknown}; choose from {sorted(GF)}")
for name, B in RUNS:
    if sys.argv[1:] and name not in sys.argv[1:]:
        continue
    kw = BACKBONES[name]
    model = build_model(random_state_dict(seed=1, **kw)).cuda()
    x = torch.randn(B, 3, kw["image_resolution"], kw["image_resolution"], device="cuda")
    with torch.no_grad():
        for _ in range(3): model.encode_image(x)          # (one warm-up pass was not enough: RN50 once read 9.7 ms instead of 6.9, profiles/r04_ab_attention16.txt)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); n = 10
        for _ in range(n): model.encode_image(x)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
    print(f"{name:9s} batch {B:5d}: {1e3*dt:8.1f} ms  {B/dt:9.0f} img/s  {B/dt*GF[name]/1e3:7.0f} TFLOP/s-equivalent", flush=True)
    del model, x; torch.cuda.empty_cache()
