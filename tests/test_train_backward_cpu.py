"""The tolerances of the training step's backward kernels (tests/train_bwd_ref.py) checked without a GPU: the float64 emulations with exactly the kernels'
documented roundings stay inside them at every shape of the GPU test (tests/test_gpu_train_backward.py), deliberately wrong kernels exceed them by 10 x,
the measured constants C_CONV / C_PROTO are twice the worst ratio seen here, the float64 references equal torch autograd, and the AdamW restatement
reproduces torch.optim.AdamW."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_bwd_ref as ref                                         # noqa: E402


def _shape_id(sh):
    return "-".join(str(v) for v in sh)


@pytest.mark.parametrize("shape", ref.CONV_SHAPES, ids=_shape_id)
def test_conv_bounds_hold_the_documented_roundings(shape):
    kind, W, D, B, _ = shape
    case = ref.conv_case(kind, W, D, B)
    rne, held = ref.conv_sigma_ratios(case)
    tol = ref.conv_tolerance(case)
    worst = max(ref.worst_ratio(case["rne"][k], case["ref"][k], tol[k]) for k in tol)
    print(f"{kind} w{W} d{D} B={B}: |emulation - float64| / max(sigma, rms sigma / 4): RNE {rne:.2f}, held out {held:.2f}; RNE at {worst:.3f} of the tolerance")
    assert 2.0 * max(rne, held) <= ref.C_CONV, (rne, held)             # C_CONV is (at least) twice the worst ratio of every shape
    assert worst <= 1.0
    for h in case["held"]:
        assert max(ref.worst_ratio(h[k], case["ref"][k], tol[k]) for k in tol) <= 1.0
    # the inputs: every parameter tensor has a gradient that is not all zeros, and a sigma that is not (bn3.bias: a sum of exact values)
    for k, v in case["ref"].items():
        assert bool(v.any()) and (k == "bn3.bias" or bool(case["sigma"][k].any())), k
    assert not bool(case["sigma"]["bn3.bias"].any())
    assert set(case["ref"]) == set(ref.CONV_KEYS if kind == "conv-3x" else [k for k in ref.CONV_KEYS if "2" not in k])


def test_conv_constant_is_twice_the_measured_worst():
    """C_CONV is not looser than 2 x the worst ratio, rounded up to its printed digits."""
    worst = [max(ref.conv_sigma_ratios(ref.conv_case(kind, W, D, B))) for kind, W, D, B, _ in ref.CONV_SHAPES]                  # cached by the tests above
    print(f"worst ratio over {len(worst)} shapes {max(worst):.3f}; C_CONV = {ref.C_CONV}")
    assert 2.0 * max(worst) <= ref.C_CONV <= 2.0 * max(worst) + 0.1


@pytest.mark.parametrize("shape", ref.CONV_SHAPES, ids=_shape_id)
def test_conv_bounds_reject_wrong_kernels(shape):
    """Where a variant cannot differ from the kernel: the circular halo, the unmirrored taps and the skipped LN2 tile need a conv2, i.e. conv-3x; statistics
    over the first D pixels are the kernel's own at D = s^2 (64, 256, 576, 1024).  A dropped last row differs at every shape."""
    kind, W, D, B, _ = shape
    case = ref.conv_case(kind, W, D, B)
    tol = ref.conv_tolerance(case)
    s2 = ref.side(D) ** 2
    variants = ["last_row_dropped"] + (["circular_halo", "unmirrored_taps", "ln2_tile_skipped"] if kind == "conv-3x" else []) + (["stats_over_D"] if D < s2 else [])
    for variant in ref.VARIANTS:
        got = ref.conv_emulate(case["x"], case["g"], case["params"], kind, "rne", variant=variant)
        ratios = {k: ref.worst_ratio(got[k], case["ref"][k], tol[k]) for k in tol}
        worst = max(ratios, key=ratios.get)
        print(f"{kind} w{W} d{D} {variant}: {ratios[worst]:.1f} x the tolerance ({worst})")
        if variant in variants:
            assert ratios[worst] >= 10.0, (variant, ratios)
        else:                                                           # the variant IS the kernel here
            assert all(torch.equal(got[k], case["rne"][k]) for k in tol), variant


@pytest.mark.parametrize("kind,W,D", [("conv-3x", 16, 3), ("conv-3x", 16, 200), ("conv-2x", 16, 100), ("conv-3x", 24, 65), ("conv-2x", 8, 640)])
def test_conv_references_equal_autograd(kind, W, D):
    """conv_reference is autograd of F.conv2d / F.layer_norm; the emulation's graph (LayerNorm and the 3x3 convolution's backward written out) without
    rounding equals it, and so does the oracle's formula (width 16) in float64."""
    x, g, params = ref.conv_inputs(kind, W, D, 5)
    want = ref.conv_reference(x, g, params, kind)
    got = ref.conv_emulate(x, g, params, kind, rounding=None)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert set(got) == set(want)
    for k in want:
        assert rel(got[k], want[k]) <= 1e-10, k
    if W == 16:
        from oracle import train_oracle as to
        p = {k: v.double().requires_grad_(True) for k, v in params.items()}
        (to.adapter_conv(x.double(), p, kind) * g.double()).sum().backward()
        for k in want:
            assert rel(p[k].grad, want[k]) <= 1e-10, k


def test_stochastic_rounding_is_unbiased_and_keeps_fp16_values():
    gen = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(2000, generator=gen, dtype=torch.float64), torch.randn(2000, generator=gen, dtype=torch.float64) * 1e-6])
    runs = torch.stack([ref.stochastic_r16(x, gen) for _ in range(64)])
    assert torch.equal(runs.float().half().double(), runs)                                     # fp16 values, subnormals included
    assert bool(((runs - x).abs() <= torch.maximum(x.abs() * 2.0 ** -10, torch.tensor(2.0 ** -24, dtype=torch.float64))).all())
    assert float(((runs.mean(0) - x) / torch.maximum(x.abs() * 2.0 ** -11, torch.tensor(2.0 ** -25, dtype=torch.float64))).abs().mean()) < 0.2
    h = x.float().half().double()
    assert torch.equal(ref.stochastic_r16(h, gen), h)


# ---- LayerNorm backward, fp16 gamma ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ref.LN_SCALES)
@pytest.mark.parametrize("D", ref.LN_WIDTHS)
@pytest.mark.parametrize("R", ref.LN_ROWS)
def test_layernorm_bounds_hold_and_reject(R, D, scale):
    """The emulation (the kernel's r16s points) is inside the analytic tolerance; a kernel that ignores dy_scale is outside it (at dy_scale = 1 it IS the kernel)."""
    x, gamma, dy = ref.ln_inputs(R, D)
    want, tol = ref.ln_backward_ref(x, gamma, dy, scale)
    got = ref.ln_backward_emulate(x, gamma, dy, scale)
    for name, a, b, t in zip(("dx", "dgamma", "dbeta"), got, want, tol):
        assert ref.worst_ratio(a, b, t) <= 1.0, name
    if scale != 1.0:
        bad = ref.ln_backward_emulate(x, gamma, dy, scale, variant="scale_dropped")
        assert max(ref.worst_ratio(a, b, t) for a, b, t in zip(bad, want, tol)) > 1.0


def test_layernorm_reference_equals_autograd():
    for R, D, scale in ((5, 65, 1.0), (17, 640, 0.2)):
        x, gamma, dy = ref.ln_inputs(R, D)
        xa, ga, ba = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(D, dtype=torch.float64, requires_grad=True)
        s = float(torch.tensor(scale, dtype=torch.float32))
        (s * F.layer_norm(xa, (D,), ga, ba, 1e-5) * dy.double()).sum().backward()
        (dx, dg, db), _ = ref.ln_backward_ref(x, gamma, dy, scale)
        rel = lambda a, b: float((a - b).norm() / b.norm())
        assert rel(dx, xa.grad) <= 1e-10 and rel(dg, ga.grad) <= 1e-10 and rel(db, ba.grad) <= 1e-10


# ---- prototype chain backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,per_shot,final", ref.PROTO_CASES)
def test_proto_bounds_hold_and_reject(N, K, D, per_shot, final):
    """The RNE emulation and the held-out stochastic runs are inside the tolerance; a kernel without the gradient through the shots' norms is outside
    it.  It is the kernel without the per-shot normalisation, and at K = 1 behind the final normalisation, whose gradient is orthogonal to the one shot."""
    case = ref.proto_case(N, K, D, per_shot, final)
    rne, held = ref.proto_sigma_ratios(case)
    print(f"proto N={N} K={K} D={D} per_shot={per_shot} final={final}: RNE {rne:.2f}, held out {held:.2f}")
    assert 2.0 * max(rne, held) <= ref.C_PROTO, (rne, held)
    tol = ref.proto_tolerance(case)
    assert ref.worst_ratio(case["rne"], case["ref"], tol) <= 1.0
    bad = ref.proto_emulate(case["mem"], case["g"], N, K, per_shot, final, variant="norm_term_dropped")
    if per_shot and not (K == 1 and final):
        r = ref.worst_ratio(bad, case["ref"], tol)
        print(f"   without the norms' gradient: {r:.1f} x the tolerance")
        assert r > 1.0
    elif not per_shot:
        assert torch.equal(bad, case["rne"])


def test_proto_constant_is_twice_the_measured_worst():
    worst = [max(ref.proto_sigma_ratios(ref.proto_case(N, K, D, ps, fin))) for N, K, D, ps, fin in ref.PROTO_CASES]
    print(f"worst ratio over {len(worst)} cases {max(worst):.3f}; C_PROTO = {ref.C_PROTO}")
    assert 2.0 * max(worst) <= ref.C_PROTO <= 2.0 * max(worst) + 0.1


def test_proto_reference_is_the_fp16_autograd_chain_in_float64():
    """proto_reference against the existing GPU test's statement of the chain (test_gpu_train.py::test_proto_backward) differentiated in float64."""
    for N, K, D, per_shot, final in ((5, 2, 70, True, True), (3, 32, 512, True, False), (4, 1, 70, False, True)):
        mem, g = ref.proto_inputs(N, K, D)
        m = mem.double().requires_grad_(True)
        zs = m.view(N, K, D)
        if per_shot:
            zs = zs / zs.norm(dim=-1, keepdim=True)
        z = zs.mean(dim=1)
        if final:
            z = z / z.norm(dim=-1, keepdim=True)
        (z * g.double()).sum().backward()
        want = ref.proto_reference(mem, g, N, K, per_shot, final)
        assert float((want - m.grad).norm() / m.grad.norm()) <= 1e-10
        assert float((ref.proto_emulate(mem, g, N, K, per_shot, final, rounding=None) - want).norm() / want.norm()) <= 1e-10


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr,scale", [(1e-3, 1e-2), (2e-3, 1e-4), (1e-4, 1.0)])
def test_adamw_restatement_reproduces_torch(lr, scale):
    """The condition of test_gpu_train.py::test_adamw_matches_torch with the restatement in the kernel's place: exp_avg and exp_avg_sq bit-equal over 7
    steps at n = 5000, at most 2 differing parameter values in total."""
    g = torch.Generator().manual_seed(3)
    n = 5000
    p = torch.nn.Parameter((torch.randn(n, generator=g) * 0.5).half())
    opt = torch.optim.AdamW([p], lr=lr, eps=1e-4, weight_decay=0.05)
    pr = p.data.clone()
    m, v = torch.zeros_like(pr), torch.zeros_like(pr)
    bad = 0
    for step in range(1, 8):
        grad = (torch.randn(n, generator=g) * scale).half()
        p.grad = grad.clone()
        opt.step()
        ref.adamw_step(pr, grad, m, v, lr, step)
        st = opt.state[p]
        assert torch.equal(m, st["exp_avg"]), step
        assert torch.equal(v, st["exp_avg_sq"]), step
        bad += (pr != p.data).sum().item()
        pr.copy_(p.data)
    assert bad <= 2
