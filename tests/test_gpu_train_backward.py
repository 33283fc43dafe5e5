"""The backward kernels of the training step per element against float64: the conv adapter (persistent MFMA kernel, per-row VALU kernel, widths 8 / 24 /
32), the fp16-gamma LayerNorm backward, the prototype chain backward and AdamW, under the tolerances of tests/train_bwd_ref.py
(tests/test_train_backward_cpu.py shows that those hold the kernels' documented roundings and reject wrong kernels).  The shapes are train_bwd_ref's lists,
each chosen for an edge; the existing whole-tensor tests (test_gpu_train.py, test_gpu_adapter_shapes.py) stay beside these."""
import pytest
import torch

import train_bwd_ref as ref
from conftest import observe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def _conv_backward(ops, x, g, params, kind, chunk):
    c = {k: v.cuda() for k, v in params.items()}
    three = kind == "conv-3x"
    return ops.adapter_conv_backward(x.cuda(), g.cuda(), three, c["conv1.weight"], c["bn1.weight"], c["bn1.bias"], c.get("conv2.weight"), c.get("bn2.weight"),
                                     c.get("bn2.bias"), c["conv3.weight"], c["bn3.weight"], c["bn3.bias"], chunk=chunk)


def _route(kind, W, D):
    if W != 16:
        return f"width {W}"
    return "persistent MFMA" if kind == "conv-3x" and D <= 576 else "per-row w16"


@pytest.mark.parametrize("kind,W,D,B,chunk", ref.CONV_SHAPES, ids=lambda v: str(v))
def test_conv_backward_against_float64(ops, kind, W, D, B, chunk):
    """Every element of every parameter gradient within tol = C_CONV max(sigma, rms sigma / 4) + A of float64 autograd; the same bits on a second call; the
    bn3 gradients of the zero-padded pixels (p >= D) exactly zero."""
    case = ref.conv_case(kind, W, D, B)
    tol = ref.conv_tolerance(case)
    got = _conv_backward(ops, case["x"], case["g"], case["params"], kind, chunk)
    assert set(got) == set(case["ref"])
    worst = {}
    for k, want in case["ref"].items():
        assert got[k].shape == want.shape and got[k].dtype == torch.float32, k
        worst[k] = ref.worst_ratio(got[k], want, tol[k])
        print(f"{kind} w{W} d{D} {k}: {worst[k]:.3f} of the tolerance")
        observe(f"conv backward, {_route(kind, W, D)}, {k}: |got - float64| / tol", worst[k], 1.0)
    assert max(worst.values()) <= 1.0, worst
    again = _conv_backward(ops, case["x"], case["g"], case["params"], kind, chunk)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    for k in ("bn3.weight", "bn3.bias"):
        assert not bool(got[k].reshape(-1)[D:].any()), k


_rows = {}


def _rows_case(ops, D):
    """x / g / parameters for 2 G + 3 rows (G = the persistent kernel's workgroups) and, for every B of the test, the float64 sum of the first B rows'
    gradients computed one row per launch — once per D."""
    from proto_clip_amd import _lib
    if D not in _rows:
        G = _lib.load().pclip_adapter_conv_backward_partials(10 ** 6, D, 1)
        assert G > 1
        Bs = (1, G - 1, G, G + 1, 2 * G + 3)
        x, g, params = ref.conv_inputs("conv-3x", 16, D, max(Bs))
        acc, snap = None, {}
        for r in range(max(Bs)):
            one = _conv_backward(ops, x[r:r + 1], g[r:r + 1], params, "conv-3x", 512)
            acc = {k: v.double() for k, v in one.items()} if acc is None else {k: acc[k] + one[k].double() for k in acc}
            if r + 1 in Bs:
                snap[r + 1] = {k: v.cpu() for k, v in acc.items()}
        _rows[D] = (G, Bs, x, g, params, snap)
    return _rows[D]


@pytest.mark.parametrize("which", range(5), ids=["B=1", "B=G-1", "B=G", "B=G+1", "B=2G+3"])
@pytest.mark.parametrize("D", [200, 576])
def test_rows_against_persistent_workgroups(ops, D, which):
    """A row's arithmetic does not depend on the workgroup, or the turn of a workgroup, that computes it: the batch equals the float64 sum of its rows
    computed one per launch, up to the fp32 accumulation alone (no sigma here) — stale LDS or registers between a workgroup's rows, a dropped or doubled row at
    B = G +- 1 or a mis-sized partial buffer cannot pass.  The single rows themselves are graded against float64 by the test above."""
    G, Bs, x, g, params, snap = _rows_case(ops, D)
    B = Bs[which]
    _, sums = ref.conv_emulate(x[:B], g[:B], params, "conv-3x", "rne", want_sums=True)
    bound = ref.conv_accumulation_bound(sums, B, D, partial_rows=min(B, G), leaf_error=False)
    got = _conv_backward(ops, x[:B], g[:B], params, "conv-3x", 512)
    worst = {k: ref.worst_ratio(got[k], snap[B][k], bound[k]) for k in got}
    for k, r in worst.items():
        observe(f"conv backward, batch vs its rows one per launch, {k}: |d| / fp32 accumulation bound", r, 1.0)
    print(f"D={D} G={G} B={B}: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    for k in ("bn3.weight", "bn3.bias"):
        assert not bool(got[k].reshape(-1)[D:].any()), k


@pytest.mark.parametrize("scale", ref.LN_SCALES)
@pytest.mark.parametrize("D", ref.LN_WIDTHS)
@pytest.mark.parametrize("R", ref.LN_ROWS)
def test_layernorm_backward_f16_gamma(ops, R, D, scale):
    """R = 1, 3 (lanes of a workgroup without a row), 4, 5, 1024 (256 workgroups, one turn each); D = 1 / 63 (lanes without an element), 64, 65, 640 and 2048 (the
    NI = 4 / 16 / 32 instantiations); dy_scale 1 and the fc blend's 0.2.  The wrapper passes contiguous rows only (no padded stride to cover)."""
    x, gamma, dy = ref.ln_inputs(R, D)
    want, tol = ref.ln_backward_ref(x, gamma, dy, scale)
    got = ops.layernorm_backward(x.cuda(), gamma.cuda(), dy.cuda(), dy_scale=scale)
    assert got[0].dtype == torch.float16 and got[1].dtype == got[2].dtype == torch.float32
    for name, a, b, t in zip(("dx", "dgamma", "dbeta"), got, want, tol):
        r = ref.worst_ratio(a, b, t)
        observe(f"LayerNorm backward (fp16 gamma) {name}: |got - float64| / derived tolerance", r, 1.0)
        assert r <= 1.0, (name, r)
    again = ops.layernorm_backward(x.cuda(), gamma.cuda(), dy.cuda(), dy_scale=scale)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("N,K,D,per_shot,final", ref.PROTO_CASES)
def test_proto_backward_against_float64(ops, N, K, D, per_shot, final):
    case = ref.proto_case(N, K, D, per_shot, final)
    got = ops.proto_backward(case["mem"].cuda(), case["g"].cuda(), N, K, per_shot, final)
    assert got.dtype == torch.float16 and got.shape == case["mem"].shape
    r = ref.worst_ratio(got, case["ref"], ref.proto_tolerance(case))
    observe("proto_backward: |got - float64| / tol", r, 1.0)
    print(f"proto N={N} K={K} D={D} per_shot={per_shot} final={final}: {r:.3f} of the tolerance")
    assert r <= 1.0, r
    assert torch.equal(got, ops.proto_backward(case["mem"].cuda(), case["g"].cuda(), N, K, per_shot, final))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5001, 16384 * 256 + 77])      # the last: past the grid cap of 16384 workgroups, the stride loop wraps
def test_adamw_bit_equal_to_the_restatement(ops, n):
    gen = torch.Generator().manual_seed(n)
    p = (torch.randn(n, generator=gen) * 0.5).half()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    pg, mg, vg = p.clone().cuda(), m.clone().cuda(), v.clone().cuda()
    for step in range(1, 4):
        grad = (torch.randn(n, generator=gen) * 1e-2).half()
        ref.adamw_step(p, grad, m, v, 1e-3, step)
        ops.adamw_(pg, grad.cuda(), mg, vg, 1e-3, step)
        assert torch.equal(mg.cpu(), m), step
        assert torch.equal(vg.cpu(), v), step
        assert torch.equal(pg.cpu(), p), step
