"""pclip_attention_backward_f16 and the small backward kernels of csrc/pclip_tower_bwd.hip against float64 under the tolerances derived from their
documented roundings (tests/attention_bwd_ref.py; tests/test_tower_backward_cpu.py shows those bounds hold the roundings and reject wrong kernels).

Shapes: L = 1 and 5 (one partial tile), 50 / 64 / 65 (two tiles; a full one; one past it), 197 / 257 / 288 (the eight-wave form: ViT-B/16, ViT-L/14, the
envelope's end = nine full tiles), causal 1 / 8 / 77 (the text tower), and a single head at L = 26."""
import pytest
import torch

import attention_bwd_ref as ref
from conftest import observe

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, L, False) for L in (1, 5, 50, 64, 65, 197, 257, 288)] + [(2, 2, L, True) for L in (1, 8, 77)] + [(2, 1, 26, False)]
_cache = {}


def case(B, H, L, causal):
    key = (B, H, L, causal)
    if key not in _cache:
        qkv, dout = ref.clustered_qkv(B, L, H, seed=100 + L)
        want, tol = ref.reference(qkv, dout, B, L, H, causal)
        _cache[key] = (qkv, dout, want, tol)
    return _cache[key]


@pytest.mark.parametrize("B,H,L,causal", SHAPES)
def test_attention_backward_against_float64(B, H, L, causal):
    from proto_clip_amd import ops
    qkv, dout, want, tol = case(B, H, L, causal)
    W = H * 64
    got = ops.attention_backward(qkv.cuda().view(B * L, 3 * W), dout.cuda().view(B * L, W), B, L, H, causal=causal)
    assert got.shape == (B * L, 3 * W) and got.dtype == torch.float16
    got = got.view(B, L, 3 * W)
    for name, sl in (("dQ", slice(0, W)), ("dK", slice(W, 2 * W)), ("dV", slice(2 * W, 3 * W))):
        r = ref.worst_ratio(got[..., sl], want[..., sl], tol[..., sl])
        print(f"L={L} H={H} causal={causal} {name}: {r:.3f} of the derived bound")
        observe(f"attention backward {name}: |got - float64| / derived tolerance", r, 1.0)
        assert r <= 1.0, (name, r)
    # the same inputs again: the same bits (no atomics, one summation order)
    again = ops.attention_backward(qkv.cuda().view(B * L, 3 * W), dout.cuda().view(B * L, W), B, L, H, causal=causal)
    assert torch.equal(again.view(B, L, 3 * W), got)


def test_causal_mask_blocks_later_keys():
    """L = 77 causal: a dout that is zero except at query row r leaves dK and dV zero at the keys after r, and dQ zero at every other row."""
    from proto_clip_amd import ops
    B, H, L, r = 2, 2, 77, 40
    W = H * 64
    qkv, dout, _, _ = case(B, H, L, True)
    one = torch.zeros_like(dout)
    one[:, r] = dout[:, r]
    got = ops.attention_backward(qkv.cuda().view(B * L, 3 * W), one.cuda().view(B * L, W), B, L, H, causal=True).view(B, L, 3 * W).cpu()
    assert not bool(got[:, r + 1:, W:].any())                                    # dK, dV of the keys the row cannot see
    assert bool(got[:, :r + 1, W:2 * W].any()) and bool(got[:, :r + 1, 2 * W:].any())
    rest = torch.ones(L, dtype=torch.bool)
    rest[r] = False
    assert not bool(got[:, rest, :W].any()) and bool(got[:, r, :W].any())
    want, tol = ref.reference(qkv, one, B, L, H, True)
    assert ref.worst_ratio(got, want, tol) <= 1.0


def test_envelope_is_refused():
    from proto_clip_amd import ops
    from proto_clip_amd._lib import PclipError
    x = torch.zeros(289, 3 * 64, dtype=torch.float16, device="cuda")
    with pytest.raises(PclipError, match="L=289"):
        ops.attention_backward(x, x[:, :64].contiguous(), 1, 289, 1)
    y = torch.zeros(16, 3 * 32, dtype=torch.float16, device="cuda")
    with pytest.raises(PclipError, match="head dim 32"):
        ops.attention_backward(y, y[:, :32].contiguous(), 1, 16, 1, dh=32)


ROWS, WIDTHS = (1, 17, 394, 1024), (64, 192, 768)
_small = {}


def small_case(R, D):
    if (R, D) not in _small:
        g = torch.Generator().manual_seed(1000 * R + D)
        rn = lambda *s: torch.randn(*s, generator=g)
        _small[(R, D)] = dict(x=(rn(R, D) * 1.5 + 0.3 * rn(1, D)).half(), dy=(rn(R, D) * 0.05).half(), res=(rn(R, D) * 0.05).half(),
                              gamma=(1 + 0.3 * rn(D)).float(), u=(rn(R, D) * 2).half())
    return _small[(R, D)]


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_quick_gelu_backward(R, D):
    from proto_clip_amd import ops
    c = small_case(R, D)
    want, tol = ref.quick_gelu_backward_ref(c["u"], c["dy"])
    r = ref.worst_ratio(ops.quick_gelu_backward(c["u"].cuda(), c["dy"].cuda()), want, tol)
    observe("QuickGELU backward: |got - float64| / derived tolerance", r, 1.0)
    assert r <= 1.0, r


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_colsum_f16(R, D):
    from proto_clip_amd import ops
    c = small_case(R, D)
    nslice = max(1, min(128, (R + 31) // 32))                                    # ops.colsum_f16's slicing
    want, tol = ref.colsum_ref(c["x"], nslice)
    got = ops.colsum_f16(c["x"].cuda())
    assert got.dtype == torch.float32 and got.shape == (D,)
    r = ref.worst_ratio(got, want, tol)
    observe("fp16 column sums: |got - float64| / derived tolerance", r, 1.0)
    assert r <= 1.0, r
    assert torch.equal(got, ops.colsum_f16(c["x"].cuda()))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("R", ROWS)
def test_layernorm_backward_f32(R, D, with_res):
    from proto_clip_amd import ops
    c = small_case(R, D)
    res = c["res"] if with_res else None
    (wdx, wdg, wdb), (tdx, tdg, tdb) = ref.layernorm_backward_ref(c["x"], c["gamma"], c["dy"], res)
    dx, dg, db = ops.layernorm_backward_f32(c["x"].cuda(), c["gamma"].cuda(), c["dy"].cuda(), residual=None if res is None else res.cuda())
    assert dx.dtype == torch.float16 and dg.dtype == db.dtype == torch.float32
    for name, got, want, tol in (("dx", dx, wdx, tdx), ("dgamma", dg, wdg, tdg), ("dbeta", db, wdb, tdb)):
        r = ref.worst_ratio(got, want, tol)
        observe(f"LayerNorm backward (fp32 gamma) {name}: |got - float64| / derived tolerance", r, 1.0)
        assert r <= 1.0, (name, r)
