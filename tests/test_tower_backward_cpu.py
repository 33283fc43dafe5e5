"""The tolerances of the attention backward (tests/attention_bwd_ref.py) checked without a GPU: a float64 emulation with exactly the kernel's documented
roundings stays inside them, three wrong kernels do not, and the float64 block backward the GPU tests lean on equals torch autograd."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_bwd_ref as ref                                     # noqa: E402

B, H = 2, 2
CASES = [(1, False), (5, False), (77, True), (197, False), (288, False)]
_cache = {}


def case(L, causal):
    """Inputs, float64 reference and tolerance of a shape, computed once."""
    key = (L, causal)
    if key not in _cache:
        qkv, dout = ref.clustered_qkv(B, L, H, seed=100 + L)
        _cache[key] = (qkv, dout) + ref.reference(qkv, dout, B, L, H, causal)
    return _cache[key]


@pytest.mark.parametrize("L,causal", CASES)
def test_bounds_hold_the_documented_roundings(L, causal):
    qkv, dout, want, tol = case(L, causal)
    got, ds16 = ref.emulate(qkv, dout, B, L, H, causal, want_ds=True)
    ratio = ref.worst_ratio(got, want, tol)
    print(f"L={L} causal={causal}: emulation at {ratio:.3f} of the bound")
    assert ratio <= 1.0
    # the inputs: no row of dS with more than one admissible key underflows to zeros in fp16 (a row with ONE key has dS = P (dP - P dP) = 0 exactly)
    nonzero = (ds16 != 0).any(dim=-1)
    rows = torch.arange(L) >= 1 if causal else torch.full((L,), L > 1)
    assert bool(nonzero[..., rows].all())


@pytest.mark.parametrize("L,causal", CASES)
def test_bounds_reject_wrong_kernels(L, causal):
    """Without the rowsum term: every shape (at L = 1 the true dS is zero and dP is not).  Without the 1/8: every shape with more than one key (at L = 1
    dQ = dK = 0 with or without it: the variant IS the kernel there).  Non-causal where causal was asked: the causal shape."""
    qkv, dout, want, tol = case(L, causal)
    variants = ["no_rowsum"] + (["no_scale"] if L > 1 else []) + (["non_causal"] if causal else [])
    for variant in variants:
        ratio = ref.worst_ratio(ref.emulate(qkv, dout, B, L, H, causal, variant=variant), want, tol)
        print(f"L={L} causal={causal} {variant}: {ratio:.1f} x the bound")
        assert ratio > 1.0, variant


@pytest.mark.parametrize("L,heads,causal", [(5, 1, False), (26, 2, False), (12, 2, True)])
def test_block_backward_restatement_matches_autograd(L, heads, causal):
    W, Bn = heads * 64, 3
    g = torch.Generator().manual_seed(7 + L)
    P = ref.random_block(W, seed=L)
    x = torch.randn(Bn * L, W, generator=g).double()
    gy = torch.randn(Bn * L, W, generator=g).double()
    y, dx, G = ref.block_forward_backward64(x, P, gy, Bn, L, heads, causal)
    xa = x.clone().requires_grad_(True)
    Pa = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ya = ref.block_forward_torch(xa, Pa, Bn, L, heads, causal)
    assert torch.allclose(y, ya.detach(), rtol=1e-11, atol=1e-11)
    (ya * gy).sum().backward()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(dx, xa.grad) < 1e-11
    for k in ref.BLOCK_KEYS:
        assert rel(G[k], Pa[k].grad) < 1e-11, k


def test_small_kernel_references_are_consistent():
    """The float64 restatements of the small kernels against autograd."""
    g = torch.Generator().manual_seed(3)
    u = torch.randn(17, 64, generator=g).half()
    dy = torch.randn(17, 64, generator=g).half()
    ua = u.double().requires_grad_(True)
    (ua * torch.sigmoid(1.702 * ua) * dy.double()).sum().backward()
    assert torch.allclose(ref.quick_gelu_backward_ref(u, dy)[0], ua.grad, rtol=1e-12, atol=1e-14)
    x = torch.randn(17, 192, generator=g).half()
    gam = (1 + 0.1 * torch.randn(192, generator=g)).float()
    res = torch.randn(17, 192, generator=g).half()
    xa, ga, ba = x.double().requires_grad_(True), gam.double().requires_grad_(True), torch.zeros(192, dtype=torch.float64, requires_grad=True)
    dyl = torch.randn(17, 192, generator=g).half()
    (torch.nn.functional.layer_norm(xa, (192,), ga, ba, 1e-5) * dyl.double()).sum().backward()
    (dx, dg, db), _ = ref.layernorm_backward_ref(x, gam, dyl, res)
    assert torch.allclose(dx, xa.grad + res.double(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(dg, ga.grad, rtol=1e-10, atol=1e-12) and torch.allclose(db, ba.grad, rtol=1e-10, atol=1e-12)


def test_unfreeze_and_the_tape_plan_on_the_host():
    """CLIP.unfreeze marks the tail it names and returns it; the plan finds the first trainable block and refuses the frozen prefix (no kernel runs)."""
    from conftest import SMALL
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.clip.model import build_model, random_state_dict
    model = build_model(random_state_dict(seed=3, **SMALL))
    assert not any(p.requires_grad for p in model.parameters())
    assert model.visual._tape_from() is None and model._text_tape_from() is None
    params = model.unfreeze(visual_blocks=1, text_blocks=2)
    named = {n for n, p in model.named_parameters() if p.requires_grad}
    assert len(params) == len(named) == 12 * 3 + 6 and all(p.requires_grad for p in params)
    assert "visual.transformer.resblocks.2.mlp.c_fc.weight" in named and "transformer.resblocks.1.ln_1.bias" in named and "visual.proj" in named
    assert not any(n.startswith(("visual.transformer.resblocks.1.", "transformer.resblocks.0.", "visual.conv1", "token_embedding")) for n in named)
    assert model.visual._tape_from() == 2 and model._text_tape_from() == 1
    for p in model.parameters():
        p.requires_grad_(False)
    assert len(model.unfreeze(heads=True)) == 6 and model.visual._tape_from() == 3 and model._text_tape_from() == 3
    assert model.unfreeze(visual_blocks=0, text_blocks=0, heads=False) == []
    with pytest.raises(PclipError, match="visual_blocks=4"):
        model.unfreeze(visual_blocks=4)
    model.visual.ln_pre.weight.requires_grad_(True)
    with pytest.raises(PclipError, match=r"visual\.ln_pre\.weight"):
        model.visual._tape_from()
    model.token_embedding.weight.requires_grad_(True)
    with pytest.raises(PclipError, match=r"token_embedding\.weight"):
        model._text_tape_from()
