"""MaPLe without a device: the CPU emulations of csrc/pclip_maple.hip's documented orders (tests/maple_ref.py) stay inside their derived tolerances against
float64 while every deliberately wrong walk falls outside, the learner's parameters are exactly its three tensors, and the refusals that need no GPU."""
import pytest
import torch

import coop_ref
import maple_ref
import vpt_ref
from spec import RESNET, SMALL, TINY


# ---- the emulations against float64 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("L,off,P", [(9, 1, 4), (9, 0, 1), (7, 3, 4), (33, 1, 4)])
def test_row_gradient_emulation_is_inside_its_tolerance_and_an_off_by_one_window_is_not(B, L, off, P):
    W = 64
    g16 = vpt_ref.synth_g(B, L, W, 3 * B + L + off)
    want, tol = maple_ref.rows_grad64(g16, B, L, off, P), maple_ref.tol_rows_grad(g16, B, L, off, P)
    assert maple_ref.worst_ratio(maple_ref.emulate_rows_grad(g16, B, L, off, P), want, tol) <= 1.0
    assert maple_ref.worst_ratio(maple_ref.emulate_rows_grad(g16, B, L, off, P, "off_by_one"), want, tol) > 1.0
    if B > 16:
        assert maple_ref.worst_ratio(maple_ref.emulate_rows_grad(g16, B, L, off, P, "drop_last_slice"), want, tol) > 1.0
    # at off = L - P the window is vpt_ref's
    if off + P == L:
        assert torch.equal(maple_ref.emulate_rows_grad(g16, B, L, off, P), vpt_ref.emulate_grad(g16, B, off, P))


def test_replace_at_an_offset_touches_the_window_only():
    B, L, off, P, W = 3, 9, 1, 4, 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B * L, W, generator=g).half()
    ctx = torch.randn(P, W, generator=g)
    out = maple_ref.replace(x, ctx, B, L, off).view(B, L, W)
    assert torch.equal(out[:, off:off + P], ctx.half().expand(B, P, W))
    assert torch.equal(out[:, :off], x.view(B, L, W)[:, :off]) and torch.equal(out[:, off + P:], x.view(B, L, W)[:, off + P:])
    assert torch.equal(maple_ref.replace(x, ctx, B, L, L - P), vpt_ref.replace(x, ctx, B, L - P))


@pytest.mark.parametrize("family", ["decades", "cancel"])
@pytest.mark.parametrize("depth,P,Wt,Wv", [(1, 1, 64, 128), (3, 5, 64, 192), (3, 2, 128, 256), (2, 16, 128, 40)])
def test_coupling_emulation_is_inside_its_tolerance_and_the_wrong_walks_are_not(depth, P, Wt, Wv, family):
    X, Wc, bc, dY = maple_ref.synth_couple(depth, P, Wt, Wv, 11 * depth + P + Wv, family)
    y64, tol = maple_ref.couple_fwd64(X, Wc, bc), maple_ref.tol_couple_fwd(X, Wc, bc)
    y = maple_ref.emulate_couple_fwd(X, Wc, bc)
    assert y.dtype == torch.float32 and y.shape == (depth, P, Wv)
    assert maple_ref.worst_ratio(y, y64, tol) <= 1.0
    assert maple_ref.worst_ratio(maple_ref.emulate_couple_fwd(X, Wc, bc, "no_bias"), y64, tol) > 1.0
    grads = maple_ref.emulate_couple_bwd(dY, X, Wc)
    for got, want, t in zip(grads, maple_ref.couple_bwd64(dY, X, Wc), maple_ref.tol_couple_bwd(dY, X, Wc)):
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert maple_ref.worst_ratio(got, want, t) <= 1.0
    if depth > 1:
        assert maple_ref.worst_ratio(maple_ref.emulate_couple_fwd(X, Wc, bc, "wrong_depth"), y64, tol) > 1.0
        assert maple_ref.worst_ratio(maple_ref.emulate_couple_bwd(dY, X, Wc, "wrong_depth")[0], maple_ref.couple_bwd64(dY, X, Wc)[0],
                                     maple_ref.tol_couple_bwd(dY, X, Wc)[0]) > 1.0
    if Wv > maple_ref.COUPLE_SLICE:
        assert maple_ref.worst_ratio(maple_ref.emulate_couple_bwd(dY, X, Wc, "drop_last_slice")[0], maple_ref.couple_bwd64(dY, X, Wc)[0],
                                     maple_ref.tol_couple_bwd(dY, X, Wc)[0]) > 1.0


# ---- the learner -----------------------------------------------------------------------------------------------------------------------------------------------

def make_model(kw, seed):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    return build_model(random_state_dict(seed=seed, **kw))


def test_parameters_are_exactly_the_three_tensors():
    from proto_clip_amd import maple
    model = make_model(SMALL, 3)
    names = [f"class{i}" for i in range(4)]
    tokens = coop_ref.prompt_tokens(4, 2, SMALL["vocab_size"], 5)
    learner = maple.MultiModalPromptLearner(names, model, n_ctx=2, depth=3, tokenized_prompts=tokens)
    got = dict(learner.named_parameters())
    assert sorted(got) == ["couple_bias", "couple_weight", "ctx"]
    Wt, Wv = SMALL["transformer_width"], SMALL["vision_width"]
    assert got["ctx"].shape == (3, 2, Wt) and got["couple_weight"].shape == (3, Wv, Wt) and got["couple_bias"].shape == (3, Wv)
    assert all(p.dtype == torch.float32 and p.requires_grad for p in got.values())
    assert float(got["couple_weight"].detach().abs().max()) <= Wt ** -0.5 and float(got["couple_bias"].detach().abs().max()) <= Wt ** -0.5      # nn.Linear's default range
    assert not torch.equal(got["couple_weight"][0], got["couple_weight"][1])
    again = maple.MultiModalPromptLearner(names, model, n_ctx=2, depth=3, tokenized_prompts=tokens)
    assert all(torch.equal(p, q) for p, q in zip(learner.parameters(), again.parameters()))                                  # the seed decides
    assert list(maple.MaPLe(model, learner).parameters()) == list(learner.parameters())
    assert not any(p.requires_grad for p in model.parameters())
    assert learner.run_length == int(tokens.argmax(1).max()) + 1
    from proto_clip_amd import MultiModalPromptLearner as _  # noqa: F401


def test_refusals_that_need_no_device():
    from proto_clip_amd import maple, ops
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.clip.model import BACKBONES, CLIP
    names = [f"class{i}" for i in range(3)]
    tokens = coop_ref.prompt_tokens(3, 2, TINY["vocab_size"], 5)
    model = make_model(TINY, 4)
    with pytest.raises(PclipError, match=r"ModifiedResNet"):
        maple.MultiModalPromptLearner(names, make_model(RESNET, 6), n_ctx=2, depth=1, tokenized_prompts=coop_ref.prompt_tokens(3, 2, RESNET["vocab_size"], 5))
    for depth in (0, 3):
        with pytest.raises(PclipError, match=r"depth=%d outside 1\.\.2" % depth):
            maple.MultiModalPromptLearner(names, model, n_ctx=2, depth=depth, tokenized_prompts=tokens)
    for n_ctx in (0, 17):
        with pytest.raises(PclipError, match=r"n_ctx=%d outside 1\.\.16" % n_ctx):
            maple.MultiModalPromptLearner(names, model, n_ctx=n_ctx, depth=1, tokenized_prompts=tokens)
    with pytest.raises(PclipError, match=r"class_specific"):
        maple.MultiModalPromptLearner(names, model, n_ctx=2, depth=1, tokenized_prompts=tokens, class_specific=True)
    with pytest.raises(PclipError, match=r"class_specific"):
        maple.run_maple({"maple_epochs": 1, "class_specific": True}, None, None, names, model)
    early = tokens.clone()
    early[1] = 0
    early[1, 0], early[1, 2] = TINY["vocab_size"] - 2, TINY["vocab_size"] - 1      # the EOT on the last context position
    with pytest.raises(PclipError, match=r"EOT of prompt 1 .* at or before the last of the\s+n_ctx=2"):
        maple.MultiModalPromptLearner(names, model, n_ctx=2, depth=1, tokenized_prompts=early)
    big = BACKBONES["ViT-L/14@336px"]                                           # 577 vision tokens of its own: refused at construction, no weights needed
    with torch.device("meta"):
        tower = CLIP(big["embed_dim"], big["image_resolution"], big["vision_layers"], big["vision_width"], big["vision_patch_size"], big["context_length"],
                     big["vocab_size"], big["transformer_width"], big["transformer_heads"], big["transformer_layers"])
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx = 577 \+ 2 = 579 vision tokens exceed the attention envelope of 288"):
        maple.MultiModalPromptLearner(names, tower, n_ctx=2, depth=1, tokenized_prompts=torch.zeros(3, 77, dtype=torch.int64))
    odd = make_model(TINY, 4)
    odd.transformer_heads = 2
    with pytest.raises(PclipError, match=r"text tower of width 64 with 2 heads \(head dimension 64 only\)"):
        maple.MultiModalPromptLearner(names, odd, n_ctx=2, depth=1, tokenized_prompts=tokens)
    odd = make_model(TINY, 4)
    odd.visual.heads = 4
    with pytest.raises(PclipError, match=r"vision tower of width 128 with 4 heads \(head dimension 64 only\)"):
        maple.MultiModalPromptLearner(names, odd, n_ctx=2, depth=1, tokenized_prompts=tokens)
    # the wrappers refuse CPU tensors the way their neighbours do
    x16, rows = torch.zeros(18, 64, dtype=torch.float16), torch.zeros(2, 64)
    X, Wc, bc = torch.zeros(1, 2, 64), torch.zeros(1, 128, 64), torch.zeros(1, 128)
    for call in (lambda: ops.rows_replace_(x16, rows, 2, 9, 1), lambda: ops.rows_grad(x16, 2, 9, 1, 2), lambda: ops.couple(X, Wc, bc),
                 lambda: ops.couple_backward(torch.zeros(1, 2, 128), X, Wc)):
        with pytest.raises(PclipError, match="device tensors only"):
            call()
