"""The backward of the embedding stages (csrc/pclip_embed_bwd.hip) without a GPU: the float64 restatements of tests/tower_prefix_ref.py equal torch's
float64 autograd; the fp32 emulation of the kernels' summation order stays inside the derived tolerances and two wrong walks do not; the entry points are
declared and exported; and CLIP.unfreeze(stem=...) marks, returns and records what it names."""
import os

import pytest
import torch

import tower_prefix_ref as ref
from conftest import REPO, SMALL

from proto_clip_amd import _lib
from proto_clip_amd._lib import PclipError

R = 128      # PCLIP_EMBED_BWD_CHUNK (test_entry_points_are_declared_and_exported pins it to the header and the binding)


def test_restatements_match_float64_autograd():
    g = torch.Generator().manual_seed(1)
    B, L, V, W = 5, 9, 23, 8
    tokens = torch.randint(0, V, (B, L), generator=g)
    tokens[:, 5:] = 0
    E = torch.randn(V, W, generator=g, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(L, W, generator=g, dtype=torch.float64, requires_grad=True)
    dx = torch.randn(B * L, W, generator=g).half()
    x = torch.nn.functional.embedding(tokens, E) + pos
    (x.reshape(B * L, W) * dx.double()).sum().backward()
    dE, dpos = ref.text_embed_backward64(dx, tokens, V)
    assert torch.allclose(dE, E.grad, rtol=1e-13, atol=1e-13) and torch.allclose(dpos, pos.grad, rtol=1e-13, atol=1e-13)
    assert not dE[[i for i in range(V) if i not in set(tokens.reshape(-1).tolist())]].any()

    cls = torch.randn(W, generator=g, dtype=torch.float64, requires_grad=True)
    patch = torch.randn(B, L - 1, W, generator=g, dtype=torch.float64, requires_grad=True)
    vpos = torch.randn(L, W, generator=g, dtype=torch.float64, requires_grad=True)
    t = torch.cat([cls.expand(B, 1, W), patch], dim=1) + vpos
    (t.reshape(B * L, W) * dx.double()).sum().backward()
    dcls, dvpos, dpatch = ref.vit_embed_backward64(dx, B, L)
    assert torch.allclose(dcls, cls.grad, rtol=1e-13, atol=1e-13) and torch.allclose(dvpos, vpos.grad, rtol=1e-13, atol=1e-13)
    assert torch.equal(dpatch, patch.grad.reshape(B * (L - 1), W)) and torch.equal(dcls, dvpos[0])


@pytest.mark.parametrize("name", ref.TEXT_CASES)
def test_emulated_summation_order_stays_inside_the_tolerance(name):
    dx, tokens, V = ref.text_case(name, R)
    B, L = tokens.shape
    dE64, dpos64 = ref.text_embed_backward64(dx, tokens, V)
    tol = ref.tol_text_dE(dx, tokens, V, R)
    got = ref.emulate_text_dE(dx, tokens, V, R)
    ratio = ref.worst_ratio(got, dE64, tol)
    rpos = ref.worst_ratio(ref.emulate_pos_sum(dx, B, L), dpos64, ref.tol_pos_sum(dx, B, L))
    print(f"{name}: dE at {ratio:.3f} of the bound, dpos at {rpos:.3f}")
    assert ratio <= 1.0 and rpos <= 1.0
    absent = torch.bincount(tokens.reshape(-1), minlength=V) == 0
    assert not got[absent].any() and not tol[absent].any()
    # rounded once to fp16 (a parameter held in fp16): half an fp16 ulp more
    assert ref.worst_ratio(got.half(), dE64, tol + torch.where(absent[:, None], torch.zeros_like(tol), ref.tol_f16(dE64))) <= 1.0


@pytest.mark.parametrize("name", ref.CROSSING_CASES)
@pytest.mark.parametrize("variant", ["drop_tail", "double_boundary"])
def test_tolerance_rejects_a_wrong_walk(name, variant):
    dx, tokens, V = ref.text_case(name, R)
    dE64, _ = ref.text_embed_backward64(dx, tokens, V)
    ratio = ref.worst_ratio(ref.emulate_text_dE(dx, tokens, V, R, variant=variant), dE64, ref.tol_text_dE(dx, tokens, V, R))
    print(f"{name} {variant}: {ratio:.3g} x the bound")
    assert ratio > 1.0


@pytest.mark.parametrize("B,L,W", ref.VIT_CASES)
def test_emulated_position_sums_stay_inside_the_tolerance(B, L, W):
    dt = ref.synth_dx(B * L, W, 20 + B)
    _, dpos64, _ = ref.vit_embed_backward64(dt, B, L)
    tol = ref.tol_pos_sum(dt, B, L)
    got = ref.emulate_pos_sum(dt, B, L)
    assert ref.worst_ratio(got, dpos64, tol) <= 1.0
    if B > 1:                                                       # a sum that drops the last sequence is outside
        assert ref.worst_ratio(ref.emulate_pos_sum(dt[:(B - 1) * L], B - 1, L), dpos64, tol) > 1.0


def test_entry_points_are_declared_and_exported():
    from proto_clip_amd import ops
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ("pclip_text_embed_backward", "pclip_vit_embed_backward_f16"):
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert f"#define PCLIP_EMBED_BWD_CHUNK {R}\n" in header and ops.EMBED_BWD_CHUNK == _lib.EMBED_BWD_CHUNK == R
    assert "clip/model.py:342-344" in header and "clip/model.py:222-227" in header


VIS_PREFIX = {"visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight", "visual.ln_pre.bias"}
TXT_PREFIX = {"token_embedding.weight", "positional_embedding"}


@pytest.mark.parametrize("stem,want", [(False, set()), (True, VIS_PREFIX | TXT_PREFIX), ("visual", VIS_PREFIX), ("text", TXT_PREFIX)])
def test_unfreeze_stem_marks_returns_and_records(stem, want):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    model = build_model(random_state_dict(seed=3, **SMALL))
    params = model.unfreeze(visual_blocks=1, text_blocks=0, heads=True, stem=stem)
    named = {n for n, p in model.named_parameters() if p.requires_grad}
    tail = {n for n, _ in model.named_parameters() if n.startswith(("visual.transformer.resblocks.2.", "visual.ln_post.", "ln_final."))
            or n in ("visual.proj", "text_projection")}
    assert named == tail | want and len(params) == len(named) and all(p.requires_grad for p in params)
    assert {id(p) for p in params} == {id(p) for n, p in model.named_parameters() if n in named}
    assert model.visual._stem_opt_in == bool(want & VIS_PREFIX) and model._text_stem_opt_in == bool(want & TXT_PREFIX)
    # the plan of the taped passes: the whole tower where a stem trains, the tail elsewhere
    assert model.visual._tape_plan() == ((0, True) if want & VIS_PREFIX else (2, False))
    assert model._text_tape_plan() == ((0, True) if want & TXT_PREFIX else (3, False))
    # _tape_from / _text_tape_from keep refusing a trainable prefix, opted in or not (coop.PromptLearner relies on it)
    if want & VIS_PREFIX:
        with pytest.raises(PclipError, match=r"visual\.conv1\.weight"):
            model.visual._tape_from()
    else:
        assert model.visual._tape_from() == 2
    if want & TXT_PREFIX:
        with pytest.raises(PclipError, match=r"token_embedding\.weight"):
            model._text_tape_from()
    else:
        assert model._text_tape_from() == 3
    # freezing everything again leaves a frozen model, opt-in or not
    for p in model.parameters():
        p.requires_grad_(False)
    assert model.visual._tape_plan() == (None, False) and model._text_tape_plan() == (None, False)


def test_unfreeze_stem_refusals_and_the_bare_flag():
    from spec import RESNET
    from proto_clip_amd.clip.model import build_model, random_state_dict
    model = build_model(random_state_dict(seed=3, **SMALL))
    with pytest.raises(PclipError, match="stem='both'"):
        model.unfreeze(stem="both")
    model.unfreeze(stem="text")                                      # the visual prefix was not opted in: a bare flag there is still refused
    model.visual.ln_pre.bias.requires_grad_(True)
    with pytest.raises(PclipError, match=r"visual\.ln_pre\.bias"):
        model.visual._tape_plan()
    rn = build_model(random_state_dict(seed=3, **RESNET))
    for stem in (True, "visual"):
        with pytest.raises(PclipError, match="ModifiedResNet visual tower"):
            rn.unfreeze(stem=stem)
    assert not any(p.requires_grad for p in rn.parameters())
    params = rn.unfreeze(heads=False, stem="text")
    assert len(params) == 2 and rn._text_stem_opt_in and rn._text_tape_plan() == (0, True)
