"""Whole-tower fine-tuning: the backward of the stages in front of block 0 (csrc/pclip_embed_bwd.hip, autograd.VitStemFn / TextEmbedFn, CLIP.unfreeze(stem=...)).

Kernel level: dE / dpos / dpatch against the float64 restatements of tests/tower_prefix_ref.py under the tolerances derived there from the rounding points,
bit for bit against the fp32 emulation of the documented summation order, run-to-run bits, NaN containment, the envelope.
Model level: taped features keep the untaped bits; every parameter gradient of a whole-model backward (prefix, blocks, heads) against the reference's own
float64 autograd at twice the reference's fp16-chain distance e_ref (fixtures of tests/golden/make_golden_prefix_grad.py, floor 0); the refusals that
stay; training lowers the loss; an optimizer step leaves no stale cached copy; passes cut into chunks."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import tower_prefix_ref as ref
from conftest import GOLDEN, observe
from spec import ODD, RESNET, SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

TOWERS = {"tiny": TINY, "small": SMALL, "odd": ODD}
VIS_PREFIX = ["visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight", "visual.ln_pre.bias"]
TXT_PREFIX = ["token_embedding.weight", "positional_embedding"]
_cases = {}


def chunk_len():
    from proto_clip_amd import ops
    return ops.EMBED_BWD_CHUNK


def text_case(name):
    """Inputs, float64 reference, tolerances and the fp32 emulation of a kernel-level case, computed once and left unchanged."""
    if name not in _cases:
        R = chunk_len()
        dx, tokens, V = ref.text_case(name, R)
        B, L = tokens.shape
        dE64, dpos64 = ref.text_embed_backward64(dx, tokens, V)
        _cases[name] = dict(dx=dx, tokens=tokens, V=V, dE64=dE64, dpos64=dpos64, tol_E=ref.tol_text_dE(dx, tokens, V, R), tol_pos=ref.tol_pos_sum(dx, B, L),
                            emu_E=ref.emulate_text_dE(dx, tokens, V, R), emu_pos=ref.emulate_pos_sum(dx, B, L))
    return _cases[name]


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ref.TEXT_CASES)
def test_text_embed_backward_against_float64(name):
    from proto_clip_amd import ops
    c = text_case(name)
    dE, dpos = ops.text_embed_backward(c["dx"].cuda(), c["tokens"].cuda(), c["V"])
    assert dE.dtype == dpos.dtype == torch.float32 and dE.shape == c["dE64"].shape and dpos.shape == c["dpos64"].shape
    dE, dpos = dE.cpu(), dpos.cpu()
    rE, rpos = ref.worst_ratio(dE, c["dE64"], c["tol_E"]), ref.worst_ratio(dpos, c["dpos64"], c["tol_pos"])
    print(f"{name}: dE at {rE:.3f} of the bound, dpos at {rpos:.3f}")
    observe("text_embed_backward: worst |dE - dE64| / tol", rE, 1.0)
    observe("text_embed_backward: worst |dpos - dpos64| / tol", rpos, 1.0)
    assert rE <= 1.0 and rpos <= 1.0
    absent = torch.bincount(c["tokens"].reshape(-1), minlength=c["V"]) == 0
    assert not dE[absent].any()                                             # every untouched row exactly zero
    assert torch.equal(dE, c["emu_E"]) and torch.equal(dpos, c["emu_pos"])  # the documented order of additions, bit for bit


def test_text_embed_backward_partial_requests():
    from proto_clip_amd import ops
    c = text_case("prompts")
    dx, tokens = c["dx"].cuda(), c["tokens"].cuda()
    dE, none = ops.text_embed_backward(dx, tokens, c["V"], want_pos=False)
    none2, dpos = ops.text_embed_backward(dx, tokens, c["V"], want_emb=False)
    assert none is None and none2 is None and torch.equal(dE.cpu(), c["emu_E"]) and torch.equal(dpos.cpu(), c["emu_pos"])
    # ids outside the vocabulary count for its ends, as the forward's clamp reads them
    wild = c["tokens"].clone()
    wild[0, 70], wild[1, 71] = -5, c["V"] + 40
    want, _ = ref.text_embed_backward64(c["dx"], wild, c["V"])
    got, _ = ops.text_embed_backward(dx, wild.cuda(), c["V"])
    assert ref.worst_ratio(got.cpu(), want, ref.tol_text_dE(c["dx"], wild, c["V"], chunk_len())) <= 1.0


@pytest.mark.parametrize("B,L,W", ref.VIT_CASES)
def test_vit_embed_backward_against_float64(B, L, W):
    from proto_clip_amd import ops
    dt = ref.synth_dx(B * L, W, 20 + B)
    _, dpos64, _ = ref.vit_embed_backward64(dt, B, L)
    dpos, dpatch = ops.vit_embed_backward(dt.cuda(), B, L)
    assert dpos.dtype == torch.float32 and dpos.shape == (L, W) and dpatch.dtype == torch.float16 and dpatch.shape == (B * (L - 1), W)
    assert torch.equal(dpatch.cpu(), dt.reshape(B, L, W)[:, 1:].reshape(B * (L - 1), W))           # bit-exact copies of the non-class rows
    r = ref.worst_ratio(dpos.cpu(), dpos64, ref.tol_pos_sum(dt, B, L))
    observe("vit_embed_backward: worst |dpos - dpos64| / tol", r, 1.0)
    assert r <= 1.0
    assert torch.equal(dpos.cpu(), ref.emulate_pos_sum(dt, B, L))
    only_pos, none = ops.vit_embed_backward(dt.cuda(), B, L, want_patch=False)
    none2, only_patch = ops.vit_embed_backward(dt.cuda(), B, L, want_pos=False)
    assert none is None and none2 is None and torch.equal(only_pos, dpos) and torch.equal(only_patch, dpatch)


def test_two_runs_give_the_same_bits():
    from proto_clip_amd import ops
    for name in ("prompts", "one_id", "straddles_boundaries"):
        c = text_case(name)
        dx, tokens = c["dx"].cuda(), c["tokens"].cuda()
        a, b = ops.text_embed_backward(dx, tokens, c["V"]), ops.text_embed_backward(dx, tokens, c["V"])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    dt = ref.synth_dx(70 * 17, 128, 90).cuda()
    a, b = ops.vit_embed_backward(dt, 70, 17), ops.vit_embed_backward(dt, 70, 17)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_nan_row_stays_in_its_own_rows():
    from proto_clip_amd import ops
    c = text_case("prompts")
    B, L = c["tokens"].shape
    b, l = 1, 2                                                             # a body token of the second prompt
    tid = int(c["tokens"][b, l])
    dx = c["dx"].clone()
    dx[b * L + l] = float("nan")
    dE, dpos = (t.cpu() for t in ops.text_embed_backward(dx.cuda(), c["tokens"].cuda(), c["V"]))
    others = torch.arange(c["V"]) != tid
    assert bool(torch.isnan(dE[tid]).all()) and torch.equal(dE[others], c["emu_E"][others])
    rest = torch.arange(L) != l
    assert bool(torch.isnan(dpos[l]).all()) and torch.equal(dpos[rest], c["emu_pos"][rest])
    Bv, Lv, W = 6, 17, 128
    dt = ref.synth_dx(Bv * Lv, W, 91)
    clean = ref.emulate_pos_sum(dt, Bv, Lv)
    dt[2 * Lv + 5] = float("nan")
    dpos, dpatch = (t.cpu() for t in ops.vit_embed_backward(dt.cuda(), Bv, Lv))
    rest = torch.arange(Lv) != 5
    assert bool(torch.isnan(dpos[5]).all()) and torch.equal(dpos[rest], clean[rest])
    assert int(torch.isnan(dpatch).any(dim=1).sum()) == 1 and bool(torch.isnan(dpatch[2 * (Lv - 1) + 4]).all())


@pytest.mark.parametrize("W", [96, 2112])
def test_envelope_refusals_come_before_a_launch(W):
    from proto_clip_amd import _lib, ops
    from proto_clip_amd._lib import PclipError
    dx = torch.zeros(2 * 5, W, dtype=torch.float16, device="cuda")
    tokens = torch.zeros(2, 5, dtype=torch.int64, device="cuda")
    with pytest.raises(PclipError, match=f"W={W} outside the envelope"):
        ops.text_embed_backward(dx, tokens, 16)
    with pytest.raises(PclipError, match=f"W={W} outside the envelope"):
        ops.vit_embed_backward(dx, 2, 5)
    # the C entry points refuse the same shapes themselves (no launch: the pointers are never read)
    lib = _lib.load()
    dpos = torch.zeros(5, W, dtype=torch.float32, device="cuda")
    assert lib.pclip_vit_embed_backward_f16(_lib.ptr(dx), 2, 5, W, _lib.ptr(dpos), None, _lib.stream()) != 0
    assert lib.pclip_text_embed_backward(_lib.ptr(dx), None, None, 2, 5, W, 16, None, _lib.ptr(dpos), None, _lib.stream()) != 0
    assert lib.pclip_vit_embed_backward_f16(_lib.ptr(dx), 2, 4097, 128, _lib.ptr(dpos), None, _lib.stream()) != 0


# ---- model ----------------------------------------------------------------------------------------------------------------------------------------------

def tokens(n, vocab, seed):
    return ref.synth_prompts(n, vocab, seed)


def make_model(kw, seed, trained=True):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    sd = random_state_dict(seed=seed, **kw)
    if trained:
        sd = trained_like_(sd, seed)
    sd["logit_scale"] = torch.tensor(math.log(20.0), dtype=torch.float32)
    return build_model(sd).cuda()


def unfreeze_all(model, kw):
    return model.unfreeze(visual_blocks=kw["vision_layers"], text_blocks=kw["transformer_layers"], stem=True)


def load_fixture(tag):
    paths = sorted(glob.glob(os.path.join(GOLDEN, f"tower_prefix_grad_{tag}_p*.npz")))
    parts = [np.load(p, allow_pickle=False) for p in paths]
    meta = next(p for p in parts if "n_parts" in p.files)
    assert int(meta["n_parts"]) == len(parts)
    slabs = {}
    for part in parts:
        for k in part.files:
            if k.startswith("g__"):
                name, _, s = k[3:].partition("__s")
                slabs.setdefault(name, {})[int(s) if s else 0] = torch.from_numpy(part[k])
    grads = {name: torch.cat([d[i] for i in sorted(d)], dim=0) if len(d) > 1 else d[0] for name, d in slabs.items()}
    return meta, grads


def contrastive64(fi, ft, logit_scale):
    """The generator's loss: float64 torch on the features."""
    fi, ft = fi.double(), ft.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    logits = math.exp(float(np.float32(logit_scale))) * fi @ ft.t()
    tgt = torch.arange(fi.shape[0], device=fi.device)
    ce = torch.nn.functional.cross_entropy
    return 0.5 * (ce(logits, tgt) + ce(logits.t(), tgt))


@pytest.mark.parametrize("tag", list(TOWERS))
def test_taped_features_keep_the_untaped_bits(tag):
    from proto_clip_amd import synth
    kw, n = TOWERS[tag], 4
    model = make_model(kw, 9)
    imgs = synth.make_images(n, kw["image_resolution"], seed=6, n_class=n).cuda()
    toks = tokens(n, kw["vocab_size"], 7).cuda()
    with torch.no_grad():
        fi0, ft0 = model.encode_image(imgs), model.encode_text(toks)
    for blocks, stem in ((0, True), (1, "visual"), (1, "text"), (None, True)):       # stem beside frozen blocks; one tower's stem; everything
        for p in model.parameters():
            p.requires_grad_(False)
        model.visual._stem_opt_in = model._text_stem_opt_in = False
        if blocks is None:
            unfreeze_all(model, kw)
        else:
            model.unfreeze(visual_blocks=blocks, text_blocks=blocks, stem=stem)
        fi, ft = model.encode_image(imgs), model.encode_text(toks)
        assert fi.requires_grad and ft.requires_grad and fi.dtype == ft.dtype == torch.float16
        assert torch.equal(fi.detach(), fi0) and torch.equal(ft.detach(), ft0), (blocks, stem)


@pytest.mark.parametrize("tag,chunk", [("tiny", None), ("small", None), ("odd", None), ("small", 3)])
def test_whole_model_gradients_against_the_reference(tag, chunk):
    """Per parameter tensor — the prefix, every block, the heads — ||g - g_f64|| / ||g_f64|| <= 2 e_ref (e_ref: the reference's own fp16 chain against its
    float64 run; the fixtures record floor 0).  chunk = 3: the 8 images / prompts run as passes of 3 + 3 + 2, each its own Function call, and autograd
    adds the parameter gradients: the same bound."""
    from proto_clip_amd import synth
    from proto_clip_amd.clip.model import build_model, random_state_dict
    meta, g64 = load_fixture(tag)
    kw, sd_seed, n = TOWERS[tag], int(meta["sd_seed"]), int(meta["n"])
    floor = float(meta["floor"])
    assert floor == 0.0
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(float(meta["logit_scale"]), dtype=torch.float32)
    model = build_model(sd).cuda()
    if chunk is not None:
        model.visual.chunk = model.text_chunk = chunk
    imgs = synth.make_images(n, kw["image_resolution"], seed=int(meta["image_seed"]), n_class=n).cuda()
    toks = torch.from_numpy(meta["tokens"]).cuda()
    params = unfreeze_all(model, kw)
    loss = contrastive64(model.encode_image(imgs), model.encode_text(toks), float(meta["logit_scale"]))
    assert abs(float(loss.detach()) - float(meta["loss_f64"])) <= 2 * abs(float(meta["loss_f16"]) - float(meta["loss_f64"])) + 1e-4
    loss.backward()
    named = {name: p for name, p in model.named_parameters() if p.requires_grad}
    assert sorted(named) == sorted(g64) == sorted(str(s) for s in meta["names"]) and len(params) == len(named)
    assert "logit_scale" not in named and all(k in named for k in VIS_PREFIX + TXT_PREFIX)
    e_ref = {str(k): float(e) for k, e in zip(meta["names"], meta["e_ref"])}
    ids = torch.from_numpy(meta["rows__token_embedding.weight"])
    worst, worst_prefix = 0.0, 0.0
    for name in sorted(named):
        p = named[name]
        assert p.grad is not None and p.grad.dtype == p.dtype and p.grad.shape == p.shape, name
        g = p.grad.double().cpu()
        if name == "token_embedding.weight":                               # the fixture stores the rows that occur; every other row is exactly zero
            rest = torch.ones(g.shape[0], dtype=torch.bool)
            rest[ids] = False
            assert not g[rest].any()
            g = g[ids]
        want = g64[name].double()
        rel = float((g - want).norm() / want.norm())
        ratio = rel / max(2 * e_ref[name], floor)
        print(f"{tag} chunk {chunk} {name:<58s} rel {rel:.3e}  e_ref {e_ref[name]:.3e}  ratio {ratio:.3f}")
        worst = max(worst, ratio)
        if name in VIS_PREFIX + TXT_PREFIX:
            worst_prefix = max(worst_prefix, ratio)
    observe(f"tower prefix {tag} chunk {chunk}: worst ||g - g64|| / ||g64|| / (2 e_ref), prefix parameters", worst_prefix, 1.0)
    observe(f"tower prefix {tag} chunk {chunk}: worst ||g - g64|| / ||g64|| / (2 e_ref), every parameter", worst, 1.0)
    assert worst <= 1.0, worst


def test_a_parameter_held_in_fp16_gets_one_rounding_of_the_fp32_gradient():
    from proto_clip_amd import synth
    kw, n = TINY, 4
    imgs = synth.make_images(n, kw["image_resolution"], seed=6, n_class=n).cuda()
    toks = tokens(n, kw["vocab_size"], 7).cuda()
    grads = []
    for half in (False, True):
        model = make_model(kw, 9)
        if half:                                                            # fp16 copies of the fp32 tables: the forward reads the same fp16 values either way
            for name in ("visual.class_embedding", "visual.positional_embedding", "token_embedding.weight", "positional_embedding"):
                p = dict(model.named_parameters())[name]
                p.data = p.data.half()
        unfreeze_all(model, kw)
        model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks)).backward()
        grads.append({k: v.grad for k, v in model.named_parameters() if k in VIS_PREFIX + TXT_PREFIX})
    for name in ("visual.class_embedding", "visual.positional_embedding", "token_embedding.weight", "positional_embedding"):
        assert grads[0][name].dtype == torch.float32 and grads[1][name].dtype == torch.float16
        assert torch.equal(grads[1][name], grads[0][name].half()), name
    assert torch.equal(grads[0]["visual.class_embedding"], grads[0]["visual.positional_embedding"][0])       # dcls is row 0 of dpos


def test_refusals_that_stay():
    from proto_clip_amd import coop, ops, synth
    from proto_clip_amd._lib import PclipError
    model = make_model(TINY, 5)
    imgs = synth.make_images(2, TINY["image_resolution"], seed=3, n_class=2).cuda()
    toks = tokens(2, TINY["vocab_size"], 4).cuda()
    # a bare requires_grad_(True) on a prefix parameter, without the opt-in (also: with the OTHER tower's opt-in)
    model.visual.class_embedding.requires_grad_(True)
    with pytest.raises(PclipError, match=r"visual\.class_embedding"):
        model.encode_image(imgs)
    model.unfreeze(heads=False, stem="text")
    with pytest.raises(PclipError, match=r"visual\.class_embedding"):
        model.encode_image(imgs)
    model.visual.class_embedding.requires_grad_(False)
    assert model.encode_text(toks).requires_grad
    # CoOp on a tower whose embeddings train
    with pytest.raises(PclipError, match=r"token_embedding\.weight"):
        coop.PromptLearner(["cat", "dog"], model, n_ctx=2, tokenized_prompts=torch.tensor([[510, 7, 7, 9, 511] + [0] * 72, [510, 7, 7, 8, 511] + [0] * 72]))()
    # a taped pass inside ops.low_latency()
    model.unfreeze(stem=True)
    with ops.low_latency():
        with pytest.raises(PclipError, match="low_latency"):
            model.encode_image(imgs)
        with pytest.raises(PclipError, match="low_latency"):
            model.encode_text(toks)
    # the ModifiedResNet tower: no visual stem, the text embeddings beside it train
    rn = make_model(RESNET, 5, trained=False)
    with pytest.raises(PclipError, match="ModifiedResNet visual tower"):
        rn.unfreeze(stem="visual")
    params = rn.unfreeze(text_blocks=1, stem="text")
    rtoks = tokens(3, RESNET["vocab_size"], 4).cuda()
    fi = rn.encode_image(synth.make_images(3, RESNET["image_resolution"], seed=3, n_class=3).cuda())
    ft = rn.encode_text(rtoks)
    assert not fi.requires_grad and ft.requires_grad
    rn.contrastive_loss(fi, ft).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in params)
    assert rn.token_embedding.weight.grad.shape == rn.token_embedding.weight.shape
    # sequences beyond the attention backward's envelope
    long = make_model(dict(embed_dim=64, image_resolution=336, vision_layers=1, vision_width=128, vision_patch_size=14, context_length=77, vocab_size=300,
                           transformer_width=64, transformer_heads=1, transformer_layers=1), 5, trained=False)
    long.unfreeze(visual_blocks=1, stem="visual")
    with pytest.raises(PclipError, match="L=577"):
        long.encode_image(synth.make_images(1, 336, seed=3, n_class=1).cuda())


def test_sgd_on_everything_lowers_the_loss():
    """lr = 0.1: the reference in fp32 on the CPU, same towers and step rule, descends 2.079 -> 1.986 monotonically in five steps at this rate (and
    overshoots at 0.3 on the sixth), a decrease a hundred times the fp16 noise of the features."""
    from proto_clip_amd import synth
    model = make_model(SMALL, 6)
    imgs = synth.make_images(8, SMALL["image_resolution"], seed=8, n_class=8).cuda()
    toks = tokens(8, SMALL["vocab_size"], 9).cuda()
    opt = torch.optim.SGD(unfreeze_all(model, SMALL), lr=0.1)
    before = {k: dict(model.named_parameters())[k].detach().clone() for k in VIS_PREFIX + TXT_PREFIX}
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))))
    print("contrastive loss over five SGD steps on everything:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    for k, v in before.items():                                             # the first layers move
        assert not torch.equal(dict(model.named_parameters())[k].detach(), v), k


def test_an_optimizer_step_leaves_no_stale_cached_copy():
    from proto_clip_amd import synth
    from proto_clip_amd.clip.model import build_model
    from proto_clip_amd.optim import TowerAdamW
    model = make_model(SMALL, 6)
    imgs = synth.make_images(8, SMALL["image_resolution"], seed=8, n_class=8).cuda()
    toks = tokens(8, SMALL["vocab_size"], 9).cuda()
    with torch.no_grad():
        fi0, ft0 = model.encode_image(imgs), model.encode_text(toks)                 # fills the cached conv1 / cls / pos / tok copies
    opt = TowerAdamW(unfreeze_all(model, SMALL), lr=1e-3, loss_scale=1024.0)
    opt.scale_loss(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))).backward()
    opt.step()
    assert int(opt.found_inf) == 0
    fresh = build_model({k: v.detach().clone() for k, v in model.state_dict().items()}).cuda()
    with torch.no_grad():
        fi1, ft1 = model.encode_image(imgs), model.encode_text(toks)
        fi2, ft2 = fresh.encode_image(imgs), fresh.encode_text(toks)
    assert not torch.equal(fi1, fi0) and not torch.equal(ft1, ft0)
    assert torch.equal(fi1, fi2) and torch.equal(ft1, ft2)
    fresh_params = unfreeze_all(fresh, SMALL)                                        # ... and the taped pass reads the fresh copies too
    assert torch.equal(model.encode_image(imgs).detach(), fi2) and torch.equal(model.encode_text(toks).detach(), ft2)
    assert len(fresh_params) == len(opt._params)
