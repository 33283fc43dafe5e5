"""Visual prompt tuning without a GPU: the three entry points and their refusals (every one fires before a launch), the CPU emulation of the gradient's
documented summation order (tests/vpt_ref.py) against float64 under the tolerance derived from that order, three wrong walks that the tolerance catches, the
host-side refusals of proto_clip_amd.vpt, and the committed fixtures.  tests/test_gpu_vpt.py compares the kernels with the emulation bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vpt_ref
from conftest import GOLDEN, REPO
from spec import RESNET, TINY

from proto_clip_amd import _lib, vpt
from proto_clip_amd._lib import PclipError
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ("pclip_vpt_append_f16", "pclip_vpt_replace_f16", "pclip_vpt_grad_f32"):
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert f"#define PCLIP_VPT_SLICE {_lib.VPT_SLICE}\n" in header and vpt_ref.SLICE == _lib.VPT_SLICE
    assert f"#define PCLIP_VPT_MAX_L {_lib.VPT_MAX_L}\n" in header and vpt_ref.MAX_L == _lib.VPT_MAX_L == 288


# ---- refusals of the C entry points: host memory stands in for the operands, no call gets as far as a launch ---------------------------------------------

@pytest.fixture(scope="module")
def host():
    buf = ctypes.create_string_buffer(4096 + 16)
    base = (ctypes.addressof(buf) + 15) & ~15
    return buf, base


def _err(rc):
    assert rc != 0
    return _lib.load().pclip_last_error().decode()


def _calls(lib, a):
    """name -> call(B, L0, P, W, ptr overrides): the three entries on one host buffer."""
    P_ = ctypes.c_void_p

    def append(B, L0, P, W, t=a, c=a + 1024, o=a + 2048):
        return lib.pclip_vpt_append_f16(P_(t) if t else None, P_(c) if c else None, B, L0, P, W, P_(o) if o else None, None)

    def replace(B, L0, P, W, x=a, c=a + 1024):
        return lib.pclip_vpt_replace_f16(P_(x) if x else None, P_(c) if c else None, B, L0, P, W, None)

    def grad(B, L0, P, W, g=a, d=a + 1024, part=a + 2048, clear=0):
        return lib.pclip_vpt_grad_f32(P_(g) if g else None, B, L0, P, W, clear, P_(d) if d else None, P_(part) if part else None, (B + 15) // 16, None)

    return {"pclip_vpt_append_f16": append, "pclip_vpt_replace_f16": replace, "pclip_vpt_grad_f32": grad}


def test_every_refusal_fires_before_a_launch(host):
    _, a = host
    lib = _lib.load()
    for name, call in _calls(lib, a).items():
        first, second = ("t", "c") if "append" in name else ("x", "c") if "replace" in name else ("g", "d")
        assert _err(call(2, 17, 4, 64, **{first: 0})) == f"{name}: null pointer"
        assert _err(call(2, 17, 4, 64, **{second: 0})) == f"{name}: null pointer"
        assert _err(call(2, 17, 4, 64, **{first: a + 8})) == f"{name}: operands must be 16-byte aligned"
        assert _err(call(2, 17, 4, 64, **{second: a + 1024 + 4})) == f"{name}: operands must be 16-byte aligned"
        for W in (0, 4, 68, -8):
            assert f"{name}: W={W} must be a positive multiple of 8" in _err(call(2, 17, 4, W))
        assert f"{name}: bad shape B=2 L0=17 P=0" in _err(call(2, 17, 0, 64))
        assert f"{name}: bad shape B=2 L0=-1 P=4" in _err(call(2, -1, 4, 64))
        assert f"{name}: bad shape B=-1 L0=17 P=4" in _err(call(-1, 17, 4, 64))
        assert f"{name}: L0 + P = 257 + 32 = 289 tokens exceed the attention envelope of 288" in _err(call(2, 257, 32, 64))
        assert f"{name}: L0 + P = 2147483647 + 1 = 2147483648 tokens" in _err(call(2, 2 ** 31 - 1, 1, 64))
        assert f"{name}: B * (L0 + P) * W = 100000 * 288 * 768 does not fit an int" in _err(call(100000, 257, 31, 768))
        assert call(0, 17, 4, 64) == 0                                          # B == 0: nothing to do, nothing touched
    out = _calls(lib, a)
    assert _err(out["pclip_vpt_append_f16"](2, 17, 4, 64, o=0)) == "pclip_vpt_append_f16: null pointer"
    assert out["pclip_vpt_append_f16"](0, 0, 4, 64, t=0) == 0                   # L0 == 0: no stem rows, t may be NULL
    P_ = ctypes.c_void_p
    assert "nslice=3, expected ceil(B / 16) = 2" in _err(lib.pclip_vpt_grad_f32(P_(a), 17, 0, 4, 64, 0, P_(a + 1024), P_(a + 2048), 3, None))
    assert "2 image slices need the part buffer" in _err(lib.pclip_vpt_grad_f32(P_(a), 17, 0, 4, 64, 0, P_(a + 1024), None, 2, None))
    assert "operands must be 16-byte aligned" in _err(lib.pclip_vpt_grad_f32(P_(a), 17, 0, 4, 64, 0, P_(a + 1024), P_(a + 2048 + 8), 2, None))


# ---- the summation order -----------------------------------------------------------------------------------------------------------------------------

def adversarial(kind, B, L0, P, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = vpt_ref.synth_g(B, L0 + P, W, seed).reshape(B, L0 + P, W)
    if kind == "cancelling":                                                 # large rows that cancel in pairs beside small ones
        big = (torch.randn(P, W, generator=g) * 3000).half()
        for b in range(0, B - 1, 2):
            x[b, L0:] += big
            x[b + 1, L0:] -= big
    elif kind == "one_huge":                                                 # one image carries nearly the whole sum
        x[B // 2, L0:] = (torch.randn(P, W, generator=g) * 20000).half()
    return x.reshape(B * (L0 + P), W)


@pytest.mark.parametrize("kind", ["spread", "cancelling", "one_huge"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_emulation_stays_inside_the_derived_tolerance(B, kind):
    for L0, P, W in ((0, 3, 8), (5, 2, 16)):
        g16 = adversarial(kind, B, L0, P, W, 10 * B + L0)
        assert bool(torch.isfinite(g16).all())
        got = vpt_ref.emulate_grad(g16, B, L0, P)
        tol = vpt_ref.tol_grad(g16, B, L0, P)
        ratio = vpt_ref.worst_ratio(got, vpt_ref.grad64(g16, B, L0, P), tol)
        assert got.dtype == torch.float32 and got.shape == (P, W) and ratio <= 1.0, ratio
    # the walk written out once more, independently of the helper's loop
    rows = vpt_ref.prompt_rows(g16, B, L0, P).float().numpy()
    parts = []
    for s in range(0, B, 16):
        acc = rows[s].copy()
        for n in range(s + 1, min(B, s + 16)):
            acc = (acc + rows[n]).astype(np.float32)
        parts.append(acc)
    want = parts[0].copy()
    for p in parts[1:]:
        want = (want + p).astype(np.float32)
    assert np.array_equal(got.numpy(), want)


def test_the_order_matters_somewhere():
    B, L0, P, W = 40, 2, 2, 64
    g16 = vpt_ref.synth_g(B, L0 + P, W, 3)
    rows = vpt_ref.prompt_rows(g16, B, L0, P).float().numpy()
    seq = rows[0].copy()
    for n in range(1, B):
        seq = (seq + rows[n]).astype(np.float32)
    assert not np.array_equal(seq, vpt_ref.emulate_grad(g16, B, L0, P).numpy())       # a plain image-order sum gives other bits


@pytest.mark.parametrize("variant", ["drop_last_slice", "double_slice", "clear_first"])
def test_wrong_walks_land_outside_the_tolerance(variant):
    """Inputs chosen so that the part a wrong walk loses or repeats is far above the tolerance: every image's prompt rows are positive, of similar size."""
    B, L0, P, W = 33, 4, 3, 16                                               # three slices, the last of one image
    g = torch.Generator().manual_seed(5)
    g16 = (torch.rand(B * (L0 + P), W, generator=g) + 0.5).half()
    tol = vpt_ref.tol_grad(g16, B, L0, P)
    exact = vpt_ref.grad64(g16, B, L0, P)
    assert vpt_ref.worst_ratio(vpt_ref.emulate_grad(g16, B, L0, P), exact, tol) <= 1.0
    wrong = vpt_ref.emulate_grad(g16, B, L0, P, variant=variant)
    err = (wrong.double() - exact).abs()
    assert bool((err > tol).all()), variant                                  # every element is off, by at least one image's term (>= 0.5)
    assert float((err / tol).min()) > 1e3


# ---- host logic --------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_model():
    return build_model(random_state_dict(seed=3, **TINY))


def test_learner_holds_one_seeded_fp32_parameter(tiny_model):
    pl = vpt.VisualPromptLearner(tiny_model, n_ctx=4, depth=2)
    assert pl.ctx.shape == (2, 4, TINY["vision_width"]) and pl.ctx.dtype == torch.float32 and pl.ctx.requires_grad
    assert [n for n, _ in pl.named_parameters()] == ["ctx"]                  # the CLIP model is referenced, not registered
    assert pl.l0 == 17 and pl.run_length == 21
    assert 0.015 < float(pl.ctx.detach().std()) < 0.025
    assert torch.equal(vpt.VisualPromptLearner(tiny_model, n_ctx=4, depth=2).ctx, pl.ctx)
    assert not torch.equal(vpt.VisualPromptLearner(tiny_model, n_ctx=4, depth=2, seed=2).ctx, pl.ctx)
    assert 0.15 < float(vpt.VisualPromptLearner(tiny_model, n_ctx=8, depth=1, init_std=0.2).ctx.detach().std()) < 0.25
    import proto_clip_amd
    assert proto_clip_amd.vpt is vpt and isinstance(vpt.VPT(tiny_model, pl).learner, vpt.VisualPromptLearner)


def test_host_side_refusals(tiny_model):
    with pytest.raises(PclipError, match="ModifiedResNet"):
        vpt.VisualPromptLearner(build_model(random_state_dict(seed=4, **RESNET)))
    with pytest.raises(PclipError, match=r"L0 \+ n_ctx = 17 \+ 272 = 289 tokens"):
        vpt.VisualPromptLearner(tiny_model, n_ctx=272)
    assert vpt.VisualPromptLearner(tiny_model, n_ctx=271).run_length == 288
    for depth in (0, 3, -1):
        with pytest.raises(PclipError, match=rf"depth={depth} outside 1\.\.2"):
            vpt.VisualPromptLearner(tiny_model, depth=depth)
    with pytest.raises(PclipError, match="n_ctx=0"):
        vpt.VisualPromptLearner(tiny_model, n_ctx=0)
    wide = dict(TINY, vision_width=96)                                       # 96 // 64 = 1 head of 96 columns
    with pytest.raises(PclipError, match="head dimension 64"):
        vpt.VisualPromptLearner(build_model(random_state_dict(seed=5, **wide)))
    pl = vpt.VisualPromptLearner(tiny_model, n_ctx=4, depth=2)
    images = torch.zeros(2, 3, 32, 32)
    with pytest.raises(PclipError, match="float16"):
        pl(images, ctx=pl.ctx.detach().half())
    pl.ctx.data = pl.ctx.data.half()
    with pytest.raises(PclipError, match="float16"):
        pl(images)
    pl.ctx.data = pl.ctx.data.float()
    with pytest.raises(PclipError, match=r"ctx \(1, 4, 128\) is not \[depth, n_ctx, W\]"):
        pl(images, ctx=pl.ctx.detach()[:1])
    with pytest.raises(PclipError, match=r"expected images \[B,3,32,32\]"):
        pl(torch.zeros(2, 3, 64, 64))


def test_stem_opt_in_and_trainable_prefix_are_refused():
    model = build_model(random_state_dict(seed=6, **TINY))
    pl = vpt.VisualPromptLearner(model, n_ctx=2)
    images = torch.zeros(2, 3, 32, 32)
    model.visual.positional_embedding.requires_grad_(True)                   # no opt-in: the tower's own refusal
    with pytest.raises(PclipError, match=r"visual\.positional_embedding"):
        pl(images)
    model.visual.positional_embedding.requires_grad_(False)
    model.unfreeze(visual_blocks=0, heads=False, stem="visual")
    with pytest.raises(PclipError, match=r"unfreeze\(stem=\.\.\.\)"):
        pl(images)
    with torch.no_grad(), pytest.raises(PclipError, match=r"unfreeze\(stem=\.\.\.\)"):
        pl(images)


def test_token_budget_of_the_released_backbones():
    """INTEGRATION's table: the prompt rows a backbone has room for.  (Towers are not built: the arithmetic of the constructor's check.)"""
    room = {}
    for name, kw in BACKBONES.items():
        if isinstance(kw["vision_layers"], (tuple, list)):
            continue
        room[name] = 288 - ((kw["image_resolution"] // kw["vision_patch_size"]) ** 2 + 1)
    assert room["ViT-B/16"] == 91 and room["ViT-B/32"] == 238 and room["ViT-L/14"] == 31
    assert all(v < 0 for k, v in room.items() if "336" in k)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(vpt_ref.FIXTURES))
def test_committed_fixture_carries_what_the_gpu_test_reads(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.exists(path) and os.path.getsize(path) < 1 << 20
    meta = np.load(path, allow_pickle=False)
    tag, sd_seed, B, P, depth, N, seed = vpt_ref.FIXTURES[name]
    kw = vpt_ref.towers()[tag]
    assert (str(meta["tag"]), int(meta["sd_seed"]), int(meta["B"]), int(meta["P"]), int(meta["depth"]), int(meta["N"]), int(meta["seed"])) == vpt_ref.FIXTURES[name]
    assert 3 <= B <= 6 and float(meta["floor"]) == 0.0
    assert meta["g_f64"].shape == (depth, P, kw["vision_width"]) and meta["feat_f64"].shape == (B, kw["embed_dim"])
    assert meta["e_ref"].shape == (depth,) and bool((meta["e_ref"] > 0).all()) and bool(np.isfinite(meta["e_ref"]).all())
    assert 0 < float(meta["feat_e_ref"]) < 1e-2 and float(meta["e_ref"].max()) < 1e-2
    assert np.isfinite(float(meta["loss_f64"])) and np.isfinite(float(meta["loss_f16"]))
    assert float(meta["logit_scale"]) == float(np.float32(vpt_ref.LOGIT_SCALE))
    L0 = (kw["image_resolution"] // kw["vision_patch_size"]) ** 2 + 1
    assert L0 + P <= 288
    if tag == "long":
        assert (L0, L0 + P) == (257, 288)
