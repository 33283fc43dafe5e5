"""CoCoOp without a device: the CPU emulations of csrc/pclip_cocoop.hip's documented orders (tests/cocoop_ref.py) stay inside their derived tolerances
against float64; the deliberately wrong walks (descending b, a slice length of 8, pi added after the rounding to fp16, the bias added first, a fused
multiply-add) are told apart; the header, the ctypes table and the Makefile agree; the envelope refusals that need no GPU; the learner on a CPU model.

How a wrong walk is told apart.  Four of the five wrong walks only reorder or fuse correctly rounded operations, so they are as close to float64 as the
documented walk (a fused multiply-add is closer): no error bound of the right size can exclude them, and a bound that did would be wrong.  What excludes
them is the bits — tests/test_gpu_cocoop.py compares the kernels with the emulation bit for bit — so this file asserts that each of them gives OTHER bits
than the documented walk on the test inputs, and that each still lies inside the tolerance (the tolerance is not an accident of one order).  The fifth,
pi added after the rounding to fp16, carries an extra fp16 rounding of ctx: where ctx + pi cancels it does leave the derived tolerance, and that is asserted."""
import ctypes
import os
import re

import pytest
import torch

import cocoop_ref as ref
import coop_ref
from conftest import REPO
from spec import RESNET, SMALL, TINY

from proto_clip_amd import _lib
from proto_clip_amd._lib import PclipError

ENTRIES = ("pclip_metanet_fwd_f32", "pclip_metanet_bwd_f32", "pclip_prompt_embed_cond_f16", "pclip_prompt_cond_grad_f32")
SHAPES = [(1, 64, 4, 64), (3, 128, 8, 128), (16, 128, 8, 64), (5, 640, 40, 512)]


# ---- the meta-net ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["decades", "cancel"])
@pytest.mark.parametrize("B,E,Hd,Wt", SHAPES)
def test_metanet_emulation_is_inside_its_tolerance_and_the_wrong_walks_give_other_bits(B, E, Hd, Wt, family):
    f, W1, b1, W2, b2, dpi = ref.synth_metanet(B, E, Hd, Wt, 7 * B + E + Hd, family)
    h, pi = ref.emulate_metanet_fwd(f, W1, b1, W2, b2)
    pre64, h64, pi64 = ref.metanet_fwd64(f, W1, b1, W2, b2)
    tol_h, tol_pi = ref.tol_metanet_fwd(f, W1, b1, W2, b2)
    assert h.dtype == pi.dtype == torch.float32 and h.shape == (B, Hd) and pi.shape == (B, Wt)
    assert bool((pre64 > 0).any()) and bool((pre64 < 0).any())                  # both sides of the ReLU occur
    assert ref.worst_ratio(h, h64, tol_h) <= 1.0 and ref.worst_ratio(pi, pi64, tol_pi) <= 1.0
    for variant in ("bias_first", "fma"):
        hv, piv = ref.emulate_metanet_fwd(f, W1, b1, W2, b2, variant)
        assert not torch.equal(hv, h) or not torch.equal(piv, pi), variant
        assert not torch.equal(piv, pi), variant
        assert ref.worst_ratio(hv, h64, tol_h) <= 1.0 and ref.worst_ratio(piv, pi64, tol_pi) <= 1.0, variant
    grads = ref.emulate_metanet_bwd(dpi, f, h, W2)
    want, tols = ref.metanet_bwd64(dpi, f, h, W2), ref.tol_metanet_bwd(dpi, f, h, W2)
    for got, w, t, shape in zip(grads, want, tols, ((Hd, E), (Hd,), (Wt, Hd), (Wt,))):
        assert got.dtype == torch.float32 and got.shape == shape
        assert ref.worst_ratio(got, w, t) <= 1.0
    for variant in ("descending_b", "fma"):
        if variant == "descending_b" and B < 3:
            continue                                                             # one or two terms: fp32 addition commutes
        gv = ref.emulate_metanet_bwd(dpi, f, h, W2, variant)
        assert any(not torch.equal(a, b) for a, b in zip(gv, grads)), variant
        assert all(ref.worst_ratio(a, w, t) <= 1.0 for a, w, t in zip(gv, want, tols)), variant


def test_a_hidden_unit_at_exactly_zero_gets_no_gradient_and_a_nan_stays_a_nan():
    f, W1, b1, W2, b2, dpi = ref.synth_metanet(3, 64, 4, 64, 5)
    W1[1] = 0.0
    b1[1] = 0.0                                                                  # unit 1: pre = +0 for every image
    b1[2] = -0.0
    W1[2] = 0.0                                                                  # unit 2: pre = -0
    h, pi = ref.emulate_metanet_fwd(f, W1, b1, W2, b2)
    assert not h[:, 1].any() and not h[:, 2].any() and not torch.signbit(h[:, 2]).any()
    dW1, db1, dW2, db2 = ref.emulate_metanet_bwd(dpi, f, h, W2)
    assert not dW1[1].any() and not dW1[2].any() and not db1[1].any() and not db1[2].any() and not dW2[:, 1].any()
    assert bool(dW1[0].any()) or bool(dW1[3].any())
    bad = f.clone()
    bad[1, 3] = float("nan")
    hb, pib = ref.emulate_metanet_fwd(bad, W1, b1, W2, b2)
    assert bool(torch.isnan(hb[1, 0])) and bool(torch.isnan(pib[1]).all())
    assert torch.equal(hb[0], h[0]) and torch.equal(pib[2], pi[2])               # the other images keep their bits


# ---- the conditional assembly and its gradient --------------------------------------------------------------------------------------------------------------------

def _operands(B, N, n_ctx, W, vocab, seed, cancel=False):
    g = torch.Generator().manual_seed(seed)
    emb16 = (torch.randn(vocab, W, generator=g) * 0.02).half()
    pos16 = (torch.randn(77, W, generator=g) * 0.01).half()
    ctx = torch.randn(n_ctx, W, generator=g) * 0.02
    pi = torch.randn(B, W, generator=g) * 0.02
    if cancel:                                                                   # ctx[j] + pi[b] far below its terms in image 0, row 0
        pi[0] = -ctx[0] * (1 + 2.0 ** -9 * torch.randn(W, generator=g))
    return ctx, pi, coop_ref.prompt_tokens(N, n_ctx, vocab, seed + 1), emb16, pos16


@pytest.mark.parametrize("L", [77, 9, 3])
def test_assembly_emulation_is_inside_its_tolerance_and_pi_after_the_rounding_is_not(L):
    B, N, n_ctx, W, vocab = 3, 5, 4, 64, 50
    ctx, pi, tokens, emb16, pos16 = _operands(B, N, n_ctx, W, vocab, 3, cancel=True)
    x = ref.prompt_embed_cond(ctx, pi, tokens, emb16, pos16, L)
    x64, tol = ref.prompt_embed_cond64(ctx, pi, tokens, emb16, pos16, L)
    assert x.dtype == torch.float16 and x.shape == (B * N * L, W)
    assert ref.worst_ratio(x, x64, tol) <= 1.0
    wrong = ref.prompt_embed_cond(ctx, pi, tokens, emb16, pos16, L, "pi_after_r16")
    assert not torch.equal(wrong, x)
    assert ref.worst_ratio(wrong, x64, tol) > 1.0
    # rows: image b's N prompts hold ctx + pi[b]; the token rows are the images' common rows; rows at l >= L do not exist
    xv, k = x.reshape(B, N, L, W), min(n_ctx, L - 1)
    for b in range(B):
        want = ((ctx[:k] + pi[b]).half().float() + pos16[1:1 + k].float()).half()
        assert torch.equal(xv[b, :, 1:1 + k], want.expand(N, k, W))
    assert torch.equal(xv[0, :, 1 + k:], xv[2, :, 1 + k:]) and torch.equal(xv[0, :, 0], xv[1, :, 0])
    # pi = 0: coop's assembly of the shared context, repeated B times
    zero = ref.prompt_embed_cond(ctx, torch.zeros(B, W), tokens, emb16, pos16, L)
    assert torch.equal(zero, coop_ref.prompt_embed(ctx, tokens, emb16, pos16, L).repeat(B, 1))


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("N", [1, 16, 17, 33])
def test_gradient_emulation_is_inside_its_tolerance_and_the_wrong_walks_give_other_bits(B, N):
    W = 64
    for n_ctx, L in ((1, 9), (4, 9), (16, 20), (4, 3)):
        dx = ref.synth_dx(B, N, L, W, 100 * B + N + n_ctx)
        got = ref.emulate_cond_grad(dx, B, N, L, n_ctx)
        want, tols = ref.cond_grad64(dx, B, N, L, n_ctx), ref.tol_cond_grad(dx, B, N, L, n_ctx)
        for g, w, t, shape in zip(got, want, tols, ((n_ctx, W), (B, W), (B, n_ctx, W))):
            assert g.dtype == torch.float32 and g.shape == shape
            assert ref.worst_ratio(g, w, t) <= 1.0
        avail = min(n_ctx, L - 1)
        assert not got[2][:, avail:].any() and not got[0][avail:].any()          # rows with no row in the stream: +0
        # image b's dshift is coop's shared-context gradient of its N prompts
        for b in range(B):
            assert torch.equal(got[2][b], coop_ref.prompt_ctx_grad(dx.reshape(B, N * L, W)[b], N, L, n_ctx, False))
        if B == 1:
            assert torch.equal(got[0], got[2][0])
        if B >= 3 and N >= 16:                                                   # (a few fp16 terms add exactly in fp32, in any order)
            wrong = ref.emulate_cond_grad(dx, B, N, L, n_ctx, "descending_b")
            assert not torch.equal(wrong[0], got[0]) and torch.equal(wrong[2], got[2])
            assert ref.worst_ratio(wrong[0], want[0], tols[0]) <= 1.0
        if N > 16:                                                               # 17 = 16 + 1 against 8 + 8 + 1: other partial sums
            wrong = ref.emulate_cond_grad(dx, B, N, L, n_ctx, "slice8")
            assert not torch.equal(wrong[2], got[2])
            assert ref.worst_ratio(wrong[2], want[2], tols[2]) <= 1.0


# ---- header, ctypes table, Makefile -----------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    makefile = open(os.path.join(REPO, "proto-clip_amd", "csrc", "Makefile")).read()
    source = open(os.path.join(REPO, "proto-clip_amd", "csrc", "pclip_cocoop.hip")).read()
    lib = _lib.load()
    assert re.search(r"^SRCS = .*\bpclip_cocoop\.hip\b", makefile, re.M)
    for name in ENTRIES:
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert len(decl.group(1).split(",")) == len(_lib._SIGS[name]), name     # one ctypes entry per declared argument
        assert f'extern "C" int {name}(' in source
    assert f"#define PCLIP_COCOOP_MAX_B {_lib.COCOOP_MAX_B}\n" in header and ref.MAX_B == _lib.COCOOP_MAX_B
    assert ref.SLICE == _lib.PROMPT_CTX_SLICE
    assert "#pragma clang fp contract(off)" in source                           # the emulation rounds every product on its own


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_envelope_refusals_fire_with_their_messages():
    from proto_clip_amd import ops
    lib = _lib.load()
    buf = ctypes.c_void_p(0x1000)      # never dereferenced: validation rejects first
    assert lib.pclip_metanet_fwd_f32(buf, buf, buf, buf, buf, 17, 64, 4, 64, buf, buf, None) == -1
    assert b"pclip_metanet_fwd_f32: B=17 images outside 1 .. 16" in lib.pclip_last_error(), lib.pclip_last_error()
    assert lib.pclip_metanet_bwd_f32(buf, buf, buf, buf, 17, 64, 4, 64, buf, buf, buf, buf, buf, None) == -1
    assert b"pclip_metanet_bwd_f32: B=17 images outside 1 .. 16" in lib.pclip_last_error()
    assert lib.pclip_prompt_embed_cond_f16(buf, 77, buf, buf, buf, buf, 4, 17, 5, 9, 64, 50, buf, None) == -1
    assert b"B=17 images outside 1 .. 16" in lib.pclip_last_error()
    assert lib.pclip_prompt_cond_grad_f32(buf, 17, 5, 9, 4, 64, buf, buf, buf, None, 1, None) == -1
    assert b"B=17 images outside 1 .. 16" in lib.pclip_last_error()
    assert lib.pclip_prompt_cond_grad_f32(buf, 2, 17, 9, 4, 64, buf, buf, buf, None, 1, None) == -1
    assert b"nslice=1, expected ceil(N / 16) = 2" in lib.pclip_last_error()
    assert lib.pclip_metanet_fwd_f32(None, buf, buf, buf, buf, 1, 64, 4, 64, buf, buf, None) == -1 and b"null pointer" in lib.pclip_last_error()
    for (E, Hd, Wt), msg in (((72, 4, 64), b"E=72 must be a positive multiple of 64"), ((64, 6, 64), b"Hd=6 must be a multiple of 4 in 4 .. 256"),
                             ((64, 260, 64), b"Hd=260 must be a multiple of 4 in 4 .. 256"), ((64, 4, 60), b"Wt=60 must be a positive multiple of 8")):
        assert lib.pclip_metanet_fwd_f32(buf, buf, buf, buf, buf, 2, E, Hd, Wt, buf, buf, None) == -1
        assert msg in lib.pclip_last_error(), lib.pclip_last_error()
    # the host checks carry the same words and come before any device is asked for
    z = torch.zeros
    for (B, E, Hd, Wt), msg in (((2, 72, 4, 64), r"metanet: E=72 must be a positive multiple of 64"),
                                ((2, 64, 6, 64), r"metanet: Hd=6 must be a multiple of 4 in 4 \.\. 256"),
                                ((2, 64, 260, 64), r"metanet: Hd=260 must be a multiple of 4 in 4 \.\. 256"),
                                ((17, 64, 4, 64), r"metanet: B=17 images outside 1 \.\. 16"),
                                ((2, 64, 4, 60), r"metanet: Wt=60 must be a positive multiple of 8")):
        with pytest.raises(PclipError, match=msg):
            ops.metanet(z(B, E).half(), z(Hd, E), z(Hd), z(Wt, Hd), z(Wt))
    with pytest.raises(PclipError, match=r"metanet_backward: Hd=6 must be a multiple of 4"):
        ops.metanet_backward(z(2, 64), z(2, 64).half(), z(2, 6), z(6, 64), z(64, 6))
    with pytest.raises(PclipError, match=r"do not chain"):
        ops.metanet(z(2, 64).half(), z(4, 128), z(4), z(64, 4), z(64))
    tokens = coop_ref.prompt_tokens(3, 2, 50, 1)
    with pytest.raises(PclipError, match=r"prompt_embed_cond: B=17 images outside 1 \.\. 16"):
        ops.prompt_embed_cond(z(2, 64), z(17, 64), tokens, z(50, 64).half(), z(77, 64).half())
    with pytest.raises(PclipError, match=r"prompt_embed_cond: pi must be float32"):
        ops.prompt_embed_cond(z(2, 64), z(2, 64).half(), tokens, z(50, 64).half(), z(77, 64).half())
    with pytest.raises(PclipError, match=r"prompt_cond_grad: dx \(10, 64\) has not B \* N \* L_out = 2 \* 3 \* 9 rows"):
        ops.prompt_cond_grad(z(10, 64).half(), 2, 3, 9, 2)
    # inside the envelope the wrappers refuse CPU tensors the way their neighbours do
    for call in (lambda: ops.metanet(z(2, 64).half(), z(4, 64), z(4), z(64, 4), z(64)),
                 lambda: ops.metanet_backward(z(2, 64), z(2, 64).half(), z(2, 4), z(4, 64), z(64, 4)),
                 lambda: ops.prompt_embed_cond(z(2, 64), z(2, 64), tokens, z(50, 64).half(), z(77, 64).half()),
                 lambda: ops.prompt_cond_grad(z(2 * 3 * 9, 64).half(), 2, 3, 9, 2)):
        with pytest.raises(PclipError, match="device tensors only"):
            call()


# ---- the learner ------------------------------------------------------------------------------------------------------------------------------------------------

def make_model(kw, seed):
    from proto_clip_amd.clip.model import build_model, random_state_dict
    return build_model(random_state_dict(seed=seed, **kw))


def test_parameters_are_exactly_the_five_tensors():
    from proto_clip_amd import cocoop
    model = make_model(SMALL, 3)
    names = [f"class{i}" for i in range(4)]
    tokens = coop_ref.prompt_tokens(4, 4, SMALL["vocab_size"], 5)
    learner = cocoop.ConditionalPromptLearner(names, model, tokenized_prompts=tokens)
    got = dict(learner.named_parameters())
    assert sorted(got) == ["ctx", "meta_b1", "meta_b2", "meta_w1", "meta_w2"]
    Wt, E = SMALL["transformer_width"], SMALL["embed_dim"]
    Hd = E // 16
    assert learner.n_ctx == 4 and learner.meta_hidden == Hd == 8
    assert got["ctx"].shape == (4, Wt) and got["meta_w1"].shape == (Hd, E) and got["meta_b1"].shape == (Hd,)
    assert got["meta_w2"].shape == (Wt, Hd) and got["meta_b2"].shape == (Wt,)
    assert all(p.dtype == torch.float32 and p.requires_grad and p.is_contiguous() for p in got.values())
    assert float(got["meta_w1"].detach().abs().max()) <= E ** -0.5 and float(got["meta_w2"].detach().abs().max()) <= Hd ** -0.5      # nn.Linear's default range
    assert 0.01 < float(got["ctx"].detach().std()) < 0.03
    again = cocoop.ConditionalPromptLearner(names, model, tokenized_prompts=tokens)
    assert all(torch.equal(p, q) for p, q in zip(learner.parameters(), again.parameters()))                                          # the seed decides
    other = cocoop.ConditionalPromptLearner(names, model, tokenized_prompts=tokens, seed=2)
    assert not torch.equal(other.meta_w1, learner.meta_w1)
    from proto_clip_amd import coop
    assert torch.equal(learner.ctx, coop.PromptLearner(names, model, n_ctx=4, tokenized_prompts=tokens).ctx)                         # coop's context, not a fork
    assert list(cocoop.CoCoOp(model, learner).parameters()) == list(learner.parameters())
    assert not any(p.requires_grad for p in model.parameters())
    assert learner.run_length == int(tokens.argmax(1).max()) + 1
    learner.truncate = False
    assert learner.run_length == 77
    assert cocoop.ConditionalPromptLearner(names, model, tokenized_prompts=tokens, meta_hidden=16).meta_w1.shape == (16, E)
    from proto_clip_amd import CoCoOp as _a, ConditionalPromptLearner as _b, run_cocoop as _c  # noqa: F401
    from proto_clip_amd import coop as coop_mod, maple as maple_mod
    assert "cocoop.py" in coop_mod.__doc__ and "cocoop.py" in maple_mod.__doc__


def test_refusals_that_need_no_device():
    from proto_clip_amd import cocoop
    names = [f"class{i}" for i in range(3)]
    tokens = coop_ref.prompt_tokens(3, 2, TINY["vocab_size"], 5)
    model = make_model(TINY, 4)
    for hidden in (6, 2, 260):
        with pytest.raises(PclipError, match=r"meta_hidden=%d must be a multiple of 4 in 4 \.\. 256" % hidden):
            cocoop.ConditionalPromptLearner(names, model, n_ctx=2, tokenized_prompts=tokens, meta_hidden=hidden)
    with pytest.raises(PclipError, match=r"n_ctx=0"):
        cocoop.ConditionalPromptLearner(names, model, n_ctx=0, tokenized_prompts=tokens)
    early = tokens.clone()
    early[1] = 0
    early[1, 0], early[1, 2] = TINY["vocab_size"] - 2, TINY["vocab_size"] - 1      # the EOT on the last context position
    with pytest.raises(PclipError, match=r"EOT of prompt 1 .* at or before the last of the\s+n_ctx=2"):
        cocoop.ConditionalPromptLearner(names, model, n_ctx=2, tokenized_prompts=early)
    odd = make_model(TINY, 4)
    odd.transformer_heads = 2
    with pytest.raises(PclipError, match=r"text tower of width 64 with 2 heads \(head dimension 64 only\)"):
        cocoop.ConditionalPromptLearner(names, odd, n_ctx=2, tokenized_prompts=tokens)
    learner = cocoop.ConditionalPromptLearner(names, model, n_ctx=2, tokenized_prompts=tokens)
    learner.meta_b1.data = learner.meta_b1.data.half()
    with pytest.raises(PclipError, match=r"meta_b1 must be torch.float32, got torch.float16"):
        learner(torch.zeros(2, 64, dtype=torch.float16))
    learner.meta_b1.data = learner.meta_b1.data.float()
    with pytest.raises(PclipError, match=r"image features torch.float32 \(2, 64\) are not float16 \[B, 64\]"):
        learner(torch.zeros(2, 64))
    with pytest.raises(PclipError, match=r"image features torch.float16 \(2, 32\) are not float16 \[B, 64\]"):
        learner(torch.zeros(2, 32, dtype=torch.float16))
    # a ModifiedResNet image tower is no concern of a learner on cached features: the text side alone is used
    rn = make_model(RESNET, 6)
    assert cocoop.ConditionalPromptLearner(names, rn, n_ctx=2, tokenized_prompts=coop_ref.prompt_tokens(3, 2, RESNET["vocab_size"], 5)).meta_hidden == 8
    with pytest.raises(PclipError, match=r"another CLIP model"):
        cocoop.run_cocoop({"cocoop_epochs": 1}, None, None, None, None, names, rn, learner=learner)
