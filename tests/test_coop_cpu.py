"""CoOp without a GPU: the CPU restatement of the two prompt kernels (tests/coop_ref.py) checked against the arithmetic their comments document — the
rounding points of the assembly, the slice order of the shared context gradient — and the host logic of proto_clip_amd.coop: placeholder prompts, EOT
positions and L_eff, `ctx_init`, the refusals.  tests/test_gpu_coop.py compares the kernels with that restatement bit for bit."""
import os

import numpy as np
import pytest
import torch

import coop_ref
from conftest import REPO
from spec import E2E, TINY

from proto_clip_amd import _lib, coop
from proto_clip_amd._lib import PclipError
from proto_clip_amd.clip.model import build_model, random_state_dict


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    for name in ("pclip_prompt_embed_f16", "pclip_prompt_ctx_grad_f32"):
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert f"#define PCLIP_PROMPT_CTX_SLICE {_lib.PROMPT_CTX_SLICE}\n" in header and coop_ref.CTX_SLICE == _lib.PROMPT_CTX_SLICE


def _operands(N, n_ctx, W, vocab, seed, class_specific):
    g = torch.Generator().manual_seed(seed)
    emb16 = (torch.randn(vocab, W, generator=g) * 0.02).half()
    pos16 = (torch.randn(77, W, generator=g) * 0.01).half()
    ctx = torch.randn(*((N, n_ctx, W) if class_specific else (n_ctx, W)), generator=g) * 0.02
    return ctx, coop_ref.prompt_tokens(N, n_ctx, vocab, seed + 1), emb16, pos16


@pytest.mark.parametrize("class_specific", [False, True])
def test_assembly_rounds_a_context_row_twice_and_a_token_row_once(class_specific):
    N, n_ctx, W, vocab = 5, 4, 24, 50
    ctx, tokens, emb16, pos16 = _operands(N, n_ctx, W, vocab, 3, class_specific)
    tokens[2, 7], tokens[3, 8] = -4, vocab + 9                              # ids outside the vocabulary clamp to its ends, as text_embed clamps
    x = coop_ref.prompt_embed(ctx, tokens, emb16, pos16).reshape(N, 77, W)
    for n in range(N):
        for l in range(77):
            if 1 <= l <= n_ctx:
                c = (ctx[n] if class_specific else ctx)[l - 1]
                want = (c.half().float() + pos16[l].float()).half()
                assert torch.equal(x[n, l], want)
            else:
                tk = min(max(int(tokens[n, l]), 0), vocab - 1)
                assert torch.equal(x[n, l], (emb16[tk].float() + pos16[l].float()).half())
    # somewhere the two roundings differ from one: the restatement would not notice a kernel that adds in fp32 otherwise
    rows = ctx if class_specific else ctx[None].expand(N, -1, -1)
    twice = (rows.half().float() + pos16[1:1 + n_ctx].float()).half()
    single = (rows + pos16[1:1 + n_ctx].float()).half()
    assert (twice != single).any()
    # the truncated form is the leading positions of the full one
    for L in (6, 33):
        assert torch.equal(coop_ref.prompt_embed(ctx, tokens, emb16, pos16, L).reshape(N, L, W), x[:, :L])


def test_assembly_of_fp16_exact_rows_is_the_token_embedding_sum():
    N, n_ctx, W, vocab = 3, 4, 16, 40
    _, tokens, emb16, pos16 = _operands(N, n_ctx, W, vocab, 5, False)
    ids = torch.tensor([7, 9, 11, 13])
    real = tokens.clone()
    real[:, 1:1 + n_ctx] = ids
    want = (emb16[real].float() + pos16.float()).half().reshape(N * 77, W)      # text_embed_kernel's arithmetic
    assert torch.equal(coop_ref.prompt_embed(emb16[ids].float(), tokens, emb16, pos16), want)


@pytest.mark.parametrize("N", [1, 7, 16, 17, 130])
def test_shared_context_gradient_follows_the_documented_slice_order(N):
    n_ctx, W, L = 3, 8, 9
    g = torch.Generator().manual_seed(N)
    dx = (torch.randn(N * L, W, generator=g) * torch.logspace(-3, 0, N * L)[torch.randperm(N * L, generator=g)][:, None]).half()
    got = coop_ref.prompt_ctx_grad(dx, N, L, n_ctx, False)
    rows = dx.reshape(N, L, W)[:, 1:1 + n_ctx].float().numpy()
    parts = []
    for s in range(0, N, 16):
        acc = rows[s].copy()
        for n in range(s + 1, min(N, s + 16)):
            acc = (acc + rows[n]).astype(np.float32)
        parts.append(acc)
    want = parts[0].copy()
    for p in parts[1:]:
        want = (want + p).astype(np.float32)
    assert np.array_equal(got.numpy(), want)
    exact = dx.reshape(N, L, W)[:, 1:1 + n_ctx].double().sum(0)
    assert float((got.double() - exact).abs().max()) <= N * 2.0 ** -24 * float(rows.astype(np.float64).__abs__().sum(0).max())
    if N > 32:                                                               # the order matters: a plain class-order sum gives other bits somewhere
        seq = rows[0].copy()
        for n in range(1, N):
            seq = (seq + rows[n]).astype(np.float32)
        assert not np.array_equal(seq, want)
    spec = coop_ref.prompt_ctx_grad(dx, N, L, n_ctx, True)
    assert spec.shape == (N, n_ctx, W) and torch.equal(spec, dx.reshape(N, L, W)[:, 1:1 + n_ctx].float())


def test_context_rows_beyond_a_truncated_length_get_no_gradient():
    N, n_ctx, W, L = 2, 8, 8, 6
    dx = torch.ones(N * L, W).half()
    got = coop_ref.prompt_ctx_grad(dx, N, L, n_ctx, False)
    assert torch.equal(got[:L - 1], torch.full((L - 1, W), float(N))) and not got[L - 1:].any()


# ---- host logic -------------------------------------------------------------------------------------------------------------------------------------

def tiny_tokenize(texts, vocab=TINY["vocab_size"]):
    """A word-level tokenizer for the test towers: SOT = vocab - 2, EOT = vocab - 1, words hashed into 1 .. vocab - 3."""
    texts = [texts] if isinstance(texts, str) else texts
    out = torch.zeros(len(texts), 77, dtype=torch.long)
    for i, text in enumerate(texts):
        words = text.replace(".", " .").split()
        ids = [vocab - 2] + [1 + sum(ord(c) * (k + 1) for k, c in enumerate(w)) % (vocab - 3) for w in words] + [vocab - 1]
        out[i, :len(ids)] = torch.tensor(ids)
    return out


@pytest.fixture(scope="module")
def tiny_model():
    return build_model(random_state_dict(seed=3, **TINY))


def test_placeholder_prompts_and_lengths(tiny_model):
    names = ["cat", "tabby_cat", "a very long class name"]
    assert coop.placeholder_prompts(names, 3) == ["X X X cat.", "X X X tabby cat.", "X X X a very long class name."]
    pl = coop.PromptLearner(names, tiny_model, n_ctx=3, tokenize=tiny_tokenize)
    toks = pl.tokenized_prompts
    assert toks.shape == (3, 77) and toks.dtype == torch.int64
    assert bool((toks[:, 1:4] == toks[0, 1]).all())                          # the n_ctx placeholders, one token each
    eot = coop.eot_positions(toks)
    assert eot.tolist() == [3 + 1 + 1 + 1, 3 + 2 + 1 + 1, 3 + 5 + 1 + 1]      # SOT + ctx + words + "." -> EOT
    assert pl.l_eff == coop.effective_length(toks) == 11 and pl.run_length == 11
    assert coop.PromptLearner(names, tiny_model, n_ctx=3, tokenize=tiny_tokenize, truncate=False).run_length == 77
    assert pl.ctx.shape == (3, 64) and pl.ctx.dtype == torch.float32 and pl.ctx.requires_grad
    assert [n for n, _ in pl.named_parameters()] == ["ctx"]                  # the CLIP model is referenced, not registered
    assert 0.01 < float(pl.ctx.detach().std()) < 0.03
    again = coop.PromptLearner(names, tiny_model, n_ctx=3, tokenize=tiny_tokenize)
    assert torch.equal(again.ctx, pl.ctx)                                    # seeded
    assert coop.PromptLearner(names, tiny_model, n_ctx=3, tokenize=tiny_tokenize, class_specific=True).ctx.shape == (3, 3, 64)


def test_eot_is_the_first_maximum():
    t = torch.tensor([[5, 1, 9, 0, 9, 0], [9, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]])
    assert coop.eot_positions(t).tolist() == [2, 0, 5] and coop.effective_length(t) == 6


def test_ctx_init_rows_are_the_token_embeddings():
    from proto_clip_amd.clip import tokenize
    model = build_model(random_state_dict(seed=4, **E2E))
    pl = coop.PromptLearner(["dog", "hot_dog"], model, ctx_init="a photo of a")
    ids = tokenize("a photo of a")[0, 1:5]
    assert pl.n_ctx == 4 and pl.ctx.shape == (4, E2E["transformer_width"])
    assert torch.equal(pl.ctx.detach(), model.token_embedding.weight[ids].float())
    assert torch.equal(pl.tokenized_prompts, tokenize(["X X X X dog.", "X X X X hot dog."]))
    x_id = int(tokenize("X")[0, 1])
    assert bool((pl.tokenized_prompts[:, 1:5] == x_id).all()) and pl.l_eff == 9
    ps = coop.PromptLearner(["dog", "hot_dog"], model, ctx_init="a photo of a", class_specific=True)
    assert ps.ctx.shape == (2, 4, E2E["transformer_width"]) and torch.equal(ps.ctx[1].detach(), pl.ctx.detach())


def test_refusals(tiny_model):
    names = ["cat", "dog"]
    with pytest.raises(PclipError, match="float16"):
        coop.PromptLearner(names, tiny_model, n_ctx=2, tokenize=tiny_tokenize, dtype=torch.float16)
    pl = coop.PromptLearner(names, tiny_model, n_ctx=2, tokenize=tiny_tokenize)
    pl.ctx.data = pl.ctx.data.half()
    with pytest.raises(PclipError, match="float16"):
        pl()
    with pytest.raises(PclipError, match="middle"):
        coop.PromptLearner(names, tiny_model, n_ctx=2, tokenize=tiny_tokenize, class_token_position="middle")
    toks = tiny_tokenize(["X X cat.", "X ."])                                # the second prompt's EOT sits at position 3 = n_ctx
    with pytest.raises(PclipError, match=r"EOT of prompt 1 \('dog'\) sits at position 3"):
        coop.PromptLearner(names, tiny_model, n_ctx=3, tokenized_prompts=toks)
    with pytest.raises(PclipError, match="3 classnames but 2 tokenized prompts"):
        coop.PromptLearner(names + ["bird"], tiny_model, n_ctx=2, tokenized_prompts=tiny_tokenize(["X X cat.", "X X dog."]))
    with pytest.raises(PclipError, match="int64"):
        coop.PromptLearner(names, tiny_model, n_ctx=2, tokenized_prompts=tiny_tokenize(["X X cat.", "X X dog."]).int())
    with pytest.raises(PclipError, match="n_ctx=0"):
        coop.PromptLearner(names, tiny_model, n_ctx=0, tokenize=tiny_tokenize)
