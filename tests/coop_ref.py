"""CPU restatement of the two kernels of csrc/pclip_prompt.hip, operation by operation as the comments beside them document the arithmetic (torch on the
CPU: IEEE fp32 additions, round-to-nearest-even conversions), and the shared inputs of the CoOp tests."""
import torch

CTX_SLICE = 16      # PCLIP_PROMPT_CTX_SLICE: consecutive classes per first-stage slice of the shared context gradient


def prompt_embed(ctx, tokens, emb16, pos16, L_out=None):
    """x [N * L_out, W] fp16 = r16(f32(src) + f32(pos16[l])): src = r16(ctx[..][l - 1]) on 1 <= l <= n_ctx (two roundings on a context row), the token
    embedding of the clamped id elsewhere (one rounding).  ctx fp32 [n_ctx, W] or [N, n_ctx, W]; tokens [N, L_tok], L_out <= L_tok."""
    N, L_tok = tokens.shape
    vocab, W = emb16.shape
    L_out = L_tok if L_out is None else L_out
    assert ctx.dtype == torch.float32 and emb16.dtype == pos16.dtype == torch.float16
    src = emb16[tokens[:, :L_out].clamp(0, vocab - 1)].clone()                  # [N, L_out, W] fp16
    k = min(ctx.shape[-2], L_out - 1)                                           # context rows at l >= L_out do not exist in the output
    src[:, 1:1 + k] = ctx[..., :k, :].half()                                    # the fp32 parameter rounded once
    return (src.float() + pos16[:L_out].float()).half().reshape(N * L_out, W)


def prompt_ctx_grad(dx16, N, L_out, n_ctx, class_specific, slice_len=CTX_SLICE):
    """dctx fp32 from dx [N * L_out, W] fp16.  Class specific: [N, n_ctx, W] = f32(dx[n, 1 + j]), exact.  Shared: [n_ctx, W]; slices of `slice_len`
    consecutive classes, each summed in class order starting from its first class, then the slice sums added in slice order starting from the first
    slice — every addition a rounded fp32 addition.  A context row with 1 + j >= L_out gets zero."""
    W = dx16.shape[1]
    d = dx16.reshape(N, L_out, W)
    g = torch.zeros(N, n_ctx, W, dtype=torch.float32)
    k = min(n_ctx, L_out - 1)
    g[:, :k] = d[:, 1:1 + k].float()
    if class_specific:
        return g
    parts = []
    for n0 in range(0, N, slice_len):
        acc = g[n0].clone()
        for n in range(n0 + 1, min(N, n0 + slice_len)):
            acc = acc + g[n]
        parts.append(acc)
    out = parts[0].clone()
    for p in parts[1:]:
        out = out + p
    return out


def prompt_tokens(N, n_ctx, vocab, seed, l_eff=None, max_name=5):
    """[N, 77] prompts: SOT (vocab - 2), n_ctx placeholders (id 1), a random class name of 1 .. max_name tokens, EOT (vocab - 1, the highest id).  With
    l_eff the first prompt's EOT sits at position l_eff - 1 and no other lies behind it."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(N, 77, dtype=torch.long)
    for i in range(N):
        n_name = int(torch.randint(1, max_name + 1, (1,), generator=g))
        if l_eff is not None:
            n_name = l_eff - 2 - n_ctx if i == 0 else int(torch.randint(1, max(2, l_eff - 1 - n_ctx), (1,), generator=g))
        t[i, 0] = vocab - 2
        t[i, 1:1 + n_ctx] = 1
        t[i, 1 + n_ctx:1 + n_ctx + n_name] = torch.randint(2, vocab - 2, (n_name,), generator=g)
        t[i, 1 + n_ctx + n_name] = vocab - 1
    return t


def loss64(feats, text, labels, logit_scale):
    """The fixtures' loss: float64 cross-entropy of exp(float32(logit_scale)) * normalize(feats) @ normalize(text).T, on the features cast to float64."""
    import numpy as np
    fi, ft = feats.double(), text.double()
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    return torch.nn.functional.cross_entropy(float(np.exp(np.float64(np.float32(logit_scale)))) * fi @ ft.t(), labels)


def fixture_inputs(kw, N, n_ctx, Q, seed, class_specific, l_eff=None):
    """Seeded (ctx fp32, tokens [N, 77], image features [Q, E] fp16, labels [Q]) of a reference fixture (tests/golden/make_golden_coop.py) — torch's
    CPU generator.  Class names of 1 .. 5 tokens; with l_eff the first prompt's EOT sits at position l_eff - 1 and the others' anywhere from n_ctx + 2 up to it."""
    g = torch.Generator().manual_seed(seed)
    W, E, vocab = kw["transformer_width"], kw["embed_dim"], kw["vocab_size"]
    ctx = torch.randn(*((N, n_ctx, W) if class_specific else (n_ctx, W)), generator=g) * 0.02
    tokens = torch.zeros(N, 77, dtype=torch.long)
    for i in range(N):
        n_name = int(torch.randint(1, 6, (1,), generator=g))
        if l_eff is not None:
            n_name = l_eff - 2 - n_ctx if i == 0 else int(torch.randint(1, l_eff - 1 - n_ctx, (1,), generator=g))
        tokens[i, 0] = vocab - 2                                     # SOT
        tokens[i, 1:1 + n_ctx] = 1                                   # placeholders: their embeddings are overwritten
        tokens[i, 1 + n_ctx:1 + n_ctx + n_name] = torch.randint(2, vocab - 2, (n_name,), generator=g)
        tokens[i, 1 + n_ctx + n_name] = vocab - 1                    # EOT, the highest id
    feats = torch.randn(Q, E, generator=g).half()
    labels = torch.randint(0, N, (Q,), generator=g)
    return ctx, tokens, feats, labels
