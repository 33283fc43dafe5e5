"""One statement of a transformer tower pass (reference clip/model.py:171-190 per block, 233-236 / 348-352 for the heads), shared by everything that runs one:
CLIP.encode_image / encode_text (clip/model.py), the taped tail (autograd.TowerTailFn), coop.PromptLearner and vpt.VisualPromptLearner.

    residual_block   the kernel calls of one block on the in-place residual stream; with a recorder it hands over what the backward reads
    _run_blocks      the frozen walk over a stack of blocks (split-K forms inside ops.low_latency)
    Tower            what a pass needs to know about one tower, built once per model: blocks, heads, final LayerNorm, projection, row pick, tape plan
    run_tower        the tower from the stream that enters block 0: frozen prefix walk, taped tail, heads — or, nothing taped, the frozen walk and the
                     closing LayerNorm + projection
    vit_stem         the frozen ViT stem (im2col + GEMM + token assembly, or the fused assembly + ln_pre + ln_1 pass)

Every kernel is reached as `ops.<name>(...)`, looked up when it is called."""
import torch

from . import ops
from ._lib import PclipError


def _block_params(blk):
    """The 12 parameters of a residual block in the order residual_block and TowerTailFn take them."""
    attn, mlp, ln_1, ln_2 = blk.attn, blk.mlp, blk.ln_1, blk.ln_2
    out, fc, pr = attn.out_proj, mlp.c_fc, mlp.c_proj
    return [ln_1.weight, ln_1.bias, attn.in_proj_weight, attn.in_proj_bias, out.weight, out.bias, ln_2.weight, ln_2.bias, fc.weight, fc.bias,
            pr.weight, pr.bias]


def residual_block(x, h, params, B, L, heads, causal, pick=None, first_token=False, splitk=False, rec=None):
    """ResidualAttentionBlock.forward (clip/model.py:187-190) on the residual stream x [B*L, W] fp16, updated IN PLACE, given h = ln_1(x):
        qkv = in_proj(h)   a = attention(qkv)   x += out_proj(a)   h = ln_2(x)   f = QuickGELU(c_fc(h))   x += c_proj(f)
    Both residual adds ride in the epilogue of the GEMM that produces the addend (pclip_gemm_f16 with `residual`: the residual rows are read in the
    coalesced store pass, r16(x + r16(acc + bias)) — the reference's two roundings); ln_2 is a read-x / write-h pass (the reference's rounding point
    h = r16(LN(x))).  params: the block's 12 parameters in `_block_params` order.  Returns (x, d): d is None, or — `splitk`, the frozen walk inside
    ops.low_latency — c_proj's output from the split-K kernel, which the caller's next LayerNorm pass still has to add (pclip_add_layernorm_f16; the
    out_proj add is taken the same way in here).

    `pick(t)` (the LAST block of a pass whose caller reads B rows only) picks those rows from a [B*L, W] tensor: the class token of the vision tower
    (clip/model.py:233), the EOT token of the text tower (:350).  The reference pushes every token through the last block and then discards all but
    that row; here the block's out_proj, LN2 and MLP run on those B rows only — the same arithmetic for the rows that matter (a GEMM row does not
    depend on the other rows), 9/12 of one layer's linear FLOPs saved (6 % of a 12-layer tower).  `first_token` (vision tower: the picked row is token
    0 of every sequence) additionally projects the QUERIES for those B rows only and runs the attention for that one query per image (keys / values
    still come from every token).

    rec (a dict, the taped pass): receives x_in, h1, qkv or q / kv, a, x_mid, h2, f, picked.  x_in and x_mid are copies taken at this point of the
    sequence — the stream is overwritten by the next GEMM.  Without it nothing is cloned."""
    ln1w, ln1b, win, bin_, wout, bout, ln2w, ln2b, wfc, bfc, wpr, bpr = params
    if rec is not None:
        rec.update(x_in=x.clone(), h1=h, picked=pick is not None)
    if pick is not None and first_token and not causal:
        W = x.shape[1]
        kv = ops.gemm(h, win[W:3 * W], bin_[W:3 * W])                          # keys | values of every token
        q = ops.gemm(pick(h), win[0:W], bin_[0:W])                             # queries of the class tokens
        a, x = ops.attention_first_queries(q, kv, B, L, 1, heads), pick(x)
        if rec is not None:
            rec.update(q=q, kv=kv)
    else:
        qkv = ops.gemm(h, win, bin_)
        a = ops.attention(qkv, B, L, heads, causal=causal)
        if rec is not None:
            rec.update(qkv=qkv)
        if pick is not None:
            a, x = pick(a), pick(x)                                            # x holds the residual stream entering this block's out_proj add
    if splitk and ops.splitk_active(a.shape[0]):
        h = ops.add_layernorm(x, ops.gemm(a, wout, bout), ln2w, ln2b)
    else:
        ops.gemm(a, wout, bout, residual=x, out=x)
        h = ops.layernorm(x, ln2w, ln2b)
    if rec is not None:
        rec.update(a=a, x_mid=x.clone(), h2=h)
    f = ops.gemm(h, wfc, bfc, act=1)
    if rec is not None:
        rec.update(f=f)
    if splitk and ops.splitk_active(f.shape[0]):
        return x, ops.gemm(f, wpr, bpr)
    ops.gemm(f, wpr, bpr, residual=x, out=x)
    return x, None


def _run_blocks(x, blocks, B, L, heads, causal, select=None, first_token=False, h0=None):
    """The frozen walk: `residual_block` per layer on x [B*L, W] fp16 (updated IN PLACE), each next block's ln_1 between them.  In low-latency mode
    (ops.low_latency: split-K linears of a serving request) the addends come from the split-K kernel and the adds stay in the LayerNorm passes.
    Returns (x, d): the stack's output is x (+ d when d is not None — low-latency mode leaves the last add to the caller's final LayerNorm), [B, W]
    rows picked by `select` when given (`select` / `first_token`: residual_block's `pick` for the last block).
    `h0`: the first block's ln_1 output when the caller's stem produced it."""
    params = [_block_params(blk) for blk in blocks]
    n, d = len(params), None
    if n > 0:
        h = h0 if h0 is not None else ops.layernorm(x, params[0][0], params[0][1])
    for i in range(n):
        last = i == n - 1
        x, d = residual_block(x, h, params[i], B, L, heads, causal, select if last else None, first_token, splitk=True)
        if not last:
            lnw, lnb = params[i + 1][0], params[i + 1][1]
            h = ops.layernorm(x, lnw, lnb) if d is None else ops.add_layernorm(x, d, lnw, lnb)
    if select is not None and n == 0:
        x = select(x)
    return x, d


def eot_positions(tokens: torch.Tensor) -> torch.Tensor:
    """Position of the FIRST maximum of every token row (int64 [N]): the row `ops.gather_eot` picks — the EOT token has the highest id."""
    L = tokens.shape[1]
    pos = torch.arange(L, device=tokens.device).expand(tokens.shape[0], L)
    return torch.where(tokens == tokens.max(dim=-1, keepdim=True).values, pos, pos.new_full((), L)).min(dim=-1).values


def class_row_pick(B, L, device, tokens=None):
    """(select, rows) of the vision tower: x[:, 0, :] (clip/model.py:233); rows() = the picked rows' indices in the [B*L, W] stream."""
    return (lambda t: t.view(B, L, -1)[:, 0, :].contiguous()), (lambda: torch.arange(B, device=device) * L)


def eot_row_pick(B, L, device, tokens):
    """(select, rows) of the text tower: x[arange, text.argmax(-1)] (clip/model.py:350) for the token rows `tokens` [B, L]."""
    return (lambda t: ops.gather_eot(t, tokens, B, L, t.shape[1])), (lambda: torch.arange(B, device=device) * L + eot_positions(tokens))


class Tower:
    """One transformer tower as the passes see it.  entry / name / stem_word: the words of the refusals; prefix, head: (name, parameter) pairs of
    everything in front of block 0 (in the stem Function's argument order) and of the final LayerNorm and projection; first_token / pick: the row the
    caller reads (class_row_pick / eot_row_pick); projT_key: the frozen pass' key of the transposed projection in `cache`; stem_opt_in:
    CLIP.unfreeze(stem=...) has opted the prefix in."""

    def __init__(self, entry, name, stem_word, *, blocks, heads, causal, ln, proj, cache, projT_key, prefix, head, pick):
        self.entry, self.name, self.stem_word = entry, name, stem_word
        self.blocks, self.heads, self.causal, self.ln, self.proj, self.cache, self.projT_key = blocks, heads, causal, ln, proj, cache, projT_key
        self.prefix, self.head, self.pick, self.first_token = prefix, head, pick, not causal
        self.stem_opt_in = False

    def tape_from(self, prefix=None):
        """Index of the first residual block with a trainable parameter (len(blocks) when only the heads train), None when nothing of the tower
        trains.  Refuses a trainable parameter in the frozen prefix, opted in or not: the taped passes of the model plan with `tape_plan`."""
        for name, p in self.prefix if prefix is None else prefix:
            if p.requires_grad:
                raise PclipError(f"{self.name}: parameter {name} requires grad but lies in the frozen prefix of the tower (only a tail of residual "
                                 "blocks, the final LayerNorm and the projection are differentiable)")
        for i, blk in enumerate(self.blocks):
            if any(p.requires_grad for p in blk.parameters()):
                return i
        return len(self.blocks) if any(p.requires_grad for _, p in self.head) else None

    def tape_plan(self):
        """(first, stem): `tape_from`, refusals included — except that a prefix opted in through CLIP.unfreeze(stem=...) with a parameter that
        requires grad puts the whole tower on the tape: (0, True)."""
        if not self.stem_opt_in:
            return self.tape_from(), False
        if any(p.requires_grad for _, p in self.prefix):
            for name, p in self.prefix:
                if p.requires_grad and p.dtype not in (torch.float16, torch.float32):
                    raise PclipError(f"{self.name}: unsupported dtype {p.dtype} of parameter {name}")
            return 0, True
        return self.tape_from(prefix=[]), False

    def what(self, first, stem):
        """The taped pass in the words of its refusals."""
        n = len(self.blocks)
        if stem:
            return f"{self.entry} ({self.name}, {self.stem_word} + blocks 0..{n - 1} + heads on the tape)"
        return f"{self.entry} ({self.name}, blocks {first}..{n - 1} + heads trainable)"


def run_tower(tw, x, B, L, plan, pick, what=None, h0=None, deep=None, deep_off=None):
    """Features [B, E] of tower `tw` from the residual stream x [B*L, W] that enters block 0.  plan = (first, stem) as `Tower.tape_plan` gives it:
    blocks[:first] run frozen, blocks[first:] + final LayerNorm + projection on the tape (autograd.run_tower_tail; only the heads when
    first == len(blocks): the frozen walk then keeps its class-row shortcut); first None: nothing is taped — the frozen walk, ln(picked row)
    (row-wise: commutes with the pick) and the projection GEMM.  pick = (select, rows) from `tw.pick`; h0: ln_1(x) of block 0 when the stem
    produced it (dropped when a frozen prefix runs first); what: the pass in the words of a refusal (default `tw.what`); deep, deep_off: TowerTailFn's pack of
    deep prompt rows and the first of its rows in a sequence (None: the last rows, which run_tower_tail resolves to L - P)."""
    first, stem = plan
    select, _ = pick
    if first is None:
        x, d = _run_blocks(x, tw.blocks, B, L, tw.heads, tw.causal, select=select, first_token=tw.first_token, h0=h0)
        if d is None:
            y = ops.layernorm(x, tw.ln.weight, tw.ln.bias)
        else:
            y = ops.add_layernorm(x, d, tw.ln.weight, tw.ln.bias, update_x=False)
        return ops.gemm(y, tw.cache.get(tw.projT_key, tw.proj, lambda t: t.t().contiguous()))
    from .autograd import run_tower_tail
    what = tw.what(first, stem) if what is None else what
    if first == len(tw.blocks) and not x.requires_grad:                        # only the heads train, behind a constant stream
        with torch.no_grad():
            x, _ = _run_blocks(x, tw.blocks, B, L, tw.heads, tw.causal, select=select, first_token=tw.first_token, h0=h0)
        return run_tower_tail(tw, x, None, first, B, L, (None, None), what)
    if first > 0:
        with torch.no_grad():
            x, _ = _run_blocks(x, tw.blocks[:first], B, L, tw.heads, tw.causal, h0=h0)
        h0 = None
    return run_tower_tail(tw, x, h0, first, B, L, pick, what, deep=deep, deep_off=deep_off)


def _pad_patch_weight(w):
    """conv1.weight [W, 3, P, P] -> GEMM rows [W, kpad]: zero columns up to the K-tile, as ops.im2col_patches pads its matrix."""
    kp = w.shape[1] * w.shape[2] * w.shape[3]
    kpad = (kp + 63) // 64 * 64
    w2 = w.reshape(w.shape[0], kp)
    if kpad != kp:
        w2 = torch.cat([w2, w2.new_zeros(w.shape[0], kpad - kp)], dim=1)
    return w2.contiguous()


def vit_stem(cache, img, wconv, cls, pos, P, fused=None):
    """The frozen ViT stem on contiguous images [B, 3, R, R]: conv1 as im2col + GEMM (clip/model.py:222), then the tokens [class ; patches] + pos
    [B*L, W] fp16 (225-226) — or, fused = (ln_pre.weight, ln_pre.bias, ln_1.weight, ln_1.bias) of block 0, the one-pass
    (x, h0) = (ln_pre(tokens), ln_1(x)) (225-227, 188)."""
    B, W = img.shape[0], wconv.shape[0]
    G2 = (img.shape[2] // P) ** 2
    w16 = cache.get("conv1", wconv, _pad_patch_weight)
    cls16 = cache.get("cls", cls, lambda t: t.half())
    pos16 = cache.get("pos", pos, lambda t: t.half().contiguous())
    patch = ops.gemm(ops.im2col_patches(img, P), w16 if w16.dtype == torch.float16 else w16.half())
    if fused is not None:
        return ops.vit_embed_ln(patch, cls16, pos16, B, G2, W, *fused)
    return ops.vit_assemble_tokens(patch, cls16, pos16, B, G2, W)
