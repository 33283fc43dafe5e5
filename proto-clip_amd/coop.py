"""CoOp (Context Optimization), the learned-prompt baseline of the few-shot tables: the context vectors of the prompt — the "a photo of a" part — are
fp32 parameters trained by gradient descent through the FROZEN text tower, on cached image features:

    prompts  = [SOT ; ctx (n_ctx learned rows) ; class-name tokens ; "." ; EOT ; padding] + positional_embedding      # csrc/pclip_prompt.hip
    text     = text_projection(ln_final(transformer(prompts))[EOT row])                                              # autograd.TowerTailFn from block 0
    loss     = cross_entropy(logit_scale.exp() * normalise(image_features) @ normalise(text).T, labels)              # autograd.cosine_cross_entropy

The tower is causal and only the EOT row is read, so positions after the last EOT cannot reach anything that is kept: with `truncate=True` the whole
step (assembly, every GEMM, LayerNorm and attention launch, forward and backward) runs at L_eff = (largest EOT position) + 1 tokens instead of 77.
A frozen tower pays for no parameter gradient (TowerTailFn skips what `needs_input_grad` does not ask for); `clip_model.unfreeze(text_blocks=k)`
composes with it: the last k blocks and the heads then train beside the context.

Envelope: the class token at the "end" (context directly after SOT) only, fp32 `ctx`, head dimension 64, prompts of at most 77 tokens.  Not here:
the "middle" / "front" positions.  CoCoOp's meta-net (an image-conditioned context) is `cocoop.py`."""
import torch

from . import autograd as pag
from . import ops
from . import utils
from ._lib import PclipError
from .prompt_train import accuracy, train_prompts
from .tower import eot_positions, run_tower

PLACEHOLDER = "X"        # one BPE token; its embedding is never read (the context rows take its positions)


def placeholder_prompts(classnames, n_ctx: int):
    """Upstream's prompt texts: n_ctx placeholder words, the class name (underscores as spaces) and a full stop."""
    prefix = " ".join([PLACEHOLDER] * n_ctx)
    return [prefix + " " + name.replace("_", " ") + "." for name in classnames]


def effective_length(tokens: torch.Tensor) -> int:
    """L_eff = (largest EOT position) + 1: no later position can influence an EOT row of a causal tower."""
    return int(eot_positions(tokens).max()) + 1


class PromptLearner(torch.nn.Module):
    """The learned context and the prompts it is spliced into.  `ctx` is the one parameter: fp32 [n_ctx, W], or with `class_specific` [N, n_ctx, W].
    ctx_init (a text such as "a photo of a"): the rows start as that text's token embeddings and n_ctx is its token count; otherwise N(0, 0.02) rows
    from `seed`.  tokenize: a callable like `clip.tokenize` (default); tokenized_prompts: the [N, context_length] int64 prompts themselves (placeholders
    at positions 1 .. n_ctx), for towers whose vocabulary the tokenizer does not cover.  forward() -> text features [N, E] fp16 with a tape to `ctx`
    (and to whatever of the text tower's tail is unfrozen); under torch.no_grad() the same kernels without a tape.  The CLIP model is referenced, not
    registered: `parameters()` is the context alone."""

    def __init__(self, classnames, clip_model, n_ctx=16, ctx_init=None, class_specific=False, tokenize=None, tokenized_prompts=None, truncate=True,
                 seed=1, class_token_position="end", dtype=torch.float32):
        super().__init__()
        if class_token_position != "end":
            raise PclipError(f"PromptLearner: class_token_position={class_token_position!r} is not supported (only 'end': the context directly "
                             "after SOT, the class name behind it)")
        if dtype != torch.float32:
            raise PclipError(f"PromptLearner: ctx must be torch.float32, got {dtype} (the context and its gradient are fp32; the kernels round it "
                             "to fp16 where an fp16 CoOp would hold fp16 values)")
        W = clip_model.transformer.width
        if W % 8 != 0 or W != 64 * clip_model.transformer_heads:
            raise PclipError(f"PromptLearner: text tower of width {W} with {clip_model.transformer_heads} heads (head dimension 64 only)")
        emb = clip_model.token_embedding.weight
        device = emb.device
        classnames = list(classnames)
        if tokenized_prompts is None or ctx_init is not None:
            if tokenize is None:
                from .clip import tokenize
        if ctx_init is not None:
            init_tokens = tokenize(ctx_init.replace("_", " "))
            n_ctx = int(eot_positions(init_tokens)[0]) - 1
            if n_ctx < 1:
                raise PclipError(f"PromptLearner: ctx_init={ctx_init!r} holds no token")
            ids = init_tokens[0, 1:1 + n_ctx].to(device)
            if int(ids.max()) >= emb.shape[0]:
                raise PclipError(f"PromptLearner: ctx_init={ctx_init!r} has token ids beyond the tower's vocabulary of {emb.shape[0]}")
            rows = emb.detach()[ids].float()
            if class_specific:
                rows = rows[None].expand(len(classnames), -1, -1)
        else:
            n_ctx = int(n_ctx)
            if n_ctx < 1:
                raise PclipError(f"PromptLearner: n_ctx={n_ctx} must be at least 1")
            g = torch.Generator().manual_seed(seed)
            shape = (len(classnames), n_ctx, W) if class_specific else (n_ctx, W)
            rows = (torch.randn(*shape, generator=g) * 0.02).to(device)
        if tokenized_prompts is None:
            tokenized_prompts = tokenize(placeholder_prompts(classnames, n_ctx))
        tokens = torch.as_tensor(tokenized_prompts)
        if tokens.dim() != 2 or tokens.dtype != torch.int64 or tokens.shape[1] != clip_model.context_length:
            raise PclipError(f"PromptLearner: tokenized_prompts must be int64 [N, {clip_model.context_length}], got {tokens.dtype} {tuple(tokens.shape)}")
        if tokens.shape[0] != len(classnames):
            raise PclipError(f"PromptLearner: {len(classnames)} classnames but {tokens.shape[0]} tokenized prompts")
        if tokens.shape[1] > 77:
            raise PclipError(f"PromptLearner: prompts of {tokens.shape[1]} tokens (at most 77)")
        eot = eot_positions(tokens)
        bad = (eot <= n_ctx).nonzero().flatten()
        if bad.numel():
            i = int(bad[0])
            raise PclipError(f"PromptLearner: the EOT of prompt {i} ({classnames[i]!r}) sits at position {int(eot[i])}, at or before the last of the "
                             f"n_ctx={n_ctx} context rows (positions 1 .. {n_ctx}): the context would overwrite it")
        self.n_ctx, self.n_cls, self.class_specific, self.truncate = n_ctx, len(classnames), bool(class_specific), bool(truncate)
        self.classnames = classnames
        self.context_length = tokens.shape[1]
        self.l_eff = int(eot.max()) + 1
        self.ctx = torch.nn.Parameter(rows.contiguous().clone())
        self.register_buffer("tokenized_prompts", tokens.to(device))
        object.__setattr__(self, "clip_model", clip_model)

    @property
    def run_length(self) -> int:
        """Tokens per prompt the tower runs at: L_eff with `truncate`, else the context length."""
        return self.l_eff if self.truncate else self.context_length

    def forward(self):
        m = self.clip_model
        if self.ctx.dtype != torch.float32:
            raise PclipError(f"PromptLearner: ctx must be torch.float32, got {self.ctx.dtype}")
        taped = False
        if torch.is_grad_enabled():
            tail = m._text_tape_from()                                     # refuses a trainable embedding in the frozen prefix
            taped = self.ctx.requires_grad or tail is not None             # the context, or something of the tower's blocks / heads, trains
        L = self.run_length
        emb16 = m._cache.get("tok", m.token_embedding.weight, lambda t: t.half().contiguous())
        pos16 = m._cache.get("pos", m.positional_embedding, lambda t: t.half().contiguous())
        with torch.set_grad_enabled(taped):
            outs = []
            for i in range(0, self.n_cls, m.text_chunk):
                tokens = self.tokenized_prompts[i:i + m.text_chunk]
                ctx = self.ctx[i:i + m.text_chunk] if self.class_specific else self.ctx
                outs.append(self._chunk(ctx, tokens, emb16, pos16, L, taped))
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _chunk(self, ctx, tokens, emb16, pos16, L, taped):
        tw = self.clip_model.text_tower
        B = tokens.shape[0]
        head = tokens[:, :L].contiguous()                                    # the EOT lies inside: the first maximum of the cut row is the full row's
        if taped:
            x = pag.PromptEmbedFn.apply(ctx, tokens, emb16, pos16, self.n_ctx, L)
            what = f"PromptLearner (n_ctx={self.n_ctx}, {L} tokens per prompt, text tower taped from block 0)"
            return run_tower(tw, x, B, L, (0, False), tw.pick(B, L, x.device, head), what=what)
        x = ops.prompt_embed(ctx.detach(), tokens, emb16, pos16, L)
        return run_tower(tw, x, B, L, (None, False), tw.pick(B, L, x.device, head))


class CoOp(torch.nn.Module):
    """A CLIP model's temperature with a `PromptLearner`'s text features: the training loss on cached image features and the classifier."""

    def __init__(self, clip_model, prompt_learner):
        super().__init__()
        self.prompt_learner = prompt_learner
        object.__setattr__(self, "clip_model", clip_model)

    def logit_scale(self):
        return self.clip_model.logit_scale.float().exp()

    def forward(self):
        return self.prompt_learner()

    def loss(self, image_features, labels):
        """Cross-entropy of logit_scale.exp() * normalise(image_features) @ normalise(text)^T against `labels`; the [Q, N] logits are never written."""
        return pag.cosine_cross_entropy(image_features, self.prompt_learner(), self.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)

    def distill_loss(self, image_features, teacher_weights, teacher_scale=None, temperature=1.0):
        """KL from a frozen classifier's prediction — `teacher_weights` [N, Et] fp16 rows, e.g. the hand-crafted prompts' text features, read against the same
        `image_features` when Et is their width — to this model's: mean KL(softmax(teacher logits / tau) || softmax(own logits / tau)) tau^2, both sides
        L2-normalised in the kernel, neither [Q, N] matrix written (autograd.cosine_kd).  teacher_scale=None: logit_scale's value."""
        return self._distill(image_features, self.prompt_learner(), teacher_weights, teacher_scale, temperature)

    def _distill(self, image_features, text, teacher_weights, teacher_scale, temperature):
        scale = self.logit_scale()
        ts = float(scale.detach()) if teacher_scale is None else teacher_scale
        return pag.cosine_kd(image_features, text, scale, image_features, teacher_weights, ts, temperature=temperature, normalize_a=True, normalize_b=True,
                             normalize_teacher_a=True, normalize_teacher_b=True)

    def kg_loss(self, image_features, labels, zs_text_features, weight=8.0):
        """KgCoOp (Yao et al., CVPR 2023): the cross-entropy plus `weight` times 1 - mean cosine of the learned text features to the frozen hand-crafted ones
        (`zs_text_features` [N, E] fp16, normalised inside the kernel, so either form will do), from ONE `prompt_learner()` forward."""
        text = self.prompt_learner()
        ce = pag.cosine_cross_entropy(image_features, text, self.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)
        return ce + weight * pag.feature_reg(text, zs_text_features, "cos", True)

    def text_rows(self):
        """The learned classifier: L2-normalised text features [N, E] fp16, a constant."""
        with torch.no_grad():
            return ops.l2norm_rows(self.prompt_learner())

    def classify(self, features, topk=0):
        """arg-max class (int64 [Q]) of `features` (cached, normalised image features) against the learned rows; with topk > 0 also the top-k values
        and indices, as `utils.clip_zero_shot` returns them."""
        return utils.clip_zero_shot(features, self.text_rows(), scale=float(self.logit_scale()), topk=topk, layout="nd")


def run_coop(cfg, train_features, train_labels, test_features, test_labels, classnames, clip_model, tokenize=None, tokenized_prompts=None,
             zs_text_features=None):
    """Train a context on cached features ([Q, D] fp16 and labels, as `pre_load_features` / `build_cache_model` hold them) with CoOp's recipe: SGD on `ctx`,
    learning rate 0.002, momentum 0.9, cosine schedule, batches of 32, cfg['coop_epochs'] epochs, cfg['n_ctx'] context rows (optional keys: 'ctx_init',
    'class_specific', 'coop_lr', 'coop_batch', 'coop_loss_scale', 'seed').  The loss goes through torch's GradScaler (initial scale 1024): the gradient
    stream inside the tower is fp16, and at 1000 classes an unscaled mean loss leaves most of it in fp16's subnormal range (profiles/coop.txt: 23 % gradient
    error unscaled, 0.4 % scaled); `ctx` and its gradient are fp32, so the scaler and the optimizer are torch's own.  Prints the test accuracy before training
    and after every epoch; returns the trained `CoOp` module (`.results`: the figures).  With cfg['kg_weight'] the loss is `CoOp.kg_loss` against
    `zs_text_features` ([N, E] fp16, the frozen hand-crafted text features: KgCoOp, weight 8 upstream); without the key nothing changes."""
    seed = int(cfg.get("seed", 1))
    kg = cfg.get("kg_weight")
    if kg is not None and zs_text_features is None:
        raise PclipError("run_coop: cfg['kg_weight'] needs zs_text_features, the frozen text features [N, E] the context is held to")
    learner = PromptLearner(classnames, clip_model, n_ctx=cfg.get("n_ctx", 16), ctx_init=cfg.get("ctx_init"), class_specific=cfg.get("class_specific", False),
                            tokenize=tokenize, tokenized_prompts=tokenized_prompts, seed=seed)
    model = CoOp(clip_model, learner)
    labels = train_labels.to(train_features.device).long()
    if kg is None:
        loss_at = lambda idx: model.loss(train_features[idx].contiguous(), labels[idx])
    else:
        loss_at = lambda idx: model.kg_loss(train_features[idx].contiguous(), labels[idx], zs_text_features, weight=float(kg))
    res, _ = train_prompts("CoOp", learner.parameters(), loss_at,
                           train_features.shape[0], train_features.device, epochs=int(cfg["coop_epochs"]), batch=int(cfg.get("coop_batch", 32)),
                           lr=cfg.get("coop_lr", 0.002), momentum=0.9, loss_scale=cfg.get("coop_loss_scale", 1024.0), seed=seed,
                           evaluate=lambda: accuracy(model.classify(test_features), test_labels))
    res["test_acc"] = res["epochs"][-1]["test_acc"] if res["epochs"] else res["start_test_acc"]
    model.results = res
    return model
