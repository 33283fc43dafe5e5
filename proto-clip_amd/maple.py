"""MaPLe (multi-modal prompt learning, Khattak et al., CVPR 2023, in the convention of its code base): learned context rows in the text tower at several
depths, a per-depth linear COUPLING FUNCTION that maps each layer's text rows to that layer's visual prompt rows, and both frozen towers trained through in
one step on images — `coop` and `vpt` joined by one fp32 kernel pair:

    text:    prompts = [SOT ; ctx[0] ; class-name tokens ; "." ; EOT ; padding] + positional_embedding            # autograd.PromptEmbedFn (coop's)
             before text block i, 1 <= i < depth:  x[:, 1 : 1 + n_ctx, :] = r16(ctx[i])                           # TowerTailFn's pack with deep_off = 1
    vision:  vctx[d] = ctx[d] @ couple_weight[d].T + couple_bias[d], every depth in one launch                     # autograd.CoupleFn, csrc/pclip_maple.hip
             t' = cat([class ; patches] + pos, r16(vctx[0]));  before vision block i, 1 <= i < depth: the last n_ctx rows = r16(vctx[i])      # vpt's path
    loss  =  cross_entropy(logit_scale.exp() * normalise(image features) @ normalise(text features).T, labels)     # autograd.cosine_cross_entropy

A replaced row passes no gradient to the block below.  The towers are frozen and pay for no parameter gradient; `clip_model.unfreeze(visual_blocks=k,
text_blocks=m)` composes with it.  depth = 1 is CoOp's context with a coupled shallow VPT.

Envelope: transformer towers of head dimension 64, fp32 parameters, 1 <= n_ctx <= 16 (the coupling kernel's rows per depth), 1 <= depth <= min(vision
layers, text layers), L0 + n_ctx <= 288 vision tokens, text width a multiple of 64, context shared by the classes.  Not here: a per-class
(class-specific) context.  PromptSRC's independent prompts and regularisers are `promptsrc.py`; CoCoOp's meta-net (an image-conditioned context) is
`cocoop.py`."""
import torch

from . import autograd as pag
from . import ops
from . import utils
from ._lib import COUPLE_MAX_P, VPT_MAX_L, PclipError
from .coop import PromptLearner
from .prompt_train import accuracy, train_prompts
from .tower import run_tower
from .vpt import VisualPromptLearner


def deep_text_features(who, clip_model, inner, ctx, n_ctx, depth):
    """[N, E] fp16: the class prompts of `inner` (a coop.PromptLearner: its tokens, EOT check and L_eff) with ctx[0] spliced in, through the text tower with
    ctx[i] replacing rows 1 .. n_ctx before block i, 1 <= i < depth.  ctx: fp32 [depth, n_ctx, Wt] on the tape.  The text path of `MultiModalPromptLearner`
    and of `promptsrc.IndependentPromptLearner`, stated once; `who` names the learner in a refusal."""
    m = clip_model
    if m._text_stem_opt_in:
        raise PclipError(f"{who}: the text embeddings have been opted in through unfreeze(stem=...); prompt learning beside a "
                         "trainable stem is not supported (the context rows are spliced into a frozen embedding)")
    taped = False
    if torch.is_grad_enabled():
        tail = m._text_tape_from()                                         # refuses a trainable embedding in the frozen prefix
        taped = ctx.requires_grad or tail is not None
    L = inner.run_length
    emb16 = m._cache.get("tok", m.token_embedding.weight, lambda t: t.half().contiguous())
    pos16 = m._cache.get("pos", m.positional_embedding, lambda t: t.half().contiguous())
    tw = m.text_tower
    deep = ctx[1:] if depth > 1 else None
    what = f"{who} (n_ctx={n_ctx}, depth={depth}, {L} tokens per prompt, text tower on the tape from block 0)"
    with torch.set_grad_enabled(taped):
        outs = []
        for i in range(0, inner.n_cls, m.text_chunk):
            tokens = inner.tokenized_prompts[i:i + m.text_chunk]
            B = tokens.shape[0]
            if ops.splitk_active(B) or ops.splitk_active(B * L):
                raise PclipError(f"{what}: a pass inside ops.low_latency() is not supported (the split-K linears have no backward and the prompted "
                                 f"tower runs the taped kernel sequence); leave the context (B={B}, L={L})")
            head = tokens[:, :L].contiguous()
            x = pag.PromptEmbedFn.apply(ctx[0], tokens, emb16, pos16, n_ctx, L)
            outs.append(run_tower(tw, x, B, L, (0, False), tw.pick(B, L, x.device, head), what=what, deep=deep,
                                  deep_off=None if deep is None else 1))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


class MultiModalPromptLearner(torch.nn.Module):
    """The three learned tensors, all fp32: `ctx` [depth, n_ctx, Wt] (slice 0 from ctx_init's token embeddings when given, as in `coop.PromptLearner`, else
    N(0, 0.02); the deeper slices N(0, 0.02)), `couple_weight` [depth, Wv, Wt] and `couple_bias` [depth, Wv] (nn.Linear's default initialisation per depth,
    from `seed`).  Prompt assembly, the EOT check and the L_eff truncation are coop.PromptLearner's (one is held, unregistered); the vision side is
    vpt.VisualPromptLearner's path with the coupled rows as its explicit `ctx` (one is held, unregistered).  text_features() -> [N, E] fp16,
    image_features(images) -> [B, E] fp16, both with a tape to the parameters (and to whatever of the towers' tails is unfrozen); under torch.no_grad() the
    same kernels without a tape, hence the same bits.  The CLIP model is referenced, not registered: `parameters()` is exactly the three tensors."""

    def __init__(self, classnames, clip_model, n_ctx=2, depth=9, ctx_init=None, tokenize=None, tokenized_prompts=None, truncate=True, seed=1,
                 class_specific=False):
        super().__init__()
        from .clip.model import ModifiedResNet
        who = "MultiModalPromptLearner"
        if class_specific:
            raise PclipError(f"{who}: class_specific contexts are not supported (one context shared by the classes: the coupling function maps n_ctx "
                             "text rows per depth, not n_ctx per class)")
        vis = clip_model.visual
        if isinstance(vis, ModifiedResNet):
            raise PclipError(f"{who}: the ModifiedResNet visual tower has no token sequence to put prompts into and no backward (only the transformer towers)")
        Wv, Wt = vis.width, clip_model.transformer.width
        if Wv % 8 != 0 or Wv != 64 * vis.heads:
            raise PclipError(f"{who}: vision tower of width {Wv} with {vis.heads} heads (head dimension 64 only)")
        if Wt % 8 != 0 or Wt != 64 * clip_model.transformer_heads:
            raise PclipError(f"{who}: text tower of width {Wt} with {clip_model.transformer_heads} heads (head dimension 64 only)")
        layers = min(len(vis.transformer.resblocks), len(clip_model.transformer.resblocks))
        depth = int(depth)
        if not 1 <= depth <= layers:
            raise PclipError(f"{who}: depth={depth} outside 1..{layers} (the shorter tower has {layers} layers)")
        L0 = (vis.input_resolution // vis.patch_size) ** 2 + 1

        def check_rows(n):
            if not 1 <= n <= COUPLE_MAX_P:
                raise PclipError(f"{who}: n_ctx={n} outside 1..{COUPLE_MAX_P} (the coupling kernel maps at most {COUPLE_MAX_P} rows per depth)")
            if L0 + n > VPT_MAX_L:
                raise PclipError(f"{who}: L0 + n_ctx = {L0} + {n} = {L0 + n} vision tokens exceed the attention envelope of {VPT_MAX_L} "
                                 f"(this tower has room for {max(0, VPT_MAX_L - L0)} prompt rows)")

        if ctx_init is None:
            check_rows(int(n_ctx))
        inner = PromptLearner(classnames, clip_model, n_ctx=n_ctx, ctx_init=ctx_init, tokenize=tokenize, tokenized_prompts=tokenized_prompts,
                              truncate=truncate, seed=seed)                     # assembly, EOT check, L_eff: coop's, not forked
        n_ctx = inner.n_ctx                                                     # ctx_init decides it when given
        check_rows(n_ctx)
        device = inner.ctx.device
        g = torch.Generator().manual_seed(seed + 1)
        rows = torch.cat([inner.ctx.detach()[None].cpu(), torch.randn(depth - 1, n_ctx, Wt, generator=g) * 0.02], 0)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            linears = [torch.nn.Linear(Wt, Wv) for _ in range(depth)]          # nn.Linear's default initialisation, per depth
        self.n_ctx, self.depth, self.n_cls = n_ctx, depth, inner.n_cls
        self.classnames = inner.classnames
        self.ctx = torch.nn.Parameter(rows.to(device).contiguous())
        self.couple_weight = torch.nn.Parameter(torch.stack([m.weight.detach() for m in linears]).to(device).contiguous())
        self.couple_bias = torch.nn.Parameter(torch.stack([m.bias.detach() for m in linears]).to(device).contiguous())
        object.__setattr__(self, "clip_model", clip_model)
        object.__setattr__(self, "_text", inner)
        object.__setattr__(self, "_vision", VisualPromptLearner(clip_model, n_ctx=n_ctx, depth=depth, seed=seed))

    @property
    def run_length(self) -> int:
        """Tokens per prompt the text tower runs at: L_eff with `truncate`, else the context length."""
        return self._text.run_length

    @property
    def truncate(self) -> bool:
        return self._text.truncate

    @truncate.setter
    def truncate(self, value):
        self._text.truncate = bool(value)

    def _check_parameters(self):
        for name in ("ctx", "couple_weight", "couple_bias"):
            p = getattr(self, name)
            if p.dtype != torch.float32:
                raise PclipError(f"MultiModalPromptLearner: {name} must be torch.float32, got {p.dtype} (the prompts, the coupling function and their "
                                 "gradients are fp32; the kernels round the rows to fp16 where they enter the stream)")

    def text_features(self):
        """[N, E] fp16: the class prompts with ctx[0] spliced in, through the text tower with ctx[i] replacing rows 1 .. n_ctx before block i."""
        self._check_parameters()
        return deep_text_features("MultiModalPromptLearner", self.clip_model, self._text, self.ctx, self.n_ctx, self.depth)

    def visual_rows(self):
        """[depth, n_ctx, Wv] fp32: the coupling function of every depth, one launch."""
        self._check_parameters()
        return pag.CoupleFn.apply(self.ctx, self.couple_weight, self.couple_bias)

    def image_features(self, images):
        """[B, E] fp16: the coupled rows as visual prompts (vpt's path with an explicit `ctx`)."""
        return self._vision(images, ctx=self.visual_rows())

    def forward(self, images):
        return self.image_features(images), self.text_features()


class MaPLe(torch.nn.Module):
    """A CLIP model's temperature with a `MultiModalPromptLearner`'s image and text features: the training loss on images and the classifier."""

    def __init__(self, clip_model, learner):
        super().__init__()
        self.learner = learner
        object.__setattr__(self, "clip_model", clip_model)

    def logit_scale(self):
        return self.clip_model.logit_scale.float().exp()

    def forward(self, images):
        return self.learner(images)

    def loss(self, images, labels):
        """Cross-entropy of logit_scale.exp() * normalise(image features) @ normalise(text features)^T against `labels`, both operands on the tape; the
        [B, N] logits are never written."""
        feats, text = self.learner.image_features(images), self.learner.text_features()
        return pag.cosine_cross_entropy(feats, text, self.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)

    def text_rows(self):
        """The learned classifier: L2-normalised text features [N, E] fp16, a constant."""
        with torch.no_grad():
            return ops.l2norm_rows(self.learner.text_features())

    def classify(self, images, topk=0):
        """arg-max class (int64 [B]) of the prompted image features against the learned rows, through the fused arg-max of the cosine-logit kernel; with
        topk > 0 also the top-k values and indices, as `utils.clip_zero_shot` returns them."""
        with torch.no_grad():
            feats = ops.l2norm_rows(self.learner.image_features(images))
            return utils.clip_zero_shot(feats, self.text_rows(), scale=float(self.logit_scale()), topk=topk, layout="nd")


def run_maple(cfg, train_images, train_labels, classnames, clip_model, test_images=None, test_labels=None, learner=None, tokenize=None,
              tokenized_prompts=None):
    """Train multi-modal prompts on pre-processed image tensors ([Q, 3, R, R]) and labels with the recipe of MaPLe's code base: SGD on the three tensors,
    learning rate 0.0035, momentum 0.9, cosine schedule, batches of 4, cfg['maple_epochs'] epochs, cfg['n_ctx'] (default 2) rows at cfg['maple_depth']
    (default 9) layers (optional keys: 'ctx_init', 'maple_lr', 'maple_batch', 'maple_loss_scale', 'maple_momentum', 'seed').  The loss goes through
    torch's GradScaler (initial scale 1024) for the reason DESIGN records for CoOp and VPT: the gradient stream inside the towers is fp16; the parameters
    and their gradients are fp32, so the scaler and the optimizer are torch's own.  Returns (learner, per-epoch mean losses); with test images the accuracy
    is printed before training and after every epoch and kept in `learner.results`.  learner: a `MultiModalPromptLearner` of this model to go on training."""
    seed = int(cfg.get("seed", 1))
    if cfg.get("class_specific", False):
        raise PclipError("run_maple: class_specific contexts are not supported (one context shared by the classes)")
    if learner is None:
        learner = MultiModalPromptLearner(classnames, clip_model, n_ctx=cfg.get("n_ctx", 2), depth=cfg.get("maple_depth", 9), ctx_init=cfg.get("ctx_init"),
                                          tokenize=tokenize, tokenized_prompts=tokenized_prompts, seed=seed)
    elif learner.clip_model is not clip_model:
        raise PclipError("run_maple: the learner belongs to another CLIP model")
    model = MaPLe(clip_model, learner)
    labels = train_labels.to(train_images.device).long()
    evaluate = None if test_images is None else lambda: accuracy(model.classify(test_images), test_labels)
    learner.results, epoch_losses = train_prompts(
        "MaPLe", learner.parameters(), lambda idx: model.loss(train_images[idx].contiguous(), labels[idx]), train_images.shape[0], train_images.device,
        epochs=int(cfg["maple_epochs"]), batch=int(cfg.get("maple_batch", 4)), lr=cfg.get("maple_lr", 0.0035), momentum=cfg.get("maple_momentum", 0.9),
        loss_scale=cfg.get("maple_loss_scale", 1024.0), seed=seed, evaluate=evaluate)
    return learner, epoch_losses
