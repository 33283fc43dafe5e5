"""Visual Prompt Tuning (VPT, Jia et al. 2022, in the convention of the CLIP prompt-learning code bases — the `VPT` trainer, the vision side of MaPLe): a
few fp32 token rows are put into the image tower's sequence and trained by gradient descent through the FROZEN vision tower; the vision-side counterpart
of `coop`.  The prompts sit at the END of the sequence — the class token stays row 0, the patch rows stay where the stem writes them:

    t    = [class ; patches] + positional_embedding                                    # [B, L0, W], the frozen stem
    t'   = cat(t, r16(ctx[0]) broadcast over the batch)                                # [B, L, W], L = L0 + P; csrc/pclip_vpt.hip, no positional embedding
    x    = ln_pre(t')                                                                  # autograd.VptEmbedFn
    for i in 0 .. layers - 1:
        if 1 <= i < depth:  x[:, L0:L, :] = r16(ctx[i])                                # deep: the last P rows REPLACED, raw, before block i's ln_1
        x = block_i(x)                                                                 # autograd.TowerTailFn from block 0, with its deep-prompt pack
    features = ln_post(x[:, 0, :]) @ proj

depth = 1 is VPT-shallow, depth = layers VPT-deep.  The gradient of a replaced row goes to ctx[i] alone, not to the block below.  A frozen tower pays for
no parameter gradient; `clip_model.unfreeze(visual_blocks=k)` composes with it: the last k blocks and the heads then train beside the prompts.

Envelope: transformer towers of head dimension 64, fp32 `ctx`, L0 + P <= 288 tokens (ViT-B/16: P <= 91, ViT-B/32: P <= 238, ViT-L/14: P <= 31; the 336-px
tower has 577 tokens of its own and is refused).  Not here: prompts directly behind the class token (Jia et al.'s order), a positional embedding on the
prompts, VPT beside a trainable stem (`unfreeze(stem=...)`).  MaPLe's coupling function lives in `maple.py`; an explicit `ctx` tensor on the tape is all
it needs from this module."""
import torch

from . import autograd as pag
from . import ops
from . import utils
from ._lib import PclipError, VPT_MAX_L
from .prompt_train import accuracy, train_prompts
from .tower import run_tower, vit_stem


class VisualPromptLearner(torch.nn.Module):
    """The learned visual prompts.  `ctx` is the one parameter: fp32 [depth, n_ctx, W], N(0, init_std) rows from `seed`.  forward(images, ctx=None) ->
    image features [B, E] fp16 with a tape to `ctx` (and to whatever of the vision tower's tail is unfrozen); under torch.no_grad() the same kernels
    without a tape, hence the same bits.  An explicit `ctx` tensor (fp32 [depth, n_ctx, W], e.g. a function of another module's parameters) stands in for
    the parameter.  Images run in chunks of `clip_model.visual.chunk`.  The CLIP model is referenced, not registered: `parameters()` is `ctx` alone."""

    def __init__(self, clip_model, n_ctx=8, depth=1, seed=1, init_std=0.02):
        super().__init__()
        from .clip.model import ModifiedResNet
        vis = clip_model.visual
        if isinstance(vis, ModifiedResNet):
            raise PclipError("VisualPromptLearner: the ModifiedResNet visual tower has no token sequence to put prompts into and no backward "
                             "(only the transformer towers)")
        W, layers = vis.width, len(vis.transformer.resblocks)
        if W % 8 != 0 or W != 64 * vis.heads:
            raise PclipError(f"VisualPromptLearner: vision tower of width {W} with {vis.heads} heads (head dimension 64 only)")
        n_ctx, depth = int(n_ctx), int(depth)
        if n_ctx < 1:
            raise PclipError(f"VisualPromptLearner: n_ctx={n_ctx} must be at least 1")
        L0 = (vis.input_resolution // vis.patch_size) ** 2 + 1
        if L0 + n_ctx > VPT_MAX_L:
            raise PclipError(f"VisualPromptLearner: L0 + n_ctx = {L0} + {n_ctx} = {L0 + n_ctx} tokens exceed the attention envelope of {VPT_MAX_L} "
                             f"(this tower has room for {max(0, VPT_MAX_L - L0)} prompt rows)")
        if not 1 <= depth <= layers:
            raise PclipError(f"VisualPromptLearner: depth={depth} outside 1..{layers} (1: shallow, {layers}: deep)")
        g = torch.Generator().manual_seed(seed)
        rows = (torch.randn(depth, n_ctx, W, generator=g) * float(init_std)).to(vis.proj.device)
        self.n_ctx, self.depth, self.l0 = n_ctx, depth, L0
        self.ctx = torch.nn.Parameter(rows.contiguous())
        object.__setattr__(self, "clip_model", clip_model)

    @property
    def run_length(self) -> int:
        """Tokens per image the tower runs at: L0 + n_ctx."""
        return self.l0 + self.n_ctx

    def forward(self, images, ctx=None):
        vis = self.clip_model.visual
        ctx = self.ctx if ctx is None else ctx
        W = vis.width
        if not isinstance(ctx, torch.Tensor) or ctx.dtype != torch.float32:
            raise PclipError(f"VisualPromptLearner: ctx must be torch.float32, got {getattr(ctx, 'dtype', type(ctx))} (the prompts and their gradient "
                             "are fp32; the kernels round them to fp16 where they enter the stream)")
        if tuple(ctx.shape) != (self.depth, self.n_ctx, W):
            raise PclipError(f"VisualPromptLearner: ctx {tuple(ctx.shape)} is not [depth, n_ctx, W] = [{self.depth}, {self.n_ctx}, {W}]")
        R = vis.input_resolution
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != R or images.shape[3] != R:
            raise PclipError(f"expected images [B,3,{R},{R}], got {tuple(images.shape)}")
        if vis._stem_opt_in:
            raise PclipError("VisualPromptLearner: the visual stem has been opted in through unfreeze(stem=...); visual prompt tuning beside a trainable "
                             "stem is not supported (the prompt rows are spliced behind a frozen stem)")
        taped = False
        if torch.is_grad_enabled():
            tail = vis._tape_from()                                            # refuses a trainable parameter in the frozen prefix
            taped = ctx.requires_grad or tail is not None                      # the prompts, or something of the tower's blocks / heads, train
        with torch.set_grad_enabled(taped):
            outs = [self._chunk(ctx, images[i:i + vis.chunk]) for i in range(0, images.shape[0], vis.chunk)]
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _chunk(self, ctx, img):
        vis = self.clip_model.visual
        B, L0, L = img.shape[0], self.l0, self.run_length
        if img.dtype not in (torch.float32, torch.float16):
            raise PclipError(f"unsupported image dtype {img.dtype}")
        what = f"VisualPromptLearner (n_ctx={self.n_ctx}, depth={self.depth}, {L} tokens per image, visual tower on the tape from block 0)"
        if ops.splitk_active(B) or ops.splitk_active(B * L):
            raise PclipError(f"{what}: a pass inside ops.low_latency() is not supported (the split-K linears have no backward and the prompted tower "
                             f"runs the taped kernel sequence); leave the context (B={B}, L={L})")
        with torch.no_grad():                                                  # the frozen stem: a constant (clip/model.py:222-226)
            t = vit_stem(vis._cache, img.contiguous(), vis.conv1.weight, vis.class_embedding, vis.positional_embedding, vis.patch_size)
        x = pag.VptEmbedFn.apply(ctx[0], t, vis.ln_pre.weight, vis.ln_pre.bias, B, L0)
        deep = ctx[1:] if self.depth > 1 else None
        return run_tower(vis.tower, x, B, L, (0, False), vis.tower.pick(B, L, x.device), what=what, deep=deep)


class VPT(torch.nn.Module):
    """A CLIP model's temperature with a `VisualPromptLearner`'s image features against fixed class weights (`utils.clip_classifier`'s [D, N], or [N, D]
    rows): the training loss and the classifier."""

    def __init__(self, clip_model, learner):
        super().__init__()
        self.learner = learner
        object.__setattr__(self, "clip_model", clip_model)

    def logit_scale(self):
        return self.clip_model.logit_scale.float().exp()

    def forward(self, images):
        return self.learner(images)

    def loss(self, images, clip_weights, labels, layout=None):
        """Cross-entropy of logit_scale.exp() * normalise(features) @ normalise(class rows)^T against `labels`; the [B, N] logits are never written."""
        feats = self.learner(images)
        rows = utils._clip_weight_rows(feats, clip_weights, layout, taped=True)
        return pag.cosine_cross_entropy(feats, rows, self.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)

    def classify(self, images, clip_weights, topk=0, layout=None):
        """arg-max class (int64 [B]) of the prompted features, through the fused arg-max of the cosine-logit kernel; with topk > 0 also the top-k values and
        indices, as `utils.clip_zero_shot` returns them."""
        with torch.no_grad():
            feats = ops.l2norm_rows(self.learner(images))
            rows = ops.l2norm_rows(utils._clip_weight_rows(feats, clip_weights, layout).contiguous())
            return utils.clip_zero_shot(feats, rows, scale=float(self.logit_scale()), topk=topk, layout="nd")


def run_vpt(cfg, train_images, train_labels, clip_weights, clip_model, test_images=None, test_labels=None, learner=None):
    """Train visual prompts on pre-processed image tensors ([Q, 3, R, R]) and labels against fixed class weights, with the optimiser and schedule choices
    of `coop.run_coop`: SGD on `ctx`, learning rate 0.002, momentum 0.9, cosine schedule, batches of 32, cfg['vpt_epochs'] epochs, cfg['n_ctx'] prompt
    rows at cfg['vpt_depth'] layers (optional keys: 'vpt_lr', 'vpt_batch', 'vpt_loss_scale', 'vpt_momentum', 'vpt_init_std', 'seed').  The loss goes
    through torch's GradScaler (initial scale 1024) for the reason DESIGN records for CoOp: the gradient stream inside the tower is fp16, and an unscaled
    mean loss leaves it in fp16's subnormal range; `ctx` and its gradient are fp32, so the scaler and the optimizer are torch's own.  Returns
    (learner, per-epoch mean losses); with test images the accuracy is printed before training and after every epoch and kept in `learner.results`.
    learner: a `VisualPromptLearner` of this model to go on training (its n_ctx and depth hold) instead of a fresh one."""
    seed = int(cfg.get("seed", 1))
    if learner is None:
        learner = VisualPromptLearner(clip_model, n_ctx=cfg.get("n_ctx", 8), depth=cfg.get("vpt_depth", 1), seed=seed, init_std=cfg.get("vpt_init_std", 0.02))
    elif learner.clip_model is not clip_model:
        raise PclipError("run_vpt: the learner belongs to another CLIP model")
    model = VPT(clip_model, learner)
    labels = train_labels.to(train_images.device).long()
    evaluate = None if test_images is None else lambda: accuracy(model.classify(test_images, clip_weights), test_labels)
    learner.results, epoch_losses = train_prompts(
        "VPT", learner.parameters(), lambda idx: model.loss(train_images[idx].contiguous(), clip_weights, labels[idx]), train_images.shape[0],
        train_images.device, epochs=int(cfg["vpt_epochs"]), batch=int(cfg.get("vpt_batch", 32)), lr=cfg.get("vpt_lr", 0.002),
        momentum=cfg.get("vpt_momentum", 0.9), loss_scale=cfg.get("vpt_loss_scale", 1024.0), seed=seed, evaluate=evaluate)
    return learner, epoch_losses
