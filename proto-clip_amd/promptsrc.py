"""PromptSRC (self-regulated prompts, Khattak et al., ICCV 2023, in the convention of its code base): independent deep prompts in both towers ("IVLP"), held
to the frozen model by three regularisers, and aggregated over the epochs with Gaussian weights:

    text:    the path of `maple` — ctx[0] spliced behind SOT, ctx[i] replacing rows 1 .. n_ctx_text before text block i            # maple.deep_text_features
    vision:  the path of `vpt` with vctx as its prompts — vctx[0] appended behind the patch rows, vctx[i] replacing them before block i
    loss  =  cross_entropy(logit_scale.exp() * normalise(img) @ normalise(txt).T, labels)                                          # autograd.cosine_cross_entropy
           + w_text   * l1_loss(normalise(txt), fixed_text)                                    # autograd.feature_reg, csrc/pclip_feature_reg.hip
           + w_image  * l1_loss(normalise(img), normalise(frozen tower's features of the same images))
           + w_logits / N * mean_b KL(softmax(zero-shot logits) || softmax(own logits))        # autograd.cosine_kd; upstream's kl_div(sum) / logits.numel()
    fixed_text = normalise(mean over the templates of the UN-normalised frozen text features)  # `frozen_text_features`
    zero-shot logits = logit_scale.exp() * normalise(frozen image features) @ fixed_text.T
    after epoch e (1-based):  acc += w_e * parameter,  w = a Gaussian over the epochs normalised to sum 1; after the last epoch the parameters ARE acc.

Unlike MaPLe the two sets of prompts are separate parameters with their own row counts and depths, and no coupling function.  The teacher is the
pre-trained model itself, so the method is refused while anything of the towers trains.  One frozen and one prompted vision pass per step, one prompted text
pass; no [B, N] matrix and no fp16 rounding of a normalised row on the way to any of the four terms.

Envelope: `maple`'s without the coupling function's limit on the text rows — transformer towers of head dimension 64, fp32 parameters, 1 <= depth_text <=
text layers, 1 <= depth_vision <= vision layers, L0 + n_ctx_vision <= 288 vision tokens, context shared by the classes.  Not here: upstream's list of 60
templates (the caller passes templates), a per-class context."""
import numpy as np
import torch

from . import autograd as pag
from . import ops
from . import utils
from ._lib import VPT_MAX_L, PclipError
from .coop import PromptLearner
from .maple import deep_text_features
from .prompt_train import accuracy, train_prompts
from .vpt import VisualPromptLearner


class IndependentPromptLearner(torch.nn.Module):
    """The two learned tensors, both fp32: `ctx` [depth_text, n_ctx_text, Wt] (slice 0 from ctx_init's token embeddings when given, as in
    `coop.PromptLearner`, else N(0, 0.02); the deeper slices N(0, 0.02)) and `vctx` [depth_vision, n_ctx_vision, Wv] (N(0, 0.02), `vpt`'s initialisation).
    Prompt assembly, the EOT check and the L_eff truncation are coop.PromptLearner's, the text path is `maple.deep_text_features`, the vision path is
    vpt.VisualPromptLearner's with `vctx` as its explicit `ctx` (one of each is held, unregistered).  text_features() -> [N, E] fp16,
    image_features(images) -> [B, E] fp16, both with a tape to the parameters; under torch.no_grad() the same kernels without a tape, hence the same bits.
    The CLIP model is referenced, not registered: `parameters()` is exactly the two tensors."""

    def __init__(self, classnames, clip_model, n_ctx_text=4, n_ctx_vision=4, depth_text=9, depth_vision=9, ctx_init=None, tokenize=None,
                 tokenized_prompts=None, truncate=True, seed=1, class_specific=False):
        super().__init__()
        from .clip.model import ModifiedResNet
        who = "IndependentPromptLearner"
        if class_specific:
            raise PclipError(f"{who}: class_specific contexts are not supported (one context shared by the classes)")
        vis = clip_model.visual
        if isinstance(vis, ModifiedResNet):
            raise PclipError(f"{who}: the ModifiedResNet visual tower has no token sequence to put prompts into and no backward (only the transformer towers)")
        Wv, Wt = vis.width, clip_model.transformer.width
        if Wv % 8 != 0 or Wv != 64 * vis.heads:
            raise PclipError(f"{who}: vision tower of width {Wv} with {vis.heads} heads (head dimension 64 only)")
        if Wt % 8 != 0 or Wt != 64 * clip_model.transformer_heads:
            raise PclipError(f"{who}: text tower of width {Wt} with {clip_model.transformer_heads} heads (head dimension 64 only)")
        depth_text, depth_vision, n_ctx_vision = int(depth_text), int(depth_vision), int(n_ctx_vision)
        for side, depth, layers in (("text", depth_text, len(clip_model.transformer.resblocks)), ("vision", depth_vision, len(vis.transformer.resblocks))):
            if not 1 <= depth <= layers:
                raise PclipError(f"{who}: depth_{side}={depth} outside 1..{layers} (the {side} tower has {layers} layers)")
        L0 = (vis.input_resolution // vis.patch_size) ** 2 + 1
        if n_ctx_vision < 1:
            raise PclipError(f"{who}: n_ctx_vision={n_ctx_vision} must be at least 1")
        if L0 + n_ctx_vision > VPT_MAX_L:
            raise PclipError(f"{who}: L0 + n_ctx_vision = {L0} + {n_ctx_vision} = {L0 + n_ctx_vision} vision tokens exceed the attention envelope of "
                             f"{VPT_MAX_L} (this tower has room for {max(0, VPT_MAX_L - L0)} prompt rows)")
        inner = PromptLearner(classnames, clip_model, n_ctx=n_ctx_text, ctx_init=ctx_init, tokenize=tokenize, tokenized_prompts=tokenized_prompts,
                              truncate=truncate, seed=seed)                     # assembly, EOT check, L_eff: coop's, not forked
        n_ctx_text = inner.n_ctx                                                # ctx_init decides it when given
        vision = VisualPromptLearner(clip_model, n_ctx=n_ctx_vision, depth=depth_vision, seed=seed)
        device = inner.ctx.device
        g = torch.Generator().manual_seed(seed + 1)
        rows = torch.cat([inner.ctx.detach()[None].cpu(), torch.randn(depth_text - 1, n_ctx_text, Wt, generator=g) * 0.02], 0)
        self.n_ctx_text, self.n_ctx_vision, self.depth_text, self.depth_vision, self.n_cls = n_ctx_text, n_ctx_vision, depth_text, depth_vision, inner.n_cls
        self.classnames = inner.classnames
        self.ctx = torch.nn.Parameter(rows.to(device).contiguous())
        self.vctx = torch.nn.Parameter(vision.ctx.detach().clone().to(device).contiguous())
        object.__setattr__(self, "clip_model", clip_model)
        object.__setattr__(self, "_text", inner)
        object.__setattr__(self, "_vision", vision)

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
        for name in ("ctx", "vctx"):
            p = getattr(self, name)
            if p.dtype != torch.float32:
                raise PclipError(f"IndependentPromptLearner: {name} must be torch.float32, got {p.dtype} (the prompts and their gradients are fp32; the "
                                 "kernels round the rows to fp16 where they enter the stream)")

    def text_features(self):
        """[N, E] fp16: the class prompts with ctx[0] spliced in, through the text tower with ctx[i] replacing rows 1 .. n_ctx_text before block i."""
        self._check_parameters()
        return deep_text_features("IndependentPromptLearner", self.clip_model, self._text, self.ctx, self.n_ctx_text, self.depth_text)

    def image_features(self, images):
        """[B, E] fp16: vctx as visual prompts (vpt's path with an explicit `ctx`)."""
        self._check_parameters()
        return self._vision(images, ctx=self.vctx)

    def forward(self, images):
        return self.image_features(images), self.text_features()


def frozen_text_features(classnames, templates, clip_model, tokenize=None):
    """PromptSRC's text target, [N, E] fp16: per class the mean over `templates` of the frozen text tower's UN-normalised features, then one normalisation —
    not `utils.clip_classifier`'s normalise, mean, normalise.  A constant, computed once: the mean and the normalisation stay fp32 (ops.l2norm_rows_f32) and
    the result is rounded to fp16 ONCE.  The prototype kernel without its per-row normalisation (ops.proto_build(per_shot_norm=False)) has the right
    convention but three fp16 roundings — the mean, the norm, the quotient — and the L1 term's gradient is the SIGN of normalise(txt) - target: every
    rounding of the target moves signs where the two are close."""
    if tokenize is None:
        from .clip import tokenize
    templates = list(templates)
    N, T = len(classnames), len(templates)
    if not T or not N:
        raise PclipError(f"frozen_text_features: {N} class names and {T} templates (at least one of each)")
    texts = [t.format(c.replace("_", " ")) for c in classnames for t in templates]
    with torch.no_grad():
        emb = clip_model.encode_text(tokenize(texts).to(clip_model.text_projection.device))       # [N * T, E] fp16, class-major
        mean = emb.float().view(N, T, emb.shape[1]).mean(dim=1).contiguous()                       # fp32; a setup-time constant, not a step's work
        return ops.cast_f16(ops.l2norm_rows_f32(mean))


class PromptSRC(torch.nn.Module):
    """A CLIP model's temperature with an `IndependentPromptLearner`'s features and the frozen model as their teacher: the four-term training loss on images
    and the classifier.  fixed_text [N, E] fp16: `frozen_text_features`' rows (L2-normalised already; taken as they are)."""

    def __init__(self, clip_model, learner, fixed_text):
        super().__init__()
        if not isinstance(fixed_text, torch.Tensor) or fixed_text.dtype != torch.float16 or fixed_text.dim() != 2:
            raise PclipError(f"PromptSRC: fixed_text must be a 2-D float16 tensor [N, E], got {getattr(fixed_text, 'dtype', type(fixed_text))}")
        if fixed_text.shape[0] != learner.n_cls:
            raise PclipError(f"PromptSRC: fixed_text has {fixed_text.shape[0]} rows, the prompt learner {learner.n_cls} classes")
        if fixed_text.requires_grad:
            raise PclipError("PromptSRC: fixed_text requires grad, but the teacher is frozen")
        if learner.clip_model is not clip_model:
            raise PclipError("PromptSRC: the learner belongs to another CLIP model")
        self.learner = learner
        self.register_buffer("fixed_text", fixed_text.detach().contiguous(), persistent=False)
        object.__setattr__(self, "clip_model", clip_model)

    def logit_scale(self):
        return self.clip_model.logit_scale.float().exp()

    def forward(self, images):
        return self.learner(images)

    def _check_frozen(self):
        m = self.clip_model
        if m.visual._stem_opt_in or m._text_stem_opt_in:
            raise PclipError("PromptSRC: a tower's stem has been opted in through unfreeze(stem=...), but the teacher of the regularisers is the frozen "
                             "pre-trained model: PromptSRC trains prompts only")
        for name, p in m.named_parameters():
            if p.requires_grad:
                raise PclipError(f"PromptSRC: parameter {name} requires grad (unfreeze), but the teacher of the regularisers is the frozen pre-trained "
                                 "model: PromptSRC trains prompts only")

    def frozen_image_features(self, images):
        """[B, E] fp16: the frozen vision tower's un-normalised features of `images`, a constant (what `loss` computes unless it is handed cached ones)."""
        with torch.no_grad():
            return self.clip_model.encode_image(images)

    def loss_terms(self, images, labels, zs_image_features=None, want=(True, True, True, True)):
        """The four UN-weighted terms (cross-entropy, text L1, image L1, batch-mean KL) from one prompted pass of each tower and one frozen vision pass
        (none with `zs_image_features` [B, E] fp16, the frozen tower's features of the same images, un-normalised or not).  want: a term that is not
        wanted is None and costs nothing — the frozen pass runs only if the image or the logit term is."""
        self._check_frozen()
        if zs_image_features is not None and zs_image_features.requires_grad:
            raise PclipError("PromptSRC: zs_image_features requires grad, but the teacher is frozen (pass zs_image_features.detach() to say so)")
        img, txt = self.learner.image_features(images), self.learner.text_features()
        scale = self.logit_scale()
        zs = zs_image_features
        if zs is None and (want[2] or want[3]):
            zs = self.frozen_image_features(images)
        ce = pag.cosine_cross_entropy(img, txt, scale, labels=labels, normalize_a=True, normalize_b=True) if want[0] else None
        l_text = pag.feature_reg(txt, self.fixed_text, "l1", False) if want[1] else None
        l_image = pag.feature_reg(img, zs, "l1", True) if want[2] else None
        kd = None
        if want[3]:
            kd = pag.cosine_kd(img, txt, scale, zs, self.fixed_text, float(scale.detach()), normalize_a=True, normalize_b=True, normalize_teacher_a=True,
                               normalize_teacher_b=False)
        return ce, l_text, l_image, kd

    def combine(self, terms, w_text=25.0, w_image=10.0, w_logits=1.0):
        """ce + w_text * text + w_image * image + (w_logits / N) * kd, in this order, over the terms that are there."""
        ce, l_text, l_image, kd = terms
        total = ce
        if l_text is not None:
            total = total + float(w_text) * l_text
        if l_image is not None:
            total = total + float(w_image) * l_image
        if kd is not None:
            total = total + (float(w_logits) / self.learner.n_cls) * kd
        return total

    def loss(self, images, labels, zs_image_features=None, w_text=25.0, w_image=10.0, w_logits=1.0):
        """The weighted sum of `loss_terms` (`combine`); a term whose weight is 0 is not computed, so it contributes nothing — not even a +0 — to any
        gradient."""
        want = (True, float(w_text) != 0.0, float(w_image) != 0.0, float(w_logits) != 0.0)
        return self.combine(self.loss_terms(images, labels, zs_image_features, want), w_text, w_image, w_logits)

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


def gpa_weights(epochs, mean, std):
    """float64 [epochs]: a Gaussian of `mean` and `std` at the epochs 1 .. epochs, normalised to sum 1 (upstream's get_gauss).  Formed relative to its
    largest value, so a mean far outside the epochs does not underflow to 0 / 0."""
    epochs, mean, std = int(epochs), float(mean), float(std)
    if epochs < 1:
        raise PclipError(f"gpa_weights: epochs={epochs} must be at least 1")
    if not (std > 0.0 and np.isfinite(std) and np.isfinite(mean)):
        raise PclipError(f"gpa_weights: mean={mean} must be finite and std={std} positive and finite")
    e = -0.5 * ((np.arange(1, epochs + 1, dtype=np.float64) - mean) / std) ** 2
    w = np.exp(e - e.max())
    return w / w.sum()


class GaussianAggregate:
    """PromptSRC's aggregate of the parameters over the epochs: add() after every epoch does acc += w_e * parameter in fp32 (one accumulator per
    tensor, from +0, epochs in order), finish_() copies acc into the parameters.  On a term's path: the rounding of w_e to fp32, the product (fused into
    the addition or not) and at most `epochs` additions, the first of them exact."""

    def __init__(self, parameters, weights):
        self.parameters = list(parameters)
        self.weights = np.asarray(weights, dtype=np.float64)
        self.acc = [torch.zeros_like(p, dtype=torch.float32) for p in self.parameters]
        self.epoch = 0

    def add(self):
        if self.epoch >= len(self.weights):
            raise PclipError(f"GaussianAggregate: add() after all {len(self.weights)} epochs")
        w = float(self.weights[self.epoch])
        with torch.no_grad():
            for a, p in zip(self.acc, self.parameters):
                a.add_(p.detach().float(), alpha=w)
        self.epoch += 1

    def finish_(self):
        if self.epoch != len(self.weights):
            raise PclipError(f"GaussianAggregate: finish_() after {self.epoch} of {len(self.weights)} epochs")
        with torch.no_grad():
            for a, p in zip(self.acc, self.parameters):
                p.copy_(a)


def run_promptsrc(cfg, train_images, train_labels, classnames, templates, clip_model, test_images=None, test_labels=None, learner=None, tokenize=None,
                  tokenized_prompts=None, fixed_text=None, snapshots=None):
    """Train independent prompts on pre-processed image tensors ([Q, 3, R, R]) and labels with the recipe of PromptSRC's code base: SGD on the two tensors,
    learning rate 0.0025, momentum 0.9, cosine schedule, batches of 4, cfg['promptsrc_epochs'] epochs; cfg['n_ctx_text'] / cfg['n_ctx_vision'] (default 4)
    rows at cfg['depth_text'] / cfg['depth_vision'] (default 9) layers; the weights cfg['w_text'] (25), cfg['w_image'] (10), cfg['w_logits'] (1); the
    Gaussian aggregation cfg['gpa_mean'] (15), cfg['gpa_std'] (1) (other optional keys: 'ctx_init', 'promptsrc_lr', 'promptsrc_batch',
    'promptsrc_loss_scale', 'promptsrc_momentum', 'seed').  After every epoch acc += w_e * parameter in fp32, and after the last the parameters are set to
    acc — before that epoch's evaluation, so the last accuracy is the aggregate's.  The loss goes through torch's GradScaler (initial scale 1024) for the
    reason DESIGN records for CoOp and VPT.  fixed_text: the text target [N, E] fp16, default `frozen_text_features(classnames, templates, ...)`.
    snapshots: a list that receives, per epoch, clones of (ctx, vctx) as they were aggregated.  Returns (learner, per-epoch mean losses); with test
    images the accuracy is printed before training and after every epoch and kept in `learner.results`."""
    seed = int(cfg.get("seed", 1))
    if cfg.get("class_specific", False):
        raise PclipError("run_promptsrc: class_specific contexts are not supported (one context shared by the classes)")
    epochs = int(cfg["promptsrc_epochs"])
    weights = gpa_weights(epochs, cfg.get("gpa_mean", 15), cfg.get("gpa_std", 1))
    if learner is None:
        learner = IndependentPromptLearner(classnames, clip_model, n_ctx_text=cfg.get("n_ctx_text", 4), n_ctx_vision=cfg.get("n_ctx_vision", 4),
                                           depth_text=cfg.get("depth_text", 9), depth_vision=cfg.get("depth_vision", 9), ctx_init=cfg.get("ctx_init"),
                                           tokenize=tokenize, tokenized_prompts=tokenized_prompts, seed=seed)
    elif learner.clip_model is not clip_model:
        raise PclipError("run_promptsrc: the learner belongs to another CLIP model")
    if fixed_text is None:
        fixed_text = frozen_text_features(classnames, templates, clip_model, tokenize)
    model = PromptSRC(clip_model, learner, fixed_text)
    model._check_frozen()
    w = dict(w_text=cfg.get("w_text", 25.0), w_image=cfg.get("w_image", 10.0), w_logits=cfg.get("w_logits", 1.0))
    labels = train_labels.to(train_images.device).long()
    aggregate = GaussianAggregate([learner.ctx, learner.vctx], weights)

    def on_epoch_end(epoch):
        if snapshots is not None:
            snapshots.append((learner.ctx.detach().clone(), learner.vctx.detach().clone()))
        aggregate.add()
        if epoch == epochs - 1:
            aggregate.finish_()

    evaluate = None if test_images is None else lambda: accuracy(model.classify(test_images), test_labels)
    learner.results, epoch_losses = train_prompts(
        "PromptSRC", learner.parameters(), lambda idx: model.loss(train_images[idx].contiguous(), labels[idx], **w), train_images.shape[0],
        train_images.device, epochs=epochs, batch=int(cfg.get("promptsrc_batch", 4)), lr=cfg.get("promptsrc_lr", 0.0025),
        momentum=cfg.get("promptsrc_momentum", 0.9), loss_scale=cfg.get("promptsrc_loss_scale", 1024.0), seed=seed, evaluate=evaluate,
        on_epoch_end=on_epoch_end)
    return learner, epoch_losses
