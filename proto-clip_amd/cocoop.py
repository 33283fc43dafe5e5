"""CoCoOp (conditional context optimisation, Zhou et al., CVPR 2022), the base-to-new generalisation baseline of the prompt-learning tables: CoOp's
context shifted per image by a two-layer meta-net of the image feature, trained through the FROZEN text tower on cached image features:

    f_b      = normalise(image_features[b])                                                                          # ops.l2norm_rows, a constant
    pi_b     = W2 relu(W1 f_b + b1) + b2                                                                             # autograd.MetaNetFn, csrc/pclip_cocoop.hip
    prompts  = [SOT ; ctx + pi_b (n_ctx rows) ; class-name tokens ; "." ; EOT ; padding] + positional_embedding      # autograd.CondPromptEmbedFn
    t_b[n]   = text_projection(ln_final(transformer(prompts_b[n]))[EOT row])           B * N prompts                 # autograd.TowerTailFn from block 0
    loss     = mean_b cross_entropy(logit_scale.exp() * f_b . normalise(t_b[:]), y_b)                                # autograd.cosine_cross_entropy per image

Every image brings its own N prompts, so a step runs the text tower on B * N prompts: batches are small (upstream trains at batch 1).  The assembly and its
gradient take at most _lib.COCOOP_MAX_B images per call; more are chunked here.  The prompts go through the tower in chunks of `clip_model.text_chunk`; a
prompt's features do not depend on what else is in its chunk.  `truncate` and `clip_model.unfreeze(text_blocks=k)` work as for `coop.PromptLearner`.

Envelope: coop.PromptLearner's (class token at the "end", head dimension 64, prompts of at most 77 tokens), a context shared by the classes, fp32 parameters,
embed_dim a multiple of 64, 4 <= meta_hidden <= 256 a multiple of 4.  Not here: a single-launch loss over [B, N] (the loss is B calls of the one-row
cross-entropy)."""
import torch

from . import autograd as pag
from . import ops
from . import utils
from ._lib import COCOOP_MAX_B, PclipError
from .coop import PromptLearner
from .prompt_train import accuracy, train_prompts
from .tower import run_tower

PARAMETERS = ("ctx", "meta_w1", "meta_b1", "meta_w2", "meta_b2")


class ConditionalPromptLearner(torch.nn.Module):
    """The five learned tensors, all fp32: `ctx` [n_ctx, Wt] (ctx_init's token embeddings when given, as in `coop.PromptLearner`, else N(0, 0.02) from
    `seed`), `meta_w1` [Hd, E], `meta_b1` [Hd], `meta_w2` [Wt, Hd], `meta_b2` [Wt] (nn.Linear's default initialisation from `seed`; Hd = meta_hidden,
    default E // 16 as upstream).  Prompt texts, the EOT check and the L_eff truncation are coop.PromptLearner's (one is held, unregistered).
    forward(features [B, E] fp16) -> text features [B, N, E] fp16 with a tape to the five tensors (and to whatever of the text tower's tail is unfrozen);
    under torch.no_grad() the same kernels without a tape, hence the same bits.  The CLIP model is referenced, not registered: `parameters()` is exactly the
    five tensors."""

    def __init__(self, classnames, clip_model, n_ctx=4, ctx_init=None, meta_hidden=None, tokenize=None, tokenized_prompts=None, truncate=True, seed=1):
        super().__init__()
        who = "ConditionalPromptLearner"
        inner = PromptLearner(classnames, clip_model, n_ctx=n_ctx, ctx_init=ctx_init, tokenize=tokenize, tokenized_prompts=tokenized_prompts,
                              truncate=truncate, seed=seed)                     # assembly texts, EOT check, L_eff, head dimension: coop's, not forked
        Wt, E = clip_model.transformer.width, clip_model.text_projection.shape[1]
        Hd = E // 16 if meta_hidden is None else int(meta_hidden)
        if E < 64 or E % 64 != 0:
            raise PclipError(f"{who}: embed_dim={E} must be a positive multiple of 64 (the meta-net kernel reads 64 feature columns per step)")
        if not 4 <= Hd <= 256 or Hd % 4 != 0:
            raise PclipError(f"{who}: meta_hidden={Hd} must be a multiple of 4 in 4 .. 256")
        device = inner.ctx.device
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            l1, l2 = torch.nn.Linear(E, Hd), torch.nn.Linear(Hd, Wt)          # nn.Linear's default initialisation
        self.n_ctx, self.n_cls, self.meta_hidden = inner.n_ctx, inner.n_cls, Hd
        self.classnames = inner.classnames
        self.ctx = torch.nn.Parameter(inner.ctx.detach().clone())
        self.meta_w1 = torch.nn.Parameter(l1.weight.detach().to(device).contiguous())
        self.meta_b1 = torch.nn.Parameter(l1.bias.detach().to(device).contiguous())
        self.meta_w2 = torch.nn.Parameter(l2.weight.detach().to(device).contiguous())
        self.meta_b2 = torch.nn.Parameter(l2.bias.detach().to(device).contiguous())
        object.__setattr__(self, "clip_model", clip_model)
        object.__setattr__(self, "_text", inner)

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

    @property
    def tokenized_prompts(self):
        return self._text.tokenized_prompts

    def _check_parameters(self):
        for name in PARAMETERS:
            p = getattr(self, name)
            if p.dtype != torch.float32:
                raise PclipError(f"ConditionalPromptLearner: {name} must be torch.float32, got {p.dtype} (the context, the meta-net and their gradients "
                                 "are fp32; the kernels round the rows to fp16 where they enter the stream)")

    def normalise(self, features):
        """f [B, E] fp16, the L2-normalised image features: the meta-net's input and the loss' left operand, a constant."""
        E = self.meta_w1.shape[1]
        if features.dim() != 2 or features.shape[1] != E or features.dtype != torch.float16:
            raise PclipError(f"ConditionalPromptLearner: image features {features.dtype} {tuple(features.shape)} are not float16 [B, {E}]")
        with torch.no_grad():
            return ops.l2norm_rows(features.contiguous())

    def forward(self, features):
        m, inner = self.clip_model, self._text
        self._check_parameters()
        if m._text_stem_opt_in:
            raise PclipError("ConditionalPromptLearner: the text embeddings have been opted in through unfreeze(stem=...); prompt learning beside a "
                             "trainable stem is not supported (the context rows are spliced into a frozen embedding)")
        f = self.normalise(features)
        taped = False
        if torch.is_grad_enabled():
            tail = m._text_tape_from()                                         # refuses a trainable embedding in the frozen prefix
            taped = any(getattr(self, name).requires_grad for name in PARAMETERS) or tail is not None
        L, N = inner.run_length, self.n_cls
        emb16 = m._cache.get("tok", m.token_embedding.weight, lambda t: t.half().contiguous())
        pos16 = m._cache.get("pos", m.positional_embedding, lambda t: t.half().contiguous())
        tokens = inner.tokenized_prompts
        head = tokens[:, :L].contiguous()                                      # the EOT lies inside: the first maximum of the cut row is the full row's
        tw = m.text_tower
        what = f"ConditionalPromptLearner (n_ctx={self.n_ctx}, {L} tokens per prompt, {N} prompts per image, text tower on the tape from block 0)"
        plan = (0, False) if taped else (None, False)
        with torch.set_grad_enabled(taped):
            outs = []
            for b0 in range(0, f.shape[0], COCOOP_MAX_B):
                fc = f[b0:b0 + COCOOP_MAX_B]
                Bc = fc.shape[0]
                if taped:
                    pi = pag.MetaNetFn.apply(fc, self.meta_w1, self.meta_b1, self.meta_w2, self.meta_b2)
                    x = pag.CondPromptEmbedFn.apply(self.ctx, pi, tokens, emb16, pos16, L)
                else:
                    pi = ops.metanet(fc, self.meta_w1.detach(), self.meta_b1.detach(), self.meta_w2.detach(), self.meta_b2.detach())[1]
                    x = ops.prompt_embed_cond(self.ctx.detach(), pi, tokens, emb16, pos16, L)
                heads = head.repeat(Bc, 1)                                     # prompt b * N + n reads the tokens of class n
                feats = []
                for i, xi in zip(range(0, Bc * N, m.text_chunk), torch.split(x, m.text_chunk * L)):
                    hi = heads[i:i + m.text_chunk]
                    P = hi.shape[0]
                    if taped and (ops.splitk_active(P) or ops.splitk_active(P * L)):
                        raise PclipError(f"{what}: a pass inside ops.low_latency() is not supported (the split-K linears have no backward); leave the "
                                         f"context (B={P}, L={L})")
                    feats.append(run_tower(tw, xi, P, L, plan, tw.pick(P, L, xi.device, hi), what=what))
                t = feats[0] if len(feats) == 1 else torch.cat(feats, dim=0)
                outs.append(t.view(Bc, N, -1))
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


class CoCoOp(torch.nn.Module):
    """A CLIP model's temperature with a `ConditionalPromptLearner`'s per-image text features: the training loss on cached image features and the
    classifier."""

    def __init__(self, clip_model, learner):
        super().__init__()
        self.learner = learner
        object.__setattr__(self, "clip_model", clip_model)

    def logit_scale(self):
        return self.clip_model.logit_scale.float().exp()

    def forward(self, features):
        return self.learner(features)

    def loss(self, features, labels):
        """mean over the images of the cross-entropy of logit_scale.exp() * normalise(features[b]) . normalise(text[b, :]) against labels[b]: the B
        one-row cosine cross-entropies as the groups of ONE grouped call (features [B, 1, D] against text [B, N, E]), each with the bits of the single
        call on that image; the [B, N] logits are never written."""
        text, scale = self.learner(features), self.logit_scale()
        labels = labels.to(features.device).long()
        return pag.cosine_cross_entropy_grouped(features.unsqueeze(1), text, scale, labels.view(-1, 1), normalize_a=True, normalize_b=True).mean()

    def classify(self, features, topk=0):
        """arg-max class (int64 [Q]) of every image against ITS OWN N text rows, image chunk by image chunk; with topk > 0 also the top-k values and
        indices, as `utils.clip_zero_shot` returns them."""
        scale = float(self.logit_scale())
        out = []
        with torch.no_grad():
            f = self.learner.normalise(features)
            for b0 in range(0, f.shape[0], COCOOP_MAX_B):
                text = self.learner(features[b0:b0 + COCOOP_MAX_B])
                for b in range(text.shape[0]):
                    out.append(utils.clip_zero_shot(f[b0 + b:b0 + b + 1], ops.l2norm_rows(text[b]), scale=scale, topk=topk, layout="nd"))
        if topk:
            return tuple(torch.cat([o[k] for o in out], dim=0) for k in range(3))
        return torch.cat(out, dim=0)


def run_cocoop(cfg, train_features, train_labels, test_features, test_labels, classnames, clip_model, tokenize=None, tokenized_prompts=None, learner=None):
    """Train a conditional context on cached features ([Q, E] fp16 and labels) with upstream's recipe: SGD on the five tensors, learning rate 0.002,
    momentum 0.9, cosine schedule, batches of cfg.get('cocoop_batch', 1), cfg['cocoop_epochs'] epochs, 4 context rows (optional keys: 'n_ctx', 'ctx_init',
    'meta_hidden', 'cocoop_lr', 'cocoop_loss_scale', 'seed').  The loss goes through torch's GradScaler (initial scale 1024) for the reason `run_coop`
    records: the gradient stream inside the tower is fp16; the parameters and their gradients are fp32, so the scaler and the optimizer are torch's own.
    Prints the test accuracy before training and after every epoch; returns the trained `CoCoOp` module (`.results`: the figures, `.epoch_losses`).
    learner: a `ConditionalPromptLearner` of this model to go on training."""
    seed = int(cfg.get("seed", 1))
    if learner is None:
        learner = ConditionalPromptLearner(classnames, clip_model, n_ctx=cfg.get("n_ctx", 4), ctx_init=cfg.get("ctx_init"),
                                           meta_hidden=cfg.get("meta_hidden"), tokenize=tokenize, tokenized_prompts=tokenized_prompts, seed=seed)
    elif learner.clip_model is not clip_model:
        raise PclipError("run_cocoop: the learner belongs to another CLIP model")
    model = CoCoOp(clip_model, learner)
    labels = train_labels.to(train_features.device).long()
    res, epoch_losses = train_prompts("CoCoOp", learner.parameters(), lambda idx: model.loss(train_features[idx].contiguous(), labels[idx]),
                           train_features.shape[0], train_features.device, epochs=int(cfg["cocoop_epochs"]), batch=int(cfg.get("cocoop_batch", 1)),
                           lr=cfg.get("cocoop_lr", 0.002), momentum=0.9, loss_scale=cfg.get("cocoop_loss_scale", 1024.0), seed=seed,
                           evaluate=None if test_features is None else lambda: accuracy(model.classify(test_features), test_labels))
    if test_features is not None:
        res["test_acc"] = res["epochs"][-1]["test_acc"] if res["epochs"] else res["start_test_acc"]
    model.results, model.epoch_losses = res, epoch_losses
    return model
