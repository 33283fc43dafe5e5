"""ProGrad (prompt-aligned gradient), CoOp's neighbour in the few-shot tables: the context is trained on the cross-entropy, but its gradient may not
undo what the frozen zero-shot classifier knows.  Per step, on cached image features:

    text     = prompt_learner()                                                          # ONE forward of the frozen text tower (coop.PromptLearner)
    ce       = cross_entropy(logit_scale * normalise(f) @ normalise(text).T, labels)     # autograd.cosine_cross_entropy
    kl       = KL(softmax(zero-shot logits / tau) || softmax(own logits / tau)) tau^2    # autograd.cosine_kd: the teacher is the hand-crafted classifier
    g_ce, g_kl = d ce / d ctx, d kl / d ctx                                              # two backward walks over the one tape
    g        = g_ce                                       where <g_ce, g_kl> >= 0
               g_ce - lam <g_ce, g_kl> / <g_kl, g_kl> g_kl   otherwise                    # the component against the general knowledge is taken out

Both losses read the one text-feature tensor, so the tower runs forward once; `TowerTailFn` and `PromptEmbedFn` keep their tape and recompute what they
need, so each loss is walked back on its own with `torch.autograd.grad` (the first with retain_graph=True).  The projection is a few fp32 device ops with
no host synchronisation; it is homogeneous of degree one in a common factor of both gradients, so it is applied to the loss-scaled gradients and the
GradScaler unscales as usual."""
import torch

from . import autograd as pag
from ._lib import PclipError
from .coop import CoOp, PromptLearner
from .prompt_train import accuracy, train_prompts


class ProGrad(CoOp):
    """`CoOp` with a frozen teacher: teacher_weights [N, Et] fp16, the hand-crafted classifier's rows (`utils.clip_classifier`'s weights, transposed to
    rows) — normalised inside the kernel, so either form will do.  lam: how much of the conflicting component is taken out (1: all of it, upstream's
    default); temperature: of the KL."""

    def __init__(self, clip_model, prompt_learner, teacher_weights, lam=1.0, temperature=1.0):
        super().__init__(clip_model, prompt_learner)
        if not isinstance(teacher_weights, torch.Tensor) or teacher_weights.dtype != torch.float16 or teacher_weights.dim() != 2:
            raise PclipError(f"ProGrad: teacher_weights must be a 2-D float16 tensor [N, E], got {getattr(teacher_weights, 'dtype', type(teacher_weights))}")
        if teacher_weights.shape[0] != prompt_learner.n_cls:
            raise PclipError(f"ProGrad: teacher_weights has {teacher_weights.shape[0]} rows, the prompt learner {prompt_learner.n_cls} classes "
                             "(rows [N, E]: transpose clip_classifier's [E, N])")
        if teacher_weights.requires_grad:
            raise PclipError("ProGrad: teacher_weights requires grad, but the teacher is frozen")
        self.register_buffer("teacher_weights", teacher_weights.detach().contiguous(), persistent=False)
        self.lam, self.temperature = float(lam), float(temperature)

    def losses(self, image_features, labels):
        """(ce, kl) of one batch from ONE `prompt_learner()` forward: both tapes end in the same text-feature tensor."""
        text = self.prompt_learner()
        ce = pag.cosine_cross_entropy(image_features, text, self.logit_scale(), labels=labels, normalize_a=True, normalize_b=True)
        kl = self._distill(image_features, text, self.teacher_weights, None, self.temperature)
        return ce, kl

    def project_(self, g_ce, g_kl):
        """Upstream's rule on one parameter's pair of gradients, in place on g_ce (fp32), which is returned: unchanged where <g_ce, g_kl> >= 0, else
        g_ce - lam <g_ce, g_kl> / <g_kl, g_kl> g_kl.  An all-zero g_kl leaves g_ce.  Device ops only (torch.where on 0-dim tensors): no host sync."""
        if g_ce.dtype != torch.float32 or g_kl.dtype != torch.float32 or g_ce.shape != g_kl.shape:
            raise PclipError(f"ProGrad.project_: two float32 gradients of one shape, got {g_ce.dtype} {tuple(g_ce.shape)} and {g_kl.dtype} {tuple(g_kl.shape)}")
        d = (g_ce * g_kl).sum()
        n = (g_kl * g_kl).sum()
        conflict = (d < 0) & (n > 0)
        coef = torch.where(conflict, self.lam * d / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(d))
        return g_ce.sub_(coef * g_kl)

    def backward(self, ce, kl, scale=1.0):
        """Two walks over the one tape — d(scale ce) and d(scale kl) with respect to the learner's parameters — then the projection, written to `.grad`
        (replacing what was there).  scale: a number or a 0-dim device tensor (a GradScaler's scale); the rule is homogeneous, so the scaled gradients are
        projected and unscaled afterwards as usual."""
        params = [p for p in self.prompt_learner.parameters() if p.requires_grad]
        g_ce = torch.autograd.grad(ce * scale, params, retain_graph=True)
        g_kl = torch.autograd.grad(kl * scale, params)
        for p, a, b in zip(params, g_ce, g_kl):
            p.grad = self.project_(a.float().clone(), b.float())


def teacher_rows(clip_weights, n_cls):
    """`utils.clip_classifier`'s [E, N] weights (or rows [N, E] already) as the [N, E] fp16 rows `ProGrad` takes."""
    if clip_weights.dim() != 2 or n_cls not in clip_weights.shape:
        raise PclipError(f"teacher_rows: weights {tuple(clip_weights.shape)} hold no axis of {n_cls} classes")
    rows = clip_weights if clip_weights.shape[0] == n_cls and clip_weights.shape[1] != n_cls else clip_weights.t()
    return rows.detach().half().contiguous()


def run_prograd(cfg, train_features, train_labels, test_features, test_labels, classnames, clip_model, template=("a photo of a {}.",), tokenize=None,
                tokenized_prompts=None, teacher_weights=None):
    """`coop.run_coop` with ProGrad's step: the same recipe and cfg keys (cfg['coop_epochs'], 'n_ctx', 'coop_lr', 'coop_batch', 'coop_loss_scale', 'seed',
    ...), and cfg['prograd_lambda'] (1.0), cfg['prograd_temperature'] (1.0).  The teacher is the hand-crafted classifier of `template` over `classnames`
    (`utils.clip_classifier`), or `teacher_weights` ([N, E] rows or clip_classifier's [E, N]) where given.  The reported loss is the cross-entropy.
    Returns the trained `ProGrad` module (`.results`: the figures)."""
    from . import utils
    seed = int(cfg.get("seed", 1))
    learner = PromptLearner(classnames, clip_model, n_ctx=cfg.get("n_ctx", 16), ctx_init=cfg.get("ctx_init"), class_specific=cfg.get("class_specific", False),
                            tokenize=tokenize, tokenized_prompts=tokenized_prompts, seed=seed)
    if teacher_weights is None:
        with torch.no_grad():
            teacher_weights = utils.clip_classifier(classnames, list(template), clip_model, tokenize)[1]
    model = ProGrad(clip_model, learner, teacher_rows(teacher_weights, len(classnames)), lam=cfg.get("prograd_lambda", 1.0),
                    temperature=cfg.get("prograd_temperature", 1.0))
    labels = train_labels.to(train_features.device).long()
    pending = {}

    def loss_at(idx):
        pending["ce"], pending["kl"] = model.losses(train_features[idx].contiguous(), labels[idx])
        return pending["ce"]

    def backward(loss, scaler):
        one = torch.ones((), dtype=torch.float32, device=loss.device)
        model.backward(pending.pop("ce"), pending.pop("kl"), scale=scaler.scale(one))

    res, _ = train_prompts("ProGrad", learner.parameters(), loss_at, train_features.shape[0], train_features.device, epochs=int(cfg["coop_epochs"]),
                           batch=int(cfg.get("coop_batch", 32)), lr=cfg.get("coop_lr", 0.002), momentum=0.9, loss_scale=cfg.get("coop_loss_scale", 1024.0),
                           seed=seed, evaluate=lambda: accuracy(model.classify(test_features), test_labels), backward=backward)
    res["test_acc"] = res["epochs"][-1]["test_acc"] if res["epochs"] else res["start_test_acc"]
    model.results = res
    return model
