"""Tip-Adapter, the training-free cache baseline the Proto-CLIP tables compare against (Tip-Adapter main.py: run_tip_adapter, search_hp), on the fused
cache-logit kernels (csrc/pclip_tip.hip):

    affinity     = features @ cache_keys                                  # [Q, NK]   never written here
    cache_logits = exp(-(beta - beta * affinity)) @ cache_values          # [Q, N]    the one-hot product is a sum over each class's contiguous rows
    tip_logits   = 100. * features @ clip_weights + alpha * cache_logits

The operands are what `utils.build_cache_model` (cache_keys [D, NK] sorted by class, cache_values one-hot [NK, N]), `utils.clip_classifier`
(clip_weights [D, N]) and `utils.pre_load_features` return.  The arithmetic is deliberately more exact than upstream's fp16 tensor chain (include/pclip.h,
pclip_tip_logits_f16): only the final logit is rounded to fp16.  `cache_values` is turned into segment offsets once per call here (`ops.tip_segments`, one
synchronisation); callers that classify many batches against one cache pass `seg=` themselves."""
import numpy as np
import torch
import torch.nn.functional as F

from . import autograd as pag
from . import ops
from . import utils
from ._lib import PclipError


def _segments(cache_values, seg):
    return ops.tip_segments(cache_values) if seg is None else seg


def _key_rows(cache_keys, adapter):
    """(keys, layout): upstream's [D, NK] cache, or — with a fine-tuned adapter — its `weight`, the [NK, D] key rows."""
    if adapter is None:
        return cache_keys, None
    return adapter.weight.detach(), "nd"


def tip_logits(features, cache_keys, cache_values, clip_weights, alpha, beta, seg=None, layout=None, key_layout=None):
    """Dense fp16 [Q, N] Tip-Adapter logits.  layout: how `clip_weights` lies (utils.clip_logits' rule); key_layout: how `cache_keys` lies — "dn" upstream's
    [D, NK], "nd" [NK, D] rows, None told from the shape, where a square tensor (NK == D) is read as upstream's [D, NK]: name it when the cache is rows."""
    rows = utils._clip_weight_rows(features, clip_weights, layout)
    return ops.tip_logits(features, cache_keys, _segments(cache_values, seg), rows, alpha, beta, layout=key_layout)[0].contiguous()


def tip_classify(features, cache_keys, cache_values, clip_weights, alpha, beta, seg=None, layout=None, key_layout=None):
    """`tip_logits(...).argmax(1)` (int64 [Q], lowest index among equal logits) without writing a matrix; layout / key_layout as there."""
    rows = utils._clip_weight_rows(features, clip_weights, layout)
    return ops.tip_logits(features, cache_keys, _segments(cache_values, seg), rows, alpha, beta, want_logits=False, want_argmax=True,
                          layout=key_layout)[2].long()


def search_lists(cfg):
    """Upstream's beta and alpha lists from cfg['search_scale'] / cfg['search_step'] (main.search_scale_step fills them): i * (scale - 0.1) / step + 0.1,
    un-rounded Python floats."""
    scale, step = cfg["search_scale"], cfg["search_step"]
    beta_list = [i * (scale[0] - 0.1) / step[0] + 0.1 for i in range(step[0])]
    alpha_list = [i * (scale[1] - 0.1) / step[1] + 0.1 for i in range(step[1])]
    return beta_list, alpha_list


def best_of_grid(grid):
    """(beta, alpha, acc) of the first strict maximum of an [n, 3] (beta, alpha, acc) array in its own (beta-major) order — upstream's `if acc > best_acc`
    starting from 0: a grid of zeros leaves (0, 0, 0)."""
    best = (0, 0, 0.0)
    for b, a, acc in np.asarray(grid, dtype=np.float64):
        if acc > best[2]:
            best = (float(b), float(a), float(acc))
    return best


def search_hp(cfg, cache_keys, cache_values, features, labels, clip_weights, adapter=None, out=None, seg=None):
    """Upstream's search over the (beta, alpha) grid on ONE launch: returns (best_beta, best_alpha, best_acc), accuracy = 100 * correct / Q, the best pair the first
    strict maximum in beta-major order.  out (a dict): out["grid"] = float64 [nb * na, 3] of (beta, alpha, acc), beta-major."""
    beta_list, alpha_list = search_lists(cfg)
    keys, key_layout = _key_rows(cache_keys, adapter)
    rows = utils._clip_weight_rows(features, clip_weights)
    correct = ops.tip_grid(features, keys, _segments(cache_values, seg), rows, beta_list, alpha_list, labels, layout=key_layout)
    acc = 100.0 * correct.cpu().numpy().astype(np.float64) / features.shape[0]
    grid = np.array([(b, a, acc[ib, ia]) for ib, b in enumerate(beta_list) for ia, a in enumerate(alpha_list)], dtype=np.float64).reshape(-1, 3)
    if out is not None:
        out["grid"] = grid
    best_beta, best_alpha, best_acc = best_of_grid(grid)
    print("\nAfter searching, the best accuarcy: {:.2f}.\n".format(best_acc))
    return best_beta, best_alpha, best_acc


def _acc(pred, labels):
    return 100.0 * float((pred == labels.to(pred.device).long()).sum().item()) / labels.shape[0]


def run_tip_adapter(cfg, cache_keys, cache_values, val_features, val_labels, test_features, test_labels, clip_weights):
    """Upstream's run_tip_adapter, same arguments and order of work: zero-shot CLIP on val, Tip-Adapter at cfg['init_alpha'] / cfg['init_beta'] on val, search_hp on
    val, then zero-shot and Tip-Adapter on test at the pair found.  Returns everything computed."""
    res = {}
    seg = ops.tip_segments(cache_values)
    res["zero_shot_val_acc"] = _acc(utils.clip_zero_shot(val_features, clip_weights), val_labels)
    print("\n**** Zero-shot CLIP's val accuracy: {:.2f}. ****\n".format(res["zero_shot_val_acc"]))
    beta, alpha = cfg["init_beta"], cfg["init_alpha"]
    res["tip_val_acc"] = _acc(tip_classify(val_features, cache_keys, cache_values, clip_weights, alpha, beta, seg=seg), val_labels)
    print("**** Tip-Adapter's val accuracy: {:.2f}. ****\n".format(res["tip_val_acc"]))
    grid = {}
    res["best_beta"], res["best_alpha"], res["best_val_acc"] = search_hp(cfg, cache_keys, cache_values, val_features, val_labels, clip_weights, out=grid, seg=seg)
    res["grid"] = grid["grid"]
    res["zero_shot_test_acc"] = _acc(utils.clip_zero_shot(test_features, clip_weights), test_labels)
    print("\n**** Zero-shot CLIP's test accuracy: {:.2f}. ****\n".format(res["zero_shot_test_acc"]))
    res["tip_test_acc"] = _acc(tip_classify(test_features, cache_keys, cache_values, clip_weights, res["best_alpha"], res["best_beta"], seg=seg), test_labels)
    print("**** Tip-Adapter's test accuracy: {:.2f}. ****\n".format(res["tip_test_acc"]))
    return res


class TipAdapterF(torch.nn.Module):
    """Tip-Adapter-F's trainable cache: upstream's `adapter = nn.Linear(D, NK, bias=False); adapter.weight = nn.Parameter(cache_keys.t())`, whose `weight` is the
    [NK, D] fp16 key rows — a saved upstream `best_F_*shots.pt` (that weight tensor) loads with `load_weight`, and `state_dict()` has the one key "weight"."""

    def __init__(self, cache_keys, layout=None):
        super().__init__()
        if cache_keys.dtype != torch.float16 or cache_keys.dim() != 2:
            raise PclipError(f"TipAdapterF: cache_keys must be a 2-D float16 tensor, got {cache_keys.dtype} {tuple(cache_keys.shape)}")
        if layout not in (None, "dn", "nd"):
            raise PclipError(f"TipAdapterF: layout={layout!r}: expected 'dn' (upstream's cache_keys [D, NK]), 'nd' ([NK, D] rows) or None (= 'dn')")
        rows = cache_keys.detach() if layout == "nd" else cache_keys.detach().t()
        self.weight = torch.nn.Parameter(rows.contiguous().clone())

    def load_weight(self, weight):
        """Upstream saves `adapter.weight` itself (torch.save(adapter.weight, .../best_F_{shots}shots.pt)): an [NK, D] tensor."""
        if tuple(weight.shape) != tuple(self.weight.shape):
            raise PclipError(f"TipAdapterF: a checkpoint of shape {tuple(weight.shape)} does not fit the [NK, D] = {tuple(self.weight.shape)} key rows")
        with torch.no_grad():
            self.weight.copy_(weight.to(self.weight.dtype))
        return self

    def logits(self, features, cache_values, clip_weights, alpha, beta, seg=None, layout=None):
        """Under grad mode: the fp32 logits [Q, N] with a tape to `weight` (autograd.TipLogitsFn).  Under torch.no_grad(): the inference kernel's fp16 logits."""
        for name, t in (("features", features), ("clip_weights", clip_weights), ("alpha", alpha), ("beta", beta)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f"TipAdapterF.logits: {name} requires grad — Tip-Adapter-F trains the cache keys only; detach it")
        rows = utils._clip_weight_rows(features, clip_weights, layout)
        seg = _segments(cache_values, seg)
        if torch.is_grad_enabled() and self.weight.requires_grad:
            return pag.TipLogitsFn.apply(self.weight, features, seg, rows, alpha, beta)
        return ops.tip_logits(features, self.weight.detach(), seg, rows, alpha, beta, layout="nd")[0].contiguous()

    def forward(self, features, cache_values, clip_weights, alpha, beta, seg=None, layout=None):
        return self.logits(features, cache_values, clip_weights, alpha, beta, seg=seg, layout=layout)


def run_tip_adapter_F(cfg, cache_keys, cache_values, val_features, val_labels, test_features, test_labels, clip_weights, clip_model, train_loader_F):
    """Upstream's run_tip_adapter_F: fine-tune the cache keys with AdamW (lr = cfg['lr'], eps 1e-4) under cosine annealing over train_epoch * len(loader) steps; per
    batch `encode_image` under no_grad, the fp16 row normalisation, the taped logits and F.cross_entropy; after every epoch the test accuracy, keeping the best
    weights (as upstream does); then search_hp with the trained adapter and the test accuracy at the pair found.  The cache logits and their gradient are the
    kernels; torch is the cross-entropy on a [B, N] fp32 tensor and the optimizer.  Returns everything computed: per-epoch figures, the adapter with the kept
    weights, `best_epoch` and `best_epoch_test_acc` (the best test accuracy over the epochs, at init_alpha / init_beta), the grid, the best pair and the test
    accuracy at it."""
    res = {"epochs": []}
    seg = ops.tip_segments(cache_values)
    adapter = TipAdapterF(cache_keys).to(val_features.device)
    optimizer = torch.optim.AdamW(adapter.parameters(), lr=cfg["lr"], eps=1e-4)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, cfg["train_epoch"] * len(train_loader_F))
    beta, alpha = cfg["init_beta"], cfg["init_alpha"]
    best_acc, best_epoch, best_weight = 0.0, 0, adapter.weight.detach().clone()
    for train_idx in range(cfg["train_epoch"]):
        adapter.train()
        correct_samples, all_samples, loss_list = 0, 0, []
        print("Train Epoch: {:} / {:}".format(train_idx, cfg["train_epoch"]))
        for images, target in train_loader_F:
            images, target = images.cuda(), target.cuda()
            with torch.no_grad():
                image_features = clip_model.encode_image(images)
                image_features = ops.l2norm_rows(image_features, out=image_features)
            tip = adapter.logits(image_features, cache_values, clip_weights, alpha, beta, seg=seg)
            loss = F.cross_entropy(tip, target)
            correct_samples += int((tip.detach().argmax(1) == target).sum().item())
            all_samples += len(tip)
            loss_list.append(loss.item())
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            scheduler.step()
        current_lr = scheduler.get_last_lr()[0]
        print("LR: {:.6f}, Acc: {:.4f} ({:}/{:}), Loss: {:.4f}".format(current_lr, correct_samples / all_samples, correct_samples, all_samples, sum(loss_list) / len(loss_list)))
        adapter.eval()
        with torch.no_grad():
            acc = _acc(tip_classify(test_features, adapter.weight.detach(), cache_values, clip_weights, alpha, beta, seg=seg, key_layout="nd"), test_labels)
        print("**** Tip-Adapter-F's test accuracy: {:.2f}. ****\n".format(acc))
        res["epochs"].append({"loss": sum(loss_list) / len(loss_list), "train_acc": 100.0 * correct_samples / all_samples, "test_acc": acc})
        if acc > best_acc:
            best_acc, best_epoch, best_weight = acc, train_idx, adapter.weight.detach().clone()
    adapter.load_weight(best_weight)
    res["adapter"], res["best_epoch"], res["best_epoch_test_acc"] = adapter, best_epoch, best_acc
    print(f"**** After fine-tuning, Tip-Adapter-F's best test accuracy: {best_acc:.2f}, at epoch: {best_epoch}. ****\n")
    grid = {}
    res["best_beta"], res["best_alpha"], res["best_val_acc"] = search_hp(cfg, cache_keys, cache_values, val_features, val_labels, clip_weights, adapter=adapter,
                                                                         out=grid, seg=seg)
    res["grid"] = grid["grid"]
    with torch.no_grad():
        res["tip_f_test_acc"] = _acc(tip_classify(test_features, adapter.weight.detach(), cache_values, clip_weights, res["best_alpha"], res["best_beta"], seg=seg,
                                                  key_layout="nd"), test_labels)
    print("**** Tip-Adapter-F's test accuracy: {:.2f}. ****\n".format(res["tip_f_test_acc"]))
    return res
