"""Mixed-precision AdamW for the tower parameters that `CLIP.unfreeze(...)` makes trainable.

    opt = TowerAdamW(model.unfreeze(visual_blocks=1, text_blocks=1), lr=1e-5, max_grad_norm=1.0)
    opt.zero_grad(); opt.scale_loss(loss).backward(); opt.step()

The towers' linears are fp16 parameters: an update of the size of a fine-tuning learning rate is below half an fp16 ulp of the weight, so it has to
accumulate in fp32 master weights.  State is fp32 (master weights of the fp16 parameters, both moments of every parameter; an fp32 parameter — the
LayerNorms — is its own master).  One step is three launches of csrc/pclip_tower_optim.hip for any number of tensors: per-chunk sums of squares of
the scaled gradients, a one-workgroup finish (overflow flag, unscaled norm, clip coefficient, bias corrections, torch.amp.GradScaler's scale rule) and
the update, which skips itself after an overflow.  Nothing is read back by the host, nothing is atomic (two runs give the same bits), and the
three launches form a linear chain that can be captured in a hipGraph (a replay does not re-run the host code: refresh() the tables and the
parameters' version counters yourself around replays).

`ops.adamw_` is NOT this: it restates the reference's fp16-state optimizer for the memory banks."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import PclipError

# the device state block (include/pclip.h: PCLIP_TOWER_STATE_BYTES)
STATE_DTYPE = np.dtype([("b1t", "<f8"), ("b2t", "<f8"), ("total", "<f8"), ("scale", "<f4"), ("tracker", "<i4"), ("step", "<i4"), ("found_inf", "<i4"),
                        ("grad_norm", "<f4"), ("clip_coef", "<f4"), ("inv_scale", "<f4"), ("bc1", "<f4"), ("sqrt_bc2", "<f4"), ("gmul", "<f4")])
assert STATE_DTYPE.itemsize == _lib.TOWER_STATE_BYTES
_DTYPES = (torch.float16, torch.float32)


def _align4(n):
    return (n + 3) // 4 * 4


class TowerAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay) with fp32 master weights, loss scaling and global-norm clipping for fp16 / fp32 device parameters.

    params_or_groups: parameters or torch param groups; a group may set its own `lr` and `weight_decay` (LR schedulers drive group["lr"]).
    max_grad_norm: clip the unscaled gradients to this global L2 norm (`clip_grad_norm_`'s coefficient); None: no clipping.
    loss_scale / dynamic / growth_interval: `scale_loss(loss)` multiplies by the device-resident scale; with `dynamic` an overflowed step is skipped
        and halves the scale, `growth_interval` clean steps in a row double it (torch.amp.GradScaler's rule).  Without `dynamic` the scale is fixed;
        an overflowed step is still skipped.
    decay_1d: weight decay also on one-dimensional tensors (biases, LayerNorm weights); off by default.
    A parameter whose .grad is None at step() is stepped with a zero gradient (its moments decay, its weight decay applies)."""

    GROWTH, BACKOFF = 2.0, 0.5

    def __init__(self, params_or_groups, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=None, loss_scale=2.0 ** 16, dynamic=True,
                 growth_interval=2000, decay_1d=False):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise PclipError(f"TowerAdamW: betas {betas} outside [0, 1)")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not loss_scale > 0.0 or growth_interval < 1:
            raise PclipError(f"TowerAdamW: lr={lr} eps={eps} weight_decay={weight_decay} loss_scale={loss_scale} growth_interval={growth_interval}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise PclipError(f"TowerAdamW: max_grad_norm={max_grad_norm} must be positive (None: no clipping)")
        super().__init__(params_or_groups, dict(lr=lr, weight_decay=weight_decay))
        self.betas, self.eps, self.max_grad_norm = (float(betas[0]), float(betas[1])), float(eps), max_grad_norm
        self.dynamic, self.growth_interval, self.decay_1d = bool(dynamic), int(growth_interval), bool(decay_1d)
        self._params = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise PclipError("TowerAdamW: no parameters")
        for i, p in enumerate(self._params):
            what = f"TowerAdamW: parameter {i} {tuple(p.shape)}"
            if not p.is_cuda:
                raise PclipError(f"{what} is not a device tensor (there is no CPU path)")
            if p.dtype not in _DTYPES:
                raise PclipError(f"{what} has dtype {p.dtype}: fp16 and fp32 parameters only")
            if not p.is_contiguous():
                raise PclipError(f"{what} is not contiguous")
            if p.numel() == 0:
                raise PclipError(f"{what} is empty")
        _lib.require_cuda(*self._params)
        dev = self._params[0].device
        # flat fp32 state, every segment 16-byte aligned: master weights of the fp16 parameters only, moments of all
        self._moff, self._soff, nm, ns = [], [], 0, 0
        for p in self._params:
            self._soff.append(ns)
            ns += _align4(p.numel())
            self._moff.append(nm if p.dtype == torch.float16 else None)
            nm += _align4(p.numel()) if p.dtype == torch.float16 else 0
        self.master = torch.zeros(max(nm, 4), dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(ns, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(ns, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self._params, self._moff):
                if off is not None:
                    self.master[off:off + p.numel()].copy_(p.detach().reshape(-1))
        first, nchunks = [], 0
        for p in self._params:
            first.append(nchunks)
            nchunks += -(-p.numel() // _lib.TOWER_CHUNK)
        self._first, self.nchunks = first, nchunks
        self.partials = torch.zeros(nchunks, dtype=torch.float32, device=dev)
        st = np.zeros(1, dtype=STATE_DTYPE)
        st["b1t"], st["b2t"], st["scale"] = 1.0, 1.0, loss_scale
        self._state = torch.from_numpy(st.view(np.uint8).copy()).to(dev)
        self._table = torch.zeros(len(self._params), 8, dtype=torch.int64, device=dev)
        self._hyper = torch.zeros(len(self._params), 2, dtype=torch.float32, device=dev)
        self._table_key = self._hyper_key = None

    def add_param_group(self, param_group):
        if getattr(self, "_params", None) is not None:
            raise PclipError("TowerAdamW: the flat state and the device table are laid out at construction; build a new optimizer for more parameters")
        super().add_param_group(param_group)

    # ---- device-resident results (no synchronisation) --------------------------------------------------------------------------------------------
    def _field(self, name, dtype):
        off = STATE_DTYPE.fields[name][1]
        return self._state[off:off + 4].view(dtype)[0]

    @property
    def loss_scale(self):
        """The current loss scale, a 0-dim fp32 device tensor (a view of the state block)."""
        return self._field("scale", torch.float32)

    @property
    def grad_norm(self):
        """Global L2 norm of the unscaled gradients at the last step (inf after an overflow), 0-dim fp32 device tensor."""
        return self._field("grad_norm", torch.float32)

    @property
    def found_inf(self):
        """1 when the last step met an Inf / NaN gradient and was skipped, 0-dim int32 device tensor."""
        return self._field("found_inf", torch.int32)

    def read_state(self):
        """The state block as a dict of host values (synchronises: for logging, checkpoints and tests)."""
        rec = self._state.cpu().numpy().view(STATE_DTYPE)[0]
        return {k: rec[k].item() for k in STATE_DTYPE.names}

    def scale_loss(self, loss):
        return loss * self.loss_scale

    def master_of(self, i):
        """fp32 master weights of parameter i (the parameter itself when it is fp32)."""
        p, off = self._params[i], self._moff[i]
        return p.detach() if off is None else self.master[off:off + p.numel()].view(p.shape)

    def moments_of(self, i):
        p, off = self._params[i], self._soff[i]
        return self.exp_avg[off:off + p.numel()].view(p.shape), self.exp_avg_sq[off:off + p.numel()].view(p.shape)

    # ---- host-side tables: compared every step, uploaded only when something moved ----------------------------------------------------------------
    def refresh(self):
        """Check the pointer table and the (lr, weight_decay) side table against the host's view and upload what changed."""
        hyper = []
        for grp in self.param_groups:
            lr, wd = float(grp["lr"]), float(grp["weight_decay"])
            for p in grp["params"]:
                hyper.append((lr, wd if (self.decay_1d or p.dim() >= 2) else 0.0))
        hyper, key = tuple(hyper), []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is not None:
                if g.device != p.device:
                    raise PclipError(f"TowerAdamW: parameter {i} {tuple(p.shape)} lives on {p.device} but its gradient on {g.device}")
                if g.is_sparse or g.dtype not in _DTYPES or not g.is_contiguous() or g.shape != p.shape:
                    raise PclipError(f"TowerAdamW: gradient of parameter {i} {tuple(p.shape)}: dense contiguous fp16 / fp32 of the parameter's shape "
                                     f"expected, got {g.dtype} {tuple(g.shape)}")
            key.append((p.data_ptr(), 0 if g is None else g.data_ptr(), None if g is None else g.dtype, hyper[i][1] != 0.0))
        key = tuple(key)
        capturing = torch.cuda.is_current_stream_capturing()
        if key != self._table_key:
            if capturing:
                raise PclipError("TowerAdamW: a parameter or gradient pointer moved during a graph capture; run one eager step first and keep the "
                                 ".grad tensors (zero_grad() keeps them)")
            mbase, abase, vbase = self.master.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
            rows = []
            for i, (p, (pp, gp, gdt, decays)) in enumerate(zip(self._params, key)):
                mp = pp if self._moff[i] is None else mbase + 4 * self._moff[i]
                ap, vp = abase + 4 * self._soff[i], vbase + 4 * self._soff[i]
                flags = (_lib.TOWER_PARAM_F16 if p.dtype == torch.float16 else 0) | (_lib.TOWER_GRAD_F16 if gdt == torch.float16 else 0)
                flags |= _lib.TOWER_DECAY if decays else 0
                if all(a % 16 == 0 for a in (pp, gp, mp, ap, vp)):
                    flags |= _lib.TOWER_ALIGNED
                rows.append([pp, gp, mp, ap, vp, p.numel(), self._first[i], flags])
            self._table.copy_(torch.tensor(rows, dtype=torch.int64))
            self._table_key = key
        if hyper != self._hyper_key:
            if capturing:
                raise PclipError("TowerAdamW: lr / weight_decay changed during a graph capture; call refresh() before the capture")
            self._hyper.copy_(torch.tensor(hyper, dtype=torch.float32))
            self._hyper_key = hyper

    def zero_grad(self, set_to_none=False):
        """Zero the gradients IN PLACE (the default here): their pointers stay in the device table, so no re-upload follows."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        grads = [p.grad for p in self._params if p.grad is not None]
        for g in grads:
            if g.grad_fn is not None:
                g.detach_()
            g.requires_grad_(False)
        if grads:
            torch._foreach_zero_(grads)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise PclipError("TowerAdamW.step takes no closure: backward runs on scale_loss(loss)")
        self.refresh()
        n = len(self._params)
        with torch.cuda.device(self._params[0].device):
            ops.tower_grad_sumsq(self._table, n, self.nchunks, self.partials)
            ops.tower_optim_finish(self.partials, self.nchunks, self._state, 0.0 if self.max_grad_norm is None else float(self.max_grad_norm),
                                   self.betas[0], self.betas[1], self.GROWTH, self.BACKOFF, self.growth_interval, self.dynamic)
            ops.tower_adamw_(self._table, self._hyper, n, self.nchunks, self._state, self.betas[0], self.betas[1], self.eps)
        # the kernels wrote the parameters behind autograd's back: advance their version counters so that every cached W^T / projT copy refreshes
        torch.autograd.graph.increment_version(self._params)

    # ---- checkpoints ------------------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd["tower"] = dict(master=self.master.cpu(), exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), state_block=self._state.cpu(),
                           numels=[p.numel() for p in self._params], dtypes=[str(p.dtype) for p in self._params])
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        tower = state_dict.get("tower")
        if tower is None:
            raise PclipError("TowerAdamW.load_state_dict: not a TowerAdamW state_dict (no 'tower' entry)")
        if tower["numels"] != [p.numel() for p in self._params] or tower["dtypes"] != [str(p.dtype) for p in self._params]:
            raise PclipError("TowerAdamW.load_state_dict: the parameter list differs from the saved one (sizes or dtypes)")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "tower"})
        self.master.copy_(tower["master"])
        self.exp_avg.copy_(tower["exp_avg"])
        self.exp_avg_sq.copy_(tower["exp_avg_sq"])
        self._state.copy_(tower["state_block"])
        for i, p in enumerate(self._params):                        # fp16 parameters follow their masters
            if self._moff[i] is not None:
                p.copy_(self.master_of(i))
        self._hyper_key = None
