"""optim.TowerAdamW on the GPU, graded bit for bit against the CPU restatement of its three kernels (tests/tower_optim_ref.py): the chunk partials within
the derived sum-of-squares bound of float64, the finish outputs equal to the restated finish fed those partials, master / m / v / parameters equal to the
restated update fed those outputs; overflow skipping and the loss-scale rule, clipping, determinism, hipGraph capture, the state_dict round trip, the
refresh of the towers' cached transposes, and fine-tuning end to end at a learning rate whose updates are below half an fp16 ulp."""
import math

import pytest
import torch

import tower_optim_ref as ref
from spec import SMALL
from test_gpu_tower_backward import make_model, tokens

pytestmark = pytest.mark.gpu

# (shape, parameter dtype, gradient dtype or None for .grad = None): 1, 7, 8, 9, 4095, 4096, 4097, 2 * 4096 + 3 elements; 2-D tensors decay
H, F = torch.float16, torch.float32
SPECS = [((1,), F, F), ((7,), H, H), ((8,), H, F), ((9,), F, H), ((5, 819), H, H), ((64, 64), H, None), ((17, 241), F, F), ((5, 1639), H, H)]
UNALIGNED = 4                       # this one is a view at storage offset 1 of its fp16 buffer: no 16-byte alignment, the element-by-element path
GROUPS = [dict(idx=[0, 1, 2, 3], lr=1e-3, weight_decay=0.01), dict(idx=[4, 5, 6, 7], lr=1e-5, weight_decay=0.1)]
SCALE = 1024.0


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_state(a, b):
    """Two state blocks as dicts, field by field (a NaN total equals a NaN total)."""
    return a.keys() == b.keys() and all(a[k] == b[k] or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) for k in a)


def make_params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    params = []
    for i, (shape, pdt, gdt) in enumerate(SPECS):
        n = math.prod(shape)
        w = ((torch.rand(n, generator=gen) * 0.48 + 0.02) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).to(pdt)
        if i == UNALIGNED:
            buf = torch.zeros(n + 1, dtype=pdt, device="cuda")
            buf[1:].copy_(w)
            p = torch.nn.Parameter(buf[1:].view(shape))
            assert p.storage_offset() == 1 and p.data_ptr() % 16 != 0 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(w.view(shape).cuda())
        if gdt is not None and gdt != pdt:
            p.grad_dtype = gdt
        params.append(p)
    return params


def make_grads(step, magnitude=1e-3, seed=100):
    """Raw (scaled) gradients of one step, on the CPU, in each tensor's gradient dtype."""
    gen = torch.Generator().manual_seed(seed + step)
    return [None if gdt is None else (torch.randn(shape, generator=gen) * magnitude * SCALE).to(gdt) for shape, _, gdt in SPECS]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif p.grad is None:
            p.grad = g.cuda()
        else:
            p.grad.copy_(g)                          # in place: the pointers in the device table stay valid


def make_opt(params, **kw):
    from proto_clip_amd.optim import TowerAdamW
    groups = [dict(params=[params[i] for i in g["idx"]], lr=g["lr"], weight_decay=g["weight_decay"]) for g in GROUPS]
    kw.setdefault("loss_scale", SCALE)
    return TowerAdamW(groups, lr=1e-4, **kw)


def hyper_of(i):
    g = GROUPS[0] if i in GROUPS[0]["idx"] else GROUPS[1]
    decays = len(SPECS[i][0]) >= 2
    return g["lr"], (g["weight_decay"] if decays else 0.0), decays


class Mirror:
    """The restatement's copy of the optimizer state, advanced with the GPU's own partials and finish outputs."""

    def __init__(self, opt, params):
        self.w = [opt.master_of(i).detach().float().cpu().clone() for i in range(len(params))]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.st = opt.read_state()

    def check_step(self, opt, params, grads, max_norm=None, growth_interval=2000, dynamic=True):
        part = opt.partials.cpu()
        numels = [p.numel() for p in params]
        exact = torch.cat([torch.stack([c.double().pow(2).sum() for c in (torch.zeros(n) if g is None else g.reshape(-1)).split(ref.CHUNK)])
                           for g, n in zip(grads, numels)])
        finite = torch.isfinite(exact)
        assert torch.equal(torch.isfinite(part), finite)
        rel = ((part.double() - exact).abs()[finite] / exact[finite].clamp_min(1e-300)).max()
        assert float(rel) <= ref.SUMSQ_REL_BOUND, float(rel)
        assert same_bits(part, ref.chunk_partials(grads, numels)) or not bool(finite.all())          # (stronger than asked: the documented order itself)
        st = opt.read_state()
        want = ref.finish(part, self.st, max_norm, 0.9, 0.999, growth_interval=growth_interval, dynamic=dynamic)
        assert same_state(st, want), (st, want)
        self.st = st
        for i, p in enumerate(params):
            lr, wd, decays = hyper_of(i)
            self.w[i], self.m[i], self.v[i] = ref.update(grads[i], self.w[i], self.m[i], self.v[i], st, lr, wd, decays)
            m, v = opt.moments_of(i)
            assert same_bits(opt.master_of(i), self.w[i]), i
            assert same_bits(m, self.m[i]) and same_bits(v, self.v[i]), i
            assert same_bits(p, self.w[i].to(p.dtype)), i                                              # an fp16 parameter is half(master)
        return st


def snapshot(opt, params):
    return [bits(p).clone() for p in params] + [bits(opt.master).clone(), bits(opt.exp_avg).clone(), bits(opt.exp_avg_sq).clone()]


def test_five_steps_equal_the_restatement_bit_for_bit():
    params = make_params()
    opt = make_opt(params)
    mirror = Mirror(opt, params)
    assert opt.nchunks == sum(-(-p.numel() // ref.CHUNK) for p in params) == 11
    for step in range(5):
        grads = make_grads(step)
        set_grads(params, grads)
        opt.step()
        st = mirror.check_step(opt, params, grads)
        assert st["found_inf"] == 0 and st["step"] == step + 1 and st["clip_coef"] == 1.0 and st["scale"] == SCALE
        print(f"step {step + 1}: grad_norm {st['grad_norm']:.6e} bc1 {st['bc1']:.6f} sqrt_bc2 {st['sqrt_bc2']:.6f}")
    assert float(opt.grad_norm) == st["grad_norm"] and float(opt.loss_scale) == SCALE and int(opt.found_inf) == 0
    assert opt.loss_scale.is_cuda and opt.grad_norm.is_cuda and opt.found_inf.is_cuda


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_overflow_skips_the_step_and_halves_the_scale(bad):
    params = make_params()
    opt = make_opt(params, growth_interval=2)
    mirror = Mirror(opt, params)
    grads = make_grads(0)
    set_grads(params, grads)
    opt.step()
    mirror.check_step(opt, params, grads, growth_interval=2)
    before, st0 = snapshot(opt, params), opt.read_state()
    grads = make_grads(1)
    grads[-1].view(-1)[-1] = bad                       # the last element of the last, ragged chunk
    set_grads(params, grads)
    opt.step()
    st = mirror.check_step(opt, params, grads, growth_interval=2)
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(opt, params)))
    assert st["found_inf"] == 1 and st["step"] == st0["step"] == 1 and st["b1t"] == st0["b1t"] and st["b2t"] == st0["b2t"]
    assert st["scale"] == SCALE / 2 and st["tracker"] == 0 and int(opt.found_inf) == 1 and math.isinf(float(opt.grad_norm))
    for k in (2, 3):                                   # two clean steps in a row double the scale
        grads = make_grads(k)
        set_grads(params, grads)
        opt.step()
        st = mirror.check_step(opt, params, grads, growth_interval=2)
    assert st["found_inf"] == 0 and st["step"] == 3 and st["scale"] == SCALE and st["tracker"] == 0


def test_clipping_by_the_global_norm():
    params = make_params()
    opt = make_opt(params, max_grad_norm=1.0)
    mirror = Mirror(opt, params)
    for step in range(2):
        grads = make_grads(step, magnitude=0.5)
        set_grads(params, grads)
        opt.step()
        st = mirror.check_step(opt, params, grads, max_norm=1.0)
        assert st["clip_coef"] < 1.0 and abs(st["clip_coef"] * st["grad_norm"] - 1.0) < 1e-5


def run_steps(n, **kw):
    params = make_params()
    opt = make_opt(params, **kw)
    for step in range(n):
        set_grads(params, make_grads(step))
        opt.step()
    return opt, params


def test_two_runs_give_the_same_bits():
    (a, pa), (b, pb) = run_steps(3, max_grad_norm=0.01), run_steps(3, max_grad_norm=0.01)
    assert all(torch.equal(x, y) for x, y in zip(snapshot(a, pa), snapshot(b, pb))) and same_state(a.read_state(), b.read_state())
    assert torch.equal(bits(a.partials), bits(b.partials))


def test_captured_step_replays_like_eager_steps():
    grads = make_grads(0)
    pa, pb = make_params(), make_params()
    a, b = make_opt(pa, max_grad_norm=0.01), make_opt(pb, max_grad_norm=0.01)
    set_grads(pa, grads)
    set_grads(pb, grads)
    for _ in range(3):
        a.step()
    b.refresh()                                        # tables uploaded before the capture; the captured step finds nothing to upload
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(snapshot(a, pa), snapshot(b, pb)))
    sa, sb = a.read_state(), b.read_state()
    assert same_state(sa, sb) and sa["step"] == 3


def test_state_dict_round_trip_continues_bit_identically():
    a, pa = run_steps(2, max_grad_norm=0.01, growth_interval=3)
    sd = a.state_dict()
    pb = make_params(seed=5)                           # other values: everything must come from the checkpoint
    with torch.no_grad():
        for p, q in zip(pa, pb):
            if q.dtype == torch.float32:
                q.copy_(p)                             # an fp32 parameter is its own master: it travels with the model's state_dict
    b = make_opt(pb, max_grad_norm=0.01, growth_interval=3, loss_scale=3.0)
    b.load_state_dict(sd)
    assert same_state(a.read_state(), b.read_state())
    for step in (2, 3):
        for opt, params in ((a, pa), (b, pb)):
            set_grads(params, make_grads(step))
            opt.step()
    assert all(torch.equal(x, y) for x, y in zip(snapshot(a, pa), snapshot(b, pb))) and same_state(a.read_state(), b.read_state())
    assert a.read_state()["scale"] == 2 * SCALE        # the growth tracker travelled too: steps 1, 2 and 3 complete the interval


def test_lr_schedulers_drive_the_side_table():
    params = make_params()
    opt = make_opt(params)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    set_grads(params, make_grads(0))
    opt.step()
    sched.step()
    opt.step()
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 5e-6]
    assert torch.equal(opt._hyper[:, 0].cpu(), torch.tensor([5e-4] * 4 + [5e-6] * 4))
    assert opt._hyper[:, 1].cpu().tolist() == [0.0, 0.0, 0.0, 0.0] + [pytest.approx(0.1)] * 4


def test_refusals():
    from proto_clip_amd._lib import PclipError
    from proto_clip_amd.optim import TowerAdamW
    with pytest.raises(PclipError, match="not contiguous"):
        TowerAdamW([torch.nn.Parameter(torch.zeros(8, 8, dtype=H, device="cuda").t())], lr=1e-5)
    with pytest.raises(PclipError, match="bfloat16"):
        TowerAdamW([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16, device="cuda"))], lr=1e-5)
    p = torch.nn.Parameter(torch.zeros(8, 8, dtype=H, device="cuda"))
    opt = TowerAdamW([p], lr=1e-5)
    p.grad = torch.zeros(8, 8, dtype=H, device="cuda").t()
    with pytest.raises(PclipError, match="gradient of parameter 0"):
        opt.step()


def small_batch():
    from proto_clip_amd import synth
    imgs = synth.make_images(8, SMALL["image_resolution"], seed=8, n_class=8).cuda()
    return imgs, tokens(8, SMALL["vocab_size"], 9).cuda()


def test_step_refreshes_the_cached_transposes():
    """One forward / backward / step, then the next forward and backward against a FRESH model built from the updated state_dict: a stale W^T or projT
    (cached by parameter version in clip/model.py and autograd.py) would change the features or the gradients."""
    from proto_clip_amd.clip.model import build_model
    from proto_clip_amd.optim import TowerAdamW
    imgs, toks = small_batch()
    model = make_model(SMALL, 6)
    params = model.unfreeze(visual_blocks=1, text_blocks=1)
    opt = TowerAdamW(params, lr=1e-3, loss_scale=SCALE)
    opt.scale_loss(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))).backward()
    versions = [p._version for p in params]
    opt.step()
    assert int(opt.found_inf) == 0 and all(p._version > v for p, v in zip(params, versions))
    opt.zero_grad()
    fresh = build_model({k: v.detach().clone() for k, v in model.state_dict().items()}).cuda()
    fresh_params = fresh.unfreeze(visual_blocks=1, text_blocks=1)
    out = []
    for mdl in (model, fresh):
        fi, ft = mdl.encode_image(imgs), mdl.encode_text(toks)
        (mdl.contrastive_loss(fi, ft) * SCALE).backward()
        out.append((fi.detach(), ft.detach()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert len(params) == len(fresh_params)
    for p, q in zip(params, fresh_params):
        assert torch.equal(p.detach(), q.detach()) and torch.equal(p.grad, q.grad)


def test_fine_tuning_end_to_end():
    from proto_clip_amd.optim import TowerAdamW
    imgs, toks = small_batch()
    model = make_model(SMALL, 6)
    opt = TowerAdamW(model.unfreeze(visual_blocks=1, text_blocks=1), lr=1e-3, max_grad_norm=1.0, loss_scale=SCALE, dynamic=True)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))
        opt.scale_loss(loss).backward()
        opt.step()
        losses.append(float(loss.detach()))
        print(f"loss {losses[-1]:.4f} grad_norm {float(opt.grad_norm):.4f} scale {float(opt.loss_scale):g} found_inf {int(opt.found_inf)}")
    with torch.no_grad():
        losses.append(float(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))))
    print("contrastive loss over five TowerAdamW steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    # a learning rate whose updates are below half an fp16 ulp of most weights: the fp16 weights still move, through the masters
    model = make_model(SMALL, 6)
    opt = TowerAdamW(model.unfreeze(visual_blocks=1, text_blocks=1), lr=1e-5, max_grad_norm=1.0, loss_scale=SCALE, dynamic=True)
    w = model.visual.transformer.resblocks[-1].mlp.c_fc.weight
    assert w.dtype == torch.float16 and w.requires_grad
    w0 = bits(w).clone()
    for _ in range(30):
        opt.zero_grad()
        opt.scale_loss(model.contrastive_loss(model.encode_image(imgs), model.encode_text(toks))).backward()
        opt.step()
    moved = int((bits(w) != w0).sum())
    print(f"lr 1e-5, 30 steps: {moved} of {w.numel()} elements of c_fc.weight moved; {opt.read_state()['step']} steps taken")
    assert moved > 0
