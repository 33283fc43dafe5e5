"""Query adapters at the widths / reductions / feature dims beyond the reference's defaults, on the GPU: conv adapters at width 8 / 24 / 32
(csrc/pclip_adapter_w.hip) and the fc adapter at hidden sizes that are multiples of 32 (RN50x4's D = 640 among them).  Forward against the
reference's own rows (tests/golden/adapter_shapes.npz) and the oracle, backward against fp16 CPU autograd, width 16 through the new entry
points bit for bit against the old ones, the trainer, the autograd drop-in and serving with hipGraph replay."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_adapter_close, observe, randomize_adapter_
from oracle import proto_oracle as po
from oracle import train_oracle as to
from proto_clip_amd import PclipError, _lib, synth
from proto_clip_amd.model import Adapter, Adapter_FC
from test_adapter_shapes_cpu import build, cases, unit_rows
from test_gpu_train import rel_l2

pytestmark = pytest.mark.gpu
P = _lib.ptr
CONV_KEYS = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight", "bn3.bias")


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import ops as _ops
    _lib.load()
    return _ops


def conv_args(sd):
    return [sd[k] for k in CONV_KEYS]


def adapter_conv_any_width(x, p, c_type):
    """oracle.train_oracle.adapter_conv (model.py:49-78 with fp16 parameters p) with the LayerNorm shape taken from the weights."""
    B, D = x.shape
    s = int(math.ceil(math.sqrt(D)))
    W = p["conv1.weight"].shape[0]
    x = F.pad(x, (0, s * s - D)).view(-1, 1, s, s)
    out = F.layer_norm(F.conv2d(x, p["conv1.weight"]), [W, s, s], p["bn1.weight"], p["bn1.bias"])
    if c_type == "conv-3x":
        out = F.layer_norm(F.conv2d(out, p["conv2.weight"], padding=1), [W, s, s], p["bn2.weight"], p["bn2.bias"])
    out = F.layer_norm(F.conv2d(out, p["conv3.weight"]), [1, s, s], p["bn3.weight"], p["bn3.bias"])
    out = out + x
    return out.view(-1, 1, s * s)[:, :, :D].reshape(-1, D)


_G, _CASES = cases()


@pytest.mark.parametrize("tag,kind,a,D", _CASES, ids=[c[0] for c in _CASES])
def test_forward_against_reference_and_oracle(ops, tag, kind, a, D):
    ad = build(kind, a, D, int(_G[tag + "__seed"]))
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    ad = ad.cuda()
    x = unit_rows(_G, D)
    with torch.no_grad():
        y = ad(x.cuda())
    assert_adapter_close(y, torch.from_numpy(_G[tag + "__out"]), tag="reference rows " + tag)
    g = torch.Generator().manual_seed(D + a)
    x300 = F.normalize(torch.randn(300, D, generator=g), dim=-1).half()
    with torch.no_grad():
        y300 = ad(x300.cuda())
        y300n = ad(x300.cuda(), l2norm_out=True)
    want = po.adapter_fc(x300, sd) if kind == "fc" else po.adapter_conv(x300, sd, kind)
    assert_adapter_close(y300, want, tag="oracle, 300 rows " + tag)
    if D % 8 == 0:
        assert torch.equal(y300n, ops.l2norm_rows(y300)), tag
    else:                                                                        # ops.l2norm_rows takes D % 8 == 0 only: its formula on the CPU
        assert_adapter_close(y300n, po.l2norm_rows(y300.cpu()), tag="fused row normalise " + tag)
    yg = ad(x300.cuda())                                                         # grad mode, trainable parameters: the autograd node's forward
    assert yg.requires_grad
    assert_adapter_close(yg.detach(), y300, tag="grad mode vs no_grad " + tag)


@pytest.mark.parametrize("B", [1, 3, 70000])
def test_row_counts_against_persistent_workgroups(ops, B):
    """Fewer rows than workgroups, and several rows per persistent workgroup: every row equals the row computed in a batch of its own kind
    (rows are independent), and the long batch matches the oracle on a sample."""
    D, W = 512, 32
    ad = build("conv-3x", W, D, 7)
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    ad = ad.cuda()
    g = torch.Generator().manual_seed(B)
    x = F.normalize(torch.randn(B, D, generator=g), dim=-1).half()
    with torch.no_grad():
        y = ad(x.cuda())
        pick = torch.arange(0, B, max(B // 150, 1))
        y_small = ad(x[pick].cuda())
    assert torch.equal(y[pick.cuda()], y_small)
    assert_adapter_close(y[pick.cuda()], po.adapter_conv(x[pick], sd, "conv-3x"), tag=f"oracle, conv-3x w32 d512 B={B}")


BWD = [("conv-3x", W, D) for W in (8, 24, 32) for D in (200, 512, 640, 1024)] + [("conv-2x", 8, 640), ("conv-2x", 24, 640), ("conv-2x", 32, 1024)]


@pytest.mark.parametrize("kind,W,D", BWD)
def test_conv_backward_against_fp16_autograd(ops, kind, W, D):
    """ops.adapter_conv_backward against fp16 CPU autograd of the reference's formulas; upstream gradient scale and bound of
    test_gpu_train.py::test_adapter_conv_backward (per parameter rel-L2 <= 2e-2; fp16 autograd is itself <= 3.3e-3 from float64 at these shapes)."""
    B = 40
    torch.manual_seed(B + D)
    ad = randomize_adapter_(Adapter(D, c_type=kind, width=W, dtype=torch.half), seed=B)
    params = {k: v.detach().clone().requires_grad_() for k, v in ad.state_dict().items()}
    g = torch.Generator().manual_seed(D)
    x = F.normalize(torch.randn(B, D, generator=g), dim=-1).half()
    up = (torch.randn(B, D, generator=g) * 1e-2).half()
    y = adapter_conv_any_width(x, params, kind)
    (y.float() * up.float()).sum().backward()
    c = {k: v.detach().cuda() for k, v in params.items()}
    got = ops.adapter_conv_backward(x.cuda(), up.cuda(), kind == "conv-3x", *conv_args(c), chunk=16)      # 40 rows in several chunks
    for k, ref in params.items():
        if ref.grad is None:
            assert k not in got, k
            continue
        assert got[k].shape == ref.shape, k
        e = observe(f"conv backward {kind} w{W} d{D}: grad {k} rel L2 vs fp16 autograd", rel_l2(got[k], ref.grad), 2e-2)
        print(f"{kind} w{W} d{D} {k}: {e:.3e}")
        assert e <= 2e-2, (k, e)


@pytest.mark.parametrize("kind,D", [("conv-3x", 512), ("conv-3x", 640), ("conv-3x", 1024), ("conv-2x", 768)])
def test_width_16_through_the_new_entry_points_is_the_old_path(ops, kind, D):
    lib = _lib.load()
    three = int(kind == "conv-3x")
    B = 300
    torch.manual_seed(D)
    ad = randomize_adapter_(Adapter(D, kind, dtype=torch.half), seed=3).cuda()
    c = [t.detach() for t in conv_args(dict(ad.state_dict()))]
    g = torch.Generator().manual_seed(D + 1)
    x = F.normalize(torch.randn(B, D, generator=g), dim=-1).half().cuda()
    up = (torch.randn(B, D, generator=g) * 1e-2).half().cuda()
    st = _lib.stream()
    y_old, y_new = torch.empty_like(x), torch.empty_like(x)
    _lib.check(lib.pclip_adapter_conv_f16(P(x), B, D, three, *[P(t) for t in c], 0, P(y_old), None, st), "old forward")
    _lib.check(lib.pclip_adapter_conv_w_f16(P(x), B, D, three, 16, *[P(t) for t in c], 0, P(y_new), None, st), "new forward")
    assert torch.equal(y_old, y_new)
    assert torch.equal(ops.adapter_conv(x, bool(three), *c), y_old)
    R = lib.pclip_adapter_conv_backward_partials(B, D, three)
    assert lib.pclip_adapter_conv_w_backward_partials(B, D, three, 16) == R
    s = int(math.ceil(math.sqrt(D)))
    sizes = dict(pw1=16, pw2=2304, pw3=16, pg1=16 * s * s, pb1=16 * s * s, pg2=16 * s * s, pb2=16 * s * s, pg3=s * s, pb3=s * s)
    bwd_params = [P(t) if (three or i not in (3, 4, 5)) else None for i, t in enumerate(c[:8])]
    outs = []
    for new in (False, True):
        bufs = {k: torch.zeros(R, n, dtype=torch.float32, device="cuda") for k, n in sizes.items()}
        ptrs = [P(bufs[k]) if (three or k not in ("pw2", "pg2", "pb2")) else None for k in sizes]
        if new:
            rc = lib.pclip_adapter_conv_w_backward_f16(P(x), P(up), B, D, three, 16, *bwd_params, *ptrs, st)
        else:
            rc = lib.pclip_adapter_conv_backward_f16(P(x), P(up), B, D, three, *bwd_params, *ptrs, st)
        _lib.check(rc, "backward")
        outs.append(bufs)
    for k in sizes:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_refusals_are_one_error_before_any_launch(ops):
    x = torch.zeros(4, 512, dtype=torch.float16, device="cuda")
    w12 = {k: v.cuda() for k, v in torch.nn.ModuleDict(dict(
        conv1=torch.nn.Conv2d(1, 12, 1, bias=False), bn1=torch.nn.LayerNorm([12, 23, 23]), conv2=torch.nn.Conv2d(12, 12, 3, padding=1, bias=False),
        bn2=torch.nn.LayerNorm([12, 23, 23]), conv3=torch.nn.Conv2d(12, 1, 1, bias=False), bn3=torch.nn.LayerNorm([1, 23, 23]))).half().state_dict().items()}
    with pytest.raises(PclipError, match="width 12"):
        ops.adapter_conv(x, True, *conv_args(w12))
    with pytest.raises(PclipError, match="width 12"):
        ops.adapter_conv_backward(x, x, True, *conv_args(w12))
    ad = Adapter_FC(640, reduction=8, dtype=torch.half).cuda()                  # H = 80
    with torch.no_grad(), pytest.raises(PclipError, match="H=80"):
        ad(torch.zeros(4, 640, dtype=torch.float16, device="cuda"))


def _one_trainer_step(cfg, ad, N, K, D, seed):
    from proto_clip_amd.train import ProtoClipTrainer, sample_epoch
    split = synth.make_split(N, K, D, 8, 8, seed=seed, sigma=3.0)
    sd = {k: v.detach().cpu().clone() for k, v in ad.state_dict().items()}
    gpu = ProtoClipTrainer(cfg, split.visual_memory_keys.cuda(), split.textual_memory_bank.cuda(), ad, cfg["alpha"], cfg["beta"])
    ref = to.Trainer(cfg, split.visual_memory_keys, split.textual_memory_bank, sd, cfg["alpha"], cfg["beta"])
    _, qi, ql = next(iter(sample_epoch(N, K, np.random.RandomState(3))))
    feats = gpu.keys_rows[torch.as_tensor(qi, device="cuda")]
    matches, loss, l1, l2, l3, l4i, l4t = gpu.step_features(feats, torch.as_tensor(ql))
    m_ref, loss_ref, terms, grads = ref.step(qi, ql)
    assert float(matches.item()) == m_ref
    assert abs(loss.item() - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    for got, key in ((l1, "L1"), (l2, "L2"), (l3, "L3"), (l4i, "L4i"), (l4t, "L4t")):
        assert abs(got.item() - terms[key]) <= 2e-5 * max(1.0, abs(terms[key])), key
    params = dict(gpu.adapter.named_parameters())
    for name, g_ref in grads.items():
        p = gpu.visual if name == "visual" else gpu.textual if name == "textual" else params[name]
        got = gpu.last_grads.get(id(p))
        if g_ref is None:
            assert got is None, name
        else:
            tol = 2e-2 if name not in ("visual", "textual") else 3e-3
            e = observe(f"trainer {cfg['adapter']} D={D}: grad {name} rel L2 vs oracle autograd", rel_l2(got.reshape(g_ref.shape), g_ref), tol)
            assert e <= tol, (name, e)


def test_trainer_with_a_width_32_conv_adapter(monkeypatch):
    """ProtoClipTrainer, one episode, every gradient against autograd of oracle.train_oracle.episode_loss (rule and tolerances of
    test_gpu_train.py::test_one_shot_episode_and_feature_step_match_autograd); the oracle's adapter_conv has [16, s, s] written in."""
    monkeypatch.setattr(to, "adapter_conv", adapter_conv_any_width)
    N, K, D = 12, 4, 512
    cfg = dict(shots=K, lr=1e-3, train_epoch=1, adapter="conv-3x", train_vis_mem_only=False, losses=["L1", "L2", "L3", "L4"], alpha=0.3, beta=5.0)
    torch.manual_seed(4)
    ad = randomize_adapter_(Adapter(D, "conv-3x", width=32, dtype=torch.half), seed=4).cuda()
    _one_trainer_step(cfg, ad, N, K, D, seed=9)


def test_trainer_with_the_fc_adapter_at_640():
    N, K, D = 6, 4, 640
    cfg = dict(shots=K, lr=1e-3, train_epoch=1, adapter="fc", train_vis_mem_only=False, losses=["L1", "L2", "L3", "L4"], alpha=0.3, beta=5.0)
    torch.manual_seed(5)
    ad = randomize_adapter_(Adapter_FC(D, dtype=torch.half), seed=5).cuda()
    _one_trainer_step(cfg, ad, N, K, D, seed=10)


@pytest.mark.parametrize("kind,D,a", [("conv-3x", 512, 32), ("fc", 640, 4), ("fc", 768, 8)])
def test_modules_under_autograd(kind, D, a):
    """The modules alone under autograd: parameter gradients (fp16, parameter-shaped) against autograd through the reference's fp16 formulas on the
    CPU for a synthetic upstream gradient (rule of test_gpu_autograd.py::test_adapter_modules_backward)."""
    B = 48
    ad = build(kind, a, D, 6).cuda()
    g = torch.Generator().manual_seed(7)
    x = F.normalize(torch.randn(B, D, generator=g), dim=-1).half()
    up = (torch.randn(B, D, generator=g) * 0.1).half()
    y = ad(x.cuda())
    assert y.requires_grad
    (y.float() * up.cuda().float()).sum().backward()
    sd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in ad.state_dict().items()}
    y_ref = to.adapter_fc(x, sd) if kind == "fc" else adapter_conv_any_width(x, sd, kind)
    (y_ref.float() * up.float()).sum().backward()
    for n_, p_ in ad.named_parameters():
        assert p_.grad is not None and p_.grad.dtype == torch.float16 and p_.grad.shape == p_.shape, n_
        e = observe(f"autograd adapter {kind} D={D} a={a}: grad {n_} rel L2 vs fp16 autograd", rel_l2(p_.grad, sd[n_].grad), 2e-2)
        assert e <= 2e-2, (n_, e)


TRAIN_FC_640 = ("T_fc_640", (6, 4, 640, 48, 48, 0.4, 6.0, "fc", 5.0, False, ["L1", "L2", "L3"], 2, 0.001))     # as tests/golden/make_golden_adapter_shapes.py


def _fc_640_run(monkeypatch):
    """The fixture of the reference's own training run with the fc adapter at D = 640 (first optimizer step recorded) and the state the run starts from:
    the split's banks and the adapter the reference's seeding order draws (checked against the reference's by the generator)."""
    from golden import spec
    from conftest import golden
    name, case = TRAIN_FC_640
    monkeypatch.setitem(spec.TRAIN, name, case)
    g = dict(golden("train_" + name).items())
    split, cfg = spec.train_inputs(name)
    N, K, D = case[:3]
    torch.manual_seed(1)
    torch.nn.Embedding(num_embeddings=N * K, embedding_dim=D)
    init = {k: v.clone() for k, v in Adapter_FC(D, dtype=torch.half).state_dict().items()}
    init["visual"], init["textual"] = split.visual_memory_keys.t().contiguous(), split.textual_memory_bank.t().contiguous()
    g.update({"init__" + k: v.numpy() for k, v in init.items()})
    names = [str(n) for n in g["names"]]
    rng = np.random.RandomState(1)
    qi, ql = next((qi, ql) for _, qi, ql in to.sample_epoch(N, K, rng))
    return name, g, names, init, split, cfg, qi, ql


def _assert_step_matches_fixture(name, g, names, cfg, noise, grads, params_after):
    """Rule and tolerances of test_gpu_train.py::test_first_steps_match_reference_and_oracle for one optimizer step from the reference's state."""
    for n in names:
        refg = torch.from_numpy(g[f"grad0__{n}"]).float()
        got = grads[n]
        assert got is not None, n
        err = (got.reshape(refg.shape).float().cpu() - refg).norm().item()
        observe(f"{name}: grad {n} |d| / (5e-3 |ref| + 3 noise)", err / (5e-3 * refg.norm().item() + 3.0 * noise[n] + 1e-30), 1.0)
        assert err <= 5e-3 * refg.norm().item() + 3.0 * noise[n], (name, n, err, refg.norm().item(), noise[n])
        after = torch.from_numpy(g[f"after0__{n}"])
        diff = (params_after[n].detach().cpu().float().reshape(after.shape) - after.float()).abs()
        big = 2.5 * cfg["lr"] + 2.0 ** -10 * after.abs().max().item()
        assert (diff > big).float().mean().item() < 5e-3, (name, n, (diff > big).float().mean().item())
        before = torch.from_numpy(g[f"init__{n}"]).float()
        upd = (after.float() - before).abs().mean().item()
        amp = cfg["lr"] / 1e-4 * 3.0 * noise[n] / after.numel() ** 0.5
        assert diff.mean().item() <= 0.02 * upd + 2.0 ** -13 * after.abs().mean().item() + amp, (name, n, diff.mean().item(), upd, amp)


def test_trainer_fc_640_first_step_matches_the_reference_run(monkeypatch):
    """ProtoClipTrainer with Adapter_FC(640) against tests/golden/train_T_fc_640.npz, the reference's own main.py run: matches, loss terms, every gradient and
    every updated parameter of the first optimizer step."""
    from proto_clip_amd.train import ProtoClipTrainer, sample_epoch
    from test_gpu_train import _oracle_noise
    name, g, names, init, split, cfg, qi, ql = _fc_640_run(monkeypatch)
    assert next((a, b) for _, a, b in sample_epoch(6, 4, np.random.RandomState(1))) == (qi, ql)
    ad = Adapter_FC(640, dtype=torch.half)
    ad.load_state_dict({k: v for k, v in init.items() if k not in ("visual", "textual")})
    gpu = ProtoClipTrainer(cfg, split.visual_memory_keys.cuda(), split.textual_memory_bank.cuda(), ad.cuda(), cfg["alpha"], cfg["beta"])
    noise = _oracle_noise(name, g, names, 0, qi, ql)
    matches, loss, l1, l2, l3, _, _ = gpu.step(qi, ql)
    assert float(matches.item()) == g["ep_matches"][0]
    assert abs(loss.item() - g["ep_loss"][0]) <= 2e-5 * max(1.0, abs(g["ep_loss"][0]))
    assert abs(l1.item() - g["ep_l1"][0]) <= 2e-5 * max(1.0, abs(g["ep_l1"][0]))
    assert abs(l2.item() - g["ep_l2"][0]) <= 2e-5 and abs(l3.item() - g["ep_l3"][0]) <= 2e-5
    adp = dict(gpu.adapter.named_parameters())
    obj = {n: (gpu.visual if n == "visual" else gpu.textual if n == "textual" else adp[n]) for n in names}
    _assert_step_matches_fixture("trainer " + name, g, names, cfg, noise, {n: gpu.last_grads.get(id(obj[n])) for n in names}, obj)


def _loop_body_step(adapter, cfg, split, visual, textual, query_index, zq_labels):
    """The reference's loop body (main.py:260-310) restated as in test_gpu_autograd.py::test_reference_loop_body_runs_under_autograd: torch's eager
    prototype block, the drop-in adapter / P / compute_loss_and_matches, loss.backward(retain_graph=True), torch.optim.AdamW."""
    from proto_clip_amd.utils import P, compute_loss_and_matches
    K = cfg["shots"]
    ndim = split.visual_memory_keys.shape[0]
    visual_memory_keys = split.visual_memory_keys.cuda()
    params = list(adapter.parameters()) + [visual] if cfg["train_vis_mem_only"] else [visual, textual] + list(adapter.parameters())
    optimizer = torch.optim.AdamW(params, lr=cfg["lr"], eps=1e-4, weight_decay=0.05, foreach=False)
    zs_imgs = visual.view(-1, K, ndim)
    zs_imgs = zs_imgs / zs_imgs.norm(dim=-1, keepdim=True)
    z_img_proto = zs_imgs.mean(dim=1).float()
    z_img_proto = z_img_proto / z_img_proto.norm(dim=-1, keepdim=True)
    zq_imgs = visual_memory_keys.t()[torch.as_tensor(query_index).cuda()]
    zq_imgs = adapter(zq_imgs).float()
    labels = torch.as_tensor(zq_labels).cuda()
    zs_text = textual
    zq_imgs = zq_imgs / zq_imgs.norm(dim=-1, keepdim=True)
    zs_text = zs_text / zs_text.norm(dim=-1, keepdim=True)
    z_text_proto = zs_text.float()
    p = P(zq_imgs, z_img_proto, z_text_proto, cfg["alpha"], cfg["beta"])
    matches, train_loss, _, l2, l3, _, _ = compute_loss_and_matches(p, labels, z_img_proto, z_text_proto, cfg)
    optimizer.zero_grad()
    train_loss.backward(retain_graph=True)
    named = dict(adapter.named_parameters())
    grads = {"visual": visual.grad, "textual": textual.grad, **{n: q.grad for n, q in named.items()}}
    grads = {n: (None if v is None else v.detach().clone()) for n, v in grads.items()}
    optimizer.step()
    return matches, train_loss, l2, l3, grads, {"visual": visual, "textual": textual, **named}


def test_reference_loop_body_under_autograd_fc_640(monkeypatch):
    """The loop body with Adapter_FC(640) against the reference's own run (tests/golden/train_T_fc_640.npz), first step, at the tolerances of
    test_gpu_autograd.py::test_reference_loop_body_runs_under_autograd."""
    from test_gpu_train import _oracle_noise
    name, g, names, init, split, cfg, qi, ql = _fc_640_run(monkeypatch)
    ad = Adapter_FC(640, dtype=torch.half)
    ad.load_state_dict({k: v for k, v in init.items() if k not in ("visual", "textual")})
    visual, textual = torch.nn.Parameter(init["visual"].cuda().clone()), torch.nn.Parameter(init["textual"].cuda().clone())
    noise = _oracle_noise(name, g, names, 0, qi, ql)
    matches, loss, l2, l3, grads, after = _loop_body_step(ad.cuda(), cfg, split, visual, textual, qi, ql)
    assert float(matches.item()) == g["ep_matches"][0]
    assert abs(loss.item() - g["ep_loss"][0]) <= 2e-5 * max(1.0, abs(g["ep_loss"][0]))
    assert abs(l2.item() - g["ep_l2"][0]) <= 2e-5 * max(1.0, abs(g["ep_l2"][0])) + 2e-5
    assert abs(l3.item() - g["ep_l3"][0]) <= 2e-5 * max(1.0, abs(g["ep_l3"][0])) + 2e-5
    _assert_step_matches_fixture("autograd loop " + name, g, names, cfg, noise, grads, after)


def test_reference_loop_body_under_autograd_conv_width_32(monkeypatch):
    """The loop body with Adapter(512, "conv-3x", width=32): one step from identical state against the oracle's trainer (autograd of
    oracle.train_oracle.episode_loss + torch AdamW on the CPU, its adapter_conv restated width-generic): matches, loss to 2e-5, gradients to 3e-3 (banks) /
    2e-2 (adapter) in relative l2, and the updated parameters by the fp16-AdamW outlier rule of test_first_steps_match_reference_and_oracle."""
    monkeypatch.setattr(to, "adapter_conv", adapter_conv_any_width)
    from proto_clip_amd.train import sample_epoch
    N, K, D = 12, 4, 512
    cfg = dict(shots=K, lr=1e-3, train_epoch=1, adapter="conv-3x", train_vis_mem_only=False, losses=["L1", "L2", "L3"], alpha=0.3, beta=5.0)
    split = synth.make_split(N, K, D, 8, 8, seed=9, sigma=3.0)
    torch.manual_seed(4)
    ad = randomize_adapter_(Adapter(D, "conv-3x", width=32, dtype=torch.half), seed=4)
    sd = {k: v.detach().clone() for k, v in ad.state_dict().items()}
    ref = to.Trainer(cfg, split.visual_memory_keys, split.textual_memory_bank, sd, cfg["alpha"], cfg["beta"])
    _, qi, ql = next(iter(sample_epoch(N, K, np.random.RandomState(3))))
    visual = torch.nn.Parameter(split.visual_memory_keys.t().contiguous().cuda())
    textual = torch.nn.Parameter(split.textual_memory_bank.t().contiguous().cuda())
    matches, loss, l2, l3, grads, after = _loop_body_step(ad.cuda(), cfg, split, visual, textual, qi, ql)
    m_ref, loss_ref, terms, g_ref = ref.step(qi, ql)
    assert float(matches.item()) == m_ref
    assert abs(loss.item() - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    ref_after = {"visual": ref.visual, "textual": ref.textual, **ref.adapter}
    for n, gr in g_ref.items():
        tol = 2e-2 if n not in ("visual", "textual") else 3e-3
        e = observe(f"autograd loop conv-3x w32: grad {n} rel L2 vs oracle autograd", rel_l2(grads[n].reshape(gr.shape), gr), tol)
        assert e <= tol, (n, e)
        want = ref_after[n].detach()
        diff = (after[n].detach().cpu().float().reshape(want.shape) - want.float()).abs()
        big = 2.5 * cfg["lr"] + 2.0 ** -10 * want.abs().max().item()
        assert (diff > big).float().mean().item() < 5e-3, (n, (diff > big).float().mean().item())


def test_serving_on_rn50x4_with_the_fc_adapter():
    """ProtoClipClassifier on the RN50x4 tower with Adapter_FC(640) at batch 1 and 4: the captured hipGraph replays to the eager result bit for bit."""
    from proto_clip_amd.serving import ProtoClipClassifier
    from test_gpu_wide_resnet import _tower
    kw, _, model = _tower("RN50x4", 25)
    D, N, K = kw["embed_dim"], 12, 4
    assert D == 640
    split = synth.make_split(N, K, D, 8, 8, seed=4, sigma=3.0)
    ev = (split.visual_memory_keys.t().float() * 1.2).half().contiguous().cuda()
    et = (split.textual_memory_bank.t().float() * 1.4).half().contiguous().cuda()
    torch.manual_seed(8)
    adapter = randomize_adapter_(Adapter_FC(D, dtype=torch.half), seed=8).cuda()
    imgs = synth.make_images(4, 288, seed=13, n_class=N).cuda()
    clf = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=3)
    for n in (1, 4):
        tp, ti = clf.classify(imgs[:n])
        assert tp.shape == (n, 3) and torch.isfinite(tp).all()
        clf.capture(n)
        for _ in range(2):
            tg, ig = clf.classify(imgs[:n])
            assert torch.equal(tg, tp) and torch.equal(ig, ti)


def test_checkpoint_loader_takes_the_shapes_from_the_checkpoint(tmp_path):
    from proto_clip_amd.serving import load_pretrained_mb_and_adapters
    D = 640
    torch.save(torch.zeros(8, D, dtype=torch.float16), tmp_path / "v.pt")
    torch.save(torch.zeros(2, D, dtype=torch.float16), tmp_path / "t.pt")
    for kind, a in (("conv-3x", 32), ("fc", 2)):
        src = build(kind, a, D, 11)
        torch.save(src.state_dict(), tmp_path / "a.pt")
        _, _, ad = load_pretrained_mb_and_adapters(memory_bank_v_path=str(tmp_path / "v.pt"), memory_bank_t_path=str(tmp_path / "t.pt"),
                                                   adapter_type=kind, adapter_weights_path=str(tmp_path / "a.pt"))
        for k, v in src.state_dict().items():
            assert torch.equal(ad.state_dict()[k].cpu(), v), k
