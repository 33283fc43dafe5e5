"""pclip_tip_logits_f16 / pclip_tip_grid_f16 / pclip_tip_keys_backward_f16 (csrc/pclip_tip.hip), their bindings in ops, autograd.TipLogitsFn and
proto_clip_amd.tip_adapter, against the float64 helper tests/tip_adapter_ref.py under ITS derived per-element tolerances, and against the kernels' own invariances bit
for bit.  The cases and (alpha, beta) points are the helper's (CASES, POINTS); every figure is recorded through conftest.observe before it is asserted."""
import numpy as np
import pytest
import torch

import tip_adapter_ref as ref
from conftest import observe

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.05
_DEV, _EXACT, _AT = {}, {}, {}


def dev(name):
    """The case's operands on the GPU (built once, never modified): features, key rows, seg, text rows."""
    if name not in _DEV:
        s = ref.case(name)
        _DEV[name] = (s["features"].cuda(), s["keys"].cuda(), s["seg"].cuda(), s["text"].cuda())
    return _DEV[name]


def exact(name):
    if name not in _EXACT:
        s = ref.case(name)
        _EXACT[name] = ref.Exact(s["features"], s["keys"], s["seg"], s["text"])
    return _EXACT[name]


def at(name, alpha, beta):
    key = (name, alpha, beta)
    if key not in _AT:
        _AT[key] = exact(name).at(alpha, beta)
    return _AT[key]


def first_argmax(l16):
    """argmax of an fp16 matrix with the lowest index among equal values (numpy's rule), on the host."""
    return torch.from_numpy(np.argmax(l16.float().cpu().numpy(), axis=1))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_logits_and_argmax_against_float64(name):
    from proto_clip_amd import ops
    f, keys, seg, w = dev(name)
    for alpha, beta in ref.POINTS:
        r = at(name, alpha, beta)
        l16, l32, am = ops.tip_logits(f, keys, seg, w, alpha, beta, want_logits=True, want_f32=True, want_argmax=True, layout="nd")
        _, _, am_only = ops.tip_logits(f, keys, seg, w, alpha, beta, want_logits=False, want_argmax=True, layout="nd")
        r16 = observe("tip logits fp16: |got - float64| / derived tolerance", ref.worst_ratio(l16, r["v"], r["tol16"]), 1.0)
        r32 = observe("tip logits fp32: |got - float64| / derived tolerance", ref.worst_ratio(l32, r["v"], r["tol32"]), 1.0)
        want, tie = ref.near_ties(r["v"], r["tol16"])
        share = observe("tip argmax: share of proven near-ties in a case", float(tie.double().mean()), NEAR_TIE_CAP)
        wrong = am.cpu().long() != want
        print(name, alpha, beta, "fp16", round(r16, 4), "fp32", round(r32, 5), "near-ties", int(tie.sum()), "argmax differs", int(wrong.sum()))
        assert r16 <= 1.0 and r32 <= 1.0, (name, alpha, beta, r16, r32)
        differ = l16.cpu() != l32.half().cpu()                                               # the fp16 logits are the one rounding of the fp32 ones
        assert not bool(differ.any()), (name, alpha, beta, int(differ.sum()), l16.cpu()[differ][:4], l32.cpu()[differ][:4])
        assert torch.equal(am.cpu().long(), first_argmax(l16)), (name, alpha, beta)          # the fused argmax is the argmax of the written matrix
        assert torch.equal(am_only, am)
        assert share <= NEAR_TIE_CAP, (name, alpha, beta, share)
        assert not bool((wrong & ~tie).any()), (name, alpha, beta, int((wrong & ~tie).sum()))


@pytest.mark.parametrize("name", ["ragged3", "gap", "pets", "caltech1", "imagenet_sub", "one", "d2048"])
def test_alpha_zero_is_the_zero_shot_kernel_bit_for_bit(name):
    from proto_clip_amd import tip_adapter, utils
    f, keys, seg, w = dev(name)
    got = tip_adapter.tip_logits(f, keys.t().contiguous(), None, w, 0.0, 5.5, seg=seg, layout="nd")
    assert torch.equal(got, utils.clip_logits(f, w, layout="nd"))


def test_a_row_does_not_depend_on_its_neighbours():
    from proto_clip_amd import ops
    f, keys, seg, w = dev("many")
    full16, full32, _ = ops.tip_logits(f, keys, seg, w, 3.0, 7.0, want_f32=True, layout="nd")
    for q in (0, 63, 7777, 19999):
        one16, one32, _ = ops.tip_logits(f[q:q + 1], keys, seg, w, 3.0, 7.0, want_f32=True, layout="nd")
        assert torch.equal(one16, full16[q:q + 1]) and torch.equal(one32, full32[q:q + 1]), q
    part16, _, part_am = ops.tip_logits(f[100:133], keys, seg, w, 3.0, 7.0, want_argmax=True, layout="nd")
    assert torch.equal(part16, full16[100:133]) and torch.equal(part_am.cpu().long(), first_argmax(full16[100:133]))


@pytest.mark.parametrize("name,n", [("pets", 10), ("ragged3", 1), ("gap", 2), ("imagenet_sub", 70)])
def test_a_column_does_not_depend_on_later_classes(name, n):
    from proto_clip_amd import ops
    f, keys, seg, w = dev(name)
    full16, full32, _ = ops.tip_logits(f, keys, seg, w, 3.0, 7.0, want_f32=True, layout="nd")
    end = int(ref.case(name)["seg"][n + 1])
    cut16, cut32, _ = ops.tip_logits(f, keys[:end], seg[:n + 2].contiguous(), w[:n + 1], 3.0, 7.0, want_f32=True, layout="nd")
    assert torch.equal(cut16, full16[:, :n + 1]) and torch.equal(cut32, full32[:, :n + 1])


def test_two_calls_give_the_same_bits():
    from proto_clip_amd import ops
    f, keys, seg, w = dev("imagenet_sub")
    a = ops.tip_logits(f, keys, seg, w, 17.0, 1.0, want_f32=True, want_argmax=True, layout="nd")
    b = ops.tip_logits(f, keys, seg, w, 17.0, 1.0, want_f32=True, want_argmax=True, layout="nd")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    betas, alphas = [0.1, 2.0, 5.5], [0.1, 1.0]
    lab = ref.case("imagenet_sub")["labels"].cuda()
    assert torch.equal(ops.tip_grid(f, keys, seg, w, betas, alphas, lab, layout="nd"), ops.tip_grid(f, keys, seg, w, betas, alphas, lab, layout="nd"))


def test_upstream_layouts_are_accepted():
    """cache_keys [D, NK] and clip_weights [D, N] as build_cache_model / clip_classifier return them, one-hot cache_values: the same bits as the row layouts."""
    from proto_clip_amd import ops, tip_adapter
    s = ref.case("pets")
    f, keys, seg, w = dev("pets")
    values = torch.nn.functional.one_hot(s["key_labels"], s["N"]).cuda()
    assert torch.equal(ops.tip_segments(values), seg) and torch.equal(ops.tip_segments(s["key_labels"].cuda(), s["N"]), seg)
    got = tip_adapter.tip_logits(f, keys.t().contiguous(), values, w.t().contiguous(), 1.0, 5.5)
    want, _, am = ops.tip_logits(f, keys, seg, w, 1.0, 5.5, want_argmax=True, layout="nd")
    assert got.is_contiguous() and torch.equal(got, want)
    pred = tip_adapter.tip_classify(f, keys.t().contiguous(), values, w.t().contiguous(), 1.0, 5.5)
    assert pred.dtype == torch.int64 and torch.equal(pred, am.long())


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------------

def lists(scale, step):
    from proto_clip_amd import tip_adapter
    return tip_adapter.search_lists({"search_scale": scale, "search_step": step})


def single_counts(name, betas, alphas):
    from proto_clip_amd import ops
    f, keys, seg, w = dev(name)
    lab = ref.case(name)["labels"].cuda()
    out = np.zeros((len(betas), len(alphas)), dtype=np.int64)
    for ib, b in enumerate(betas):
        for ia, a in enumerate(alphas):
            am = ops.tip_logits(f, keys, seg, w, a, b, want_logits=False, want_argmax=True, layout="nd")[2]
            out[ib, ia] = int((am.long() == lab).sum())
    return out


def float64_counts(name, betas, alphas):
    """(counts, proven near-ties) per pair from the float64 logits."""
    ex, lab = exact(name), ref.case(name)["labels"]
    counts = np.zeros((len(betas), len(alphas)), dtype=np.int64)
    ties = np.zeros_like(counts)
    for ib, b in enumerate(betas):
        for ia, a in enumerate(alphas):
            r = ex.at(a, b)
            am, tie = ref.near_ties(r["v"], r["tol16"])
            counts[ib, ia], ties[ib, ia] = int((am == lab).sum()), int(tie.sum())
    return counts, ties


@pytest.mark.parametrize("scale", [[7, 3], [50, 50]])
@pytest.mark.parametrize("name", ["ragged3", "gap", "pets", "caltech1", "d2048"])
def test_grid_counts(name, scale):
    from proto_clip_amd import ops, tip_adapter
    betas, alphas = lists(scale, [20, 10])
    f, keys, seg, w = dev(name)
    s = ref.case(name)
    got = ops.tip_grid(f, keys, seg, w, betas, alphas, s["labels"].cuda(), layout="nd").cpu().numpy()
    assert np.array_equal(got, single_counts(name, betas, alphas))                           # exactly nb x na single calls
    want, ties = float64_counts(name, betas, alphas)
    excess = observe("tip grid: |count - float64 count| - proven near-ties at a pair (<= 0)", float((np.abs(got - want) - ties).max()), 0.0)
    print(name, scale, "pairs that differ from float64", int((got != want).sum()), "most near-ties at a pair", int(ties.max()))
    assert excess <= 0
    out = {}
    values = torch.nn.functional.one_hot(s["key_labels"], s["N"]).cuda()
    best = tip_adapter.search_hp({"search_scale": scale, "search_step": [20, 10]}, keys.t().contiguous(), values, f, s["labels"].cuda(), w.t().contiguous(), out=out)
    acc = 100.0 * got.astype(np.float64) / f.shape[0]
    grid = np.array([(b, a, acc[ib, ia]) for ib, b in enumerate(betas) for ia, a in enumerate(alphas)])
    assert np.array_equal(out["grid"], grid) and best == tip_adapter.best_of_grid(grid)
    k = int(np.argmax(grid[:, 2]))                                                           # numpy's first maximum is the first strict one
    assert best == ((float(grid[k, 0]), float(grid[k, 1]), float(grid[k, 2])) if grid[k, 2] > 0 else (0, 0, 0.0))


def test_grid_on_the_large_cache():
    from proto_clip_amd import ops
    betas, alphas = lists([7, 3], [20, 10])
    betas, alphas = betas[::4], alphas[::3]                                                  # 5 x 4 pairs: a chunk and a ragged one
    f, keys, seg, w = dev("imagenet_sub")
    got = ops.tip_grid(f, keys, seg, w, betas, alphas, ref.case("imagenet_sub")["labels"].cuda(), layout="nd").cpu().numpy()
    assert np.array_equal(got, single_counts("imagenet_sub", betas, alphas))
    want, ties = float64_counts("imagenet_sub", betas, alphas)
    assert (np.abs(got - want) <= ties).all()


@pytest.mark.parametrize("nb", [1, 7, 201])
def test_grid_with_a_ragged_beta_chunk(nb):
    from proto_clip_amd import ops
    betas = [0.1 + 0.037 * i for i in range(nb)]
    alphas = [0.1, 1.7, 30.0]
    f, keys, seg, w = dev("pets")
    labels = ref.case("pets")["labels"].clone()
    labels[3], labels[4] = -1, 37                                                            # labels outside [0, N) match nothing
    got = ops.tip_grid(f, keys, seg, w, betas, alphas, labels.cuda(), layout="nd").cpu().numpy()
    want = np.zeros_like(got)
    for ib, b in enumerate(betas):
        for ia, a in enumerate(alphas):
            am = ops.tip_logits(f, keys, seg, w, a, b, want_logits=False, want_argmax=True, layout="nd")[2]
            want[ib, ia] = int((am.long().cpu() == labels).sum())
    assert got.shape == (nb, 3) and np.array_equal(got, want)


def test_run_tip_adapter_end_to_end():
    from proto_clip_amd import tip_adapter, utils
    s = ref.case("pets")
    f, keys, seg, w = dev("pets")
    values = torch.nn.functional.one_hot(s["key_labels"], s["N"]).cuda()
    val_f, val_y, test_f, test_y = f[:66], s["labels"][:66].cuda(), f[66:], s["labels"][66:].cuda()
    cfg = {"init_alpha": 1.0, "init_beta": 5.5, "search_scale": [7, 3], "search_step": [20, 10]}
    res = tip_adapter.run_tip_adapter(cfg, keys.t().contiguous(), values, val_f, val_y, test_f, test_y, w.t().contiguous())

    def acc64(rows, labels, alpha, beta):
        """(float64 accuracy, how many queries of difference the proven near-ties allow)"""
        r = at("pets", alpha, beta)
        v, tol = r["v"][rows], r["tol16"][rows]
        _, tie = ref.near_ties(v, tol)
        return utils.cls_acc(v, labels.cpu()), int(tie.sum())

    val, test = slice(0, 66), slice(66, 131)
    for got, (want, slack), n in ((res["tip_val_acc"], acc64(val, val_y, 1.0, 5.5), 66),
                                  (res["tip_test_acc"], acc64(test, test_y, res["best_alpha"], res["best_beta"]), 65)):
        assert abs(got - want) * n / 100.0 <= slack + 1e-9, (got, want, slack)
    zs = first_argmax(utils.clip_logits(val_f, w, layout="nd"))
    assert res["zero_shot_val_acc"] == 100.0 * int((zs == val_y.cpu()).sum()) / 66
    assert res["grid"].shape == (200, 3) and res["best_val_acc"] == res["grid"][:, 2].max()


# ---- the key gradient ----------------------------------------------------------------------------------------------------------------------------

BWD_POINTS = [(1.0, 5.5), (3.0, 7.0), (17.0, 1.0)]


def upstream_gradient(name, alpha, beta, B=None, loss_scale=1.0):
    """(rows, dL [B, N] fp32): the gradient of F.cross_entropy on the float64 logits of the case's first B queries."""
    s = ref.case(name)
    B = s["features"].shape[0] if B is None else B
    v = at(name, alpha, beta)["v"][:B]
    return B, ref.ce_grad(v, s["labels"][:B], loss_scale=loss_scale)[0]


def sub_exact(name, B):
    s = ref.case(name)
    key = (name, B)
    if key not in _EXACT:
        _EXACT[key] = ref.Exact(s["features"][:B], s["keys"], s["seg"], s["text"]) if B != s["features"].shape[0] else exact(name)
    return _EXACT[key]


@pytest.mark.parametrize("name", ["ragged3", "gap", "pets", "eurosat", "imagenet_sub"])
def test_key_gradient_against_float64_autograd(name):
    from proto_clip_amd import ops
    f, keys, seg, w = dev(name)
    for alpha, beta in BWD_POINTS:
        for B in (None, 3):
            B, dL = upstream_gradient(name, alpha, beta, B)
            want, tol = ref.keys_backward(sub_exact(name, B), alpha, beta, dL)
            got = ops.tip_keys_backward(f[:B], keys, seg, dL.cuda(), alpha, beta, layout="nd")
            r = observe("tip dkeys: |got - float64| / derived tolerance", ref.worst_ratio(got, want, tol), 1.0)
            print(name, alpha, beta, "B", B, "dkeys", round(r, 4), "max |dkeys|", float(want.abs().max()))
            assert r <= 1.0, (name, alpha, beta, B, r)
            assert torch.equal(got, ops.tip_keys_backward(f[:B], keys, seg, dL.cuda(), alpha, beta, layout="nd"))      # deterministic


def test_a_scaled_loss_scales_the_gradient():
    from proto_clip_amd import ops
    f, keys, seg, w = dev("pets")
    B, dL = upstream_gradient("pets", 3.0, 7.0)
    want, tol = ref.keys_backward(exact("pets"), 3.0, 7.0, dL)
    got = ops.tip_keys_backward(f, keys, seg, (dL * 1024.0).cuda(), 3.0, 7.0, layout="nd")
    r = observe("tip dkeys, loss x 1024: |got - 1024 float64| / (1024 tolerance)", ref.worst_ratio(got, 1024.0 * want, 1024.0 * tol), 1.0)
    assert r <= 1.0, r
    assert torch.equal(got, 1024.0 * ops.tip_keys_backward(f, keys, seg, dL.cuda(), 3.0, 7.0, layout="nd"))          # a power of two only moves the exponent


def test_a_key_row_does_not_depend_on_the_other_rows():
    from proto_clip_amd import ops
    s = ref.case("pets")
    f, keys, seg, w = dev("pets")
    B, dL = upstream_gradient("pets", 3.0, 7.0)
    full = ops.tip_keys_backward(f, keys, seg, dL.cuda(), 3.0, 7.0, layout="nd")
    n = 9                                                                                    # only class 9's rows stay: every other class is empty
    lo, hi = int(s["seg"][n]), int(s["seg"][n + 1])
    seg1 = torch.zeros_like(s["seg"])
    seg1[n + 1:] = hi - lo
    rows = keys[lo:hi].clone()                                                               # (the slice starts at row 36: copied to an aligned base)
    alone = ops.tip_keys_backward(f, rows, seg1.cuda(), dL.cuda(), 3.0, 7.0, layout="nd")
    assert torch.equal(alone, full[lo:hi])
    # empty classes leave their neighbours' rows untouched: `gap` against the same rows without its two empty classes; the result is written into the middle
    # of a poisoned buffer, whose guard rows before row 0 and after row NK - 1 must stay as they were
    fg, kg, sg, _ = dev("gap")
    Bg, dLg = upstream_gradient("gap", 3.0, 7.0)
    buf = torch.full((2 + 9 + 2, 64), float("nan"), dtype=torch.float32, device="cuda")
    with_gaps = ops.tip_keys_backward(fg, kg, sg, dLg.cuda(), 3.0, 7.0, layout="nd", out=buf[2:11])
    assert with_gaps.data_ptr() == buf[2:11].data_ptr() and bool(torch.isnan(buf[:2]).all()) and bool(torch.isnan(buf[11:]).all())
    dense = ops.tip_keys_backward(fg, kg, torch.tensor([0, 3, 7, 9], dtype=torch.int32).cuda(), dLg[:, [0, 2, 4]].contiguous().cuda(), 3.0, 7.0, layout="nd")
    assert torch.equal(with_gaps, dense) and with_gaps.shape == (9, 64) and bool(torch.isfinite(with_gaps).all())


# ---- TipAdapterF ---------------------------------------------------------------------------------------------------------------------------------

def test_adapter_gradient_lands_on_the_weight_only():
    from proto_clip_amd import tip_adapter
    s = ref.case("pets")
    f, keys, seg, w = dev("pets")
    values = torch.nn.functional.one_hot(s["key_labels"], s["N"]).cuda()
    adapter = tip_adapter.TipAdapterF(keys.t().contiguous())
    assert adapter.weight.dtype == torch.float16 and tuple(adapter.weight.shape) == tuple(keys.shape) and torch.equal(adapter.weight.detach(), keys)
    assert list(adapter.state_dict()) == ["weight"]
    logits = adapter.logits(f, values, w.t().contiguous(), 1.0, 5.5)
    assert logits.dtype == torch.float32 and logits.requires_grad
    r = at("pets", 1.0, 5.5)
    assert ref.worst_ratio(logits.detach(), r["v"], r["tol32"]) <= 1.0
    loss = torch.nn.functional.cross_entropy(logits, s["labels"].cuda())
    loss.backward()
    g = adapter.weight.grad
    assert g is not None and g.dtype == torch.float16 and g.shape == adapter.weight.shape and float(g.float().abs().max()) > 0
    want, tol = ref.keys_backward(exact("pets"), 1.0, 5.5, ref.ce_grad(r["v"], s["labels"])[0])
    got32 = g.float().cpu().double()                                                          # the fp16 cast of the kernel's fp32 gradient: half an fp16 ulp more
    assert bool(((got32 - want).abs() <= tol + want.abs() * 2.0 ** -11 + 2.0 ** -25).all())
    with torch.no_grad():
        plain = adapter.logits(f, values, w.t().contiguous(), 1.0, 5.5)
    assert plain.dtype == torch.float16 and not plain.requires_grad and plain.grad_fn is None
    assert torch.equal(plain, tip_adapter.tip_logits(f, keys.t().contiguous(), values, w.t().contiguous(), 1.0, 5.5))
    for bad in ("features", "clip_weights"):
        fr, wr = f.clone().requires_grad_(bad == "features"), w.t().contiguous().requires_grad_(bad == "clip_weights")
        with pytest.raises(NotImplementedError, match=bad):
            adapter.logits(fr, values, wr, 1.0, 5.5)
    with pytest.raises(NotImplementedError, match="alpha"):
        adapter.logits(f, values, w.t().contiguous(), torch.tensor(1.0, requires_grad=True), 5.5)
    upstream_checkpoint = (keys.float() * 1.01).half().cpu()                                  # what torch.save(adapter.weight, best_F_4shots.pt) holds: [NK, D]
    adapter.load_weight(upstream_checkpoint)
    assert torch.equal(adapter.weight.detach().cpu(), upstream_checkpoint)


def test_five_adamw_steps_lower_the_loss():
    from proto_clip_amd import ops, tip_adapter
    s = ref.case("eurosat")
    f, keys, seg, w = dev("eurosat")
    adapter = tip_adapter.TipAdapterF(keys, layout="nd")
    optimizer = torch.optim.AdamW(adapter.parameters(), lr=1e-3, eps=1e-4)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, 5)
    labels, losses = s["labels"].cuda(), []
    for _ in range(5):
        feats = ops.l2norm_rows(f.clone())                                                    # cached features in place of encode_image under no_grad
        loss = torch.nn.functional.cross_entropy(adapter.logits(feats, None, w, 1.0, 5.5, seg=seg, layout="nd"), labels)
        losses.append(float(loss))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        scheduler.step()
    print("losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0] and all(np.isfinite(losses))


def test_run_tip_adapter_F_end_to_end():
    """A TINY tower (embed_dim 64) encodes two batches of synthetic images per epoch; cache, val and test features are a 37 x 4-shot split at D = 64."""
    from conftest import TINY
    from proto_clip_amd import synth, tip_adapter
    from proto_clip_amd.clip.model import build_model, random_state_dict
    model = build_model(random_state_dict(seed=5, **TINY)).cuda()
    s = ref.tip_split(37, [4] * 37, 64, 130, seed=23, sigma=2.0)
    f, keys, w = s["features"].cuda(), s["keys"].cuda(), s["text"].cuda()
    values = torch.nn.functional.one_hot(s["key_labels"], 37).cuda()
    y = synth.randint(16, 37, 3, 9)
    imgs = synth.make_images(16, TINY["image_resolution"], seed=4, labels=y)
    loader = [(imgs[:8], torch.from_numpy(y[:8])), (imgs[8:], torch.from_numpy(y[8:]))]
    cfg = {"init_alpha": 1.0, "init_beta": 5.5, "search_scale": [7, 3], "search_step": [20, 10], "lr": 1e-3, "train_epoch": 2}
    val_f, val_y, test_f, test_y = f[:66], s["labels"][:66].cuda(), f[66:], s["labels"][66:].cuda()
    res = tip_adapter.run_tip_adapter_F(cfg, keys.t().contiguous(), values, val_f, val_y, test_f, test_y, w.t().contiguous(), model, loader)
    adapter = res["adapter"]
    assert len(res["epochs"]) == 2 and all(np.isfinite(e["loss"]) for e in res["epochs"]) and res["grid"].shape == (200, 3)
    assert not torch.equal(adapter.weight.detach(), keys) or res["best_epoch"] == 0
    ex = ref.Exact(test_f.cpu(), adapter.weight.detach().cpu(), s["seg"], s["text"])          # float64 on the trained keys
    r = ex.at(res["best_alpha"], res["best_beta"])
    want, tie = ref.near_ties(r["v"], r["tol16"])
    acc64 = 100.0 * int((want == test_y.cpu()).sum()) / 64
    assert abs(res["tip_f_test_acc"] - acc64) * 64 / 100.0 <= int(tie.sum()) + 1e-9, (res["tip_f_test_acc"], acc64, int(tie.sum()))


# ---- every compiled variant is launched: the widest panels, the grid's 32-row panels, the wider backward register panels -------------------------------

WIDE_POINTS = [(1.0, 5.5), (17.0, 1.0), (50.0, 50.0)]


@pytest.mark.parametrize("name", list(ref.WIDE_CASES))
def test_widest_forward_panels(name):
    """Q past the launcher's threshold: 64-row panels at D = 512, 32-row panels at D = 1024.  Per element against float64, the argmax rules, and bit for bit
    against the same rows sent alone or in a small batch (16-row panels)."""
    from proto_clip_amd import ops, utils
    f, keys, seg, w = dev(name)
    Q = f.shape[0]
    for alpha, beta in WIDE_POINTS:
        r = at(name, alpha, beta)
        l16, l32, am = ops.tip_logits(f, keys, seg, w, alpha, beta, want_f32=True, want_argmax=True, layout="nd")
        _, _, am_only = ops.tip_logits(f, keys, seg, w, alpha, beta, want_logits=False, want_argmax=True, layout="nd")
        r16 = observe("tip logits fp16 (widest panels): |got - float64| / derived tolerance", ref.worst_ratio(l16, r["v"], r["tol16"]), 1.0)
        r32 = observe("tip logits fp32 (widest panels): |got - float64| / derived tolerance", ref.worst_ratio(l32, r["v"], r["tol32"]), 1.0)
        want, tie = ref.near_ties(r["v"], r["tol16"])
        share = observe("tip argmax: share of proven near-ties in a case", float(tie.double().mean()), NEAR_TIE_CAP)
        wrong = am.cpu().long() != want
        print(name, alpha, beta, "fp16", round(r16, 4), "fp32", round(r32, 5), "near-ties", int(tie.sum()), "argmax differs", int(wrong.sum()))
        assert r16 <= 1.0 and r32 <= 1.0 and share <= NEAR_TIE_CAP, (name, alpha, beta, r16, r32, share)
        assert torch.equal(l16.cpu(), l32.half().cpu()) and torch.equal(am.cpu().long(), first_argmax(l16)) and torch.equal(am_only, am)
        assert not bool((wrong & ~tie).any())
        for lo, hi in ((0, 1), (Q - 1, Q), (1000, 1037)):                                     # the same rows in 16-row panels
            s16, s32, sam = ops.tip_logits(f[lo:hi], keys, seg, w, alpha, beta, want_f32=True, want_argmax=True, layout="nd")
            assert torch.equal(s16, l16[lo:hi]) and torch.equal(s32, l32[lo:hi]) and torch.equal(sam, am[lo:hi]), (name, lo, hi)
    assert torch.equal(ops.tip_logits(f, keys, seg, w, 0.0, 5.5, layout="nd")[0].contiguous(), utils.clip_logits(f, w, layout="nd"))


@pytest.mark.parametrize("name", ["many", "wide512", "wide1024"])
def test_grid_on_32_row_panels(name):
    """ceil(Q / 32) * (beta chunks) >= 512: the grid kernel keeps its 32-row panels (D = 512 and D = 1024; 5 betas are at least 2 chunks at any chunk size up
    to 4).  Exactly the single calls; float64 up to near-ties."""
    from proto_clip_amd import ops
    betas, alphas = [0.1, 1.0, 5.5, 7.0, 50.0], [0.1, 1.0, 17.0]
    f, keys, seg, w = dev(name)
    assert -(-f.shape[0] // 32) * 2 >= 512
    got = ops.tip_grid(f, keys, seg, w, betas, alphas, ref.case(name)["labels"].cuda(), layout="nd").cpu().numpy()
    assert np.array_equal(got, single_counts(name, betas, alphas))
    want, ties = float64_counts(name, betas, alphas)
    excess = observe("tip grid: |count - float64 count| - proven near-ties at a pair (<= 0)", float((np.abs(got - want) - ties).max()), 0.0)
    assert excess <= 0


def test_no_cache_rows_at_all():
    """NK = 0 (every class empty, no key pointer): the logits are the zero-shot ones at any alpha, the grid counts the zero-shot hits."""
    from proto_clip_amd import ops, utils
    f, keys, seg, w = dev("pets")
    seg0 = torch.zeros_like(seg)
    l16, l32, am = ops.tip_logits(f, keys[:0], seg0, w, 17.0, 1.0, want_f32=True, want_argmax=True, layout="nd")
    zs = utils.clip_logits(f, w, layout="nd")
    assert torch.equal(l16.contiguous(), zs) and torch.equal(l32.half(), zs) and torch.equal(am.cpu().long(), first_argmax(zs))
    lab = ref.case("pets")["labels"].cuda()
    got = ops.tip_grid(f, keys[:0], seg0, w, [0.1, 5.5], [0.1, 3.0], lab, layout="nd")
    assert bool((got == int((am.long() == lab).sum())).all())
    dk = ops.tip_keys_backward(f, keys[:0], seg0, torch.ones(f.shape[0], 37, device="cuda"), 1.0, 5.5, layout="nd")
    assert tuple(dk.shape) == (0, 512)


def cut_cache(name, nclasses):
    """The case with only its first `nclasses` classes holding rows (the later ones empty; N and the queries stay): (Exact, key rows, seg) ."""
    s = ref.case(name)
    end = int(s["seg"][nclasses])
    seg = torch.clamp(s["seg"], max=end)
    return ref.Exact(s["features"], s["keys"][:end], seg, s["text"]), dev(name)[1][:end], seg.cuda()


# (case, classes kept | None) -> the register panel the launcher takes: D = 1024 with 32 and 16 key rows per panel, D = 2048, and D = 512 with NK in 17 .. 32
@pytest.mark.parametrize("name,kept", [("caltech1", None), ("caltech1", 10), ("d2048", None), ("pets", 6), ("eurosat", 2)])
def test_key_gradient_on_the_other_register_panels(name, kept):
    from proto_clip_amd import ops
    s = ref.case(name)
    f = dev(name)[0]
    ex, keys, seg = (exact(name), dev(name)[1], dev(name)[2]) if kept is None else cut_cache(name, kept)
    assert kept is None or 1 <= keys.shape[0] <= 32
    for alpha, beta in BWD_POINTS:
        v = ex.at(alpha, beta)["v"]
        dL = ref.ce_grad(v, s["labels"])[0]
        want, tol = ref.keys_backward(ex, alpha, beta, dL)
        got = ops.tip_keys_backward(f, keys, seg, dL.cuda(), alpha, beta, layout="nd")
        r = observe("tip dkeys: |got - float64| / derived tolerance", ref.worst_ratio(got, want, tol), 1.0)
        print(name, kept, alpha, beta, "NK", keys.shape[0], "dkeys", round(r, 4), "max |dkeys|", float(want.abs().max()))
        assert r <= 1.0 and float(want.abs().max()) > 0, (name, kept, alpha, beta, r)
        assert torch.equal(got, ops.tip_keys_backward(f, keys, seg, dL.cuda(), alpha, beta, layout="nd"))
    if kept is not None:                                                                     # the rows' bits inside the whole cache (a wider panel there)
        full = ops.tip_keys_backward(f, dev(name)[1], dev(name)[2], dL.cuda(), alpha, beta, layout="nd")
        assert torch.equal(got, full[:keys.shape[0]])
