"""pclip_cosine_ce_f16 / pclip_cosine_ce_backward_f16 (csrc/pclip_cosine_ce.hip), ops.cosine_cross_entropy(_backward), autograd.CosineCeFn and the losses of
utils / CLIP built on them, against the float64 helper tests/cosine_ce_ref.py under ITS derived tolerances (loss and lse: the logit error plus 2^-20;
gradients: elementwise, from the fp16 rounding of the exp tile and the fp32 sums, c = 2), and against the kernels' own invariances bit for bit.

Shapes: a panel is 16 RF rows (RF = 1, 2, 4 by the row count; at most 4 up to D = 512, 2 up to 1024, 1 beyond; the forward takes the wider ones only once
there are 256 panels) walked in blocks of 64 columns by eight waves; the backward walks tiles of 64 rows of the other side, each of four waves owning a
quarter of D, and shares the tiles between workgroups in chunks where the panels are few (symmetric 65 and 200, the class gradient of (130, 70)).  (3, 5), (17, 37), (33, 100), (130, 70) are one past 0 / 16 / 32 /
128 rows and off every 64-column block; (64, 1000, 1024) and (20, 65, 2048) run the RF caps of the two wider register panels; 65 / 200 / 512 symmetric rows
are 2, 4 and 8 panels whose column partials are merged across workgroups."""
import numpy as np
import pytest
import torch

from conftest import observe
from contrastive_ref import grade, scaled_rows
from cosine_ce_ref import cluster_labels, clustered, reference, worst_ratio

pytestmark = pytest.mark.gpu

SCALES = [100.0, 14.2857]
LABELLED = [(1, 1, 64), (3, 5, 64), (17, 37, 128), (33, 100, 512), (130, 70, 64), (64, 1000, 1024), (20, 65, 2048)]
SYMMETRIC = [(1, 64), (65, 64), (200, 64), (200, 512), (512, 1024)]

_CASES = {}


def case(M, T, D):
    """fp16 operands and labels on the host, shared between the tests (never modified)."""
    key = (M, T, D)
    if key not in _CASES:
        a, b = clustered(M, T, D, 7 + M)
        _CASES[key] = (a, b, cluster_labels(M, T, 3 + M))
    return _CASES[key]


_REFS = {}


def gpu_reference(a, b, scale, labels=None, symmetric=False, na=False, nb=False):
    """The float64 helper on the kernels' own a' / b': where a side is normalised, the rows ops.l2norm_rows gives (the definition of a' / b')."""
    from proto_clip_amd import ops
    unit = lambda x, on: ops.l2norm_rows(x.cuda().contiguous()).cpu() if on else None
    return reference(a, b, scale, labels, symmetric, na, nb, a_unit16=unit(a, na), b_unit16=unit(b, nb))


def ref_of(key, a, b, scale, labels, symmetric, na, nb):
    if key not in _REFS:
        _REFS[key] = gpu_reference(a, b, scale, labels, symmetric, na, nb)
    return _REFS[key]


def run(a, b, scale, labels=None, symmetric=False, na=False, nb=False):
    from proto_clip_amd import ops
    loss, lse_row, lse_col, rows = ops.cosine_cross_entropy(a, b, scale, labels, symmetric, na, nb, want_rows=True)
    da, db, ds = ops.cosine_cross_entropy_backward(a, b, scale, lse_row, lse_col, labels, symmetric, na, nb)
    return dict(loss=loss, lse_row=lse_row, lse_col=lse_col, rows=rows, da=da, db=db, dscale=ds)


def check(tag, got, ref):
    """Every delivered item against the float64 helper; the figures are recorded before anything is asserted."""
    items = [("loss", "tol_loss"), ("lse_row", "tol_loss"), ("rows", "tol_loss"), ("da", "tol_da"), ("db", "tol_db"), ("dscale", "tol_dscale")]
    if ref["lse_col"] is not None:
        items.append(("lse_col", "tol_loss"))
    ratios = {}
    for name, tol in items:
        ratios[name] = observe(f"cosine ce {name}: |got - float64| / derived tolerance", worst_ratio(got[name], ref[name], ref[tol]), 1.0)
    print(tag, {k: round(v, 4) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)


def guarded(x, pad):
    """The rows of x as a strided view of a wider buffer with NaN in the padding columns and in two guard rows."""
    buf = torch.full((x.shape[0] + 2, x.shape[1] + pad), float("nan"), dtype=torch.float16)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf.cuda()[:x.shape[0], :x.shape[1]]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M,T,D", LABELLED)
def test_labelled_against_float64(M, T, D, scale):
    a, b, labels = case(M, T, D)
    ad, bd = guarded(a, 8), guarded(b, 16)
    lab = labels.cuda() if M % 2 else labels.int().cuda()                            # int64 and int32 labels
    for na, nb in ((False, False), (True, False), (False, True), (True, True)):
        ref = ref_of(("lab", M, T, D, scale, na, nb), a, b, scale, labels, False, na, nb)
        check(f"labelled {M}x{T}x{D} scale {scale} norm {int(na)}{int(nb)}", run(ad, bd, scale, lab, False, na, nb), ref)


def test_a_tall_batch_runs_the_widest_forward_panel():
    """The forward takes 64-row panels only once there are 256 of them (M >= 16 384), 32-row panels from M = 8192 (test_no_m_by_t_tensor_in_memory); three
    classes keep the float64 side small.  The first rows keep the bits they have in a 17-row call."""
    from proto_clip_amd import ops
    a, b, labels = case(16400, 3, 64)
    ref = ref_of(("lab", 16400, 3, 64, 100.0, True, False), a, b, 100.0, labels, False, True, False)
    ad, bd, lab = a.cuda(), b.cuda(), labels.cuda()
    check("labelled 16400x3x64", run(ad, bd, 100.0, lab, False, True, False), ref)
    tall = ops.cosine_cross_entropy(ad, bd, 100.0, lab, normalize_a=True, want_rows=True)
    short = ops.cosine_cross_entropy(ad[:17], bd, 100.0, lab[:17], normalize_a=True, want_rows=True)
    assert torch.equal(tall[1][:17], short[1]) and torch.equal(tall[3][:17], short[3])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("M,D", SYMMETRIC)
def test_symmetric_against_float64(M, D, scale):
    a, b, _ = case(M, M, D)
    ref = ref_of(("sym", M, D, scale), a, b, scale, None, True, True, True)
    ad, bd = a.cuda(), b.cuda()
    got = run(ad, bd, scale, None, True, True, True)
    check(f"symmetric {M}x{D} scale {scale}", got, ref)
    # b, a instead of a, b: the same loss, the gradients exchanged
    swapped = run(bd, ad, scale, None, True, True, True)
    sref = dict(ref, lse_row=ref["lse_col"], lse_col=ref["lse_row"], da=ref["db"], db=ref["da"], tol_da=ref["tol_db"], tol_db=ref["tol_da"])
    check(f"symmetric {M}x{D} scale {scale}, operands exchanged", swapped, sref)
    if M > 1:
        plain = ref_of(("sym plain", M, D, scale), a, b, scale, None, True, False, False)
        check(f"symmetric {M}x{D} scale {scale}, rows as given", run(ad, bd, scale, None, True, False, False), plain)


def test_padding_never_counts():
    """All rows of b identical: every lse_row is s + log 65 — a clamped or padded column counted once would move it by log(66 / 65) = 0.015.  Mirrored for the
    column statistic of symmetric mode with all rows of a identical."""
    from proto_clip_amd import ops
    a, b, labels = case(17, 65, 128)
    b1 = b[:1].expand(65, -1).contiguous()
    ref = reference(a, b1, 100.0, labels[:17] % 65, False, False, False)
    _, lse_row, _ = ops.cosine_cross_entropy(a.cuda(), b1.cuda(), 100.0, (labels[:17] % 65).cuda())
    want = ref["s"][:, 0] + np.log(65.0)
    r = observe("cosine ce lse_row over identical columns / tolerance", worst_ratio(lse_row, want, ref["tol_loss"]), 1.0)
    assert r <= 1.0 and 10 * float(ref["tol_loss"]) < np.log(66 / 65), (r, float(ref["tol_loss"]))     # (the miscount is ten tolerances away)
    a65, b65, _ = case(65, 65, 64)
    a1 = a65[:1].expand(65, -1).contiguous()
    ref = reference(a1, b65, 100.0, None, True, False, False)
    _, _, lse_col = ops.cosine_cross_entropy(a1.cuda(), b65.cuda(), 100.0, symmetric=True)
    want = ref["s"][0, :] + np.log(65.0)
    r = observe("cosine ce lse_col over identical rows / tolerance", worst_ratio(lse_col, want, ref["tol_loss"]), 1.0)
    assert r <= 1.0 and 10 * float(ref["tol_loss"]) < np.log(66 / 65), (r, float(ref["tol_loss"]))     # (the miscount is ten tolerances away)


def test_extremes_at_scale_100():
    """35 unit rows and their antipodes as both the classes and the samples (each three times): a sure sample has its target logit at 100 against
    -100 from the antipode, loss and gradient ~ 0; T = 70 is off the 64-column block with targets in the last column; then all labels equal."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(35, 64, generator=g)
    v = (v / v.norm(dim=1, keepdim=True)).half()
    b = torch.cat([v, -v])                                                           # 70 classes, class t + 35 antipodal to class t
    a = b.repeat(3, 1)                                                               # 210 samples
    sure = torch.arange(210) % 70
    for tag, labels in (("sure", sure), ("target in the last column", torch.full((210,), 69)), ("all labels 0", torch.zeros(210, dtype=torch.long))):
        ref = gpu_reference(a, b, 100.0, labels, False, True, True)
        got = run(a.cuda(), b.cuda(), 100.0, labels.cuda(), False, True, True)
        for name in ("loss", "rows", "da", "db", "dscale"):
            assert bool(torch.isfinite(got[name]).all()), (tag, name)
        check(f"extremes, {tag}", got, ref)
        if tag == "sure":
            assert float(got["loss"]) < 1e-4 and float(got["rows"].abs().max()) < 1e-4      # (a wrong sample's term is ~ 100, its gradient ~ 100 / 210 |b'|)
            assert float(got["da"].abs().max()) < 1e-4 and float(got["dscale"].abs()) < 1e-4
        else:
            assert float(got["loss"]) > 50.0                                         # most samples are far from the one class they are all given


def test_batch_independence_and_determinism_bitwise():
    from proto_clip_amd import ops
    a, b, labels = case(130, 70, 64)
    ad, bd, lab = a.cuda(), b.cuda(), labels.cuda()
    for na in (False, True):
        _, lse_big, _, rows_big = ops.cosine_cross_entropy(ad, bd, 100.0, lab, normalize_a=na, want_rows=True)
        _, lse_small, _, rows_small = ops.cosine_cross_entropy(ad[:17], bd, 100.0, lab[:17], normalize_a=na, want_rows=True)
        assert torch.equal(lse_big[:17], lse_small) and torch.equal(rows_big[:17], rows_small)
        da_big, _, _ = ops.cosine_cross_entropy_backward(ad, bd, 100.0, lse_big, None, lab, normalize_a=na, want_b=False, want_scale=False)
        da_small, _, _ = ops.cosine_cross_entropy_backward(ad[:17], bd, 100.0, lse_small, None, lab[:17], normalize_a=na, want_b=False, want_scale=False,
                                                           mean_over=130)
        assert torch.equal(da_big[:17], da_small)
    s, t, _ = case(200, 200, 64)
    first = run(s.cuda(), t.cuda(), 100.0, None, True, True, True)
    second = run(s.cuda(), t.cuda(), 100.0, None, True, True, True)
    for name, x in first.items():
        assert torch.equal(x, second[name]), name


def test_autograd_surface():
    from proto_clip_amd import utils
    feats, w, labels = case(33, 100, 512)
    ref = ref_of(("lab", 33, 100, 512, 100.0, False, False), feats, w, 100.0, labels, False, False, False)
    lab = labels.cuda()
    for layout, weights in ((None, w.cuda().t().contiguous()), (None, w.cuda()), ("nd", w.cuda()), ("dn", w.cuda().t().contiguous())):
        f = feats.cuda().requires_grad_(True)
        wt = weights.clone().requires_grad_(True)
        loss = utils.clip_logits_loss(f, wt, lab, layout=layout)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
        loss.backward()
        assert f.grad.dtype == torch.float16 and wt.grad.dtype == torch.float16 and wt.grad.shape == weights.shape
        gw = wt.grad if weights.shape == w.shape else wt.grad.t()
        half = lambda name, x, tol: observe(f"cosine ce autograd {name} / (tolerance + fp16 rounding)", worst_ratio(x, ref[name], ref[tol] + ref[name].abs() * 2.0 ** -11), 1.0)
        assert worst_ratio(loss, ref["loss"], ref["tol_loss"]) <= 1.0
        assert half("da", f.grad, "tol_da") <= 1.0 and half("db", gw, "tol_db") <= 1.0   # (the fp16 gradient adds one rounding, unit 2^-11)
    with torch.no_grad():
        quiet = utils.clip_logits_loss(feats.cuda().requires_grad_(True), w.cuda(), lab)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, loss.detach())
    # fp32 leaves cast to fp16 on the way in get fp32 gradients from torch's own cast node
    w32 = w.float().cuda().requires_grad_(True)
    utils.clip_logits_loss(feats.cuda(), w32.half(), lab, layout="nd").backward()
    assert w32.grad.dtype == torch.float32 and worst_ratio(w32.grad, ref["db"], ref["tol_db"] + ref["db"].abs() * 2.0 ** -11) <= 1.0
    # a tensor scale that requires grad
    img, txt, _ = case(65, 65, 64)
    sref = ref_of(("sym", 65, 64, 14.2857), img, txt, 14.2857, None, True, True, True)
    scale = torch.tensor(14.2857, device="cuda", requires_grad=True)
    i16, t16 = img.cuda().requires_grad_(True), txt.cuda().requires_grad_(True)
    loss = utils.clip_contrastive_loss(i16, t16, scale)
    loss.backward()
    assert worst_ratio(loss, sref["loss"], sref["tol_loss"]) <= 1.0
    assert scale.grad.dtype == torch.float32 and scale.grad.dim() == 0 and worst_ratio(scale.grad, sref["dscale"], sref["tol_dscale"]) <= 1.0
    assert worst_ratio(i16.grad, sref["da"], sref["tol_da"] + sref["da"].abs() * 2.0 ** -11) <= 1.0
    assert worst_ratio(t16.grad, sref["db"], sref["tol_db"] + sref["db"].abs() * 2.0 ** -11) <= 1.0


def test_clip_contrastive_loss_trains_the_temperature():
    from proto_clip_amd.clip.model import build_model, random_state_dict
    kw = dict(embed_dim=64, image_resolution=32, vision_layers=2, vision_width=128, vision_patch_size=8, context_length=77,
              vocab_size=512, transformer_width=64, transformer_heads=1, transformer_layers=2)
    model = build_model(random_state_dict(seed=11, **kw)).cuda()
    from proto_clip_amd import synth
    g = torch.Generator().manual_seed(2)
    images = synth.make_images(8, 32, seed=5, n_class=8).cuda()
    tokens = torch.zeros(8, 77, dtype=torch.long)                                    # start token, a random body, the end token (the highest id), zero padding
    for i in range(8):
        n = 4 + 2 * i
        tokens[i, 0], tokens[i, n] = 510, 511
        tokens[i, 1:n] = torch.randint(1, 510, (n - 1,), generator=g)
    with torch.no_grad():
        fi, ft = model.encode_image(images), model.encode_text(tokens.cuda())
    assert not model.logit_scale.requires_grad
    frozen = model.contrastive_loss(fi, ft)
    assert frozen.grad_fn is None
    model.logit_scale.requires_grad_(True)
    loss = model.contrastive_loss(fi.detach(), ft.detach())
    loss.backward()
    scale = float(model.logit_scale.detach().float().exp())
    ref = gpu_reference(fi.cpu(), ft.cpu(), scale, None, True, True, True)
    assert worst_ratio(loss, ref["loss"], ref["tol_loss"]) <= 1.0 and torch.equal(loss.detach(), frozen)
    # d loss / d logit_scale = dscale * exp(logit_scale): torch's own exp node
    want, tol = ref["dscale"] * scale, ref["tol_dscale"] * scale + ref["dscale"].abs() * scale * 2.0 ** -22
    assert model.logit_scale.grad is not None and worst_ratio(model.logit_scale.grad, want, tol) <= 1.0


def test_a_short_descent_follows_float64():
    """20 steps of plain SGD on an [N, D] classifier from a seeded start.  The float64 helper takes its own 20 steps on the CPU from the same start, with the
    same fp16 rounding of the gradient and of the weights after each step: the loss of every step is within the loss tolerance of the helper's."""
    from proto_clip_amd import utils
    feats, w0, _ = case(256, 37, 512)
    labels = torch.arange(256) % 37
    lr, scale = 0.05, 14.2857
    fd, lab = feats.cuda(), labels.cuda()
    w = w0.clone().cuda().requires_grad_(True)
    w64, losses, ratios = w0.clone(), [], []
    for step in range(21):
        loss = utils.clip_logits_loss(fd, w, lab, scale=scale, layout="nd")
        ref = reference(feats, w64, scale, labels)
        losses.append((float(loss), float(ref["loss"])))
        ratios.append(observe("cosine ce descent: |loss - float64 trajectory| / tolerance", worst_ratio(loss, ref["loss"], ref["tol_loss"]), 1.0))
        loss.backward()
        with torch.no_grad():
            w.copy_((w.float() - lr * w.grad.float()).half())
            w.grad = None
        w64 = (w64.float() - lr * ref["db"].half().float()).half()
    print("descent (kernel, float64):", [(round(x, 5), round(y, 5)) for x, y in losses], [round(r, 3) for r in ratios])
    assert max(ratios) <= 1.0, ratios
    assert losses[20][0] < losses[0][0] and losses[20][1] < losses[0][1]


def test_no_m_by_t_tensor_in_memory():
    from proto_clip_amd import ops
    M, D = 8192, 512
    g = torch.Generator().manual_seed(1)
    a = (torch.randn(M, D, generator=g) / D ** 0.5).half().cuda()
    b = (a.float() + 0.5 * torch.randn(M, D, generator=g).cuda() / D ** 0.5).half()
    ops.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = run(a, b, 14.2857, None, True, True, True)
    torch.cuda.synchronize()
    outputs = sum(x.numel() * x.element_size() for x in got.values())
    growth = torch.cuda.max_memory_allocated() - base - outputs
    observe("cosine ce 8192^2 x 512: peak growth over operands and gradients / (M T 2 bytes)", growth / (M * M * 2), 1.0)
    assert growth < M * M * 2, growth
    assert bool(torch.isfinite(got["loss"])) and 0.0 < float(got["loss"]) < 2 * np.log(M)
    ops.release_workspaces()


def test_forward_and_backward_capture_in_one_graph():
    a, b, _ = case(65, 65, 64)
    ad, bd = a.cuda(), b.cuda()
    eager = run(ad, bd, 100.0, None, True, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(ad, bd, 100.0, None, True, True, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = run(ad, bd, 100.0, None, True, True, True)
    for _ in range(2):
        for o in out.values():
            o.zero_()
        gr.replay()
        torch.cuda.synchronize()
        for name, o in out.items():
            assert torch.equal(o, eager[name]), name


@pytest.mark.parametrize("M,T,D", [(17, 37, 128), (130, 1000, 512)])
def test_the_inference_kernel_did_not_move(M, T, D):
    """ops.cosine_logits as tests/test_gpu_contrastive.py grades it (the device code of the row normalisation is shared with the new kernels)."""
    from proto_clip_amd import ops
    g = torch.Generator().manual_seed(1000 + M)
    a = (torch.randn(M, D, generator=g) / D ** 0.5).half()
    b = (torch.randn(T, D, generator=g) / D ** 0.5).half()
    got = ops.cosine_logits(a.cuda(), b.cuda(), 100.0)[0]
    worst, differ = grade(got, scaled_rows(a, 100.0), b)
    assert worst <= 1.0 and differ <= 0.01, (worst, differ)
    fused = ops.cosine_logits(a.cuda(), b.cuda(), 100.0, normalize_a=True, normalize_b=True)[0]
    apart = ops.cosine_logits(ops.l2norm_rows(a.cuda()), ops.l2norm_rows(b.cuda()), 100.0)[0]
    assert torch.equal(fused, apart)
