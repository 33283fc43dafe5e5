"""pclip_cosine_sigmoid_f16 / pclip_cosine_sigmoid_backward_f16 (csrc/pclip_cosine_sigmoid.hip), ops.cosine_sigmoid(_backward), autograd.CosineSigmoidFn and the
losses of utils / CLIP built on them, against the float64 helper tests/cosine_sigmoid_ref.py under ITS derived tolerances, and against the kernels' own
invariances bit for bit.

Shapes: the edges of the cross-entropy tests (tests/test_gpu_cosine_ce.py) — a panel is 16 RF rows walked in blocks of 64 columns by eight waves (forward) or in
tiles of 64 rows of the other side by four waves (backward); (3, 5), (17, 37), (33, 100), (130, 70) are one past 0 / 16 / 32 / 128 rows and off every 64-column
block; (64, 1000, 1024) and (20, 65, 2048) run the two wider register panels; the class gradient of (130, 70) and the diagonal 65 / 200 share their walk between
workgroups in chunks; the row gradient does from 2048 columns on, in chunks T alone decides (40 x 2100, 40 x 4160).  Ids: i % k against j % k, k = min(4, M, T) — every row and column has several positives — with every fifth id of a at -1; int32 on even
M, int64 on odd.  (scale, bias): SigLIP's start (10, -10), all logits negative; (14.2857, -5), positives above zero and negatives below; (100, -95), where three
quarters of sigma fall below 2^-28: the scaled fp16 tile and its flush to zero."""
import pytest
import torch

from conftest import observe
from cosine_sigmoid_ref import case_ids, clustered, reference, worst_ratio

pytestmark = pytest.mark.gpu

PAIRS = [(10.0, -10.0), (14.2857, -5.0), (100.0, -95.0)]
RECTANGULAR = [(1, 1, 64), (3, 5, 64), (17, 37, 128), (33, 100, 512), (130, 70, 64), (64, 1000, 1024), (20, 65, 2048)]
DIAGONAL = [(1, 64), (65, 64), (200, 64), (200, 512), (512, 1024)]
NORMS = ((False, False), (True, False), (False, True), (True, True))

_CASES, _REFS = {}, {}


def case(M, T, D):
    """fp16 operands and ids on the host, shared between the tests (never modified)."""
    key = (M, T, D)
    if key not in _CASES:
        a, b = clustered(M, T, D, 7 + M)
        _CASES[key] = (a, b) + case_ids(M, T, M % 2 == 1)
    return _CASES[key]


def gpu_reference(a, b, scale, bias, ia=None, ib=None, na=False, nb=False):
    """The float64 helper on the kernels' own a' / b': where a side is normalised, the rows ops.l2norm_rows gives (the definition of a' / b')."""
    from proto_clip_amd import ops
    unit = lambda x, on: ops.l2norm_rows(x.cuda().contiguous()).cpu() if on else None
    return reference(a, b, scale, bias, ia, ib, na, nb, a_unit16=unit(a, na), b_unit16=unit(b, nb))


def ref_of(key, *args):
    if key not in _REFS:
        _REFS[key] = gpu_reference(*args)
    return _REFS[key]


def run(a, b, scale, bias, ia=None, ib=None, na=False, nb=False):
    """Everything the two entry points deliver; the scalars from either direction."""
    from proto_clip_amd import ops
    loss, rows = ops.cosine_sigmoid(a, b, scale, bias, ia, ib, na, nb, want_rows=True)
    da, _, ds0, dbi0 = ops.cosine_sigmoid_backward(a, b, scale, bias, ia, ib, na, nb, want_b=False)
    _, db, ds1, dbi1 = ops.cosine_sigmoid_backward(a, b, scale, bias, ia, ib, na, nb, want_a=False)
    return dict(loss=loss, rows=rows, da=da, db=db, dscale=ds0, dbias=dbi0, dscale_from_b=ds1, dbias_from_b=dbi1)


ITEMS = [("loss", "loss", "tol_loss"), ("rows", "rows", "tol_rows"), ("da", "da", "tol_da"), ("db", "db", "tol_db"), ("dscale", "dscale", "tol_dscale"),
         ("dbias", "dbias", "tol_dbias"), ("dscale_from_b", "dscale", "tol_dscale"), ("dbias_from_b", "dbias", "tol_dbias")]


def check(tag, got, ref):
    """Every delivered item against the float64 helper; the figures are recorded before anything is asserted."""
    ratios = {}
    for name, want, tol in ITEMS:
        ratios[name] = observe(f"cosine sigmoid {name}: |got - float64| / derived tolerance", worst_ratio(got[name], ref[want], ref[tol]), 1.0)
    print(tag, {k: round(v, 4) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)


def guarded(x, pad):
    """The rows of x as a strided view of a wider buffer with NaN in the padding columns and in two guard rows."""
    buf = torch.full((x.shape[0] + 2, x.shape[1] + pad), float("nan"), dtype=torch.float16)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf.cuda()[:x.shape[0], :x.shape[1]]


@pytest.mark.parametrize("scale,bias", PAIRS)
@pytest.mark.parametrize("M,T,D", RECTANGULAR)
def test_rectangular_against_float64(M, T, D, scale, bias):
    a, b, ia, ib = case(M, T, D)
    ad, bd, iad, ibd = guarded(a, 8), guarded(b, 16), ia.cuda(), ib.cuda()
    for na, nb in NORMS:
        ref = ref_of(("ids", M, T, D, scale, bias, na, nb), a, b, scale, bias, ia, ib, na, nb)
        check(f"ids {M}x{T}x{D} ({scale}, {bias}) norm {int(na)}{int(nb)}", run(ad, bd, scale, bias, iad, ibd, na, nb), ref)


@pytest.mark.parametrize("scale,bias", PAIRS)
@pytest.mark.parametrize("n,D", DIAGONAL)
def test_diagonal_against_float64(n, D, scale, bias):
    a, b, _, _ = case(n, n, D)
    ad, bd = guarded(a, 16), guarded(b, 8)
    for na, nb in NORMS:
        ref = ref_of(("diag", n, D, scale, bias, na, nb), a, b, scale, bias, None, None, na, nb)
        check(f"diagonal {n}x{D} ({scale}, {bias}) norm {int(na)}{int(nb)}", run(ad, bd, scale, bias, None, None, na, nb), ref)


def test_two_calls_give_the_same_bits():
    a, b, ia, ib = case(130, 70, 64)
    args = (a.cuda(), b.cuda(), 14.2857, -5.0, ia.cuda(), ib.cuda(), True, True)
    first, second = run(*args), run(*args)
    for name, x in first.items():
        assert torch.equal(x, second[name]), name
    s, t, _, _ = case(200, 200, 64)
    first, second = run(s.cuda(), t.cuda(), 100.0, -95.0, None, None, True, True), run(s.cuda(), t.cuda(), 100.0, -95.0, None, None, True, True)
    for name, x in first.items():
        assert torch.equal(x, second[name]), name


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_ids_are_arange_ids_bitwise(dtype):
    a, b, _, _ = case(200, 200, 64)
    ad, bd = a.cuda(), b.cuda()
    ar = torch.arange(200, dtype=dtype, device="cuda")
    plain, ids = run(ad, bd, 14.2857, -5.0, None, None, True, False), run(ad, bd, 14.2857, -5.0, ar, ar.clone(), True, False)
    for name, x in plain.items():
        assert torch.equal(x, ids[name]), name


def test_one_vs_rest_is_the_generic_call_bitwise():
    from proto_clip_amd import ops, utils
    feats, w, _, _ = case(33, 100, 512)
    labels = (torch.arange(33) * 7) % 100
    labels[5] = -1                                                                   # a sample of no class
    fd, wd, lab = feats.cuda(), w.cuda(), labels.cuda()
    classes = torch.arange(100, device="cuda")
    want = ops.cosine_sigmoid(fd, wd, 100.0, -95.0, lab, classes)
    gda, gdb, _, _ = ops.cosine_sigmoid_backward(fd, wd, 100.0, -95.0, lab, classes, want_scale=False, want_bias=False)
    for layout, weights in (("nd", wd), ("dn", wd.t().contiguous()), (None, wd)):
        f, wt = fd.clone().requires_grad_(True), weights.clone().requires_grad_(True)
        loss = utils.clip_logits_sigmoid_loss(f, wt, lab, scale=100.0, bias=-95.0, layout=layout)
        assert torch.equal(loss.detach(), want) and loss.grad_fn is not None
        loss.backward()
        gw = wt.grad if weights.shape == w.shape else wt.grad.t()
        assert torch.equal(f.grad, gda.half()) and torch.equal(gw, gdb.half())
    ref = gpu_reference(feats, w, 100.0, -95.0, labels, torch.arange(100))
    assert worst_ratio(want, ref["loss"], ref["tol_loss"]) <= 1.0


def test_a_slice_of_the_batch_keeps_its_bits():
    """Rows 16..47 of a alone: their row terms, and with mean_over = M their rows of dL/da, whatever the rest of the batch."""
    from proto_clip_amd import ops
    a, b, ia, ib = case(130, 70, 64)
    ad, bd, iad, ibd = a.cuda(), b.cuda(), ia.cuda(), ib.cuda()
    for na in (False, True):
        _, rows_big = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, iad, ibd, normalize_a=na, want_rows=True)
        _, rows_small = ops.cosine_sigmoid(ad[16:48], bd, 14.2857, -5.0, iad[16:48], ibd, normalize_a=na, want_rows=True)
        assert torch.equal(rows_big[16:48], rows_small)
        da_big = ops.cosine_sigmoid_backward(ad, bd, 14.2857, -5.0, iad, ibd, normalize_a=na, want_b=False, want_scale=False, want_bias=False)[0]
        da_small = ops.cosine_sigmoid_backward(ad[16:48], bd, 14.2857, -5.0, iad[16:48], ibd, normalize_a=na, want_b=False, want_scale=False, want_bias=False,
                                               mean_over=130)[0]
        assert torch.equal(da_big[16:48], da_small)


@pytest.mark.parametrize("T", [2100, 4160])
def test_a_wide_batch_shares_the_row_gradient_walk(T):
    """From 2048 columns on the walk of dL/da is shared between workgroups in chunks whose number T alone decides (2 at 2100, 4 — the most — at 4160): every item
    against float64, and a slice of the rows still keeps its bits."""
    from proto_clip_amd import ops
    a, b, ia, ib = case(40, T, 64)
    ref = ref_of(("ids", 40, T, 64, 14.2857, -5.0, True, True), a, b, 14.2857, -5.0, ia, ib, True, True)
    ad, bd, iad, ibd = a.cuda(), b.cuda(), ia.cuda(), ib.cuda()
    got = run(ad, bd, 14.2857, -5.0, iad, ibd, True, True)
    check(f"ids 40x{T}x64", got, ref)
    part = ops.cosine_sigmoid_backward(ad[16:40], bd, 14.2857, -5.0, iad[16:40], ibd, True, True, want_b=False, want_scale=False, want_bias=False, mean_over=40)[0]
    assert torch.equal(got["da"][16:40], part)


def test_a_tall_batch_runs_the_widest_forward_panel():
    """The forward takes 64-row panels only once there are 256 of them (M > 16 320, the cross-entropy forward's rule); three columns keep the float64 side small.
    The first rows keep the bits they have in a 17-row call."""
    from proto_clip_amd import ops
    a, b, ia, ib = case(16400, 3, 64)
    ref = ref_of(("ids", 16400, 3, 64, 14.2857, -5.0, True, False), a, b, 14.2857, -5.0, ia, ib, True, False)
    ad, bd, iad, ibd = a.cuda(), b.cuda(), ia.cuda(), ib.cuda()
    check("ids 16400x3x64", run(ad, bd, 14.2857, -5.0, iad, ibd, True, False), ref)
    tall = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, iad, ibd, normalize_a=True, want_rows=True)[1]
    short = ops.cosine_sigmoid(ad[:17], bd, 14.2857, -5.0, iad[:17], ibd, normalize_a=True, want_rows=True)[1]
    assert torch.equal(tall[:17], short)


def test_int64_ids_are_compared_in_64_bits():
    from proto_clip_amd import ops
    a, b, _, _ = case(17, 37, 128)
    ad, bd = a.cuda(), b.cuda()
    low_a, low_b = (torch.arange(17) % 4).cuda(), (torch.arange(37) % 4).cuda()
    high = 1 << 32
    none = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, torch.full((17,), -1, device="cuda"), low_b, want_rows=True)
    some = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, low_a, low_b, want_rows=True)
    assert not torch.equal(none[1], some[1])
    # the same low words, different high words: no pair matches
    apart = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, low_a + high, low_b + 2 * high, want_rows=True)
    assert torch.equal(apart[0], none[0]) and torch.equal(apart[1], none[1])
    # equal 64-bit ids beyond 2^32 match as the small ones do
    far = ops.cosine_sigmoid(ad, bd, 14.2857, -5.0, low_a + high, low_b + high, want_rows=True)
    assert torch.equal(far[0], some[0]) and torch.equal(far[1], some[1])
    g_apart = ops.cosine_sigmoid_backward(ad, bd, 14.2857, -5.0, low_a + high, low_b + 2 * high)
    g_none = ops.cosine_sigmoid_backward(ad, bd, 14.2857, -5.0, torch.full((17,), -1, device="cuda"), low_b)
    for x, y in zip(g_apart, g_none):
        assert torch.equal(x, y)


def test_ids_all_negative_have_no_target_term():
    """loss = sum softplus(x) / M, G = w sigma(x): the helper with no positive pair."""
    a, b, _, _ = case(33, 100, 512)
    ia, ib = torch.full((33,), -1), torch.full((100,), -1)                            # -1 == -1, and still no match
    for scale, bias in PAIRS:
        ref = gpu_reference(a, b, scale, bias, ia, ib, True, True)
        assert not bool(ref["y"].any())
        want = torch.nn.functional.softplus(ref["x"]).sum() / 33
        assert abs(float(want) - float(ref["loss"])) <= 1e-12 * float(want)
        check(f"no positives ({scale}, {bias})", run(a.cuda(), b.cuda(), scale, bias, ia.cuda(), ib.cuda(), True, True), ref)


def test_autograd_surface():
    from proto_clip_amd import utils
    img, txt, ia, ib = case(130, 70, 64)
    scale, bias = 14.2857, -5.0
    ref = ref_of(("ids", 130, 70, 64, scale, bias, True, True), img, txt, scale, bias, ia, ib, True, True)
    st, bt = torch.tensor(scale, device="cuda", requires_grad=True), torch.tensor(bias, device="cuda", requires_grad=True)
    i16, t16 = img.cuda().requires_grad_(True), txt.cuda().requires_grad_(True)
    loss = utils.clip_sigmoid_loss(i16, t16, st, bt, ia.cuda(), ib.cuda())
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    loss.backward()
    assert worst_ratio(loss.detach(), ref["loss"], ref["tol_loss"]) <= 1.0
    for name, t in (("dscale", st), ("dbias", bt)):
        assert t.grad.dtype == torch.float32 and t.grad.dim() == 0
        assert observe(f"cosine sigmoid autograd {name} / tolerance", worst_ratio(t.grad, ref[name], ref["tol_" + name]), 1.0) <= 1.0
    # (the fp16 gradient adds one rounding, unit 2^-11)
    half = lambda name, x: observe(f"cosine sigmoid autograd {name} / (tolerance + fp16 rounding)",
                                   worst_ratio(x, ref[name], ref["tol_" + name] + ref[name].abs() * 2.0 ** -11), 1.0)
    assert i16.grad.dtype == torch.float16 and t16.grad.dtype == torch.float16
    assert half("da", i16.grad) <= 1.0 and half("db", t16.grad) <= 1.0
    with torch.no_grad():
        quiet = utils.clip_sigmoid_loss(i16, t16, st, bt, ia.cuda(), ib.cuda())
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, loss.detach())
    # float scalars: constants; fp32 leaves cast to fp16 on the way in get fp32 gradients from torch's own cast node
    t32 = txt.float().cuda().requires_grad_(True)
    utils.clip_sigmoid_loss(img.cuda(), t32.half(), scale, bias, ia.cuda(), ib.cuda()).backward()
    assert t32.grad.dtype == torch.float32 and worst_ratio(t32.grad, ref["db"], ref["tol_db"] + ref["db"].abs() * 2.0 ** -11) <= 1.0


def test_clip_sigmoid_loss_trains_the_towers_and_keeps_the_state_dict():
    from proto_clip_amd import synth
    from proto_clip_amd.clip.model import build_model, random_state_dict
    from spec import TINY
    sd = random_state_dict(seed=5, **TINY)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    assert set(model.state_dict().keys()) == set(sd.keys()) and not any("bias" in k and "logit" in k for k in model.state_dict())
    n, vocab = 4, TINY["vocab_size"]
    g = torch.Generator().manual_seed(4)
    toks = torch.zeros(n, 77, dtype=torch.long)                                       # SOT, a random body, EOT (the highest id), zero padding
    for i in range(n):
        ln = 4 + 2 * i
        toks[i, 0], toks[i, ln] = vocab - 2, vocab - 1
        toks[i, 1:ln] = torch.randint(1, vocab - 2, (ln - 1,), generator=g)
    imgs = synth.make_images(6, TINY["image_resolution"], seed=3, n_class=3).cuda()
    image_ids, text_ids = torch.tensor([0, 0, 1, 1, 2, -1]).cuda(), torch.tensor([0, 1, 2, 7]).cuda()      # two images per class; a text and an image of no partner
    params = model.unfreeze(visual_blocks=1, text_blocks=1)
    logit_bias = torch.tensor(-10.0, device="cuda", requires_grad=True)
    loss = model.sigmoid_loss(model.encode_image(imgs), model.encode_text(toks.cuda()), logit_bias, image_ids, text_ids)
    assert loss.grad_fn is not None and bool(torch.isfinite(loss))
    loss.backward()
    assert len(params) > 0
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.float().abs().max()) > 0.0
    assert logit_bias.grad is not None and bool(torch.isfinite(logit_bias.grad)) and float(logit_bias.grad.abs()) > 0.0
    assert set(model.state_dict().keys()) == set(sd.keys())
    with torch.no_grad():
        fi, ft = model.encode_image(imgs), model.encode_text(toks.cuda())
        quiet = model.sigmoid_loss(fi, ft, -10.0, image_ids, text_ids)
    assert quiet.grad_fn is None
    scale = float(model.logit_scale.detach().float().exp())
    ref = gpu_reference(fi.cpu(), ft.cpu(), scale, -10.0, image_ids.cpu(), text_ids.cpu(), True, True)
    assert worst_ratio(quiet, ref["loss"], ref["tol_loss"]) <= 1.0


def test_the_wrappers_refuse_what_the_kernels_cannot_take():
    from proto_clip_amd import ops
    from proto_clip_amd._lib import PclipError
    a, b, ia, ib = case(17, 37, 128)
    ad, bd, iad, ibd = a.cuda(), b.cuda(), ia.cuda(), ib.cuda()
    bad = [
        lambda f: f(a, b, 10.0, -10.0, ia, ib),                                       # CPU tensors
        lambda f: f(ad, bd, 10.0, -10.0, ia, ibd),                                    # CPU ids
        lambda f: f(ad, bd, 10.0, -10.0),                                             # no ids, M != T
        lambda f: f(ad, bd, 10.0, -10.0, iad, None),                                  # one side's ids
        lambda f: f(ad, bd, 10.0, -10.0, iad, ibd.int()),                             # int64 against int32
        lambda f: f(ad, bd, 10.0, -10.0, iad[:16], ibd),                              # too few ids
        lambda f: f(ad, bd, float("inf"), -10.0, iad, ibd),
        lambda f: f(ad, bd, 10.0, float("nan"), iad, ibd),
        lambda f: f(ad[:, :96], bd[:, :96], 10.0, -10.0, iad, ibd),                   # D % 64
        lambda f: f(ad, bd[:, :64], 10.0, -10.0, iad, ibd),                           # D of a != D of b
        lambda f: f(ad.float(), bd, 10.0, -10.0, iad, ibd),                           # fp32 operands
        lambda f: f(torch.zeros(4, 2112, dtype=torch.float16, device="cuda"), torch.zeros(4, 2112, dtype=torch.float16, device="cuda"), 10.0, -10.0),   # D > 2048
    ]
    for f in (ops.cosine_sigmoid, ops.cosine_sigmoid_backward):
        for i, call in enumerate(bad):
            with pytest.raises(PclipError):
                call(f)
                pytest.fail(f"{f.__name__}: case {i} was accepted")
