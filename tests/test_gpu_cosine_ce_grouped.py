"""The grouped cosine cross-entropy (pclip_cosine_ce_grouped_f16 / _backward_f16, ops.cosine_cross_entropy_grouped(_backward), autograd.GroupedCosineCeFn,
utils.clip_logits_loss_grouped, cocoop.CoCoOp.loss): G independent labelled problems in one call.  The defining requirement is that a group's numbers are the
BITS of the plain call on that group alone, so most of this file compares bit patterns; the float64 helper tests/cosine_ce_ref.py grades two shapes under
its derived tolerances on top.

Shapes (G, M, T, D): one row per group is CoCoOp's case (M = 1: one workgroup per group in the forward); G = 16 / 17 straddle a slice of sixteen, T = 65 and
130 are one past a 64-column block, T = 1000 at D = 1024 and T = 3 at D = 2048 run the two wider register panels, M = 17 two row fragments."""
import pytest
import torch

from conftest import observe
from cosine_ce_ref import cluster_labels, clustered, reference, worst_ratio
from spec import SMALL

pytestmark = pytest.mark.gpu

# (3, 130, 5, 64): the class gradient (direction 1) walks Ro = 5 own rows — one panel — over Rw = 130 rows, three tiles of 64; ce_chunks(5, 130, 64, true) is
# min(ceil(512 / 1 panel), cap 4 (5 + 130) / 5 = 108, 3 tiles) = 3 > 1: the branch `nchunks > 1` of the backward entry, partial panels [G][3][5 x 64] in the
# workspace summed by the grouped instantiation of ce_sum_chunks_kernel.  Every other shape here walks in one chunk.
SHAPES = [(1, 1, 1, 64), (3, 1, 37, 512), (16, 1, 65, 64), (17, 1, 5, 128), (2, 17, 130, 64), (2, 1, 1000, 1024), (2, 1, 3, 2048), (3, 130, 5, 64)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
NAMES = ("loss", "lse_row", "rows", "da", "db", "dscale")

_CASES = {}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def case(G, M, T, D, odd_labels=True):
    """fp16 operands [G, M, D], [G, T, D] and labels [G, M] on the host, every group from its own seeds; shared between the tests (never modified).
    odd_labels: the last group's first label is T (one past the classes) and the first label of the first group — of the last group's last row where M > 1 —
    is -1: neither is ever an index."""
    key = (G, M, T, D, odd_labels)
    if key not in _CASES:
        pairs = [clustered(M, T, D, 1000 * G + 17 * g + M) for g in range(G)]
        a, b = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
        labels = torch.stack([cluster_labels(M, T, 500 * G + g + T) for g in range(G)])
        if odd_labels:
            labels[G - 1, 0] = T
            labels[G - 1 if M > 1 else 0, M - 1] = -1
        _CASES[key] = (a, b, labels)
    return _CASES[key]


def run_grouped(a, b, scale, labels, na, nb, **kw):
    from proto_clip_amd import ops
    loss, lse_row, rows = ops.cosine_cross_entropy_grouped(a, b, scale, labels, na, nb)
    da, db, ds = ops.cosine_cross_entropy_grouped_backward(a, b, scale, lse_row, labels, na, nb, **kw)
    return dict(loss=loss, lse_row=lse_row, rows=rows, da=da, db=db, dscale=ds)


def run_single(a, b, scale, labels, na, nb, **kw):
    from proto_clip_amd import ops
    loss, lse_row, _, rows = ops.cosine_cross_entropy(a, b, scale, labels, False, na, nb, want_rows=True)
    da, db, ds = ops.cosine_cross_entropy_backward(a, b, scale, lse_row, None, labels, False, na, nb, **kw)
    return dict(loss=loss, lse_row=lse_row, rows=rows, da=da, db=db, dscale=ds)


def assert_groups_are_the_single_calls(tag, got, a, b, scale, labels, na, nb, **kw):
    for g in range(a.shape[0]):
        want = run_single(a[g], b[g], scale, labels[g], na, nb, **kw)
        for name in NAMES:
            assert torch.equal(bits(got[name][g]), bits(want[name])), (tag, g, name)


@pytest.mark.parametrize("G,M,T,D", SHAPES)
def test_every_group_has_the_bits_of_the_single_call(G, M, T, D):
    a, b, labels = case(G, M, T, D)
    ad, bd = a.cuda(), b.cuda()
    for na, nb in FLAGS:
        lab = labels.cuda() if na == nb else labels.int().cuda()                     # int64 and int32 labels
        kw = dict(mean_over=3 * M) if na else {}                                     # the default mean and a slice of a larger batch
        for scale in ((100.0, 14.2857) if na and nb else (100.0,)):
            got = run_grouped(ad, bd, scale, lab, na, nb, **kw)
            assert got["loss"].shape == (G,) and got["lse_row"].shape == (G, M) and got["da"].shape == (G, M, D) and got["db"].shape == (G, T, D)
            assert got["dscale"].shape == (G,)
            assert_groups_are_the_single_calls((G, M, T, D, na, nb, scale), got, ad, bd, scale, lab, na, nb, **kw)
    if M == 1:                                                                       # a [G, D]: one row per group, labels [G]
        from proto_clip_amd import ops
        flat = ops.cosine_cross_entropy_grouped(ad[:, 0], bd, 100.0, lab[:, 0], True, True)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(flat, ops.cosine_cross_entropy_grouped(ad, bd, 100.0, lab, True, True)))


def in_a_larger_buffer(x, rows, cols):
    """x [G, R, D] as a view into a NaN-filled [G, R + rows, D + cols] buffer: group stride > rows x pitch, pitch > D."""
    G, R, D = x.shape
    buf = torch.full((G, R + rows, D + cols), float("nan"), dtype=torch.float16)
    buf[:, :R, :D] = x
    buf = buf.cuda()
    return buf, buf[:, :R, :D]


@pytest.mark.parametrize("G,M,T,D", [(3, 1, 37, 512), (2, 17, 130, 64), (3, 130, 5, 64)])
def test_views_are_read_in_place_and_nothing_is_written_outside_the_outputs(G, M, T, D):
    """The operands are slices of larger buffers whose gaps hold NaN; the entries are called with output buffers of this test's own, each followed by a guard
    band.  The outputs equal those of dense operands, the buffers keep their bits (gaps included), the bands stay intact."""
    from proto_clip_amd import _lib, ops
    a, b, labels = case(G, M, T, D)
    abuf, av = in_a_larger_buffer(a, 2, 8)
    bbuf, bv = in_a_larger_buffer(b, 3, 16)
    assert av.stride(0) > M * av.stride(1) and av.stride(1) > D and bv.stride(0) > T * bv.stride(1) and bv.stride(1) > D
    before = bits(abuf).clone(), bits(bbuf).clone()
    lab = labels.cuda()
    dense = run_grouped(a.cuda(), b.cuda(), 100.0, lab, True, True)
    viewed = run_grouped(av, bv, 100.0, lab, True, True)
    for name in NAMES:
        assert torch.equal(bits(viewed[name]), bits(dense[name])), name
    # the C entries on guarded outputs
    lib, GUARD, MARK = _lib.load(), 64, -12345.0
    def guarded(n):
        return torch.full((n + GUARD,), MARK, dtype=torch.float32, device="cuda")
    lse, rows, loss = guarded(G * M), guarded(G * M), guarded(G)
    nws = int(lib.pclip_cosine_ce_grouped_workspace(1, G, M, T, D))
    assert nws >= int(lib.pclip_cosine_ce_grouped_workspace(0, G, M, T, D))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    p, flags = _lib.ptr, _lib.CE_NORMALIZE_A | _lib.CE_NORMALIZE_B | _lib.CE_LABELS_I64
    common = (p(av), av.stride(1) if M > 1 else D, av.stride(0), M, p(bv), bv.stride(1), bv.stride(0), T, D, G, 100.0, flags, p(lab))
    _lib.check(lib.pclip_cosine_ce_grouped_f16(*common, p(lse), p(rows), p(loss), p(ws), nws, _lib.stream()), "forward")
    outs = [("lse_row", lse, G * M), ("rows", rows, G * M), ("loss", loss, G)]
    for direction, R in ((0, M), (1, T)):
        grad, ds = guarded(G * R * D), guarded(G) if direction == 0 else None        # (ops takes dscale from the dL/da walk; NULL: not asked for)
        _lib.check(lib.pclip_cosine_ce_grouped_backward_f16(*common, p(lse), 1.0 / M, direction, p(grad), p(ds), p(ws), nws, _lib.stream()), "backward")
        outs += [("db" if direction else "da", grad, G * R * D)] + ([("dscale", ds, G)] if direction == 0 else [])
    torch.cuda.synchronize()
    for name, buf, n in outs:
        assert torch.equal(bits(buf[:n]), bits(dense[name].reshape(-1))), name
        assert bool((buf[n:] == MARK).all()), name
    assert torch.equal(bits(abuf), before[0]) and torch.equal(bits(bbuf), before[1])


def test_groups_are_independent_and_the_call_is_deterministic():
    G, M, T, D = 5, 17, 37, 128
    a, b, labels = case(G, M, T, D)
    ad, bd, lab = a.cuda(), b.cuda(), labels.cuda()
    clean = run_grouped(ad, bd, 100.0, lab, True, True)
    again = run_grouped(ad, bd, 100.0, lab, True, True)
    for name in NAMES:
        assert torch.equal(bits(clean[name]), bits(again[name])), name
    # a NaN in one group's a reaches that group's outputs and no other's
    bad = ad.clone()
    bad[2, 3, 5] = float("nan")
    got = run_grouped(bad, bd, 100.0, lab, True, True)
    others = [0, 1, 3, 4]
    for name in NAMES:
        assert torch.equal(bits(got[name][others]), bits(clean[name][others])), name
    # (the row's maximum skips a NaN logit, so its lse is -inf, not NaN; the target logit, the loss term and the exp tile carry the NaN on)
    assert bool(torch.isnan(got["loss"][2])) and bool(torch.isnan(got["rows"][2, 3])) and not bool(torch.isfinite(got["lse_row"][2, 3]))
    assert not bool(torch.isfinite(got["dscale"][2])) and not bool(torch.isfinite(got["da"][2, 3]).any()) and not bool(torch.isfinite(got["db"][2]).any())
    alone = run_single(bad[2], bd[2], 100.0, lab[2], True, True)
    for name in NAMES:
        assert torch.equal(bits(got[name][2]), bits(alone[name])), name
    # permuting the groups permutes every output
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    moved = run_grouped(ad[perm].contiguous(), bd[perm].contiguous(), 100.0, lab[perm].contiguous(), True, True)
    for name in NAMES:
        assert torch.equal(bits(moved[name]), bits(clean[name][perm])), name


@pytest.mark.parametrize("scale", [100.0, 14.29])
@pytest.mark.parametrize("G,M,T,D", [(3, 1, 37, 512), (2, 17, 130, 64)])
def test_against_float64(G, M, T, D, scale):
    """Every group against the float64 helper under its derived tolerances, both sides normalised (CoCoOp's mode) at both scales, the rows as given at 14.29.
    Not graded: the rows as given at scale 100.  The helper's gradient tolerance models the rounding of the exp tile as a RELATIVE 2^-11, which the
    kernel's fp16 tile (2^14 E) delivers down to E = 2^-28 and no further (csrc/pclip_cosine_ce.hip, CE_ESCALE).  With the unnormalised clustered rows of
    (2, 17, 130, 64) at scale 100 one class of group 0 and two of group 1 are 2^-30 .. 2^-31 for EVERY sample — float64, no kernel involved — so their rows
    of dL/db consist of fp16 subnormals alone, and the plain kernel and the grouped one alike miss the helper's bound there (1.46 of it, measured on dL/db;
    normalised, the smallest such class is 2^-9).  That case stays compared bit for bit with the plain call above; what is graded asserts
    the premise on the float64 side."""
    from proto_clip_amd import ops
    a, b, labels = case(G, M, T, D, odd_labels=False)
    ad, bd, lab = a.cuda(), b.cuda(), labels.cuda()
    for na, nb in ((True, True),) + (((False, False),) if scale < 100.0 else ()):
        got = run_grouped(ad, bd, scale, lab, na, nb)
        for g in range(G):
            unit = lambda x, on: ops.l2norm_rows(x.contiguous()).cpu() if on else None
            ref = reference(a[g], b[g], scale, labels[g], False, na, nb, a_unit16=unit(ad[g], na), b_unit16=unit(bd[g], nb))
            assert float(torch.softmax(ref["s"], 1).max(0).values.min()) >= 2.0 ** -28          # every row of dL/db has an entry the fp16 tile holds at 2^-11
            ratios = {}
            for name, tol in (("loss", "tol_loss"), ("lse_row", "tol_loss"), ("rows", "tol_loss"), ("da", "tol_da"), ("db", "tol_db"), ("dscale", "tol_dscale")):
                ratios[name] = observe(f"grouped cosine ce {name}: |got - float64| / derived tolerance", worst_ratio(got[name][g], ref[name], ref[tol]), 1.0)
            print((G, M, T, D, scale, na, nb, g), {k: round(v, 4) for k, v in ratios.items()})
            for name, r in ratios.items():
                assert r <= 1.0, ((G, M, T, D, scale, na, nb, g), name, r)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_autograd_is_the_stack_and_mean_of_the_single_functions(dtype):
    """The reference side gives every group leaves of its own, so that each gradient comes straight out of CosineCeFn (torch's accumulation of B zero-padded
    slices into one tensor would turn a -0 of the fp16 cast into +0)."""
    from proto_clip_amd import autograd as pag, utils
    G, M, T, D = 3, 2, 37, 128
    a, b, labels = case(G, M, T, D)
    lab = labels.cuda()
    mk = lambda x: x.to(dtype).cuda().requires_grad_(True)
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        ag, bg, sg = mk(a).requires_grad_(need_a), mk(b).requires_grad_(need_b), torch.tensor(14.29, device="cuda", requires_grad=True)
        loss = pag.cosine_cross_entropy_grouped(ag, bg, sg, lab, normalize_a=True, normalize_b=True)
        assert loss.shape == (G,) and loss.dtype == torch.float32
        (loss.mean() * 8.0).backward()
        singles_a = [mk(a[g]).requires_grad_(need_a) for g in range(G)]
        singles_b = [mk(b[g]).requires_grad_(need_b) for g in range(G)]
        ss = torch.tensor(14.29, device="cuda", requires_grad=True)
        terms = [pag.cosine_cross_entropy(singles_a[g], singles_b[g], ss, labels=lab[g], normalize_a=True, normalize_b=True) for g in range(G)]
        want = torch.stack([t.reshape(()) for t in terms])
        (want.mean() * 8.0).backward()
        assert torch.equal(bits(loss), bits(want))
        if need_a:
            assert ag.grad.dtype == dtype and torch.equal(bits(ag.grad), bits(torch.stack([x.grad for x in singles_a])))
        else:
            assert ag.grad is None
        if need_b:
            assert bg.grad.dtype == dtype and torch.equal(bits(bg.grad), bits(torch.stack([x.grad for x in singles_b])))
        else:
            assert bg.grad is None
        # the scale: g[q] * dscale[q] rounded to fp32, added in ascending q in fp32
        from proto_clip_amd import ops
        a16, b16 = ag.detach().half(), bg.detach().half()
        _, lse_row, _ = ops.cosine_cross_entropy_grouped(a16, b16, 14.29, lab, True, True)
        ds = ops.cosine_cross_entropy_grouped_backward(a16, b16, 14.29, lse_row, lab, True, True, want_a=need_a, want_b=need_b)[2].cpu()
        up = torch.full((G,), 8.0) / G                                               # d (8 mean) / d loss[q], as torch's mean delivers it
        acc = (ds[0] * up[0]).clone()
        for q in range(1, G):
            acc = acc + ds[q] * up[q]
        assert sg.grad.dtype == torch.float32 and sg.grad.dim() == 0 and torch.equal(bits(sg.grad), bits(acc))
    with torch.no_grad():
        quiet = utils.clip_logits_loss_grouped(mk(a), mk(b), lab, scale=14.29, normalize_features=True, normalize_weights=True)
    assert quiet.grad_fn is None and torch.equal(bits(quiet), bits(loss.detach().mean()))


@pytest.fixture(scope="module")
def cocoop_model():
    from test_gpu_cocoop import make_model
    return make_model(SMALL, 31)


def test_cocoop_keeps_its_bits_and_loses_its_loop(cocoop_model, monkeypatch):
    """CoCoOp.loss is one grouped call: the loss and the five parameter gradients have the bits of the per-image loop it replaces (restated here), no plain
    cosine cross-entropy call is left in it, and the number of grouped-entry calls does not depend on the batch."""
    import cocoop_ref
    from proto_clip_amd import autograd as pag, cocoop, ops
    from test_gpu_cocoop import PARAMS, make_learner

    def loop_loss(head, features, labels):
        text, scale = head.learner(features), head.logit_scale()
        labels = labels.to(features.device).long()
        terms = [pag.cosine_cross_entropy(features[b:b + 1].contiguous(), text[b], scale, labels=labels[b:b + 1], normalize_a=True, normalize_b=True)
                 for b in range(features.shape[0])]
        return torch.stack([t.reshape(()) for t in terms]).mean()

    calls = {}
    for B in (3, 19):
        *params, tokens, feats, labels = cocoop_ref.fixture_inputs(SMALL, B, 5, 4, 3)
        feats, labels = feats.cuda(), labels.cuda()
        out = {}
        for how in ("loop", "grouped"):
            learner = make_learner(cocoop_model, params, tokens)
            head = cocoop.CoCoOp(cocoop_model, learner)
            with monkeypatch.context() as m:
                counted = []
                if how == "grouped":
                    def refuse(*args, **kw):
                        raise AssertionError("CoCoOp.loss called the plain cosine cross-entropy")
                    m.setattr(ops, "cosine_cross_entropy", refuse)
                    for name in ("cosine_cross_entropy_grouped", "cosine_cross_entropy_grouped_backward"):
                        def counting(*args, _f=getattr(ops, name), _n=name, **kw):
                            counted.append(_n)
                            return _f(*args, **kw)
                        m.setattr(ops, name, counting)
                loss = head.loss(feats, labels) if how == "grouped" else loop_loss(head, feats, labels)
                (loss * 1024).backward()
                torch.cuda.synchronize()
            out[how] = (loss.detach(), [getattr(learner, n).grad.clone() for n in PARAMS])
            if how == "grouped":
                calls[B] = sorted(counted)
        assert torch.equal(bits(out["grouped"][0]), bits(out["loop"][0])), B
        for name, got, want in zip(PARAMS, out["grouped"][1], out["loop"][1]):
            assert bool(got.any()) and torch.equal(bits(got), bits(want)), (B, name)
    assert calls[3] == calls[19] == ["cosine_cross_entropy_grouped", "cosine_cross_entropy_grouped_backward"], calls


def test_forward_and_backward_capture_in_one_graph():
    G, M, T, D = 3, 17, 130, 64
    a, b, labels = case(G, M, T, D)
    ad, bd, lab = a.cuda(), b.cuda(), labels.cuda()
    eager = run_grouped(ad, bd, 100.0, lab, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_grouped(ad, bd, 100.0, lab, True, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = run_grouped(ad, bd, 100.0, lab, True, True)
    for _ in range(2):
        for o in out.values():
            o.zero_()
        gr.replay()
        torch.cuda.synchronize()
        for name, o in out.items():
            assert torch.equal(bits(o), bits(eager[name])), name
