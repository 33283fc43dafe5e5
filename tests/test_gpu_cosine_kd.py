"""pclip_cosine_kd_f16 / pclip_cosine_kd_backward_f16 (csrc/pclip_cosine_kd.hip), ops.cosine_kd(_backward), autograd.CosineKdFn and the losses built on them,
against the float64 helper tests/cosine_kd_ref.py under ITS derived tolerances, against identities (teacher == student, a one-hot teacher is the
cross-entropy) and against the kernels' own invariances bit for bit.

Shapes: a panel is 16 RF rows (RF <= 2 here) — M = 1, 15, 17, 33 are one row, a ragged panel, a second fragment, a second panel; the forward deals blocks of
64 columns to eight waves and the backward walks tiles of 64 rows of the other side — T = 1, 3, 37, 64, 65, 577 are below, on and one past a block, and 577
> 8 x 64 gives one forward wave two blocks and the class gradient several chunks.  (D, Dt): 64 / 64, 512 / 512, 512 / 768 (the teacher's own width: the
wider row loader, another k-step count) and 2048 / 2048 (both panels at the LDS limit)."""
import pytest
import torch

import cosine_ce_ref
import cosine_kd_ref as kr
from conftest import observe
from cosine_ce_ref import clustered, worst_ratio

pytestmark = pytest.mark.gpu

MS, TS = (1, 15, 17, 33), (1, 3, 37, 64, 65, 577)
SHAPES = [(M, T, 64, 64) for M in MS for T in TS]
SHAPES += [(M, T, D, Dt) for (D, Dt) in ((512, 512), (512, 768)) for M in (1, 17, 33) for T in (1, 65, 577)]
SHAPES += [(M, T, 2048, 2048) for M in (17, 33) for T in (65, 577)]
ALL_ON = (True, True, True, True)

_CASES, _REFS = {}, {}


def scales_of(M, T):
    return (100.0, 100.0) if (M + T) % 2 else (20.0, 50.0)


def case(M, T, D, Dt, far=False):
    """fp16 operands on the host, shared between the tests (never modified): `clustered` rows for the student, a teacher around centres of its own."""
    key = (M, T, D, Dt, far)
    if key not in _CASES:
        a, b = clustered(M, T, D, 7 + M)
        ta, tb = kr.teacher_like(M, T, Dt, 7 + M)
        if far:
            b, tb = kr.with_far_class(b, tb, 7 + M)
        _CASES[key] = (a, b, ta, tb)
    return _CASES[key]


def gpu_reference(a, b, scale, ta, tb, tscale, flags):
    """The float64 helper on the kernels' own normalised rows: where a side is normalised, the rows ops.l2norm_rows gives."""
    from proto_clip_amd import ops
    unit = lambda x, on: ops.l2norm_rows(x.cuda().contiguous()).cpu() if on else None
    na, nb, nta, ntb = flags
    return kr.reference(a, b, scale, ta, tb, tscale, na, nb, nta, ntb, a_unit16=unit(a, na), b_unit16=unit(b, nb), ta_unit16=unit(ta, nta), tb_unit16=unit(tb, ntb))


def ref_of(key, *args):
    if key not in _REFS:
        _REFS[key] = gpu_reference(*args)
    return _REFS[key]


def run(a, b, scale, ta, tb, tscale, flags=ALL_ON):
    from proto_clip_amd import ops
    loss, lse_row, tlse_row, rows = ops.cosine_kd(a, b, scale, ta, tb, tscale, *flags, want_rows=True)
    da, db, ds = ops.cosine_kd_backward(a, b, scale, ta, tb, tscale, lse_row, tlse_row, *flags)
    return dict(loss=loss, lse_row=lse_row, tlse_row=tlse_row, rows=rows, da=da, db=db, dscale=ds)


ITEMS = (("loss", "tol_loss"), ("rows", "tol_rows"), ("lse_row", "tol_lse"), ("tlse_row", "tol_tlse"), ("da", "tol_da"), ("db", "tol_db"), ("dscale", "tol_dscale"))


def check(tag, got, ref):
    """Every delivered item against the float64 helper; the figures are recorded before anything is asserted."""
    ratios = {}
    for name, tol in ITEMS:
        ratios[name] = observe(f"cosine kd {name}: |got - float64| / derived tolerance", worst_ratio(got[name], ref[name], ref[tol]), 1.0)
    print(tag, {k: round(v, 4) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (tag, name, r)


def guarded(x, pad):
    """The rows of x as a strided view of a wider buffer with NaN in the padding columns and in two guard rows."""
    buf = torch.full((x.shape[0] + 2, x.shape[1] + pad), float("nan"), dtype=torch.float16)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf.cuda()[:x.shape[0], :x.shape[1]]


def dev(*ts):
    return [t.cuda() for t in ts]


def same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("M,T,D,Dt", SHAPES)
def test_against_float64(M, T, D, Dt):
    a, b, ta, tb = case(M, T, D, Dt)
    scale, tscale = scales_of(M, T)
    ref = ref_of((M, T, D, Dt, False, scale, tscale, ALL_ON), a, b, scale, ta, tb, tscale, ALL_ON)
    check(f"kd {M}x{T}x{D}/{Dt} scales {scale}/{tscale}", run(*dev(a, b), scale, *dev(ta, tb), tscale), ref)


@pytest.mark.parametrize("flags", [tuple(bool(i >> k & 1) for k in range(4)) for i in range(16)])
def test_every_combination_of_the_normalise_flags(flags):
    M, T, D, Dt = 17, 37, 64, 128
    a, b, ta, tb = case(M, T, D, Dt)
    for scale, tscale in ((100.0, 100.0), (20.0, 50.0)):
        ref = ref_of((M, T, D, Dt, False, scale, tscale, flags), a, b, scale, ta, tb, tscale, flags)
        check(f"kd flags {flags} scales {scale}/{tscale}", run(*dev(a, b), scale, *dev(ta, tb), tscale, flags), ref)


@pytest.mark.parametrize("scale,tscale", [(20.0, 50.0), (50.0, 20.0)])
def test_a_class_no_sample_is_near(scale, tscale):
    """Entries of the E tile near 2^-26: what the 2^14 scaling keeps (the wrong walks of tests/test_cosine_kd_cpu.py fail here)."""
    M, T, D, Dt = 33, 64, 512, 512
    a, b, ta, tb = case(M, T, D, Dt, far=True)
    ref = ref_of((M, T, D, Dt, True, scale, tscale, ALL_ON), a, b, scale, ta, tb, tscale, ALL_ON)
    check(f"kd far class scales {scale}/{tscale}", run(*dev(a, b), scale, *dev(ta, tb), tscale), ref)


# ---- identities ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,T,D", [(17, 37, 64), (33, 577, 512)])
def test_teacher_equal_to_student_gives_zero_within_tolerance(M, T, D):
    a, b, _, _ = case(M, T, D, D)
    ref = ref_of(("same", M, T, D), a, b, 100.0, a, b, 100.0, ALL_ON)
    ad, bd = dev(a, b)
    got = run(ad, bd, 100.0, ad, bd, 100.0)
    zero = lambda k: torch.zeros_like(ref[k])
    r = {"loss": worst_ratio(got["loss"], zero("loss"), ref["tol_loss"]), "rows": worst_ratio(got["rows"], zero("rows"), ref["tol_rows"])}
    for k in ("da", "db", "dscale"):
        r[k] = worst_ratio(got[k], zero(k), ref["tol_" + k])
    print("teacher == student", {k: round(v, 4) for k, v in r.items()}, "loss", float(got["loss"]))
    for k, v in r.items():
        assert observe(f"cosine kd teacher == student {k}: |got| / derived tolerance", v, 1.0) <= 1.0, (k, v)


@pytest.mark.parametrize("M,T,D,Dt", [(17, 37, 64, 64), (33, 65, 512, 768)])
def test_one_hot_teacher_gives_the_cross_entropy(M, T, D, Dt):
    from proto_clip_amd import ops
    a, b, ta, tb, labels = kr.planted(M, T, D, Dt, 5)
    ad, bd, tad, tbd = dev(a, b, ta, tb)
    kd_ref = ref_of(("planted", M, T, D, Dt), a, b, 100.0, ta, tb, kr.PLANTED_TSCALE, ALL_ON)
    unit = lambda x: ops.l2norm_rows(x.contiguous()).cpu()
    ce_ref = cosine_ce_ref.reference(a, b, 100.0, labels, False, True, True, a_unit16=unit(ad), b_unit16=unit(bd))
    got = run(ad, bd, 100.0, tad, tbd, kr.PLANTED_TSCALE)
    loss, lse_row, _ = ops.cosine_cross_entropy(ad, bd, 100.0, labels.cuda(), False, True, True)
    da, db, ds = ops.cosine_cross_entropy_backward(ad, bd, 100.0, lse_row, None, labels.cuda(), False, True, True)
    ce = dict(loss=loss, da=da, db=db, dscale=ds)
    for k in ("loss", "da", "db", "dscale"):
        r = worst_ratio(got[k], ce[k].double().cpu(), kd_ref["tol_" + k] + ce_ref["tol_" + k])
        assert observe(f"cosine kd one-hot teacher {k}: |kd - ce| / sum of the two tolerances", r, 1.0) <= 1.0, (k, r)


@pytest.mark.parametrize("M,T,D,Dt", [(17, 37, 64, 64), (33, 577, 512, 768), (15, 65, 2048, 2048)])
def test_lse_vectors_have_the_bits_of_the_cross_entropy_forward(M, T, D, Dt):
    from proto_clip_amd import ops
    a, b, ta, tb = dev(*case(M, T, D, Dt))
    labels = torch.zeros(M, dtype=torch.int64, device="cuda")
    for flags in (ALL_ON, (False, True, True, False)):
        _, lse_row, tlse_row = ops.cosine_kd(a, b, 20.0, ta, tb, 50.0, *flags)
        assert same_bits(lse_row, ops.cosine_cross_entropy(a, b, 20.0, labels, False, flags[0], flags[1])[1])
        assert same_bits(tlse_row, ops.cosine_cross_entropy(ta, tb, 50.0, labels, False, flags[2], flags[3])[1])


# ---- invariances, bit for bit --------------------------------------------------------------------------------------------------------------------------

def all_same_bits(x, y, keys=("loss", "lse_row", "tlse_row", "rows", "da", "db", "dscale")):
    return [k for k in keys if not same_bits(x[k], y[k])]


@pytest.mark.parametrize("T,D,Dt", [(37, 64, 64), (577, 512, 768)])
def test_a_row_alone_and_rows_permuted(T, D, Dt):
    M = 33
    a, b, ta, tb = dev(*case(M, T, D, Dt))
    full = run(a, b, 100.0, ta, tb, 100.0)
    from proto_clip_amd import ops
    for m in (0, 16, 32):
        one = ops.cosine_kd(a[m:m + 1], b, 100.0, ta[m:m + 1], tb, 100.0, *ALL_ON, want_rows=True)
        assert same_bits(one[1], full["lse_row"][m:m + 1]) and same_bits(one[2], full["tlse_row"][m:m + 1]) and same_bits(one[3], full["rows"][m:m + 1])
        da = ops.cosine_kd_backward(a[m:m + 1], b, 100.0, ta[m:m + 1], tb, 100.0, one[1], one[2], *ALL_ON, want_b=False, want_scale=False, mean_over=M)[0]
        assert same_bits(da, full["da"][m:m + 1]), m
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).cuda()
    shuffled = run(a[perm].contiguous(), b, 100.0, ta[perm].contiguous(), tb, 100.0)
    for k in ("lse_row", "tlse_row", "rows", "da"):
        assert same_bits(shuffled[k], full[k][perm]), k


def test_strided_views_with_nan_guard_bands_two_calls_and_an_aliased_teacher():
    M, T, D, Dt = 33, 65, 512, 768
    a, b, ta, tb = case(M, T, D, Dt)
    dense = run(*dev(a, b), 20.0, *dev(ta, tb), 50.0)
    strided = run(guarded(a, 8), guarded(b, 16), 20.0, guarded(ta, 24), guarded(tb, 8), 50.0)
    assert all_same_bits(strided, dense) == []
    assert all_same_bits(run(*dev(a, b), 20.0, *dev(ta, tb), 50.0), dense) == []
    ad, bd = dev(a, b)
    aliased = run(ad, bd, 100.0, ad, bd, 50.0)                         # ta is a, tb is b: one buffer read as both
    copied = run(ad, bd, 100.0, ad.clone(), bd.clone(), 50.0)
    assert all_same_bits(aliased, copied) == []


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------------------

def test_autograd_gradients_are_the_backward_ops_times_the_upstream_value():
    from proto_clip_amd import autograd as pag, ops
    M, T, D, Dt = 17, 37, 64, 128
    a, b, ta, tb = dev(*case(M, T, D, Dt))
    a32, b32 = a.float().requires_grad_(True), b.float().requires_grad_(True)
    scale = torch.tensor(20.0, device="cuda", requires_grad=True)
    loss = pag.cosine_kd(a32, b32, scale, ta, tb, 50.0, normalize_a=True, normalize_b=True, normalize_teacher_a=True, normalize_teacher_b=True)
    kept = [t for t in loss.grad_fn.saved_tensors if t is not None]                      # the four operands and the two lse vectors: nothing of size M T
    assert sorted(tuple(t.shape) for t in kept) == sorted([(M, D), (T, D), (M, Dt), (T, Dt), (M,), (M,)])
    (3.0 * loss).backward()
    fwd = ops.cosine_kd(a, b, 20.0, ta, tb, 50.0, *ALL_ON)
    assert same_bits(loss.detach(), fwd[0])
    da, db, ds = ops.cosine_kd_backward(a, b, 20.0, ta, tb, 50.0, fwd[1], fwd[2], *ALL_ON)
    three = torch.tensor(3.0, device="cuda")
    assert same_bits(a32.grad, da * three) and same_bits(b32.grad, db * three) and same_bits(scale.grad, ds * three)


def test_temperature_is_the_explicit_rescaling():
    from proto_clip_amd import autograd as pag
    M, T, D, Dt = 17, 37, 64, 128
    a, b, ta, tb = dev(*case(M, T, D, Dt))
    kw = dict(normalize_a=True, normalize_b=True, normalize_teacher_a=True, normalize_teacher_b=True)
    b1, b2 = b.float().requires_grad_(True), b.float().requires_grad_(True)
    pag.cosine_kd(a, b1, 100.0, ta, tb, 50.0, temperature=2.0, **kw).backward()
    (4.0 * pag.cosine_kd(a, b2, 50.0, ta, tb, 25.0, **kw)).backward()
    assert same_bits(b1.grad, b2.grad)
    with torch.no_grad():
        l1, l2 = pag.cosine_kd(a, b, 100.0, ta, tb, 50.0, temperature=2.0, **kw), 4.0 * pag.cosine_kd(a, b, 50.0, ta, tb, 25.0, **kw)
    assert same_bits(l1, l2)


def test_no_tape_under_no_grad_and_the_public_losses():
    from proto_clip_amd import autograd as pag, ops, utils
    M, T, D = 17, 37, 64
    a, b, _, tb = dev(*case(M, T, D, D))
    w = b.float().requires_grad_(True)
    with torch.no_grad():
        loss = pag.cosine_kd(a, w, 100.0, a, tb, 100.0)
    assert loss.grad_fn is None and not loss.requires_grad
    an, bn, tbn = ops.l2norm_rows(a), ops.l2norm_rows(b), ops.l2norm_rows(tb)
    got = utils.clip_logits_distill_loss(an, bn, tbn, layout="nd")
    assert same_bits(got, ops.cosine_kd(an, bn, 100.0, an, tbn, 100.0)[0])
    got_dn = utils.clip_logits_distill_loss(an, ops.transpose(bn), ops.transpose(tbn), scale=20.0, teacher_scale=50.0, temperature=2.0, layout="dn")
    assert same_bits(got_dn, 4.0 * ops.cosine_kd(an, bn, 10.0, an, tbn, 25.0)[0])
