"""The fp32 kernels of the training step graded per element against float64 (tests/train_f32_ref.py: the references, the derived tolerances, the case lists, the restated
routes): pclip_gemm_f32 on the single-pass and the split-K route with all four operand dtypes and transposes, pclip_colsum_f32 single- and two-pass, addscaled_rows,
nll_grad, fuse_probs_backward, nll_rows, nll_mean_backward, softmax_ce_rows, the fp32 l2norm and its backward, and — bit for bit — the two casts, the argmax (the lowest
index among equal maxima) and the exact zeros.

Every case: worst |got - float64| / tolerance <= 1 (printed as a LEDGER line: profiles/train_f32_ledger.txt is made from those), the output inside a buffer with a guard row
on either side and guard columns behind a leading dimension that must keep their fill, NaN in the padding of strided inputs, NaN in an output the kernel must not read
(beta = 0, accumulate = 0), and a second call with the same bits.  A route is asserted twice: from the entry's own condition restated in train_f32_ref (a case named split-K
or two-pass cannot silently take the other) and from the workspace, which the split routes write and the single pass must leave untouched.

softmax_ce_rows has no case in the row loop's second iteration: it requires C >= R, and 32 773 columns of 32 773 rows are 4.3 GB per tensor.  That gap stays open
(DESIGN.md says so): the `r += gridDim.x * 4` stride of that one kernel is not exercised."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_f32_ref as ref                                         # noqa: E402
from conftest import observe                                        # noqa: E402
from test_gpu_row_passes import FILL, guarded, guards_intact, padded          # noqa: E402
from train_f32_ref import worst_ratio                               # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
FLAT_BIG = (4099, 1024)                                             # > 16 384 x 256 elements: the grid-stride loop of the flat kernels iterates


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def L():
    from proto_clip_amd import _lib
    return _lib


def record(kernel, route, shape, fam, ratio):
    print(f"LEDGER {kernel} | {route} | {shape} | {fam} | {ratio:.3f}")
    observe(f"train f32 {kernel}, {route}: |got - float64| / derived tolerance", ratio, 1.0)
    assert ratio <= 1.0, (kernel, route, shape, fam, ratio)


def window(R, C, pad=5, dtype=torch.float32, fill=None):
    """(buffer, view [R, C] with row stride C + pad) inside guard rows and guard columns holding FILL; the view starts as `fill` (a tensor or a value; default NaN)."""
    buf, mid = guarded(R, C + pad, dtype)
    view = mid[:, :C]
    if torch.is_tensor(fill):
        view.copy_(fill)
    else:
        view.fill_(NAN if fill is None else fill)
    return buf, view


def vector(n, dtype=torch.float32, fill=None):
    buf, view = window(1, n, 0, dtype, fill if fill is not None else (NAN if dtype.is_floating_point else -1))
    return buf, view[0]


def intact(buf, C):
    """The guard rows and the guard columns (behind column C of the middle rows) of a `window` still hold FILL."""
    return guards_intact(buf) and bool((buf[1:-1, C:] == FILL).all())


def flat(n, dtype, guard=64):
    """(buffer, view [n]) with `guard` elements of FILL on either side; the view starts 128-byte aligned (the casts move 16 bytes per lane)."""
    buf = torch.full((n + 2 * guard,), FILL, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n]


def flat_intact(buf, guard=64):
    torch.cuda.synchronize()
    return bool((buf[:guard] == FILL).all()) and bool((buf[-guard:] == FILL).all())


def scratch(floats, tail=64):
    """A workspace of `floats` fp32 followed by `tail` guard elements, all FILL."""
    return torch.full((max(floats, 1) + tail,), FILL, dtype=torch.float32, device="cuda")


def dev(t, pad):
    return padded(t, pad) if pad else t.cuda()


def twice(run):
    """Run a case twice from the same inputs: the second call must give the same bits, guards included."""
    first = run()
    second = run()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "a second call gave other bits"
    return first


# ---- gemm_f32 ---------------------------------------------------------------------------------------------------------------------------------------------------------
def run_gemm(L, case, ws_bytes, ws_floats):
    """One raw call; returns (whole output buffer, workspace) and asserts the guards."""
    lib = L.load()
    a, b, c0 = ref.gemm_inputs(case)
    ad, bd = dev(a, case.pad), dev(b, case.pad + 1 if case.pad else 0)
    M, N, K = case.M, case.N, case.K
    ldc = N + 5
    buf, out = window(M, N, 5, fill=c0 if case.beta != 0 else None)
    ws = scratch(ws_floats)
    rsa, csa = (1, ad.stride(0)) if case.ta else (ad.stride(0), 1)
    rsb, csb = (1, bd.stride(0)) if case.tb else (bd.stride(0), 1)
    L.check(lib.pclip_gemm_f32(L.ptr(ad), int(case.a16), rsa, csa, L.ptr(bd), int(case.b16), rsb, csb, L.ptr(out), ldc, M, N, K, case.alpha, case.beta,
                               L.ptr(ws) if ws_bytes else None, ws_bytes, L.stream()), "pclip_gemm_f32")
    assert intact(buf, N), ("a guard of C was written", case)
    assert bool((ws[max(ws_floats, 1):] == FILL).all()), "the workspace was written past its end"
    return buf, ws


def gemm_case(L, case, route, label):
    M, N, K = case.M, case.N, case.K
    full = ref.gemm_route(M, N, K, 1 << 40)                         # the route with all the workspace one could want
    if route == "split":
        S, kper = full
        ws_floats = S * M * N
        ws_bytes = 4 * ws_floats                                    # exactly what the entry asks for
    elif route == "short":
        ws_floats = full[0] * M * N
        ws_bytes = 4 * ws_floats - 4
        S, kper = 1, K
    elif route == "ample":                                          # room for the most slabs the entry ever asks for: if it stays untouched, the CONDITION said no
        ws_floats = 32 * M * N
        ws_bytes = 4 * ws_floats
        S, kper = full
    else:
        ws_floats, ws_bytes, S, kper = 0, 0, 1, K
    assert ref.gemm_route(M, N, K, ws_bytes) == (S, kper)            # the entry's own condition
    buf, ws = twice(lambda: run_gemm(L, case, ws_bytes, ws_floats))
    written = ws[:max(ws_floats, 1)] != FILL
    used = S * M * N if S > 1 else 0
    assert bool(written[:used].all()), "the split-K route left slabs unwritten"
    assert not bool(written[used:].any()), "the single pass touched the workspace" if S == 1 else "slabs beyond S were written"
    want, tol = ref.gemm_reference(case, S)
    got = buf[1:-1, :N]
    dt = ("f16" if case.a16 else "f32") + "x" + ("f16" if case.b16 else "f32")
    record("gemm_f32", f"{label} S={S} {'T' if case.ta else 'N'}{'T' if case.tb else 'N'} {dt} alpha={case.alpha} beta={case.beta}" + (" padded" if case.pad else ""),
           f"{M}x{N}x{K}", case.family, worst_ratio(got, want, tol))


@pytest.mark.parametrize("group", ["small", "transposes", "dtypes", "scalars", "padded"])
def test_gemm_single_pass(L, group):
    cases = {"small": ref.GEMM_SMALL, "transposes": ref.GEMM_TRANS, "dtypes": ref.GEMM_DTYPES, "scalars": ref.GEMM_SCALARS, "padded": ref.GEMM_PADDED}[group]
    for case in cases:
        gemm_case(L, case, "none", "single")


@pytest.mark.parametrize("case", ref.GEMM_SPLIT, ids=lambda c: f"{c.M}x{c.N}x{c.K}")
def test_gemm_split_k(L, case):
    S = ref.GEMM_EXPECT_S[(case.M, case.N, case.K)]
    assert ref.gemm_route(case.M, case.N, case.K, 1 << 40)[0] == S
    if S > 1:
        gemm_case(L, case, "split", "split")                        # the workspace exactly as large as the entry asks for
    gemm_case(L, case, "ample", "ample workspace" if S > 1 else "no split")          # 32 M N floats offered: S == 1 only if the condition itself refuses the split
    gemm_case(L, case, "none", "unsplit")                           # the same inputs without a workspace: both grade, they need not be equal
    if (case.M, case.N, case.K) in ((1, 64, 1025), (130, 70, 3000)):
        gemm_case(L, case, "short", "workspace 4 bytes short")


def test_gemm_wrapper(ops):
    for case in (ref.GEMM_SPLIT[7], ref.GEMM_SCALARS[2], ref.GEMM_PADDED[1]):
        a, b, c0 = ref.gemm_inputs(case)
        S, _ = ref.gemm_slabs(case) if case.split else (1, case.K)
        out = c0.cuda() if case.beta != 0 else None
        if case.split:                                              # the wrapper must hand its workspace on: the restated condition on its 32 M N floats, and the slabs in it
            nbytes = 32 * case.M * case.N * 4
            assert S == 11 and ref.gemm_route(case.M, case.N, case.K, nbytes)[0] == 11
            wsb = ops._workspace(nbytes, torch.device("cuda", torch.cuda.current_device()))
            wsf = wsb[:wsb.numel() // 4 * 4].view(torch.float32)
            wsf.fill_(FILL)
        got = ops.gemm_f32(dev(a, case.pad), dev(b, case.pad), trans_a=case.ta, trans_b=case.tb, alpha=case.alpha, out=out, beta=case.beta)
        assert got.shape == (case.M, case.N) and (out is None or got is out)
        if case.split:
            assert bool((wsf[:S * case.M * case.N] != FILL).all()), "ops.gemm_f32 did not take the split-K route"
        record("gemm_f32", f"ops.gemm_f32 S={S}", f"{case.M}x{case.N}x{case.K}", case.family, worst_ratio(got, *ref.gemm_reference(case, S)))


def test_wrappers_refuse_bad_operands(ops, L):
    a, b = torch.randn(8, 16, device="cuda"), torch.randn(16, 12, device="cuda")
    for bad in (torch.zeros(8, 12, device="cuda", dtype=torch.float16), torch.zeros(8, 13, device="cuda"), torch.zeros(12, 8, device="cuda").t(),
                torch.zeros(8, 24, device="cuda")[:, ::2]):
        with pytest.raises(L.PclipError, match="gemm_f32: `out`"):
            ops.gemm_f32(a, b, out=bad, beta=1.0)
    x = torch.randn(8, 12, device="cuda")
    for bad in (torch.zeros(12, device="cuda", dtype=torch.float64), torch.zeros(11, device="cuda"), torch.zeros(24, device="cuda")[::2]):
        with pytest.raises(L.PclipError, match="colsum_f32: `out`"):
            ops.colsum_f32(x, out=bad)
    rs = torch.randn(8, device="cuda")
    for c, xx, r, name in ((x.half(), x, rs, "c"), (x, x.half(), rs, "x"), (x, x[:7], rs, "x"), (x, x, rs.double(), "rowscale"), (x, x, rs[:7], "rowscale"),
                           (x.t().contiguous().t(), x, rs, "c"), (x, torch.randn(8, 24, device="cuda")[:, ::2], rs, "x")):
        with pytest.raises(L.PclipError, match=f"addscaled_rows_: `{name}`"):
            ops.addscaled_rows_(c, xx, r, 1.0)


# ---- colsum_f32 -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.COLSUM_CASES, ids=lambda c: f"{c.R}x{c.C}{'-short' if c.ws == 'short' else ''}{'' if c.ws else '-nows'}")
def test_colsum(L, case):
    lib = L.load()
    x, out0, scale = ref.colsum_inputs(case)
    R, C = case.R, case.C
    xd = padded(x if R else torch.zeros(1, C), 3)
    ws_bytes = ref.colsum_ws_bytes(case)
    rb = ref.colsum_route(R, C, ws_bytes)
    ws_floats = 64 * C                                               # what ref.colsum_ws_bytes offers at most: room for any split

    def run():
        buf, out = vector(C, fill=out0.cuda() if case.accumulate else None)
        ws = scratch(ws_floats)
        L.check(lib.pclip_colsum_f32(L.ptr(xd), C + 3, R, C, scale, L.ptr(out), int(case.accumulate), L.ptr(ws) if ws_bytes else None, ws_bytes, L.stream()), "pclip_colsum_f32")
        assert intact(buf, C) and bool((ws[ws_floats:] == FILL).all())
        return buf, ws
    buf, ws = twice(run)
    written = ws[:ws_floats] != FILL
    used = rb * C if rb > 1 else 0
    assert bool(written[:used].all()) and not bool(written[used:].any()), "the workspace tells another route than the entry's condition"
    want, tol = ref.colsum_reference(case)
    record("colsum_f32", ("two-pass rb=%d" % rb) if rb > 1 else ("single pass" + (", workspace 4 bytes short" if case.ws == "short" else "")),
           f"{R}x{C} acc={int(case.accumulate)} scale={'1/R' if case.mean else '1'}", case.family, worst_ratio(buf[1], want, tol))


def test_colsum_wrapper(ops):
    for case in (ref.COLSUM_CASES[9], ref.COLSUM_CASES[4]):
        x, out0, scale = ref.colsum_inputs(case)
        out = out0.cuda() if case.accumulate else None
        got = ops.colsum_f32(padded(x, 3), scale=scale, out=out)
        record("colsum_f32", "ops.colsum_f32", f"{case.R}x{case.C}", case.family, worst_ratio(got, *ref.colsum_reference(case)))


# ---- the flat kernels -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.ADDSCALED_CASES + [FLAT_BIG + ("normal",)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_addscaled_rows(L, ops, shape):
    R, D, fam = shape
    assert (R * D > ref.FLAT_SWEEP) == (shape[:2] == FLAT_BIG)
    c, x, rs, s = ref.addscaled_inputs(R, D, fam)
    xd, rsd = padded(x, 3), rs.cuda()

    def run():
        buf, cd = window(R, D, 5, fill=c)
        L.check(L.load().pclip_addscaled_rows_f32(L.ptr(cd), D + 5, L.ptr(xd), D + 3, L.ptr(rsd), s, R, D, L.stream()), "pclip_addscaled_rows_f32")
        assert intact(buf, D)
        return (buf,)
    (buf,) = twice(run)
    want, tol = ref.addscaled_reference(c.cuda(), x.cuda(), rsd, s)
    record("addscaled_rows", "grid-stride x2" if shape[:2] == FLAT_BIG else "one sweep", f"{R}x{D}", fam, worst_ratio(buf[1:-1, :D], want, tol))
    if R == 23:
        got = ops.addscaled_rows_(c.clone().cuda(), xd, rsd, s)
        record("addscaled_rows", "ops.addscaled_rows_", f"{R}x{D}", fam, worst_ratio(got, want, tol))


@pytest.mark.parametrize("case", ref.SOFT_CASES[:6] + [ref.Soft(FLAT_BIG[0], FLAT_BIG[1], 0.2, 12.0, 0, "uniform")], ids=lambda c: f"{c.Q}x{c.N}")
def test_nll_mean_backward(L, ops, case):
    Q, N = case.Q, case.N
    if case.family == "uniform":
        g = torch.Generator().manual_seed(5)
        p32, labels = 0.01 + 0.99 * torch.rand(Q, N, generator=g), torch.randint(0, N, (Q,), generator=g)
    else:
        p32, labels = ref.soft_p32(case), ref.soft_inputs(case)[2]
    assert (Q * N > ref.FLAT_SWEEP) == (case.family == "uniform") and int(labels.min()) >= 0 and int(labels.max()) < N
    pd, lab, gd = padded(p32, 3), labels.to(torch.int32).cuda(), torch.tensor([0.37], device="cuda")

    def run():
        buf, dp = window(Q, N, 5)
        L.check(L.load().pclip_nll_mean_backward(L.ptr(pd), N + 3, L.ptr(lab), Q, N, L.ptr(gd), L.ptr(dp), N + 5, L.stream()), "pclip_nll_mean_backward")
        assert intact(buf, N)
        return (buf,)
    (buf,) = twice(run)
    want, tol = ref.nll_mean_bwd_reference(p32.cuda(), labels.cuda(), 0.37)
    got = buf[1:-1, :N]
    assert bool((got[want == 0] == 0).all()), "a non-zero off the label"
    record("nll_mean_backward", "grid-stride x2" if case.family == "uniform" else "one sweep", f"{Q}x{N}", case.family, worst_ratio(got, want, tol))
    if Q == 23:
        got = ops.nll_mean_backward(pd, labels.cuda(), gd)
        record("nll_mean_backward", "ops.nll_mean_backward", f"{Q}x{N}", case.family, worst_ratio(got, want, tol))


def _nan_equal_bits(got, want, as_int):
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and torch.equal(got.view(as_int)[~nan], want.view(as_int)[~nan])


@pytest.mark.parametrize("n", [1, 7, 8, 13, 2051, FLAT_BIG[0] * FLAT_BIG[1]])
def test_cast_f16_f32_bit_exact(L, ops, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int32).to(torch.int16).view(torch.float16)          # every fp16 bit pattern: subnormals, infinities, NaNs
    xd = x.cuda()

    def run():
        buf, y = flat(n, torch.float32)
        L.check(L.load().pclip_cast_f16_f32(L.ptr(xd), L.ptr(y), n, L.stream()), "pclip_cast_f16_f32")
        assert flat_intact(buf)
        return (buf[64:64 + n].clone(),)
    (y,) = run()
    assert _nan_equal_bits(y.cpu(), x.float(), torch.int32)
    assert _nan_equal_bits(run()[0], y, torch.int32)
    if n == 2051:
        assert _nan_equal_bits(ops.cast_f32(xd).cpu(), x.float(), torch.int32)
    print(f"LEDGER cast_f16_f32 | {'grid-stride x2' if n > ref.FLAT_SWEEP else 'one sweep'} | n={n} | bit patterns | 0.000")


@pytest.mark.parametrize("n", [1, 5, 8, 13, 2051, FLAT_BIG[0] * FLAT_BIG[1], 8 * FLAT_BIG[0] * FLAT_BIG[1] + 5])
def test_cast_f32_f16_round_to_nearest_even(L, ops, n):
    """RNE with subnormals, overflow to +-inf, NaN and +-0, bit for bit.  This kernel moves eight elements per lane: its grid-stride loop iterates above 8 x 16 384 x 256
    elements, the last size (the 4099 x 1024 block eight times over and a tail of five for the scalar tail)."""
    base = ref.cast_f32_input(min(n, FLAT_BIG[0] * FLAT_BIG[1]))
    x = base if n <= base.numel() else torch.cat([base] * 8 + [base[:5]])
    assert x.numel() == n
    xd = x.cuda()

    def run():
        buf, y = flat(n, torch.float16)
        L.check(L.load().pclip_cast_f32_f16(L.ptr(xd), L.ptr(y), n, L.stream()), "pclip_cast_f32_f16")
        assert flat_intact(buf)
        return buf[64:64 + n].clone()
    y = run()
    assert ref.half_bits_equal(y, x)
    assert _nan_equal_bits(run(), y, torch.int16)
    if n == 2051:
        assert ref.half_bits_equal(ops.cast_f16(xd), x)
    print(f"LEDGER cast_f32_f16 | {'grid-stride x2' if n > 8 * ref.FLAT_SWEEP else 'one sweep'} | n={n} | specials + bit patterns | 0.000")


# ---- the row kernels --------------------------------------------------------------------------------------------------------------------------------------------------
def _soft_id(c):
    return f"{c.Q}x{c.N}-a{c.alpha}-b{c.beta}-{c.family}"


SOFT_ALL = ref.SOFT_CASES + [ref.SOFT_BIG]


def _sweeps(rows):
    return "row loop x2" if rows > ref.ROW_SWEEP else "one sweep"


@pytest.mark.parametrize("case", SOFT_ALL, ids=_soft_id)
def test_nll_grad(L, ops, case):
    lib = L.load()
    Q, N, qt = case.Q, case.N, case.Q + case.q_extra
    di, dt, labels, _ = ref.soft_inputs(case)
    assert int(labels.min()) >= 0 and int(labels.max()) < N          # the kernel indexes with the label
    ldd = N + 3
    did, dtd, lab = padded(di, 3), padded(dt, 3), labels.to(torch.int32).cuda()
    al, oma = ref.f32(case.alpha), ref.f32(1.0 - case.alpha)

    def run():
        (bgi, gi), (bgt, gt) = window(Q, N, 3, fill=FILL), window(Q, N, 3, fill=FILL)
        (brs, rs), (bnl, nl), (bpm, pm), (bam, am) = vector(Q), vector(Q), vector(Q), vector(Q, torch.int32)
        L.check(lib.pclip_nll_grad(L.ptr(did), L.ptr(dtd), L.ptr(lab), Q, qt, N, ldd, al, oma, case.beta, L.ptr(gi), L.ptr(gt), L.ptr(rs), L.ptr(nl), L.ptr(pm), L.ptr(am),
                                   L.stream()), "pclip_nll_grad")
        assert intact(bgi, N) and intact(bgt, N), "columns >= N of gi / gt (or a guard row) were written"
        assert all(guards_intact(b) for b in (brs, bnl, bpm, bam))
        return bgi, bgt, brs, bnl, bpm, bam
    bgi, bgt, brs, bnl, bpm, bam = twice(run)
    got = dict(gi=bgi[1:-1, :N], gt=bgt[1:-1, :N], rowsum=brs[1], nll=bnl[1])
    want, tol, p, tol_p = ref.nll_grad_reference(di, dt, labels, case.alpha, case.beta, qt)
    shape, route = f"{Q}x{N} alpha={case.alpha} beta={case.beta} q_total={qt}", _sweeps(Q)
    for k in ("gi", "gt", "rowsum", "nll"):
        record(f"nll_grad.{k}", route, shape, case.family, worst_ratio(got[k], want[k], tol[k]))
    record("nll_grad.argmax+pmax", route, shape, case.family, ref.grade_argmax(bam[1].cpu(), bpm[1].cpu(), p, tol_p, ref.tie_classes(di, dt, case.beta)))
    if case.alpha == 0.0:
        assert bool((got["gi"] == 0).all()), "gi must be exact zeros at alpha = 0"
    if case.alpha == 1.0:
        assert bool((got["gt"] == 0).all()), "gt must be exact zeros at alpha = 1"
    if case.family == "ties" or case.beta == 0:                      # three equal maxima (every column at beta = 0): the lowest index, exactly
        assert torch.equal(bam[1].cpu().long(), ref.first_max(p))
    if (Q, N) == (23, 1000):
        gi, gt, rs, nll, pmax, am = ops.nll_grad(did._base, dtd._base, labels.cuda(), N, case.alpha, case.beta, q_total=qt)          # the wrapper takes the padded rows whole
        assert gi.shape == (Q, ldd) and torch.equal(am, bam[1]) and torch.equal(pmax, bpm[1])
        for k, t in (("gi", gi[:, :N]), ("gt", gt[:, :N]), ("rowsum", rs), ("nll", nll)):
            record(f"nll_grad.{k}", "ops.nll_grad", shape, case.family, worst_ratio(t, want[k], tol[k]))


@pytest.mark.parametrize("case", SOFT_ALL, ids=_soft_id)
def test_fuse_probs_backward(L, ops, case):
    lib = L.load()
    Q, N = case.Q, case.N
    di, dt, _, dp = ref.soft_inputs(case)
    ldd, ldp = N + 3, N + 2
    did, dtd, dpd = padded(di, 3), padded(dt, 3), padded(dp, 2)
    al, oma, be = ref.f32(case.alpha), ref.f32(1.0 - case.alpha), ref.f32(case.beta)

    def run():
        (bgi, gi), (bgt, gt), (brs, rs) = window(Q, N, 3, fill=FILL), window(Q, N, 3, fill=FILL), vector(Q)
        L.check(lib.pclip_fuse_probs_backward(L.ptr(did), L.ptr(dtd), L.ptr(dpd), ldp, Q, N, ldd, al, oma, be, L.ptr(gi), L.ptr(gt), L.ptr(rs), L.stream()),
                "pclip_fuse_probs_backward")
        assert intact(bgi, N) and intact(bgt, N), "columns >= N of gi / gt (or a guard row) were written"
        assert guards_intact(brs)
        return bgi, bgt, brs
    bgi, bgt, brs = twice(run)
    got = dict(gi=bgi[1:-1, :N], gt=bgt[1:-1, :N], rowsum=brs[1])
    want, tol = ref.fuse_bwd_reference(di, dt, dp, case.alpha, case.beta)
    shape = f"{Q}x{N} alpha={case.alpha} beta={case.beta}"
    for k in ("gi", "gt", "rowsum"):
        record(f"fuse_probs_backward.{k}", _sweeps(Q), shape, case.family, worst_ratio(got[k], want[k], tol[k]))
    if case.alpha == 0.0:
        assert bool((got["gi"] == 0).all())
    if case.alpha == 1.0:
        assert bool((got["gt"] == 0).all())
    if (Q, N) == (23, 1000):
        gi, gt, rs = ops.fuse_probs_backward(did._base, dtd._base, dp.cuda(), N, case.alpha, case.beta)
        for k, t in (("gi", gi[:, :N]), ("gt", gt[:, :N]), ("rowsum", rs)):
            record(f"fuse_probs_backward.{k}", "ops.fuse_probs_backward", shape, case.family, worst_ratio(t, want[k], tol[k]))


@pytest.mark.parametrize("case", SOFT_ALL, ids=_soft_id)
def test_nll_rows(L, ops, case):
    Q, N = case.Q, case.N
    p32, labels = ref.soft_p32(case), ref.soft_inputs(case)[2]
    pd, lab = padded(p32, 3), labels.to(torch.int32).cuda()

    def run():
        (bnl, nl), (bpm, pm), (bam, am) = vector(Q), vector(Q), vector(Q, torch.int32)
        L.check(L.load().pclip_nll_rows(L.ptr(pd), N + 3, L.ptr(lab), Q, N, L.ptr(nl), L.ptr(pm), L.ptr(am), L.stream()), "pclip_nll_rows")
        assert all(guards_intact(b) for b in (bnl, bpm, bam))
        return bnl, bpm, bam
    bnl, bpm, bam = twice(run)
    nll, tol, pmax, am = ref.nll_rows_reference(p32, labels)
    assert torch.equal(bam[1].cpu().long(), am), "argmax is not the lowest index of the maximum"
    assert torch.equal(bpm[1].cpu(), pmax)
    record("nll_rows.nll", _sweeps(Q), f"{Q}x{N}", case.family, worst_ratio(bnl[1], nll, tol))
    if (Q, N) == (23, 1000):
        g_nll, g_pmax, g_am = ops.nll_rows(pd, labels.cuda())
        assert torch.equal(g_am.cpu().long(), am) and torch.equal(g_pmax.cpu(), pmax)
        record("nll_rows.nll", "ops.nll_rows", f"{Q}x{N}", case.family, worst_ratio(g_nll, nll, tol))


@pytest.mark.parametrize("shape", ref.CE_CASES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_softmax_ce_rows(L, ops, shape):
    R, C, fam = shape
    S, scale = ref.ce_inputs(R, C, fam)
    Sd = padded(S, 3)

    def run():
        (bd, dS), (bl, loss) = window(R, C, 5), vector(R)
        L.check(L.load().pclip_softmax_ce_rows(L.ptr(Sd), C + 3, R, C, scale, L.ptr(dS), C + 5, L.ptr(loss), L.stream()), "pclip_softmax_ce_rows")          # lds != ldds
        assert intact(bd, C) and guards_intact(bl)
        return bd, bl
    bd, bl = twice(run)
    (w_loss, w_dS), (t_loss, t_dS) = ref.ce_reference(S, scale)
    record("softmax_ce_rows.loss", "one sweep", f"{R}x{C}", fam, worst_ratio(bl[1], w_loss, t_loss))
    record("softmax_ce_rows.dS", "one sweep", f"{R}x{C}", fam, worst_ratio(bd[1:-1, :C], w_dS, t_dS))
    if (R, C) == (23, 130):
        loss, dS = ops.softmax_ce_rows(Sd, scale)
        record("softmax_ce_rows.loss", "ops.softmax_ce_rows", f"{R}x{C}", fam, worst_ratio(loss, w_loss, t_loss))
        record("softmax_ce_rows.dS", "ops.softmax_ce_rows", f"{R}x{C}", fam, worst_ratio(dS[:, :C], w_dS, t_dS))


@pytest.mark.parametrize("shape", ref.L2_CASES + [ref.L2_BIG], ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_l2norm_rows_and_backward(L, ops, shape):
    R, D, fam = shape                                                # R rows are launched; the zero row and the row below eps are among them (ref.l2_special)
    x, gy, gx0 = ref.l2_inputs(R, D, fam)
    zero, sub = ref.l2_special(R, fam)
    assert x.shape == (R, D) and (zero is None or float(x[zero].abs().max()) == 0.0) and (sub is None or 0.0 < float(x[sub].norm()) < ref.L2_EPS)
    xd, gyd = x.cuda(), gy.cuda()
    x64, gy64, gx64 = x.double().cuda(), gy.double().cuda(), gx0.double().cuda()
    route = _sweeps(R)

    def fwd():
        buf, y = window(R, D, 0)
        L.check(L.load().pclip_l2norm_rows_f32(L.ptr(xd), L.ptr(y), R, D, ref.L2_EPS, L.stream()), "pclip_l2norm_rows_f32")
        assert guards_intact(buf)
        return (buf,)
    (buf,) = twice(fwd)
    want, tol = ref.l2_reference(x64)
    assert zero is None or bool((buf[1 + zero] == 0).all()), "the zero row"
    record("l2norm_rows_f32", route, f"{R}x{D}", fam, worst_ratio(buf[1:-1], want, tol))
    for acc in (False, True):
        def bwd():
            buf, gx = window(R, D, 0, fill=gx0 if acc else None)      # accumulate = 0 must not read gx: it holds NaN
            L.check(L.load().pclip_l2norm_rows_backward_f32(L.ptr(xd), L.ptr(gyd), L.ptr(gx), R, D, ref.L2_EPS, int(acc), L.stream()), "pclip_l2norm_rows_backward_f32")
            assert guards_intact(buf)
            return (buf,)
        (buf,) = twice(bwd)
        want, tol = ref.l2_bwd_reference(x64, gy64, gx64 if acc else None)
        record("l2norm_rows_backward_f32", f"{route} accumulate={int(acc)}", f"{R}x{D}", fam, worst_ratio(buf[1:-1], want, tol))
    if (R, D) == (23, 65):
        record("l2norm_rows_f32", "ops.l2norm_rows_f32", f"{R}x{D}", fam, worst_ratio(ops.l2norm_rows_f32(xd), *ref.l2_reference(x64)))
        got = ops.l2norm_rows_backward_f32_(gx0.clone().cuda(), xd, gyd)
        record("l2norm_rows_backward_f32", "ops.l2norm_rows_backward_f32_", f"{R}x{D}", fam, worst_ratio(got, *ref.l2_bwd_reference(x64, gy64, gx64)))
