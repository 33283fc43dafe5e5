"""pclip_feature_reg_f16 / pclip_feature_reg_backward_f16 (csrc/pclip_feature_reg.hip), ops.feature_reg(_backward), autograd.FeatureRegFn and the losses
built on them: against float64 under the tolerances tests/feature_reg_ref.py derives, BIT FOR BIT against its numpy-float32 emulation of the walk the kernel
file's header documents, and against the kernels' own identities bit for bit.

BIT_EXACT: every operation of the kernel is one correctly rounded fp32 operation (no approximate reciprocal or square root: the file's header), so the
emulation is graded by equality of bits, not by tolerance.

Shapes (M, D): one wave takes a row and four rows make a workgroup — M = 1, 3, 4, 33, 65 are one row, a ragged workgroup, a full one, and several; a lane
holds ceil(D / 512) vectors in a kernel compiled for 1, 2, 4 or 8 of them — D = 8 and 64 leave most lanes empty, 72 and 520 are ragged (520: one lane with
a second vector), 512 and 1024 fill one and two, 2056 and 4096 reach the other two kernels.  The loss's second stage starts past PCLIP_FREG_CHUNK = 1024
rows: M = 1000 is below, 1024 on it, 1025 and 2051 past it (two and three chunks, the last one ragged)."""
import numpy as np
import pytest
import torch

import feature_reg_ref as fr
from conftest import observe

pytestmark = pytest.mark.gpu

BIT_EXACT = True
SHAPES = fr.GPU_SHAPES
MODES = [("l1", False), ("l1", True), ("cos", False), ("cos", True)]
_CASES = {}


def case(M, D):
    """fp16 operands on the host, shared between the tests and never modified; the target pulled halfway towards x (tests/test_feature_reg_cpu.py holds the
    same cases and shows that float64 alone leaves at most 0.1 % of their L1 elements undecided)."""
    if (M, D) not in _CASES:
        _CASES[(M, D)] = fr.make_case(M, D, fr.case_seed(M, D), cluster=0.5)
    return _CASES[(M, D)]


def dev(a):
    return torch.from_numpy(a).cuda()


def run(x, t, mode, nt, grad=1.0, mean_over=None):
    from proto_clip_amd import ops
    loss, inv, rows = ops.feature_reg(x, t, mode, nt, want_rows=True)
    dx = ops.feature_reg_backward(x, t, inv, mode, nt, grad=grad, mean_over=mean_over)
    return {"loss": loss, "rows": rows, "inv_norm": inv, "dx": dx}


def host(got):
    return {k: v.detach().cpu().numpy() for k, v in got.items()}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def check(tag, got, x16, t16, mode, nt, **kw):
    """float64 under the derived tolerances (figures recorded before anything is asserted), then the emulation bit for bit."""
    r = fr.grade(got, x16, t16, mode, nt, **kw)
    for k in ("loss", "rows", "inv_norm", "dx"):
        observe(f"feature reg {mode} {k}: |got - float64| / derived tolerance", r[k], 1.0)
    print(tag, {k: (round(v, 4) if k != "undecided_share" else v) for k, v in r.items()})
    assert r["undecided_share"] <= 1e-3, r
    for k in ("loss", "rows", "inv_norm", "dx"):
        assert r[k] <= 1.0, (tag, k, r[k])
    if BIT_EXACT:
        emu = fr.emulate(x16, t16, mode, nt, **kw)
        for k in ("rows", "inv_norm", "dx", "loss"):
            same = bits(got[k]) == bits(emu[k])
            assert same.all(), (tag, k, int((~same).sum()), "elements differ from the emulation")


@pytest.mark.parametrize("mode,nt", MODES)
@pytest.mark.parametrize("M,D", SHAPES)
def test_against_float64_and_the_emulation(M, D, mode, nt):
    x16, t16 = case(M, D)
    check(f"freg {mode} nt={nt} {M}x{D}", host(run(dev(x16), dev(t16), mode, nt)), x16, t16, mode, nt)


@pytest.mark.parametrize("mode,nt", MODES)
def test_strided_views_between_guard_bands(mode, nt):
    """Columns 8 .. 8 + D of wider buffers (row strides 96 and 112 halves, NaN everywhere else), and the outputs inside NaN-filled buffers that must keep
    their guard bands: nothing outside [M, D] is read, nothing outside the outputs written."""
    from proto_clip_amd import _lib
    from proto_clip_amd._lib import check as rc_check, ptr, stream
    M, D = 9, 72
    x16, t16 = case(M, D)

    def wide(a, ld):
        buf = torch.full((M + 2, ld), float("nan"), dtype=torch.float16)
        buf[1:M + 1, 8:8 + D] = torch.from_numpy(a)
        return buf.cuda()
    xb, tb = wide(x16, 96), wide(t16, 112)
    xv, tv = xb[1:M + 1, 8:8 + D], tb[1:M + 1, 8:8 + D]
    got = host(run(xv, tv, mode, nt))
    dense = host(run(dev(x16), dev(t16), mode, nt))
    for k in got:
        assert (bits(got[k]) == bits(dense[k])).all(), k
    # the C entries on the views, outputs in the middle of guarded buffers
    G = 16
    out = {k: torch.full((n + 2 * G,), float("nan"), dtype=torch.float32, device="cuda") for k, n in (("loss", 1), ("rows", M), ("inv_norm", M), ("dx", M * D))}
    mid = {k: v[G:v.numel() - G] for k, v in out.items()}
    lib, m = _lib.load(), {"l1": _lib.FREG_L1, "cos": _lib.FREG_COS}[mode]
    rc_check(lib.pclip_feature_reg_f16(ptr(xv), 96, ptr(tv), 112, M, D, m, int(nt), ptr(mid["loss"]), ptr(mid["rows"]), ptr(mid["inv_norm"]), None, 0, stream()),
             "forward")
    w = float(np.float32(fr.weight_of(M, D, mode)))
    rc_check(lib.pclip_feature_reg_backward_f16(ptr(xv), 96, ptr(tv), 112, M, D, m, int(nt), w, ptr(mid["dx"]), stream()), "backward")
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool(torch.isnan(v[:G]).all()) and bool(torch.isnan(v[-G:]).all()), k
        assert (bits(mid[k].cpu().numpy().reshape(dense[k].shape)) == bits(dense[k])).all(), k
    check(f"freg strided {mode} nt={nt}", got, x16, t16, mode, nt)


def test_target_equal_to_x_gives_plus_zero_in_l1_and_rounding_level_in_cos():
    """t is x under normalize_t: n and t' come from one instruction sequence, so every L1 difference is exactly 0: rows and loss +0, dx all zeros, bit for
    bit.  COS has no such identity (1 - sum n_d^2 is a rounding residue, not 0): it is graded by its tolerance against float64's 0."""
    M, D = 33, 520
    x16, _ = case(M, D)
    got = host(run(dev(x16), dev(x16), "l1", True))
    assert (bits(got["loss"]) == 0).all() and (bits(got["rows"]) == 0).all()
    assert (got["dx"] == 0).all()
    check("freg cos t == x", host(run(dev(x16), dev(x16), "cos", True)), x16, x16, "cos", True)


@pytest.mark.parametrize("mode,nt", MODES)
def test_a_row_keeps_its_bits_under_permutation_and_in_another_batch(mode, nt):
    M, D = 65, 512
    x16, t16 = case(M, D)
    base = host(run(dev(x16), dev(t16), mode, nt, mean_over=M))
    perm = np.random.default_rng(0).permutation(M)
    got = host(run(dev(x16[perm]), dev(t16[perm]), mode, nt, mean_over=M))
    for k in ("rows", "inv_norm", "dx"):
        assert (bits(got[k]) == bits(base[k][perm])).all(), k
    sub = slice(7, 12)
    got = host(run(dev(x16[sub].copy()), dev(t16[sub].copy()), mode, nt, mean_over=M))
    for k in ("rows", "inv_norm", "dx"):
        assert (bits(got[k]) == bits(base[k][sub])).all(), k
    big_x, big_t = fr.make_case(1030, D, 5)                              # the same rows at the far end of a batch past the chunk boundary
    big_x[-5:], big_t[-5:] = x16[sub], t16[sub]
    got = host(run(dev(big_x), dev(big_t), mode, nt, mean_over=M))
    for k in ("rows", "inv_norm", "dx"):
        assert (bits(got[k][-5:]) == bits(base[k][sub])).all(), k


@pytest.mark.parametrize("mode,nt", MODES)
def test_a_zero_row_poisons_itself_and_the_loss_only(mode, nt):
    M, D = 33, 520
    x16, t16 = case(M, D)
    base = host(run(dev(x16), dev(t16), mode, nt, mean_over=M))
    z = x16.copy()
    z[17] = 0
    got = host(run(dev(z), dev(t16), mode, nt, mean_over=M))
    assert np.isnan(got["loss"]) and np.isnan(got["rows"][17]) and np.isnan(got["dx"][17]).all() and np.isinf(got["inv_norm"][17])
    keep = np.arange(M) != 17
    for k in ("rows", "inv_norm", "dx"):
        assert (bits(got[k][keep]) == bits(base[k][keep])).all(), k


def test_empty_batch_is_plus_zero():
    from proto_clip_amd import ops
    x = torch.zeros(0, 64, dtype=torch.float16, device="cuda")
    loss, inv, rows = ops.feature_reg(x, x, "l1", False, want_rows=True)
    assert bits(loss.cpu().numpy()) == 0 and inv.shape == (0,) and rows.shape == (0,)
    assert ops.feature_reg_backward(x, x, inv, "l1", False).shape == (0, 64)


@pytest.mark.parametrize("mode,nt", MODES)
def test_graph_replay_reproduces_the_eager_bits(mode, nt):
    from proto_clip_amd import ops
    M, D = 1025, 16                                                      # three forward launches
    x16, t16 = case(M, D)
    x, t = dev(x16), dev(t16)
    eager = host(run(x, t, mode, nt))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, t, mode, nt)                                              # warm the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(x, t, mode, nt)
    for v in captured.values():
        v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    replayed = host(captured)
    for k in eager:
        assert (bits(replayed[k]) == bits(eager[k])).all(), k


@pytest.mark.parametrize("mode,nt", MODES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_autograd_function_agrees_with_the_ops_pair(mode, nt, dtype):
    """FeatureRegFn's gradient is the kernel's dx times the upstream gradient in fp32, cast to x's dtype: fp32 in, fp32 out."""
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import ops
    M, D = 33, 520
    x16, t16 = case(M, D)
    x = dev(x16).to(dtype).requires_grad_(True)
    t = dev(t16)
    loss = pag.feature_reg(x, t, mode, nt)
    (loss * 3.0).backward()
    want = run(dev(x16), t, mode, nt)
    assert torch.equal(loss.detach(), want["loss"]) and loss.dtype == torch.float32
    g = want["dx"] * torch.tensor(3.0, device="cuda")
    assert x.grad.dtype == dtype
    assert torch.equal(x.grad, ops.cast_f16(g.contiguous()) if dtype == torch.float16 else g)
    with torch.no_grad():
        assert torch.equal(pag.feature_reg(x, t, mode, nt), want["loss"])
    # finite differences of the float64 function agree with float64's own gradient (the reference the kernel is graded against)
    ref = fr.reference(x16, t16, mode, nt)
    m, d, h = 5, 17, 2.0 ** -8
    xp, xm = x16.astype(np.float64), x16.astype(np.float64)
    xp[m, d] += h
    xm[m, d] -= h
    f = lambda xx: _loss64(xx, t16.astype(np.float64), mode, nt)
    assert abs((f(xp) - f(xm)) / (2 * h) - ref["dx"][m, d]) <= 1e-6 * abs(ref["dx"][m, d]) + 1e-12


def _loss64(x, t, mode, nt):
    n = x / np.sqrt((x * x).sum(1, keepdims=True))
    tp = t / np.sqrt((t * t).sum(1, keepdims=True)) if nt else t
    return np.abs(n - tp).mean() if mode == "l1" else 1.0 - (n * tp).sum(1).mean()


def test_utils_losses_are_the_autograd_function():
    from proto_clip_amd import autograd as pag
    from proto_clip_amd import utils
    x16, t16 = case(33, 520)
    x, t = dev(x16), dev(t16)
    assert torch.equal(utils.clip_feature_l1_loss(x, t), pag.feature_reg(x, t, "l1", False))
    assert torch.equal(utils.clip_feature_l1_loss(x, t, normalize_target=True), pag.feature_reg(x, t, "l1", True))
    assert torch.equal(utils.clip_feature_cosine_loss(x, t, normalize_target=True), pag.feature_reg(x, t, "cos", True))
