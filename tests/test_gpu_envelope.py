"""Classification and its neighbours across the documented shape envelope ("Supported shapes": N <= 4096 classes, D <= 4096 features,
K <= 32 shots) against a plain float64 reference written here — not the kernels, not the fp32 oracle.

Acceptance rules, the same for every route (tolerances recorded with observe()):
  p        max |p - p64| <= tau, tau = max(1e-5, 2 max |po.P - p64|) on the same rows: the kernel may be at most twice as far from exact as the
           reference's own fp32 arithmetic (at D = 4096, beta = 20 that error exceeds 1e-5 by itself).
  argmax   0 <= am < N for every query (checked on the host); where the fp64 top-2 margin is > tau the fp64 argmax, elsewhere p64[am] >= max p64 - tau;
           exact duplicate prototypes: the lowest class (main.py:190).
  top-k    the t-th index's p64 within tau of the t-th largest p64, distinct indices, topk_p within tau of p64 there.
  hp_sweep each grid point's count within (number of queries whose fp64 top-2 margin there is < tau) of the fp64 count.
Returned class ids are compared on the host only and never used to index a device tensor."""
import math

import numpy as np
import pytest
import torch

from conftest import assert_adapter_close, observe, ulp_diff
from oracle import proto_oracle as po

pytestmark = pytest.mark.gpu
nrm = torch.nn.functional.normalize
TWO, PANELS = "two stages", "fused row panels"


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


# ---------------------------------------------------------------- float64 reference -------------------------------------------------
def f32(x):
    return float(np.float32(x))


def d64(q16, z16):
    """|q|^2 + |z|^2 - 2 q.z in float64 from the fp16 operands, clamped at 0."""
    q, z = q16.double(), z16.double()
    return (q.pow(2).sum(-1, keepdim=True) + z.pow(2).sum(-1)[None] - 2.0 * (q @ z.t())).clamp_min(0)


def softmax64(d, b32):
    x = -b32 * d
    e = (x - x.max(1, keepdim=True).values).exp()
    return e / e.sum(1, keepdim=True)


def p64_from_d(di, dt, alpha, beta):
    """alpha softmax(-beta di) + (1 - alpha) softmax(-beta dt) with the float32 alpha, 1 - alpha, beta the library receives (ops.classify: a32, oma32)."""
    b = f32(beta)
    return f32(alpha) * softmax64(di, b) + f32(1 - float(alpha)) * softmax64(dt, b)


def reference(q16, zi16, zt16, alpha, beta, chunk=512):
    """(p64 [R, N], tau) for CPU fp16 rows, in chunks of rows; tau from the fp32 oracle's own distance to p64 on the same rows."""
    ps, err = [], 0.0
    for i in range(0, q16.shape[0], chunk):
        qc = q16[i:i + chunk]
        p = p64_from_d(d64(qc, zi16), d64(qc, zt16), alpha, beta)
        err = max(err, (po.P(qc, zi16, zt16, alpha, beta).double() - p).abs().max().item())
        ps.append(p)
    return torch.cat(ps), max(1e-5, 2 * err)


def check_p(p, p64, tau, tag):
    e = observe(f"{tag}: max |p - p64| (bound: max(1e-5, 2 x the fp32 oracle's))", (p.cpu().double() - p64).abs().max().item(), tau)
    assert e <= tau, (tag, e, tau)


def check_argmax(am, p64, tau, N, tag):
    am = am.cpu().long()
    assert am.shape[0] == p64.shape[0]
    assert int(am.min()) >= 0 and int(am.max()) < N, (tag, int(am.min()), int(am.max()))
    top2 = p64.topk(2, dim=1)
    sure = (top2.values[:, 0] - top2.values[:, 1]) > tau
    wrong = (sure & (am != top2.indices[:, 0])).nonzero().flatten()
    assert len(wrong) == 0, (tag, wrong.tolist()[:10], am[wrong].tolist()[:10], top2.indices[wrong, 0].tolist()[:10])
    short = observe(f"{tag}: max p64 - p64[argmax] (near-ties)", (top2.values[:, 0] - p64.gather(1, am[:, None])[:, 0]).max().item(), tau)
    assert short <= tau, (tag, short, tau)


def check_topk(tp, ti, p64, tau, tag):
    tp, ti = tp.cpu().double(), ti.cpu().long()
    k = ti.shape[1]
    assert int(ti.min()) >= 0 and int(ti.max()) < p64.shape[1]
    assert bool((ti.sort(1).values.diff(dim=1) > 0).all()), f"{tag}: repeated top-k index"
    at = p64.gather(1, ti)
    e_ord = observe(f"{tag}: top-k |p64[t-th index] - t-th largest p64|", (at - p64.topk(k, dim=1).values).abs().max().item(), tau)
    e_val = observe(f"{tag}: top-k |topk_p - p64[index]|", (tp - at).abs().max().item(), tau)
    assert e_ord <= tau and e_val <= tau, (tag, e_ord, e_val, tau)


def banks(N, D, seed, device="cpu", structured=True):
    """(zi, zt, q-maker): class-structured prototypes (two noisy views of one centre per class) or structureless ones, unit rows in fp16."""
    g = torch.Generator(device=device).manual_seed(seed)
    cen = torch.randn(N, D, generator=g, device=device)
    if structured:
        zi = nrm(cen + 0.3 * torch.randn(N, D, generator=g, device=device), dim=-1).half()
        zt = nrm(cen + 0.5 * torch.randn(N, D, generator=g, device=device), dim=-1).half()
    else:
        zi = nrm(torch.randn(N, D, generator=g, device=device), dim=-1).half()
        zt = nrm(torch.randn(N, D, generator=g, device=device), dim=-1).half()

    def queries(Q, y=None):
        if y is None:
            y = torch.randint(0, N, (Q,), generator=g, device=device)
        noise = torch.randn(Q, D, generator=g, device=device)
        return nrm(cen[y] + 0.8 * noise if structured else noise, dim=-1).half(), y
    return zi, zt, queries


def panel_rows(Q):
    """The rows a large-Q reference is computed on: the first and last 256-row panels (the last one ragged unless Q % 256 == 0) and the middle panel."""
    mid = (Q // 512) * 256
    return sorted(set(range(0, min(Q, 256))) | set(range(mid, min(Q, mid + 256))) | set(range((Q - 1) // 256 * 256, Q)))


# ---------------------------------------------------------------- two stages: sqdist + fuse_probs ------------------------------------
# N at the DISPATCH_NV boundaries of fuse_probs / hp_sweep (NV = 1, 4, 16, 64 classes per lane) and the envelope's edge
TWO_STAGE = [(N, D) for N in (64, 65, 256, 257, 1024, 1025, 2048, 2049, 4095, 4096) for D in (64, 512)] + [(4096, 2112), (4096, 4096)]


@pytest.mark.parametrize("N,D", TWO_STAGE)
def test_two_stage_envelope_vs_float64(ops, N, D):
    Q = 300
    zi, zt, queries = banks(N, D, seed=N * 7 + D)
    q, _ = queries(Q)
    tags = f"two stages N={N} D={D}"
    for alpha, beta in ((0.5, 12.0), (0.8, 20.0)):
        p64, tau = reference(q, zi, zt, alpha, beta)
        with ops.classify_two_stage():
            assert ops.classify_route(Q, N, D, alpha, beta, want_p=True, want_argmax=True, topk=16) == TWO
            ops.classify_panel_stats(reset=True)
            p, am, tp, ti = ops.classify(q.cuda(), zi.cuda(), zt.cuda(), alpha, beta, want_p=True, want_argmax=True, topk=16)
            assert ops.classify_panel_stats()[0] == 0
        check_p(p, p64, tau, tags)
        check_argmax(am, p64, tau, N, tags)
        check_topk(tp, ti, p64, tau, tags)


def test_two_stage_distance_rows_beyond_2_31_bytes(ops):
    """Q = 140 000, N = 4096: a bank's distance rows (and p) span 2.3 GB, row 131 072 starts at byte 2^31.  Reference rows: the start, both sides of that
    offset, the end."""
    Q, N, D, alpha, beta = 140000, 4096, 512, 0.5, 12.0
    zi, zt, _ = banks(N, D, seed=31)
    g = torch.Generator(device="cuda").manual_seed(32)
    y = torch.randint(0, N, (Q,), generator=g, device="cuda")
    zic, ztc = zi.cuda(), zt.cuda()
    cen = (zi.float() + zt.float()).cuda()
    q = nrm(nrm(cen, dim=-1)[y] + 0.03 * torch.randn(Q, D, generator=g, device="cuda"), dim=-1).half()
    del cen
    with ops.classify_two_stage():
        assert ops.classify_route(Q, N, D, alpha, beta, want_p=True, want_argmax=True) == TWO
        p, am, _, _ = ops.classify(q, zic, ztc, alpha, beta, want_p=True, want_argmax=True)
    am_h = am.cpu().long()
    assert int(am_h.min()) >= 0 and int(am_h.max()) < N
    edge = 2 ** 31 // (N * 4)
    rows = list(range(0, 128)) + list(range(edge - 128, edge + 128)) + list(range(Q - 128, Q))
    idx = torch.tensor(rows, device="cuda")
    p64, tau = reference(q[idx].cpu(), zi, zt, alpha, beta)
    check_p(p[idx], p64, tau, "two stages across 2^31 bytes")
    check_argmax(am_h[rows], p64, tau, N, "two stages across 2^31 bytes")
    assert (am_h == y.cpu()).float().mean().item() > 0.9              # the queries sit next to their class: the whole batch is classified, not only the sampled rows
    del p, am, q
    ops.release_workspaces()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N", [1025, 4096])
def test_fuse_probs_nan_padding_nv64(ops, N):
    """fuse_probs straight from distance rows whose padding columns are NaN: the NV = 64 build must never read past N; an exact tie between class 5 and the
    last class resolves to 5."""
    Q = 200
    g = torch.Generator().manual_seed(N)
    d2i = torch.rand(Q, N, generator=g) * 4
    d2t = torch.rand(Q, N, generator=g) * 4
    d2i[3, 5] = d2i[3, N - 1] = 0.0
    d2t[3, 5] = d2t[3, N - 1] = 0.0
    ldd = ops.padded_ld(N) + 64
    pad = lambda d: torch.nn.functional.pad(d, (0, ldd - N), value=float("nan")).cuda()
    for alpha, beta in ((0.5, 20.0), (1.0, 3.0), (0.0, 0.5), (0.3, 0.0)):
        p64 = p64_from_d(d2i.double(), d2t.double(), alpha, beta)
        tau = max(1e-5, 2 * (po.P_from_dists(d2i, d2t, alpha, beta).double() - p64).abs().max().item())
        p, am, tp, ti = ops.fuse_probs(pad(d2i), pad(d2t), N, alpha, beta, want_p=True, want_argmax=True, topk=16)
        tag = f"fuse_probs NaN padding N={N}"
        check_p(p, p64, tau, tag)
        assert not bool(torch.isnan(p).any() | torch.isnan(tp).any())
        check_argmax(am, p64, tau, N, tag)
        check_topk(tp, ti, p64, tau, tag)
        if beta > 0:
            assert int(am[3]) == 5
        else:
            assert bool((am.cpu() == 0).all())                             # beta = 0: every class ties, the lowest wins


@pytest.mark.parametrize("N", [1025, 4096])
def test_hp_sweep_nv64_vs_float64(ops, N):
    """The (alpha, beta) grid of main.hp_grid() (11 x 29 = 319 pairs) at N past 1024 (the NV = 64 build): every count against the fp64 count, up to the queries
    whose fp64 top-2 margin at that pair is below tau."""
    from proto_clip_amd import main as pm
    Q, D = (1000 if N < 2048 else 512), 512
    zi, zt, queries = banks(N, D, seed=N + 5)
    q, y = queries(Q)
    noise = torch.rand(Q, generator=torch.Generator().manual_seed(1)) < 0.3
    y = torch.where(noise, (y + 1) % N, y)                                  # 30 % wrong labels: accuracies well inside (0, 1)
    al, bl = pm.hp_grid()
    d2i, d2t, _ = ops.sqdist(q.cuda(), zi.cuda(), zt.cuda())
    cnt = ops.hp_sweep(d2i, d2t, N, y.cuda(), al, bl).cpu().numpy()
    di64, dt64 = d64(q, zi), d64(q, zt)
    di32, dt32 = po.sqdist(q, zi), po.sqdist(q, zt)
    worst, excess = 0.0, 0.0
    for ib, beta in enumerate(bl):
        b = f32(beta)
        si, st = softmax64(di64, b), softmax64(dt64, b)
        si32, st32 = po.softmax_neg(di32, beta), po.softmax_neg(dt32, beta)
        for ia, alpha in enumerate(al):
            a, oma = f32(alpha), f32(1 - float(alpha))
            p64 = a * si + oma * st
            p32 = torch.tensor(float(alpha), dtype=torch.float32) * si32 + torch.tensor(1 - float(alpha), dtype=torch.float32) * st32   # po.P_from_dists
            tau = max(1e-5, 2 * (p32.double() - p64).abs().max().item())
            top2 = p64.topk(2, dim=1)
            ref = int((top2.indices[:, 0] == y).sum())
            ties = int(((top2.values[:, 0] - top2.values[:, 1]) < tau).sum())
            d = abs(int(cnt[ia, ib]) - ref)
            worst = max(worst, d)
            excess = max(excess, d - ties)
            assert d <= ties, (N, alpha, beta, int(cnt[ia, ib]), ref, ties)
    observe(f"hp_sweep N={N}: queries of difference at a grid point minus the fp64 near-ties there", excess, 0.0)
    observe(f"hp_sweep N={N}: queries of difference at a grid point", worst, float(Q))
    acc = cnt[5, 11] / Q                                                    # alpha = 0.5, beta = 3
    assert 0.5 < acc < 0.85, acc


# ---------------------------------------------------------------- fused row panels ---------------------------------------------------
_FUSED_PASSES = {}


FUSED_ENVELOPE = [(N, D) for N in (1025, 2048, 2049, 3000, 4095, 4096) for D in (128, 512, 2112, 4096)]


@pytest.mark.parametrize("structured", [True, False])
@pytest.mark.parametrize("N,D", FUSED_ENVELOPE)
def test_fused_row_panels_envelope_vs_float64(ops, N, D, structured):
    """Forced fused row panels, argmax only, at N past 16 class tiles (2049 .. 4096: the proof without per-tile masks, 32 tiles in the mask) and D past 2048
    (the PCLIP_PREP(8) preparation build).  Three panels, the last one ragged; one pass + proof == always two passes == second pass forced, bit for bit."""
    fused_row_panels_envelope(ops, N, D, structured, exact=False)


@pytest.mark.parametrize("structured", [True, False])
@pytest.mark.parametrize("N,D", FUSED_ENVELOPE)
def test_fused_row_panels_envelope_sqrt_round_trip_vs_float64(ops, N, D, structured):
    """The same with torch.cdist's sqrt round trip kept in the fused kernel (classify_panel_exact)."""
    fused_row_panels_envelope(ops, N, D, structured, exact=True)


def fused_row_panels_envelope(ops, N, D, structured, exact):
    Q, alpha, beta = 520, 0.5, 12.0
    zi, zt, queries = banks(N, D, seed=N + D + structured, structured=structured)
    q, _ = queries(Q)
    qc, zic, ztc = q.cuda(), zi.cuda(), zt.cuda()
    tag = f"fused panels N={N} D={D} {'structured' if structured else 'structureless'}{' exact' if exact else ''}"
    with ops.classify_fused(), ops.classify_panel_exact(exact):
        assert ops.classify_route(Q, N, D, alpha, beta) == PANELS
        outs = {}
        for passes in (0, 1, 2):
            with ops.classify_panel_passes(passes):
                ops.classify_panel_stats(reset=True)
                outs[passes] = ops.classify(qc, zic, ztc, alpha, beta, want_p=False, want_argmax=True)[1]
                npan, nsecond = ops.classify_panel_stats()
                if passes != 1:                                 # (the counters live in the candidate form: mode 1, two passes always, counts nothing)
                    assert npan == math.ceil(Q / 256), (passes, npan)
                if passes == 0:
                    stats = (npan, nsecond)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (tag, int((outs[0] != outs[1]).sum()), int((outs[0] != outs[2]).sum()))
    observe(f"{tag}: fraction of panels through the second pass", stats[1] / stats[0], 1.0)
    if N > 2048:
        _FUSED_PASSES[(N, D, structured, exact)] = stats
    p64, tau = reference(q, zi, zt, alpha, beta)
    check_argmax(outs[0], p64, tau, N, tag)


def test_fused_row_panels_both_proof_outcomes_ran(ops):
    """Across the N > 2048 cases above (no per-tile masks) some panels were proven in one pass and some took the second pass."""
    if len(_FUSED_PASSES) < 32:
        pytest.skip("runs after test_fused_row_panels_envelope_vs_float64 in the same session")
    npan = sum(s[0] for s in _FUSED_PASSES.values())
    nsecond = sum(s[1] for s in _FUSED_PASSES.values())
    assert 0 < nsecond < npan, (npan, nsecond)
    assert any(s[1] < s[0] for s in _FUSED_PASSES.values()) and any(s[1] > 0 for s in _FUSED_PASSES.values())


@pytest.mark.parametrize("N,D", [(4096, 512), (3000, 128), (2049, 2112)])
def test_beta_zero_every_class_ties(ops, N, D):
    """beta = 0: p = 1 / N for every class, an exact tie of all of them — every route returns class 0 for every query."""
    Q = 520
    zi, zt, queries = banks(N, D, seed=3 * N + D)
    q, _ = queries(Q)
    qc, zic, ztc = q.cuda(), zi.cuda(), zt.cuda()
    for alpha in (0.5, 1.0, 0.0):
        with ops.classify_fused():
            assert ops.classify_route(Q, N, D, alpha, 0.0) == PANELS
            for passes in (0, 1):
                with ops.classify_panel_passes(passes):
                    ops.classify_panel_stats(reset=True)
                    am = ops.classify(qc, zic, ztc, alpha, 0.0, want_p=False, want_argmax=True)[1].cpu()
                    assert passes == 1 or ops.classify_panel_stats()[0] == math.ceil(Q / 256)
                assert bool((am == 0).all()), (alpha, passes, am.unique()[:10].tolist())
        with ops.classify_two_stage():
            p, am, _, ti = ops.classify(qc, zic, ztc, alpha, 0.0, want_p=True, want_argmax=True, topk=16)
        assert bool((am.cpu() == 0).all()) and torch.equal(ti.cpu()[0], torch.arange(16, dtype=torch.int32))
        e = observe(f"beta = 0, N={N}: max |p - 1/N|", (p.double() - 1.0 / N).abs().max().item(), 1e-6)
        assert e <= 1e-6


@pytest.mark.parametrize("N,D", [(4096, 2112), (2049, 512), (4095, 128)])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_fused_alpha_at_the_ends(ops, N, D, alpha):
    """alpha = 0 (text bank only) and alpha = 1 (visual bank only) through the forced row panels against float64; the two stages agree with the same rule."""
    Q, beta = 520, 12.0
    zi, zt, queries = banks(N, D, seed=N + 11 * D)
    q, _ = queries(Q)
    p64, tau = reference(q, zi, zt, alpha, beta)
    tag = f"alpha={alpha} N={N} D={D}"
    with ops.classify_fused():
        assert ops.classify_route(Q, N, D, alpha, beta) == PANELS
        ops.classify_panel_stats(reset=True)
        am = ops.classify(q.cuda(), zi.cuda(), zt.cuda(), alpha, beta, want_p=False, want_argmax=True)[1]
        assert ops.classify_panel_stats()[0] == math.ceil(Q / 256)
    check_argmax(am, p64, tau, N, f"fused panels {tag}")
    with ops.classify_two_stage():
        p, am2, _, _ = ops.classify(q.cuda(), zi.cuda(), zt.cuda(), alpha, beta, want_p=True, want_argmax=True)
    check_p(p, p64, tau, f"two stages {tag}")
    check_argmax(am2, p64, tau, N, f"two stages {tag}")


def test_duplicate_prototypes_across_far_tiles(ops):
    """Class 100 copied to 3000 and 4095 in both banks (tiles 0, 23 and 31), class 1500 copied to 3500 in the visual bank only: the lowest class wins every
    exact tie, on every route (one pass + proof, two passes, the two stages); never a duplicate."""
    Q, N, D = 1200, 4096, 512
    zi, zt, queries = banks(N, D, seed=77)
    for dup in (3000, 4095):
        zi[dup] = zi[100]
        zt[dup] = zt[100]
    zi[3500] = zi[1500]
    y = torch.cat([torch.full((300,), 100), torch.full((200,), 1500), torch.randint(0, N, (Q - 500,), generator=torch.Generator().manual_seed(4))])
    q, _ = queries(Q, y)
    qc, zic, ztc = q.cuda(), zi.cuda(), zt.cuda()
    for alpha, beta in ((0.5, 12.0), (1.0, 3.0), (0.0, 5.0)):
        p64, tau = reference(q, zi, zt, alpha, beta)
        outs = {}
        with ops.classify_fused():
            for passes in (0, 1):
                with ops.classify_panel_passes(passes):
                    ops.classify_panel_stats(reset=True)
                    outs[passes] = ops.classify(qc, zic, ztc, alpha, beta, want_p=False, want_argmax=True)[1].cpu()
                    npan, nsecond = ops.classify_panel_stats()
                    if passes == 0:                                  # (the three copies of class 100 are candidates of different tiles: the proof may stand)
                        assert npan == math.ceil(Q / 256)
                        observe(f"duplicates alpha={alpha}: fraction of panels through the second pass", nsecond / npan, 1.0)
        with ops.classify_two_stage():
            outs["two"] = ops.classify(qc, zic, ztc, alpha, beta, want_p=False, want_argmax=True)[1].cpu()
        for route, am in outs.items():
            tag = f"duplicates alpha={alpha} route={route}"
            check_argmax(am, p64, tau, N, tag)
            assert not bool(((am == 3000) | (am == 4095)).any()), f"{tag}: a duplicate of class 100 won a tie"
            assert int((am[:300] == 100).sum()) > 250, tag
            if alpha == 1.0:
                assert not bool((am == 3500).any()), f"{tag}: the visual duplicate of class 1500 won a tie at alpha = 1"
                assert int((am[300:500] == 1500).sum()) > 150, tag
        assert torch.equal(outs[0], outs[1]), alpha


def test_default_routing_at_the_envelope_edge(ops):
    """Q = 20 000, N = 4096, D = 512 without forcing anything: the product's own routing takes the fused row panels (79 panels, the last one of 32 rows)."""
    Q, N, D, alpha, beta = 20000, 4096, 512, 0.5, 12.0
    zi, zt, queries = banks(N, D, seed=20)
    q, _ = queries(Q)
    assert ops.classify_route(Q, N, D, alpha, beta) == PANELS
    ops.classify_panel_stats(reset=True)
    am = ops.classify(q.cuda(), zi.cuda(), zt.cuda(), alpha, beta, want_p=False, want_argmax=True)[1].cpu()
    npan, nsecond = ops.classify_panel_stats()
    assert npan == math.ceil(Q / 256)
    observe("default routing Q=20000 N=4096: fraction of panels through the second pass", nsecond / npan, 1.0)
    assert int(am.min()) >= 0 and int(am.max()) < N
    rows = panel_rows(Q)
    p64, tau = reference(q[rows], zi, zt, alpha, beta)
    check_argmax(am[rows], p64, tau, N, "default routing Q=20000 N=4096 D=512")
    ops.release_workspaces()


def test_route_depends_on_the_shape_only(ops):
    """`classify_route` names the route a call takes whatever ran on the stream before: a large classification first grows the stream's cached workspace; a
    call at a shape whose two-stage workspace is smaller than the row panels' scratch (Q = 600, N = 4096, D = 4096) then takes the route `classify_route`
    reports — counted by the panel counters — and the same route after the cache is dropped."""
    Q, N, D, alpha, beta = 600, 4096, 4096, 0.5, 12.0
    zi, zt, queries = banks(N, D, seed=600)
    q, _ = queries(Q)
    qc, zic, ztc = q.cuda(), zi.cuda(), zt.cuda()
    p64, tau = reference(q, zi, zt, alpha, beta)
    zb, zbt, _ = banks(4096, 512, seed=1, device="cuda")
    big = nrm(torch.randn(20000, 512, device="cuda"), dim=-1).half()
    for fused in (True, False):
        seen = []
        for prime in (True, False):
            if prime:
                ops.classify(big, zb, zbt, alpha, beta, want_p=False, want_argmax=True)           # grows the cached buffer to ~0.66 GB
            else:
                ops.release_workspaces()
            with (ops.classify_fused() if fused else ops.classify_two_stage()):
                route = ops.classify_route(Q, N, D, alpha, beta)
                ops.classify_panel_stats(reset=True)
                am = ops.classify(qc, zic, ztc, alpha, beta, want_p=False, want_argmax=True)[1].cpu()
                npan = ops.classify_panel_stats()[0]
            assert npan == (math.ceil(Q / 256) if route == PANELS else 0), (fused, prime, route, npan)
            check_argmax(am, p64, tau, N, f"route test fused={fused}")
            seen.append((route, am))
        assert seen[0][0] == seen[1][0] and torch.equal(seen[0][1], seen[1][1]), (fused, seen[0][0], seen[1][0])
        assert seen[0][0] == (PANELS if fused else TWO)
    ops.release_workspaces()


# ---------------------------------------------------------------- refusals just past the envelope ------------------------------------
def _refusal_call(ops, case):
    """The call of one refusal case (arguments built on the device, nothing computed)."""
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    unit = lambda R, D: nrm(torch.randn(R, D, device="cuda", generator=g), dim=-1).half()
    d = torch.zeros(64, 4160, dtype=torch.float32, device="cuda")
    if case.startswith("classify "):
        _, shape, mode = case.split(" ", 2)
        Q, N = (int(v) for v in shape.split("/"))
        qq, z1, z2 = unit(Q, 512), unit(N, 512), unit(N, 512)
        cm = {"default": None, "fused": ops.classify_fused, "two-stage": ops.classify_two_stage}[mode]

        def call():
            if cm is None:
                return ops.classify(qq, z1, z2, 0.5, 12.0, want_p=False, want_argmax=True)
            with cm():
                return ops.classify(qq, z1, z2, 0.5, 12.0, want_p=False, want_argmax=True)
        return call
    return {
        "fuse_probs N=4097": lambda: ops.fuse_probs(d, d, 4097, 0.5, 12.0, want_p=True, want_argmax=True),
        "hp_sweep N=4097": lambda: ops.hp_sweep(d, d, 4097, torch.zeros(64, dtype=torch.int32, device="cuda"), [0.5], [12.0]),
        "sqdist D=4160": lambda: ops.sqdist(h(8, 4160), h(8, 4160), h(8, 4160)),
        "sqdist D=4100": lambda: ops.sqdist(h(8, 4100), h(8, 4100), h(8, 4100)),
        "classify_panel_distances N=4097": lambda: ops.classify_panel_distances(unit(300, 512), unit(4097, 512), unit(4097, 512)),
        "proto_backward K=33": lambda: ops.proto_backward(h(4 * 33, 256), torch.zeros(4, 256, device="cuda"), 4, 33, True, True),
        "proto_backward D=3136": lambda: ops.proto_backward(h(4 * 2, 3136), torch.zeros(4, 3136, device="cuda"), 4, 2, True, True),
        "layernorm_backward D=2056": lambda: ops.layernorm_backward(h(8, 2056), h(2056), h(8, 2056)),
        "l2norm_rows D=4104": lambda: ops.l2norm_rows(h(8, 4104)),
        "adapter_fc D=4352": lambda: ops.adapter_fc(h(8, 4352), h(1088, 4352), h(1088), h(1088), h(4352, 1088), h(4352), h(4352)),
    }[case]


REFUSALS = [f"classify {s} {m}" for s in ("600/4097", "20000/5000") for m in ("default", "fused", "two-stage")] + [
    "fuse_probs N=4097", "hp_sweep N=4097", "sqdist D=4160", "sqdist D=4100", "classify_panel_distances N=4097", "proto_backward K=33",
    "proto_backward D=3136", "layernorm_backward D=2056", "l2norm_rows D=4104", "adapter_fc D=4352"]


@pytest.fixture(scope="module")
def valid_case():
    """A valid classification (Q = 300, N = 1025, D = 512) with its float64 reference, for after a refusal."""
    zi, zt, queries = banks(1025, 512, seed=9)
    q, _ = queries(300)
    p64, tau = reference(q, zi, zt, 0.5, 12.0)
    return q.cuda(), zi.cuda(), zt.cuda(), p64, tau


@pytest.mark.parametrize("case", REFUSALS)
def test_refusal_past_the_envelope(ops, valid_case, case):
    """Every entry point refuses a shape just past its limit with a PclipError and a message — never a result (N > 4096 on every classification route,
    the Q = 20 000 / N = 5 000 call included) — and the stream stays usable: a valid classification after the refusal is checked against float64."""
    from proto_clip_amd import PclipError
    call = _refusal_call(ops, case)
    with pytest.raises(PclipError) as exc:
        call()
    msg = str(exc.value)
    assert "failed (rc=" in msg and len(msg.split(": ", 1)[1]) > 10 and not msg.endswith(": ?"), (case, msg)
    torch.cuda.synchronize()
    q, zi, zt, p64, tau = valid_case
    with ops.classify_two_stage():
        p, am, _, _ = ops.classify(q, zi, zt, 0.5, 12.0, want_p=True, want_argmax=True)
    check_p(p, p64, tau, "valid call after a refusal")
    check_argmax(am, p64, tau, 1025, "valid call after a refusal")
    ops.release_workspaces()


# ---------------------------------------------------------------- prototypes, row normalisation, adapter at the envelope --------------
def proto64(mem16, N, K, per_shot=True):
    """The prototype chain (main.py:399-402) in float64 with the reference's fp16 rounding points: per-shot r16(x / r16(|x|)), r16(mean), then
    (fp16 output) r16(z / r16(|z|)) and (fp32 output) z / |z|."""
    D = mem16.shape[1]
    x = mem16.double().view(N, K, D)
    if per_shot:
        x = (x / x.pow(2).sum(-1, keepdim=True).sqrt().half().double()).half().double()
    z = (x.sum(1) / K).half().double()
    n = z.pow(2).sum(-1, keepdim=True).sqrt()
    return (z / n.half().double()).half(), z / n


@pytest.mark.parametrize("N,K,D", [(4096, 32, 512), (64, 32, 4096)])
@pytest.mark.parametrize("per_shot", [True, False])
def test_proto_build_envelope_vs_float64(ops, N, K, D, per_shot):
    g = torch.Generator().manual_seed(N + K + D)
    mem = (torch.randn(N * K, D, generator=g) * 0.7).half()
    out16, sq = ops.proto_build(mem.cuda(), N, K, per_shot_norm=per_shot, want_sq=True)
    out32 = ops.proto_build(mem.cuda(), N, K, per_shot_norm=per_shot, fp32_out=True).cpu()
    ref16, ref32 = [], []
    for c in range(0, N, 256):
        a, b = proto64(mem[c * K:(c + min(256, N - c)) * K], min(256, N - c), K, per_shot)
        ref16.append(a)
        ref32.append(b)
    ref16, ref32 = torch.cat(ref16), torch.cat(ref32)
    tag = f"proto_build N={N} K={K} D={D} per_shot={per_shot}"
    u = observe(f"{tag}: fp16 prototypes vs float64 (fp16 ulps)", ulp_diff(out16, ref16), 2.0)
    assert u <= 2
    e = observe(f"{tag}: fp32 prototypes vs float64 (abs)", (out32.double() - ref32).abs().max().item(), 3e-4)
    assert e <= 3e-4
    assert (out32.double() - ref32).abs().gt(2e-5).float().mean().item() < 1e-3
    torch.testing.assert_close(sq.cpu().double(), out16.cpu().double().pow(2).sum(-1), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("D", [8, 4088, 4096])
def test_l2norm_rows_envelope_vs_float64(ops, D):
    R = 333
    x = (torch.randn(R, D, generator=torch.Generator().manual_seed(D)) * 3).half()
    y, sq = ops.l2norm_rows(x.cuda(), want_sq=True)
    x64 = x.double()
    ref = (x64 / x64.pow(2).sum(-1, keepdim=True).sqrt().half().double()).half()
    u = observe(f"l2norm_rows D={D} vs float64 (fp16 ulps)", ulp_diff(y, ref), 1.0)
    assert u <= 1
    assert (y.cpu() == ref).float().mean().item() > 0.995
    torch.testing.assert_close(sq.cpu().double(), y.cpu().double().pow(2).sum(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ops.row_sqnorm(x.cuda()).cpu().double(), x64.pow(2).sum(-1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("D", [2048, 4096])
def test_adapter_fc_envelope_vs_oracle(ops, D):
    from proto_clip_amd.model import Adapter_FC
    torch.manual_seed(D)
    ad = Adapter_FC(D, dtype=torch.half)
    with torch.no_grad():
        for n_, p_ in ad.named_parameters():
            if "fc.1" in n_ or "fc.3" in n_:
                p_.add_((torch.randn(p_.shape) * 0.1).half())
    x = po.l2norm_rows(torch.randn(300, D, generator=torch.Generator().manual_seed(D + 1)).half())
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    ref = po.adapter_fc(x, sd)
    with torch.no_grad():
        adc = ad.cuda()
        y = adc(x.cuda())
        y1 = adc(x[7:8].cuda())
    assert_adapter_close(y, ref, tag=f"adapter fc D={D} vs oracle")
    assert torch.equal(y1[0], y[7])
