"""GPU parity proper: the HIP path (through the C ABI / ctypes) against the ORACLE on seeded inputs, and
against the committed reference outputs (tests/golden).  Bit-exact for index work (argmax, counts);
floating point within the tolerances BASELINE.json's north_star states (p within 1e-3, top-1 identical),
prototypes within 2 fp16 ulp."""
import os

import numpy as np
import pytest
import torch

from conftest import (FEWSHOT, adapter_sd, assert_adapter_close, assert_grid_close, fewshot_inputs, golden, observe, ulp_diff)
from oracle import proto_oracle as po
from proto_clip_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def dev(t):
    return t.cuda()


# ---------------------------------------------------------------- row reductions -------------------
@pytest.mark.parametrize("R,D", [(1, 512), (5, 64), (1000, 512), (333, 768), (4097, 1024), (7, 2048), (65, 4096)])
def test_l2norm_rows(ops, R, D):
    x = torch.from_numpy(synth.normal((R, D), 3, 0)).half() * 3
    y, sq = ops.l2norm_rows(dev(x), want_sq=True)
    ref = po.l2norm_rows(x)
    assert ulp_diff(y, ref) <= 1
    assert (y.cpu() == ref).float().mean().item() > 0.995       # 1-ulp flips of the fp16 norm are rare
    torch.testing.assert_close(sq.cpu(), y.cpu().float().pow(2).sum(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ops.row_sqnorm(dev(x)).cpu(), x.float().pow(2).sum(-1), rtol=1e-5, atol=1e-5)


def test_l2norm_inplace_and_empty(ops):
    x = dev(torch.from_numpy(synth.normal((9, 512), 4, 0)).half())
    ref = po.l2norm_rows(x.cpu())
    out = ops.l2norm_rows(x, out=x)
    assert out.data_ptr() == x.data_ptr() and ulp_diff(x, ref) <= 1
    e = ops.l2norm_rows(torch.empty(0, 512, dtype=torch.float16, device="cuda"))
    assert e.shape == (0, 512)


@pytest.mark.parametrize("N,K,D", [(10, 16, 512), (100, 1, 1024), (198, 16, 768), (1000, 16, 512), (37, 3, 512), (5, 7, 64), (300, 32, 512), (16, 32, 4096)])
@pytest.mark.parametrize("per_shot", [True, False])
def test_proto_build(ops, N, K, D, per_shot):
    mem = (torch.from_numpy(synth.normal((N * K, D), 5, 1)).float() * 0.7).half()
    ref16 = po.proto_build(mem, N, K, per_shot_norm=per_shot)
    out16, sq = ops.proto_build(dev(mem), N, K, per_shot_norm=per_shot, want_sq=True)
    assert ulp_diff(out16, ref16) <= 2
    torch.testing.assert_close(sq.cpu(), out16.cpu().float().pow(2).sum(-1), rtol=1e-5, atol=1e-6)
    ref32 = po.proto_build(mem, N, K, per_shot_norm=per_shot, fp32=True)
    out32 = ops.proto_build(dev(mem), N, K, per_shot_norm=per_shot, fp32_out=True)
    # z = r16(mean) can differ by one fp16 ulp (norm summation order); the fp32 quotient z/||z|| inherits it
    torch.testing.assert_close(out32.cpu(), ref32, rtol=0, atol=3e-4)
    assert (out32.cpu() - ref32).abs().gt(2e-5).float().mean().item() < 1e-3


@pytest.mark.parametrize("A,R,D", [(10, 160, 512), (2, 24, 64), (3, 1000, 768)])
def test_bank_reduce_and_transpose(ops, A, R, D):
    feats = torch.from_numpy(synth.normal((A, R, D), 6, 2)).half()
    labels = torch.from_numpy(synth.randint(R, 7, 6, 3))
    perm = torch.argsort(labels, stable=True)
    ref = po.bank_reduce(feats, perm)
    out = ops.bank_reduce(dev(feats), perm=dev(perm))
    assert ulp_diff(out, ref) <= 2
    assert ulp_diff(ops.bank_reduce(dev(feats)), po.bank_reduce(feats)) <= 2
    t = ops.transpose(out)
    assert torch.equal(t.cpu(), out.cpu().t())           # byte-exact data movement
    assert torch.equal(ops.transpose(t).cpu(), out.cpu())


def test_transpose_ragged(ops):
    for R, C in [(1, 1), (3, 130), (65, 63), (512, 16000)]:
        x = torch.from_numpy(synth.normal((R, C), 8, 0)).half()
        assert torch.equal(ops.transpose(dev(x)).cpu(), x.t().contiguous())


@pytest.mark.parametrize("W", [1, 2, 8])
def test_partial_sums_and_finalize(ops, W):
    """Sharded prototype mean == single-GPU prototype build, bit for bit."""
    from proto_clip_amd.dist import shard_bounds
    N, K, D = 50, 16, 512
    mem = (torch.from_numpy(synth.normal((N * K, D), 9, 0)).float()).half()
    labels = torch.arange(N).repeat_interleave(K).int()
    sums, counts = [], []
    for r in range(W):
        lo, hi = shard_bounds(N * K, r, W)
        s, c = ops.partial_sums(dev(mem[lo:hi]), dev(labels[lo:hi]), N)
        so, co = po.partial_sums(mem[lo:hi], labels[lo:hi], N)
        torch.testing.assert_close(s.cpu(), so, rtol=0, atol=1e-5)
        assert torch.equal(c.cpu(), co)
        sums.append(s)
        counts.append(c)
    out = ops.proto_finalize(torch.stack(sums), torch.stack(counts))
    single = ops.proto_build(dev(mem), N, K)
    assert torch.equal(out.cpu(), single.cpu())
    assert ulp_diff(out, po.proto_finalize(torch.stack([s.cpu() for s in sums]), torch.stack([c.cpu() for c in counts]))) <= 2


@pytest.mark.parametrize("W", [2, 7, 8])
def test_partial_sums_and_finalize_imagenet_size(ops, W):
    """The same at the C4 size (BASELINE configs[3]: ImageNet 16-shot, N = 1000, K = 16, D = 512): 8 slabs of 2000 rows end on class
    boundaries, 2 slabs of 8000 too, 7 slabs of 2285 / 2286 rows do not (classes straddle ranks) — the rank-ordered combine of the fp32
    class sums must reproduce the single-GPU prototype build bit for bit in all three."""
    from proto_clip_amd.dist import shard_bounds
    N, K, D = 1000, 16, 512
    mem = (torch.from_numpy(synth.normal((N * K, D), 19, 0)).float() * 1.2).half()
    labels = torch.arange(N).repeat_interleave(K).int()
    mem_d, lab_d = dev(mem), dev(labels)
    sums, counts, straddle = [], [], 0
    for r in range(W):
        lo, hi = shard_bounds(N * K, r, W)
        straddle += int(lo % K != 0)
        s, c = ops.partial_sums(mem_d[lo:hi], lab_d[lo:hi], N)
        sums.append(s)
        counts.append(c)
    assert (straddle > 0) == (W == 7)
    assert int(torch.stack(counts).sum().item()) == N * K and torch.equal(torch.stack(counts).sum(0).cpu(), torch.full((N,), K, dtype=torch.int32))
    out = ops.proto_finalize(torch.stack(sums), torch.stack(counts))
    single = ops.proto_build(mem_d, N, K)
    assert torch.equal(out.cpu(), single.cpu())


def test_partial_sums_missing_classes(ops):
    N, D = 12, 64
    mem = torch.from_numpy(synth.normal((20, D), 10, 0)).half()
    labels = torch.tensor([2] * 5 + [3] * 1 + [9] * 14).int()
    s, c = ops.partial_sums(dev(mem), dev(labels), N)
    so, co = po.partial_sums(mem, labels, N)
    assert torch.equal(c.cpu(), co)
    torch.testing.assert_close(s.cpu(), so, rtol=0, atol=1e-5)
    assert s.cpu()[[0, 1, 4, 11]].abs().max().item() == 0


# ---------------------------------------------------------------- classification ---------------------
@pytest.mark.parametrize("Q,N,D", [(1, 10, 512), (300, 10, 512), (129, 1000, 512), (2048, 1000, 512), (32, 198, 768),
                                   (257, 100, 1024), (1000, 37, 64), (128, 128, 128)])
def test_sqdist(ops, Q, N, D):
    q = po.l2norm_rows(torch.from_numpy(synth.normal((Q, D), 11, 0)).half())
    zi = po.l2norm_rows(torch.from_numpy(synth.normal((N, D), 11, 1)).half())
    zt = (po.l2norm_rows(torch.from_numpy(synth.normal((N, D), 11, 2)).half()).float() * 1.45).half()   # non-unit bank
    d2i, d2t, ldd = ops.sqdist(dev(q), dev(zi), dev(zt))
    assert (d2i.cpu()[:, :N] - po.sqdist(q, zi)).abs().max().item() <= 2e-6 * 4
    assert (d2t.cpu()[:, :N] - po.sqdist(q, zt)).abs().max().item() <= 2e-5
    # asymmetric operands: a transposed / permuted accumulator layout cannot pass
    q2 = (torch.arange(Q * D).reshape(Q, D).float() % 13 / 16).half()
    z2 = (torch.arange(N * D).reshape(N, D).float() % 7 / 8).half()
    d, _, _ = ops.sqdist(dev(q2), dev(z2))
    torch.testing.assert_close(d.cpu()[:, :N], po.sqdist(q2, z2), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("name", list(FEWSHOT))
def test_P_against_reference_fixture(ops, name):
    """utils.py:225-244 on the reference's own prototypes and adapted queries (first 64 rows are the
    reference's; the rest come from the oracle's adapter, which only feeds rows not compared to p_rows)."""
    from proto_clip_amd.utils import P, P_argmax, P_topk
    g = golden("fewshot_" + name)
    split, emb_v, emb_t, cfg = fewshot_inputs(name)
    sd = adapter_sd(g)
    ad = (lambda x: po.adapter_fc(x, sd)) if cfg["adapter"] == "fc" else (lambda x: po.adapter_conv(x, sd, cfg["adapter"]))
    zq = torch.cat([torch.from_numpy(g["adapted_test_norm"]), po.l2norm_rows(ad(split.test_features))[64:]])
    zi, zt = torch.from_numpy(g["test_proto_img"]), torch.from_numpy(g["test_proto_txt"])
    p = P(dev(zq), dev(zi), dev(zt), cfg["alpha"], cfg["beta"]).cpu()
    p_or = po.P(zq, zi, zt, cfg["alpha"], cfg["beta"])
    assert (p - p_or).abs().max().item() <= 1e-5                       # vs oracle: summation order only
    idx = torch.from_numpy(g["p_rows_idx"]).long()
    sel = idx < 64                                                        # rows whose inputs are the reference's own
    assert (p[idx][sel] - torch.from_numpy(g["p_rows"])[sel]).abs().max().item() <= 1e-3
    am = P_argmax(dev(zq), dev(zi), dev(zt), cfg["alpha"], cfg["beta"]).cpu()
    assert torch.equal(am, p_or.max(1)[1])                                # top-1 identical to the oracle
    assert torch.equal(am[:64], torch.from_numpy(g["fixed_argmax"]).long()[:64])   # ... and to the reference
    k = min(5, split.N)
    tv, ti = P_topk(dev(zq), dev(zi), dev(zt), cfg["alpha"], cfg["beta"], k)
    rv, ri = p_or.topk(k, dim=1)
    torch.testing.assert_close(tv.cpu(), rv, rtol=0, atol=1e-5)
    assert (ti.cpu() == ri).float().mean().item() > 0.999                 # ties between ~0 probabilities may reorder


@pytest.mark.parametrize("Q,N,D", [(1, 1, 32), (15, 3, 64), (16, 10, 512), (8100, 10, 512), (333, 16, 512), (100, 17, 768),
                                   (1000, 32, 1024), (77, 31, 96), (500, 37, 512), (260, 47, 512), (129, 64, 512), (50, 64, 1024)])
@pytest.mark.parametrize("alpha,beta", [(0.5, 12.0), (1.0, 0.7), (0.0, 3.0), (0.3, -2.0)])
def test_classify_single_launch_small_N(ops, Q, N, D, alpha, beta):
    """N <= 64 with the mid-N kernel off: the one-launch kernel (classify_small_kernel: banks in LDS, a wave per 16 queries) for N <= 32,
    the two stages beyond: same results as the two-stage path (distance rows + softmax pass) up to fp32
    summation order, p within 1e-5 of the oracle, top-1 / top-k identical wherever the runner-up is not within 1e-6."""
    with ops.classify_mid(0):                                                      # this is classify_small's test: the mid-N kernel (which takes N > 16 by default) is tested below
        q = po.l2norm_rows(torch.from_numpy(synth.normal((Q, D), 21, 0)).half())
        zi = po.l2norm_rows(torch.from_numpy(synth.normal((N, D), 21, 1)).half() + 0.3 * q[:1])
        zt = (po.l2norm_rows(torch.from_numpy(synth.normal((N, D), 21, 2)).half()).float() * 1.2).half()    # non-unit bank
        k = min(3, N)
        p, am, tp, ti = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=True, want_argmax=True, topk=k)
        p_or = po.P(q, zi, zt, alpha, beta)
        assert (p.cpu() - p_or).abs().max().item() <= 1e-5
        top2 = p_or.topk(min(2, N), dim=1)[0]
        clear = (top2[:, 0] - top2[:, -1] > 1e-6) if N > 1 else torch.ones(Q, dtype=torch.bool)
        assert torch.equal(am.cpu().long()[clear], p_or.max(1)[1][clear])
        assert torch.equal(p.cpu().max(1)[1], am.cpu().long())                        # argmax of the p it wrote: first index on ties
        rv, ri = p_or.topk(k, dim=1)
        torch.testing.assert_close(tp.cpu(), rv, rtol=0, atol=1e-5)
        assert torch.equal(tp.cpu()[:, 0], p.cpu().max(1)[0])
        assert (ti.cpu() == ri).float().mean().item() > 0.99
        _, am_only, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
        assert torch.equal(am_only, am)
        if D % 64 == 0:                                                                # the two-stage entry points need D % 64 == 0
            d2i, d2t, _ = ops.sqdist(dev(q), dev(zi), dev(zt))
            p2, am2, _, _ = ops.fuse_probs(d2i, d2t, N, alpha, beta, want_p=True, want_argmax=True)
            assert (p - p2).abs().max().item() <= 2e-6
            assert (am != am2).sum().item() <= (~clear).sum().item()


@pytest.mark.parametrize("Q,N,D", [(2465, 100, 1024), (666, 198, 768), (32, 198, 768), (3669, 37, 512), (1692, 47, 512), (17, 33, 128), (5000, 256, 512), (100, 129, 384),
                                   (1, 40, 512), (4100, 64, 2048), (9000, 101, 512), (300, 250, 1024), (77, 160, 640), (1000, 70, 1280)])
@pytest.mark.parametrize("alpha,beta", [(0.5, 12.0), (0.8, 9.0), (0.2, 12.0), (1.0, 0.7), (0.0, 3.0), (0.3, -2.0)])
def test_classify_one_launch_mid_N(ops, Q, N, D, alpha, beta):
    """32 < N <= 256 (Caltech-101, FewSOL-198, OxfordPets, DTD ...): the one-launch kernel (csrc/pclip_classify_mid.hip — eight waves per group of 16
    queries, both banks streamed once, norms in-kernel) against the oracle's P (utils.py:225-244; p within 1e-5, argmax wherever the oracle's top two are 1e-6 apart)
    and against the two stages it replaces (p within 2e-6, argmax up to the same ties); p-only, argmax-only and both; the argmax is the first maximum of the p it wrote."""
    q = po.l2norm_rows(torch.from_numpy(synth.normal((Q, D), 23, 0)).half())
    cen = torch.from_numpy(synth.normal((N, D), 23, 1)).float()
    q = po.l2norm_rows((q.float() + 0.8 * po.l2norm_rows(cen)[torch.arange(Q) % N]).half())           # class structure: a clear winner for most queries
    zi = po.l2norm_rows((cen + 0.3 * torch.from_numpy(synth.normal((N, D), 23, 3)).float()).half())
    zt = (po.l2norm_rows((cen + 0.5 * torch.from_numpy(synth.normal((N, D), 23, 2)).float()).half()).float() * 1.2).half()    # non-unit bank
    with ops.classify_mid(2):
        p, am, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=True, want_argmax=True)
        _, am_only, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
        p_only, _, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=True, want_argmax=False)
    p_or = po.P(q, zi, zt, alpha, beta)
    assert (p.cpu() - p_or).abs().max().item() <= 1e-5
    top2 = p_or.double().topk(2, dim=1)[0]
    clear = top2[:, 0] - top2[:, 1] > 1e-6
    assert torch.equal(am.cpu().long()[clear], p_or.max(1)[1][clear])
    assert torch.equal(p.cpu().max(1)[1], am.cpu().long())
    assert torch.equal(am_only, am) and torch.equal(p_only, p)
    if D % 64 == 0:
        with ops.classify_two_stage():
            p2, am2, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=True, want_argmax=True)
        assert (p - p2).abs().max().item() <= 2e-6
        assert (am != am2).sum().item() <= (~clear).sum().item()
    # top-k requests keep the two stages (the kernel writes p and argmax only)
    if D % 64 == 0:
        k = 3
        _, _, tp, ti = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=False, topk=k)
        rv, ri = p_or.topk(k, dim=1)
        torch.testing.assert_close(tp.cpu(), rv, rtol=0, atol=1e-5)


def test_classify_route_is_reported(ops):
    """ops.classify_route names the kernels a call takes (the routes differ in summation order, callers can ask / pin)."""
    assert ops.classify_route(8100, 10, 512, 1.0, 0.7) == "one launch, small N"
    assert ops.classify_route(2465, 100, 1024, 0.8, 9.0) == "one launch, mid N"
    assert ops.classify_route(666, 198, 768, 0.2, 12.0, want_p=True) == "one launch, mid N"
    assert ops.classify_route(50000, 1000, 512, 0.5, 12.0) == "fused row panels"
    assert ops.classify_route(50000, 1000, 512, 0.5, 12.0, want_p=True) == "two stages"
    assert ops.classify_route(50000, 1000, 512, 1.2, 12.0) == "two stages"                    # alpha outside [0, 1]: the candidate proof does not apply
    assert ops.classify_route(1024, 1000, 512, 0.5, 12.0) == "two stages"                      # the bench's step: too few panels for the fused kernel
    assert ops.classify_route(300, 100, 1024, 0.8, 9.0, topk=5) == "two stages"
    with ops.classify_two_stage():
        assert ops.classify_route(2465, 100, 1024, 0.8, 9.0) == "two stages" and ops.classify_route(50000, 1000, 512, 0.5, 12.0) == "two stages"


def test_classify_mid_default_routing_and_graph_replay(ops):
    """The product's own routing takes the one-launch kernel at the C1 / C5 shapes (no context manager), also inside a captured graph; a second launch on fresh
    queries leaves no state behind."""
    for Q, N, D in ((2465, 100, 1024), (666, 198, 768)):
        g = torch.Generator(device="cuda").manual_seed(N)
        nrm = torch.nn.functional.normalize
        zi = nrm(torch.randn(N, D, device="cuda", generator=g), dim=-1).half()
        zt = nrm(torch.randn(N, D, device="cuda", generator=g), dim=-1).half()
        q = nrm(torch.randn(Q, D, device="cuda", generator=g) + 2 * zi[torch.arange(Q, device="cuda") % N].float(), dim=-1).half()
        _, am, _, _ = ops.classify(q, zi, zt, 0.5, 12.0)
        with ops.classify_two_stage():
            p2, am2, _, _ = ops.classify(q, zi, zt, 0.5, 12.0, want_p=True, want_argmax=True)
        margin = p2.double().topk(2, dim=1)[0]
        diff = (am != am2).nonzero().flatten()
        assert bool(((margin[:, 0] - margin[:, 1])[diff] < 1e-6).all())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.classify(q, zi, zt, 0.5, 12.0)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = ops.classify(q, zi, zt, 0.5, 12.0)[1]
        for rep in range(3):
            q.copy_(nrm(torch.randn(Q, D, device="cuda", generator=g) + 2 * zi[torch.arange(Q, device="cuda") % N].float(), dim=-1).half())
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, ops.classify(q, zi, zt, 0.5, 12.0)[1])


FUSED_SHAPES = [(300, 200, 512), (1000, 1000, 512), (257, 100, 1024), (5000, 198, 768), (33, 40, 128)]


@pytest.mark.parametrize("Q,N,D", FUSED_SHAPES)
def test_classify_fused_row_panels(ops, Q, N, D):
    """The fused large-N classification (csrc/pclip_classify_panel.hip): (i) the distances it forms (sampled tile: query rows 0..255 x classes 0..127, both banks) are the BITS
    pclip_sqdist_f16 writes when it keeps torch.cdist's sqrt round trip, and within one fp32 ulp of them in the product's faster form; (ii) its argmax is the two-stage path's — and where it is not, the two-stage p of that query ties its top
    two classes to 1e-6 (proven per query, not budgeted); (iii) against the oracle's P the same; several (alpha, beta) incl. the configurations' own."""
    classify_fused_row_panels(ops, Q, N, D, exact=False)


@pytest.mark.parametrize("Q,N,D", FUSED_SHAPES)
def test_classify_fused_row_panels_sqrt_round_trip(ops, Q, N, D):
    """test_classify_fused_row_panels with torch.cdist's sqrt round trip kept in the classification itself (classify_panel_exact)."""
    classify_fused_row_panels(ops, Q, N, D, exact=True)


def classify_fused_row_panels(ops, Q, N, D, exact):
    g = torch.Generator().manual_seed(Q + N + D)
    cen = torch.randn(N, D, generator=g)
    nrm = torch.nn.functional.normalize
    zi = nrm(cen + 0.3 * torch.randn(N, D, generator=g), dim=-1).half()
    zt = nrm(cen + 0.5 * torch.randn(N, D, generator=g), dim=-1).half()
    y = torch.randint(0, N, (Q,), generator=g)
    q = nrm(cen[y] + 0.8 * torch.randn(Q, D, generator=g), dim=-1).half()
    d2i, d2t, _ = ops.sqdist(dev(q), dev(zi), dev(zt))
    r, c = min(Q, 256), min(N, 128)
    di, dt = ops.classify_panel_distances(dev(q), dev(zi), dev(zt), exact=True)            # same contraction, same norms, same expression: same bits
    assert torch.equal(di[:r, :c], d2i[:r, :c]) and torch.equal(dt[:r, :c], d2t[:r, :c])
    di, dt = ops.classify_panel_distances(dev(q), dev(zi), dev(zt), exact=False)           # the product's arithmetic: no sqrt -> square round trip, <= 1 ulp away
    for a, b in ((di[:r, :c], d2i[:r, :c]), (dt[:r, :c], d2t[:r, :c])):
        assert int((a.contiguous().view(torch.int32) - b.contiguous().view(torch.int32)).abs().max()) <= 1
    for alpha, beta in ((0.5, 12.0), (0.2, 12.0), (1.0, 0.7), (0.0, 5.0), (0.35, 1.0)):
        with ops.classify_fused(), ops.classify_panel_exact(exact):
            ops.classify_panel_stats(reset=True)
            with ops.classify_panel_passes(0):
                _, am, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
            npan, nsecond = ops.classify_panel_stats()
            # one pass + candidates + proof (default) == always two passes == candidates with the second pass forced: the same argmax, bit for bit
            with ops.classify_panel_passes(1):
                _, am_two, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
            with ops.classify_panel_passes(2):
                _, am_forced, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
            assert torch.equal(am, am_two) and torch.equal(am, am_forced), (alpha, beta, (am != am_two).sum().item(), (am != am_forced).sum().item())
            assert npan == (Q + 255) // 256
            observe(f"fused classify Q={Q} N={N} alpha={alpha} beta={beta}: fraction of panels that needed the second pass", nsecond / npan, 1.0)
        with ops.classify_two_stage():
            _, am2, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)
        p2, _, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=True, want_argmax=False)
        top2 = p2.double().topk(2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).cpu()
        diff = (am != am2).nonzero().flatten().cpu()
        observe(f"fused classify Q={Q} N={N}: two-stage top-2 margin of a query whose fused argmax differs (tie proof)", margin[diff].max().item() if len(diff) else 0.0, 1e-6)
        assert bool((margin[diff] < 1e-6).all()), (alpha, beta, diff.tolist(), margin[diff].tolist())
        assert len(diff) <= max(1, Q // 1000)
        p_or = po.P(q, zi, zt, alpha, beta).double()
        t2 = p_or.topk(2, dim=1).values
        d_or = (am.cpu().long() != p_or.max(1)[1]).nonzero().flatten()
        assert bool(((t2[:, 0] - t2[:, 1])[d_or] < 1e-6).all()), (alpha, beta, d_or.tolist())
        assert int(am.min()) >= 0 and int(am.max()) < N


def test_classify_fused_exact_ties_take_the_lowest_class(ops):
    """Duplicated prototypes (classes 7 == 150 == 151 in both banks, 30 == 31 in the visual bank only) make EXACT ties of p: main.py:190's `.max(1)[1]` on the CPU returns the
    lowest class.  The fused kernel's candidate proof cannot separate a tie (bound == best) and must hand such panels to its second pass; every routing — one pass +
    candidates, always two passes, the two stages — returns the same, lowest, class, and never the duplicate."""
    classify_fused_exact_ties(ops, exact=False)


def test_classify_fused_exact_ties_sqrt_round_trip(ops):
    """The same with torch.cdist's sqrt round trip kept in the fused kernel (classify_panel_exact)."""
    classify_fused_exact_ties(ops, exact=True)


def classify_fused_exact_ties(ops, exact):
    Q, N, D = 700, 200, 512
    g = torch.Generator().manual_seed(5)
    nrm = torch.nn.functional.normalize
    cen = torch.randn(N, D, generator=g)
    zi = nrm(cen + 0.3 * torch.randn(N, D, generator=g), dim=-1).half()
    zt = nrm(cen + 0.5 * torch.randn(N, D, generator=g), dim=-1).half()
    for dup in (150, 151):
        zi[dup] = zi[7]
        zt[dup] = zt[7]
    zi[31] = zi[30]
    y = torch.cat([torch.full((300,), 7), torch.full((100,), 30), torch.randint(0, N, (Q - 400,), generator=g)])
    q = nrm(cen[y] + 0.8 * torch.randn(Q, D, generator=g), dim=-1).half()
    for alpha, beta in ((0.5, 12.0), (1.0, 3.0), (0.0, 5.0)):
        outs = {}
        with ops.classify_fused(), ops.classify_panel_exact(exact):
            for passes in (0, 1):
                with ops.classify_panel_passes(passes):
                    ops.classify_panel_stats(reset=True)
                    outs[passes] = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)[1]
                    if passes == 0:
                        assert ops.classify_panel_stats()[1] > 0, "tied rows must fail the candidate proof"
        with ops.classify_two_stage():
            am2 = ops.classify(dev(q), dev(zi), dev(zt), alpha, beta, want_p=False, want_argmax=True)[1]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], am2), (alpha, beta)
        am = outs[0].cpu()
        assert not bool(((am == 150) | (am == 151)).any()), "a duplicate of class 7 won a tie"
        assert int((am[:300] == 7).sum()) > 250                                    # (the queries drawn around class 7 do land on it)
        if alpha > 0.99:
            assert not bool((am == 31).any()), "the visual duplicate of class 30 won a tie at alpha = 1"
        p_or = po.P(q, zi, zt, alpha, beta)
        assert (am.long() == p_or.max(1)[1]).float().mean().item() > 0.995          # the oracle's fp32 p may break a tie the other way only through rounding


def test_classify_routings_differential_fuzz():
    """tools/fuzz_classify.py: 80 random (shape, alpha, beta, data regime) cases — class-structured, structureless, un-normalised, duplicated prototypes / queries, tiny and
    huge scales, alpha in {0, 1}, beta in {0, ..., 20} — fused row panels (one pass + candidate proof) against the two stages: differences only at proven ties."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_classify.py"), "80", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "unproven differences in 0 cases" in r.stdout


def test_small_class_count_differential_fuzz():
    """tools/fuzz_small.py: 60 random (Q, N <= 256, K, D, alpha, beta, regime) cases — the one-launch classifications (N <= 32: classify_small, 32 < N <= 256:
    classify_mid) against the oracle's P (1e-5, argmax unless the oracle ties) and against the two stages (p within 2e-6)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_small.py"), "60", "11"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "failures in 0" in r.stdout


def test_fuse_probs_edge_cases(ops):
    Q, N = 70, 130
    d2i = torch.from_numpy(synth.uniform(Q * N, 12, 0).reshape(Q, N)).float() * 4
    d2t = torch.from_numpy(synth.uniform(Q * N, 12, 1).reshape(Q, N)).float() * 4
    d2i[3, 5] = d2i[3, 77] = 0.0          # exact tie: lowest index wins (main.py:190 on CPU)
    d2t[3, 5] = d2t[3, 77] = 0.0
    ldd = ops.padded_ld(N)
    pad = lambda d: torch.nn.functional.pad(d, (0, ldd - N), value=float("nan"))   # padding must never be read
    for alpha, beta in [(0.0, 1.0), (1.0, 0.1), (0.5, 20.0), (0.3, 0.0), (0.7, 5.5)]:
        p, am, _, _ = ops.fuse_probs(dev(pad(d2i)), dev(pad(d2t)), N, alpha, beta, want_p=True, want_argmax=True)
        ref = po.P_from_dists(d2i, d2t, alpha, beta)
        torch.testing.assert_close(p.cpu(), ref, rtol=1e-5, atol=1e-7)
        assert torch.equal(am.cpu().long(), ref.max(1)[1]) or beta == 0.0
        torch.testing.assert_close(p.cpu().sum(1), torch.ones(Q), rtol=0, atol=1e-5)
    assert am is not None and ops.fuse_probs(dev(pad(d2i)), dev(pad(d2t)), N, 0.5, 20.0, want_p=False, want_argmax=True)[1][3].item() == 5


@pytest.mark.parametrize("name", ["C2", "C6", "C5", "C1", "C3"])
def test_zero_shot_grid_equals_reference_up_to_proven_ties(ops, name, tmp_path):
    """main.py:172-199: all three [319, 3] grids of the zero-shot search against the reference's.  Identical — except at grid points where a query's two best
    classes TIE in the reference's own fp32 arithmetic: there the fp32 summation order of the 512-long dot products decides (MFMA tile vs CPU BLAS).  That is
    PROVEN, not budgeted (VERDICT r4 #4b): for every grid point that differs, every query whose GPU top-1 differs from the oracle's (the reference's P restated,
    pinned to it) must have a reference top-2 margin below 1e-6 in p, and the accuracy difference must be exactly what those queries account for."""
    from proto_clip_amd import main as pm
    g = golden("fewshot_" + name)
    split, emb_v, emb_t, cfg = fewshot_inputs(name)
    N, K = split.N, split.K
    rows = dev(split.visual_memory_keys.t().contiguous())
    zi = ops.proto_build(rows, N, K, per_shot_norm=False)
    zt = ops.l2norm_rows(dev(split.textual_memory_bank.t().contiguous()))
    assert ulp_diff(zi, torch.from_numpy(g["zs_proto_img"])) <= 2 and ulp_diff(zt, torch.from_numpy(g["zs_proto_txt"])) <= 2
    al, bl = pm.hp_grid()
    train_y = split.visual_memory_values.argmax(1)
    for s, f, y in (("val", split.val_features, split.val_labels), ("test", split.test_features, split.test_labels),
                    ("train", split.visual_memory_keys.t().contiguous(), train_y)):
        fq = ops.l2norm_rows(dev(f))
        got = pm.grid_accuracy(fq, dev(y), zi, zt, al, bl)
        ref = g["zs_" + s]
        np.testing.assert_array_equal(got[:, :2], ref[:, :2])
        differ = np.nonzero(got[:, 2] != ref[:, 2])[0]
        assert len(differ) <= 0.02 * len(ref), (name, s, len(differ))             # a handful of grid points at most (observed: <= 4 per split)
        for gi in differ:
            alpha, beta = float(ref[gi, 0]), float(ref[gi, 1])
            p_or = po.P(fq.cpu(), zi.cpu(), zt.cpu(), alpha, beta).double()
            am_or = p_or.max(1)[1]
            top2 = p_or.topk(2, dim=1).values
            margin = top2[:, 0] - top2[:, 1]
            ties = margin < 1e-6                                                   # queries whose two best classes tie in the reference's own fp32 arithmetic
            # the grid kernel's count differs from the reference's by no more than there are such queries ...
            dq = round(abs(float(got[gi, 2]) - float(ref[gi, 2])) * len(y), 2)   # the grids hold accuracies as float32 fractions: whole queries up to rounding
            observe(f"zero-shot grid {name}/{s}: queries of difference at a differing grid point over the number of proven ties there", dq, float(ties.sum()))
            assert int(ties.sum()) >= 1 and dq <= float(ties.sum()) + 0.01, (name, s, alpha, beta, dq, int(ties.sum()))
            # ... the oracle's count IS the reference's up to the same queries, and either classification path of the library differs from the oracle on tied queries only
            acc_or = (am_or == y.long()).double().mean().item()
            assert abs(acc_or - float(ref[gi, 2])) * len(y) <= float(ties.sum()) + 0.01
            for two_stage in (False, True):
                if two_stage:
                    with ops.classify_two_stage():
                        _, am, _, _ = ops.classify(fq, zi, zt, alpha, beta, want_p=False, want_argmax=True)
                else:
                    with ops.classify_fused():
                        _, am, _, _ = ops.classify(fq, zi, zt, alpha, beta, want_p=False, want_argmax=True)
                flipped = (am.cpu().long() != am_or)
                assert bool((ties | ~flipped).all()), (name, s, alpha, beta, two_stage, flipped.nonzero().flatten().tolist(), margin[flipped].tolist())
        assert_grid_close(got[:, 2], ref[:, 2], len(y), exact=True, tag=f"zero-shot grid {name}")


# ---------------------------------------------------------------- adapters -----------------------------
@pytest.mark.parametrize("name", list(FEWSHOT))
def test_adapter_against_reference_fixture(ops, name):
    from proto_clip_amd.model import Adapter, Adapter_FC
    g = golden("fewshot_" + name)
    split, emb_v, emb_t, cfg = fewshot_inputs(name)
    sd = adapter_sd(g)
    ad = Adapter_FC(split.D, dtype=torch.half) if cfg["adapter"] == "fc" else Adapter(split.D, cfg["adapter"], dtype=torch.half)
    ad.load_state_dict(sd)
    ad = ad.cuda()
    assert list(ad.state_dict().keys()) == list(sd.keys())            # reference key names and order
    with torch.no_grad():
        val_raw = ad(dev(split.val_features[:64]))
        test_n = ad(dev(split.test_features[:64]), l2norm_out=True)
        test_2 = ops.l2norm_rows(ad(dev(split.test_features[:64])))
    assert_adapter_close(val_raw, torch.from_numpy(g["adapted_val_raw"]), tag=f"adapter {cfg['adapter']} vs reference rows ({name})")
    assert_adapter_close(test_n, torch.from_numpy(g["adapted_test_norm"]), tag=f"adapter {cfg['adapter']} vs reference rows ({name})")
    assert torch.equal(test_n.cpu(), test_2.cpu())                      # fused normalise == separate kernel
    y_tape = ad(dev(split.val_features[:4]))                            # grad mode, trainable parameters: an autograd node (tests/test_gpu_autograd.py)
    assert y_tape.requires_grad
    assert_adapter_close(y_tape.detach(), val_raw[:4], tag=f"adapter {cfg['adapter']} under autograd vs its no_grad kernel ({name})")


# conv-3x runs on the matrix pipe (pclip_adapter.hip adapter_conv3x_mfma_kernel<NT>, NT = ceil(s^2 / 64)): D = 200 (s = 15: a partial last tile),
# 576 (s = 24: nine full 64-pixel groups, the last two-workgroups-per-CU size), 577 (s = 25: NT = 10, one workgroup per CU), 768 (NT = 13), 1024 (NT = 16)
@pytest.mark.parametrize("kind,D", [("conv-3x", 512), ("conv-2x", 768), ("conv-3x", 1024), ("fc", 1024), ("conv-2x", 100), ("conv-3x", 200), ("conv-3x", 576),
                                    ("conv-3x", 577), ("conv-3x", 768), ("conv-3x", 64)])
def test_adapter_random_weights_vs_oracle(ops, kind, D):
    from proto_clip_amd.model import Adapter, Adapter_FC
    if kind == "fc" and D % 256:
        pytest.skip("fc kernel needs D/4 % 64 == 0")
    torch.manual_seed(3)
    ad = Adapter_FC(D, dtype=torch.half) if kind == "fc" else Adapter(D, kind, dtype=torch.half)
    with torch.no_grad():
        for n_, p_ in ad.named_parameters():
            if "bn" in n_ or "fc.1" in n_ or "fc.3" in n_:
                p_.add_((torch.randn(p_.shape) * 0.1).half())
    x = po.l2norm_rows(torch.from_numpy(synth.normal((300, D), 13, 0)).half())
    sd = {k: v.clone() for k, v in ad.state_dict().items()}
    ref = po.adapter_fc(x, sd) if kind == "fc" else po.adapter_conv(x, sd, kind)
    with torch.no_grad():
        adc = ad.cuda()
        y = adc(dev(x))
        y1 = adc(dev(x[7:8]))                                 # persistent kernel: a row alone (grid of one workgroup) == the row in the batch
    assert_adapter_close(y, ref, tag=f"adapter {kind} D={D} vs oracle")
    assert torch.equal(y1[0], y[7])


# ---------------------------------------------------------------- whole test pass ----------------------
@pytest.mark.parametrize("name", ["C2", "C6", "C5", "C1", "C3"])
def test_run_proto_clip_test_pass(ops, name, tmp_path, monkeypatch):
    """reference main.py:383-455 through proto_clip_amd.main.run_proto_clip, against the reference's grids."""
    import os
    import types
    from proto_clip_amd import main as pm
    from proto_clip_amd.utils import get_model_dir_root
    g = golden("fewshot_" + name)
    split, emb_v, emb_t, cfg = fewshot_inputs(name)
    cfg["cache_dir"] = str(tmp_path / "caches")
    model_dir = f"{get_model_dir_root(cfg)}/alpha-beta/{cfg['alpha']}-{cfg['beta']}"
    os.makedirs(model_dir, exist_ok=True)
    prefix = f"{model_dir}/best_lr_{cfg['lr']}_aug_{cfg['augment_epoch']}_epochs_{cfg['train_epoch']}"
    torch.save(torch.nn.Parameter(emb_v), prefix + "_v.pt")               # reference file layout (main.py:367-369)
    torch.save(torch.nn.Parameter(emb_t), prefix + "_t.pt")
    torch.save(adapter_sd(g), prefix + "_a.pt")
    out = pm.run_proto_clip(cfg, dev(split.visual_memory_keys), dev(split.visual_memory_values), dev(split.val_features),
                            dev(split.val_labels), dev(split.test_features), dev(split.test_labels),
                            dev(split.textual_memory_bank), types.SimpleNamespace(dtype=torch.float16), None)
    n = dict(val=len(split.val_labels), test=len(split.test_labels), train=split.N * split.K)
    for s in ("val", "test", "train"):
        assert_grid_close(out["zero_shot"][s][:, 2], g["zs_" + s][:, 2], n[s], exact=True, tag=f"run_proto_clip zero-shot grid {name}")
        assert_grid_close(out["test"][s][:, 2], g["test_" + s][:, 2], n[s], tag=f"run_proto_clip test grid {name} [{cfg['adapter']}]")
    dq = observe(f"run_proto_clip fixed-(alpha,beta) accuracy {name}: queries differing", abs(out["test"]["fixed_acc"] - float(g["fixed_acc"])) * n["test"], 0.5)
    assert dq <= 0.5            # observed: identical on all five configurations (round 1 allowed one query)
    # the pickles the reference writes (main.py:205-207) exist with the reference's names
    for s in ("val", "test", "train"):
        assert os.path.exists(os.path.join(get_model_dir_root(cfg), f"zero_shot_hp_search_{s}_ViT_B_16_K_{cfg['shots']}.pkl"))


# ---------------------------------------------------------------- error behaviour ----------------------
def test_loud_failures(ops):
    from proto_clip_amd import PclipError
    with pytest.raises(PclipError):
        ops.l2norm_rows(torch.zeros(4, 512, dtype=torch.float16))          # CPU tensor: no fallback
    with pytest.raises(PclipError):
        ops.l2norm_rows(torch.zeros(4, 510, dtype=torch.float16, device="cuda"))
    with pytest.raises(PclipError):
        ops.sqdist(torch.zeros(4, 72, dtype=torch.float16, device="cuda"), torch.zeros(3, 72, dtype=torch.float16, device="cuda"))
    from proto_clip_amd.utils import P
    with pytest.raises(PclipError):
        P(torch.zeros(4, 512, device="cuda").double(), torch.zeros(3, 512, device="cuda"), torch.zeros(3, 512, device="cuda"), 0.5, 1.0)


@pytest.mark.parametrize("Q,N,D", [(70, 10, 512), (257, 198, 768), (33, 1000, 100), (1, 1, 8)])
def test_P_fp32_operands_training_path(ops, Q, N, D):
    """main.py:262-281: fp32 prototypes (train variant of the prototype kernel) and fp32 queries through P."""
    from proto_clip_amd.utils import P
    q = torch.nn.functional.normalize(torch.from_numpy(synth.normal((Q, D), 31, 0)).float(), dim=-1)
    zi = torch.nn.functional.normalize(torch.from_numpy(synth.normal((N, D), 31, 1)).float(), dim=-1)
    zt = torch.nn.functional.normalize(torch.from_numpy(synth.normal((N, D), 31, 2)).float(), dim=-1) * 1.3
    d2i, d2t, _ = ops.sqdist_f32(dev(q), dev(zi), dev(zt))
    assert (d2i.cpu()[:, :N] - po.sqdist(q, zi)).abs().max().item() <= 5e-6
    assert (d2t.cpu()[:, :N] - po.sqdist(q, zt)).abs().max().item() <= 1e-5
    p = P(dev(q), dev(zi), dev(zt), 0.4, 9.0).cpu()
    ref = po.P(q, zi, zt, 0.4, 9.0)
    assert (p - ref).abs().max().item() <= 1e-5
    assert torch.equal(p.max(1)[1], ref.max(1)[1]) or N == 1
    pm = P(dev(q), dev(zi.half()), dev(zt), 0.4, 9.0).cpu()             # mixed dtypes promote like .float()
    assert (pm - po.P(q, zi.half(), zt, 0.4, 9.0)).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- full-size properties -----------------
def test_full_size_properties_C3(ops):
    """BASELINE sizes (Q=50 000, N=1000, D=512): size-independent properties instead of an oracle run."""
    split = synth.make_split(1000, 16, 512, 64, 50000, seed=1, sigma=4.0, sigma_text=2.4)
    rows = dev(split.visual_memory_keys.t().contiguous())
    zi, zi_sq = ops.proto_build(rows, 1000, 16, want_sq=True)
    zt = ops.l2norm_rows(dev(split.textual_memory_bank.t().contiguous()))
    assert (zi_sq - 1).abs().max().item() < 2e-3                          # unit norm in fp16
    acc_lo, acc_hi = 0.2, 0.99
    assert torch.equal(ops.l2norm_rows(zt), zt) or ulp_diff(ops.l2norm_rows(zt), zt) <= 1   # idempotent up to 1 ulp
    q = dev(split.test_features)
    d2i, d2t, ldd = ops.sqdist(q, zi, zt)
    # distance to self: a prototype queried against its own bank sits on the diagonal at ~0 and is the row min
    dself, _, _ = ops.sqdist(zi, zi)
    assert dself[:, :1000].diagonal().abs().max().item() < 1e-3
    assert torch.equal(dself[:, :1000].argmin(1).cpu(), torch.arange(1000))
    # permutation equivariance over queries and over classes
    perm = torch.randperm(50000, generator=torch.Generator().manual_seed(0)).cuda()
    d2p, _, _ = ops.sqdist(q[perm], zi)
    assert torch.equal(d2p[:, :1000], d2i[perm][:, :1000])
    p, am, _, _ = ops.fuse_probs(d2i, d2t, 1000, 0.5, 12.0, want_p=True, want_argmax=True)
    assert (p.sum(1) - 1).abs().max().item() < 1e-5 and p.min().item() >= 0
    assert torch.equal(am.long(), p.max(1)[1])
    # the sweep's count at (alpha, beta) equals the argmax path's count; alpha=1 ignores the text bank
    al, bl = np.array([0.0, 0.5, 1.0]), np.array([0.7, 12.0])
    cnt = ops.hp_sweep(d2i, d2t, 1000, dev(split.test_labels), al, bl).cpu()
    assert cnt[1, 1].item() == (am.long().cpu() == split.test_labels).sum().item()
    _, am1, _, _ = ops.fuse_probs(d2i, None, 1000, 1.0, 12.0, want_p=False, want_argmax=True)
    assert cnt[2, 1].item() == (am1.long().cpu() == split.test_labels).sum().item()
    assert acc_lo < cnt[1, 1].item() / 50000 < acc_hi, cnt


@pytest.mark.parametrize("structured", [True, False])
def test_full_size_default_routing_C3(ops, structured):
    """The DEFAULT routing of `ops.classify(argmax)` at BASELINE's full size (Q = 50 000, N = 1000, D = 512; utils.py:225-244 + main.py:190): the fused row-panel kernel
    (csrc/pclip_classify_panel.hip) — asserted through its panel counters, 196 panels — against (i) the two-stage path's argmax up to PROVEN ties (two-stage top-2
    margin < 1e-6 for every query that differs), (ii) the oracle's P on 2048 sampled rows, same rule.  structured: the few-shot split (one pass + candidate proof on every
    panel); not structured: queries unrelated to any class (flat p) — the candidate proof fails and the second pass runs on the full grid of panels."""
    Q, N, D, alpha, beta = 50000, 1000, 512, 0.5, 12.0
    split = synth.make_split(N, 16, D, 64, Q, seed=1, sigma=4.0, sigma_text=2.4)
    zi = ops.proto_build(dev(split.visual_memory_keys.t().contiguous()), N, 16)
    zt = ops.l2norm_rows(dev(split.textual_memory_bank.t().contiguous()))
    if structured:
        q = dev(split.test_features)
    else:
        g = torch.Generator().manual_seed(11)
        q = dev(torch.nn.functional.normalize(torch.randn(Q, D, generator=g), dim=-1).half())
    ops.classify_panel_stats(reset=True)
    _, am, _, _ = ops.classify(q, zi, zt, alpha, beta, want_p=False, want_argmax=True)         # no context manager: the product's own routing
    npan, nsecond, ntiles2 = ops.classify_panel_stats(tiles=True)
    assert npan == (Q + 255) // 256, f"the fused row-panel kernel did not take the call ({npan} panels counted)"
    # a second pass walks only the class tiles that hold a bound its panel could not beat (round 6): on this split fewer than all eight; and the merge of its
    # result with the candidates is the argmax of the WHOLE second pass (mode 2: forced over every tile) and of two passes without candidates (mode 1), bit for bit
    observe(f"C3 full size, {'structured' if structured else 'structureless'}: class tiles walked per second pass (of 8)", ntiles2 / max(nsecond, 1), 8.0)
    assert nsecond <= ntiles2 <= 8 * nsecond
    for mode in (1, 2):
        with ops.classify_panel_passes(mode):
            _, am_m, _, _ = ops.classify(q, zi, zt, alpha, beta, want_p=False, want_argmax=True)
        assert torch.equal(am, am_m), (mode, int((am != am_m).sum()))
    observe(f"C3 full size, default routing, {'structured' if structured else 'structureless'} queries: fraction of panels that needed the second pass", nsecond / npan, 1.0)
    if structured:
        assert nsecond < npan // 2               # class-structured rows: most panels are proven by their candidates (this split: 23 of 196 are not)
    else:
        assert nsecond > npan // 4               # flat rows: the second pass is what is being tested (82 - 156 of 196 panels by seed)
    with ops.classify_two_stage():
        ops.classify_panel_stats(reset=True)
        _, am2, _, _ = ops.classify(q, zi, zt, alpha, beta, want_p=False, want_argmax=True)
        assert ops.classify_panel_stats()[0] == 0
    p2, _, _, _ = ops.classify(q, zi, zt, alpha, beta, want_p=True, want_argmax=False)
    assert torch.equal(am2.long(), p2.max(1)[1])
    top2 = p2.topk(2, dim=1).values.double()
    margin = (top2[:, 0] - top2[:, 1]).cpu()
    diff = (am != am2).nonzero().flatten().cpu()
    observe(f"C3 full size ({'structured' if structured else 'structureless'}): two-stage top-2 margin of a query whose fused argmax differs (tie proof)",
            margin[diff].max().item() if len(diff) else 0.0, 1e-6)
    assert bool((margin[diff] < 1e-6).all()), (diff.tolist()[:10], margin[diff].tolist()[:10])
    assert len(diff) <= Q // 1000
    idx = torch.randperm(Q, generator=torch.Generator().manual_seed(3))[:2048]
    p_or = po.P(q[idx.cuda()].cpu(), zi.cpu(), zt.cpu(), alpha, beta).double()
    t2 = p_or.topk(2, dim=1).values
    d_or = (am[idx.cuda()].cpu().long() != p_or.max(1)[1]).nonzero().flatten()
    assert bool(((t2[:, 0] - t2[:, 1])[d_or] < 1e-6).all()), d_or.tolist()[:10]
    assert (p2[idx.cuda()].cpu().double() - p_or).abs().max().item() <= 1e-5
    if structured:
        acc = (am.cpu().long() == split.test_labels).float().mean().item()
        assert 0.2 < acc < 0.99


def test_classify_alpha_outside_unit_interval_takes_two_stages(ops):
    """The fused kernel's one-pass candidate proof bounds a class through p's monotonicity in BOTH distances, which needs alpha >= 0 and 1 - alpha >= 0:
    a user-supplied --alpha outside [0, 1] must not reach it.  Such calls route to the two stages even when the fused kernel is forced; results = the oracle's."""
    Q, N, D = 600, 200, 512
    g = torch.Generator().manual_seed(2)
    nrm = torch.nn.functional.normalize
    cen = torch.randn(N, D, generator=g)
    zi, zt = nrm(cen + 0.3 * torch.randn(N, D, generator=g), dim=-1).half(), nrm(cen + 0.5 * torch.randn(N, D, generator=g), dim=-1).half()
    q = nrm(cen[torch.randint(0, N, (Q,), generator=g)] + 0.8 * torch.randn(Q, D, generator=g), dim=-1).half()
    for alpha in (1.2, -0.1):
        with ops.classify_fused():
            ops.classify_panel_stats(reset=True)
            _, am, _, _ = ops.classify(dev(q), dev(zi), dev(zt), alpha, 3.0, want_p=False, want_argmax=True)
            assert ops.classify_panel_stats()[0] == 0
        p_or = po.P(q, zi, zt, alpha, 3.0).double()
        t2 = p_or.topk(2, dim=1).values
        d_or = (am.cpu().long() != p_or.max(1)[1]).nonzero().flatten()
        assert bool(((t2[:, 0] - t2[:, 1])[d_or] < 1e-6).all())


def test_sqdist_big_tile_path_matches_small_tile_path_and_oracle():
    """Problems with >= 3 x #CU tiles of 256x256 (ImageNet-sized grids) run the persistent big-tile kernel; a row subset of
    the same problem runs the one-shot 128x128 kernel.  Same MFMA k-order -> the distances must agree bit for bit; a sample is
    also checked against the oracle.  Q is a multiple of 4 but not of 256 (ragged last tile), N = 1000 (ragged last column tile)."""
    from proto_clip_amd import ops
    Q, N, D = 25004, 1000, 128
    g = torch.Generator(device="cuda").manual_seed(12)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=g), dim=-1).half()
    zi = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=-1).half()
    zt = (torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=-1) * 1.2).half()
    d2i, d2t, ldd = ops.sqdist(q, zi, zt)
    for lo, hi in ((0, 700), (12345, 12345 + 513), (Q - 300, Q)):
        si, st, _ = ops.sqdist(q[lo:hi].contiguous(), zi, zt)
        assert torch.equal(d2i[lo:hi, :N], si[:, :N]) and torch.equal(d2t[lo:hi, :N], st[:, :N]), (lo, hi)
    ref_i, ref_t = po.sqdist(q[Q - 64:].cpu(), zi.cpu()), po.sqdist(q[Q - 64:].cpu(), zt.cpu())
    torch.testing.assert_close(d2i[Q - 64:, :N].cpu(), ref_i, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(d2t[Q - 64:, :N].cpu(), ref_t, rtol=1e-5, atol=2e-5)
