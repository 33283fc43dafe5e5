"""CLIP towers on the GPU against the reference's own encoder outputs
(tests/golden/encoder_*.npz: fp16-weight model = the reference's GPU precision, and the fp32 CPU model)
and against the oracle.  Tolerances are stated relative to the fp16<->fp32 gap of the reference itself."""
import numpy as np
import os
import pytest
import torch

from conftest import ENCODERS, golden, observe, ulp_diff
from oracle import clip_oracle, proto_oracle as po
from proto_clip_amd import synth
from proto_clip_amd.clip.model import build_model, random_state_dict

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


# ---------------------------------------------------------------- building blocks --------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (1, 64, 64), (197, 2304, 768), (1000, 512, 3072), (257, 100, 128), (4096, 768, 768),
                                   (3000, 2304, 128), (2560, 1024, 64), (5000, 768, 192)])
def test_gemm_epilogues(ops, M, N, K):
    a = (torch.from_numpy(synth.normal((M, K), 21, 0)).float() * 0.5).half()
    w = (torch.from_numpy(synth.normal((N, K), 21, 1)).float() * K ** -0.5).half()
    bias = (torch.from_numpy(synth.normal((N,), 21, 2)).float() * 0.1).half()
    res = torch.from_numpy(synth.normal((M, N), 21, 3)).half()
    acc = a.float() @ w.float().t()
    y = ops.gemm(a.cuda(), w.cuda()).cpu()
    assert ulp_diff(y, acc.half()) <= 1
    y = ops.gemm(a.cuda(), w.cuda(), bias.cuda()).cpu()
    assert ulp_diff(y, (acc + bias.float()).half()) <= 1
    h = po.r16(acc + bias.float())
    gelu = po.r16(h * po.r16(torch.sigmoid(po.r16(1.702 * h))))
    y = ops.gemm(a.cuda(), w.cuda(), bias.cuda(), act=1).cpu()
    assert ulp_diff(y, gelu.half()) <= 3                    # three fp16 elementwise roundings on a 1-ulp-different h
    y = ops.gemm(a.cuda(), w.cuda(), bias.cuda(), residual=res.cuda()).cpu()
    assert ulp_diff(y, (res.float() + h).half()) <= 2      # 1-ulp h (summation order) re-rounded after the add
    # asymmetric integer-valued operands: exact, catches any transposed / permuted fragment layout
    ai = (torch.arange(M * K).reshape(M, K) % 5 - 2).half()
    wi = (torch.arange(N * K).reshape(N, K) % 3 - 1).half()
    assert torch.equal(ops.gemm(ai.cuda(), wi.cuda()).cpu().float(), (ai.float() @ wi.float().t()).half().float())


@pytest.mark.parametrize("M,N,K", [(50432, 768, 64), (50432, 3072, 64), (70001, 512, 64), (201728, 768, 64)])
def test_gemm_row_split(ops, M, N, K):
    """Shapes whose last round of persistent tiles is mostly empty are dispatched as two launches (full rounds with the
    large tile + the remaining rows with a smaller one): every output row must come out exactly as from one launch.
    Integer-valued operands make the product exact, so any dropped / doubled / misplaced row block shows."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a = torch.randint(-3, 4, (M, K), device="cuda", generator=g).half()
    w = torch.randint(-2, 3, (N, K), device="cuda", generator=g).half()
    bias = torch.randint(-4, 5, (N,), device="cuda", generator=g).half()
    n0 = ops._lib.load().pclip_gemm_kernel_launches()
    y = ops.gemm(a, w, bias)
    launches = ops._lib.load().pclip_gemm_kernel_launches() - n0
    ref = torch.empty_like(y)
    for i in range(0, M, 16384):                            # fp32 reference in slabs (bounded memory)
        ref[i:i + 16384] = (a[i:i + 16384].float() @ w.float().t() + bias.float()).half()
    assert torch.equal(y, ref)
    if ops._lib.load().pclip_device_cus() == 256 and (M, N) == (50432, 768):
        assert launches == 2                                # 2 full rounds of 256x256 tiles + the last 6912 rows


def test_gemm_banded_tile_order_is_bit_identical(ops):
    """PCLIP_GEMM_BAND (tile order in bands of column tiles): a pure speed knob — same bits, including a
    ragged last band (12 column tiles in bands of 5) and a partial last row block.  The orders are taken per call through the test entry
    (the process reads PCLIP_GEMM_BAND / _REV once, at its first GEMM: setting them here compared the default order with itself) and every
    launch's order is asserted from the entry's report."""
    M, N, K = 70001, 3072, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(M, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    b = torch.randn(N, device="cuda", generator=g).half()
    ref, plain = ops.gemm_route(a, w, b, act=1, band=0, rev=0)                # column tiles fastest, ascending
    assert plain and all((l["rev"], l["band"]) == (False, 0) for l in plain), plain
    assert torch.equal(ops.gemm(a, w, b, act=1), ref)                        # the product entry: the same bits in its own order
    for band in (6, 5, 1):
        got, launches = ops.gemm_route(a, w, b, act=1, band=band, rev=0)
        assert [(l["family"], l["rows"]) for l in launches] == [(l["family"], l["rows"]) for l in plain]
        assert all((l["rev"], l["band"]) == (False, band) for l in launches), launches        # every launch has >= 12 column tiles: all of them banded
        assert torch.equal(got, ref), band
    for rev in (0, 1, 2):                                   # PCLIP_GEMM_REV: tiles in descending order (default 2: launches with K <= 1024) — same bits
        got, launches = ops.gemm_route(a, w, b, act=1, rev=rev)
        assert all(l["rev"] == (rev != 0) and l["band"] == 0 for l in launches), launches
        assert torch.equal(got, ref), rev


def test_gemm_quickgelu_pipelined_epilogue_is_the_two_slab_epilogue(ops):
    """256 x 256 tiles stage a QuickGELU epilogue as a four-slab pipeline (pgemm::epilogue_pipe: slab k = 32-row block k of every wave, two halves of the
    staging buffer, the activation arithmetic of slab k + 1 under the stores of slab k); every other tile shape keeps the two-slab pass.  Same bits —
    on a shape with a partial last row block — and within 3 fp16 ulp of the fp32 reference with the reference's three roundings."""
    M, N, K = 70001, 3072, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(M, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    b = torch.randn(N, device="cuda", generator=g).half()
    big, l_big = ops.gemm_route(a, w, b, act=1, cfg=2, use4w=0)      # 256 x 256 tiles on eight waves (forced per call: PCLIP_GEMM_CFG is read once per process)
    small, l_small = ops.gemm_route(a, w, b, act=1, cfg=0)           # 128 x 128 tiles: epilogue_f16
    assert [(l["family"], l["rows"]) for l in l_big] == [("cfg2", M)] and [(l["family"], l["rows"]) for l in l_small] == [("cfg0", M)], (l_big, l_small)
    assert torch.equal(small, big)
    rows = torch.cat([torch.arange(0, 600), torch.arange(M - 300, M)]).cuda()
    h = po.r16((a[rows].float() @ w.float().t() + b.float()).cpu())
    ref = po.r16(h * po.r16(torch.sigmoid(po.r16(1.702 * h))))
    assert ulp_diff(big[rows].cpu(), ref.half()) <= 3


@pytest.mark.parametrize("M,N,K,act", [(197, 768, 3072, 0), (1, 768, 3072, 0), (8, 3072, 3072, 1), (32, 512, 3072, 1), (257, 1024, 4096, 0),
                                        (130, 64, 2048, 1), (64, 1024, 4096, 0)])
def test_gemm_splitk_small_M(ops, M, N, K, act):
    """Serving shapes through pclip_gemm_splitk_f16 (K cut into slices, a second launch adds the slabs in slice order):
    within 1 fp16 ulp of the fp32 reference like the unsplit kernel (3 with QuickGELU), deterministic (bit-identical runs),
    rows beyond M untouched, the slicing independent of M (a row alone == the row in the batch),
    and EXACT on integer-valued operands (any dropped / doubled slice or misplaced register group shows)."""
    lib = ops._lib.load()
    need = lib.pclip_gemm_splitk_workspace(M, N, K)
    assert need > 0, "shape should be a split-K shape on this device"
    a = (torch.from_numpy(synth.normal((M, K), 31, 0)).float() * 0.5).half().cuda()
    w = (torch.from_numpy(synth.normal((N, K), 31, 1)).float() * K ** -0.5).half().cuda()
    bias = (torch.from_numpy(synth.normal((N,), 31, 2)).float() * 0.1).half().cuda()
    h = po.r16(a.float().cpu() @ w.float().cpu().t() + bias.float().cpu())
    ref = po.r16(h * po.r16(torch.sigmoid(po.r16(1.702 * h)))) if act else h
    out = torch.full((M + 3, N), 7.0, dtype=torch.float16, device="cuda")
    with ops.low_latency():
        y = ops.gemm(a, w, bias, act, None, out[:M])
        assert ulp_diff(y.cpu(), ref.half()) <= (3 if act else 1)
        assert (out[M:] == 7.0).all()
        y2 = ops.gemm(a, w, bias, act)
        assert torch.equal(y2, y)
        r = M // 2
        y1 = ops.gemm(a[r:r + 1].contiguous(), w, bias, act)
        if lib.pclip_gemm_splitk_workspace(1, N, K):
            assert torch.equal(y1[0], y[r])
        ai = (torch.arange(M * K, device="cuda").reshape(M, K) % 5 - 2).half()
        wi = (torch.arange(N * K, device="cuda").reshape(N, K) % 3 - 1).half()
        assert torch.equal(ops.gemm(ai, wi).float(), (ai.float() @ wi.float().t()).half().float())
    unsplit = ops.gemm(a, w, bias, act)                     # outside the context: the persistent kernel
    assert ulp_diff(unsplit.cpu(), y.cpu()) <= (3 if act else 1)


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 576, 1024])
@pytest.mark.parametrize("M,N", [(1, 64), (127, 192), (128, 64), (129, 128), (300, 320), (1000, 64)])
def test_gemm_ring_kernel_every_k_tile_count(ops, M, N, K):
    """Calls with no more 128x64 tiles than CUs run the ring kernel (4 K-tile slots, 3 LDS-DMA stages in flight, counted waits):
    every prologue / steady-state / tail combination of the ring (1 .. 16 K-tiles) and every row-tile edge, EXACT on
    integer-valued operands (a tile consumed before it landed, or overwritten while still being read, cannot pass), and equal
    to the fp32 reference with bias / QuickGELU within the usual fp16 rounding."""
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    a = torch.randint(-3, 4, (M, K), device="cuda", generator=g).half()
    w = torch.randint(-2, 3, (N, K), device="cuda", generator=g).half()
    bias = torch.randint(-4, 5, (N,), device="cuda", generator=g).half()
    ref = a.float() @ w.float().t() + bias.float()
    for _ in range(3):                                      # repeated: a race would not fail every time
        assert torch.equal(ops.gemm(a, w, bias).float(), ref.half().float())
    assert torch.equal(ops.gemm(a, w).float(), (a.float() @ w.float().t()).half().float())
    af = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    wf = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    h = po.r16((af.float() @ wf.float().t() + bias.float()).cpu())
    gelu = po.r16(h * po.r16(torch.sigmoid(po.r16(1.702 * h))))
    assert ulp_diff(ops.gemm(af, wf, bias, act=1).cpu(), gelu.half()) <= 3


@pytest.mark.parametrize("M,N,K", [(256, 256, 192), (1000, 512, 256), (777, 768, 320), (40000, 768, 448), (33333, 1024, 832), (20000, 2304, 768),
                                   (20000, 768, 3072), (70001, 768, 768)])
def test_gemm4w_is_the_eight_wave_kernel_bit_for_bit(ops, M, N, K):
    """The four-wave kernel with the hand-scheduled asm K-loop (csrc/pclip_gemm4w.hip) against the eight-wave persistent kernel it replaces
    for 256 x 256 tiles: torch.equal for every epilogue — same MFMA, operand roles and k order per accumulator.  The shapes cover every tail variant of the
    loop (3, 4, 5 K-tiles ...), every phase of the five-slot ring across consecutive output tiles of a workgroup (2 nt mod 5 with several tiles per workgroup),
    ragged last row tiles and a guard row behind the output; the RACE-STRESS build of the same loop (variant 1: one wave paused in front of every counted wait
    and barrier) must produce the same bits again, and an exact integer-valued product pins both to the mathematical result."""
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + K)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    res = torch.randn(M, N, device="cuda", generator=g).half()
    for act, b, r in ((0, None, None), (0, bias, None), (1, bias, None), (0, bias, res)):
        with ops.gemm_eight_wave():
            ref = ops.gemm(a, w, b, act, r)
        for var in (0, 1):                                                     # the product loop and its race-stress build
            out = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.float16)
            ops.gemm4w(a, w, b, act, r, out[:M], var)
            assert torch.equal(out[:M], ref), (act, var)
            assert bool((out[M] == 7.0).all())
        assert torch.equal(ops.gemm(a, w, b, act, r), ref)                     # the default route (four-wave for these shapes)
    ai = torch.randint(-3, 4, (M, K), device="cuda", generator=g).half()
    wi = torch.randint(-2, 3, (N, K), device="cuda", generator=g).half()
    bi = torch.randint(-4, 5, (N,), device="cuda", generator=g).half()
    exact = (ai[:4096].float() @ wi.float().t() + bi.float()).half()
    for var in (0, 1):
        for _ in range(2):
            assert torch.equal(ops.gemm4w(ai, wi, bi, var=var)[:4096], exact)


def test_gemm4w_instrument_builds(ops):
    """The two instrument builds of the four-wave kernel run the product K-loop with different C++ around it.  The stamped build (var 8) must give the product's
    bits and leave the guard row alone while it fills its stamp buffer; the no-epilogue build (var 6) must store nothing.  One shape that reaches what they can
    get wrong: 524 tiles over at most 256 workgroups (consecutive tiles per workgroup), 13 K-tiles (the ring phase changes from tile to tile), a ragged last
    row tile."""
    M, N, K = 33333, 1024, 832
    g = torch.Generator(device="cuda").manual_seed(M + 3 * N + K)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    res = torch.randn(M, N, device="cuda", generator=g).half()
    lib = ops._lib.load()
    stamps = torch.zeros(260, dtype=torch.int32, device="cuda")
    ops._lib.check(lib.pclip_gemm4w_stamp_buffer(ops._lib.ptr(stamps)), "pclip_gemm4w_stamp_buffer")
    try:
        for act, b, r in ((0, bias, None), (1, bias, None), (0, bias, res)):
            ref = ops.gemm4w(a, w, b, act, r)
            stamps.zero_()
            out = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.float16)
            ops.gemm4w(a, w, b, act, r, out[:M], 8)
            assert torch.equal(out[:M], ref), act
            assert bool((out[M] == 7.0).all())
            assert bool((stamps[:64] != 0).any()), act                         # the stamp block of workgroup 0 / wave 0
            out.fill_(7.0)
            ops.gemm4w(a, w, b, act, r, out[:M], 6)
            assert bool((out == 7.0).all()), act
    finally:
        torch.cuda.synchronize()
        lib.pclip_gemm4w_stamp_buffer(None)


@pytest.mark.parametrize("M,N,K,band", [(20000, 2304, 768, 3), (20000, 3072, 768, 6), (33333, 1024, 832, 2), (70001, 768, 768, 1), (9000, 3072, 768, 5)])
def test_gemm4w_band_tile_order_is_bit_identical(ops, M, N, K, band, monkeypatch):
    """PCLIP_GEMM_BAND's tile order in the four-wave kernel (bands of `band` column tiles, row panels fastest inside a band): a permutation of the
    same output tiles — every epilogue gives the bits of the default order, ragged last band and ragged last row tile included."""
    g = torch.Generator(device="cuda").manual_seed(M + N + K + band)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    res = torch.randn(M, N, device="cuda", generator=g).half()
    for act, b, r in ((0, bias, None), (1, bias, None), (0, bias, res)):
        monkeypatch.delenv("PCLIP_GEMM4W_BAND", raising=False)
        ref = ops.gemm4w(a, w, b, act, r)
        monkeypatch.setenv("PCLIP_GEMM4W_BAND", str(band))                     # (read per call by the test entry pclip_gemm4w_var_f16)
        out = torch.full((M + 1, N), 7.0, device="cuda", dtype=torch.float16)
        ops.gemm4w(a, w, b, act, r, out[:M])
        assert torch.equal(out[:M], ref), (act, band)
        assert bool((out[M] == 7.0).all())
    monkeypatch.delenv("PCLIP_GEMM4W_BAND", raising=False)


def test_gemm4w_in_place_residual_and_refusals(ops):
    a = torch.randn(5000, 768, device="cuda").half()
    w = (torch.randn(768, 768, device="cuda") * 0.03).half()
    bias = torch.randn(768, device="cuda").half()
    x = torch.randn(5000, 768, device="cuda").half()
    with ops.gemm_eight_wave():
        ref = ops.gemm(a, w, bias, 0, x)
    y = x.clone()
    ops.gemm4w(a, w, bias, 0, y, y)                                            # residual stream updated in place
    assert torch.equal(y, ref)
    # strided operands and output (views of wider buffers), a single row, fewer rows than a tile
    g = torch.Generator(device="cuda").manual_seed(1)
    A2 = (torch.randn(3000, 2 * 768, device="cuda", generator=g) * 0.5).half()
    W2 = (torch.randn(512, 3 * 768, device="cuda", generator=g) * 0.03).half()
    O2 = torch.full((3000, 1024), 7.0, device="cuda", dtype=torch.float16)
    b2 = torch.randn(512, device="cuda", generator=g).half()
    av, wv, ov = A2[:, 768:], W2[:, 768:2 * 768], O2[:, 256:768]
    with ops.gemm_eight_wave():
        ref2 = ops.gemm(av.contiguous(), wv.contiguous(), b2, 1)
    ops.gemm4w(av, wv, b2, 1, None, ov)
    assert torch.equal(ov, ref2) and bool((O2[:, :256] == 7.0).all()) and bool((O2[:, 768:] == 7.0).all())
    for m in (1, 100):
        with ops.gemm_eight_wave():
            r3 = ops.gemm(a[:m].contiguous(), w, bias, 0)
        assert torch.equal(ops.gemm4w(a[:m].contiguous(), w, bias, 0), r3)
    from proto_clip_amd._lib import PclipError
    for bad in (lambda: ops.gemm4w(a[:, :128], w[:, :128]),                     # K < 192
                lambda: ops.gemm4w(a, w[:700]),                                # N % 256
                lambda: ops.gemm4w(a, w, None, 0, x),                          # residual without bias
                lambda: ops.gemm4w(a, w, bias, 1, x)):                         # residual with an activation
        with pytest.raises(PclipError):
            bad()


def test_gemm_splitk_refusals(ops):
    lib = ops._lib.load()
    assert lib.pclip_gemm_splitk_workspace(50432, 768, 768) == 0        # plenty of tiles: the persistent kernel's shape
    assert lib.pclip_gemm_splitk_workspace(197, 768, 128) == 0          # K too short to cut
    assert lib.pclip_gemm_splitk_workspace(197, 768, 768) == 0          # 12 K-tiles: the ring kernel's one launch is faster
    assert lib.pclip_gemm_splitk_workspace(197, 100, 768) == 0          # N % 64 != 0
    assert lib.pclip_gemm_splitk_workspace(197, 3072, 768) == 0         # slab traffic would cost more than the K-loop it saves
    a = torch.zeros(197, 768, dtype=torch.float16, device="cuda")
    w = torch.zeros(768, 768, dtype=torch.float16, device="cuda")
    out = torch.empty(197, 768, dtype=torch.float16, device="cuda")
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    from proto_clip_amd._lib import ptr, stream
    a = torch.zeros(197, 3072, dtype=torch.float16, device="cuda")
    w = torch.zeros(768, 3072, dtype=torch.float16, device="cuda")
    rc = lib.pclip_gemm_splitk_f16(ptr(a), 3072, ptr(w), 3072, ptr(out), 768, 197, 768, 3072, None, 0, ptr(ws), ws.numel(), stream())
    assert rc == -3 and b"workspace" in lib.pclip_last_error()
    rc = lib.pclip_gemm_splitk_f16(ptr(a), 768, ptr(w), 768, ptr(out), 768, 50432, 768, 768, None, 0, ptr(ws), ws.numel(), stream())
    assert rc == -1


@pytest.mark.parametrize("R,D", [(7, 64), (500, 768), (197, 1024), (3, 512)])
def test_layernorm(ops, R, D):
    x = (torch.from_numpy(synth.normal((R, D), 22, 0)).float() * 2 + 0.3).half()
    g = 1 + 0.1 * torch.from_numpy(synth.normal((D,), 22, 1)).float()
    b = 0.1 * torch.from_numpy(synth.normal((D,), 22, 2)).float()
    y = ops.layernorm(x.cuda(), g.cuda(), b.cuda()).cpu()
    ref = torch.nn.functional.layer_norm(x.float(), [D], g, b).half()
    assert ulp_diff(y, ref) <= 1
    # strided rows (ln_post on the CLS rows only, clip/model.py:233)
    if R < 3:
        return
    xs = x[: (R // 3) * 3].reshape(-1, 3 * D).contiguous()
    y2 = ops.layernorm(xs.cuda().view(-1, D), g.cuda(), b.cuda(), rows=xs.shape[0], ld=3 * D).cpu()
    assert ulp_diff(y2, torch.nn.functional.layer_norm(xs[:, :D].float(), [D], g, b).half()) <= 1


@pytest.mark.parametrize("D", [512, 768, 1024])
def test_layernorm_big_batch_kernel_is_the_small_batch_kernel(ops, D):
    """More than 65 536 rows take layernorm_pf_kernel (next row's loads ahead of the reductions), fewer layernorm_kernel: same source
    arithmetic, but two compilations — hipcc's contraction / SLP choices can move a rounding between them (seen once while editing a
    shared header: one fp16 ulp on 0.4 % of the rows).  "A row alone == the row in a batch" needs them equal bit for bit."""
    for R in (70000, 140001):       # 140 001 rows: the whole-batch form (>= 16 rows per workgroup of the 32-per-CU grid) with gamma / beta from the workgroup's LDS copy
        g = torch.Generator(device="cuda").manual_seed(D)
        x = (torch.randn(R, D, device="cuda", generator=g) * 1.3 + 0.2).half()
        gam, bet = 1 + 0.3 * torch.randn(D, device="cuda", generator=g), 0.2 * torch.randn(D, device="cuda", generator=g)
        big = ops.layernorm(x, gam, bet)
        small = torch.cat([ops.layernorm(x[i:i + 5000].contiguous(), gam, bet) for i in range(0, R, 5000)])
        assert torch.equal(big, small), R


@pytest.mark.parametrize("R,D,L", [(12, 64, 3), (394, 768, 197), (77, 512, 7)])
def test_add_layernorm(ops, R, D, L):
    """Residual add fused into the LayerNorm: x += delta (fp16 rounding), y = LN(x); also the strided CLS-row form."""
    x = (torch.from_numpy(synth.normal((R, D), 25, 0)).float() * 2).half()
    dl = torch.from_numpy(synth.normal((R, D), 25, 1)).half()
    g = 1 + 0.1 * torch.from_numpy(synth.normal((D,), 25, 2)).float()
    b = 0.1 * torch.from_numpy(synth.normal((D,), 25, 3)).float()
    xs = (x.float() + dl.float()).half()
    ref = torch.nn.functional.layer_norm(xs.float(), [D], g, b).half()
    xd = x.cuda()
    y = ops.add_layernorm(xd, dl.cuda(), g.cuda(), b.cuda())
    assert torch.equal(xd.cpu(), xs)                       # x updated in place, bit exact
    assert ulp_diff(y, ref) <= 1
    xd = x.cuda()
    y2 = ops.add_layernorm(xd, dl.cuda(), g.cuda(), b.cuda(), update_x=False, rows=R // L, ld=L * D)
    assert torch.equal(xd.cpu(), x)                        # untouched
    assert ulp_diff(y2, ref[::L][: R // L]) <= 1


# L = 129 .. 256 (five to eight query tiles) take the query-first / split-barrier form of the eight-wave kernel, whose counted wait depends on how many K / V
# pieces a wave stages (2 - 4 by L): every class of it is here (129 / 160: 2 | 3 pieces, 161 / 192: 3, 193 / 197 / 224: 3 | 4, 225 / 256: 4), causal too
@pytest.mark.parametrize("B,L,H,causal", [(2, 50, 2, False), (3, 197, 12, False), (2, 77, 8, True), (1, 257, 16, False),
                                          (4, 26, 3, False), (1, 1, 1, False), (2, 33, 1, True), (2, 129, 2, False), (3, 160, 3, False), (2, 161, 2, True),
                                          (2, 192, 4, False), (2, 193, 2, False), (3, 224, 2, True), (2, 225, 3, False), (2, 256, 2, False), (5, 200, 7, False),
                                          (3, 32, 2, False), (2, 64, 3, False), (2, 65, 2, False), (3, 100, 2, False), (2, 128, 4, False)])      # the query-first four-wave form: 1 - 4 tiles
def test_attention(ops, B, L, H, causal):
    W = H * 64
    qkv = (torch.from_numpy(synth.normal((B, L, 3 * W), 23, 0)).float() * 1.5).half()
    out = ops.attention(qkv.cuda().reshape(B * L, 3 * W), B, L, H, causal=causal).cpu().view(B, L, W)
    q, k, v = (t.view(B, L, H, 64).transpose(1, 2).float() for t in qkv.split(W, dim=-1))
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf")).triu_(1)
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, W)
    # probabilities are rounded to fp16 before P.V (as the reference's fp16 attention does): ~1e-3 relative
    assert (out.float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
    assert rel_err(out.reshape(-1, W), ref.reshape(-1, W)) < 2e-3


@pytest.mark.parametrize("L,H", [(17, 4), (26, 3), (32, 2), (33, 2), (50, 12), (64, 2), (100, 2), (128, 4), (197, 12), (256, 2)])
def test_attention_counted_waits_under_load(ops, L, H):
    """The query-first kernels go through their first barrier on a COUNTED s_waitcnt (K landed, V in flight): a count one too high lets a wave multiply against K rows
    that have not arrived — which single small launches rarely show (the four-wave form at L <= 32 did exactly that and passed the shapes above; an image -> logits
    fixture on 17-token towers failed in two of four runs).  Here: a batch large enough to fill the chip several times over (HBM-cold K / V for most workgroups), repeated,
    every repetition EQUAL to the first and close to fp32 attention."""
    B = max(64, 60000 // (L * H))
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(L * 131 + H)
    qkv = (torch.randn(B * L, 3 * W, device="cuda", generator=g) * 1.5).half()
    first = None
    for rep in range(12):
        junk = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").random_(0, 255)        # push K / V out of the caches between repetitions
        out = ops.attention(qkv, B, L, H, causal=False)
        if first is None:
            first = out.clone()
            q, k, v = (t.view(B, L, H, 64).transpose(1, 2).float() for t in qkv.split(W, dim=-1))
            ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(B * L, W)
            assert (first.float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
        else:
            assert torch.equal(out, first), (rep, int((out != first).any(1).sum()))
        del junk


@pytest.mark.parametrize("B,L,H,causal,grid", [(40, 197, 12, False, 0), (9, 197, 3, False, 5), (30, 50, 12, False, 7), (16, 77, 8, True, 6),
                                                (5, 256, 2, False, 3), (7, 225, 2, False, 4), (3, 33, 1, True, 2), (2, 1, 1, False, 0),
                                                (6, 128, 2, True, 4), (3, 129, 2, False, 1)])
def test_attention_pipelined_kernel_is_bit_identical(ops, B, L, H, causal, grid):
    """The persistent double-buffered attention (whole batches: next item's K / V / Q rows prefetched by LDS-DMA while the current
    one is multiplied) against the one-workgroup-per-item kernel: same per-tile arithmetic, so the outputs must be EQUAL; `grid`
    caps the persistent grid so that workgroups walk several items (odd counts: both buffers, a ragged last round)."""
    from proto_clip_amd import _lib
    lib = _lib.load()
    W = H * 64
    qkv = (torch.from_numpy(synth.normal((B * L, 3 * W), 29, L)).float() * 1.5).half().cuda()
    try:
        _lib.check(lib.pclip_attention_config(0, 0), "pclip_attention_config")
        ref = ops.attention(qkv, B, L, H, causal=causal)
        _lib.check(lib.pclip_attention_config(1, grid), "pclip_attention_config")
        got = torch.full_like(ref, float("nan"))
        ops.attention(qkv, B, L, H, causal=causal, out=got)
        again = ops.attention(qkv, B, L, H, causal=causal)
    finally:
        _lib.check(lib.pclip_attention_config(-1, 0), "pclip_attention_config")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(again, ref)


def test_stems(ops):
    B, R, P, W = 3, 32, 8, 128
    img = torch.from_numpy(synth.normal((B, 3, R, R), 24, 0)).half()
    cols = ops.im2col_patches(img.cuda(), P).cpu()
    ref = torch.nn.functional.unfold(img.float(), kernel_size=P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P).half()
    assert torch.equal(cols, ref)
    img14 = torch.from_numpy(synth.normal((2, 3, 70, 70), 24, 1)).half()        # P=14: K=588 padded to 640 with zeros
    cols = ops.im2col_patches(img14.cuda(), 14).cpu()
    ref = torch.nn.functional.unfold(img14.float(), kernel_size=14, stride=14).transpose(1, 2).reshape(-1, 588).half()
    assert cols.shape[1] == 640 and torch.equal(cols[:, :588], ref) and cols[:, 588:].abs().max().item() == 0
    x32 = torch.from_numpy(synth.normal((1000,), 24, 2)).float()
    assert torch.equal(ops.cast_f16(x32.cuda()).cpu(), x32.half())
    # fp32 images: the cast to fp16 rides on the gather (vector path P % 8 == 0 and the scalar path of P = 14)
    for im, pp in ((torch.from_numpy(synth.normal((B, 3, R, R), 24, 5)).float() * 1.7, P), (torch.from_numpy(synth.normal((2, 3, 70, 70), 24, 6)).float(), 14)):
        assert torch.equal(ops.im2col_patches(im.cuda(), pp), ops.im2col_patches(im.half().cuda(), pp))
    toks = torch.tensor([[5, 9, 2, 11, 0, 0], [5, 11, 0, 0, 0, 0]])
    emb = torch.from_numpy(synth.normal((12, 64), 24, 3)).half()
    pos = torch.from_numpy(synth.normal((6, 64), 24, 4)).half()
    x = ops.text_embed(toks.cuda(), emb.cuda(), pos.cuda())
    assert torch.equal(x.cpu().view(2, 6, 64), (emb[toks].float() + pos.float()).half())
    eot = ops.gather_eot(x, toks.cuda(), 2, 6, 64).cpu()
    assert torch.equal(eot, x.cpu().view(2, 6, 64)[torch.arange(2), toks.argmax(-1)])


# ---------------------------------------------------------------- whole towers ---------------------------
@pytest.mark.parametrize("tag", list(ENCODERS))
def test_towers_against_reference(ops, tag):
    g = golden("encoder_" + tag)
    kw = ENCODERS[tag]
    sd = random_state_dict(seed=11, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    assert list(model.state_dict().keys()) == [k for k in sd.keys()] or set(model.state_dict()) == set(sd)
    imgs = synth.make_images(24, kw["image_resolution"], seed=5, n_class=6)
    toks = torch.from_numpy(g["tokens"]).long()
    fi, ft = model.encode_image(imgs.cuda()), model.encode_text(toks.cuda())
    assert fi.dtype == torch.float16 and fi.shape == (24, kw["embed_dim"]) and ft.shape == (12, kw["embed_dim"])
    for key in ("img", "txt"):
        out = fi if key == "img" else ft
        r16_, r32_ = torch.from_numpy(g[key + "_f16"]), torch.from_numpy(g[key + "_f32"])
        gap = rel_err(r16_, r32_)                 # the reference's own fp16-vs-fp32 disagreement
        observe(f"tower {tag}/{key}: reference fp16<->fp32 gap (yard-stick)", gap, gap)
        assert observe(f"tower {tag}/{key}: rel err vs reference fp32", rel_err(out, r32_), max(2.0 * gap, 3e-3)) <= max(2.0 * gap, 3e-3)
        assert observe(f"tower {tag}/{key}: rel err vs reference fp16", rel_err(out, r16_), max(2.0 * gap, 3e-3)) <= max(2.0 * gap, 3e-3)
    # and against the oracle (same rounding points by construction)
    oi = clip_oracle.encode_image(sd, imgs, half=True)
    assert observe(f"tower {tag}/img: rel err vs oracle fp16", rel_err(fi, oi), 3e-3) <= 3e-3


def test_bank_builders_against_reference(ops, tmp_path):
    """utils.py:284-361 through proto_clip_amd.utils with the tiny tower and list-of-batches loaders."""
    from proto_clip_amd.utils import build_cache_model, pre_load_features
    g = golden("encoder_tiny")
    kw = ENCODERS["tiny"]
    model = build_model(random_state_dict(seed=11, **kw)).cuda()
    imgs = synth.make_images(24, 32, seed=5, n_class=6)
    labels = torch.from_numpy(g["cache_labels"]).long()
    loader = [(imgs[:10], labels[:10]), (imgs[10:], labels[10:])]
    cfg = dict(cache_dir=str(tmp_path), backbone="tiny", shots=4, augment_epoch=2)
    keys, values = build_cache_model(cfg, model, loader)
    feats, flabels = pre_load_features(cfg, "val", model, loader)
    assert keys.shape == (64, 24) and values.shape == (24, 6) and values.dtype == torch.int64
    assert torch.equal(values.cpu().argmax(1), torch.sort(labels, stable=True).values)
    assert torch.equal(flabels.cpu(), labels)
    # the reference's argsort is unstable: compare per-class column SETS via sorted order of a stable key
    ref_keys, ref_vals = torch.from_numpy(g["cache_keys"]).float(), torch.from_numpy(g["cache_values"]).long().argmax(1)
    ours = keys.cpu().float()
    for c in range(6):
        a, b = ours[:, values.cpu().argmax(1) == c], ref_keys[:, ref_vals == c]
        assert a.shape == b.shape
        # match columns greedily by cosine similarity
        sim = a.t() @ b
        assert sim.max(dim=1).values.min().item() > 0.999       # fp16 tower noise on the tiny random-init model (reference fp16 vs fp32: same size)
    assert rel_err(feats, torch.from_numpy(g["pre_features"])) <= 5e-3
    # caches were written with the reference's file names and are re-read on the second call
    import os
    assert os.path.exists(f"{tmp_path}/models/tiny/K-4/aug/visual_mb_keys_aug_2_4_shots.pt")
    k2, v2 = build_cache_model(cfg, None, None)
    assert torch.equal(k2.cpu(), keys.cpu())


def test_clip_classifier_batched(ops):
    """utils.py:256-273 with synthetic token ids: batched text tower + fused normalise/mean/normalise."""
    from proto_clip_amd.utils import clip_classifier
    kw = ENCODERS["tiny"]
    sd = random_state_dict(seed=11, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    names, templ = [f"c{i}" for i in range(5)], ["a {}.", "b {}.", "c {}."]
    ids = {}

    def fake_tokenize(texts):
        t = torch.zeros(len(texts), 77, dtype=torch.long)
        for i, s in enumerate(texts):
            body = [(hash_ % 500) + 1 for hash_ in (sum(map(ord, s)), len(s) * 7, ord(s[0]) * 3)]
            t[i, 0], t[i, 1:4], t[i, 4] = 510, torch.tensor(body), 511
        return t

    _, w = clip_classifier(names, templ, model, tokenize=fake_tokenize)
    assert w.shape == (64, 5) and w.dtype == torch.float16
    toks = fake_tokenize([t.format(c) for c in names for t in templ])
    emb = clip_oracle.encode_text(sd, toks, half=True)
    ref = po.proto_build(emb, 5, 3, per_shot_norm=True)               # normalise rows, mean over templates, normalise
    assert rel_err(w.t(), ref) <= 5e-3


def test_serving_entry_eager_and_graph(ops, tmp_path):
    """toolkit-style consumer (proto_clip_classifier.py:48-71, 132-147): banks + adapter from disk, top-k per
    request; hipGraph replay must reproduce the eager launch sequence bit for bit."""
    from proto_clip_amd.model import Adapter
    from proto_clip_amd.serving import ProtoClipClassifier, load_pretrained_mb_and_adapters
    from conftest import randomize_adapter_
    kw = ENCODERS["tiny"]
    sd = random_state_dict(seed=11, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    N, K, D = 9, 4, 64
    split = synth.make_split(N, K, D, 8, 8, seed=6, sigma=2.0)
    emb_v = (split.visual_memory_keys.t().float() * 1.3).half().contiguous()
    emb_t = (split.textual_memory_bank.t().float() * 1.4).half().contiguous()
    torch.manual_seed(5)
    ad = randomize_adapter_(Adapter(D, "conv-3x", dtype=torch.half), 5)
    torch.save(torch.nn.Parameter(emb_v), tmp_path / "v.pt")
    torch.save(torch.nn.Parameter(emb_t), tmp_path / "t.pt")
    torch.save(ad.state_dict(), tmp_path / "a.pt")
    ev, et, adapter = load_pretrained_mb_and_adapters(memory_bank_v_path=str(tmp_path / "v.pt"), memory_bank_t_path=str(tmp_path / "t.pt"),
                                                      adapter_type="conv-3x", adapter_weights_path=str(tmp_path / "a.pt"))
    clf = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.3, beta=7.0, top_k=3, class_names=[f"c_{i}" for i in range(N)])
    imgs = synth.make_images(4, 32, seed=9, n_class=N).cuda()
    tp, ti = clf.classify(imgs)
    assert tp.shape == (4, 3) and ti.shape == (4, 3) and ti.dtype == torch.int64
    # oracle on the GPU's own adapted features isolates the classification arithmetic
    with torch.no_grad(), ops.low_latency():              # the serving entry runs its linears in low-latency (split-K) mode
        f = ops.l2norm_rows(model.encode_image(imgs))
        a = adapter(f, l2norm_out=True)
    p = po.P(a.cpu(), po.proto_build(emb_v, N, K), po.l2norm_rows(emb_t), 0.3, 7.0)
    rv, ri = p.topk(3, dim=1)
    torch.testing.assert_close(tp.cpu(), rv, rtol=0, atol=1e-4)
    assert torch.equal(ti.cpu(), ri)
    clf.capture(4)
    for _ in range(3):
        tg, ig = clf.classify(imgs)
        assert torch.equal(tg, tp) and torch.equal(ig, ti)
    imgs2 = synth.make_images(4, 32, seed=10, n_class=N).cuda()
    t2, i2 = clf.classify(imgs2)                     # replay on new inputs == eager on new inputs
    e2, j2 = clf._forward(imgs2)
    assert torch.equal(t2, e2) and torch.equal(i2, j2.long())
    names, probs = clf.classify_objects(imgs)
    assert names[0][0] == f"c {int(ti[0, 0])}" and torch.equal(probs, tp)
    # out-of-distribution evaluation entry (toolkit ood_utils.py:58-111) over a list-of-batches loader
    from proto_clip_amd.serving import test_ood_performance as ood
    labels = torch.from_numpy(synth.randint(8, N, 3, 77)).long()
    imgs8 = synth.make_images(8, 32, seed=12, n_class=N)
    cfg = dict(cache_dir=str(tmp_path / "ood"), backbone="tiny", shots=K, alpha=0.3, beta=7.0)
    acc = ood(cfg, [(imgs8[:5], labels[:5]), (imgs8[5:], labels[5:])], clip_model=model, memory_bank_v_path=str(tmp_path / "v.pt"),
              memory_bank_t_path=str(tmp_path / "t.pt"), adapter_type="conv-3x", adapter_weights_path=str(tmp_path / "a.pt"))
    with torch.no_grad():
        a8 = adapter(ops.l2norm_rows(model.encode_image(imgs8.cuda())), l2norm_out=True)
    p8 = po.P(a8.cpu(), po.proto_build(emb_v, N, K), po.l2norm_rows(emb_t), 0.3, 7.0)
    assert abs(acc - 100.0 * (p8.max(1)[1] == labels).float().mean().item()) < 1e-4


def test_resnet_building_blocks(ops):
    """im2col 3x3 (NHWC and NCHW-strided, stride 1 and 2), eval BatchNorm + residual + ReLU, average pool,
    attention-pool token assembly — each against a torch restatement, byte-exact where it is data movement."""
    B, H, W, C = 2, 9, 7, 16
    x = torch.from_numpy(synth.normal((B, C, H, W), 41, 0)).half()
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    for stride in (1, 2):
        cols = ops.im2col3x3(nhwc.cuda(), (H * W * C, W * C, C, 1), B, H, W, C, stride).cpu()
        ref = torch.nn.functional.unfold(x.float(), 3, padding=1, stride=stride)              # [B, C*9, L] (c, ky, kx)
        Lo = ref.shape[-1]
        ref = ref.view(B, C, 9, Lo).permute(0, 3, 2, 1).reshape(B * Lo, 9 * C).half()        # -> (ky,kx,c)
        assert cols.shape[1] == 192 and torch.equal(cols[:, :144], ref) and cols[:, 144:].abs().max().item() == 0
    img = torch.from_numpy(synth.normal((B, 3, 8, 8), 41, 1)).half()                             # NCHW image, C=3 (scalar path)
    cols = ops.im2col3x3(img.cuda(), (3 * 64, 8, 1, 64), B, 8, 8, 3, 2).cpu()
    ref = torch.nn.functional.unfold(img.float(), 3, padding=1, stride=2)
    ref = ref.view(B, 3, 9, -1).permute(0, 3, 2, 1).reshape(-1, 27).half()
    assert cols.shape[1] == 64 and torch.equal(cols[:, :27], ref) and cols[:, 27:].abs().max().item() == 0
    rows = nhwc.reshape(-1, C)
    sc = 1 + 0.2 * torch.from_numpy(synth.normal((C,), 41, 2)).float()
    sh = 0.3 * torch.from_numpy(synth.normal((C,), 41, 3)).float()
    res = torch.from_numpy(synth.normal(tuple(rows.shape), 41, 4)).half()
    y = ops.bn_act(rows.cuda(), sc.cuda(), sh.cuda(), residual=res.cuda(), relu=True).cpu()
    ref = torch.relu(po.r16(po.r16(rows.float() * sc + sh) + res.float())).half()
    assert ulp_diff(y, ref) <= 1
    y = ops.bn_act(rows.cuda(), sc.cuda(), sh.cuda(), relu=False).cpu()
    assert ulp_diff(y, po.r16(rows.float() * sc + sh).half()) <= 1
    x8 = torch.from_numpy(synth.normal((B, C, 8, 6), 41, 5)).half()
    p = ops.avgpool_nhwc(x8.permute(0, 2, 3, 1).contiguous().cuda(), B, 8, 6, C, 2).cpu().view(B, 4, 3, C).permute(0, 3, 1, 2)
    assert ulp_diff(p.reshape(B * C, -1), torch.nn.functional.avg_pool2d(x8.float(), 2).half().reshape(B * C, -1)) <= 1
    pos = torch.from_numpy(synth.normal((H * W + 1, C), 41, 6)).half()
    t = ops.attnpool_tokens(rows.cuda(), pos.cuda(), B, H * W, C).cpu().view(B, H * W + 1, C)
    tok = nhwc.view(B, H * W, C).float()
    ref = torch.cat([po.r16(tok.mean(1, keepdim=True)), tok], 1)
    assert ulp_diff(t.reshape(-1, C), po.r16(ref + pos.float()).half().reshape(-1, C)) <= 1


@pytest.mark.parametrize("tag", ["rn_a", "rn_b"])
def test_resnet_tower_against_reference(ops, tag):
    """ModifiedResNet (clip/model.py:95-152) end to end against the reference's fp32 and fp16-weight towers."""
    from conftest import RESNETS
    g = golden("encoder_" + tag)
    kw = RESNETS[tag]
    sd = random_state_dict(seed=13, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    assert set(model.state_dict()) == set(sd)
    imgs = synth.make_images(6, kw["image_resolution"], seed=5, n_class=6)
    f = model.encode_image(imgs.cuda())
    assert f.dtype == torch.float16 and f.shape == (6, kw["embed_dim"])
    r16_, r32_ = torch.from_numpy(g["img_f16"]), torch.from_numpy(g["img_f32"])
    gap = rel_err(r16_, r32_)
    assert rel_err(f, r32_) <= max(2.0 * gap, 5e-3), (rel_err(f, r32_), gap)
    assert rel_err(f, r16_) <= max(2.0 * gap, 5e-3), (rel_err(f, r16_), gap)
    assert rel_err(f, clip_oracle.encode_image_resnet(sd, imgs, half=True)) <= 5e-3
    model.visual.chunk = 4                                 # chunked path == single pass
    assert torch.equal(model.encode_image(imgs.cuda()).cpu(), f.cpu())


BN_TILES = ((128, 128), (256, 128), (256, 256), (256, 64), (256, 32))      # the tile configurations PCLIP_GEMM_BN_CFG forces (read once per process: never in a test)


def _with_forced_cfgs(cases):
    """The cases as they were (cfg None: the product entry, ids unchanged) + every tile configuration that fits N, forced per call."""
    out = [pytest.param(*c, None, id="-".join(str(v) for v in c)) for c in cases]
    return out + [pytest.param(*c, cfg, id="-".join(str(v) for v in c) + f"-cfg{cfg}") for c in cases for cfg, (_, bn) in enumerate(BN_TILES) if c[1] % bn == 0]


@pytest.mark.parametrize("M,N,K,relu,cfg", _with_forced_cfgs([(5000, 64, 576, True), (3136 * 4, 64, 64, True), (2000, 32, 64, True), (4096, 256, 64, False),
                                                              (70000, 128, 1152, True), (777, 2048, 512, True), (50432, 512, 128, False)]))
def test_gemm_bn_equals_gemm_then_bn_act(ops, M, N, K, relu, cfg):
    """conv + eval BatchNorm (+ ReLU) as one GEMM launch (scale / shift strips in the epilogue; 256x64 tiles for 64-channel
    convolutions, the generic kernel for 32) must reproduce conv-GEMM followed by pclip_bn_act_f16 bit for bit.  cfg: the tile
    configuration forced through the test entry, asserted from its report."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    ss = torch.stack([1 + 0.3 * torch.randn(N, device="cuda", generator=g), 0.2 * torch.randn(N, device="cuda", generator=g)]).contiguous()
    ref = ops.bn_act(ops.gemm(a, w), ss[0], ss[1], relu=relu)
    if cfg is None:
        got = ops.gemm_bn(a, w, ss[0], ss[1], relu=relu)
    else:
        got, launches = ops.gemm_route(a, w, act=3 if relu else 2, scale=ss[0], shift=ss[1], cfg=cfg)
        assert [(l["family"], l["rows"]) for l in launches] == [(f"cfg{cfg}", M)], launches
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M,N,K,cfg", _with_forced_cfgs([(5000, 256, 64), (3136 * 8, 256, 64), (70000, 512, 128), (777, 2048, 512), (49, 2048, 512), (200, 64, 64),
                                                         (50432, 1024, 256)]))
def test_gemm_bn_residual_relu_equals_separate(ops, M, N, K, cfg):
    """conv3 + bn3 + identity add + ReLU of a bottleneck in one launch (pclip_gemm_bn_res_f16: persistent kernels incl. the row
    split, and the ring kernel for small M) against GEMM followed by pclip_bn_act_f16: bit for bit.  cfg: the tile configuration forced
    through the test entry, asserted from its report."""
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    res = torch.randn(M, N, device="cuda", generator=g).half()
    ss = torch.stack([1 + 0.3 * torch.randn(N, device="cuda", generator=g), 0.2 * torch.randn(N, device="cuda", generator=g)]).contiguous()
    ref = ops.bn_act(ops.gemm(a, w), ss[0], ss[1], residual=res, relu=True)
    if cfg is None:
        got = ops.gemm_bn_res_relu(a, w, ss[0], ss[1], res)
    else:
        got, launches = ops.gemm_route(a, w, act=5, residual=res, scale=ss[0], shift=ss[1], cfg=cfg)
        assert [(l["family"], l["rows"]) for l in launches] == [(f"cfg{cfg}", M)], launches
    assert torch.equal(got, ref)
    assert (got >= 0).all()


@pytest.mark.parametrize("B,H,W,Cin,Cout,relu", [(2, 56, 56, 64, 64, True), (3, 28, 28, 128, 128, True), (2, 14, 14, 256, 256, True),
                                                 (5, 7, 7, 512, 512, True), (1, 9, 7, 64, 128, False), (3, 13, 11, 64, 64, True),
                                                 (64, 56, 56, 64, 64, True), (1, 1, 1, 64, 64, True), (2, 28, 28, 32, 64, True),
                                                 (16, 112, 112, 32, 64, True), (1, 9, 11, 16, 64, False), (3, 7, 5, 8, 128, True),
                                                 (16, 112, 112, 32, 32, True), (2, 10, 6, 32, 32, False), (1, 5, 5, 64, 32, True)])
def test_conv3x3_implicit_gemm_equals_im2col_path(ops, B, H, W, Cin, Cout, relu):
    """The implicit-GEMM convolution (LDS-DMA gather of every tap, zero line outside the image) against the materialised
    im2col + fused GEMM/BN path: same MFMA k-order -> bit-identical; plus a torch conv2d reference on the small cases."""
    g = torch.Generator(device="cuda").manual_seed(B * H + Cin)
    x = (torch.randn(B * H * W, Cin, device="cuda", generator=g) * 0.7).half()
    w = (torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) * (9 * Cin) ** -0.5).half()
    ss = torch.stack([1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)]).contiguous()
    w2 = w.reshape(Cout, 9 * Cin)
    if (9 * Cin) % 64:                                       # Cin < 64: rows zero-padded to the K-tile
        w2 = torch.cat([w2, w2.new_zeros(Cout, (9 * Cin + 63) // 64 * 64 - 9 * Cin)], dim=1)
    w2 = w2.contiguous()
    cols = ops.im2col3x3(x, (H * W * Cin, W * Cin, Cin, 1), B, H, W, Cin, 1)
    ref = ops.gemm_bn(cols, w2, ss[0], ss[1], relu=relu)
    with ops.conv_strip(False):                              # (the narrow layers have a kernel of their own: next test)
        got = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin, relu=relu)
    assert torch.equal(got, ref)
    if B * H * W <= 2000:
        xt = x.view(B, H, W, Cin).permute(0, 3, 1, 2).float().cpu()
        conv = torch.nn.functional.conv2d(xt, w.permute(0, 3, 1, 2).float().cpu(), padding=1).half().float()
        y = (conv * ss[0].cpu()[None, :, None, None] + ss[1].cpu()[None, :, None, None]).half().float()
        if relu:
            y = y.clamp_min(0)
        yt = y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
        assert (got.float().cpu() - yt).abs().max().item() <= 2e-2 * yt.abs().max().item()


@pytest.mark.parametrize("B,H,W,Cin,Cout,relu", [(3, 112, 112, 32, 32, True), (2, 112, 112, 32, 64, True), (6, 56, 56, 64, 64, True), (40, 8, 56, 64, 64, False),
                                                 (9, 16, 56, 32, 64, True), (2, 56, 112, 64, 32, True), (300, 56, 56, 64, 64, True), (70, 112, 112, 32, 32, False),
                                                 (1, 24, 168, 64, 64, True), (1, 8, 56, 32, 32, True), (7, 40, 168, 32, 64, False), (3, 72, 224, 64, 32, True)])
def test_conv3x3_strip_kernel(ops, B, H, W, Cin, Cout, relu):
    """The narrow 3x3 convolutions of the ModifiedResNet tower (stem conv2 / conv3, layer1 conv2; clip/model.py:100-108, 20-22 of the reference) through
    csrc/pclip_conv_strip.hip — weights in registers, the tile's input block with its halo once in LDS, zero padding by out-of-range buffer loads — against
    (i) the implicit-GEMM kernel it replaces: the same rounding points, another fp32 summation order, so fp16 results agree except for single-ulp flips of the convolution's fp16 output, bounded and counted;
    (ii) torch's fp32 conv2d of the same fp16 operands + the BatchNorm affine in fp32 (small cases); every border (one-strip images: top and bottom in the same
    tile; 112-wide images: two tiles per row) and more tiles than CUs (persistent walk, both block buffers)."""
    with ops.conv_strip(True):
        assert ops.conv_strip_applies(B, H, W, Cin, Cout)
    g = torch.Generator(device="cuda").manual_seed(B * H + Cin + Cout)
    x = (torch.randn(B * H * W, Cin, device="cuda", generator=g) * 0.7).half()
    w = (torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) * (9 * Cin) ** -0.5).half()
    ss = torch.stack([1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)]).contiguous()
    w2 = w.reshape(Cout, 9 * Cin)
    if (9 * Cin) % 64:
        w2 = torch.cat([w2, w2.new_zeros(Cout, (9 * Cin + 63) // 64 * 64 - 9 * Cin)], dim=1)
    w2 = w2.contiguous()
    with ops.conv_strip(False):
        ref = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin, relu=relu)
    with ops.conv_strip(True):                               # (named: the test also runs under PCLIP_CONV_STRIP=0)
        got = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin, relu=relu)
        again = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin, relu=relu)
    assert torch.equal(got, again)                           # deterministic
    d = (got.float() - ref.float()).abs()
    # one fp16 ulp of the CONVOLUTION's output (r16(acc), the first rounding point) moves the result by 2^-10 |conv| scale = 2^-10 |y - shift| <= 2^-10 (|y| + |shift|);
    # one more ulp of y itself where the second rounding flips with it
    bound = 2.0 ** -10 * (2 * ref.float().abs() + ss[1].abs()[None, :]) * 1.01 + 2.0 ** -24
    assert bool((d <= bound).all()), (d / bound).max().item()
    frac = (d > 0).float().mean().item()
    observe(f"conv3x3 strip kernel {Cin}->{Cout} {H}x{W}: fraction of fp16 results one ulp from the implicit GEMM's", frac, 5e-3)
    assert frac <= 5e-3
    if B * H * W <= 80000:
        xt = x.view(B, H, W, Cin).permute(0, 3, 1, 2).float().cpu()
        conv = torch.nn.functional.conv2d(xt, w.permute(0, 3, 1, 2).float().cpu(), padding=1).half().float()
        y = (conv * ss[0].cpu()[None, :, None, None] + ss[1].cpu()[None, :, None, None]).half().float()
        if relu:
            y = y.clamp_min(0)
        yt = y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
        err = (got.float().cpu() - yt).abs()
        # the border rows / columns by themselves: a wrong halo shows there first
        m = torch.zeros(B, H, W, dtype=torch.bool)
        m[:, 0] = m[:, -1] = True
        m[:, :, 0] = m[:, :, -1] = True
        m[:, :, 55:57] = True
        bound = 4e-3 * yt.abs().max().item()
        assert err.max().item() <= bound and err[m.reshape(-1)].max().item() <= bound, (err.max().item(), bound)


@pytest.mark.parametrize("strip", [True, False])
def test_conv3x3_batches_beyond_32_bit_offsets_go_in_slices(ops, strip):
    """The convolution kernels address their input through buffer descriptors with 32-bit offsets: a batch of more than 2^31 bytes (2 700 stem-sized images) is cut
    into slices of whole images by the launcher — the result of every image must be the bits it has in a small batch (first, middle around the cut, last images)."""
    B, H, W, Cin, Cout = 2700, 112, 112, 32, 32
    assert B * H * W * Cin * 2 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.empty(B * H * W, Cin, dtype=torch.float16, device="cuda")
    x.view(-1)[:] = (torch.randn(64 * H * W * Cin, device="cuda", generator=g) * 0.7).half().repeat(B // 64 + 1)[: x.numel()]
    w = (torch.randn(Cout, 320, device="cuda", generator=g) * 288 ** -0.5).half()
    w[:, 288:] = 0
    sc, sh = 1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)
    with ops.conv_strip(strip):
        y = ops.conv3x3_bn(x, w, sc, sh, B, H, W, Cin, relu=True).view(B, H * W, Cout)
        cut = (2 ** 31) // (H * W * Cin * 2)
        for b0, n in ((0, 3), (cut - 2, 4), (B - 3, 3)):
            part = ops.conv3x3_bn(x.view(B, -1)[b0:b0 + n].reshape(n * H * W, Cin), w, sc, sh, n, H, W, Cin, relu=True).view(n, H * W, Cout)
            assert torch.equal(y[b0:b0 + n], part), (strip, b0)
    del x, y


@pytest.mark.parametrize("B,H,W", [(3, 112, 112), (40, 8, 56), (70, 112, 112), (5, 16, 112)])
def test_conv3x3_bn_relu_avgpool_in_one_launch(ops, B, H, W):
    """The stem's tail — conv3 / bn3 / relu / AvgPool2d(2), clip/model.py:104-105, 142-143 of the reference — in one launch (the strip kernel's pooling epilogue) must
    be pclip_conv3x3_bn_f16 followed by pclip_avgpool_nhwc_f16 bit for bit."""
    Cin, Cout = 32, 64
    if os.environ.get("PCLIP_CONV_POOL") == "0" or os.environ.get("PCLIP_CONV_STRIP") == "0":
        pytest.skip("the fused form is switched off in this environment")
    assert ops.conv3x3_pool_applies(H, W, Cin, Cout)
    g = torch.Generator(device="cuda").manual_seed(B + H)
    x = (torch.randn(B * H * W, Cin, device="cuda", generator=g) * 0.7).half()
    w = (torch.randn(Cout, 320, device="cuda", generator=g) * 288 ** -0.5).half()
    w[:, 288:] = 0
    sc, sh = 1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)
    ref = ops.avgpool_nhwc(ops.conv3x3_bn(x, w, sc, sh, B, H, W, Cin, relu=True), B, H, W, Cout, 2)
    got = ops.conv3x3_bn_pool(x, w, sc, sh, B, H, W, Cin)
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("B,R,Cout,f32,relu", [(3, 224, 32, True, True), (2, 224, 64, False, True), (5, 112, 32, True, False), (70, 224, 32, True, True)])
def test_stem_conv_from_nchw_images(ops, B, R, Cout, f32, relu):
    """The stem's first convolution (3 -> Cout, stride 2) + bn1 + relu straight from the NCHW images (csrc/pclip_conv_strip.hip: stem_conv_kernel; clip/model.py:100-102, 138
    of the reference) against the path it replaces — cast to fp16, pclip_im2col3x3_f16 through the image's strides, pclip_gemm_bn_f16 — on the same operands: one MFMA
    K-step over the same 27 products, so the results are compared for EQUALITY first and, where the summation order of the two MFMA shapes differs, by the bound of one
    ulp of the convolution's fp16 output; plus torch's fp32 conv2d.  Image borders (top / left padding; the last row / column are interior at an even side) included."""
    assert ops.stem_conv_applies(R, Cout) or os.environ.get("PCLIP_CONV_STEM") == "0"        # (the switch only concerns the model's routing: the kernel is called directly below)
    g = torch.Generator(device="cuda").manual_seed(B + R + Cout)
    img = torch.randn(B, 3, R, R, device="cuda", generator=g)
    if not f32:
        img = img.half()
    w = (torch.randn(Cout, 3, 3, 3, device="cuda", generator=g) * 27 ** -0.5).half()           # [Cout, ky, kx, channel]
    w2 = torch.cat([w.reshape(Cout, 27), w.new_zeros(Cout, 37)], dim=1).contiguous()
    ss = torch.stack([1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)]).contiguous()
    got = ops.stem_conv_bn(img, w2, ss[0], ss[1], relu=relu)
    i16 = (ops.cast_f16(img) if f32 else img).contiguous()
    cols = ops.im2col3x3(i16, (3 * R * R, R, 1, R * R), B, R, R, 3, 2)
    ref = ops.gemm_bn(cols, w2, ss[0], ss[1], relu=relu)
    d = (got.float() - ref.float()).abs()
    bound = 2.0 ** -10 * (2 * ref.float().abs() + ss[1].abs()[None, :]) * 1.01 + 2.0 ** -24
    assert bool((d <= bound).all()), (d / bound).max().item()
    frac = (d > 0).float().mean().item()
    observe(f"stem conv 3->{Cout} R={R}: fraction of fp16 results differing from the im2col + GEMM path", frac, 5e-3)
    assert frac <= 5e-3
    if B <= 5:
        Ho = R // 2
        conv = torch.nn.functional.conv2d(i16.float().cpu(), w.permute(0, 3, 1, 2).float().cpu(), stride=2, padding=1).half().float()
        yv = (conv * ss[0].cpu()[None, :, None, None] + ss[1].cpu()[None, :, None, None]).half().float()
        if relu:
            yv = yv.clamp_min(0)
        yt = yv.permute(0, 2, 3, 1).reshape(B * Ho * Ho, Cout)
        err = (got.float().cpu() - yt).abs()
        assert err.max().item() <= 4e-3 * yt.abs().max().item(), err.max().item()


@pytest.mark.parametrize("B,L,H,Lq", [(5, 197, 12, 1), (3, 50, 12, 1), (2, 257, 16, 1), (4, 197, 12, 40), (2, 77, 8, 77), (2, 280, 4, 200), (3, 257, 16, 160), (2, 288, 2, 256)])      # the last three: 5 - 8 query tiles against MORE than 8 key tiles (the query-first kernel must not take them)
def test_attention_first_queries_matches_full_attention(ops, B, L, H, Lq):
    """Separate-operand attention (queries of the first Lq tokens, keys / values of all tokens) against the fused-QKV kernel:
    the rows it produces must be bit-identical to the same rows of the full attention."""
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(L + H)
    qkv = torch.randn(B * L, 3 * W, device="cuda", generator=g).half()
    full = ops.attention(qkv, B, L, H).view(B, L, W)
    q = qkv.view(B, L, 3 * W)[:, :Lq, :W].contiguous().view(B * Lq, W)
    kv = qkv[:, W:].contiguous()
    got = ops.attention_first_queries(q, kv, B, L, Lq, H).view(B, Lq, W)
    assert torch.equal(got, full[:, :Lq])


def test_full_size_vit_b16_against_oracle():
    """The real ViT-B/16 architecture (12 layers x 768, 197 tokens; random-init weights) on 6 images against the oracle in both
    of the reference's precisions: depth-12 amplification of the fp16 rounding differences stays inside the fp16 <-> fp32 gap."""
    from proto_clip_amd.clip.model import BACKBONES
    kw = BACKBONES["ViT-B/16"]
    sd = random_state_dict(seed=21, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    imgs = synth.make_images(6, 224, seed=8, n_class=6)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
    o16 = clip_oracle.encode_image(sd, imgs, half=True).float()
    o32 = clip_oracle.encode_image(sd, imgs, half=False).float()
    gap = rel_err(o16, o32)
    observe("full-size ViT-B/16: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe("full-size ViT-B/16: rel err vs oracle fp16", rel_err(f, o16), max(2 * gap, 3e-3)) <= max(2 * gap, 3e-3)
    assert observe("full-size ViT-B/16: rel err vs oracle fp32", rel_err(f, o32), max(2 * gap, 3e-3)) <= max(2 * gap, 3e-3)
    # the class-token shortcut of the last block and the one-pass batch must not depend on the batch: same rows alone
    with torch.no_grad():
        f1 = model.encode_image(imgs[2:3].cuda()).float().cpu()
    assert torch.equal(f1[0], f[2])


@pytest.mark.parametrize("tag", ["vitb16", "vitb32", "rn50", "vitl14"])
def test_full_size_towers_against_reference(tag):
    """The real architectures of BASELINE.json's configurations through the REFERENCE's own towers (tests/golden/encoder_<tag>.npz: make_golden.make_encoder_full
    runs /root/reference's build_model at the hyper-parameters OpenAI's checkpoints resolve to — ViT-B/16: 12 x 768, 197 tokens, 12 heads; ViT-B/32; RN50:
    ModifiedResNet (3, 4, 6, 3) + attention pool; ViT-L/14: 24 x 1024, 257 tokens; text 12 x 512 / 768 — on 4 - 8 images and prompts, fp16-weight and fp32):
    encode_image / encode_text of the HIP path within max(2 x the reference's own fp16 <-> fp32 gap, 3e-3), the bound of the toy-tower fixtures
    (clip/model.py:10-152, 221-238, 338-354, 397-434)."""
    from proto_clip_amd.clip.model import BACKBONES
    from spec import ENCODERS_FULL
    g = golden("encoder_" + tag)
    spec_ = ENCODERS_FULL[tag]
    kw = BACKBONES[spec_["backbone"]]
    sd = random_state_dict(seed=spec_["sd_seed"], **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    imgs = synth.make_images(spec_["n_img"], kw["image_resolution"], seed=5, n_class=6)
    toks = torch.from_numpy(g["tokens"]).long()
    with torch.no_grad():
        fi, ft = model.encode_image(imgs.cuda()), model.encode_text(toks.cuda())
    name = spec_["backbone"]
    for key, out in (("img", fi), ("txt", ft)):
        r16_, r32_ = torch.from_numpy(g[key + "_f16"]), torch.from_numpy(g[key + "_f32"])
        gap = rel_err(r16_, r32_)
        observe(f"full-size {name} {key}: reference fp16<->fp32 gap (yard-stick)", gap, gap)
        assert observe(f"full-size {name} {key}: rel err vs REFERENCE fp32", rel_err(out, r32_), max(2.0 * gap, 3e-3)) <= max(2.0 * gap, 3e-3)
        assert observe(f"full-size {name} {key}: rel err vs REFERENCE fp16", rel_err(out, r16_), max(2.0 * gap, 3e-3)) <= max(2.0 * gap, 3e-3)


def test_bench_configuration_rows_equal_small_batches():
    """What bench.py times, tested: ViT-B/16 encode_image on the bench's own 1024 images (M = 201 728 token rows: persistent 256 x 256 tiles
    over 37 rounds, the row-split 128 x 128 tails, descending tile order, the whole-batch LayerNorm kernel, the four-slab QuickGELU epilogue)
    must give, for rows {0 .. 5, 511, 1018 .. 1023}, exactly the bits of the same images encoded in a batch of 6 / alone — the contract
    `a row alone == the row in a batch` that test_full_size_vit_b16_against_oracle states at B = 6; and the whole hot-path step's top-1 for those rows equals the step on the sub-batch."""
    import bench
    from proto_clip_amd.dist import HipPath, PrototypeExchange, hot_path_step
    st = bench.build_state(torch.device("cuda", 0), 0, 1)
    rows = list(range(6)) + [511] + list(range(1018, 1024))
    if True:
        with torch.no_grad():
            big = st["model"].encode_image(st["images"])
            sub = st["model"].encode_image(st["images"][rows].contiguous())
            one = st["model"].encode_image(st["images"][511:512].contiguous())
            assert big.shape == (bench.BATCH, bench.DIM)
            assert torch.equal(big[rows], sub), f"rows of the B = 1024 pass differ from the B = {len(rows)} pass"
            assert torch.equal(big[511], one[0])
            path, ex = HipPath(st["model"], st["adapter"]), PrototypeExchange()
            top_big = hot_path_step(path, ex, st["bank"], st["bank_labels"], bench.N_CLASS, st["images"], st["text"], bench.ALPHA, bench.BETA)
            top_sub = hot_path_step(path, ex, st["bank"], st["bank_labels"], bench.N_CLASS, st["images"][rows].contiguous(), st["text"], bench.ALPHA, bench.BETA)
            assert top_big.shape == (bench.BATCH,) and torch.equal(top_big[rows], top_sub)
            assert len(torch.unique(top_big)) >= 2             # not a constant answer (random-init towers spread 1024 synthetic images over a handful of classes)


@pytest.mark.parametrize("B,G2,W", [(3, 49, 768), (2, 196, 768), (1, 256, 1024), (5, 4, 128), (2, 9, 64)])
def test_vit_stem_fused_equals_separate(ops, B, G2, W):
    """tokens + ln_pre + the first block's ln_1 in one pass (pclip_vit_embed_ln_f16) against the three separate kernels: the row
    arithmetic is the same, so both outputs must agree bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(B * G2 + W)
    patch = (torch.randn(B * G2, W, device="cuda", generator=g) * 0.8).half()
    cls = torch.randn(W, device="cuda", generator=g).half()
    pos = (torch.randn(G2 + 1, W, device="cuda", generator=g) * 0.1).half()
    gp, bp = 1 + 0.2 * torch.randn(W, device="cuda", generator=g), 0.1 * torch.randn(W, device="cuda", generator=g)
    g1, b1 = 1 + 0.2 * torch.randn(W, device="cuda", generator=g), 0.1 * torch.randn(W, device="cuda", generator=g)
    x0, h = ops.vit_embed_ln(patch, cls, pos, B, G2, W, gp, bp, g1, b1)
    t = ops.vit_assemble_tokens(patch, cls, pos, B, G2, W)
    r0 = ops.layernorm(t, gp, bp)
    assert torch.equal(x0, r0)
    assert torch.equal(h, ops.layernorm(r0, g1, b1))


def test_serving_low_latency_mode_full_size():
    """A ViT-B/16 request through the serving entry with the split-K linears (default) and without: the split changes fp32
    summation order only, so the top-5 probabilities agree within the north star's 1e-3 and the top-1 class is the same; the
    hipGraph replay of the low-latency request reproduces its eager launches bit for bit."""
    from proto_clip_amd.clip.model import BACKBONES
    from proto_clip_amd.model import Adapter_FC
    from proto_clip_amd.serving import ProtoClipClassifier
    kw = BACKBONES["ViT-B/16"]
    model = build_model(random_state_dict(seed=24, **kw)).cuda()
    D, N, K = kw["embed_dim"], 198, 16
    split = synth.make_split(N, K, D, 8, 8, seed=3, sigma=3.0)
    ev = (split.visual_memory_keys.t().float() * 1.2).half().contiguous().cuda()
    et = (split.textual_memory_bank.t().float() * 1.4).half().contiguous().cuda()
    torch.manual_seed(7)
    adapter = Adapter_FC(D, dtype=torch.half).cuda()
    imgs = synth.make_images(3, 224, seed=12, n_class=N).cuda()
    fast = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=5)
    slow = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=5, low_latency=False)
    tp, ti = fast.classify(imgs)
    rp, ri = slow.classify(imgs)
    torch.testing.assert_close(tp, rp, rtol=0, atol=1e-3)
    assert torch.equal(ti[:, 0], ri[:, 0]) or (rp[:, 0] - rp[:, 1]).min().item() < 1e-3
    fast.capture(3)
    tg, ig = fast.classify(imgs)
    assert torch.equal(tg, tp) and torch.equal(ig, ti)
    auto = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=5, auto_graph=True)
    for n in (3, 1, 3):                                     # a graph per batch size, captured on first use
        ta, ia = auto.classify(imgs[:n])
        assert torch.equal(ta, tp[:n]) and torch.equal(ia, ti[:n])
    assert sorted(auto._graphs) == [1, 3]


def test_full_size_rn50_against_oracle():
    """The real RN50 tower (3-4-6-3 bottlenecks, 224 px, attention pool with 32 heads) on 4 images against the oracle: fused
    conv+BN launches, implicit-GEMM 3x3 convolutions, narrow tiles and the one-query attention pool all in play."""
    from proto_clip_amd.clip.model import BACKBONES
    kw = BACKBONES["RN50"]
    sd = random_state_dict(seed=22, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    imgs = synth.make_images(4, 224, seed=9, n_class=4)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
    o16 = clip_oracle.encode_image_resnet(sd, imgs, half=True).float()
    o32 = clip_oracle.encode_image_resnet(sd, imgs, half=False).float()
    gap = rel_err(o16, o32)
    observe("full-size RN50: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe("full-size RN50: rel err vs oracle fp16", rel_err(f, o16), max(2 * gap, 5e-3)) <= max(2 * gap, 5e-3)
    with torch.no_grad():
        f1 = model.encode_image(imgs[1:2].cuda()).float().cpu()
    assert torch.equal(f1[0], f[1])


def test_full_size_text_tower_against_oracle():
    """The real ViT-B/16 text tower (12 layers x 512, 8 heads, 77 tokens, vocabulary 49408) on 10 synthetic prompts of varying
    length against the oracle in both precisions (causal attention, EOT gather before the last block's tail)."""
    from proto_clip_amd.clip.model import BACKBONES
    kw = BACKBONES["ViT-B/16"]
    sd = random_state_dict(seed=23, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    V = kw["vocab_size"]
    g = torch.Generator().manual_seed(4)
    toks = torch.zeros(10, 77, dtype=torch.long)
    for i in range(10):
        n = int(torch.randint(1, 74, (1,), generator=g))
        toks[i, 0] = V - 2
        toks[i, 1:1 + n] = torch.randint(1, V - 2, (n,), generator=g)
        toks[i, 1 + n] = V - 1                                       # EOT = highest id (the argmax gather, clip/model.py:350)
    with torch.no_grad():
        f = model.encode_text(toks.cuda()).float().cpu()
    o16 = clip_oracle.encode_text(sd, toks, half=True).float()
    o32 = clip_oracle.encode_text(sd, toks, half=False).float()
    gap = rel_err(o16, o32)
    observe("full-size text tower: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe("full-size text tower: rel err vs oracle fp16", rel_err(f, o16), max(2 * gap, 3e-3)) <= max(2 * gap, 3e-3)
    with torch.no_grad():
        f1 = model.encode_text(toks[3:4].cuda()).float().cpu()
    assert torch.equal(f1[0], f[3])


@pytest.mark.parametrize("name", ["ViT-B/32", "ViT-L/14"])
def test_full_size_other_vits_against_oracle(name):
    """The other transformer backbones build_model infers (clip/model.py:397-434) at their REAL size, random-init weights, 4
    images, against the oracle in both of the reference's precisions.  ViT-L/14 (BASELINE configs[4]) exercises what ViT-B/16
    does not: patch 14 (K = 588 zero-padded to 640), L = 257 (nine query tiles: one wave of attention_kernel<8> takes two),
    width 1024 / 16 heads / 24 layers, embed 768; ViT-B/32 (configs[1]) the 50-token sequences of the four-wave attention."""
    from proto_clip_amd.clip.model import BACKBONES
    kw = BACKBONES[name]
    sd = random_state_dict(seed=25, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    imgs = synth.make_images(4, 224, seed=10, n_class=4)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
    assert f.shape == (4, kw["embed_dim"])
    o16 = clip_oracle.encode_image(sd, imgs, half=True).float()
    o32 = clip_oracle.encode_image(sd, imgs, half=False).float()
    gap = rel_err(o16, o32)
    e16, e32 = rel_err(f, o16), rel_err(f, o32)
    print(f"\n[observed] {name}: rel err vs oracle fp16 {e16:.2e}, vs fp32 {e32:.2e}; oracle fp16<->fp32 gap {gap:.2e}")
    observe(f"full-size {name}: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    observe(f"full-size {name}: rel err vs oracle fp16", e16, max(2 * gap, 3e-3))
    observe(f"full-size {name}: rel err vs oracle fp32", e32, max(2 * gap, 3e-3))
    assert e16 <= max(2 * gap, 3e-3), (e16, gap)
    assert e32 <= max(2 * gap, 3e-3), (e32, gap)
    with torch.no_grad():
        f1 = model.encode_image(imgs[2:3].cuda()).float().cpu()
    assert torch.equal(f1[0], f[2])                          # a row alone == the row in the batch, bit for bit


def test_full_size_rn101_against_oracle():
    """RN101 (3-4-23-3 bottlenecks, embed 512, 32 attention-pool heads) at real size on 4 images against the oracle."""
    from proto_clip_amd.clip.model import BACKBONES
    kw = BACKBONES["RN101"]
    sd = random_state_dict(seed=26, **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    imgs = synth.make_images(4, 224, seed=11, n_class=4)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
    o16 = clip_oracle.encode_image_resnet(sd, imgs, half=True).float()
    o32 = clip_oracle.encode_image_resnet(sd, imgs, half=False).float()
    gap = rel_err(o16, o32)
    e16, e32 = rel_err(f, o16), rel_err(f, o32)
    print(f"\n[observed] RN101: rel err vs oracle fp16 {e16:.2e}, vs fp32 {e32:.2e}; oracle fp16<->fp32 gap {gap:.2e}")
    observe("full-size RN101: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    observe("full-size RN101: rel err vs oracle fp16", e16, max(2 * gap, 5e-3))
    observe("full-size RN101: rel err vs oracle fp32", e32, max(2 * gap, 5e-3))
    assert e16 <= max(2 * gap, 5e-3), (e16, gap)
    assert e32 <= max(2 * gap, 5e-3), (e32, gap)
    with torch.no_grad():
        f1 = model.encode_image(imgs[1:2].cuda()).float().cpu()
    assert torch.equal(f1[0], f[1])


def test_clip_load_runs_on_gpu(tmp_path):
    """clip.load (clip/clip.py:92-139) of a state-dict file and of a TorchScript archive -> the same gfx950 model as
    build_model on the dict; images pre-processed by the returned transform go through encode_image."""
    from conftest import TINY
    from proto_clip_amd.clip import clip as pclip
    sd = random_state_dict(seed=3, **TINY)
    torch.save(sd, tmp_path / "m.pt")
    ref = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    model, preprocess = pclip.load(str(tmp_path / "m.pt"), device="cuda")
    imgs = synth.make_images(5, TINY["image_resolution"], seed=4, n_class=3).cuda()
    assert torch.equal(model.encode_image(imgs), ref.encode_image(imgs))
    rgb = (np.random.RandomState(0).rand(50, 41, 3) * 255).astype(np.uint8)
    x = preprocess(rgb)
    assert x.shape == (3, TINY["image_resolution"], TINY["image_resolution"]) and x.is_cuda
    assert model.encode_image(x[None]).shape == (1, TINY["embed_dim"])
    toks = pclip.tokenize(["a photo of a dog.", "itap of a tench."])        # ids beyond the tiny vocabulary are clamped by the embedding gather
    assert model.encode_text(toks.cuda()).shape == (2, TINY["embed_dim"])


@pytest.mark.parametrize("M,N,K", [(50432, 768, 768), (197, 768, 3072), (8, 768, 768), (1024, 768, 3072), (3000, 512, 2048), (777, 1024, 64),
                                   (20000, 1024, 256), (257, 100, 128), (130, 72, 72)])
def test_gemm_residual_epilogue_in_place(ops, M, N, K):
    """`x += linear(a)` of a transformer block (clip/model.py:188-189) as the epilogue of the GEMM (persistent kernels incl. the row
    split, the ring kernel for small M — (130, 72, 72): its K-tail instantiation, a partial row tile and a ragged column tile —, the generic kernel for ragged N), with the output written over the residual operand:
    bit-identical to the GEMM followed by a separate fp16 add, and to the fused add + LayerNorm pass it replaces."""
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = (torch.randn(M, K, device="cuda", generator=g) * 0.5).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    bias = (torch.randn(N, device="cuda", generator=g) * 0.1).half()
    x = torch.randn(M, N, device="cuda", generator=g).half()
    d = ops.gemm(a, w, bias)
    ref = (x.float() + d.float()).half()
    out = ops.gemm(a, w, bias, residual=x)                 # separate output
    assert torch.equal(out, ref)
    x2 = x.clone()
    got = ops.gemm(a, w, bias, residual=x2, out=x2)        # in place
    assert got.data_ptr() == x2.data_ptr() and torch.equal(x2, ref)
    if N % 8 == 0:
        gam, bet = 1 + 0.1 * torch.randn(N, device="cuda", generator=g), 0.1 * torch.randn(N, device="cuda", generator=g)
        x3 = x.clone()
        h_old = ops.add_layernorm(x3, d, gam, bet)         # the pass the fused epilogue replaces
        assert torch.equal(x3, x2) and torch.equal(ops.layernorm(x2, gam, bet), h_old)
