"""Every forward GEMM route and epilogue graded per element against float64 (tests/gemm_fwd_ref.py: the reference, the derived tolerance, the families).

Every case has three parts: worst |got - float64| / tolerance <= 1 (recorded per kernel and epilogue), the route asserted from the report of the test entry
(ops.gemm_route: a test that claims a kernel cannot go vacuous), and guard rows / columns around a strided output (ldc = N + 8, lda = ldb = K + 8, the padding
of the operands NaN) still holding their fill value.

Shapes are the smallest that reach what can go wrong, with `cus` = 4 standing in for the device's CU count (4 workgroups, 8 for the two-workgroup configurations):
  persistent kernels   M = 4 (8) full row blocks + 1 row and THREE column tiles (six of 32 columns where act 5 needs N % 64 == 0): 15 tiles on 4 workgroups,
                       27 or 54 on 8.  A workgroup steps by the grid, and neither 4 nor 8 is a multiple of 3 or 6, so each of its three or four tiles lies in another column tile than the one before — the double-buffered
                       bias / scale / shift strip copied one tile ahead, the next tile's operand descriptors, the four-wave kernel's carried bias fragment
                       always belong to a different column tile than the one in the accumulators.  Every such case computes the walk of every workgroup
                       (gemm_fwd_ref.walks: xcd_remap and the tile order of the report) and asserts it.  K = 192 = three K-tiles, plus 1, 2 and 4 K-tiles
                       (K = 64 has a wait of its own for the next strip); the tail instantiation at K % 64 in {8, 40, 56} with N % BN != 0, N % 8 == 0;
                       M in {1, BM - 1, BM, BM + 1}
  ring kernel          1 to 9 K-tiles on four slots, three tails, 3 x 3 tiles of 128 x 64 with ragged rows
  four-wave kernel     3 to 8 K-tiles on the five-slot ring, 15 tiles (three column tiles) on 4 workgroups, both builds
  generic kernel       forced on an aligned call; N % 8 != 0 with a K-tail and an odd ldc, which nothing else takes
  split-K              S = 4, and S = 8 with a last slice of one K-tile
  row split            a shape the dispatch cuts into two launches under cus = 4"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fwd_ref as ref                                          # noqa: E402
from conftest import observe                                        # noqa: E402

pytestmark = pytest.mark.gpu
CUS = ref.CUS
FILL = 777.0
SHAPES = ref.main_shapes()
LINEAR = ("plain", "bias", "gelu", "bias_gelu", "res")


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


def padded(t, pad=8, fill=float("nan")):
    """A [R, C] view with row stride C + pad; the padding holds `fill`."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


_cases = {}


def case(M, N, K, family, gelu=False, ldc_pad=8):
    """Operands of a case on the GPU (strided, NaN in the padding; the residual with the row stride of the output) and their float64 products, computed once."""
    key = (M, N, K, family, gelu and family == "large", ldc_pad)
    if key not in _cases:
        if len(_cases) > 24:
            _cases.clear()
        op = ref.operands(family, M, N, K, seed=100 + K + N, epilogue="gelu" if key[4] else "bias")
        dev = dict(a=padded(op["a"]), w=padded(op["w"]), bias=op["bias"].cuda(), res=padded(op["res"], ldc_pad), scale=op["scale"].cuda(), shift=op["shift"].cuda())
        _cases[key] = (op, dev, ref.products(op, "cuda"))
    return _cases[key]


def run(ops, dev, epilogue, in_place=False, ldc_pad=8, call=None, **route):
    """One call through the test entry (or `call`, a product entry) into a guarded, strided output.  Returns (result [M, N], launches)."""
    has_bias, act = ref.EPILOGUES[epilogue]
    M, N = dev["res"].shape
    buf = torch.full((M + 2, N + ldc_pad), FILL, dtype=torch.float16, device="cuda")
    out = buf[1:M + 1, :N]
    res = None
    if act in (5, 6):
        res = dev["res"]
        if in_place:
            out.copy_(res)
            res = out
    kw = dict(bias=dev["bias"] if has_bias else None, act=0 if act == 6 else act, residual=res, out=out)
    if act in (2, 3, 5):
        kw.update(scale=dev["scale"], shift=dev["shift"])
    if call is not None:
        call(dev["a"], dev["w"], **kw)
        launches = None
    else:
        _, launches = ops.gemm_route(dev["a"], dev["w"], cus=CUS, **kw, **route)
    torch.cuda.synchronize()
    assert bool((buf[0] == FILL).all()) and bool((buf[M + 1] == FILL).all()) and bool((buf[:, N:] == FILL).all()), "a guard row or column was written"
    return out, launches


def assert_crosses(launch, bm, bn, N, grid):
    """The launch's workgroups (their number and the tile order taken from the report) each compute three or more tiles, never two in a row in one column tile."""
    walk = ref.walks(-(-launch["rows"] // bm), -(-N // bn), grid, launch["rev"], launch["band"])
    assert len(walk) == grid and ref.crosses_column_tiles(walk), (launch, walk)


def graded(ops, kernel, shape, epilogue, families=ref.FAMILIES, S=1, expect=None, in_place=False, ldc_pad=8, call=None, cross=None, **route):
    """Run `epilogue` at `shape` on every family: route, guards, per-element grade (and exact equality on `integer`).  expect: (family, kt) of the one launch;
    cross: (BM, BN, workgroups) — assert that every workgroup of the launch changes column tile from each tile to the next."""
    M, N, K = shape
    act = ref.EPILOGUES[epilogue][1]
    for family in families:
        op, dev, pre = case(M, N, K, family, act == 1, ldc_pad)
        want, tol = ref.reference(op, epilogue, S=S, device="cuda", pre=pre)
        got, launches = run(ops, dev, epilogue, in_place, ldc_pad, call, **route)
        if expect is not None:
            assert launches == [dict(family=expect[0], kt=expect[1], rows=M, rev=launches[0]["rev"], band=launches[0]["band"])], launches
        if cross is not None:
            assert_crosses(launches[0], cross[0], cross[1], N, cross[2])
        ratio = ref.grade(got, want, tol)
        print(f"{kernel} {epilogue} {family} M={M} N={N} K={K}{' in place' if in_place else ''}: {ratio:.3f} of the bound")
        observe(f"gemm forward {kernel}, {epilogue}: |got - float64| / derived tolerance", ratio, 1.0)
        assert ratio <= 1.0, (kernel, epilogue, family, ratio)
        if family == "integer" and act != 1:
            assert torch.equal(got.cpu(), ref.integer_exact(op, epilogue)), (kernel, epilogue)
        if family == "large" and act != 1:
            assert bool(torch.isinf(got).any()) and bool(torch.isfinite(got).any())              # both sides of the overflow boundary were produced


# ---- the five persistent configurations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", list(ref.EPILOGUES))
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("cfg", list(ref.PERSISTENT))
def test_persistent_kernel(ops, cfg, tail, epilogue):
    (bm, bn), plain, ragged = ref.PERSISTENT[cfg]
    M, N, K = shape = ragged if tail else plain
    if tail and epilogue == "bn_res_relu":
        N = ref.TAIL_N_ACT5[cfg]                                     # N % 64 == 0: ragged against the 128- and 256-column tiles only
        shape = (M, N, K)
    slots = CUS * (2 if cfg in (0, 4) else 1)
    tiles = -(-M // bm) * -(-N // bn)
    assert tiles >= 3 * slots and -(-N // bn) in (3, 6) and M % bm == 1 and (K % 64 != 0) == tail and (not tail or N % bn or epilogue == "bn_res_relu")
    name = f"persistent {bm}x{bn}" + (" tail" if tail else "")
    graded(ops, name, shape, epilogue, expect=(f"cfg{cfg}", tail), cross=(bm, bn, slots), cfg=cfg, use4w=0)
    graded(ops, name, shape, epilogue, families=("normal", "integer"), expect=(f"cfg{cfg}", tail), cross=(bm, bn, slots), cfg=cfg, use4w=0, rev=0)      # ascending
    if epilogue == "res":
        graded(ops, name, shape, epilogue, families=("normal", "integer"), expect=(f"cfg{cfg}", tail), cross=(bm, bn, slots), in_place=True, cfg=cfg, use4w=0)


@pytest.mark.parametrize("K", ref.PERSISTENT_KS)
@pytest.mark.parametrize("cfg", [0, 2])
def test_persistent_kernel_k_tile_counts(ops, cfg, K):
    """1, 2 and 4 K-tiles with three or four tiles per workgroup across column tiles: one K-tile has a wait and a barrier of its own, because no K-loop barrier
    stands between the copy of the next tile's strip and its use."""
    (bm, bn), (M, N, _), _ = ref.PERSISTENT[cfg]
    slots = CUS * (2 if cfg == 0 else 1)
    for epilogue, in_place in (("bias", False), ("bias_gelu", False), ("res", True), ("bn_relu", False), ("bn_res_relu", False)):
        graded(ops, f"persistent {bm}x{bn}", (M, N, K), epilogue, families=("normal", "cancel", "integer"), expect=(f"cfg{cfg}", False), cross=(bm, bn, slots),
               in_place=in_place, cfg=cfg, use4w=0)


@pytest.mark.parametrize("cfg", list(ref.PERSISTENT))
def test_persistent_kernel_row_edges(ops, cfg):
    """M in {1, BM - 1, BM, BM + 1}: a lone row, a block one row short, a full block, a full block and a lone row."""
    (bm, bn), (_, N, K), (_, Nt, Kt) = ref.PERSISTENT[cfg]
    for M in (1, bm - 1, bm, bm + 1):
        for epilogue in ("bias_gelu", "res", "bn_res_relu"):
            graded(ops, f"persistent {bm}x{bn}", (M, N, K), epilogue, families=("normal", "integer"), expect=(f"cfg{cfg}", False), cfg=cfg, use4w=0)
            graded(ops, f"persistent {bm}x{bn} tail", (M, ref.TAIL_N_ACT5[cfg] if epilogue == "bn_res_relu" else Nt, Kt), epilogue, families=("normal",),
                   expect=(f"cfg{cfg}", True), cfg=cfg, use4w=0)


# ---- the ring kernel (S == 1) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", list(ref.EPILOGUES))
@pytest.mark.parametrize("tail", [False, True])
def test_ring_kernel(ops, tail, epilogue):
    shape = ref.RING[tail]
    if tail and epilogue == "bn_res_relu":
        shape = (shape[0], ref.TAIL_N_ACT5["ring"], shape[2])
    name = "ring" + (" tail" if tail else "")
    graded(ops, name, shape, epilogue, expect=("ring", tail), cfg=ops.ROUTE_RING)
    if epilogue == "res":
        graded(ops, name, shape, epilogue, families=("normal", "integer"), expect=("ring", tail), in_place=True, cfg=ops.ROUTE_RING)


@pytest.mark.parametrize("K", ref.RING_KS)
def test_ring_kernel_every_k_tile_count(ops, K):
    """1 to 9 K-tiles on the four-slot ring and the three tails, forced and as the cost model's own choice for a call with no more tiles than `cus`."""
    tail = K % 64 != 0
    for epilogue in ("bias", "bn_res_relu"):
        graded(ops, "ring" + (" tail" if tail else ""), (300, 168 if tail and epilogue == "bias" else 192, K), epilogue, families=("normal", "cancel", "integer"),
               expect=("ring", tail), cfg=ops.ROUTE_RING)
    graded(ops, "ring" + (" tail" if tail else ""), (129, 104 if tail else 128, K), "bias_gelu", families=("normal",), expect=("ring", tail), cfg=ops.ROUTE_AUTO)


# ---- the four-wave kernel and the eight-wave 256 x 256 kernel it replaces -------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", LINEAR)
@pytest.mark.parametrize("use4w", [1, 2])
def test_four_wave_kernel(ops, use4w, epilogue):
    name = "four-wave" + (" race-stress" if use4w == 2 else "")
    graded(ops, name, ref.FOUR_WAVE, epilogue, expect=("four_wave", False), cross=(256, 256, CUS), cfg=2, use4w=use4w)
    graded(ops, name, ref.FOUR_WAVE, epilogue, families=("normal", "integer"), expect=("four_wave", False), cross=(256, 256, CUS), cfg=2, use4w=use4w, rev=0)
    if epilogue == "res":
        graded(ops, name, ref.FOUR_WAVE, epilogue, families=("normal", "integer"), expect=("four_wave", False), cross=(256, 256, CUS), in_place=True, cfg=2,
               use4w=use4w)


@pytest.mark.parametrize("K", ref.FOUR_WAVE_KS)
def test_four_wave_kernel_every_k_tile_count(ops, K):
    """3 to 8 K-tiles on the five-slot ring, 15 tiles on 4 workgroups, each tile in another column tile than the one before: the ring phase and the next tile's
    descriptors and bias fragment carried from tile to tile."""
    M, N, _ = ref.FOUR_WAVE
    for epilogue, in_place in (("bias_gelu", False), ("res", True)):
        graded(ops, "four-wave", (M, N, K), epilogue, families=("normal", "cancel", "integer"), expect=("four_wave", False), cross=(256, 256, CUS),
               in_place=in_place, cfg=2, use4w=1)


@pytest.mark.parametrize("var", [0, 1])
def test_four_wave_product_entry(ops, var):
    """ops.gemm4w (pclip_gemm4w_var_f16) with the device's own CU count: var 0 and the race-stress var 1."""
    for epilogue in ("bias_gelu", "res"):
        graded(ops, "four-wave entry" + (" race-stress" if var else ""), ref.FOUR_WAVE, epilogue, families=("normal", "large", "integer"),
               call=lambda a, w, **kw: ops.gemm4w(a, w, var=var, **kw))


@pytest.mark.parametrize("epilogue", ["gelu", "bias_gelu"])
def test_eight_wave_four_slab_quickgelu_epilogue(ops, epilogue):
    """256 x 256 tiles on eight waves stage QuickGELU as a four-slab pipeline (pgemm::epilogue_pipe), full and ragged row blocks alike; graded, and bit for bit
    the two-slab epilogue of the 128 x 128 tiles."""
    (_, shape, _) = ref.PERSISTENT[2]
    graded(ops, "persistent 256x256 four-slab", shape, epilogue, expect=("cfg2", False), cross=(256, 256, CUS), cfg=2, use4w=0)
    for family in ("normal", "large"):
        _, dev, _ = case(*shape, family, True)
        big, lb = run(ops, dev, epilogue, cfg=2, use4w=0)
        small, ls = run(ops, dev, epilogue, cfg=0)
        assert (lb[0]["family"], ls[0]["family"]) == ("cfg2", "cfg0")
        assert torch.equal(big.view(torch.int16), small.view(torch.int16))


# ---- the generic kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", list(ref.EPILOGUES)[:7])
def test_generic_kernel(ops, epilogue):
    graded(ops, "generic", ref.GENERIC[0], epilogue, expect=("generic", False), cfg=ops.ROUTE_GENERIC)
    graded(ops, "generic tail", ref.GENERIC[1], epilogue, expect=("generic", True), cfg=ops.ROUTE_AUTO)                     # N % 8 != 0 with a K-tail
    graded(ops, "generic", ref.GENERIC[0], epilogue, families=("normal", "integer"), expect=("generic", False), ldc_pad=3, cfg=ops.ROUTE_AUTO)      # odd ldc
    if epilogue == "res":                                                                                                   # the residual stream updated in place
        graded(ops, "generic", ref.GENERIC[0], epilogue, families=("normal", "integer"), expect=("generic", False), in_place=True, cfg=ops.ROUTE_GENERIC)
        graded(ops, "generic tail", ref.GENERIC[1], epilogue, families=("normal", "integer"), expect=("generic", True), in_place=True, cfg=ops.ROUTE_AUTO)


# ---- split-K -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", LINEAR[:4])
@pytest.mark.parametrize("which", [0, 1])
def test_splitk(ops, which, epilogue):
    M, N, K = shape = ref.SPLITK[which]
    S, per = ref.splitk_slices(K)
    assert S == (4, 8)[which] and (which == 0 or K // 64 - (S - 1) * per == 1)                       # S = 8: a last slice of one K-tile
    lib = ops._lib.load()
    need = lib.pclip_gemm_splitk_workspace(M, N, K)
    assert need == S * M * N * 4                                                                      # the product entry cuts K as the reference assumes
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(a, w, bias, act, residual, out):
        """pclip_gemm_splitk_f16 itself (ops.gemm would fall back to pclip_gemm_f16 on a stride or alignment it does not like): an error if it cannot split."""
        before = lib.pclip_gemm_kernel_launches()
        ops.check(lib.pclip_gemm_splitk_f16(ops.ptr(a), a.stride(0), ops.ptr(w), w.stride(0), ops.ptr(out), out.stride(0), M, N, K, ops.ptr(bias), act,
                                            ops.ptr(ws), need, ops.stream()), "pclip_gemm_splitk_f16")
        assert residual is None and lib.pclip_gemm_kernel_launches() == before                        # nothing went through pclip_gemm_f16's dispatch
    graded(ops, f"split-K S={S}", shape, epilogue, S=S, call=call)

    def through_ops(a, w, **kw):                                                                      # ... and the route ops.gemm takes under low_latency()
        before = lib.pclip_gemm_kernel_launches()
        with ops.low_latency():
            assert ops.splitk_active(M)
            ops.gemm(a, w, **kw)
        assert lib.pclip_gemm_kernel_launches() == before
    graded(ops, f"split-K S={S}", shape, epilogue, families=("normal",), S=S, call=through_ops)


# ---- row split and tile orders -----------------------------------------------------------------------------------------------------------------------------
def test_row_split_under_a_small_cu_count(ops):
    """The dispatch cuts 1300 rows into 1280 (15 tiles of 256 x 256 over three column tiles: the full rounds on 4 workgroups, each changing column tile from tile
    to tile) and 20 (128 x 128 tiles): graded, exact on integers row for row, the residual updated in place across the cut."""
    M, N, K = ref.ROW_SPLIT
    for epilogue, in_place in (("bias", False), ("res", True), ("bn_res_relu", False)):
        for family in ("normal", "integer"):
            op, dev, pre = case(M, N, K, family)
            want, tol = ref.reference(op, epilogue, device="cuda", pre=pre)
            got, launches = run(ops, dev, epilogue, in_place, cfg=ops.ROUTE_AUTO, may_split=True)
            assert [(l["family"], l["rows"]) for l in launches] == [("cfg2" if epilogue == "bn_res_relu" else "four_wave", 1280), ("cfg0", 20)], launches
            assert_crosses(launches[0], 256, 256, N, CUS)
            ratio = ref.grade(got, want, tol)
            observe(f"gemm forward row split, {epilogue}: |got - float64| / derived tolerance", ratio, 1.0)
            assert ratio <= 1.0, (epilogue, family, ratio)
            if family == "integer":
                assert torch.equal(got.cpu(), ref.integer_exact(op, epilogue))
            one, l1 = run(ops, dev, epilogue, in_place, cfg=ops.ROUTE_AUTO, may_split=False)
            assert len(l1) == 1 and torch.equal(one.view(torch.int16), got.view(torch.int16))


def test_tile_orders(ops):
    """Bands of column tiles (a ragged last band) and the descending order, on the eight-wave kernel (8 column tiles of 128) and the four-wave kernel (band_n:
    3 column tiles in bands of 2): graded, the order asserted from the report, the same bits as the default order."""
    for shape, route, orders in (((400, 1024, 192), dict(cfg=0), (dict(band=3, rev=0), dict(band=0, rev=1), dict(band=0, rev=2))),
                                 ((1537, 768, 192), dict(cfg=2, use4w=1), (dict(band_n=2, rev=0), dict(band_n=2, rev=1), dict(band_n=0, rev=1)))):
        family = "four_wave" if route["cfg"] == 2 else "cfg0"
        _, dev, _ = case(*shape, "normal")
        base, l0 = run(ops, dev, "bias_gelu", rev=0, **route)
        assert (l0[0]["family"], l0[0]["rev"], l0[0]["band"]) == (family, False, 0)
        for order in orders:
            graded(ops, f"tile order {family}", shape, "bias_gelu", families=("normal",), expect=(family, False), **route, **order)
            got, l = run(ops, dev, "bias_gelu", **route, **order)
            assert (l[0]["rev"], l[0]["band"]) == (order["rev"] != 0, order.get("band", 0) or order.get("band_n", 0)), l
            assert torch.equal(got.view(torch.int16), base.view(torch.int16)), order


# ---- ops.bn_act: the anchor of the fused-against-separate identities ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", ref.BN_ACT)
def test_bn_act(ops, R, C):
    g = torch.Generator().manual_seed(R + C)
    for scale_x in (1.0, 2.0 ** -15, 3e4):                                # ordinary values, fp16 subnormals, both sides of the overflow boundary
        x = (scale_x * torch.randn(R, C, generator=g)).clamp(-65504, 65504).half().cuda()
        res = (scale_x * torch.randn(R, C, generator=g)).half().cuda() if scale_x < 3e4 else torch.randint(-4, 5, (R, C), generator=g).half().cuda()
        sc = (1 + 0.3 * torch.randn(C, generator=g)).cuda() if scale_x < 3e4 else (1 + torch.randint(0, 5, (C,), generator=g).float() / 64).cuda()
        sh = (0.2 * scale_x * torch.randn(C, generator=g)).cuda() if scale_x < 3e4 else torch.randint(-4, 5, (C,), generator=g).float().cuda()
        for residual in (None, res):
            for relu in (True, False):
                want, tol = ref.bn_act_reference(x, sc, sh, residual, relu)
                ratio = ref.grade(ops.bn_act(x, sc, sh, residual=residual, relu=relu), want, tol)
                observe(f"bn_act{' + residual' if residual is not None else ''}: |got - float64| / derived tolerance", ratio, 1.0)
                assert ratio <= 1.0, (scale_x, residual is not None, relu, ratio)
