"""The tolerance of the forward GEMMs (tests/gemm_fwd_ref.py) checked without a GPU, at the shapes tests/test_gpu_gemm_forward.py grades the kernels at: an fp32
emulation of the documented chain stays inside it for every epilogue, input family and summation order, with and without fused operations; every wrong kernel
lands outside it on the families that reach it; the `large` family leaves fewer than 1 % of its elements in the band where a finite result and an infinity are
both accepted."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fwd_ref as ref                                          # noqa: E402
from conftest import observe                                        # noqa: E402

SHAPES = ref.main_shapes()
UNDECIDED_CAP = 0.01
_cache = {}


def case(name, family, gelu=False):
    """Operands, float64 products and the fp32 accumulators of every order (with and without bias) of a case, computed once.  gelu: `large` has a draw of its
    own for the QuickGELU epilogues."""
    key = (name, family, gelu and family == "large")
    if key not in _cache:
        (M, N, K), S, _ = SHAPES[name]
        op = ref.operands(family, M, N, K, seed=100 + K + N, epilogue="gelu" if key[2] else "bias")
        orders = ref.ORDERS if S == 1 else (("asc", 64),)
        accs = {(b, o): ref.accumulate(op, b, o, S) for b in (False, True) for o in orders}
        _cache.clear()                                              # one case at a time: the accumulators of the largest shape are 40 MB
        _cache[key] = (op, ref.products(op), accs)
    return _cache[key]


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bound_holds_the_documented_roundings(name, family):
    _, S, epilogues = SHAPES[name]
    for epi in epilogues:
        has_bias, act = ref.EPILOGUES[epi]
        op, pre, accs = case(name, family, act == 1)
        want, tol = ref.reference(op, epi, S=S, pre=pre)
        worst = 0.0
        for (b, order), acc in accs.items():
            if b != has_bias:
                continue
            for fma in (True, False):
                worst = max(worst, ref.grade(ref.emulate(op, epi, order, fma, S=S, acc=acc), want, tol))
        print(f"{name} {family} {epi}: emulation at {worst:.3f} of the bound")
        observe(f"gemm forward emulation, {epi}, {family}: |emu - float64| / derived tolerance", worst, 1.0)
        assert worst <= 1.0, (epi, worst)
        if family == "integer" and act != 1:
            assert torch.equal(ref.emulate(op, epi, S=S, acc=accs[(has_bias, ("asc", 64))]).half(), ref.integer_exact(op, epi)), epi
        if family == "large":
            share = ref.undecided_share(want, tol)
            print(f"{name} large {epi}: {100 * share:.3f} % of the elements undecided between finite and infinite")
            observe(f"gemm forward, large family, {epi}: undecided share", share, UNDECIDED_CAP)
            assert share < UNDECIDED_CAP, (epi, share)
            if act in (0, 6, 2):
                assert bool((want.abs() - tol > ref.F16_EDGE).any()) and bool((want.abs() + tol < ref.F16_EDGE).any())     # both sides of the boundary occur
            if act == 1:
                z = pre[0] + (op["bias"].double() if has_bias else 0)
                assert float(z.min()) < -38500 and float(z.min()) > -64000 and float(z.max()) > ref.F16_EDGE      # t overflows on both sides, h on the positive one only


# The families on which a wrong kernel differs from the right one by more than the kernel's own roundings:
#   bias_after_round        needs results with bits below the bias's last place: `integer` is exact either way, in `tiny` both are multiples of 2^-24, `cancel`'s
#                           tolerance is its accumulation term, `large`'s bias is a tenth of its ulp
#   round_between_ktiles    needs two K-tiles and a rounding that loses bits: not `integer`
#   residual_neighbour_row  `large` keeps |res| <= 4 under a tolerance of 60 (it has to: docstring of gemm_fwd_ref, OVERFLOW)
#   relu_before_residual    needs a negative BatchNorm value under a residual: not `large` (its negative rows stay negative)
#   gelu_nan                needs t to overflow: `large` only
REACH = {
    "drop_tail_chunk": ref.FAMILIES,
    "bias_after_round": ("normal", "subnormal"),
    "round_between_ktiles": ("normal", "cancel", "large", "tiny", "subnormal"),
    "slab_twice": ref.FAMILIES,
    "slab_dropped": ref.FAMILIES,
    "stale_strip": ref.FAMILIES,
    "residual_neighbour_row": ("normal", "cancel", "tiny", "subnormal", "integer"),
    "relu_before_residual": ("normal", "cancel", "tiny", "subnormal", "integer"),
    "gelu_nan": ("large",),
}


def wrong_kernels(name):
    """(variant, epilogue, bn_tile) that exist on a shape."""
    (M, N, K), S, epilogues = SHAPES[name]
    out = []
    if S > 1:
        return [("slab_twice", "bias", 0), ("slab_dropped", "bias", 0), ("slab_twice", "bias_gelu", 0)]
    if K % 64 and "bias" in epilogues:
        out.append(("drop_tail_chunk", "bias", 0))
    if "bias" in epilogues:
        out += [("bias_after_round", "bias", 0), ("bias_after_round", "res", 0), ("residual_neighbour_row", "res", 0), ("gelu_nan", "bias_gelu", 0)]
    if K > 64 and "bias" in epilogues:
        out.append(("round_between_ktiles", "bias", 0))
    if "bn_res_relu" in epilogues:
        out += [("residual_neighbour_row", "bn_res_relu", 0), ("relu_before_residual", "bn_res_relu", 0)]
    bn = {"cfg0": 128, "cfg1": 128, "cfg2": 256, "cfg3": 64, "cfg4": 32}.get(name[:4], 64)
    out += [("stale_strip", e, bn) for e in ("bn", "bn_res_relu") if e in epilogues and N > bn]
    return out


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_bound_rejects_wrong_kernels(name, family):
    _, S, _ = SHAPES[name]
    for variant, epi, bn_tile in wrong_kernels(name):
        if family not in REACH[variant]:
            continue
        op, pre, _ = case(name, family, ref.EPILOGUES[epi][1] == 1)
        want, tol = ref.reference(op, epi, S=S, pre=pre)
        ratio = ref.grade(ref.emulate(op, epi, S=S, variant=variant, bn_tile=bn_tile), want, tol)
        print(f"{name} {family} {epi} {variant}: {ratio:.2f} x the bound")
        assert ratio > 1.0, (variant, epi, ratio)


def test_every_wrong_kernel_is_reached():
    """REACH and `wrong_kernels` must not hollow the test: every wrong kernel of the list is rejected on at least one shape and family."""
    seen = {v for name in SHAPES for v, _, _ in wrong_kernels(name)}
    assert seen == set(ref.VARIANTS) and all(REACH[v] for v in ref.VARIANTS)


@pytest.mark.parametrize("K", ref.RING_KS + ref.FOUR_WAVE_KS)
def test_bound_holds_at_every_k_tile_count(K):
    """The K sweeps of the ring kernels (1 to 9 K-tiles and the three tails): the accumulation term follows K."""
    M, N = 150, 128
    for family in ("normal", "cancel"):
        op = ref.operands(family, M, N, K, seed=K)
        want, tol = ref.reference(op, "bias")
        worst = max(ref.grade(ref.emulate(op, "bias", order), want, tol) for order in ref.ORDERS)
        observe(f"gemm forward emulation, bias, {family}: |emu - float64| / derived tolerance", worst, 1.0)
        assert worst <= 1.0, (family, worst)


def test_route_entry_validates_before_any_launch():
    """pclip_gemm_route_f16 refuses what the product entries refuse, and a route that does not exist, before it touches the GPU (pointers never dereferenced)."""
    import ctypes
    from proto_clip_amd import _lib
    lib = _lib.load()
    buf, rep = ctypes.c_void_p(0x1000), (ctypes.c_int * 41)()

    def call(M=4, N=64, K=64, lda=64, ldb=64, ldc=64, bias=None, act=0, res=None, sc=None, sh=None, cfg=-1, use4w=1, cus=4, report=rep, n=41, rev=2):
        return lib.pclip_gemm_route_f16(buf, lda, buf, ldb, buf, ldc, M, N, K, bias, act, res, sc, sh, cfg, 1, 0, 0, rev, use4w, cus, report, n, None)
    assert call(K=100) == -1 and b"multiple of 8" in lib.pclip_last_error()
    assert call(lda=32) == -1 and call(ldc=32) == -1
    assert call(act=4) == -1 and call(act=7) == -1 and call(cfg=7) == -1 and call(cfg=-2) == -1 and call(use4w=3) == -1 and call(cus=0) == -1 and call(rev=3) == -1
    assert call(act=2) == -1 and call(act=3, sc=buf, sh=buf, bias=buf) == -1 and call(sc=buf, sh=buf) == -1          # BatchNorm takes scale and shift, no bias
    assert call(act=5, sc=buf, sh=buf) == -1 and call(act=5, sc=buf, sh=buf, res=buf, N=72, ldc=72) == -1              # act 5: residual, N % 64 == 0
    assert call(act=1, bias=buf, res=buf) == -1 and call(report=None) == -1 and call(n=0) == -1
    rep[0] = 99
    assert call(M=0) == 0 and rep[0] == 0                                                                              # no rows: no launch, an empty report


def test_graded_walks_change_column_tile():
    """The shapes put every persistent workgroup on three or more tiles, no two consecutive ones in one column tile, in both tile orders — and the check itself
    tells: with TWO column tiles on 4 or 8 workgroups every workgroup stays in one column for its whole walk."""
    for cfg, ((bm, bn), plain, tail) in ref.PERSISTENT.items():
        grid = ref.CUS * (2 if cfg in (0, 4) else 1)
        for M, N, _ in (plain, tail, (tail[0], ref.TAIL_N_ACT5[cfg], tail[2])):
            for rev in (False, True):
                assert ref.crosses_column_tiles(ref.walks(-(-M // bm), -(-N // bn), grid, rev)), (cfg, M, N, rev)
                stuck = ref.walks(-(-M // bm) * 2, 2, grid, rev)
                assert not ref.crosses_column_tiles(stuck) and all(len({tn for _, tn in w}) == 1 for w in stuck)
    M, N, _ = ref.FOUR_WAVE
    assert ref.crosses_column_tiles(ref.walks(-(-M // 256), N // 256, ref.CUS, True))
    assert [ref.xcd_remap(b, 20) for b in range(20)] == [0, 3, 6, 9, 12, 14, 16, 18, 1, 4, 7, 10, 13, 15, 17, 19, 2, 5, 8, 11]      # 20 = 8 x 2 + 4
    assert ref.walks(2, 3, 1, False, 2)[0] == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (1, 2)]                                      # bands of two column tiles


def test_route_constants_mirror_the_header():
    import re
    from proto_clip_amd import _lib
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pclip.h")).read()
    h = {k: int(v.strip("()")) for k, v in re.findall(r"#define PCLIP_ROUTE_(\w+) (\(?-?\d+\)?)", txt)}
    assert (h["AUTO"], h["GENERIC"], h["RING"], h["FIELDS"]) == (_lib.ROUTE_AUTO, _lib.ROUTE_GENERIC, _lib.ROUTE_RING, _lib.ROUTE_FIELDS)
    assert {h["RAN_FOUR_WAVE"]: "four_wave", h["RAN_RING"]: "ring", h["RAN_GENERIC"]: "generic"}.items() <= _lib.ROUTE_RAN.items()
    assert not set(_lib.ROUTE_RAN) - set(range(5)) & {h["GENERIC"], h["RING"]}                          # what ran is numbered apart from what to run
