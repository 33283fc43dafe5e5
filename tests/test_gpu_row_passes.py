"""The forward row passes graded per element against float64 (tests/row_passes_ref.py: the reference, the derived tolerance, the families): the three routes of
pclip_layernorm_f16, add_layernorm, both routes of vit_embed_ln, the fp16-affine blend with its row normalise and sq_out, l2norm_rows, row_sqnorm, the two pools,
and — bit for bit — the token assembly, the text embedding and the EOT gather.

Every case: worst |got - float64| / tolerance <= 1 (recorded per kernel and route, and printed per width and family as a LEDGER line: profiles/row_passes_ledger.txt
is made from those), the route asserted from the row count against the CU count the library reports (pclip_device_cus: a case that claims a kernel cannot silently
take another), inputs strided where the entry allows it (NaN in the padding), and the output inside a buffer with a guard row on either side that must keep its fill.

Shapes are the smallest that reach what can go wrong:
  widths       8 (one lane), 64, 520 / 1032 / 2056 (a last chunk of 8 columns behind 1, 2 and 4 full ones: the `d < D` guards), 768, 776, 2048, 4096 (NCH = 8)
  small kernel R in {1, 3, 4, 5, 23}: a workgroup holds 4 rows
  prefetching  R = 65 543 (> 4 x 16 384 waves: the row loop iterates, rows r and r + 65 536 take their own statistics), only while that is below 512 x CUs
  LDS route    R = 512 x CUs + 5 (>= 16 rows per workgroup of the resident grid); widths that are no multiple of 256 exercise the plane layout's `i < D`
Whole-batch inputs are a block of 102 rows (17 of every family) repeated: 102 divides neither 32 768 nor 65 536, so rows r and r + stride differ in family.  Their
float64 reference is computed on the GPU in slabs of rows (temporaries below 1 GB)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_passes_ref as ref                                        # noqa: E402
from conftest import observe                                        # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 777.0
SLAB_ELEMS = 1 << 22                                                # elements per float64 temporary: 32 MB each, a few dozen alive in ln_parts
BLOCK = 102                                                         # rows of a repeated block: a multiple of 6, no divisor of a grid's row stride
PF_ROWS = 65536 + 7                                                 # 65 537 + 6: every family in the second iteration of the row loop
F6 = ref.FAMILIES


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from proto_clip_amd import _lib
    return _lib


def record(kernel, route, D, fam, ratio):
    print(f"LEDGER {kernel} | {route} | D={D} | {fam} | {ratio:.3f}")
    observe(f"row passes {kernel}, {route}: |got - float64| / derived tolerance", ratio, 1.0)
    assert ratio <= 1.0, (kernel, route, D, fam, ratio)


def padded(t, pad=8, fill=float("nan")):
    """A [R, C] device view with row stride C + pad; the padding holds `fill`."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def guarded(R, D, dtype=torch.float16):
    """(buffer [R + 2, D] filled with FILL, its rows 1 .. R): the output goes into the middle."""
    buf = torch.full((R + 2, D), FILL, dtype=dtype, device="cuda")
    return buf, buf[1:R + 1]


def guards_intact(buf):
    torch.cuda.synchronize()
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


def rotations(R):
    """Family orders for a call of R rows: fewer than six rows take six calls, each family once in every row position."""
    return [F6[k:] + F6[:k] for k in range(6 if R < 6 else 1)]


def grade_ln(x16, gamma, beta, got, families=F6, eps=1e-5):
    """family -> worst ratio of `got` against the LayerNorm of the device rows `x16` (any row stride), float64 in slabs of rows."""
    R, D = got.shape
    slab = max(6, SLAB_ELEMS // D // 6 * 6)
    worst = {}
    for r0 in range(0, R, slab):
        want, tol = ref.ln_reference(x16[r0:r0 + slab], gamma, beta, eps)
        assert ref.undecided_share(want, tol) == 0.0
        for fam, ratio in ref.by_family(got[r0:r0 + slab], want, tol, want.shape[0], families).items():
            worst[fam] = max(worst.get(fam, 0.0), ratio)
    return worst


def repeated(base, R):
    """[R, D] on the device: the CPU block `base` repeated."""
    b = base.cuda()
    return b.repeat(-(-R // b.shape[0]), 1)[:R].contiguous()


def ln_route(R, cus):
    """The kernel pclip_layernorm_f16 takes (csrc/pclip_layernorm.hip): whole batches the LDS form, more rows than waves of the grid the prefetching one."""
    return "lds" if cus > 0 and R >= 512 * cus else "prefetch" if R > 4 * 16384 else "small"


def r16_sum_dev(a16, b16):
    """r16(a + b) on the device: the fp32 sum of two fp16 values rounded to fp16 IS the correctly rounded sum (test_row_passes_cpu.py::test_exact_sums_round_once)."""
    return (a16.float() + b16.float()).half()


# ---- layernorm: the small-batch kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (8, 64, 520, 768, 1032, 2048, 2056, 4096))
def test_layernorm_small(ops, lib, D):
    cus = lib.load().pclip_device_cus()
    gamma, beta = (t.cuda() for t in ref.affine(D, seed=D))
    for R in (1, 3, 4, 5, 23):
        assert ln_route(R, cus) == "small"
        for fams in rotations(R):
            x = padded(ref.rows(R, D, seed=1000 + R + D, families=fams))
            buf, out = guarded(R, D)
            ops.layernorm(x, gamma, beta, out=out, rows=R, ld=D + 8)
            assert guards_intact(buf), "a guard row was written"
            for fam, ratio in grade_ln(x, gamma, beta, out, fams).items():
                record("layernorm", f"small R={R} ld=D+8", D, fam, ratio)
    # the strided CLS-row form: every L-th row of a contiguous [R, D]
    R, L = 35, 5                                                    # 5 and 6 are coprime: the seven rows of the call cover every family
    x = ref.rows(R, D, seed=77 + D).cuda()
    buf, out = guarded(R // L, D)
    ops.layernorm(x, gamma, beta, out=out, rows=R // L, ld=L * D)
    assert guards_intact(buf)
    fams = tuple(F6[(L * i) % 6] for i in range(6))                 # row i of the call is row L i of x
    for fam, ratio in grade_ln(x[:R // L * L:L], gamma, beta, out, fams).items():
        record("layernorm", "small rows=R/L ld=L D", D, fam, ratio)


# ---- layernorm: the two whole-batch routes --------------------------------------------------------------------------------------------------------------------
def whole_batch(ops, D, R, route):
    gamma, beta = (t.cuda() for t in ref.affine(D, seed=D))
    base = ref.rows(BLOCK, D, seed=500 + D)
    xb = torch.full((R, D + 8), float("nan"), dtype=torch.float16, device="cuda")
    x = xb[:, :D]
    x.copy_(repeated(base, R))
    buf, out = guarded(R, D)
    ops.layernorm(x, gamma, beta, out=out, rows=R, ld=D + 8)
    assert guards_intact(buf), "a guard row was written"
    for fam, ratio in grade_ln(x, gamma, beta, out).items():
        record("layernorm", route, D, fam, ratio)
    # one row alone (the small kernel) has the bits of the row in the batch, the last row included
    for r in (0, R - 1):
        assert torch.equal(ops.layernorm(x[r:r + 1], gamma, beta, rows=1, ld=D + 8), out[r:r + 1])


@pytest.mark.parametrize("D", (8, 520, 1032, 2056))
def test_layernorm_prefetch_route(ops, lib, D):
    cus = lib.load().pclip_device_cus()
    if not (cus > 0 and PF_ROWS < 512 * cus):
        pytest.skip(f"{PF_ROWS} rows take the LDS route on a device of {cus} CUs: the prefetching kernel without LDS cannot be reached")
    assert ln_route(PF_ROWS, cus) == "prefetch"
    whole_batch(ops, D, PF_ROWS, "prefetch")


@pytest.mark.parametrize("D", (8, 520, 776, 1024, 2056))
def test_layernorm_lds_route(ops, lib, D):
    cus = lib.load().pclip_device_cus()
    assert cus > 0, "the library does not know the CU count: the LDS route is never taken"
    R = 512 * cus + 5
    assert ln_route(R, cus) == "lds" and ln_route(R - 6, cus) != "lds"
    whole_batch(ops, D, R, "lds")


# ---- add_layernorm ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (8, 520, 1032, 4096))
def test_add_layernorm(ops, D):
    gamma, beta = (t.cuda() for t in ref.affine(D, seed=D + 1))
    for R in (1, 5, 23):
        for fams in rotations(R):
            x16, d16 = ref.rows(R, D, seed=2000 + R + D, families=fams), ref.rows(R, D, seed=3000 + R + D, families=fams[1:] + fams[:1])
            xs = ref.r16_sum(x16, d16)
            assert bool(torch.isfinite(xs.float()).all())
            for pad in (0, 8):
                for update in (False, True):
                    x, delta = padded(x16, pad), padded(d16, pad)
                    buf, out = guarded(R, D)
                    ops.add_layernorm(x, delta, gamma, beta, out=out, update_x=update, rows=R, ld=D + pad)
                    assert guards_intact(buf), "a guard row was written"
                    assert torch.equal(x.cpu(), xs if update else x16), "xs = r16(x + delta) must be the correctly rounded sum (or x untouched)"
                    for fam, ratio in grade_ln(xs.cuda(), gamma, beta, out, fams).items():
                        record("add_layernorm", f"ld=D+{pad} update_x={update}", D, fam, ratio)
    # the strided row form: every L-th row, updated in place
    R, L = 35, 5                                                    # 5 and 6 are coprime: the seven rows of the call cover every family
    x16, d16 = ref.rows(R, D, seed=81 + D), ref.rows(R, D, seed=82 + D, families=("normal", "tiny"))
    x, delta = x16.cuda(), d16.cuda()
    buf, out = guarded(R // L, D)
    ops.add_layernorm(x, delta, gamma, beta, out=out, update_x=True, rows=R // L, ld=L * D)
    assert guards_intact(buf)
    xs = x16.clone()
    xs[:R // L * L:L] = ref.r16_sum(x16[:R // L * L:L], d16[:R // L * L:L])
    assert torch.equal(x.cpu(), xs), "only every L-th row is updated"
    fams = tuple(F6[(L * i) % 6] for i in range(6))
    for fam, ratio in grade_ln(xs[:R // L * L:L].cuda(), gamma, beta, out, fams).items():
        record("add_layernorm", "rows=R/L ld=L D update_x=True", D, fam, ratio)


# ---- vit_embed_ln -----------------------------------------------------------------------------------------------------------------------------------------------
def vit_embed_case(lib, B, G2, W, with_h, route):
    L = G2 + 1
    R = B * L
    g = torch.Generator().manual_seed(B + G2 + W)
    patch = repeated(ref.rows(min(BLOCK, B * G2), W, seed=600 + W), B * G2)
    cls, pos = torch.randn(W, generator=g).half().cuda(), (0.1 * torch.randn(L, W, generator=g)).half().cuda()
    (g0, b0), (g1, b1) = [[t.cuda() for t in ref.affine(W, seed=W + k)] for k in (2, 3)]
    buf0, x0 = guarded(R, W)
    buf1, h = guarded(R, W)
    lib.check(lib.load().pclip_vit_embed_ln_f16(lib.ptr(patch), lib.ptr(cls), lib.ptr(pos), B, G2, W, lib.ptr(g0), lib.ptr(b0), lib.ptr(g1), lib.ptr(b1), 1e-5,
                                                lib.ptr(x0), lib.ptr(h) if with_h else None, lib.stream()), "pclip_vit_embed_ln_f16")
    assert guards_intact(buf0) and guards_intact(buf1), "a guard row was written"
    if not with_h:
        assert bool((buf1 == FILL).all()), "h was written without being asked for"
    tok = torch.cat([cls.view(1, 1, W).expand(B, 1, W), patch.view(B, G2, W)], 1)
    tokens = r16_sum_dev(tok, pos.view(1, L, W).expand(B, L, W)).view(R, W)
    fams = ("tokens",)
    record("vit_embed_ln", f"{route} x0", W, "tokens", max(grade_ln(tokens, g0, b0, x0, fams).values()))
    if with_h:                                                      # against LN_1 of the x0 the kernel returned: an exact input
        record("vit_embed_ln", f"{route} h", W, "tokens", max(grade_ln(x0, g1, b1, h, fams).values()))
    return tokens


@pytest.mark.parametrize("with_h", (True, False))
@pytest.mark.parametrize("B,G2,W", ((1, 1, 8), (3, 4, 520), (2, 9, 1032), (2, 3, 2056)))
def test_vit_embed_ln_plain(ops, lib, B, G2, W, with_h):
    cus = lib.load().pclip_device_cus()
    assert not (cus > 0 and B * (G2 + 1) >= 512 * cus and W <= 1024)
    vit_embed_case(lib, B, G2, W, with_h, "plain")


@pytest.mark.parametrize("W", (8, 520, 1024))
def test_vit_embed_ln_lds_route(ops, lib, W):
    cus = lib.load().pclip_device_cus()
    assert cus > 0, "the library does not know the CU count: the LDS route is never taken"
    B, G2 = -(-512 * cus // 5) + 1, 4
    assert B * (G2 + 1) >= 512 * cus and W <= 1024 and (B - 2) * (G2 + 1) < 512 * cus      # the entry's own condition, and the smallest batch near it
    tokens = vit_embed_case(lib, B, G2, W, True, "lds")
    # the assembly on its own agrees bit for bit with the tokens the fused kernel normalised
    patch = repeated(ref.rows(min(BLOCK, B * G2), W, seed=600 + W), B * G2)
    g = torch.Generator().manual_seed(B + G2 + W)
    cls, pos = torch.randn(W, generator=g).half().cuda(), (0.1 * torch.randn(G2 + 1, W, generator=g)).half().cuda()
    assert torch.equal(ops.vit_assemble_tokens(patch, cls, pos, B, G2, W), tokens)


# ---- layernorm_blend --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2norm", (False, True))
@pytest.mark.parametrize("D", (8, 520, 1032, 4096))
def test_layernorm_blend(ops, D, l2norm):
    gamma, beta = ref.affine(D, seed=D + 4, half=True)
    for R in (1, 5):
        for ratio in (0.2, 1.0, 0.0):
            omr = ref.f32(1 - ratio)
            for fams in rotations(R):
                h16, res16 = ref.rows(R, D, seed=4000 + R + D, families=fams), ref.rows(R, D, seed=5000 + R + D, families=fams)
                want, tol, (lo, hi) = ref.blend_parts(h16, gamma, beta, res16, ratio, omr)
                buf, out = guarded(R, D)
                y, sq = ops.layernorm_blend(h16.cuda(), gamma.cuda(), beta.cuda(), res16.cuda(), ratio=ratio, l2norm_out=l2norm, want_sq=True, out=out)
                assert guards_intact(buf), "a guard row was written"
                y, sq = y.cpu(), sq.cpu()
                route = f"ratio={ratio}{' l2norm' if l2norm else ''} R={R}"
                if l2norm:
                    want, tol, zone = ref.norm_parts(want, tol)
                    assert bool((zone != 0).all()), "a row's norm is undecided between finite and infinite"
                    extra = ref.grade_zero_rows(y, zone)
                else:
                    extra = ref.grade_interval(y, lo, hi)
                    if ratio == 0.0:
                        assert torch.equal(y, res16)
                record("layernorm_blend", route + " sq_out", D, "all", ref.grade_sq(sq, y))
                record("layernorm_blend", route + (" zero rows" if l2norm else " interval"), D, "all", extra)
                for fam, r in ref.by_family(y, want, tol, R, fams).items():
                    record("layernorm_blend", route, D, fam, r)
    assert torch.equal(ops.layernorm_blend(h16.cuda(), gamma.cuda(), beta.cuda(), res16.cuda(), ratio=0.0, l2norm_out=l2norm), y.cuda())      # without want_sq: the same rows


# ---- l2norm_rows, row_sqnorm ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (8, 520, 1032, 2056, 4096))
def test_l2norm_rows_and_row_sqnorm(ops, D):
    x16 = ref.l2norm_rows_input(12, D, seed=60 + D)
    R = x16.shape[0]
    want, tol, zone = ref.norm_parts(x16.double(), torch.zeros(x16.shape, dtype=torch.float64))
    assert bool((zone != 0).all()) and int(zone[-1]) == 1 and int(zone[-2]) == -1      # the two edge rows: an infinite rounded norm, a subnormal one
    for in_place in (False, True):
        buf, out = guarded(R, D)
        x = x16.cuda()
        if in_place:
            out.copy_(x)
            x = out
        y, sq = ops.l2norm_rows(x, out=out, want_sq=True)
        assert guards_intact(buf), "a guard row was written"
        y, sq = y.cpu(), sq.cpu()
        how = "in place" if in_place else "out of place"
        record("l2norm_rows", how, D, "all + edge rows", ref.grade(y, want, tol))
        record("l2norm_rows", how + " zero rows", D, "norm > 65520", ref.grade_zero_rows(y, zone))
        record("l2norm_rows", how + " sq_out", D, "all + edge rows", ref.grade_sq(sq, y))
        assert bool((y[-1] == 0).all()) and bool((sq[-1] == 0).all())
    buf, sq = guarded(R, 1, torch.float32)
    from proto_clip_amd import _lib
    x = x16.cuda()
    _lib.check(_lib.load().pclip_row_sqnorm_f16(_lib.ptr(x), R, D, _lib.ptr(sq), _lib.stream()), "pclip_row_sqnorm_f16")
    assert guards_intact(buf)
    record("row_sqnorm", "-", D, "all + edge rows", ref.grade_sq(sq.view(R).cpu(), x16))
    assert torch.equal(ops.row_sqnorm(x), sq.view(R))


# ---- the pools --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C", ((1, 1, 8), (2, 49, 64), (3, 144, 2048)))
def test_attnpool_tokens(lib, B, HW, C):
    g = torch.Generator().manual_seed(HW + C)
    x16, pos16 = (0.3 + 2 * torch.randn(B * HW, C, generator=g)).half(), (0.5 * torch.randn(HW + 1, C, generator=g)).half()
    buf, out = guarded(B * (HW + 1), C)
    x, pos = x16.cuda(), pos16.cuda()
    lib.check(lib.load().pclip_attnpool_tokens_f16(lib.ptr(x), lib.ptr(pos), B, HW, C, lib.ptr(out), lib.stream()), "pclip_attnpool_tokens_f16")
    assert guards_intact(buf), "a guard row was written"
    want, tol, exact = ref.attnpool_reference(x16, pos16, B, HW, C)
    t = out.cpu().view(B, HW + 1, C)
    record("attnpool_tokens", f"HW={HW}", C, "normal", ref.grade(t[:, 0], want, tol))
    assert torch.equal(t[:, 1:], exact), "rows 1 .. HW are r16(x + pos): one rounding"


@pytest.mark.parametrize("k", (2, 3))
def test_avgpool_nhwc(lib, k):
    B, H, W, C = 2, 6, 12, 24
    g = torch.Generator().manual_seed(k)
    x16 = (0.3 + 2 * torch.randn(B * H * W, C, generator=g)).half()
    R = B * (H // k) * (W // k)
    buf, out = guarded(R, C)
    x = x16.cuda()
    lib.check(lib.load().pclip_avgpool_nhwc_f16(lib.ptr(x), B, H, W, C, k, lib.ptr(out), lib.stream()), "pclip_avgpool_nhwc_f16")
    assert guards_intact(buf), "a guard row was written"
    want, tol = ref.avgpool_reference(x16, B, H, W, C, k)
    record("avgpool_nhwc", f"k={k}", C, "normal", ref.grade(out.cpu(), want, tol))


# ---- the exact assembly kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (8, 520))
def test_vit_assemble_tokens_exact(lib, W):
    B, G2 = 3, 4
    patch16, cls16, pos16 = ref.rows(B * G2, W, seed=W), ref.rows(1, W, seed=W + 1)[0], ref.rows(G2 + 1, W, seed=W + 2, families=("normal", "tiny", "offset"))
    buf, out = guarded(B * (G2 + 1), W)
    patch, cls, pos = patch16.cuda(), cls16.cuda(), pos16.cuda()
    lib.check(lib.load().pclip_vit_assemble_tokens_f16(lib.ptr(patch), lib.ptr(cls), lib.ptr(pos), B, G2, W, lib.ptr(out), lib.stream()), "pclip_vit_assemble_tokens_f16")
    assert guards_intact(buf), "a guard row was written"
    assert torch.equal(out.cpu(), ref.assemble_reference(patch16, cls16, pos16, B, G2, W))


@pytest.mark.parametrize("W", (8, 520))
def test_text_embed_exact_and_clamped(lib, W):
    vocab, B, L = 24, 3, 7
    emb16, pos16 = ref.rows(vocab, W, seed=W + 5), ref.rows(L, W, seed=W + 6, families=("normal", "tiny", "offset"))
    g = torch.Generator().manual_seed(W)
    toks = torch.randint(0, vocab, (B, L), generator=g)
    toks[0, 0], toks[0, 1], toks[1, 2], toks[1, 3], toks[2, 4], toks[2, 5] = 0, vocab - 1, -1, -(2 ** 40), vocab, 2 ** 40      # both ends, and ids outside [0, vocab): clamped
    buf, out = guarded(B * L, W)
    t, emb, pos = toks.cuda(), emb16.cuda(), pos16.cuda()
    lib.check(lib.load().pclip_text_embed_f16(lib.ptr(t), lib.ptr(emb), lib.ptr(pos), B, L, W, vocab, lib.ptr(out), lib.stream()), "pclip_text_embed_f16")
    assert guards_intact(buf), "a guard row was written"
    want = ref.text_embed_reference(toks, emb16, pos16)
    assert torch.equal(out.cpu(), want)
    assert torch.equal(want.view(B, L, W)[1, 2], ref.r16_sum(emb16[0], pos16[2])) and torch.equal(want.view(B, L, W)[2, 5], ref.r16_sum(emb16[vocab - 1], pos16[5]))


def gather(lib, toks, W, seed):
    B, L = toks.shape
    x16 = torch.randn(B * L, W, generator=torch.Generator().manual_seed(seed)).half()
    buf, out = guarded(B, W)
    x, t = x16.cuda(), toks.cuda()
    lib.check(lib.load().pclip_gather_eot_f16(lib.ptr(x), lib.ptr(t), B, L, W, lib.ptr(out), lib.stream()), "pclip_gather_eot_f16")
    assert guards_intact(buf), "a guard row was written"
    return out.cpu(), x16.view(B, L, W)[torch.arange(B), torch.argmax(toks, dim=1)]


@pytest.mark.parametrize("W", (8, 520, 1024))
@pytest.mark.parametrize("L", (1, 6, 64, 65, 77, 130))
def test_gather_eot_is_argmax(lib, L, W):
    pats = ref.eot_patterns(L)
    toks = torch.stack(list(pats.values()))
    got, want = gather(lib, toks, W, L + W)
    for i, name in enumerate(pats):
        assert torch.equal(got[i], want[i]), (name, L, W, int(torch.argmax(toks[i])))


def test_gather_eot_all_negative_row(lib):
    """A row of negative ids selects its first maximum like torch.argmax (the kernel used to start from -1 and read row INT_MAX of x)."""
    for L in (1, 77, 130):
        toks = torch.stack([ref.eot_all_negative(L), ref.eot_patterns(L)["max_last"], ref.eot_all_negative(L, seed=1)])
        got, want = gather(lib, toks, 520, L)
        assert torch.equal(got, want), L
