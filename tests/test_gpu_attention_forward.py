"""The forward attention kernels graded per element against float64 (tests/attention_fwd_ref.py: the tolerance follows from the roundings attn_key_tiles /
attn_store_tile document) on every launch form of pclip_attention_q_f16 / pclip_attention_long_q_f16 and on inputs that drive the online-softmax state
machine — a maximum that moves on every pair of key tiles, one that creeps up under the deferral threshold, |S| of 87 and 213, one-hot and flat rows —
plus what a per-wave or per-item leak would break: a row's bits under a permutation of the rows of its wave, items next to a poisoned one, repeated calls."""
import pytest
import torch

import attention_fwd_ref as ref
from conftest import observe

pytestmark = pytest.mark.gpu

B, H = 2, 3
W = H * 64
# (form, L, causal, Lq): the launch is chosen by the shape alone (pclip_attention_q_f16; L > 288: pclip_attention_long_q_f16)
FORMS = ([("four-wave query-first", L, False, None) for L in (1, 31, 32, 33, 64, 65, 97, 128)]                      # NT <= 4, all queries, non-causal
         + [("four-wave looping", L, True, None) for L in (1, 33, 65, 77, 128)]                                      # VAR_SHORT, causal
         + [("eight-wave query-first", L, c, None) for L in (129, 160, 161, 193, 197, 225, 256) for c in (False, True)]   # 5 .. 8 query tiles
         + [("eight-wave looping", 257, False, None), ("eight-wave looping", 288, True, None)]                       # 9 tiles
         + [("four-wave long variant", L, False, Lq) for L in (197, 257) for Lq in (1, 40)]                           # VAR_LONG: few queries against NT > 4
         + [("streamed", L, False, Lq) for L in (289, 384, 385, 416, 577) for Lq in (None, 1, 33)])                   # stages of 128 keys: full, + 1 key, a lone last tile
EVERY_SHAPE = ("normal", "ramp", "creep", "hot25", "hot40")
ONE_PER_FORM = ("descend", "onehot", "flat", "bigv", "steep")
ONE_SHAPE = {"four-wave query-first": ("four-wave query-first", 97, False, None), "four-wave looping": ("four-wave looping", 77, True, None),
             "eight-wave query-first": ("eight-wave query-first", 197, False, None), "eight-wave looping": ("eight-wave looping", 257, False, None),
             "four-wave long variant": ("four-wave long variant", 257, False, 40), "streamed": ("streamed", 385, False, None)}
CASES = [(f,) + s for s in FORMS for f in EVERY_SHAPE] + [(f,) + s for s in ONE_SHAPE.values() for f in ONE_PER_FORM]
FAMILIES = dict(ref.FAMILIES, steep=ref.steep, mixed=ref.mixed_rows)
_inputs, _graded = {}, {}


def inputs(family, b, L, h):
    """fp16 qkv [b, L, 3 h 64] of a family on the host and on the GPU, made once."""
    key = (family, b, L, h)
    if key not in _inputs:
        qkv = FAMILIES[family](b, L, h, seed=2000 + L)
        _inputs[key] = (qkv, qkv.cuda())
    return _inputs[key]


def graded(family, b, L, h, causal, Lq=None):
    """The float64 reference and tolerance of the first Lq rows, computed once and left unchanged."""
    key = (family, b, L, h, causal, Lq)
    if key not in _graded:
        _graded[key] = ref.reference(inputs(family, b, L, h)[0], b, L, h, causal, Lq)
    return _graded[key]


def run(ops, qkv, b, L, h, causal=False, Lq=None):
    """[b, Lq, h 64] through ops.attention (all queries) or ops.attention_first_queries (the first Lq < L)."""
    w = h * 64
    if Lq is None:
        return ops.attention(qkv.view(b * L, 3 * w), b, L, h, causal=causal).view(b, L, w)
    q = qkv[:, :Lq, :w].contiguous().view(b * Lq, w)
    kv = qkv[:, :, w:].contiguous().view(b * L, 2 * w)
    return ops.attention_first_queries(q, kv, b, L, Lq, h).view(b, Lq, w)


def grade(got, family, b, L, h, causal, Lq, what="attention forward"):
    want, tol = graded(family, b, L, h, causal, Lq)
    r = ref.worst_ratio(got, want, tol)
    print(f"{what} {family} L={L} Lq={Lq} causal={causal}: {r:.3f} of the derived bound")
    observe(f"{what}, {family}: |got - float64| / derived tolerance", r, 1.0)
    return r


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import _lib, ops as _ops
    _lib.load()
    return _ops


@pytest.fixture
def config():
    """pclip_attention_config for the length of a test: the automatic mode comes back whatever happens."""
    from proto_clip_amd import _lib
    lib = _lib.load()
    try:
        yield lambda mode, grid=0: _lib.check(lib.pclip_attention_config(mode, grid), "pclip_attention_config")
    finally:
        _lib.check(lib.pclip_attention_config(-1, 0), "pclip_attention_config")


@pytest.mark.parametrize("family,form,L,causal,Lq", CASES)
def test_every_launch_form_against_float64(ops, family, form, L, causal, Lq):
    """(a) every element of every launch form within the derived tolerance of float64 attention."""
    got = run(ops, inputs(family, B, L, H)[1], B, L, H, causal, Lq)
    assert got.dtype == torch.float16 and got.shape == (B, Lq or L, W)
    r = grade(got, family, B, L, H, causal, Lq)
    assert r <= 1.0, (form, r)


@pytest.mark.parametrize("family", ["ramp", "hot25", "hot40"])
@pytest.mark.parametrize("b,L,h,causal,grid", [(3, 197, 3, False, 5), (3, 50, 3, False, 3), (3, 77, 3, True, 3), (3, 256, 2, False, 3), (3, 129, 2, False, 1),
                                               (3, 128, 3, True, 5)])
def test_pipelined_kernel_on_adversarial_inputs(ops, config, family, b, L, h, causal, grid):
    """(b) the persistent pipelined kernel (mode 1) equals the one-workgroup-per-item kernel bit for bit where the running maximum moves on every pair of key
    tiles and at |S| of 87 / 213; the grid is capped at an odd count below the number of items, so workgroups walk several.  And it is inside the bound."""
    qkv = inputs(family, b, L, h)[1]
    config(0)
    want = run(ops, qkv, b, L, h, causal)
    config(1, grid)
    got = torch.full_like(want, float("nan"))
    ops.attention(qkv.view(b * L, 3 * h * 64), b, L, h, causal=causal, out=got.view(b * L, h * 64))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert grade(got, family, b, L, h, causal, None, what="attention forward (pipelined)") <= 1.0


def _long(qkv, b, L, h, Lq=None):
    """pclip_attention_long_q_f16 on a fused QKV buffer at a length ops.attention gives to the resident kernels."""
    from proto_clip_amd import _lib
    lib, w = _lib.load(), h * 64
    Lq = Lq or L
    out = torch.full((b, Lq, w), float("nan"), dtype=torch.float16, device=qkv.device)
    _lib.check(lib.pclip_attention_long_q_f16(_lib.ptr(qkv), 3 * w, L * 3 * w, _lib.ptr(qkv), 3 * w, w, 2 * w, _lib.ptr(out), b, L, Lq, h, 64, 0, _lib.stream()),
               "pclip_attention_long_q_f16")
    return out


@pytest.mark.parametrize("family", ["ramp", "hot25", "hot40"])
@pytest.mark.parametrize("L", [197, 288])
def test_streamed_kernel_on_adversarial_inputs(ops, family, L):
    """(c) the streamed kernel carries the online-softmax state across its stages of 128 keys: the resident kernel's bits where every stage moves the maximum."""
    qkv = inputs(family, B, L, H)[1]
    assert torch.equal(_long(qkv, B, L, H), run(ops, qkv, B, L, H))
    for Lq in (1, 40):
        assert torch.equal(_long(qkv, B, L, H, Lq=Lq), run(ops, qkv, B, L, H, Lq=Lq))


@pytest.mark.parametrize("L", [50, 197, 385])
def test_row_bits_do_not_depend_on_the_rows_of_its_wave(ops, L):
    """(d) the rescale is taken when ANY row of the wave moved its maximum, the decision to move is per row: `mixed` puts rows that move on every pair, rows
    that never move and rows that move once side by side in every 32-row tile.  The rows of the first-queries form with Lq = L are the same bits in the
    original order and under a fixed permutation of the query rows; the Lq = 1 form gives row 0 of the full attention."""
    qkv = inputs("mixed", B, L, H)[1]
    q, kv = qkv[:, :, :W].contiguous(), qkv[:, :, W:].contiguous().view(B * L, 2 * W)
    full = run(ops, qkv, B, L, H)
    assert grade(full, "mixed", B, L, H, False, None) <= 1.0
    orig = ops.attention_first_queries(q.view(B * L, W), kv, B, L, L, H).view(B, L, W)
    assert torch.equal(orig, full)
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(L)).cuda()
    moved = ops.attention_first_queries(q[:, perm].contiguous().view(B * L, W), kv, B, L, L, H).view(B, L, W)
    assert torch.equal(moved, full[:, perm])
    assert torch.equal(run(ops, qkv, B, L, H, Lq=1), full[:, :1])


def _poison(qkv, item):
    """Item `item` of [b, L, 3 w] overwritten with NaN, +-Inf and +-65504 in turn."""
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 65504.0, -65504.0], dtype=torch.float16, device=qkv.device)
    out = qkv.clone()
    out[item] = bad[torch.arange(out[item].numel(), device=qkv.device) % 5].view_as(out[item])
    return out


@pytest.mark.parametrize("L", [50, 197, 257, 385])
def test_items_are_isolated(ops, config, L):
    """(e) three items, the middle one's q, k and v all NaN / Inf / 65504: items 0 and 2 keep the bits of the clean buffer (L is no multiple of 32: the padded
    key and value rows of the last tile re-read the item's own last row) — per-item kernel, pipelined kernel (L <= 256), and the first-queries form, whose
    output buffer is one item longer than needed and keeps its NaN fill there."""
    from proto_clip_amd import _lib
    b, h, Lq = 3, 2, 33
    w = h * 64
    clean = inputs("normal", b, L, h)[1]
    dirty = _poison(clean, 1)
    modes = [(0, 0)] + ([(1, 2)] if L <= 256 else [])                   # grid 2 for 6 items: a workgroup meets the poisoned item between clean ones
    for mode, grid in modes:
        config(mode, grid)
        want, got = run(ops, clean, b, L, h), run(ops, dirty, b, L, h)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), mode
        assert bool(torch.isfinite(want).all())
    config(-1)
    lib = _lib.load()
    fn = lib.pclip_attention_long_q_f16 if L > 288 else lib.pclip_attention_q_f16
    outs = []
    for qkv in (clean, dirty):
        q, kv = qkv[:, :Lq, :w].contiguous(), qkv[:, :, w:].contiguous()
        out = torch.full((b + 1, Lq, w), float("nan"), dtype=torch.float16, device="cuda")
        _lib.check(fn(_lib.ptr(q), w, Lq * w, _lib.ptr(kv), 2 * w, 0, w, _lib.ptr(out), b, L, Lq, h, 64, 0, _lib.stream()), "first queries")
        outs.append(out)
    torch.cuda.synchronize()
    want, got = outs
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert torch.equal(want[:b], run(ops, clean, b, L, h)[:, :Lq])
    assert bool(torch.isnan(want[b]).all()) and bool(torch.isnan(got[b]).all())


@pytest.mark.parametrize("form,L,causal,Lq", list(ONE_SHAPE.values()))
def test_second_call_gives_the_same_bits(ops, form, L, causal, Lq):
    """(f) no atomics, one summation order: the same call again, the same bits."""
    qkv = inputs("ramp", B, L, H)[1]
    first = run(ops, qkv, B, L, H, causal, Lq).clone()
    assert torch.equal(run(ops, qkv, B, L, H, causal, Lq), first), form
