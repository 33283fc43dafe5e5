"""pclip_cosine_logits_f16 (csrc/pclip_logits.hip), ops.cosine_logits, CLIP.forward and the zero-shot helpers of utils against (i) the float64 dot products
of the same fp16 operands under a DERIVED tolerance (contrastive_ref.logit_tolerance: the worst fp32 summation error in any order plus one fp16 rounding;
at most 1 % of the elements may differ from r16(exact) at all), (ii) the kernel's own invariances, bit for bit, and (iii) the reference's CLIP.forward
(fixtures of tests/golden/make_golden_contrastive.py) under the e2e rule: twice the reference's own fp16 <-> fp32 gap.

The kernel's workgroup tile is 16 RF rows (RF = 1, 2, 4 by M and by what the LDS holds at D) x 4 waves x 64 columns: (65, 257, 64) is one past each of
16 / 32 / 64 rows and 64 / 256 columns; (33, 17, 2048) runs two RF = 2 panels, (8, 3, 4096) RF = 1.  RF is capped by D as well (4 up to D = 1024, 2 up to
2048, 1 beyond) although four fragments would still fit the LDS up to D = 1216 and two up to 2496: (65, 37, 1088), (70, 9, 1216), (33, 17, 2112) and
(40, 5, 2496) sit in those two gaps with more rows than one panel of the capped RF holds, so every row past the first panel shows whether the grid and the
launch agree."""
import math

import numpy as np
import pytest
import torch

from conftest import golden, observe
from contrastive_ref import grade, scaled_rows
from spec import SMALL, TINY, trained_like_

pytestmark = pytest.mark.gpu

SCALE = 100.0
SENTINEL = -777.0


def rows(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, D, generator=g) / math.sqrt(D)).half()


_CASES = {}


def case(M, T, D):
    """fp16 operands on the host and the device, shared between the tests (never modified)."""
    key = (M, T, D)
    if key not in _CASES:
        a, b = rows(M, D, 1000 + M), rows(T, D, 2000 + T)
        _CASES[key] = (a, b, a.cuda(), b.cuda())
    return _CASES[key]


def check_against_exact(tag, got16, a16, b16, scale=SCALE):
    worst, differ = grade(got16, scaled_rows(a16, scale), b16)
    observe(f"cosine logits {tag}: |got - exact| / derived tolerance", worst, 1.0)
    observe(f"cosine logits {tag}: share of elements != r16(exact)", differ, 0.01)
    assert worst <= 1.0, worst
    assert differ <= 0.01, differ


RF_GAPS = [(65, 37, 1088), (70, 9, 1216), (33, 17, 2112), (40, 5, 2496)]
SHAPES = [(1, 1, 64), (3, 5, 64), (17, 33, 128), (65, 37, 512), (300, 1000, 640), (8, 3, 4096), (65, 257, 64), (33, 17, 2048)] + RF_GAPS


@pytest.mark.parametrize("M,T,D", SHAPES)
def test_logits_against_float64(M, T, D):
    """normalize = 0 on strided operands: NaN in the padding columns and in guard rows of the inputs, a sentinel in the output buffer."""
    from proto_clip_amd import ops
    a, b, _, _ = case(M, T, D)
    abuf = torch.full((M + 2, D + 8), float("nan"), dtype=torch.float16)
    bbuf = torch.full((T + 2, D + 16), float("nan"), dtype=torch.float16)
    abuf[:M, :D], bbuf[:T, :D] = a, b
    abuf, bbuf = abuf.cuda(), bbuf.cuda()
    ldl = (T + 7) // 8 * 8 + 8
    obuf = torch.full((M + 2, ldl), SENTINEL, dtype=torch.float16, device="cuda")
    logits, am, tv, ti = ops.cosine_logits(abuf[:M, :D], bbuf[:T, :D], SCALE, out=obuf[:M])
    assert am is None and tv is None and ti is None
    assert logits.shape == (M, T) and logits.dtype == torch.float16 and logits.data_ptr() == obuf.data_ptr()
    got = obuf.cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[:M, T:] == SENTINEL).all()) and bool((got[M:] == SENTINEL).all())
    check_against_exact("normalize=0", got[:M, :T], a, b)
    dense = ops.cosine_logits(abuf[:M, :D].contiguous(), bbuf[:T, :D].contiguous(), SCALE)[0]
    assert torch.equal(dense.cpu(), got[:M, :T])                                     # the strides change nothing


@pytest.mark.parametrize("M,T,D", [(17, 33, 128), (65, 37, 512), (300, 1000, 640), (8, 3, 4096), (33, 17, 2048)] + RF_GAPS)
def test_fused_normalisation_is_l2norm_rows(M, T, D):
    from proto_clip_amd import ops
    _, _, a, b = case(M, T, D)
    a, b = (a.float() * 3.7).half(), (b.float() * 0.21).half()                       # far from unit norm
    an, bn = ops.l2norm_rows(a), ops.l2norm_rows(b)
    want = ops.cosine_logits(an, bn, SCALE)[0]
    assert torch.equal(ops.cosine_logits(a, bn, SCALE, normalize_a=True)[0], want)
    assert torch.equal(ops.cosine_logits(an, b, SCALE, normalize_b=True)[0], want)
    assert torch.equal(ops.cosine_logits(a, b, SCALE, normalize_a=True, normalize_b=True)[0], want)
    check_against_exact("normalize=1", want.cpu(), an.cpu(), bn.cpu())


def test_rows_do_not_depend_on_M_nor_columns_on_T():
    from proto_clip_amd import ops
    _, _, a, b = case(300, 1000, 640)
    full = ops.cosine_logits(a, b, SCALE)[0]
    for r in (0, 131, 299):
        assert torch.equal(ops.cosine_logits(a[r:r + 1], b, SCALE)[0], full[r:r + 1]), r
    assert torch.equal(ops.cosine_logits(a, b[:37], SCALE)[0], full[:, :37])
    # ... and not on the outputs that travel with them (one workgroup per panel walks every column when a reduction is fused)
    assert torch.equal(ops.cosine_logits(a, b, SCALE, want_argmax=True, topk=5)[0], full)


def host_reduction(L16, k):
    L = L16.float().cpu().numpy()
    order = np.argsort(-L, axis=1, kind="stable")[:, :max(k, 1)]                     # descending, ascending index among equal values
    return np.argmax(L, axis=1), order, np.take_along_axis(L, order, axis=1)


def check_fused(a, b, k, tag):
    from proto_clip_amd import ops
    M, T = a.shape[0], b.shape[0]
    none, am, tv, ti = ops.cosine_logits(a, b, SCALE, want_logits=False, want_argmax=True, topk=k)
    assert none is None and am.dtype == torch.int32 and am.shape == (M,)
    L, am2, tv2, ti2 = ops.cosine_logits(a, b, SCALE, want_logits=True, want_argmax=True, topk=k)
    assert torch.equal(am, am2), tag
    assert (tv is None and tv2 is None and ti is None and ti2 is None) if k == 0 else (torch.equal(tv, tv2) and torch.equal(ti, ti2)), tag
    ref_am, ref_i, ref_v = host_reduction(L, k)
    assert np.array_equal(am.cpu().numpy(), ref_am), tag
    if k:
        assert tv.dtype == torch.float16 and ti.dtype == torch.int32 and tv.shape == ti.shape == (M, k)
        ti_h, tv_h = ti.cpu().numpy(), tv.float().cpu().numpy()
        assert np.array_equal(tv_h, ref_v[:, :k]), tag                               # values exactly
        assert all(len(set(r)) == k for r in ti_h.tolist()), tag                     # distinct indices
        assert np.array_equal(np.take_along_axis(L.float().cpu().numpy(), ti_h.astype(np.int64), axis=1), tv_h), tag
        assert np.array_equal(ti_h, ref_i[:, :k]), tag                               # lowest index first among equal values
    only_am = ops.cosine_logits(a, b, SCALE, want_logits=False, want_argmax=True)[1]
    assert torch.equal(only_am, am), tag
    if k:
        assert torch.equal(ops.cosine_logits(a, b, SCALE, want_logits=False, topk=k)[3], ti), tag


@pytest.mark.parametrize("k", [0, 1, 5, 16])
def test_fused_argmax_and_topk(k):
    _, _, a, b = case(65, 37, 512)
    check_fused(a, b, k, f"(65, 37, 512) k={k}")
    _, _, a, b = case(300, 1000, 640)
    check_fused(a, b, k, f"(300, 1000, 640) k={k}")
    _, _, a, b = case(33, 17, 2048)
    check_fused(a, b, k, f"(33, 17, 2048) k={k}")


@pytest.mark.parametrize("M,T,D", RF_GAPS)
def test_fused_outputs_where_the_depth_caps_the_panel(M, T, D):
    _, _, a, b = case(M, T, D)
    for k in (0, 1, 5):
        check_fused(a, b, k, f"({M}, {T}, {D}) k={k}")
    from proto_clip_amd import ops
    full = ops.cosine_logits(a, b, SCALE)[0]
    for r in (0, M // 2, M - 1):                                                     # the last rows are the ones a short grid would leave unwritten
        assert torch.equal(ops.cosine_logits(a[r:r + 1], b, SCALE)[0], full[r:r + 1]), r


@pytest.mark.parametrize("k", [1, 5, 16])
def test_fused_outputs_break_ties_by_index(k):
    """T = 40 with duplicated prompt rows: inside one lane's four columns (4, 5), across a 16-column fragment edge (15, 16), across fragments (3, 17, 35);
    every image row is pulled towards the duplicated prompts so that the ties sit at the top of its list."""
    _, _, a, b = case(19, 40, 128)
    b = b.clone()
    b[5], b[16], b[17], b[35] = b[4], b[15], b[3], b[3]
    a = a.clone()
    a[0::3] += 2 * b[15]
    a[1::3] += 2 * b[3]
    a[2::3] += 2 * b[4]
    check_fused(a, b, k, f"ties k={k}")
    L = check_ties_present(a, b)
    assert L


def check_ties_present(a, b):
    from proto_clip_amd import ops
    L = ops.cosine_logits(a, b, SCALE)[0].cpu()
    assert torch.equal(L[:, 15], L[:, 16]) and torch.equal(L[:, 4], L[:, 5]) and torch.equal(L[:, 3], L[:, 17]) and torch.equal(L[:, 3], L[:, 35])
    top = L.float().argmax(1)
    return bool(((top == 15) | (top == 16)).any()) and bool(((top == 3) | (top == 17) | (top == 35)).any())


def test_class_envelope_of_the_fused_outputs():
    from proto_clip_amd import PclipError, ops
    a, b, ad, bd = case(5, 4097, 64)
    check_fused(ad, bd[:4096], 16, "T = 4096")
    with pytest.raises(PclipError):
        ops.cosine_logits(ad, bd, SCALE, want_logits=False, want_argmax=True)
    with pytest.raises(PclipError):
        ops.cosine_logits(ad, bd, SCALE, topk=5)
    check_against_exact("T = 4097, logits only", ops.cosine_logits(ad, bd, SCALE)[0].cpu(), a, b)


FIXTURES = {"tiny": TINY, "small": SMALL}


@pytest.mark.parametrize("tag", ["tiny", "small"])
def test_model_forward_against_the_reference(tag):
    from proto_clip_amd import synth
    from proto_clip_amd.clip.model import build_model, random_state_dict
    g, kw = golden("contrastive_" + tag), FIXTURES[tag]
    sd_seed, n_img, n_txt = int(g["sd_seed"]), int(g["n_img"]), int(g["n_txt"])
    sd = trained_like_(random_state_dict(seed=sd_seed, **kw), sd_seed)
    sd["logit_scale"] = torch.tensor(float(g["logit_scale"]), dtype=torch.float32)
    model = build_model(sd).cuda()
    imgs = synth.make_images(n_img, kw["image_resolution"], seed=int(g["image_seed"]), n_class=n_img).cuda()
    toks = torch.from_numpy(g["tokens"]).cuda()
    logits_per_image, logits_per_text = model(imgs, toks)
    assert logits_per_image.shape == (n_img, n_txt) and logits_per_text.shape == (n_txt, n_img)
    assert logits_per_image.dtype == logits_per_text.dtype == torch.float16 and not logits_per_image.requires_grad
    assert logits_per_text.data_ptr() == logits_per_image.data_ptr() and logits_per_text.stride() == logits_per_image.stride()[::-1]
    assert torch.equal(logits_per_text, logits_per_image.t())
    got = logits_per_image.float().cpu()
    l16, l32 = torch.from_numpy(g["logits_f16"]).float(), torch.from_numpy(g["logits_f32"])
    tol = 2 * (l16 - l32).abs().max().item()                                         # the reference's own precision gap, doubled: one draw of it is all there is
    e32 = observe(f"model(image, text) {tag}: max |logits - reference fp32|", (got - l32).abs().max().item(), tol)
    e16 = observe(f"model(image, text) {tag}: max |logits - reference fp16|", (got - l16).abs().max().item(), tol)
    assert e32 <= tol, (e32, tol)
    assert e16 <= tol, (e16, tol)
    top2 = l32.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * tol
    assert decided.float().mean().item() >= 0.75
    assert torch.equal(got.argmax(1)[decided], l32.argmax(1)[decided])
    # the forward IS the kernel on the model's own features
    f, t = model.encode_image(imgs), model.encode_text(toks)
    s16 = float(np.float16(np.exp(np.float32(g["logit_scale"]))))
    from proto_clip_amd import ops
    assert torch.equal(ops.cosine_logits(f, t, s16, normalize_a=True, normalize_b=True)[0], logits_per_image)
    # dense as the reference's, whatever the prompt count (3 and 17 are no multiples of 8)
    assert logits_per_image.is_contiguous() and logits_per_image.view(-1).shape == (n_img * n_txt,)


def test_zero_shot_helpers():
    from proto_clip_amd import ops, utils
    _, _, f, w = case(300, 37, 512)
    w = ops.l2norm_rows(w)
    f = ops.l2norm_rows((f.float() + 3 * w[torch.arange(300, device="cuda") % 37].float()).half())   # every row has a clear class: no tie at the top
    wt = ops.transpose(w)                                                            # clip_classifier's [D, N]
    L = utils.clip_logits(f, wt)
    assert L.shape == (300, 37) and torch.equal(L, utils.clip_logits(f, w)) and torch.equal(L, ops.cosine_logits(f, w, 100.0)[0])
    check_against_exact("clip_logits", L.cpu(), f.cpu(), w.cpu(), 100.0)
    am = utils.clip_zero_shot(f, wt)
    assert am.dtype == torch.int64 and torch.equal(am, utils.clip_zero_shot(f, w))
    am5, tv, ti = utils.clip_zero_shot(f, wt, topk=5)
    assert torch.equal(am5, am) and torch.equal(ti[:, 0], am) and tv.shape == (300, 5)
    y = am.clone()
    y[::3] = (y[::3] + 1) % 37
    assert utils.cls_acc(L, y) == 100.0 * (am == y).float().sum().item() / 300
    assert 60 < utils.cls_acc(L, y) < 70
    L2 = utils.clip_logits(f, wt, scale=14.2890625)
    check_against_exact("clip_logits, scale 14.29", L2.cpu(), f.cpu(), w.cpu(), 14.2890625)
    assert L.is_contiguous() and L.view(-1).shape == (300 * 37,)                     # 37 % 8 != 0: the kernel's buffer is wider, the result is dense


def test_layout_settles_a_square_classifier():
    """N == D: [N, D] rows and `clip_classifier`'s [D, N] have one shape.  Without `layout` it is the reference's [D, N]."""
    from proto_clip_amd import PclipError, ops, utils
    _, _, f, w = case(21, 64, 64)                                                    # 64 prompts of width 64
    want = ops.cosine_logits(f, w, 100.0)[0]
    assert not torch.equal(want, ops.cosine_logits(f, ops.transpose(w), 100.0)[0])
    assert torch.equal(utils.clip_logits(f, w, layout="nd"), want)
    assert torch.equal(utils.clip_logits(f, ops.transpose(w), layout="dn"), want)
    assert torch.equal(utils.clip_logits(f, ops.transpose(w)), want)
    assert torch.equal(utils.clip_zero_shot(f, w, layout="nd"), utils.clip_zero_shot(f, ops.transpose(w)))
    assert torch.equal(utils.clip_zero_shot(f, w, layout="nd").cpu(), torch.from_numpy(np.argmax(want.float().cpu().numpy(), axis=1)))
    _, _, _, w37 = case(21, 37, 64)
    with pytest.raises(PclipError, match="is not"):
        utils.clip_logits(f, w37, layout="dn")                                       # [37, 64] is [N, D]


def test_misaligned_and_strided_views_are_copied():
    """Views the kernel cannot address (a column offset that breaks the 16-byte alignment, a row stride off the 8-half grid) give the bits of their dense
    copies, a single row included."""
    from proto_clip_amd import ops
    _, _, a, b = case(17, 33, 128)
    wide = torch.zeros(17, 134, dtype=torch.float16, device="cuda")
    wide[:, 2:130] = a
    want = ops.cosine_logits(a, b, SCALE)[0]
    assert wide[0:1, 2:130].is_contiguous() and wide[0:1, 2:130].data_ptr() % 16
    assert torch.equal(ops.cosine_logits(wide[0:1, 2:130], b, SCALE)[0], want[0:1])
    assert torch.equal(ops.cosine_logits(wide[:, 2:130], b, SCALE)[0], want)
    assert torch.equal(ops.cosine_logits(b, wide[3:4, 2:130], SCALE)[0], ops.cosine_logits(b, a[3:4], SCALE)[0])
    flat = torch.zeros(17 * 128 + 2, dtype=torch.float16, device="cuda")
    flat[2:] = a.reshape(-1)
    dense_off = flat[2:].view(17, 128)                                               # dense, yet 4 bytes off the alignment
    assert dense_off.is_contiguous() and dense_off.data_ptr() % 16
    assert torch.equal(ops.cosine_logits(dense_off, b, SCALE)[0], want)


def test_one_call_is_capturable_in_a_graph():
    from proto_clip_amd import ops
    _, _, a, b = case(8, 37, 512)
    a = a.clone()
    kw = dict(normalize_a=True, normalize_b=True, want_argmax=True, topk=5)
    eager = ops.cosine_logits(a, b, SCALE, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.cosine_logits(a, b, SCALE, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = ops.cosine_logits(a, b, SCALE, **kw)
    for _ in range(2):
        for o in out:
            o.zero_()
        gr.replay()
        torch.cuda.synchronize()
        for o, e in zip(out, eager):
            assert torch.equal(o, e)
