"""RN50x4 / RN50x16 (OpenAI's wide ResNets) end to end, and the two kernel extensions they need: the GEMM family at K % 64 != 0
(K % 8 == 0: the K-tail instantiations, whose chunks beyond column K load zeros) with N ragged against the tile, and the implicit-GEMM
3x3 convolution at any Cin, Cout that are multiples of 8.  Bit-identity against the existing kernels on zero-padded operands, fp32
references, the full towers against the oracle and the reference's own fixtures (tests/golden/make_golden_wide_rn.py), batch
independence, text towers, loading, serving with hipGraph replay, the race-stress build, refusals and 288 / 384-px pre-processing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden, observe
from oracle import clip_oracle
from oracle import preprocess_oracle as pp
from proto_clip_amd import PclipError, _lib, synth
from proto_clip_amd.clip.model import BACKBONES, build_model, random_state_dict

pytestmark = pytest.mark.gpu
STRESS = os.path.join(os.path.dirname(_lib.LIB_PATH), "libpclip_stress.so")
P = _lib.ptr


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


def up(n, m):
    return (n + m - 1) // m * m


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import ops as _ops
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def slib():
    if not os.path.exists(STRESS):
        pytest.fail(f"{STRESS} is missing: `make -C proto-clip_amd/csrc` builds it beside libpclip.so")
    lib = ctypes.CDLL(STRESS)
    for name, argtypes in _lib._SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _lib._RESTYPES.get(name, ctypes.c_int)
    return lib


def nan_tail(rows, K, g, scale):
    """[rows, K] fp16 view of a buffer whose columns K .. round_up(K, 64) + 7 are NaN (ld > K): a kernel that reads a byte beyond
    column K of any row poisons its output."""
    ld = up(K, 64) + 8
    buf = torch.full((rows, ld), float("nan"), dtype=torch.float16, device="cuda")
    buf[:, :K] = (torch.randn(rows, K, device="cuda", generator=g) * scale).half()
    return buf[:, :K]


def padded(t, rows, cols):
    """zero-padded contiguous copy [rows, cols] of a 2-D fp16 tensor."""
    out = torch.zeros(rows, cols, dtype=torch.float16, device="cuda")
    out[:t.shape[0], :t.shape[1]] = t
    return out


def gemm_bn_raw(lib, a, w, scale, shift, relu, N):
    M, K = a.shape
    out = torch.empty(M, N, dtype=torch.float16, device="cuda")
    _lib.check(lib.pclip_gemm_bn_f16(P(a), a.stride(0), P(w), w.stride(0), P(out), N, M, N, K, P(scale), P(shift), int(relu), _lib.stream()),
               "pclip_gemm_bn_f16")
    return out


def gemm_bn_res_raw(lib, a, w, scale, shift, res):
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, dtype=torch.float16, device="cuda")
    _lib.check(lib.pclip_gemm_bn_res_f16(P(a), a.stride(0), P(w), w.stride(0), P(out), N, M, N, K, P(scale), P(shift), P(res), _lib.stream()),
               "pclip_gemm_bn_res_f16")
    return out


def gemm_raw(lib, a, w, bias, act, N):
    M, K = a.shape
    out = torch.empty(M, N, dtype=torch.float16, device="cuda")
    _lib.check(lib.pclip_gemm_f16(P(a), a.stride(0), P(w), w.stride(0), P(out), N, M, N, K, P(bias), act, None, _lib.stream()), "pclip_gemm_f16")
    return out


KS = [8, 40, 80, 96, 160, 200, 328, 1000]
NS = [40, 48, 80, 96, 160, 320, 384, 640]
MS = [7, 300, 20000, 70001]                    # the ring kernel (few tiles), and the persistent tiles incl. the row split


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_gemm_k_tail_bit_identical_to_zero_padded(ops, K, N):
    """(1) ops.gemm (plain and bias + QuickGELU), gemm_bn (relu on / off) and gemm_bn_res_relu at K % 64 != 0 on operands whose columns
    beyond K are NaN, against the same calls on copies zero-padded to round_up(K, 64) columns and round_up(N, 64) rows — the existing
    kernels (a column's result does not depend on the other columns; zero products are exact): bit for bit.  Plus an fp32 matmul."""
    lib = _lib.load()
    Kp, Np = up(K, 64), up(N, 64)
    g = torch.Generator(device="cuda").manual_seed(K * 1000 + N)
    w = nan_tail(N, K, g, K ** -0.5)
    wp = padded(w, Np, Kp)
    bias = (torch.randn(N, device="cuda", generator=g) * 0.1).half()
    ss = torch.stack([1 + 0.3 * torch.randn(N, device="cuda", generator=g), 0.2 * torch.randn(N, device="cuda", generator=g)]).contiguous()
    ssp = torch.stack([torch.ones(Np, device="cuda"), torch.zeros(Np, device="cuda")])
    ssp[:, :N] = ss
    ssp = ssp.contiguous()
    biasp = torch.zeros(Np, dtype=torch.float16, device="cuda")
    biasp[:N] = bias
    for M in MS:
        a = nan_tail(M, K, g, 0.5)
        ap = padded(a, M, Kp)
        ref32 = a.float() @ w.float().t()
        bound = 4e-3 * max(1.0, ref32.abs().max().item())
        got = ops.gemm(a, w)
        assert torch.equal(got, ops.gemm(ap, wp)[:, :N]), (M, "gemm")
        err = (got.float() - ref32).abs().max().item()
        assert err <= bound, (M, err)
        got = ops.gemm(a, w, bias, act=1)
        assert torch.equal(got, ops.gemm(ap, wp, biasp, act=1)[:, :N]), (M, "gemm bias + QuickGELU")
        for relu in (True, False):
            got = gemm_bn_raw(lib, a, w, ss[0], ss[1], relu, N)
            assert torch.equal(got, ops.gemm_bn(ap, wp, ssp[0], ssp[1], relu=relu)[:, :N]), (M, "gemm_bn", relu)
            y = (ref32.half().float() * ss[0] + ss[1]).half().float()
            y = y.clamp_min(0) if relu else y
            assert (got.float() - y).abs().max().item() <= 2 * bound, (M, relu)
        if N % 64 == 0:
            res = torch.randn(M, N, device="cuda", generator=g).half()
            got = gemm_bn_res_raw(lib, a, w, ss[0], ss[1], res)
            assert torch.equal(got, ops.gemm_bn_res_relu(ap, wp, ss[0], ss[1], res)), (M, "gemm_bn_res")
            assert torch.isfinite(got).all()
    observe(f"K-tail GEMM K={K} N={N}: max abs err vs fp32 (M={MS[-1]})", err, bound)


def test_gemm_k_tail_unaligned_takes_generic_kernel_with_same_bits(ops):
    """(1) the generic kernel's K-tail instantiation (here: an output row stride that is not a multiple of 8) gives the persistent kernels' bits."""
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    M, N, K = 3000, 80, 80
    a, w = nan_tail(M, K, g, 0.5), nan_tail(N, K, g, K ** -0.5)
    want = ops.gemm(a, w)
    out = torch.empty(M, N + 3, dtype=torch.float16, device="cuda")
    _lib.check(lib.pclip_gemm_f16(P(a), a.stride(0), P(w), w.stride(0), P(out), N + 3, M, N, K, None, 0, None, _lib.stream()), "pclip_gemm_f16")
    assert torch.equal(out[:, :N], want)


def _conv_case(B, H, W, Cin, Cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(B * H * W, Cin, device="cuda", generator=g) * 0.7).half()
    w = (torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) * (9 * Cin) ** -0.5).half()
    ss = torch.stack([1 + 0.3 * torch.randn(Cout, device="cuda", generator=g), 0.2 * torch.randn(Cout, device="cuda", generator=g)]).contiguous()
    w2 = padded(w.reshape(Cout, 9 * Cin), Cout, up(9 * Cin, 64))
    return x, w, w2, ss


CONV_CASES = [(2, 144, 144, 40, 40), (2, 144, 144, 40, 80), (4, 72, 72, 80, 80), (4, 72, 72, 160, 160), (8, 36, 36, 160, 160),
              (1, 192, 192, 48, 48), (1, 192, 192, 48, 96), (3, 96, 96, 96, 96),
              (3, 9, 7, 40, 48), (1, 5, 5, 88, 24), (1, 12, 12, 80, 80), (2, 14, 14, 64, 40), (2, 20, 20, 40, 64), (1, 3, 4, 8, 8)]


@pytest.mark.parametrize("B,H,W,Cin,Cout", CONV_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_conv3x3_tail_equals_im2col_path(ops, B, H, W, Cin, Cout, relu):
    """(2) ops.conv3x3_bn at Cin / Cout outside {8, 16, 32, 64k} / {32, 64k} equals im2col3x3 + gemm_bn bit for bit: on the K-tail GEMM
    (K = 9 Cin, the im2col columns without their padding) and on the existing kernels (K padded to the K-tile, Cout padded to 64 with zero
    weights); plus torch's conv2d on the small cases."""
    x, w, w2, ss = _conv_case(B, H, W, Cin, Cout, B * H + Cin + Cout)
    with ops.conv_strip(False):
        got = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin, relu=relu)
    cols = ops.im2col3x3(x, (H * W * Cin, W * Cin, Cin, 1), B, H, W, Cin, 1)
    K, Cp = 9 * Cin, up(Cout, 64)
    if K % 64:
        ref = ops.gemm_bn(cols[:, :K].contiguous(), w2[:, :K].contiguous(), ss[0], ss[1], relu=relu)
        assert torch.equal(got, ref)
    ssp = torch.stack([torch.ones(Cp, device="cuda"), torch.zeros(Cp, device="cuda")])
    ssp[:, :Cout] = ss
    ref_p = ops.gemm_bn(cols, padded(w2, Cp, w2.shape[1]), ssp[0].contiguous(), ssp[1].contiguous(), relu=relu)[:, :Cout]
    assert torch.equal(got, ref_p)
    if Cout % 32 == 0:
        assert torch.equal(got, ops.gemm_bn(cols, w2, ss[0], ss[1], relu=relu))
    if B * H * W <= 2000:
        xt = x.view(B, H, W, Cin).permute(0, 3, 1, 2).float().cpu()
        conv = torch.nn.functional.conv2d(xt, w.permute(0, 3, 1, 2).float().cpu(), padding=1).half().float()
        y = (conv * ss[0].cpu()[None, :, None, None] + ss[1].cpu()[None, :, None, None]).half().float()
        if relu:
            y = y.clamp_min(0)
        yt = y.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
        assert (got.float().cpu() - yt).abs().max().item() <= 2e-2 * yt.abs().max().item()


def _tower(name, seed):
    kw = BACKBONES[name]
    sd = random_state_dict(seed=seed, **kw)
    return kw, sd, build_model({k: v.clone() for k, v in sd.items()}).cuda()


@pytest.mark.parametrize("name,tag", [("RN50x4", "rn50x4"), ("RN50x16", "rn50x16")])
def test_wide_resnet_tower_against_oracle_and_reference(name, tag):
    """(3) the full tower (random init, 4 images) against clip_oracle.encode_image_resnet in both precisions and against the reference's
    own towers (tests/golden/encoder_<tag>.npz), within max(2 x the fp16 <-> fp32 gap, 5e-3) — the rule of test_full_size_rn50_against_oracle."""
    g = golden("encoder_" + tag)
    kw, sd, model = _tower(name, int(g["sd_seed"]))
    R = kw["image_resolution"]
    assert model.visual.input_resolution == R
    imgs = synth.make_images(int(g["n_img"]), R, seed=int(g["image_seed"]), n_class=6)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
    assert f.shape == (imgs.shape[0], kw["embed_dim"]) and torch.isfinite(f).all()
    o16 = clip_oracle.encode_image_resnet(sd, imgs, half=True).float()
    o32 = clip_oracle.encode_image_resnet(sd, imgs, half=False).float()
    gap = rel_err(o16, o32)
    bound = max(2 * gap, 5e-3)
    observe(f"{name}: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe(f"{name}: rel err vs oracle fp16", rel_err(f, o16), bound) <= bound
    assert observe(f"{name}: rel err vs oracle fp32", rel_err(f, o32), bound) <= bound
    r16, r32 = torch.from_numpy(g["img_f16"]).float(), torch.from_numpy(g["img_f32"]).float()
    rgap = rel_err(r16, r32)
    rbound = max(2 * rgap, 5e-3)
    observe(f"{name}: reference fp16<->fp32 gap (yard-stick)", rgap, rgap)
    assert observe(f"{name}: rel err vs REFERENCE fp32", rel_err(f, r32), rbound) <= rbound
    assert observe(f"{name}: rel err vs REFERENCE fp16", rel_err(f, r16), rbound) <= rbound


@pytest.mark.parametrize("name,big", [("RN50x4", 300), ("RN50x16", 3)])
def test_wide_resnet_batch_independence(name, big):
    """(4) image i encoded alone (the ring kernels), in a batch of 3 and in a batch of 300 (crossing the 256-image pass) gives the same bits."""
    kw, _, model = _tower(name, 7)
    R = kw["image_resolution"]
    imgs = synth.make_images(big, R, seed=3, n_class=5).cuda()
    with torch.no_grad():
        fb = model.encode_image(imgs)
        f3 = model.encode_image(imgs[:3])
        for i in (0, 2):
            assert torch.equal(model.encode_image(imgs[i:i + 1])[0], fb[i])
    assert torch.equal(f3, fb[:3])
    if big > 256:
        with torch.no_grad():
            assert torch.equal(model.encode_image(imgs[257:258])[0], fb[257])


@pytest.mark.parametrize("name", ["RN50x4", "RN50x16"])
def test_wide_text_towers_against_oracle(name):
    """(5) the 640-wide / 10-head and 768-wide / 12-head text towers against clip_oracle.encode_text (rule of test_full_size_text_tower_against_oracle)."""
    kw, sd, model = _tower(name, 9)
    V = kw["vocab_size"]
    g = torch.Generator().manual_seed(6)
    toks = torch.zeros(6, 77, dtype=torch.long)
    for i in range(6):
        n = int(torch.randint(1, 74, (1,), generator=g))
        toks[i, 0] = V - 2
        toks[i, 1:1 + n] = torch.randint(1, V - 2, (n,), generator=g)
        toks[i, 1 + n] = V - 1
    with torch.no_grad():
        f = model.encode_text(toks.cuda()).float().cpu()
    assert f.shape == (6, kw["embed_dim"])
    o16 = clip_oracle.encode_text(sd, toks, half=True).float()
    o32 = clip_oracle.encode_text(sd, toks, half=False).float()
    gap = rel_err(o16, o32)
    bound = max(2 * gap, 3e-3)
    observe(f"{name} text tower: oracle fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe(f"{name} text tower: rel err vs oracle fp16", rel_err(f, o16), bound) <= bound


def test_clip_load_rn50x4_path_and_name(tmp_path):
    """(6) clip.load(<path>) and clip.load("RN50x4", download_root=...) of a saved RN50x4 state dict give build_model's features, and the 288-px pre-processing."""
    from proto_clip_amd import clip
    kw = BACKBONES["RN50x4"]
    sd = random_state_dict(seed=2, **kw)
    torch.save(sd, tmp_path / "RN50x4.pt")
    m_path, pre = clip.load(str(tmp_path / "RN50x4.pt"))
    m_name, _ = clip.load("RN50x4", download_root=str(tmp_path))
    ref = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    assert pre.n_px == 288
    rng = np.random.RandomState(4)
    x = pre.batch([rng.randint(0, 256, size=(300, 400, 3)).astype(np.uint8), rng.randint(0, 256, size=(288, 288, 3)).astype(np.uint8)])
    with torch.no_grad():
        a, b, c = m_path.encode_image(x), m_name.encode_image(x), ref.encode_image(x)
    assert a.shape == (2, 640) and torch.isfinite(a.float()).all()
    assert torch.equal(a, c) and torch.equal(b, c)


def test_serving_on_rn50x4():
    """(7) ProtoClipClassifier on the RN50x4 tower (a conv adapter: the fc adapter is refused at D = 640) at batch 1 and 4: the hipGraph
    replay gives the eager call's top-k bits."""
    from proto_clip_amd.model import Adapter
    from proto_clip_amd.serving import ProtoClipClassifier
    kw, _, model = _tower("RN50x4", 25)
    D, N, K = kw["embed_dim"], 12, 4
    split = synth.make_split(N, K, D, 8, 8, seed=4, sigma=3.0)
    ev = (split.visual_memory_keys.t().float() * 1.2).half().contiguous().cuda()
    et = (split.textual_memory_bank.t().float() * 1.4).half().contiguous().cuda()
    torch.manual_seed(8)
    adapter = Adapter(D, "conv-3x", dtype=torch.half).cuda()
    imgs = synth.make_images(4, 288, seed=13, n_class=N).cuda()
    clf = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=3)
    for n in (1, 4):
        tp, ti = clf.classify(imgs[:n])
        assert tp.shape == (n, 3) and torch.isfinite(tp).all()
        clf.capture(n)
        for _ in range(2):
            tg, ig = clf.classify(imgs[:n])
            assert torch.equal(tg, tp) and torch.equal(ig, ti)


def test_k_tail_and_conv_tail_under_jitter(ops, slib):
    """(8) the race-stress build (every wait_vm / lds_barrier / TileSrc stage pauses its wave at random) reproduces the normal library's bits
    for the K-tail GEMM (persistent and ring) and a tail convolution."""
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(88)
    for M, N, K in ((50000, 320, 80), (70001, 640, 160), (300, 96, 96)):
        a, w = nan_tail(M, K, g, 0.5), nan_tail(N, K, g, K ** -0.5)
        bias = (torch.randn(N, device="cuda", generator=g) * 0.1).half()
        want = gemm_raw(lib, a, w, bias, 0, N)
        for _ in range(3):
            assert torch.equal(gemm_raw(slib, a, w, bias, 0, N), want), (M, N, K)
    B, H, W, Cin, Cout = 4, 72, 72, 80, 80
    x, _, w2, ss = _conv_case(B, H, W, Cin, Cout, 17)
    want = ops.conv3x3_bn(x, w2, ss[0], ss[1], B, H, W, Cin)
    z = torch.zeros(64, dtype=torch.float16, device="cuda")
    for _ in range(3):
        y = torch.empty_like(want)
        _lib.check(slib.pclip_conv3x3_bn_f16(P(x), P(w2), P(z), B, H, W, Cin, Cout, P(ss[0]), P(ss[1]), 1, P(y), _lib.stream()), "pclip_conv3x3_bn_f16")
        assert torch.equal(y, want)


def test_k_tail_refusals(ops):
    """(9) K = 84, Cin = 36 and Cout = 20 raise PclipError with a message; a valid call on the same stream afterwards is correct."""
    g = torch.Generator(device="cuda").manual_seed(9)
    buf = torch.randn(64, 88, device="cuda", generator=g).half()
    w = torch.randn(40, 88, device="cuda", generator=g).half()
    with pytest.raises(PclipError, match="K=84 must be a multiple of 8"):
        ops.gemm(buf[:, :84], w[:, :84])
    x = torch.randn(2 * 5 * 5, 36, device="cuda", generator=g).half()
    ss = torch.stack([torch.ones(40, device="cuda"), torch.zeros(40, device="cuda")]).contiguous()
    with pytest.raises(PclipError, match="Cin=36"):
        ops.conv3x3_bn(x, torch.zeros(40, up(9 * 36, 64), dtype=torch.float16, device="cuda"), ss[0], ss[1], 2, 5, 5, 36)
    x40 = torch.randn(2 * 5 * 5, 40, device="cuda", generator=g).half()
    with pytest.raises(PclipError, match="Cout=20"):
        ops.conv3x3_bn(x40, torch.zeros(20, up(9 * 40, 64), dtype=torch.float16, device="cuda"), ss[0, :20].contiguous(), ss[1, :20].contiguous(), 2, 5, 5, 40)
    a, ww = buf[:, :80], w[:, :80]
    out = ops.gemm(a, ww)
    torch.cuda.synchronize()
    ref = a.float() @ ww.float().t()
    assert (out.float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())


def _img(h, w, seed):
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, size=(h // 7 + 2, w // 7 + 2, 3)).astype(np.float64)
    up_ = np.kron(base, np.ones((7, 7, 1)))[:h, :w]
    return np.clip(up_ + rng.normal(0, 20, size=(h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("n", [288, 384])
def test_clip_preprocess_wide_resnet_bit_exact(n):
    """(10) clip._transform(288 / 384) bit-exact against the Pillow restatement (oracle/preprocess_oracle.py)."""
    from proto_clip_amd.clip.clip import _transform
    sizes = [(480, 640), (640, 480), (n, n), (300, 225), (n + 1, n), (2 * n, 3 * n), (200, 200)]
    imgs = [_img(h, w, h * 13 + w) for h, w in sizes]
    pre = _transform(n)
    out = pre.batch(imgs).cpu().numpy()
    assert out.shape == (len(imgs), 3, n, n)
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i], pp.clip_transform(im, n)), sizes[i]
        assert np.array_equal(pre(im).cpu().numpy(), out[i])
