"""Attention beyond 288 tokens (csrc/pclip_attention_long.hip: K / V streamed through LDS 128 keys at a time) and the tower it opens,
ViT-L/14@336px (577 tokens): accuracy against fp32 attention, the first-queries form bit for bit, the bits of the resident-K/V kernel
where both apply, the full tower against the oracle and the reference's own fixture (tests/golden/make_golden_long.py), serving with
hipGraph replay, repetition under load, the race-stress build, refusals and 336-px pre-processing."""
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
L_MAX = 4096
STRESS = os.path.join(os.path.dirname(_lib.LIB_PATH), "libpclip_stress.so")


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()


@pytest.fixture(scope="module")
def ops():
    from proto_clip_amd import ops as _ops
    _lib.load()
    return _ops


def _long(lib, qkv, B, L, H, Lq=None, out=None):
    """The new entry on a fused QKV buffer [B*L, 3W] (Lq < L: the queries of the first Lq tokens, read in place)."""
    W = H * 64
    Lq = L if Lq is None else Lq
    if out is None:
        out = torch.full((B * Lq, W), float("nan"), dtype=torch.float16, device=qkv.device)
    rc = lib.pclip_attention_long_q_f16(_lib.ptr(qkv), 3 * W, L * 3 * W, _lib.ptr(qkv), 3 * W, W, 2 * W, _lib.ptr(out), B, L, Lq, H, 64, 0,
                                        _lib.stream())
    assert rc == 0, lib.pclip_last_error()
    return out


def _ref(qkv, B, L, H):
    W = H * 64
    q, k, v = (t.view(B, L, H, 64).transpose(1, 2).float() for t in qkv.split(W, dim=-1))
    return (torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v).transpose(1, 2).reshape(B * L, W)


@pytest.mark.parametrize("B,L,H,Lq", [(2, 289, 4, 289), (2, 320, 2, 320), (2, 577, 16, 577), (1, 1025, 2, 1025), (1, L_MAX, 2, L_MAX)])
def test_long_attention_against_fp32(ops, B, L, H, Lq):
    """(a) the acceptance of test_gpu_encoder.py::test_attention at sequences the resident-K/V kernels refuse."""
    W = H * 64
    qkv = (torch.from_numpy(synth.normal((B * L, 3 * W), 23, L)).float() * 1.5).half().cuda()
    out = ops.attention(qkv, B, L, H).float()
    ref = _ref(qkv, B, L, H)
    err = (out - ref).abs().max().item()
    bound = 4e-3 * max(1.0, ref.abs().max().item())
    observe(f"long attention L={L} H={H}: max abs err vs fp32", err, bound)
    assert err <= bound
    assert observe(f"long attention L={L} H={H}: rel err vs fp32", rel_err(out, ref), 2e-3) < 2e-3


@pytest.mark.parametrize("L", [289, 577, 1025])
@pytest.mark.parametrize("Lq", [1, 33, 200])
def test_long_first_queries_match_full_attention(ops, L, Lq):
    """(b) the construction of test_attention_first_queries_matches_full_attention: the rows of the first-queries form EQUAL the
    same rows of the full attention (the class-row trick of the last vision block stays exact at 577 tokens)."""
    B, H = 2, 3
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(L + H + Lq)
    qkv = torch.randn(B * L, 3 * W, device="cuda", generator=g).half()
    full = ops.attention(qkv, B, L, H).view(B, L, W)
    q = qkv.view(B, L, 3 * W)[:, :Lq, :W].contiguous().view(B * Lq, W)
    kv = qkv[:, W:].contiguous()
    got = ops.attention_first_queries(q, kv, B, L, Lq, H).view(B, Lq, W)
    assert torch.equal(got, full[:, :Lq])


@pytest.mark.parametrize("L", [197, 257, 288])
def test_long_kernel_is_bit_identical_to_resident_kernel(ops, L):
    """(c) for 128 < L <= 288 the streamed kernel walks the same 32-key tiles in the same order with the same per-tile code
    (attn_key_tiles) as the resident-K/V kernels: the same bits, full and first-queries forms."""
    B, H = 5, 4
    W = H * 64
    qkv = (torch.from_numpy(synth.normal((B * L, 3 * W), 31, L)).float() * 1.5).half().cuda()
    lib = _lib.load()
    assert torch.equal(_long(lib, qkv, B, L, H), ops.attention(qkv, B, L, H))
    for Lq in (1, 40):
        q = qkv.view(B, L, 3 * W)[:, :Lq, :W].contiguous().view(B * Lq, W)
        kv = qkv[:, W:].contiguous()
        assert torch.equal(_long(lib, qkv, B, L, H, Lq=Lq), ops.attention_first_queries(q, kv, B, L, Lq, H))


def test_vit_l14_336_tower_against_oracle_and_reference():
    """(d) ViT-L/14@336px (24 x 1024, 577 tokens, random init) through encode_image against the oracle and against the reference's
    own towers (tests/golden/encoder_vitl14_336.npz), both precisions, within max(2 x the reference's fp16 <-> fp32 gap, 3e-3) —
    the rule of test_full_size_towers_against_reference; one image alone gives the bits it gets inside the batch."""
    g = golden("encoder_vitl14_336")
    kw = BACKBONES["ViT-L/14@336px"]
    sd = random_state_dict(seed=int(g["sd_seed"]), **kw)
    model = build_model({k: v.clone() for k, v in sd.items()}).cuda()
    assert model.visual.input_resolution == 336
    imgs = synth.make_images(int(g["n_img"]), 336, seed=int(g["image_seed"]), n_class=6)
    with torch.no_grad():
        f = model.encode_image(imgs.cuda()).float().cpu()
        f1 = model.encode_image(imgs[1:2].cuda()).float().cpu()
    assert torch.equal(f1[0], f[1])
    r16, r32 = torch.from_numpy(g["img_f16"]).float(), torch.from_numpy(g["img_f32"]).float()
    gap = rel_err(r16, r32)
    bound = max(2.0 * gap, 3e-3)
    observe("ViT-L/14@336px img: reference fp16<->fp32 gap (yard-stick)", gap, gap)
    assert observe("ViT-L/14@336px img: rel err vs REFERENCE fp32", rel_err(f, r32), bound) <= bound
    assert observe("ViT-L/14@336px img: rel err vs REFERENCE fp16", rel_err(f, r16), bound) <= bound
    for half in (True, False):
        o = clip_oracle.encode_image(sd, imgs, half=half).float()
        assert observe(f"ViT-L/14@336px img: rel err vs oracle half={half}", rel_err(f, o), bound) <= bound


def test_clip_load_336px_by_name_and_path(tmp_path):
    """clip.load("random:ViT-L/14@336px") and clip.load(<path to a 336-px state dict>) build the 577-token tower, return the 336-px
    pre-processing, and encode on the GPU; the two loads of the same weights agree bit for bit."""
    from proto_clip_amd import clip
    sd = random_state_dict(seed=1, **BACKBONES["ViT-L/14@336px"])
    path = tmp_path / "ViT-L-14-336px.pt"
    torch.save(sd, path)
    m_name, pre_name = clip.load("random:ViT-L/14@336px")
    m_path, pre_path = clip.load(str(path))
    assert pre_name.n_px == 336 and pre_path.n_px == 336 and m_path.visual.input_resolution == 336
    rng = np.random.RandomState(3)
    imgs = [rng.randint(0, 256, size=(400, 500, 3)).astype(np.uint8), rng.randint(0, 256, size=(336, 336, 3)).astype(np.uint8)]
    x = pre_path.batch(imgs)
    assert x.shape == (2, 3, 336, 336)
    with torch.no_grad():
        a, b = m_name.encode_image(x), m_path.encode_image(x)
    assert a.shape == (2, 768) and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)


def test_serving_on_336px_tower():
    """(e) ProtoClipClassifier on the 336-px tower at batch 1 and 4: the hipGraph replay gives the eager call's top-k bits."""
    from proto_clip_amd.model import Adapter_FC
    from proto_clip_amd.serving import ProtoClipClassifier
    kw = BACKBONES["ViT-L/14@336px"]
    model = build_model(random_state_dict(seed=25, **kw)).cuda()
    D, N, K = kw["embed_dim"], 12, 4
    split = synth.make_split(N, K, D, 8, 8, seed=4, sigma=3.0)
    ev = (split.visual_memory_keys.t().float() * 1.2).half().contiguous().cuda()
    et = (split.textual_memory_bank.t().float() * 1.4).half().contiguous().cuda()
    torch.manual_seed(8)
    adapter = Adapter_FC(D, dtype=torch.half).cuda()
    imgs = synth.make_images(4, 336, seed=13, n_class=N).cuda()
    clf = ProtoClipClassifier(model, ev, et, adapter, shots=K, alpha=0.2, beta=12.0, top_k=3)
    for n in (1, 4):
        tp, ti = clf.classify(imgs[:n])
        assert tp.shape == (n, 3) and torch.isfinite(tp).all()
        clf.capture(n)
        for _ in range(2):
            tg, ig = clf.classify(imgs[:n])
            assert torch.equal(tg, tp) and torch.equal(ig, ti)


def test_long_attention_under_load(ops):
    """(f) the pattern of test_attention_counted_waits_under_load at 577 tokens, 16 heads: a batch that fills the chip several times
    over (HBM-cold K / V for most workgroups), four repetitions with the caches pushed out in between, every one EQUAL to the first and
    within (a)'s bound of fp32 attention."""
    B, L, H = 48, 577, 16
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(577)
    qkv = (torch.randn(B * L, 3 * W, device="cuda", generator=g) * 1.5).half()
    first = None
    for rep in range(4):
        junk = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").random_(0, 255)
        out = ops.attention(qkv, B, L, H)
        if first is None:
            first = out.clone()
            for b0 in range(0, B, 8):                      # fp32 reference in slices (the full score tensor would be 1 GiB)
                sl = qkv[b0 * L:(b0 + 8) * L]
                ref = _ref(sl, 8, L, H)
                assert (first[b0 * L:(b0 + 8) * L].float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())
        else:
            assert torch.equal(out, first), (rep, int((out != first).any(1).sum()))
        del junk


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


@pytest.mark.parametrize("L", [289, 577])
def test_long_attention_under_jitter(ops, slib, L):
    """(g) the race-stress build (every wait_vm / lds_barrier of the streamed kernel first pauses its wave at random) reproduces the
    normal library's bits, all queries and the first-query form."""
    B, H = 24, 8
    W = H * 64
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = (torch.randn(B * L, 3 * W, device="cuda", generator=g) * 1.5).half()
    lib = _lib.load()
    for Lq in (L, 1):
        want = _long(lib, qkv, B, L, H, Lq=Lq)
        for _ in range(3):
            assert torch.equal(_long(slib, qkv, B, L, H, Lq=Lq), want)


def test_long_attention_refusals(ops):
    """(h) each refusal raises PclipError with a message before any launch; a valid call afterwards still runs."""
    lib = _lib.load()
    B, L, H = 1, 300, 2
    W = H * 64
    qkv = torch.randn(B * 4100, 3 * W, device="cuda").half()
    out = torch.empty(B * 4100, W, device="cuda", dtype=torch.float16)
    P = _lib.ptr

    def call(L=L, Lq=L, dh=64, causal=0, ldq=3 * W, ldkv=3 * W, k_off=W, v_off=2 * W):
        _lib.check(lib.pclip_attention_long_q_f16(P(qkv), ldq, L * ldq, P(qkv), ldkv, k_off, v_off, P(out), B, L, Lq, H, dh, causal,
                                                  _lib.stream()), "pclip_attention_long_q_f16")
    for kw, msg in ((dict(L=L_MAX + 1, Lq=L_MAX + 1), "L <= 4096"), (dict(causal=1), "causal"), (dict(dh=32), "head dim"),
                    (dict(Lq=L + 1), "Lq <= L"), (dict(ldq=3 * W + 4), "multiples of 8"), (dict(k_off=W + 2), "multiples of 8")):
        with pytest.raises(PclipError, match=msg):
            call(**kw)
    call()
    torch.cuda.synchronize()
    ref = _ref(qkv[:L], 1, L, H)
    assert (out[:L].float() - ref).abs().max().item() <= 4e-3 * max(1.0, ref.abs().max().item())


def _img(h, w, seed):
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, size=(h // 7 + 2, w // 7 + 2, 3)).astype(np.float64)
    up = np.kron(base, np.ones((7, 7, 1)))[:h, :w]
    return np.clip(up + rng.normal(0, 20, size=(h, w, 3)), 0, 255).astype(np.uint8)


def test_clip_preprocess_336_bit_exact():
    """(i) clip._transform(336) / pclip_preprocess_u8 at n_px = 336, bit-exact against the Pillow restatement (pinned to Pillow in
    tests/test_preprocess_cpu.py), and against Pillow's own resize."""
    from proto_clip_amd.clip.clip import _transform
    n = 336
    sizes = [(480, 640), (640, 480), (n, n), (300, 225), (n + 1, n), (2 * n, 3 * n), (200, 200)]
    imgs = [_img(h, w, h * 11 + w) for h, w in sizes]
    pre = _transform(n)
    out = pre.batch(imgs).cpu().numpy()
    assert out.shape == (len(imgs), 3, n, n)
    for i, im in enumerate(imgs):
        assert np.array_equal(out[i], pp.clip_transform(im, n)), sizes[i]
        assert np.array_equal(pre(im).cpu().numpy(), out[i])
    try:
        from PIL import Image
    except ImportError:
        return
    for i, im in enumerate(imgs):                           # Pillow doing the resize itself, the torchvision crop / normalise rules restated
        h, w = im.shape[:2]
        oh, ow = pp.resize_output_size(h, w, n)
        r = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BICUBIC))
        top, left = pp.center_crop_offsets(oh, ow, n)
        assert np.array_equal(out[i], pp.to_tensor_normalize(r[top:top + n, left:left + n])), sizes[i]
