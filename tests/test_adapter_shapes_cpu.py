"""Query adapters beyond `Adapter(D, kind)` / `Adapter_FC(D)` at D % 256 == 0 — conv widths 8 / 16 / 24 / 32, the fc adapter's `reduction`, the fc adapter
at RN50x4's D = 640 — as far as they can be checked without a GPU: construction against the reference's own state-dict layout
(tests/golden/adapter_shapes.npz, written by make_golden_adapter_shapes.py from the reference's `model.Adapter(width=W)` / `model.Adapter_FC(reduction=r)`),
the up-front shape envelope, the C ABI, and the oracle (the GPU tests' yardstick) against the reference's rows at the new shapes."""
import os
import re

import pytest
import torch

from conftest import REPO, assert_adapter_close, golden, randomize_adapter_
from oracle import proto_oracle as po
from proto_clip_amd import PclipError, _lib, synth
from proto_clip_amd.main import check_shape_envelope
from proto_clip_amd.model import Adapter, Adapter_FC


def cases():
    g = golden("adapter_shapes")
    out = []
    for tag in (str(t) for t in g["tags"]):
        kind, a, d = re.fullmatch(r"(conv-3x|conv-2x|fc)_[wr](\d+)_d(\d+)", tag).groups()
        out.append((tag, kind, int(a), int(d)))
    return g, out


def build(kind, a, D, seed):
    """The product's own module with the fixture's weights: the same draws in the same order as the reference's constructor + randomize_adapter_."""
    torch.manual_seed(seed)
    ad = Adapter_FC(D, reduction=a, dtype=torch.half) if kind == "fc" else Adapter(D, kind, width=a, dtype=torch.half)
    return randomize_adapter_(ad, seed)


def unit_rows(g, D):
    return synth.make_split(4, 4, D, 4, 4, seed=int(g["row_seed"])).visual_memory_keys.t().contiguous()[:int(g["rows"])]


def test_modules_construct_with_the_reference_layout():
    g, cs = cases()
    assert len(cs) == 31
    for tag, kind, a, D in cs:
        sd = build(kind, a, D, int(g[tag + "__seed"])).state_dict()
        assert list(sd.keys()) == [str(k) for k in g[tag + "__keys"]], tag
        assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(s) for s in g[tag + "__shapes"]], tag
    for kind in ("conv-3x", "conv-2x"):
        ad = Adapter(512, kind, width=16, dtype=torch.half)                    # the reference's default keeps constructing
        assert ad.conv2.weight.shape == (16, 16, 3, 3) and ad.bn1.weight.shape == (16, 23, 23)
        assert sorted(vars(ad)["_modules"]) == ["bn1", "bn2", "bn3", "conv1", "conv2", "conv3", "relu"]
        for width in (12, 64):
            with pytest.raises(PclipError, match=r"8, 16, 24, 32"):
                Adapter(512, kind, width=width, dtype=torch.half)


def test_reference_checkpoint_layout_loads_unchanged():
    """A state dict with the reference's keys and shapes at width 32 loads with load_state_dict as it is."""
    g, _ = cases()
    tag = "conv-3x_w32_d640"
    ad = Adapter(640, "conv-3x", width=32, dtype=torch.half)
    sd = {str(k): torch.zeros([int(n) for n in str(s).split(",")], dtype=torch.half) for k, s in zip(g[tag + "__keys"], g[tag + "__shapes"])}
    assert ad.load_state_dict(sd, strict=True)


def test_shape_envelope():
    for training in (False, True):
        check_shape_envelope(10, 4, 640, "fc", training)
        check_shape_envelope(10, 4, 640, "fc", training, reduction=2)
        check_shape_envelope(10, 4, 768, "fc", training, reduction=8)
        check_shape_envelope(10, 4, 512, "fc", training, reduction=16)
        check_shape_envelope(10, 4, 1024, "fc", training, reduction=32)
        for width in (8, 16, 24, 32):
            check_shape_envelope(10, 4, 1024, "conv-3x", training, width=width)
            check_shape_envelope(10, 4, 640, "conv-2x", training, width=width)
        with pytest.raises(PclipError, match="fc adapter"):
            check_shape_envelope(10, 4, 640, "fc", training, reduction=8)       # H = 80
        with pytest.raises(PclipError, match="fc adapter"):
            check_shape_envelope(10, 4, 768, "fc", training, reduction=16)      # H = 48
        with pytest.raises(PclipError, match="fc adapter"):
            check_shape_envelope(10, 4, 576, "fc", training)                    # H = 144
        with pytest.raises(PclipError, match="width 12"):
            check_shape_envelope(10, 4, 512, "conv-3x", training, width=12)
        with pytest.raises(PclipError, match="width 64"):
            check_shape_envelope(10, 4, 512, "conv-2x", training, width=64)
    check_shape_envelope(10, 4, 512, "conv-3x", False, True)                    # the positional signature is unchanged


def test_abi_is_additive():
    header = open(os.path.join(REPO, "include", "pclip.h")).read()
    lib = _lib.load()
    assert lib.pclip_abi_version() == 1
    for name in ("pclip_adapter_conv_w_f16", "pclip_adapter_conv_w_backward_f16", "pclip_adapter_conv_w_backward_partials"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    for name in ("pclip_adapter_conv_f16", "pclip_adapter_conv_backward_f16", "pclip_adapter_conv_backward_partials", "pclip_adapter_fc_f16"):
        assert hasattr(lib, name), name
    # refusals come before any launch: no device is needed to get them
    assert lib.pclip_adapter_conv_w_backward_partials(40, 512, 1, 32) == 40
    one = torch.zeros(8, dtype=torch.float16)
    p = _lib.ptr(one)
    rc = lib.pclip_adapter_conv_w_f16(p, 1, 512, 1, 12, p, p, p, p, p, p, p, p, p, 0, p, None, None)
    assert rc != 0 and b"width=12" in lib.pclip_last_error()
    rc = lib.pclip_adapter_fc_f16(p, 1, 640, 80, p, p, p, p, p, p, 0.2, 0.8, 0, p, None, p, 0, None)
    assert rc != 0 and b"H=80" in lib.pclip_last_error()


def test_oracle_reproduces_the_reference_at_the_new_shapes():
    g, cs = cases()
    for tag, kind, a, D in cs:
        sd = build(kind, a, D, int(g[tag + "__seed"])).state_dict()
        x = unit_rows(g, D)
        y = po.adapter_fc(x, sd) if kind == "fc" else po.adapter_conv(x, sd, kind)
        assert_adapter_close(y, torch.from_numpy(g[tag + "__out"]), tag="oracle vs reference " + tag)
