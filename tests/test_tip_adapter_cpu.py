"""Tip-Adapter on the fused cache-logit kernels, the parts that need no GPU: the float64 reference and its derived tolerances (tests/tip_adapter_ref.py) judge an
emulation of the documented walk and catch five wrong ones; the near-tie cap holds for the reference alone; search_hp's lists and its first-strict-maximum rule;
the exported symbols; the host-side envelope checks of the bindings."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tip_adapter_ref as ref

NAMES = list(ref.CASES)
NEAR_TIE_CAP = 0.05

_EXACT = {}


def exact(name):
    if name not in _EXACT:
        s = ref.case(name)
        _EXACT[name] = ref.Exact(s["features"], s["keys"], s["seg"], s["text"])
    return _EXACT[name]


def ratios(name, wrong=None):
    """worst |emulated - float64| / tolerance over the (alpha, beta) points: (fp32 logits, fp16 logits)."""
    ex = exact(name)
    r32 = r16 = 0.0
    for alpha, beta in ref.POINTS:
        at = ex.at(alpha, beta)
        v32, v16 = ref.emulate(ex, alpha, beta, wrong)
        r32 = max(r32, ref.worst_ratio(v32, at["v"], at["tol32"]))
        r16 = max(r16, ref.worst_ratio(v16, at["v"], at["tol16"]))
    return r32, r16


@pytest.mark.parametrize("name", NAMES)
def test_documented_walk_stays_inside_the_tolerance(name):
    r32, r16 = ratios(name)
    print(name, "fp32 logits", round(r32, 4), "fp16 logits", round(r16, 4))
    assert r32 <= 1.0 and r16 <= 1.0, (name, r32, r16)


@pytest.mark.parametrize("wrong", ref.WRONG_WALKS)
def test_a_wrong_walk_leaves_the_tolerance(wrong):
    """On at least one of the small cases, by the fp32 logits (the fp16 rounding of a logit of several hundred hides more than the fp32 path does)."""
    worst = {}
    for name in ("ragged3", "gap", "pets", "eurosat", "caltech1", "d2048"):
        worst[name] = max(ratios(name, wrong))
        if worst[name] > 1.0:
            break
    print(wrong, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 1.0, (wrong, worst)


@pytest.mark.parametrize("name", NAMES)
def test_near_tie_cap_is_met_by_the_reference(name):
    ex = exact(name)
    for alpha, beta in ref.POINTS:
        at = ex.at(alpha, beta)
        _, tie = ref.near_ties(at["v"], at["tol16"])
        share = float(tie.double().mean())
        assert share <= NEAR_TIE_CAP, (name, alpha, beta, share)


def test_split_puts_affinities_where_clips_lie():
    s = ref.tip_split(10, [16] * 10, 512, 300, seed=3, sigma=3.0)
    aff = s["features"].double() @ s["keys"].double().t()
    own = s["labels"][:, None] == s["key_labels"][None, :]
    assert 0.30 < float(aff[own].mean()) < 0.40 and 0.22 < float(aff[~own].mean()) < 0.32
    s = ref.tip_split(10, [16] * 10, 512, 300, seed=3, sigma=2.0)
    aff = s["features"].double() @ s["keys"].double().t()
    assert 0.50 < float(aff[own].mean()) < 0.58


def test_upstream_chain_is_the_coarser_one():
    """The yardstick: upstream's fp16 chain sits further from float64 than the documented walk on a case with a long segment."""
    ex = exact("ragged3")
    s = ref.case("ragged3")
    at = ex.at(17.0, 1.0)
    up = ref.upstream_fp16_chain(s["features"], s["keys"], s["seg"], s["text"], 17.0, 1.0)
    _, mine = ref.emulate(ex, 17.0, 1.0)
    assert float((up.double() - at["v"]).abs().max()) >= float((mine.double() - at["v"]).abs().max())


def test_search_lists_are_upstreams_for_every_dataset():
    from proto_clip_amd import main, tip_adapter
    assert main._SEARCH
    for dataset, (scale, step) in main._SEARCH.items():
        cfg = main.search_scale_step({"dataset": dataset})
        betas, alphas = tip_adapter.search_lists(cfg)
        assert betas == [i * (cfg['search_scale'][0] - 0.1) / cfg['search_step'][0] + 0.1 for i in range(cfg['search_step'][0])]
        assert alphas == [i * (cfg['search_scale'][1] - 0.1) / cfg['search_step'][1] + 0.1 for i in range(cfg['search_step'][1])]
        assert len(betas) == step[0] and len(alphas) == step[1] and betas[0] == 0.1 and alphas[0] == 0.1
        assert all(type(v) is float for v in betas + alphas)


def test_first_strict_maximum_in_beta_major_order():
    from proto_clip_amd import tip_adapter
    grid = [(0.1, 0.1, 50.0), (0.1, 0.6, 71.0), (1.0, 0.1, 71.0), (1.0, 0.6, 70.0)]          # a tie: the earlier pair stays
    assert tip_adapter.best_of_grid(np.array(grid)) == (0.1, 0.6, 71.0)
    assert tip_adapter.best_of_grid(np.array([(0.1, 0.1, 0.0), (0.1, 0.6, 0.0)])) == (0, 0, 0.0)   # upstream starts from best_acc = 0


def test_library_exports_the_header_symbols():
    from proto_clip_amd import _lib
    lib = _lib.load()
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "pclip.h")).read()
    for name, nargs in (("pclip_tip_logits_f16", 19), ("pclip_tip_grid_f16", 19), ("pclip_tip_keys_backward_f16", 16)):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert f"int {name}(" in header
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(_lib._SIGS[name]) == nargs, name
        assert getattr(lib, name).argtypes == _lib._SIGS[name] and getattr(lib, name).restype is ctypes.c_int
    assert lib.pclip_abi_version() == 1
    assert _lib.OP_TIP_BACKWARD == 7 and "#define PCLIP_OP_TIP_BACKWARD 7" in header


def _operands(Q=4, D=64, N=3, NK=6):
    f = torch.zeros(Q, D, dtype=torch.float16)
    keys = torch.zeros(NK, D, dtype=torch.float16)
    seg = torch.tensor([0, 2, 4, 6][:N + 1], dtype=torch.int32)
    w = torch.zeros(N, D, dtype=torch.float16)
    return f, keys, seg, w


def test_bindings_refuse_before_any_device_call():
    from proto_clip_amd import ops, tip_adapter
    from proto_clip_amd._lib import PclipError
    f, keys, seg, w = _operands()
    # cache_values that is not one-hot, or not sorted by class
    with pytest.raises(PclipError, match="one-hot"):
        ops._tip_segment_table(torch.tensor([[1, 0], [1, 1]]))
    with pytest.raises(PclipError, match="one-hot"):
        ops._tip_segment_table(torch.tensor([[0.5, 0.5], [0.0, 1.0]]))
    with pytest.raises(PclipError, match="sorted"):
        ops._tip_segment_table(torch.tensor([[0, 1], [1, 0]]))
    with pytest.raises(PclipError, match="sorted"):
        ops._tip_segment_table(torch.tensor([0, 2, 1]))
    with pytest.raises(PclipError, match="outside"):
        ops._tip_segment_table(torch.tensor([0, 1, 5]), N=3)
    table, N = ops._tip_segment_table(torch.nn.functional.one_hot(torch.tensor([0, 0, 2, 4, 4, 4]), 5))
    assert N == 5 and table.dtype == torch.int32 and table.tolist() == [0, 2, 2, 3, 3, 6]
    assert ops._tip_segment_table(torch.tensor([1, 1, 3]), N=5)[0].tolist() == [0, 0, 2, 2, 3, 3]
    # the envelope, checked on the host: the operands are CPU tensors, so reaching the device check would also raise — the message says which check fired
    with pytest.raises(PclipError, match="multiple of 64"):
        ops.tip_logits(f[:, :32], keys[:, :32], seg, w[:, :32], 1.0, 1.0)
    with pytest.raises(PclipError, match="multiple of 64"):
        ops.tip_logits(torch.zeros(2, 2112, dtype=torch.float16), torch.zeros(6, 2112, dtype=torch.float16), seg, torch.zeros(3, 2112, dtype=torch.float16), 1.0, 1.0)
    with pytest.raises(PclipError, match="4096"):
        ops.tip_logits(f, keys, torch.zeros(4098, dtype=torch.int32), torch.zeros(4097, 64, dtype=torch.float16), 1.0, 1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(PclipError, match="alpha"):
            ops.tip_logits(f, keys, seg, w, bad, 1.0)
        with pytest.raises(PclipError, match="beta"):
            ops.tip_logits(f, keys, seg, w, 1.0, bad)
        with pytest.raises(PclipError, match="betas"):
            ops.tip_grid(f, keys, seg, w, [1.0, bad], [1.0], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(PclipError, match="at most 32 alphas"):
        ops.tip_grid(f, keys, seg, w, [1.0], [0.1] * 33, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(PclipError, match="seg"):
        ops.tip_logits(f, keys, seg[:3], w, 1.0, 1.0)
    # everything in the envelope: only the device check is left
    with pytest.raises(PclipError, match="device tensors"):
        ops.tip_logits(f, keys, seg, w, 1.0, 1.0)
    with pytest.raises(PclipError, match="device tensors"):
        ops.tip_grid(f, keys, seg, w, [1.0], [0.1] * 32, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(PclipError, match="device tensors"):
        ops.tip_segments(torch.tensor([0, 1]))
    with pytest.raises(PclipError, match="device tensors"):
        tip_adapter.tip_logits(f, keys.t(), torch.nn.functional.one_hot(torch.tensor([0, 0, 1, 1, 2, 2])), w.t(), 1.0, 1.0)
    assert math.isfinite(ref.f32(1.0))
